"""tests/golden/deep.json (tests/golden/gen/gen_deep_fixtures.js) for the tests that read it: the
records with their inputs and toJSON values resolved, loaded once, and the one rule by which an
update of the engine's is compared with the one Yjs 13.5.16 answered.

The file holds Yjs's inputs as bytes and Yjs's answers as digests (sha below). The oracle rebuilds
the forward answers byte for byte (tests/test_deep_fixture.py checks it against the digests), so a
failing comparison can still be looked at in bytes.

Yjs's encodeStateAsUpdate depends on the order of its applyUpdate calls in one respect: how adjacent
GC structs of a client are cut (it re-merges only the structs a transaction touched). A batch has
no order, so the engine always merges GC + GC. Where Yjs's bytes are already in that coalesced form
the comparison is exact; elsewhere the engine's bytes are coalesced (tests/v1util.py coalesce_gc)
and compared with the digest of Yjs's coalesced bytes, which the generator took with a coalescer of
its own (v1.js coalesceGc). State vectors, toJSON, pending flags and delete sets are compared
exactly, always.
"""
import base64
import functools
import hashlib
import json
import os
import zlib

from tests.v1util import coalesce_gc

_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deep.json")
RANDOM_FORMS = ("log_", "full_", "mixed_")


@functools.lru_cache(maxsize=None)
def load():
    """{"roots", "histories", "cases", "parked"}: every input (updates, requested state vectors) as
    bytes, every "json" as the parsed value, what Yjs answered in bytes as its digest record (sha,
    assert_same_update). Shared by all tests of a session: read it, never change it."""
    with open(_PATH) as f:
        raw = json.load(f)
    cat, blobs = zlib.decompress(base64.b64decode(raw["blobs_z"])), []
    for n in raw["blob_lens"]:
        blobs.append(cat[:n])
        cat = cat[n:]
    assert not cat
    jsons = json.loads(zlib.decompress(base64.b64decode(raw["jsons_z"])))

    def diff(d):
        return {"sv": blobs[d[0]], "update": d[1]}

    cases = []
    for c in raw["cases"]:
        c = dict(c)
        c["updates"] = [blobs[i] for i in c["updates"]]
        c["json"] = jsons[c["json"]]
        c["diffs"] = [diff(d) for d in c["diffs"]]
        f = c.pop("flags")  # the names of the flags that are set
        c["pending"], c["pending_rev"] = ("pending" in f, "pending_ds" in f), ("pending_rev" in f, "pending_ds_rev" in f)
        c["live_depth"] = max(c["root_depth"].values())
        cases.append(c)
    parked = []
    for c in raw["parked"]:
        c = dict(c)
        c["updates"] = [blobs[i] for i in c["updates"]]
        c["steps"] = [dict(s, delta=diff(s["delta"]), json=jsons[s["json"]], **{k: k in s["flags"] for k in ("pending", "pending_ds", "parked")})
                      for s in c["steps"]]
        parked.append(c)
    return {"roots": raw["roots"], "histories": raw["histories"], "cases": cases, "parked": parked}


def is_random(c):
    return c["name"].startswith(RANDOM_FORMS)


def quiet_cases():
    """The cases with nothing pending after the forward or the reversed apply."""
    return [c for c in load()["cases"] if not any(c["pending"]) and not any(c["pending_rev"])]


def hand_built():
    return [c for c in load()["cases"] if not is_random(c)]


def random_sample(n):
    """n random cases spread over the seeds, the three forms in turn."""
    rnd = [c for c in quiet_cases() if is_random(c)]
    return rnd[:: max(1, len(rnd) // n)][:n]


def sha(b):
    """The fixture's digest of a byte string: the first 16 hex digits of its SHA-256."""
    return hashlib.sha256(bytes(b)).hexdigest()[:16]


def exact(want):
    """Whether Yjs's bytes were already in the order-free form (then the engine must equal them):
    the digest record is one digest, not [digest of the bytes, digest of their coalesced form]."""
    return isinstance(want, str)


def coalesced(want):
    """The digest of the coalesced form of the bytes a digest record stands for."""
    return want if exact(want) else want[1]


def assert_same_update(got, want, tag):
    """`got` against the digest record of Yjs's update. The delete set is part of the bytes on both
    sides of either comparison (coalesce_gc leaves it as it stands), so it is compared exactly."""
    if exact(want):
        assert sha(got) == want, tag
    else:
        assert sha(coalesce_gc(got)) == want[1], tag
