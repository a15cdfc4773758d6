"""tests/golden/text.json (tests/golden/gen/gen_text_fixtures.js) for the tests that read it: concurrent
Y.Text histories and hand-built ContentString updates with what Yjs 13.5.16 answered, every byte
string resolved out of the file's one deflated table and loaded once.

A case: `updates`, `update_svs` (encodeStateVectorFromUpdate of each), `state_raw` (13.5 order), `state` / `sv` / `state_rev` / `merged` / `merged_rev`
(delete sets and state vectors in canonical order), `replies` (per requested state vector Yjs's
encodeStateAsUpdate(doc, sv) as `update` and diffUpdate(merged, sv) as `diff`; None where Yjs threw),
`json_m` / `json_t` (Node's JSON.stringify text of getMap('m') and of the root `t` read as a list),
`len_t`, and `pair_split`: a cut fell between the two units of a surrogate pair."""
import base64
import functools
import json
import os
import zlib

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "text.json")


@functools.lru_cache(maxsize=None)
def load():
    """{"histories", "hand", "long"}. Shared by all tests of a session: read it, never change it."""
    with open(PATH) as f:
        raw = json.load(f)
    cat, blobs = zlib.decompress(base64.b64decode(raw["blobs_z"])), []
    for n in raw["blob_lens"]:
        blobs.append(cat[:n])
        cat = cat[n:]
    assert not cat

    def val(x):  # bytes, or None where Yjs threw
        return None if isinstance(x, dict) else blobs[x]

    def case(c):
        c = dict(c)
        c["updates"] = [blobs[i] for i in c["updates"]]
        c["update_svs"] = [blobs[i] for i in c["update_svs"]]
        for k in ("state_raw", "state", "sv", "state_rev", "merged", "merged_rev"):
            c[k] = val(c[k])
        c["replies"] = [{"sv": blobs[r["sv"]], "update": val(r["update"]), "diff": val(r["diff"])} for r in c["replies"]]
        c["json_m"] = blobs[c["json_m"]].decode()
        c["json_t"] = blobs[c["json_t"]].decode()
        return c

    return {"histories": [case(c) for c in raw["histories"]], "hand": [case(c) for c in raw["hand"]], "long": case(raw["long"])}


def all_cases():
    fx = load()
    return fx["histories"] + fx["hand"] + [fx["long"]]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)
