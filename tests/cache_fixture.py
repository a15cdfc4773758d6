"""tests/golden/cache.json (tests/golden/gen/gen_cache_fixtures.js): small Yjs 13.5.16 documents that
keep an index map of their roots, with the cache object `c` crdt.js's open / refresh loop builds from
each. Shared by the cache tests."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
_FX = None


def cases():
    global _FX
    if _FX is None:
        with open(os.path.join(HERE, "golden", "cache.json")) as f:
            _FX = json.load(f)["cases"]
    return _FX


def updates(case):
    return [bytes.fromhex(u) for u in case["updates"]]


def element_bytes(entry) -> bytes:
    """The bytes of the value element of an index entry's winning item: ContentAny is written as a
    count (1) and the values, and the view hands over the last value; other contents as they are."""
    b = bytes.fromhex(entry["content"])
    if entry["ref"] == 8:
        assert b[0] == 1
        return b[1:]
    return b
