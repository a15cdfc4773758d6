"""The cache fixture is self-consistent: what the generator recorded of Yjs's answers agrees with
itself, and it holds the cases the cache tests rely on."""
import os

from tests.cache_fixture import cases


def test_c_keys_are_ix_keys():
    for c in cases():
        assert list(c["c"].keys()) == c["ix_keys"], c["name"]
        assert [e["name"] for e in c["entries"]] == c["ix_keys"], c["name"]
        # JSON.stringify drops undefined values: ix holds the others
        undef = {e["name"] for e in c["entries"] if e["content"] == "017f"}
        assert set(c["ix"].keys()) == set(c["ix_keys"]) - undef, c["name"]
        for e in c["entries"]:
            assert e["is_array"] == isinstance(c["c"][e["name"]], list), (c["name"], e["name"])
            # loose equality with 'map', as far as the recorded JSON shows it
            v = c["ix"].get(e["name"])
            while isinstance(v, list) and len(v) == 1:
                v = v[0]
            assert e["is_array"] == (v != "map"), (c["name"], e["name"])


def test_cases_present():
    by = {c["name"]: c for c in cases()}
    assert len(by) == len(cases()) >= 30
    assert os.path.getsize(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cache.json")) <= 200_000
    assert by["empty"]["c"] == {} and by["no_index"]["c"] == {} and by["all_deleted"]["c"] == {}
    assert by["other_index"]["index"] == "index"
    assert "ix" in by["lists_itself"]["c"]
    assert "" in by["empty_name"]["c"]
    assert {len(n.encode()) for n in by["name_64"]["c"]} == {64, 1} and {len(n.encode()) for n in by["name_65"]["c"]} == {65, 1}
    assert {"\"", "\\", "\x01", " ", "\U0001F600"} <= set(by["escaped_names"]["c"])
    assert {"10", "9"} <= set(by["integer_names"]["c"])
    assert by["wrong_kind"]["c"] == {"list": {}, "dict": []}
    assert by["ghost_roots"]["c"] == {"ghost": {}, "ghost2": []}
    assert by["concurrent_low_wins"]["c"]["r"] != by["concurrent_high_wins"]["c"]["r"]
    vals = {e["name"]: e for n in ("values_0", "values_1", "values_2") for e in by[n]["entries"]}
    maps = {n for n, e in vals.items() if not e["is_array"]}
    assert maps == {"v_map", "v_amap", "v_aamap", "v_aaamap"}
    assert {"v_array", "v_Map", "v_1", "v_null", "v_undef", "v_obj", "v_ymap", "v_bytes"} <= set(vals)
    assert vals["v_ymap"]["ref"] == 7 and vals["v_bytes"]["ref"] == 3
