"""A staged batch follows the environment it was staged under (crdt_amd/csrc/yc_switches.h: ycrdt_batch::sw).

layout() decides by YCRDT_DECODE which updates get chunk groups; the merge decides by it again (the
exit-table walk, the wavefront decode's tables). Both read the batch's one snapshot, so a batch staged
under `chunks` and merged while the environment says `direct` (and the other way round) is the batch
staged and merged under its staging setting: the same bytes as with no change in between, and as the
CPU oracle's.

Inputs: three updates of one map document (329 bytes each, a client each, no key written twice), and
the same three with one update of 76 806 bytes — above DIRECT_MAX_BYTES (16 384), so under `direct`
both of layout()'s lists are populated. No key is overwritten and nothing deleted, so the document's
state is exactly Y.mergeUpdates of the updates (oracle/ymerge.py; the delete set, empty here, in 13.6's
order), and its state vector each client's last clock, clients descending."""
import pytest

crdt_amd = pytest.importorskip("crdt_amd")
from oracle.ymerge import Dec, lazy_structs, merge_updates, wvu  # noqa: E402
from oracle.yref import Doc as ODoc  # noqa: E402
from tests.histories import any_str  # noqa: E402
from tests.v1util import canonical_update  # noqa: E402

pytestmark = pytest.mark.gpu


def _update(client, nkeys, name, value):
    d = ODoc(client)
    for k in range(nkeys):
        d.map_set("users", f"{name}{k:05d}", any_str(value))
    return d.encode_state_as_update()


def _state_vector(update):
    end = {}
    for s in lazy_structs(Dec(update)):
        end[s.client] = max(end.get(s.client, 0), s.clock + s.length)
    out = bytearray()
    wvu(out, len(end))
    for c in sorted(end, reverse=True):
        wvu(out, c)
        wvu(out, end[c])
    return bytes(out)


@pytest.fixture(scope="module")
def cases():
    small = [_update(c, 12, f"s{c}_", "v" * 7) for c in (3, 5, 9)]
    big = _update(11, 2400, "big", "x" * 12)
    assert all(len(u) < 1024 for u in small) and 70 << 10 < len(big) < 90 << 10
    out = []
    for ups in (small, small + [big]):
        update = canonical_update(merge_updates(ups))
        out.append((ups, (update, _state_vector(update))))
    return out


def _merge(monkeypatch, ups, staged, merged):
    monkeypatch.setenv("YCRDT_DECODE", staged)
    b = crdt_amd.Batch(ups)
    monkeypatch.setenv("YCRDT_DECODE", merged)
    b.merge()
    return b.result()


@pytest.mark.parametrize("staged,merged", [("chunks", "direct"), ("direct", "chunks")])
def test_batch_keeps_its_staging_switches(cases, monkeypatch, staged, merged):
    for ups, want in cases:
        got = _merge(monkeypatch, ups, staged, merged)
        assert got == want, (staged, merged, len(ups))
        assert got == _merge(monkeypatch, ups, staged, staged), (staged, merged, len(ups))
