"""CPU restatement of Y.encodeStateVectorFromUpdate (Yjs 13.5.16 `os`, update v1) — test infrastructure.

Yjs reads the update's structs in byte order with a LazyStructReader that keeps Skips, and holds one
(client, clock, stop) state per run of equal client ids:

    a run starts with stop = (first clock != 0) and clock = 0; a Skip sets stop; while not stopped,
    clock = struct clock + struct length; at each client change and at the end the pair
    (client, clock) is written if clock != 0.

The result is varuint(pairs) and the pairs in the update's own order (never re-sorted); the delete
set is not read. Two things follow from the loop as Yjs wrote it: neighbouring sections of one client
are one run, and the update's very first struct sets clock = its end BEFORE its kind is looked at
(`let o = n ? 0 : i.id.clock + i.length` in front of the loop), so an update that opens with a Skip
at clock 0 reports that Skip's length. Pinned against Yjs's own bytes in
tests/test_update_store_ref.py."""
from oracle.ymerge import SKIP, Dec, lazy_structs, wvu


def sv_from_update(u):
    structs = lazy_structs(Dec(bytes(u)))
    out = bytearray()
    if not structs:
        wvu(out, 0)
        return bytes(out)
    pairs = []
    first = structs[0]
    client = first.client
    stop = first.clock != 0
    clock = 0 if stop else first.clock + first.length
    for s in structs:
        if s.client != client:
            if clock:
                pairs.append((client, clock))
            client = s.client
            clock = 0
            stop = s.clock != 0
        if s.kind == SKIP:
            stop = True
        if not stop:
            clock = s.clock + s.length
    if clock:
        pairs.append((client, clock))
    wvu(out, len(pairs))
    for c, k in pairs:
        wvu(out, c)
        wvu(out, k)
    return bytes(out)
