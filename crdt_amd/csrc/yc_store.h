// yc_store.h — the doc-less update store (a persistence worker that keeps topics as update bytes):
// Y.encodeStateVectorFromUpdate for many updates in one pass, over the lazy decode's tables
// (yc_store.hip).
#pragma once
#include "yc_common.h"
#include "yc_work.h"

namespace yc {

struct StoreSv {
  uint32_t* sec_skip;   // [nsections] the first Skip struct of every section (NONE: it has none)
  uint32_t* size;       // [nupd + 1] bytes of every update's state vector, 0 behind the last
  uint64_t* offs;       // [nupd + 1] their exclusive scan: update u's bytes are out[offs[u] .. offs[u + 1])
  uint8_t* out;
  uint64_t out_cap;     // bytes of `out` (a write past it raises ERR_CAPACITY instead)
  uint32_t nstructs, nsections;  // rows of the decode's struct and section tables
};
// bytes that hold the state vectors of nupd updates with nsections sections in all: a count and one
// (client, clock) pair per section at the most, 5 bytes per varuint
inline uint64_t store_sv_bound(uint64_t nupd, uint64_t nsections) { return 5 * nupd + 10 * nsections; }
// first Skips, sizes, offsets, then the bytes (w.tmp: scan space for nupd + 1 values)
void launch_update_svs(const Work& w, const StoreSv& a, hipStream_t s);

}  // namespace yc
