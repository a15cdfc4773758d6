// yc_store.hip — Y.encodeStateVectorFromUpdate (`os`, Yjs 13.5.16) for every update of a staged
// batch, over the tables of the lazy decode (sections, usec_start / usec_n, s_clock, s_len, s_info).
//
// Yjs walks the update's structs in byte order, Skips included (a LazyStructReader that does not
// filter them), with one (client, clock, stop) state per run of equal client ids:
//   a run starts with stop = (its first struct's clock != 0) and clock = 0; a Skip sets stop; while
//   not stopped, clock = struct clock + struct length; at each client change and at the end the pair
//   (client, clock) is written if clock != 0. The result is varuint(pairs), then the pairs in the
//   update's own order: never re-sorted, the delete set never read.
// Two things follow from the loop as written and are kept: neighbouring sections of one client are
// ONE run (only the run's first clock is tested against 0), and the update's very first struct sets
// clock = its end before its kind is looked at, so an update that opens with a Skip at clock 0
// reports that Skip's length.
// Structs of a section have contiguous clocks, so a section contributes either nothing (the run is
// stopped), its end clock (no Skip), or the clock of its first Skip: one lane per struct finds the
// first Skips (k_usv_skips), one lane per update folds its sections (k_usv_sizes, k_usv_write).
#include "yc_store.h"

namespace yc {
namespace {

__global__ __launch_bounds__(256) void k_usv_skips(Work w, StoreSv a) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= a.nstructs) return;
  if ((w.s_info[j] & 31u) != REF_SKIP) return;
  const uint32_t sec = w.s_sec[j];
  if (sec < a.nsections) atomicMin(&a.sec_skip[sec], j);
  else raise_err(&w.ctr->err, ERR_CAPACITY);
}

// the state vector of update u: its pairs written behind q (WRITE), their count and bytes returned
template <bool WRITE>
__device__ __forceinline__ uint32_t usv_fold(const Work& w, const StoreSv& a, uint32_t u, uint8_t* __restrict__ out, uint64_t q,
                                             uint32_t& count) {
  const uint32_t s0 = w.usec_start[u], s1 = s0 + w.usec_n[u];
  if (s1 < s0 || s1 > a.nsections) { raise_err(&w.ctr->err, ERR_CAPACITY); count = 0; return 0; }  // (the decode's tables disagree)
  bool have = false, stop = false;
  uint32_t client = 0, clock = 0, n = 0, bytes = 0;
  auto emit = [&]() {
    if (!have || !clock) return;
    ++n;
    bytes += vu_size(client) + vu_size(clock);
    if (WRITE) { q = wr_vu(out, q, client); q = wr_vu(out, q, clock); }
  };
  for (uint32_t i = s0; i < s1; ++i) {
    const Section S = w.sections[i];
    if (!S.n) continue;  // (no struct: the reader never sees the section)
    const uint32_t sk = a.sec_skip[i];
    if (S.first_idx >= a.nstructs || S.n > a.nstructs - S.first_idx) { raise_err(&w.ctr->err, ERR_CAPACITY); break; }
    if (!have || S.client != client) {
      emit();
      const bool first = !have;
      have = true;
      client = S.client;
      clock = 0;
      stop = S.clock != 0;
      if (first && !stop && sk == S.first_idx) clock = w.s_len[sk];  // the update opens with a Skip at clock 0
    }
    if (stop) continue;
    if (sk == NONE) {
      const uint32_t last = S.first_idx + S.n - 1;
      clock = w.s_clock[last] + w.s_len[last];
    } else {
      if (sk > S.first_idx) clock = w.s_clock[sk];  // the end of the struct in front of the Skip
      stop = true;
    }
  }
  emit();
  count = n;
  return bytes;
}

__global__ __launch_bounds__(256) void k_usv_sizes(Work w, StoreSv a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u > w.nupd) return;
  if (u == w.nupd) { a.size[u] = 0; return; }
  uint32_t count = 0;
  const uint32_t bytes = usv_fold<false>(w, a, u, nullptr, 0, count);
  a.size[u] = vu_size(count) + bytes;
}

__global__ __launch_bounds__(256) void k_usv_write(Work w, StoreSv a) {
  const uint32_t u = blockIdx.x * blockDim.x + threadIdx.x;
  if (u >= w.nupd) return;
  const uint64_t q0 = a.offs[u], q1 = a.offs[u + 1];
  if (q1 > a.out_cap || q1 - q0 != a.size[u]) { raise_err(&w.ctr->err, ERR_CAPACITY); return; }
  // the fold runs twice, once for the count and once to write the pairs behind it (a few sections)
  uint32_t count = 0;
  const uint32_t bytes = usv_fold<false>(w, a, u, nullptr, 0, count);
  if (vu_size(count) + bytes != a.size[u]) { raise_err(&w.ctr->err, ERR_CAPACITY); return; }
  const uint64_t q = wr_vu(a.out, q0, count);
  usv_fold<true>(w, a, u, a.out, q, count);
}

inline uint32_t G(uint64_t n) { return (uint32_t)(n / 256 + 1); }

}  // namespace

void launch_update_svs(const Work& w, const StoreSv& a, hipStream_t s) {
  const uint32_t nstructs = a.nstructs, nsections = a.nsections;
  if (nsections) fill_u32_multi({{a.sec_skip, (uint64_t)nsections, NONE}}, s);
  if (nstructs) hipLaunchKernelGGL(k_usv_skips, dim3(G(nstructs)), dim3(256), 0, s, w, a);
  hipLaunchKernelGGL(k_usv_sizes, dim3(G(w.nupd + 1)), dim3(256), 0, s, w, a);
  scan_u32_to_u64(w.tmp, w.tmp_bytes, a.size, a.offs, (uint64_t)w.nupd + 1, s);
  hipLaunchKernelGGL(k_usv_write, dim3(G(w.nupd)), dim3(256), 0, s, w, a);
}

}  // namespace yc
