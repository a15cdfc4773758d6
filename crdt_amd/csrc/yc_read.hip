// yc_read.hip — fleet point reads on gfx950 (ycrdt_docs_read): YMap.get / size and YArray.get /
// length of many documents, answered over the view of ONE multi-document merge after the front half
// of the fleet toJSON pass (yc_json.hip: keys sorted by container and entry name, every item sized
// bottom-up). A read is one lane:
//   k_rvisible    per sorted key a live-entry flag (view_map_size's rule), per list segment its
//                 visible elements (visible() of yc_host.cpp); one 64-bit scan over both follows
//   k_rresolve    the root container by (document, root name hash) — k_jindex has compared the
//                 names —, a nested target through the parent key's entry, then the entry by binary
//                 search in the sorted keys (yc_read.h) or the element by binary search in the
//                 visible-length scan; sizes and lengths are differences of the scan; the value is
//                 sized with the shared writer (yc_json.h), a nested type from the sizing sweeps
//   k_rwrite      scalar values at their offsets; a nested type's brackets, and its container's
//                 position for k_jplace / k_jwrite, which then fill in only what was seeded
// Every index read from a view record is checked before use, every search is a bounded loop, no lane
// waits for another. What the bounds refuse is flagged and answered by the single calls.
#include "yc_common.h"
#define YC_JSON_DEVICE
#include "yc_read.h"

namespace yc {

namespace {

// The value a read names — element `elem` of segment s, or the one element of a YMap entry — written
// to `o` as view_map_get / view_array_get write it: its state (0 none, 1 written, 2 undefined). A
// nested type writes nothing here: `box` is its text.
__device__ int32_t read_value(const JsonArgs& a, const ViewSeg& s, bool entry, uint32_t elem, JText& o, uint32_t& flags, Box& box,
                              bool& is_type) {
  is_type = false;
  SegCursor c(a.bytes, s.b0, s.b1, s.ref, s.len, entry, (s.flags >> VS_HALF_SHIFT) & 3u);
  uint32_t rem[ANY_JSON_DEPTH];
  JStack<ANY_JSON_DEPTH> st(rem);
  JText skipped{nullptr, 0};
  for (uint32_t k = 0; k < elem; ++k) {  // (view_array_get steps the same cursor; elem < s.len)
    const uint32_t el = c.next(skipped, st);
    if (el == EL_BAD || el == EL_DEEP) { flags |= RF_OPEN; return 0; }
  }
  switch (c.next(o, st)) {
    case EL_OK: return 1;
    case EL_UNDEF: return 2;
    case EL_END: return 0;
    case EL_TYPE:
      box = type_box(a, s.unit + s.len - 1, c.type_ref);
      if (box.unres) { flags |= RF_OPEN; return 0; }
      is_type = true;
      return 1;
    default: flags |= RF_OPEN; return 0;  // EL_BAD, EL_DEEP
  }
}

__device__ __forceinline__ bool seeds(const Box& b) { return b.lo != VNONE && b.mode != BOX_XML; }

__global__ void k_rvisible(ReadArgs A) {
  const JsonArgs& a = A.j;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = a.ck + a.narr;
  if (i > n) return;
  uint32_t v = 0;
  if (i < a.ck) {
    const uint32_t ki = a.ord[i];
    if (ki < *a.nkeys && ki < a.ck) v = entry_live(a.keys[ki]) ? 1u : 0u;
  } else if (i < n) {
    const ViewSeg& s = a.segs[i - a.ck];
    if ((s.flags & VS_ITEM) && !(s.flags & VS_DELETED) && (s.flags & VS_COUNTABLE)) v = s.len;
  }
  A.vis[i] = v;
}

__global__ void k_rresolve(ReadArgs A) {
  const JsonArgs& a = A.j;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > A.nreads) return;
  if (r == A.nreads) { A.vsize[r] = 0; return; }
  const ReadReq q = A.reads[r];
  const bool map_op = q.op == RD_MAP_GET || q.op == RD_MAP_SIZE;
  uint32_t flags = 0, item = READ_NONE, elem = 0, size = 0;
  int32_t state = 0;
  uint64_t count = 0;
  do {
    if (q.root >= a.nreq) { flags = RF_OPEN; break; }
    if (a.rflag[q.root]) { flags = RF_NAME; break; }
    uint64_t g = a.reqs[q.root].rkey;
    if (q.pkey_len != READ_NONE) {  // resolve_parent: the type stored in the root map under the parent key
      const uint32_t p = find_entry(a, g, a.names + q.pkey_pos, q.pkey_len, flags);
      if (flags || p == READ_NONE) break;
      const ViewSeg& w = a.keys[a.ord[p]].win;
      if (!(w.flags & VS_SET) || (w.flags & VS_DELETED) || w.ref != REF_TYPE) break;
      if (w.b0 > w.b1 || w.b1 > a.nbytes) { flags = RF_OPEN; break; }
      JRd rd{a.bytes, w.b0, w.b1, true};
      const uint32_t tr = rd.vu();
      if (!rd.ok || tr != (map_op ? 1u : 0u)) break;
      g = (uint32_t)(w.unit + w.len - 1);
    }
    if (q.op == RD_MAP_GET) {
      const uint32_t p = find_entry(a, g, a.names + q.key_pos, q.key_len, flags);
      if (flags || p == READ_NONE) break;
      const ViewSeg& w = a.keys[a.ord[p]].win;
      if (!(w.flags & VS_SET) || (w.flags & VS_DELETED) || !(w.flags & VS_ITEM)) break;
      item = p;
    } else {
      const uint32_t lo = lower_bound_u64(a.gk, a.ck, g), hi = upper_bound_u64(a.gk, a.ck, g);
      if (q.op == RD_MAP_SIZE) { count = A.scan_v[hi] - A.scan_v[lo]; break; }
      const uint32_t kp = first_list(a, lo, hi);
      if (kp == VNONE) break;
      uint32_t x0 = 0, x1 = 0;
      if (!list_range(a, kp, x0, x1)) { flags = RF_OPEN; break; }
      const uint64_t* sv = A.scan_v + a.ck;
      const uint64_t total = sv[x1] - sv[x0];
      if (q.op == RD_ARRAY_LENGTH) { count = total; break; }
      if (q.index >= total) break;
      const uint64_t target = sv[x0] + q.index;
      // the last segment that starts at or before the element: the ones without a visible element in
      // front of it start where it does
      const uint32_t x = x0 + upper_bound_u64(sv + x0, x1 - x0 + 1, target) - 1;
      if (x < x0 || x >= x1 || target - sv[x] >= A.vis[a.ck + x]) { flags = RF_OPEN; break; }
      item = a.ck + x;
      elem = (uint32_t)(target - sv[x]);
    }
    if (a.state[item] != JS_SIZED) { flags = RF_OPEN; break; }  // (the sizing sweeps refused it or something nested in it)
    const bool entry = item < a.ck;
    const ViewSeg& s = entry ? a.keys[a.ord[item]].win : a.segs[item - a.ck];
    if (s.b0 > s.b1 || s.b1 > a.nbytes) { flags = RF_OPEN; break; }
    JText o{nullptr, 0};
    Box box{};
    bool is_type = false;
    state = read_value(a, s, entry, elem, o, flags, box, is_type);
    if (flags) break;
    const uint64_t bytes = is_type ? box.size : o.n;
    if (bytes > 0xFFFFFFF0ull) { flags = RF_SIZE; break; }
    if (is_type && seeds(box) && atomicCAS((box.mode == BOX_MAP ? a.own_m : a.own_a) + box.lo, VNONE, r) != VNONE) {
      flags = RF_SEED;
      break;
    }
    size = state == 1 ? (uint32_t)bytes : 0u;
  } while (false);
  if (flags) { state = 0; count = 0; size = 0; item = READ_NONE; }
  if (!flags && (q.op == RD_MAP_SIZE || q.op == RD_ARRAY_LENGTH)) state = 1;
  A.flags[r] = flags;
  A.states[r] = state;
  A.counts[r] = count;
  A.item[r] = item;
  A.elem[r] = elem;
  A.vsize[r] = size;
}

__global__ void k_rwrite(ReadArgs A) {
  const JsonArgs& a = A.j;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.nreads || A.flags[r] || A.states[r] != 1) return;
  const uint32_t item = A.item[r];
  if (item >= a.ck + a.narr) return;
  const uint64_t at = A.voffs[r], size = A.voffs[r + 1] - at;
  if (!size || at + size > a.out_cap) return;
  const bool entry = item < a.ck;
  const ViewSeg& s = entry ? a.keys[a.ord[item]].win : a.segs[item - a.ck];
  JText o{a.out, at, at + size};
  Box box{};
  bool is_type = false;
  uint32_t flags = 0;
  read_value(a, s, entry, A.elem[r], o, flags, box, is_type);
  if (!is_type || size < 2) return;
  a.out[at] = box.mode == BOX_MAP ? '{' : box.mode == BOX_ARRAY ? '[' : '"';
  a.out[at + size - 1] = box.mode == BOX_MAP ? '}' : box.mode == BOX_ARRAY ? ']' : '"';
  if (!seeds(box)) return;
  if (box.mode == BOX_MAP) { if (a.own_m[box.lo] == r) st64(&a.mbase[box.lo], at); }
  else if (a.own_a[box.lo] == r) st64(&a.abase[box.lo], at | (box.mode == BOX_TEXT ? TEXT_BIT : 0));
}

inline dim3 grid(uint64_t n) { return dim3((uint32_t)(n / 256 + 1)); }

}  // namespace

void launch_read_visible(const ReadArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_rvisible, grid((uint64_t)a.j.ck + a.j.narr + 1), dim3(256), 0, s, a);
}
void launch_read_resolve(const ReadArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_rresolve, grid((uint64_t)a.nreads + 1), dim3(256), 0, s, a); }
void launch_read_write(const ReadArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_rwrite, grid(a.nreads), dim3(256), 0, s, a); }

}  // namespace yc
