// yc_json.hip — fleet toJSON on gfx950: the JSON text of many (document, root, kind) requests,
// written on the device over the view (yc_view.hip) of ONE multi-document merge. The host never
// sees the state bytes or the view records; it gets the blob and the offsets (ycrdt_docs_json).
//
// Items are the view keys (a YMap entry each) in the host's order and the list segments in document
// order, so that every container — a root map, a nested YMap, a YArray / YText list — is a
// contiguous item range and its size is a difference of one exclusive scan:
//   k_jsort_key   radix keys of the stable passes that order the keys by (container, entry name
//                 bytes, name length, slot) — HostView::index's order
//   k_jindex      inverse order; every root key checks the name of the requests that share its slot
//   k_jsize       sweep 1, by level bottom-up: an item's bytes in its container (`"name":value,` /
//                 `v,v,`); an item holding a nested type is sized once the scan of the round before
//                 has sized all of the type's members (JSON_DEPTH_MAX + 1 rounds, a scan after each)
//   k_jrequests   the size of every request (sweep 2: their exclusive scan gives the offsets)
//   k_jroots      root brackets and the root containers' positions
//   k_jplace      offsets top-down, one level per launch: an item placed in its container hands the
//                 position of its nested type's opener to that type's container
//   k_jwrite      sweep 3: every placed item writes its own bytes, all in parallel
// Whatever the bounds refuse (entry names past JSON_NAME_MAX, types nested past JSON_DEPTH_MAX, an
// `any` past ANY_JSON_DEPTH, malformed content) leaves its item unsized, which leaves every
// container above it unsized: the request is flagged and the host answers it through ycrdt_doc_json,
// whose writer (yc_host.cpp) is built from the same value writer and segment cursor (yc_json.h).
#include "yc_common.h"
#define YC_JSON_DEVICE  // the device helpers shared with yc_read.hip
#include "yc_json.h"

namespace yc {

namespace {

// the container a view key belongs to: its parent type item's unit, or (document, root name)
__device__ __forceinline__ uint64_t group_key(const JsonArgs& a, const ViewKey& K) {
  if (K.parent_unit != VNONE) return K.parent_unit;
  const uint32_t r = K.slot < a.ck ? a.krep[K.slot] : VNONE;
  if (r == VNONE || !in_bytes(a, K.name_pos, K.name_len)) return NONE64;
  const uint32_t doc = a.cl_doc ? a.cl_doc[a.g_cidx[r]] : 0u;
  return (1ull << 63) | ((uint64_t)(doc & 0x7FFFFFFFu) << 32) | (fnv_key(a.bytes, K.name_pos, K.name_len) >> 1);  // (the host hashes the requests alike)
}

__global__ void k_jsort_key(JsonArgs a, uint32_t pass, const uint32_t* __restrict__ ord_in, uint64_t* __restrict__ key) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.ck) return;
  const uint32_t i = ord_in ? ord_in[p] : p;
  if (pass == 0) a.ord[p] = p;  // (the first pass sorts the identity)
  if (i >= *a.nkeys || i >= a.ck) { key[p] = NONE64; return; }
  const ViewKey& K = a.keys[i];
  const bool ps = (K.flags & VK_PSUB) && in_bytes(a, K.psub_pos, K.psub_len);
  const uint32_t len = ps ? K.psub_len : 0u;
  uint64_t k = 0;
  if (pass == 0) {
    k = ((uint64_t)len << 32) | K.slot;
  } else if (pass <= JSON_NAME_MAX / 8) {  // name bytes [8c, 8c + 8), big-endian, zero padded: the last chunk first
    const uint32_t c = JSON_NAME_MAX / 8 - pass;
    for (uint32_t j = 0; j < 8; ++j) {
      const uint32_t x = 8 * c + j;
      k = (k << 8) | (x < len ? a.bytes[K.psub_pos + x] : 0u);
    }
  } else {
    k = group_key(a, K);
  }
  key[p] = k;
}

__global__ void k_jindex(JsonArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.ck) return;
  const uint32_t i = a.ord[p];
  if (i >= *a.nkeys || i >= a.ck) return;
  a.inv[i] = p;
  const uint64_t g = a.gk[p];
  if (!(g >> 63) || g == NONE64) return;
  // the requests of this document and name hash: each must name this root
  const ViewKey& K = a.keys[i];
  uint32_t lo = 0, hi = a.nreq;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a.reqs[mid].rkey < g) lo = mid + 1; else hi = mid;
  }
  for (uint32_t r = lo; r < a.nreq && a.reqs[r].rkey == g; ++r) {
    const JsonReq& q = a.reqs[r];
    bool same = q.name_len == K.name_len;
    for (uint32_t j = 0; same && j < K.name_len; ++j) same = a.names[q.name_pos + j] == a.bytes[K.name_pos + j];
    if (!same) atomicOr(&a.rflag[r], JR_NAME);
  }
}

// The elements of a visible view segment as JSON (SegCursor, yc_json.h). `entry`: a YMap entry's
// value — its one element, nothing behind it, EM_OMIT when it is undefined; otherwise every
// element followed by a separator, except the one that would stand where the container closes.
__device__ __forceinline__ uint32_t emit_seg(const JsonArgs& a, const ViewSeg& s, bool entry, bool scans, JText& o, uint64_t cend) {
  if (s.b0 > s.b1 || s.b1 > a.nbytes) return EM_REFUSED;
  SegCursor c(a.bytes, s.b0, s.b1, s.ref, s.len, entry, (s.flags >> VS_HALF_SHIFT) & 3u);
  uint32_t rem[ANY_JSON_DEPTH];
  JStack<ANY_JSON_DEPTH> st(rem);
  for (;;) {
    switch (c.next(o, st)) {
      case EL_OK: break;
      case EL_UNDEF:
        if (entry) return EM_OMIT;
        o.lit("null");
        break;
      case EL_END: return entry ? EM_OMIT : EM_OK;  // (an entry returns at its element: this one has none)
      case EL_TYPE: {
        if (!scans) return EM_PENDING;
        const Box b = type_box(a, s.unit + s.len - 1, c.type_ref);
        if (b.unres) return EM_PENDING;
        if (o.o) {
          const uint32_t open = b.mode == BOX_MAP ? '{' : b.mode == BOX_ARRAY ? '[' : '"';
          const uint32_t close = b.mode == BOX_MAP ? '}' : b.mode == BOX_ARRAY ? ']' : '"';
          JText t{o.o, o.n, o.cap};
          t.ch(open);
          t.n = o.n + b.size - 1;
          t.ch(close);
        }
        o.n += b.size;
        break;
      }
      default: return EM_REFUSED;  // EL_BAD, EL_DEEP
    }
    if (entry) return EM_OK;
    if (!o.o || o.n != cend) o.ch(',');
  }
}

// sweep 1, one level: sizes of the items still open
__global__ void k_jsize(JsonArgs a, uint32_t round) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = a.ck + a.narr;
  if (i > n) return;
  if (i == n) { a.contrib[n] = 0; a.unres[n] = 0; a.tcontrib[a.narr] = 0; return; }
  if (round && a.state[i] != JS_OPEN) return;
  uint32_t st = JS_SIZED, bytes = 0;
  JText o{nullptr, 0};
  uint32_t em = EM_OMIT;
  if (i < a.ck) {
    const uint32_t ki = a.ord[i];
    if (ki < *a.nkeys && ki < a.ck) {
      const ViewKey& K = a.keys[ki];
      if (entry_live(K)) {
        if (K.psub_len > JSON_NAME_MAX || !in_bytes(a, K.psub_pos, K.psub_len)) {
          em = EM_REFUSED;
        } else {
          json_put_str(o, a.bytes + K.psub_pos, K.psub_len);
          o.ch(':');
          em = emit_seg(a, K.win, true, round != 0, o, NONE64);
          o.ch(',');
        }
      }
    }
  } else {
    const ViewSeg& s = a.segs[i - a.ck];
    if (round == 0) {  // what the segment adds to a YText: its escaped string, no quotes
      uint32_t t = 0;
      if (!(s.flags & VS_DELETED) && (s.flags & VS_ITEM) && s.ref == REF_STRING && s.b0 <= s.b1 && s.b1 <= a.nbytes) {
        JText q{nullptr, 0};
        json_put_piece(q, a.bytes + s.b0, s.b1 - s.b0, (s.flags >> VS_HALF_SHIFT) & 3u);
        t = q.n > 0xFFFFFFF0ull ? 0u : (uint32_t)q.n;
        if (q.n > 0xFFFFFFF0ull) em = EM_REFUSED;
      }
      a.tcontrib[i - a.ck] = t;
    }
    if (em != EM_REFUSED && member_live(s)) em = emit_seg(a, s, false, round != 0, o, NONE64);
  }
  if (em == EM_OK) {
    if (o.n > 0xFFFFFFF0ull) st = JS_REFUSED; else bytes = (uint32_t)o.n;
  } else if (em == EM_PENDING) {
    st = JS_OPEN;
  } else if (em == EM_REFUSED) {
    st = JS_REFUSED;
  }
  a.state[i] = st;
  a.contrib[i] = bytes;
  a.unres[i] = st != JS_SIZED;
}

__global__ void k_jrequests(JsonArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > a.nreq) return;
  if (r == a.nreq) { a.rsize[r] = 0; return; }
  a.rsize[r] = 0;
  if (a.rflag[r]) return;
  uint32_t lo, hi, kp;
  root_range(a, a.reqs[r], lo, hi, kp);
  if (a.scan_u[hi] - a.scan_u[lo]) { a.rflag[r] = JR_OPEN; return; }
  const uint64_t size = boxed(a.scan_c[hi] - a.scan_c[lo]);
  if (size > 0xFFFFFFF0ull) { a.rflag[r] = JR_SIZE; return; }
  a.rsize[r] = (uint32_t)size;
}

__global__ void k_jroots(JsonArgs a) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= a.nreq || a.rflag[r]) return;
  const JsonReq& q = a.reqs[r];
  const uint64_t at = a.roffs[r], size = a.roffs[r + 1] - at;
  if (size < 2 || at + size > a.out_cap) return;
  a.out[at] = q.kind == 0 ? '{' : '[';
  a.out[at + size - 1] = q.kind == 0 ? '}' : ']';
  uint32_t lo, hi, kp;
  root_range(a, q, lo, hi, kp);
  if (q.kind == 0) {
    if (lo < hi) st64(&a.mbase[lo], at);
  } else if (kp != VNONE) {
    st64(&a.abase[kp], at);
  }
}

// the list key (sorted position) a segment item belongs to
__device__ __forceinline__ uint32_t list_of_seg(const JsonArgs& a, uint32_t sp) {
  if (!a.nlists) return VNONE;
  uint32_t lo = 0, hi = a.nlists;  // last list l with y_lstart[l] <= sp
  while (hi - lo > 1) { const uint32_t m = (lo + hi) >> 1; if (a.y_lstart[m] <= sp) lo = m; else hi = m; }
  const uint32_t slot = a.y_keys[a.y_lstart[lo]];
  if (slot >= a.ck) return VNONE;
  const uint32_t ki = a.kmap[slot];
  if (ki == VNONE || ki >= a.ck) return VNONE;
  return a.inv[ki];
}

// offsets, one level: an item whose container has a position takes its own, and hands the position
// of its nested type's opener on to that type's container
__global__ void k_jplace(JsonArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = a.ck + a.narr;
  if (i >= n || a.apos[i] != NONE64) return;
  uint64_t at = NONE64, end = NONE64;
  const ViewSeg* sg = nullptr;
  uint64_t vpos = 0;
  uint32_t owner = VNONE;  // (point reads: the read this item's container was placed for)
  if (i < a.ck) {
    if (!a.contrib[i]) return;
    const uint64_t g = a.gk[i];
    const uint32_t lo = lower_bound_u64(a.gk, a.ck, g), hi = upper_bound_u64(a.gk, a.ck, g);
    const uint64_t base = ld64(&a.mbase[lo]);
    if (base == NONE64) return;
    if (a.own_m) { __threadfence(); owner = __hip_atomic_load(&a.own_m[lo], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    at = base + 1 + (a.scan_c[i] - a.scan_c[lo]);
    end = base + (a.scan_c[hi] - a.scan_c[lo]);  // = base + boxed(..) - 1
    const ViewKey& K = a.keys[a.ord[i]];
    sg = &K.win;
    JText o{nullptr, 0};
    json_put_str(o, a.bytes + K.psub_pos, K.psub_len);
    vpos = at + o.n + 1;
  } else {
    const uint32_t sp = i - a.ck;
    const uint32_t kp = list_of_seg(a, sp);
    if (kp == VNONE || kp >= a.ck) return;
    const uint64_t base = ld64(&a.abase[kp]);
    if (base == NONE64) return;
    if (a.own_a) { __threadfence(); owner = __hip_atomic_load(&a.own_a[kp], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    uint32_t x0 = 0, x1 = 0;
    if (!list_range(a, kp, x0, x1) || sp < x0 || sp >= x1) return;
    if (base & TEXT_BIT) {
      if (!a.tcontrib[sp]) return;
      a.apos[i] = (base & ~TEXT_BIT) + 1 + (a.scan_t[sp] - a.scan_t[x0]);
      a.cend[i] = NONE64;
      return;
    }
    if (!a.contrib[i]) return;
    at = base + 1 + (a.scan_c[i] - a.scan_c[a.ck + x0]);
    end = base + (a.scan_c[a.ck + x1] - a.scan_c[a.ck + x0]);
    sg = &a.segs[sp];
    vpos = at;
  }
  a.cend[i] = end;
  a.apos[i] = at;
  if (sg->ref != REF_TYPE) return;
  JRd r{a.bytes, sg->b0, sg->b1, true};
  const uint32_t tr = r.vu();
  if (!r.ok) return;
  const Box b = type_box(a, sg->unit + sg->len - 1, tr);
  if (b.lo == VNONE || b.mode == BOX_XML) return;
  if (a.own_m) {  // a container another read seeded keeps that read's position: this read's text has a hole there
    const uint32_t prev = atomicCAS((b.mode == BOX_MAP ? a.own_m : a.own_a) + b.lo, VNONE, owner);
    if (prev != VNONE && prev != owner) {
      if (owner < a.nown) atomicOr(&a.oflag[owner], 1u);
      return;
    }
    __threadfence();
  }
  if (b.mode == BOX_MAP) st64(&a.mbase[b.lo], vpos);
  else st64(&a.abase[b.lo], vpos | (b.mode == BOX_TEXT ? TEXT_BIT : 0));
}

// sweep 3: every placed item writes its bytes
__global__ void k_jwrite(JsonArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t n = a.ck + a.narr;
  if (i >= n) return;
  const uint64_t at = a.apos[i];
  if (at == NONE64 || at >= a.out_cap) return;
  const uint64_t end = a.cend[i];
  JText o{a.out, at, a.out_cap};
  if (i < a.ck) {
    const ViewKey& K = a.keys[a.ord[i]];
    json_put_str(o, a.bytes + K.psub_pos, K.psub_len);
    o.ch(':');
    emit_seg(a, K.win, true, true, o, end);
    if (o.n != end) o.ch(',');
    return;
  }
  const ViewSeg& s = a.segs[i - a.ck];
  if (end == NONE64) {  // a YText member: the escaped string between the type's quotes
    json_put_piece(o, a.bytes + s.b0, s.b1 - s.b0, (s.flags >> VS_HALF_SHIFT) & 3u);
    return;
  }
  emit_seg(a, s, false, true, o, end);
}

inline dim3 grid(uint64_t n) { return dim3((uint32_t)(n / 256 + 1)); }

}  // namespace

void launch_json_sort_key(const JsonArgs& a, uint32_t pass, const uint32_t* ord_in, uint64_t* key, hipStream_t s) {
  hipLaunchKernelGGL(k_jsort_key, grid(a.ck), dim3(256), 0, s, a, pass, ord_in, key);
}
void launch_json_index(const JsonArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_jindex, grid(a.ck), dim3(256), 0, s, a); }
void launch_json_size(const JsonArgs& a, uint32_t round, hipStream_t s) {
  hipLaunchKernelGGL(k_jsize, grid((uint64_t)a.ck + a.narr + 1), dim3(256), 0, s, a, round);
}
void launch_json_requests(const JsonArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_jrequests, grid(a.nreq + 1), dim3(256), 0, s, a); }
void launch_json_roots(const JsonArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_jroots, grid(a.nreq), dim3(256), 0, s, a); }
void launch_json_place(const JsonArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_jplace, grid((uint64_t)a.ck + a.narr), dim3(256), 0, s, a); }
void launch_json_write(const JsonArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_jwrite, grid((uint64_t)a.ck + a.narr), dim3(256), 0, s, a); }

}  // namespace yc
