// yc_cache.hip — the fleet cache refresh on gfx950 (ycrdt_docs_cache): for every document the text
// of crdt.js's cache object `c`, { "<root>": <root's toJSON>, ... } with one member per live entry
// of the document's index map, from ONE multi-document merge. The host uploads one request per
// document, (document, index, map), so the front half of the fleet toJSON pass (json_front,
// yc_json.hip) runs unchanged: the keys sorted, every container of every document sized. The index
// entries are then sorted view keys, and the roots they name are root groups of the same array:
//   k_cmark     one lane per sorted key: is it a live entry of its document's index group; does its
//               root name differ from the key before it in the same hash group (two roots share a slot)
//   (scans)     ranks of the live entries; running count of the mixed marks
//   k_cmembers  one lane per live entry: the request it stands for — root key hashed from the entry's
//               name bytes in the batch buffer, kind from index_kind over the winner's content — the
//               root's item range (root_range), the name check, the member's size
//   (scan)      member offsets
//   k_cdocs     one lane per document: its text's size, its flags, its members counted
//   (scan)      document offsets; they come back with the flags in the pass's one size read-back
//   k_cwrite    braces, `"name":`, the roots' brackets and separators, and the roots' positions
//               handed to k_jplace / k_jwrite (yc_json.hip), which then run as they do for toJSON
// A document is flagged, and composed on the host from the same definitions (yc_cache.h, yc_host.cpp),
// when a member's root is unsized or shares its hash slot with another name, when the index holds a
// name past JSON_NAME_MAX (the device order stops there) or an unsized value, or past 4 GiB.
// Every loop is a binary search over ck or runs over a name's bytes; no lane waits for another.
#include "yc_common.h"
#define YC_JSON_DEVICE
#include "yc_cache.h"

namespace yc {

namespace {

__device__ __forceinline__ uint32_t doc_of_group(uint64_t g) { return (uint32_t)(g >> 32) & 0x7FFFFFFFu; }
__device__ __forceinline__ bool root_group(uint64_t g) { return (g >> 63) && g != NONE64; }

__device__ __forceinline__ bool same_bytes(const JsonArgs& a, uint32_t p0, uint32_t n0, uint32_t p1, uint32_t n1) {
  if (n0 != n1 || !in_bytes(a, p0, n0) || !in_bytes(a, p1, n1)) return false;
  for (uint32_t j = 0; j < n0; ++j)
    if (a.bytes[p0 + j] != a.bytes[p1 + j]) return false;
  return true;
}

// the view key at sorted position p (nullptr: none)
__device__ __forceinline__ const ViewKey* key_at(const JsonArgs& a, uint32_t p) {
  const uint32_t i = a.ord[p];
  return i < *a.nkeys && i < a.ck ? &a.keys[i] : nullptr;
}

__global__ void k_cmark(CacheArgs c) {
  const JsonArgs& a = c.j;
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p > a.ck) return;
  uint32_t live = 0, mixed = 0;
  if (p < a.ck) {
    const uint64_t g = a.gk[p];
    const ViewKey* K = key_at(a, p);
    if (K && root_group(g)) {
      if (p && a.gk[p - 1] == g) {
        const ViewKey* Q = key_at(a, p - 1);
        mixed = !Q || !same_bytes(a, K->name_pos, K->name_len, Q->name_pos, Q->name_len);
      }
      const uint32_t d = doc_of_group(g);
      live = d < a.nreq && a.reqs[d].rkey == g && entry_live(*K);
    }
    c.mkind[p] = 1;
  }
  c.live[p] = live;
  c.mixed[p] = mixed;
  c.msize[p] = 0;
}

// the request a live index entry stands for
__device__ __forceinline__ JsonReq member_request(const JsonArgs& a, const ViewKey& K, uint32_t d, uint32_t kind) {
  return JsonReq{(1ull << 63) | ((uint64_t)d << 32) | (fnv_key(a.bytes, K.psub_pos, K.psub_len) >> 1), K.psub_pos, K.psub_len, kind, 0};
}

__global__ void k_cmembers(CacheArgs c) {
  const JsonArgs& a = c.j;
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.ck || !c.live[p]) return;
  const ViewKey& K = *key_at(a, p);  // (live: k_cmark saw it)
  const uint64_t g = a.gk[p];
  const uint32_t d = doc_of_group(g);
  if (K.psub_len > JSON_NAME_MAX || !in_bytes(a, K.psub_pos, K.psub_len)) { atomicOr(&a.rflag[d], JR_INDEX); return; }
  const ViewSeg& s = K.win;
  const uint32_t kind = s.b0 <= s.b1 && s.b1 <= a.nbytes && index_kind(a.bytes, s.b0, s.b1, s.ref) ? 0u : 1u;
  const JsonReq q = member_request(a, K, d, kind);
  uint32_t flags = 0;
  // the keys of the root's hash group must all carry the entry's name
  const uint32_t klo = lower_bound_u64(a.gk, a.ck, q.rkey), khi = upper_bound_u64(a.gk, a.ck, q.rkey);
  if (klo < khi) {
    const ViewKey* R = key_at(a, klo);
    if (c.smixed[khi] - c.smixed[klo + 1] || !R || !same_bytes(a, R->name_pos, R->name_len, K.psub_pos, K.psub_len)) flags |= JR_NAME;
  }
  uint32_t lo, hi, kp;
  root_range(a, q, lo, hi, kp);
  if (a.scan_u[hi] - a.scan_u[lo]) flags |= JR_OPEN;
  JText o{nullptr, 0};
  cache_put_name(o, a.bytes + K.psub_pos, K.psub_len);
  const bool last = c.lrank[p + 1] == c.lrank[upper_bound_u64(a.gk, a.ck, g)];
  const uint64_t size = o.n + boxed(a.scan_c[hi] - a.scan_c[lo]) + (last ? 0 : 1);
  if (size > 0xFFFFFFF0ull) flags |= JR_SIZE;
  if (flags) { atomicOr(&a.rflag[d], flags); return; }
  c.msize[p] = (uint32_t)size;
  c.mkind[p] = kind;
}

__global__ void k_cdocs(CacheArgs c) {
  const JsonArgs& a = c.j;
  const uint32_t d = blockIdx.x * blockDim.x + threadIdx.x;
  if (d > a.nreq) return;
  a.rsize[d] = 0;
  if (d == a.nreq || a.rflag[d]) return;
  const uint64_t g = a.reqs[d].rkey;
  const uint32_t lo = lower_bound_u64(a.gk, a.ck, g), hi = upper_bound_u64(a.gk, a.ck, g);
  if (a.scan_u[hi] - a.scan_u[lo]) { a.rflag[d] = JR_INDEX; return; }
  const uint64_t size = 2 + (c.moffs[hi] - c.moffs[lo]);
  if (size > 0xFFFFFFF0ull) { a.rflag[d] = JR_SIZE; return; }
  a.rsize[d] = (uint32_t)size;
  if (c.lrank[hi] - c.lrank[lo]) atomicAdd(c.roots, c.lrank[hi] - c.lrank[lo]);
}

// lanes [0, ck): a member each; lanes [ck, ck + nreq): a document's braces
__global__ void k_cwrite(CacheArgs c) {
  const JsonArgs& a = c.j;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= a.ck) {
    const uint32_t d = t - a.ck;
    if (d >= a.nreq || a.rflag[d]) return;
    const uint64_t at = a.roffs[d], size = a.roffs[d + 1] - at;
    if (size < 2 || at + size > a.out_cap) return;
    a.out[at] = '{';
    a.out[at + size - 1] = '}';
    return;
  }
  const uint32_t p = t, n = c.msize[p];
  if (!c.live[p] || !n) return;
  const uint64_t g = a.gk[p];
  const uint32_t d = doc_of_group(g);
  if (a.rflag[d]) return;
  const ViewKey& K = *key_at(a, p);
  const uint32_t dlo = lower_bound_u64(a.gk, a.ck, g), dhi = upper_bound_u64(a.gk, a.ck, g);
  const uint64_t at = a.roffs[d] + 1 + (c.moffs[p] - c.moffs[dlo]);
  if (at + n >= a.roffs[d + 1] || a.roffs[d + 1] > a.out_cap) return;  // (the document's closer stands behind its members)
  JText o{a.out, at, a.out_cap};
  cache_put_name(o, a.bytes + K.psub_pos, K.psub_len);
  const bool last = c.lrank[p + 1] == c.lrank[dhi];
  const uint64_t used = o.n - at + (last ? 0 : 1);
  if (used + 2 > n) return;
  const uint64_t size = n - used, root = o.n;
  const JsonReq q = member_request(a, K, d, c.mkind[p]);
  a.out[root] = q.kind == 0 ? '{' : '[';
  a.out[root + size - 1] = q.kind == 0 ? '}' : ']';
  if (!last) a.out[root + size] = ',';
  uint32_t lo, hi, kp;
  root_range(a, q, lo, hi, kp);
  if (q.kind == 0) {
    if (lo < hi) st64(&a.mbase[lo], root);
  } else if (kp != VNONE) {
    st64(&a.abase[kp], root);
  }
}

inline dim3 grid(uint64_t n) { return dim3((uint32_t)(n / 256 + 1)); }

}  // namespace

void launch_cache_mark(const CacheArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_cmark, grid((uint64_t)a.j.ck + 1), dim3(256), 0, s, a); }
void launch_cache_members(const CacheArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_cmembers, grid(a.j.ck), dim3(256), 0, s, a); }
void launch_cache_docs(const CacheArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_cdocs, grid((uint64_t)a.j.nreq + 1), dim3(256), 0, s, a); }
void launch_cache_write(const CacheArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_cwrite, grid((uint64_t)a.j.ck + a.j.nreq), dim3(256), 0, s, a); }

}  // namespace yc
