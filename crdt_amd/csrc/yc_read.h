// yc_read.h — fleet point reads (ycrdt_docs_read): YMap.get / size and YArray.get / length for many
// documents over the view of ONE multi-document merge (yc_read.hip).
//
// The fleet toJSON front half (yc_json.hip) leaves the view keys sorted by (container, entry name
// bytes zero-padded to the ordering's bound, name length, slot). The comparator of that order and
// the search for one entry name inside one container are defined here once, for the device and for
// the host (tests/csrc/read_order_main.cpp runs them under sanitizers).
#pragma once
#include <cstdint>

#include "yc_parse.h"  // YC_HD

namespace yc {

constexpr uint32_t READ_NAME_MAX = 64;       // = JSON_NAME_MAX: the name bytes the radix passes order by
constexpr uint32_t READ_NONE = 0xFFFFFFFFu;

// read flags: any one sends the read to the single call
constexpr uint32_t RF_NAME = 1u;     // a root of another name shares the root's hash slot
constexpr uint32_t RF_LONG = 2u;     // an entry name past READ_NAME_MAX stands where the request's would
constexpr uint32_t RF_OPEN = 4u;     // the value is refused by the writer's bounds, or a view record is out of range
constexpr uint32_t RF_SIZE = 8u;     // its text would pass 4 GiB
constexpr uint32_t RF_SEED = 16u;    // another read's value is the same nested type

// (group, name, length) x against y in the order the radix passes produce: group, then the first
// READ_NAME_MAX name bytes big-endian and zero padded, then the whole name's length. <0, 0, >0.
// `ly_order`: the length y sorts by, where it is not the ly bytes that ny holds (a search bound).
YC_HD inline int read_order_cmp(uint64_t gx, const uint8_t* nx, uint32_t lx, uint64_t gy, const uint8_t* ny, uint32_t ly,
                                uint32_t ly_order) {
  if (gx != gy) return gx < gy ? -1 : 1;
  for (uint32_t j = 0; j < READ_NAME_MAX && (j < lx || j < ly); ++j) {
    const uint32_t a = j < lx ? nx[j] : 0u, b = j < ly ? ny[j] : 0u;
    if (a != b) return a < b ? -1 : 1;
  }
  return lx != ly_order ? (lx < ly_order ? -1 : 1) : 0;
}
YC_HD inline int read_order_cmp(uint64_t gx, const uint8_t* nx, uint32_t lx, uint64_t gy, const uint8_t* ny, uint32_t ly) {
  return read_order_cmp(gx, nx, lx, gy, ny, ly, ly);
}

// whether two names agree in their first READ_NAME_MAX bytes, zero padded
YC_HD inline bool read_same_padded(const uint8_t* nx, uint32_t lx, const uint8_t* ny, uint32_t ly) {
  for (uint32_t j = 0; j < READ_NAME_MAX && (j < lx || j < ly); ++j)
    if ((j < lx ? nx[j] : 0u) != (j < ly ? ny[j] : 0u)) return false;
  return true;
}

// First sorted position in [0, n) whose entry is not below (g, name, len sorting as len_order). `E`:
// group(p), name(p), len(p) of the entry at sorted position p (name(p) is read for min(len(p),
// READ_NAME_MAX) bytes).
template <class E>
YC_HD inline uint32_t read_lower_bound(const E& e, uint32_t n, uint64_t g, const uint8_t* name, uint32_t len, uint32_t len_order) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {  // (at most 32 steps)
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (read_order_cmp(e.group(mid), e.name(mid), e.len(mid), g, name, len, len_order) < 0) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// The first entry named (name, len) in container g: its sorted position, or READ_NONE.
// `ambiguous`: the request is past READ_NAME_MAX, or the container holds a name past READ_NAME_MAX
// with the request's padded bytes in front — the order does not tell such names from one another,
// so the caller must not decide.
template <class E>
YC_HD inline uint32_t read_find_name(const E& e, uint32_t n, uint64_t g, const uint8_t* name, uint32_t len, bool& ambiguous) {
  ambiguous = len > READ_NAME_MAX;
  if (ambiguous) return READ_NONE;
  // the longest name of the same group and padded bytes stands last among them
  const uint32_t q = read_lower_bound(e, n, g, name, len, 0xFFFFFFFFu);
  const uint32_t last = q < n && read_order_cmp(e.group(q), e.name(q), e.len(q), g, name, len, 0xFFFFFFFFu) == 0 ? q : q - 1;  // (q == 0: READ_NONE)
  if (last < n && e.group(last) == g && e.len(last) > READ_NAME_MAX && read_same_padded(e.name(last), e.len(last), name, len))
    ambiguous = true;
  const uint32_t p = read_lower_bound(e, n, g, name, len, len);
  if (p >= n || read_order_cmp(e.group(p), e.name(p), e.len(p), g, name, len) != 0) return READ_NONE;
  return p;
}

}  // namespace yc

#if defined(__HIP__) || defined(__HIPCC__)
#include "yc_json.h"

namespace yc {

static_assert(READ_NAME_MAX == JSON_NAME_MAX, "the search compares what the radix passes ordered");

enum : uint32_t { RD_MAP_GET = 0, RD_MAP_SIZE = 1, RD_ARRAY_GET = 2, RD_ARRAY_LENGTH = 3 };  // = YCRDT_READ_*

struct ReadReq {             // one distinct read
  uint64_t index;            // RD_ARRAY_GET
  uint32_t root;             // its (document, root) among JsonArgs::reqs (k_jindex checks the name)
  uint32_t op;               // RD_*
  uint32_t pkey_pos, pkey_len;  // the parent key in the name pool (pkey_len == READ_NONE: the root type itself)
  uint32_t key_pos, key_len;    // RD_MAP_GET
};

struct ReadArgs {
  JsonArgs j;                // after the toJSON front half: sorted keys, sizes and their scans
  const ReadReq* reads;
  uint32_t nreads;
  uint32_t* vis;             // [n + 1] key: 1 = a live entry; segment: its visible elements
  uint64_t* scan_v;          // [n + 1]
  uint32_t* item;            // [nreads] the item holding the value (READ_NONE: none)
  uint32_t* elem;            // [nreads] RD_ARRAY_GET: the element's offset inside its segment
  uint32_t* vsize;           // [nreads + 1] bytes of the value's text
  uint64_t* voffs;           // [nreads + 1]
  uint64_t* counts;          // [nreads]
  int32_t* states;           // [nreads]
  uint32_t* flags;           // [nreads] RF_*
};

void launch_read_visible(const ReadArgs& a, hipStream_t s);   // live flags and visible lengths (one scan follows)
void launch_read_resolve(const ReadArgs& a, hipStream_t s);   // the item of every read, its size, sizes and lengths
void launch_read_write(const ReadArgs& a, hipStream_t s);     // scalar values; brackets and seeds of nested types

}  // namespace yc
#ifdef YC_JSON_DEVICE
// ---- the entry search over the sorted view keys, shared by the point-read kernels (yc_read.hip)
// and the write kernels (yc_write.hip)
namespace yc {
namespace {

struct KeyOrder {            // the sorted view keys as yc_read.h's searches read them (k_jsort_key's names)
  const JsonArgs& a;
  __device__ __forceinline__ const ViewKey* key(uint32_t p) const {
    const uint32_t i = a.ord[p];
    return i < *a.nkeys && i < a.ck ? &a.keys[i] : nullptr;
  }
  __device__ __forceinline__ bool named(const ViewKey* K) const { return K && (K->flags & VK_PSUB) && in_bytes(a, K->psub_pos, K->psub_len); }
  __device__ __forceinline__ uint64_t group(uint32_t p) const { return a.gk[p]; }
  __device__ __forceinline__ uint32_t len(uint32_t p) const {
    const ViewKey* K = key(p);
    return named(K) ? K->psub_len : 0u;
  }
  __device__ __forceinline__ const uint8_t* name(uint32_t p) const {
    const ViewKey* K = key(p);
    return named(K) ? a.bytes + K->psub_pos : a.bytes;
  }
};

// the YMap entry `name` of container g: its sorted position (the lowest slot, as HostView::index keeps), or READ_NONE
__device__ uint32_t find_entry(const JsonArgs& a, uint64_t g, const uint8_t* name, uint32_t len, uint32_t& flags) {
  const KeyOrder e{a};
  bool ambiguous = false;
  uint32_t p = read_find_name(e, a.ck, g, name, len, ambiguous);
  if (ambiguous) { flags |= RF_LONG; return READ_NONE; }
  // a list key sorts as the empty name: the entry "" may stand behind it (bounded by the keys)
  for (; p < a.ck; ++p) {
    if (read_order_cmp(e.group(p), e.name(p), e.len(p), g, name, len) != 0) return READ_NONE;
    const ViewKey* K = e.key(p);
    if (!K) return READ_NONE;
    if (!(K->flags & VK_PSUB)) continue;
    if (!e.named(K)) { flags |= RF_OPEN; return READ_NONE; }
    return p;
  }
  return READ_NONE;
}

}  // namespace
}  // namespace yc
#endif
#endif
