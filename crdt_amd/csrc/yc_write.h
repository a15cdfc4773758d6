// yc_write.h — fleet writes (ycrdt_docs_write): YMap.set / delete and YArray.insert / push / delete for
// many documents over the view of ONE multi-document merge (yc_write.hip).
//
// The bytes of a local op's update are defined here once, for the device and for the host
// (tests/csrc/write_bytes_main.cpp runs them under sanitizers): the one-struct update of an item
// (Item.write, Y@80416, between the update's header and an empty delete set) and the delete-set-only
// update. Each comes as a sizing call and a writing call over a plain byte pointer. yc_host.cpp's
// write_item_update / write_ds_update are the reference they are checked against.
#pragma once
#include <cstdint>

#include "yc_parse.h"  // YC_HD

namespace yc {

constexpr uint32_t WRITE_RANGES_MAX = 8;     // visible segments one array delete may touch on the device
constexpr uint32_t WRITE_NONE = 0xFFFFFFFFu;

// bytes appended at o + n, or only counted (o == nullptr); nothing is written at or past `cap`
struct WBytes {
  uint8_t* o;
  uint64_t n, cap;
  YC_HD void u8(uint32_t v) {
    if (o && n < cap) o[n] = (uint8_t)v;
    ++n;
  }
  YC_HD void vu(uint32_t v) {  // lib0 writeVarUint
    while (v > 0x7Fu) { u8(0x80u | (v & 0x7Fu)); v >>= 7; }
    u8(v);
  }
  YC_HD void raw(const uint8_t* p, uint32_t len) {
    for (uint32_t i = 0; i < len; ++i) u8(p[i]);
  }
  YC_HD void str(const uint8_t* p, uint32_t len) { vu(len); raw(p, len); }
};

struct WId { uint32_t client, clock; };

// One new item. The parent is written only when there is neither origin: the root type's name, or
// the id of the type item it lives in; the entry key behind it. The content is `lead` as a varUint
// (ContentAny: the number of values; ContentType: the type ref) and then `content` as it stands.
struct WItem {
  WId id;
  uint32_t ref;              // content ref (info bits 0-4)
  bool has_origin, has_right, parent_item, has_key;
  WId origin, right, parent;
  const uint8_t* root;
  uint32_t root_len;
  const uint8_t* key;
  uint32_t key_len;
  uint32_t lead;
  const uint8_t* content;
  uint32_t content_len;
};

YC_HD inline void item_update_put(WBytes& w, const WItem& it) {
  w.vu(1);  // one client
  w.vu(1);  // one struct
  w.vu(it.id.client);
  w.vu(it.id.clock);
  w.u8((it.ref & 31u) | (it.has_origin ? 0x80u : 0u) | (it.has_right ? 0x40u : 0u) | (it.has_key ? 0x20u : 0u));
  if (it.has_origin) { w.vu(it.origin.client); w.vu(it.origin.clock); }
  if (it.has_right) { w.vu(it.right.client); w.vu(it.right.clock); }
  if (!it.has_origin && !it.has_right) {
    if (it.parent_item) { w.vu(0); w.vu(it.parent.client); w.vu(it.parent.clock); }
    else { w.vu(1); w.str(it.root, it.root_len); }
    if (it.has_key) w.str(it.key, it.key_len);
  }
  w.vu(it.lead);
  w.raw(it.content, it.content_len);
  w.vu(0);  // delete set: no clients
}
YC_HD inline uint64_t item_update_size(const WItem& it) {
  WBytes w{nullptr, 0, 0};
  item_update_put(w, it);
  return w.n;
}
// writes item_update_size(it) bytes at o (at most cap): the bytes written
YC_HD inline uint64_t item_update_write(uint8_t* o, uint64_t cap, const WItem& it) {
  WBytes w{o, 0, cap};
  item_update_put(w, it);
  return w.n;
}

struct WRange { uint32_t client, clock, len; };

// The ranges as write_ds_update orders them: sorted by (client, clock, len), ranges of one client
// adjacent in clock merged. In place, n <= WRITE_RANGES_MAX (an insertion sort); the ranges left.
YC_HD inline uint32_t ds_ranges_merge(WRange* r, uint32_t n) {
  for (uint32_t i = 1; i < n && i < WRITE_RANGES_MAX; ++i) {
    const WRange x = r[i];
    uint32_t j = i;
    for (; j > 0; --j) {
      const WRange& y = r[j - 1];
      const bool above = y.client != x.client ? y.client > x.client : y.clock != x.clock ? y.clock > x.clock : y.len > x.len;
      if (!above) break;
      r[j] = y;
    }
    r[j] = x;
  }
  uint32_t m = 0;
  for (uint32_t i = 0; i < n && i < WRITE_RANGES_MAX; ++i) {
    if (m && r[m - 1].client == r[i].client && r[m - 1].clock + r[m - 1].len == r[i].clock) r[m - 1].len += r[i].len;
    else r[m++] = r[i];
  }
  return m;
}

// the delete-set-only update of the ranges r[0, n), n <= WRITE_RANGES_MAX, in any order
YC_HD inline void ds_update_put(WBytes& w, const WRange* r, uint32_t n) {
  WRange m[WRITE_RANGES_MAX];
  if (n > WRITE_RANGES_MAX) n = WRITE_RANGES_MAX;
  for (uint32_t i = 0; i < n; ++i) m[i] = r[i];
  n = ds_ranges_merge(m, n);
  uint32_t clients = 0;
  for (uint32_t i = 0; i < n; ++i)
    if (i == 0 || m[i].client != m[i - 1].client) ++clients;
  w.vu(0);  // no structs
  w.vu(clients);
  for (uint32_t i = 0; i < n;) {
    uint32_t j = i + 1;
    while (j < n && m[j].client == m[i].client) ++j;
    w.vu(m[i].client);
    w.vu(j - i);
    for (; i < j; ++i) { w.vu(m[i].clock); w.vu(m[i].len); }
  }
}
YC_HD inline uint64_t ds_update_size(const WRange* r, uint32_t n) {
  WBytes w{nullptr, 0, 0};
  ds_update_put(w, r, n);
  return w.n;
}
YC_HD inline uint64_t ds_update_write(uint8_t* o, uint64_t cap, const WRange* r, uint32_t n) {
  WBytes w{o, 0, cap};
  ds_update_put(w, r, n);
  return w.n;
}

}  // namespace yc

#if defined(__HIP__) || defined(__HIPCC__)
#include "yc_read.h"

namespace yc {

enum : uint32_t { WR_MAP_SET = 0, WR_MAP_SET_TYPE = 1, WR_MAP_DELETE = 2, WR_ARRAY_INSERT = 3, WR_ARRAY_PUSH = 4, WR_ARRAY_DELETE = 5 };  // = YCRDT_WRITE_*

constexpr uint32_t WF_RANGES = 32u;  // beside the reads' RF_*: an array delete touches more than WRITE_RANGES_MAX visible segments

// why an op fails with YCRDT_E_ARG (the single call's message)
enum : int32_t { WHY_OK = 0, WHY_NO_TYPE = 1, WHY_MISMATCH = 2, WHY_LENGTH = 3 };

struct WriteReq {            // one op of the device path
  uint32_t root;             // its (document, root) among JsonArgs::reqs (k_jindex checks the name)
  uint32_t op;               // WR_*
  uint32_t pkey_pos, pkey_len;  // the parent key in the name pool (pkey_len == READ_NONE: the root type itself)
  uint32_t key_pos, key_len;    // map ops
  uint32_t client, clock;    // the new item's id (the host hands the clocks out in advance)
  uint32_t index, length;    // INSERT: index; DELETE: index, length
  uint32_t lead;             // MAP_SET: 1; MAP_SET_TYPE: the type ref; INSERT / PUSH: the number of values
  uint32_t any_pos, any_len; // the values' bytes in the name pool
};

struct WritePlan {           // what k_wplan found for k_wwrite
  uint32_t kind;             // 0 nothing, 1 an item, 2 a delete set
  uint32_t has;              // 1 origin, 2 right origin, 4 the parent is an item
  WId origin, right, parent;
  uint32_t nr;
  WRange r[WRITE_RANGES_MAX];
};

struct WriteArgs {
  JsonArgs j;                // after the toJSON front half: the sorted keys
  const WriteReq* ops;
  uint32_t nops;
  const uint32_t* vis;       // [n + 1] k_rvisible
  const uint64_t* scan_v;    // [n + 1]
  WritePlan* plan;           // [nops]
  uint32_t* size;            // [nops + 1] bytes of the op's update
  uint64_t* offs;            // [nops + 1]
  int32_t* why;              // [nops] WHY_*
  uint32_t* flags;           // [nops] RF_* | WF_RANGES: the single calls answer the document
};

void launch_write_plan(const WriteArgs& a, hipStream_t s);    // every op resolved and sized
void launch_write_write(const WriteArgs& a, hipStream_t s);   // the updates at their offsets

}  // namespace yc
#endif
