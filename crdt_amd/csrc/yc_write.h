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
#include "yc_read.h"   // RF_*
#include "yc_write_ops.h"

namespace yc {

constexpr uint32_t WRITE_RANGES_MAX = 8;     // visible segments one array delete may touch on the device

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

constexpr uint32_t WF_RANGES = 32u;  // beside the reads' RF_*: an array delete touches more than WRITE_RANGES_MAX visible segments

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

// ---- transactions (ycrdt_docs_transact): an op planned behind the earlier ops of
// its call on the same list, without the state those ops leave. The list is a small piece table over
// the view: a piece is a range of the view's visible positions or a run of an earlier op, alive or
// dead through an earlier delete of the call; dead pieces stay where they are, as deleted items do.
// The planner reads the view through `V` (the device's view records, or a plain segment list on the
// host: tests/csrc/write_chain_main.cpp):
//   uint64_t total() const                                    visible elements
//   bool first(WId& id) const                                 the list's first segment, visible or not
//   bool at(uint64_t t, WId& id, bool& has_next, WId& next)   visible element t and what follows it in
//                                                             the list, deleted or not
//   bool span(uint64_t t, uint64_t end, WRange& r) const      the visible elements from t inside one
//                                                             segment, up to `end`
// at / span return false where a view record is out of range (the op is flagged).
constexpr uint32_t WRITE_PIECES_MAX = 1 + 2 * WRITE_CHAIN_MAX;   // every earlier op adds at most two
constexpr uint32_t WF_PIECES = 64u;  // the piece table is full
constexpr uint32_t WF_CHAIN = 128u;  // a link that does not point at an earlier op of the right kind, or a chain past WRITE_CHAIN_MAX

struct WPiece {
  uint32_t src;              // WRITE_NONE: view positions [off, off + len); else elements [off, off + len) of chain op `src`
  uint32_t off, len;
  uint32_t dead;
};

struct WListTable {
  WPiece p[WRITE_PIECES_MAX];
  uint32_t n;
  uint32_t client;
  uint32_t clock[WRITE_CHAIN_MAX];   // per chain op: its run's first clock,
  uint32_t rhas[WRITE_CHAIN_MAX];    // ... and the right origin it was inserted with
  WId right[WRITE_CHAIN_MAX];
};

YC_HD inline uint64_t wl_length(const WListTable& T) {
  uint64_t len = 0;
  for (uint32_t k = 0; k < T.n && k < WRITE_PIECES_MAX; ++k)
    if (!T.p[k].dead) len += T.p[k].len;
  return len;
}
YC_HD inline WId wl_run_id(const WListTable& T, const WPiece& c, uint32_t o) {
  return WId{T.client, T.clock[c.src < WRITE_CHAIN_MAX ? c.src : 0] + c.off + o};
}
// the piece k that holds alive element e, and e's offset o in it
YC_HD inline bool wl_locate(const WListTable& T, uint64_t e, uint32_t& k, uint32_t& o) {
  uint64_t pos = 0;
  for (k = 0; k < T.n && k < WRITE_PIECES_MAX; ++k) {
    if (T.p[k].dead) continue;
    if (e - pos < T.p[k].len) { o = (uint32_t)(e - pos); return true; }
    pos += T.p[k].len;
  }
  return false;
}
YC_HD inline bool wl_insert_piece(WListTable& T, uint32_t at, const WPiece& x) {
  if (T.n >= WRITE_PIECES_MAX || at > T.n) return false;
  for (uint32_t j = T.n; j > at; --j) T.p[j] = T.p[j - 1];
  T.p[at] = x;
  ++T.n;
  return true;
}
// piece k cut behind its first `head` elements (0 < head < len): no piece is ever empty
YC_HD inline bool wl_split(WListTable& T, uint32_t k, uint32_t head) {
  if (k >= T.n || !head || head >= T.p[k].len) return false;
  WPiece tail = T.p[k];
  tail.off += head;
  tail.len -= head;
  if (!wl_insert_piece(T, k + 1, tail)) return false;
  T.p[k].len = head;
  return true;
}

// typeListInsertGenericsAfter over the table, 0 <= index <= wl_length(T): the origin is the alive
// element at index - 1, the right origin its structural successor
template <class V>
YC_HD inline void wl_plan_insert(const V& v, const WListTable& T, uint64_t index, uint32_t& has, WId& origin, WId& right, uint32_t& flags) {
  has = 0;
  if (index == 0) {
    WId f{};
    if (T.n && T.p[0].src != WRITE_NONE) { has |= 2u; right = wl_run_id(T, T.p[0], 0); }
    else if (v.first(f)) { has |= 2u; right = f; }
    return;
  }
  uint32_t k = 0, o = 0;
  if (!wl_locate(T, index - 1, k, o)) { flags |= RF_OPEN; return; }
  const WPiece& c = T.p[k];
  const bool last = o + 1 == c.len;
  const bool run_next = last && k + 1 < T.n && T.p[k + 1].src != WRITE_NONE;
  has |= 1u;
  if (c.src != WRITE_NONE) {
    if (c.src >= WRITE_CHAIN_MAX) { flags |= RF_OPEN; return; }
    origin = wl_run_id(T, c, o);
    // (a piece that is not its run's end is followed by a run: the rest of its own, or one inserted behind it)
    if (!last) { has |= 2u; right = wl_run_id(T, c, o + 1); }
    else if (run_next) { has |= 2u; right = wl_run_id(T, T.p[k + 1], 0); }
    else if (T.rhas[c.src]) { has |= 2u; right = T.right[c.src]; }
    return;
  }
  WId next{};
  bool has_next = false;
  if (!v.at((uint64_t)c.off + o, origin, has_next, next)) { flags |= RF_OPEN; return; }
  if (run_next) { has |= 2u; right = wl_run_id(T, T.p[k + 1], 0); }
  else if (has_next) { has |= 2u; right = next; }
}

// the run of chain op `slot` put behind alive element index - 1 (in front of everything at 0)
YC_HD inline bool wl_apply_insert(WListTable& T, uint64_t index, uint32_t slot, uint32_t count) {
  uint32_t at = 0;
  if (index) {
    uint32_t k = 0, o = 0;
    if (!wl_locate(T, index - 1, k, o)) return false;
    if (o + 1 < T.p[k].len && !wl_split(T, k, o + 1)) return false;
    at = k + 1;
  }
  return wl_insert_piece(T, at, WPiece{slot, 0, count, 0});
}

// typeListDelete over the table: the alive elements [from, to) die; with `p`, their ranges are recorded
template <class V>
YC_HD inline void wl_delete(const V& v, WListTable& T, uint64_t from, uint64_t to, WritePlan* p, uint32_t& flags) {
  uint64_t pos = 0;
  for (uint32_t k = 0; k < T.n && k < WRITE_PIECES_MAX && pos < to; ++k) {
    if (T.p[k].dead) continue;
    const uint64_t len = T.p[k].len;
    if (pos + len <= from) { pos += len; continue; }
    const uint32_t a = from > pos ? (uint32_t)(from - pos) : 0u;
    const uint32_t b = to - pos < len ? (uint32_t)(to - pos) : (uint32_t)len;
    if (b < len && !wl_split(T, k, b)) { flags |= WF_PIECES; return; }
    if (a) {
      if (!wl_split(T, k, a)) { flags |= WF_PIECES; return; }
      pos += a;
      ++k;
    }
    WPiece& c = T.p[k];  // covered as a whole
    c.dead = 1;
    pos += c.len;
    if (!p) continue;
    if (c.src != WRITE_NONE) {
      if (p->nr >= WRITE_RANGES_MAX) { flags |= WF_RANGES; return; }
      const WId id = wl_run_id(T, c, 0);
      p->r[p->nr++] = WRange{id.client, id.clock, c.len};
      continue;
    }
    // one search per visible segment the piece covers
    uint64_t t = c.off;
    const uint64_t end = (uint64_t)c.off + c.len;
    for (uint32_t i = 0; i <= WRITE_RANGES_MAX && t < end; ++i) {
      WRange r{};
      if (!v.span(t, end, r) || !r.len || r.len > end - t) { flags |= RF_OPEN; return; }
      if (p->nr >= WRITE_RANGES_MAX) { flags |= WF_RANGES; return; }
      p->r[p->nr++] = r;
      t += r.len;
    }
  }
}

// List op q planned behind chain[0, nc), the earlier ops of its call on the same list in call order
// (nc < WRITE_CHAIN_MAX; indices into ops). Fills p.kind, p.has & 3, origin, right, the ranges and why.
template <class V>
YC_HD inline void write_list_plan(const V& v, const WriteReq* ops, const uint32_t* chain, uint32_t nc, const WriteReq& q, WritePlan& p,
                                  int32_t& why, uint32_t& flags) {
  if (nc >= WRITE_CHAIN_MAX) { flags |= WF_CHAIN; return; }
  const uint64_t total = v.total();
  if (total > 0xFFFFFFFFull) { flags |= RF_SIZE; return; }
  WListTable T;
  T.n = 0;
  T.client = q.client;
  for (uint32_t c = 0; c < WRITE_CHAIN_MAX; ++c) { T.clock[c] = 0; T.rhas[c] = 0; T.right[c] = WId{0, 0}; }
  if (total) T.p[T.n++] = WPiece{WRITE_NONE, 0, (uint32_t)total, 0};
  for (uint32_t c = 0; c <= nc; ++c) {
    const bool cur = c == nc;
    const WriteReq& e = cur ? q : ops[chain[c]];
    const uint64_t len = wl_length(T);
    if (e.op == WR_ARRAY_DELETE) {
      if (!e.length) continue;
      const uint64_t from = e.index < len ? e.index : len;
      const uint64_t to = (uint64_t)e.index + e.length < len ? (uint64_t)e.index + e.length : len;
      wl_delete(v, T, from, to, cur ? &p : nullptr, flags);
      if (flags) return;
      if (cur) {
        if (p.nr) p.kind = 2;
        if ((uint64_t)e.index + e.length > len) why = WHY_LENGTH;  // Yjs throws after deleting what exists
      }
      continue;
    }
    const uint64_t index = e.op == WR_ARRAY_PUSH ? len : e.index;
    if (index > len) { if (cur) why = WHY_LENGTH; continue; }
    if (!e.lead) continue;
    uint32_t has = 0;
    WId origin{}, right{};
    wl_plan_insert(v, T, index, has, origin, right, flags);
    if (flags) return;
    if (cur) {
      p.has |= has;
      p.origin = origin;
      p.right = right;
      p.kind = 1;
      return;
    }
    T.clock[c] = e.clock;
    T.rhas[c] = has & 2u;
    T.right[c] = right;
    if (!wl_apply_insert(T, index, c, e.lead)) { flags |= WF_PIECES; return; }
  }
}

// Map op q behind the earlier ops of its call on the same entry. `set`: the latest earlier MAP_SET /
// MAP_SET_TYPE (nullptr: none); `deleted`: a MAP_DELETE of the call lies behind it (or, without a
// set, behind the view's item); `win`: the view's item range, len 0 where there is none; `win_dead`.
YC_HD inline void write_entry_plan(const WriteReq& q, const WriteReq* set, bool deleted, const WRange& win, bool win_dead, WritePlan& p) {
  if (q.op == WR_MAP_DELETE) {  // typeMapDelete: nothing unless the entry's item is there and alive
    if (deleted) return;
    if (set) { p.kind = 2; p.nr = 1; p.r[0] = WRange{set->client, set->clock, 1}; }
    else if (win.len && !win_dead) { p.kind = 2; p.nr = 1; p.r[0] = win; }
    return;
  }
  // typeMapSet: left = parent._map.get(key), the entry's rightmost item, deleted or not
  if (set) { p.has |= 1u; p.origin = WId{set->client, set->clock}; }
  else if (win.len) { p.has |= 1u; p.origin = WId{win.client, win.clock + win.len - 1}; }
  p.kind = 1;
}

}  // namespace yc

#if defined(__HIP__) || defined(__HIPCC__)

namespace yc {

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
// ycrdt_docs_transact: every op resolved and sized behind the earlier ops of its call (links[nops])
void launch_transact_plan(const WriteArgs& a, const WriteLink* links, hipStream_t s);

}  // namespace yc
#endif
