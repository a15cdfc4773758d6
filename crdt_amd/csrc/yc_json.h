// yc_json.h — the JSON.stringify text of view content, defined once for the host and the device.
//
// any_json_text writes one lib0 `any` value (lib0 readAny L0@1937 -> JSON.stringify) without
// recursion and without allocation: undefined members are dropped from objects and written null in
// arrays, numbers take Number::toString's text (yc_num.h), float32 is widened, BigInt64 is its
// signed decimal, a Uint8Array is {"0":b0,...}, object members keep their encoded order. SegCursor
// walks the elements of one view segment, whatever its content kind. Both write into a sink and
// keep their open containers on a stack the caller hands in: the fleet toJSON kernels (yc_json.hip)
// pass JText (one function sizes, o == nullptr, and writes) and 64 levels, the host writer
// (yc_host.cpp) appends to a std::string through JString and follows ANY_HOST_DEPTH levels. So the
// per-document answers and the fleet answers are the same bytes by construction.
#pragma once
#include <cstdint>
#include <cstring>
#include <string>

#include "yc_parse.h"  // YC_HD, yc_num.h
#include "yc_str.h"    // ContentString pieces

namespace yc {

constexpr uint32_t ANY_JSON_DEPTH = 64;    // container levels of one `any` value the device follows
constexpr uint32_t ANY_HOST_DEPTH = 4000;  // ... the host follows (lib0 readAny recurses without a limit; V8 overflows its stack near here)
enum : uint32_t {
  AJ_OK = 0,
  AJ_UNDEF = 1,  // the value is `undefined`: nothing written (a map entry is omitted, an array member is null)
  AJ_BAD = 2,    // truncated or not an `any` encoding
  AJ_DEEP = 3,   // nested past the caller's stack (the device: the host writer answers)
};

struct JText {        // byte sink at position n; o == nullptr only counts; nothing is stored at or past cap
  uint8_t* o;
  uint64_t n;
  uint64_t cap = ~0ull;
  YC_HDI void ch(uint32_t c) {
    if (o && n < cap) o[n] = (uint8_t)c;
    ++n;
  }
  YC_HDI void lit(const char* s) {
    for (; *s; ++s) ch((uint8_t)*s);
  }
  YC_HDI void raw(const uint8_t* s, uint64_t k) {
    for (uint64_t i = 0; i < k; ++i) ch(s[i]);
  }
};

struct JString {         // the host sink: appends to a string
  std::string& s;
  void ch(uint32_t c) { s.push_back((char)c); }
  void lit(const char* t) { s += t; }
  void raw(const uint8_t* t, uint64_t k) { s.append((const char*)t, k); }
  uint64_t n() const { return s.size(); }
};

template <class Sink>
YC_HD inline void json_put_esc(Sink& o, const uint8_t* s, uint64_t n) {  // a JSON string's text without the quotes
  for (uint64_t i = 0; i < n; ++i) {
    const uint32_t c = s[i];
    switch (c) {
      case '"': o.ch('\\'); o.ch('"'); break;
      case '\\': o.ch('\\'); o.ch('\\'); break;
      case '\b': o.ch('\\'); o.ch('b'); break;
      case '\f': o.ch('\\'); o.ch('f'); break;
      case '\n': o.ch('\\'); o.ch('n'); break;
      case '\r': o.ch('\\'); o.ch('r'); break;
      case '\t': o.ch('\\'); o.ch('t'); break;
      default:
        if (c < 0x20) {
          o.ch('\\'); o.ch('u'); o.ch('0'); o.ch('0');
          o.ch(c >> 4 ? '1' : '0');
          o.ch("0123456789abcdef"[c & 15u]);
        } else {
          o.ch(c);
        }
    }
  }
}
template <class Sink>
YC_HD inline void json_put_str(Sink& o, const uint8_t* s, uint64_t n) {
  o.ch('"');
  json_put_esc(o, s, n);
  o.ch('"');
}

// ... of a ContentString piece with its half pairs (yc_str.h): U+FFFD, which needs no escape
template <class Sink>
YC_HD inline void json_put_piece(Sink& o, const uint8_t* s, uint64_t n, uint32_t halves) {
  str_put(s, n, halves, [&](uint32_t x) { o.ch(x); }, [&](const uint8_t* t, uint64_t k) { json_put_esc(o, t, k); });
}

template <class Sink>
YC_HD inline void json_put_u64(Sink& o, uint64_t v) {
  char t[20];
  uint32_t k = 0;
  do { t[k++] = (char)('0' + v % 10); v /= 10; } while (v);
  while (k) o.ch((uint8_t)t[--k]);
}

template <class Sink>
YC_HD inline void json_put_number(Sink& o, double x) {  // JSON.stringify(Number)
  uint64_t u;
  memcpy(&u, &x, 8);
  if (((u >> 52) & 0x7ffu) == 0x7ffu) { o.lit("null"); return; }  // NaN, +-Infinity
  if (x == 0) { o.ch('0'); return; }
  char d[20], t[40];
  int32_t n;
  const uint32_t k = f64_shortest(x < 0 ? -x : x, d, n);
  const uint32_t len = num_text(x < 0, d, k, n, t);
  o.raw((const uint8_t*)t, len);
}

template <class Sink>
YC_HD inline void json_put_bytes(Sink& o, const uint8_t* p, uint64_t n) {  // JSON.stringify(Uint8Array)
  o.ch('{');
  for (uint64_t i = 0; i < n; ++i) {
    if (i) o.ch(',');
    o.ch('"');
    json_put_u64(o, i);
    o.ch('"');
    o.ch(':');
    json_put_u64(o, p[i]);
  }
  o.ch('}');
}

struct JRd {  // bounded reader over b[p, end): the lib0 0.2.42 forms
  const uint8_t* b;
  uint64_t p, end;
  bool ok;
  YC_HDI uint32_t u8() {
    if (p >= end) { ok = false; return 0; }
    return b[p++];
  }
  YC_HD inline uint32_t vu() {
    uint32_t v = 0, shift = 0;
    for (;;) {
      if (p >= end) { ok = false; return 0; }
      const uint32_t r = b[p++];
      if (shift < 32) v |= (r & 0x7fu) << shift;
      shift += 7;
      if (r < 0x80u) return v;
      if (shift > 35) { ok = false; return 0; }
    }
  }
  YC_HD inline double vi() {  // readVarInt: JS 32-bit shifts, `num >>> 0` on multi-byte values
    uint32_t r = u8();
    uint32_t num = r & 63u;
    const double sign = (r & 64u) ? -1.0 : 1.0;
    if (!(r & 128u)) return sign * (double)num;
    uint32_t len = 6;
    for (;;) {
      r = u8();
      if (!ok) return 0;
      num |= (r & 127u) << (len & 31u);
      len += 7;
      if (r < 128u) return sign * (double)num;
      if (len > 41) { ok = false; return 0; }
    }
  }
  YC_HDI const uint8_t* take(uint64_t n) {
    if (p > end || end - p < n) { ok = false; p = end; return b; }
    const uint8_t* q = b + p;
    p += n;
    return q;
  }
};

// The open containers of one `any` value: members left (in the caller's N words, an array of its
// own so that the rest stays in registers on the device), object or array, nothing written yet.
template <uint32_t N>
struct JStack {
  static constexpr uint32_t W = (N + 63) / 64;
  uint32_t* rem;
  uint64_t obj[W], fresh[W];  // one bit per level; a word is cleared when its first level opens
  uint32_t depth;
  YC_HDI explicit JStack(uint32_t* words) : rem(words), depth(0) {}
  YC_HDI static uint32_t word(uint32_t t) { return W == 1 ? 0u : t >> 6; }
  YC_HDI bool push(bool is_obj, uint32_t members) {  // false: full
    if (depth == N) return false;
    const uint64_t bit = 1ull << (depth & 63u);
    const uint32_t w = word(depth);
    if (bit == 1) obj[w] = fresh[w] = 0;
    rem[depth++] = members;
    fresh[w] |= bit;
    if (is_obj) obj[w] |= bit; else obj[w] &= ~bit;
    return true;
  }
  YC_HDI uint32_t& top() { return rem[depth - 1]; }  // members left
  YC_HDI bool top_obj() const { return (obj[word(depth - 1)] >> ((depth - 1) & 63u)) & 1u; }
  YC_HDI bool take_fresh() {  // true once per level: its first written member takes no comma
    const uint64_t bit = 1ull << ((depth - 1) & 63u);
    uint64_t& f = fresh[word(depth - 1)];
    const bool was = (f & bit) != 0;
    f &= ~bit;
    return was;
  }
  YC_HDI void pop() { --depth; }
};

// One lib0 `any` value at b[p, end) as JSON text appended to `o`; p moves past the value. Iterative:
// `st` holds one level per open container.
template <class Sink, class Stack>
YC_HD inline uint32_t any_json_text(const uint8_t* b, uint64_t& p, uint64_t end, Sink& o, Stack& st) {
  JRd r{b, p, end, true};
  st.depth = 0;
  for (;;) {
    if (st.depth) {
      if (st.top() == 0) {
        o.ch(st.top_obj() ? '}' : ']');
        st.pop();
        if (st.depth == 0) break;
        continue;
      }
      --st.top();
      if (st.top_obj()) {
        const uint32_t kl = r.vu();
        const uint8_t* k = r.take(kl);
        if (!r.ok) return AJ_BAD;
        if (r.p < r.end && b[r.p] == 127) { ++r.p; continue; }  // an undefined member is dropped
        if (!st.take_fresh()) o.ch(',');
        json_put_str(o, k, kl);
        o.ch(':');
      } else {
        if (!st.take_fresh()) o.ch(',');
        if (r.p < r.end && b[r.p] == 127) { ++r.p; o.lit("null"); continue; }
      }
    }
    const uint32_t tag = r.u8();
    if (!r.ok) return AJ_BAD;
    switch (tag) {
      case 127: p = r.p; return AJ_UNDEF;  // (only at the top: members are handled above)
      case 126: o.lit("null"); break;
      case 125: { const double v = r.vi(); if (r.ok) json_put_number(o, v); break; }
      case 124: {
        const uint8_t* q = r.take(4);
        if (!r.ok) break;
        const uint32_t u = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
        float f;
        memcpy(&f, &u, 4);
        json_put_number(o, (double)f);
        break;
      }
      case 123: case 122: {
        const uint8_t* q = r.take(8);
        if (!r.ok) break;
        uint64_t u = 0;
        for (int i = 0; i < 8; ++i) u = (u << 8) | q[i];
        if (tag == 123) {
          double d;
          memcpy(&d, &u, 8);
          json_put_number(o, d);
        } else {  // BigInt64 (JSON.stringify would throw): its signed decimal
          if (u >> 63) { o.ch('-'); u = ~u + 1; }
          json_put_u64(o, u);
        }
        break;
      }
      case 121: o.lit("false"); break;
      case 120: o.lit("true"); break;
      case 119: { const uint32_t n = r.vu(); const uint8_t* q = r.take(n); if (r.ok) json_put_str(o, q, n); break; }
      case 116: { const uint32_t n = r.vu(); const uint8_t* q = r.take(n); if (r.ok) json_put_bytes(o, q, n); break; }
      case 118: case 117: {
        const uint32_t n = r.vu();
        if (!r.ok) break;
        if (!st.push(tag == 118, n)) return AJ_DEEP;
        o.ch(tag == 118 ? '{' : '[');
        continue;
      }
      default: return AJ_BAD;
    }
    if (!r.ok) return AJ_BAD;
    if (st.depth == 0) break;
  }
  p = r.p;
  return AJ_OK;
}

// The elements of one visible view segment (its content bytes b[b0, b1), b0 <= b1 inside the
// buffer), one per next(): ContentAny and ContentJSON hold `len` values, a ContentString one
// element per UTF-8 character (a half pair at an edge of the piece, `halves`: U+FFFD, yc_str.h; a
// tail truncated otherwise is clipped to the segment), ContentBinary,
// ContentEmbed and ContentType one, a ContentFormat one `undefined` (getContent() is []), anything
// else (ContentDoc is outside crdt.c) one null. `entry`: the value of a YMap entry, that is one
// element — of a ContentString the last character (or half pair), of an empty string nothing.
enum : uint32_t {
  EL_OK = 0,     // one element written
  EL_UNDEF = 1,  // the element is `undefined`: nothing written (an entry is omitted, a list member is null)
  EL_END = 2,    // no element left
  EL_BAD = 3,    // truncated or malformed content (what was written of it stays in the sink); END follows
  EL_DEEP = 4,   // an `any` nested past the stack; END follows
  EL_TYPE = 5,   // a ContentType of type ref `type_ref`: nothing written, the caller writes the nested type
};
struct SegCursor {
  JRd r;
  uint32_t ref, left, type_ref = 0;
  uint32_t head, tail;  // bytes of the piece's half pairs (ContentString)
  YC_HDI SegCursor(const uint8_t* b, uint64_t b0, uint64_t b1, uint32_t ref_, uint32_t len, bool entry, uint32_t halves = 0)
      : r{b, b0, b1, true}, ref(ref_), left(ref_ == REF_ANY || ref_ == REF_JSON ? (entry ? 1u : len) : 1u),
        head(ref_ == REF_STRING ? str_head_len(halves, b1 - b0) : 0u), tail(ref_ == REF_STRING ? str_tail_len(halves, b1 - b0, head) : 0u) {
    if (entry && ref == REF_STRING) {  // (a string ends where its bytes end: `left` is not read)
      bool half;
      for (uint64_t p = b0, h = head; p < b1; p += char_at(p, h, half), h = 0) r.p = p;
      if (r.p != b0) head = 0;
    }
  }
  // bytes of the character at p < r.end (`h`: a head half of h bytes stands there); half: it is U+FFFD
  YC_HDI uint64_t char_at(uint64_t p, uint64_t h, bool& half) const {
    half = h != 0;
    if (h) return h;
    uint64_t l = utf8_len(r.b[p]);
    if (l > r.end - p) l = r.end - p;
    half = tail && p + tail == r.end;
    return l;
  }
  YC_HDI uint32_t stop(uint32_t e) { left = 0; r.p = r.end; return e; }
  template <class Sink, class Stack>
  YC_HD inline uint32_t next(Sink& o, Stack& st) {
    if (ref == REF_STRING) {
      if (r.p >= r.end) return EL_END;
      bool half;
      const uint64_t l = char_at(r.p, head, half);
      head = 0;
      if (half) { o.ch('"'); for (uint32_t i = 0; i < 3; ++i) o.ch(fffd_byte(i)); o.ch('"'); }
      else json_put_str(o, r.b + r.p, l);
      r.p += l;
      return EL_OK;
    }
    if (!left) return EL_END;
    --left;
    switch (ref) {
      case REF_ANY: {
        uint64_t p = r.p;
        const uint32_t a = any_json_text(r.b, p, r.end, o, st);
        if (a == AJ_BAD || a == AJ_DEEP) return stop(a == AJ_BAD ? EL_BAD : EL_DEEP);
        r.p = p;
        return a == AJ_UNDEF ? EL_UNDEF : EL_OK;
      }
      case REF_JSON: {
        const uint32_t k = r.vu();
        const uint8_t* q = r.take(k);
        if (!r.ok) return stop(EL_BAD);
        const char* u = "undefined";
        bool undef = k == 9;
        for (uint32_t j = 0; undef && j < 9; ++j) undef = q[j] == (uint8_t)u[j];
        if (undef) return EL_UNDEF;
        o.raw(q, k);
        return EL_OK;
      }
      case REF_BINARY: case REF_EMBED: {
        const uint32_t k = r.vu();
        const uint8_t* q = r.take(k);
        if (!r.ok) return stop(EL_BAD);
        if (ref == REF_BINARY) json_put_bytes(o, q, k); else o.raw(q, k);
        return EL_OK;
      }
      case REF_TYPE:
        type_ref = r.vu();
        return r.ok ? EL_TYPE : stop(EL_BAD);
      case REF_FORMAT: return EL_UNDEF;
      default: o.lit("null"); return EL_OK;
    }
  }
};

}  // namespace yc

#if defined(__HIP__) || defined(__HIPCC__)
// ---- fleet toJSON (ycrdt_docs_json): root JSON of many (document, root, kind) requests written on
// the device over the view of ONE multi-document merge (yc_json.hip; DESIGN.md §Fleet toJSON).
#include <hip/hip_runtime.h>

#include "yc_view.h"

namespace yc {

constexpr uint32_t JSON_DEPTH_MAX = 4;   // nested-type levels below a root the device path follows
constexpr uint32_t JSON_NAME_MAX = 64;   // longest map-entry name (bytes) the device ordering takes
constexpr uint32_t JSON_SORT_PASSES = 2 + JSON_NAME_MAX / 8;  // (length, slot) | name chunks | group

constexpr uint32_t JR_NAME = 1u;     // request flag: a root of another name shares its hash slot
constexpr uint32_t JR_OPEN = 2u;     // ... something under the root is refused, malformed or nested too deep
constexpr uint32_t JR_SIZE = 4u;     // ... its text would pass 4 GiB

struct JsonReq {             // one distinct (document, root, kind), sorted by rkey
  uint64_t rkey;             // root group key: 1 << 63 | document << 32 | name hash >> 1
  uint32_t name_pos, name_len;  // in the uploaded name pool
  uint32_t kind, pad;
};

// Items: [0, ck) the view keys in sorted order (a YMap entry each), [ck, ck + narr) the list segments.
struct JsonArgs {
  const uint8_t* bytes;      // the merged batch buffer the view's byte ranges point into
  uint64_t nbytes;
  const ViewKey* keys;
  const ViewSeg* segs;
  const uint32_t* nkeys;
  const uint32_t* kmap;      // [ck] key slot -> view key
  const uint32_t* krep;      // [ck] key slot -> a member segment
  const uint32_t* g_cidx;    // segment -> client index
  const uint32_t* cl_doc;    // client index -> document (nullptr: one document)
  const uint32_t* y_lstart;  // [nlists + 1]
  const uint32_t* y_keys;
  uint32_t ck, narr, nlists, nreq;
  uint32_t* ord;             // [ck] sorted position -> view key
  uint64_t* gk;              // [ck] sorted group keys (parent unit | root key | ~0 past the keys)
  uint32_t* inv;             // [ck] view key -> sorted position
  uint32_t* state;           // [n] 0 open, 1 sized, 2 refused
  uint32_t* contrib;         // [n + 1] bytes the item adds to its container, separator included
  uint32_t* tcontrib;        // [narr + 1] ... to a YText (escaped, no quotes)
  uint32_t* unres;           // [n + 1] 1: not sized
  uint64_t* scan_c;          // [n + 1]
  uint64_t* scan_t;          // [narr + 1]
  uint32_t* scan_u;          // [n + 1]
  uint64_t* apos;            // [n] where the item's text starts in the blob
  uint64_t* cend;            // [n] where its container's closer stands (~0: a YText member)
  uint64_t* mbase;           // [ck] group start -> position of the map's opener
  uint64_t* abase;           // [ck] list key -> position of the list's opener (bit 63: a YText)
  const JsonReq* reqs;
  const uint8_t* names;
  uint32_t* rsize;           // [nreq + 1]
  uint32_t* rflag;           // [nreq]
  uint64_t* roffs;           // [nreq + 1]
  uint8_t* out;
  uint64_t out_cap;
  // point reads only (ycrdt_docs_read seeds many containers; nullptr: every position comes from a root)
  uint32_t* own_m;           // [ck] group start -> the read whose value the map's text belongs to
  uint32_t* own_a;           // [ck] list key -> ...
  uint32_t* oflag;           // [nown] 1: the read's value holds a container another read seeded
  uint32_t nown;
};

void launch_json_sort_key(const JsonArgs& a, uint32_t pass, const uint32_t* ord_in, uint64_t* key, hipStream_t s);
void launch_json_index(const JsonArgs& a, hipStream_t s);          // inverse order, request names
void launch_json_size(const JsonArgs& a, uint32_t round, hipStream_t s);
void launch_json_requests(const JsonArgs& a, hipStream_t s);       // per-request sizes
void launch_json_roots(const JsonArgs& a, hipStream_t s);          // root brackets, root container bases
void launch_json_place(const JsonArgs& a, hipStream_t s);          // one level of positions, top-down
void launch_json_write(const JsonArgs& a, hipStream_t s);

}  // namespace yc
#ifdef YC_JSON_DEVICE
// ---- device helpers over JsonArgs, shared by the toJSON kernels (yc_json.hip), the point-read
// kernels (yc_read.hip) and the cache kernels (yc_cache.hip)
namespace yc {
namespace {

constexpr uint64_t NONE64 = ~0ull;
constexpr uint64_t TEXT_BIT = 1ull << 63;
enum : uint32_t { JS_OPEN = 0, JS_SIZED = 1, JS_REFUSED = 2 };
enum : uint32_t { EM_OK = 0, EM_OMIT = 1, EM_PENDING = 2, EM_REFUSED = 3 };
enum : uint32_t { BOX_MAP = 0, BOX_ARRAY = 1, BOX_TEXT = 2, BOX_XML = 3 };

__device__ __forceinline__ uint64_t ld64(const uint64_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st64(uint64_t* p, uint64_t v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ uint32_t lower_bound_u64(const uint64_t* __restrict__ a, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] < key) lo = mid + 1; else hi = mid;
  }
  return lo;
}
__device__ __forceinline__ uint32_t upper_bound_u64(const uint64_t* __restrict__ a, uint32_t n, uint64_t key) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (a[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool in_bytes(const JsonArgs& a, uint32_t pos, uint32_t len) { return (uint64_t)pos + len <= a.nbytes; }

// the first YArray / YText list among the keys [lo, hi) of one container (lists sort in front:
// they carry no entry name)
__device__ __forceinline__ uint32_t first_list(const JsonArgs& a, uint32_t lo, uint32_t hi) {
  for (uint32_t p = lo; p < hi; ++p) {
    const uint32_t i = a.ord[p];
    if (i >= a.ck) return VNONE;
    const ViewKey& K = a.keys[i];
    if (!(K.flags & VK_PSUB)) return p;
    if (K.psub_len) return VNONE;
  }
  return VNONE;
}

struct Box {                 // a nested type's text
  uint64_t size;
  uint32_t unres;            // members not sized
  uint32_t mode;             // BOX_*
  uint32_t lo;               // BOX_MAP: first key of its group (VNONE: no entry); else its list key (VNONE: no list)
};

__device__ __forceinline__ uint64_t boxed(uint64_t members) { return 2 + members - (members ? 1 : 0); }  // (every member ends in a separator)

// segment items [x0, x1) of list key at sorted position kp
__device__ __forceinline__ bool list_range(const JsonArgs& a, uint32_t kp, uint32_t& x0, uint32_t& x1) {
  const uint32_t i = a.ord[kp];
  if (i >= a.ck) return false;
  const ViewKey& K = a.keys[i];
  if ((uint64_t)K.seg0 + K.nseg > a.narr) return false;
  x0 = K.seg0;
  x1 = K.seg0 + K.nseg;
  return true;
}

// the item range of a request's root container: keys [lo, hi) of its group (kind 0), or the
// segments of the root's list (kind 1; kp = its key, VNONE: no such list)
__device__ __forceinline__ void root_range(const JsonArgs& a, const JsonReq& q, uint32_t& lo, uint32_t& hi, uint32_t& kp) {
  lo = lower_bound_u64(a.gk, a.ck, q.rkey);
  hi = upper_bound_u64(a.gk, a.ck, q.rkey);
  kp = VNONE;
  if (q.kind == 0) return;
  kp = first_list(a, lo, hi);
  uint32_t x0 = 0, x1 = 0;
  if (kp != VNONE && !list_range(a, kp, x0, x1)) kp = VNONE;
  lo = a.ck + x0;
  hi = a.ck + x1;
}

__device__ __forceinline__ Box type_box(const JsonArgs& a, uint32_t unit, uint32_t tr) {
  Box b{2, 0, BOX_ARRAY, VNONE};
  if (tr >= 3 && tr <= 6) { b.mode = BOX_XML; return b; }
  const uint32_t lo = lower_bound_u64(a.gk, a.ck, unit), hi = upper_bound_u64(a.gk, a.ck, unit);
  if (tr == 1) {
    b.mode = BOX_MAP;
    if (lo < hi) {
      b.lo = lo;
      b.size = boxed(a.scan_c[hi] - a.scan_c[lo]);
      b.unres = a.scan_u[hi] - a.scan_u[lo];
    }
    return b;
  }
  b.mode = tr == 2 ? BOX_TEXT : BOX_ARRAY;
  const uint32_t kp = first_list(a, lo, hi);
  uint32_t x0 = 0, x1 = 0;
  if (kp == VNONE) return b;
  if (!list_range(a, kp, x0, x1)) { b.unres = 1; return b; }
  b.lo = kp;
  if (tr == 2) {
    b.size = 2 + (a.scan_t[x1] - a.scan_t[x0]);
  } else {
    b.size = boxed(a.scan_c[a.ck + x1] - a.scan_c[a.ck + x0]);
    b.unres = a.scan_u[a.ck + x1] - a.scan_u[a.ck + x0];
  }
  return b;
}

__device__ __forceinline__ bool entry_live(const ViewKey& K) {
  return (K.flags & VK_PSUB) && (K.win.flags & VS_SET) && !(K.win.flags & VS_DELETED) && (K.win.flags & VS_ITEM);
}
__device__ __forceinline__ bool member_live(const ViewSeg& s) {
  return !(s.flags & VS_DELETED) && (s.flags & VS_COUNTABLE) && (s.flags & VS_ITEM);
}

}  // namespace
}  // namespace yc
#endif
#endif
