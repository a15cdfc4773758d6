// yc_cache.h — the fleet cache refresh (ycrdt_docs_cache): for every document the object `c` of
// crdt.js:201-216 / 297-305, one member per live entry of the document's index map (`ix`), each the
// toJSON of the root the entry names. Two definitions live here once, for the kernels
// (yc_cache.hip) and the host composition (yc_host.cpp) alike:
//   index_kind     which kind of root an index entry's value asks for (`val == 'map'`)
//   cache_put_name a member's name prefix, `"name":`
#pragma once
#include "yc_json.h"

namespace yc {

// JavaScript's `val == 'map'` for the value of an index entry, read off the winning item's content
// bytes b[b0, b1) of content kind `ref`: true = the root is read as a YMap, false = as a YArray.
// Loose equality with a string holds for that string and for an array whose toString() is that
// string: a chain of one-element arrays ending in "map" ([] joins its members with ',', so any
// other length gives another text). Numbers, booleans, null, undefined, objects, byte arrays
// ("109,97,112"), shared types and a one-character ContentString never compare equal. ContentJSON
// and ContentEmbed hold JSON text (what JSON.parse gives is compared): the same chain, written
// with brackets and the literal "map", JSON whitespace allowed, no escapes. Reads nothing outside
// [b0, b1); truncated or malformed bytes give false. Every loop advances by at least one byte.
YC_HD inline bool index_kind(const uint8_t* b, uint64_t b0, uint64_t b1, uint32_t ref) {
  if (b0 > b1) return false;
  JRd r{b, b0, b1, true};
  if (ref == REF_ANY) {
    for (;;) {
      const uint32_t tag = r.u8();
      if (!r.ok) return false;
      if (tag == 117) {  // an array: only a single member can give "map"
        const uint32_t n = r.vu();
        if (!r.ok || n != 1) return false;
        continue;
      }
      if (tag != 119) return false;
      const uint32_t n = r.vu();
      const uint8_t* q = r.take(n);
      return r.ok && n == 3 && q[0] == 'm' && q[1] == 'a' && q[2] == 'p';
    }
  }
  if (ref != REF_JSON && ref != REF_EMBED) return false;
  const uint32_t n = r.vu();
  const uint8_t* q = r.take(n);
  if (!r.ok) return false;
  uint32_t i = 0, open = 0;
  for (; i < n && (json_ws(q[i]) || q[i] == '['); ++i) open += q[i] == '[';
  if (n - i < 5 || q[i] != '"' || q[i + 1] != 'm' || q[i + 2] != 'a' || q[i + 3] != 'p' || q[i + 4] != '"') return false;
  uint32_t close = 0;
  for (i += 5; i < n && (json_ws(q[i]) || q[i] == ']'); ++i) close += q[i] == ']';
  return i == n && open == close;
}

// `"name":` — the name escaped as the entry names of a map are (json_put_str)
template <class Sink>
YC_HD inline void cache_put_name(Sink& o, const uint8_t* name, uint64_t len) {
  json_put_str(o, name, len);
  o.ch(':');
}

}  // namespace yc

#if defined(__HIP__) || defined(__HIPCC__)
namespace yc {

constexpr uint32_t JR_INDEX = 8u;    // document flag: the index root holds an entry the device ordering refuses

// The columns of one ycrdt_docs_cache pass beside the front half's (JsonArgs j): the uploaded
// requests are one (document, index, map) per document, so request d is document d and j.rsize /
// j.roffs / j.rflag are per document. Everything else is indexed by sorted key position.
struct CacheArgs {
  JsonArgs j;
  uint32_t* live;            // [ck + 1] 1: a live entry of its document's index group
  uint32_t* lrank;           // [ck + 1] exclusive scan of live: the member's rank (the last is the member count)
  uint32_t* mixed;           // [ck + 1] 1: a root key whose root name differs from the key before it in the same hash group
  uint32_t* smixed;          // [ck + 1] exclusive scan of mixed
  uint32_t* msize;           // [ck + 1] bytes of the member: name prefix, root text, separator
  uint64_t* moffs;           // [ck + 1] exclusive scan of msize
  uint32_t* mkind;           // [ck] 0 map, 1 array
  uint32_t* roots;           // [1] members of the documents the device answers
};

void launch_cache_mark(const CacheArgs& a, hipStream_t s);     // live index entries, mixed hash groups
void launch_cache_members(const CacheArgs& a, hipStream_t s);  // per member: request, root range, size
void launch_cache_docs(const CacheArgs& a, hipStream_t s);     // per document: size, flags
void launch_cache_write(const CacheArgs& a, hipStream_t s);    // braces, name prefixes, root brackets and bases

}  // namespace yc
#endif
