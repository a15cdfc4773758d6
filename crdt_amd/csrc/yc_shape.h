// yc_shape.h — the 24-byte register window of the struct walks and the shape class of a struct.
//
// Compiled by hipcc (yc_decode.hip) and by g++ (tests/shape_check.cpp): everything here is a pure
// function of six words.
#pragma once
#include "yc_parse.h"  // YC_HDI, the content refs

namespace yc {

// ---- the register-window sizer (fast path of every struct walk)
// The 24 bytes from the word holding a struct's start sit in six registers, loaded in one round
// (from the lane's LDS window, or from the batch buffer); T marks the bytes that end a varuint
// (high bit clear). A varuint's length is then a count of trailing zeros of T, and the few bytes
// whose values matter (info byte, element counts, tags, short lengths) come out of the registers
// through a three-level select: one round of loads per struct instead of one dependent LDS /
// memory round trip per field. 24 bytes hold the common structs whole (a map set with a 5-byte
// client id and a short value; a root-map item with its parent name and key).
struct RegWin {
  // named words, not an array: an array indexed through the select tree is turned back into a
  // dynamically indexed (LDS-promoted) alloca by the compiler
  uint32_t r0, r1, r2, r3, r4, r5;
  uint32_t T;
  YC_HDI static uint32_t sel(uint32_t m, uint32_t a1, uint32_t a0) { return (a1 & m) | (a0 & ~m); }
  YC_HDI uint32_t word(uint32_t k) const {  // k < 6
    const uint32_t m0 = 0u - (k & 1u), m1 = 0u - ((k >> 1) & 1u), m2 = 0u - ((k >> 2) & 1u);
    const uint32_t a0 = sel(m0, r1, r0), a1 = sel(m0, r3, r2), a2 = sel(m0, r5, r4);
    return sel(m2, a2, sel(m1, a1, a0));
  }
  YC_HDI uint32_t byte(uint32_t i) const { return (word(i >> 2) >> ((i & 3u) * 8)) & 0xFFu; }
  // length (1..5) of the varuint at byte i < 24; 0: it does not end inside the window within 5 bytes
  YC_HDI uint32_t vlen(uint32_t i) const {
    const uint32_t t = T >> i;
    const uint32_t e = t ? (uint32_t)__builtin_ctz(t) + 1u : 0u;
    return e <= 5 ? e : 0u;
  }
  YC_HDI static uint32_t nib(uint32_t x) {  // bit j = byte j of x < 0x80
    return ((~x & 0x80808080u) * 0x204081u) >> 28;
  }
  YC_HDI void mask() {
    T = nib(r0) | nib(r1) << 4 | nib(r2) << 8 | nib(r3) << 12 | nib(r4) << 16 | nib(r5) << 20;
  }
  YC_HDI void load(const uint32_t* g) {
    r0 = g[0]; r1 = g[1]; r2 = g[2]; r3 = g[3]; r4 = g[4]; r5 = g[5];
    mask();
  }
};
constexpr uint32_t WIN_SPAN = 24;

// ---- shape class of a struct (k_struct_decode's workgroup sort key)
// What parse_struct will have to do for the struct whose info byte is window byte o (o < 4), told
// from the window alone: header kind, content ref and, for a ContentAny, the first value's tag.
// Numbered by expected parse cost, so that neighbours in a sort are similar. A hint only: the
// struct decode groups its lanes by it and nothing else reads it, so a wrong class costs time and
// never a byte of output. Straight-line code (selects, no loop over data); a field that falls
// outside the window, an unknown ref or a length byte of two bytes gives SHAPE_OTHER.
enum : uint32_t {
  SHAPE_GC = 0,        // GC / Skip
  SHAPE_DELETED = 1,   // placed by origin: ContentDeleted
  SHAPE_SCALAR = 2,    //   ContentAny, first value a scalar (varInt, float, bool, null, ...)
  SHAPE_STRING = 3,    //   ContentAny string / bytes first, ContentString, ContentBinary
  SHAPE_CONTAINER = 4, //   ContentAny, first value an object / array
  SHAPE_MISC = 5,      //   Type, Embed, Format, JSON, Doc, an empty or long ContentAny
  SHAPE_RO_LIGHT = 6,  // with a right origin: Deleted / scalar
  SHAPE_RO_HEAVY = 7,  //   every other content
  SHAPE_ROOT_LIGHT = 8,   // parent by name (and key): Deleted / scalar
  SHAPE_ROOT_STRING = 9,  //   string
  SHAPE_ROOT_HEAVY = 10,  //   container / misc
  SHAPE_ROOT_ID = 11,  // parent by id
  SHAPE_OTHER = 12,
  NCLASS = 13
};
YC_HDI uint32_t shape_class(const RegWin& x, uint32_t o) {
  const uint32_t info = x.byte(o), ref = info & 31u;
  const bool root = (info & 0xC0u) == 0, both = (info & 0xC0u) == 0xC0u;
  uint32_t q = o + 1;
  bool bad = ref > REF_SKIP;
  // first varuint: an origin's client, or the parent info of a root-header item
  uint32_t l = x.vlen(q);  // (q <= 4)
  const bool byname = root && l == 1 && x.byte(q) == 1u;
  bad = bad || !l;
  q += l;
  // the other id varuints: origin clock; right origin (client, clock) or parent id (client, clock)
  const bool on2 = !byname, on3 = !byname && (root || both), on4 = both;
  l = x.vlen(q < 31u ? q : 31u);  // (T holds 24 bits: 0 past the window)
  bad = bad || (on2 && !l);
  q += on2 ? l : 0u;
  l = x.vlen(q < 31u ? q : 31u);
  bad = bad || (on3 && !l);
  q += on3 ? l : 0u;
  l = x.vlen(q < 31u ? q : 31u);
  bad = bad || (on4 && !l);
  q += on4 ? l : 0u;
  // parent name and key: strings with a one-byte length
  const bool key = root && (info & 0x20u) != 0;
  uint32_t n = x.byte(q < WIN_SPAN ? q : WIN_SPAN - 1);
  bad = bad || (byname && (q >= WIN_SPAN || n >= 128u));
  q += byname ? 1u + n : 0u;
  n = x.byte(q < WIN_SPAN ? q : WIN_SPAN - 1);
  bad = bad || (key && (q >= WIN_SPAN || n >= 128u));
  q += key ? 1u + n : 0u;
  // content: the ref and, for ContentAny, the element count and the first tag
  const uint32_t nel = x.byte(q < WIN_SPAN ? q : WIN_SPAN - 1), tag = x.byte(q + 1 < WIN_SPAN ? q + 1 : WIN_SPAN - 1);
  uint32_t cc = 4;  // 0 Deleted, 1 scalar, 2 string, 3 container, 4 misc
  if (ref == REF_DELETED) cc = 0;
  if (ref == REF_STRING || ref == REF_BINARY) cc = 2;
  if (ref == REF_ANY) {
    bad = bad || q + 1 >= WIN_SPAN;
    const bool one = nel >= 1u && nel < 128u;
    if (one && tag >= 120u && tag <= 127u) cc = 1;
    if (one && (tag == 119u || tag == 116u)) cc = 2;
    if (one && (tag == 117u || tag == 118u)) cc = 3;
  }
  uint32_t cls = SHAPE_DELETED + cc;
  if (info & 0x40u) cls = cc <= 1 ? SHAPE_RO_LIGHT : SHAPE_RO_HEAVY;
  if (root) cls = byname ? (cc <= 1 ? SHAPE_ROOT_LIGHT : cc == 2 ? SHAPE_ROOT_STRING : SHAPE_ROOT_HEAVY) : SHAPE_ROOT_ID;
  if (bad) cls = SHAPE_OTHER;
  if (ref == REF_GC || ref == REF_SKIP) cls = SHAPE_GC;
  return cls;
}

}  // namespace yc
