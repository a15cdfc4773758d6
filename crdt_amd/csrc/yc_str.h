// yc_str.h — ContentString pieces, defined once for the host and the device.
//
// A ContentString counts UTF-16 code units over UTF-8 bytes: a 4-byte character is a surrogate pair,
// two units. Yjs may split a string between the two units of a pair (an origin, a delete-set range,
// a partly known duplicate, mergeUpdates' sliceStruct); ContentString.splice (Y@70000..) then leaves
// U+FFFD, one unit, on each side, for good. A piece cut there is kept as 3 of the character's 4
// bytes — its last three (continuation bytes) for the low half, its first three for the high half —
// which is the size of the EF BF BD that stands there, so a piece's byte count is its written size
// and no table says which edge was cut: the bytes do (str_halves). str_slice finds the piece,
// str_put writes it. The view (yc_view.hip) notes the halves of a piece in its record's flags, so the
// readers (SegCursor and json_put_piece, yc_json.h) take no other bytes for a half.
//
// Compiled by hipcc (__host__ __device__) and by g++ (plain inline), as yc_parse.h is.
#pragma once
#include <cstdint>

#include "yc_parse.h"  // YC_HD

namespace yc {

constexpr uint64_t STR_REFUSED = ~0ull;

YC_HDI uint32_t utf8_len(uint32_t c) { return c < 0x80u ? 1u : c < 0xE0u ? 2u : c < 0xF0u ? 3u : 4u; }
YC_HDI bool utf8_cont(uint32_t c) { return (c & 0xC0u) == 0x80u; }

// Byte range of UTF-16 units [e0, e1) of the UTF-8 text by[p, end), b1 << 32 | b0. An edge between the
// two units of a pair takes 3 of the character's 4 bytes (above), except that `e0_write` — e0 is an
// offset Yjs writes at, not a split it made: lib0 throws there — refuses it. Refused too
// (STR_REFUSED): text shorter than e1 units or ending inside a character.
YC_HD inline uint64_t str_slice(const uint8_t* __restrict__ by, uint32_t p, uint32_t end, uint32_t e0, uint32_t e1, bool e0_write) {
  uint32_t u = 0;  // units before p
  uint32_t b0 = 0xFFFFFFFFu;
  for (;;) {
    if (u == e0) b0 = p;
    if (u >= e1 || p >= end) break;
    const uint32_t n = utf8_len(by[p]);
    if (n > end - p) return STR_REFUSED;
    if (n == 4) {
      if (u + 1 == e0) {
        if (e0_write) return STR_REFUSED;
        b0 = p + 1;
      }
      if (u + 1 == e1) return b0 == 0xFFFFFFFFu ? STR_REFUSED : ((uint64_t)(p + 3) << 32) | b0;
      ++u;
    }
    p += n;
    ++u;
  }
  return b0 != 0xFFFFFFFFu && u == e1 ? ((uint64_t)p << 32) | b0 : STR_REFUSED;
}

// The half pairs at the edges of piece s[0, n), from its bytes: STR_HEAD — it starts on a
// continuation byte, the rest of a character cut before it; STR_TAIL — its last lead byte opens a
// 4-byte character that its end cuts short. Each half is 3 bytes in a piece str_slice made.
enum : uint32_t { STR_HEAD = 1u, STR_TAIL = 2u };
YC_HD inline uint32_t str_halves(const uint8_t* __restrict__ s, uint64_t n) {
  uint32_t h = n && utf8_cont(s[0]) ? (uint32_t)STR_HEAD : 0u;
  for (uint32_t k = 1; k <= 3 && k <= n; ++k) {
    const uint32_t c = s[n - k];
    if (utf8_cont(c)) continue;
    if (c >= 0xF0u) h |= STR_TAIL;  // (k < 4: the character is not whole)
    break;
  }
  return h;
}
// bytes of the half at the head of a piece of n bytes, and at its tail behind a head of `head` bytes
YC_HDI uint32_t str_head_len(uint32_t halves, uint64_t n) { return (halves & STR_HEAD) ? (n < 3 ? (uint32_t)n : 3u) : 0u; }
YC_HDI uint32_t str_tail_len(uint32_t halves, uint64_t n, uint32_t head) {
  return (halves & STR_TAIL) ? (n - head < 3 ? (uint32_t)(n - head) : 3u) : 0u;
}

YC_HDI uint32_t fffd_byte(uint32_t i) { return i == 0 ? 0xEFu : i == 1 ? 0xBFu : 0xBDu; }

// Piece s[0, n) as Yjs holds it: its half pairs (`halves`) as U+FFFD, byte for byte (n bytes in all:
// through put(x)), the text between them through mid(s + head, count).
template <class Put, class Mid>
YC_HD inline void str_put(const uint8_t* __restrict__ s, uint64_t n, uint32_t halves, Put put, Mid mid) {
  const uint32_t head = str_head_len(halves, n), tail = str_tail_len(halves, n, head);
  for (uint32_t i = 0; i < head; ++i) put(fffd_byte(i));
  mid(s + head, n - head - tail);
  for (uint32_t i = 0; i < tail; ++i) put(fffd_byte(i));
}
// ... a piece str_slice made, copied to out + q; returns the position behind it
YC_HDI uint64_t str_copy(uint8_t* __restrict__ out, uint64_t q, const uint8_t* __restrict__ s, uint64_t n) {
  str_put(s, n, str_halves(s, n), [&](uint32_t x) { out[q++] = (uint8_t)x; },
          [&](const uint8_t* t, uint64_t k) { for (uint64_t i = 0; i < k; ++i) out[q++] = t[i]; });
  return q;
}

}  // namespace yc
