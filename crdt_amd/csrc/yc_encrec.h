// yc_encrec.h — the 8-byte encode record of an output struct (o_rec, yc_encode.hip).
//
// Compiled by hipcc (yc_encode.hip) and by g++ (tests/encrec_check.cpp): pure functions of two words.
//
// The size pass (out_sizes_at) writes one record per output struct that the whole-item encoder
// (encode_struct_fast) takes; the write pass then emits the struct from the record and the source
// bytes alone, without gathering the segment's and the source struct's columns a second time.
//   word 0          s_pos[src]: the struct's first byte within its window
//   word 1  0..7    the final info byte (content ref -> Deleted when deleted, the input's origin bits,
//                   the parentSub bit of the merged state)
//           8       deleted
//           9..19   header length s_cpos - s_pos - 1 (origin / right origin / parent / parentSub bytes)
//           20..30  tail: the content length s_cend - s_cpos of a live item, s_len of a deleted one
//           31      REC_VALID
// A struct whose header or tail does not fit 11 bits gets no valid record (0) and is encoded from
// its columns as before: the record is a cache of the common case, never the only source of truth.
#pragma once
#include "yc_parse.h"  // YC_HDI

namespace yc {

constexpr uint32_t REC_VALID = 0x80000000u;
constexpr uint32_t REC_MAX = 2047u;  // largest header length / tail a record holds

struct EncRec {
  uint32_t pos, info, hdr, tail;
  bool del;
};

YC_HDI uint32_t rec_vu_size(uint32_t v) {
  return v < (1u << 7) ? 1u : v < (1u << 14) ? 2u : v < (1u << 21) ? 3u : v < (1u << 28) ? 4u : 5u;
}
// 0: the struct cannot have a record
YC_HDI uint64_t rec_pack(uint32_t pos, uint32_t info, bool del, uint32_t hdr, uint32_t tail) {
  if (hdr > REC_MAX || tail > REC_MAX) return 0ull;
  const uint32_t hi = REC_VALID | (tail << 20) | (hdr << 9) | (del ? 0x100u : 0u) | (info & 0xFFu);
  return ((uint64_t)hi << 32) | pos;
}
YC_HDI bool rec_valid(uint64_t r) { return ((uint32_t)(r >> 32) & REC_VALID) != 0; }
YC_HDI EncRec rec_unpack(uint64_t r) {
  const uint32_t hi = (uint32_t)(r >> 32);
  EncRec x;
  x.pos = (uint32_t)r;
  x.info = hi & 0xFFu;
  x.del = (hi & 0x100u) != 0;
  x.hdr = (hi >> 9) & REC_MAX;
  x.tail = (hi >> 20) & REC_MAX;
  return x;
}
// encoded size of the struct: info byte, header, then ContentDeleted's length or the content bytes
YC_HDI uint32_t rec_size(uint64_t r) {
  const EncRec x = rec_unpack(r);
  return 1u + x.hdr + (x.del ? rec_vu_size(x.tail) : x.tail);
}

}  // namespace yc
