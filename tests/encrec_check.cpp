// Host check of the encode record (crdt_amd/csrc/yc_encrec.h), built with
// -fsanitize=address,undefined by tests/test_encode_record.py and run as a program of its own.
//
//   encrec_check    packs, unpacks and sizes records at the edges of every field and over random
//                   fields; prints "ok <records checked>" and exits 0, or names the first mismatch
#include <cstdint>
#include <cstdio>

#include "../crdt_amd/csrc/yc_encrec.h"

// the varuint size the encoder writes (yc_common.h vu_size), counted the slow way
static uint32_t vu_size_ref(uint32_t v) {
  uint32_t n = 1;
  while (v > 127u) { ++n; v >>= 7; }
  return n;
}

static uint64_t checked = 0;
static bool check(uint32_t pos, uint32_t info, bool del, uint32_t hdr, uint32_t tail) {
  const uint64_t r = yc::rec_pack(pos, info, del, hdr, tail);
  const bool fits = hdr <= 2047u && tail <= 2047u;
  ++checked;
  if (!fits) {
    if (r != 0 || yc::rec_valid(r)) { fprintf(stderr, "hdr %u tail %u: not refused\n", hdr, tail); return false; }
    return true;
  }
  if (!yc::rec_valid(r)) { fprintf(stderr, "hdr %u tail %u: refused\n", hdr, tail); return false; }
  const yc::EncRec x = yc::rec_unpack(r);
  if (x.pos != pos || x.info != info || x.del != del || x.hdr != hdr || x.tail != tail) {
    fprintf(stderr, "round trip: pos %u info %u del %d hdr %u tail %u -> pos %u info %u del %d hdr %u tail %u\n", pos, info, (int)del,
            hdr, tail, x.pos, x.info, (int)x.del, x.hdr, x.tail);
    return false;
  }
  if ((uint32_t)r != pos) { fprintf(stderr, "word 0 is not the position\n"); return false; }
  const uint32_t want = 1u + hdr + (del ? vu_size_ref(tail) : tail);
  if (yc::rec_size(r) != want) { fprintf(stderr, "size: hdr %u tail %u del %d: %u, want %u\n", hdr, tail, (int)del, yc::rec_size(r), want); return false; }
  return true;
}

int main() {
  const uint32_t edges[] = {0u, 1u, 127u, 128u, 2046u, 2047u, 2048u, 2049u, 4095u, 0xFFFFFFFFu};
  const uint32_t poss[] = {0u, 1u, 0x7FFFFFFFu, 0x80000000u, 0xFFFFFFFFu};
  for (uint32_t hdr : edges)
    for (uint32_t tail : edges)
      for (uint32_t pos : poss)
        for (uint32_t del = 0; del < 2; ++del)
          for (uint32_t info = 0; info < 256; ++info)
            if (!check(pos, info, del != 0, hdr, tail)) return 1;
  // every width below the limit, and the first past it
  for (uint32_t v = 0; v <= 2048u; ++v)
    for (uint32_t del = 0; del < 2; ++del)
      if (!check(v * 2654435761u, v & 0xFFu, del != 0, v, 2047u - (v > 2047u ? 0u : v)) || !check(v, 0xFFu - (v & 0xFFu), del != 0, 2047u - (v > 2047u ? 0u : v), v))
        return 1;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  for (uint32_t it = 0; it < 200000; ++it) {
    const uint64_t a = next(), b = next();
    if (!check((uint32_t)a, (uint32_t)(a >> 32) & 0xFFu, (a >> 40) & 1u, (uint32_t)b % 2100u, (uint32_t)(b >> 32) % 2100u)) return 1;
  }
  // the varuint sizes at their own edges (a deleted item's length is below 2048, the function is total)
  const uint32_t vs[] = {0u, 127u, 128u, 16383u, 16384u, 2097151u, 2097152u, 268435455u, 268435456u, 0xFFFFFFFFu};
  for (uint32_t v : vs)
    if (yc::rec_vu_size(v) != vu_size_ref(v)) { fprintf(stderr, "rec_vu_size(%u)\n", v); return 1; }
  // an invalid record never looks valid: word 1 without bit 31
  if (yc::rec_valid(0ull) || yc::rec_valid(0x7FFFFFFFFFFFFFFFull) || !yc::rec_valid(0x8000000000000000ull)) { fprintf(stderr, "rec_valid\n"); return 1; }
  printf("ok %llu\n", (unsigned long long)checked);
  return 0;
}
