// Host check of the struct decode's shape classifier (crdt_amd/csrc/yc_shape.h), built with
// -fsanitize=address,undefined by tests/test_shape_class.py and run as a program of its own.
//
//   shape_check                 random windows: the class is below NCLASS and depends on the 24
//                               window bytes alone
//   shape_check <records file>  25-byte records (24 window bytes from the word holding a struct's
//                               start, then the start's offset in that word): the same checks, and
//                               one class number per record on stdout
//
// Every window is classified from a heap block of exactly 24 bytes (a read past either end is a
// sanitizer report) and again from the middle of a block whose bytes around the window are
// filled two different ways (a class that changes with them read outside the window).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../crdt_amd/csrc/yc_shape.h"

static uint32_t classify_exact(const uint8_t* w24, uint32_t o) {
  uint32_t* blk = new uint32_t[6];
  memcpy(blk, w24, 24);
  yc::RegWin x;
  x.load(blk);
  const uint32_t c = yc::shape_class(x, o);
  delete[] blk;
  return c;
}
static uint32_t classify_guarded(const uint8_t* w24, uint32_t o, uint8_t fill) {
  alignas(4) uint8_t buf[64 + 24 + 64];
  memset(buf, fill, sizeof buf);
  memcpy(buf + 64, w24, 24);
  yc::RegWin x;
  x.load((const uint32_t*)(buf + 64));
  return yc::shape_class(x, o);
}
static bool check(const uint8_t* w24, uint32_t o, uint32_t* cls) {
  const uint32_t c = classify_exact(w24, o);
  *cls = c;
  if (c >= yc::NCLASS) { fprintf(stderr, "class %u out of range\n", c); return false; }
  if (classify_guarded(w24, o, 0x00) != c || classify_guarded(w24, o, 0xFF) != c) {
    fprintf(stderr, "class depends on bytes outside the window\n");
    return false;
  }
  return true;
}

int main(int argc, char** argv) {
  uint32_t cls;
  if (argc > 1) {
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    uint8_t rec[25];
    size_t n = 0;
    while (fread(rec, 1, 25, f) == 25) {
      if (rec[24] > 3) { fprintf(stderr, "record %zu: offset %u\n", n, rec[24]); return 2; }
      if (!check(rec, rec[24], &cls)) return 1;
      printf("%u\n", cls);
      ++n;
    }
    fclose(f);
    fprintf(stderr, "%zu records ok\n", n);
    return 0;
  }
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
  uint32_t hist[yc::NCLASS] = {};
  for (uint32_t it = 0; it < 400000; ++it) {
    uint8_t w[24];
    for (uint32_t k = 0; k < 24; k += 8) { const uint64_t r = next(); memcpy(w + k, &r, 8); }
    const uint64_t r = next();
    const uint32_t o = r & 3u, mode = (r >> 2) & 3u;
    // raw noise; a plausible info byte; short varuints behind it; short string lengths as well
    if (mode >= 1) w[o] = (uint8_t)(((r >> 8) & 0xE0u) | ((r >> 16) % 11u));
    if (mode >= 2) for (uint32_t k = o + 1; k < 24; ++k) if ((r >> (24 + k)) & 1u) w[k] &= 0x7Fu;
    if (mode == 3) for (uint32_t k = o + 1; k < 24; ++k) if (w[k] < 0x80u && ((r >> k) & 1u)) w[k] &= 0x0Fu;
    if (!check(w, o, &cls)) return 1;
    ++hist[cls];
  }
  for (uint32_t c = 0; c < yc::NCLASS; ++c) printf("class %u: %u\n", c, hist[c]);
  return 0;
}
