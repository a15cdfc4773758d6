// Host build of yc_json.h any_json_text (tests/test_any_json_text.py). stdin, one case per line:
//   V <hex>   one lib0 `any` value      -> "V <status> <size-only bytes> <written bytes> <consumed> <text as hex>"
//             (the device's forms: JText and the 64-level stack; the string sink must give the same bytes)
//   H <hex>   ... as the host writes it -> "H <status> <consumed> <text as hex>" (JString, the 4000-level stack)
//   T <hex>   every strict prefix of it -> "T <prefixes> <prefixes refused as AJ_BAD>"
// Inputs and outputs live in heap blocks of their exact size, so a sanitizer build sees any read
// past a truncated value and any write past the size the size-only pass reported.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>
#include <vector>

#include "yc_json.h"

static std::vector<uint8_t> unhex(const std::string& h) {
  std::vector<uint8_t> o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((uint8_t)strtoul(h.substr(i, 2).c_str(), nullptr, 16));
  return o;
}

template <uint32_t N, class Sink>
static uint32_t any_text(const uint8_t* in, uint64_t& p, uint64_t end, Sink& o) {
  static uint32_t rem[N];
  yc::JStack<N> st(rem);
  return yc::any_json_text(in, p, end, o, st);
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    if (line.size() < 2) continue;
    const std::vector<uint8_t> v = unhex(line.substr(2));
    if (line[0] == 'V') {
      uint8_t* in = (uint8_t*)malloc(v.size() ? v.size() : 1);
      memcpy(in, v.data(), v.size());
      uint64_t p0 = 0, p1 = 0;
      yc::JText sz{nullptr, 0};
      const uint32_t s0 = any_text<yc::ANY_JSON_DEPTH>(in, p0, v.size(), sz);
      uint8_t* out = (uint8_t*)malloc(sz.n ? sz.n : 1);
      yc::JText wr{out, 0};
      const uint32_t s1 = s0 == yc::AJ_OK ? any_text<yc::ANY_JSON_DEPTH>(in, p1, v.size(), wr) : s0;
      if (s1 != s0 || (s0 == yc::AJ_OK && p0 != p1)) { printf("MISMATCH\n"); return 1; }
      std::string text;
      yc::JString ws{text};
      uint64_t p2 = 0;
      const uint32_t s2 = any_text<yc::ANY_JSON_DEPTH>(in, p2, v.size(), ws);
      if (s2 != s0 || (s0 == yc::AJ_OK && (p2 != p0 || text != std::string((const char*)out, wr.n)))) { printf("SINKS DIFFER\n"); return 1; }
      printf("V %u %llu %llu %llu ", s0, (unsigned long long)sz.n, (unsigned long long)wr.n, (unsigned long long)p0);
      for (uint64_t i = 0; i < wr.n; ++i) printf("%02x", out[i]);
      printf("\n");
      free(out);
      free(in);
    } else if (line[0] == 'H') {
      uint8_t* in = (uint8_t*)malloc(v.size() ? v.size() : 1);
      memcpy(in, v.data(), v.size());
      std::string text;
      yc::JString ws{text};
      uint64_t p = 0;
      const uint32_t s0 = any_text<yc::ANY_HOST_DEPTH>(in, p, v.size(), ws);
      printf("H %u %llu ", s0, (unsigned long long)p);
      if (s0 == yc::AJ_OK)
        for (unsigned char c : text) printf("%02x", c);
      printf("\n");
      free(in);
    } else if (line[0] == 'T') {
      unsigned bad = 0;
      for (size_t k = 0; k < v.size(); ++k) {
        uint8_t* in = (uint8_t*)malloc(k ? k : 1);
        memcpy(in, v.data(), k);
        uint64_t p = 0;
        yc::JText sz{nullptr, 0};
        bad += any_text<yc::ANY_JSON_DEPTH>(in, p, k, sz) == yc::AJ_BAD;
        free(in);
      }
      printf("T %zu %u\n", v.size(), bad);
    }
  }
  return 0;
}
