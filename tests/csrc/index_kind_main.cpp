// Host build of yc_cache.h for tests/test_index_kind.py: index_kind (an index entry's value ==
// 'map') and cache_put_name (a member's `"name":` prefix), driven line by line from stdin.
//   K <ref> <hex>  -> "K <0|1>"         index_kind over the bytes as content of kind <ref>
//   N <hex>        -> "N <sized> <hex>" the prefix of the name: bytes the size-only pass counted, the text written
// Every input sits in a heap block of its exact size, and the text is written into a block of
// exactly the counted size, so under AddressSanitizer a read past a truncated value or a write
// past the reported size aborts the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "yc_cache.h"

static uint8_t* exact(const std::string& hex, size_t& n) {
  n = hex.size() / 2;
  uint8_t* p = (uint8_t*)malloc(n ? n : 1);
  if (!n) { free(p); p = (uint8_t*)malloc(0); }
  for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
  return p;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, hex;
    in >> op;
    if (op == "K") {
      uint32_t ref = 0;
      in >> ref >> hex;
      size_t n = 0;
      uint8_t* b = exact(hex, n);
      printf("K %d\n", yc::index_kind(b, 0, n, ref) ? 1 : 0);
      free(b);
    } else if (op == "N") {
      in >> hex;
      size_t n = 0;
      uint8_t* b = exact(hex, n);
      yc::JText size{nullptr, 0};
      yc::cache_put_name(size, b, n);
      uint8_t* out = (uint8_t*)malloc(size.n ? size.n : 1);
      yc::JText w{out, 0, size.n};
      yc::cache_put_name(w, b, n);
      std::string s;  // the host sink must receive the same bytes
      yc::JString hs{s};
      yc::cache_put_name(hs, b, n);
      if (w.n != size.n || s.size() != size.n || memcmp(s.data(), out, size.n) != 0) { printf("N mismatch\n"); return 1; }
      printf("N %llu ", (unsigned long long)size.n);
      for (uint64_t i = 0; i < w.n; ++i) printf("%02x", out[i]);
      printf("\n");
      free(out);
      free(b);
    } else {
      return 2;
    }
  }
  return 0;
}
