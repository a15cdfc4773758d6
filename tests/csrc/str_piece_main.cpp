// Host build of yc_str.h and of SegCursor (yc_json.h) for tests/test_str_piece.py, driven line by
// line from stdin: `<mode> <hex of the UTF-8 text> <e0> <e1>`, the piece being UTF-16 units [e0, e1).
//   S  a split at both edges        -> hex of the piece as a struct writer puts it (str_copy)
//   W  e0 is an offset Yjs writes at -> the same, or "refused" between the two units of a pair
//   T  a split                       -> hex of the piece inside a YText's JSON (json_put_piece)
//   L  a split, read as a list       -> hex of the SegCursor elements, joined by ','
//   E  a split, read as a map entry  -> hex of the one SegCursor element
// T, L and E are given the piece's halves as the view notes them in a record's flags (str_halves over
// the sliced bytes, yc_view.hip). The text sits in a heap block of its exact size and the piece is written into a block of exactly
// b1 - b0 bytes, so under AddressSanitizer a read past the text or a write past the piece's size
// aborts the run.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>

#include "yc_json.h"

static void put_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) printf("%02x", p[i]);
  printf("\n");
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, hex;
    uint32_t e0 = 0, e1 = 0;
    in >> op >> hex >> e0 >> e1;
    if (op.size() != 1 || !strchr("SWTLE", op[0])) return 2;
    const size_t n = hex.size() / 2;
    uint8_t* b = (uint8_t*)malloc(n);
    for (size_t i = 0; i < n; ++i) b[i] = (uint8_t)strtoul(hex.substr(2 * i, 2).c_str(), nullptr, 16);
    const uint64_t r = yc::str_slice(b, 0, (uint32_t)n, e0, e1, op == "W");
    if (r == yc::STR_REFUSED) {
      printf("refused\n");
      free(b);
      continue;
    }
    const uint32_t b0 = (uint32_t)r, b1 = (uint32_t)(r >> 32);
    if (b0 > b1 || b1 > n) return 3;
    const uint32_t halves = yc::str_halves(b + b0, b1 - b0);  // (as the view notes them: VS_HALF_*)
    if (op == "S" || op == "W") {
      uint8_t* out = (uint8_t*)malloc(b1 - b0);
      if (yc::str_copy(out, 0, b + b0, b1 - b0) != b1 - b0) return 4;
      put_hex(out, b1 - b0);
      free(out);
    } else if (op == "T") {
      std::string s;
      yc::JString w{s};
      yc::json_put_piece(w, b + b0, b1 - b0, halves);
      yc::JText size{nullptr, 0};  // the device's size pass counts what its write pass stores
      yc::json_put_piece(size, b + b0, b1 - b0, halves);
      if (size.n != s.size()) return 5;
      put_hex((const uint8_t*)s.data(), s.size());
    } else {
      std::string s;
      yc::JString w{s};
      uint32_t rem[4];
      yc::JStack<4> st(rem);
      yc::SegCursor cur(b, b0, b1, yc::REF_STRING, e1 - e0, op == "E", halves);
      for (uint32_t k = 0;; ++k) {
        const size_t mark = s.size();
        if (k) s.push_back(',');
        const uint32_t el = cur.next(w, st);
        if (el == yc::EL_END) { s.resize(mark); break; }
        if (el != yc::EL_OK) return 6;
        if (k > e1 - e0) return 7;  // more elements than units
      }
      put_hex((const uint8_t*)s.data(), s.size());
    }
    free(b);
  }
  return 0;
}
