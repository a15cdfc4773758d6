// Host build of the number writers (tests/test_num_text.py). stdin, one case per line:
//   D <16 hex digits>  a double's bit pattern through yc_json.h json_put_number into a JString
//   F <8 hex digits>   a float32's bit pattern, widened, the same way
//   N <text>          a JSON number text through yc_num.h json_number_canon
// stdout: the text of each, one per line ("!" when json_number_canon refuses the digits).
// The number text sits in a heap block of its exact size and the output in one of the 32 bytes
// json_number_canon asks for, so a sanitizer build sees any read or write past either.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <string>

#include "yc_json.h"

int main() {
  std::string line, out;
  while (std::getline(std::cin, line)) {
    if (line.size() < 3 || line[1] != ' ') continue;
    if (line[0] == 'D' || line[0] == 'F') {
      const uint64_t u = strtoull(line.c_str() + 2, nullptr, 16);
      double x;
      if (line[0] == 'D') {
        memcpy(&x, &u, 8);
      } else {  // widened as any_json_text widens tag 124
        const uint32_t u32 = (uint32_t)u;
        float f;
        memcpy(&f, &u32, 4);
        x = (double)f;
      }
      std::string text;
      yc::JString ws{text};
      yc::json_put_number(ws, x);
      out += text;
    } else if (line[0] == 'N') {
      const size_t n = line.size() - 2;
      uint8_t* in = (uint8_t*)malloc(n);
      memcpy(in, line.data() + 2, n);
      char* t = (char*)malloc(32);
      const uint32_t m = yc::json_number_canon(in, 0, (uint32_t)n, t);
      if (m) out.append(t, m); else out += '!';
      free(t);
      free(in);
    } else {
      continue;
    }
    out += '\n';
  }
  fwrite(out.data(), 1, out.size(), stdout);
  return 0;
}
