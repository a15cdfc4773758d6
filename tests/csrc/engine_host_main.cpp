// Test harness (TEST INFRASTRUCTURE ONLY): runs the pure-host helpers of the engine's host layer
// (crdt_amd/csrc/yc_engine_host.h) over command lines on stdin and prints what they give, one line per
// command. tests/test_engine_host.py holds the expected lines, written out by hand.
//   sv <hex|->                       parse_sv_sorted: "bad", or "ok client:clock ..."
//   marks <nw> <cap>                 marks_layout over a heap block of exactly its size, every region written
//                                    at its offset: the offsets of fbits sbits secs meta, the size
#include <cstdio>
#include <cstring>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "yc_engine_host.h"

static std::vector<uint8_t> unhex(const std::string& hex) {
  std::vector<uint8_t> b;
  if (hex == "-") return b;
  for (size_t i = 0; i + 1 < hex.size(); i += 2) b.push_back((uint8_t)std::stoul(hex.substr(i, 2), nullptr, 16));
  return b;
}
// the bytes in a heap block of their exact size (a read past the end is the sanitizer's to find)
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& b) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[b.size()]);
  if (!b.empty()) memcpy(p.get(), b.data(), b.size());
  return p;
}

int main() {
  char buf[1 << 16];
  while (fgets(buf, sizeof buf, stdin)) {
    std::istringstream in(buf);
    std::string cmd, tok;
    if (!(in >> cmd)) continue;
    if (cmd == "sv") {
      in >> tok;
      const std::vector<uint8_t> b = unhex(tok);
      const auto p = exact(b);
      std::vector<std::pair<uint32_t, uint32_t>> v{{9, 9}};  // (cleared by the call)
      if (!yc::parse_sv_sorted(p.get(), b.size(), v)) { printf("bad\n"); continue; }
      printf("ok");
      for (const auto& kv : v) printf(" %u:%u", kv.first, kv.second);
      printf("\n");
    } else if (cmd == "marks") {
      uint32_t nw = 0, cap = 0;
      in >> nw >> cap;
      const yc::MarksLayout at = yc::marks_layout(nw, cap, 32);  // (32 = sizeof(Section), asserted in yc_engine.hip)
      std::unique_ptr<uint8_t[]> block(new uint8_t[at.bytes]);
      memset(block.get(), 1, 8ull * nw);
      memset(block.get() + at.sbits, 2, 8ull * nw);
      memset(block.get() + at.secs, 3, 32ull * cap);
      memset(block.get() + at.meta, 4, 16);
      printf("fbits 0 sbits %zu secs %zu meta %zu bytes %zu nw %u cap %u\n", at.sbits, at.secs, at.meta, at.bytes, nw, cap);
    } else {
      printf("? %s\n", cmd.c_str());
    }
  }
  return 0;
}
