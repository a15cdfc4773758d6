// Test harness (TEST INFRASTRUCTURE ONLY): runs the pure-host helpers of the engine's host layer
// (crdt_amd/csrc/yc_engine_host.h) over command lines on stdin and prints what they give, one line per
// command. tests/test_engine_host.py holds the expected lines, written out by hand.
//   sv <hex|->                       parse_sv_sorted: "bad", or "ok client:clock ..."
//   marks <nw> <cap>                 marks_layout over a heap block of exactly its size, every region written
//                                    at its offset: the offsets of fbits sbits secs meta, the size
//   passbytes <unset|empty|text> <cap>  pass_bytes over the environment's text (unset: a null pointer, empty: "")
//   windows <pass_bytes> <len> ...   pass_windows: "[a,b) ..." one per window, or "none"
//   lay <bytes> ...                  Lay: the offset of every region, then the size
//   blob <hex|-> ...                 pack_blob over the parts, each in a heap block of its exact size: the
//                                    total, every offset, the blob's bytes (a zero total: its one byte is written)
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
    } else if (cmd == "passbytes") {
      uint64_t cap = 0;
      in >> tok >> cap;
      const std::string text = tok == "empty" ? "" : tok;
      printf("%llu\n", (unsigned long long)yc::pass_bytes(tok == "unset" ? nullptr : text.c_str(), cap));
    } else if (cmd == "windows") {
      uint64_t pass = 0, len = 0;
      in >> pass;
      std::vector<uint64_t> lens;
      while (in >> len) lens.push_back(len);
      const std::vector<size_t> cut = yc::pass_windows(lens, pass);
      if (cut.size() < 2) printf("none");
      for (size_t k = 0; k + 1 < cut.size(); ++k) printf("%s[%zu,%zu)", k ? " " : "", cut[k], cut[k + 1]);
      printf("\n");
    } else if (cmd == "lay") {
      yc::Lay lay;
      uint64_t bytes = 0;
      while (in >> bytes) printf("%llu ", (unsigned long long)lay(bytes));
      printf("size %llu\n", (unsigned long long)lay.at);
    } else if (cmd == "blob") {
      std::vector<std::vector<uint8_t>> bytes;
      std::vector<std::unique_ptr<uint8_t[]>> blocks;
      std::vector<yc::BlobPart> parts;
      while (in >> tok) {
        bytes.push_back(unhex(tok));
        blocks.push_back(exact(bytes.back()));
        parts.push_back(yc::BlobPart{blocks.back().get(), bytes.back().size()});
      }
      std::unique_ptr<uint64_t[]> offs(new uint64_t[parts.size() + 1]);
      uint64_t total = 99;
      uint8_t* blob = yc::pack_blob(parts, offs.get(), total);
      if (!blob) { printf("null\n"); continue; }
      if (!total) blob[0] = 0;
      printf("total %llu offs", (unsigned long long)total);
      for (size_t i = 0; i <= parts.size(); ++i) printf(" %llu", (unsigned long long)offs[i]);
      printf(" bytes %s", total ? "" : "-");
      for (uint64_t i = 0; i < total; ++i) printf("%02x", blob[i]);
      printf("\n");
      free(blob);
    } else {
      printf("? %s\n", cmd.c_str());
    }
  }
  return 0;
}
