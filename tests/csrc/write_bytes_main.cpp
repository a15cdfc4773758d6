// Host build of yc_write.h's update writers (the ones the fleet-write kernels compile).
// stdin, one case per line, names and bytes as hex ("-": empty):
//   "I <client> <clock> <ref> <has_origin> <oc> <ok> <has_right> <rc> <rk> <parent_item> <pc> <pk>
//      <has_key> <root> <key> <lead> <content> <want>"     a one-item update
//   "D <n> (<client> <clock> <len>) x n <want>"            a delete-set update of n ranges, in the given order
// Each case is sized, then written into a heap block of exactly that size (a byte past it aborts
// under ASan), its names and content in exact-size blocks too, and compared with <want>. Every case
// prints "ok <size>" or "FAIL ..."; any violation exits 1.
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "yc_write.h"

using namespace yc;

static std::string unhex(const std::string& h) {
  std::string o;
  if (h == "-") return o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return o;
}

static std::unique_ptr<uint8_t[]> exact(const std::string& s) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[s.size()]);
  if (!s.empty()) memcpy(p.get(), s.data(), s.size());
  return p;
}

static bool same(const uint8_t* got, uint64_t n, const std::string& want, const char* what) {
  if (n == want.size() && (n == 0 || memcmp(got, want.data(), n) == 0)) return true;
  printf("FAIL %s: %llu bytes written, %zu wanted:", what, (unsigned long long)n, want.size());
  for (uint64_t i = 0; i < n; ++i) printf(" %02x", got[i]);
  printf("\n");
  return false;
}

int main() {
  std::string line;
  int bad = 0, cases = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream is(line);
    char kind;
    is >> kind;
    ++cases;
    if (kind == 'I') {
      WItem it{};
      uint32_t ho, hr, pi, hk;
      std::string root, key, content, want;
      is >> it.id.client >> it.id.clock >> it.ref >> ho >> it.origin.client >> it.origin.clock >> hr >> it.right.client >> it.right.clock >>
          pi >> it.parent.client >> it.parent.clock >> hk >> root >> key >> it.lead >> content >> want;
      if (!is) { printf("FAIL unreadable case: %s\n", line.c_str()); ++bad; continue; }
      const std::string r = unhex(root), k = unhex(key), c = unhex(content), w = unhex(want);
      const auto rp = exact(r), kp = exact(k), cp = exact(c);
      it.has_origin = ho != 0;
      it.has_right = hr != 0;
      it.parent_item = pi != 0;
      it.has_key = hk != 0;
      it.root = rp.get();
      it.root_len = (uint32_t)r.size();
      it.key = kp.get();
      it.key_len = (uint32_t)k.size();
      it.content = cp.get();
      it.content_len = (uint32_t)c.size();
      const uint64_t size = item_update_size(it);
      std::unique_ptr<uint8_t[]> out(new uint8_t[size]);
      const uint64_t wrote = item_update_write(out.get(), size, it);
      if (wrote != size) { printf("FAIL item: sized %llu, wrote %llu\n", (unsigned long long)size, (unsigned long long)wrote); ++bad; continue; }
      if (!same(out.get(), size, w, "item")) { ++bad; continue; }
      printf("ok %llu\n", (unsigned long long)size);
    } else if (kind == 'D') {
      uint32_t n = 0;
      is >> n;
      if (!is || n > WRITE_RANGES_MAX) { printf("FAIL ranges: %s\n", line.c_str()); ++bad; continue; }
      std::unique_ptr<WRange[]> r(new WRange[n]);
      for (uint32_t i = 0; i < n; ++i) is >> r[i].client >> r[i].clock >> r[i].len;
      std::string want;
      is >> want;
      if (!is) { printf("FAIL unreadable case: %s\n", line.c_str()); ++bad; continue; }
      const std::string w = unhex(want);
      const uint64_t size = ds_update_size(r.get(), n);
      std::unique_ptr<uint8_t[]> out(new uint8_t[size]);
      const uint64_t wrote = ds_update_write(out.get(), size, r.get(), n);
      if (wrote != size) { printf("FAIL delete set: sized %llu, wrote %llu\n", (unsigned long long)size, (unsigned long long)wrote); ++bad; continue; }
      if (!same(out.get(), size, w, "delete set")) { ++bad; continue; }
      printf("ok %llu\n", (unsigned long long)size);
    } else {
      printf("FAIL unknown case: %s\n", line.c_str());
      ++bad;
    }
  }
  printf("%s %d cases\n", bad ? "BAD" : "OK", cases);
  return bad ? 1 : 0;
}
