// Host build of yc_read.h's comparator and entry search (the ones the point-read kernels compile).
// stdin: "P <group> <hex name>" an entry present in container <group>, "A <group> <hex name>" a
// name to look for that is absent, "L <group> <hex name>" a present entry the search must call
// ambiguous for requests sharing its first READ_NAME_MAX bytes. The entries are sorted the way the
// device sorts them — stable passes, least significant key first: (length, slot), the name chunks
// from the last to the first, the group — and every answer is printed; any violation exits 1.
// Names sit in heap blocks of their exact size, so a read past a name aborts under ASan.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include <vector>

#include "yc_read.h"

using namespace yc;

struct Entry {
  uint64_t group;
  std::unique_ptr<uint8_t[]> name;  // exact size
  uint32_t len, slot;
  char kind;
};

struct Order {
  const std::vector<const Entry*>& v;
  uint64_t group(uint32_t p) const { return v[p]->group; }
  const uint8_t* name(uint32_t p) const { return v[p]->name.get(); }
  uint32_t len(uint32_t p) const { return v[p]->len; }
};

static std::string unhex(const std::string& h) {
  std::string o;
  for (size_t i = 0; i + 1 < h.size(); i += 2) o.push_back((char)std::stoi(h.substr(i, 2), nullptr, 16));
  return o;
}

static uint64_t chunk(const Entry& e, uint32_t c) {  // name bytes [8c, 8c + 8), big-endian, zero padded
  uint64_t k = 0;
  for (uint32_t j = 0; j < 8; ++j) {
    const uint32_t x = 8 * c + j;
    k = (k << 8) | (x < e.len ? e.name[x] : 0u);
  }
  return k;
}

int main() {
  std::vector<Entry> all;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream is(line);
    char kind;
    uint64_t g;
    std::string hex;
    is >> kind >> g;
    if (!(is >> hex)) hex.clear();
    if (hex == "-") hex.clear();
    const std::string n = unhex(hex);
    Entry e{g, std::unique_ptr<uint8_t[]>(new uint8_t[n.size()]), (uint32_t)n.size(), (uint32_t)all.size(), kind};
    if (!n.empty()) memcpy(e.name.get(), n.data(), n.size());
    all.push_back(std::move(e));
  }
  std::vector<const Entry*> v;
  for (const Entry& e : all)
    if (e.kind != 'A') v.push_back(&e);
  // the radix passes
  std::stable_sort(v.begin(), v.end(), [](const Entry* a, const Entry* b) {
    return (((uint64_t)a->len << 32) | a->slot) < (((uint64_t)b->len << 32) | b->slot);
  });
  for (uint32_t pass = 1; pass <= READ_NAME_MAX / 8; ++pass) {
    const uint32_t c = READ_NAME_MAX / 8 - pass;
    std::stable_sort(v.begin(), v.end(), [c](const Entry* a, const Entry* b) { return chunk(*a, c) < chunk(*b, c); });
  }
  std::stable_sort(v.begin(), v.end(), [](const Entry* a, const Entry* b) { return a->group < b->group; });
  const Order ord{v};
  const uint32_t n = (uint32_t)v.size();
  int bad = 0;
  for (uint32_t p = 0; p + 1 < n; ++p)
    if (read_order_cmp(ord.group(p), ord.name(p), ord.len(p), ord.group(p + 1), ord.name(p + 1), ord.len(p + 1)) >= 0) {
      printf("FAIL order %u\n", p);
      ++bad;
    }
  auto longer = [&](const Entry& q) {  // whether an L entry of q's group shares q's padded bytes
    for (const Entry& e : all)
      if (e.kind == 'L' && e.group == q.group && e.len > READ_NAME_MAX && read_same_padded(e.name.get(), e.len, q.name.get(), q.len)) return true;
    return false;
  };
  for (const Entry& q : all) {
    bool amb = false;
    const uint32_t p = read_find_name(ord, n, q.group, q.name.get(), q.len, amb);
    const bool want_amb = q.len > READ_NAME_MAX || longer(q);
    bool ok = amb == want_amb;
    if (!amb) {
      if (q.kind == 'A') ok = ok && p == READ_NONE;
      else ok = ok && p < n && v[p] == &q;
    }
    printf("%c %u %s %d\n", q.kind, q.slot, p == READ_NONE ? "none" : std::to_string(p).c_str(), amb ? 1 : 0);
    if (!ok) { printf("FAIL find %u\n", q.slot); ++bad; }
  }
  // an empty key set and a group past every entry
  bool amb = false;
  const std::vector<const Entry*> none;
  if (read_find_name(Order{none}, 0, 1, nullptr, 0, amb) != READ_NONE || amb) { printf("FAIL empty\n"); ++bad; }
  if (read_find_name(ord, n, ~0ull, nullptr, 0, amb) != READ_NONE || amb) { printf("FAIL past\n"); ++bad; }
  printf("%s %u\n", bad ? "BAD" : "OK", n);
  return bad ? 1 : 0;
}
