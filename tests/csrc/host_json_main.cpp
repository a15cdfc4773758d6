// Host build of the view writer of yc_host.cpp (tests/test_host_json.py). stdin, one line each:
//   V <name>                                                  a new view; prints "V <name>"
//   S <client> <clock> <len> <flags> <ref> <unit> <hex|->     a list segment (content bytes as hex)
//   K <slot> <parent unit|-> <root name|-> <entry name|-> <seg0> <nseg>   a key (`-` entry: a list)
//   W <client> <clock> <len> <flags> <ref> <unit> <hex|->     the winner of the last key
//   I                                                         build the HostView and index() it
//   root <name> <kind> | type <root> <key|-> <kind> | entries <root> <key|->
//   mget <root> <nested key|-> <key> | aget <root> <nested key|-> <index>
// Every request prints "<request> => <state> <text>". The view's bytes live in a heap block of their
// exact size (segments in the order given), so a sanitizer build sees any read past the last segment.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "yc_host.h"

using namespace yc;

static std::vector<uint8_t> pool;

static void put(const std::string& hex, uint32_t& b0, uint32_t& b1) {
  b0 = (uint32_t)pool.size();
  if (hex != "-")
    for (size_t i = 0; i + 1 < hex.size(); i += 2) pool.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
  b1 = (uint32_t)pool.size();
}
static void put_name(const std::string& s, uint32_t& pos, uint32_t& len) {
  pos = (uint32_t)pool.size();
  len = s == "-" ? 0u : (uint32_t)s.size();
  if (s != "-") pool.insert(pool.end(), s.begin(), s.end());
}
static ViewSeg seg(std::istringstream& in) {
  ViewSeg s{};
  std::string hex;
  in >> s.client >> s.clock >> s.len >> s.flags >> s.ref >> s.unit >> hex;
  put(hex, s.b0, s.b1);
  return s;
}
static OpTarget target(const std::string& root, const std::string& key) {
  OpTarget t;
  t.root = root;
  t.nested = key != "-";
  if (t.nested) t.key = key;
  return t;
}

int main() {
  HostView v;
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string op, a, b, c;
    if (!(in >> op)) continue;
    std::string err, out;
    int state = 1;
    if (op == "V") {
      v = HostView();
      pool.clear();
      printf("%s\n", line.c_str());
      continue;
    } else if (op == "S") {
      v.segs.push_back(seg(in));
      continue;
    } else if (op == "K") {
      ViewKey K{};
      std::string parent, name, entry;
      in >> K.slot >> parent >> name >> entry >> K.seg0 >> K.nseg;
      K.parent_unit = parent == "-" ? VNONE : (uint32_t)strtoul(parent.c_str(), nullptr, 10);
      K.flags = entry == "-" ? 0u : VK_PSUB;
      put_name(name, K.name_pos, K.name_len);
      put_name(entry, K.psub_pos, K.psub_len);
      v.keys.push_back(K);
      continue;
    } else if (op == "W") {
      v.keys.back().win = seg(in);
      continue;
    } else if (op == "I") {
      v.bytes = std::vector<uint8_t>(pool.begin(), pool.end());  // capacity == size
      v.index();
      v.valid = true;
      continue;
    } else if (op == "root") {
      int kind;
      in >> a >> kind;
      view_root_json(v, a, kind, out, err);
    } else if (op == "type") {
      int kind;
      in >> a >> b >> kind;
      view_type_json(v, target(a, b), kind, out, err);
    } else if (op == "entries") {
      in >> a >> b;
      view_map_entries(v, target(a, b), out);
    } else if (op == "mget") {
      in >> a >> b >> c;
      view_map_get(v, target(a, b), c, state, out);
    } else if (op == "aget") {
      unsigned long long i;
      in >> a >> b >> i;
      view_array_get(v, target(a, b), i, state, out);
    } else {
      fprintf(stderr, "unknown line: %s\n", line.c_str());
      return 2;
    }
    printf("%s => %d %s\n", line.c_str(), state, out.c_str());
  }
  return 0;
}
