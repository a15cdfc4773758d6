// The transaction planner of yc_write.h and the host analysis of yc_engine_host.h on the CPU
// (tests/test_write_chain.py builds this with -fsanitize=address,undefined and feeds it on stdin).
//
//   L own nseg {client clock len visible}*nseg nops {op index length count clock}*nops
//       a list given as segments and a chain of ops on it by client `own`; op i is planned behind
//       ops [0, i) with write_list_plan. Answer, one line per op:
//       P kind has origin.client origin.clock right.client right.clock why flags nr {client clock len}*nr
//       (the ranges after ds_ranges_merge)
//   A nops {op root parent_key key type_ref}*nops        ('-' is a null name)
//       transact_links. Answer: one line `K prev_entry prev_list creator why` per op, then `LONGEST n`
//       (-1 stands for WRITE_NONE)
// The last lines are `FLAGGED ranges pieces other` and `OK n cases`.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "yc_engine_host.h"
#include "yc_write.h"

using namespace yc;

struct Seg { uint32_t client, clock, len, visible; };

struct HostList {            // the view a lane reads on the device, over plain segments
  const std::vector<Seg>& s;
  uint64_t total() const {
    uint64_t n = 0;
    for (const Seg& x : s) n += x.visible ? x.len : 0;
    return n;
  }
  bool first(WId& id) const {
    if (s.empty()) return false;
    id = WId{s[0].client, s[0].clock};
    return true;
  }
  bool find(uint64_t t, size_t& x, uint32_t& off) const {
    uint64_t pos = 0;
    for (x = 0; x < s.size(); ++x) {
      if (!s[x].visible) continue;
      if (t - pos < s[x].len) { off = (uint32_t)(t - pos); return true; }
      pos += s[x].len;
    }
    return false;
  }
  bool at(uint64_t t, WId& id, bool& has_next, WId& next) const {
    size_t x;
    uint32_t off;
    if (!find(t, x, off)) return false;
    id = WId{s[x].client, s[x].clock + off};
    has_next = true;
    if (off + 1 < s[x].len) next = WId{s[x].client, s[x].clock + off + 1};
    else if (x + 1 < s.size()) next = WId{s[x + 1].client, s[x + 1].clock};
    else has_next = false;
    return true;
  }
  bool span(uint64_t t, uint64_t end, WRange& r) const {
    size_t x;
    uint32_t off;
    if (!find(t, x, off)) return false;
    const uint64_t left = s[x].len - off;
    r = WRange{s[x].client, s[x].clock + off, (uint32_t)(left < end - t ? left : end - t)};
    return true;
  }
};

int main() {
  std::string line;
  size_t cases = 0, f_ranges = 0, f_pieces = 0, f_other = 0;
  while (std::getline(std::cin, line)) {
    if (line.empty()) continue;
    std::istringstream in(line);
    std::string what;
    in >> what;
    ++cases;
    if (what == "L") {
      uint32_t own = 0;
      size_t nseg = 0, nops = 0;
      in >> own >> nseg;
      std::vector<Seg> segs(nseg);
      for (Seg& s : segs) in >> s.client >> s.clock >> s.len >> s.visible;
      in >> nops;
      std::vector<WriteReq> ops(nops);
      for (WriteReq& q : ops) {
        q = WriteReq{};
        in >> q.op >> q.index >> q.length >> q.lead >> q.clock;
        q.client = own;
      }
      if (!in) { printf("FAIL parse %zu\n", cases); return 1; }
      const HostList v{segs};
      for (size_t i = 0; i < nops; ++i) {
        std::vector<uint32_t> chain(i);  // exactly the earlier ops: a read past them is the sanitizer's to find
        for (size_t k = 0; k < i; ++k) chain[k] = (uint32_t)k;
        WritePlan p{};
        int32_t why = WHY_OK;
        uint32_t flags = 0;
        write_list_plan(v, ops.data(), chain.data(), (uint32_t)i, ops[i], p, why, flags);
        if (flags) { p.kind = 0; p.nr = 0; }
        if (flags & WF_RANGES) ++f_ranges;
        else if (flags & WF_PIECES) ++f_pieces;
        else if (flags) ++f_other;
        if (p.kind == 2) p.nr = ds_ranges_merge(p.r, p.nr);
        printf("P %u %u %u %u %u %u %d %u %u", p.kind, p.has, p.origin.client, p.origin.clock, p.right.client, p.right.clock, why, flags,
               p.kind == 2 ? p.nr : 0u);
        for (uint32_t k = 0; p.kind == 2 && k < p.nr; ++k) printf(" %u %u %u", p.r[k].client, p.r[k].clock, p.r[k].len);
        printf("\n");
      }
    } else if (what == "A") {
      size_t nops = 0;
      in >> nops;
      std::vector<std::string> names(nops * 3);
      std::vector<TransactOp> ops(nops);
      for (size_t i = 0; i < nops; ++i) {
        in >> ops[i].op >> names[3 * i] >> names[3 * i + 1] >> names[3 * i + 2] >> ops[i].type_ref;
      }
      if (!in) { printf("FAIL parse %zu\n", cases); return 1; }
      auto name = [&](size_t k) { return names[k] == "-" ? nullptr : names[k].c_str(); };
      for (size_t i = 0; i < nops; ++i) {
        ops[i].root = name(3 * i);
        ops[i].parent_key = name(3 * i + 1);
        ops[i].key = name(3 * i + 2);
      }
      std::vector<WriteLink> links;
      const uint32_t longest = transact_links(ops, links);
      for (const WriteLink& l : links) printf("K %d %d %d %d\n", (int)l.prev_entry, (int)l.prev_list, (int)l.creator, l.why);
      printf("LONGEST %u\n", longest);
    } else {
      printf("FAIL line %zu\n", cases);
      return 1;
    }
  }
  printf("FLAGGED %zu %zu %zu\n", f_ranges, f_pieces, f_other);
  printf("OK %zu cases\n", cases);
  return 0;
}
