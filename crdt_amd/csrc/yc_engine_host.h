// yc_engine_host.h — the engine host layer's helpers that make no HIP call: state-vector parsing, the
// byte layout of a doc's marks block, and what the calls over many documents share (the bytes of a device
// pass, the pass windows, 64-byte aligned layouts, the answer blob, the dependencies among a transaction's ops). The header builds with a plain C++ compiler (tests/csrc/engine_host_main.cpp runs it under the sanitizers).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <unordered_map>
#include <utility>
#include <vector>

#include "yc_write_ops.h"  // WriteLink, WR_*, WHY_*

#pragma GCC visibility push(hidden)
namespace yc {

// decode a state vector (varuint n, (client, clock) × n): put(client, clock) per entry
template <class Put>
bool parse_sv_each(const uint8_t* p, size_t n, Put put) {
  size_t pos = 0;
  auto vu = [&](uint32_t& v) -> bool {
    uint32_t r = 0;
    int shift = 0;
    for (;;) {
      if (pos >= n) return false;
      uint32_t b = p[pos++];
      if (shift < 32) r |= (b & 0x7fu) << shift;
      shift += 7;
      if (b < 0x80) { v = r; return true; }
      if (shift >= 35) return false;  // (a 32-bit value ends within 5 bytes: a 6th is refused, not dropped)
    }
  };
  uint32_t k;
  if (!vu(k)) return false;
  for (uint32_t i = 0; i < k; ++i) {
    uint32_t c, cl;
    if (!vu(c) || !vu(cl)) return false;
    put(c, cl);
  }
  return true;
}
inline bool parse_sv(const uint8_t* p, size_t n, std::unordered_map<uint32_t, uint32_t>& out) {
  return parse_sv_each(p, n, [&](uint32_t c, uint32_t cl) { out[c] = cl; });
}
// the same as (client, clock) pairs with the clients ascending (a client named twice: its last
// clock, as the map gives). Yjs writes state vectors in descending or store order: no hashing,
// and no sort when the input is already in either order.
inline bool parse_sv_sorted(const uint8_t* p, size_t n, std::vector<std::pair<uint32_t, uint32_t>>& v) {
  v.clear();
  if (!parse_sv_each(p, n, [&](uint32_t c, uint32_t cl) { v.emplace_back(c, cl); })) return false;
  auto before = [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; };
  auto after = [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first > b.first; };
  if (std::adjacent_find(v.begin(), v.end(), [&](const auto& a, const auto& b) { return !before(a, b); }) == v.end()) return true;
  if (std::adjacent_find(v.begin(), v.end(), [&](const auto& a, const auto& b) { return !after(a, b); }) == v.end()) {
    std::reverse(v.begin(), v.end());
    return true;
  }
  std::stable_sort(v.begin(), v.end(), before);
  size_t w = 0;
  for (size_t i = 0; i < v.size(); ++i) {
    if (i + 1 < v.size() && v[i + 1].first == v[i].first) continue;  // (the last of equal clients wins)
    v[w++] = v[i];
  }
  v.resize(w);
  return true;
}

// The marks block of a doc (yc_work.h PreMarks; written by k_state_marks, read by k_predecoded and the
// sync replies): fbits[nw] | sbits[nw] | secs[cap] | meta, nw = the state's 64-byte words, cap = its
// client slots + 1, section_bytes = sizeof(Section). THE definition of the block's byte layout: the
// allocation and every reader take their offsets from here (fbits is at 0).
struct MarksLayout {
  size_t sbits, secs, meta, bytes;
};
inline MarksLayout marks_layout(uint32_t nw, uint32_t cap, size_t section_bytes) {
  MarksLayout m;
  m.sbits = 8ull * nw;
  m.secs = 16ull * nw;
  m.meta = m.secs + section_bytes * cap;
  m.bytes = m.meta + 16;
  return m;
}

// ---- shared by the calls over many documents (ycrdt_docs_json / _cache / _read / _write / _diff)

// Resident state bytes merged per device pass (one 4 GiB window holds them), and the state from
// which a document is too large for the device path of these calls.
constexpr uint64_t JSON_PASS_BYTES = uint64_t(1) << 31;

// Resident state bytes merged per device pass: `cap`, or what the call's environment variable `env`
// asks for (tests shrink a pass to run the several-pass path on a few documents): unset or 0 is the
// cap, and no value exceeds it.
inline uint64_t pass_bytes(const char* env, uint64_t cap) {
  const uint64_t x = env ? strtoull(env, nullptr, 10) : 0;
  return x ? std::min(x, cap) : cap;
}

// The device passes over documents of the state lengths `lens`: documents in call order, as many as
// one pass holds (each padded to 64 bytes, 64 spare), a window never empty. Window k is the documents
// [cut[k], cut[k + 1]); no documents: no window.
inline std::vector<size_t> pass_windows(const std::vector<uint64_t>& lens, uint64_t pass_bytes) {
  std::vector<size_t> cut{0};
  uint64_t bytes = 0;
  for (size_t j = 0; j < lens.size(); ++j) {
    if (j > cut.back() && bytes + lens[j] + 64 > pass_bytes) { cut.push_back(j); bytes = 0; }
    bytes += (lens[j] + 63) & ~uint64_t(63);
  }
  if (!lens.empty()) cut.push_back(lens.size());
  return cut;
}

// offsets of consecutive regions, each starting on a 64-byte line; `at` is the size so far
struct Lay {
  uint64_t at = 0;
  uint64_t operator()(uint64_t bytes) {
    const uint64_t o = at;
    at = (at + bytes + 63) & ~uint64_t(63);
    return o;
  }
};

// The answer blob of a call: the parts back to back in one malloc'ed block, part i at offs[i], the
// total at offs[parts.size()] and in `total`. A zero total gives a one-byte block; nullptr: the
// allocation failed.
struct BlobPart {
  const void* p;
  size_t len;
};
inline uint8_t* pack_blob(const std::vector<BlobPart>& parts, uint64_t* offs, uint64_t& total) {
  total = 0;
  for (size_t i = 0; i < parts.size(); ++i) { offs[i] = total; total += parts[i].len; }
  offs[parts.size()] = total;
  uint8_t* out = (uint8_t*)malloc(total ? total : 1);
  if (!out) return nullptr;
  for (size_t i = 0; i < parts.size(); ++i)
    if (parts[i].len) memcpy(out + offs[i], parts[i].p, parts[i].len);
  return out;
}

// ---- ycrdt_docs_transact: how the ops of ONE document in one call depend on one another
struct TransactOp {          // what the analysis reads of an op (ycrdt_write's fields)
  int op;                    // WR_*
  const char* root;
  const char* parent_key;    // nullptr: the root type
  const char* key;           // the map ops
  uint32_t type_ref;         // MAP_SET_TYPE
};

// For the ops of one document in call order: links[i] names the previous op on op i's map entry,
// the previous op on its list, and the MAP_SET_TYPE of this call that made its container (indices
// into ops; WRITE_NONE: none). A container is (root, parent_key, epoch): every op that writes the
// root-map entry (root, key = P) starts a new epoch of (root, P). Behind a MAP_SET_TYPE of the kind
// an op needs the container is new and empty; behind any other write there is none, and the op
// fails as the single call does (links[i].why). Such an op stands in no chain. Returns the longest chain.
inline uint32_t transact_links(const std::vector<TransactOp>& ops, std::vector<WriteLink>& links) {
  auto id = [](std::initializer_list<const char*> parts) {  // lengths in front of the names (a null part apart from "")
    std::string k;
    for (const char* p : parts) {
      const uint64_t len = p ? strlen(p) + 1 : 0;
      k.append((const char*)&len, 8);
      if (p) k += p;
    }
    return k;
  };
  struct Epoch { uint32_t n = 0, writer = WRITE_NONE; };  // writer: the latest op that wrote the root-map entry
  std::unordered_map<std::string, Epoch> epochs;
  std::unordered_map<std::string, uint32_t> last_entry, last_list;
  std::vector<uint32_t> depth(ops.size(), 1);
  uint32_t longest = ops.empty() ? 0 : 1;
  links.assign(ops.size(), WriteLink{WRITE_NONE, WRITE_NONE, WRITE_NONE, WHY_OK});
  for (uint32_t i = 0; i < ops.size(); ++i) {
    const TransactOp& q = ops[i];
    const bool map_op = q.op <= (int)WR_MAP_DELETE;
    WriteLink& L = links[i];
    uint32_t epoch = 0;
    if (q.parent_key) {
      const auto at = epochs.find(id({q.root, q.parent_key}));
      if (at != epochs.end()) {
        epoch = at->second.n;
        const TransactOp& w = ops[at->second.writer];
        if (w.op != (int)WR_MAP_SET_TYPE) L.why = WHY_NO_TYPE;
        else if (w.type_ref != (map_op ? 1u : 0u)) L.why = WHY_MISMATCH;
        else L.creator = at->second.writer;
      }
    }
    if (L.why == WHY_OK) {
      std::string container = id({q.root, q.parent_key});
      container.append((const char*)&epoch, 4);
      auto& last = map_op ? last_entry : last_list;
      const std::string k = map_op ? container + id({q.key}) : container;
      const auto at = last.find(k);
      if (at != last.end()) {
        (map_op ? L.prev_entry : L.prev_list) = at->second;
        depth[i] = depth[at->second] + 1;
        longest = std::max(longest, depth[i]);
      }
      last[k] = i;
    }
    if (map_op && !q.parent_key) {
      Epoch& e = epochs[id({q.root, q.key})];
      ++e.n;
      e.writer = i;
    }
  }
  return longest;
}

}  // namespace yc
#pragma GCC visibility pop
