// yc_write_ops.h — what the fleet writes' device side (yc_write.h) and the engine's host analysis
// (yc_engine_host.h, which builds without the parsers) both name: the op kinds, why an op fails, and
// the links of a transaction's op to the earlier ops of its call (ycrdt_docs_transact).
#pragma once
#include <cstdint>

namespace yc {

constexpr uint32_t WRITE_NONE = 0xFFFFFFFFu;

enum : uint32_t { WR_MAP_SET = 0, WR_MAP_SET_TYPE = 1, WR_MAP_DELETE = 2, WR_ARRAY_INSERT = 3, WR_ARRAY_PUSH = 4, WR_ARRAY_DELETE = 5 };  // = YCRDT_WRITE_*

// why an op fails with YCRDT_E_ARG (the single call's message)
enum : int32_t { WHY_OK = 0, WHY_NO_TYPE = 1, WHY_MISMATCH = 2, WHY_LENGTH = 3 };

constexpr uint32_t WRITE_CHAIN_MAX = 8;  // ops of one call on one list or one map entry the device takes

struct WriteLink {           // what the host's analysis (yc_engine_host.h transact_links) found for one op
  uint32_t prev_entry;       // the previous op of the call on the same map entry (WRITE_NONE: none)
  uint32_t prev_list;        // ... on the same list
  uint32_t creator;          // the MAP_SET_TYPE of this call that made its container (WRITE_NONE: the view's)
  int32_t why;               // WHY_NO_TYPE / WHY_MISMATCH: an earlier op of the call took its container away
};

}  // namespace yc
