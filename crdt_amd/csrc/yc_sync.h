// yc_sync.h — batched sync replies (ycrdt_docs_diff): Y.encodeStateAsUpdate(doc, sv) for many
// (document, peer state vector) pairs, answered from the documents' resident states without a
// decode or a merge (yc_sync.hip; DESIGN.md §Sync replies). Positions are the state's own.
#pragma once
#include "yc_common.h"
#include "yc_work.h"

namespace yc {

struct SyncDoc {             // one resident document named by the call
  const uint8_t* state;      // its canonical state in HBM
  const uint64_t* fbits;     // struct-start bitmap of the state (the doc's marks, or the walk's)
  const Section* secs;       // [nslots] client blocks, the state's byte order = descending slot (n = 0: no block)
  const uint32_t* meta;      // meta[1] = delete-set start
  uint32_t state_len;
  uint32_t nslots;
  uint32_t sv_off, sv_n;     // the doc's own state vector (end clocks) in the sorted sv arrays
};
struct SyncWalk {            // a mark-less document the walk gives temporary marks
  uint32_t doc;              // index into the SyncDoc table
  uint32_t pad;
  uint64_t* fbits;           // zeroed words of its own
  Section* secs;
  uint32_t* meta;
};
struct SyncPair {
  uint32_t doc;
  uint32_t sv_off, sv_n;     // the peer's state vector, clients ascending
  uint32_t ibase;            // first plan item (one per slot of its doc)
};
struct SyncItem {            // plan of one (pair, client block)
  uint32_t pair;
  uint32_t size;             // bytes the block contributes to the reply (0: left out)
  uint32_t npieces;          // verbatim pieces of at most piece_max bytes
  uint32_t pos, pbase;       // their prefixes in the reply's block order (k_sync_pairs)
  uint32_t hdr_pos, end_pos; // the block in the state: [header start, next header / delete set)
  uint32_t cut_pos;          // NONE: the block is copied whole; else the struct holding the peer's clock
  uint32_t off;              // clock offset inside it (0: it is copied too)
  uint32_t cut_clock;
  uint32_t k;                // structs left out in front of it
  uint32_t tail_pos;         // first verbatim byte behind the new header and the re-encoded struct
  uint32_t len;              // the cut struct's clock length
  uint32_t pad[3];
};
struct SyncCtr {
  uint32_t err, err_info, cut_structs, npieces;
};
constexpr uint32_t SYNC_REFUSED = 1;  // pair flag: the slice helper refused the cut (the per-doc path answers)

struct SyncArgs {
  const SyncDoc* docs;
  const SyncPair* pairs;
  const uint32_t* svk;       // state-vector clients / clocks, one sorted run per pair and per doc
  const uint32_t* svv;
  SyncItem* items;
  uint32_t* psize;           // [np + 1] reply bytes
  uint32_t* ppieces;         // [np + 1] pieces, then their exclusive scan
  uint32_t* pincl;           // [np] included blocks
  uint32_t* pflag;           // [np]
  uint64_t* offs;            // [np + 1]
  SyncCtr* ctr;
  uint32_t np, nitems;
  uint32_t piece_max;
  uint32_t dbg_bounds;
};

void launch_sync_walk(const SyncDoc* docs, const SyncWalk* walks, uint32_t nwalk, SyncCtr* ctr, uint32_t dbg_bounds, hipStream_t s);
void launch_sync_plan(const SyncArgs& a, hipStream_t s);   // plan, per-pair sizes, offsets
void launch_sync_write(const SyncArgs& a, uint8_t* out, Piece* pieces, hipStream_t s);  // headers, cut structs, pieces

}  // namespace yc
