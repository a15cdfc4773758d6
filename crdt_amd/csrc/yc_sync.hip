// yc_sync.hip — batched sync replies (ycrdt_docs_diff): Y.encodeStateAsUpdate(docs[i], svs[i]) for
// many (document, peer state vector) pairs, answered from the resident canonical states.
//
// A reply is [block count][the state's client blocks the peer lacks, in the state's order][the
// state's delete set]. A block the peer has nothing of is the state's bytes; a block the peer has
// part of is a new header (n - k, client, svc), the struct holding svc written at its offset
// (Item.write(encoder, offset), Y@80416) and the structs behind it — the state's bytes again, since
// Item.write(encoder, 0) does not depend on position. So a reply is a plan (k_sync_plan: which
// blocks, which struct is cut, found from the state's struct-start bitmap without decoding the
// document), sizes (k_sync_pairs, k_sync_offsets), a few written bytes and a list of verbatim
// ranges (k_sync_write -> copy_pieces). Every read of state bytes is bounded by the block's end,
// which is checked against the state's length first; an inconsistency between a state and its
// marks raises ERR_DECODE (YCRDT_DEBUG_BOUNDS: the bounds error of the other kernels).
#include "yc_sync.h"

namespace yc {
namespace {

constexpr uint32_t CUT_REFUSED = 0xFFFFFFFFu;  // the peer's clock falls inside a surrogate pair: Yjs throws (content_slice_walk, e0_write)
constexpr uint32_t CUT_BAD = 0xFFFFFFFEu;      // the bytes are no struct that can be cut there

__device__ __forceinline__ void sync_fail(SyncCtr* ctr, uint32_t dbg, uint32_t where) {
  if (atomicCAS(&ctr->err, 0u, dbg ? (uint32_t)ERR_CAPACITY : (uint32_t)ERR_DECODE) == 0u)
    ctr->err_info = dbg ? (0xB0DE0000u | BOUNDS_SYNC) : where;
}

// clock of `client` in a sorted state-vector run
__device__ __forceinline__ bool sv_find(const uint32_t* __restrict__ k, const uint32_t* __restrict__ v, uint32_t off, uint32_t n,
                                        uint32_t client, uint32_t& clock) {
  const uint32_t i = lower_bound_u32(k + off, n, client);
  if (i >= n || k[off + i] != client) return false;
  clock = v[off + i];
  return true;
}

__device__ __forceinline__ uint32_t hdr_size(uint32_t n, uint32_t client, uint32_t clock) {
  return vu_size(n) + vu_size(client) + vu_size(clock);
}

// Clock length of the struct at s, from its bytes alone (never past `end`): the info byte, the
// origin / right-origin ids or the parent and parentSub are skipped, then GC / Deleted: the varuint,
// Any / JSON: the count, String: the UTF-16 units of its UTF-8 bytes, everything else 1. No value
// is skipped: the caller knows the next struct's start. cpos = the content's first byte.
__device__ __forceinline__ uint32_t struct_len_at(const uint8_t* __restrict__ b, uint32_t s, uint32_t end, uint32_t& cpos, bool& ok) {
  uint32_t p = s;
  cpos = s;
  if (p >= end) { ok = false; return 0; }
  const uint32_t info = b[p++], ref = info & 31u;
  if (ref == REF_GC) { cpos = p; return rd_vu(b, p, end, ok); }
  if (ref > REF_DOC) { ok = false; return 0; }
  if (info & 0x80u) { rd_vu(b, p, end, ok); rd_vu(b, p, end, ok); }
  if (info & 0x40u) { rd_vu(b, p, end, ok); rd_vu(b, p, end, ok); }
  if (!(info & 0xC0u)) {
    const uint32_t pinfo = rd_vu(b, p, end, ok);
    if (pinfo == 1) {
      const uint32_t n = rd_vu(b, p, end, ok);
      if (ok) skip_bytes(p, n, end, ok);
    } else {
      rd_vu(b, p, end, ok);
      rd_vu(b, p, end, ok);
    }
    if (info & 0x20u) {
      const uint32_t n = rd_vu(b, p, end, ok);
      if (ok) skip_bytes(p, n, end, ok);
    }
  }
  cpos = p;
  if (!ok) return 0;
  if (ref == REF_DELETED || ref == REF_ANY || ref == REF_JSON) return rd_vu(b, p, end, ok);
  if (ref == REF_STRING) {
    const uint32_t k = rd_vu(b, p, end, ok);
    if (!ok || end - p < k) { ok = false; return 0; }
    uint32_t u = 0;
    for (uint32_t i = 0; i < k; ++i) {
      const uint32_t c = b[p + i];
      u += ((c & 0xC0u) != 0x80u ? 1u : 0u) + (c >= 0xF0u ? 1u : 0u);  // a 4-byte sequence is a surrogate pair
    }
    return u;
  }
  return 1;
}

// The struct at [pos, cend) of `client`, clock length len, written at offset off > 0
// (Item.write(encoder, off) / GC.write): the info byte is the state's with the origin bit set (the
// right-origin bit and bit 0x20 as the state has them), the origin is (client, clock + off - 1),
// the right origin is copied, no parent and no parentSub, the content sliced. Returns the bytes.
template <bool WRITE>
__device__ uint32_t cut_struct(const uint8_t* __restrict__ st, uint32_t pos, uint32_t cend, uint32_t client, uint32_t clock,
                               uint32_t off, uint32_t len, uint8_t* __restrict__ out, uint64_t q0) {
  uint64_t q = q0;
  bool ok = true;
  uint32_t cpos;
  if (struct_len_at(st, pos, cend, cpos, ok) != len || !ok || off >= len) return CUT_BAD;
  const uint32_t info = st[pos], ref = info & 31u, rem = len - off;
  if (ref == REF_GC) {
    if (WRITE) { out[q++] = REF_GC; wr_vu(out, q, rem); }
    return 1 + vu_size(rem);
  }
  uint32_t p = pos + 1;
  if (info & 0x80u) { rd_vu(st, p, cend, ok); rd_vu(st, p, cend, ok); }
  const uint32_t ro0 = p;
  if (info & 0x40u) { rd_vu(st, p, cend, ok); rd_vu(st, p, cend, ok); }
  const uint32_t ro1 = p;
  if (!ok) return CUT_BAD;
  uint32_t size = 1 + vu_size(client) + vu_size(clock + off - 1) + (ro1 - ro0);
  if (WRITE) {
    out[q++] = (uint8_t)(info | 0x80u);
    q = wr_vu(out, q, client);
    q = wr_vu(out, q, clock + off - 1);
    for (uint32_t i = ro0; i < ro1; ++i) out[q++] = st[i];
  }
  if (ref == REF_DELETED) {
    if (WRITE) wr_vu(out, q, rem);
    return size + vu_size(rem);
  }
  if (ref != REF_ANY && ref != REF_JSON && ref != REF_STRING) return CUT_BAD;  // (length 1: never cut)
  uint32_t celem = cpos;
  rd_vu(st, celem, cend, ok);  // the element count / the string's byte length
  if (!ok) return CUT_BAD;
  const uint64_t r = content_slice_walk(st, ref, celem, cpos, cend, off, len, true);  // (off: the peer's clock)
  if (r == ~0ull) return CUT_REFUSED;
  const uint32_t b0 = (uint32_t)r, b1 = (uint32_t)(r >> 32);
  if (b0 > b1 || b1 > cend) return CUT_BAD;
  const uint32_t lead = ref == REF_STRING ? b1 - b0 : rem;
  if (WRITE) {
    q = wr_vu(out, q, lead);
    if (ref == REF_STRING) str_copy(out, q, st + b0, b1 - b0);
    else for (uint32_t i = b0; i < b1; ++i) out[q++] = st[i];
  }
  return size + vu_size(lead) + (b1 - b0);
}

// Mark-less states (a fleet merged by ycrdt_apply_updates_multi): one lane per document walks the
// struct section with parse_struct and leaves what a doc's marks hold — struct starts, one record
// per client block (slot = blocks - 1 - position, so the state's order is descending slot as in the
// marks), the delete-set start. The plan then reads both kinds of document the same way.
__global__ __launch_bounds__(64) void k_sync_walk(const SyncDoc* __restrict__ docs, const SyncWalk* __restrict__ walks, uint32_t nwalk,
                                                  SyncCtr* ctr, uint32_t dbg) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nwalk) return;
  const SyncWalk W = walks[t];
  const SyncDoc D = docs[W.doc];
  const uint8_t* __restrict__ b = D.state;
  const uint32_t end = D.state_len;
  Section none;
  none.upd = 0; none.n = 0; none.client = 0; none.clock = 0; none.first_pos = NONE; none.cidx = NONE; none.first_idx = NONE; none.pad = 0;
  for (uint32_t s = 0; s < D.nslots; ++s) W.secs[s] = none;
  W.meta[0] = 0; W.meta[1] = end; W.meta[2] = D.nslots;
  uint32_t p = 0;
  bool ok = true;
  const uint32_t nb = rd_vu(b, p, end, ok);
  if (!ok || nb > D.nslots) { sync_fail(ctr, dbg, 0x5A000001u); return; }
  for (uint32_t i = 0; i < nb; ++i) {
    Section sec = none;
    sec.n = rd_vu(b, p, end, ok);
    sec.client = rd_vu(b, p, end, ok);
    sec.clock = rd_vu(b, p, end, ok);
    sec.first_pos = p;
    if (!ok || !sec.n) { sync_fail(ctr, dbg, 0x5A000002u); return; }
    for (uint32_t k = 0; k < sec.n; ++k) {
      if (p >= end) { sync_fail(ctr, dbg, 0x5A000003u); return; }
      W.fbits[p >> 6] |= 1ull << (p & 63);  // (the words are this lane's own)
      if (parse_struct<false>(b, p, end, 0xFFFFFFFFu, nullptr) != 1) { sync_fail(ctr, dbg, 0x5A000003u); return; }
    }
    W.secs[nb - 1 - i] = sec;
  }
  W.meta[0] = nb;
  W.meta[1] = p;
}

// One lane per (pair, client block) classifies it: (a) the peer has all of it — left out, (b) the
// peer has none of it — copied whole, (c) the peer's clock falls inside. The wavefront then takes
// its (c) blocks in turn: 64 words of the struct-start bitmap per step, one per lane; a lane reads
// the clock lengths of the structs starting in its 64 bytes; a wave-wide prefix sum of the lanes'
// sums finds the lane, and that lane the struct, that holds the peer's clock.
__global__ __launch_bounds__(256) void k_sync_plan(SyncArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63;
  SyncItem it;
  it.pair = 0; it.size = 0; it.npieces = 0; it.pos = 0; it.pbase = 0; it.hdr_pos = 0; it.end_pos = 0; it.cut_pos = NONE;
  it.off = 0; it.cut_clock = 0; it.k = 0; it.tail_pos = 0; it.len = 0; it.pad[0] = it.pad[1] = it.pad[2] = 0;
  bool need = false;
  uint32_t svc = 0;
  if (i < a.nitems) {
    uint32_t lo = 0, hi = a.np;  // the last pair whose first item is <= i
    while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a.pairs[mid].ibase <= i) lo = mid + 1; else hi = mid; }
    it.pair = lo - 1;
    const SyncPair P = a.pairs[it.pair];
    const SyncDoc D = a.docs[P.doc];
    const uint32_t slot = i - P.ibase;
    if (slot >= D.nslots) {
      sync_fail(a.ctr, a.dbg_bounds, 0x5A000010u);
    } else {
      const Section sec = D.secs[slot];
      if (sec.n) {
        const uint32_t ds = D.meta[1], hdr = hdr_size(sec.n, sec.client, sec.clock);
        uint32_t endp = ds;  // the next block of the state (the next lower slot that has one), else the delete set
        for (uint32_t s2 = slot; s2-- > 0;) {
          const Section o = D.secs[s2];
          if (o.n) { endp = o.first_pos - hdr_size(o.n, o.client, o.clock); break; }
        }
        uint32_t endc = 0;
        if (ds > D.state_len || sec.first_pos < hdr + 1 || sec.first_pos >= endp || endp > ds ||
            !sv_find(a.svk, a.svv, D.sv_off, D.sv_n, sec.client, endc)) {
          sync_fail(a.ctr, a.dbg_bounds, 0x5A000011u);
        } else {
          sv_find(a.svk, a.svv, P.sv_off, P.sv_n, sec.client, svc);
          it.hdr_pos = sec.first_pos - hdr;
          it.end_pos = endp;
          if (svc >= endc) {
            // (a)
          } else if (svc <= sec.clock) {  // (b)
            it.tail_pos = it.hdr_pos;
            it.size = endp - it.hdr_pos;
            it.npieces = (it.size + a.piece_max - 1) / a.piece_max;
          } else {
            need = true;
          }
        }
      }
    }
  }
  unsigned long long todo = __ballot(need);
  while (todo) {
    const int src = __ffsll((long long)todo) - 1;
    todo &= todo - 1;
    // the block of lane `src`, for every lane
    const uint32_t bi = (uint32_t)__shfl((int)i, src), bpair = (uint32_t)__shfl((int)it.pair, src);
    const uint32_t bsvc = (uint32_t)__shfl((int)svc, src), bend = (uint32_t)__shfl((int)it.end_pos, src);
    const SyncPair P = a.pairs[bpair];
    const SyncDoc D = a.docs[P.doc];
    const Section sec = D.secs[bi - P.ibase];
    const uint8_t* __restrict__ st = D.state;
    const uint32_t fp = sec.first_pos, w0 = fp >> 6, wl = (bend - 1) >> 6;
    uint32_t base = sec.clock, kbase = 0;
    // the result, in the finder lane: position, clock, index, length, bytes of the cut struct
    uint32_t r_pos = NONE, r_clock = 0, r_k = 0, r_len = 0, r_tail = 0, r_size = 0;
    int finder = -1;
    bool bad = false;
    for (uint32_t ws = w0; ws <= wl; ws += 64) {
      const uint32_t wi = ws + lane;
      uint64_t m = 0;
      if (wi <= wl) {
        m = D.fbits[wi];
        if (wi == w0) m &= ~0ull << (fp & 63);
        if (wi == wl && (bend & 63)) m &= (1ull << (bend & 63)) - 1;
      }
      uint32_t sum = 0;
      const uint32_t cnt = (uint32_t)__popcll(m);
      bool ok = true;
      for (uint64_t mm = m; mm; mm &= mm - 1) {
        uint32_t cp;
        sum += struct_len_at(st, (wi << 6) + (uint32_t)__ffsll((long long)mm) - 1, bend, cp, ok);
      }
      if (__ballot(!ok)) { bad = true; break; }
      uint32_t isum = sum, icnt = cnt;
      for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t x = (uint32_t)__shfl_up((int)isum, d), y = (uint32_t)__shfl_up((int)icnt, d);
        if (lane >= d) { isum += x; icnt += y; }
      }
      const uint32_t tot = (uint32_t)__shfl((int)isum, 63), totc = (uint32_t)__shfl((int)icnt, 63);
      if (bsvc - base >= tot) { base += tot; kbase += totc; continue; }
      const uint32_t c0 = base + isum - sum;
      const bool mine = sum && bsvc >= c0 && bsvc - c0 < sum;
      if (mine) {
        uint32_t c = c0, kk = kbase + icnt - cnt;
        for (uint64_t mm = m; mm; mm &= mm - 1, ++kk) {
          const uint32_t pos = (wi << 6) + (uint32_t)__ffsll((long long)mm) - 1;
          uint32_t cp;
          const uint32_t len = struct_len_at(st, pos, bend, cp, ok);
          if (bsvc - c < len) {
            r_pos = pos; r_clock = c; r_k = kk; r_len = len;
            // the next struct's start: the next set bit below the block's end
            uint64_t rest = (mm & (mm - 1));
            uint32_t nw = wi;
            while (!rest && nw < wl) {
              ++nw;
              rest = D.fbits[nw];
              if (nw == wl && (bend & 63)) rest &= (1ull << (bend & 63)) - 1;
            }
            r_tail = rest ? (nw << 6) + (uint32_t)__ffsll((long long)rest) - 1 : bend;
            break;
          }
          c += len;
        }
        if (r_pos != NONE && bsvc > r_clock) {
          r_size = cut_struct<false>(st, r_pos, r_tail, sec.client, r_clock, bsvc - r_clock, r_len, nullptr, 0);
        } else if (r_pos != NONE) {
          r_size = 0;        // the peer's clock is a struct's first: it is copied with the rest
          r_tail = r_pos;
        }
      }
      const unsigned long long hit = __ballot(mine && r_pos != NONE);
      if (hit) finder = __ffsll((long long)hit) - 1;
      break;
    }
    if (bad || finder < 0) {
      if (lane == (uint32_t)src) sync_fail(a.ctr, a.dbg_bounds, 0x5A000012u);
      continue;
    }
    const uint32_t f_pos = (uint32_t)__shfl((int)r_pos, finder), f_clock = (uint32_t)__shfl((int)r_clock, finder);
    const uint32_t f_k = (uint32_t)__shfl((int)r_k, finder), f_len = (uint32_t)__shfl((int)r_len, finder);
    const uint32_t f_tail = (uint32_t)__shfl((int)r_tail, finder), f_size = (uint32_t)__shfl((int)r_size, finder);
    if (lane == (uint32_t)src) {
      if (f_size == CUT_BAD || f_k >= sec.n || f_tail > bend || f_tail < f_pos) {
        sync_fail(a.ctr, a.dbg_bounds, 0x5A000013u);
      } else if (f_size == CUT_REFUSED) {
        a.pflag[bpair] = SYNC_REFUSED;  // (the block contributes nothing: the host takes the pair's reply from the per-doc path)
      } else {
        it.cut_pos = f_pos; it.cut_clock = f_clock; it.off = bsvc - f_clock; it.k = f_k; it.len = f_len; it.tail_pos = f_tail;
        it.size = hdr_size(sec.n - f_k, sec.client, bsvc) + f_size + (bend - f_tail);
        it.npieces = (bend - f_tail + a.piece_max - 1) / a.piece_max;
      }
    }
  }
  wave_count_add(&a.ctr->cut_structs, it.cut_pos != NONE && it.off > 0);
  if (i < a.nitems) a.items[i] = it;
}

// One wavefront per pair: the included blocks in the reply's order (descending slot) get their
// byte and piece prefixes; the pair its size (count, blocks, delete set) and piece count.
__global__ __launch_bounds__(256) void k_sync_pairs(SyncArgs a) {
  const uint32_t p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
  if (p >= a.np) return;
  if (p == 0 && lane == 0) { a.psize[a.np] = 0; a.ppieces[a.np] = 0; }
  const SyncPair P = a.pairs[p];
  const SyncDoc D = a.docs[P.doc];
  uint64_t run = 0;
  uint32_t runp = 0, nin = 0;
  for (uint32_t s0 = 0; s0 < D.nslots; s0 += 64) {
    const uint32_t r = s0 + lane;
    SyncItem* it = r < D.nslots ? &a.items[P.ibase + (D.nslots - 1 - r)] : nullptr;
    const uint32_t sz = it ? it->size : 0u, npc = it ? it->npieces : 0u;
    uint64_t isz = sz;
    uint32_t inp = npc;
    for (uint32_t d = 1; d < 64; d <<= 1) {
      const uint32_t xl = (uint32_t)__shfl_up((int)(uint32_t)isz, d), xh = (uint32_t)__shfl_up((int)(uint32_t)(isz >> 32), d);
      const uint32_t y = (uint32_t)__shfl_up((int)inp, d);
      if (lane >= d) { isz += ((uint64_t)xh << 32) | xl; inp += y; }
    }
    if (it) {
      const uint64_t at = run + isz - sz;
      it->pos = (uint32_t)min(at, (uint64_t)0xFFFFFFFFull);
      it->pbase = runp + inp - npc;
    }
    const uint32_t tl = (uint32_t)__shfl((int)(uint32_t)isz, 63), th = (uint32_t)__shfl((int)(uint32_t)(isz >> 32), 63);
    run += ((uint64_t)th << 32) | tl;
    runp += (uint32_t)__shfl((int)inp, 63);
    nin += (uint32_t)__popcll(__ballot(sz != 0));
  }
  if (lane == 0) {
    const uint32_t ds = D.meta[1], dslen = ds <= D.state_len ? D.state_len - ds : 0u;
    if (ds > D.state_len) sync_fail(a.ctr, a.dbg_bounds, 0x5A000020u);
    const uint64_t total = vu_size(nin) + run + dslen;
    if (total > 0xFFFFFFFFull) raise_err(&a.ctr->err, ERR_CAPACITY);  // a single reply over 4 GiB
    a.psize[p] = (uint32_t)min(total, (uint64_t)0xFFFFFFFFull);
    a.ppieces[p] = runp + (dslen + a.piece_max - 1) / a.piece_max;
    a.pincl[p] = nin;
  }
}

// the replies' 64-bit offsets and the pairs' piece bases (one workgroup)
__global__ __launch_bounds__(1024) void k_sync_offsets(SyncArgs a) {
  __shared__ uint64_t part[1024];
  __shared__ uint32_t part32[1024];
  block_scan_u32_u64<1024>(a.psize, a.offs, a.np + 1, part);
  block_scan_u32<1024>(a.ppieces, a.ppieces, a.np + 1, part32);
  if (threadIdx.x == 0) a.ctr->npieces = a.ppieces[a.np];
}

// One lane per included block: the new header and the cut struct written, the verbatim range —
// the whole block, or the structs behind the cut — emitted as pieces.
__global__ __launch_bounds__(256) void k_sync_write(SyncArgs a, uint8_t* __restrict__ out, Piece* __restrict__ pieces) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.nitems) return;
  const SyncItem it = a.items[i];
  if (!it.size) return;
  const SyncPair P = a.pairs[it.pair];
  const SyncDoc D = a.docs[P.doc];
  uint64_t q = a.offs[it.pair] + vu_size(a.pincl[it.pair]) + it.pos;
  const uint64_t qend = q + it.size;
  uint32_t from = it.hdr_pos;
  if (it.cut_pos != NONE) {
    const Section sec = D.secs[i - P.ibase];
    q = wr_vu(out, q, sec.n - it.k);
    q = wr_vu(out, q, sec.client);
    q = wr_vu(out, q, it.cut_clock + it.off);
    if (it.off) q += cut_struct<true>(D.state, it.cut_pos, it.tail_pos, sec.client, it.cut_clock, it.off, it.len, out, q);
    from = it.tail_pos;
  }
  if (q + (it.end_pos - from) != qend) { sync_fail(a.ctr, a.dbg_bounds, 0x5A000030u); return; }  // (sizes and bytes disagree)
  Piece* pc = pieces + a.ppieces[it.pair] + it.pbase;
  for (uint32_t k = from; k < it.end_pos; k += a.piece_max) {
    Piece X;
    X.src = D.state + k;
    X.dst = out + q;
    X.len = min(a.piece_max, it.end_pos - k);
    for (uint32_t j = 0; j < 8; ++j) X.inl[j] = 0;
    *pc++ = X;
    q += X.len;
  }
}
// one lane per pair: the block count in front, the state's delete set behind
__global__ __launch_bounds__(256) void k_sync_write_pairs(SyncArgs a, uint8_t* __restrict__ out, Piece* __restrict__ pieces) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.np) return;
  const SyncDoc D = a.docs[a.pairs[p].doc];
  wr_vu(out, a.offs[p], a.pincl[p]);
  const uint32_t ds = D.meta[1], dslen = ds <= D.state_len ? D.state_len - ds : 0u;
  const uint32_t npc = (dslen + a.piece_max - 1) / a.piece_max;
  Piece* pc = pieces + a.ppieces[p + 1] - npc;
  uint64_t q = a.offs[p + 1] - dslen;
  for (uint32_t k = ds; k < D.state_len; k += a.piece_max) {
    Piece X;
    X.src = D.state + k;
    X.dst = out + q;
    X.len = min(a.piece_max, D.state_len - k);
    for (uint32_t j = 0; j < 8; ++j) X.inl[j] = 0;
    *pc++ = X;
    q += X.len;
  }
}

}  // namespace

void launch_sync_walk(const SyncDoc* docs, const SyncWalk* walks, uint32_t nwalk, SyncCtr* ctr, uint32_t dbg_bounds, hipStream_t s) {
  if (nwalk) hipLaunchKernelGGL(k_sync_walk, dim3((nwalk + 63) / 64), dim3(64), 0, s, docs, walks, nwalk, ctr, dbg_bounds);
}
void launch_sync_plan(const SyncArgs& a, hipStream_t s) {
  if (a.nitems) hipLaunchKernelGGL(k_sync_plan, dim3((a.nitems + 255) / 256), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sync_pairs, dim3((a.np + 3) / 4), dim3(256), 0, s, a);
  hipLaunchKernelGGL(k_sync_offsets, dim3(1), dim3(1024), 0, s, a);
}
void launch_sync_write(const SyncArgs& a, uint8_t* out, Piece* pieces, hipStream_t s) {
  if (a.nitems) hipLaunchKernelGGL(k_sync_write, dim3((a.nitems + 255) / 256), dim3(256), 0, s, a, out, pieces);
  hipLaunchKernelGGL(k_sync_write_pairs, dim3((a.np + 255) / 256), dim3(256), 0, s, a, out, pieces);
}

}  // namespace yc
