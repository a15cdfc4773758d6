// yc_write.hip — fleet writes on gfx950 (ycrdt_docs_write): YMap.set / delete and YArray.insert /
// push / delete of many documents, encoded over the view of ONE multi-document merge after the front
// half of the fleet read pass (yc_json.hip: keys sorted by container and entry name; yc_read.hip:
// k_rvisible and its scan give the visible lengths). An op is one lane:
//   k_wplan       the root container by (document, root name hash) — k_jindex has compared the
//                 names —, a nested target through the parent key's entry as k_rresolve does, then
//                 what the op's update names: the entry's last item (typeMapSet's origin), the
//                 entry's range (typeMapDelete), the element at index - 1 and what follows it in the
//                 list (typeListInsertGenericsAfter), or the visible ranges a delete covers
//                 (typeListDelete); the update's byte size with the shared writers (yc_write.h)
//   k_wwrite      every update at its offset (one scan of the sizes), the values' bytes from the
//                 uploaded pool
//   k_tplan       k_wplan for ycrdt_docs_transact: an op behind earlier ops of its call on the same
//                 entry, list or freshly made container is planned through them (yc_write.h)
// Every index read from a view record is checked before use, every search is a bounded loop, no lane
// waits for another. What the bounds refuse is flagged and its document answered by the single calls.
#include "yc_common.h"
#define YC_JSON_DEVICE
#include "yc_write.h"

namespace yc {

namespace {

__device__ __forceinline__ WItem item_of(const JsonArgs& a, const WriteReq& q, const WritePlan& p) {
  WItem it{};
  it.id = WId{q.client, q.clock};
  it.ref = q.op == WR_MAP_SET_TYPE ? REF_TYPE : REF_ANY;
  it.has_origin = (p.has & 1u) != 0;
  it.has_right = (p.has & 2u) != 0;
  it.parent_item = (p.has & 4u) != 0;
  it.has_key = q.op <= WR_MAP_SET_TYPE;
  it.origin = p.origin;
  it.right = p.right;
  it.parent = p.parent;
  const JsonReq& root = a.reqs[q.root];
  it.root = a.names + root.name_pos;
  it.root_len = root.name_len;
  it.key = a.names + q.key_pos;
  it.key_len = q.key_len;
  it.lead = q.lead;
  it.content = a.names + q.any_pos;
  it.content_len = q.any_len;
  return it;
}

// the segment of list items [x0, x1) that holds visible element t (a position in the visible scan)
__device__ __forceinline__ bool seg_of(const WriteArgs& A, uint32_t x0, uint32_t x1, uint64_t t, uint32_t& x) {
  const uint64_t* sv = A.scan_v + A.j.ck;
  // the last segment that starts at or before the element: the ones without a visible element in
  // front of it start where it does
  x = x0 + upper_bound_u64(sv + x0, x1 - x0 + 1, t) - 1;
  return x >= x0 && x < x1 && t >= sv[x] && t - sv[x] < A.vis[A.j.ck + x];
}

__global__ void k_wplan(WriteArgs A) {
  const JsonArgs& a = A.j;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > A.nops) return;
  if (r == A.nops) { A.size[r] = 0; return; }
  const WriteReq q = A.ops[r];
  const bool map_op = q.op <= WR_MAP_DELETE;
  uint32_t flags = 0;
  int32_t why = WHY_OK;
  uint64_t size = 0;
  WritePlan p{};
  do {
    if (q.root >= a.nreq || q.op > WR_ARRAY_DELETE) { flags = RF_OPEN; break; }
    if (a.rflag[q.root]) { flags = RF_NAME; break; }
    uint64_t g = a.reqs[q.root].rkey;
    if (q.pkey_len != READ_NONE) {  // resolve_parent: the type stored in the root map under the parent key
      const uint32_t e = find_entry(a, g, a.names + q.pkey_pos, q.pkey_len, flags);
      if (flags) break;
      if (e == READ_NONE) { why = WHY_NO_TYPE; break; }
      const ViewSeg& w = a.keys[a.ord[e]].win;
      if (!(w.flags & VS_SET) || (w.flags & VS_DELETED) || w.ref != REF_TYPE) { why = WHY_NO_TYPE; break; }
      if (w.b0 > w.b1 || w.b1 > a.nbytes || !w.len) { flags = RF_OPEN; break; }
      JRd rd{a.bytes, w.b0, w.b1, true};
      const uint32_t tr = rd.vu();
      if (!rd.ok || tr != (map_op ? 1u : 0u)) { why = WHY_MISMATCH; break; }
      p.has |= 4u;
      p.parent = WId{w.client, w.clock + w.len - 1};
      g = (uint32_t)(w.unit + w.len - 1);
    }
    if (map_op) {
      const uint32_t e = find_entry(a, g, a.names + q.key_pos, q.key_len, flags);
      if (flags) break;
      const ViewSeg* w = e == READ_NONE ? nullptr : &a.keys[a.ord[e]].win;
      if (w && (w->flags & VS_SET) && !w->len) { flags = RF_OPEN; break; }
      if (q.op == WR_MAP_DELETE) {  // typeMapDelete: nothing unless the entry's item is there and alive
        if (!w || !(w->flags & VS_SET) || (w->flags & VS_DELETED)) break;
        p.kind = 2;
        p.nr = 1;
        p.r[0] = WRange{w->client, w->clock, w->len};
        break;
      }
      // typeMapSet: left = parent._map.get(key), the entry's rightmost item, deleted or not
      if (w && (w->flags & VS_SET)) { p.has |= 1u; p.origin = WId{w->client, w->clock + w->len - 1}; }
      p.kind = 1;
      break;
    }
    const uint32_t lo = lower_bound_u64(a.gk, a.ck, g), hi = upper_bound_u64(a.gk, a.ck, g);
    const uint32_t kp = first_list(a, lo, hi);
    uint32_t x0 = 0, x1 = 0;
    if (kp != VNONE && !list_range(a, kp, x0, x1)) { flags = RF_OPEN; break; }
    const uint64_t* sv = A.scan_v + a.ck;
    const uint64_t total = sv[x1] - sv[x0];
    if (q.op == WR_ARRAY_DELETE) {
      if (!q.length) break;
      const uint64_t from = q.index < total ? q.index : total;
      const uint64_t to = (uint64_t)q.index + q.length < total ? (uint64_t)q.index + q.length : total;
      uint64_t t = sv[x0] + from;
      const uint64_t end = sv[x0] + to;
      // one search per visible segment the range covers (the deleted ones between them are stepped over)
      for (uint32_t k = 0; k <= WRITE_RANGES_MAX && t < end; ++k) {
        uint32_t x = 0;
        if (!seg_of(A, x0, x1, t, x)) { flags = RF_OPEN; break; }
        if (p.nr == WRITE_RANGES_MAX) { flags = WF_RANGES; break; }
        const ViewSeg& s = a.segs[x];
        const uint64_t stop = sv[x] + A.vis[a.ck + x] < end ? sv[x] + A.vis[a.ck + x] : end;
        p.r[p.nr++] = WRange{s.client, s.clock + (uint32_t)(t - sv[x]), (uint32_t)(stop - t)};
        t = stop;
      }
      if (flags) break;
      if (p.nr) p.kind = 2;
      if ((uint64_t)q.index + q.length > total) why = WHY_LENGTH;  // Yjs throws after deleting what exists
      break;
    }
    // typeListInsertGenerics: left = the element at index - 1, right = whatever follows it in the
    // list, deleted or not
    if (total > 0xFFFFFFFFull) { flags = RF_SIZE; break; }
    const uint64_t index = q.op == WR_ARRAY_PUSH ? total : q.index;
    if (index > total) { why = WHY_LENGTH; break; }
    if (!q.lead) break;
    if (x1 > x0) {
      if (index == 0) {
        const ViewSeg& s = a.segs[x0];
        p.has |= 2u;
        p.right = WId{s.client, s.clock};
      } else {
        const uint64_t t = sv[x0] + index - 1;
        uint32_t x = 0;
        if (!seg_of(A, x0, x1, t, x)) { flags = RF_OPEN; break; }
        const ViewSeg& s = a.segs[x];
        const uint32_t off = (uint32_t)(t - sv[x]);
        p.has |= 1u;
        p.origin = WId{s.client, s.clock + off};
        if (off + 1 < s.len) { p.has |= 2u; p.right = WId{s.client, s.clock + off + 1}; }
        else if (x + 1 < x1) { p.has |= 2u; p.right = WId{a.segs[x + 1].client, a.segs[x + 1].clock}; }
      }
    }
    p.kind = 1;
  } while (false);
  if (flags) { p.kind = 0; p.nr = 0; }  // (a failed op has set no kind, but for the delete that runs past the end)
  if (p.kind == 1) size = item_update_size(item_of(a, q, p));
  else if (p.kind == 2) size = ds_update_size(p.r, p.nr);
  if (size > 0xFFFFFFF0ull) { flags |= RF_SIZE; size = 0; p.kind = 0; }
  A.plan[r] = p;
  A.size[r] = (uint32_t)size;
  A.why[r] = flags ? WHY_OK : why;
  A.flags[r] = flags;
}

// the list segments [x0, x1) as write_list_plan reads a view (x0 == x1: no list, or a container made in this call)
struct DevList {
  const WriteArgs& A;
  uint32_t x0, x1;
  __device__ __forceinline__ const uint64_t* sv() const { return A.scan_v + A.j.ck; }
  __device__ __forceinline__ uint64_t total() const { return sv()[x1] - sv()[x0]; }
  __device__ __forceinline__ bool first(WId& id) const {
    if (x1 <= x0) return false;
    id = WId{A.j.segs[x0].client, A.j.segs[x0].clock};
    return true;
  }
  __device__ __forceinline__ bool at(uint64_t t, WId& id, bool& has_next, WId& next) const {
    uint32_t x = 0;
    t += sv()[x0];
    if (!seg_of(A, x0, x1, t, x)) return false;
    const ViewSeg& s = A.j.segs[x];
    const uint32_t off = (uint32_t)(t - sv()[x]);
    id = WId{s.client, s.clock + off};
    has_next = true;
    if (off + 1 < s.len) next = WId{s.client, s.clock + off + 1};
    else if (x + 1 < x1) next = WId{A.j.segs[x + 1].client, A.j.segs[x + 1].clock};
    else has_next = false;
    return true;
  }
  __device__ __forceinline__ bool span(uint64_t t, uint64_t end, WRange& r) const {
    uint32_t x = 0;
    t += sv()[x0];
    end += sv()[x0];
    if (!seg_of(A, x0, x1, t, x)) return false;
    const ViewSeg& s = A.j.segs[x];
    const uint64_t stop = sv()[x] + A.vis[A.j.ck + x] < end ? sv()[x] + A.vis[A.j.ck + x] : end;
    r = WRange{s.client, s.clock + (uint32_t)(t - sv()[x]), (uint32_t)(stop - t)};
    return true;
  }
};

// k_wplan for ycrdt_docs_transact: an op with earlier ops of its call on the same map entry or list,
// or in a container one of them made, is planned behind them (yc_write.h). A lane reads the ops and
// links the host uploaded and the view, never what another lane writes; every walk along a chain
// is bounded by WRITE_CHAIN_MAX and every link must point at an earlier op.
__global__ void k_tplan(WriteArgs A, const WriteLink* links) {
  const JsonArgs& a = A.j;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r > A.nops) return;
  if (r == A.nops) { A.size[r] = 0; return; }
  const WriteReq q = A.ops[r];
  const WriteLink L = links[r];
  const bool map_op = q.op <= WR_MAP_DELETE;
  uint32_t flags = 0;
  int32_t why = WHY_OK;
  uint64_t size = 0;
  WritePlan p{};
  do {
    if (q.root >= a.nreq || q.op > WR_ARRAY_DELETE) { flags = RF_OPEN; break; }
    if (a.rflag[q.root]) { flags = RF_NAME; break; }
    if (L.why != WHY_OK) {  // an earlier op of the call replaced or removed the type under the parent key
      if (L.why != WHY_NO_TYPE && L.why != WHY_MISMATCH) { flags = WF_CHAIN; break; }
      why = L.why;
      break;
    }
    uint64_t g = a.reqs[q.root].rkey;
    bool fresh = false;  // the container was made in this call: no view behind it
    if (q.pkey_len != READ_NONE && L.creator != WRITE_NONE) {
      if (L.creator >= r) { flags = WF_CHAIN; break; }
      const WriteReq c = A.ops[L.creator];
      if (c.op != WR_MAP_SET_TYPE || c.client != q.client || c.root != q.root || c.lead != (map_op ? 1u : 0u)) { flags = WF_CHAIN; break; }
      p.has |= 4u;
      p.parent = WId{c.client, c.clock};
      fresh = true;
    } else if (q.pkey_len != READ_NONE) {  // resolve_parent: the type stored in the root map under the parent key
      const uint32_t e = find_entry(a, g, a.names + q.pkey_pos, q.pkey_len, flags);
      if (flags) break;
      if (e == READ_NONE) { why = WHY_NO_TYPE; break; }
      const ViewSeg& w = a.keys[a.ord[e]].win;
      if (!(w.flags & VS_SET) || (w.flags & VS_DELETED) || w.ref != REF_TYPE) { why = WHY_NO_TYPE; break; }
      if (w.b0 > w.b1 || w.b1 > a.nbytes || !w.len) { flags = RF_OPEN; break; }
      JRd rd{a.bytes, w.b0, w.b1, true};
      const uint32_t tr = rd.vu();
      if (!rd.ok || tr != (map_op ? 1u : 0u)) { why = WHY_MISMATCH; break; }
      p.has |= 4u;
      p.parent = WId{w.client, w.clock + w.len - 1};
      g = (uint32_t)(w.unit + w.len - 1);
    }
    if (map_op) {
      // back along the entry's chain to the latest set
      WriteReq set{};
      bool has_set = false, deleted = false;
      uint32_t k = L.prev_entry, below = r;
      for (uint32_t i = 0; i < WRITE_CHAIN_MAX - 1 && k != WRITE_NONE && !has_set; ++i) {
        if (k >= below) { flags = WF_CHAIN; break; }
        const WriteReq e = A.ops[k];
        if (e.op > WR_MAP_DELETE || e.client != q.client) { flags = WF_CHAIN; break; }
        if (e.op == WR_MAP_DELETE) deleted = true;
        else { set = e; has_set = true; }
        below = k;
        k = links[k].prev_entry;
      }
      if (flags) break;
      if (!has_set && k != WRITE_NONE) { flags = WF_CHAIN; break; }  // longer than the device takes
      WRange win{0, 0, 0};
      bool win_dead = false;
      if (!has_set && !fresh) {
        const uint32_t e = find_entry(a, g, a.names + q.key_pos, q.key_len, flags);
        if (flags) break;
        const ViewSeg* w = e == READ_NONE ? nullptr : &a.keys[a.ord[e]].win;
        if (w && (w->flags & VS_SET)) {
          if (!w->len) { flags = RF_OPEN; break; }
          win = WRange{w->client, w->clock, w->len};
          win_dead = (w->flags & VS_DELETED) != 0;
        }
      }
      write_entry_plan(q, has_set ? &set : nullptr, deleted, win, win_dead, p);
      break;
    }
    // the earlier ops on the list, in call order
    uint32_t chain[WRITE_CHAIN_MAX];
    uint32_t nc = 0;
    {
      uint32_t k = L.prev_list, below = r;
      for (uint32_t i = 0; i < WRITE_CHAIN_MAX - 1 && k != WRITE_NONE; ++i) {
        if (k >= below) { flags = WF_CHAIN; break; }
        const uint32_t eop = A.ops[k].op;
        if (eop < WR_ARRAY_INSERT || eop > WR_ARRAY_DELETE || A.ops[k].client != q.client) { flags = WF_CHAIN; break; }
        chain[nc++] = k;
        below = k;
        k = links[k].prev_list;
      }
      if (flags) break;
      if (k != WRITE_NONE) { flags = WF_CHAIN; break; }
      for (uint32_t i = 0; i < nc / 2; ++i) { const uint32_t t = chain[i]; chain[i] = chain[nc - 1 - i]; chain[nc - 1 - i] = t; }
    }
    uint32_t x0 = 0, x1 = 0;
    if (!fresh) {
      const uint32_t lo = lower_bound_u64(a.gk, a.ck, g), hi = upper_bound_u64(a.gk, a.ck, g);
      const uint32_t kp = first_list(a, lo, hi);
      if (kp != VNONE && !list_range(a, kp, x0, x1)) { flags = RF_OPEN; break; }
    }
    write_list_plan(DevList{A, x0, x1}, A.ops, chain, nc, q, p, why, flags);
  } while (false);
  if (flags) { p.kind = 0; p.nr = 0; }
  if (p.kind == 1) size = item_update_size(item_of(a, q, p));
  else if (p.kind == 2) size = ds_update_size(p.r, p.nr);
  if (size > 0xFFFFFFF0ull) { flags |= RF_SIZE; size = 0; p.kind = 0; }
  A.plan[r] = p;
  A.size[r] = (uint32_t)size;
  A.why[r] = flags ? WHY_OK : why;
  A.flags[r] = flags;
}

__global__ void k_wwrite(WriteArgs A) {
  const JsonArgs& a = A.j;
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= A.nops || A.flags[r]) return;
  const uint64_t at = A.offs[r], size = A.offs[r + 1] - at;
  if (!size || at + size > a.out_cap) return;
  const WritePlan p = A.plan[r];
  const WriteReq q = A.ops[r];
  if (q.root >= a.nreq) return;
  if (p.kind == 1) item_update_write(a.out + at, size, item_of(a, q, p));
  else if (p.kind == 2) ds_update_write(a.out + at, size, p.r, p.nr);
}

inline dim3 grid(uint64_t n) { return dim3((uint32_t)(n / 256 + 1)); }

}  // namespace

void launch_write_plan(const WriteArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_wplan, grid((uint64_t)a.nops + 1), dim3(256), 0, s, a); }
void launch_transact_plan(const WriteArgs& a, const WriteLink* links, hipStream_t s) {
  hipLaunchKernelGGL(k_tplan, grid((uint64_t)a.nops + 1), dim3(256), 0, s, a, links);
}
void launch_write_write(const WriteArgs& a, hipStream_t s) { hipLaunchKernelGGL(k_wwrite, grid(a.nops), dim3(256), 0, s, a); }

}  // namespace yc
