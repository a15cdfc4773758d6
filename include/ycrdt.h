/* ycrdt.h — C ABI of the MI355X-native batched Yjs merge engine (libycrdt.so).
 *
 * This is the drop-in boundary for the path @ypear/crdt delegates to Yjs. The reference injects
 * its CRDT engine through `router.options.Y` (reference crdt.js:175-180) and only ever calls the
 * entry points listed below; each function cites the reference call sites it replaces. A Node
 * N-API addon (crdt_amd/js) and a Python ctypes mirror (crdt_amd/__init__.py) are the callers.
 *
 * Conventions
 *  - Inputs are borrowed for the duration of the call and copied (to HBM) before it returns.
 *  - Outputs (ycrdt_out) are library-owned until ycrdt_free().
 *  - Every function returns YCRDT_OK (0) or a negative YCRDT_E_* code; ycrdt_last_error() gives
 *    the message (thread-local). Decode errors are atomic: the doc is unchanged (Yjs decodes the
 *    whole struct section before integrating, Y@21330).
 *  - Output byte order is Yjs 13.6 canonical (delete-set / state-vector clients sorted
 *    descending); see DESIGN.md §Compat for the 13.5.16 insertion-order difference.
 *  - There is no CPU fallback: without a usable HIP device every compute entry point fails
 *    with YCRDT_E_DEVICE.
 *  - Threads: calls on one engine are serialised by the caller, with one exception — a batch may
 *    be created (ycrdt_batch_stage*: host packing + H2D on the engine's copy stream) by one thread
 *    while another thread merges a different batch or reads its result (the serving loop:
 *    batch k+1 staged beside batch k's merge).
 */
#ifndef YCRDT_H
#define YCRDT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ycrdt_engine ycrdt_engine;
typedef struct ycrdt_doc ycrdt_doc;
typedef struct ycrdt_batch ycrdt_batch;
typedef struct ycrdt_comm ycrdt_comm; /* RCCL communicator (multi-GPU exchanges) */
#define YCRDT_COMM_ID_BYTES 128

typedef struct { const uint8_t *ptr; size_t len; } ycrdt_buf; /* borrowed */
typedef struct { uint8_t *ptr; size_t len; } ycrdt_out;       /* library-owned */

enum {
  YCRDT_OK = 0,
  YCRDT_E_DECODE = -1,      /* malformed update (Yjs: Error('Integer out of range!')) */
  YCRDT_E_PENDING = -2,     /* internal: missing dependencies seen by a merge that must have none */
  YCRDT_E_UNSUPPORTED = -3, /* valid Yjs input outside the engine's coverage */
  YCRDT_E_CAPACITY = -4,
  YCRDT_E_DEVICE = -5,      /* no HIP device / HIP runtime error */
  YCRDT_E_ARG = -6,
};

typedef struct {
  uint64_t in_bytes;        /* bytes of all input updates */
  uint64_t items;           /* Σ struct clock lengths of the inputs (Item + GC, Skip excluded) */
  uint64_t structs;         /* decoded structs */
  uint64_t units;           /* distinct (client, clock) units in the merged store */
  uint64_t segments;        /* split-point segments */
  uint64_t out_structs;     /* structs in the encoded state */
  uint64_t out_bytes;       /* encoded update bytes */
  uint64_t clients;
  double device_ms;         /* device time of the merge (events on the engine stream) */
} ycrdt_merge_stats;

/* ---- engine ------------------------------------------------------------------------------ */
/* device: HIP device ordinal. compat: 136 (default, Yjs 13.6 order) */
int ycrdt_engine_create(int device, int compat, ycrdt_engine **out);
void ycrdt_engine_destroy(ycrdt_engine *e);
/* optional per-phase device timing (hipEvents on the engine stream) */
int ycrdt_engine_set_profiling(ycrdt_engine *e, int on);
/* fills up to `cap` (name, milliseconds) pairs of the last merge; returns the count */
int ycrdt_engine_phase_times(ycrdt_engine *e, const char **names, double *ms, int cap);
/* HBM the engine holds: its grow-only merge workspace, the doc-state arena and the staging batch */
int ycrdt_engine_device_bytes(ycrdt_engine *e, uint64_t *bytes);
/* Releases the engine's merge workspace (grow-only HBM buffers) and every doc's spare state block
 * (a folded merge keeps the previous state's block for the next one; doc states and batches stay):
 * after a giant merge, e.g. the >= 1 B-item replay of crdt.js:79-98, a server gets its HBM back.
 * The next merge allocates what it needs again. */
int ycrdt_engine_trim(ycrdt_engine *e);

/* ---- Y.Doc ------------------------------------------------------------------------------- */
/* new Y.Doc()  (crdt.js:33,54,56,80,221) */
int ycrdt_doc_create(ycrdt_engine *e, uint32_t client_id, ycrdt_doc **out);
void ycrdt_doc_destroy(ycrdt_doc *d);
/* Y.applyUpdate(doc, u8)  (crdt.js:35,56,58,85,294). Yjs semantics, including missing
 * dependencies: structs whose dependencies are unknown are parked (Yjs store.pendingStructs /
 * pendingDs, readUpdateV2 Y@21330), retried when a later update supplies them, and emitted by
 * ycrdt_encode_state_as_update exactly as Yjs does. The update is validated now (a malformed one
 * fails with YCRDT_E_DECODE: the doc is unchanged if the struct section is malformed; a malformed
 * delete set keeps the structs and the ranges read before the error, as in Yjs); the merge itself
 * is DEFERRED to the next read of the doc (encode*, json, map_type_at, a local op, flush), so a
 * burst of n applies costs one batched merge (crdt.js:294 onData bursts, crdt.js:79-98 replay). */
int ycrdt_apply_update(ycrdt_doc *d, ycrdt_buf update);
/* n sequential Y.applyUpdate calls (LevelDB replay crdt.js:79-98, ingest); stops at the first
 * malformed update, as a loop of Y.applyUpdate would. */
int ycrdt_apply_updates(ycrdt_doc *d, const ycrdt_buf *ups, size_t n);
/* Fleet ingest (crdt.js:235 one doc per topic, crdt.js:294 onData per message):
 * Y.applyUpdate(docs[i], ups[i]) for i = 0..n-1, validated as ycrdt_apply_updates, then merged in
 * this call — ONE device pass for every document that has nothing pending (multi-document batch,
 * results split back into each document's HBM state on the device). Documents with pending
 * structs / delete ranges, or an engine with compat 135, take their own flush. All documents must
 * belong to `e`. A malformed update i: updates before it are applied (and merged), then
 * YCRDT_E_DECODE. */
int ycrdt_apply_updates_multi(ycrdt_engine *e, ycrdt_doc *const *docs, const ycrdt_buf *ups, size_t n);
/* Y.encodeStateAsUpdate + Y.encodeStateVector of n documents in one call (a fleet's LevelDB
 * snapshot / sync answers, crdt.js:33-40,260,288): deferred applies are flushed as one batched merge
 * and the states gathered on the device, then copied with one pipelined D2H. Document i's update
 * is dst[offs[2i] .. offs[2i+1]), its state vector dst[offs[2i+1] .. offs[2i+2]); offs holds 2n+1
 * entries. dst == NULL only fills offs / total (size query). */
int ycrdt_docs_states_packed(ycrdt_engine *e, ycrdt_doc *const *docs, size_t n, uint8_t *dst, uint64_t cap, uint64_t *offs,
                             uint64_t *total);
/* Sync replies for many (document, peer state vector) pairs in one device pass: the responder of
 * crdt.js:286-291 (`Y.encodeStateAsUpdate(y.doc, d.stateVector)` per joining or lagging peer)
 * batched over peers and topics. Reply i = blob[offs[i] .. offs[i+1]) is byte-identical to
 * ycrdt_encode_state_as_update(docs[i], svs[i]); offs holds n+1 entries; blob is released with
 * ycrdt_free. svs[i].len == 0 means the full state. A doc may appear any number of times.
 * A reply is planned from the document's resident state (which client blocks the peer lacks, which
 * struct its clock cuts) and assembled from ranges of that state: no decode, no merge, no host
 * round trip of the state (Sync replies). Documents with pending structs or a pending
 * delete set, engines with compat 135, mark-less states over walk_max bytes and cuts the slice
 * helper refuses take ycrdt_encode_state_as_update one by one (error included); YCRDT_SYNC=0 sends
 * every pair there. Queued applies are flushed first (one batched merge). A state vector that does
 * not parse fails the whole call with YCRDT_E_DECODE and no output. n == 0 needs no device. */
typedef struct {
  uint64_t pairs_marks;   /* answered from the doc's marks */
  uint64_t pairs_walk;    /* mark-less state walked on the device */
  uint64_t pairs_single;  /* went through ycrdt_encode_state_as_update, one by one */
  uint64_t cut_structs;   /* structs re-encoded at an offset > 0 */
  uint64_t out_bytes;
  uint32_t walk_max;      /* largest mark-less state (bytes) the walk path takes */
  double device_ms;
} ycrdt_sync_stats;
int ycrdt_docs_diff(ycrdt_engine *e, ycrdt_doc *const *docs, const ycrdt_buf *svs, size_t n,
                    ycrdt_out *blob, uint64_t *offs, ycrdt_sync_stats *st /* may be NULL */);
/* Root toJSON for many (document, root, kind) requests in one device pass: the `c[key] =
 * h[key].toJSON()` refresh of crdt.js:297-305 batched over documents. Request i = blob[offs[i] ..
 * offs[i+1]) is byte-identical to ycrdt_doc_json(docs[i], roots[i], kinds[i]) (kind 0 = map, 1 =
 * array; a kind that does not match the root, or an absent root, gives {} / []); offs holds n+1
 * entries; blob is released with ycrdt_free. A document may repeat, and so may a triple (it is
 * computed once). The distinct documents' resident states are merged as ONE multi-document batch,
 * the view kernels run over it, and the JSON text is sized, laid out and written on the device
 * (Fleet toJSON): the host sees neither the state bytes nor the view records. Empty
 * documents are answered inline. Documents with pending structs or a pending delete set, engines
 * with compat 135, and whatever the device path's bounds refuse (shared types nested more than
 * depth_max levels below the root, a map-entry name over name_max bytes, an `any` value nested
 * past 64 levels, malformed content) take ycrdt_doc_json one by one (error included);
 * YCRDT_DOCS_JSON=0 sends every request there. Queued applies are flushed first (one batched
 * merge). pairs_device + pairs_single + pairs_empty == n. n == 0 needs no device. A null root, a
 * kind outside {0, 1} or a document of another engine gives YCRDT_E_ARG and no output. */
typedef struct {
  uint64_t pairs_device;  /* text written on the device */
  uint64_t pairs_single;  /* went through ycrdt_doc_json, one by one */
  uint64_t pairs_empty;   /* empty document: "{}" / "[]", no device work */
  uint64_t out_bytes;
  uint32_t depth_max;     /* nested-type levels the device path takes (constant) */
  uint32_t name_max;      /* longest map-entry name (bytes) the device ordering takes (constant) */
  double device_ms;       /* view and JSON kernels of the passes (the merge before them not included) */
} ycrdt_json_stats;
int ycrdt_docs_json(ycrdt_engine *e, ycrdt_doc *const *docs, const char *const *roots, const int *kinds,
                    size_t n, ycrdt_out *blob, uint64_t *offs, ycrdt_json_stats *st /* may be NULL */);
/* The cache refresh for many documents in one device pass: the loop of crdt.js:201-216 / 297-305,
 *   for (const [key, val] of Object.entries(ix.toJSON())) c[key] = (val == 'map' ? doc.getMap(key) : doc.getArray(key)).toJSON()
 * batched over documents, with every document's index map read on the device. Document i =
 * blob[offs[i] .. offs[i+1]) is the text of its `c`: one JSON object with one member for every live
 * entry of root map `index` (NULL: "ix"), an entry whose value is `undefined` included, in the member
 * order of ycrdt_doc_json(doc, index, 0); each member is the entry's name, escaped as map entry
 * names are, `:` and exactly ycrdt_doc_json(doc, name, kind), kind 0 iff the entry's value == 'map'
 * in JavaScript's loose sense (the string, or one-element arrays around it), else 1. No index root,
 * no live entry or an empty document give {}. offs holds n+1 entries; blob is released with
 * ycrdt_free. A document may repeat (it is computed once). One (document, index, map) request per
 * document goes through the fleet toJSON front half; the requests for the listed roots are derived
 * on the device from the sorted view keys. Empty documents are answered inline.
 * Documents with pending structs or a pending delete set, engines with compat 135, and documents
 * the device flags (an index name over name_max bytes, a listed root the toJSON bounds refuse, two
 * root names in one hash slot) are composed on the host from the same definitions, byte for byte;
 * YCRDT_DOCS_CACHE=0 sends every document there. Queued applies are flushed first.
 * docs_device + docs_single + docs_empty == n. n == 0 needs no device. A document of another
 * engine gives YCRDT_E_ARG and no output. */
typedef struct {
  uint64_t docs_device;   /* text written on the device */
  uint64_t docs_single;   /* composed on the host, one by one */
  uint64_t docs_empty;    /* empty document: "{}", no device work */
  uint64_t roots;         /* members written on the device */
  uint64_t out_bytes;
  uint32_t depth_max;     /* nested-type levels the device path takes (constant) */
  uint32_t name_max;      /* longest index or map-entry name (bytes) the device ordering takes (constant) */
  double device_ms;       /* view, JSON and cache kernels of the passes (the merge before them not included) */
} ycrdt_cache_stats;
int ycrdt_docs_cache(ycrdt_engine *e, ycrdt_doc *const *docs, size_t n, const char *index /* NULL: "ix" */,
                     ycrdt_out *blob, uint64_t *offs /* n+1 */, ycrdt_cache_stats *st /* may be NULL */);
/* Point reads for many documents in one device pass: the `h[name].has(key)` / `.get(key)` /
 * `.length` reads of crdt.js:423-430 batched over documents. Read i gives exactly what the single
 * call gives for the same arguments. MAP_GET / ARRAY_GET: states[i] is ycrdt_map_get's /
 * ycrdt_array_get's state (0 absent, 1 present, 2 `undefined`), blob[offs[i] .. offs[i+1]) its json
 * byte for byte (empty for states 0 and 2), counts[i] 0; a value that is a shared type is that
 * type's toJSON. MAP_SIZE / ARRAY_LENGTH: counts[i] is ycrdt_map_size's / ycrdt_array_length's
 * answer, states[i] 1, the blob range empty. parent_key NULL addresses the root type `root`, else
 * the type stored in root map `root` under it (a type that does not exist, or of the other kind,
 * reads as empty). offs holds n+1 entries; blob is released with ycrdt_free. A document may repeat,
 * and so may a read (it is computed once). The pass is the fleet toJSON pass up to its sizing
 * sweeps, then one lane per read: the entry found by binary search in the sorted view keys, the
 * element in a scan of the visible lengths, the value written by the shared value writer (DESIGN.md
 * §5.2e). Empty documents are answered inline. Documents with pending structs or a pending delete
 * set, engines with compat 135, a key or parent_key over name_max bytes, a container holding an
 * entry name over name_max bytes that shares its first name_max bytes with the request, and values
 * the writer's bounds refuse (nested past depth_max, an `any` past 64 levels, malformed content)
 * take the single call one by one (its error included); YCRDT_DOCS_READ=0 sends every read there.
 * Queued applies are flushed first (one batched merge). reads_device + reads_single + reads_empty
 * == n. n == 0 needs no device. A null doc or root, a null key for MAP_GET, an op outside the four
 * or a document of another engine gives YCRDT_E_ARG and no output. */
enum { YCRDT_READ_MAP_GET = 0, YCRDT_READ_MAP_SIZE = 1, YCRDT_READ_ARRAY_GET = 2, YCRDT_READ_ARRAY_LENGTH = 3 };
typedef struct {
  ycrdt_doc *doc;
  const char *root;
  const char *parent_key; /* NULL: the root type; else the type stored in root map `root` under it */
  const char *key;        /* MAP_GET */
  uint64_t index;         /* ARRAY_GET */
  int op;                 /* YCRDT_READ_* */
} ycrdt_read;
typedef struct {
  uint64_t reads_device;  /* answered on the device */
  uint64_t reads_single;  /* went through the single call, one by one */
  uint64_t reads_empty;   /* empty document: state 0 / count 0, no device work */
  uint64_t out_bytes;
  uint32_t depth_max;     /* nested-type levels the device path takes (constant) */
  uint32_t name_max;      /* longest entry name (bytes) the device search takes (constant) */
  double device_ms;       /* view and read kernels of the passes (the merge before them not included) */
} ycrdt_read_stats;
int ycrdt_docs_read(ycrdt_engine *e, const ycrdt_read *reads, size_t n, ycrdt_out *blob, uint64_t *offs,
                    int32_t *states, uint64_t *counts, ycrdt_read_stats *st /* may be NULL */);
/* Local ops for many documents in one device pass: the `set` / `del` / `push` / `insert` / `cut` of
 * crdt.js:423-611 batched over documents. Op i gives exactly what the single call of its kind gives
 * for the same arguments: blob[offs[i] .. offs[i+1]) is the update that call would have enqueued,
 * byte for byte — empty where it writes nothing: a delete of an absent or deleted entry, count == 0,
 * length == 0, a failed op that deleted nothing — and codes[i] is what it would have returned.
 * YCRDT_E_ARG stands for "Length exceeded!", "no shared type at ...", a type mismatch, a null key or
 * a bad `any` value; an ARRAY_DELETE that runs past the end deletes what exists (a non-empty update)
 * and has code YCRDT_E_ARG, as ycrdt_array_delete. ARRAY_PUSH is ARRAY_INSERT at the list's visible
 * length (YArray.push without a read of the length first). Every non-empty update is enqueued as a
 * local transaction, as the single calls enqueue theirs (ycrdt_doc_take_local_update sees it). The
 * last failed op leaves its message in ycrdt_last_error. offs holds n+1 entries; blob is released
 * with ycrdt_free. A document may repeat: its ops run in the call's order.
 * The pass is the fleet read pass up to its visible-length scan, then one lane per op: the entry by
 * binary search in the sorted view keys, the element at index - 1 in the scan of the visible
 * lengths, the bytes by the writers of yc_write.h. The path is chosen per
 * document. Empty documents run the single calls (ops_empty). The single calls, in order, also run
 * (ops_single) the ops of documents with pending structs or a pending delete set, of engines with
 * compat 135, with a key or parent_key over name_max bytes, whose ops in this call are not
 * independent of one another (two name one map entry or one list, or one writes the root-map entry
 * another's parent_key names), with an op the device flags (the reads' refusals; an ARRAY_DELETE
 * over more than ranges_max visible segments), or with a failed op that is not the document's last;
 * YCRDT_DOCS_WRITE=0 sends every op there (under it, and under compat 135, an empty document's ops
 * count as ops_single too). ops_device + ops_single + ops_empty == n; ops_noop counts
 * the ops with code 0 and an empty update. Queued applies are flushed first (one batched merge).
 * n == 0 needs no device. The call itself fails only with YCRDT_E_ARG for a null pointer, a null
 * doc or root, an op outside the six or a document of another engine — checked before anything is
 * enqueued — and with what is no per-op result (YCRDT_E_DEVICE). */
enum { YCRDT_WRITE_MAP_SET = 0, YCRDT_WRITE_MAP_SET_TYPE = 1, YCRDT_WRITE_MAP_DELETE = 2,
       YCRDT_WRITE_ARRAY_INSERT = 3, YCRDT_WRITE_ARRAY_PUSH = 4, YCRDT_WRITE_ARRAY_DELETE = 5 };
typedef struct {
  ycrdt_doc *doc;
  const char *root;
  const char *parent_key; /* NULL: the root type; else the type stored in root map `root` under it */
  const char *key;        /* the map ops */
  const uint8_t *any;     /* MAP_SET: one value; ARRAY_INSERT / ARRAY_PUSH: count values */
  size_t any_len;
  uint32_t count;
  uint32_t type_ref;      /* MAP_SET_TYPE: 0 = YArray, 1 = YMap */
  uint32_t index;         /* ARRAY_INSERT, ARRAY_DELETE */
  uint32_t length;        /* ARRAY_DELETE */
  int op;                 /* YCRDT_WRITE_* */
} ycrdt_write;
typedef struct {
  uint64_t ops_device;    /* encoded on the device */
  uint64_t ops_single;    /* went through the single calls, in order */
  uint64_t ops_empty;     /* empty document: the single calls, no device work */
  uint64_t ops_noop;      /* code 0 and an empty update (whatever the path) */
  uint64_t out_bytes;
  uint32_t ranges_max;    /* visible segments one ARRAY_DELETE may touch on the device (constant) */
  uint32_t name_max;      /* longest key / parent_key (bytes) the device search takes (constant) */
  double device_ms;       /* view, sort, sizing and write kernels of the passes (the merge before them not included) */
} ycrdt_write_stats;
int ycrdt_docs_write(ycrdt_engine *e, const ycrdt_write *ops, size_t n, ycrdt_out *blob, uint64_t *offs /* n + 1 */,
                     int32_t *codes /* n */, ycrdt_write_stats *st /* may be NULL */);
/* ycrdt_docs_write for a queue of ops that depend on one another, as crdt.js:329-355 (execBatch)
 * runs one per document: op i's update is byte for byte the one the single call of its kind would
 * have enqueued had the call's earlier ops on that document already run, codes[i] that call's
 * result. The op struct, the updates' enqueueing in call order, the argument errors, ops_noop,
 * ops_empty and n == 0 are those of ycrdt_docs_write; the difference is only which documents stay
 * on the device. Two ops of one map entry, of one list, or a MAP_SET_TYPE and the ops under its key
 * (crdt.js:422-431: `new Y.Array()` under a fresh key, then a push into it) no longer send their
 * document to the single calls: the host finds, per op, the previous op on its entry, on its list
 * and the op that made its container, and one lane per op replays the earlier ops of its chain over
 * a small piece table. ops_chained counts the device ops planned through an
 * earlier op of the call. Still single (ops_single), per document: what ycrdt_docs_write sends
 * there for reasons other than dependence (pending structs or delete set, compat 135, a state of
 * 2 GiB, a name over name_max, an op the device flags), more than chain_max ops of the call on one
 * list or one map entry, and a failed op that is not the document's last (the clocks behind it were
 * handed out as if it took its own). YCRDT_DOCS_TRANSACT=0 sends every op to the single calls. */
typedef struct {
  uint64_t ops_device, ops_single, ops_empty, ops_noop;  /* as ycrdt_write_stats */
  uint64_t ops_chained;   /* device ops planned through an earlier op of the same call */
  uint64_t out_bytes;
  uint32_t ranges_max, name_max;
  uint32_t chain_max;     /* ops of one call on one container chain the device takes (constant) */
  double device_ms;
} ycrdt_transact_stats;
int ycrdt_docs_transact(ycrdt_engine *e, const ycrdt_write *ops, size_t n, ycrdt_out *blob, uint64_t *offs /* n + 1 */,
                        int32_t *codes /* n */, ycrdt_transact_stats *st /* may be NULL */);
/* Runs the deferred applies now (every read does this implicitly). */
int ycrdt_doc_flush(ycrdt_doc *d);
/* Whether Yjs would hold pending structs (store.pendingStructs) / a pending delete set
 * (store.pendingDs) for this doc. */
int ycrdt_doc_pending(ycrdt_doc *d, int *structs, int *delete_set);
/* Y.encodeStateAsUpdate(doc[, sv])  (crdt.js:56,260,288,347,383,443,471,505,533,560,585,611);
 * sv.len == 0 ⇒ full state */
int ycrdt_encode_state_as_update(ycrdt_doc *d, ycrdt_buf sv, ycrdt_out *out);
/* Y.encodeStateVector(doc)  (crdt.js:59,239,258,289) */
int ycrdt_encode_state_vector(ycrdt_doc *d, ycrdt_out *out);
/* stats of the doc's last merge */
int ycrdt_doc_last_stats(ycrdt_doc *d, ycrdt_merge_stats *st);

/* Y.mergeUpdates(updates) — north_star; Yjs-internal for pending structs (Y@39011). Lazy k-way
 * merge of the updates' structs (no integration), delete sets unioned. One input is returned
 * unchanged, as Yjs does. */
int ycrdt_merge_updates(ycrdt_engine *e, const ycrdt_buf *ups, size_t n, ycrdt_out *out);
/* Y.diffUpdate(update, sv) (Y@40711): the structs of `update` missing from state vector `sv`,
 * with the update's delete set. */
int ycrdt_diff_update(ycrdt_engine *e, ycrdt_buf update, ycrdt_buf sv, ycrdt_out *out);
/* n independent Y.diffUpdate(updates[i], svs[i]) in ONE batched device pass: the sync responder
 * of crdt.js:286-291 (`Y.encodeStateAsUpdate(doc, peerStateVector)` per joining peer) batched
 * across peers and topics. outs[i] is byte-identical to
 * ycrdt_diff_update(updates[i], svs[i]); each must be released with ycrdt_free. A malformed
 * update or state vector fails the whole batch (no output is produced). */
int ycrdt_diff_updates(ycrdt_engine *e, const ycrdt_buf *updates, const ycrdt_buf *svs, size_t n, ycrdt_out *outs);

/* ---- the doc-less update store ------------------------------------------------------------
 * A persistence worker that keeps every topic as update bytes and never builds a Y.Doc (the Yjs
 * update API: mergeUpdates / encodeStateVectorFromUpdate / diffUpdate). crdt.js does this work with
 * throw-away docs: storeUpdate (crdt.js:28-77) builds two temporary docs, applies twice and encodes
 * a state vector for every stored message; getYDoc (crdt.js:79-98) replays a log that is never
 * compacted. */
typedef struct {
  uint64_t groups_device;  /* answered in the batched device pass */
  uint64_t groups_single;  /* went through the single call, one by one */
  uint64_t groups_copied;  /* 0 or 1 update: answered on the host (1 update = returned unchanged, as Yjs) */
  uint64_t out_bytes;
  double device_ms;
} ycrdt_store_stats;
/* Y.mergeUpdates per group, many groups in ONE device pass: compacting the logs of many topics at
 * once (the log getYDoc replays, crdt.js:79-98, is never compacted; storeUpdate, crdt.js:28-77,
 * merges per message through two temporary docs). Update i belongs to group group_of[i] < ngroups;
 * groups may interleave in the input, and a group's updates keep their input order (the reader
 * order Yjs sees: it decides the ties). Group g's result = blob[offs[g] .. offs[g+1]), byte-identical
 * to ycrdt_merge_updates over that group's updates; offs holds ngroups+1 entries; blob is released
 * with ycrdt_free. A group with no update gives the empty update (00 00, what ycrdt_merge_updates
 * gives for n == 0); a group of one update is returned unchanged, as Yjs does, even when that
 * update is not canonical (both: groups_copied). The other groups are staged as one multi-document
 * batch and merged in one pass — sizes, offsets and the per-group varuint headers computed and
 * written on the device, one copy back — except those that take
 * ycrdt_merge_updates one by one (groups_single; its error, if any, is returned): a group holding
 * an update whose sections are not in strictly descending client order, a group of more than 1024
 * updates, every group of an engine with compat 135, and every group when YCRDT_STORE=0 is set.
 * groups_device + groups_single + groups_copied == ngroups. group_of[i] >= ngroups gives
 * YCRDT_E_ARG; a malformed update fails the whole call with YCRDT_E_DECODE and no output; more than
 * 4 GiB staged at once is YCRDT_E_CAPACITY. ngroups == 0 needs no device. */
int ycrdt_merge_updates_groups(ycrdt_engine *e, const ycrdt_buf *ups, const uint32_t *group_of, size_t n,
                               uint32_t ngroups, ycrdt_out *blob, uint64_t *offs,
                               ycrdt_store_stats *st /* may be NULL */);
/* Y.encodeStateVectorFromUpdate(ups[i]) for n updates in ONE device pass: what a store holds of
 * every topic, refreshed after a write (the `Y.encodeStateVector(tempDoc)` of crdt.js:28-77 without
 * the doc). blob[offs[i] .. offs[i+1]) is Yjs's result for ups[i]; offs holds n+1 entries; blob is
 * released with ycrdt_free. As in Yjs the pairs keep the update's own client order (not re-sorted),
 * a client counts up to its first Skip and only when its first struct starts at clock 0,
 * neighbouring sections of one client count as one, the delete set is not read, and the result is
 * the same under compat 135 and 136; the empty update (00 00) gives 00. A malformed update fails
 * the whole call with YCRDT_E_DECODE and no output. n == 0 needs no device. The stats' groups_*
 * count updates (all of them groups_device). */
int ycrdt_updates_state_vectors(ycrdt_engine *e, const ycrdt_buf *ups, size_t n, ycrdt_out *blob, uint64_t *offs,
                                ycrdt_store_stats *st /* may be NULL */);
/* the single-call form: Y.encodeStateVectorFromUpdate(update) */
int ycrdt_update_state_vector(ycrdt_engine *e, ycrdt_buf update, ycrdt_out *out);

/* ---- crdt.c materialisation and local ops ------------------------------------------------
 * A "target" is root type `root`, or (parent_key != NULL) the shared type stored in root YMap
 * `root` under `parent_key` (crdt.js nests one YArray per map key, crdt.js:423-430).
 * The device computes map winners and list order (a view of the merged state); the host
 * decodes values and writes each local op as a one-struct Yjs v1 update, applied like a remote
 * one, so the doc's bytes match a Yjs doc that performed the same ops. */
/* YMap.toJSON / YArray.toJSON of a root (kind 0 = map, 1 = array) as JSON.stringify text
 * (crdt.js:202,214,304,372,494,528,555,581,607; YMap.toJSON Y@51558, typeListToArray Y@46408) */
int ycrdt_doc_json(ycrdt_doc *d, const char *root, int kind, ycrdt_out *out);
/* toJSON of the shared type at a target (parent_key == NULL: root type `root`; else the YMap
 * (kind 0) / YArray (kind 1) stored in root map `root` under parent_key — crdt.js:423-430 nests one
 * YArray per key): reads that type's own list only. A key holding no such type gives {} / []. */
int ycrdt_type_json(ycrdt_doc *d, const char *root, const char *parent_key, int kind, ycrdt_out *out);
/* The live entries of a YMap target with the id of each entry's winning item, as JSON text
 * {"key": ["client:clock", value], ...} — what YMap.observe's keysChanged (Y@51190) is computed
 * from: a key changed iff its winning item changed (crdt.js:620-657 observers). */
int ycrdt_map_entries(ycrdt_doc *d, const char *root, const char *parent_key, ycrdt_out *out);
/* YMap.get(key) of root map `root`: *type_ref = the type ref (0 YArray, 1 YMap, ...) when the
 * key holds a live shared type, else -1 (a plain value or nothing)  (crdt.js:423-424) */
int ycrdt_map_type_at(ycrdt_doc *d, const char *root, const char *key, int32_t *type_ref);
/* YMap.set(key, value) with a lib0 `any` value (crdt.js:375,434; typeMapSet Y@49334) */
int ycrdt_map_set(ycrdt_doc *d, const char *root, const char *parent_key, const char *key, const uint8_t *any,
                  size_t anylen);
/* YMap.set(key, new Y.Array()) (type_ref 0) / new Y.Map() (1)  (crdt.js:423) */
int ycrdt_map_set_type(ycrdt_doc *d, const char *root, const char *parent_key, const char *key, uint32_t type_ref);
/* YMap.delete(key)  (crdt.js:465; typeMapDelete Y@49261) */
int ycrdt_map_delete(ycrdt_doc *d, const char *root, const char *parent_key, const char *key);
/* YArray.insert(index, values) / push / unshift with `count` concatenated lib0 `any` values
 * (crdt.js:426-428,527,554,580; typeListInsertGenerics Y@48365). "Length exceeded!" past the end. */
int ycrdt_array_insert(ycrdt_doc *d, const char *root, const char *parent_key, uint32_t index, const uint8_t *anys,
                       size_t len, uint32_t count);
/* YArray.delete(index, length)  (crdt.js:429,606; typeListDelete Y@48835). Like Yjs, deletes
 * what exists and then fails with "Length exceeded!" when the range runs past the end. */
int ycrdt_array_delete(ycrdt_doc *d, const char *root, const char *parent_key, uint32_t index, uint32_t length);
/* doc.clientID */
int ycrdt_doc_client_id(ycrdt_doc *d, uint32_t *out);
/* Per-key reads of the materialised view, replacing a full toJSON per call (facade YMap.get / has /
 * size, YArray.length / get; crdt.js:423-424 `h[name].has(key)` / `.get(key)`, push's length):
 * state 0 = absent, 1 = present (`json` = JSON text of the value), 2 = present, value `undefined`.
 * `json` is always allocated (free with ycrdt_free). A nested target whose type does not exist
 * reads as empty. */
int ycrdt_map_get(ycrdt_doc *d, const char *root, const char *parent_key, const char *key, int *state, ycrdt_out *json);
int ycrdt_map_size(ycrdt_doc *d, const char *root, const char *parent_key, uint32_t *size);
int ycrdt_array_length(ycrdt_doc *d, const char *root, const char *parent_key, uint64_t *length);
int ycrdt_array_get(ycrdt_doc *d, const char *root, const char *parent_key, uint64_t index, int *state, ycrdt_out *json);
/* Incremental local-op encode: the updates of the local ops
 * (ycrdt_map_* / ycrdt_array_*) applied since the previous call, as ONE update (Y.mergeUpdates of
 * them; a single op's own update is returned as is; none = the empty update). crdt.js broadcasts
 * Y.encodeStateAsUpdate(doc) after every local op (crdt.js:347,383,443,471,505,533,560,585,611);
 * this delta is wire-compatible (Y.applyUpdate accepts it) but changes the bytes on the wire, so a
 * host opts in. Remote updates applied in between are not part of it. */
int ycrdt_doc_take_local_update(ycrdt_doc *d, ycrdt_out *out);
/* Starts (on != 0) or stops recording local-op updates for ycrdt_doc_take_local_update. Off by
 * default; the first take turns it on. A long untaken list is folded into one update. */
int ycrdt_doc_track_local(ycrdt_doc *d, int on);

/* ---- device-resident batches (ingest queue / benchmark) ---------------------------------- */
/* Copies the updates into HBM. */
int ycrdt_batch_stage(ycrdt_engine *e, const ycrdt_buf *ups, size_t n, ycrdt_batch **out);
/* Merges the staged updates into a fresh doc entirely on the device; the encoded state stays in
 * HBM. Equivalent to applying every update to a new Y.Doc and encodeStateAsUpdate(doc). */
int ycrdt_batch_merge(ycrdt_batch *b, ycrdt_merge_stats *st);
/* Copies the merge result (encoded update and state vector) to the host. The result lives in the
 * engine workspace: any other engine call in between makes this fail with YCRDT_E_ARG. */
int ycrdt_batch_result(ycrdt_batch *b, ycrdt_out *update, ycrdt_out *state_vector);
void ycrdt_batch_destroy(ycrdt_batch *b);
/* Multi-document batches (C5 fleets: one Y.Doc per topic, crdt.js:235; and many independent replica
 * sets per device pass): update i belongs to document doc_of[i] < ndocs. One device pass merges
 * every document on its own (clients, lists and delete sets never mix across documents); the
 * result of document d equals merging its updates alone. */
int ycrdt_batch_stage_docs(ycrdt_engine *e, const ycrdt_buf *ups, const uint32_t *doc_of, size_t n, uint32_t ndocs,
                           ycrdt_batch **out);
/* updates[ndocs] (and state_vectors[ndocs] unless NULL) receive every document's encoded state */
int ycrdt_batch_result_docs(ycrdt_batch *b, ycrdt_out *updates, ycrdt_out *state_vectors);
/* The same results packed back to back in caller memory, split per document on the device (one
 * HBM buffer, one pipelined D2H through pinned staging; no per-document allocation): document d's
 * encodeStateAsUpdate is dst[offs[2d] .. offs[2d+1]) and its encodeStateVector dst[offs[2d+1] ..
 * offs[2d+2]); offs holds 2*ndocs+1 entries, *total = offs[2*ndocs]. dst == NULL only fills offs /
 * total (size query); cap < total is YCRDT_E_ARG. A sync responder / LevelDB writer hands the
 * slices on as they are (crdt.js:260,288 send Y.encodeStateAsUpdate bytes; crdt.js:79-98 store). */
int ycrdt_batch_result_docs_packed(ycrdt_batch *b, uint8_t *dst, uint64_t cap, uint64_t *offs, uint64_t *total);
/* one-shot form of the two above (host buffers in and out) */
int ycrdt_merge_docs(ycrdt_engine *e, const ycrdt_buf *ups, const uint32_t *doc_of, size_t n, uint32_t ndocs,
                     ycrdt_out *updates, ycrdt_out *state_vectors);

/* ---- host-only entry points (no HIP device needed) ---------------------------------------- */
/* The validation Y.applyUpdate runs before queueing an update: YCRDT_OK, or YCRDT_E_DECODE with
 * *structs_ok = 1 when only the delete set is malformed (Yjs then keeps the structs). */
int ycrdt_validate_update(ycrdt_buf update, int *structs_ok);
/* Test hook for the pending-struct emulation (yc_ingest.cpp): replays n Y.applyUpdate calls into
 * an empty doc on struct headers only, with Y.mergeUpdates supplied by the caller (`merge` fills
 * *out with caller-owned bytes that must stay valid until it returns). Outputs the store's state
 * vector (clients ascending), the pending-structs update (len 0 = none) and the pending delete set
 * (len 0 = none); release them with ycrdt_free. */
typedef int (*ycrdt_merge_fn)(void *ctx, const ycrdt_buf *ups, size_t n, ycrdt_out *out);
int ycrdt_debug_replay(const ycrdt_buf *ups, size_t n, ycrdt_merge_fn merge, void *ctx, ycrdt_out *sv,
                       ycrdt_out *pending, ycrdt_out *pending_ds);

/* ---- multi-GPU: RCCL over xGMI inside the library, one rank per GPU.
 * Rank 0 creates the unique id; the caller hands those bytes to every rank (any channel), then each
 * rank creates its communicator on its engine's device. */
int ycrdt_comm_unique_id(uint8_t id[YCRDT_COMM_ID_BYTES]);
int ycrdt_comm_create(ycrdt_engine *e, int nranks, int rank, const uint8_t id[YCRDT_COMM_ID_BYTES], ycrdt_comm **out);
void ycrdt_comm_destroy(ycrdt_comm *c);
/* A communicator over the caller's own transport: the library's exchanges run their collectives
 * through these host callbacks instead of RCCL (device buffers are staged through host memory).
 * Each callback returns 0 on success; every rank must make the same calls in the same order. Used
 * by hosts without RCCL between their processes (and by the world-size-2 gloo tests, two processes
 * on one GPU). Failure inside an exchange: a rank that fails between two collectives of one
 * exchange cannot abort a host transport the way it aborts an RCCL communicator (ncclCommAbort),
 * so its peers stay in the callback they are in until the TRANSPORT gives up: host transports must
 * carry their own timeout (gloo's process-group timeout does) and return nonzero from the callback,
 * which then fails the merge on that rank. Failures before an exchange never block: every exchange
 * starts with a one-word status agreement. */
typedef struct {
  void *ctx;
  /* in place over n host words of every rank: op 0 = sum, 1 = max */
  int (*allreduce_u32)(void *ctx, uint32_t *words, size_t n, int op);
  /* recv[r * bytes .. (r + 1) * bytes) = rank r's send (bytes is the same on every rank) */
  int (*allgather)(void *ctx, const uint8_t *send, size_t bytes, uint8_t *recv);
} ycrdt_exchange;
int ycrdt_comm_create_exchange(ycrdt_engine *e, int nranks, int rank, const ycrdt_exchange *x, ycrdt_comm **out);
/* Stable owner rank of a document / topic id (crdt.js:221,235: one Y.Doc per topic): the same on
 * every rank, process and run (64-bit FNV-1a of the id bytes, mixed, mod world). A fleet routes
 * every update of a topic to its owner, which merges it alone (weak scaling, no data collective). */
uint32_t ycrdt_route(const uint8_t *id, size_t len, uint32_t world);
/* Key-hash sharded merge of ONE document (C4): every rank stages the same updates; the integrate
 * phases (map winner, YATA, dead types, merge adjacency) run for the rank's shard only — lists
 * owned by hash(top-level entry) % nshards — and the per-segment flag words are summed over RCCL;
 * every rank then encodes the full result. comm == NULL: all nshards logical shards run in turn on
 * this GPU (the partition check: byte-identical to ycrdt_batch_merge). Read the result with
 * ycrdt_batch_result. */
int ycrdt_batch_merge_sharded(ycrdt_batch *b, ycrdt_comm *comm, uint32_t nshards, ycrdt_merge_stats *st);
/* State vector of the union of what the ranks hold of one document (crdt.js:239,289 exchange):
 * all-gather + max per client, descending client order. */
int ycrdt_comm_sv_allreduce_max(ycrdt_comm *c, ycrdt_engine *e, ycrdt_buf sv, ycrdt_out *out);
/* Fleet state vectors (C5; crdt.js:239,289 per topic, batched over the fleet): this rank holds n
 * documents (ids docs[i] < 0xFFFFFFFF, state vectors svs[i]) — any subset of the fleet. Every rank
 * receives, for each document ANY rank holds, the state vector of the union (max clock per client,
 * descending client order): *doc_ids = u32[m] ascending, *offs = u64[m + 1], document doc_ids[j]'s
 * state vector = blob[offs[j] .. offs[j+1]). One dense all-reduce(MAX) over the fleet's sorted
 * (document, client) key space, built on the device (sort, reduce, all-gather of distinct keys,
 * unique). Release the three outputs with ycrdt_free. */
int ycrdt_comm_fleet_sv_allreduce_max(ycrdt_comm *c, ycrdt_engine *e, const uint32_t *docs, const ycrdt_buf *svs, size_t n,
                                      ycrdt_out *doc_ids, ycrdt_out *offs, ycrdt_out *blob);
/* Delete sets of all ranks (each a delete-set-only or full update) all-gathered and merged with the
 * engine's HIP mergeUpdates (the delete-set union): every rank receives the same update. */
int ycrdt_comm_ds_allgather(ycrdt_comm *c, ycrdt_engine *e, ycrdt_buf update, ycrdt_out *out);

/* Every rank's byte string, in rank order (variable lengths): blob = the concatenation, offs =
 * (nranks + 1) u64 offsets into it. The host-side control exchange of a multi-rank job (barrier,
 * the max of the ranks' step times, per-rank reports) over the library's own transport. */
int ycrdt_comm_allgather(ycrdt_comm *c, ycrdt_engine *e, ycrdt_buf mine, ycrdt_out *blob, ycrdt_out *offs);
/* HIP devices visible to this process (a launcher assigns rank r to device r % count) */
int ycrdt_device_count(int *count);

void ycrdt_free(ycrdt_out *o);
const char *ycrdt_last_error(void);
const char *ycrdt_version(void);

#ifdef __cplusplus
}
#endif
#endif
