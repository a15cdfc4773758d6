/* ycrdt_napi.c — Node-API addon over the C ABI (include/ycrdt.h).
 *
 * This is the reference-language host binding: @ypear/crdt loads its CRDT engine from
 * `router.options.Y` (reference crdt.js:175-180), so a Node module exporting the Yjs functions
 * the reference calls is the drop-in. crdt_amd/js/index.js builds that `Y` object on top of this
 * binding. Plain C + node_api.h (NAPI 8, Node >= 12.22); no node-gyp needed:
 *   gcc -shared -fPIC -I/usr/include/node ycrdt_napi.c -L.. -lycrdt -Wl,-rpath,'$ORIGIN/..'
 * Errors from the engine become JS `Error`s carrying ycrdt_last_error() (the reference only reads
 * e.message, crdt.js:38-39) and a numeric `code`.
 */
#define NAPI_VERSION 8
#include <node_api.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/ycrdt.h"

#define CHECK(env, call)                                                 \
  do {                                                                   \
    if ((call) != napi_ok) {                                             \
      napi_throw_error((env), NULL, "ycrdt: N-API call failed: " #call); \
      return NULL;                                                       \
    }                                                                    \
  } while (0)

static ycrdt_engine *g_engine = NULL; /* one engine (HIP device + stream) per process */
static int g_device = 0;

static napi_value throw_rc(napi_env env, int rc) {
  napi_value msg, err, code;
  const char *m = ycrdt_last_error();
  napi_create_string_utf8(env, m && m[0] ? m : "ycrdt error", NAPI_AUTO_LENGTH, &msg);
  napi_create_error(env, NULL, msg, &err);
  napi_create_int32(env, rc, &code);
  napi_set_named_property(env, err, "code", code);
  napi_throw(env, err);
  return NULL;
}

static ycrdt_engine *engine(napi_env env) {
  if (!g_engine) {
    /* YCRDT_COMPAT=135: Yjs 13.5.16 client order in delete sets / state vectors (include/ycrdt.h) */
    const char *cv = getenv("YCRDT_COMPAT");
    int rc = ycrdt_engine_create(g_device, cv && atoi(cv) == 135 ? 135 : 136, &g_engine);
    if (rc != YCRDT_OK) {
      g_engine = NULL;
      throw_rc(env, rc);
      return NULL;
    }
  }
  return g_engine;
}

/* Uint8Array / Buffer argument → borrowed (ptr, len) */
static int get_bytes(napi_env env, napi_value v, ycrdt_buf *out) {
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (is_ta) {
    napi_typedarray_type t;
    size_t len, off;
    void *data;
    napi_value ab;
    if (napi_get_typedarray_info(env, v, &t, &len, &data, &ab, &off) != napi_ok || t != napi_uint8_array) return 0;
    out->ptr = (const uint8_t *)data;
    out->len = len;
    return 1;
  }
  bool is_buf = false;
  napi_is_buffer(env, v, &is_buf);
  if (is_buf) {
    void *data;
    size_t len;
    if (napi_get_buffer_info(env, v, &data, &len) != napi_ok) return 0;
    out->ptr = (const uint8_t *)data;
    out->len = len;
    return 1;
  }
  return 0;
}


static napi_value u8_from_out(napi_env env, ycrdt_out *o) {
  napi_value ab, ta;
  void *data = NULL;
  size_t n = o->len;
  CHECK(env, napi_create_arraybuffer(env, n, &data, &ab));
  if (n) memcpy(data, o->ptr, n);
  ycrdt_free(o);
  CHECK(env, napi_create_typedarray(env, napi_uint8_array, n, ab, 0, &ta));
  return ta;
}

static void doc_finalize(napi_env env, void *data, void *hint) {
  (void)env;
  (void)hint;
  ycrdt_doc_destroy((ycrdt_doc *)data);
}

static ycrdt_doc *get_doc(napi_env env, napi_value v) {
  void *p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, NULL, "ycrdt: expected a doc handle");
    return NULL;
  }
  return (ycrdt_doc *)p;
}

/* setDevice(ordinal) — before the first engine use */
static napi_value js_set_device(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t dev = 0;
  if (argc > 0) napi_get_value_int32(env, argv[0], &dev);
  g_device = dev;
  return NULL;
}

/* docCreate(clientId) → handle   (new Y.Doc(), crdt.js:33,54,56,80,221) */
static napi_value js_doc_create(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], out;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t cid = 0;
  if (argc > 0) napi_get_value_uint32(env, argv[0], &cid);
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_doc *d = NULL;
  int rc = ycrdt_doc_create(e, cid, &d);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_external(env, d, doc_finalize, NULL, &out));
  return out;
}

/* applyUpdates(doc, update | update[])   (Y.applyUpdate, crdt.js:35,56,58,85,294) */
static napi_value js_apply_updates(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 2) { napi_throw_type_error(env, NULL, "applyUpdates(doc, updates)"); return NULL; }
  ycrdt_doc *d = get_doc(env, argv[0]);
  if (!d) return NULL;
  bool is_arr = false;
  napi_is_array(env, argv[1], &is_arr);
  if (!is_arr) {
    ycrdt_buf b;
    if (!get_bytes(env, argv[1], &b)) { napi_throw_type_error(env, NULL, "update must be a Uint8Array"); return NULL; }
    int rc = ycrdt_apply_update(d, b);
    return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
  }
  uint32_t n = 0;
  napi_get_array_length(env, argv[1], &n);
  ycrdt_buf *bufs = (ycrdt_buf *)calloc(n ? n : 1, sizeof(ycrdt_buf));
  for (uint32_t i = 0; i < n; ++i) {
    napi_value el;
    napi_get_element(env, argv[1], i, &el);
    if (!get_bytes(env, el, &bufs[i])) {
      free(bufs);
      napi_throw_type_error(env, NULL, "updates must be Uint8Arrays");
      return NULL;
    }
  }
  int rc = ycrdt_apply_updates(d, bufs, n);
  free(bufs);
  return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
}

/* encodeStateAsUpdate(doc[, sv])   (crdt.js:56,260,288,347,383,443,471,505,533,560,585,611) */
/* applyUpdatesMulti(docs[], updates[]) — Y.applyUpdate(docs[i], updates[i]) for a fleet, merged in
 * one device pass (ycrdt_apply_updates_multi; crdt.js:235 one doc per topic, :294 onData) */
static napi_value js_apply_updates_multi(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool a0 = false, a1 = false;
  if (argc >= 2) { napi_is_array(env, argv[0], &a0); napi_is_array(env, argv[1], &a1); }
  uint32_t n = 0, m = 0;
  if (a0) napi_get_array_length(env, argv[0], &n);
  if (a1) napi_get_array_length(env, argv[1], &m);
  if (!a0 || !a1 || n != m) { napi_throw_type_error(env, NULL, "applyUpdatesMulti(docs[], updates[]) of equal length"); return NULL; }
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_doc **docs = (ycrdt_doc **)calloc(n ? n : 1, sizeof(ycrdt_doc *));
  ycrdt_buf *bufs = (ycrdt_buf *)calloc(n ? n : 1, sizeof(ycrdt_buf));
  if (!docs || !bufs) {
    free(docs); free(bufs);
    napi_throw_error(env, NULL, "applyUpdatesMulti: out of host memory");
    return NULL;
  }
  for (uint32_t i = 0; i < n; ++i) {
    napi_value d, u;
    napi_get_element(env, argv[0], i, &d);
    napi_get_element(env, argv[1], i, &u);
    docs[i] = get_doc(env, d);
    /* get_doc has already thrown for a non-Doc; only a bad update still needs an error */
    const int doc_ok = docs[i] != NULL;
    if (!doc_ok || !get_bytes(env, u, &bufs[i])) {
      free(docs); free(bufs);
      if (doc_ok) napi_throw_type_error(env, NULL, "updates must be Uint8Arrays");
      return NULL;
    }
  }
  int rc = ycrdt_apply_updates_multi(e, docs, bufs, n);
  free(docs); free(bufs);
  return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
}

static napi_value js_encode_state_as_update(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_doc *d = argc > 0 ? get_doc(env, argv[0]) : NULL;
  if (!d) return NULL;
  ycrdt_buf sv = {NULL, 0};
  if (argc > 1) {
    napi_valuetype t;
    napi_typeof(env, argv[1], &t);
    if (t != napi_undefined && t != napi_null && !get_bytes(env, argv[1], &sv)) {
      napi_throw_type_error(env, NULL, "state vector must be a Uint8Array");
      return NULL;
    }
  }
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_encode_state_as_update(d, sv, &o);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  return u8_from_out(env, &o);
}

/* encodeStatesAsUpdates(docs[], sv[]) → Uint8Array[]   (Y.encodeStateAsUpdate(docs[i], svs[i]) for
 * every pair in one device pass, ycrdt_docs_diff: the sync responder of crdt.js:286-291 batched
 * over peers and topics; a null / undefined state vector asks for the full state) */
static napi_value js_encode_states_as_updates(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool a0 = false, a1 = false;
  if (argc >= 2) { napi_is_array(env, argv[0], &a0); napi_is_array(env, argv[1], &a1); }
  uint32_t n = 0, m = 0;
  if (a0) napi_get_array_length(env, argv[0], &n);
  if (a1) napi_get_array_length(env, argv[1], &m);
  if (!a0 || !a1 || n != m) {
    napi_throw_type_error(env, NULL, "encodeStatesAsUpdates(docs[], stateVectors[]) with one state vector per doc");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_doc **docs = (ycrdt_doc **)calloc(n ? n : 1, sizeof(ycrdt_doc *));
  ycrdt_buf *svs = (ycrdt_buf *)calloc(n ? n : 1, sizeof(ycrdt_buf));
  uint64_t *offs = (uint64_t *)calloc((size_t)n + 1, sizeof(uint64_t));
  if (!docs || !svs || !offs) {
    free(docs); free(svs); free(offs);
    napi_throw_error(env, NULL, "encodeStatesAsUpdates: out of host memory");
    return NULL;
  }
  for (uint32_t i = 0; i < n; ++i) {
    napi_value d, v;
    napi_valuetype t;
    napi_get_element(env, argv[0], i, &d);
    napi_get_element(env, argv[1], i, &v);
    napi_typeof(env, v, &t);
    docs[i] = get_doc(env, d);
    const int doc_ok = docs[i] != NULL;
    if (!doc_ok || (t != napi_undefined && t != napi_null && !get_bytes(env, v, &svs[i]))) {
      free(docs); free(svs); free(offs);
      if (doc_ok) napi_throw_type_error(env, NULL, "state vectors must be Uint8Arrays");
      return NULL;
    }
  }
  ycrdt_out blob = {NULL, 0};
  int rc = ycrdt_docs_diff(e, docs, svs, n, &blob, offs, NULL);
  free(docs); free(svs);
  if (rc != YCRDT_OK) { free(offs); return throw_rc(env, rc); }
  napi_value arr = NULL;
  if (napi_create_array_with_length(env, n, &arr) != napi_ok) arr = NULL;
  for (uint32_t i = 0; arr && i < n; ++i) {
    napi_value ab, ta;
    void *data = NULL;
    const size_t len = (size_t)(offs[i + 1] - offs[i]);
    if (napi_create_arraybuffer(env, len, &data, &ab) != napi_ok ||
        napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta) != napi_ok) { arr = NULL; break; }
    if (len) memcpy(data, blob.ptr + offs[i], len);
    napi_set_element(env, arr, i, ta);
  }
  ycrdt_free(&blob);
  free(offs);
  if (!arr) napi_throw_error(env, NULL, "ycrdt: N-API call failed: encodeStatesAsUpdates result");
  return arr;
}

/* encodeStateVector(doc)   (crdt.js:59,239,258,289) */
static napi_value js_encode_state_vector(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_doc *d = argc > 0 ? get_doc(env, argv[0]) : NULL;
  if (!d) return NULL;
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_encode_state_vector(d, &o);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  return u8_from_out(env, &o);
}

/* takeLocalUpdate(doc) → Uint8Array: the local ops since the previous call as one update */
static napi_value js_take_local_update(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_doc *d = argc > 0 ? get_doc(env, argv[0]) : NULL;
  if (!d) return NULL;
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_doc_take_local_update(d, &o);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  return u8_from_out(env, &o);
}

/* trackLocalUpdates(doc[, on = true]): record local-op updates for takeLocalUpdate (opt-in) */
static napi_value js_track_local(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_doc *d = argc > 0 ? get_doc(env, argv[0]) : NULL;
  if (!d) return NULL;
  bool on = true;
  if (argc > 1) CHECK(env, napi_get_value_bool(env, argv[1], &on));
  int rc = ycrdt_doc_track_local(d, on ? 1 : 0);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  return NULL;
}

/* lastStats(doc) → {items, structs, units, segments, outBytes, deviceMs} */
static napi_value js_last_stats(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1], obj, v;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_doc *d = argc > 0 ? get_doc(env, argv[0]) : NULL;
  if (!d) return NULL;
  ycrdt_merge_stats st;
  int rc = ycrdt_doc_last_stats(d, &st);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_object(env, &obj));
#define PUT(name, val) napi_create_double(env, (double)(val), &v); napi_set_named_property(env, obj, name, v)
  PUT("inBytes", st.in_bytes);
  PUT("items", st.items);
  PUT("structs", st.structs);
  PUT("units", st.units);
  PUT("segments", st.segments);
  PUT("outBytes", st.out_bytes);
  PUT("clients", st.clients);
  PUT("deviceMs", st.device_ms);
#undef PUT
  return obj;
}

/* mergeUpdates(update[]) → Uint8Array   (Y.mergeUpdates, north_star / Y@39011) */
static napi_value js_merge_updates(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool is_arr = false;
  if (argc > 0) napi_is_array(env, argv[0], &is_arr);
  if (!is_arr) { napi_throw_type_error(env, NULL, "mergeUpdates(updates[])"); return NULL; }
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  uint32_t n = 0;
  napi_get_array_length(env, argv[0], &n);
  ycrdt_buf *bufs = (ycrdt_buf *)calloc(n ? n : 1, sizeof(ycrdt_buf));
  for (uint32_t i = 0; i < n; ++i) {
    napi_value el;
    napi_get_element(env, argv[0], i, &el);
    if (!get_bytes(env, el, &bufs[i])) { free(bufs); napi_throw_type_error(env, NULL, "updates must be Uint8Arrays"); return NULL; }
  }
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_merge_updates(e, bufs, n, &o);
  free(bufs);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  return u8_from_out(env, &o);
}

/* diffUpdate(update, sv) → Uint8Array   (Y.diffUpdate, Y@40711) */
static napi_value js_diff_update(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_buf u, sv;
  if (argc < 2 || !get_bytes(env, argv[0], &u) || !get_bytes(env, argv[1], &sv)) {
    napi_throw_type_error(env, NULL, "diffUpdate(update, stateVector)");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_diff_update(e, u, sv, &o);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  return u8_from_out(env, &o);
}

/* diffUpdates(update[], sv[]) → Uint8Array[]   (n x Y.diffUpdate in one batched device pass: the
 * sync responder of crdt.js:286-291 across peers / topics) */
static int get_buf_array(napi_env env, napi_value arr, ycrdt_buf **out, uint32_t *n) {
  bool is_arr = false;
  napi_is_array(env, arr, &is_arr);
  if (!is_arr) return 0;
  napi_get_array_length(env, arr, n);
  *out = (ycrdt_buf *)calloc(*n ? *n : 1, sizeof(ycrdt_buf));
  for (uint32_t i = 0; i < *n; ++i) {
    napi_value el;
    napi_get_element(env, arr, i, &el);
    if (!get_bytes(env, el, &(*out)[i])) { free(*out); *out = NULL; return 0; }
  }
  return 1;
}
static napi_value js_diff_updates(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_buf *ups = NULL, *svs = NULL;
  uint32_t n = 0, m = 0;
  if (argc < 2 || !get_buf_array(env, argv[0], &ups, &n) || !get_buf_array(env, argv[1], &svs, &m) || n != m) {
    free(ups);
    free(svs);
    napi_throw_type_error(env, NULL, "diffUpdates(updates[], stateVectors[]) with one state vector per update");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) { free(ups); free(svs); return NULL; }
  ycrdt_out *outs = (ycrdt_out *)calloc(n ? n : 1, sizeof(ycrdt_out));
  int rc = ycrdt_diff_updates(e, ups, svs, n, outs);
  free(ups);
  free(svs);
  if (rc != YCRDT_OK) { free(outs); return throw_rc(env, rc); }
  napi_value arr;
  napi_create_array_with_length(env, n, &arr);
  for (uint32_t i = 0; i < n; ++i) napi_set_element(env, arr, i, u8_from_out(env, &outs[i]));
  free(outs);
  return arr;
}

/* a blob and its n + 1 offsets → Uint8Array[n], views of one ArrayBuffer (releases both) */
static napi_value slices_from_blob(napi_env env, ycrdt_out *blob, uint64_t *offs, uint32_t n) {
  napi_value ab, arr;
  void *data = NULL;
  if (napi_create_arraybuffer(env, blob->len, &data, &ab) != napi_ok) {
    ycrdt_free(blob);
    free(offs);
    napi_throw_error(env, NULL, "ycrdt: N-API call failed: napi_create_arraybuffer");
    return NULL;
  }
  if (blob->len) memcpy(data, blob->ptr, blob->len);
  ycrdt_free(blob);
  napi_create_array_with_length(env, n, &arr);
  for (uint32_t i = 0; i < n; ++i) {
    napi_value ta;
    napi_create_typedarray(env, napi_uint8_array, (size_t)(offs[i + 1] - offs[i]), ab, (size_t)offs[i], &ta);
    napi_set_element(env, arr, i, ta);
  }
  free(offs);
  return arr;
}

/* encodeStateVectorFromUpdate(update) → Uint8Array   (Y.encodeStateVectorFromUpdate: what a doc-less
 * store holds of a topic, crdt.js:28-77 without the temporary doc) */
static napi_value js_update_state_vector(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_buf u;
  if (argc < 1 || !get_bytes(env, argv[0], &u)) {
    napi_throw_type_error(env, NULL, "encodeStateVectorFromUpdate(update)");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_update_state_vector(e, u, &o);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  return u8_from_out(env, &o);
}

/* encodeStateVectorsFromUpdates(update[]) → Uint8Array[]   (n x Y.encodeStateVectorFromUpdate in one
 * device pass; the results are views of one ArrayBuffer) */
static napi_value js_updates_state_vectors(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_buf *ups = NULL;
  uint32_t n = 0;
  if (argc < 1 || !get_buf_array(env, argv[0], &ups, &n)) {
    napi_throw_type_error(env, NULL, "encodeStateVectorsFromUpdates(updates[])");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) { free(ups); return NULL; }
  uint64_t *offs = (uint64_t *)calloc((size_t)n + 1, sizeof(uint64_t));
  if (!offs) {
    free(ups);
    napi_throw_error(env, NULL, "ycrdt: out of memory");
    return NULL;
  }
  ycrdt_out blob = {NULL, 0};
  int rc = ycrdt_updates_state_vectors(e, ups, n, &blob, offs, NULL);
  free(ups);
  if (rc != YCRDT_OK) { free(offs); return throw_rc(env, rc); }
  return slices_from_blob(env, &blob, offs, n);
}

/* mergeUpdatesGroups(update[][]) → Uint8Array[]   (Y.mergeUpdates of every group in one device pass:
 * compacting the logs of many topics, crdt.js:79-98) */
static napi_value js_merge_updates_groups(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool is_arr = false;
  if (argc > 0) napi_is_array(env, argv[0], &is_arr);
  if (!is_arr) { napi_throw_type_error(env, NULL, "mergeUpdatesGroups(groups[][])"); return NULL; }
  uint32_t ng = 0;
  napi_get_array_length(env, argv[0], &ng);
  size_t n = 0, cap = 16;
  ycrdt_buf *ups = (ycrdt_buf *)malloc(cap * sizeof(ycrdt_buf));
  uint32_t *gof = (uint32_t *)malloc(cap * sizeof(uint32_t));
  for (uint32_t g = 0; g < ng && ups && gof; ++g) {
    napi_value el;
    ycrdt_buf *gu = NULL;
    uint32_t k = 0;
    napi_get_element(env, argv[0], g, &el);
    if (!get_buf_array(env, el, &gu, &k)) {
      free(ups);
      free(gof);
      napi_throw_type_error(env, NULL, "mergeUpdatesGroups: every group is an array of Uint8Arrays");
      return NULL;
    }
    if (n + k > cap) {
      while (n + k > cap) cap *= 2;
      ups = (ycrdt_buf *)realloc(ups, cap * sizeof(ycrdt_buf));
      gof = (uint32_t *)realloc(gof, cap * sizeof(uint32_t));
    }
    for (uint32_t i = 0; i < k && ups && gof; ++i) { ups[n] = gu[i]; gof[n++] = g; }
    free(gu);
  }
  uint64_t *offs = (uint64_t *)calloc((size_t)ng + 1, sizeof(uint64_t));
  ycrdt_engine *e = ups && gof && offs ? engine(env) : NULL;
  if (!e) {
    if (!(ups && gof && offs)) napi_throw_error(env, NULL, "ycrdt: out of memory");
    free(ups);
    free(gof);
    free(offs);
    return NULL;
  }
  ycrdt_out blob = {NULL, 0};
  int rc = ycrdt_merge_updates_groups(e, ups, gof, n, ng, &blob, offs, NULL);
  free(ups);
  free(gof);
  if (rc != YCRDT_OK) { free(offs); return throw_rc(env, rc); }
  return slices_from_blob(env, &blob, offs, ng);
}

static napi_value js_version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value s;
  CHECK(env, napi_create_string_utf8(env, ycrdt_version(), NAPI_AUTO_LENGTH, &s));
  return s;
}

/* ---- crdt.c materialisation and local ops (YMap / YArray methods of the facade) ------------ */
/* JS string (or null/undefined → NULL when `opt`) into a malloc'd UTF-8 buffer; 0 on a type error */
static int get_str(napi_env env, napi_value v, char **out, int opt) {
  napi_valuetype t;
  napi_typeof(env, v, &t);
  *out = NULL;
  if (opt && (t == napi_undefined || t == napi_null)) return 1;
  if (t != napi_string) return 0;
  size_t n = 0;
  if (napi_get_value_string_utf8(env, v, NULL, 0, &n) != napi_ok) return 0;
  *out = (char *)malloc(n + 1);
  if (napi_get_value_string_utf8(env, v, *out, n + 1, &n) != napi_ok) { free(*out); *out = NULL; return 0; }
  return 1;
}

typedef struct { ycrdt_doc *d; char *root, *pkey, *key; } op_args;

/* (doc, root, parentKey|null[, key]) — the target of every view/local-op call */
static int op_target(napi_env env, napi_value *argv, size_t argc, int want_key, op_args *a) {
  memset(a, 0, sizeof(*a));
  if (argc < (size_t)(3 + want_key)) { napi_throw_type_error(env, NULL, "ycrdt: missing arguments"); return 0; }
  a->d = get_doc(env, argv[0]);
  if (!a->d) return 0;
  if (!get_str(env, argv[1], &a->root, 0) || !get_str(env, argv[2], &a->pkey, 1) ||
      (want_key && !get_str(env, argv[3], &a->key, 0))) {
    free(a->root); free(a->pkey);
    napi_throw_type_error(env, NULL, "ycrdt: type name and keys must be strings");
    return 0;
  }
  return 1;
}
static void op_free(op_args *a) { free(a->root); free(a->pkey); free(a->key); }

/* docJson(doc, root, kind) → JSON text of YMap.toJSON (kind 0) / YArray.toJSON (kind 1)
 * (crdt.js:202,214,304,372,494,528,555,581,607) */
static napi_value js_doc_json(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], s;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  ycrdt_doc *d = argc > 2 ? get_doc(env, argv[0]) : NULL;
  if (!d) return NULL;
  char *root = NULL;
  int32_t kind = 0;
  if (!get_str(env, argv[1], &root, 0) || napi_get_value_int32(env, argv[2], &kind) != napi_ok) {
    free(root);
    napi_throw_type_error(env, NULL, "docJson(doc, root, kind)");
    return NULL;
  }
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_doc_json(d, root, kind, &o);
  free(root);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_string_utf8(env, (const char *)o.ptr, o.len, &s));
  ycrdt_free(&o);
  return s;
}

/* docsJson(docs[], roots[], kinds[]) → string[]   (docJson(docs[i], roots[i], kinds[i]) for every
 * request in one device pass, ycrdt_docs_json: the `c[key] = h[key].toJSON()` refresh of
 * crdt.js:297-305 batched over documents; kinds 0 = YMap, 1 = YArray) */
static napi_value js_docs_json(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool a0 = false, a1 = false, a2 = false;
  if (argc >= 3) { napi_is_array(env, argv[0], &a0); napi_is_array(env, argv[1], &a1); napi_is_array(env, argv[2], &a2); }
  uint32_t n = 0, m = 0, k = 0;
  if (a0) napi_get_array_length(env, argv[0], &n);
  if (a1) napi_get_array_length(env, argv[1], &m);
  if (a2) napi_get_array_length(env, argv[2], &k);
  if (!a0 || !a1 || !a2 || n != m || n != k) {
    napi_throw_type_error(env, NULL, "docsJson(docs[], roots[], kinds[]) with one root and one kind per doc");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_doc **docs = (ycrdt_doc **)calloc(n ? n : 1, sizeof(ycrdt_doc *));
  char **roots = (char **)calloc(n ? n : 1, sizeof(char *));
  int *kinds = (int *)calloc(n ? n : 1, sizeof(int));
  uint64_t *offs = (uint64_t *)calloc((size_t)n + 1, sizeof(uint64_t));
  int ok = docs && roots && kinds && offs;
  if (!ok) napi_throw_error(env, NULL, "docsJson: out of host memory");
  for (uint32_t i = 0; ok && i < n; ++i) {
    napi_value d, r, q;
    int32_t kind = 0;
    napi_get_element(env, argv[0], i, &d);
    napi_get_element(env, argv[1], i, &r);
    napi_get_element(env, argv[2], i, &q);
    docs[i] = get_doc(env, d);
    if (!docs[i]) { ok = 0; break; }
    if (!get_str(env, r, &roots[i], 0) || napi_get_value_int32(env, q, &kind) != napi_ok) {
      napi_throw_type_error(env, NULL, "docsJson: roots must be strings, kinds 0 (map) or 1 (array)");
      ok = 0;
      break;
    }
    kinds[i] = kind;
  }
  ycrdt_out blob = {NULL, 0};
  napi_value arr = NULL;
  if (ok) {
    int rc = ycrdt_docs_json(e, docs, (const char *const *)roots, kinds, n, &blob, offs, NULL);
    if (rc != YCRDT_OK) {
      throw_rc(env, rc);
    } else {
      if (napi_create_array_with_length(env, n, &arr) != napi_ok) arr = NULL;
      for (uint32_t i = 0; arr && i < n; ++i) {
        napi_value s;
        if (napi_create_string_utf8(env, (const char *)blob.ptr + offs[i], (size_t)(offs[i + 1] - offs[i]), &s) != napi_ok) { arr = NULL; break; }
        napi_set_element(env, arr, i, s);
      }
      ycrdt_free(&blob);
      if (!arr) napi_throw_error(env, NULL, "ycrdt: N-API call failed: docsJson result");
    }
  }
  if (roots) for (uint32_t i = 0; i < n; ++i) free(roots[i]);
  free(docs); free(roots); free(kinds); free(offs);
  return arr;
}

/* docsCache(docs[], index | null) → string[]   (the text of crdt.js's cache object `c` of every
 * document in one device pass, ycrdt_docs_cache: the loop of crdt.js:201-216 / 297-305 batched over
 * documents, the index map read on the device; null: the index root "ix") */
static napi_value js_docs_cache(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool a0 = false;
  if (argc >= 1) napi_is_array(env, argv[0], &a0);
  uint32_t n = 0;
  if (a0) napi_get_array_length(env, argv[0], &n);
  char *index = NULL;
  if (!a0 || (argc >= 2 && !get_str(env, argv[1], &index, 1))) {
    napi_throw_type_error(env, NULL, "docsCache(docs[], index | null)");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) { free(index); return NULL; }
  ycrdt_doc **docs = (ycrdt_doc **)calloc(n ? n : 1, sizeof(ycrdt_doc *));
  uint64_t *offs = (uint64_t *)calloc((size_t)n + 1, sizeof(uint64_t));
  int ok = docs && offs;
  if (!ok) napi_throw_error(env, NULL, "docsCache: out of host memory");
  for (uint32_t i = 0; ok && i < n; ++i) {
    napi_value d;
    napi_get_element(env, argv[0], i, &d);
    docs[i] = get_doc(env, d);
    if (!docs[i]) ok = 0;
  }
  ycrdt_out blob = {NULL, 0};
  napi_value arr = NULL;
  if (ok) {
    int rc = ycrdt_docs_cache(e, docs, n, index, &blob, offs, NULL);
    if (rc != YCRDT_OK) {
      throw_rc(env, rc);
    } else {
      if (napi_create_array_with_length(env, n, &arr) != napi_ok) arr = NULL;
      for (uint32_t i = 0; arr && i < n; ++i) {
        napi_value s;
        if (napi_create_string_utf8(env, (const char *)blob.ptr + offs[i], (size_t)(offs[i + 1] - offs[i]), &s) != napi_ok) { arr = NULL; break; }
        napi_set_element(env, arr, i, s);
      }
      ycrdt_free(&blob);
      if (!arr) napi_throw_error(env, NULL, "ycrdt: N-API call failed: docsCache result");
    }
  }
  free(docs); free(offs); free(index);
  return arr;
}

/* docsRead(docs[], ops[], roots[], parentKeys[], keys[], indexes[]) → (string | undefined | number)[]
 * (mapGet / mapSize / arrayGet / arrayLength of every request in one device pass, ycrdt_docs_read:
 * the `h[name].get(key)` / `.length` reads of crdt.js:423-430 batched over documents; ops are
 * YCRDT_READ_*; a get gives its JSON text or undefined, a size or length a number) */
static napi_value js_docs_read(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  uint32_t n = 0;
  int shape = argc >= 6;
  for (int j = 0; shape && j < 6; ++j) {
    bool is = false;
    uint32_t m = 0;
    napi_is_array(env, argv[j], &is);
    if (is) napi_get_array_length(env, argv[j], &m);
    if (j == 0) n = m;
    if (!is || m != n) shape = 0;
  }
  if (!shape) {
    napi_throw_type_error(env, NULL, "docsRead(docs[], ops[], roots[], parentKeys[], keys[], indexes[]) of one length");
    return NULL;
  }
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_read *reads = (ycrdt_read *)calloc(n ? n : 1, sizeof(ycrdt_read));
  uint64_t *offs = (uint64_t *)calloc((size_t)n + 1, sizeof(uint64_t));
  int32_t *states = (int32_t *)calloc(n ? n : 1, sizeof(int32_t));
  uint64_t *counts = (uint64_t *)calloc(n ? n : 1, sizeof(uint64_t));
  int ok = reads && offs && states && counts;
  if (!ok) napi_throw_error(env, NULL, "docsRead: out of host memory");
  for (uint32_t i = 0; ok && i < n; ++i) {
    napi_value v[6];
    for (int j = 0; j < 6; ++j) napi_get_element(env, argv[j], i, &v[j]);
    int32_t op = -1;
    double index = 0;
    napi_valuetype it;
    reads[i].doc = get_doc(env, v[0]);
    if (!reads[i].doc) { ok = 0; break; }
    napi_typeof(env, v[5], &it);
    if (napi_get_value_int32(env, v[1], &op) != napi_ok || !get_str(env, v[2], (char **)&reads[i].root, 0) ||
        !get_str(env, v[3], (char **)&reads[i].parent_key, 1) || !get_str(env, v[4], (char **)&reads[i].key, 1) ||
        (it == napi_number && napi_get_value_double(env, v[5], &index) != napi_ok) || index < 0 ||
        (op == YCRDT_READ_MAP_GET && !reads[i].key) || (op == YCRDT_READ_ARRAY_GET && it != napi_number)) {
      napi_throw_type_error(env, NULL, "docsRead: op 0..3, root and keys strings, index a number >= 0");
      ok = 0;
      break;
    }
    reads[i].op = op;
    reads[i].index = (uint64_t)index;
  }
  ycrdt_out blob = {NULL, 0};
  napi_value arr = NULL;
  if (ok) {
    int rc = ycrdt_docs_read(e, reads, n, &blob, offs, states, counts, NULL);
    if (rc != YCRDT_OK) {
      throw_rc(env, rc);
    } else {
      if (napi_create_array_with_length(env, n, &arr) != napi_ok) arr = NULL;
      for (uint32_t i = 0; arr && i < n; ++i) {
        napi_value s;
        napi_status st;
        if (reads[i].op == YCRDT_READ_MAP_SIZE || reads[i].op == YCRDT_READ_ARRAY_LENGTH) st = napi_create_double(env, (double)counts[i], &s);
        else if (states[i] != 1) st = napi_get_undefined(env, &s);
        else st = napi_create_string_utf8(env, (const char *)blob.ptr + offs[i], (size_t)(offs[i + 1] - offs[i]), &s);
        if (st != napi_ok) { arr = NULL; break; }
        napi_set_element(env, arr, i, s);
      }
      ycrdt_free(&blob);
      if (!arr) napi_throw_error(env, NULL, "ycrdt: N-API call failed: docsRead result");
    }
  }
  if (reads) for (uint32_t i = 0; i < n; ++i) { free((char *)reads[i].root); free((char *)reads[i].parent_key); free((char *)reads[i].key); }
  free(reads); free(offs); free(states); free(counts);
  return arr;
}

/* docsWrite(ops[]) → [updates: Uint8Array[], codes: number[], message: string]
 * (mapSet / mapSetType / mapDelete / arrayInsert / arrayPush / arrayDelete of every op in one device
 * pass, ycrdt_docs_write: the `set` / `del` / `push` / `insert` / `cut` of crdt.js:423-611 batched
 * over documents). An op is [doc, op (YCRDT_WRITE_*), root, parentKey | null, key | null,
 * values (encoded `any`s) | null, count, typeRef, index, length]. updates[i] is the update the op
 * enqueued (empty where it wrote nothing), codes[i] what its single call returns, message the last
 * failed op's text.
 * docsTransact(ops[]) is the same call through ycrdt_docs_transact: a document's ops may depend on
 * one another (crdt.js:329-355 execBatch) and still run in the one pass. */
static napi_value docs_write_call(napi_env env, napi_callback_info info, int transact) {
  size_t argc = 1;
  napi_value argv[1];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  bool is = false;
  uint32_t n = 0;
  if (argc >= 1) napi_is_array(env, argv[0], &is);
  if (!is) {
    napi_throw_type_error(env, NULL, "docsWrite(ops[])");
    return NULL;
  }
  napi_get_array_length(env, argv[0], &n);
  ycrdt_engine *e = engine(env);
  if (!e) return NULL;
  ycrdt_write *ops = (ycrdt_write *)calloc(n ? n : 1, sizeof(ycrdt_write));
  uint64_t *offs = (uint64_t *)calloc((size_t)n + 1, sizeof(uint64_t));
  int32_t *codes = (int32_t *)calloc(n ? n : 1, sizeof(int32_t));
  int ok = ops && offs && codes;
  if (!ok) napi_throw_error(env, NULL, "docsWrite: out of host memory");
  for (uint32_t i = 0; ok && i < n; ++i) {
    napi_value op, v[10];
    bool arr = false;
    uint32_t m = 0;
    napi_get_element(env, argv[0], i, &op);
    napi_is_array(env, op, &arr);
    if (arr) napi_get_array_length(env, op, &m);
    if (m != 10) { napi_throw_type_error(env, NULL, "docsWrite: an op is an array of 10"); ok = 0; break; }
    for (int j = 0; j < 10; ++j) napi_get_element(env, op, j, &v[j]);
    ops[i].doc = get_doc(env, v[0]);
    if (!ops[i].doc) { ok = 0; break; }
    int32_t code = -1;
    uint32_t num[4] = {0, 0, 0, 0};
    napi_valuetype vt;
    ycrdt_buf any = {NULL, 0};
    napi_typeof(env, v[5], &vt);
    int good = napi_get_value_int32(env, v[1], &code) == napi_ok && get_str(env, v[2], (char **)&ops[i].root, 0) &&
               get_str(env, v[3], (char **)&ops[i].parent_key, 1) && get_str(env, v[4], (char **)&ops[i].key, 1) &&
               (vt == napi_null || vt == napi_undefined || get_bytes(env, v[5], &any));
    for (int j = 0; good && j < 4; ++j) good = napi_get_value_uint32(env, v[6 + j], &num[j]) == napi_ok;
    if (!good) {
      napi_throw_type_error(env, NULL, "docsWrite: op 0..5, root and keys strings, values a Uint8Array, count, typeRef, index and length numbers");
      ok = 0;
      break;
    }
    ops[i].op = code;
    ops[i].any = any.ptr; /* borrowed: the JS array keeps the values alive over the call */
    ops[i].any_len = any.len;
    ops[i].count = num[0];
    ops[i].type_ref = num[1];
    ops[i].index = num[2];
    ops[i].length = num[3];
  }
  ycrdt_out blob = {NULL, 0};
  napi_value res = NULL;
  if (ok) {
    int rc = transact ? ycrdt_docs_transact(e, ops, n, &blob, offs, codes, NULL) : ycrdt_docs_write(e, ops, n, &blob, offs, codes, NULL);
    if (rc != YCRDT_OK) {
      throw_rc(env, rc);
    } else {
      napi_value ups = NULL, cs = NULL, msg = NULL;
      const char *m = ycrdt_last_error();
      int made = napi_create_array_with_length(env, 3, &res) == napi_ok && napi_create_array_with_length(env, n, &ups) == napi_ok &&
                 napi_create_array_with_length(env, n, &cs) == napi_ok &&
                 napi_create_string_utf8(env, m ? m : "", NAPI_AUTO_LENGTH, &msg) == napi_ok;
      for (uint32_t i = 0; made && i < n; ++i) {
        napi_value ab, ta, c;
        void *data = NULL;
        const size_t len = (size_t)(offs[i + 1] - offs[i]);
        made = napi_create_arraybuffer(env, len, &data, &ab) == napi_ok && napi_create_typedarray(env, napi_uint8_array, len, ab, 0, &ta) == napi_ok &&
               napi_create_int32(env, codes[i], &c) == napi_ok;
        if (!made) break;
        if (len) memcpy(data, blob.ptr + offs[i], len);
        napi_set_element(env, ups, i, ta);
        napi_set_element(env, cs, i, c);
      }
      ycrdt_free(&blob);
      if (made) {
        napi_set_element(env, res, 0, ups);
        napi_set_element(env, res, 1, cs);
        napi_set_element(env, res, 2, msg);
      } else {
        res = NULL;
        napi_throw_error(env, NULL, "ycrdt: N-API call failed: docsWrite result");
      }
    }
  }
  if (ops) for (uint32_t i = 0; i < n; ++i) { free((char *)ops[i].root); free((char *)ops[i].parent_key); free((char *)ops[i].key); }
  free(ops); free(offs); free(codes);
  return res;
}
static napi_value js_docs_write(napi_env env, napi_callback_info info) { return docs_write_call(env, info, 0); }
static napi_value js_docs_transact(napi_env env, napi_callback_info info) { return docs_write_call(env, info, 1); }

/* typeJson(doc, root, parentKey, kind) → toJSON of the root type (parentKey null) or of the YMap
 * (kind 0) / YArray (kind 1) stored under root[parentKey], reading that type's own list only */
static napi_value js_type_json(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4], s;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 0, &a)) return NULL;
  int32_t kind = 0;
  if (argc < 4 || napi_get_value_int32(env, argv[3], &kind) != napi_ok) {
    op_free(&a);
    napi_throw_type_error(env, NULL, "typeJson(doc, root, parentKey, kind)");
    return NULL;
  }
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_type_json(a.d, a.root, a.pkey, kind, &o);
  op_free(&a);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_string_utf8(env, (const char *)o.ptr, o.len, &s));
  ycrdt_free(&o);
  return s;
}

/* mapEntries(doc, root, parentKey) → JSON text {"key": ["client:clock", value]} (map observers) */
static napi_value js_map_entries(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], s;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 0, &a)) return NULL;
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_map_entries(a.d, a.root, a.pkey, &o);
  op_free(&a);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_string_utf8(env, o.ptr ? (const char *)o.ptr : "{}", o.ptr ? o.len : 2, &s));
  ycrdt_free(&o);
  return s;
}

/* mapSet(doc, root, parentKey, key, anyBytes)   (YMap.set, crdt.js:375,434) */
static napi_value js_map_set(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 1, &a)) return NULL;
  ycrdt_buf v;
  int rc = YCRDT_E_ARG;
  if (argc > 4 && get_bytes(env, argv[4], &v)) rc = ycrdt_map_set(a.d, a.root, a.pkey, a.key, v.ptr, v.len);
  else { op_free(&a); napi_throw_type_error(env, NULL, "mapSet: value must be lib0 any bytes"); return NULL; }
  op_free(&a);
  return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
}

/* mapSetType(doc, root, parentKey, key, typeRef)   (YMap.set(key, new Y.Array()), crdt.js:423) */
static napi_value js_map_set_type(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 1, &a)) return NULL;
  uint32_t tr = 0;
  if (argc > 4) napi_get_value_uint32(env, argv[4], &tr);
  int rc = ycrdt_map_set_type(a.d, a.root, a.pkey, a.key, tr);
  op_free(&a);
  return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
}

/* mapDelete(doc, root, parentKey, key)   (YMap.delete, crdt.js:465) */
static napi_value js_map_delete(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 1, &a)) return NULL;
  int rc = ycrdt_map_delete(a.d, a.root, a.pkey, a.key);
  op_free(&a);
  return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
}

/* arrayInsert(doc, root, parentKey, index, anysBytes, count)   (insert/push/unshift, crdt.js:426-428,527,554,580) */
static napi_value js_array_insert(napi_env env, napi_callback_info info) {
  size_t argc = 6;
  napi_value argv[6];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 0, &a)) return NULL;
  uint32_t index = 0, count = 0;
  ycrdt_buf v;
  if (argc < 6 || napi_get_value_uint32(env, argv[3], &index) != napi_ok || !get_bytes(env, argv[4], &v) ||
      napi_get_value_uint32(env, argv[5], &count) != napi_ok) {
    op_free(&a);
    napi_throw_type_error(env, NULL, "arrayInsert(doc, root, parentKey, index, anys, count)");
    return NULL;
  }
  int rc = ycrdt_array_insert(a.d, a.root, a.pkey, index, v.ptr, v.len, count);
  op_free(&a);
  return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
}

/* arrayDelete(doc, root, parentKey, index, length)   (YArray.delete, crdt.js:429,606) */
static napi_value js_array_delete(napi_env env, napi_callback_info info) {
  size_t argc = 5;
  napi_value argv[5];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 0, &a)) return NULL;
  uint32_t index = 0, length = 0;
  if (argc < 5 || napi_get_value_uint32(env, argv[3], &index) != napi_ok ||
      napi_get_value_uint32(env, argv[4], &length) != napi_ok) {
    op_free(&a);
    napi_throw_type_error(env, NULL, "arrayDelete(doc, root, parentKey, index, length)");
    return NULL;
  }
  int rc = ycrdt_array_delete(a.d, a.root, a.pkey, index, length);
  op_free(&a);
  return rc == YCRDT_OK ? NULL : throw_rc(env, rc);
}

/* mapTypeAt(doc, root, key) → type ref of the shared type under root[key], -1 if none (YMap.get) */
static napi_value js_map_type_at(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[4], v;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (argc < 3) { napi_throw_type_error(env, NULL, "mapTypeAt(doc, root, key)"); return NULL; }
  napi_get_null(env, &argv[3]);
  napi_value args[4] = {argv[0], argv[1], argv[3], argv[2]};  /* (doc, root, null, key) */
  op_args a;
  if (!op_target(env, args, 4, 1, &a)) return NULL;
  int32_t tr = -1;
  int rc = ycrdt_map_type_at(a.d, a.root, a.key, &tr);
  op_free(&a);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_int32(env, tr, &v));
  return v;
}

/* per-key reads: JSON text, or undefined when absent / `undefined` (state 0 / 2); mapHas → bool */
static napi_value read_result(napi_env env, int rc, int state, ycrdt_out *o, int want_has) {
  napi_value v;
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  if (want_has) CHECK(env, napi_get_boolean(env, state != 0, &v));
  else if (state == 1) CHECK(env, napi_create_string_utf8(env, (const char *)o->ptr, o->len, &v));
  else CHECK(env, napi_get_undefined(env, &v));
  ycrdt_free(o);
  return v;
}

/* mapGet(doc, root, parentKey, key) → JSON text | undefined   (YMap.get, crdt.js:424) */
static napi_value js_map_get(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 1, &a)) return NULL;
  int state = 0;
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_map_get(a.d, a.root, a.pkey, a.key, &state, &o);
  op_free(&a);
  return read_result(env, rc, state, &o, 0);
}

/* mapHas(doc, root, parentKey, key) → bool   (YMap.has, crdt.js:423) */
static napi_value js_map_has(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 1, &a)) return NULL;
  int state = 0;
  ycrdt_out o = {NULL, 0};
  int rc = ycrdt_map_get(a.d, a.root, a.pkey, a.key, &state, &o);
  op_free(&a);
  return read_result(env, rc, state, &o, 1);
}

/* mapSize(doc, root, parentKey) → number   (YMap.size) */
static napi_value js_map_size(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], v;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 0, &a)) return NULL;
  uint32_t n = 0;
  int rc = ycrdt_map_size(a.d, a.root, a.pkey, &n);
  op_free(&a);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_uint32(env, n, &v));
  return v;
}

/* arrayLength(doc, root, parentKey) → number   (YArray.length; push, crdt.js:427) */
static napi_value js_array_length(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3], v;
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 0, &a)) return NULL;
  uint64_t n = 0;
  int rc = ycrdt_array_length(a.d, a.root, a.pkey, &n);
  op_free(&a);
  if (rc != YCRDT_OK) return throw_rc(env, rc);
  CHECK(env, napi_create_double(env, (double)n, &v));
  return v;
}

/* arrayGet(doc, root, parentKey, index) → JSON text | undefined   (YArray.get) */
static napi_value js_array_get(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  CHECK(env, napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  op_args a;
  if (!op_target(env, argv, argc, 0, &a)) return NULL;
  int64_t index = 0;
  if (argc < 4 || napi_get_value_int64(env, argv[3], &index) != napi_ok) {
    op_free(&a);
    napi_throw_type_error(env, NULL, "arrayGet(doc, root, parentKey, index)");
    return NULL;
  }
  int state = 0;
  ycrdt_out o = {NULL, 0};
  int rc = index < 0 ? YCRDT_OK : ycrdt_array_get(a.d, a.root, a.pkey, (uint64_t)index, &state, &o);
  op_free(&a);
  return read_result(env, rc, state, &o, 0);
}

static napi_value init(napi_env env, napi_value exports) {
  napi_property_descriptor props[] = {
      {"setDevice", NULL, js_set_device, NULL, NULL, NULL, napi_default, NULL},
      {"docCreate", NULL, js_doc_create, NULL, NULL, NULL, napi_default, NULL},
      {"applyUpdates", NULL, js_apply_updates, NULL, NULL, NULL, napi_default, NULL},
      {"applyUpdatesMulti", NULL, js_apply_updates_multi, NULL, NULL, NULL, napi_default, NULL},
      {"encodeStateAsUpdate", NULL, js_encode_state_as_update, NULL, NULL, NULL, napi_default, NULL},
      {"encodeStateVector", NULL, js_encode_state_vector, NULL, NULL, NULL, napi_default, NULL},
      {"mergeUpdates", NULL, js_merge_updates, NULL, NULL, NULL, napi_default, NULL},
      {"diffUpdate", NULL, js_diff_update, NULL, NULL, NULL, napi_default, NULL},
      {"diffUpdates", NULL, js_diff_updates, NULL, NULL, NULL, napi_default, NULL},
      {"encodeStateVectorFromUpdate", NULL, js_update_state_vector, NULL, NULL, NULL, napi_default, NULL},
      {"encodeStateVectorsFromUpdates", NULL, js_updates_state_vectors, NULL, NULL, NULL, napi_default, NULL},
      {"mergeUpdatesGroups", NULL, js_merge_updates_groups, NULL, NULL, NULL, napi_default, NULL},
      {"encodeStatesAsUpdates", NULL, js_encode_states_as_updates, NULL, NULL, NULL, napi_default, NULL},
      {"takeLocalUpdate", NULL, js_take_local_update, NULL, NULL, NULL, napi_default, NULL},
      {"trackLocalUpdates", NULL, js_track_local, NULL, NULL, NULL, napi_default, NULL},
      {"lastStats", NULL, js_last_stats, NULL, NULL, NULL, napi_default, NULL},
      {"version", NULL, js_version, NULL, NULL, NULL, napi_default, NULL},
      {"mapTypeAt", NULL, js_map_type_at, NULL, NULL, NULL, napi_default, NULL},
      {"docJson", NULL, js_doc_json, NULL, NULL, NULL, napi_default, NULL},
      {"docsJson", NULL, js_docs_json, NULL, NULL, NULL, napi_default, NULL},
      {"docsCache", NULL, js_docs_cache, NULL, NULL, NULL, napi_default, NULL},
      {"docsRead", NULL, js_docs_read, NULL, NULL, NULL, napi_default, NULL},
      {"docsWrite", NULL, js_docs_write, NULL, NULL, NULL, napi_default, NULL},
      {"docsTransact", NULL, js_docs_transact, NULL, NULL, NULL, napi_default, NULL},
      {"typeJson", NULL, js_type_json, NULL, NULL, NULL, napi_default, NULL},
      {"mapEntries", NULL, js_map_entries, NULL, NULL, NULL, napi_default, NULL},
      {"mapSet", NULL, js_map_set, NULL, NULL, NULL, napi_default, NULL},
      {"mapSetType", NULL, js_map_set_type, NULL, NULL, NULL, napi_default, NULL},
      {"mapDelete", NULL, js_map_delete, NULL, NULL, NULL, napi_default, NULL},
      {"arrayInsert", NULL, js_array_insert, NULL, NULL, NULL, napi_default, NULL},
      {"arrayDelete", NULL, js_array_delete, NULL, NULL, NULL, napi_default, NULL},
      {"mapGet", NULL, js_map_get, NULL, NULL, NULL, napi_default, NULL},
      {"mapHas", NULL, js_map_has, NULL, NULL, NULL, napi_default, NULL},
      {"mapSize", NULL, js_map_size, NULL, NULL, NULL, napi_default, NULL},
      {"arrayLength", NULL, js_array_length, NULL, NULL, NULL, napi_default, NULL},
      {"arrayGet", NULL, js_array_get, NULL, NULL, NULL, napi_default, NULL},
  };
  napi_define_properties(env, exports, sizeof(props) / sizeof(props[0]), props);
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
