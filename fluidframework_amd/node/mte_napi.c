/*
 * mte_napi.c — Node N-API addon over the C-ABI of libmte.so (include/mte.h).
 *
 * This is the "thin C-ABI exposed as a Node N-API addon" of BASELINE.json's
 * north star: the JavaScript host layer (index.js, BatchClient) packs
 * ISequencedDocumentMessage objects into 32-byte op records and hands them to
 * the engine through these functions.  Every function takes plain typed
 * arrays; nothing here interprets merge-tree semantics.
 *
 * Errors: a negative mte status becomes a thrown JS Error whose `code` is the
 * MTE_E_* value and whose message carries mte_strerror + mte_last_error (the
 * reference raises asserts with hex codes, client.ts:525-528; the JS layer
 * adds `assertCode` where a 1:1 equivalent exists).
 *
 * Built with gcc against /usr/include/node (N-API v8), linked to libmte.so
 * with an $ORIGIN rpath, so no node-gyp run is needed (Makefile).
 */
#define NAPI_VERSION 8
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/mte.h"

#define NAPI_CALL(env, call)                                          \
  do {                                                                \
    napi_status s_ = (call);                                          \
    if (s_ != napi_ok) {                                              \
      const napi_extended_error_info* ei_ = NULL;                     \
      napi_get_last_error_info((env), &ei_);                          \
      napi_throw_error((env), NULL,                                   \
                       ei_ && ei_->error_message ? ei_->error_message \
                                                 : "N-API call failed"); \
      return NULL;                                                    \
    }                                                                 \
  } while (0)

/* Throw Error(code) for rc < 0; returns 1 if thrown. */
static int throw_rc(napi_env env, int rc, mte_ctx* ctx, const char* what) {
  if (rc >= 0) return 0;
  char msg[768];
  snprintf(msg, sizeof msg, "%s: %s%s%s", what, mte_strerror(rc), ctx ? ": " : "",
           ctx ? mte_last_error(ctx) : "");
  napi_value m, err, code;
  napi_create_string_utf8(env, msg, NAPI_AUTO_LENGTH, &m);
  napi_create_error(env, NULL, m, &err);
  napi_create_int32(env, rc, &code);
  napi_set_named_property(env, err, "code", code);
  napi_throw(env, err);
  return 1;
}

typedef struct {
  mte_ctx* ctx;
  uint32_t n_keys; /* the context's property planes: the read-outs size their buffers by it */
  uint16_t* text;  /* readTexts: where mte_read_texts fills, kept from call to call */
  uint64_t text_cap;
  mte_seg* rows;   /* readSegmentLists: where mte_read_segment_lists fills, kept likewise */
  uint32_t* rprops;
  uint16_t* rtext;
  uint64_t rows_cap, rtext_cap;
} ctx_box;

static void ctx_finalize(napi_env env, void* data, void* hint) {
  (void)env;
  (void)hint;
  ctx_box* b = (ctx_box*)data;
  if (b->ctx) mte_destroy(b->ctx);
  free(b->text);
  free(b->rows);
  free(b->rprops);
  free(b->rtext);
  free(b);
}

static int get_args(napi_env env, napi_callback_info info, size_t want, napi_value* argv) {
  size_t argc = want;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok) return 0;
  if (argc < want) {
    napi_throw_type_error(env, NULL, "too few arguments");
    return 0;
  }
  return 1;
}

static ctx_box* get_box(napi_env env, napi_value v) {
  ctx_box* b = NULL;
  if (napi_get_value_external(env, v, (void**)&b) != napi_ok || !b || !b->ctx) {
    napi_throw_type_error(env, NULL, "expected a live engine context");
    return NULL;
  }
  return b;
}

static mte_ctx* get_ctx(napi_env env, napi_value v) {
  ctx_box* b = get_box(env, v);
  return b ? b->ctx : NULL;
}

/* The read-outs write the context's n_keys values per segment: a caller's nKeys
   that differs would size the property buffers wrongly (MTE_E_INVALID_ARG). */
static int check_nkeys(napi_env env, const ctx_box* b, uint32_t nk) {
  if (nk == b->n_keys) return 1;
  throw_rc(env, MTE_E_INVALID_ARG, b->ctx, "nKeys differs from the context's n_keys");
  return 0;
}

/* Raw bytes of any TypedArray (or null/undefined -> NULL, 0). */
static int get_bytes(napi_env env, napi_value v, void** data, size_t* nbytes) {
  napi_valuetype t;
  *data = NULL;
  *nbytes = 0;
  if (napi_typeof(env, v, &t) != napi_ok) return 0;
  if (t == napi_null || t == napi_undefined) return 1;
  bool is_ta = false;
  napi_is_typedarray(env, v, &is_ta);
  if (!is_ta) {
    napi_throw_type_error(env, NULL, "expected a TypedArray");
    return 0;
  }
  napi_typedarray_type tt;
  size_t len = 0, off = 0;
  napi_value ab;
  if (napi_get_typedarray_info(env, v, &tt, &len, data, &ab, &off) != napi_ok) return 0;
  size_t el = 1;
  switch (tt) {
    case napi_int8_array: case napi_uint8_array: case napi_uint8_clamped_array: el = 1; break;
    case napi_int16_array: case napi_uint16_array: el = 2; break;
    case napi_int32_array: case napi_uint32_array: case napi_float32_array: el = 4; break;
    default: el = 8; break;
  }
  *nbytes = len * el;
  return 1;
}

static napi_value js_abi_version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  NAPI_CALL(env, napi_create_int32(env, mte_abi_version(), &r));
  return r;
}

static napi_value js_strerror(napi_env env, napi_callback_info info) {
  napi_value argv[1], r;
  if (!get_args(env, info, 1, argv)) return NULL;
  int32_t code = 0;
  NAPI_CALL(env, napi_get_value_int32(env, argv[0], &code));
  NAPI_CALL(env, napi_create_string_utf8(env, mte_strerror(code), NAPI_AUTO_LENGTH, &r));
  return r;
}

/* create(device, nKeys, segCapacity) -> external ctx */
static napi_value js_create(napi_env env, napi_callback_info info) {
  napi_value argv[3], r;
  if (!get_args(env, info, 3, argv)) return NULL;
  mte_config cfg;
  memset(&cfg, 0, sizeof cfg);
  uint32_t nk = 0, cap = 0;
  NAPI_CALL(env, napi_get_value_int32(env, argv[0], &cfg.device));
  NAPI_CALL(env, napi_get_value_uint32(env, argv[1], &nk));
  NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &cap));
  cfg.n_keys = nk;
  cfg.seg_capacity = cap;
  mte_ctx* ctx = NULL;
  int rc = mte_create(&cfg, &ctx);
  if (throw_rc(env, rc, NULL, "mte_create")) return NULL;
  ctx_box* b = (ctx_box*)calloc(1, sizeof *b);
  if (!b) {
    mte_destroy(ctx);
    throw_rc(env, MTE_E_OOM, NULL, "mte_create");
    return NULL;
  }
  b->ctx = ctx;
  b->n_keys = nk;
  NAPI_CALL(env, napi_create_external(env, b, ctx_finalize, NULL, &r));
  return r;
}

static napi_value js_destroy(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return NULL;
  ctx_box* b = NULL;
  NAPI_CALL(env, napi_get_value_external(env, argv[0], (void**)&b));
  if (b && b->ctx) {
    mte_destroy(b->ctx);
    b->ctx = NULL;
  }
  return NULL;
}

static napi_value js_last_error(napi_env env, napi_callback_info info) {
  napi_value argv[1], r;
  if (!get_args(env, info, 1, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  NAPI_CALL(env, napi_create_string_utf8(env, mte_last_error(ctx), NAPI_AUTO_LENGTH, &r));
  return r;
}

/* loadDocs(ctx, inits Uint8Array(24*n), text Uint16Array, propsets Uint32Array, props Uint32Array) */
static napi_value js_load_docs(napi_env env, napi_callback_info info) {
  napi_value argv[5];
  if (!get_args(env, info, 5, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  void *inits, *text, *ps, *pe;
  size_t ni, nt, nps, npe;
  if (!get_bytes(env, argv[1], &inits, &ni) || !get_bytes(env, argv[2], &text, &nt) ||
      !get_bytes(env, argv[3], &ps, &nps) || !get_bytes(env, argv[4], &pe, &npe))
    return NULL;
  if (ni % sizeof(mte_doc_init) || nt % 2 || nps % sizeof(mte_propset) || npe % sizeof(mte_prop)) {
    throw_rc(env, MTE_E_INVALID_ARG, ctx, "loadDocs: buffer sizes");
    return NULL;
  }
  int rc = mte_load_docs(ctx, (uint32_t)(ni / sizeof(mte_doc_init)), (const mte_doc_init*)inits,
                         (const uint16_t*)text, nt / 2, (const mte_propset*)ps,
                         (uint32_t)(nps / sizeof(mte_propset)), (const mte_prop*)pe,
                         (uint32_t)(npe / sizeof(mte_prop)));
  throw_rc(env, rc, ctx, "mte_load_docs");
  return NULL;
}

/* loadSegments(ctx, offsets BigUint64Array(n+1), segs Uint8Array(32*k)) -> mte_load_segments */
static napi_value js_load_segments(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  void *offs, *segs;
  size_t no, ns;
  if (!get_bytes(env, argv[1], &offs, &no) || !get_bytes(env, argv[2], &segs, &ns)) return NULL;
  if (no % 8 || ns % sizeof(mte_seg)) {
    throw_rc(env, MTE_E_INVALID_ARG, ctx, "loadSegments: buffer sizes");
    return NULL;
  }
  int rc = mte_load_segments(ctx, (const uint64_t*)offs, (const mte_seg*)segs, ns / sizeof(mte_seg));
  throw_rc(env, rc, ctx, "mte_load_segments");
  return NULL;
}

/* submit(ctx, offsets BigUint64Array(n+1), ops Uint8Array(32*k), text Uint16Array,
 *        propsets Uint32Array, props Uint32Array) */
static napi_value js_submit(napi_env env, napi_callback_info info) {
  napi_value argv[6];
  if (!get_args(env, info, 6, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  void *off, *ops, *text, *ps, *pe;
  size_t noff, nops, nt, nps, npe;
  if (!get_bytes(env, argv[1], &off, &noff) || !get_bytes(env, argv[2], &ops, &nops) ||
      !get_bytes(env, argv[3], &text, &nt) || !get_bytes(env, argv[4], &ps, &nps) ||
      !get_bytes(env, argv[5], &pe, &npe))
    return NULL;
  if (noff < 8 || noff % 8 || nops % sizeof(mte_op) || nt % 2 || nps % sizeof(mte_propset) ||
      npe % sizeof(mte_prop)) {
    throw_rc(env, MTE_E_INVALID_ARG, ctx, "submit: buffer sizes");
    return NULL;
  }
  mte_batch b;
  memset(&b, 0, sizeof b);
  b.n_docs = (uint32_t)(noff / 8 - 1);
  b.op_offsets = (const uint64_t*)off;
  b.ops = (const mte_op*)ops;
  b.n_ops = nops / sizeof(mte_op);
  b.text = (const uint16_t*)text;
  b.text_units = nt / 2;
  b.propsets = (const mte_propset*)ps;
  b.n_propsets = (uint32_t)(nps / sizeof(mte_propset));
  b.props = (const mte_prop*)pe;
  b.n_props = (uint32_t)(npe / sizeof(mte_prop));
  throw_rc(env, mte_submit(ctx, &b), ctx, "mte_submit");
  return NULL;
}

#define SIMPLE(name, fn)                                                  \
  static napi_value name(napi_env env, napi_callback_info info) {        \
    napi_value argv[1];                                                   \
    if (!get_args(env, info, 1, argv)) return NULL;                       \
    mte_ctx* ctx = get_ctx(env, argv[0]);                                 \
    if (!ctx) return NULL;                                                \
    throw_rc(env, fn(ctx), ctx, #fn);                                     \
    return NULL;                                                          \
  }
SIMPLE(js_run, mte_run)
SIMPLE(js_sync, mte_sync)
SIMPLE(js_reset, mte_reset)

/* digest(ctx, out BigUint64Array(4*n)) */
static napi_value js_digest(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  void* out;
  size_t n;
  if (!get_bytes(env, argv[1], &out, &n)) return NULL;
  throw_rc(env, mte_digest(ctx, (uint64_t*)out, (uint32_t)(n / 32)), ctx, "mte_digest");
  return NULL;
}

/* docStatus(ctx, out Int32Array(n)) */
static napi_value js_doc_status(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  void* out;
  size_t n;
  if (!get_bytes(env, argv[1], &out, &n)) return NULL;
  throw_rc(env, mte_doc_status(ctx, (int32_t*)out, (uint32_t)(n / 4)), ctx, "mte_doc_status");
  return NULL;
}

static void set_i32(napi_env env, napi_value o, const char* k, int32_t v) {
  napi_value x;
  napi_create_int32(env, v, &x);
  napi_set_named_property(env, o, k, x);
}
static void set_f64(napi_env env, napi_value o, const char* k, double v) {
  napi_value x;
  napi_create_double(env, v, &x);
  napi_set_named_property(env, o, k, x);
}

static napi_value u32_array(napi_env env, const uint32_t* src, size_t n) {
  napi_value ab, ta;
  void* p = NULL;
  if (napi_create_arraybuffer(env, n * 4, &p, &ab) != napi_ok) return NULL;
  if (n) memcpy(p, src, n * 4);
  if (napi_create_typedarray(env, napi_uint32_array, n, ab, 0, &ta) != napi_ok) return NULL;
  return ta;
}

/* readDoc(ctx, doc, nKeys) -> {status, curSeq, minSeq, length, text, segLen, segKind, segProps} */
/* readSegments(ctx, doc, nKeys) -> {segs Uint8Array(32*n) (mte_seg, text_off into text),
   props Uint32Array(n*nKeys), text Uint16Array} (mte_read_segments) */
static napi_value js_read_segments(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  ctx_box* box = get_box(env, argv[0]);
  if (!box) return NULL;
  mte_ctx* ctx = box->ctx;
  uint32_t doc = 0, nk = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, argv[1], &doc));
  NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &nk));
  if (!check_nkeys(env, box, nk)) return NULL;
  mte_seg_list v;
  memset(&v, 0, sizeof v);
  if (throw_rc(env, mte_read_segments(ctx, doc, &v), ctx, "mte_read_segments")) return NULL;  // sizes
  napi_value o = NULL, ab_s, ab_p, ab_t, ts, tp, tt;
  void *ps, *pp, *pt;
  const size_t ns = (size_t)v.n_segs, nt = (size_t)v.n_text, npv = ns * nk;
  NAPI_CALL(env, napi_create_arraybuffer(env, ns * sizeof(mte_seg), &ps, &ab_s));
  NAPI_CALL(env, napi_create_arraybuffer(env, npv * 4, &pp, &ab_p));
  NAPI_CALL(env, napi_create_arraybuffer(env, nt * 2, &pt, &ab_t));
  v.segs = (mte_seg*)ps;
  v.props = nk ? (uint32_t*)pp : NULL;
  v.seg_cap = ns;
  v.text = (uint16_t*)pt;
  v.text_cap = nt;
  if (throw_rc(env, mte_read_segments(ctx, doc, &v), ctx, "mte_read_segments")) return NULL;
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, ns * sizeof(mte_seg), ab_s, 0, &ts));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, npv, ab_p, 0, &tp));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint16_array, nt, ab_t, 0, &tt));
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_set_named_property(env, o, "segs", ts);
  napi_set_named_property(env, o, "props", tp);
  napi_set_named_property(env, o, "text", tt);
  return o;
}

static napi_value js_read_doc(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  ctx_box* box = get_box(env, argv[0]);
  if (!box) return NULL;
  mte_ctx* ctx = box->ctx;
  uint32_t doc = 0, nk = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, argv[1], &doc));
  NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &nk));
  if (!check_nkeys(env, box, nk)) return NULL;
  mte_doc_view v;
  memset(&v, 0, sizeof v);
  if (throw_rc(env, mte_read_doc(ctx, doc, &v), ctx, "mte_read_doc")) return NULL;  // sizes
  const size_t nt = v.n_text, ns = v.n_segs;
  uint16_t* text = (uint16_t*)malloc((nt + 1) * 2);
  uint32_t* sl = (uint32_t*)malloc((ns + 1) * 4);
  uint32_t* sk = (uint32_t*)malloc((ns + 1) * 4);
  uint32_t* sp = (uint32_t*)malloc((ns * (nk ? nk : 1) + 1) * 4);
  napi_value o = NULL;
  if (!text || !sl || !sk || !sp) {
    throw_rc(env, MTE_E_OOM, ctx, "readDoc");
    goto done;
  }
  v.text = text;
  v.text_cap = (uint32_t)nt;
  v.seg_len = sl;
  v.seg_kind = sk;
  v.seg_props = nk ? sp : NULL;
  v.seg_cap = (uint32_t)ns;
  if (throw_rc(env, mte_read_doc(ctx, doc, &v), ctx, "mte_read_doc")) goto done;
  napi_create_object(env, &o);
  set_i32(env, o, "status", v.status);
  set_i32(env, o, "curSeq", v.cur_seq);
  set_i32(env, o, "minSeq", v.min_seq);
  set_f64(env, o, "length", (double)v.length);
  {
    napi_value s;
    napi_create_string_utf16(env, (const char16_t*)text, v.n_text, &s);
    napi_set_named_property(env, o, "text", s);
    napi_set_named_property(env, o, "segLen", u32_array(env, sl, v.n_segs));
    napi_set_named_property(env, o, "segKind", u32_array(env, sk, v.n_segs));
    napi_set_named_property(env, o, "segProps", u32_array(env, sp, nk ? (size_t)v.n_segs * nk : 0));
  }
done:
  free(text);
  free(sl);
  free(sk);
  free(sp);
  return o;
}

static napi_value js_stats(napi_env env, napi_callback_info info) {
  napi_value argv[1], o;
  if (!get_args(env, info, 1, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  mte_stats s;
  if (throw_rc(env, mte_stats_get(ctx, &s), ctx, "mte_stats_get")) return NULL;
  NAPI_CALL(env, napi_create_object(env, &o));
  set_f64(env, o, "opsApplied", (double)s.ops_applied);
  set_f64(env, o, "segsScanned", (double)s.segs_scanned);
  set_f64(env, o, "segsWritten", (double)s.segs_written);
  set_f64(env, o, "propWrites", (double)s.prop_writes);
  set_f64(env, o, "unitsInserted", (double)s.units_inserted);
  set_f64(env, o, "maxSegs", (double)s.max_segs);
  set_f64(env, o, "kernelMs", s.kernel_ms);
  set_f64(env, o, "algoBytes", s.algo_bytes);
  set_f64(env, o, "chunkScanned", (double)s.chunk_scanned);
  set_f64(env, o, "roundBytes", s.round_bytes);
  return o;
}

/* ---- node level over RCCL (mte_comm_*) ---- */
/* commUniqueId() -> Uint8Array(128) */
static napi_value js_comm_unique_id(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value ab, ta;
  void* p = NULL;
  NAPI_CALL(env, napi_create_arraybuffer(env, MTE_COMM_ID_BYTES, &p, &ab));
  if (throw_rc(env, mte_comm_unique_id((uint8_t*)p), NULL, "mte_comm_unique_id")) return NULL;
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, MTE_COMM_ID_BYTES, ab, 0, &ta));
  return ta;
}

/* commInit(ctx, world, rank, id Uint8Array(128)) */
static napi_value js_comm_init(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  int32_t world = 0, rank = 0;
  NAPI_CALL(env, napi_get_value_int32(env, argv[1], &world));
  NAPI_CALL(env, napi_get_value_int32(env, argv[2], &rank));
  void* id;
  size_t n;
  if (!get_bytes(env, argv[3], &id, &n)) return NULL;
  if (n != MTE_COMM_ID_BYTES) {
    throw_rc(env, MTE_E_INVALID_ARG, ctx, "commInit: id must be 128 bytes");
    return NULL;
  }
  throw_rc(env, mte_comm_init(ctx, world, rank, (const uint8_t*)id), ctx, "mte_comm_init");
  return NULL;
}

/* commShare(ctx, srcCtx) */
static napi_value js_comm_share(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  mte_ctx* src = get_ctx(env, argv[1]);
  if (!src) return NULL;
  throw_rc(env, mte_comm_share(ctx, src), ctx, "mte_comm_share");
  return NULL;
}

/* commBarrier(ctx) */
static napi_value js_comm_barrier(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  throw_rc(env, mte_comm_barrier(ctx), ctx, "mte_comm_barrier");
  return NULL;
}

/* commAllreduce(ctx, value, op 0 sum / 1 max) -> number */
static napi_value js_comm_allreduce(napi_env env, napi_callback_info info) {
  napi_value argv[3], r;
  if (!get_args(env, info, 3, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  double v = 0;
  int32_t op = 0;
  NAPI_CALL(env, napi_get_value_double(env, argv[1], &v));
  NAPI_CALL(env, napi_get_value_int32(env, argv[2], &op));
  if (throw_rc(env, mte_comm_allreduce_f64(ctx, &v, op), ctx, "mte_comm_allreduce_f64")) return NULL;
  NAPI_CALL(env, napi_create_double(env, v, &r));
  return r;
}

/* commGatherDigests(ctx, out BigUint64Array(world * docsPerRank * 4), docsPerRank) */
static napi_value js_comm_gather_digests(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  void* out;
  size_t n;
  if (!get_bytes(env, argv[1], &out, &n)) return NULL;
  uint32_t per = 0;
  NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &per));
  /* the byte length of the caller's array bounds the gather (mte.h) */
  throw_rc(env, mte_comm_gather_digests(ctx, (uint64_t*)out, (uint64_t)(n / sizeof(uint64_t)), per), ctx,
           "mte_comm_gather_digests");
  return NULL;
}

/* commDestroy(ctx) */
static napi_value js_comm_destroy(napi_env env, napi_callback_info info) {
  napi_value argv[1];
  if (!get_args(env, info, 1, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  throw_rc(env, mte_comm_destroy(ctx), ctx, "mte_comm_destroy");
  return NULL;
}

/* readDeltas(ctx, doc) -> Int32Array(5 n): op, kind, pos, len, removed per
   event (mte_read_deltas) */
static napi_value js_read_deltas(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t doc = 0;
  if (napi_get_value_uint32(env, argv[1], &doc) != napi_ok) {
    napi_throw_type_error(env, NULL, "doc must be a number");
    return NULL;
  }
  uint64_t n = 0;
  if (throw_rc(env, mte_read_deltas(ctx, doc, NULL, 0, &n), ctx, "mte_read_deltas")) return NULL;
  mte_delta* buf = (mte_delta*)malloc((size_t)(n ? n : 1) * sizeof(mte_delta));
  if (!buf) {
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  if (throw_rc(env, mte_read_deltas(ctx, doc, buf, n, &n), ctx, "mte_read_deltas")) {
    free(buf);
    return NULL;
  }
  napi_value out = u32_array(env, (const uint32_t*)buf, (size_t)n * 5);
  free(buf);
  return out;
}

/* setEventCapacity(ctx, perOp) (mte_set_event_capacity) */
static napi_value js_set_event_capacity(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t per = 0;
  if (napi_get_value_uint32(env, argv[1], &per) != napi_ok) {
    napi_throw_type_error(env, NULL, "setEventCapacity: the per-op capacity must be a number");
    return NULL;
  }
  throw_rc(env, mte_set_event_capacity(ctx, per), ctx, "mte_set_event_capacity");
  return NULL;
}

/* setRefCapacity(ctx, perDoc) (mte_set_ref_capacity) */
static napi_value js_set_ref_capacity(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t per = 0;
  if (napi_get_value_uint32(env, argv[1], &per) != napi_ok) {
    napi_throw_type_error(env, NULL, "setRefCapacity: the per-document capacity must be a number");
    return NULL;
  }
  throw_rc(env, mte_set_ref_capacity(ctx, per), ctx, "mte_set_ref_capacity");
  return NULL;
}

/* readRefs(ctx, doc, n[, transient]) -> Int32Array(n): positions of reference
   slots [0, n) (mte_read_refs; -1 detached / unused); transient true: as
   Transient references (mte_read_refs_transient) */
static napi_value js_read_refs(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  size_t argc = 4;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok) return NULL;
  if (argc < 3) {
    napi_throw_type_error(env, NULL, "too few arguments");
    return NULL;
  }
  bool transient = false;
  if (argc > 3 && napi_get_value_bool(env, argv[3], &transient) != napi_ok) transient = false;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t doc = 0, n = 0;
  if (napi_get_value_uint32(env, argv[1], &doc) != napi_ok || napi_get_value_uint32(env, argv[2], &n) != napi_ok) {
    napi_throw_type_error(env, NULL, "readRefs: doc and n must be numbers");
    return NULL;
  }
  int32_t* buf = (int32_t*)malloc((size_t)(n ? n : 1) * sizeof(int32_t));
  if (!buf) {
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  if (throw_rc(env, (transient ? mte_read_refs_transient : mte_read_refs)(ctx, doc, buf, n), ctx, "mte_read_refs")) {
    free(buf);
    return NULL;
  }
  napi_value out = u32_array(env, (const uint32_t*)buf, (size_t)n);
  free(buf);
  return out;
}

/* readRefOrder(ctx, doc, n) -> Float64Array(n): document order of reference
   slots [0, n) (mte_read_ref_order; -1 detached / unused) */
static napi_value js_read_ref_order(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  mte_ctx* ctx = get_ctx(env, argv[0]);
  if (!ctx) return NULL;
  uint32_t doc = 0, n = 0;
  if (napi_get_value_uint32(env, argv[1], &doc) != napi_ok || napi_get_value_uint32(env, argv[2], &n) != napi_ok) {
    napi_throw_type_error(env, NULL, "readRefOrder: doc and n must be numbers");
    return NULL;
  }
  int64_t* buf = (int64_t*)malloc((size_t)(n ? n : 1) * sizeof(int64_t));
  if (!buf) {
    napi_throw_error(env, NULL, "out of memory");
    return NULL;
  }
  if (throw_rc(env, mte_read_ref_order(ctx, doc, buf, n), ctx, "mte_read_ref_order")) {
    free(buf);
    return NULL;
  }
  napi_value ab, out;
  void* data = NULL;
  if (napi_create_arraybuffer(env, (size_t)n * 8, &data, &ab) != napi_ok ||
      napi_create_typedarray(env, napi_float64_array, n, ab, 0, &out) != napi_ok) {
    free(buf);
    napi_throw_error(env, NULL, "readRefOrder: allocation");
    return NULL;
  }
  for (uint32_t i = 0; i < n; i++) ((double*)data)[i] = (double)buf[i];
  free(buf);
  return out;
}

/* findTiles(ctx, queries, values, nKeys) -> {hits Int32Array(4n) (mte_tile_hit: pos,
   status, refType, 0), props Uint32Array(n * nKeys)}: mte_find_tiles over
   queries = Uint32Array(6n) (mte_tile_query: doc, pos, key, first, count,
   flags) and the value ids their (first, count) slices index.  The symbol is
   weak: an engine library without it (the CPU restatement the tests link this
   file against) loads, and findTiles throws code MTE_E_UNSUPPORTED. */
extern __typeof__(mte_find_tiles) mte_find_tiles __attribute__((weak));

static napi_value js_find_tiles(napi_env env, napi_callback_info info) {
  napi_value argv[4];
  if (!get_args(env, info, 4, argv)) return NULL;
  ctx_box* box = get_box(env, argv[0]);
  if (!box) return NULL;
  void *q = NULL, *vals = NULL;
  size_t qb = 0, vb = 0;
  uint32_t nk = 0;
  if (!get_bytes(env, argv[1], &q, &qb) || !get_bytes(env, argv[2], &vals, &vb)) return NULL;
  NAPI_CALL(env, napi_get_value_uint32(env, argv[3], &nk));
  if (!check_nkeys(env, box, nk)) return NULL;
  if (!mte_find_tiles) {
    throw_rc(env, MTE_E_UNSUPPORTED, NULL, "findTiles: this engine library has no mte_find_tiles");
    return NULL;
  }
  if (qb % sizeof(mte_tile_query) || vb % 4 || qb / sizeof(mte_tile_query) > 0xffffffffu || vb / 4 > 0xffffffffu) {
    throw_rc(env, MTE_E_INVALID_ARG, box->ctx, "findTiles: buffer sizes");
    return NULL;
  }
  const size_t n = qb / sizeof(mte_tile_query);
  napi_value o, ab_h, ab_p, th, tp;
  void *ph = NULL, *pp = NULL;
  NAPI_CALL(env, napi_create_arraybuffer(env, n * sizeof(mte_tile_hit), &ph, &ab_h));
  NAPI_CALL(env, napi_create_arraybuffer(env, n * nk * 4, &pp, &ab_p));
  if (throw_rc(env, mte_find_tiles(box->ctx, (const mte_tile_query*)q, (uint32_t)n, (const uint32_t*)vals,
                                   (uint32_t)(vb / 4), (mte_tile_hit*)ph, n && nk ? (uint32_t*)pp : NULL),
               box->ctx, "mte_find_tiles"))
    return NULL;
  NAPI_CALL(env, napi_create_typedarray(env, napi_int32_array, n * 4, ab_h, 0, &th));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n * nk, ab_p, 0, &tp));
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_set_named_property(env, o, "hits", th);
  napi_set_named_property(env, o, "props", tp);
  return o;
}

/* readTexts(ctx, queries) -> {info Uint32Array(8n) (mte_text_info: status,
   curSeq, minSeq, length, nUnits, 0, offset low, offset high), text
   Uint16Array(n_text)}: mte_read_texts over queries = Uint32Array(4n)
   (mte_text_query: doc, start, end, flags), one call (a second only when the
   context's fill buffer has to grow first).  Weak, as mte_find_tiles is. */
extern __typeof__(mte_read_texts) mte_read_texts __attribute__((weak));
extern __typeof__(mte_props_at) mte_props_at __attribute__((weak));

static napi_value js_read_texts(napi_env env, napi_callback_info info) {
  napi_value argv[2];
  if (!get_args(env, info, 2, argv)) return NULL;
  ctx_box* box = get_box(env, argv[0]);
  if (!box) return NULL;
  void* q = NULL;
  size_t qb = 0;
  if (!get_bytes(env, argv[1], &q, &qb)) return NULL;
  if (!mte_read_texts) {
    throw_rc(env, MTE_E_UNSUPPORTED, NULL, "readTexts: this engine library has no mte_read_texts");
    return NULL;
  }
  if (qb % sizeof(mte_text_query) || qb / sizeof(mte_text_query) > 0xffffffffu) {
    throw_rc(env, MTE_E_INVALID_ARG, box->ctx, "readTexts: buffer size");
    return NULL;
  }
  const size_t n = qb / sizeof(mte_text_query);
  napi_value o, ab_i, ab_t, ti, tt;
  void *pi = NULL, *pt = NULL;
  uint64_t nt = 0;
  NAPI_CALL(env, napi_create_arraybuffer(env, n * sizeof(mte_text_info), &pi, &ab_i));
  for (int pass = 0; pass < 2; pass++) {
    if (throw_rc(env, mte_read_texts(box->ctx, (const mte_text_query*)q, (uint32_t)n, (mte_text_info*)pi, box->text,
                                     box->text_cap, &nt),
                 box->ctx, "mte_read_texts"))
      return NULL;
    if (nt <= box->text_cap) break;
    if (pass == 1) { /* the documents cannot change between the two calls */
      throw_rc(env, MTE_E_STATE, box->ctx, "readTexts: the text grew between the size and the fill");
      return NULL;
    }
    free(box->text);
    box->text_cap = 0;
    box->text = (uint16_t*)malloc((size_t)nt * 4);
    if (!box->text) {
      throw_rc(env, MTE_E_OOM, box->ctx, "readTexts");
      return NULL;
    }
    box->text_cap = nt * 2;
  }
  NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)nt * 2, &pt, &ab_t));
  if (nt) memcpy(pt, box->text, (size_t)nt * 2);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n * 8, ab_i, 0, &ti));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint16_array, (size_t)nt, ab_t, 0, &tt));
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_set_named_property(env, o, "info", ti);
  napi_set_named_property(env, o, "text", tt);
  return o;
}

/* propsAt(ctx, queries, nKeys) -> {hits Int32Array(4n) (mte_pos_hit: status,
   found, kind, 0), props Uint32Array(n * nKeys)}: mte_props_at over queries =
   Uint32Array(2n) (mte_pos_query: doc, pos). */
static napi_value js_props_at(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  ctx_box* box = get_box(env, argv[0]);
  if (!box) return NULL;
  void* q = NULL;
  size_t qb = 0;
  uint32_t nk = 0;
  if (!get_bytes(env, argv[1], &q, &qb)) return NULL;
  NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &nk));
  if (!check_nkeys(env, box, nk)) return NULL;
  if (!mte_props_at) {
    throw_rc(env, MTE_E_UNSUPPORTED, NULL, "propsAt: this engine library has no mte_props_at");
    return NULL;
  }
  if (qb % sizeof(mte_pos_query) || qb / sizeof(mte_pos_query) > 0xffffffffu) {
    throw_rc(env, MTE_E_INVALID_ARG, box->ctx, "propsAt: buffer size");
    return NULL;
  }
  const size_t n = qb / sizeof(mte_pos_query);
  napi_value o, ab_h, ab_p, th, tp;
  void *ph = NULL, *pp = NULL;
  NAPI_CALL(env, napi_create_arraybuffer(env, n * sizeof(mte_pos_hit), &ph, &ab_h));
  NAPI_CALL(env, napi_create_arraybuffer(env, n * nk * 4, &pp, &ab_p));
  if (throw_rc(env, mte_props_at(box->ctx, (const mte_pos_query*)q, (uint32_t)n, (mte_pos_hit*)ph,
                                 n && nk ? (uint32_t*)pp : NULL),
               box->ctx, "mte_props_at"))
    return NULL;
  NAPI_CALL(env, napi_create_typedarray(env, napi_int32_array, n * 4, ab_h, 0, &th));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n * nk, ab_p, 0, &tp));
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_set_named_property(env, o, "hits", th);
  napi_set_named_property(env, o, "props", tp);
  return o;
}

/* readRefPositions(ctx, queries, wantOrder) -> {info Uint32Array(6n)
   (mte_ref_info: status, curSeq, minSeq, length, offset low, offset high), pos
   Int32Array(total), order Float64Array(total) with wantOrder}:
   mte_read_ref_positions over queries = Uint32Array(4n) (mte_ref_query: doc,
   first, count, flags), total = the sum of the counts.  Weak, as
   mte_find_tiles is. */
extern __typeof__(mte_read_ref_positions) mte_read_ref_positions __attribute__((weak));

static napi_value js_read_ref_positions(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  ctx_box* box = get_box(env, argv[0]);
  if (!box) return NULL;
  void* q = NULL;
  size_t qb = 0;
  bool want_order = false;
  if (!get_bytes(env, argv[1], &q, &qb)) return NULL;
  if (napi_get_value_bool(env, argv[2], &want_order) != napi_ok) want_order = false;
  if (!mte_read_ref_positions) {
    throw_rc(env, MTE_E_UNSUPPORTED, NULL, "readRefPositions: this engine library has no mte_read_ref_positions");
    return NULL;
  }
  if (qb % sizeof(mte_ref_query) || qb / sizeof(mte_ref_query) > 0xffffffffu) {
    throw_rc(env, MTE_E_INVALID_ARG, box->ctx, "readRefPositions: buffer size");
    return NULL;
  }
  const size_t n = qb / sizeof(mte_ref_query);
  uint64_t total = 0;
  for (size_t i = 0; i < n; i++) total += ((const mte_ref_query*)q)[i].count;
  napi_value o, ab_i, ab_p, ab_o, ti, tp, to;
  void *pi = NULL, *pp = NULL, *po = NULL;
  NAPI_CALL(env, napi_create_arraybuffer(env, n * sizeof(mte_ref_info), &pi, &ab_i));
  NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)total * 4, &pp, &ab_p));
  if (want_order) NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)total * 8, &po, &ab_o));
  if (throw_rc(env, mte_read_ref_positions(box->ctx, (const mte_ref_query*)q, (uint32_t)n, (mte_ref_info*)pi,
                                           (int32_t*)pp, want_order ? (int64_t*)po : NULL, total),
               box->ctx, "mte_read_ref_positions"))
    return NULL;
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n * 6, ab_i, 0, &ti));
  NAPI_CALL(env, napi_create_typedarray(env, napi_int32_array, (size_t)total, ab_p, 0, &tp));
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_set_named_property(env, o, "info", ti);
  napi_set_named_property(env, o, "pos", tp);
  if (want_order) { /* the keys as doubles, in place: readRefOrder's form */
    for (uint64_t i = 0; i < total; i++) {
      int64_t k;
      memcpy(&k, (const char*)po + 8 * i, 8);
      const double v = (double)k;
      memcpy((char*)po + 8 * i, &v, 8);
    }
    NAPI_CALL(env, napi_create_typedarray(env, napi_float64_array, (size_t)total, ab_o, 0, &to));
    napi_set_named_property(env, o, "order", to);
  }
  return o;
}

/* readSegmentLists(ctx, queries, nKeys) -> {info Uint32Array(10n)
   (mte_segs_info: status, curSeq, minSeq, nSegs, nText, 0, seg offset low,
   high, text offset low, high), segs Uint8Array(32 rows) (mte_seg records),
   props Uint32Array(rows * nKeys), text Uint16Array(n_text)}:
   mte_read_segment_lists over queries = Uint32Array(4n) (mte_segs_query: doc,
   mode, minSeq, flags), one call (a second only when the context's fill
   buffers have to grow first).  Weak, as mte_find_tiles is. */
extern __typeof__(mte_read_segment_lists) mte_read_segment_lists __attribute__((weak));

static napi_value js_read_segment_lists(napi_env env, napi_callback_info info) {
  napi_value argv[3];
  if (!get_args(env, info, 3, argv)) return NULL;
  ctx_box* box = get_box(env, argv[0]);
  if (!box) return NULL;
  void* q = NULL;
  size_t qb = 0;
  uint32_t nk = 0;
  if (!get_bytes(env, argv[1], &q, &qb)) return NULL;
  NAPI_CALL(env, napi_get_value_uint32(env, argv[2], &nk));
  if (!check_nkeys(env, box, nk)) return NULL;
  if (!mte_read_segment_lists) {
    throw_rc(env, MTE_E_UNSUPPORTED, NULL, "readSegmentLists: this engine library has no mte_read_segment_lists");
    return NULL;
  }
  if (qb % sizeof(mte_segs_query) || qb / sizeof(mte_segs_query) > 0xffffffffu) {
    throw_rc(env, MTE_E_INVALID_ARG, box->ctx, "readSegmentLists: buffer size");
    return NULL;
  }
  const size_t n = qb / sizeof(mte_segs_query);
  napi_value o, ab_i, ab_s, ab_p, ab_t, ti, ts, tp, tt;
  void *pi = NULL, *ps = NULL, *pp = NULL, *pt = NULL;
  uint64_t ns = 0, nt = 0;
  NAPI_CALL(env, napi_create_arraybuffer(env, n * sizeof(mte_segs_info), &pi, &ab_i));
  for (int pass = 0; pass < 2; pass++) {
    if (throw_rc(env, mte_read_segment_lists(box->ctx, (const mte_segs_query*)q, (uint32_t)n, (mte_segs_info*)pi,
                                             box->rows, box->rprops, box->rows_cap, box->rtext, box->rtext_cap, &ns, &nt),
                 box->ctx, "mte_read_segment_lists"))
      return NULL;
    if (ns <= box->rows_cap && nt <= box->rtext_cap) break;
    if (pass == 1) { /* the documents cannot change between the two calls */
      throw_rc(env, MTE_E_STATE, box->ctx, "readSegmentLists: the lists grew between the size and the fill");
      return NULL;
    }
    free(box->rows), free(box->rprops), free(box->rtext);
    box->rows_cap = box->rtext_cap = 0;
    box->rows = (mte_seg*)malloc((size_t)(2 * ns + 1) * sizeof(mte_seg));
    box->rprops = (uint32_t*)malloc((size_t)(2 * ns + 1) * (nk ? nk : 1) * 4);
    box->rtext = (uint16_t*)malloc((size_t)(2 * nt + 1) * 2);
    if (!box->rows || !box->rprops || !box->rtext) {
      free(box->rows), free(box->rprops), free(box->rtext);
      box->rows = NULL, box->rprops = NULL, box->rtext = NULL;
      throw_rc(env, MTE_E_OOM, box->ctx, "readSegmentLists");
      return NULL;
    }
    box->rows_cap = 2 * ns + 1;
    box->rtext_cap = 2 * nt + 1;
  }
  const size_t npv = (size_t)ns * nk;
  NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)ns * sizeof(mte_seg), &ps, &ab_s));
  NAPI_CALL(env, napi_create_arraybuffer(env, npv * 4, &pp, &ab_p));
  NAPI_CALL(env, napi_create_arraybuffer(env, (size_t)nt * 2, &pt, &ab_t));
  if (ns) memcpy(ps, box->rows, (size_t)ns * sizeof(mte_seg));
  if (npv) memcpy(pp, box->rprops, npv * 4);
  if (nt) memcpy(pt, box->rtext, (size_t)nt * 2);
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, n * 10, ab_i, 0, &ti));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint8_array, (size_t)ns * sizeof(mte_seg), ab_s, 0, &ts));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint32_array, npv, ab_p, 0, &tp));
  NAPI_CALL(env, napi_create_typedarray(env, napi_uint16_array, (size_t)nt, ab_t, 0, &tt));
  NAPI_CALL(env, napi_create_object(env, &o));
  napi_set_named_property(env, o, "info", ti);
  napi_set_named_property(env, o, "segs", ts);
  napi_set_named_property(env, o, "props", tp);
  napi_set_named_property(env, o, "text", tt);
  return o;
}

static napi_value init(napi_env env, napi_value exports) {
  const napi_property_descriptor d[] = {
      {"abiVersion", NULL, js_abi_version, NULL, NULL, NULL, napi_enumerable, NULL},
      {"strerror", NULL, js_strerror, NULL, NULL, NULL, napi_enumerable, NULL},
      {"create", NULL, js_create, NULL, NULL, NULL, napi_enumerable, NULL},
      {"destroy", NULL, js_destroy, NULL, NULL, NULL, napi_enumerable, NULL},
      {"lastError", NULL, js_last_error, NULL, NULL, NULL, napi_enumerable, NULL},
      {"loadDocs", NULL, js_load_docs, NULL, NULL, NULL, napi_enumerable, NULL},
      {"loadSegments", NULL, js_load_segments, NULL, NULL, NULL, napi_enumerable, NULL},
      {"submit", NULL, js_submit, NULL, NULL, NULL, napi_enumerable, NULL},
      {"run", NULL, js_run, NULL, NULL, NULL, napi_enumerable, NULL},
      {"sync", NULL, js_sync, NULL, NULL, NULL, napi_enumerable, NULL},
      {"reset", NULL, js_reset, NULL, NULL, NULL, napi_enumerable, NULL},
      {"digest", NULL, js_digest, NULL, NULL, NULL, napi_enumerable, NULL},
      {"docStatus", NULL, js_doc_status, NULL, NULL, NULL, napi_enumerable, NULL},
      {"readDoc", NULL, js_read_doc, NULL, NULL, NULL, napi_enumerable, NULL},
      {"readSegments", NULL, js_read_segments, NULL, NULL, NULL, napi_enumerable, NULL},
      {"stats", NULL, js_stats, NULL, NULL, NULL, napi_enumerable, NULL},
      {"commUniqueId", NULL, js_comm_unique_id, NULL, NULL, NULL, napi_enumerable, NULL},
      {"commInit", NULL, js_comm_init, NULL, NULL, NULL, napi_enumerable, NULL},
      {"commShare", NULL, js_comm_share, NULL, NULL, NULL, napi_enumerable, NULL},
      {"commBarrier", NULL, js_comm_barrier, NULL, NULL, NULL, napi_enumerable, NULL},
      {"commAllreduce", NULL, js_comm_allreduce, NULL, NULL, NULL, napi_enumerable, NULL},
      {"commGatherDigests", NULL, js_comm_gather_digests, NULL, NULL, NULL, napi_enumerable, NULL},
      {"commDestroy", NULL, js_comm_destroy, NULL, NULL, NULL, napi_enumerable, NULL},
      {"readDeltas", NULL, js_read_deltas, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setEventCapacity", NULL, js_set_event_capacity, NULL, NULL, NULL, napi_enumerable, NULL},
      {"setRefCapacity", NULL, js_set_ref_capacity, NULL, NULL, NULL, napi_enumerable, NULL},
      {"readRefs", NULL, js_read_refs, NULL, NULL, NULL, napi_enumerable, NULL},
      {"readRefOrder", NULL, js_read_ref_order, NULL, NULL, NULL, napi_enumerable, NULL},
      /* not enumerable: Object.keys() of the addon stays the list of functions
         every engine library serves; findTiles depends on the library (above) */
      {"findTiles", NULL, js_find_tiles, NULL, NULL, NULL, napi_default, NULL},
      {"readTexts", NULL, js_read_texts, NULL, NULL, NULL, napi_default, NULL},
      {"propsAt", NULL, js_props_at, NULL, NULL, NULL, napi_default, NULL},
      {"readRefPositions", NULL, js_read_ref_positions, NULL, NULL, NULL, napi_default, NULL},
      {"readSegmentLists", NULL, js_read_segment_lists, NULL, NULL, NULL, napi_default, NULL},
  };
  if (napi_define_properties(env, exports, sizeof d / sizeof d[0], d) != napi_ok) return NULL;
  return exports;
}

NAPI_MODULE(NODE_GYP_MODULE_NAME, init)
