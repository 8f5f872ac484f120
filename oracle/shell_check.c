/*
 * shell_check.c — the API shell of the four CPU restatements under ASan and
 * UBSan (`make -C oracle check-san`; TEST INFRASTRUCTURE, run by hand on a CPU).
 *
 * For orc_, ort_, oti_ and och_ alike: create / load_docs / load_segments /
 * apply_batch / every read-out / destroy on hand-made two-document inputs,
 * every refusal tests/test_oracle_shell.py pins, and a reload after each
 * refused load.  Exits 0 when every call answered as expected and the
 * sanitizers (leak check included) found nothing.
 */
#include <stdio.h>
#include <string.h>

#include "chunked.h"
#include "oracle.h"
#include "titems.h"
#include "tree.h"

static int failures;
#define CHECK(what, got, want)                                                              \
  do {                                                                                      \
    const int g_ = (got), w_ = (want);                                                      \
    if (g_ != w_) {                                                                         \
      failures++;                                                                           \
      fprintf(stderr, "%s:%d: %s: %s = %d, expected %d\n", __FILE__, __LINE__, pre, what, g_, w_); \
    }                                                                                       \
  } while (0)

#define INV MTE_E_INVALID_ARG
#define N_KEYS 2
#define NEWCALC MTE_DOC_NEW_LENGTH_CALC
#define LOCAL (MTE_DOC_NEW_LENGTH_CALC | MTE_DOC_LOCAL_CLIENT)

static const uint16_t TEXT[11] = {'h', 'e', 'l', 'l', 'o', ' ', 'w', 'o', 'r', 'l', 'd'};
static const uint16_t BATCH_TEXT[2] = {'x', 'y'};
static const mte_propset PROPSETS[1] = {{0, 1}};
static const mte_prop PROPS[1] = {{1, 7}};

static mte_op op(uint8_t type, int32_t seq, int32_t pos1, int32_t pos2, uint32_t a, uint32_t b, uint16_t flags,
                 uint8_t client) {
  mte_op o;
  memset(&o, 0, sizeof o);
  o.seq = seq;
  o.type = type;
  o.client = client;
  o.flags = flags;
  o.pos1 = pos1;
  o.pos2 = pos2;
  o.a = a;
  o.b = b;
  return o;
}

/* n0 records for document 0, the rest of n for document 1 */
static mte_batch batch(const mte_op* ops, uint64_t n0, uint64_t n, uint64_t* offs) {
  offs[0] = 0;
  offs[1] = n0;
  offs[2] = n;
  mte_batch b;
  memset(&b, 0, sizeof b);
  b.n_docs = 2;
  b.op_offsets = offs;
  b.ops = ops;
  b.n_ops = n;
  b.text = BATCH_TEXT;
  b.text_units = 2;
  b.propsets = PROPSETS;
  b.n_propsets = 1;
  b.props = PROPS;
  b.n_props = 1;
  return b;
}

static void inits(mte_doc_init* d, uint32_t flags0) {
  memset(d, 0, 2 * sizeof *d);
  d[0].text_len = 5;
  d[0].flags = flags0;
  d[0].propset = MTE_NO_PROPS;
  d[1].text_off = 5;
  d[1].text_len = 6;
  d[1].flags = NEWCALC;
  d[1].propset = 0;
}

static void segs(mte_seg* s) {
  memset(s, 0, 2 * sizeof *s);
  s[0].len = 5;
  s[0].removed_seq = MTE_NOT_REMOVED;
  s[0].client = -1;
  s[0].propset = MTE_NO_PROPS;
  s[1].text_off = 5;
  s[1].len = 6;
  s[1].removed_seq = MTE_NOT_REMOVED;
  s[1].client = -1;
  s[1].propset = 0;
}

/* One restatement, start to end.  LOCAL_RULES: it validates local records
 * (orc, oti); the others take such a batch and stop the document.  EXTRA: the
 * read-outs only it has. */
#define DRIVE(P, LOCAL_RULES, EXTRA)                                                                          \
  static void drive_##P(void) {                                                                               \
    const char* pre = #P;                                                                                     \
    P##_ctx* c = NULL;                                                                                        \
    mte_doc_init di[2];                                                                                       \
    mte_seg sg[2];                                                                                            \
    uint64_t offs[3], so[3] = {0, 1, 2}, so_bad[3] = {0, 1, 1};                                               \
    mte_op ops[4];                                                                                            \
    mte_batch b;                                                                                              \
    CHECK("create n_keys > max", P##_create(MTE_MAX_KEYS + 1, &c), INV);                                      \
    CHECK("create", P##_create(N_KEYS, &c), MTE_OK);                                                          \
    /* refused loads, each followed by a good one */                                                          \
    inits(di, NEWCALC);                                                                                       \
    di[0].text_len = 12;                                                                                      \
    CHECK("initial text out of range", P##_load_docs(c, 2, di, TEXT, 11, PROPSETS, 1, PROPS, 1), INV);        \
    inits(di, NEWCALC);                                                                                       \
    di[0].propset = 1;                                                                                        \
    CHECK("initial propset out of range", P##_load_docs(c, 2, di, TEXT, 11, PROPSETS, 1, PROPS, 1), INV);     \
    inits(di, NEWCALC);                                                                                       \
    CHECK("load_docs", P##_load_docs(c, 2, di, TEXT, 11, PROPSETS, 1, PROPS, 1), MTE_OK);                     \
    segs(sg);                                                                                                 \
    CHECK("seg_offsets not ending at n_segs", P##_load_segments(c, so_bad, sg, 2), INV);                      \
    for (int bad = 0; bad < 5; bad++) {                                                                       \
      static const char* const what[] = {"marker of length 2", "text past the load text", "client >= max",   \
                                         "removed without removers", "bad segment propset"};                  \
      segs(sg);                                                                                               \
      if (bad == 0) sg[1].kind = 1, sg[1].len = 2;                                                            \
      if (bad == 1) sg[1].text_off = 8;                                                                       \
      if (bad == 2) sg[1].client = MTE_MAX_CLIENTS;                                                           \
      if (bad == 3) sg[1].removed_seq = 3;                                                                    \
      if (bad == 4) sg[1].propset = 1;                                                                        \
      CHECK(what[bad], P##_load_segments(c, so, sg, 2), INV);                                                 \
      CHECK("reload", P##_load_docs(c, 2, di, TEXT, 11, PROPSETS, 1, PROPS, 1), MTE_OK);                      \
    }                                                                                                         \
    segs(sg);                                                                                                 \
    CHECK("load_segments", P##_load_segments(c, so, sg, 2), MTE_OK);                                          \
    /* refused batches, table bounds: every restatement */                                                    \
    ops[0] = ops[1] = op(MTE_OP_REMOVE, 1, 0, 1, 0, 0, MTE_F_MSG_END, 1);                                     \
    b = batch(ops, 1, 2, offs);                                                                               \
    b.n_ops = 1;                                                                                              \
    CHECK("op_offsets not ending at n_ops", P##_apply_batch(c, &b, 2), INV);                                  \
    ops[0] = op(MTE_OP_INSERT, 1, 0, 2, 1, MTE_NO_PROPS, MTE_F_MSG_END, 1);                                   \
    b = batch(ops, 1, 1, offs);                                                                               \
    CHECK("insert text out of range", P##_apply_batch(c, &b, 2), INV);                                        \
    ops[0] = op(MTE_OP_INSERT, 1, 0, 2, 0, 1, MTE_F_MSG_END, 1);                                              \
    CHECK("insert propset out of range", P##_apply_batch(c, &b, 2), INV);                                     \
    ops[0] = op(MTE_OP_ANNOTATE, 1, 0, 2, 1, 0, MTE_F_MSG_END, 1);                                            \
    CHECK("annotate propset out of range", P##_apply_batch(c, &b, 2), INV);                                   \
    /* local-record rules: a refusal (orc, oti) or a stopped document */                                      \
    for (int bad = 0; bad < 6; bad++) {                                                                       \
      static const char* const what[] = {"type above RELPOS", "RBKEY outside a rollback", "local record, no local client", \
                                         "ack pos1 > pos2", "REF without DOC_REFS", "RELPOS as last record"};  \
      inits(di, bad == 1 || bad == 3 || bad == 4 ? LOCAL : NEWCALC);                                          \
      CHECK("reload", P##_load_docs(c, 2, di, TEXT, 11, PROPSETS, 1, PROPS, 1), MTE_OK);                      \
      uint64_t n = 1;                                                                                         \
      if (bad == 0) ops[0] = op(MTE_OP_RELPOS + 1, 1, 0, 0, 0, 0, MTE_F_MSG_END, 1);                          \
      if (bad == 1) ops[0] = op(MTE_OP_RBKEY, 1, 0, 0, 0, 0, MTE_F_LOCAL, 0);                                 \
      if (bad == 2) ops[0] = op(MTE_OP_REMOVE, 1, 0, 1, 0, 0, MTE_F_LOCAL | MTE_F_MSG_END, 0);                \
      if (bad == 3) {                                                                                         \
        ops[0] = op(MTE_OP_REMOVE, 1, 0, 1, 0, 0, MTE_F_LOCAL, 0);                                            \
        ops[1] = op(MTE_OP_ACK, 1, 2, 1, 0, 0, MTE_F_MSG_END, 0);                                             \
        n = 2;                                                                                                \
      }                                                                                                       \
      if (bad == 4) ops[0] = op(MTE_OP_REF, 0, 1, 0, 0, 0, MTE_F_LOCAL, 0);                                   \
      if (bad == 5) {                                                                                         \
        ops[0] = op(MTE_OP_REMOVE, 1, 0, 1, 0, 0, MTE_F_MSG_END, 1);                                          \
        ops[1] = op(MTE_OP_RELPOS, 0, 0, 0, 0, 0, MTE_RP_POS1, 1);                                            \
        n = 2;                                                                                                \
      }                                                                                                       \
      b = batch(ops, n, n, offs);                                                                             \
      CHECK(what[bad], P##_apply_batch(c, &b, 2), (LOCAL_RULES) ? INV : MTE_OK);                              \
    }                                                                                                         \
    /* a good batch on a fresh load, then every read-out */                                                   \
    inits(di, NEWCALC);                                                                                       \
    CHECK("reload", P##_load_docs(c, 2, di, TEXT, 11, PROPSETS, 1, PROPS, 1), MTE_OK);                        \
    CHECK("apply_batch, one thread, no records",                                                              \
          P##_apply_batch(c, &(mte_batch){.n_docs = 2, .op_offsets = (uint64_t[3]){0, 0, 0}}, 1), MTE_OK);    \
    ops[0] = op(MTE_OP_INSERT, 1, 2, 2, 0, 0, MTE_F_MSG_END, 1);                                              \
    ops[1] = op(MTE_OP_ANNOTATE, 2, 0, 4, 0, 0, MTE_F_MSG_END, 1);                                            \
    ops[2] = op(MTE_OP_REMOVE, 1, 1, 3, 0, 0, MTE_F_MSG_END, 1);                                              \
    ops[3] = op(MTE_OP_INSERT, 2, 0, 1, 0, MTE_NO_PROPS, MTE_F_MSG_END | MTE_F_MARKER, 1);                    \
    b = batch(ops, 2, 4, offs);                                                                               \
    CHECK("apply_batch", P##_apply_batch(c, &b, 2), MTE_OK);                                                  \
    int32_t st[2] = {1, 1};                                                                                   \
    CHECK("doc_status", P##_doc_status(c, st, 2), MTE_OK);                                                    \
    CHECK("status 0", st[0], 0);                                                                              \
    CHECK("status 1", st[1], 0);                                                                              \
    uint64_t dg[8];                                                                                           \
    CHECK("digest", P##_digest(c, dg, 2), MTE_OK);                                                            \
    CHECK("digest units 0", (int)dg[0], 7);                                                                   \
    CHECK("digest units 1", (int)dg[4], 5);                                                                   \
    for (uint32_t d = 0; d < 2; d++) {                                                                        \
      /* sizes first, then short buffers, then full ones */                                                   \
      uint16_t text[16];                                                                                      \
      uint32_t len[8], kind[8], props[8 * N_KEYS], nsegs = 0;                                                 \
      mte_doc_view v;                                                                                         \
      memset(&v, 0, sizeof v);                                                                                \
      CHECK("read_doc sizes", P##_read_doc(c, d, &v), MTE_OK);                                                \
      CHECK("read_doc length", (int)v.length, d ? 5 : 7);                                                     \
      v.text = text, v.text_cap = 1, v.seg_len = len, v.seg_kind = kind, v.seg_props = props, v.seg_cap = 1; \
      CHECK("read_doc short", P##_read_doc(c, d, &v), MTE_OK);                                                \
      v.text_cap = 16, v.seg_cap = 8;                                                                         \
      CHECK("read_doc", P##_read_doc(c, d, &v), MTE_OK);                                                      \
      CHECK("read_doc fits", v.n_segs <= 8 && v.n_text <= 16, 1);                                             \
      mte_seg out[8];                                                                                         \
      mte_seg_list l;                                                                                         \
      memset(&l, 0, sizeof l);                                                                                \
      CHECK("read_segments sizes", P##_read_segments(c, d, &l), MTE_OK);                                      \
      l.segs = out, l.props = props, l.seg_cap = 1, l.text = text, l.text_cap = 1;                            \
      CHECK("read_segments short", P##_read_segments(c, d, &l), MTE_OK);                                      \
      l.seg_cap = 8, l.text_cap = 16;                                                                         \
      CHECK("read_segments", P##_read_segments(c, d, &l), MTE_OK);                                            \
      CHECK("read_segments fits", l.n_segs <= 8 && l.n_text <= 16, 1);                                        \
      CHECK("doc_nsegs", P##_doc_nsegs(c, d, &nsegs), MTE_OK);                                                \
      CHECK("doc_nsegs == read_segments", (int)nsegs, (int)l.n_segs);                                         \
      EXTRA                                                                                                   \
    }                                                                                                         \
    CHECK("read_doc past the documents", P##_read_doc(c, 2, &(mte_doc_view){0}), INV);                        \
    mte_stats stats;                                                                                          \
    CHECK("stats_get", P##_stats_get(c, &stats), MTE_OK);                                                     \
    CHECK("ops applied", (int)stats.ops_applied, 4);                                                          \
    CHECK("destroy", P##_destroy(c), MTE_OK);                                                                 \
  }

#define SHAPE(P)                                               \
  {                                                            \
    char shape[64];                                            \
    CHECK("doc_shape", P##_doc_shape(c, d, shape, 64) >= 0, 1); \
    CHECK("doc_shape short", P##_doc_shape(c, d, shape, 2) >= 0, 1); \
  }
#define REFS(P)                                                                \
  {                                                                            \
    mte_delta dl[4];                                                           \
    uint64_t n_dl = 9;                                                         \
    int32_t pos[2];                                                            \
    int64_t key[2];                                                            \
    CHECK("read_deltas", P##_read_deltas(c, d, dl, 4, &n_dl), MTE_OK);          \
    CHECK("no events", (int)n_dl, 0);                                          \
    CHECK("read_refs", P##_read_refs(c, d, pos, 2), MTE_OK);                    \
    CHECK("read_refs_transient", P##_read_refs_transient(c, d, pos, 2), MTE_OK); \
    CHECK("read_ref_order", P##_read_ref_order(c, d, key, 2), MTE_OK);          \
    CHECK("no reference", pos[0] == -1 && key[1] == -1, 1);                    \
  }

DRIVE(orc, 1, REFS(orc))
DRIVE(ort, 0, SHAPE(ort))
DRIVE(oti, 1, SHAPE(oti) REFS(oti) CHECK("set_limit", oti_set_limit(c, 4), INV); CHECK("set_limit", oti_set_limit(c, 1024), MTE_OK);)
DRIVE(och, 0, )

int main(void) {
  drive_orc();
  drive_ort();
  drive_oti();
  drive_och();
  printf("shell_check: %d failure%s\n", failures, failures == 1 ? "" : "s");
  return failures ? 1 : 0;
}
