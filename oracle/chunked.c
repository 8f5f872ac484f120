/*
 * chunked.c — the flat restatement (oracle.c) with a chunk index, for
 * documents of millions of segments (TEST INFRASTRUCTURE: config 5's full-size
 * checker and CPU baseline).
 *
 * oracle.c recomputes every perspective length and prefix per op, O(S) per op:
 * at config 5 (2^20 segments per document) that is a strawman.  This file keeps
 * the same document -- the same segments, split on op boundaries, never
 * append-merged, tombstones dropped when removedSeq <= minSeq -- as a list of
 * chunks of at most CH segments, and per client a column of chunk lengths in
 * that client's perspective: the flat counterpart of the per-client entries of
 * PartialSequenceLengths.getPartialLength (partialLengths.ts:667-702) at chunk
 * granularity, as the GPU's chunk pass keeps them.  An op of
 * client c with refSeq r resolves its position on column c (rebuilt when c's
 * refSeq or the window's minSeq changed since it was built), then applies the
 * flat rules of oracle.c (doc_split_at, the insert slot, the range marks) to
 * the chunk(s) it lands in; per op O(chunks + CH), not O(S).
 *
 * Why a column stays exact across other clients' ops (new length calculation,
 * mergeTree.ts:1003-1026): an op (seq s, client c) makes a segment of seq s --
 * visible only to c in every held perspective, whose refSeqs are < s -- or
 * marks removals at s > every held refSeq, or adds c to removedClientIds; none
 * of that changes L(x; r', c') for c' != c.  Splits move no length between
 * chunks.  Only column c moves, by the op's own length change.
 *
 * Only remote (observer) replay with the new length calculation: the config-5
 * documents.  Other documents are refused (MTE_E_UNSUPPORTED).
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg load it.
 *
 * The replay rules end at the API banner below; under it is glue over the shell
 * the four restatements share (orc_shell.h: arena, load tables, load and batch
 * validation, thread pool, read-out emitters).  What this file does differently
 * from the other three stands there once, at its call site, with a comment.
 */
#include <limits.h>

#include "chunked.h"
#include "orc_shell.h"

#define NONE_SEQ ORC_NONE_SEQ
#define CH 512           /* segments per chunk at most */
#define CH_FILL 256      /* segments per chunk after a rebuild */

typedef struct {
  int32_t len, seq, rseq;
  uint32_t rmask;
  int32_t cli;
  uint32_t kind, toff;
  uint32_t props[MTE_MAX_KEYS];
} cseg;

typedef struct {
  cseg s[CH];
  uint32_t n;
} chunk;

typedef struct {
  chunk** ch;
  uint32_t nch, cap_ch;
  int32_t min_seq, cur_seq;
  uint32_t flags;
  int32_t status;
  /* per client: the perspective (refSeq, minSeq) column `col` holds, and the
   * chunk lengths in it (undefined leaves count 0) */
  int32_t col_r[MTE_MAX_CLIENTS], col_m[MTE_MAX_CLIENTS];
  int32_t* col[MTE_MAX_CLIENTS];
  uint32_t col_cap;
  uint64_t ops, rebuilds;
  mte_doc_init init;
  uint32_t init_props[MTE_MAX_KEYS];
} __attribute__((aligned(128))) cdoc;

struct och_ctx {
  uint32_t n_keys, n_docs;
  cdoc* docs;
  orc_arena arena;
  orc_load_tables load;
};

/* ---- lengths (oracle.c leaf_len, new calculation) -------------------------- */

static inline int32_t leaf_len(const cseg* s, int32_t r, int c, int32_t m) {
  if (s->rseq != NONE_SEQ) {
    if (s->rseq <= m) return -1;
    if (s->rseq <= r || ((s->rmask >> c) & 1u)) return 0;
  }
  return (s->seq <= r || s->cli == c) ? s->len : 0;
}

static int32_t chunk_len(const chunk* k, int32_t r, int c, int32_t m) {
  int32_t t = 0;
  for (uint32_t i = 0; i < k->n; i++) {
    const int32_t l = leaf_len(&k->s[i], r, c, m);
    if (l > 0) t += l;
  }
  return t;
}

/* ---- chunk list ---------------------------------------------------------------- */

static int cols_reserve(cdoc* d, uint32_t need) {
  if (need <= d->col_cap) return MTE_OK;
  uint32_t nc = d->col_cap ? d->col_cap : 64;
  while (nc < need) nc *= 2;
  for (int c = 0; c < MTE_MAX_CLIENTS; c++) {
    int32_t* x = (int32_t*)realloc(d->col[c], (size_t)nc * sizeof(int32_t));
    if (!x) return MTE_E_OOM;
    d->col[c] = x;
  }
  d->col_cap = nc;
  return MTE_OK;
}

static int chunks_reserve(cdoc* d, uint32_t need) {
  if (need > d->cap_ch) {
    uint32_t nc = d->cap_ch ? d->cap_ch : 16;
    while (nc < need) nc *= 2;
    chunk** x = (chunk**)realloc(d->ch, (size_t)nc * sizeof(chunk*));
    if (!x) return MTE_E_OOM;
    d->ch = x;
    d->cap_ch = nc;
  }
  return cols_reserve(d, need);
}

static void invalidate_cols(cdoc* d) {
  for (int c = 0; c < MTE_MAX_CLIENTS; c++) d->col_r[c] = INT32_MIN;
}

/* column c for (r, m): rebuilt from the chunks when it holds another perspective */
static void ensure_col(cdoc* d, int c, int32_t r, int32_t m) {
  if (d->col_r[c] == r && d->col_m[c] == m) return;
  for (uint32_t k = 0; k < d->nch; k++) d->col[c][k] = chunk_len(d->ch[k], r, c, m);
  d->col_r[c] = r;
  d->col_m[c] = m;
  d->rebuilds++;
}

/* split chunk k in two halves (it is full); every valid column gets the halves' lengths */
static int split_chunk(cdoc* d, uint32_t k) {
  int rc = chunks_reserve(d, d->nch + 1);
  if (rc) return rc;
  chunk* a = d->ch[k];
  chunk* b = (chunk*)malloc(sizeof(chunk));
  if (!b) return MTE_E_OOM;
  const uint32_t h = a->n / 2;
  b->n = a->n - h;
  memcpy(b->s, a->s + h, (size_t)b->n * sizeof(cseg));
  a->n = h;
  memmove(d->ch + k + 2, d->ch + k + 1, (size_t)(d->nch - k - 1) * sizeof(chunk*));
  d->ch[k + 1] = b;
  for (int c = 0; c < MTE_MAX_CLIENTS; c++) {
    if (d->col_r[c] == INT32_MIN) continue;
    memmove(d->col[c] + k + 2, d->col[c] + k + 1, (size_t)(d->nch - k - 1) * sizeof(int32_t));
    const int32_t la = chunk_len(a, d->col_r[c], c, d->col_m[c]);
    d->col[c][k + 1] = d->col[c][k] - la;
    d->col[c][k] = la;
  }
  d->nch++;
  return MTE_OK;
}

/* open a slot at index i of chunk k (splitting a full chunk first); returns
 * the slot's (chunk, index) through *k / *i */
static int open_slot(cdoc* d, uint32_t* k, uint32_t* i) {
  if (d->ch[*k]->n == CH) {
    int rc = split_chunk(d, *k);
    if (rc) return rc;
    const uint32_t h = d->ch[*k]->n;
    if (*i > h) {
      *i -= h;
      (*k)++;
    }
  }
  chunk* ck = d->ch[*k];
  memmove(ck->s + *i + 1, ck->s + *i, (size_t)(ck->n - *i) * sizeof(cseg));
  ck->n++;
  return MTE_OK;
}

/* rebuild the chunk list: drop tombstones at or below minSeq (setMinSeq's
 * zamboni, content-equivalent, oracle.c doc_compact), CH_FILL per chunk */
static int relayout(cdoc* d) {
  uint32_t total = 0;
  for (uint32_t k = 0; k < d->nch; k++) total += d->ch[k]->n;
  cseg* all = (cseg*)malloc((size_t)(total ? total : 1) * sizeof(cseg));
  if (!all) return MTE_E_OOM;
  uint32_t w = 0;
  for (uint32_t k = 0; k < d->nch; k++) {
    const chunk* ck = d->ch[k];
    for (uint32_t i = 0; i < ck->n; i++)
      if (!(ck->s[i].rseq != NONE_SEQ && ck->s[i].rseq <= d->min_seq)) all[w++] = ck->s[i];
  }
  const uint32_t need = w ? (w + CH_FILL - 1) / CH_FILL : 1;
  for (uint32_t k = need; k < d->nch; k++) free(d->ch[k]);
  int rc = chunks_reserve(d, need);
  if (rc) {
    free(all);
    return rc;
  }
  for (uint32_t k = d->nch; k < need; k++) {
    d->ch[k] = (chunk*)malloc(sizeof(chunk));
    if (!d->ch[k]) {
      free(all);
      return MTE_E_OOM;
    }
  }
  d->nch = need;
  for (uint32_t k = 0; k < need; k++) {
    const uint32_t a = k * CH_FILL, b = a + CH_FILL < w ? a + CH_FILL : w;
    d->ch[k]->n = b > a ? b - a : 0;
    if (b > a) memcpy(d->ch[k]->s, all + a, (size_t)(b - a) * sizeof(cseg));
  }
  free(all);
  invalidate_cols(d);
  return MTE_OK;
}

/* ---- position lookups on column c ----------------------------------------------- */

/* the first chunk whose end (prefix + length) satisfies end > pos (strict) or
 * end >= pos; *pre = the prefix before it; nch when none */
static uint32_t find_chunk(const cdoc* d, int c, int64_t pos, int strict, int64_t* pre) {
  int64_t p = 0;
  const int32_t* col = d->col[c];
  for (uint32_t k = 0; k < d->nch; k++) {
    const int64_t e = p + col[k];
    if (strict ? e > pos : e >= pos) {
      *pre = p;
      return k;
    }
    p = e;
  }
  *pre = p;
  return d->nch;
}

/* ensureIntervalBoundary(pos) (oracle.c doc_split_at): split the leaf with
 * L > 0 and P < pos < P + L; column c is unchanged by a split */
static int split_at(cdoc* d, int c, int32_t r, int32_t m, int64_t pos) {
  int64_t p;
  uint32_t k = find_chunk(d, c, pos, 1, &p);
  if (k == d->nch) return MTE_OK;
  chunk* ck = d->ch[k];
  for (uint32_t i = 0; i < ck->n; i++) {
    const int32_t l = leaf_len(&ck->s[i], r, c, m);
    if (l <= 0) continue;
    if (pos < p) return MTE_OK;
    if (pos < p + l) {
      const int64_t off = pos - p;
      if (off == 0 || ck->s[i].kind != 0) return MTE_OK;
      uint32_t kk = k, ii = i + 1;
      int rc = open_slot(d, &kk, &ii);
      if (rc) return rc;
      /* after a chunk split the head may have moved too: locate it again */
      uint32_t kh = kk, ih = ii;
      if (ih == 0) {
        kh = kk - 1;
        ih = d->ch[kh]->n - 1;
      } else {
        ih--;
      }
      cseg* head = &d->ch[kh]->s[ih];
      cseg* tail = &d->ch[kk]->s[ii];
      *tail = *head;
      tail->len = head->len - (int32_t)off;
      tail->toff = head->toff + (uint32_t)off;
      head->len = (int32_t)off;
      /* a split moves no length between chunks except when head and tail land
       * in different chunks: then the columns of both chunks move */
      if (kh != kk) {
        for (int cc = 0; cc < MTE_MAX_CLIENTS; cc++) {
          if (d->col_r[cc] == INT32_MIN) continue;
          const int32_t lt = leaf_len(tail, d->col_r[cc], cc, d->col_m[cc]);
          if (lt > 0) {
            d->col[cc][kh] -= lt;
            d->col[cc][kk] += lt;
          }
        }
      }
      return MTE_OK;
    }
    p += l;
  }
  return MTE_OK;
}

/* ---- one op ------------------------------------------------------------------------------ */

typedef struct {
  const mte_batch* b;
  uint64_t text_base;
  uint32_t n_keys;
} env_t;

static int doc_apply(cdoc* d, const mte_op* op, const env_t* env) {
  const int32_t r = op->ref_seq, s = op->seq, m = d->min_seq;
  const int c = op->client;
  int rc;
  if (c >= MTE_MAX_CLIENTS) return MTE_E_CLIENT_RANGE;
  if (op->flags & MTE_F_LOCAL) return MTE_E_UNSUPPORTED;
  if (op->type > MTE_OP_ANNOTATE && op->type != MTE_OP_NOOP) return MTE_E_UNSUPPORTED;
  d->ops++;
  if (op->type == MTE_OP_INSERT) {
    ensure_col(d, c, r, m);
    if ((rc = split_at(d, c, r, m, op->pos1))) return rc;
    const int is_marker = (op->flags & MTE_F_MARKER) != 0;
    const int32_t len = is_marker ? 1 : op->pos2;
    if (len > 0) {
      /* before the first defined leaf with P >= pos, else at the end
       * (oracle.c doc_apply); pos past the length fails */
      const int64_t pos = op->pos1;
      int64_t p;
      uint32_t k = find_chunk(d, c, pos, 0, &p), at_k = d->nch, at_i = 0;
      for (; k < d->nch && at_k == d->nch; k++) {
        const chunk* ck = d->ch[k];
        for (uint32_t i = 0; i < ck->n; i++) {
          const int32_t l = leaf_len(&ck->s[i], r, c, m);
          if (l >= 0 && p >= pos) {
            at_k = k;
            at_i = i;
            break;
          }
          if (l > 0) p += l;
        }
      }
      if (at_k == d->nch) {
        if (pos > p) return MTE_E_INSERT_FAILED;
        at_k = d->nch - 1;
        at_i = d->ch[at_k]->n;
      }
      if ((rc = open_slot(d, &at_k, &at_i))) return rc;
      cseg* ns = &d->ch[at_k]->s[at_i];
      memset(ns, 0, sizeof(*ns));
      ns->len = len;
      ns->seq = s;
      ns->cli = c;
      ns->rseq = NONE_SEQ;
      if (is_marker) {
        ns->kind = 1u + (uint32_t)op->pos2;
      } else {
        ns->toff = (uint32_t)(env->text_base + op->a);
      }
      if (op->b != MTE_NO_PROPS) orc_apply_props(ns->props, env->n_keys, &env->b->propsets[op->b], env->b->props, 0);
      d->col[c][at_k] += len; /* only the inserting client sees it */
    }
  } else if (op->type == MTE_OP_REMOVE || op->type == MTE_OP_ANNOTATE) {
    const int64_t start = op->pos1, end = op->pos2;
    ensure_col(d, c, r, m);
    if ((rc = split_at(d, c, r, m, start))) return rc;
    if ((rc = split_at(d, c, r, m, end))) return rc;
    if (end > start) {
      int64_t p;
      uint32_t k = find_chunk(d, c, start, 1, &p);
      for (; k < d->nch && p < end; k++) {
        chunk* ck = d->ch[k];
        for (uint32_t i = 0; i < ck->n && p < end; i++) {
          cseg* g = &ck->s[i];
          const int32_t l = leaf_len(g, r, c, m);
          if (l <= 0) continue;
          if (p + l > start) {
            if (op->type == MTE_OP_REMOVE) {
              if (g->rseq == NONE_SEQ) {
                g->rseq = s;
                g->rmask = 1u << c;
              } else {
                g->rmask |= 1u << c;
              }
              d->col[c][k] -= l; /* removed for c (by_c); no one else's length moves */
            } else {
              orc_apply_props(g->props, env->n_keys, &env->b->propsets[op->a], env->b->props,
                              (op->flags & MTE_F_REWRITE) != 0);
            }
          }
          p += l;
        }
      }
    }
  } else if (op->type != MTE_OP_NOOP) {
    return MTE_E_INVALID_ARG;
  }
  if (op->type != MTE_OP_NOOP) {
    if (!(d->cur_seq < s)) return MTE_E_SEQ_ORDER;
    if (!(d->min_seq <= op->min_seq)) return MTE_E_MSN_ORDER;
  }
  if (op->flags & MTE_F_MSG_END) {
    if (!(d->cur_seq <= s)) return MTE_E_SEQ_ORDER;
    d->cur_seq = s;
    if (!(op->min_seq <= s)) return MTE_E_MSN_GT_SEQ;
    if (!(d->min_seq <= op->min_seq)) return MTE_E_MSN_ORDER;
    if (op->min_seq > d->min_seq) {
      d->min_seq = op->min_seq;
      if ((rc = relayout(d))) return rc;
    }
  }
  return MTE_OK;
}

/* ---- API --------------------------------------------------------------------------------- */

int och_create(uint32_t n_keys, och_ctx** out) {
  if (!out || n_keys > MTE_MAX_KEYS) return MTE_E_INVALID_ARG;
  och_ctx* c = (och_ctx*)calloc(1, sizeof(och_ctx));
  if (!c) return MTE_E_OOM;
  c->n_keys = n_keys;
  *out = c;
  return MTE_OK;
}

static void free_doc(cdoc* d) {
  for (uint32_t k = 0; k < d->nch; k++) free(d->ch[k]);
  free(d->ch);
  for (int c = 0; c < MTE_MAX_CLIENTS; c++) free(d->col[c]);
  memset(d, 0, sizeof(*d));
}

static void free_docs(och_ctx* c) {
  for (uint32_t i = 0; i < c->n_docs; i++) free_doc(&c->docs[i]);
  free(c->docs);
  c->docs = NULL;
  c->n_docs = 0;
  orc_load_tables_free(&c->load);
}

int och_destroy(och_ctx* c) {
  if (!c) return MTE_E_INVALID_ARG;
  free_docs(c);
  free(c->arena.p);
  free(c);
  return MTE_OK;
}

/* a document from one segment list (the load text or a summary body) */
static int doc_from(cdoc* d, const cseg* segs, uint32_t n) {
  for (uint32_t k = 0; k < d->nch; k++) free(d->ch[k]);
  d->nch = 0;
  const uint32_t need = n ? (n + CH_FILL - 1) / CH_FILL : 1;
  int rc = chunks_reserve(d, need);
  if (rc) return rc;
  for (uint32_t k = 0; k < need; k++) {
    d->ch[k] = (chunk*)malloc(sizeof(chunk));
    if (!d->ch[k]) return MTE_E_OOM;
    const uint32_t a = k * CH_FILL, b = a + CH_FILL < n ? a + CH_FILL : n;
    d->ch[k]->n = b > a ? b - a : 0;
    if (b > a) memcpy(d->ch[k]->s, segs + a, (size_t)(b - a) * sizeof(cseg));
  }
  d->nch = need;
  invalidate_cols(d);
  return MTE_OK;
}

int och_load_docs(och_ctx* c, uint32_t n_docs, const mte_doc_init* docs, const uint16_t* text, uint64_t text_units,
                  const mte_propset* propsets, uint32_t n_propsets, const mte_prop* props, uint32_t n_props) {
  if (!c || (n_docs && !docs)) return MTE_E_INVALID_ARG;
  free_docs(c);
  c->arena.n = 0;
  uint64_t base = 0;
  int rc = orc_arena_append(&c->arena, text, text_units, &base);
  if (rc) return rc;
  if (!(c->docs = (cdoc*)orc_docs_alloc(n_docs, sizeof(cdoc)))) return MTE_E_OOM;
  c->n_docs = n_docs;
  if ((rc = orc_load_tables_copy(&c->load, propsets, n_propsets, props, n_props, text_units))) return rc;
  for (uint32_t i = 0; i < n_docs; i++) {
    cdoc* d = &c->docs[i];
    const mte_doc_init* in = &docs[i];
    if ((rc = orc_init_text_check(in, text_units))) return rc;
    d->init = *in;
    d->flags = in->flags;
    d->min_seq = in->min_seq;
    d->cur_seq = in->cur_seq;
    /* a document this restatement does not replay (legacy calculation, local
     * client, events) stops alone; the load goes on (oracle.c refuses the load) */
    if (!(in->flags & MTE_DOC_NEW_LENGTH_CALC) || (in->flags & (MTE_DOC_LOCAL_CLIENT | MTE_DOC_EVENTS)))
      d->status = MTE_E_UNSUPPORTED;
    cseg g;
    memset(&g, 0, sizeof g);
    g.len = (int32_t)in->text_len;
    g.cli = -1;
    g.rseq = NONE_SEQ;
    g.toff = (uint32_t)(base + in->text_off);
    if (in->propset != MTE_NO_PROPS) {
      if (in->propset >= n_propsets) return MTE_E_INVALID_ARG;
      orc_apply_props(g.props, c->n_keys, &propsets[in->propset], props, 0);
    }
    if ((rc = doc_from(d, &g, in->text_len > 0 ? 1u : 0u))) return rc;
  }
  return MTE_OK;
}

int och_load_segments(och_ctx* c, const uint64_t* seg_offsets, const mte_seg* segs, uint64_t n_segs) {
  if (!c || orc_seg_offsets_check(seg_offsets, c->n_docs, segs, n_segs)) return MTE_E_INVALID_ARG;
  for (uint32_t di = 0; di < c->n_docs; di++) {
    const uint64_t b = seg_offsets[di], e = seg_offsets[di + 1];
    if (e < b) return MTE_E_INVALID_ARG;
    if (e == b) continue;
    const uint32_t n = (uint32_t)(e - b);
    cseg* tmp = (cseg*)calloc(n, sizeof(cseg));
    if (!tmp) return MTE_E_OOM;
    int rc = MTE_OK;
    for (uint32_t k = 0; k < n; k++) {
      orc_seg_fields f;
      if ((rc = orc_seg_in(&segs[b + k], &c->load, &f))) break;
      ORC_SEG_TAKE(&tmp[k], f);
      tmp[k].toff = f.toff;
      orc_seg_in_props(&segs[b + k], &c->load, tmp[k].props, c->n_keys);
    }
    if (!rc) rc = doc_from(&c->docs[di], tmp, n);
    free(tmp);
    if (rc) return rc;
  }
  return MTE_OK;
}

typedef struct {
  och_ctx* c;
  const mte_batch* b;
  uint64_t base;
} batch_arg;

/* one document's records: remote ones only, no MTE_OP_RELPOS stepping */
static void apply_doc(void* p, uint32_t di) {
  const batch_arg* w = (const batch_arg*)p;
  env_t env = {w->b, w->base, w->c->n_keys};
  cdoc* d = &w->c->docs[di];
  if (d->status) return;
  for (uint64_t k = w->b->op_offsets[di]; k < w->b->op_offsets[di + 1]; k++) {
    const int rc = doc_apply(d, &w->b->ops[k], &env);
    if (rc) {
      d->status = rc;
      break;
    }
  }
}

int och_apply_batch(och_ctx* c, const mte_batch* b, int n_threads) {
  if (!c) return MTE_E_INVALID_ARG;
  /* no document flags: a local-client document stopped at its load, and a
   * record this restatement does not replay stops its document in doc_apply */
  int rc = orc_check_batch(b, c->n_docs, NULL, 0);
  if (rc) return rc;
  batch_arg w = {c, b, 0};
  if ((rc = orc_arena_append(&c->arena, b->text, b->text_units, &w.base))) return rc;
  /* its one statistic, the records applied, runs on over the batches */
  return orc_run_docs(n_threads, c->n_docs, apply_doc, &w);
}

int och_digest(och_ctx* c, uint64_t* out, uint32_t n_docs) {
  if (!c || !out || n_docs != c->n_docs) return MTE_E_INVALID_ARG;
  for (uint32_t di = 0; di < n_docs; di++) {
    const cdoc* d = &c->docs[di];
    orc_digest_acc acc = {0, 0, 0, 0};
    for (uint32_t k = 0; k < d->nch; k++) {
      const chunk* ck = d->ch[k];
      for (uint32_t i = 0; i < ck->n; i++) {
        const cseg* g = &ck->s[i];
        if (g->rseq != NONE_SEQ) continue;
        orc_digest_seg(&acc, g->kind, g->kind == 0 ? c->arena.p + g->toff : NULL, g->len, g->props, c->n_keys);
      }
    }
    orc_digest_out(out, di, &acc);
  }
  return MTE_OK;
}

int och_doc_status(och_ctx* c, int32_t* out, uint32_t n_docs) {
  if (!c || !out || n_docs != c->n_docs) return MTE_E_INVALID_ARG;
  for (uint32_t i = 0; i < n_docs; i++) out[i] = c->docs[i].status;
  return MTE_OK;
}

int och_doc_nsegs(och_ctx* c, uint32_t doc, uint32_t* out) {
  if (!c || !out || doc >= c->n_docs) return MTE_E_INVALID_ARG;
  uint32_t n = 0;
  for (uint32_t k = 0; k < c->docs[doc].nch; k++) n += c->docs[doc].ch[k]->n;
  *out = n;
  return MTE_OK;
}

int och_read_doc(och_ctx* c, uint32_t doc, mte_doc_view* v) {
  if (!c || !v || doc >= c->n_docs) return MTE_E_INVALID_ARG;
  const cdoc* d = &c->docs[doc];
  orc_view_begin(v, d->status, d->cur_seq, d->min_seq);
  for (uint32_t k = 0; k < d->nch; k++) {
    const chunk* ck = d->ch[k];
    for (uint32_t i = 0; i < ck->n; i++) {
      const cseg* g = &ck->s[i];
      if (g->rseq != NONE_SEQ) continue;
      orc_view_seg(v, c->n_keys, g->kind, g->len, g->props, g->kind == 0 ? c->arena.p + g->toff : NULL, 0);
    }
  }
  return MTE_OK;
}

/* every held segment, tombstones included, in document order (as
 * mte_read_segments / orc_read_segments) */
int och_read_segments(och_ctx* c, uint32_t doc, mte_seg_list* v) {
  if (!c || !v || doc >= c->n_docs) return MTE_E_INVALID_ARG;
  const cdoc* d = &c->docs[doc];
  orc_segs_begin(v);
  for (uint32_t k = 0; k < d->nch; k++) {
    const chunk* ck = d->ch[k];
    for (uint32_t j = 0; j < ck->n; j++) {
      const cseg* g = &ck->s[j];
      orc_segs_seg(v, c->n_keys, ORC_SEG_GIVE(g), g->props, g->kind == 0 ? c->arena.p + g->toff : NULL, 0);
    }
  }
  return MTE_OK;
}

int och_stats_get(och_ctx* c, mte_stats* o) {
  if (!c || !o) return MTE_E_INVALID_ARG;
  memset(o, 0, sizeof(*o));
  for (uint32_t i = 0; i < c->n_docs; i++) o->ops_applied += c->docs[i].ops;
  return MTE_OK;
}
