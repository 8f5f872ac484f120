/*
 * orc_shell.h — what the four CPU restatements share (TEST INFRASTRUCTURE):
 * oracle.c (orc_, flat), tree.c (ort_, pointer tree), titems.c (oti_, the tree
 * on an item array) and chunked.c (och_, config 5).  The canonical digest
 * (DESIGN.md "Digest"), the remote-observer PropertiesManager.addProperties,
 * and the API shell under each restatement's replay rules: text arena, load
 * tables, load and batch validation, the document thread pool and the read-out
 * emitters.  Plain functions over plain data; each restatement keeps its own
 * loops over its own storage and calls them (DESIGN.md §4 "The shell" lists
 * what differs between the four on purpose).
 */
#ifndef MTE_ORC_SHELL_H_
#define MTE_ORC_SHELL_H_

#include <pthread.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/mte.h"

#define ORC_NONE_SEQ INT32_MAX /* "removedSeq undefined" */

/* ---- canonical digest --------------------------------------------------- */
#define ORC_M61 ((1ull << 61) - 1)
static const uint64_t ORC_DIG_B1 = 0x1d8e4e27c47d124full % ((1ull << 61) - 1);
static const uint64_t ORC_DIG_B2 = 0x0a0761d6478bd642ull % ((1ull << 61) - 1);

static inline uint64_t orc_mix64(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
  return z ^ (z >> 31);
}
static inline uint64_t orc_mulmod61(uint64_t a, uint64_t b) {
  unsigned __int128 p = (unsigned __int128)a * b;
  uint64_t lo = (uint64_t)(p & ORC_M61), hi = (uint64_t)(p >> 61);
  uint64_t r = lo + hi;
  if (r >= ORC_M61) r -= ORC_M61;
  return r;
}
static inline uint64_t orc_addmod61(uint64_t a, uint64_t b) {
  uint64_t r = a + b;
  if (r >= ORC_M61) r -= ORC_M61;
  return r;
}

/* running digest state of one document */
typedef struct {
  uint64_t n, h1, h2, sum;
} orc_digest_acc;

/* feed one visible segment: `units` (text) or a marker of `kind` (1 + refType) */
static inline void orc_digest_seg(orc_digest_acc* a, uint32_t kind, const uint16_t* units, int32_t len,
                                  const uint32_t* props, uint32_t n_keys) {
  uint64_t ph = 0;
  for (uint32_t k = 0; k < n_keys; k++)
    if (props[k]) ph += orc_mix64(((uint64_t)(k + 1) << 32) | props[k]);
  for (int32_t u = 0; u < len; u++) {
    uint64_t rec = kind == 0 ? (uint64_t)units[u] : ((1ull << 32) | (uint64_t)(kind - 1));
    uint64_t x = orc_mix64(rec * 0x9E3779B97F4A7C15ull + ph) % ORC_M61;
    a->h1 = orc_addmod61(orc_mulmod61(a->h1, ORC_DIG_B1), x);
    a->h2 = orc_addmod61(orc_mulmod61(a->h2, ORC_DIG_B2), x);
    a->sum += x;
    a->n++;
  }
}

/* PropertiesManager.addProperties for a remote observer (collaborating, no
 * pending local keys, so shouldModifyKey is true for every key):
 * segmentPropertiesManager.ts:63-151.  rewrite first clears the keys not in
 * newProps (105-119); then null deletes, anything else sets (121-148).  The
 * falsy-value test of the rewrite loop cancels against the set loop, so the net
 * effect is "clear all, then apply". */
static inline uint64_t orc_apply_props(uint32_t* props, uint32_t n_keys, const mte_propset* ps,
                                       const mte_prop* pe, int rewrite) {
  uint64_t w = 0;
  if (rewrite) {
    for (uint32_t k = 0; k < n_keys; k++) props[k] = 0;
  }
  for (uint32_t j = 0; j < ps->count; j++) {
    const mte_prop* p = &pe[ps->first + j];
    if (p->key < n_keys) {
      props[p->key] = p->value; /* value 0 == null == delete */
      w++;
    }
  }
  return w;
}

/* ---- text arena: load text first, then every batch's text ----------------- */
typedef struct {
  uint16_t* p;
  uint64_t n, cap;
} orc_arena;

static inline int orc_arena_append(orc_arena* a, const uint16_t* t, uint64_t n, uint64_t* base) {
  if (a->n + n > a->cap) {
    uint64_t nc = a->cap ? a->cap : 1024;
    while (nc < a->n + n) nc *= 2;
    uint16_t* p = (uint16_t*)realloc(a->p, nc * sizeof(uint16_t));
    if (!p) return MTE_E_OOM;
    a->p = p;
    a->cap = nc;
  }
  *base = a->n;
  if (n) memcpy(a->p + a->n, t, n * sizeof(uint16_t));
  a->n += n;
  return MTE_OK;
}

/* ---- what *_load_docs keeps for *_load_segments ---------------------------- */
typedef struct {
  mte_propset* ps;
  uint32_t n_ps;
  mte_prop* pe;
  uint32_t n_pe;
  uint64_t units; /* text units of the load */
} orc_load_tables;

static inline void orc_load_tables_free(orc_load_tables* l) {
  free(l->ps);
  free(l->pe);
  memset(l, 0, sizeof(*l));
}

static inline int orc_load_tables_copy(orc_load_tables* l, const mte_propset* ps, uint32_t n_ps, const mte_prop* pe,
                                       uint32_t n_pe, uint64_t units) {
  orc_load_tables_free(l);
  l->units = units;
  if (n_ps && !(l->ps = (mte_propset*)malloc((size_t)n_ps * sizeof(mte_propset)))) return MTE_E_OOM;
  if (n_pe && !(l->pe = (mte_prop*)malloc((size_t)n_pe * sizeof(mte_prop)))) return MTE_E_OOM;
  if (n_ps) memcpy(l->ps, ps, (size_t)n_ps * sizeof(mte_propset));
  if (n_pe) memcpy(l->pe, pe, (size_t)n_pe * sizeof(mte_prop));
  l->n_ps = n_ps;
  l->n_pe = n_pe;
  return MTE_OK;
}

/* a zeroed document array (one element at least, so &docs[0] stands) */
static inline void* orc_docs_alloc(uint32_t n_docs, size_t doc_size) {
  const size_t bytes = (size_t)(n_docs ? n_docs : 1) * doc_size;
  void* p = aligned_alloc(128, bytes);
  if (p) memset(p, 0, bytes);
  return p;
}

/* the initial text of one mte_doc_init lies in the load text */
static inline int orc_init_text_check(const mte_doc_init* in, uint64_t text_units) {
  return (uint64_t)in->text_off + in->text_len > text_units ? MTE_E_INVALID_ARG : MTE_OK;
}

/* ---- segment intake (*_load_segments) and its way back (*_read_segments) --- */
static inline int orc_seg_offsets_check(const uint64_t* seg_offsets, uint32_t n_docs, const mte_seg* segs,
                                        uint64_t n_segs) {
  if (!seg_offsets || (n_segs && !segs) || seg_offsets[0] != 0 || seg_offsets[n_docs] != n_segs)
    return MTE_E_INVALID_ARG;
  return MTE_OK;
}

typedef struct {
  int32_t len, seq, cli, rseq;
  uint32_t rmask, kind, toff; /* toff: offset in the load text, 0 for a marker */
} orc_seg_fields;
/* into / out of a restatement's segment: oseg, tnode, item and cseg name these
 * fields alike (toff apart: tree.c has none, oracle.c renames some markers) */
#define ORC_SEG_TAKE(g, f) \
  ((g)->len = (f).len, (g)->seq = (f).seq, (g)->cli = (f).cli, (g)->rseq = (f).rseq, (g)->rmask = (f).rmask, \
   (g)->kind = (f).kind)
#define ORC_SEG_GIVE(g) \
  (orc_seg_fields) { (g)->len, (g)->seq, (g)->cli, (g)->rseq, (uint32_t)(g)->rmask, (g)->kind, 0 }

/* one mte_seg of a summary body, checked against the load and converted */
static inline int orc_seg_in(const mte_seg* sg, const orc_load_tables* l, orc_seg_fields* f) {
  const int marker = sg->kind != 0;
  if ((marker && sg->len != 1) || (!marker && (sg->len == 0 || (uint64_t)sg->text_off + sg->len > l->units)) ||
      sg->client < -1 || sg->client >= MTE_MAX_CLIENTS || sg->seq < 0 ||
      (sg->removed_seq != MTE_NOT_REMOVED && sg->removers == 0) ||
      (sg->propset != MTE_NO_PROPS && sg->propset >= l->n_ps))
    return MTE_E_INVALID_ARG;
  f->len = (int32_t)sg->len;
  f->seq = sg->seq;
  f->cli = sg->client;
  f->rseq = sg->removed_seq == MTE_NOT_REMOVED ? ORC_NONE_SEQ : sg->removed_seq;
  f->rmask = sg->removed_seq == MTE_NOT_REMOVED ? 0u : sg->removers;
  f->kind = sg->kind;
  f->toff = marker ? 0u : sg->text_off;
  return MTE_OK;
}

/* its properties onto a zeroed plane row; -> 1 if it has any (a tree's `po`) */
static inline int orc_seg_in_props(const mte_seg* sg, const orc_load_tables* l, uint32_t* props, uint32_t n_keys) {
  if (sg->propset == MTE_NO_PROPS) return 0;
  orc_apply_props(props, n_keys, &l->ps[sg->propset], l->pe, 0);
  return 1;
}

/* ---- record validation (*_apply_batch), as mte_submit validates -----------
 * The table-bounds rules hold for every restatement.  The local-record rules
 * need each document's MTE_DOC_* flags: doc_flags points at document 0's, in
 * structs doc_stride bytes apart; NULL (tree.c, chunked.c: no local clients)
 * leaves such records to the restatement's doc_apply. */
static inline int orc_check_batch(const mte_batch* b, uint32_t n_docs, const uint32_t* doc_flags, size_t doc_stride) {
  if (!b || b->n_docs != n_docs || !b->op_offsets) return MTE_E_INVALID_ARG;
  if (b->op_offsets[b->n_docs] != b->n_ops) return MTE_E_INVALID_ARG;
  uint32_t dcur = 0;
  uint64_t rbkey_end = 0; /* records up to here are an annotate rollback's MTE_OP_RBKEY */
  for (uint64_t k = 0; k < b->n_ops; k++) {
    const mte_op* op = &b->ops[k];
    if (op->type == MTE_OP_INSERT && !(op->flags & MTE_F_MARKER) && op->pos2 > 0 &&
        (uint64_t)op->a + (uint64_t)op->pos2 > b->text_units)
      return MTE_E_INVALID_ARG;
    if (op->type == MTE_OP_INSERT && op->b != MTE_NO_PROPS && op->b >= b->n_propsets) return MTE_E_INVALID_ARG;
    if (op->type == MTE_OP_ANNOTATE && op->a >= b->n_propsets) return MTE_E_INVALID_ARG;
    if (!doc_flags) continue;
    while (dcur + 1 < b->n_docs && b->op_offsets[dcur + 1] <= k) dcur++;
    const uint32_t flags = *(const uint32_t*)((const char*)doc_flags + (size_t)dcur * doc_stride);
    const int local_doc = (flags & MTE_DOC_LOCAL_CLIENT) != 0;
    if ((op->type == MTE_OP_RBKEY) != (k < rbkey_end)) return MTE_E_INVALID_ARG;
    if (op->type == MTE_OP_ROLLBACK && op->pos1 == MTE_OP_ANNOTATE) {
      if (op->pos2 < 0 || k + 1 + (uint64_t)op->pos2 > b->op_offsets[dcur + 1]) return MTE_E_INVALID_ARG;
      rbkey_end = k + 1 + (uint64_t)op->pos2;
    }
    if (op->type > MTE_OP_RELPOS) return MTE_E_INVALID_ARG;
    if (op->type == MTE_OP_RELPOS) {
      const uint32_t rp = MTE_RP_POS1 | MTE_RP_BEFORE1 | MTE_RP_POS2 | MTE_RP_BEFORE2;
      if ((op->flags & ~rp) || !(op->flags & (MTE_RP_POS1 | MTE_RP_POS2)) || k + 1 >= b->op_offsets[dcur + 1] ||
          op[1].type > MTE_OP_ANNOTATE)
        return MTE_E_INVALID_ARG;
      continue;
    }
    if (op->type >= MTE_OP_ROLLBACK && !(op->flags & MTE_F_LOCAL)) return MTE_E_INVALID_ARG;
    if (op->type == MTE_OP_REF) {
      if (!(flags & MTE_DOC_REFS) || op->seq != 0 || op->pos2 < 0 || op->b > 5 || op->client >= MTE_MAX_CLIENTS)
        return MTE_E_INVALID_ARG;
      continue;
    }
    if ((op->flags & MTE_F_LOCAL) && op->type == MTE_OP_ANNOTATE && op->b != MTE_NO_PROPS &&
        op->b >= MTE_ANNOTATE_SLOTS)
      return MTE_E_INVALID_ARG;
    if ((op->flags & MTE_F_LOCAL) || op->type == MTE_OP_ACK) {
      if (!local_doc) return MTE_E_INVALID_ARG;
      if ((op->flags & MTE_F_LOCAL) && op->type != MTE_OP_RBKEY &&
          (op->type == MTE_OP_ACK || op->seq <= 0 || op->seq >= MTE_LOCAL_SEQ_BASE))
        return MTE_E_INVALID_ARG;
      if (op->type == MTE_OP_RBKEY && (op->seq < 0 || op->seq >= MTE_LOCAL_SEQ_BASE || op->pos1 < 0 ||
                                       op->pos1 >= MTE_MAX_KEYS || op->pos2 < 0 || op->pos2 > MTE_ANNOTATE_SLOTS))
        return MTE_E_INVALID_ARG;
      if (op->type == MTE_OP_ACK && (op->pos1 <= 0 || op->pos1 > op->pos2)) return MTE_E_INVALID_ARG;
    }
    if (local_doc && !(op->flags & MTE_F_LOCAL) && op->seq >= MTE_LOCAL_SEQ_BASE) return MTE_E_INVALID_ARG;
  }
  return MTE_OK;
}

/* ---- the pool: fn(arg, doc) once per document, documents strided over threads */
typedef void (*orc_doc_fn)(void* arg, uint32_t doc);
typedef struct {
  orc_doc_fn fn;
  void* arg;
  uint32_t d0, n_docs, stride;
  pthread_t th;
} orc_run_arg;

static inline void* orc_run_thread(void* p) {
  const orc_run_arg* w = (const orc_run_arg*)p;
  for (uint32_t di = w->d0; di < w->n_docs; di += w->stride) w->fn(w->arg, di);
  return NULL;
}

static inline int orc_run_docs(int n_threads, uint32_t n_docs, orc_doc_fn fn, void* arg) {
  if (n_threads < 1) n_threads = 1;
  if ((uint32_t)n_threads > n_docs) n_threads = n_docs ? (int)n_docs : 1;
  orc_run_arg* w = (orc_run_arg*)calloc((size_t)n_threads, sizeof(orc_run_arg));
  if (!w) return MTE_E_OOM;
  for (int t = 0; t < n_threads; t++) w[t] = (orc_run_arg){.fn = fn, .arg = arg, .d0 = (uint32_t)t, .n_docs = n_docs, .stride = (uint32_t)n_threads};
  if (n_threads == 1) {
    orc_run_thread(&w[0]);
  } else {
    for (int t = 0; t < n_threads; t++) pthread_create(&w[t].th, NULL, orc_run_thread, &w[t]);
    for (int t = 0; t < n_threads; t++) pthread_join(w[t].th, NULL);
  }
  free(w);
  return MTE_OK;
}

/* ---- read-out emitters ------------------------------------------------------
 * Each restatement walks its own storage and hands over one segment at a time:
 * its fields, its property row and, for text, its units.  join: the segment
 * continues the one before (titems.c's merged leaves) and reads as part of it. */
static inline void orc_text_out(uint16_t* text, uint64_t cap, uint64_t* nt, const uint16_t* units, int32_t len) {
  for (int32_t u = 0; u < len; u++, (*nt)++)
    if (*nt < cap && text) text[*nt] = units[u];
}

/* mte_doc_view (*_read_doc): the visible segments */
static inline void orc_view_begin(mte_doc_view* v, int32_t status, int32_t cur_seq, int32_t min_seq) {
  v->status = status;
  v->cur_seq = cur_seq;
  v->min_seq = min_seq;
  v->length = v->n_text = v->n_segs = 0;
}

static inline void orc_view_seg(mte_doc_view* v, uint32_t n_keys, uint32_t kind, int32_t len, const uint32_t* props,
                                const uint16_t* units, int join) {
  if (join) {
    if (v->n_segs - 1 < v->seg_cap && v->seg_len) v->seg_len[v->n_segs - 1] += (uint32_t)len;
  } else {
    const uint32_t ns = v->n_segs++;
    if (ns < v->seg_cap) {
      if (v->seg_len) v->seg_len[ns] = (uint32_t)len;
      if (v->seg_kind) v->seg_kind[ns] = kind;
      if (v->seg_props)
        for (uint32_t k = 0; k < n_keys; k++) v->seg_props[(size_t)ns * n_keys + k] = props[k];
    }
  }
  v->length += (uint32_t)len;
  if (kind == 0) {
    uint64_t nt = v->n_text;
    orc_text_out(v->text, v->text_cap, &nt, units, len);
    v->n_text = (uint32_t)nt;
  }
}

/* mte_seg_list (*_read_segments): every held segment, tombstones included */
static inline void orc_segs_begin(mte_seg_list* v) { v->n_segs = v->n_text = 0; }

static inline void orc_segs_seg(mte_seg_list* v, uint32_t n_keys, orc_seg_fields f, const uint32_t* props,
                                const uint16_t* units, int join) {
  if (join) {
    if (v->n_segs - 1 < v->seg_cap && v->segs) v->segs[v->n_segs - 1].len += (uint32_t)f.len;
  } else {
    const uint64_t i = v->n_segs++;
    if (i < v->seg_cap && v->segs) {
      mte_seg* s = &v->segs[i];
      s->text_off = f.kind == 0 ? (uint32_t)v->n_text : 0u;
      s->len = (uint32_t)f.len;
      s->seq = f.seq;
      s->removed_seq = f.rseq == ORC_NONE_SEQ ? MTE_NOT_REMOVED : f.rseq;
      s->removers = f.rseq == ORC_NONE_SEQ ? 0u : f.rmask;
      s->client = f.cli;
      s->kind = f.kind;
      s->propset = MTE_NO_PROPS;
      if (v->props)
        for (uint32_t k = 0; k < n_keys; k++) v->props[(size_t)i * n_keys + k] = props[k];
    }
  }
  if (f.kind == 0) {
    uint64_t nt = v->n_text;
    orc_text_out(v->text, v->text_cap, &nt, units, f.len);
    v->n_text = nt;
  }
}

/* one document's four digest words */
static inline void orc_digest_out(uint64_t* out, uint32_t doc, const orc_digest_acc* a) {
  out[4 * (size_t)doc + 0] = a->n;
  out[4 * (size_t)doc + 1] = a->h1;
  out[4 * (size_t)doc + 2] = a->h2;
  out[4 * (size_t)doc + 3] = a->sum;
}

/* the events of a document's last batch (*_read_deltas) */
static inline void orc_deltas_out(const mte_delta* dl, uint64_t dl_n, mte_delta* out, uint64_t cap, uint64_t* n) {
  *n = dl_n;
  if (out && dl_n) memcpy(out, dl, (size_t)(cap < dl_n ? cap : dl_n) * sizeof(mte_delta));
}

/* mte_stats of the flat counters: one document's share, then the byte model */
static inline void orc_stats_add(mte_stats* o, uint64_t ops, uint64_t scanned, uint64_t written, uint64_t pwrites,
                                 uint64_t units, uint64_t max_segs) {
  o->ops_applied += ops;
  o->segs_scanned += scanned;
  o->segs_written += written;
  o->prop_writes += pwrites;
  o->units_inserted += units;
  if (max_segs > o->max_segs) o->max_segs = max_segs;
}

static inline void orc_stats_end(mte_stats* o) {
  o->algo_bytes = 32.0 * (double)o->ops_applied + 20.0 * (double)o->segs_scanned + 20.0 * (double)o->segs_written +
                  4.0 * (double)o->prop_writes + 2.0 * (double)o->units_inserted;
}

#endif
