// Lexical channel: Okapi BM25 top-k over a CSR inverted index (gfx950).
//
// Stands where the reference calls SQL rag2_lexical_search
// (database/migrations/20260114_rag2_schema.sql:341-374, from
// src/voice_agent/rag2/retrieval.py:282-290).  The reference ranks with
// PostgreSQL's ts_rank_cd; the north-star mandates BM25, whose exact form is
// the oracle's (oracle/thr_oracle.py bm25_scores): OR semantics, float64,
// contributions added in query-term order, every operation one IEEE rounding.
//
// Work decomposition: a query whose lists hold more postings than one slice (24576 when the
// batch fills the chip, down to 8192 when it does not) is cut
// into DOC-RANGE slices of ~equal posting counts (the slice edges are docs of its longest
// list), one work item per slice; short queries are one item.  A persistent grid of
// workgroups pulls items from a device-side counter, so a stop-word query of millions of
// postings is the job of up to 128 workgroups instead of one; the slices of a query share
// the pruning threshold through a global atomic max and a last kernel merges their lists.
// (thr_bm25_plan_kernel / bm25_edges_kernel / bm25_topk_kernel / bm25_merge_kernel.)
//
// Inside an item the posting lists are doc-sorted, so a doc's score is
// assembled by its OWNER posting -- the posting of the first query term that
// contains the doc.  That gives the fixed summation order with no atomics and
// no hash table.  The doc ids are staged in LDS (posting-block staging, in
// doc-range passes that always fit).  How a pass finds the owners depends on
// its lists: dense lists (narrow doc range) OR a term bit into a doc-slot
// mask; sparse lists set a Bloom bit per (list, doc) and a posting whose doc
// shows in no other list's bits is scored at once (one contribution, no
// search), the few others are searched from a dense work list; in between,
// with a threshold to prune against, owners and the sum of their terms' score
// bounds come from binary searches in LDS and only the survivors touch memory.
// Term frequencies and doc lengths are read only for the postings that need them.
// Algorithmic bytes per query: sum_t df_t * (4 doc + 4 tf + 4 doclen) + T * 16.
//
// Stop words (ABI 7): terms held by a large share of the docs also have per-doc ROWS of
// quantised impacts and term frequencies (bm25_dense_rows_kernel).  A query that holds such
// terms is split the MaxScore way: stage A walks only its other terms' postings and PROBES the
// rows where a doc is scored (bm25_topk_kernel<.., DP = true>); stage B sweeps the docs that hold
// none of the other terms in doc windows over the rows (bm25_window_kernel) -- unless the dense
// terms' bounds cannot reach stage A's threshold (bm25_sweep_filter_kernel), the usual case.
//
// This unit is the host side of a query batch: the workspace, the knobs and thr_bm25_topk.  The
// kernels live with their families -- bm25_plan.hip, bm25_walk_block.hip, bm25_walk_wave.hip,
// bm25_window.hip; index set-up in bm25_index.hip -- and are launched through bm25_common.hpp.
#include <cstdlib>
#include "bm25_common.hpp"
#ifdef BM_STAMPS
#include "bm25_stamps.hpp"
#endif

namespace thr {

constexpr int BM_EXTRA_ITEMS = 16384;  // item list capacity = 2 * n_queries + this (8 K / 16 K / 32 K / 64 K measured on 256 and
                                       // 2048 stop-word queries: 0.95 / 0.86 / 0.85 / 0.86 and 2.07 / 1.90 / 1.94 / 2.19 ms)
constexpr int BM_WAVE_ITEMS = 16384;   // item slots for the waves' slices beyond one per query, on top of the list's capacity

// The workspace carved from `ws`; from null, its size alone.
static BmLayout bm_layout(void* ws, int nq, int mt, int k) {
    BmLayout L;
    static int extra = 0;
    if (!extra) {
        const char* ev = getenv("THR_BM25_ITEMS");   // item slots beyond two per query (A/B knob)
        extra = ev && atoi(ev) >= 1024 && atoi(ev) <= (1 << 24) ? atoi(ev) : BM_EXTRA_ITEMS;   // (L.cap stays far below 2^31)
    }
    // (a query with dense terms is at least two items: stage A, stage B; the wave walk cuts stage A
    // into ~1 K-posting slices: 16 K more items for them, and one per query -- the fewest the waves
    // can be given, so that bm25_plan_kernel's fit loop always has a slice size that fits)
    L.cap_base = 2 * nq + extra;
    L.cap_wave = nq + BM_WAVE_ITEMS;
    L.cap = L.cap_base + L.cap_wave;
    const size_t cap = (size_t)L.cap;
    Arena A{(char*)ws};
    L.ctl = A.take<int32_t>(CTL_WORDS);
    L.theta = A.take<unsigned long long>(nq);
    L.q_tot = A.take<int64_t>(nq);
    L.q_dub = A.take<double>(nq);
    L.q_nt = A.take<int32_t>(nq);
    L.q_S = A.take<int32_t>(nq);
    L.q_SA = A.take<int32_t>(nq);
    L.q_pmask = A.take<int32_t>(nq);
    L.q_item0 = A.take<int32_t>(nq);
    L.q_long = A.take<int32_t>(nq);
    L.q_terms = A.take<int32_t>((size_t)nq * mt);
    L.items = A.take<int2>(cap);
    L.sweep_items = A.take<int32_t>(cap);
    L.ipos = A.take<int32_t>(2 * cap * mt);
    L.wrec = A.take<WwItem>(cap);
    L.wterm = A.take<WwTerm>(cap * 8);
    L.slice_s = A.take<double>(cap * k);
    L.slice_id = A.take<int64_t>(cap * k);
    L.slice_cnt = A.take<int32_t>(cap);
    BM_STAMPS_ONLY(L.stamps = A.take<unsigned long long>(bm_stamps_words(L.cap)));
    L.total = A.total;
    return L;
}

// The A/B knobs, each read once per process.
struct BmKnobs {
    BmShape shape = BM_SHAPE_BIG;
    int dense = 1, walk_div = 64, fuse_div = 8, wave = 1;
};
static const BmKnobs& bm_knobs() {
    static const BmKnobs knobs = [] {
        BmKnobs K;
        const char* ei = getenv("THR_BM25_DENSE");    // 0: every term through its postings (A/B knob)
        K.dense = !(ei && ei[0] == '0');
        ei = getenv("THR_BM25_WALK_DIV");             // a term with rows may be walked when held by < 1/this of the docs
        if (ei && atoi(ei) > 0) K.walk_div = atoi(ei);
        ei = getenv("THR_BM25_WALK");                 // b(lock): stage A on the workgroup walk (the round-3 path; A/B knob)
        K.wave = !(ei && ei[0] == 'b');
        ei = getenv("THR_BM25_FUSE_DIV");             // one launch for ordinary items + stage A from 1/this of the queries (0: never)
        if (ei && atoi(ei) >= 0) K.fuse_div = atoi(ei);
        const char* ev = getenv("THR_BM25_SHAPE");
        K.shape = (ev && ev[0] == 's') ? BM_SHAPE_SMALL : (ev && ev[0] == 'h') ? BM_SHAPE_HUGE : BM_SHAPE_BIG;   // s(mall) / h(uge)
        return K;
    }();
    return knobs;
}

}  // namespace thr

using namespace thr;

extern "C" size_t thr_bm25_workspace_bytes(int n_queries, int max_terms, int k) {
    if (n_queries <= 0 || n_queries > THR_BM25_MAX_QUERIES || max_terms <= 0 || k <= 0) return 0;
    return bm_layout(nullptr, n_queries, max_terms, k).total;
}

extern "C" int thr_bm25_topk(const int64_t* rowptr, const int32_t* post_doc, const int32_t* post_tf,
                             const float* doclen, const double* idf, const double* term_ub,
                             const double* block_ub, const uint8_t* post_imp, const int32_t* dense_slot,
                             const uint8_t* dense_imp, const uint16_t* dense_tf, int64_t dense_stride,
                             double avgdl, double k1, double b,
                             int64_t n_docs, int64_t n_vocab, int64_t id_base,
                             const int32_t* query_terms, int n_queries, int max_terms, int k,
                             int conjunctive, const int32_t* doc_coll, const int32_t* query_coll,
                             double* out_scores, int64_t* out_ids, int32_t* out_counts,
                             void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    // (the item counts and indices of a batch are 32 bits: 3 n_queries + 32 K slots, 256 slices per query
    // at most; the caller splits a larger batch)
    THR_RETURN_IF(n_queries > THR_BM25_MAX_QUERIES, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!rowptr || !post_doc || !post_tf || !doclen || !idf || !query_terms ||
                      !out_scores || !out_ids || !out_counts || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_docs <= 0 || n_vocab <= 0 || n_queries <= 0 || k <= 0 || k > THR_TOPK_MAX ||
                      max_terms <= 0 || max_terms > THR_BM25_MAX_TERMS || !(avgdl > 0.0),
                  THR_ERR_INVALID);
    THR_RETURN_IF((query_coll != nullptr) != (doc_coll != nullptr), THR_ERR_INVALID);
    // the dense rows come as a set, need the impacts, and are padded by one window
    THR_RETURN_IF(dense_slot && (!dense_imp || !dense_tf || !post_imp || !term_ub ||
                                 dense_stride < n_docs + BW_PAD || (dense_stride & 3)),
                  THR_ERR_INVALID);
    const BmLayout L = bm_layout(workspace, n_queries, max_terms, k);
    THR_RETURN_IF(workspace_bytes < L.total, THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(L.ctl, 0, (char*)L.q_tot - (char*)L.ctl, st);   // ctl + theta
    if (e != hipSuccess) return (int)e;
    BM_STAMPS_ONLY(bm_stamps_begin(L, st));
    const BmKnobs& K = bm_knobs();
    // OR queries of <= 8 terms by waves (bm25_walk_wave_kernel) when the impacts are there and k fits a
    // wave's buffer; AND queries, longer ones and calls without bounds keep the workgroup walk
    const bool wave = K.wave && k <= 64 && term_ub != nullptr && post_imp != nullptr && !conjunctive;
    const int32_t* dslot = K.dense ? dense_slot : nullptr;
    const BmIndex X{rowptr, post_doc, post_tf, doclen, idf, term_ub, term_ub ? block_ub : nullptr,
                    term_ub ? post_imp : nullptr, dslot, dense_imp, dense_tf, dense_stride, avgdl, k1, b,
                    n_docs, n_vocab, id_base, (k1 + 1.0) / 255.0, 255.0 / (k1 + 1.0)};
    const BmBatch B{query_terms, n_queries, max_terms, k, conjunctive, doc_coll, query_coll, out_scores,
                    out_ids, out_counts, wave, K.walk_div, wave ? -1 : dslot ? K.fuse_div : 0, st};
    // persistent grid: as many workgroups as the chip holds at once (never more than items can exist)
    int grid = num_cus() * (K.shape == BM_SHAPE_HUGE ? 1 : K.shape == BM_SHAPE_BIG ? 2 : 4);
    if (grid > L.cap) grid = L.cap;
    bm_launch_plan(X, B, L, grid, wave ? num_cus() * 4 * WW_WAVES : 0);
    int rc = launch_status();
    if (rc) return rc;
    BM_STAMPS_ONLY(if (grid > 4096) grid = 4096);   // (a stamp area holds 4096 workgroups)
    // The walks.  Wave mode: every OR query of <= 8 terms -- stage A of the ones with probed terms and
    // the ones without -- is the wave kernel's; the workgroup walk further down takes what is left
    // (nothing, usually).  Else: queries with dense terms are stage A of the workgroup walk (fused with
    // the ordinary items, or on its own: the kernels themselves pick who works), the rest ordinary items.
    if (wave) {
        int wgrid_w = num_cus() * 4;   // sixteen waves per CU; a small batch has no use for thousands of waves
        if ((long long)n_queries * 32 + 32 < wgrid_w) wgrid_w = n_queries * 32 + 32;
        bm_launch_walk_wave(X, B, L, wgrid_w);
        BM_STAMPS_ONLY(bm_stamps_report_waves(L, st, wgrid_w * WW_WAVES));
    } else if (dslot) {
        bm_launch_walk_block(X, B, L, K.shape, 2, grid BM_STAMPS_ONLY(, bm_stamps_area(L, 0), bm_stamps_walk_log(L)));
        bm_launch_walk_block(X, B, L, K.shape, 1, grid BM_STAMPS_ONLY(, bm_stamps_area(L, 2), bm_stamps_walk_log(L)));
    }
    if (dslot) {
        // stage B: doc-window sweeps, skipped where stage A's threshold rules them out
        if ((rc = launch_status())) return rc;
        bm_launch_sweep_filter(B, L);
        int wgrid = num_cus() * 2;
        if (wgrid > L.cap) wgrid = L.cap;
        bm_launch_window(X, B, L, wgrid BM_STAMPS_ONLY(, bm_stamps_area(L, 1)));
        if ((rc = launch_status())) return rc;
    }
    // the ordinary items, then the best k of every sliced query
    bm_launch_walk_block(X, B, L, K.shape, 0, grid BM_STAMPS_ONLY(, bm_stamps_area(L, 0), bm_stamps_walk_log(L)));
    BM_STAMPS_ONLY(bm_stamps_report(L, st, n_queries, grid, dslot != nullptr));
    if ((rc = launch_status())) return rc;
    bm_launch_merge(B, L);
    return launch_status();
}
