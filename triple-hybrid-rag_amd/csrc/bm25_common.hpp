// What the BM25 translation units share: the records and device helpers more than one kernel family
// uses, the constants two units need, the BM_STAMPS macros, the control words and the workspace of
// thr_bm25_topk, and the host functions bm25.hip launches the other units' kernels through -- each
// defined beside its kernels, each with that one caller.
#pragma once
#include "thr_common.hpp"

namespace thr {

constexpr int BM_BLOCK = 128;   // postings under one block_ub bound (bm25_bounds_kernel)
constexpr int BW_PAD = 65536;   // docs per window of bm25_window_kernel = zero padding of a dense row
constexpr int WW_WAVES = 4;     // waves per workgroup of bm25_walk_wave_kernel (independent: they never synchronise)

// What bm25_walk_wave_kernel needs of an item and of its terms, gathered by bm25_edges_kernel so that
// a wave's set-up is two dependent loads, not five (item -> query words -> term ids -> list heads).
struct WwItem {
    int32_t q, sl, SA, S, nt, pm, qc, pad;
};
struct WwTerm {
    int64_t lo;     // first posting of the term's slice (absolute)
    double idf, ub;
    int64_t row;    // probed term: offset of its per-doc row; else -1
    int32_t len;    // postings of the slice (0 for a probed term)
    int32_t pad;
};

struct TermRange {
    int64_t lo;   // first posting of the term
    int len;      // postings of the term
    int cur;      // postings already consumed by earlier doc-range passes
    int sub;      // postings of the current pass: [cur, cur + sub)
    int lds_off;  // offset of the current pass's doc ids in the staged array
};

// lower_bound on a doc-sorted posting list; returns index or -1
template <typename Ptr>
__device__ __forceinline__ int find_doc(Ptr docs, int len, int32_t d) {
    int lo = 0, hi = len;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if (docs[mid] < d) lo = mid + 1; else hi = mid;
    }
    return (lo < len && docs[lo] == d) ? lo : -1;
}
// number of postings with doc < d
__device__ __forceinline__ int count_below(const int32_t* docs, int len, int64_t d) {
    int lo = 0, hi = len;
    while (lo < hi) {
        int mid = (lo + hi) >> 1;
        if ((int64_t)docs[mid] < d) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ double bm25_contrib(double idf, double tf, double dl, double avgdl,
                                               double k1, double b) {
    // nrm = k1*((1-b) + b*(dl/avgdl)); contrib = idf*((tf*(k1+1))/(tf+nrm))
    const double nrm = __dmul_rn(k1, __dadd_rn(__dsub_rn(1.0, b), __dmul_rn(b, __ddiv_rn(dl, avgdl))));
    return __dmul_rn(idf, __ddiv_rn(__dmul_rn(tf, __dadd_rn(k1, 1.0)), __dadd_rn(tf, nrm)));
}

// first doc of slice s of S of a window-kernel query (a multiple of 4: the dword loads of the dense rows)
__device__ __forceinline__ int64_t bm_window_edge(int64_t n_docs, int s, int S) {
    return s >= S ? n_docs : (n_docs * s / S) & ~(int64_t)3;
}

// BM_STAMPS (diagnostic build, _build.build_variant("stamps", ["BM_STAMPS"]); scripts/bm25_stamps.py):
// thread 0 of every workgroup adds the cycles between consecutive phase marks into buckets,
// written behind the workspace; thr_bm25_topk then waits for the launch and prints the shares.
#ifdef BM_STAMPS
constexpr int BM_NSTAMP = 20;   // 0-13 phases (cycles), 14-19 counters
#define BM_STAMP(i)                                                       \
    do {                                                                  \
        if (threadIdx.x == 0) {                                           \
            const unsigned long long now_ = __builtin_readcyclecounter(); \
            stamp_acc[i] += now_ - stamp_last;                            \
            stamp_last = now_;                                            \
        }                                                                 \
    } while (0)
#define BM_COUNT(i, v) do { if (threadIdx.x == 0) stamp_acc[i] += (unsigned long long)(v); } while (0)
#define BM_STAMPS_ONLY(...) __VA_ARGS__
#else
#define BM_STAMP(i)
#define BM_COUNT(i, v)
#define BM_STAMPS_ONLY(...)
#endif

// ctl: the words the kernels of one thr_bm25_topk call talk through (zeroed per call)
enum BmCtl {
    CTL_ITEMS = 0,        // work items (bm25_plan_kernel)
    CTL_NEXT_BLOCK = 1,   // next item of the workgroup walk's ordinary or fused launch
    CTL_NEXT_SWEEP = 2,   // next sweep of bm25_window_kernel
    CTL_DENSE_Q = 3,      // queries with dense (probed) terms
    CTL_NEXT_A = 4,       // next item of stage A: the wave walk, or the workgroup walk's stage-A launch
    CTL_SWEEPS = 5,       // sweeps still needed (bm25_sweep_filter_kernel)
    CTL_PLAN_DONE = 6,    // plan workgroups done
    CTL_TARGET_A = 7,     // postings a stage-A slice was aimed at
    CTL_BLOCK_Q = 8,      // queries of the workgroup walk
    CTL_WORDS = 16
};

// ---- workspace of thr_bm25_topk (carved by bm_layout, bm25.hip) ----
struct BmLayout {
    int32_t* ctl;                  // BmCtl                      } zeroed
    unsigned long long* theta;     // shared thresholds (keys)   } per call
    int64_t* q_tot;
    double* q_dub;
    int32_t *q_nt, *q_S, *q_SA, *q_pmask, *q_item0, *q_long, *q_terms;
    int2* items;
    int32_t *sweep_items, *ipos;
    WwItem* wrec;
    WwTerm* wterm;
    double* slice_s;
    int64_t* slice_id;
    int32_t* slice_cnt;
    BM_STAMPS_ONLY(unsigned long long* stamps;)
    size_t total;
    int cap, cap_base, cap_wave;   // item slots: all / sweeps + workgroup walk / waves
};

// ---- what the launch functions take: filled once by thr_bm25_topk ----
// The index as set_lexical fixed it, with what the call's knobs and null arguments make of it.
struct BmIndex {
    const int64_t* rowptr;
    const int32_t *post_doc, *post_tf;
    const float* doclen;
    const double *idf, *term_ub;
    const double* block_ub;        // null without term_ub
    const uint8_t* post_imp;       // null without term_ub
    const int32_t* dense_slot;     // null under THR_BM25_DENSE=0
    const uint8_t* dense_imp;
    const uint16_t* dense_tf;
    int64_t dense_stride;
    double avgdl, k1, b;
    int64_t n_docs, n_vocab, id_base;
    double imp_unit, imp_per_unit; // (k1 + 1) / 255 and 255 / (k1 + 1): the host's divisions
};
// The batch of one call.
struct BmBatch {
    const int32_t* query_terms;
    int n_queries, max_terms, k, conjunctive;
    const int32_t *doc_coll, *query_coll;
    double* out_s;
    int64_t* out_id;
    int32_t* out_cnt;
    bool wave;       // OR queries of <= 8 terms go to bm25_walk_wave_kernel
    int walk_div;    // THR_BM25_WALK_DIV
    int fuse_div;    // of bm25_topk_kernel: -1 in wave mode, THR_BM25_FUSE_DIV with dense rows, else 0
    hipStream_t st;
};
enum BmShape { BM_SHAPE_BIG = 0, BM_SHAPE_SMALL = 1, BM_SHAPE_HUGE = 2 };   // THR_BM25_SHAPE

// bm25_plan.hip.  n_slots: workgroups of the workgroup walk; wave_slots: waves of the wave walk the
// chip holds at once (0 without it)
void bm_launch_plan(const BmIndex& X, const BmBatch& B, const BmLayout& L, int n_slots, int wave_slots);
void bm_launch_sweep_filter(const BmBatch& B, const BmLayout& L);
void bm_launch_merge(const BmBatch& B, const BmLayout& L);
// bm25_walk_block.hip, bm25_walk_wave.hip, bm25_window.hip (the stamp areas: bm25_stamps.hpp)
void bm_launch_walk_block(const BmIndex& X, const BmBatch& B, const BmLayout& L, BmShape shape, int dpm, int grid
                          BM_STAMPS_ONLY(, unsigned long long* stamps, unsigned long long* walk_log));
void bm_launch_walk_wave(const BmIndex& X, const BmBatch& B, const BmLayout& L, int grid);
void bm_launch_window(const BmIndex& X, const BmBatch& B, const BmLayout& L, int grid
                      BM_STAMPS_ONLY(, unsigned long long* stamps));

}  // namespace thr
