// Scoped queries: which rows a query may see, resolved on the device.
//
// The reference filters in SQL, before its LIMIT: every RPC carries p_org_id
// (database/migrations/20260114_rag2_schema.sql:341-410), the RAG 2.0 ones p_collection, the RAG 1.0
// ones p_category / p_source_document (src/voice_agent/retrieval/hybrid_search.py:227-231).  Here a
// SCOPE is a conjunction of equalities over per-row int32 attribute columns; a batch names up to P
// distinct scopes (its PREDICATES: int32 [P, C], -1 = any value, below -1 = no row).
//
// thr_scope_resolve    columns + predicates -> per predicate its matching rows, ascending (rowptr /
//                      rows), and per row the lowest predicate it matches (labels: the doc_coll of
//                      the unchanged scan and BM25 kernels when the predicates are disjoint).  Built
//                      as compact.hip builds its compaction: count per position slice, one scan,
//                      scatter -- no workgroup waits for another, no atomic, the same bits every run.
//                      A wave owns SC_WSLICE consecutive rows (lane l of round r: row r * 64 + l), the
//                      workgroup's column values sit in LDS, the predicate values are wave-uniform
//                      (scalar loads), a match is a ballot and a row's place in the list of p is
//                      base[p][wave slice] + popcount of the lanes below it.
// The row lists are ranked by thr_dense_topk_rows (dense_rows.hip); the labels filter the graph channel
// (graph.hip) and, as doc_coll, the scan and BM25 kernels.
#include "thr_common.hpp"

namespace thr {

constexpr int SC_THREADS = 256;
constexpr int SC_WAVES = SC_THREADS / WAVE;
constexpr int SC_ROUNDS = 8;                        // rows per lane
constexpr int SC_WSLICE = WAVE * SC_ROUNDS;         // consecutive rows per wave
constexpr int SC_SLICE = SC_WSLICE * SC_WAVES;      // rows per workgroup (8 KiB of LDS per column)

struct ScopeCols {
    const int32_t* c[THR_SCOPE_MAX_COLS];
};

// The column values of the workgroup's rows -> LDS [C][SC_SLICE] (rows behind n_docs: never read).
__device__ __forceinline__ void sc_stage(const ScopeCols& cols, int C, int64_t n_docs, int64_t s0, int32_t* vals) {
    for (int c = 0; c < C; ++c) {
        const int32_t* __restrict__ col = cols.c[c];
        for (int i = threadIdx.x; i < SC_SLICE; i += SC_THREADS) {
            const int64_t row = s0 + i;
            vals[c * SC_SLICE + i] = row < n_docs ? col[row] : 0;
        }
    }
    __syncthreads();
}

// does row slot i (of the workgroup) satisfy predicate p?  pv is wave-uniform.
__device__ __forceinline__ bool sc_match(const int32_t* __restrict__ preds, int p, int C, const int32_t* vals, int i) {
    bool m = true;
    for (int c = 0; c < C; ++c) {
        const int32_t pv = preds[(int64_t)p * C + c];
        m = m && (pv == -1 || (pv >= 0 && vals[c * SC_SLICE + i] == pv));
    }
    return m;
}

__global__ __launch_bounds__(SC_THREADS) void scope_count(ScopeCols cols, int C, int64_t n_docs,
                                                          const int32_t* __restrict__ preds, int P, int64_t n_ws,
                                                          int32_t* __restrict__ ws_count, int32_t* __restrict__ labels,
                                                          int32_t* __restrict__ overlap) {
    extern __shared__ int32_t sc_vals[];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t s0 = (int64_t)blockIdx.x * SC_SLICE;
    sc_stage(cols, C, n_docs, s0, sc_vals);
    const int64_t ws = (int64_t)blockIdx.x * SC_WAVES + wave;
    int32_t lab[SC_ROUNDS];
    bool two = false;
#pragma unroll
    for (int r = 0; r < SC_ROUNDS; ++r) lab[r] = -2;
    for (int p = 0; p < P; ++p) {
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < SC_ROUNDS; ++r) {
            const int i = wave * SC_WSLICE + r * WAVE + lane;
            const bool m = s0 + i < n_docs && sc_match(preds, p, C, sc_vals, i);
            cnt += __popcll(__ballot(m));
            if (m) {
                two = two || lab[r] != -2;
                if (lab[r] == -2) lab[r] = p;
            }
        }
        if (lane == 0 && ws < n_ws) ws_count[(int64_t)p * n_ws + ws] = cnt;
    }
    if (labels) {
#pragma unroll
        for (int r = 0; r < SC_ROUNDS; ++r) {
            const int64_t row = s0 + wave * SC_WSLICE + r * WAVE + lane;
            if (row < n_docs) labels[row] = lab[r];
        }
        if (two) *overlap = 1;   // (every writer writes the same value)
    }
}

// One workgroup: exclusive scan of the P * n_ws counts in predicate-major order (the list of
// predicate p is the concatenation of its wave slices) -> bases; rowptr[p] = base of its first slice.
__global__ __launch_bounds__(SC_THREADS) void scope_scan(const int32_t* __restrict__ ws_count, int P, int64_t n_ws,
                                                         int64_t* __restrict__ ws_base, int64_t* __restrict__ rowptr) {
    __shared__ int64_t s_sum[SC_THREADS];
    const int64_t n = (int64_t)P * n_ws;
    const int64_t per = (n + SC_THREADS - 1) / SC_THREADS;
    const int64_t lo = per * threadIdx.x < n ? per * threadIdx.x : n;
    const int64_t hi = lo + per < n ? lo + per : n;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += ws_count[i];
    s_sum[threadIdx.x] = sum;
    block_inclusive_scan<SC_THREADS>(s_sum);
    int64_t run = s_sum[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        ws_base[i] = run;
        run += ws_count[i];
    }
    __syncthreads();   // (the bases are written)
    for (int p = threadIdx.x; p <= P; p += SC_THREADS)
        rowptr[p] = p < P ? ws_base[(int64_t)p * n_ws] : s_sum[SC_THREADS - 1];
}

__global__ __launch_bounds__(SC_THREADS) void scope_scatter(ScopeCols cols, int C, int64_t n_docs,
                                                            const int32_t* __restrict__ preds, int P, int64_t n_ws,
                                                            const int64_t* __restrict__ ws_base,
                                                            int32_t* __restrict__ rows, int64_t cap) {
    extern __shared__ int32_t sc_vals[];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t s0 = (int64_t)blockIdx.x * SC_SLICE;
    sc_stage(cols, C, n_docs, s0, sc_vals);
    const int64_t ws = (int64_t)blockIdx.x * SC_WAVES + wave;
    if (ws >= n_ws) return;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int p = 0; p < P; ++p) {
        int64_t off = ws_base[(int64_t)p * n_ws + ws];
#pragma unroll
        for (int r = 0; r < SC_ROUNDS; ++r) {
            const int i = wave * SC_WSLICE + r * WAVE + lane;
            const bool m = s0 + i < n_docs && sc_match(preds, p, C, sc_vals, i);
            const uint64_t b = __ballot(m);
            if (m) {
                const int64_t dst = off + __popcll(b & below);
                if (dst >= 0 && dst < cap) rows[dst] = (int32_t)(s0 + i);
            }
            off += __popcll(b);
        }
    }
}

}  // namespace thr

using namespace thr;

static int64_t scope_wave_slices(int64_t n_docs) { return (n_docs + SC_SLICE - 1) / SC_SLICE * SC_WAVES; }

static void scope_plan(Arena& A, int64_t n_docs, int P, int32_t** ws_count, int64_t** ws_base) {
    const size_t n = (size_t)P * (size_t)scope_wave_slices(n_docs);
    *ws_count = A.take<int32_t>(n);
    *ws_base = A.take<int64_t>(n);
}

extern "C" size_t thr_scope_resolve_workspace_bytes(int64_t n_docs, int n_preds) {
    if (n_docs <= 0 || n_docs > ((int64_t)1 << 31) - 1 || n_preds <= 0 || n_preds > THR_SCOPE_MAX_PREDS) return 0;
    Arena A;
    int32_t* c;
    int64_t* b;
    scope_plan(A, n_docs, n_preds, &c, &b);
    return A.total;
}

extern "C" int thr_scope_resolve(const int32_t* const* h_cols, int n_cols, int64_t n_docs, const int32_t* preds,
                                 int n_preds, int64_t* rowptr, int32_t* rows, int64_t cap, int32_t* labels,
                                 int32_t* overlap, void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(n_cols <= 0 || n_cols > THR_SCOPE_MAX_COLS || n_preds <= 0 || n_preds > THR_SCOPE_MAX_PREDS,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_docs <= 0 || n_docs > ((int64_t)1 << 31) - 1 || cap < 0, THR_ERR_INVALID);
    THR_RETURN_IF(!h_cols || !preds || !rowptr || !workspace, THR_ERR_INVALID);
    THR_RETURN_IF((rows != nullptr) != (cap > 0), THR_ERR_INVALID);
    THR_RETURN_IF((labels != nullptr) != (overlap != nullptr), THR_ERR_INVALID);
    ScopeCols cols = {};
    for (int c = 0; c < n_cols; ++c) {
        THR_RETURN_IF(!h_cols[c], THR_ERR_INVALID);
        cols.c[c] = h_cols[c];
    }
    THR_RETURN_IF(workspace_bytes < thr_scope_resolve_workspace_bytes(n_docs, n_preds), THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    int32_t* ws_count;
    int64_t* ws_base;
    scope_plan(A, n_docs, n_preds, &ws_count, &ws_base);
    const int64_t n_blocks = (n_docs + SC_SLICE - 1) / SC_SLICE, n_ws = n_blocks * SC_WAVES;
    const size_t lds = sizeof(int32_t) * (size_t)n_cols * SC_SLICE;
    if (overlap) {
        hipError_t e = hipMemsetAsync(overlap, 0, sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    // (eight columns are exactly 64 KiB of dynamic LDS: launch_lds asks for the size it launches with)
    int rc = launch_lds(scope_count, dim3((unsigned)n_blocks), dim3(SC_THREADS), lds, st, cols, n_cols, n_docs, preds,
                        n_preds, n_ws, ws_count, labels, overlap);
    if (rc) return rc;
    hipLaunchKernelGGL(scope_scan, dim3(1), dim3(SC_THREADS), 0, st, ws_count, n_preds, n_ws, ws_base, rowptr);
    rc = launch_status();
    if (rc || !rows) return rc;
    return launch_lds(scope_scatter, dim3((unsigned)n_blocks), dim3(SC_THREADS), lds, st, cols, n_cols, n_docs, preds,
                      n_preds, n_ws, (const int64_t*)ws_base, rows, cap);
}
