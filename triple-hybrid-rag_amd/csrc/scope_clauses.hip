// Scoped queries, the general predicate: per column a CLAUSE instead of a value.
//
// thr_scope_resolve_clauses   thr_scope_resolve's outputs and kernel shape (count per wave slice, one
//                      scan, scatter; no workgroup waits for another, no atomic, the same bits every
//                      run: scope.hip's frame, a second copy of it -- as templates over the match test
//                      the equality kernels did not keep their ISA) over conjunctions of
//                      clauses int32 (kind, a, b, 0):
//                          0 any       1 none       2 range a <= v <= b       3 set: v is one of
//                          set_values[a .. a + b) (ascending, distinct, >= 0)       6 / 7 = 2 / 3 negated.
//                      A row whose value is -1 (it has none) matches no clause, negated or not: SQL's
//                      NULL under =, IN, BETWEEN, <> and NOT IN.  The clause words are wave-uniform
//                      (scalar loads); a set is a per-lane binary search with a wave-uniform trip
//                      count over the wave-uniform window of set_values (vector loads of a small,
//                      cache-resident array).
// The table lives on the device and the host cannot read it, so the kernels are safe for ANY table:
// a kind outside the list matches no row, and a set's window is clamped into [0, n_set_values] before
// anything is read.
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

// Does row slot i (of the workgroup) satisfy predicate p?  The clause words are wave-uniform.
struct ClauseMatch {
    const int32_t* __restrict__ clauses;      // [P, C, 4]
    const int32_t* __restrict__ set_values;   // [n_set]
    int32_t n_set;

    __device__ __forceinline__ bool operator()(int p, int C, const int32_t* vals, int i) const {
        bool m = true;
        for (int c = 0; c < C; ++c) {
            const int32_t* __restrict__ cl = clauses + ((int64_t)p * C + c) * 4;
            const int32_t kind = cl[0], a = cl[1], b = cl[2];
            if (kind == 0) continue;
            const int32_t v = vals[c * SC_SLICE + i];
            const int32_t base = kind & ~4;                 // 2 / 3 for the kinds that test a value
            bool in = false;
            if (kind >= 2 && kind <= 7 && base == 2) {
                in = v >= a && v <= b;
            } else if (kind >= 2 && kind <= 7 && base == 3) {
                // the window, clamped: lo in [0, n_set], len in [0, n_set - lo] (all wave-uniform)
                const int32_t lo = a < 0 ? 0 : (a > n_set ? n_set : a);
                const int32_t len = b < 0 ? 0 : (b > n_set - lo ? n_set - lo : b);
                if (len > 0) {
                    const int32_t* __restrict__ sv = set_values + lo;
                    // the largest index whose member is <= v stays inside [at, at + n)
                    int32_t at = 0;
                    for (int32_t n = len; n > 1;) {
                        const int32_t half = n >> 1;
                        if (sv[at + half] <= v) at += half;
                        n -= half;
                    }
                    in = sv[at] == v;
                }
            } else {
                m = false;                                  // none, or a kind this kernel does not know
                continue;
            }
            m = m && v >= 0 && in != ((kind & 4) != 0);
        }
        return m;
    }
};

// Per wave slice and predicate the number of matching rows; per row the lowest predicate it matches.
__device__ __forceinline__ void sc_count_body(const ClauseMatch& match, const ScopeCols& cols, int C, int64_t n_docs, int P,
                                              int64_t n_ws, int32_t* __restrict__ ws_count,
                                              int32_t* __restrict__ labels, int32_t* __restrict__ overlap) {
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
            const bool m = s0 + i < n_docs && match(p, C, sc_vals, i);
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

// A matching row's place in the list of p: the base of its wave slice + the matching lanes below it.
__device__ __forceinline__ void sc_scatter_body(const ClauseMatch& match, const ScopeCols& cols, int C, int64_t n_docs, int P,
                                                int64_t n_ws, const int64_t* __restrict__ ws_base,
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
            const bool m = s0 + i < n_docs && match(p, C, sc_vals, i);
            const uint64_t b = __ballot(m);
            if (m) {
                const int64_t dst = off + __popcll(b & below);
                if (dst >= 0 && dst < cap) rows[dst] = (int32_t)(s0 + i);
            }
            off += __popcll(b);
        }
    }
}

__global__ __launch_bounds__(SC_THREADS) void scope_clauses_count(ScopeCols cols, int C, int64_t n_docs,
                                                                  const int32_t* __restrict__ clauses,
                                                                  const int32_t* __restrict__ set_values, int32_t n_set,
                                                                  int P, int64_t n_ws, int32_t* __restrict__ ws_count,
                                                                  int32_t* __restrict__ labels,
                                                                  int32_t* __restrict__ overlap) {
    sc_count_body(ClauseMatch{clauses, set_values, n_set}, cols, C, n_docs, P, n_ws, ws_count, labels, overlap);
}

__global__ __launch_bounds__(SC_THREADS) void scope_clauses_scatter(ScopeCols cols, int C, int64_t n_docs,
                                                                    const int32_t* __restrict__ clauses,
                                                                    const int32_t* __restrict__ set_values, int32_t n_set,
                                                                    int P, int64_t n_ws,
                                                                    const int64_t* __restrict__ ws_base,
                                                                    int32_t* __restrict__ rows, int64_t cap) {
    sc_scatter_body(ClauseMatch{clauses, set_values, n_set}, cols, C, n_docs, P, n_ws, ws_base, rows, cap);
}

// One workgroup: exclusive scan of the P * n_ws counts in predicate-major order -> bases; rowptr[p] =
// base of its first slice (scope.hip's scope_scan).
__global__ __launch_bounds__(SC_THREADS) void scope_clauses_scan(const int32_t* __restrict__ ws_count, int P,
                                                                 int64_t n_ws, int64_t* __restrict__ ws_base,
                                                                 int64_t* __restrict__ rowptr) {
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

}  // namespace thr

using namespace thr;

static int64_t scope_wave_slices(int64_t n_docs) { return (n_docs + SC_SLICE - 1) / SC_SLICE * SC_WAVES; }

static void scope_plan(Arena& A, int64_t n_docs, int P, int32_t** ws_count, int64_t** ws_base) {
    const size_t n = (size_t)P * (size_t)scope_wave_slices(n_docs);
    *ws_count = A.take<int32_t>(n);
    *ws_base = A.take<int64_t>(n);
}

extern "C" size_t thr_scope_resolve_clauses_workspace_bytes(int64_t n_docs, int n_preds) {
    if (n_docs <= 0 || n_docs > ((int64_t)1 << 31) - 1 || n_preds <= 0 || n_preds > THR_SCOPE_MAX_PREDS) return 0;
    Arena A;
    int32_t* c;
    int64_t* b;
    scope_plan(A, n_docs, n_preds, &c, &b);
    return A.total;
}

extern "C" int thr_scope_resolve_clauses(const int32_t* const* h_cols, int n_cols, int64_t n_docs,
                                         const int32_t* clauses, int n_preds, const int32_t* set_values,
                                         int64_t n_set_values, int64_t* rowptr, int32_t* rows, int64_t cap,
                                         int32_t* labels, int32_t* overlap, void* workspace, size_t workspace_bytes,
                                         thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(n_cols <= 0 || n_cols > THR_SCOPE_MAX_COLS || n_preds <= 0 || n_preds > THR_SCOPE_MAX_PREDS,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_docs <= 0 || n_docs > ((int64_t)1 << 31) - 1 || cap < 0, THR_ERR_INVALID);
    THR_RETURN_IF(n_set_values < 0 || n_set_values > THR_SCOPE_MAX_SET_VALUES, THR_ERR_INVALID);
    THR_RETURN_IF(!h_cols || !clauses || !rowptr || !workspace, THR_ERR_INVALID);
    THR_RETURN_IF((set_values != nullptr) != (n_set_values > 0), THR_ERR_INVALID);
    THR_RETURN_IF((rows != nullptr) != (cap > 0), THR_ERR_INVALID);
    THR_RETURN_IF((labels != nullptr) != (overlap != nullptr), THR_ERR_INVALID);
    ScopeCols cols = {};
    for (int c = 0; c < n_cols; ++c) {
        THR_RETURN_IF(!h_cols[c], THR_ERR_INVALID);
        cols.c[c] = h_cols[c];
    }
    THR_RETURN_IF(workspace_bytes < thr_scope_resolve_clauses_workspace_bytes(n_docs, n_preds), THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    int32_t* ws_count;
    int64_t* ws_base;
    scope_plan(A, n_docs, n_preds, &ws_count, &ws_base);
    const int64_t n_blocks = (n_docs + SC_SLICE - 1) / SC_SLICE, n_ws = n_blocks * SC_WAVES;
    const size_t lds = sizeof(int32_t) * (size_t)n_cols * SC_SLICE;
    const int32_t n_set = (int32_t)n_set_values;
    if (overlap) {
        hipError_t e = hipMemsetAsync(overlap, 0, sizeof(int32_t), st);
        if (e != hipSuccess) return (int)e;
    }
    int rc = launch_lds(scope_clauses_count, dim3((unsigned)n_blocks), dim3(SC_THREADS), lds, st, cols, n_cols, n_docs,
                        clauses, set_values, n_set, n_preds, n_ws, ws_count, labels, overlap);
    if (rc) return rc;
    hipLaunchKernelGGL(scope_clauses_scan, dim3(1), dim3(SC_THREADS), 0, st, ws_count, n_preds, n_ws, ws_base, rowptr);
    rc = launch_status();
    if (rc || !rows) return rc;
    return launch_lds(scope_clauses_scatter, dim3((unsigned)n_blocks), dim3(SC_THREADS), lds, st, cols, n_cols, n_docs,
                      clauses, set_values, n_set, n_preds, n_ws, (const int64_t*)ws_base, rows, cap);
}
