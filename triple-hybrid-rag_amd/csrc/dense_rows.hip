// Dense channel, exact top-k over row lists: thr_dense_topk_rows, the scoped kin of
// thr_dense_topk_exact (dense_exact.hip).  The row lists are thr_scope_resolve's (scope.hip).
//
// Exact cosine top-k of every query over the row list of its scope, the oracle's arithmetic
// (sequential float64 accumulation of the float32 products in dimension order).  exact_slab_topk
// (dense_exact.hip) gives one thread one row and ONE query: a row is fetched once per query,
// neighbouring lanes read a row apart.  Here the queries of a scope share its rows: a work item is
// (tile of up to RW_QT queries of one scope, slice of its row list); a lane owns RW_R rows of a batch
// and keeps RW_R x RW_QT float64 chains; the rows of a wave reach LDS in 64-byte pieces (four lanes per
// row: whole 64-byte segments per load), the next piece is in flight while the current one is consumed,
// and a query element is one broadcast LDS read for all lanes and both rows.
// a * b of two floats is exact in float64, so fma(a, b, s) rounds once, exactly where the oracle's
// s + a * b rounds: the chains are v_fma_f64, the bits the same.
// The slice lists of a query are ranked by merge_lists (dense_exact.hip) in its gated flavour: a query
// whose scope is outside [0, P) gets the empty list, because its slabs were never written.
#include <algorithm>

#include "dense_common.hpp"

namespace thr {

constexpr int RW_THREADS = 256;
constexpr int RW_WAVES = RW_THREADS / WAVE;
constexpr int RW_QT = 8;                           // queries of a tile: float64 chains per lane and row
constexpr int RW_R = 2;                            // rows per lane and batch
constexpr int RW_WROWS = WAVE * RW_R;              // rows of a wave's batch
constexpr int RW_BATCH = RW_WROWS * RW_WAVES;      // rows of a workgroup's batch
constexpr int RW_STEP = 16;                        // floats per row and staging step: a 64-byte segment
constexpr int RW_STRIDE = RW_STEP + 4;             // words between staged rows: lanes 0..15 reading their
                                                   // row's float4 touch all 64 banks once (20 l mod 64)
constexpr int RW_LOADS = RW_WROWS * (RW_STEP / 4) / WAVE;   // float4 loads per lane and step
constexpr int RW_DC = 1024;                        // query floats per tile row in LDS (longer rows: re-staged per 1024 dims)
constexpr int RW_CAP = 512;                        // selection buffer per query (k <= 256, 256 pushed at a time)
constexpr int RW_MAX_SLICES = 32;
constexpr size_t RW_LDS = sizeof(float) * (RW_QT * RW_DC + RW_WAVES * RW_WROWS * RW_STRIDE) +
                          (sizeof(double) + sizeof(int64_t)) * RW_QT * RW_CAP;

// One workgroup: the queries grouped by scope, in query order inside a scope (a stable counting
// sort: chunk by chunk, a thread ranks its query among the chunk's queries of the same scope), and
// the tiles of RW_QT queries counted.  qptr / tptr [P + 1]; queries whose scope is outside [0, P)
// are in no group.
__global__ __launch_bounds__(RW_THREADS) void rows_group(const int32_t* __restrict__ query_scope, int nq, int P,
                                                         int32_t* __restrict__ cnt /* [P], zeroed */,
                                                         int32_t* __restrict__ qptr, int32_t* __restrict__ tptr,
                                                         int32_t* __restrict__ cursor, int32_t* __restrict__ scope_q) {
    __shared__ int s_sum[RW_THREADS], s_til[RW_THREADS], s_sc[RW_THREADS];
    for (int q = threadIdx.x; q < nq; q += RW_THREADS) {
        const int p = query_scope[q];
        if (p >= 0 && p < P) atomicAdd(&cnt[p], 1);   // (a count: no order in it)
    }
    __threadfence();
    __syncthreads();
    const int per = (P + RW_THREADS - 1) / RW_THREADS;
    const int lo = per * (int)threadIdx.x < P ? per * (int)threadIdx.x : P;
    const int hi = lo + per < P ? lo + per : P;
    int sum = 0, til = 0;
    for (int i = lo; i < hi; ++i) {
        const int c = __hip_atomic_load(&cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        sum += c;
        til += (c + RW_QT - 1) / RW_QT;
    }
    s_sum[threadIdx.x] = sum;
    s_til[threadIdx.x] = til;
    __syncthreads();
    for (int d = 1; d < RW_THREADS; d <<= 1) {   // block_inclusive_scan of both arrays behind the same barriers
        const int a = threadIdx.x >= d ? s_sum[threadIdx.x - d] : 0;
        const int b = threadIdx.x >= d ? s_til[threadIdx.x - d] : 0;
        __syncthreads();
        s_sum[threadIdx.x] += a;
        s_til[threadIdx.x] += b;
        __syncthreads();
    }
    int run = s_sum[threadIdx.x] - sum, trun = s_til[threadIdx.x] - til;
    for (int i = lo; i < hi; ++i) {
        const int c = __hip_atomic_load(&cnt[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        qptr[i] = run;
        tptr[i] = trun;
        cursor[i] = run;
        run += c;
        trun += (c + RW_QT - 1) / RW_QT;
    }
    if (threadIdx.x == RW_THREADS - 1) {
        qptr[P] = s_sum[RW_THREADS - 1];
        tptr[P] = s_til[RW_THREADS - 1];
    }
    __syncthreads();
    for (int base = 0; base < nq; base += RW_THREADS) {
        const int q = base + threadIdx.x;
        int p = q < nq ? query_scope[q] : -1;
        if (p < 0 || p >= P) p = -1;
        s_sc[threadIdx.x] = p;
        __syncthreads();
        int rank = 0, total = 0;
        if (p >= 0)
            for (int j = 0; j < RW_THREADS; ++j) {
                const int same = s_sc[j] == p;
                total += same;
                rank += same && j < (int)threadIdx.x;
            }
        const int at = p >= 0 ? cursor[p] : 0;
        __syncthreads();   // (every cursor of this chunk is read)
        if (p >= 0) {
            if (at + rank < nq) scope_q[at + rank] = q;
            if (rank == 0) cursor[p] = at + total;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(RW_THREADS) void rows_score(
    const float* __restrict__ docs, const double* __restrict__ dnorm, int64_t n_docs, int dim,
    const float* __restrict__ queries, int n_queries, int k, int P, const int64_t* __restrict__ rowptr,
    const int32_t* __restrict__ rows, int64_t rows_cap, const int32_t* __restrict__ qptr,
    const int32_t* __restrict__ tptr, const int32_t* __restrict__ scope_q, int S, double* __restrict__ slab_s,
    int64_t* __restrict__ slab_id) {
    extern __shared__ __align__(16) unsigned char rw_lds[];
    float* q_lds = reinterpret_cast<float*>(rw_lds);                       // [RW_QT][RW_DC]
    float* stage = q_lds + RW_QT * RW_DC;                                  // [RW_WAVES][RW_WROWS * RW_STRIDE]
    double* b_s = reinterpret_cast<double*>(stage + RW_WAVES * RW_WROWS * RW_STRIDE);   // [RW_QT][RW_CAP]
    int64_t* b_id = reinterpret_cast<int64_t*>(b_s + RW_QT * RW_CAP);
    __shared__ int b_cnt[RW_QT];
    __shared__ double t_s[RW_QT];
    __shared__ int64_t t_id[RW_QT];
    __shared__ double s_qn[RW_QT];
    __shared__ int s_q[RW_QT];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int tile = blockIdx.x / S, slice = blockIdx.x % S;
    if (tile >= tptr[P]) return;
    int p = 0;
    for (int hi = P; hi - p > 1;) {   // the last scope whose first tile is <= tile (tptr[0] == 0)
        const int mid = (p + hi) >> 1;
        if (tptr[mid] <= tile) p = mid; else hi = mid;
    }
    const int q0 = qptr[p] + (tile - tptr[p]) * RW_QT;
    int nqt = qptr[p + 1] - q0;
    nqt = nqt < RW_QT ? nqt : RW_QT;
    if (q0 < 0 || nqt <= 0 || q0 + nqt > n_queries) return;
    int64_t r0 = rowptr[p], r1 = rowptr[p + 1];
    r0 = r0 < 0 ? 0 : (r0 > rows_cap ? rows_cap : r0);
    r1 = r1 < r0 ? r0 : (r1 > rows_cap ? rows_cap : r1);
    const int64_t per = (((r1 - r0) + S - 1) / S + RW_BATCH - 1) / RW_BATCH * RW_BATCH;
    const int64_t lo_r = r0 + slice * per;
    const int64_t hi_r = lo_r + per < r1 ? lo_r + per : r1;

    if (threadIdx.x < RW_QT) {
        int q = threadIdx.x < nqt ? scope_q[q0 + threadIdx.x] : -1;
        if (q < 0 || q >= n_queries) q = -1;
        s_q[threadIdx.x] = q;
        double qn = 0.0;
        if (q >= 0 && lo_r < hi_r) {
            const float* __restrict__ qv = queries + (int64_t)q * dim;
            for (int i = 0; i < dim; ++i) qn = __fma_rn((double)qv[i], (double)qv[i], qn);
            qn = __dsqrt_rn(qn);
        }
        s_qn[threadIdx.x] = qn;
    }
    __syncthreads();
    if (lo_r >= hi_r) {   // an empty slice: an empty list per query
        for (int qi = 0; qi < nqt; ++qi) {
            const int q = s_q[qi];
            if (q < 0) continue;
            for (int i = threadIdx.x; i < k; i += RW_THREADS) {
                const int64_t o = ((int64_t)q * S + slice) * k + i;
                slab_s[o] = -INFINITY;
                slab_id[o] = INT64_MAX;
            }
        }
        return;
    }
    auto topk = [&](int qi) {
        BlockTopK<RW_CAP, RW_THREADS> tk;
        tk.s = b_s + qi * RW_CAP;
        tk.id = b_id + qi * RW_CAP;
        tk.count = &b_cnt[qi];
        tk.thr_s = &t_s[qi];
        tk.thr_id = &t_id[qi];
        tk.k = k;
        return tk;
    };
    for (int qi = 0; qi < nqt; ++qi) {
        BlockTopK<RW_CAP, RW_THREADS> tk;
        tk.init(b_s + qi * RW_CAP, b_id + qi * RW_CAP, &b_cnt[qi], &t_s[qi], &t_id[qi], k);
    }
    float* wstage = stage + wave * (RW_WROWS * RW_STRIDE);
    const int piece = lane & 3;   // which float4 of a row's 64-byte segment this lane fetches

    for (int64_t base = lo_r; base < hi_r; base += RW_BATCH) {
        const int64_t wbase = base + wave * RW_WROWS;
        // staging: float4 t of this lane is piece `piece` of the wave's row t * 16 + lane / 4
        const float* src[RW_LOADS];
#pragma unroll
        for (int t = 0; t < RW_LOADS; ++t) {
            const int64_t gi = wbase + t * (WAVE / 4) + (lane >> 2);
            int64_t row = gi < hi_r ? (int64_t)rows[gi] : -1;
            if (row < 0 || row >= n_docs) row = -1;
            src[t] = row >= 0 ? docs + row * dim + piece * 4 : nullptr;
        }
        int64_t own[RW_R];
        double dn[RW_R];
#pragma unroll
        for (int j = 0; j < RW_R; ++j) {
            const int64_t gi = wbase + j * WAVE + lane;
            int64_t row = gi < hi_r ? (int64_t)rows[gi] : -1;
            if (row < 0 || row >= n_docs) row = -1;
            own[j] = row;
            dn[j] = row >= 0 ? dnorm[row] : 0.0;
        }
        double acc[RW_R][RW_QT];
#pragma unroll
        for (int j = 0; j < RW_R; ++j)
#pragma unroll
            for (int qi = 0; qi < RW_QT; ++qi) acc[j][qi] = 0.0;
        float4 pf[RW_LOADS];
        auto fetch = [&](int d0) {
            const bool in = d0 + piece * 4 < dim;
#pragma unroll
            for (int t = 0; t < RW_LOADS; ++t)
                pf[t] = (src[t] && in) ? *reinterpret_cast<const float4*>(src[t] + d0) : make_float4(0.f, 0.f, 0.f, 0.f);
        };
        fetch(0);
        for (int d0 = 0; d0 < dim; d0 += RW_STEP) {
            const int dq = d0 % RW_DC;
            __syncthreads();   // (the previous step's reads of the stage and of the query tile are done)
#pragma unroll
            for (int t = 0; t < RW_LOADS; ++t)
                *reinterpret_cast<float4*>(wstage + (t * (WAVE / 4) + (lane >> 2)) * RW_STRIDE + piece * 4) = pf[t];
            if (dq == 0 && (dim > RW_DC || base == lo_r)) {
                const int len = dim - d0 < RW_DC ? dim - d0 : RW_DC;
                for (int qi = 0; qi < nqt; ++qi) {
                    const int q = s_q[qi];
                    for (int i = threadIdx.x; i < len; i += RW_THREADS)
                        q_lds[qi * RW_DC + i] = q >= 0 ? queries[(int64_t)q * dim + d0 + i] : 0.f;
                }
            }
            __syncthreads();
            if (d0 + RW_STEP < dim) fetch(d0 + RW_STEP);
            const int nv = (dim - d0) / 4 < RW_STEP / 4 ? (dim - d0) / 4 : RW_STEP / 4;
#pragma unroll
            for (int c = 0; c < RW_STEP / 4; ++c) {
                if (c >= nv) continue;
                double xd[RW_R][4];
#pragma unroll
                for (int j = 0; j < RW_R; ++j) {
                    const float4 x = *reinterpret_cast<const float4*>(wstage + (j * WAVE + lane) * RW_STRIDE + c * 4);
                    xd[j][0] = (double)x.x; xd[j][1] = (double)x.y; xd[j][2] = (double)x.z; xd[j][3] = (double)x.w;
                }
                static_for<0, RW_QT>([&](auto QI) {
                    constexpr int qi = decltype(QI)::value;
                    if (qi < nqt) {
                        const float4 qv = *reinterpret_cast<const float4*>(q_lds + qi * RW_DC + dq + c * 4);
                        const double qd[4] = {(double)qv.x, (double)qv.y, (double)qv.z, (double)qv.w};
#pragma unroll
                        for (int e = 0; e < 4; ++e)
#pragma unroll
                            for (int j = 0; j < RW_R; ++j) acc[j][qi] = __fma_rn(xd[j][e], qd[e], acc[j][qi]);
                    }
                });
            }
        }
        // cosine with the oracle's two roundings; rows without an embedding are absent
#pragma unroll
        for (int j = 0; j < RW_R; ++j) {
            const bool valid = own[j] >= 0 && dn[j] > 0.0;
            static_for<0, RW_QT>([&](auto QI) {
                constexpr int qi = decltype(QI)::value;
                if (qi < nqt) {
                    const double qn = s_qn[qi];
                    const double sim = valid ? (qn > 0.0 ? __ddiv_rn(acc[j][qi], __dmul_rn(qn, dn[j])) : 0.0) : -INFINITY;
                    topk(qi).push(valid && s_q[qi] >= 0, sim, own[j]);
                }
            });
        }
    }
    for (int qi = 0; qi < nqt; ++qi) {
        const int n = topk(qi).finish();
        const int q = s_q[qi];
        if (q < 0) continue;
        for (int i = threadIdx.x; i < k; i += RW_THREADS) {
            const int64_t o = ((int64_t)q * S + slice) * k + i;
            slab_s[o] = i < n ? b_s[qi * RW_CAP + i] : -INFINITY;
            slab_id[o] = i < n ? b_id[qi * RW_CAP + i] : INT64_MAX;
        }
    }
}

}  // namespace thr

using namespace thr;

// slices of a scope's row list: enough work items for the chip when the batch has few tiles
static int rows_slices(int n_queries, int n_scopes) {
    const int64_t tiles = std::min<int64_t>(n_queries, (int64_t)n_scopes + n_queries / RW_QT);
    const int64_t s = (2 * (int64_t)num_cus() + tiles - 1) / tiles;
    return (int)std::max<int64_t>(1, std::min<int64_t>(s, RW_MAX_SLICES));
}

struct RowsPlan {
    int S;
    int32_t *cnt, *qptr, *tptr, *cursor, *scope_q;
    double* slab_s;
    int64_t* slab_id;
};

static RowsPlan rows_plan(Arena& A, int n_queries, int n_scopes, int k) {
    RowsPlan R;
    R.S = rows_slices(n_queries, n_scopes);
    R.cnt = A.take<int32_t>((size_t)n_scopes);
    R.qptr = A.take<int32_t>((size_t)n_scopes + 1);
    R.tptr = A.take<int32_t>((size_t)n_scopes + 1);
    R.cursor = A.take<int32_t>((size_t)n_scopes);
    R.scope_q = A.take<int32_t>((size_t)n_queries);
    R.slab_s = A.take<double>((size_t)n_queries * R.S * k);
    R.slab_id = A.take<int64_t>((size_t)n_queries * R.S * k);
    return R;
}

extern "C" size_t thr_dense_topk_rows_workspace_bytes(int n_queries, int n_scopes, int k) {
    if (n_queries <= 0 || n_queries > THR_SCOPE_MAX_QUERIES || n_scopes <= 0 || n_scopes > THR_SCOPE_MAX_PREDS ||
        k <= 0 || k > THR_DENSE_MAX_K)
        return 0;
    Arena A;
    rows_plan(A, n_queries, n_scopes, k);
    return A.total;
}

extern "C" int thr_dense_topk_rows(const float* docs, const double* dnorm, int64_t n_docs, int dim, int64_t id_base,
                                   const float* queries, int n_queries, int k, const int64_t* rowptr,
                                   const int32_t* rows, int64_t rows_cap, int n_scopes, const int32_t* query_scope,
                                   double* out_scores, int64_t* out_ids, int32_t* out_counts, uint32_t* out_flags,
                                   void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!docs || !dnorm || !queries || !rowptr || !query_scope || !out_scores || !out_ids || !out_counts ||
                      !out_flags || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_docs <= 0 || n_docs > ((int64_t)1 << 31) - 1 || n_queries <= 0 || k <= 0 || k > THR_DENSE_MAX_K ||
                      id_base < 0 || rows_cap < 0 || n_scopes <= 0 || n_scopes > THR_SCOPE_MAX_PREDS,
                  THR_ERR_INVALID);
    THR_RETURN_IF((rows != nullptr) != (rows_cap > 0), THR_ERR_INVALID);
    THR_RETURN_IF(n_queries > THR_SCOPE_MAX_QUERIES, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(dim <= 0 || dim % 4 != 0, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(workspace_bytes < thr_dense_topk_rows_workspace_bytes(n_queries, n_scopes, k), THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    const RowsPlan R = rows_plan(A, n_queries, n_scopes, k);
    hipError_t e = hipMemsetAsync(R.cnt, 0, sizeof(int32_t) * (size_t)n_scopes, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(rows_group, dim3(1), dim3(RW_THREADS), 0, st, query_scope, n_queries, n_scopes, R.cnt, R.qptr,
                       R.tptr, R.cursor, R.scope_q);
    int rc = launch_status();
    if (rc) return rc;
    const int64_t tiles = std::min<int64_t>(n_queries, (int64_t)n_scopes + n_queries / RW_QT);
    rc = launch_lds(rows_score, dim3((unsigned)(tiles * R.S)), dim3(RW_THREADS), RW_LDS, st, docs, dnorm, n_docs, dim,
                    queries, n_queries, k, n_scopes, rowptr, rows, rows_cap, (const int32_t*)R.qptr,
                    (const int32_t*)R.tptr, (const int32_t*)R.scope_q, R.S, R.slab_s, R.slab_id);
    if (rc) return rc;
    return launch_merge_scoped(R.slab_s, R.slab_id, n_queries, R.S, k, id_base, query_scope, n_scopes, out_scores,
                               out_ids, out_counts, out_flags, st);
}
