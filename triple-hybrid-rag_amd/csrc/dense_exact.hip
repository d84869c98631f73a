// Dense channel, the exhaustive path and the merges: thr_dense_topk_exact, thr_dense_rescue (K5 of
// the pipeline, dense.hip) and thr_merge_topk; the merge of thr_dense_topk_rows (dense_rows.hip).
#include "dense_common.hpp"

namespace thr {

// sequential float64 accumulation of float32 products: the oracle's contract
// (oracle/thr_oracle.py seq_dot_f64).  Products are exact in float64.
__device__ __forceinline__ double seq_dot_f64(const float* __restrict__ a, const float* b, int d) {
    double s = 0.0;
    const float4* a4 = reinterpret_cast<const float4*>(a);
    for (int i = 0; i < d / 4; ++i) {
        float4 x = a4[i];
        s = __dadd_rn(s, __dmul_rn((double)x.x, (double)b[4 * i + 0]));
        s = __dadd_rn(s, __dmul_rn((double)x.y, (double)b[4 * i + 1]));
        s = __dadd_rn(s, __dmul_rn((double)x.z, (double)b[4 * i + 2]));
        s = __dadd_rn(s, __dmul_rn((double)x.w, (double)b[4 * i + 3]));
    }
    return s;
}

// ---------------------------------------------------------------------------
// Exhaustive float64 path: every row scored with the oracle's arithmetic, then an
// exact block top-k per (query, slab); slabs merged by a second kernel.
// ---------------------------------------------------------------------------
constexpr int EX_THREADS = 256;
constexpr int EX_CAP = 1024;
constexpr int EX_SLABS = 64;

__global__ __launch_bounds__(EX_THREADS) void exact_slab_topk(
    const float* __restrict__ docs, const double* __restrict__ dnorm, int64_t n_docs, int dim,
    const float* __restrict__ queries, int n_queries, int k, double* __restrict__ slab_s,
    int64_t* __restrict__ slab_id, const uint32_t* __restrict__ skip_certified,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll,
    int32_t* __restrict__ n_done) {
    extern __shared__ float lds_qv[];
    __shared__ double b_s[EX_CAP];
    __shared__ int64_t b_id[EX_CAP];
    __shared__ int b_cnt;
    __shared__ double t_s;
    __shared__ int64_t t_id;
    __shared__ double s_qn;
    __shared__ unsigned long long s_todo;
    const int slab = blockIdx.x;
    // the counter merge_lists adds to in the next launch starts at zero (no fill launch of the caller's)
    if (n_done && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) *n_done = 0;
    // queries strided over gridDim.y, at most 64 per block: in rescue mode (skip_certified) the
    // grid is small and one ballot tells the block which of its queries still need the work
    // (instead of one mostly-empty block per query)
    {
        const int q = blockIdx.y + (int)threadIdx.x * (int)gridDim.y;
        const bool todo = threadIdx.x < 64 && q < n_queries &&
                          !(skip_certified && (skip_certified[q] & THR_FLAG_CERTIFIED));
        const unsigned long long m = __ballot(todo);
        if (threadIdx.x == 0) s_todo = m;
        __syncthreads();
    }
    for (unsigned long long todo = s_todo; todo; todo &= todo - 1) {
        const int q = blockIdx.y + (__ffsll((long long)todo) - 1) * (int)gridDim.y;
        __syncthreads();
        for (int i = threadIdx.x; i < dim; i += EX_THREADS) lds_qv[i] = queries[(int64_t)q * dim + i];
        __syncthreads();
        if (threadIdx.x == 0) s_qn = __dsqrt_rn(seq_dot_f64(lds_qv, lds_qv, dim));
        BlockTopK<EX_CAP, EX_THREADS> tk;
        tk.init(b_s, b_id, &b_cnt, &t_s, &t_id, k);
        const double qn = s_qn;
        const int qc = query_coll ? query_coll[q] : -1;
        const int64_t per = (n_docs + EX_SLABS - 1) / EX_SLABS;
        const int64_t lo = slab * per, hi = (lo + per < n_docs) ? lo + per : n_docs;
        for (int64_t base = lo; base < hi; base += EX_THREADS) {
            int64_t row = base + threadIdx.x;
            bool ok = row < hi;
            double sim = -INFINITY;
            if (ok) {
                double dn = dnorm[row];
                if (qc != -1 && doc_coll[row] != qc) dn = 0.0;   // another collection: not a row of this search
                if (dn > 0.0) {
                    double dot = seq_dot_f64(docs + row * dim, lds_qv, dim);
                    sim = qn > 0.0 ? __ddiv_rn(dot, __dmul_rn(qn, dn)) : 0.0;
                }
            }
            tk.push(ok && sim > -INFINITY, sim, row);
        }
        int n = tk.finish();
        for (int i = threadIdx.x; i < k; i += EX_THREADS) {
            int64_t o = ((int64_t)q * EX_SLABS + slab) * k + i;
            slab_s[o] = i < n ? b_s[i] : -INFINITY;
            slab_id[o] = i < n ? b_id[i] : INT64_MAX;
        }
    }
}

// merges n_lists ranked lists of k_in per query (entry j of list l of query q at
// q * q_stride + l * list_stride + j) -> top k_out, ids + id_add, padded with (-inf, -1).
// GATED (thr_dense_topk_rows): a query whose query_scope is outside [0, P) gets the empty list -- its
// lists were never written.  The ungated flavour ignores query_scope and P.
template <bool GATED>
__global__ __launch_bounds__(256) void merge_lists(const double* __restrict__ in_s,
                                                   const int64_t* __restrict__ in_id,
                                                   int64_t q_stride, int64_t list_stride,
                                                   int n_lists, int k_in, int k_out,
                                                   int64_t id_add, uint32_t flag_value,
                                                   double* __restrict__ out_s,
                                                   int64_t* __restrict__ out_id,
                                                   int32_t* __restrict__ out_counts,
                                                   uint32_t* __restrict__ out_flags,
                                                   const uint32_t* __restrict__ skip_certified,
                                                   int32_t* __restrict__ n_done,
                                                   const int32_t* __restrict__ query_scope, int P) {
    if (skip_certified && (skip_certified[blockIdx.x] & THR_FLAG_CERTIFIED)) return;
    if (n_done && threadIdx.x == 0) atomicAdd(n_done, 1);
    __shared__ double b_s[EX_CAP];
    __shared__ int64_t b_id[EX_CAP];
    __shared__ int b_cnt;
    __shared__ double t_s;
    __shared__ int64_t t_id;
    const int q = blockIdx.x;
    bool live = true;
    if constexpr (GATED) live = query_scope[q] >= 0 && query_scope[q] < P;
    int n = 0;
    if (live) {
        BlockTopK<EX_CAP, EX_THREADS> tk;
        tk.init(b_s, b_id, &b_cnt, &t_s, &t_id, k_out);
        const int total = n_lists * k_in;
        for (int base = 0; base < total; base += blockDim.x) {
            int i = base + threadIdx.x;
            bool ok = i < total;
            double s = -INFINITY;
            int64_t id = INT64_MAX;
            if (ok) {
                int64_t o = (int64_t)q * q_stride + (int64_t)(i / k_in) * list_stride + (i % k_in);
                s = in_s[o];
                id = in_id[o];
            }
            tk.push(ok && s > -INFINITY && id >= 0 && id != INT64_MAX, s, id);
        }
        n = tk.finish();
    }
    for (int i = threadIdx.x; i < k_out; i += blockDim.x) {
        out_s[(int64_t)q * k_out + i] = i < n ? b_s[i] : -INFINITY;
        out_id[(int64_t)q * k_out + i] = i < n ? b_id[i] + id_add : -1;
    }
    if (threadIdx.x == 0) {
        if (out_counts) out_counts[q] = n;
        if (out_flags) out_flags[q] = flag_value;
    }
}

// Merge of at most EX_CAP candidates per query held entirely in LDS: the per-shard lists of the
// multi-GPU path (8 x <= 128).  The lists arrive ranked under (score desc, id asc), so an entry's
// place in the merged order is its own position plus, per other list, the number of entries ahead
// of it there (one binary search each) -- no sort.  "Ahead" is the total order extended by the list
// index: against a LOWER-numbered list an equal (score, id) pair counts as ahead, against a
// higher-numbered one it does not, so copies of one pair in several lists (shards that are not
// disjoint) take consecutive places instead of one place and a hole.  A list that is NOT ranked
// makes the block fall back to a bitonic sort of everything (same result, slower).
__global__ __launch_bounds__(256) void merge_ranked_lists(const double* __restrict__ in_s,
                                                          const int64_t* __restrict__ in_id,
                                                          int64_t q_stride, int64_t list_stride,
                                                          int n_lists, int k_in, int k_out,
                                                          double* __restrict__ out_s,
                                                          int64_t* __restrict__ out_id,
                                                          int32_t* __restrict__ out_counts) {
    __shared__ double b_s[EX_CAP];
    __shared__ int64_t b_id[EX_CAP];
    __shared__ int unsorted, n_valid;
    const int q = blockIdx.x;
    const int total = n_lists * k_in;
    if (threadIdx.x == 0) unsorted = 0, n_valid = 0;
    for (int i = threadIdx.x; i < EX_CAP; i += blockDim.x) {
        double sc = -INFINITY;
        int64_t id = INT64_MAX;
        if (i < total) {
            const int64_t o = (int64_t)q * q_stride + (int64_t)(i / k_in) * list_stride + (i % k_in);
            sc = in_s[o];
            id = in_id[o];
            if (!(sc > -INFINITY) || id < 0) sc = -INFINITY, id = INT64_MAX;
        }
        b_s[i] = sc;
        b_id[i] = id;
    }
    for (int i = threadIdx.x; i < k_out; i += blockDim.x) {
        out_s[(int64_t)q * k_out + i] = -INFINITY;
        out_id[(int64_t)q * k_out + i] = -1;
    }
    __syncthreads();
    int mine = 0;
    for (int i = threadIdx.x; i < total; i += blockDim.x) {
        mine += b_id[i] != INT64_MAX ? 1 : 0;
        if (i % k_in + 1 < k_in && better(b_s[i + 1], b_id[i + 1], b_s[i], b_id[i])) unsorted = 1;
    }
    if (mine) atomicAdd(&n_valid, mine);
    __syncthreads();
    if (!unsorted) {
        for (int i = threadIdx.x; i < total; i += blockDim.x) {
            const double ms = b_s[i];
            const int64_t mi = b_id[i];
            if (mi == INT64_MAX) continue;
            const int a = i / k_in;
            int rank = i % k_in;
            for (int b = 0; b < n_lists && rank < k_out; ++b) {
                if (b == a) continue;
                int lo = 0, hi = k_in;  // first position of list b that is not ahead of (ms, mi)
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    const double os = b_s[b * k_in + mid];
                    const int64_t oi = b_id[b * k_in + mid];
                    // b < a: not worse than mine; b > a: strictly better
                    const bool ahead = b < a ? !better(ms, mi, os, oi) : better(os, oi, ms, mi);
                    if (ahead) lo = mid + 1;
                    else hi = mid;
                }
                rank += lo;
            }
            if (rank < k_out) {
                out_s[(int64_t)q * k_out + rank] = ms;
                out_id[(int64_t)q * k_out + rank] = mi;
            }
        }
    } else {
        bitonic_sort_desc<EX_CAP>(b_s, b_id);
        for (int i = threadIdx.x; i < k_out && i < n_valid; i += blockDim.x) {
            out_s[(int64_t)q * k_out + i] = b_s[i];
            out_id[(int64_t)q * k_out + i] = b_id[i];
        }
    }
    if (threadIdx.x == 0 && out_counts) out_counts[q] = n_valid < k_out ? n_valid : k_out;
}

}  // namespace thr

using namespace thr;

extern "C" size_t thr_dense_exact_workspace_bytes(int64_t n_docs, int n_queries) {
    (void)n_docs;
    return (size_t)n_queries * EX_SLABS * THR_DENSE_MAX_K * (sizeof(double) + sizeof(int64_t));
}

extern "C" size_t thr_dense_rescue_workspace_bytes(int n_queries, int k) {
    if (n_queries <= 0 || k <= 0) return 0;
    return (size_t)n_queries * EX_SLABS * (size_t)k * (sizeof(double) + sizeof(int64_t));
}

// The exhaustive path of thr_dense_topk_exact and thr_dense_rescue: the slabs carved from the
// workspace (`need` bytes), exact_slab_topk on EX_SLABS x grid_y workgroups, merge_lists.  With
// `certified` (the flags of an earlier call) only the queries that lack THR_FLAG_CERTIFIED are redone.
static int exact_topk(const float* docs, const double* dnorm, int64_t n_docs, int dim, int64_t id_base,
                      const float* queries, int n_queries, int k, const int32_t* doc_coll,
                      const int32_t* query_coll, double* out_scores, int64_t* out_ids,
                      int32_t* out_counts, uint32_t* out_flags, void* workspace, size_t workspace_bytes,
                      size_t need, thr_stream_t stream, int grid_y, const uint32_t* certified,
                      int32_t* n_rescued) {
    clear_status();
    THR_RETURN_IF(!docs || !dnorm || !queries || !out_scores || !out_ids || !out_counts ||
                      !out_flags || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_docs <= 0 || n_queries <= 0 || k <= 0 || k > THR_DENSE_MAX_K, THR_ERR_INVALID);
    THR_RETURN_IF(dim <= 0 || dim % 4 != 0, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(workspace_bytes < need, THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    double* slab_s = (double*)workspace;
    int64_t* slab_id = (int64_t*)(slab_s + (size_t)n_queries * EX_SLABS * k);
    hipLaunchKernelGGL(exact_slab_topk, dim3(EX_SLABS, grid_y), dim3(EX_THREADS),
                       sizeof(float) * dim, st, docs, dnorm, n_docs, dim, queries, n_queries, k,
                       slab_s, slab_id, certified, doc_coll, query_coll, n_rescued);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(merge_lists<false>, dim3(n_queries), dim3(256), 0, st, slab_s, slab_id,
                       (int64_t)EX_SLABS * k, (int64_t)k, EX_SLABS, k, k, id_base,
                       THR_FLAG_CERTIFIED | THR_FLAG_EXACT, out_scores, out_ids, out_counts,
                       out_flags, certified, n_rescued, (const int32_t*)nullptr, 0);
    return launch_status();
}

// thr_dense_topk_rows (dense_rows.hip): the n_slabs lists of k of every query, [q][slab][k], ranked by
// the gated merge_lists
int thr::launch_merge_scoped(const double* slab_s, const int64_t* slab_id, int n_queries, int n_slabs, int k,
                             int64_t id_base, const int32_t* query_scope, int n_scopes, double* out_scores,
                             int64_t* out_ids, int32_t* out_counts, uint32_t* out_flags, hipStream_t st) {
    hipLaunchKernelGGL(merge_lists<true>, dim3(n_queries), dim3(256), 0, st, slab_s, slab_id,
                       (int64_t)n_slabs * k, (int64_t)k, n_slabs, k, k, id_base,
                       THR_FLAG_CERTIFIED | THR_FLAG_EXACT, out_scores, out_ids, out_counts, out_flags,
                       (const uint32_t*)nullptr, (int32_t*)nullptr, query_scope, n_scopes);
    return launch_status();
}

extern "C" int thr_dense_topk_exact(const float* docs, const double* dnorm, int64_t n_docs, int dim,
                                    int64_t id_base, const float* queries, int n_queries, int k,
                                    const int32_t* doc_coll, const int32_t* query_coll,
                                    double* out_scores, int64_t* out_ids, int32_t* out_counts,
                                    uint32_t* out_flags, void* workspace, size_t workspace_bytes,
                                    thr_stream_t stream) {
    return exact_topk(docs, dnorm, n_docs, dim, id_base, queries, n_queries, k, doc_coll, query_coll,
                      out_scores, out_ids, out_counts, out_flags, workspace, workspace_bytes,
                      thr_dense_exact_workspace_bytes(n_docs, n_queries), stream, n_queries, nullptr,
                      nullptr);
}

// Device-side completion of thr_dense_topk[_f16]: the queries whose flags lack
// THR_FLAG_CERTIFIED are redone on the exhaustive float64 path, in place, with no host read-back
// (workgroups of certified queries exit at once).  *n_rescued (device int32) is set to the number
// of redone queries: zeroed by the first kernel, incremented once per redone query by the second.
extern "C" int thr_dense_rescue(const float* docs, const double* dnorm, int64_t n_docs, int dim,
                                int64_t id_base, const float* queries, int n_queries, int k,
                                const int32_t* doc_coll, const int32_t* query_coll,
                                double* io_scores, int64_t* io_ids, int32_t* io_counts,
                                uint32_t* io_flags, int32_t* n_rescued, void* workspace,
                                size_t workspace_bytes, thr_stream_t stream) {
    // (a block takes up to 64 queries and skips the certified ones: a small grid)
    const int rows = (n_queries + 63) / 64 > 16 ? (n_queries + 63) / 64 : (n_queries < 16 ? n_queries : 16);
    return exact_topk(docs, dnorm, n_docs, dim, id_base, queries, n_queries, k, doc_coll, query_coll,
                      io_scores, io_ids, io_counts, io_flags, workspace, workspace_bytes,
                      thr_dense_rescue_workspace_bytes(n_queries, k), stream, rows, io_flags, n_rescued);
}

extern "C" int thr_merge_topk(const double* in_scores, const int64_t* in_ids, int n_queries,
                              int n_lists, int k_in, int64_t list_stride, int k_out,
                              double* out_scores, int64_t* out_ids, int32_t* out_counts,
                              thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!in_scores || !in_ids || !out_scores || !out_ids, THR_ERR_INVALID);
    THR_RETURN_IF(n_queries <= 0 || n_lists <= 0 || k_in <= 0 || k_out <= 0 || k_out > EX_CAP / 2,
                  THR_ERR_INVALID);
    if (list_stride == 0) list_stride = (int64_t)n_queries * k_in;  // [n_lists, n_queries, k_in]
    THR_RETURN_IF(list_stride < (int64_t)n_queries * k_in, THR_ERR_INVALID);
    if ((int64_t)n_lists * k_in <= EX_CAP) {
        hipLaunchKernelGGL(merge_ranked_lists, dim3(n_queries), dim3(256), 0, (hipStream_t)stream,
                           in_scores, in_ids, (int64_t)k_in, list_stride, n_lists, k_in, k_out,
                           out_scores, out_ids, out_counts);
        return launch_status();
    }
    hipLaunchKernelGGL(merge_lists<false>, dim3(n_queries), dim3(256), 0, (hipStream_t)stream, in_scores,
                       in_ids, (int64_t)k_in, list_stride, n_lists, k_in, k_out,
                       (int64_t)0, 0u, out_scores, out_ids, out_counts, (uint32_t*)nullptr,
                       (const uint32_t*)nullptr, (int32_t*)nullptr, (const int32_t*)nullptr, 0);
    return launch_status();
}
