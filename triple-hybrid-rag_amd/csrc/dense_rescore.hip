// Dense channel, K4b of the pipeline (dense.hip): the shortlist of select_band (dense_select.hip)
// re-scored in float64 SEQUENTIAL sums (the oracle's contract), rank-sorted under (score desc,
// id asc) and certified with the scan's error bound.  One block (2 waves) per query.
#include "dense_common.hpp"

namespace thr {

constexpr int RS_STRIDE = 9;       // float4 slots per staged row: 8 + 1 pad (conflict-free b128)
// K4b: float64 scores of the shortlist, rank sort, certificate.  NB = the rows it can take: the
// first launch (256) serves every query whose shortlist fits, the second (1024) the few whose
// band was wider (score distributions squeezed into a narrow range: anisotropic embeddings put
// hundreds of rows within the f16 error band of the k-th); each exits at once on the others.
//
// Two waves per query, 64 rows per wave (every lane holds a row).  What bounds it is the gather:
// 2048 queries x ~105 rows x 3 KB = 645 MB read as scattered 128-byte lines, 4.3 TB/s at 150 us --
// four waves of 32 rows, two of 64, two or four chunks in flight, three to six workgroups per CU
// all land within 5 % of each other; 256-byte steps per row (half the occupancy) are 17 % slower.  The query is one more row of the shortlist: its dot
// product with itself, in the same sequential order, is ||q||^2.
constexpr int RR_WAVES = 2, RR_THREADS = 64 * RR_WAVES, RR_ROWS = 64;
static size_t rescore_lds_bytes(int dim) {   // the query as float64 | the waves' stage tiles
    return sizeof(double) * dim + sizeof(float4) * RR_WAVES * RR_ROWS * RS_STRIDE;
}
// One pass of a wave over its (up to) 8 U staged rows: U row groups of 8 per 32-dim chunk, 16 / U
// (at most 8) chunks of them in flight in registers.  Lanes of the groups that are not staged
// compute on stale LDS words; their slots are beyond the list and nothing reads the result.
// dim / 32 is a multiple of 8 for every row length the tuned scans are built for; TAIL is the form for
// the other lengths of dense_scan_anydim (any dim / 32 >= 1): the chunks in flight never pass the
// row's last one and the trip of a chunk that does not exist is skipped (wave-uniform), so the sum
// is the same sequential one in dimension order.
template <int U, bool TAIL = false>
//
// dot += x * y as ONE v_fma_f64 per element: the product of two float32 values is exact in
// float64 (48 significant bits), so fma(x, y, dot) rounds the same real number as the oracle's
// separate multiply and add -- the same bits at half the float64 instructions; the query is
// converted once per workgroup (q64), the rows as they are read.
__device__ __forceinline__ double rescore_pass(const f32x4* (&rp)[8], f32x4* stage, const double* q64,
                                               int nchunk, int lane, int lrow, int lch) {
    constexpr int D = U >= 2 ? 16 / U : 8;
    f32x4 nxt[D][U];
#pragma unroll
    for (int dd = 0; dd < D; ++dd)
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[dd][u] = rp[u][8 * (TAIL && dd >= nchunk ? nchunk - 1 : dd)];   // (else nchunk >= D)
    double dot = 0.0;
#pragma unroll 1
    for (int ck0 = 0; ck0 < nchunk; ck0 += D) {
#pragma unroll
        for (int dd = 0; dd < D; ++dd) {
            const int ck = ck0 + dd;
            if (TAIL && ck >= nchunk) break;
#pragma unroll
            for (int u = 0; u < U; ++u) stage[(lrow + 8 * u) * RS_STRIDE + lch] = nxt[dd][u];
            // (the last trips re-request the last chunk)
            const int cn = ck + D < nchunk ? ck + D : nchunk - 1;
#pragma unroll
            for (int u = 0; u < U; ++u) nxt[dd][u] = rp[u][8 * cn];
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const f32x4* src = stage + lane * RS_STRIDE;
            const double* qv = q64 + 32 * ck;
#pragma unroll
            for (int ch = 0; ch < 8; ++ch) {
                const f32x4 x = src[ch];
                dot = __fma_rn((double)x.x, qv[4 * ch + 0], dot);
                dot = __fma_rn((double)x.y, qv[4 * ch + 1], dot);
                dot = __fma_rn((double)x.z, qv[4 * ch + 2], dot);
                dot = __fma_rn((double)x.w, qv[4 * ch + 3], dot);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }
    return dot;
}

// TAIL: rescore_pass's tail form, for the row lengths of dense_scan_anydim with dim % 256 != 0
template <int NB, bool TAIL = false>
__global__ __launch_bounds__(RR_THREADS, 3) void rescore_rank(
    const float* __restrict__ docs, const double* __restrict__ dnorm, int dim, int64_t id_base,
    const float* __restrict__ queries, int k, double eps32, double doc_relerr,
    const float* __restrict__ qerr, const int32_t* __restrict__ sel_rows,
    const int32_t* __restrict__ sel_meta, double* __restrict__ out_scores,
    int64_t* __restrict__ out_ids, int32_t* __restrict__ out_counts, uint32_t* __restrict__ out_flags) {
    const int q = blockIdx.x;
    const int ns = sel_meta[4 * q + 0];
    if (NB == THR_DENSE_MAX_K ? ns > THR_DENSE_MAX_K : ns <= THR_DENSE_MAX_K) return;
    const float floor32 = __uint_as_float((uint32_t)sel_meta[4 * q + 1]);
    const bool overflow = sel_meta[4 * q + 2] != 0;
    extern __shared__ float4 lds_sel[];  // [dim/2] the query as float64 | RR_WAVES stage tiles
    __shared__ double s_s[NB], o_s[NB];
    __shared__ int64_t s_id[NB], o_id[NB];
    __shared__ double s_qn;
    __shared__ int n_valid;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double eq = qerr ? (double)qerr[q] : 0.0;
    const double eps = eps32 + doc_relerr * (1.0 + eq) + eq;
    double* q64 = reinterpret_cast<double*>(lds_sel);
    for (int i = threadIdx.x; i < dim; i += RR_THREADS) q64[i] = (double)queries[(int64_t)q * dim + i];
    for (int i = threadIdx.x; i < NB; i += RR_THREADS) {
        s_s[i] = o_s[i] = -INFINITY;
        s_id[i] = i < ns ? (int64_t)sel_rows[(int64_t)q * SEL_BIG_BAND + i] : INT64_MAX;
        o_id[i] = INT64_MAX;
    }
    if (threadIdx.x == 0) n_valid = 0;
    __syncthreads();

    // ---- float64 rescoring: SEQUENTIAL sums (the oracle's contract), one lane per row ----
    // (native vectors, not HIP's float4 class: see dense_scan_mfma2 -- a float4 array that is
    // copied into LDS is demoted to scratch memory)
    f32x4* stage = reinterpret_cast<f32x4*>(lds_sel + dim / 2) + wave * (RR_ROWS * RS_STRIDE);
    const f32x4* docs4 = reinterpret_cast<const f32x4*>(docs);
    const int lrow = lane >> 3, lch = lane & 7;
    const int cpr = dim / 4, nchunk = dim / 32;
    const f32x4* q4 = reinterpret_cast<const f32x4*>(queries + (int64_t)q * dim);
    // (the row norm of this thread's first shortlist slot: requested now, used after the loop)
    const double dn_first = (int)threadIdx.x < ns ? dnorm[s_id[threadIdx.x]] : 0.0;
    for (int b0 = 0; b0 <= ns; b0 += RR_WAVES * RR_ROWS) {
        // slot of (wave, staged row r) is b0 + wave + RR_WAVES r; slot ns is the query itself;
        // a lane loads 16 bytes of rows lrow + 8 u (8 lanes per 128-byte line)
        const int rem = ns - b0 - wave;          // this wave's slots of the pass: r <= rem / RR_WAVES
        if (rem < 0) continue;                   // (wave-uniform)
        const f32x4* rp[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            int j = b0 + wave + RR_WAVES * (lrow + 8 * u);
            j = j < ns ? j : ns;
            rp[u] = (j < ns ? docs4 + s_id[j] * cpr : q4) + lch;
        }
        const int jm = b0 + wave + RR_WAVES * lane;  // this lane's own slot
        // A short list (a shard under the common floor rescores ~k / G rows, a top-10 search ~12)
        // fills only the first row groups of the wave: it stages those alone and keeps more
        // chunks of them in flight instead -- the pass is a chain of memory round trips.
        const int groups = rem / RR_WAVES / 8 + 1;
        double dot;
        if (groups <= 1) dot = rescore_pass<1, TAIL>(rp, stage, q64, nchunk, lane, lrow, lch);
        else if (groups <= 2) dot = rescore_pass<2, TAIL>(rp, stage, q64, nchunk, lane, lrow, lch);
        else if (groups <= 4) dot = rescore_pass<4, TAIL>(rp, stage, q64, nchunk, lane, lrow, lch);
        else dot = rescore_pass<8, TAIL>(rp, stage, q64, nchunk, lane, lrow, lch);
        if (jm < ns) s_s[jm] = dot;               // the raw dot product for now
        else if (jm == ns) s_qn = __dsqrt_rn(dot);  // ||q||
    }
    __syncthreads();
    for (int p = threadIdx.x; p < ns; p += RR_THREADS) {
        const int64_t row = s_id[p];
        const double qn = s_qn, dn = p == (int)threadIdx.x ? dn_first : dnorm[row], dot = s_s[p];
        double sim = -INFINITY;
        if (dn > 0.0) sim = qn > 0.0 ? __ddiv_rn(dot, __dmul_rn(qn, dn)) : 0.0;
        s_s[p] = sim;
        s_id[p] = sim == -INFINITY ? INT64_MAX : row + id_base;
    }
    __syncthreads();
    // rank sort: ids are distinct, so (score desc, id asc) is a strict order on the valid rows;
    // rows without an embedding all carry (-inf, INT64_MAX), which is what o_s/o_id hold already
    for (int p = threadIdx.x; p < ns; p += RR_THREADS) {
        const double ms = s_s[p];
        const int64_t mi = s_id[p];
        if (mi == INT64_MAX) continue;
        int rank = 0;
        for (int i = 0; i < ns; ++i) rank += better(s_s[i], s_id[i], ms, mi) ? 1 : 0;
        o_s[rank] = ms;
        o_id[rank] = mi;
    }
    __syncthreads();

    // results + certificate
    int mine_valid = 0;
    for (int i = threadIdx.x; i < k; i += RR_THREADS) {
        const bool ok = o_s[i] > -INFINITY;
        mine_valid += ok ? 1 : 0;
        out_scores[(int64_t)q * k + i] = ok ? o_s[i] : -INFINITY;
        out_ids[(int64_t)q * k + i] = ok ? o_id[i] : -1;
    }
    if (mine_valid) atomicAdd(&n_valid, mine_valid);
    __syncthreads();
    if (threadIdx.x == 0) {
        const int valid = n_valid;
        uint32_t flag = overflow ? THR_FLAG_OVERFLOW : 0u;
        bool cert;
        if (overflow) {
            cert = false;
        } else if (floor32 == -INFINITY) {
            cert = true;  // every row with an embedding was rescored
        } else {
            // rows outside the shortlist have scan score <= floor32, hence true
            // cosine <= floor32/||q|| + eps; the k-th best must clear that strictly -- this
            // shard's own k-th best, or the k-th best of all the shards, of which gF / ||q|| is a
            // lower bound (then the list may be shorter than k: the rest is on other shards).
            const float gF = __uint_as_float((uint32_t)sel_meta[4 * q + 3]);
            const bool own = valid >= k && s_qn > 0.0 && (o_s[k - 1] - (double)floor32 / s_qn) > eps;
            const bool all = gF > -INFINITY && s_qn > 0.0 &&
                             ((double)gF / s_qn - (double)floor32 / s_qn) > eps;
            cert = own || all;
        }
        out_flags[q] = flag | (cert ? THR_FLAG_CERTIFIED : 0u);
        out_counts[q] = valid;
    }
}

// K4b: every query whose shortlist fits 256 rows, then the few whose band was wider.  dim % 256 == 0:
// the instantiation without the tail.  Beyond dim 1024 the query as float64 and the stage tiles (50 KiB
// of dynamic LDS at dim 4096) pass 64 KiB together with the 1024-row kernel's 32 KiB of static lists:
// those launches raise the function attribute first.
int launch_rescore(const DensePlan& P, const DenseIndex& X, const DenseBatch& B) {
    const bool tail = X.dim % 256 != 0, big_lds = X.dim > 1024;
    for (auto kern : {tail ? rescore_rank<THR_DENSE_MAX_K, true> : rescore_rank<THR_DENSE_MAX_K, false>,
                      tail ? rescore_rank<SEL_BIG_BAND, true> : rescore_rank<SEL_BIG_BAND, false>}) {
        int rc;
        if (big_lds) {
            rc = launch_lds(kern, dim3(B.n_queries), dim3(RR_THREADS), rescore_lds_bytes(X.dim), B.st,
                            X.docs, X.dnorm, X.dim, X.id_base, B.queries, B.k, scan_eps(X.dim),
                            X.doc_rel_err, (const float*)P.qerr, (const int32_t*)P.sel_rows,
                            (const int32_t*)P.sel_meta, B.out_scores, B.out_ids, B.out_counts, B.out_flags);
        } else {
            hipLaunchKernelGGL(kern, dim3(B.n_queries), dim3(RR_THREADS), rescore_lds_bytes(X.dim), B.st,
                               X.docs, X.dnorm, X.dim, X.id_base, B.queries, B.k, scan_eps(X.dim),
                               X.doc_rel_err, P.qerr, P.sel_rows, P.sel_meta, B.out_scores, B.out_ids,
                               B.out_counts, B.out_flags);
            rc = launch_status();
        }
        if (rc) return rc;
    }
    return THR_OK;
}

}  // namespace thr
