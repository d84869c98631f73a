// Diversified top-k on the device (include/thr_hip_diversify.h holds the contract): Maximal Marginal
// Relevance over the candidates of a fused list, the similarities taken from the index's float32 rows
// under the cosine contract of the dense channel (sequential float64 sum in dimension order).
//
// One workgroup per query, one thread per position of the list (n <= THR_RRF_MAX_TOP_K), the block
// rounded up to whole waves.  A thread keeps its candidate's rel, pen, row and norm in registers for the
// whole selection; LDS holds the newly selected row and one staging tile per wave.
//
// Similarities are lazy: after a selection every remaining candidate takes its sim against the new row
// alone and folds it into pen -- (steps - 1) * m dot products, no Gram matrix.  The order of a sum is
// the contract, so a dot product is never split across lanes: lane l of wave w owns position 64 w + l
// and walks its dimensions in order.  The global reads still coalesce: a wave stages MMR_TILE
// dimensions of its 64 rows through LDS, 8 lanes on the 128 bytes of one row, 8 rows per load
// instruction, written at a row stride of MMR_TILE + 1 floats so that both the stores (rows r .. r + 3,
// 4 (l % 8) + j) and the per-lane reads (33 l + k) fall on 32 distinct banks.  The loads of tile i + 1
// are in flight while tile i is summed; which rows a lane loads comes from the wave's own
// registers by shuffle.
//
// Every index is checked: a position at or beyond cnt, an unusable score, an id outside
// [id_base, id_base + n_docs) and a row with dnorm <= 0 have no row number (-1) and are never
// dereferenced (where such a position's turn comes in a wave's load pattern, the selected row is read).  No atomics; the reductions are fixed trees: the same bits every run.
#include "thr_common.hpp"

#include "../../include/thr_hip_diversify.h"

namespace thr {

constexpr int MMR_TILE = 32;                     // dimensions staged per tile: 128 bytes of a row
constexpr int MMR_STRIDE = MMR_TILE + 1;         // floats between two rows of a tile
constexpr int MMR_GRANULES = MMR_TILE / 4;       // float4 pieces of a row's tile: the lanes on one row
constexpr int MMR_ROWS_PER_LOAD = WAVE / MMR_GRANULES;
constexpr int MMR_LOADS = WAVE / MMR_ROWS_PER_LOAD;
constexpr int MMR_MAX_THREADS = THR_RRF_MAX_TOP_K;
constexpr int MMR_MAX_WAVES = MMR_MAX_THREADS / WAVE;
constexpr double MMR_SCORE_MAX = 1e300;          // a candidate's |score| is at most this

static size_t mmr_lds_bytes(int threads, int dim) {
    return sizeof(float) * ((size_t)dim + (size_t)(threads / WAVE) * WAVE * MMR_STRIDE);
}

// (value, position) of the better of two: the greater value, the lower position on a tie; position -1 = none
__device__ __forceinline__ void mmr_take(double& v, int& p, double ov, int op) {
    if (op >= 0 && (p < 0 || ov > v || (ov == v && op < p))) {
        v = ov;
        p = op;
    }
}

__global__ __launch_bounds__(MMR_MAX_THREADS, 4) void mmr_select_kernel(
    const int64_t* __restrict__ ids, const double* __restrict__ scores, const int32_t* __restrict__ counts, int n,
    const float* __restrict__ docs, const double* __restrict__ dnorm, int64_t n_docs, int dim, int64_t id_base,
    double lam, double one_minus_lam, int top_k, int64_t* __restrict__ out_ids, double* __restrict__ out_scores,
    int32_t* __restrict__ out_pos, double* __restrict__ out_mmr, int32_t* __restrict__ out_counts) {
    extern __shared__ __attribute__((aligned(16))) float mmr_lds[];
    __shared__ double red_a[MMR_MAX_WAVES], red_b[MMR_MAX_WAVES];
    __shared__ int red_i[MMR_MAX_WAVES];
    __shared__ int sel_row;
    __shared__ double sel_norm;

    const int p = threadIdx.x;
    const int lane = p & (WAVE - 1), wave = p >> 6;
    const int waves = blockDim.x >> 6;
    float* sel = mmr_lds;                                                 // [dim]: the newly selected row
    float* tile = sel + dim + (size_t)wave * WAVE * MMR_STRIDE;           // [WAVE][MMR_STRIDE]: this wave's staging tile
    const int64_t q = blockIdx.x;

    int cnt = n;
    if (counts) {
        cnt = counts[q];
        cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    }
    // ---- this position: candidate?  row?
    bool cand = false;
    int64_t id = -1;
    double sc = 0.0, nrm = 0.0;
    int32_t row = -1;
    if (p < cnt) {
        id = ids[q * n + p];
        sc = scores[q * n + p];
        cand = fabs(sc) <= MMR_SCORE_MAX;      // false for NaN and +-inf
        if (cand && id >= id_base) {
            const uint64_t r = (uint64_t)id - (uint64_t)id_base;
            if (r < (uint64_t)n_docs) {
                const double d = dnorm[r];
                if (d > 0.0) {
                    row = (int32_t)r;
                    nrm = d;
                }
            }
        }
    }

    // ---- m, lo, hi over the candidates
    double lo = cand ? sc : INFINITY, hi = cand ? sc : -INFINITY;
    int m = __popcll(__ballot(cand));
#pragma unroll
    for (int o = WAVE / 2; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, WAVE));
        hi = fmax(hi, __shfl_xor(hi, o, WAVE));
    }
    if (lane == 0) {
        red_a[wave] = lo;
        red_b[wave] = hi;
        red_i[wave] = m;
    }
    __syncthreads();
    lo = red_a[0];
    hi = red_b[0];
    m = red_i[0];
    for (int w = 1; w < waves; ++w) {
        lo = fmin(lo, red_a[w]);
        hi = fmax(hi, red_b[w]);
        m += red_i[w];
    }
    __syncthreads();      // (the reduction arrays are written again below)
    const double rel = hi == lo ? 1.0 : __ddiv_rn(__dsub_rn(sc, lo), __dsub_rn(hi, lo));
    const double lam_rel = __dmul_rn(lam, rel);
    const int steps = m < top_k ? m : top_k;

    if (p == 0) out_counts[q] = steps;
    if (p >= steps && p < top_k) {      // padding behind the count
        const int64_t o = q * top_k + p;
        out_ids[o] = -1;
        out_scores[o] = -INFINITY;
        out_pos[o] = -1;
        if (out_mmr) out_mmr[o] = -INFINITY;
    }

    bool open = cand;                   // a candidate not selected yet
    double pen = -INFINITY;
    const int dim4 = dim >> 2;
#pragma unroll 1
    for (int t = 0; t < steps; ++t) {
        // ---- the unselected candidate of greatest value, the lowest position on a tie
        double v = t == 0 ? lam_rel : __dsub_rn(lam_rel, __dmul_rn(one_minus_lam, pen));
        int bp = open ? p : -1;
#pragma unroll
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            const double ov = __shfl_xor(v, o, WAVE);
            const int op = __shfl_xor(bp, o, WAVE);
            mmr_take(v, bp, ov, op);
        }
        if (lane == 0) {
            red_a[wave] = v;
            red_i[wave] = bp;
        }
        __syncthreads();
        v = red_a[0];
        bp = red_i[0];
        for (int w = 1; w < waves; ++w) mmr_take(v, bp, red_a[w], red_i[w]);
        if (bp < 0) break;              // (values that compare with nothing: outside the contract; uniform)
        if (p == bp) {
            const int64_t o = q * top_k + t;
            out_ids[o] = id;
            out_scores[o] = sc;
            out_pos[o] = p;
            if (out_mmr) out_mmr[o] = v;
            open = false;
            sel_row = row;
            sel_norm = nrm;
        }
        if (t == steps - 1) break;
        __syncthreads();
        const int32_t srow = sel_row;
        const double snorm = sel_norm;
        if (srow < 0) {                 // the selected candidate has no row: similarity 0.0 to everything
            if (open) pen = 0.0 > pen ? 0.0 : pen;
            continue;
        }
        // ---- the selected row into LDS
        {
            const float4* src = reinterpret_cast<const float4*>(docs + (int64_t)srow * dim);
            for (int i = p; i < dim4; i += blockDim.x) reinterpret_cast<float4*>(sel)[i] = src[i];
        }
        // ---- sim of every open candidate with a row against it: tiles of this wave's 64 rows through LDS
        const bool mine = open && row >= 0;
        const bool any = __ballot(mine) != 0ull;        // wave-uniform: a wave without work only keeps the barriers
        const int g = lane & (MMR_GRANULES - 1), r0 = lane / MMR_GRANULES;
        // The rows of this wave's 64 positions are in its lanes' registers: load i of lane l is for position
        // i * MMR_ROWS_PER_LOAD + l / MMR_GRANULES of the wave.  A position without work (selected, no candidate,
        // no row) loads the selected row in its place -- a row that exists -- so no load and no store is
        // conditional; nobody reads what it stages.  In the last, partial tile a granule past the row's end is
        // moved back onto the row's last one: the columns it fills are past dim - d0 and are not summed.
        const float* src[MMR_LOADS];
#pragma unroll
        for (int i = 0; i < MMR_LOADS; ++i) {
            const int32_t r = __shfl(mine ? row : srow, i * MMR_ROWS_PER_LOAD + r0, WAVE);
            src[i] = docs + (int64_t)r * dim;
        }
        float4 reg[MMR_LOADS];                          // the next tile, in flight while this one is summed
        auto fetch = [&](int d0) {
            if (!any || d0 >= dim) return;              // (wave-uniform)
            const int at = d0 + 4 * g < dim ? d0 + 4 * g : dim - 4;
#pragma unroll
            for (int i = 0; i < MMR_LOADS; ++i) reg[i] = *reinterpret_cast<const float4*>(src[i] + at);
        };
        double acc = 0.0;
        const float* my = tile + lane * MMR_STRIDE;
        float* dst = tile + r0 * MMR_STRIDE + 4 * g;
        fetch(0);
#pragma unroll 1
        for (int d0 = 0; d0 < dim; d0 += MMR_TILE) {      // registers -> LDS, barrier, the next loads, the sum, barrier
            if (any) {
#pragma unroll
                for (int i = 0; i < MMR_LOADS; ++i) {
                    float* d = dst + i * MMR_ROWS_PER_LOAD * MMR_STRIDE;
                    d[0] = reg[i].x;
                    d[1] = reg[i].y;
                    d[2] = reg[i].z;
                    d[3] = reg[i].w;
                }
            }
            __syncthreads();
            fetch(d0 + MMR_TILE);
            if (mine) {
                const float* s = sel + d0;
                if (d0 + MMR_TILE <= dim) {
#pragma unroll 4
                    for (int k = 0; k < MMR_TILE; ++k) acc = fma((double)my[k], (double)s[k], acc);
                } else {
                    for (int k = 0; k < dim - d0; ++k) acc = fma((double)my[k], (double)s[k], acc);
                }
            }
            __syncthreads();
        }
        if (mine) {
            const double sim = __ddiv_rn(acc, __dmul_rn(nrm, snorm));
            pen = sim > pen ? sim : pen;
        } else if (open) {
            pen = 0.0 > pen ? 0.0 : pen;
        }
    }
}

}  // namespace thr

using namespace thr;

// Largest gridDim.x of the current device (2^31 - 1 when it cannot be asked)
static int mmr_max_grid_x() {
    static int x = 0;
    if (!x) {
        int dev = 0, px = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) px = prop.maxGridSize[0];
        x = px > 0 ? px : 0x7fffffff;
    }
    return x;
}

extern "C" int thr_mmr_select(const int64_t* ids, const double* scores, const int32_t* counts, int n_queries, int n,
                              const float* docs, const double* dnorm, int64_t n_docs, int dim, int64_t id_base,
                              double lam, int top_k, int64_t* out_ids, double* out_scores, int32_t* out_pos,
                              double* out_mmr, int32_t* out_counts, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(dim < 4 || dim > THR_DENSE_ANYDIM_MAX || dim % 4 != 0, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n < 1 || n > THR_RRF_MAX_TOP_K, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(top_k < 1 || top_k > n, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n_docs > 0x7fffffffll, THR_ERR_UNSUPPORTED);      // a row number is an int32
    THR_RETURN_IF(!ids || !scores || !docs || !dnorm || !out_ids || !out_scores || !out_pos || !out_counts,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_queries <= 0 || n_docs <= 0, THR_ERR_INVALID);
    THR_RETURN_IF(!(lam >= 0.0 && lam <= 1.0), THR_ERR_INVALID);     // NaN included
    const int threads = (n + WAVE - 1) / WAVE * WAVE;
    const size_t lds = mmr_lds_bytes(threads, dim);
    const double one_minus_lam = 1.0 - lam;                          // formed once
    const int gx = mmr_max_grid_x();
    // queries sit on gridDim.x: a batch above the device's limit goes out in slices of at most that many
    for (int q0 = 0; q0 < n_queries; q0 += gx) {
        const int nq = n_queries - q0 < gx ? n_queries - q0 : gx;
        const int64_t in = (int64_t)q0 * n, out = (int64_t)q0 * top_k;
        const int rc = launch_lds(mmr_select_kernel, dim3((unsigned)nq), dim3((unsigned)threads), lds, (hipStream_t)stream,
                                  ids + in, scores + in, counts ? counts + q0 : nullptr, n, docs, dnorm, n_docs, dim,
                                  id_base, lam, one_minus_lam, top_k, out_ids + out, out_scores + out, out_pos + out,
                                  out_mmr ? out_mmr + out : nullptr, out_counts + q0);
        if (rc != THR_OK) return rc;
        if (n_queries - q0 <= gx) break;      // (q0 + gx may not fit an int)
    }
    return THR_OK;
}
