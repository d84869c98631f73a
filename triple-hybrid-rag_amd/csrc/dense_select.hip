// Dense channel, selection: K2, K3b and K4a of the pipeline (dense.hip) and the shards' common floor.
// kth_select (kth_select_top behind the register-resident scans, whose sample pass keeps only each
// lane's best) turns the sample scores into the scan's threshold, bucket_candidates splits a tile's
// candidate list by query, select_band picks the rows that get a float64 score (or, before the
// shards' exchange, the query's top-m lower bounds), dense_floor_kernel is the k-th largest of the
// exchanged bounds.  The launch functions at the end are what dense.hip calls.
#include "dense_common.hpp"

namespace thr {

// K3b: split a tile's mixed candidate list into the per-query lists K4 reads.  Each block
// owns a contiguous slice of the list and reserves its output ranges with ONE global atomic
// per query (counts first, in LDS), instead of one returning global atomic per entry.
constexpr int BUCKET_BLOCKS = 32;
__global__ __launch_bounds__(256) void bucket_candidates(const int* __restrict__ tile_cnt,
                                                         const Cand* __restrict__ tile_list,
                                                         int tile_cap, int qtile, int row_bits,
                                                         int* __restrict__ cand_cnt,
                                                         Cand* __restrict__ cand) {
    __shared__ int count[128], base[128], fill[128];
    const uint32_t row_mask = (1u << row_bits) - 1u;
    const int tile = blockIdx.y;
    int n = tile_cnt[tile];
    n = n < tile_cap ? n : tile_cap;
    const int per = (n + gridDim.x - 1) / gridDim.x;
    const int lo = blockIdx.x * per, hi = lo + per < n ? lo + per : n;
    const Cand* list = tile_list + (int64_t)tile * tile_cap;
    if (threadIdx.x < 128) count[threadIdx.x] = fill[threadIdx.x] = 0;
    __syncthreads();
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x)
        atomicAdd(&count[list[i].doc >> row_bits], 1);
    __syncthreads();
    if (threadIdx.x < qtile && count[threadIdx.x] > 0)
        base[threadIdx.x] = atomicAdd(&cand_cnt[tile * qtile + threadIdx.x], count[threadIdx.x]);
    __syncthreads();
    for (int i = lo + threadIdx.x; i < hi; i += blockDim.x) {
        const Cand e = list[i];
        const int ql = (int)(e.doc >> row_bits);
        const int p = base[ql] + atomicAdd(&fill[ql], 1);
        if (p < CAND_CAP)
            cand[(int64_t)(tile * qtile + ql) * CAND_CAP + p] = Cand{e.score, e.doc & row_mask};
    }
}

// ---------------------------------------------------------------------------
// 8-bit-digit radix select of the kk-th largest key (block-wide) over items each thread
// enumerates itself: keyfn(u) -> uint32 order-preserving key, u in [0, my_n) (the candidate lists
// of select_band: a thread's items are my_ptr[u * my_stride]).  Returns the key.
// hist = 256 ints of LDS, bc = 4 ints of LDS.
// ---------------------------------------------------------------------------
template <typename KeyFn>
__device__ uint32_t block_radix_select_local(KeyFn keyfn, int my_n, int kk, int* hist, int* bc) {
    uint32_t prefix = 0, mask = 0;
    int remaining = kk;
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = threadIdx.x; i < 256; i += blockDim.x) hist[i] = 0;
        __syncthreads();
        for (int u0 = 0; u0 < my_n; u0 += 8) {
            uint32_t key[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) key[u] = u0 + u < my_n ? keyfn(u0 + u) : 0u;
#pragma unroll
            for (int u = 0; u < 8; ++u)
                if (u0 + u < my_n && (key[u] & mask) == prefix) atomicAdd(&hist[(key[u] >> shift) & 255], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            int cum = 0, b = 255;
            for (; b > 0; --b) {
                if (cum + hist[b] >= remaining) break;
                cum += hist[b];
            }
            bc[0] = b;
            bc[1] = cum;
        }
        __syncthreads();
        remaining -= bc[1];
        prefix |= (uint32_t)bc[0] << shift;
        mask |= 255u << shift;
        __syncthreads();
    }
    return prefix;
}

// ---------------------------------------------------------------------------
// Two-pass LOWER BOUND of the kk-th largest key: 12-bit digits over the top 24 key bits, the
// low 8 bits of the result are zero.  For a float key that is a value at most 2^-15 (relative)
// below the true kk-th -- all a threshold needs (it only has to let the top kk through), at
// half the passes of the exact select.  key(i) is evaluated for i in [0, n); the bins of a pass
// are searched by all threads (per-thread partial sums + one wave scan).
// hist = 4096 ints of LDS, aux = 8 ints of LDS.  blockDim.x must be 256.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void coarse_find_bin(const int* hist, int remaining, int* aux) {
    // thread t owns the 16 bins [4096 - 16(t+1), 4096 - 16t): t = 0 holds the largest keys
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    const int top = CS_BINS - 16 * t;
    int mine = 0;
#pragma unroll
    for (int b = 1; b <= 16; ++b) mine += hist[top - b];
    int incl = mine;  // inclusive scan over t within the wave
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(incl, o, WAVE);
        if (lane >= o) incl += v;
    }
    if (lane == 63) aux[4 + w] = incl;
    if (t == 0) aux[0] = 0, aux[1] = -1;
    __syncthreads();
    int before = 0;
    for (int x = 0; x < w; ++x) before += aux[4 + x];
    incl += before;
    const int excl = incl - mine;
    if (excl < remaining && remaining <= incl) {
        int cum = excl, b = top - 1;
        for (; b > top - 16; --b) {
            if (cum + hist[b] >= remaining) break;
            cum += hist[b];
        }
        aux[0] = b;
        aux[1] = cum;
    }
    __syncthreads();
    if (aux[1] < 0) {  // fewer than `remaining` keys in all: bin 0 (cannot happen for kk <= n)
        if (t == 255) aux[0] = 0, aux[1] = incl - hist[0];
        __syncthreads();
    }
}

template <typename KeyFn>
__device__ uint32_t block_coarse_select(KeyFn keyfn, int n, int kk, int* hist, int* aux) {
    uint32_t prefix = 0;
    int remaining = kk;
#pragma unroll 1
    for (int pass = 0; pass < 2; ++pass) {
        for (int i = threadIdx.x; i < CS_BINS; i += 256) hist[i] = 0;
        __syncthreads();
        for (int base = threadIdx.x; base < n; base += 8 * 256) {
            uint32_t key[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * 256;
                key[u] = i < n ? keyfn(i) : 0u;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = base + u * 256;
                if (i >= n) continue;
                if (pass == 0) atomicAdd(&hist[key[u] >> 20], 1);
                else if ((key[u] >> 20) == (prefix >> 20)) atomicAdd(&hist[(key[u] >> 8) & 4095], 1);
            }
        }
        __syncthreads();
        coarse_find_bin(hist, remaining, aux);
        remaining -= aux[1];
        prefix |= (uint32_t)aux[0] << (pass == 0 ? 20 : 8);
        __syncthreads();
    }
    return prefix;
}
// float value of a truncated key; a truncated -inf key decodes to NaN: map it back
__device__ __forceinline__ float coarse_value(uint32_t key) {
    const float v = fkey_inv(key);
    return v == v ? v : -INFINITY;
}

// The queries a scan must not emit for, judged on the values THE SCAN multiplies (half_image: their
// float16 image, as every f16 scan rounds them; else the float32 values of the fp32 scan).  Such a
// query gets a threshold nothing passes, ends up uncertified and is answered by the exhaustive path,
// which works in float64 from the float32 values.
//   Q_VOID  a padding row of the tile, or no value the scan can tell from zero: an all-zero vector
//           (-0.0 included), a float16 image that is all zero (every |v| <= 2^-25), float32 values
//           all below 2^-96 (their products with the rows underflow, which eps32 does not cover).
//           Every row would tie at 0 and flood the tile's candidate list: tau = +inf.
//   Q_WILD  a value the scan's arithmetic leaves finite range with: a float16 image that holds an
//           infinity or a NaN (|v| >= 65520), a float32 value of 2^96 or more (or not finite: ||q||
//           x ||d|| may then overflow float32).  Scores of +inf would pass tau = +inf: tau = NaN,
//           which `score >= tau` is false for whatever the score.
constexpr int Q_LIVE = 0, Q_VOID = 1, Q_WILD = 2;
constexpr float F32_SCAN_LO = 0x1p-96f, F32_SCAN_HI = 0x1p96f;
__device__ int query_kind(const float* __restrict__ queries, int n_queries, int dim, int q,
                          bool half_image, int* flag) {
    if (threadIdx.x == 0) *flag = 0;
    __syncthreads();
    if (q < n_queries) {
        int f = 0;   // 1: a value that counts, 2: a value out of range
        for (int i = threadIdx.x; i < dim; i += blockDim.x) {
            const float v = queries[(int64_t)q * dim + i];
            const float a = fabsf(half_image ? (float)(_Float16)v : v);
            f |= (half_image ? a > 0.f : a >= F32_SCAN_LO) ? 1 : 0;
            f |= a < (half_image ? INFINITY : F32_SCAN_HI) ? 0 : 2;   // (NaN: out of range)
        }
        if (f) atomicOr(flag, f);
    }
    __syncthreads();
    const int f = *flag;
    return (f & 2) ? Q_WILD : (f & 1) ? Q_LIVE : Q_VOID;
}
__device__ __forceinline__ float tau_of_kind(int kind) { return kind == Q_VOID ? INFINITY : __builtin_nanf(""); }

// K2: tau[q] = kk-th largest of sample_scores[q][0..n_sample)  (+inf for void queries;
// n_sample == 0 means "no sample pass": tau = -inf, every row is a candidate)
// With a collection filter (query_coll[q] != -1) the sample rows of other collections count as
// -inf: tau becomes the kk-th best SAMPLED ROW OF THAT COLLECTION, so the scan lets through about
// as many rows of the collection as it would unfiltered rows (sample entry i is row
// (i / unit) * stride * unit + i % unit); fewer than kk such rows in the sample -> tau = -inf.
__global__ __launch_bounds__(256) void kth_select(const float* __restrict__ sample_scores,
                                                  int64_t sample_ld, int n_sample, int kk,
                                                  const float* __restrict__ queries, int n_queries,
                                                  int dim, float* __restrict__ tau,
                                                  float* __restrict__ qerr, int half_image,
                                                  const int32_t* __restrict__ doc_coll,
                                                  const int32_t* __restrict__ query_coll, int unit,
                                                  int64_t stride, int64_t n_docs) {
    __shared__ int hist[CS_BINS];
    __shared__ int aux[8];
    __shared__ int flag;
    __shared__ double red[2][256];
    const int q = blockIdx.x;
    if (qerr) {
        // eq = ||fp16(q) - q|| / ||q||, rounded up: the query-side term of the f16 certificate
        double e = 0.0, nn = 0.0;
        if (q < n_queries)
            for (int i = threadIdx.x; i < dim; i += blockDim.x) {
                const float v = queries[(int64_t)q * dim + i];
                const double dd = (double)v - (double)(float)(_Float16)v;
                e += dd * dd;
                nn += (double)v * (double)v;
            }
        red[0][threadIdx.x] = e;
        red[1][threadIdx.x] = nn;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (threadIdx.x < o) {
                red[0][threadIdx.x] += red[0][threadIdx.x + o];
                red[1][threadIdx.x] += red[1][threadIdx.x + o];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            float rel = red[1][0] > 0.0 ? (float)sqrt(red[0][0] / red[1][0]) : 0.f;
            qerr[q] = __uint_as_float(__float_as_uint(rel) + 1u);
        }
    }
    // (half_image: the call is an f16 scan's -- also the copy scan's on a corpus too small to sample,
    // which asks for no qerr here)
    if (const int kind = query_kind(queries, n_queries, dim, q, half_image != 0, &flag)) {
        if (threadIdx.x == 0) tau[q] = tau_of_kind(kind);
        return;
    }
    if (n_sample < kk) {
        if (threadIdx.x == 0) tau[q] = -INFINITY;
        return;
    }
    const float* s = sample_scores + (int64_t)q * sample_ld;
    const int qc = (query_coll && q < n_queries) ? query_coll[q] : -1;
    auto val = [&](int i) {
        float v = s[i];
        if (qc != -1) {
            const int64_t row = (int64_t)(i / unit) * stride * unit + i % unit;
            if (row >= n_docs || doc_coll[row] != qc) v = -INFINITY;
        }
        return v;
    };
    // Any threshold near the kk-th sample score serves (the certificate only needs "the scan
    // emitted every row >= tau"), and kk is a fraction of a percent of the sample.  Fast path:
    // with M the largest sample score, only the values in [M/2, M] are binned (4096 linear
    // bins: a handful of LDS atomics instead of one per sample, most of which would collide on
    // the two or three exponent bins around zero); when at least kk of them sit there, tau is
    // the lower edge of the bin that holds the kk-th.  Otherwise (M <= 0, or a sample that is
    // not bell-shaped) the two-pass key select below decides.
    __shared__ float kred[4];
    __shared__ int kcnt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    auto sweep = [&](auto&& fn) {   // 8 loads in flight per thread
        for (int base = threadIdx.x; base < n_sample; base += 8 * 256) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = base + u * 256 < n_sample ? val(base + u * 256) : -INFINITY;
#pragma unroll
            for (int u = 0; u < 8; ++u) fn(v[u]);
        }
    };
    float m = -INFINITY;
    sweep([&](float v) { m = fmaxf(m, v); });
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, WAVE));
    if (lane == 0) kred[wave] = m;
    if (threadIdx.x == 0) kcnt = 0;
    for (int i = threadIdx.x; i < CS_BINS; i += 256) hist[i] = 0;
    __syncthreads();
    m = fmaxf(fmaxf(kred[0], kred[1]), fmaxf(kred[2], kred[3]));
    if (m > 0.f && m < INFINITY) {
        const float thr = 0.5f * m, scale = 4095.f / (m - thr);
        int c = 0;
        sweep([&](float v) {
            if (v >= thr) {
                const int bn = (int)((v - thr) * scale);
                atomicAdd(&hist[bn > CS_BINS - 1 ? CS_BINS - 1 : bn], 1);
                ++c;
            }
        });
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, WAVE);
        if (lane == 0 && c) atomicAdd(&kcnt, c);
        __syncthreads();
        if (kcnt >= kk) {   // (block-uniform)
            coarse_find_bin(hist, kk, aux);
            if (threadIdx.x == 0) tau[q] = thr + (float)aux[0] / scale;
            return;
        }
        __syncthreads();
    }
    // a lower bound of the kk-th sample score is as good a threshold as the score itself
    const uint32_t key = block_coarse_select([&](int i) { return fkey(val(i)); }, n_sample, kk, hist, aux);
    if (threadIdx.x == 0) tau[q] = coarse_value(key);
}

// K2 of the register-resident scans: tau[q] = the kk-th largest of the n_vals = nseg * SAMPLE_TOP
// values their sample pass kept of query q (sample[q][segment][0..SAMPLE_TOP), -inf padded; the
// collection filter is already applied), by the exact radix select -- a few hundred values.
// +inf for void queries, as kth_select; -inf when fewer than kk values are finite.
// BOUND: the kept values are a subset of the query's sample scores (a segment holds its lane's
// SAMPLE_TOP best), so the kk-th largest of them is AT MOST the kk-th largest sample score, and
// equal to it unless one lane saw more than SAMPLE_TOP of the sample's kk best.  At most is the safe
// side: a lower tau lets more rows through, and the certificate only needs "the scan emitted every
// row >= tau".
// (The select: 8-bit digits, the keys in registers -- n_vals <= QREG_MAX_SEG * SAMPLE_TOP = 4096 is
// at most KT_REG per thread -- and the bin of a pass found by all 256 threads, one bin each: a scan
// over the waves instead of block_radix_select_local's walk of one thread over the histogram: with
// so few values per block that serial walk, four times per query, would be most of the kernel.)
constexpr int KT_REG = 16;
static_assert(QREG_MAX_SEG * SAMPLE_TOP <= 256 * KT_REG, "kth_select_top holds every kept value in registers");
__global__ __launch_bounds__(256) void kth_select_top(const float* __restrict__ sample, int n_vals, int kk,
                                                      const float* __restrict__ queries, int n_queries,
                                                      int dim, float* __restrict__ tau) {
    __shared__ int hist[256];
    __shared__ int wsum[4];
    __shared__ int bc[2];
    __shared__ int flag;
    const int q = blockIdx.x, t = threadIdx.x, lane = t & 63, wave = t >> 6;
    if (const int kind = query_kind(queries, n_queries, dim, q, true, &flag)) {
        if (t == 0) tau[q] = tau_of_kind(kind);
        return;
    }
    if (n_vals < kk) {
        if (t == 0) tau[q] = -INFINITY;
        return;
    }
    // thread t takes values t, t + 256, .. (the slots past n_vals are not counted)
    uint32_t key[KT_REG];
#pragma unroll
    for (int u = 0; u < KT_REG; ++u) {
        const int i = t + u * 256;
        key[u] = fkey(i < n_vals ? sample[(int64_t)q * n_vals + i] : -INFINITY);
    }
    uint32_t prefix = 0, mask = 0;
    int remaining = kk;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[t] = 0;
        __syncthreads();
#pragma unroll
        for (int u = 0; u < KT_REG; ++u)
            if (t + u * 256 < n_vals && (key[u] & mask) == prefix) atomicAdd(&hist[(key[u] >> shift) & 255], 1);
        __syncthreads();
        // thread t owns bin 255 - t: incl = the keys in its bin and in the larger ones
        const int mine = hist[255 - t];
        int incl = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        for (int x = 0; x < wave; ++x) incl += wsum[x];
        if (incl - mine < remaining && remaining <= incl) {   // (exactly one thread: remaining <= the keys left)
            bc[0] = 255 - t;
            bc[1] = incl - mine;
        }
        __syncthreads();
        remaining -= bc[1];
        prefix |= (uint32_t)bc[0] << shift;
        mask |= 255u << shift;
    }
    if (t == 0) tau[q] = fkey_inv(prefix);
}

// K4: shortlist (select_band), then float64 rescoring, ordering, certificate (rescore_rank,
// dense_rescore.hip).  One block per query in each.  They were one kernel until the counters showed
// its two halves wanting different things: the selection is a chain of dependent memory round trips
// that only occupancy hides, the rescoring is float64-ALU and LDS bound and heavy on registers.
//
//  band    the candidates that can still reach the top-k: with a_k the k-th largest scan score,
//          k rows have true cosine >= a_k/||q|| - eps, so a row whose scan score is below
//          a_k - 2*eps*||q|| cannot beat them.  a_k is replaced by a lower bound from one
//          histogram pass (a slightly wider band, never a narrower one); the first 16
//          candidates per thread stay in registers across the passes.
constexpr int SEL_THREADS = 256;
constexpr int SEL_REG = 16;        // candidates per thread kept in registers (4096 per query; the scan aims at ~1500 to ~2900)
constexpr int SEL_FLAT = 8192;     // candidates of the per-lane segments addressed through a flat LDS index
static size_t band_lds_bytes(int dim) { return sizeof(float) * dim + sizeof(int) * CS_BINS; }
// K4a: the shortlist of one query -- which candidate rows get a float64 score.  Light on
// registers and LDS (four workgroups per CU): its phases are chains of dependent memory round
// trips (segment counts -> candidates -> histogram -> band), which only occupancy hides.
// Writes sel_rows[q][0..ns), sel_meta[q] = {ns, floor (float bits), overflow}.
constexpr int CAPB = SEL_BIG_BAND;   // rows the band may hold
//
// Document shards (thr_dense_shortlist_f16 / thr_dense_floor / thr_dense_finish_f16): TOPM = true is
// the pass BEFORE the exchange -- the query's top_m largest scan scores, each lowered by the scan's
// error bound to a lower bound of ||q|| x (true cosine) of its row, written to top_lb[q][0..top_m)
// (-inf padded) and nothing else.  The k-th largest of the shards' values together, gfloor[q], is
// then a lower bound of ||q|| x (the GLOBAL k-th best cosine): in the pass after the exchange a
// row whose scan score is below gfloor - 1.5 eps ||q|| cannot be one of the global k best and is
// not rescored -- a shard of G rescores about k / G rows instead of k.
template <bool TOPM>
__global__ __launch_bounds__(SEL_THREADS, 4) void select_band(
    int dim, const float* __restrict__ queries, const float* __restrict__ tau,
    const int* __restrict__ cand_cnt, const Cand* __restrict__ cand,
    const int* __restrict__ tile_cnt, int tile_cap, int qtile, int k, int kprime, double eps32,
    double doc_relerr, const float* __restrict__ qerr, int nseg, int seg_cap,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll,
    int32_t* __restrict__ sel_rows, int32_t* __restrict__ sel_meta,
    const float* __restrict__ gfloor, const float* __restrict__ lb_all, int n_shards, int lb_m,
    float* __restrict__ top_lb, int top_m) {
    extern __shared__ float4 lds_sel[];  // [dim/4] query | hist
    __shared__ int aux[8];
    __shared__ int bc[4];
    __shared__ int32_t s_id[CAPB];
    __shared__ int n_sel;
    __shared__ double wsum[4];
    float* lds_qv = reinterpret_cast<float*>(lds_sel);
    int* hist = reinterpret_cast<int*>(lds_sel + dim / 4);

    const int q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // scan error bound relative to ||q||*||d||: fp32 accumulation, plus -- for the f16 matrix
    // core scans -- row and query quantisation: ea*(1+eq) + eq
    const double eq = qerr ? (double)qerr[q] : 0.0;
    const double eps = eps32 + doc_relerr * (1.0 + eq) + eq;
    const Cand* c = cand + (int64_t)q * CAND_CAP;
    // A thread's candidates: cand_at(u), u in [0, my_n).
    //   nseg == 0  one flat list of cand_cnt[q] entries (K3b's output): thread t takes t, t+256, ..
    //   nseg  > 0  dense_scan_f16q's layout: nseg segments of seg_cap slots, segment s filled by
    //              ONE lane of the scan with cand_cnt[q * nseg + s] entries (a count above seg_cap
    //              means entries were dropped).  Up to SEL_FLAT candidates are addressed through
    //              src_off, a flat index of the filled slots: thread t takes items t, t+256, ..
    const Cand* my_ptr = c + threadIdx.x;
    int my_n, my_c[4] = {0, 0, 0, 0};
    bool overflow, flat = true;
    int n;
    __shared__ unsigned short src_off[SEL_FLAT];
    if (nseg == 0) {
        const int cnt = cand_cnt[q];
        overflow = cnt > CAND_CAP || tile_cnt[q / qtile] > tile_cap;
        // Only slots [0, min(cnt, CAND_CAP)) were written.  (Round 1 read all CAND_CAP slots
        // whenever the TILE list had overflowed, even for a query of that tile with few
        // candidates of its own: stale workspace words became row indices -> out-of-bounds
        // gathers, the rc 134 abort of gpurun_out/t1.log.  An overflowed query is never
        // certified; thr_dense_rescue redoes it.)
        n = cnt < CAND_CAP ? cnt : CAND_CAP;
        my_n = n > (int)threadIdx.x ? (n - (int)threadIdx.x + SEL_THREADS - 1) / SEL_THREADS : 0;
    } else {
        // thread t owns segments t, t + 256, t + 512, t + 768 (host keeps nseg <= 4 * SEL_THREADS);
        // the flat order is thread-major: an exclusive scan of the per-thread totals places them
        __shared__ int wtot[4];
        bool over = false;
        int tot = 0;
#pragma unroll
        for (int x = 0; x < 4; ++x) {
            const int sg = (int)threadIdx.x + x * SEL_THREADS;
            int sc = sg < nseg ? cand_cnt[(int64_t)q * nseg + sg] : 0;
            over |= sc > seg_cap;
            my_c[x] = sc < seg_cap ? sc : seg_cap;
            tot += my_c[x];
        }
        int incl = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += v;
        }
        if (lane == 63) wtot[wave] = incl;
        overflow = __syncthreads_or(over) != 0;
        int base = incl - tot;
        for (int x = 0; x < wave; ++x) base += wtot[x];
        n = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        flat = n <= SEL_FLAT;
        if (flat) {
            // src_off[i] = slot of flat candidate i: the reads below are then coalesced (lane l
            // of a wave takes flat item l + 64 * ..., i.e. neighbouring slots of a segment)
            // instead of one segment per lane, which cost a cache line per lane and load
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const int first = ((int)threadIdx.x + x * SEL_THREADS) * seg_cap;
                for (int j = 0; j < my_c[x]; ++j) src_off[base + j] = (unsigned short)(first + j);
                base += my_c[x];
            }
            __syncthreads();
            my_n = n > (int)threadIdx.x ? (n - (int)threadIdx.x + SEL_THREADS - 1) / SEL_THREADS : 0;
        } else {
            my_n = tot;   // (rare: a threshold far too low) each thread walks its own segments
        }
    }
    auto cand_at = [&](int u) -> Cand {
        if (nseg == 0) return my_ptr[(int64_t)u * SEL_THREADS];
        if (flat) return c[src_off[(int)threadIdx.x + u * SEL_THREADS]];
        int sg = threadIdx.x;
#pragma unroll
        for (int x = 0; x < 3; ++x)
            if (u >= my_c[x]) {
                u -= my_c[x];
                sg += SEL_THREADS;
            } else {
                break;
            }
        return c[(int64_t)sg * seg_cap + u];
    };

    // Collection filter (rag2_schema.sql:404-408): a candidate of another collection is read as
    // score -inf and skipped everywhere below (a row that passed the scan never scores -inf
    // itself).  The floor of the certificate still bounds every row of the RIGHT collection
    // outside the shortlist.
    const int qc = query_coll ? query_coll[q] : -1;
    auto load_cand = [&](int u) -> Cand {
        Cand e = cand_at(u);
        if (qc != -1 && doc_coll[e.doc] != qc) e.score = -INFINITY;
        return e;
    };
    // candidates this thread keeps in registers (loads in flight while the query is staged)
    Cand mine[SEL_REG];
#pragma unroll
    for (int u = 0; u < SEL_REG; ++u) mine[u] = u < my_n ? load_cand(u) : Cand{-INFINITY, 0u};
    if (qc != -1) {   // n = the candidates that pass the filter
        __shared__ int n_pass;
        if (threadIdx.x == 0) n_pass = 0;
        __syncthreads();
        int mine_ok = 0;
#pragma unroll
        for (int u = 0; u < SEL_REG; ++u) mine_ok += (u < my_n && mine[u].score > -INFINITY) ? 1 : 0;
        for (int u = SEL_REG; u < my_n; ++u) mine_ok += load_cand(u).score > -INFINITY ? 1 : 0;
        if (mine_ok) atomicAdd(&n_pass, mine_ok);
        __syncthreads();
        n = n_pass;
    }
    for (int i = threadIdx.x; i < dim / 4; i += SEL_THREADS)
        lds_sel[i] = reinterpret_cast<const float4*>(queries + (int64_t)q * dim)[i];
    if (threadIdx.x == 0) n_sel = 0;
    __syncthreads();

    // ||q|| upper bound (parallel float64 sum, inflated) -- only used to size the band
    {
        double part = 0.0;
        for (int i = threadIdx.x; i < dim; i += SEL_THREADS) part += (double)lds_qv[i] * (double)lds_qv[i];
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o, WAVE);
        if (lane == 0) wsum[wave] = part;
        __syncthreads();
    }
    const double qn_hi = sqrt(wsum[0] + wsum[1] + wsum[2] + wsum[3]) * (1.0 + 1e-6);

    // the shards' common floor: rows below it cannot be among the k best of all the shards.  Given
    // as gfloor[q], or as the shards' gathered lower bounds lb_all [n_shards, nq, lb_m]: the k-th
    // largest of this query's n_shards * lb_m values, found here by rank counting (<= 4096 values
    // in the LDS words of the histogram, which is not in use yet).
    float gF = -INFINITY;
    if (!TOPM) {
        if (gfloor) {
            gF = gfloor[q];
        } else if (lb_all && n_shards * lb_m >= k) {
            __shared__ float s_gF;
            float* fv = reinterpret_cast<float*>(hist);
            const int nv = n_shards * lb_m, nv4 = (nv + 3) & ~3;   // (-inf padding never counts)
            for (int i = threadIdx.x; i < nv4; i += SEL_THREADS)
                fv[i] = i < nv ? lb_all[((int64_t)(i / lb_m) * gridDim.x + q) * lb_m + i % lb_m] : -INFINITY;
            if (threadIdx.x == 0) s_gF = -INFINITY;
            __syncthreads();
            const f32x4* fv4 = reinterpret_cast<const f32x4*>(fv);
            for (int i = threadIdx.x; i < nv; i += SEL_THREADS) {
                const float v = fv[i];
                if (!(v > -INFINITY)) continue;
                int rank = 0;   // values ahead of v: larger ones, equal ones of a lower index
#pragma unroll 4
                for (int j = 0; j < nv4; j += 4) {   // (the same addresses in every lane: broadcast reads)
                    const f32x4 w = fv4[j >> 2];
                    rank += (w.x > v || (w.x == v && j < i)) ? 1 : 0;
                    rank += (w.y > v || (w.y == v && j + 1 < i)) ? 1 : 0;
                    rank += (w.z > v || (w.z == v && j + 2 < i)) ? 1 : 0;
                    rank += (w.w > v || (w.w == v && j + 3 < i)) ? 1 : 0;
                }
                if (rank == k - 1) s_gF = v;
            }
            __syncthreads();
            gF = s_gF;
            __syncthreads();   // (hist is zeroed below)
        }
    }
    float band_lo = -INFINITY;
    if (gF > -INFINITY) band_lo = nextafterf((float)((double)gF - 1.5 * eps * qn_hi), -INFINITY);
    float floor32 = tau[q];
    bool band_done = false;
    const int kk = TOPM ? top_m : k;   // the rank the histogram pass looks for
    float a_kk = -INFINITY;            // TOPM: a lower bound of the top_m-th largest scan score
    if (n > kk) {
        // a_k, a lower bound of the k-th largest scan score: ONE histogram pass over 4096 LINEAR
        // bins between the smallest and the largest live candidate (the scores all sit just above
        // tau: binned by float exponent, as the sample select does, they fall into two or three
        // bins and the LDS atomics of a wave serialise on one address), then the smallest score
        // of the bins that hold the k largest.  bin_of is monotone in the score (IEEE subtract,
        // multiply by a positive constant, truncate), so those bins hold every score >= a_k.
        __shared__ float fred[3][4];
        float lo = INFINITY, hi = -INFINITY;
#pragma unroll
        for (int u = 0; u < SEL_REG; ++u)
            if (u < my_n && mine[u].score > -INFINITY) {
                lo = fminf(lo, mine[u].score);
                hi = fmaxf(hi, mine[u].score);
            }
        for (int u = SEL_REG; u < my_n; ++u) {
            const float sc = load_cand(u).score;
            if (sc > -INFINITY) {
                lo = fminf(lo, sc);
                hi = fmaxf(hi, sc);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            lo = fminf(lo, __shfl_xor(lo, o, WAVE));
            hi = fmaxf(hi, __shfl_xor(hi, o, WAVE));
        }
        if (lane == 0) fred[0][wave] = lo, fred[1][wave] = hi;
        for (int i = threadIdx.x; i < CS_BINS; i += SEL_THREADS) hist[i] = 0;
        __syncthreads();
        lo = fminf(fminf(fred[0][0], fred[0][1]), fminf(fred[0][2], fred[0][3]));
        hi = fmaxf(fmaxf(fred[1][0], fred[1][1]), fmaxf(fred[1][2], fred[1][3]));
        const float scale = hi - lo > 1e-30f ? 4095.f / (hi - lo) : 0.f;
        auto bin_of = [&](float sc) {
            const int bn = (int)((sc - lo) * scale);
            return bn > CS_BINS - 1 ? CS_BINS - 1 : bn;
        };
#pragma unroll
        for (int u = 0; u < SEL_REG; ++u)
            if (u < my_n && mine[u].score > -INFINITY) atomicAdd(&hist[bin_of(mine[u].score)], 1);
        for (int u = SEL_REG; u < my_n; ++u) {
            const float sc = load_cand(u).score;
            if (sc > -INFINITY) atomicAdd(&hist[bin_of(sc)], 1);
        }
        __syncthreads();
        coarse_find_bin(hist, kk, aux);
        const int kbin = aux[0];
        float a_k = INFINITY;
#pragma unroll
        for (int u = 0; u < SEL_REG; ++u)
            if (u < my_n && mine[u].score > -INFINITY && bin_of(mine[u].score) >= kbin)
                a_k = fminf(a_k, mine[u].score);
        for (int u = SEL_REG; u < my_n; ++u) {
            const float sc = load_cand(u).score;
            if (sc > -INFINITY && bin_of(sc) >= kbin) a_k = fminf(a_k, sc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) a_k = fminf(a_k, __shfl_xor(a_k, o, WAVE));
        if (lane == 0) fred[2][wave] = a_k;
        __syncthreads();
        a_k = fminf(fminf(fred[2][0], fred[2][1]), fminf(fred[2][2], fred[2][3]));
        a_kk = a_k;
        const float band = (float)((double)a_k - 2.5 * eps * qn_hi);
        // (the float conversion may have rounded up); either bound rules a row out: the higher one
        band_lo = fmaxf(band_lo, nextafterf(band, -INFINITY));
    }
    if (TOPM) {
        // the top_m largest scan scores, each as a lower bound of ||q|| x cosine of its row (the
        // float conversion may round up: one step down).  The scores >= a_kk are the top_m and the
        // few more that share the last histogram bin: collected in LDS, ranked by counting.
        float* o = top_lb + (int64_t)q * top_m;
        float* vals = reinterpret_cast<float*>(s_id);   // CAPB values
        const double drop = eps * qn_hi;
        auto lowered = [&](float sc) { return nextafterf((float)((double)sc - drop), -INFINITY); };
        for (int i = threadIdx.x; i < top_m; i += SEL_THREADS) o[i] = -INFINITY;
        for (int u = 0; u < my_n; ++u) {
            const float sc = load_cand(u).score;
            if (sc > -INFINITY && sc >= a_kk) {
                const int p = atomicAdd(&n_sel, 1);
                if (p < CAPB) vals[p] = sc;
            }
        }
        __syncthreads();
        const int c = n_sel;
        if (c <= CAPB) {
            for (int i = threadIdx.x; i < c; i += SEL_THREADS) {
                const float v = vals[i];
                int rank = 0;
                for (int j = 0; j < c; ++j) {
                    const float w = vals[j];
                    rank += (w > v || (w == v && j < i)) ? 1 : 0;
                }
                if (rank < top_m) o[rank] = lowered(v);
            }
            return;
        }
        // (a tie wider than the LDS list at the top: the exact select, four passes)
        __syncthreads();
        if (threadIdx.x == 0) n_sel = 0;
        __syncthreads();
        const uint32_t tkey = block_radix_select_local(
            [&](int u) { return fkey(load_cand(u).score); }, my_n, top_m, hist, bc);
        for (int u = 0; u < my_n; ++u) {
            const Cand e = load_cand(u);
            if (fkey(e.score) > tkey) o[atomicAdd(&n_sel, 1)] = lowered(e.score);
        }
        __syncthreads();
        for (int u = 0; u < my_n; ++u) {
            const Cand e = load_cand(u);
            if (fkey(e.score) == tkey) {
                const int p = atomicAdd(&n_sel, 1);
                if (p < top_m) o[p] = lowered(e.score);
            }
        }
        return;
    }
    if (band_lo > -INFINITY) {
        // count and collect in one sweep; past CAPB rows only the count matters
#pragma unroll
        for (int u = 0; u < SEL_REG; ++u) {   // (one LDS atomic per wave and register slot)
            const bool in = u < my_n && mine[u].score >= band_lo;
            const unsigned long long m = __ballot(in);
            if (m) {
                int base = 0;
                if (lane == 0) base = atomicAdd(&n_sel, __popcll(m));
                base = __shfl(base, 0, WAVE);
                const int p = base + __popcll(m & ((1ull << lane) - 1ull));
                if (in && p < CAPB) s_id[p] = mine[u].doc;
            }
        }
        for (int u = SEL_REG; u < my_n; ++u) {
            const Cand e = load_cand(u);
            if (e.score >= band_lo) {   // (band_lo > -inf: filtered candidates never pass)
                const int p = atomicAdd(&n_sel, 1);
                if (p < CAPB) s_id[p] = e.doc;
            }
        }
        __syncthreads();
        if (n_sel <= CAPB) {
            // rows outside the band: uncollected ones are below tau, collected ones below band_lo
            floor32 = fmaxf(floor32, band_lo);
            band_done = true;
        } else {
            __syncthreads();
            if (threadIdx.x == 0) n_sel = 0;
            __syncthreads();
        }
    }
    if (!band_done) {
        // the band does not fit the block (or the list is short): the kprime best, exactly
        if (n > kprime) {
            // (n > kprime candidates pass the filter, so the kprime-th largest key is a real score)
            const uint32_t tkey = block_radix_select_local(
                [&](int u) { return fkey(load_cand(u).score); }, my_n, kprime, hist, bc);
            floor32 = fkey_inv(tkey);
            for (int u = 0; u < my_n; ++u) {
                const Cand e = load_cand(u);
                if (fkey(e.score) > tkey) {
                    const int p = atomicAdd(&n_sel, 1);
                    s_id[p] = e.doc;
                }
            }
            __syncthreads();
            for (int u = 0; u < my_n; ++u) {
                const Cand e = load_cand(u);
                if (fkey(e.score) == tkey) {
                    const int p = atomicAdd(&n_sel, 1);
                    if (p < kprime) s_id[p] = e.doc;
                }
            }
            __syncthreads();
            if (threadIdx.x == 0 && n_sel > kprime) n_sel = kprime;
        } else {
            for (int u = 0; u < my_n; ++u) {
                const Cand e = load_cand(u);
                if (e.score > -INFINITY) {
                    const int p = atomicAdd(&n_sel, 1);
                    s_id[p] = e.doc;
                }
            }
        }
    }
    __syncthreads();
    const int ns = n_sel;
    for (int i = threadIdx.x; i < ns; i += SEL_THREADS) sel_rows[(int64_t)q * CAPB + i] = s_id[i];
    if (threadIdx.x == 0) {
        sel_meta[4 * q + 0] = ns;
        sel_meta[4 * q + 1] = (int32_t)__float_as_uint(floor32);
        sel_meta[4 * q + 2] = overflow ? 1 : 0;
        sel_meta[4 * q + 3] = (int32_t)__float_as_uint(gF);
    }
}

// The shards' common floor: the k-th largest of the n_shards * m lower bounds of a query
// (select_band<true> of every shard, gathered shard-major), -inf when fewer than k are finite.
// One workgroup per query; rank counting in LDS (n_shards * m is a few hundred values).
__global__ __launch_bounds__(256) void dense_floor_kernel(const float* __restrict__ lb, int n_shards,
                                                          int n_queries, int m, int k,
                                                          float* __restrict__ gfloor) {
    extern __shared__ float fl_v[];
    const int q = blockIdx.x, n = n_shards * m;
    for (int i = threadIdx.x; i < n; i += blockDim.x)
        fl_v[i] = lb[((int64_t)(i / m) * n_queries + q) * m + i % m];
    if (threadIdx.x == 0) gfloor[q] = -INFINITY;
    __syncthreads();
    if (n < k) return;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float v = fl_v[i];
        if (!(v > -INFINITY)) continue;
        int rank = 0;   // values ahead of v: larger ones, equal ones of a lower index
        for (int j = 0; j < n; ++j) {
            const float w = fl_v[j];
            rank += (w > v || (w == v && j < i)) ? 1 : 0;
        }
        if (rank == k - 1) gfloor[q] = v;
    }
}

// ---- launches (dense.hip's pipeline) ----
// K2.  Without a sample pass (a corpus the candidate lists hold anyway: sample_docs == 0) tau = -inf.
// sample_nseg > 0: the sample area holds the kept values of the register-resident sample pass.
// (the register-resident scan's query image comes with the query-side error term; kth_select then skips it)
int launch_threshold(const DensePlan& P, const DenseIndex& X, const DenseBatch& B, int sample_nseg) {
    if (P.sampled && sample_nseg > 0) {
        hipLaunchKernelGGL(kth_select_top, dim3(P.qpad), dim3(256), 0, B.st, (const float*)P.sample,
                           sample_nseg * SAMPLE_TOP, P.ksample, B.queries, B.n_queries, X.dim, P.tau);
        return launch_status();
    }
    hipLaunchKernelGGL(kth_select, dim3(P.qpad), dim3(256), 0, B.st,
                       P.sampled ? (const float*)P.sample : nullptr, P.sample_docs, (int)P.sample_docs,
                       P.ksample, B.queries, B.n_queries, X.dim, P.tau, P.packed ? nullptr : P.qerr,
                       P.kind == KIND_F16 ? 1 : 0, X.doc_coll, B.query_coll, MF_ROWS,
                       P.sampled ? P.sample_stride : (int64_t)1, X.n_docs);
    return launch_status();
}

int launch_bucket(const DensePlan& P, hipStream_t st) {
    hipLaunchKernelGGL(bucket_candidates, dim3(BUCKET_BLOCKS, P.ntiles), dim3(256), 0, st, P.tcnt,
                       P.tlist, P.tile_cap, P.qtile, P.row_bits, P.cnt, P.cand);
    return launch_status();
}

// K4a.  PIPE_SHORTLIST: the top_m lower bounds alone; else the shortlist, under the shards' floor if
// one is given (top_m is then the row length of lb_all).
int launch_band(const DensePlan& P, const DenseIndex& X, const DenseBatch& B, const DensePhase& S,
                int nseg) {
    const bool topm = S.phase == PIPE_SHORTLIST;
    hipLaunchKernelGGL(topm ? select_band<true> : select_band<false>, dim3(B.n_queries),
                       dim3(SEL_THREADS), band_lds_bytes(X.dim), B.st, X.dim, B.queries, P.tau, P.cnt,
                       P.cand, P.tcnt, P.tile_cap, P.qtile, B.k, B.kprime, scan_eps(X.dim),
                       X.doc_rel_err, P.qerr, nseg, nseg ? CAND_CAP / nseg : 0, X.doc_coll,
                       B.query_coll, P.sel_rows, P.sel_meta, S.gfloor, S.lb_all, S.n_shards,
                       topm ? 0 : S.top_m, S.top_lb, topm ? S.top_m : 0);
    return launch_status();
}

}  // namespace thr

using namespace thr;

extern "C" int thr_dense_floor(const float* top_lb, int n_shards, int n_queries, int m, int k,
                               float* gfloor, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!top_lb || !gfloor || n_shards <= 0 || n_queries <= 0 || m <= 0 || k <= 0, THR_ERR_INVALID);
    THR_RETURN_IF((int64_t)n_shards * m > 8192, THR_ERR_CAPACITY);
    hipLaunchKernelGGL(dense_floor_kernel, dim3(n_queries), dim3(256), sizeof(float) * n_shards * m,
                       (hipStream_t)stream, top_lb, n_shards, n_queries, m, k, gfloor);
    return launch_status();
}
