// The float16 images the f16 scans read, and their rounding errors (the terms of the f16
// certificate, dense_scan_f16.hpp): pack_queries_f16 writes the fragment-major query image of the
// register-resident scans (dense_scan_f16q.hpp), quantize_f16_norm the fragment-major copy of the
// normalised rows, measure_f16_error the row term of the scans that round float32 rows in flight.
#pragma once
#include "dense_common.hpp"

namespace thr {

// queries float32 [n, DIM] -> fragment-major float16 image [qpad/32][KS][64 lanes][8 halves]
// (lane (c, h) of k-step s holds dims 16 s + 8 h .. + 8 of query 32 tile + c: the B operand of
// v_mfma_f32_32x32x16_f16), zeros for padding queries, plus
// qerr[q] = ||fp16(q) - q|| / ||q|| rounded up (the query-side term of the f16 certificate).
// One wave per 32 queries.
template <int DIM, int SHAPE>
__global__ __launch_bounds__(256) void pack_queries_f16(const float* __restrict__ queries,
                                                        int n_queries, f32x4* __restrict__ qfrag,
                                                        float* __restrict__ qerr) {
    constexpr int KS = DIM / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    __shared__ double red[4][4][32];   // [wave][e, n of query half 0 | e, n of half 1][c]
    double e = 0.0, nn = 0.0, e_hi = 0.0, n_hi = 0.0;
    // SHAPE 32: lane (c, h) of fragment s holds dims 16 s + 8 h .. + 8 of query 32 tile + c.
    // SHAPE 16: fragment qb * KS/2 + k32, lane (c, g) holds dims 32 k32 + 8 g .. + 8 of query
    //           32 tile + 16 qb + c (the B operand of v_mfma_f32_16x16x32_f16).
    // The 4 waves of the block take every fourth fragment.
#pragma unroll 4
    for (int s = wave; s < KS; s += 4) {
        int q, d0;
        if constexpr (SHAPE == 32) {
            q = blockIdx.x * 32 + (lane & 31);
            d0 = 16 * s + 8 * (lane >> 5);
        } else {
            q = blockIdx.x * 32 + 16 * (s / (KS / 2)) + (lane & 15);
            d0 = 32 * (s % (KS / 2)) + 8 * (lane >> 4);
        }
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
        if (q < n_queries) {
            const f32x4* src = reinterpret_cast<const f32x4*>(queries + (int64_t)q * DIM + d0);
            lo = src[0];
            hi = src[1];
        }
        const f32x4 packed = pack_f16x8(lo, hi);
        qfrag[((int64_t)blockIdx.x * KS + s) * 64 + lane] = packed;
        const half8 hv = __builtin_bit_cast(half8, packed);
        double e1 = 0.0, n1 = 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float v = j < 4 ? lo[j] : hi[j - 4];
            const double d = (double)v - (double)(float)hv[j];
            e1 += d * d;
            n1 += (double)v * (double)v;
        }
        if (SHAPE == 32 || s < KS / 2) {
            e += e1;
            nn += n1;
        } else {   // SHAPE 16, second query half (16 + c)
            e_hi += e1;
            n_hi += n1;
        }
    }
    // eq = ||fp16(q) - q|| / ||q||, rounded up: lanes of one query first, then the 4 waves
    if constexpr (SHAPE == 32) {
        e += __shfl_xor(e, 32, WAVE);
        nn += __shfl_xor(nn, 32, WAVE);
        if (lane < 32) {
            red[wave][0][lane] = e;
            red[wave][1][lane] = nn;
        }
    } else {
#pragma unroll
        for (int m = 16; m <= 32; m <<= 1) {
            e += __shfl_xor(e, m, WAVE);
            nn += __shfl_xor(nn, m, WAVE);
            e_hi += __shfl_xor(e_hi, m, WAVE);
            n_hi += __shfl_xor(n_hi, m, WAVE);
        }
        if (lane < 16) {
            red[wave][0][lane] = e;
            red[wave][1][lane] = nn;
            red[wave][0][16 + lane] = e_hi;
            red[wave][1][16 + lane] = n_hi;
        }
    }
    __syncthreads();
    if (threadIdx.x < 32) {
        double es = 0.0, ns = 0.0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            es += red[w][0][threadIdx.x];
            ns += red[w][1][threadIdx.x];
        }
        const float rel = ns > 0.0 ? (float)sqrt(es / ns) : 0.f;
        qerr[blockIdx.x * 32 + threadIdx.x] = __uint_as_float(__float_as_uint(rel) + 1u);
    }
}

// float32 corpus -> fragment-major float16 copy of the NORMALISED rows (d * (1/||d||), round to
// nearest even); rows with ||d|| = 0 and the padding rows of the last tile are NaN.  Also
// max over rows of ||d16 - d/||d|| || (float64, against the exactly normalised row), rounded up,
// via atomicMax on the float bits.  packed == nullptr: measure only.  One wave per row (rows of
// the padded tail included).
__global__ __launch_bounds__(256) void quantize_f16_norm(const float* __restrict__ docs,
                                                         int64_t n_docs, int dim, int shape,
                                                         _Float16* __restrict__ packed,
                                                         unsigned int* __restrict__ max_err_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    const int64_t n_pad = (n_docs + 31) / 32 * 32;
    if (row >= n_pad) return;
    const int64_t tile = row >> 5;
    const int r = (int)(row & 31), ks = dim / 16;
    const float* x = docs + row * dim;
    double nn = 0.0;
    if (row < n_docs)
        for (int i = lane; i < dim; i += WAVE) nn += (double)x[i] * (double)x[i];
    for (int m = 32; m >= 1; m >>= 1) nn += __shfl_xor(nn, m, WAVE);
    const double dn = sqrt(nn);
    const bool live = dn > 0.0;  // same rows thr_doc_norms gives inv_norm = 0 ("no embedding")
    double err = 0.0;
    for (int i = lane; i < dim; i += WAVE) {
        const float v = live ? x[i] : 0.f;
        const _Float16 hv = live ? (_Float16)(float)((double)v / dn) : (_Float16)__builtin_nanf("");
        if (packed) {
            if (shape == 32) {   // piece s = 32 rows x dims [16 s, +16): lane r + 32 hh, hh = dim half
                const int s = i >> 4, hh = (i >> 3) & 1, e = i & 7;
                packed[(((tile * ks + s) * 64) + r + 32 * hh) * 8 + e] = hv;
            } else {             // piece 2 k32 + ra = rows [16 ra, +16) x dims [32 k32, +32): lane (r & 15) + 16 g
                const int k32 = i >> 5, g = (i >> 3) & 3, e = i & 7, ra = r >> 4;
                packed[(((tile * ks + 2 * k32 + ra) * 64) + (r & 15) + 16 * g) * 8 + e] = hv;
            }
        }
        if (live) {
            const double d = (double)v / dn - (double)(float)hv;
            err += d * d;
        }
    }
    for (int m = 32; m >= 1; m >>= 1) err += __shfl_xor(err, m, WAVE);
    if (lane == 0 && live) {
        float rel = (float)sqrt(err);
        rel = __uint_as_float(__float_as_uint(rel) + 1u);
        atomicMax(max_err_bits, __float_as_uint(rel));
    }
}

// The in-flight-rounding scan (dense_scan_f16) rounds the float32 rows AS THEY ARE: its row error
// term is max_d ||fp16(d) - d|| / ||d|| (+inf when a value leaves the float16 range), rounded up,
// accumulated as ordered float bits with atomicMax.  One wave per row.
__global__ __launch_bounds__(256) void measure_f16_error(const float* __restrict__ docs, int64_t n_docs,
                                                         int dim, unsigned int* __restrict__ max_rel_bits) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (row >= n_docs) return;
    const float* x = docs + row * dim;
    double err = 0.0, nrm = 0.0;
    for (int i = lane; i < dim; i += WAVE) {
        const float v = x[i];
        const double d = (double)v - (double)(float)(_Float16)v;
        err += d * d;
        nrm += (double)v * (double)v;
    }
    for (int m = 32; m >= 1; m >>= 1) {
        err += __shfl_xor(err, m, WAVE);
        nrm += __shfl_xor(nrm, m, WAVE);
    }
    if (lane == 0 && nrm > 0.0) {
        float rel = (float)sqrt(err / nrm);
        rel = __uint_as_float(__float_as_uint(rel) + 1u);
        atomicMax(max_rel_bits, __float_as_uint(rel));  // positive floats order like their bits
    }
}

}  // namespace thr
