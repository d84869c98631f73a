// Late-interaction rerank over an FP8 (OCP E4M3FN) document-token store with one float32 scale per
// token: half the bytes per candidate of csrc/maxsim.hip's float16 store (include/thr_hip_rerank.h holds
// the contract: format, image, quantiser rule, error model).
//
// The scorer is maxsim.hip's kernel with another A operand.  One wave per (query, candidate); the product
// is formed TRANSPOSED, S^T = D * Q^T, with v_mfma_f32_32x32x16_f16: A = 32 doc tokens x 16 dims, B = 16
// dims x 32 query tokens (float16, straight from memory, as there).  A lane's 16-byte load of the image
//     [doc][tile of 32 tokens][k-pair][lane][16 bytes]
// holds the A fragments of TWO k-steps: bytes 0..7 are dims 32 kp + 8 h .. + 8 of token 32 tile + r
// (lane = 32 h + r), bytes 8..15 dims 32 kp + 16 + 8 h .. + 8.  Four v_cvt_scalef32_pk_f16_fp8 (scale 1.0:
// every E4M3 value is a float16, so the conversion is exact) make each half8.  The accumulator of the
// 32x32 MFMA has the query token on the lane (col = lane & 31) and doc token
//     row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
// in register reg, so the 16 scales a lane needs for a tile are four float4 loads at tile + 8 g + 4 h
// (g = reg >> 2); they are multiplied in float32 into the accumulator (one rounding, none for a power of
// two) before the per-lane max over doc tokens.  The rest -- the lane-pair exchange, the sum over query
// tokens -- is maxsim.hip's.
//
// Bytes in flight: a 32-token tile is tok_dim * 32 bytes of codes (4 KiB at 128 dims, half the float16
// tile) + 128 bytes of scales, so a wave issues the loads of TWO tiles before the first MFMA of the pair;
// an odd tile count ends with a single tile.
// Algorithmic bytes per (q, c): d_tokens * (tok_dim + 4); flops 2 * q_tokens * d_tokens * tok_dim.
#include "thr_common.hpp"

#include "../../include/thr_hip_rerank.h"

namespace thr {

typedef _Float16 f8_half2 __attribute__((ext_vector_type(2)));
typedef _Float16 f8_half8 __attribute__((ext_vector_type(8)));
typedef float f8_f32x4 __attribute__((ext_vector_type(4)));
typedef float f8_f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t f8_u32x2 __attribute__((ext_vector_type(2)));
typedef uint32_t f8_u32x4 __attribute__((ext_vector_type(4)));

constexpr int M8_THREADS = 256;
constexpr int M8_WAVES = M8_THREADS / WAVE;

// ---------------------------------------------------------------------------------------- quantiser
// RNE of an exact float32 a, |a| <= 448, onto the E4M3FN grid, on the bits: normals keep three mantissa
// bits (the carry of the rounding runs into the exponent field, which is what the next binade is);
// below 2^-6 the grid is the multiples of 2^-9, and 8 of them is the smallest normal's code.
__host__ __device__ __forceinline__ uint32_t e4m3_code(float y) {
    const uint32_t b = __builtin_bit_cast(uint32_t, y);
    const uint32_t sign = (b >> 24) & 0x80u;
    const uint32_t a = b & 0x7fffffffu;
    uint32_t code;
    if (a >= (121u << 23)) {    // |y| >= 2^-6
        code = ((a + 0x7ffffu + ((a >> 20) & 1u)) >> 20) - (120u << 3);
    } else {
        code = (uint32_t)__builtin_rintf(__builtin_bit_cast(float, a) * 512.0f);    // ties to even
    }
    return sign | code;
}

// e = floor(log2(448 / amax)): the largest e with amax * 2^e <= 448 = 1.75 * 2^8; 0 for amax == 0.
// amax is a float16 value, so a normal float32: -8 <= e <= 32.
__host__ __device__ __forceinline__ int fp8_exponent(float amax) {
    if (!(amax > 0.f)) return 0;
    const uint32_t ab = __builtin_bit_cast(uint32_t, amax);
    return 8 - ((int)(ab >> 23) - 127) - ((ab & 0x7fffffu) > 0x600000u ? 1 : 0);
}

// One HALF-WAVE per token, lane g of it over dims 8 g .. 8 g + 8: amax over the half-wave, the exponent
// from amax's bits, eight codes, one 8-byte store in the packed place.  GROUPS = tok_dim / 8 <= 32.
__global__ __launch_bounds__(M8_THREADS) void maxsim_quantize_fp8_kernel(
    const _Float16* __restrict__ dtok, int64_t n_tokens, int d_tokens, int groups,
    uint8_t* __restrict__ codes, float* __restrict__ scales) {
    const int g = threadIdx.x & 31;
    const int64_t T = (int64_t)blockIdx.x * (M8_THREADS / 32) + (threadIdx.x >> 5);
    const bool live = T < n_tokens && g < groups;
    const int td = groups * 8;
    f8_half8 x;
#pragma unroll
    for (int j = 0; j < 8; ++j) x[j] = (_Float16)0.0f;
    if (live) x = *reinterpret_cast<const f8_half8*>(dtok + T * td + 8 * g);
    float amax = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) amax = fmaxf(amax, fabsf((float)x[j]));
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m, WAVE));   // stays in the half-wave
    const int e = fp8_exponent(amax);
    if (!live) return;
    const float up = __uint_as_float((uint32_t)(127 + e) << 23);    // 2^e, e in -8 .. 32
    uint32_t w[2] = {0u, 0u};
#pragma unroll
    for (int j = 0; j < 8; ++j) w[j >> 2] |= e4m3_code((float)x[j] * up) << (8 * (j & 3));
    const int64_t doc = T / d_tokens;
    const int tok = (int)(T % d_tokens);
    const int tile = tok >> 5, r = tok & 31;
    const int kp = g >> 2, h = g & 1, half = (g >> 1) & 1;
    const int kpairs = groups / 4;
    const int64_t at = doc * (int64_t)d_tokens * td +
                       ((int64_t)(tile * kpairs + kp) * 64 + 32 * h + r) * 16 + 8 * half;
    f8_u32x2 out;
    out[0] = w[0];
    out[1] = w[1];
    *reinterpret_cast<f8_u32x2*>(codes + at) = out;
    if (g == 0) scales[T] = __uint_as_float((uint32_t)(127 - e) << 23);
}

// ------------------------------------------------------------------------------------------- scorer
template <int KPAIRS>
struct Tile8 {
    f8_u32x4 c[KPAIRS];
    f8_f32x4 s[4];
};

template <int KPAIRS>
__device__ __forceinline__ void tile8_load(Tile8<KPAIRS>& t, const f8_u32x4* __restrict__ codes,
                                           const float* __restrict__ scales, int tile, int lane) {
    const f8_u32x4* p = codes + (int64_t)tile * KPAIRS * 64 + lane;
#pragma unroll
    for (int kp = 0; kp < KPAIRS; ++kp) t.c[kp] = __builtin_nontemporal_load(p + kp * 64);
    const float* sc = scales + tile * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) t.s[g] = *reinterpret_cast<const f8_f32x4*>(sc + 8 * g);
}

// eight codes (two words) -> the float16 A fragment of one k-step; byte 0 of a word is the lower dim
__device__ __forceinline__ f8_half8 dequant8(uint32_t w0, uint32_t w1) {
    const f8_half2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false);
    const f8_half2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
    const f8_half2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false);
    const f8_half2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
    f8_half8 o;
    o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1];
    o[4] = c[0]; o[5] = c[1]; o[6] = d[0]; o[7] = d[1];
    return o;
}

template <int KPAIRS>
__device__ __forceinline__ float tile8_max(const Tile8<KPAIRS>& t, const f8_half8 (&bq)[2 * KPAIRS], float mx) {
    f8_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int kp = 0; kp < KPAIRS; ++kp) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dequant8(t.c[kp][0], t.c[kp][1]), bq[2 * kp], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(dequant8(t.c[kp][2], t.c[kp][3]), bq[2 * kp + 1], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, acc[i] * t.s[i >> 2][i & 3]);
    return mx;
}

template <int KPAIRS>
__global__ __launch_bounds__(M8_THREADS) void maxsim_fp8_kernel(
    const _Float16* __restrict__ qtok, int q_tokens, const uint8_t* __restrict__ codes,
    const float* __restrict__ scales, int64_t n_docs, int d_tokens, const int32_t* __restrict__ cand,
    const int64_t* __restrict__ cand_ids, int64_t id_base, int n_cand, float* __restrict__ out) {
    constexpr int TD = KPAIRS * 32;
    constexpr int KSTEPS = KPAIRS * 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = blockIdx.y;
    const int c = blockIdx.x * M8_WAVES + wave;
    if (c >= n_cand) return;
    // local doc index: given directly, or as a global id of a shard that starts at id_base
    int64_t doc;
    if (cand_ids) {
        const int64_t g = cand_ids[(int64_t)q * n_cand + c];
        doc = g >= 0 ? g - id_base : -1;
    } else {
        doc = cand[(int64_t)q * n_cand + c];
    }
    if (doc < 0 || doc >= n_docs) {
        if (lane == 0) out[(int64_t)q * n_cand + c] = -INFINITY;
        return;
    }
    const int r = lane & 31, h = lane >> 5;
    const f8_u32x4* C = reinterpret_cast<const f8_u32x4*>(codes + doc * (int64_t)d_tokens * TD);
    const float* S = scales + doc * (int64_t)d_tokens;
    const int tiles = d_tokens / 32;
    float total = 0.f;
    for (int n0 = 0; n0 < q_tokens; n0 += 32) {
        // B fragments of this 32-query-token tile: lane holds Q[n0 + r][16*ks + 8*h + j]
        f8_half8 bq[KSTEPS];
        const _Float16* Q = qtok + ((int64_t)q * q_tokens + n0 + r) * TD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) bq[ks] = *reinterpret_cast<const f8_half8*>(Q + 16 * ks);
        float mx = -INFINITY;
        int t = 0;
        for (; t + 1 < tiles; t += 2) {    // the loads of both tiles go out before the first MFMA
            Tile8<KPAIRS> t0, t1;
            tile8_load<KPAIRS>(t0, C, S, t, lane);
            tile8_load<KPAIRS>(t1, C, S, t + 1, lane);
            __builtin_amdgcn_sched_barrier(0);    // (the scheduler would sink half of them between the MFMAs)
            mx = tile8_max<KPAIRS>(t0, bq, mx);
            mx = tile8_max<KPAIRS>(t1, bq, mx);
        }
        if (t < tiles) {
            Tile8<KPAIRS> t0;
            tile8_load<KPAIRS>(t0, C, S, t, lane);
            mx = tile8_max<KPAIRS>(t0, bq, mx);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));  // the two 16-row halves of every tile
        float s = mx;
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m, WAVE);
        total += s;
    }
    if (lane == 0) out[(int64_t)q * n_cand + c] = total;
}

}  // namespace thr

using namespace thr;

// tok_dim / 32 of the scorer's instantiations.  THE list: the switch of launch_maxsim_fp8 and the shape
// check of every entry point here are both made from it; _native.MAXSIM_FP8_TOK_DIMS restates it and
// tests/test_maxsim_fp8_host.py holds the two together.  (maxsim.hip's own list and shape check are
// restated, not shared: that file stays as it is, to the byte of its object code.)
#define THR_M8_KPAIRS(X) X(1) X(2) X(3) X(4) X(6) X(8)

static bool fp8_tok_dim_supported(int tok_dim) {
    if (tok_dim <= 0 || tok_dim % 32) return false;
    switch (tok_dim / 32) {
#define THR_M8_LABEL(KP) case KP:
        THR_M8_KPAIRS(THR_M8_LABEL)
#undef THR_M8_LABEL
        return true;
        default:
            return false;
    }
}

// Shapes are refused before any pointer is looked at (host arithmetic: no GPU needed to ask).
static bool fp8_tokens_supported(int n_tokens, int tok_dim) {
    return n_tokens > 0 && n_tokens % 32 == 0 && fp8_tok_dim_supported(tok_dim);
}

// Largest gridDim.y of the current device (65535 when it cannot be asked)
static int fp8_max_grid_y() {
    static int gy = 0;
    if (!gy) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            gy = prop.maxGridSize[1];
        if (gy <= 0) gy = 65535;
    }
    return gy;
}

extern "C" int thr_maxsim_quantize_fp8(const uint16_t* dtok, int64_t n_docs, int d_tokens, int tok_dim,
                                       uint8_t* out_codes, float* out_scales, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!fp8_tokens_supported(d_tokens, tok_dim), THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!dtok || !out_codes || !out_scales || (const void*)dtok == (const void*)out_codes || n_docs <= 0,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_docs > INT64_MAX / d_tokens, THR_ERR_UNSUPPORTED);
    const int64_t n_tokens = n_docs * d_tokens;
    constexpr int per_block = M8_THREADS / 32;
    const int64_t blocks = (n_tokens + per_block - 1) / per_block;
    THR_RETURN_IF(blocks > 0x7fffffffll, THR_ERR_UNSUPPORTED);
    hipLaunchKernelGGL(maxsim_quantize_fp8_kernel, dim3((unsigned)blocks), dim3(M8_THREADS), 0,
                       (hipStream_t)stream, reinterpret_cast<const _Float16*>(dtok), n_tokens, d_tokens,
                       tok_dim / 8, out_codes, out_scales);
    return launch_status();
}

static int launch_maxsim_fp8(const uint16_t* qtok, int n_queries, int q_tokens, const uint8_t* codes,
                             const float* scales, int64_t n_docs, int d_tokens, int tok_dim,
                             const int32_t* cand, const int64_t* cand_ids, int64_t id_base, int n_cand,
                             float* out_scores, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!fp8_tokens_supported(q_tokens, tok_dim) || !fp8_tokens_supported(d_tokens, tok_dim),
                  THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!qtok || !codes || !scales || (!cand && !cand_ids) || !out_scores, THR_ERR_INVALID);
    THR_RETURN_IF(n_queries <= 0 || n_docs <= 0 || n_cand <= 0, THR_ERR_INVALID);
    hipStream_t st = (hipStream_t)stream;
    // queries sit on gridDim.y: a batch above the device's limit goes out in slices of at most
    // that many queries, each a launch of its own over its rows of qtok, cand / cand_ids and out
    const int slice = fp8_max_grid_y();
    for (int q0 = 0; q0 < n_queries; q0 += slice) {
        dim3 grid((n_cand + M8_WAVES - 1) / M8_WAVES, n_queries - q0 < slice ? n_queries - q0 : slice);
        const _Float16* Q = reinterpret_cast<const _Float16*>(qtok) + (int64_t)q0 * q_tokens * tok_dim;
        const int32_t* C = cand ? cand + (int64_t)q0 * n_cand : nullptr;
        const int64_t* G = cand_ids ? cand_ids + (int64_t)q0 * n_cand : nullptr;
        float* out = out_scores + (int64_t)q0 * n_cand;
#define THR_M8_CASE(KP)                                                                             \
    case KP:                                                                                        \
        hipLaunchKernelGGL((maxsim_fp8_kernel<KP>), grid, dim3(M8_THREADS), 0, st, Q, q_tokens,     \
                           codes, scales, n_docs, d_tokens, C, G, id_base, n_cand, out);            \
        break;
        switch (tok_dim / 32) {
            THR_M8_KPAIRS(THR_M8_CASE)
            default:
                return THR_ERR_UNSUPPORTED;
        }
#undef THR_M8_CASE
    }
    return launch_status();
}

extern "C" int thr_maxsim_fp8(const uint16_t* qtok, int n_queries, int q_tokens, const uint8_t* codes,
                              const float* scales, int64_t n_docs, int d_tokens, int tok_dim,
                              const int32_t* cand, int n_cand, float* out_scores, thr_stream_t stream) {
    return launch_maxsim_fp8(qtok, n_queries, q_tokens, codes, scales, n_docs, d_tokens, tok_dim, cand,
                             nullptr, 0, n_cand, out_scores, stream);
}

extern "C" int thr_maxsim_fp8_ids(const uint16_t* qtok, int n_queries, int q_tokens, const uint8_t* codes,
                                  const float* scales, int64_t n_docs, int d_tokens, int tok_dim,
                                  const int64_t* cand_ids, int64_t id_base, int n_cand, float* out_scores,
                                  thr_stream_t stream) {
    return launch_maxsim_fp8(qtok, n_queries, q_tokens, codes, scales, n_docs, d_tokens, tok_dim, nullptr,
                             cand_ids, id_base, n_cand, out_scores, stream);
}
