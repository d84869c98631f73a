/* thr_hip_rerank.h -- the FP8 token store of the late-interaction rerank: entry points of libthr_hip.so
 * that came after ABI version 9.
 *
 * An additive companion of thr_hip.h (same library, same conventions, THR_ABI_VERSION unchanged): every
 * pointer is device memory, all work is enqueued on ``stream``, nothing synchronises, allocates or frees,
 * no entry point here takes a workspace; 0 on success, a negative THR_ERR_* for an argument error, a
 * positive hipError_t if a launch failed.
 *
 * THE STORE.  A document token x (float16 [tok_dim]) is kept as tok_dim OCP E4M3FN bytes and one float32
 * scale:  x_k ~ scale * value_e4m3(code_k).  Only the DOCUMENT tokens are compressed; query tokens stay
 * float16 and the product stays v_mfma_f32_32x32x16_f16 -- a code is turned into the float16 of the same
 * value in registers (every E4M3 value is a float16: the conversion is exact), the scale is applied in
 * float32 to the accumulator row of its token, after the matrix product and before the max:
 *
 *     s_ij     = scale[c][j] * sum_k qtok[q][i][k] * value_e4m3(code[c][j][k])     (sum in float32)
 *     score    = sum_i max_j s_ij
 *
 * so the oracle of a score is MaxSim over the DEQUANTISED tokens (scale * value, in float64), and the
 * float32 forward-error bound of thr_maxsim holds with one more rounding, that of the scale multiply,
 * which is exact when the scale is a power of two (tests/maxsim_fp8_cases.py error_bound_fp8).
 *
 * THE IMAGE (codes).  Always fragment-major, d_tokens * tok_dim bytes per document, documents back to back:
 *
 *     [doc][tile of 32 tokens][k-pair = tok_dim / 32][lane 0..63][16 bytes]
 *
 * lane 32 h + r holds token 32 tile + r; its bytes 0..7 are dims 32 kp + 8 h .. + 8 (the A operand of
 * k-step 2 kp), its bytes 8..15 dims 32 kp + 16 + 8 h .. + 8 (k-step 2 kp + 1).  A load instruction of
 * the scorer reads 1 KiB contiguous and each lane's 16 bytes feed two MFMAs.  tok_dim is therefore a
 * multiple of 32 -- the entry points take 32, 64, 96, 128, 192 and 256 (16, which thr_maxsim takes, is
 * refused) -- and d_tokens, q_tokens are positive multiples of 32, as for thr_maxsim.
 * scales is float32 [n_docs][d_tokens], row-major.
 *
 * THE QUANTISER that ships (thr_maxsim_quantize_fp8) chooses a power of two per token:
 *
 *     amax = max_k |x_k|;   e = floor(log2(448 / amax)), 0 when amax == 0
 *     code_k = RNE_e4m3(x_k * 2^e);   scale = 2^-e
 *
 * x_k * 2^e is exact in float32 and at most 448 in magnitude, so nothing saturates and the NaN code (0x7f
 * / 0xff) is never produced; rounding is to nearest, ties to the even code, subnormals of the E4M3 grid
 * included; the sign of a zero is kept.  For finite float16 input e lies in -8 .. 32.  One half-wave per
 * token: amax, exponent, convert, write in the packed place; out of place, no workspace, integer
 * arithmetic on the bits of exact float32 values only: the same bits every run.
 * NON-FINITE input tokens (inf, NaN) are outside the contract, as NaN is everywhere in this library: what
 * is stored for such a token is unspecified (nothing outside the token's own bytes and scale is written).
 *
 * THE SCORERS (thr_maxsim_fp8, thr_maxsim_fp8_ids) take ANY finite positive scale, a power of two or not,
 * and any of the 254 finite codes (0x7f / 0xff are E4M3FN's NaNs: outside the contract, as NaN is); their
 * candidate semantics are thr_maxsim's / thr_maxsim_ids': cand holds local document indices, cand_ids global ids of a
 * shard that starts at id_base; a negative candidate, one at or above n_docs and one of another shard
 * score -inf; one wave per (query, candidate); any n_queries, sent out in slices of at most the device's
 * gridDim.y.  A wave issues the loads of two 32-token tiles (codes and scales) before the first MFMA of
 * the pair; an odd tile count ends with a single tile.
 *
 * Refused before any pointer is looked at (THR_ERR_UNSUPPORTED): a tok_dim outside the list, a q_tokens /
 * d_tokens that is not a positive multiple of 32, a store of more than 2^31 - 1 half-wave groups of 8
 * tokens (quantiser).  THR_ERR_INVALID: a null pointer, a non-positive n_docs / n_queries / n_cand,
 * out_codes == dtok. */
#ifndef THR_HIP_RERANK_H
#define THR_HIP_RERANK_H

#include "thr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int thr_maxsim_quantize_fp8(const uint16_t *dtok /* f16 [n_docs, d_tokens, tok_dim] */, int64_t n_docs,
                            int d_tokens, int tok_dim, uint8_t *out_codes /* the packed image */,
                            float *out_scales /* [n_docs, d_tokens] */, thr_stream_t stream);
int thr_maxsim_fp8(const uint16_t *qtok /* f16 [n_queries, q_tokens, tok_dim] */, int n_queries, int q_tokens,
                   const uint8_t *codes, const float *scales, int64_t n_docs, int d_tokens, int tok_dim,
                   const int32_t *cand /* [n_queries, n_cand] */, int n_cand,
                   float *out_scores /* [n_queries, n_cand] */, thr_stream_t stream);
int thr_maxsim_fp8_ids(const uint16_t *qtok, int n_queries, int q_tokens, const uint8_t *codes,
                       const float *scales, int64_t n_docs, int d_tokens, int tok_dim,
                       const int64_t *cand_ids /* [n_queries, n_cand] */, int64_t id_base, int n_cand,
                       float *out_scores, thr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* THR_HIP_RERANK_H */
