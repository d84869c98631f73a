// Stand-alone host check of the argument checks of thr_maxsim_quantize_fp8, thr_maxsim_fp8 and
// thr_maxsim_fp8_ids: built together with csrc/maxsim_fp8.hip with the host side under AddressSanitizer +
// UBSan and run on the CPU (tests/test_maxsim_fp8_host.py does both).  Every call below is refused on the
// host, before any launch: no device is needed and none is touched.
#include <cstdint>
#include <cstdio>

#include "../../include/thr_hip_rerank.h"

static int failures = 0;

#define EXPECT(cond)                                               \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                            \
        }                                                          \
    } while (0)

// non-null, aligned pointer values that are never dereferenced on the host
static const uint16_t* const P16 = (const uint16_t*)4096;
static uint8_t* const P8 = (uint8_t*)8192;
static float* const PF = (float*)12288;
static const int32_t* const P32 = (const int32_t*)16384;
static const int64_t* const P64 = (const int64_t*)20480;
static float* const POUT = (float*)24576;

static int quant(int64_t n_docs, int d_tokens, int tok_dim, const uint16_t* dtok = nullptr, uint8_t* codes = nullptr,
                 float* scales = nullptr) {
    return thr_maxsim_quantize_fp8(dtok, n_docs, d_tokens, tok_dim, codes, scales, nullptr);
}

static int score(int n_queries, int q_tokens, int64_t n_docs, int d_tokens, int tok_dim, int n_cand,
                 const uint16_t* q = nullptr, const uint8_t* codes = nullptr, const float* scales = nullptr,
                 const int32_t* cand = nullptr, float* out = nullptr) {
    return thr_maxsim_fp8(q, n_queries, q_tokens, codes, scales, n_docs, d_tokens, tok_dim, cand, n_cand, out, nullptr);
}

static int score_ids(int n_queries, int q_tokens, int64_t n_docs, int d_tokens, int tok_dim, int n_cand,
                     const uint16_t* q = nullptr, const uint8_t* codes = nullptr, const float* scales = nullptr,
                     const int64_t* cand = nullptr, float* out = nullptr) {
    return thr_maxsim_fp8_ids(q, n_queries, q_tokens, codes, scales, n_docs, d_tokens, tok_dim, cand, 7, n_cand, out,
                              nullptr);
}

int main() {
    // shapes first, before any pointer is looked at: with null pointers a supported shape is THR_ERR_INVALID
    for (int td = -64; td <= 288; ++td) {
        const bool ok = td == 32 || td == 64 || td == 96 || td == 128 || td == 192 || td == 256;
        const int want = ok ? THR_ERR_INVALID : THR_ERR_UNSUPPORTED;
        EXPECT(quant(1, 32, td) == want);
        EXPECT(score(1, 32, 1, 32, td, 1) == want);
        EXPECT(score_ids(1, 32, 1, 32, td, 1) == want);
    }
    const int bad_tokens[] = {0, -32, 1, 31, 33, 48, INT32_MIN, INT32_MAX};
    for (int n : bad_tokens) {
        EXPECT(quant(1, n, 128) == THR_ERR_UNSUPPORTED);
        EXPECT(score(1, n, 1, 32, 128, 1) == THR_ERR_UNSUPPORTED && score(1, 32, 1, n, 128, 1) == THR_ERR_UNSUPPORTED);
        EXPECT(score_ids(1, n, 1, 32, 128, 1) == THR_ERR_UNSUPPORTED && score_ids(1, 32, 1, n, 128, 1) == THR_ERR_UNSUPPORTED);
        // ... even with every pointer given
        EXPECT(quant(1, n, 128, P16, P8, PF) == THR_ERR_UNSUPPORTED);
        EXPECT(score(1, n, 1, 32, 128, 1, P16, P8, PF, P32, POUT) == THR_ERR_UNSUPPORTED);
    }
    // the quantiser: null pointers, in place, counts, a store above the grid
    EXPECT(quant(1, 32, 128, nullptr, P8, PF) == THR_ERR_INVALID);
    EXPECT(quant(1, 32, 128, P16, nullptr, PF) == THR_ERR_INVALID);
    EXPECT(quant(1, 32, 128, P16, P8, nullptr) == THR_ERR_INVALID);
    EXPECT(quant(1, 32, 128, P16, (uint8_t*)P16, PF) == THR_ERR_INVALID);
    EXPECT(quant(0, 32, 128, P16, P8, PF) == THR_ERR_INVALID);
    EXPECT(quant(-1, 32, 128, P16, P8, PF) == THR_ERR_INVALID);
    EXPECT(quant(INT64_MAX, 32, 128, P16, P8, PF) == THR_ERR_UNSUPPORTED);
    EXPECT(quant((int64_t)1 << 29, 32, 128, P16, P8, PF) == THR_ERR_UNSUPPORTED);    // 2^31 blocks of 8 tokens
    // the scorers: null pointers and non-positive counts
    EXPECT(score(1, 32, 1, 32, 128, 1, nullptr, P8, PF, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score(1, 32, 1, 32, 128, 1, P16, nullptr, PF, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score(1, 32, 1, 32, 128, 1, P16, P8, nullptr, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score(1, 32, 1, 32, 128, 1, P16, P8, PF, nullptr, POUT) == THR_ERR_INVALID);
    EXPECT(score(1, 32, 1, 32, 128, 1, P16, P8, PF, P32, nullptr) == THR_ERR_INVALID);
    EXPECT(score(0, 32, 1, 32, 128, 1, P16, P8, PF, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score(-1, 32, 1, 32, 128, 1, P16, P8, PF, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score(1, 32, 0, 32, 128, 1, P16, P8, PF, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score(1, 32, 1, 32, 128, 0, P16, P8, PF, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score(1, 32, 1, 32, 128, -5, P16, P8, PF, P32, POUT) == THR_ERR_INVALID);
    EXPECT(score_ids(1, 32, 1, 32, 128, 1, nullptr, P8, PF, P64, POUT) == THR_ERR_INVALID);
    EXPECT(score_ids(1, 32, 1, 32, 128, 1, P16, nullptr, PF, P64, POUT) == THR_ERR_INVALID);
    EXPECT(score_ids(1, 32, 1, 32, 128, 1, P16, P8, nullptr, P64, POUT) == THR_ERR_INVALID);
    EXPECT(score_ids(1, 32, 1, 32, 128, 1, P16, P8, PF, nullptr, POUT) == THR_ERR_INVALID);
    EXPECT(score_ids(1, 32, 1, 32, 128, 1, P16, P8, PF, P64, nullptr) == THR_ERR_INVALID);
    EXPECT(score_ids(0, 32, 1, 32, 128, 1, P16, P8, PF, P64, POUT) == THR_ERR_INVALID);
    EXPECT(score_ids(1, 32, -1, 32, 128, 1, P16, P8, PF, P64, POUT) == THR_ERR_INVALID);
    EXPECT(score_ids(1, 32, 1, 32, 128, 0, P16, P8, PF, P64, POUT) == THR_ERR_INVALID);
    std::printf(failures ? "maxsim_fp8 host check: %d FAILED\n" : "maxsim_fp8 host check: ok\n", failures);
    return failures ? 1 : 0;
}
