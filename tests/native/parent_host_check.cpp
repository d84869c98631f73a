// Stand-alone host check of the argument checks of thr_parent_groups, thr_maxsim_parent_ids and
// thr_maxsim_parent_fp8_ids: built together with csrc/maxsim_parent.hip with the host side under
// AddressSanitizer + UBSan and run on the CPU (tests/test_parent_host.py does both).  Every call below is
// refused on the host, before any launch: no device is needed and none is touched.
#include <cstdint>
#include <cstdio>

#include "../../include/thr_hip_parent.h"

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
static const uint8_t* const P8 = (const uint8_t*)8192;
static const float* const PF = (const float*)12288;
static int32_t* const P32 = (int32_t*)16384;
static int64_t* const P64 = (int64_t*)20480;
static float* const POUT = (float*)24576;

struct Args {
    const uint16_t* q = P16;
    int n_queries = 1, q_tokens = 32;
    const void* store = P8;
    const float* scales = PF;
    int64_t n_docs = 4;
    int d_tokens = 32, tok_dim = 128;
    const int64_t* cand = P64;
    int n_cand = 1;
    const int32_t* parent_of = P32;
    const int64_t* rowptr = P64;
    const int32_t* child = P32;
    int n_parents = 2;
    int64_t nnz = 4;
    float* out = POUT;
};

static Args nulls() {
    Args a;
    a.q = nullptr;
    a.store = nullptr;
    a.scales = nullptr;
    a.cand = nullptr;
    a.parent_of = nullptr;
    a.rowptr = nullptr;
    a.child = nullptr;
    a.out = nullptr;
    return a;
}

static int f16(const Args& a) {
    return thr_maxsim_parent_ids(a.q, a.n_queries, a.q_tokens, (const uint16_t*)a.store, a.n_docs, a.d_tokens, a.tok_dim,
                                 a.cand, 7, a.n_cand, a.parent_of, a.rowptr, a.child, a.n_parents, a.nnz, a.out, nullptr);
}

static int fp8(const Args& a) {
    return thr_maxsim_parent_fp8_ids(a.q, a.n_queries, a.q_tokens, (const uint8_t*)a.store, a.scales, a.n_docs, a.d_tokens,
                                     a.tok_dim, a.cand, 7, a.n_cand, a.parent_of, a.rowptr, a.child, a.n_parents, a.nnz,
                                     a.out, nullptr);
}

static int groups(int n_queries, int n, int64_t n_docs, const int64_t* ids = P64, const int32_t* counts = nullptr,
                  const int32_t* parent_of = P32, int32_t* leader = P32, int32_t* slot = P32, int64_t* uniq = P64,
                  int32_t* n_uniq = P32) {
    return thr_parent_groups(ids, counts, n_queries, n, parent_of, n_docs, 0, leader, slot, uniq, n_uniq, nullptr);
}

int main() {
    // shapes first, before any pointer is looked at: with null pointers a supported shape is THR_ERR_INVALID
    for (int td = -64; td <= 288; ++td) {
        const bool ok8 = td == 32 || td == 64 || td == 96 || td == 128 || td == 192 || td == 256;
        const bool ok16 = ok8 || td == 16;
        Args a = nulls();
        a.tok_dim = td;
        EXPECT(f16(a) == (ok16 ? THR_ERR_INVALID : THR_ERR_UNSUPPORTED));
        EXPECT(fp8(a) == (ok8 ? THR_ERR_INVALID : THR_ERR_UNSUPPORTED));
    }
    const int bad_tokens[] = {0, -32, 1, 31, 33, 48, INT32_MIN, INT32_MAX};
    for (int n : bad_tokens) {
        Args a;     // ... even with every pointer given
        a.q_tokens = n;
        EXPECT(f16(a) == THR_ERR_UNSUPPORTED && fp8(a) == THR_ERR_UNSUPPORTED);
        Args b;
        b.d_tokens = n;
        EXPECT(f16(b) == THR_ERR_UNSUPPORTED && fp8(b) == THR_ERR_UNSUPPORTED);
    }
    {
        Args a;
        a.n_docs = (int64_t)1 << 31;      // children are int32 rows
        EXPECT(f16(a) == THR_ERR_UNSUPPORTED && fp8(a) == THR_ERR_UNSUPPORTED);
        a.n_docs = INT64_MAX;
        EXPECT(f16(a) == THR_ERR_UNSUPPORTED && fp8(a) == THR_ERR_UNSUPPORTED);
    }
    // null pointers, one at a time
    for (int i = 0; i < 8; ++i) {
        Args a;
        switch (i) {
            case 0: a.q = nullptr; break;
            case 1: a.store = nullptr; break;
            case 2: a.cand = nullptr; break;
            case 3: a.parent_of = nullptr; break;
            case 4: a.rowptr = nullptr; break;
            case 5: a.child = nullptr; break;
            case 6: a.out = nullptr; break;
            default: a.scales = nullptr; break;
        }
        EXPECT(fp8(a) == THR_ERR_INVALID);
        if (i < 7) EXPECT(f16(a) == THR_ERR_INVALID);      // (the float16 scorer takes no scales)
    }
    // non-positive counts
    for (int i = 0; i < 5; ++i) {
        for (int v : {0, -1}) {
            Args a;
            switch (i) {
                case 0: a.n_queries = v; break;
                case 1: a.n_docs = v; break;
                case 2: a.n_cand = v; break;
                case 3: a.n_parents = v; break;
                default: a.nnz = v; break;
            }
            EXPECT(f16(a) == THR_ERR_INVALID && fp8(a) == THR_ERR_INVALID);
        }
    }
    // the groups: n outside 1 .. THR_RRF_MAX_TOP_K first, then pointers, then counts
    const int bad_n[] = {0, -1, THR_RRF_MAX_TOP_K + 1, INT32_MAX, INT32_MIN};
    for (int n : bad_n) {
        EXPECT(groups(1, n, 4) == THR_ERR_UNSUPPORTED);
        EXPECT(groups(1, n, 4, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == THR_ERR_UNSUPPORTED);
    }
    EXPECT(groups(1, 1, 4, nullptr) == THR_ERR_INVALID);
    EXPECT(groups(1, THR_RRF_MAX_TOP_K, 4, P64, nullptr, nullptr) == THR_ERR_INVALID);
    EXPECT(groups(1, 8, 4, P64, nullptr, P32, nullptr) == THR_ERR_INVALID);
    EXPECT(groups(1, 8, 4, P64, nullptr, P32, P32, nullptr) == THR_ERR_INVALID);
    EXPECT(groups(1, 8, 4, P64, nullptr, P32, P32, P32, nullptr) == THR_ERR_INVALID);
    EXPECT(groups(1, 8, 4, P64, nullptr, P32, P32, P32, P64, nullptr) == THR_ERR_INVALID);
    EXPECT(groups(0, 8, 4) == THR_ERR_INVALID && groups(-2, 8, 4) == THR_ERR_INVALID);
    EXPECT(groups(1, 8, 0) == THR_ERR_INVALID && groups(1, 8, -1) == THR_ERR_INVALID);
    std::printf(failures ? "parent host check: %d FAILED\n" : "parent host check: ok\n", failures);
    return failures ? 1 : 0;
}
