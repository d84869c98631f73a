// Stand-alone host check of the argument checks of thr_mmr_select: built together with csrc/mmr.hip with the
// host side under AddressSanitizer + UBSan and run on the CPU (tests/test_mmr_host.py does both).  Every call
// below is refused on the host, before any launch: no device is needed and none is touched.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "../../include/thr_hip_diversify.h"

static int failures = 0;

#define EXPECT(cond)                                               \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                            \
        }                                                          \
    } while (0)

// non-null, aligned pointer values that are never dereferenced on the host
static int64_t* const P64 = (int64_t*)4096;
static double* const PD = (double*)8192;
static int32_t* const P32 = (int32_t*)12288;
static float* const PF = (float*)16384;

struct Args {
    const int64_t* ids = P64;
    const double* scores = PD;
    const int32_t* counts = nullptr;
    int n_queries = 2, n = 8;
    const float* docs = PF;
    const double* dnorm = PD;
    int64_t n_docs = 16;
    int dim = 64;
    int64_t id_base = 7;
    double lam = 0.5;
    int top_k = 4;
    int64_t* out_ids = P64;
    double* out_scores = PD;
    int32_t* out_pos = P32;
    double* out_mmr = nullptr;
    int32_t* out_counts = P32;
};

static Args nulls() {
    Args a;
    a.ids = nullptr;
    a.scores = nullptr;
    a.docs = nullptr;
    a.dnorm = nullptr;
    a.out_ids = nullptr;
    a.out_scores = nullptr;
    a.out_pos = nullptr;
    a.out_counts = nullptr;
    return a;
}

static int call(const Args& a) {
    return thr_mmr_select(a.ids, a.scores, a.counts, a.n_queries, a.n, a.docs, a.dnorm, a.n_docs, a.dim, a.id_base, a.lam,
                          a.top_k, a.out_ids, a.out_scores, a.out_pos, a.out_mmr, a.out_counts, nullptr);
}

int main() {
    // shapes first, before any pointer is looked at: with null pointers a supported shape is THR_ERR_INVALID
    for (int dim = -8; dim <= THR_DENSE_ANYDIM_MAX + 8; ++dim) {
        const bool ok = dim >= 4 && dim <= THR_DENSE_ANYDIM_MAX && dim % 4 == 0;
        Args a = nulls();
        a.dim = dim;
        EXPECT(call(a) == (ok ? THR_ERR_INVALID : THR_ERR_UNSUPPORTED));
    }
    for (int dim : {INT32_MIN, INT32_MAX, 1 << 20}) {
        Args a;     // ... even with every pointer given
        a.dim = dim;
        EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    }
    for (int n : {0, -1, THR_RRF_MAX_TOP_K + 1, INT32_MAX, INT32_MIN}) {
        Args a;
        a.n = n;
        a.top_k = 1;
        EXPECT(call(a) == THR_ERR_UNSUPPORTED);
        Args b = nulls();
        b.n = n;
        EXPECT(call(b) == THR_ERR_UNSUPPORTED);
    }
    for (int n : {1, 64, THR_RRF_MAX_TOP_K}) {
        for (int k : {0, -1, n + 1, INT32_MAX, INT32_MIN}) {
            Args a;
            a.n = n;
            a.top_k = k;
            EXPECT(call(a) == THR_ERR_UNSUPPORTED);
        }
        Args a = nulls();
        a.n = n;
        a.top_k = n;
        EXPECT(call(a) == THR_ERR_INVALID);
    }
    for (int64_t nd : {(int64_t)1 << 31, INT64_MAX}) {
        Args a;
        a.n_docs = nd;          // a row number is an int32
        EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    }
    // null pointers, one at a time; counts and out_mmr may be null
    for (int i = 0; i < 8; ++i) {
        Args a;
        a.counts = P32;
        a.out_mmr = PD;
        switch (i) {
            case 0: a.ids = nullptr; break;
            case 1: a.scores = nullptr; break;
            case 2: a.docs = nullptr; break;
            case 3: a.dnorm = nullptr; break;
            case 4: a.out_ids = nullptr; break;
            case 5: a.out_scores = nullptr; break;
            case 6: a.out_pos = nullptr; break;
            default: a.out_counts = nullptr; break;
        }
        EXPECT(call(a) == THR_ERR_INVALID);
    }
    // non-positive counts
    for (int v : {0, -1, INT32_MIN}) {
        Args a;
        a.n_queries = v;
        EXPECT(call(a) == THR_ERR_INVALID);
        Args b;
        b.n_docs = v;
        EXPECT(call(b) == THR_ERR_INVALID);
    }
    // lam outside [0, 1]
    const double inf = std::numeric_limits<double>::infinity();
    for (double lam : {std::nextafter(0.0, -1.0), -1.0, std::nextafter(1.0, 2.0), 2.0, inf, -inf,
                       std::numeric_limits<double>::quiet_NaN()}) {
        Args a;
        a.lam = lam;
        EXPECT(call(a) == THR_ERR_INVALID);
    }
    // (the shape wins over lam and the pointers)
    {
        Args a = nulls();
        a.lam = 2.0;
        a.dim = 6;
        EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    }
    std::printf(failures ? "mmr host check: %d FAILED\n" : "mmr host check: ok\n", failures);
    return failures ? 1 : 0;
}
