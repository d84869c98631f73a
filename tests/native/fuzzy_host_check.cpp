// Stand-alone host check of the argument checks and the size functions of thr_vocab_nearest and
// thr_query_terms_fuzzy: built together with csrc/fuzzy.hip with the host side under AddressSanitizer + UBSan and
// run on the CPU (tests/test_fuzzy_host.py does both).  Every call below is refused on the host, before any
// launch: no device is needed and none is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/thr_hip_fuzzy.h"

static int failures = 0;

#define EXPECT(cond)                                               \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                            \
        }                                                          \
    } while (0)

struct Nearest {
    // non-null, aligned pointer values that are never dereferenced on the host
    const uint8_t* text_bytes = (const uint8_t*)4097;       // (no alignment is asked of the text)
    int64_t n_bytes = 100;
    const uint32_t* table = (const uint32_t*)8192;
    const int64_t* unknown_off = (const int64_t*)12288;
    const int32_t* unknown_len = (const int32_t*)16384;
    const int32_t* n_unknown = (const int32_t*)20480;
    int64_t unknown_capacity = 50;
    const uint8_t* term_bytes = (const uint8_t*)24577;      // (nor of the key store)
    const int64_t* term_ptr = (const int64_t*)28672;
    int64_t n_vocab = 512, n_term_bytes = 4000;
    const int64_t* term_rowptr = (const int64_t*)32768;
    int max_edits = 2, n_best = 4;
    int32_t* near_term = (int32_t*)36864;
    int32_t* near_dist = (int32_t*)40960;
    void* workspace = (void*)45056;
    size_t workspace_bytes = 0;      // too small for everything that gets that far
};

static int call(const Nearest& a) {
    return thr_vocab_nearest(a.text_bytes, a.n_bytes, a.table, a.unknown_off, a.unknown_len, a.n_unknown,
                             a.unknown_capacity, a.term_bytes, a.term_ptr, a.n_vocab, a.n_term_bytes, a.term_rowptr,
                             a.max_edits, a.n_best, a.near_term, a.near_dist, a.workspace, a.workspace_bytes, nullptr);
}

struct Query {
    const int32_t* tok_term = (const int32_t*)4096;
    const int32_t* n_tokens = (const int32_t*)8192;
    const int32_t* text_flags = (const int32_t*)12288;
    const int32_t* n_total = (const int32_t*)16384;
    int64_t token_capacity = 52;
    int n_queries = 3;
    const int32_t* near_term = (const int32_t*)20480;
    int64_t near_capacity = 52;
    int n_best = 3, n_use = 2;
    int32_t* out_terms = (int32_t*)24576;
    int32_t* n_distinct = (int32_t*)28672;
    int32_t* out_flags = (int32_t*)32768;
    void* workspace = (void*)36864;
    size_t workspace_bytes = 0;
};

static int call(const Query& a) {
    return thr_query_terms_fuzzy(a.tok_term, a.n_tokens, a.text_flags, a.n_total, a.token_capacity, a.n_queries,
                                 a.near_term, a.near_capacity, a.n_best, a.n_use, a.out_terms, a.n_distinct, a.out_flags,
                                 a.workspace, a.workspace_bytes, nullptr);
}

int main() {
    EXPECT(THR_FUZZY_MAX_LEN == 32 && THR_FUZZY_MAX_BEST == 4 && THR_FUZZY_SLICE_BYTES == 8192 && THR_TEXT_CORRECTED == 8);
    EXPECT((THR_TEXT_CORRECTED & (THR_TEXT_EXCEPTIONAL | THR_TEXT_UNKNOWN | THR_TEXT_TOO_MANY)) == 0);

    // ---- thr_vocab_nearest
    const size_t need = thr_vocab_nearest_workspace_bytes(100, 50, 512, 4000, 4);
    // two needle tables of 64 bytes a row, four int32 per needle, the length table, the slots: in 256-byte pieces
    EXPECT(need == 3328 + 3328 + 4 * 256 + 256 + 1792);
    EXPECT(thr_vocab_nearest_workspace_bytes(100, 50, 512, 4000, 1) == need - 1792 + 512);
    EXPECT(thr_vocab_nearest_workspace_bytes(-1, 50, 512, 4000, 4) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes((int64_t)THR_TEXT_MAX_BYTES + 1, 50, 512, 4000, 4) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes(100, 0, 512, 4000, 4) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes(100, (int64_t)THR_TEXT_MAX_BYTES + 1, 512, 4000, 4) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes(100, 50, (int64_t)INT32_MAX + 1, 4000, 4) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes(100, 50, 512, ((int64_t)1 << 43) + 1, 4) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes(100, 50, 512, 4000, 0) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes(100, 50, 512, 4000, 5) == 0);
    EXPECT(thr_vocab_nearest_workspace_bytes(0, 1, 0, 0, 1) > 0);          // an empty batch against an empty vocabulary

    Nearest ok;
    EXPECT(call(ok) == THR_ERR_WORKSPACE);      // every argument check passed: only the workspace is short
    Nearest a;
    a = ok; a.n_bytes = -1;                                       EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_bytes = (int64_t)THR_TEXT_MAX_BYTES + 1;          EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.unknown_capacity = 0;                               EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.unknown_capacity = (int64_t)THR_TEXT_MAX_BYTES + 1; EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_vocab = (int64_t)INT32_MAX + 1;                   EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_term_bytes = ((int64_t)1 << 43) + 1;              EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.text_bytes = nullptr;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.table = nullptr;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_off = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_len = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_unknown = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_bytes = nullptr;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_ptr = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.near_term = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.near_dist = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_rowptr = nullptr; EXPECT(call(a) == THR_ERR_WORKSPACE);      // no document frequencies
    a = ok; a.n_vocab = -1;          EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_vocab = 0;           EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.n_term_bytes = -1;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.max_edits = 0;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.max_edits = 3;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.max_edits = 1;         EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.n_best = 0;            EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_best = THR_FUZZY_MAX_BEST + 1;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_best = 1;            EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.unknown_off = (const int64_t*)12292;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_ptr = (const int64_t*)28676;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_rowptr = (const int64_t*)32772;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.table = (const uint32_t*)8194;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_len = (const int32_t*)16386;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_unknown = (const int32_t*)20482;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.near_term = (int32_t*)36866;           EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.near_dist = (int32_t*)40962;           EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace = (void*)45064; a.workspace_bytes = (size_t)1 << 20;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = need - 1;            EXPECT(call(a) == THR_ERR_WORKSPACE);

    // ---- thr_query_terms_fuzzy
    EXPECT(thr_query_terms_fuzzy_workspace_bytes(3) == 256 + 256);         // the rows' and the unknowns' scans
    EXPECT(thr_query_terms_fuzzy_workspace_bytes(0) == 0 && thr_query_terms_fuzzy_workspace_bytes(THR_TEXT_MAX_TEXTS + 1) == 0);
    Query qok;
    EXPECT(call(qok) == THR_ERR_WORKSPACE);
    Query q;
    q = qok; q.n_queries = 0;                          EXPECT(call(q) == THR_ERR_UNSUPPORTED);
    q = qok; q.n_queries = THR_TEXT_MAX_TEXTS + 1;     EXPECT(call(q) == THR_ERR_UNSUPPORTED);
    q = qok; q.token_capacity = 0;                     EXPECT(call(q) == THR_ERR_UNSUPPORTED);
    q = qok; q.token_capacity = (int64_t)THR_TEXT_MAX_BYTES + 1;   EXPECT(call(q) == THR_ERR_UNSUPPORTED);
    q = qok; q.tok_term = nullptr;    EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_tokens = nullptr;    EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.text_flags = nullptr;  EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_total = nullptr;     EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.near_term = nullptr;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.out_terms = nullptr;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_distinct = nullptr;  EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.out_flags = nullptr;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.workspace = nullptr;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.near_capacity = 0;     EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_best = 0;            EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_best = THR_FUZZY_MAX_BEST + 1; q.n_use = 1;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_use = 0;             EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_use = 4;             EXPECT(call(q) == THR_ERR_INVALID);      // above n_best
    q = qok; q.n_use = 3;             EXPECT(call(q) == THR_ERR_WORKSPACE);
    q = qok; q.workspace = (void*)36866; q.workspace_bytes = (size_t)1 << 20;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.workspace_bytes = thr_query_terms_fuzzy_workspace_bytes(3) - 1;  EXPECT(call(q) == THR_ERR_WORKSPACE);
    std::printf(failures ? "fuzzy host check: %d FAILED\n" : "fuzzy host check: ok\n", failures);
    return failures ? 1 : 0;
}
