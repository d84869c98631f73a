// Stand-alone host check of the argument checks and size functions of thr_vocab_insert, thr_text_tokens and
// thr_query_terms: built together with csrc/text.hip with the host side under AddressSanitizer + UBSan
// and run on the CPU (tests/test_text_host.py does both).  Every call below is refused on the host,
// before any launch: no device is needed and none is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/thr_hip.h"

static int failures = 0;

#define EXPECT(cond)                                               \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                            \
        }                                                          \
    } while (0)

struct Tokens {
    // non-null, aligned pointer values that are never dereferenced on the host
    const uint8_t* text_bytes = (const uint8_t*)4096;
    const int64_t* text_ptr = (const int64_t*)8192;
    int64_t n_texts = 3, n_bytes = 100;
    const uint32_t* table = (const uint32_t*)12288;
    const void* slots = (const void*)16384;
    int64_t capacity = 1024;
    const uint8_t* term_bytes = (const uint8_t*)20481;     // (bytes: no alignment asked)
    const int64_t* term_ptr = (const int64_t*)24576;
    int64_t n_vocab = 512, token_capacity = 52;
    int32_t* tok_doc = (int32_t*)28672;
    int32_t* tok_term = (int32_t*)32768;
    int32_t* n_tokens = (int32_t*)36864;
    int32_t* flags = (int32_t*)40960;
    int32_t* n_total = (int32_t*)45056;
    int64_t* unknown_off = (int64_t*)49152;
    int32_t* unknown_len = (int32_t*)53248;
    int32_t* n_unknown = (int32_t*)57344;
    void* workspace = (void*)61440;
    size_t workspace_bytes = 0;      // too small for everything that gets that far
};

static int call(const Tokens& a) {
    return thr_text_tokens(a.text_bytes, a.text_ptr, a.n_texts, a.n_bytes, a.table, a.slots, a.capacity, a.term_bytes,
                           a.term_ptr, a.n_vocab, a.token_capacity, a.tok_doc, a.tok_term, a.n_tokens, a.flags,
                           a.n_total, a.unknown_off, a.unknown_len, a.n_unknown, a.workspace, a.workspace_bytes, nullptr);
}

struct Query {
    const int32_t* tok_term = (const int32_t*)4096;
    const int32_t* n_tokens = (const int32_t*)8192;
    const int32_t* text_flags = (const int32_t*)12288;
    const int32_t* n_total = (const int32_t*)16384;
    int64_t token_capacity = 100;
    int n_queries = 7;
    int32_t* out_terms = (int32_t*)20480;
    int32_t* n_distinct = (int32_t*)24576;
    int32_t* out_flags = (int32_t*)28672;
    void* workspace = (void*)32768;
    size_t workspace_bytes = 0;
};

static int call(const Query& a) {
    return thr_query_terms(a.tok_term, a.n_tokens, a.text_flags, a.n_total, a.token_capacity, a.n_queries, a.out_terms,
                           a.n_distinct, a.out_flags, a.workspace, a.workspace_bytes, nullptr);
}

static int insert(void* slots, int64_t capacity, const void* bytes, const void* ptr, int64_t first, int64_t count) {
    return thr_vocab_insert(slots, capacity, (const uint8_t*)bytes, (const int64_t*)ptr, first, count, nullptr);
}

int main() {
    // ---- the vocabulary table
    EXPECT(thr_vocab_table_bytes(1024) == 16 * 1024 && thr_vocab_table_bytes(THR_VOCAB_MIN_SLOTS) == 16 * THR_VOCAB_MIN_SLOTS);
    EXPECT(thr_vocab_table_bytes(1000) == 0 && thr_vocab_table_bytes(0) == 0 && thr_vocab_table_bytes(-1024) == 0);
    EXPECT(thr_vocab_table_bytes(THR_VOCAB_MIN_SLOTS / 2) == 0 && thr_vocab_table_bytes(2 * (int64_t)THR_VOCAB_MAX_SLOTS) == 0);
    EXPECT(thr_vocab_table_bytes(THR_VOCAB_MAX_SLOTS) == (size_t)16 * THR_VOCAB_MAX_SLOTS);
    void* const S = (void*)4096;
    void* const B = (void*)8193;
    void* const P = (void*)12288;
    EXPECT(insert(nullptr, 1024, B, P, 0, 10) == THR_ERR_INVALID);
    EXPECT(insert(S, 1024, nullptr, P, 0, 10) == THR_ERR_INVALID);
    EXPECT(insert(S, 1024, B, nullptr, 0, 10) == THR_ERR_INVALID);
    EXPECT(insert(S, 1000, B, P, 0, 10) == THR_ERR_INVALID);                  // not a power of two
    EXPECT(insert(S, 0, B, P, 0, 10) == THR_ERR_INVALID);
    EXPECT(insert((void*)4104, 1024, B, P, 0, 10) == THR_ERR_INVALID);        // slots: 16-byte aligned
    EXPECT(insert(S, 1024, B, (void*)12292, 0, 10) == THR_ERR_INVALID);       // term_ptr: 8-byte aligned
    EXPECT(insert(S, 1024, B, P, -1, 10) == THR_ERR_INVALID);
    EXPECT(insert(S, 1024, B, P, 0, 0) == THR_ERR_INVALID);
    EXPECT(insert(S, 1024, B, P, 0, 513) == THR_ERR_INVALID);                 // above 1/2 load
    EXPECT(insert(S, 1024, B, P, 512, 1) == THR_ERR_INVALID);
    EXPECT(insert(S, 1024, B, P, INT64_MAX, 1) == THR_ERR_INVALID);

    // ---- thr_text_tokens
    EXPECT(THR_TEXT_SLICE_BYTES % 4096 == 0 && THR_TEXT_MAX_TEXTS == (1 << 20) && (int64_t)THR_TEXT_MAX_BYTES < ((int64_t)1 << 31));
    // the workspace: two int32 per quarter slice (+ 1), 12 bytes per token row; each piece rounded up to 256 bytes
    EXPECT(thr_text_tokens_workspace_bytes(1, 0, 1) == 4 * 256);
    EXPECT(thr_text_tokens_workspace_bytes(3, 100, 52) == 256 + 256 + 512 + 256);
    EXPECT(thr_text_tokens_workspace_bytes(1, (int64_t)THR_TEXT_SLICE_BYTES * 64, 1000) == 2 * 1280 + 8192 + 4096);
    EXPECT(thr_text_tokens_workspace_bytes(THR_TEXT_MAX_TEXTS, THR_TEXT_MAX_BYTES, THR_TEXT_MAX_BYTES) > (size_t)12 * THR_TEXT_MAX_BYTES);
    EXPECT(thr_text_tokens_workspace_bytes(0, 100, 52) == 0 && thr_text_tokens_workspace_bytes(-1, 100, 52) == 0);
    EXPECT(thr_text_tokens_workspace_bytes(THR_TEXT_MAX_TEXTS + 1, 100, 52) == 0);
    EXPECT(thr_text_tokens_workspace_bytes(3, -1, 52) == 0 && thr_text_tokens_workspace_bytes(3, (int64_t)THR_TEXT_MAX_BYTES + 1, 52) == 0);
    EXPECT(thr_text_tokens_workspace_bytes(3, INT64_MAX, 52) == 0);
    EXPECT(thr_text_tokens_workspace_bytes(3, 100, 0) == 0 && thr_text_tokens_workspace_bytes(3, 100, INT64_MAX) == 0);

    Tokens ok;
    EXPECT(call(ok) == THR_ERR_WORKSPACE);      // every argument check passed: only the workspace is short
    Tokens a;
    a = ok; a.n_texts = 0;                               EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_texts = THR_TEXT_MAX_TEXTS + 1;          EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_texts = THR_TEXT_MAX_TEXTS;              EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.n_bytes = -1;                              EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_bytes = (int64_t)THR_TEXT_MAX_BYTES + 1; EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_bytes = 0;                               EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.token_capacity = 0;                        EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.text_bytes = nullptr;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.text_ptr = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.table = nullptr;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.slots = nullptr;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_bytes = nullptr;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_ptr = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.tok_doc = nullptr;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.tok_term = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_tokens = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.flags = nullptr;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_total = nullptr;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_off = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_len = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_unknown = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.capacity = 1000;       EXPECT(call(a) == THR_ERR_INVALID);      // not a power of two
    a = ok; a.n_vocab = 513;         EXPECT(call(a) == THR_ERR_INVALID);      // above 1/2 load
    a = ok; a.n_vocab = -1;          EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_vocab = 0;           EXPECT(call(a) == THR_ERR_WORKSPACE);    // an empty vocabulary: fine
    a = ok; a.text_bytes = (const uint8_t*)4104;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.slots = (const void*)16392;          EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.text_ptr = (const int64_t*)8196;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.term_ptr = (const int64_t*)24580;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_off = (int64_t*)49156;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.table = (const uint32_t*)12290;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace = (void*)61444; a.workspace_bytes = (size_t)1 << 20;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = thr_text_tokens_workspace_bytes(ok.n_texts, ok.n_bytes, ok.token_capacity) - 1;
    EXPECT(call(a) == THR_ERR_WORKSPACE);

    // ---- thr_query_terms
    EXPECT(thr_query_terms_workspace_bytes(7) == 256 && thr_query_terms_workspace_bytes(64) == 512);
    EXPECT(thr_query_terms_workspace_bytes(0) == 0 && thr_query_terms_workspace_bytes(-5) == 0);
    EXPECT(thr_query_terms_workspace_bytes(THR_TEXT_MAX_TEXTS + 1) == 0 && thr_query_terms_workspace_bytes(THR_TEXT_MAX_TEXTS) > 0);
    Query qok;
    EXPECT(call(qok) == THR_ERR_WORKSPACE);
    Query q;
    q = qok; q.n_queries = 0;                           EXPECT(call(q) == THR_ERR_UNSUPPORTED);
    q = qok; q.n_queries = THR_TEXT_MAX_TEXTS + 1;      EXPECT(call(q) == THR_ERR_UNSUPPORTED);
    q = qok; q.token_capacity = 0;                      EXPECT(call(q) == THR_ERR_UNSUPPORTED);
    q = qok; q.tok_term = nullptr;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_tokens = nullptr;   EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.text_flags = nullptr; EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_total = nullptr;    EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.out_terms = nullptr;  EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.n_distinct = nullptr; EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.out_flags = nullptr;  EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.workspace = nullptr;  EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.workspace = (void*)32770; q.workspace_bytes = 4096; EXPECT(call(q) == THR_ERR_INVALID);
    q = qok; q.workspace_bytes = 255; EXPECT(call(q) == THR_ERR_WORKSPACE);
    std::printf(failures ? "text host check: %d FAILED\n" : "text host check: ok\n", failures);
    return failures ? 1 : 0;
}
