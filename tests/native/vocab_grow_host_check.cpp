// Stand-alone host check of the argument checks and the size function of thr_vocab_grow: built together with
// csrc/vocab_grow.hip with the host side under AddressSanitizer + UBSan and run on the CPU
// (tests/test_vocab_grow_host.py does both).  Every call below is refused on the host, before any launch: no
// device is needed and none is touched.
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

struct Grow {
    // non-null, aligned pointer values that are never dereferenced on the host
    const uint8_t* text_bytes = (const uint8_t*)4096;
    const int64_t* text_ptr = (const int64_t*)8192;
    int64_t n_texts = 3, n_bytes = 100;
    const uint32_t* table = (const uint32_t*)12288;
    const int32_t* flags = (const int32_t*)16384;
    const int64_t* unknown_off = (const int64_t*)20480;
    const int32_t* unknown_len = (const int32_t*)24576;
    const int32_t* n_unknown = (const int32_t*)28672;
    int64_t unknown_capacity = 52, n_vocab = 512;
    uint64_t hash_mask = ~(uint64_t)0;
    int32_t* tok_term = (int32_t*)32768;
    const int32_t* n_total = (const int32_t*)36864;
    int64_t token_capacity = 52;
    int32_t* unknown_term = (int32_t*)40960;
    uint8_t* new_bytes = (uint8_t*)45057;                  // (bytes: no alignment asked)
    int64_t new_bytes_capacity = 1000;
    int64_t* new_ptr = (int64_t*)49152;
    int32_t* n_new = (int32_t*)53248;
    int64_t* n_new_bytes = (int64_t*)57344;
    int32_t* status = (int32_t*)61440;
    void* workspace = (void*)65536;
    size_t workspace_bytes = 0;      // too small for everything that gets that far
};

static int call(const Grow& a) {
    return thr_vocab_grow(a.text_bytes, a.text_ptr, a.n_texts, a.n_bytes, a.table, a.flags, a.unknown_off, a.unknown_len,
                          a.n_unknown, a.unknown_capacity, a.n_vocab, a.hash_mask, a.tok_term, a.n_total, a.token_capacity,
                          a.unknown_term, a.new_bytes, a.new_bytes_capacity, a.new_ptr, a.n_new, a.n_new_bytes, a.status,
                          a.workspace, a.workspace_bytes, nullptr);
}

int main() {
    EXPECT(THR_VOCAB_GROW_COLLISION == 1 && THR_VOCAB_GROW_OVERFLOW == 2);
    // the workspace: 16 bytes per slot of the smallest power of two >= 2 * capacity (at least 16), 4 + 4 + 4 + 8
    // bytes per entry (+ 1 for the two scans), 16385 int32 of the tok_term patch; each piece rounded up to 256
    EXPECT(thr_vocab_grow_workspace_bytes(1) == 256 + 4 * 256 + 65792);
    EXPECT(thr_vocab_grow_workspace_bytes(52) == 128 * 16 + 3 * 256 + 512 + 65792);
    EXPECT(thr_vocab_grow_workspace_bytes(512) == 1024 * 16 + 2048 + 2048 + 2304 + 4352 + 65792);
    EXPECT(thr_vocab_grow_workspace_bytes(513) > 2048 * 16);
    EXPECT(thr_vocab_grow_workspace_bytes(THR_TEXT_MAX_BYTES) > ((size_t)1 << 36));
    EXPECT(thr_vocab_grow_workspace_bytes(0) == 0 && thr_vocab_grow_workspace_bytes(-1) == 0);
    EXPECT(thr_vocab_grow_workspace_bytes((int64_t)THR_TEXT_MAX_BYTES + 1) == 0 && thr_vocab_grow_workspace_bytes(INT64_MAX) == 0);

    Grow ok;
    EXPECT(call(ok) == THR_ERR_WORKSPACE);      // every argument check passed: only the workspace is short
    Grow a;
    a = ok; a.n_texts = 0;                               EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_texts = THR_TEXT_MAX_TEXTS + 1;          EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_texts = THR_TEXT_MAX_TEXTS;              EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.n_bytes = -1;                              EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_bytes = (int64_t)THR_TEXT_MAX_BYTES + 1; EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_bytes = 0;                               EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.unknown_capacity = 0;                      EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.unknown_capacity = -7;                     EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.unknown_capacity = (int64_t)THR_TEXT_MAX_BYTES + 1; EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.unknown_capacity = INT64_MAX;              EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.token_capacity = 0;                        EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.token_capacity = (int64_t)THR_TEXT_MAX_BYTES + 1; EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.tok_term = nullptr; a.token_capacity = 0; a.n_total = nullptr; EXPECT(call(a) == THR_ERR_WORKSPACE);   // no patch asked
    a = ok; a.n_total = nullptr;       EXPECT(call(a) == THR_ERR_INVALID);      // a patch without its row count
    a = ok; a.text_bytes = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.text_ptr = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.table = nullptr;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.flags = nullptr;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_off = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_len = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_unknown = nullptr;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_term = nullptr;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.new_bytes = nullptr;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.new_ptr = nullptr;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_new = nullptr;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_new_bytes = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.status = nullptr;        EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace = nullptr;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_vocab = -1;            EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_vocab = 0;             EXPECT(call(a) == THR_ERR_WORKSPACE);    // an empty vocabulary: fine
    a = ok; a.n_vocab = (int64_t)INT32_MAX - 52;     EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.n_vocab = (int64_t)INT32_MAX - 51;     EXPECT(call(a) == THR_ERR_INVALID);    // ids past int32
    a = ok; a.n_vocab = INT64_MAX;                   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.hash_mask = 0;                         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.hash_mask = 7;                         EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.new_bytes_capacity = -1;               EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.new_bytes_capacity = 0;                EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.text_bytes = (const uint8_t*)4104;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.text_ptr = (const int64_t*)8196;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.unknown_off = (const int64_t*)20484;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.new_ptr = (int64_t*)49156;             EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_new_bytes = (int64_t*)57348;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.table = (const uint32_t*)12290;        EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace = (void*)65544; a.workspace_bytes = (size_t)1 << 20;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = thr_vocab_grow_workspace_bytes(ok.unknown_capacity) - 1;
    EXPECT(call(a) == THR_ERR_WORKSPACE);
    std::printf(failures ? "vocab grow host check: %d FAILED\n" : "vocab grow host check: ok\n", failures);
    return failures ? 1 : 0;
}
