// Stand-alone host check of the argument checks and the size function of thr_text_tokens_analyzed: built
// together with csrc/text.hip with the host side under AddressSanitizer + UBSan and run on the CPU
// (tests/test_text_analyzer_host.py does both).  Every call below is refused on the host, before any launch:
// no device is needed and none is touched.  The step pointers are host memory and ARE read.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/thr_hip_text.h"

static int failures = 0;

#define EXPECT(cond)                                               \
    do {                                                           \
        if (!(cond)) {                                             \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);  \
            ++failures;                                            \
        }                                                          \
    } while (0)

static const int32_t STEPS_OK[3] = {0, 3, 10};

struct Args {
    // non-null, aligned pointer values that are never dereferenced on the host
    const uint8_t* text_bytes = (const uint8_t*)4096;
    const int64_t* text_ptr = (const int64_t*)8192;
    int64_t n_texts = 3, n_bytes = 100;
    const uint32_t* table = (const uint32_t*)12288;
    const void* slots = (const void*)16384;
    int64_t capacity = 1024;
    const uint8_t* term_bytes = (const uint8_t*)20481;
    const int64_t* term_ptr = (const int64_t*)24576;
    int64_t n_vocab = 512;
    const void* stop_slots = (const void*)65536;
    int64_t stop_capacity = 64;
    const uint8_t* stop_bytes = (const uint8_t*)69633;
    const int64_t* stop_ptr = (const int64_t*)73728;
    int64_t n_stop = 20;
    const int32_t* h_step_ptr = STEPS_OK;       // host memory: read by the call
    int n_steps = 2;
    const void* rules = (const void*)77824;
    int64_t token_capacity = 52;
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

static int call(const Args& a) {
    return thr_text_tokens_analyzed(a.text_bytes, a.text_ptr, a.n_texts, a.n_bytes, a.table, a.slots, a.capacity,
                                    a.term_bytes, a.term_ptr, a.n_vocab, a.stop_slots, a.stop_capacity, a.stop_bytes,
                                    a.stop_ptr, a.n_stop, a.h_step_ptr, a.n_steps, a.rules, a.token_capacity, a.tok_doc,
                                    a.tok_term, a.n_tokens, a.flags, a.n_total, a.unknown_off, a.unknown_len, a.n_unknown,
                                    a.workspace, a.workspace_bytes, nullptr);
}

int main() {
    EXPECT(THR_STEM_MAX_SUFFIX == 8 && THR_STEM_MAX_STEPS == 4 && THR_STEM_MAX_RULES == 1024 && THR_STEM_RULE_BYTES == 24);
    // the workspace is thr_text_tokens'
    EXPECT(thr_text_tokens_analyzed_workspace_bytes(3, 100, 52) == thr_text_tokens_workspace_bytes(3, 100, 52));
    EXPECT(thr_text_tokens_analyzed_workspace_bytes(3, 100, 52) == 256 + 256 + 512 + 256);
    EXPECT(thr_text_tokens_analyzed_workspace_bytes(0, 100, 52) == 0 && thr_text_tokens_analyzed_workspace_bytes(3, -1, 52) == 0);
    EXPECT(thr_text_tokens_analyzed_workspace_bytes(3, 100, 0) == 0);

    Args ok;
    EXPECT(call(ok) == THR_ERR_WORKSPACE);      // every argument check passed: only the workspace is short
    Args a;
    // ---- thr_text_tokens' refusals
    a = ok; a.n_texts = 0;                               EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_texts = THR_TEXT_MAX_TEXTS + 1;          EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_bytes = -1;                              EXPECT(call(a) == THR_ERR_UNSUPPORTED);
    a = ok; a.n_bytes = (int64_t)THR_TEXT_MAX_BYTES + 1; EXPECT(call(a) == THR_ERR_UNSUPPORTED);
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
    a = ok; a.capacity = 1000;       EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_vocab = 513;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.text_bytes = (const uint8_t*)4104;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.table = (const uint32_t*)12290;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace = (void*)61444; a.workspace_bytes = (size_t)1 << 20;  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = thr_text_tokens_analyzed_workspace_bytes(ok.n_texts, ok.n_bytes, ok.token_capacity) - 1;
    EXPECT(call(a) == THR_ERR_WORKSPACE);

    // ---- the rule table
    a = ok; a.n_steps = -1;                     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_steps = THR_STEM_MAX_STEPS + 1; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.h_step_ptr = nullptr;             EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.h_step_ptr = nullptr; a.n_steps = 0; a.rules = nullptr;   EXPECT(call(a) == THR_ERR_WORKSPACE);   // no rules at all
    const int32_t from_one[3] = {1, 3, 10}, descending[3] = {0, 5, 4}, too_many[3] = {0, 3, THR_STEM_MAX_RULES + 1};
    const int32_t full[5] = {0, 0, 1000, 1000, THR_STEM_MAX_RULES}, negative[3] = {0, -1, 4}, none[3] = {0, 0, 0};
    a = ok; a.h_step_ptr = from_one;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.h_step_ptr = descending; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.h_step_ptr = too_many;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.h_step_ptr = negative;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.h_step_ptr = full; a.n_steps = 4;    EXPECT(call(a) == THR_ERR_WORKSPACE);   // empty steps and the limit itself
    a = ok; a.rules = nullptr;                     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.rules = (const void*)77828;          EXPECT(call(a) == THR_ERR_INVALID);     // 8-byte aligned
    a = ok; a.h_step_ptr = none; a.rules = nullptr; EXPECT(call(a) == THR_ERR_WORKSPACE);  // steps without a rule

    // ---- the stop set
    a = ok; a.stop_capacity = 0; a.stop_slots = nullptr; a.stop_bytes = nullptr; a.stop_ptr = nullptr; a.n_stop = 0;
    EXPECT(call(a) == THR_ERR_WORKSPACE);                                                  // no stop list
    a = ok; a.stop_capacity = 0;                   EXPECT(call(a) == THR_ERR_INVALID);     // pointers without a capacity
    a = ok; a.stop_capacity = 0; a.stop_slots = nullptr; a.stop_bytes = nullptr; a.stop_ptr = nullptr;
    EXPECT(call(a) == THR_ERR_INVALID);                                                    // n_stop without a table
    a = ok; a.stop_slots = nullptr;                EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.stop_bytes = nullptr;                EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.stop_ptr = nullptr;                  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.stop_capacity = 60;                  EXPECT(call(a) == THR_ERR_INVALID);     // not a power of two
    a = ok; a.stop_capacity = 8;  a.n_stop = 2;    EXPECT(call(a) == THR_ERR_INVALID);     // below THR_VOCAB_MIN_SLOTS
    a = ok; a.n_stop = 33;                         EXPECT(call(a) == THR_ERR_INVALID);     // above 1/2 load
    a = ok; a.n_stop = -1;                         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_stop = 32;                         EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.stop_slots = (const void*)65544;     EXPECT(call(a) == THR_ERR_INVALID);     // 16-byte aligned
    a = ok; a.stop_ptr = (const int64_t*)73732;    EXPECT(call(a) == THR_ERR_INVALID);     // 8-byte aligned
    std::printf(failures ? "text analyzer host check: %d FAILED\n" : "text analyzer host check: ok\n", failures);
    return failures ? 1 : 0;
}
