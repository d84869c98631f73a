// Stand-alone host check of thr_csr_merge's argument checks and thr_csr_merge_workspace_bytes: built
// together with csrc/csr_merge.hip with the host side under AddressSanitizer + UBSan and run on the
// CPU (tests/test_graph_ingest_host.py does both).  Every call below is refused on the host, before
// any launch: no device is needed and none is touched.
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

struct Args {
    // non-null, aligned pointer values that are never dereferenced on the host
    const int64_t* rowptr_a = (const int64_t*)4096;
    int64_t rows_a = 4, nnz_a = 8;
    const int32_t* ids_a = (const int32_t*)8192;
    const void* pay_a = (const void*)12288;
    const int64_t* rowptr_b = (const int64_t*)16384;
    int64_t rows_b = 6, nnz_b = 3;
    const int32_t* ids_b = (const int32_t*)20480;
    const void* pay_b = (const void*)24576;
    int drop_present = 0;
    int64_t* rowptr_out = (int64_t*)28672;
    int32_t* ids_out = (int32_t*)32768;
    void* pay_out = (void*)36864;
    int64_t out_capacity = 11;
    int64_t* nnz_out = (int64_t*)40960;
    int32_t* status_out = (int32_t*)45056;
    void* workspace = (void*)49152;
    size_t workspace_bytes = 0;      // too small for everything that gets that far
};

static int call(const Args& a) {
    return thr_csr_merge(a.rowptr_a, a.rows_a, a.nnz_a, a.ids_a, a.pay_a, a.rowptr_b, a.rows_b, a.nnz_b, a.ids_b,
                         a.pay_b, a.drop_present, a.rowptr_out, a.ids_out, a.pay_out, a.out_capacity, a.nnz_out,
                         a.status_out, a.workspace, a.workspace_bytes, nullptr);
}

int main() {
    EXPECT(thr_csr_merge_slice() == THR_CSR_MERGE_SLICE);
    // the workspace: one 4-byte word per position of B, 12 bytes per slice of B, one total; each
    // piece rounded up to 256 bytes
    EXPECT(thr_csr_merge_workspace_bytes(10, 0, 0) == 256);
    EXPECT(thr_csr_merge_workspace_bytes(10, 1000000, 1) == 4 * 256);
    EXPECT(thr_csr_merge_workspace_bytes(10, 5, THR_CSR_MERGE_SLICE + 1) == 256 + 4352 + 256 + 256);
    const int64_t big = (int64_t)1 << 30;
    EXPECT(thr_csr_merge_workspace_bytes(10, 0, big) >= (size_t)big * 4 + (size_t)(big / THR_CSR_MERGE_SLICE) * 12);
    EXPECT(thr_csr_merge_workspace_bytes(-1, 0, 0) == 0 && thr_csr_merge_workspace_bytes(1, -1, 0) == 0);
    EXPECT(thr_csr_merge_workspace_bytes(1, 0, -1) == 0 && thr_csr_merge_workspace_bytes(1, 0, INT64_MAX) == 0);
    EXPECT(thr_csr_merge_workspace_bytes(INT64_MAX, 0, 0) == 0);

    Args ok;
    EXPECT(call(ok) == THR_ERR_WORKSPACE);      // every argument check passed: only the workspace is short
    Args a;
    a = ok; a.rowptr_b = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.rowptr_out = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_out = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.status_out = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.rowptr_a = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_a = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_b = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_out = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.rows_b = 3;           EXPECT(call(a) == THR_ERR_INVALID);     // rows_b < rows_a
    a = ok; a.rows_a = -1;          EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_a = -1;           EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_b = -2;           EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.out_capacity = -1;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_a = INT64_MAX;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.drop_present = 2;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_a = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);     // a payload on one side only
    a = ok; a.pay_b = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_out = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_a = a.pay_b = nullptr; EXPECT(call(a) == THR_ERR_INVALID);   // ... or on the result only
    a = ok; a.pay_a = a.pay_b = a.pay_out = nullptr; EXPECT(call(a) == THR_ERR_WORKSPACE);   // none: fine
    a = ok; a.rows_a = 0; a.rowptr_a = nullptr;              EXPECT(call(a) == THR_ERR_INVALID);   // entries without rows
    a = ok; a.rows_a = 0; a.rowptr_a = nullptr; a.nnz_a = 0; a.ids_a = nullptr; a.pay_a = nullptr;
    EXPECT(call(a) == THR_ERR_WORKSPACE);                                    // an empty A: fine
    a = ok; a.rows_a = 0; a.rows_b = 0; a.nnz_a = 0;         EXPECT(call(a) == THR_ERR_INVALID);   // B entries without rows
    a = ok; a.rowptr_out = (int64_t*)ok.rowptr_b;            EXPECT(call(a) == THR_ERR_INVALID);   // out of place only
    a = ok; a.ids_out = (int32_t*)ok.ids_a;                  EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_out = (void*)ok.pay_b;                     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_out = (void*)ok.ids_out;                   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = (size_t)1 << 20; a.workspace = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = (size_t)1 << 20; a.workspace = (void*)49156; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = thr_csr_merge_workspace_bytes(ok.rows_b, ok.nnz_a, ok.nnz_b) - 1;
    EXPECT(call(a) == THR_ERR_WORKSPACE);
    std::printf(failures ? "csr_merge host check: %d FAILED\n" : "csr_merge host check: ok\n", failures);
    return failures ? 1 : 0;
}
