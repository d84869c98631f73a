// Stand-alone host check of thr_csr_prune's argument checks and thr_csr_prune_workspace_bytes: built
// together with csrc/csr_prune.hip with the host side under AddressSanitizer + UBSan and run on the
// CPU (tests/test_graph_delete_host.py does both).  Every call below is refused on the host, before
// any launch: no device is needed and none is touched.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../include/thr_hip_graph.h"

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
    int64_t rows_a = 6, nnz_a = 8;
    const int32_t* ids_a = (const int32_t*)8192;
    const void* pay_a = (const void*)12288;
    const int32_t* row_remap = (const int32_t*)16384;
    int64_t rows_out = 4;
    const int32_t* id_remap = (const int32_t*)20480;
    int64_t n_ids = 6, id_base = 0;
    const int64_t* rowptr_b = (const int64_t*)24576;
    int64_t nnz_b = 3;
    const int32_t* ids_b = (const int32_t*)28672;
    int64_t* rowptr_out = (int64_t*)32768;
    int32_t* ids_out = (int32_t*)36864;
    void* pay_out = (void*)40960;
    int64_t out_capacity = 8;
    uint8_t* keep_out = (uint8_t*)45056;
    int64_t* nnz_out = (int64_t*)49152;
    int32_t* status_out = (int32_t*)53248;
    void* workspace = (void*)57344;
    size_t workspace_bytes = 0;      // too small for everything that gets that far
};

static int call(const Args& a) {
    return thr_csr_prune(a.rowptr_a, a.rows_a, a.nnz_a, a.ids_a, a.pay_a, a.row_remap, a.rows_out, a.id_remap, a.n_ids,
                         a.id_base, a.rowptr_b, a.nnz_b, a.ids_b, a.rowptr_out, a.ids_out, a.pay_out, a.out_capacity,
                         a.keep_out, a.nnz_out, a.status_out, a.workspace, a.workspace_bytes, nullptr);
}

int main() {
    EXPECT(thr_csr_prune_slice() == THR_CSR_PRUNE_SLICE);
    // the workspace: one 4-byte word per position of A, 12 bytes per slice of A, one total; each piece
    // rounded up to 256 bytes
    EXPECT(thr_csr_prune_workspace_bytes(10, 0) == 256);
    EXPECT(thr_csr_prune_workspace_bytes(0, 0) == 256);
    EXPECT(thr_csr_prune_workspace_bytes(10, 1) == 4 * 256);
    EXPECT(thr_csr_prune_workspace_bytes(1000000, THR_CSR_PRUNE_SLICE + 1) == 256 + 4352 + 256 + 256);
    const int64_t big = (int64_t)1 << 30;
    EXPECT(thr_csr_prune_workspace_bytes(10, big) >= (size_t)big * 4 + (size_t)(big / THR_CSR_PRUNE_SLICE) * 12);
    EXPECT(thr_csr_prune_workspace_bytes(-1, 0) == 0 && thr_csr_prune_workspace_bytes(1, -1) == 0);
    EXPECT(thr_csr_prune_workspace_bytes(1, INT64_MAX) == 0 && thr_csr_prune_workspace_bytes(INT64_MAX, 0) == 0);

    Args ok;
    EXPECT(call(ok) == THR_ERR_WORKSPACE);      // every argument check passed: only the workspace is short
    Args a;
    a = ok; a.rowptr_out = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_out = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.status_out = nullptr; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.rowptr_a = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_a = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_out = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.id_remap = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);     // n_ids > 0 without a remap
    a = ok; a.ids_b = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);     // nnz_b > 0 without ids
    a = ok; a.rowptr_b = nullptr;   EXPECT(call(a) == THR_ERR_INVALID);     // B's ids without its row pointers
    a = ok; a.rowptr_b = nullptr; a.nnz_b = 0; EXPECT(call(a) == THR_ERR_INVALID);   // ... even with none to read
    a = ok; a.rows_a = -1;          EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_a = -1;           EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_b = -2;           EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.n_ids = -1;           EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.id_base = -1;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.rows_out = -1;        EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.rows_out = 7;         EXPECT(call(a) == THR_ERR_INVALID);     // more rows than A has
    a = ok; a.out_capacity = -1;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.nnz_a = INT64_MAX;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.row_remap = nullptr;  EXPECT(call(a) == THR_ERR_INVALID);     // no row leaves: rows_out == rows_a
    a = ok; a.row_remap = nullptr; a.rows_out = 6; EXPECT(call(a) == THR_ERR_WORKSPACE);
    a = ok; a.pay_a = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);     // a payload on one side only
    a = ok; a.pay_out = nullptr;    EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_a = nullptr; a.pay_out = nullptr; EXPECT(call(a) == THR_ERR_WORKSPACE);   // none: fine
    a = ok; a.id_remap = nullptr; a.n_ids = 0;      EXPECT(call(a) == THR_ERR_WORKSPACE);   // ids pass through
    a = ok; a.rowptr_b = nullptr; a.ids_b = nullptr; a.nnz_b = 0; EXPECT(call(a) == THR_ERR_WORKSPACE);   // no B
    a = ok; a.keep_out = nullptr;   EXPECT(call(a) == THR_ERR_WORKSPACE);   // optional
    a = ok; a.rows_a = 0; a.rows_out = 0;           EXPECT(call(a) == THR_ERR_INVALID);     // entries without rows
    a = ok; a.rows_a = 0; a.rows_out = 0; a.nnz_a = 0; a.nnz_b = 0; a.rowptr_a = nullptr; a.ids_a = nullptr;
    EXPECT(call(a) == THR_ERR_WORKSPACE);                                    // an empty A: fine
    a = ok; a.rowptr_out = (int64_t*)ok.rowptr_a;   EXPECT(call(a) == THR_ERR_INVALID);     // out of place only
    a = ok; a.rowptr_out = (int64_t*)ok.rowptr_b;   EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_out = (int32_t*)ok.ids_a;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_out = (int32_t*)ok.ids_b;         EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_out = (int32_t*)ok.row_remap;     EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.ids_out = (int32_t*)ok.id_remap;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_out = (void*)ok.pay_a;            EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.pay_out = (void*)ok.ids_out;          EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.keep_out = (uint8_t*)ok.ids_a;        EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.keep_out = (uint8_t*)ok.ids_out;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = (size_t)1 << 20; a.workspace = nullptr;      EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = (size_t)1 << 20; a.workspace = (void*)57348; EXPECT(call(a) == THR_ERR_INVALID);
    a = ok; a.workspace_bytes = thr_csr_prune_workspace_bytes(ok.rows_a, ok.nnz_a) - 1;
    EXPECT(call(a) == THR_ERR_WORKSPACE);
    std::printf(failures ? "csr_prune host check: %d FAILED\n" : "csr_prune host check: ok\n", failures);
    return failures ? 1 : 0;
}
