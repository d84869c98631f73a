// Graph delete on the device: one order-preserving pass over a CSR that drops rows, entries by id
// and (row, id) pairs, and renumbers what survives.
//
// Stands where the reference's store deletes by cascade: rag_entities.document_id,
// rag_entity_mentions.entity_id, rag_relations.subject_entity_id / object_entity_id and
// rag_relations.document_id are ON DELETE CASCADE (database/migrations/20260114_rag2_schema.sql:187,
// 217-220, 254, 258-259), so a deleted document takes the entities first extracted from it, every
// relation that touches them and every mention of them.  thr_csr_compact drops entries by id only
// (a deleted chunk leaves every list it was in); here rows leave as well (a deleted entity is a row
// of both graph CSRs and an id of the entity CSR), and single (row, id) pairs -- one edge, one
// mention -- named by a second CSR B over the same rows.
//
//     t(p)           = the row of position p                                               p in A
//     keep(p)        = (row_remap == NULL || 0 <= row_remap[t(p)] < rows_out)
//                      && (id_remap == NULL || (0 <= ids_a[p] - id_base < n_ids && id_remap[ids_a[p] - id_base] >= 0))
//                      && ids_a[p] is not in B's row t(p)
//     rank(p)        = number of kept positions before p
//     ids_out[rank(p)] = id_remap ? id_remap[ids_a[p] - id_base] + id_base : ids_a[p],  pay_out[rank(p)] = pay_a[p]
//     rowptr_out[row_remap[t]] = rank(rowptr_a[t])   for a surviving t,   rowptr_out[rows_out] = rank(nnz_a)
//
// The entries of a removed row are not kept, so the rank at the start of the next surviving row is
// the rank at the end of the last one: the survivors' row pointers are the ranks at their old
// starts.  Work is cut by POSITION of A, not by row (csr_merge.hip's shape: a star entity of
// thousands of mentions next to runs of empty rows): a thread finds the row of its first position by
// binary search in the row pointer and searches again only when a position leaves that row.  Three
// plain launches, no workgroup waits for another, no host round trip:
//   1. csr_prune_count    a workgroup owns CP_SLICE consecutive positions of A (keep flags, their
//                         prefix inside the slice into the workspace, the slice's count) or of B (the
//                         ordering precondition: an entry against its predecessor in the row);
//   2. csr_prune_scan     one workgroup: exclusive scan of the slice counts -> slice bases, the kept
//                         total, *nnz_out, the capacity bit of *status_out;
//   3. csr_prune_scatter  a workgroup owns CP_SLICE positions of A or CP_SLICE row pointers.
// Every source index is clamped to nnz_a / nnz_b before it is used, every remap index is checked
// against its length and every destination against out_capacity / rows_out: row pointers, remaps or
// ids that break the contract cannot make a kernel leave its buffers or write behind *nnz_out.
#include "thr_common.hpp"

#include "../../include/thr_hip_graph.h"

namespace thr {

constexpr int CP_THREADS = 256;
constexpr int CP_PER = 4;                           // consecutive positions per thread
constexpr int CP_SLICE = CP_THREADS * CP_PER;       // positions per workgroup
static_assert(CP_SLICE == THR_CSR_PRUNE_SLICE, "thr_hip_graph.h names the slice length");

__device__ __forceinline__ int64_t cp_clamp(int64_t v, int64_t lo, int64_t hi) {
    return v < lo ? lo : (v > hi ? hi : v);
}

// Row of position p: the last t in [0, rows) with rowptr[t] <= p (rows >= 1; empty rows are stepped over).
__device__ __forceinline__ int64_t cp_row_of(const int64_t* __restrict__ rowptr, int64_t rows, int64_t p) {
    int64_t lo = 1, hi = rows;     // first i in [1, rows] with rowptr[i] > p, or rows
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (rowptr[m] > p) hi = m; else lo = m + 1;
    }
    return lo - 1;
}

// The row of the positions a thread walks: searched at the first one and when a position leaves it.
struct CpRow {
    int64_t t = -1, end = -1;      // the row, and the first position behind it
    __device__ __forceinline__ int64_t at(const int64_t* __restrict__ rowptr, int64_t rows, int64_t p) {
        if (t < 0 || p >= end) {
            t = cp_row_of(rowptr, rows, p);
            end = t + 1 < rows ? rowptr[t + 1] : INT64_MAX;    // (the last row takes what is left)
        }
        return t;
    }
};

// Does the row survive, with a destination inside rowptr_out?
__device__ __forceinline__ bool cp_row_kept(const int32_t* __restrict__ row_remap, int64_t rows_out, int64_t t) {
    if (!row_remap) return t < rows_out;
    const int32_t r = row_remap[t];
    return r >= 0 && (int64_t)r < rows_out;
}

// Is v in [lo, hi) of the strictly ascending ids?
__device__ __forceinline__ bool cp_holds(const int32_t* __restrict__ ids, int64_t lo, const int64_t end, int32_t v) {
    int64_t hi = end;
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (ids[m] < v) lo = m + 1; else hi = m;
    }
    return lo < end && ids[lo] == v;
}

// Kept positions of A before p (p in [0, nnz_a]).  loc[p] = (kept before p inside its slice) << 1 | keep(p).
__device__ __forceinline__ int64_t cp_kept_before(const uint32_t* __restrict__ loc,
                                                  const int64_t* __restrict__ slice_base,
                                                  const int64_t* __restrict__ total, int64_t nnz_a, int64_t p) {
    if (p >= nnz_a) return *total;
    return slice_base[p / CP_SLICE] + (int64_t)(loc[p] >> 1);
}

__global__ __launch_bounds__(CP_THREADS) void csr_prune_count(
    const int64_t* __restrict__ rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t* __restrict__ ids_a,
    const int32_t* __restrict__ row_remap, int64_t rows_out, const int32_t* __restrict__ id_remap, int64_t n_ids,
    int64_t id_base, const int64_t* __restrict__ rowptr_b, int64_t nnz_b, const int32_t* __restrict__ ids_b,
    int64_t slices_a, uint32_t* __restrict__ loc, int32_t* __restrict__ slice_count,
    int32_t* __restrict__ status_out) {
    __shared__ int s_scan[CP_THREADS];
    if ((int64_t)blockIdx.x >= slices_a) {      // (workgroup-uniform) a slice of B: the precondition only
        const int64_t q0 = ((int64_t)blockIdx.x - slices_a) * CP_SLICE + (int64_t)threadIdx.x * CP_PER;
        bool bad = false;
        CpRow row;
        for (int e = 0; e < CP_PER; ++e) {
            const int64_t q = q0 + e;
            if (q >= nnz_b) break;
            const int64_t t = row.at(rowptr_b, rows_a, q);
            if (!cp_row_kept(row_remap, rows_out, t)) continue;       // (B under a removed row: ignored)
            if (q > cp_clamp(rowptr_b[t], 0, nnz_b)) bad |= ids_b[q - 1] >= ids_b[q];
        }
        if (bad) atomicOr(status_out, THR_CSR_PRUNE_UNSORTED_B);
        return;
    }
    const int64_t p0 = (int64_t)blockIdx.x * CP_SLICE + (int64_t)threadIdx.x * CP_PER;
    uint32_t flags = 0;
    CpRow row;
    for (int e = 0; e < CP_PER; ++e) {
        const int64_t p = p0 + e;
        if (p >= nnz_a) break;
        const int64_t t = row.at(rowptr_a, rows_a, p);
        bool keep = cp_row_kept(row_remap, rows_out, t);
        const int32_t v = ids_a[p];
        if (keep && id_remap) {
            const int64_t i = (int64_t)v - id_base;
            keep = i >= 0 && i < n_ids && id_remap[i] >= 0;
        }
        if (keep && ids_b) {
            const int64_t lo = cp_clamp(rowptr_b[t], 0, nnz_b);
            const int64_t hi = cp_clamp(rowptr_b[t + 1], lo, nnz_b);
            keep = !cp_holds(ids_b, lo, hi, v);
        }
        flags |= (keep ? 1u : 0u) << e;
    }
    const int mine = __popc(flags);
    s_scan[threadIdx.x] = mine;
    block_inclusive_scan<CP_THREADS>(s_scan);
    int before = s_scan[threadIdx.x] - mine;
    for (int e = 0; e < CP_PER; ++e) {
        const int64_t p = p0 + e;
        if (p >= nnz_a) break;
        loc[p] = ((uint32_t)before << 1) | (flags >> e & 1u);
        before += (int)(flags >> e & 1u);
    }
    if (threadIdx.x == CP_THREADS - 1) slice_count[blockIdx.x] = s_scan[CP_THREADS - 1];
}

// One workgroup: thread i sums a contiguous run of slices, the 256 sums are scanned through LDS, and
// the thread writes its run's exclusive bases (csr_compact_scan's shape).
__global__ __launch_bounds__(CP_THREADS) void csr_prune_scan(const int32_t* __restrict__ slice_count, int64_t n_slices,
                                                             int64_t* __restrict__ slice_base,
                                                             int64_t* __restrict__ total, int64_t out_capacity,
                                                             int64_t* __restrict__ nnz_out,
                                                             int32_t* __restrict__ status_out) {
    __shared__ int64_t s_sum[CP_THREADS];
    const int64_t per = (n_slices + CP_THREADS - 1) / CP_THREADS;
    const int64_t lo = per * threadIdx.x < n_slices ? per * threadIdx.x : n_slices;
    const int64_t hi = lo + per < n_slices ? lo + per : n_slices;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += slice_count[i];
    s_sum[threadIdx.x] = sum;
    block_inclusive_scan<CP_THREADS>(s_sum);
    int64_t run = s_sum[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        slice_base[i] = run;
        run += slice_count[i];
    }
    if (threadIdx.x == CP_THREADS - 1) {
        const int64_t kept = s_sum[CP_THREADS - 1];
        *total = kept;
        *nnz_out = kept;
        if (kept > out_capacity) atomicOr(status_out, THR_CSR_PRUNE_OVERFLOW);
    }
}

__global__ __launch_bounds__(CP_THREADS) void csr_prune_scatter(
    const int64_t* __restrict__ rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t* __restrict__ ids_a,
    const uint32_t* __restrict__ pay_a, const int32_t* __restrict__ row_remap, int64_t rows_out,
    const int32_t* __restrict__ id_remap, int64_t n_ids, int64_t id_base, int64_t slices_a,
    const uint32_t* __restrict__ loc, const int64_t* __restrict__ slice_base, const int64_t* __restrict__ total,
    int64_t* __restrict__ rowptr_out, int32_t* __restrict__ ids_out, uint32_t* __restrict__ pay_out,
    int64_t out_capacity, uint8_t* __restrict__ keep_out, int32_t* __restrict__ status_out) {
    const int64_t blk = blockIdx.x;
    if (blk < slices_a) {                        // the entries of A
        const int64_t p0 = blk * CP_SLICE + (int64_t)threadIdx.x * CP_PER;
        const int64_t base = slice_base[blk];
        for (int e = 0; e < CP_PER; ++e) {
            const int64_t p = p0 + e;
            if (p >= nnz_a) break;
            const uint32_t l = loc[p];
            if (keep_out) keep_out[p] = (uint8_t)(l & 1u);
            if (!(l & 1u)) continue;
            int32_t v = ids_a[p];
            if (id_remap) {
                const int64_t i = (int64_t)v - id_base;
                if (i < 0 || i >= n_ids) continue;       // (kept entries passed this check in the count)
                v = (int32_t)(id_remap[i] + id_base);
            }
            const int64_t dst = base + (int64_t)(l >> 1);
            if (dst >= 0 && dst < out_capacity) {
                ids_out[dst] = v;
                if (pay_out) pay_out[dst] = pay_a[p];
            }
        }
    } else {                                     // row pointers: t == rows_a is the end of the last row
        const int64_t t0 = (blk - slices_a) * CP_SLICE + (int64_t)threadIdx.x * CP_PER;
        for (int e = 0; e < CP_PER; ++e) {
            const int64_t t = t0 + e;
            if (t > rows_a) break;
            if (t == rows_a) {
                rowptr_out[rows_out] = *total;
                break;
            }
            int64_t r = t;
            if (row_remap) {
                r = row_remap[t];
                if (r >= rows_out) atomicOr(status_out, THR_CSR_PRUNE_BAD_ROW);
            }
            if (r < 0 || r >= rows_out) continue;
            rowptr_out[r] = cp_kept_before(loc, slice_base, total, nnz_a, cp_clamp(rowptr_a[t], 0, nnz_a));
        }
    }
}

}  // namespace thr

using namespace thr;

static int64_t prune_slices(int64_t n) { return (n + CP_SLICE - 1) / CP_SLICE; }

static void prune_plan(Arena& A, int64_t nnz_a, uint32_t** loc, int32_t** slice_count, int64_t** slice_base,
                       int64_t** total) {
    const size_t n_slices = (size_t)prune_slices(nnz_a);
    *total = A.take<int64_t>(1);
    *loc = A.take<uint32_t>((size_t)nnz_a);
    *slice_count = A.take<int32_t>(n_slices);
    *slice_base = A.take<int64_t>(n_slices);
}

static bool prune_sizes_ok(int64_t rows_a, int64_t nnz_a) {
    const int64_t max_nnz = (int64_t)1 << 38, max_rows = ((int64_t)1 << 31) - 2;
    return rows_a >= 0 && rows_a <= max_rows && nnz_a >= 0 && nnz_a <= max_nnz;
}

extern "C" int thr_csr_prune_slice(void) { return CP_SLICE; }

extern "C" size_t thr_csr_prune_workspace_bytes(int64_t rows_a, int64_t nnz_a) {
    if (!prune_sizes_ok(rows_a, nnz_a)) return 0;
    Arena A;
    uint32_t* l;
    int32_t* c;
    int64_t *b, *t;
    prune_plan(A, nnz_a, &l, &c, &b, &t);
    return A.total;
}

extern "C" int thr_csr_prune(const int64_t* rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t* ids_a,
                             const void* pay_a, const int32_t* row_remap, int64_t rows_out, const int32_t* id_remap,
                             int64_t n_ids, int64_t id_base, const int64_t* rowptr_b, int64_t nnz_b,
                             const int32_t* ids_b, int64_t* rowptr_out, int32_t* ids_out, void* pay_out,
                             int64_t out_capacity, uint8_t* keep_out, int64_t* nnz_out, int32_t* status_out,
                             void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    const int64_t max_id = ((int64_t)1 << 31) - 1;
    THR_RETURN_IF(!rowptr_out || !nnz_out || !status_out, THR_ERR_INVALID);
    THR_RETURN_IF(!prune_sizes_ok(rows_a, nnz_a) || out_capacity < 0 || nnz_b < 0 || nnz_b > ((int64_t)1 << 38),
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_ids < 0 || n_ids > max_id || id_base < 0 || id_base > max_id, THR_ERR_INVALID);
    THR_RETURN_IF(rows_out < 0 || rows_out > rows_a || (!row_remap && rows_out != rows_a), THR_ERR_INVALID);
    THR_RETURN_IF(rows_a > 0 && !rowptr_a, THR_ERR_INVALID);
    THR_RETURN_IF(rows_a == 0 && (nnz_a != 0 || nnz_b != 0), THR_ERR_INVALID);
    THR_RETURN_IF(nnz_a > 0 && !ids_a, THR_ERR_INVALID);
    THR_RETURN_IF(n_ids > 0 && !id_remap, THR_ERR_INVALID);
    // B: its ids come with its row pointers, and with A's rows
    THR_RETURN_IF((nnz_b > 0 && (!ids_b || !rowptr_b)) || (ids_b && !rowptr_b), THR_ERR_INVALID);
    THR_RETURN_IF(out_capacity > 0 && nnz_a > 0 && !ids_out, THR_ERR_INVALID);
    // a payload travels into the result, or there is none
    THR_RETURN_IF((pay_a != nullptr) != (pay_out != nullptr), THR_ERR_INVALID);
    // out of place: the destinations are buffers of their own
    THR_RETURN_IF(rowptr_out == rowptr_a || rowptr_out == rowptr_b, THR_ERR_INVALID);
    THR_RETURN_IF(ids_out && (ids_out == ids_a || ids_out == ids_b || ids_out == row_remap || ids_out == id_remap ||
                              (const void*)ids_out == pay_out || (const void*)ids_out == pay_a), THR_ERR_INVALID);
    THR_RETURN_IF(pay_out && (pay_out == pay_a || pay_out == (const void*)ids_a), THR_ERR_INVALID);
    THR_RETURN_IF(keep_out && ((const void*)keep_out == (const void*)ids_a || (const void*)keep_out == pay_a ||
                               (void*)keep_out == (void*)ids_out || (void*)keep_out == pay_out), THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_csr_prune_workspace_bytes(rows_a, nnz_a), THR_ERR_WORKSPACE);
    THR_RETURN_IF(!workspace || ((uintptr_t)workspace & 7) != 0, THR_ERR_INVALID);
    clear_status();
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    uint32_t* loc;
    int32_t* slice_count;
    int64_t *slice_base, *total;
    prune_plan(A, nnz_a, &loc, &slice_count, &slice_base, &total);
    const bool with_b = nnz_b > 0;     // (an empty B drops nothing)
    const int64_t slices_a = prune_slices(nnz_a), slices_b = with_b ? prune_slices(nnz_b) : 0;
    const int64_t slices_r = prune_slices(rows_a + 1);
    hipError_t e = hipMemsetAsync(status_out, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    int rc;
    if (slices_a + slices_b > 0) {
        hipLaunchKernelGGL(csr_prune_count, dim3((unsigned)(slices_a + slices_b)), dim3(CP_THREADS), 0, st, rowptr_a,
                           rows_a, nnz_a, ids_a, row_remap, rows_out, id_remap, n_ids, id_base, rowptr_b, nnz_b,
                           with_b ? ids_b : nullptr, slices_a, loc, slice_count, status_out);
        rc = launch_status();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(csr_prune_scan, dim3(1), dim3(CP_THREADS), 0, st, slice_count, slices_a, slice_base, total,
                       out_capacity, nnz_out, status_out);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(csr_prune_scatter, dim3((unsigned)(slices_a + slices_r)), dim3(CP_THREADS), 0, st, rowptr_a,
                       rows_a, nnz_a, ids_a, (const uint32_t*)pay_a, row_remap, rows_out, id_remap, n_ids, id_base,
                       slices_a, loc, slice_base, total, rowptr_out, ids_out, (uint32_t*)pay_out, out_capacity, keep_out,
                       status_out);
    return launch_status();
}
