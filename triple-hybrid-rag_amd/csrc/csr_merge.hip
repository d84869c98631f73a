// Graph ingest on the device: row-wise stable merge of two CSRs over one row space.
//
// Stands where the reference's entity extraction writes behind the chunks of a document that are
// already stored: it upserts rag_entities rows, inserts rag_relations and inserts rag_entity_mentions
// (src/voice_agent/rag2/entity_extraction.py:449-554).  thr_csr_append could concatenate because
// appended chunks carry the largest ids; here a new relation may join two old entities and land
// anywhere inside a sorted row, may be there already, and a new mention of an old chunk lands in the
// middle of its entity's chunk-ascending row.  So row t of the result is the MERGE of A's and B's row
// t by id -- on equal ids A's entries first, each side in its own order: what a stable sort gives a
// fresh build whose input lists the old rows before the new ones.
//
//     A = the index so far, B = the canonicalised batch, rows_b >= rows_a (rows >= rows_a empty in A)
//     drop_present = 1   set union (relations): a B entry whose id is in A's row is dropped
//     drop_present = 0   multiset merge (mentions + payload): nothing is dropped
//
//     keep(p)        = !drop_present || ids_b[p] is not in A's row of p                    p in B
//     kb(p)          = number of kept B positions before p
//     rowptr_out[t]  = rowptr_a[min(t, rows_a)] + kb(rowptr_b[t])
//     dst(kept p)    = rowptr_out[t] + (kb(p) - kb(rowptr_b[t])) + |{A entries of row t with id <= ids_b[p]}|
//                    = kb(p) + (first position of A's row t whose id is > ids_b[p])
//     dst(q in A)    = rowptr_out[t] + (q - rowptr_a[t]) + |{kept B entries of row t with id < ids_a[q]}|
//                    = q + kb(first position of B's row t whose id is >= ids_a[q])
//                      (with drop_present the B entries equal to ids_a[q] are dropped, without it they
//                       come behind: either way the kept ones in front are those below)
//
// Work is cut by POSITION, not by row (a star entity of thousands of edges next to a long tail of
// singletons): a thread finds the row of its position by binary search in the row pointer, its
// offset by a binary search inside the other side's row.  Three plain launches, no workgroup waits
// for another, no host round trip:
//   1. csr_merge_count    a workgroup owns CM_SLICE consecutive positions of B (keep flags, their
//                         prefix inside the slice into the workspace, the slice's count) or of A; both
//                         kinds verify the ordering precondition of the mode (an entry against its
//                         predecessor in the row) and report it in *status_out;
//   2. csr_merge_scan     one workgroup: exclusive scan of the slice counts -> slice bases, the kept
//                         total, *nnz_out, the capacity bit of *status_out;
//   3. csr_merge_scatter  a workgroup owns CM_SLICE positions of B, of A, or CM_SLICE row pointers.
// Every source index is clamped to nnz_a / nnz_b before it is used and every destination is checked
// against out_capacity; destinations lie below nnz_a + kept for any input, so row pointers or ids
// that break the contract cannot make a kernel leave its buffers or write behind *nnz_out.
#include "thr_common.hpp"

namespace thr {

constexpr int CM_THREADS = 256;
constexpr int CM_PER = 4;                           // consecutive positions per thread
constexpr int CM_SLICE = CM_THREADS * CM_PER;       // positions per workgroup
static_assert(CM_SLICE == THR_CSR_MERGE_SLICE, "thr_hip.h names the slice length");

__device__ __forceinline__ int64_t cm_clamp(int64_t v, int64_t lo, int64_t hi) {
    return v < lo ? lo : (v > hi ? hi : v);
}

// Row of position p: the last t in [0, rows) with rowptr[t] <= p (rows >= 1; empty rows are stepped over).
__device__ __forceinline__ int64_t cm_row_of(const int64_t* __restrict__ rowptr, int64_t rows, int64_t p) {
    int64_t lo = 1, hi = rows;     // first i in [1, rows] with rowptr[i] > p, or rows
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        if (rowptr[m] > p) hi = m; else lo = m + 1;
    }
    return lo - 1;
}

// [lo, hi) of row t, inside [0, nnz] whatever the row pointers hold; a row >= rows is empty at nnz.
__device__ __forceinline__ void cm_row_range(const int64_t* __restrict__ rowptr, int64_t rows, int64_t nnz, int64_t t,
                                             int64_t& lo, int64_t& hi) {
    if (t >= rows) {
        lo = hi = nnz;
        return;
    }
    lo = cm_clamp(rowptr[t], 0, nnz);
    hi = cm_clamp(rowptr[t + 1], lo, nnz);
}

// First position in [lo, hi) whose id is >= v (UPPER: > v), or hi.
template <bool UPPER>
__device__ __forceinline__ int64_t cm_bound(const int32_t* __restrict__ ids, int64_t lo, int64_t hi, int32_t v) {
    while (lo < hi) {
        const int64_t m = (lo + hi) >> 1;
        const int32_t x = ids[m];
        if (UPPER ? x <= v : x < v) lo = m + 1; else hi = m;
    }
    return lo;
}

// An entry against its predecessor inside the row: strictly ascending for the union, non-decreasing else.
__device__ __forceinline__ bool cm_out_of_order(const int32_t* __restrict__ ids, int64_t p, int64_t row_lo,
                                                int drop_present) {
    if (p <= row_lo) return false;
    const int32_t prev = ids[p - 1], cur = ids[p];
    return drop_present ? prev >= cur : prev > cur;
}

// Kept B positions before p (p in [0, nnz_b]).  loc[p] = (kept before p inside its slice) << 1 | keep(p).
__device__ __forceinline__ int64_t cm_kept_before(const uint32_t* __restrict__ loc,
                                                  const int64_t* __restrict__ slice_base,
                                                  const int64_t* __restrict__ total, int64_t nnz_b, int64_t p) {
    if (p >= nnz_b) return *total;
    return slice_base[p / CM_SLICE] + (int64_t)(loc[p] >> 1);
}

__global__ __launch_bounds__(CM_THREADS) void csr_merge_count(
    const int64_t* __restrict__ rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t* __restrict__ ids_a,
    const int64_t* __restrict__ rowptr_b, int64_t rows_b, int64_t nnz_b, const int32_t* __restrict__ ids_b,
    int drop_present, int64_t slices_b, uint32_t* __restrict__ loc, int32_t* __restrict__ slice_count,
    int32_t* __restrict__ status_out) {
    __shared__ int s_scan[CM_THREADS];
    if ((int64_t)blockIdx.x >= slices_b) {      // (workgroup-uniform) a slice of A: the precondition only
        const int64_t q0 = ((int64_t)blockIdx.x - slices_b) * CM_SLICE + (int64_t)threadIdx.x * CM_PER;
        bool bad = false;
        for (int e = 0; e < CM_PER; ++e) {
            const int64_t q = q0 + e;
            if (q >= nnz_a) break;
            const int64_t t = cm_row_of(rowptr_a, rows_a, q);
            bad |= cm_out_of_order(ids_a, q, cm_clamp(rowptr_a[t], 0, nnz_a), drop_present);
        }
        if (bad) atomicOr(status_out, THR_CSR_MERGE_UNSORTED_A);
        return;
    }
    const int64_t p0 = (int64_t)blockIdx.x * CM_SLICE + (int64_t)threadIdx.x * CM_PER;
    uint32_t flags = 0;
    bool bad = false;
    for (int e = 0; e < CM_PER; ++e) {
        const int64_t p = p0 + e;
        if (p >= nnz_b) break;
        const int64_t t = cm_row_of(rowptr_b, rows_b, p);
        bad |= cm_out_of_order(ids_b, p, cm_clamp(rowptr_b[t], 0, nnz_b), drop_present);
        bool keep = true;
        if (drop_present) {
            int64_t lo, hi;
            cm_row_range(rowptr_a, rows_a, nnz_a, t, lo, hi);
            const int32_t v = ids_b[p];
            const int64_t at = cm_bound<false>(ids_a, lo, hi, v);
            keep = !(at < hi && ids_a[at] == v);
        }
        flags |= (keep ? 1u : 0u) << e;
    }
    if (bad) atomicOr(status_out, THR_CSR_MERGE_UNSORTED_B);
    const int mine = __popc(flags);
    s_scan[threadIdx.x] = mine;
    block_inclusive_scan<CM_THREADS>(s_scan);
    int before = s_scan[threadIdx.x] - mine;
    for (int e = 0; e < CM_PER; ++e) {
        const int64_t p = p0 + e;
        if (p >= nnz_b) break;
        loc[p] = ((uint32_t)before << 1) | (flags >> e & 1u);
        before += (int)(flags >> e & 1u);
    }
    if (threadIdx.x == CM_THREADS - 1) slice_count[blockIdx.x] = s_scan[CM_THREADS - 1];
}

// One workgroup: thread i sums a contiguous run of slices, the 256 sums are scanned through LDS, and
// the thread writes its run's exclusive bases (csr_compact_scan's shape).
__global__ __launch_bounds__(CM_THREADS) void csr_merge_scan(const int32_t* __restrict__ slice_count, int64_t n_slices,
                                                             int64_t* __restrict__ slice_base,
                                                             int64_t* __restrict__ total, int64_t nnz_a,
                                                             int64_t out_capacity, int64_t* __restrict__ nnz_out,
                                                             int32_t* __restrict__ status_out) {
    __shared__ int64_t s_sum[CM_THREADS];
    const int64_t per = (n_slices + CM_THREADS - 1) / CM_THREADS;
    const int64_t lo = per * threadIdx.x < n_slices ? per * threadIdx.x : n_slices;
    const int64_t hi = lo + per < n_slices ? lo + per : n_slices;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += slice_count[i];
    s_sum[threadIdx.x] = sum;
    block_inclusive_scan<CM_THREADS>(s_sum);
    int64_t run = s_sum[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        slice_base[i] = run;
        run += slice_count[i];
    }
    if (threadIdx.x == CM_THREADS - 1) {
        const int64_t kept = s_sum[CM_THREADS - 1];
        *total = kept;
        *nnz_out = nnz_a + kept;
        if (nnz_a + kept > out_capacity) atomicOr(status_out, THR_CSR_MERGE_OVERFLOW);
    }
}

__global__ __launch_bounds__(CM_THREADS) void csr_merge_scatter(
    const int64_t* __restrict__ rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t* __restrict__ ids_a,
    const uint32_t* __restrict__ pay_a, const int64_t* __restrict__ rowptr_b, int64_t rows_b, int64_t nnz_b,
    const int32_t* __restrict__ ids_b, const uint32_t* __restrict__ pay_b, int64_t slices_a, int64_t slices_b,
    const uint32_t* __restrict__ loc, const int64_t* __restrict__ slice_base, const int64_t* __restrict__ total,
    int64_t* __restrict__ rowptr_out, int32_t* __restrict__ ids_out, uint32_t* __restrict__ pay_out,
    int64_t out_capacity) {
    const int64_t blk = blockIdx.x;
    if (blk < slices_b) {                        // kept entries of B
        const int64_t p0 = blk * CM_SLICE + (int64_t)threadIdx.x * CM_PER;
        for (int e = 0; e < CM_PER; ++e) {
            const int64_t p = p0 + e;
            if (p >= nnz_b) break;
            const uint32_t l = loc[p];
            if (!(l & 1u)) continue;
            const int64_t t = cm_row_of(rowptr_b, rows_b, p);
            int64_t lo, hi;
            cm_row_range(rowptr_a, rows_a, nnz_a, t, lo, hi);
            const int32_t v = ids_b[p];
            const int64_t dst = slice_base[blk] + (int64_t)(l >> 1) + cm_bound<true>(ids_a, lo, hi, v);
            if (dst >= 0 && dst < out_capacity) {
                ids_out[dst] = v;
                if (pay_out) pay_out[dst] = pay_b[p];
            }
        }
    } else if (blk < slices_b + slices_a) {      // every entry of A
        const int64_t q0 = (blk - slices_b) * CM_SLICE + (int64_t)threadIdx.x * CM_PER;
        for (int e = 0; e < CM_PER; ++e) {
            const int64_t q = q0 + e;
            if (q >= nnz_a) break;
            const int64_t t = cm_row_of(rowptr_a, rows_a, q);
            int64_t lo, hi;
            cm_row_range(rowptr_b, rows_b, nnz_b, t, lo, hi);
            const int32_t v = ids_a[q];
            const int64_t dst = q + cm_kept_before(loc, slice_base, total, nnz_b, cm_bound<false>(ids_b, lo, hi, v));
            if (dst >= 0 && dst < out_capacity) {
                ids_out[dst] = v;
                if (pay_out) pay_out[dst] = pay_a[q];
            }
        }
    } else {                                     // row pointers
        const int64_t t0 = (blk - slices_b - slices_a) * CM_SLICE + (int64_t)threadIdx.x * CM_PER;
        for (int e = 0; e < CM_PER; ++e) {
            const int64_t t = t0 + e;
            if (t > rows_b) break;
            const int64_t a = t < rows_a ? cm_clamp(rowptr_a[t], 0, nnz_a) : nnz_a;   // (rowptr_a[rows_a] == nnz_a)
            rowptr_out[t] = a + cm_kept_before(loc, slice_base, total, nnz_b, cm_clamp(rowptr_b[t], 0, nnz_b));
        }
    }
}

}  // namespace thr

using namespace thr;

static int64_t merge_slices(int64_t n) { return (n + CM_SLICE - 1) / CM_SLICE; }

static void merge_plan(Arena& A, int64_t nnz_b, uint32_t** loc, int32_t** slice_count, int64_t** slice_base,
                       int64_t** total) {
    const size_t n_slices = (size_t)merge_slices(nnz_b);
    *total = A.take<int64_t>(1);
    *loc = A.take<uint32_t>((size_t)nnz_b);
    *slice_count = A.take<int32_t>(n_slices);
    *slice_base = A.take<int64_t>(n_slices);
}

static bool merge_sizes_ok(int64_t rows_a, int64_t rows_b, int64_t nnz_a, int64_t nnz_b) {
    const int64_t max_nnz = (int64_t)1 << 38, max_rows = ((int64_t)1 << 31) - 2;
    return rows_a >= 0 && rows_b >= rows_a && rows_b <= max_rows && nnz_a >= 0 && nnz_b >= 0 && nnz_a <= max_nnz &&
           nnz_b <= max_nnz;
}

extern "C" int thr_csr_merge_slice(void) { return CM_SLICE; }

extern "C" size_t thr_csr_merge_workspace_bytes(int64_t rows_b, int64_t nnz_a, int64_t nnz_b) {
    if (!merge_sizes_ok(0, rows_b, nnz_a, nnz_b)) return 0;
    Arena A;
    uint32_t* l;
    int32_t* c;
    int64_t *b, *t;
    merge_plan(A, nnz_b, &l, &c, &b, &t);
    return A.total;
}

extern "C" int thr_csr_merge(const int64_t* rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t* ids_a,
                             const void* pay_a, const int64_t* rowptr_b, int64_t rows_b, int64_t nnz_b,
                             const int32_t* ids_b, const void* pay_b, int drop_present, int64_t* rowptr_out,
                             int32_t* ids_out, void* pay_out, int64_t out_capacity, int64_t* nnz_out,
                             int32_t* status_out, void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    THR_RETURN_IF(!rowptr_b || !rowptr_out || !nnz_out || !status_out, THR_ERR_INVALID);
    THR_RETURN_IF(!merge_sizes_ok(rows_a, rows_b, nnz_a, nnz_b) || out_capacity < 0, THR_ERR_INVALID);
    THR_RETURN_IF(drop_present != 0 && drop_present != 1, THR_ERR_INVALID);
    THR_RETURN_IF(rows_a > 0 && !rowptr_a, THR_ERR_INVALID);
    THR_RETURN_IF((rows_a == 0 && nnz_a != 0) || (rows_b == 0 && nnz_b != 0), THR_ERR_INVALID);
    THR_RETURN_IF((nnz_a > 0 && !ids_a) || (nnz_b > 0 && !ids_b), THR_ERR_INVALID);
    THR_RETURN_IF(out_capacity > 0 && nnz_a + nnz_b > 0 && !ids_out, THR_ERR_INVALID);
    // a payload travels on both sides and into the result, or on neither
    const bool two = pay_out != nullptr;
    THR_RETURN_IF((nnz_a > 0 && (pay_a != nullptr) != two) || (nnz_b > 0 && (pay_b != nullptr) != two), THR_ERR_INVALID);
    THR_RETURN_IF(nnz_a == 0 && nnz_b == 0 && ((pay_a != nullptr) != (pay_b != nullptr)), THR_ERR_INVALID);
    // out of place: the destinations are buffers of their own
    THR_RETURN_IF(rowptr_out == rowptr_a || rowptr_out == rowptr_b, THR_ERR_INVALID);
    THR_RETURN_IF(ids_out && (ids_out == ids_a || ids_out == ids_b || (const void*)ids_out == pay_out), THR_ERR_INVALID);
    THR_RETURN_IF(pay_out && (pay_out == pay_a || pay_out == pay_b), THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_csr_merge_workspace_bytes(rows_b, nnz_a, nnz_b), THR_ERR_WORKSPACE);
    THR_RETURN_IF(!workspace || ((uintptr_t)workspace & 7) != 0, THR_ERR_INVALID);
    clear_status();
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    uint32_t* loc;
    int32_t* slice_count;
    int64_t *slice_base, *total;
    merge_plan(A, nnz_b, &loc, &slice_count, &slice_base, &total);
    const int64_t slices_a = merge_slices(nnz_a), slices_b = merge_slices(nnz_b);
    const int64_t slices_r = merge_slices(rows_b + 1);
    hipError_t e = hipMemsetAsync(status_out, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    int rc;
    if (slices_a + slices_b > 0) {
        hipLaunchKernelGGL(csr_merge_count, dim3((unsigned)(slices_b + slices_a)), dim3(CM_THREADS), 0, st, rowptr_a,
                           rows_a, nnz_a, ids_a, rowptr_b, rows_b, nnz_b, ids_b, drop_present, slices_b, loc,
                           slice_count, status_out);
        rc = launch_status();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(csr_merge_scan, dim3(1), dim3(CM_THREADS), 0, st, slice_count, slices_b, slice_base, total,
                       nnz_a, out_capacity, nnz_out, status_out);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(csr_merge_scatter, dim3((unsigned)(slices_b + slices_a + slices_r)), dim3(CM_THREADS), 0, st,
                       rowptr_a, rows_a, nnz_a, ids_a, (const uint32_t*)pay_a, rowptr_b, rows_b, nnz_b, ids_b,
                       (const uint32_t*)pay_b, slices_a, slices_b, loc, slice_base, total, rowptr_out, ids_out,
                       (uint32_t*)pay_out, out_capacity);
    return launch_status();
}
