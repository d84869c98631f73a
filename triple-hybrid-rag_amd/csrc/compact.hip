// Delete on the device: order-preserving removal of entries from a CSR, with renumbering.
//
// Stands where the reference's store deletes rows: every RAG 2.0 table hangs on its parent with
// ON DELETE CASCADE (database/migrations/20260114_rag2_schema.sql:65-66, 106-108, 187, 217-218), its
// end-to-end tests clear a tenant with table(...).delete().eq(...) (tests/test_rag2_e2e.py:276-293)
// and the RAG 1.0 ingestor has delete_by_source (src/voice_agent/ingestion/kb_ingest.py:492-510).
// Here a delete compacts: the surviving chunks keep their order and are renumbered 0 .. n' - 1, so
// a list that was id-ascending stays id-ascending with no sort, and what is left is what a fresh
// build over the survivors would hold.  The same call serves the inverted index (post_doc +
// post_tf) and the entity -> chunk mentions (men_chunk + men_conf, global chunk ids: id_base).
//
//     keep(p)         = 0 <= ids[p] - id_base < n_ids  &&  remap[ids[p] - id_base] >= 0
//     rank(p)         = number of kept positions before p
//     ids_out[rank(p)] = remap[ids[p] - id_base] + id_base,  pay_out[rank(p)] = pay[p]      kept p
//     rowptr_out[t]   = rank(rowptr[t])                                                     t in [0, rows]
//
// Work is cut by INPUT POSITION, not by row (the skew append.hip describes: a handful of rows
// with >= 1e5 entries, a long tail of singletons).  Three plain launches, no workgroup waits for
// another:
//   1. csr_compact_count    a workgroup owns CC_SLICE consecutive positions and writes how many it keeps;
//   2. csr_compact_scan     one workgroup: exclusive scan of the slice counts -> slice bases, *nnz_out;
//   3. csr_compact_scatter  the workgroup recomputes its flags, ranks them (ballot + popcount inside a
//                           wave, wave totals through LDS) and writes the kept entries at base + rank;
//                           the rank of every group of four positions stays in LDS, and the rows whose
//                           rowptr[t] falls in the slice (two wave-uniform binary searches) read their
//                           rowptr_out[t] from there -- any number of empty rows inside one slice is a
//                           strided loop.  The last slice also takes the rows with rowptr[t] == nnz.
// A wave owns a contiguous quarter of the slice, a lane four consecutive positions per round (one
// dwordx4 when the arrays are 16-byte aligned).  Every source index is checked against nnz, every
// remap index against n_ids, every row index against rows and every destination against
// out_capacity before it is used: row pointers or ids that do not match the counts the caller
// passed cannot make a kernel leave its buffers.
#include "thr_common.hpp"

namespace thr {

constexpr int CC_THREADS = 256;
constexpr int CC_WAVES = CC_THREADS / WAVE;
constexpr int CC_SLICE = 8192;                        // input positions per workgroup (32 KiB per payload)
constexpr int CC_ROUNDS = CC_SLICE / (CC_THREADS * 4);   // rounds of one dwordx4 per lane
constexpr int CC_GROUPS = CC_SLICE / 4;

struct CVec4 {
    int32_t v[4];
};

// The new ids of the 4 * CC_ROUNDS positions this lane owns (-1: dropped or behind the end) and the
// wave's kept count.  Position of (round r, element e): s0 + 4 * ((wave * CC_ROUNDS + r) * 64 + lane) + e.
__device__ __forceinline__ int cc_load(const int32_t* __restrict__ ids, const int32_t* __restrict__ remap,
                                       int64_t n_ids, int64_t id_base, int64_t s0, int64_t nnz, int vec_ok,
                                       int32_t (&nid)[CC_ROUNDS][4]) {
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    int kept = 0;
#pragma unroll
    for (int r = 0; r < CC_ROUNDS; ++r) {
        const int64_t p = s0 + 4 * (int64_t)((wave * CC_ROUNDS + r) * WAVE + lane);
        CVec4 x = {{-1, -1, -1, -1}};
        bool in[4] = {p < nnz, p + 1 < nnz, p + 2 < nnz, p + 3 < nnz};
        if (vec_ok && in[3]) {
            x = *reinterpret_cast<const CVec4*>(ids + p);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (in[e]) x.v[e] = ids[p + e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int64_t i = (int64_t)x.v[e] - id_base;
            int32_t m = -1;
            if (in[e] && i >= 0 && i < n_ids) m = remap[i];
            nid[r][e] = m >= 0 ? (int32_t)(m + id_base) : -1;
            kept += __popcll(__ballot(m >= 0));
        }
    }
    return kept;   // wave-uniform
}

__global__ __launch_bounds__(CC_THREADS) void csr_compact_count(const int32_t* __restrict__ ids, int64_t nnz,
                                                                const int32_t* __restrict__ remap, int64_t n_ids,
                                                                int64_t id_base, int vec_ok,
                                                                int32_t* __restrict__ slice_count) {
    __shared__ int s_wave[CC_WAVES];
    int32_t nid[CC_ROUNDS][4];
    const int kept = cc_load(ids, remap, n_ids, id_base, (int64_t)blockIdx.x * CC_SLICE, nnz, vec_ok, nid);
    if (threadIdx.x % WAVE == 0) s_wave[threadIdx.x / WAVE] = kept;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < CC_WAVES; ++w) total += s_wave[w];
        slice_count[blockIdx.x] = total;
    }
}

// One workgroup: thread i sums a contiguous run of slices, the 256 sums are scanned through LDS, and
// the thread writes its run's exclusive bases.  (3 845 slices at 31.5 M postings: 16 per thread.)
__global__ __launch_bounds__(CC_THREADS) void csr_compact_scan(const int32_t* __restrict__ slice_count, int64_t n_slices,
                                                               int64_t* __restrict__ slice_base,
                                                               int64_t* __restrict__ nnz_out) {
    __shared__ int64_t s_sum[CC_THREADS];
    const int64_t per = (n_slices + CC_THREADS - 1) / CC_THREADS;
    const int64_t lo = per * threadIdx.x < n_slices ? per * threadIdx.x : n_slices;
    const int64_t hi = lo + per < n_slices ? lo + per : n_slices;
    int64_t sum = 0;
    for (int64_t i = lo; i < hi; ++i) sum += slice_count[i];
    s_sum[threadIdx.x] = sum;
    block_inclusive_scan<CC_THREADS>(s_sum);        // over the 256 sums
    int64_t run = s_sum[threadIdx.x] - sum;
    for (int64_t i = lo; i < hi; ++i) {
        slice_base[i] = run;
        run += slice_count[i];
    }
    if (threadIdx.x == CC_THREADS - 1) *nnz_out = s_sum[CC_THREADS - 1];
}

template <bool TWO>
__global__ __launch_bounds__(CC_THREADS) void csr_compact_scatter(
    const int64_t* __restrict__ rowptr, int64_t rows, int64_t nnz, const int32_t* __restrict__ ids,
    const uint32_t* __restrict__ pay, const int32_t* __restrict__ remap, int64_t n_ids, int64_t id_base,
    const int64_t* __restrict__ slice_base, int64_t* __restrict__ rowptr_out, int32_t* __restrict__ ids_out,
    uint32_t* __restrict__ pay_out, int64_t out_capacity, int vec_ok) {
    // per group of four positions: (kept positions of the slice before the group) << 4 | its four flags;
    // entry CC_GROUPS: the slice's total
    __shared__ uint32_t s_grp[CC_GROUPS + 1];
    __shared__ int s_wave[CC_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t s0 = (int64_t)blockIdx.x * CC_SLICE;
    const int64_t s1 = s0 + CC_SLICE < nnz ? s0 + CC_SLICE : nnz;
    const bool last = s1 >= nnz;
    int32_t nid[CC_ROUNDS][4];
    const int kept = cc_load(ids, remap, n_ids, id_base, s0, nnz, vec_ok, nid);
    if (lane == 0) s_wave[wave] = kept;
    __syncthreads();
    int before = 0, total = 0;     // kept by the waves in front of this one; by the slice
    for (int w = 0; w < CC_WAVES; ++w) {
        if (w < wave) before += s_wave[w];
        total += s_wave[w];
    }
    const int64_t base = slice_base[blockIdx.x];
    const uint64_t below = ((uint64_t)1 << lane) - 1;
#pragma unroll
    for (int r = 0; r < CC_ROUNDS; ++r) {
        const int g = (wave * CC_ROUNDS + r) * WAVE + lane;
        const int64_t p = s0 + 4 * (int64_t)g;
        int mine = 0, wave_kept = 0;
        uint32_t flags = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t b = __ballot(nid[r][e] >= 0);
            mine += __popcll(b & below);
            wave_kept += __popcll(b);
            flags |= (nid[r][e] >= 0 ? 1u : 0u) << e;
        }
        s_grp[g] = ((uint32_t)(before + mine) << 4) | flags;
        if (flags) {
            CVec4 w = {{0, 0, 0, 0}};
            if (TWO) {
                if (vec_ok && p + 3 < nnz) {
                    w = *reinterpret_cast<const CVec4*>(pay + p);
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (p + e < nnz) w.v[e] = (int32_t)pay[p + e];
                }
            }
            int64_t dst = base + before + mine;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (!(flags >> e & 1)) continue;
                if (dst >= 0 && dst < out_capacity) {
                    ids_out[dst] = nid[r][e];
                    if (TWO) pay_out[dst] = (uint32_t)w.v[e];
                }
                ++dst;
            }
        }
        before += wave_kept;
    }
    if (threadIdx.x == 0) s_grp[CC_GROUPS] = (uint32_t)total << 4;
    // rows whose pointer lies in [s0, s1) -- the last slice: in [s0, nnz] -- searched side by side,
    // wave-uniform: t_lo = first t with rowptr[t] >= s0, t_hi = first t with rowptr[t] >= s1
    int64_t lo1 = 0, hi1 = rows + 1, lo2 = 0, hi2 = rows + 1;
    while (lo1 < hi1 || lo2 < hi2) {
        if (lo1 < hi1) {
            const int64_t m = (lo1 + hi1) >> 1;
            if (rowptr[m] < s0) lo1 = m + 1; else hi1 = m;
        }
        if (lo2 < hi2) {
            const int64_t m = (lo2 + hi2) >> 1;
            if (rowptr[m] < s1) lo2 = m + 1; else hi2 = m;
        }
    }
    const int64_t t_hi = last ? rows + 1 : lo2;
    __syncthreads();   // (s_grp is complete)
    for (int64_t t = lo1 + threadIdx.x; t < t_hi; t += CC_THREADS) {
        const int64_t o = rowptr[t] - s0;
        if (o < 0 || o > s1 - s0 || (o == s1 - s0 && !last)) continue;   // (row pointers that are not sorted)
        const uint32_t g = s_grp[o >> 2];
        rowptr_out[t] = base + (g >> 4) + __popc(g & ((1u << (o & 3)) - 1u));
    }
}

}  // namespace thr

using namespace thr;

static void compact_plan(Arena& A, int64_t nnz, int32_t** slice_count, int64_t** slice_base) {
    const size_t n_slices = (size_t)((nnz + CC_SLICE - 1) / CC_SLICE);
    *slice_count = A.take<int32_t>(n_slices);
    *slice_base = A.take<int64_t>(n_slices);
}

extern "C" size_t thr_csr_compact_workspace_bytes(int64_t rows, int64_t nnz) {
    (void)rows;
    if (nnz <= 0) return 0;
    Arena A;
    int32_t* c;
    int64_t* b;
    compact_plan(A, nnz, &c, &b);
    return A.total;
}

extern "C" int thr_csr_compact(const int64_t* rowptr, int64_t rows, int64_t nnz, const int32_t* ids, const void* pay,
                               const int32_t* remap, int64_t n_ids, int64_t id_base, int64_t* rowptr_out,
                               int32_t* ids_out, void* pay_out, int64_t out_capacity, int64_t* nnz_out,
                               void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!rowptr || !rowptr_out || !nnz_out, THR_ERR_INVALID);
    THR_RETURN_IF(rows <= 0 || nnz < 0 || n_ids < 0 || id_base < 0 || out_capacity < 0, THR_ERR_INVALID);
    THR_RETURN_IF(rows > ((int64_t)1 << 31) - 2 || nnz > ((int64_t)1 << 40) || n_ids > ((int64_t)1 << 31) - 1 ||
                      id_base > ((int64_t)1 << 31) - 1, THR_ERR_INVALID);
    THR_RETURN_IF(nnz > 0 && (!ids || !ids_out || (n_ids > 0 && !remap)), THR_ERR_INVALID);
    const bool two = pay != nullptr;
    THR_RETURN_IF(two != (pay_out != nullptr), THR_ERR_INVALID);
    // out of place: the destinations are buffers of their own
    THR_RETURN_IF(rowptr_out == rowptr, THR_ERR_INVALID);
    THR_RETURN_IF(nnz > 0 && ((const void*)ids_out == (const void*)ids || (two && pay_out == pay) ||
                              (const void*)ids_out == pay_out), THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_csr_compact_workspace_bytes(rows, nnz), THR_ERR_WORKSPACE);
    THR_RETURN_IF(nnz > 0 && !workspace, THR_ERR_INVALID);
    hipStream_t st = (hipStream_t)stream;
    if (nnz == 0) {   // every row is empty and stays so
        hipError_t e = hipMemsetAsync(rowptr_out, 0, sizeof(int64_t) * (size_t)(rows + 1), st);
        if (e == hipSuccess) e = hipMemsetAsync(nnz_out, 0, sizeof(int64_t), st);
        return e == hipSuccess ? THR_OK : (int)e;
    }
    Arena A;
    A.base = (char*)workspace;
    int32_t* slice_count;
    int64_t* slice_base;
    compact_plan(A, nnz, &slice_count, &slice_base);
    const int64_t n_slices = (nnz + CC_SLICE - 1) / CC_SLICE;
    auto al = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const int vec_ok = al(ids) && al(pay);
    hipLaunchKernelGGL(csr_compact_count, dim3((unsigned)n_slices), dim3(CC_THREADS), 0, st, ids, nnz, remap, n_ids,
                       id_base, vec_ok, slice_count);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(csr_compact_scan, dim3(1), dim3(CC_THREADS), 0, st, slice_count, n_slices, slice_base, nnz_out);
    rc = launch_status();
    if (rc) return rc;
    if (two)
        hipLaunchKernelGGL(csr_compact_scatter<true>, dim3((unsigned)n_slices), dim3(CC_THREADS), 0, st, rowptr, rows,
                           nnz, ids, (const uint32_t*)pay, remap, n_ids, id_base, slice_base, rowptr_out, ids_out,
                           (uint32_t*)pay_out, out_capacity, vec_ok);
    else
        hipLaunchKernelGGL(csr_compact_scatter<false>, dim3((unsigned)n_slices), dim3(CC_THREADS), 0, st, rowptr, rows,
                           nnz, ids, (const uint32_t*)pay, remap, n_ids, id_base, slice_base, rowptr_out, ids_out,
                           (uint32_t*)pay_out, out_capacity, vec_ok);
    return launch_status();
}
