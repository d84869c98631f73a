// What the tile-list scans share -- dense_scan_mfma / dense_scan_mfma2 (dense_scan_mfma.hpp),
// dense_scan_f16 (dense_scan_f16.hpp) and dense_scan_anydim (dense_scan_anydim.hpp): the flush of a
// wave's candidate buffer into the tile list and the ballot that fills it, the per-lane tau /
// collection filter, and the loader tables of the LDS-transpose kernels.  Which kernel takes which
// piece, and what was tried and left in the kernels because it changed their instructions:
// DESIGN.md 4.1.
#pragma once
#include "dense_common.hpp"

namespace thr {

// ---- the wave's candidate buffer: WBUF staging slots in LDS (wbuf, wcnt entries used), filled by
// ballot compaction, flushed into the query tile's list before a ballot could overflow it and once
// at the end of the launch: atomic reservation in tile_cnt, bounded copy.
// DRAIN: whether the flush waits for its copy (vmcnt(0)) before the wave goes on, so that only row
// loads are pending afterwards.  dense_scan_mfma / mfma2 / f16 were written with the drain and
// dense_scan_anydim without it (all its waits are hipcc's, which counts the copy's stores among the
// row loads in flight by itself); the drain is not needed for correctness in either, its cost was
// never measured, and the flag says which form a kernel has.  (dense_scan_anydim carries its flush
// written out: through this function its MODE_FILTER kernels gain two instructions.)
template <bool DRAIN>
__device__ __forceinline__ void tilelist_flush(const Cand* wbuf, int& wcnt, int lane, int qtile, int* tile_cnt,
                                               Cand* tile_list, int tile_cap) {
    int base = 0;
    if (lane == 0) base = atomicAdd(&tile_cnt[qtile], wcnt);
    base = __shfl(base, 0, WAVE);
    for (int i = lane; i < wcnt; i += WAVE)
        if (base + i < tile_cap) tile_list[(int64_t)qtile * tile_cap + base + i] = wbuf[i];
    if constexpr (DRAIN) __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): only loads pending afterwards
    wcnt = 0;
}
// One ballot over the wave: the lanes that pass append Cand{sc, doc} (doc is evaluated by those
// lanes only), then the flush if the next ballot, which can add 64 more, could overflow.  Over the
// kernel's own wbuf, wcnt, lane and flush().  (A macro: as a function, or as a type with push() and
// flush(), every MODE_FILTER kernel comes out with other registers -- DESIGN.md 4.1.)
#define THR_TILELIST_PUSH(pass, sc, doc)                                       \
    {                                                                          \
        const uint64_t m = __ballot(pass);                                     \
        if (m) {                                                               \
            const int pos = wcnt + __popcll(m & ((1ull << lane) - 1ull));      \
            if (pass) wbuf[pos] = Cand{sc, doc};                               \
            wcnt += __popcll(m);                                               \
            if (wcnt > WBUF - WAVE) flush();                                   \
        }                                                                      \
    }

// ---- tau and the collection filter of query qg of the batch, one of the lane's queries
template <int MODE>
__device__ __forceinline__ float lane_tau(const float* tau, int qg) {
    return MODE == MODE_FILTER ? tau[qg] : 0.f;
}
// collection filter of this lane's query (-1: none), applied as rows pass tau: tau was taken
// from the sample rows of THAT collection, so without the filter here a collection of 1/c of
// the corpus lets c times the aimed candidates through and overflows the tile list
template <int MODE>
__device__ __forceinline__ int lane_coll(const int32_t* query_coll, int qg, int n_queries) {
    return (MODE == MODE_FILTER && query_coll && qg < n_queries) ? query_coll[qg] : -1;
}

// ---- the loader tables of the LDS-transpose kernels (dense_scan_mfma2 / dense_scan_f16).  Loader
// role of a lane: row (lane >> 3) + 8 i of the tile, 16-byte chunk (lane & 7).
// float4 offset of the lane's chunk in loader row i of row tile t (gpr float4 per row; the row is
// clamped at the tail: a clamped row is never emitted)
__device__ __forceinline__ int64_t loader_off(int64_t t, int i, int lane, int64_t tile_stride, int64_t n_docs, int gpr) {
    int64_t row = t * tile_stride * MF_ROWS + (lane >> 3) + 8 * i;
    row = row < n_docs ? row : n_docs - 1;
    return row * gpr + (lane & 7);
}
// the stage-tile slot the lane writes for loader row i
__device__ __forceinline__ int loader_wslot(int lane, int i) { return mf2_slot((lane >> 3) + 8 * i, lane & 7); }
// the swizzled low part of the query-chunk index of lane (r, h) for x = 4 * (stage parity) + quad
__device__ __forceinline__ int query_low_chunk(int x, int r, int h) { return (((x >> 2) * 8 + 2 * (x & 3) + h) ^ r) & 15; }

}  // namespace thr
