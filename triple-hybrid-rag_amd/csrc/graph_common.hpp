// What the graph channel's kernels share (graph.hip: thr_graph_topk; graph_scope.hip:
// thr_graph_topk_scoped): capacities of the two on-chip tiers, the LDS hash set and sort of the walk,
// the distance bytes of the global-memory tier.  The workspace layout is one: GR_MAX_CON float64
// contribution values per query, then GR_FB_BLOCKS distance arrays (thr_graph_workspace_bytes).
#pragma once
#include "thr_common.hpp"

namespace thr {

constexpr int GR_THREADS = 256;
constexpr int GR_MAX_CON = 8192;   // contributions per query (full capacities; workspace stride)
constexpr uint32_t GR_EMPTY = 0xffffffffu;

// on-chip capacities of one launch flavour
struct GrSmall {
    static constexpr int SLOTS = 2048, MAX_ENT = 1024, MAX_CON = 2048, CAP = 512;
};
struct GrFull {
    static constexpr int SLOTS = 8192, MAX_ENT = 4096, MAX_CON = GR_MAX_CON, CAP = 1024;
};

// insert entity e at BFS level `lvl`; returns true if newly inserted
template <int GR_SLOTS>
__device__ __forceinline__ bool gr_insert(uint32_t* keys, uint8_t* dist, uint32_t e, int lvl) {
    uint32_t h = (e * 2654435761u) >> (32 - __builtin_ctz(GR_SLOTS));
    for (int probe = 0; probe < GR_SLOTS; ++probe) {
        uint32_t old = atomicCAS(&keys[h], GR_EMPTY, e);
        if (old == GR_EMPTY) {
            dist[h] = (uint8_t)lvl;
            return true;
        }
        if (old == e) return false;
        h = (h + 1) & (GR_SLOTS - 1);
    }
    return false;
}

// block-wide bitonic sort of uint64 keys, ascending, n = power of two.  Thread t takes PAIR t of a
// stage (i = t with a zero bit inserted at j, partner i | j): every thread of every trip does a
// compare-exchange (the i ^ j form leaves half of them idle).
__device__ inline void sort_u64_asc(uint64_t* a, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += blockDim.x) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), p = i | j;
                const bool up = (i & k) == 0;
                const uint64_t x = a[i], y = a[p];
                if (up ? (x > y) : (x < y)) {
                    a[i] = y;
                    a[p] = x;
                }
            }
            __syncthreads();
        }
}

// (64 workgroups: a quarter of the CUs -- a batch of many hub-seeded queries costs
// O(E * hops + mentions) per query and would serialise on fewer; 1 byte per entity and workgroup)
constexpr int GR_FB_BLOCKS = 64;
__device__ __forceinline__ void gr_set_dist(uint8_t* dist, int64_t e, uint8_t v) {
    __hip_atomic_store(dist + e, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint32_t gr_dist(const uint8_t* dist, uint32_t e) {
    const uint32_t w = __hip_atomic_load(reinterpret_cast<const uint32_t*>(dist) + (e >> 2),
                                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (w >> (8 * (e & 3))) & 0xffu;
}

// The on-chip walk of one query, shared by graph_topk_kernel and graph_scoped_kernel: seeds at level 0,
// level-synchronous BFS over the entity CSR into the LDS hash set (keys / hdist, emptied by the caller)
// and the reached list, then the reached entities sorted ascending with their distances (through `big`).
// -> the number of reached entities kept (at most C::MAX_ENT; `overflow` is set beyond).  The whole
// workgroup calls it; n_reached and overflow were zeroed by the caller before a barrier.
template <typename C>
__device__ __forceinline__ int gr_walk_onchip(
    uint32_t* keys, uint8_t* hdist, uint64_t* big, uint32_t* reached, uint8_t* reached_dist,
    int& n_reached, int& lvl_begin, int& lvl_end, int& overflow,
    const int64_t* __restrict__ ent_rowptr, const int32_t* __restrict__ ent_col, int64_t n_entities,
    const int32_t* __restrict__ query_seeds, int q, int max_seeds, int hops) {
    constexpr int GR_SLOTS = C::SLOTS, GR_MAX_ENT = C::MAX_ENT;
    // ---- level 0: seeds ----
    if (threadIdx.x < max_seeds) {
        int32_t e = query_seeds[(int64_t)q * max_seeds + threadIdx.x];
        if (e >= 0 && e < n_entities && gr_insert<GR_SLOTS>(keys, hdist, (uint32_t)e, 0)) {
            int p = atomicAdd(&n_reached, 1);
            reached[p] = (uint32_t)e;
            reached_dist[p] = 0;
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        lvl_begin = 0;
        lvl_end = n_reached;
    }
    __syncthreads();

    // ---- BFS levels 1..hops: one wave per frontier entity, lanes over its edges ----
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = GR_THREADS / WAVE;
    for (int lvl = 1; lvl <= hops; ++lvl) {
        const int fb = lvl_begin, fe = lvl_end;
        for (int f = fb + wave; f < fe; f += nw) {
            const uint32_t e = reached[f];
            const int64_t lo = ent_rowptr[e], hi = ent_rowptr[e + 1];
            for (int64_t j = lo + lane; j < hi; j += WAVE) {
                const int32_t t = ent_col[j];
                if (*(volatile int*)&overflow) break;  // the hash set must not fill up
                if (t >= 0 && t < n_entities && gr_insert<GR_SLOTS>(keys, hdist, (uint32_t)t, lvl)) {
                    int p = atomicAdd(&n_reached, 1);
                    if (p < GR_MAX_ENT) {
                        reached[p] = (uint32_t)t;
                        reached_dist[p] = (uint8_t)lvl;
                    } else {
                        overflow = 1;
                    }
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            lvl_begin = fe;
            lvl_end = n_reached < GR_MAX_ENT ? n_reached : GR_MAX_ENT;
        }
        __syncthreads();
        if (overflow) break;
    }
    const int nr = n_reached < GR_MAX_ENT ? n_reached : GR_MAX_ENT;

    // ---- sort reached entities ascending (key = entity << 8 | dist) ----
    __syncthreads();
    {
        const int np = next_pow2(nr > 1 ? nr : 2);
        for (int i = threadIdx.x; i < np; i += GR_THREADS)
            big[i] = i < nr ? ((uint64_t)reached[i] << 8) | reached_dist[i] : ~0ull;
        __syncthreads();
        sort_u64_asc(big, np);
        for (int i = threadIdx.x; i < nr; i += GR_THREADS) {
            reached[i] = (uint32_t)(big[i] >> 8);
            reached_dist[i] = (uint8_t)(big[i] & 0xff);
        }
        __syncthreads();
    }
    return nr;
}

// The walk of one query in GLOBAL memory (third tier of both entry points): the workgroup's distance
// array reset to 0xFF, seeds at 0, then level-synchronous BFS by scanning the array for the previous
// level's entities (see graph.hip).  Ends behind a fence and a barrier: every thread may read dist.
__device__ __forceinline__ void gr_walk_global(
    uint8_t* dist, int64_t e_pad, const int64_t* __restrict__ ent_rowptr,
    const int32_t* __restrict__ ent_col, int64_t n_entities, const int32_t* __restrict__ query_seeds,
    int q, int max_seeds, int hops) {
    const int lane = threadIdx.x & 63;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < e_pad / 4; i += GR_THREADS)
        __hip_atomic_store(reinterpret_cast<uint32_t*>(dist) + i, 0xffffffffu, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    // (the distance bytes are written and read with agent-scope relaxed atomics; a release /
    // acquire fence pair around each barrier orders the levels)
    __threadfence();
    __syncthreads();
    if (threadIdx.x < max_seeds) {
        const int32_t e = query_seeds[(int64_t)q * max_seeds + threadIdx.x];
        if (e >= 0 && e < n_entities) gr_set_dist(dist, e, 0);
    }
    __threadfence();
    __syncthreads();
    for (int lvl = 1; lvl <= hops; ++lvl) {
        for (int64_t base = 0; base < n_entities; base += GR_THREADS) {
            const int64_t e = base + threadIdx.x;
            const bool in_frontier = e < n_entities && gr_dist(dist, (uint32_t)e) == (uint32_t)(lvl - 1);
            uint64_t m = __ballot(in_frontier);
            while (m) {
                const int src = __ffsll((long long)m) - 1;
                m &= m - 1;
                const int64_t f = base + (threadIdx.x & ~63) + src;
                const int64_t lo = ent_rowptr[f], hi = ent_rowptr[f + 1];
                for (int64_t j = lo + lane; j < hi; j += WAVE) {
                    const int32_t t = ent_col[j];
                    if (t >= 0 && t < n_entities && gr_dist(dist, (uint32_t)t) == 0xffu)
                        gr_set_dist(dist, t, (uint8_t)lvl);
                }
            }
        }
        __threadfence();
        __syncthreads();
    }
}

inline size_t graph_dist_pad(int64_t n_entities) { return (size_t)((n_entities + 255) / 256 * 256); }

}  // namespace thr
