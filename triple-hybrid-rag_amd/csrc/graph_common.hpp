// What the graph channel's kernels share (graph.hip: thr_graph_topk and thr_graph_topk_scoped):
// capacities of the two on-chip tiers, the LDS hash set and sort of the walk, the ranking tail behind
// the placed contributions, the distance bytes of the global-memory tier.  The workspace layout is one:
// GR_MAX_CON float64 contribution values per query, then GR_FB_BLOCKS distance arrays
// (thr_graph_workspace_bytes).
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
// compare-exchange (the i ^ j form leaves half of them idle).  The stride is the constant GR_THREADS that
// every graph kernel is launched with.
__device__ inline void sort_u64_asc(uint64_t* a, int n) {
    for (int k = 2; k <= n; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < n / 2; t += GR_THREADS) {
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

// The on-chip walk of one query, shared by both flavours of graph_topk_kernel: seeds at level 0,
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

// A query's ranked list -> its k output slots, padded with (-inf, -1), its count and its flags.
__device__ __forceinline__ void gr_write_topk(const double* b_s, const int64_t* b_id, int n, int q, int k,
                                              int64_t chunk_base, uint32_t flags, double* __restrict__ out_s,
                                              int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt,
                                              uint32_t* __restrict__ out_flags) {
    for (int i = threadIdx.x; i < k; i += GR_THREADS) {
        out_s[(int64_t)q * k + i] = i < n ? b_s[i] : -INFINITY;
        out_id[(int64_t)q * k + i] = i < n ? b_id[i] + chunk_base : -1;
    }
    if (threadIdx.x == 0) {
        out_cnt[q] = n;
        out_flags[q] = flags;
    }
}

// The tail of an on-chip tier, behind the placed contributions: big[0 .. nc) holds the keys
// (local chunk << 32 | position, ~0 for a slot that counts for nothing), con_val[position] the values.
// Keys padded to a power of two and sorted; each chunk's segment summed left to right in float64 by
// the thread that owns its head; streaming block top-k (b_s / b_id may alias bytes the emitter used:
// they are first written here, behind the sort's barriers); the padded write.
template <typename C>
__device__ __forceinline__ void gr_rank_and_write(
    uint64_t* big, int nc, const double* __restrict__ con_val, double* b_s, int64_t* b_id, int* b_cnt,
    double* th_s, int64_t* th_id, const int& overflow, int q, int k, int64_t chunk_base,
    double* __restrict__ out_s, int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt,
    uint32_t* __restrict__ out_flags) {
    const int ncp = next_pow2(nc > 1 ? nc : 2);
    for (int i = nc + threadIdx.x; i < ncp; i += GR_THREADS) big[i] = ~0ull;
    __syncthreads();
    sort_u64_asc(big, ncp);
    __threadfence_block();

    // ---- segmented left-to-right sums + top-k ----
    BlockTopK<C::CAP, GR_THREADS> tk;
    tk.init(b_s, b_id, b_cnt, th_s, th_id, k);
    for (int base = 0; base < nc; base += GR_THREADS) {
        const int i = base + threadIdx.x;
        bool head = false;
        double score = 0.0;
        int64_t chunk = 0;
        if (i < nc && big[i] != ~0ull) {
            const uint32_t c = (uint32_t)(big[i] >> 32);
            head = (i == 0) || ((uint32_t)(big[i - 1] >> 32) != c);
            if (head) {
                chunk = c;
                for (int j = i; j < nc && big[j] != ~0ull && (uint32_t)(big[j] >> 32) == c; ++j)
                    score = __dadd_rn(score, con_val[(uint32_t)big[j]]);
            }
        }
        tk.push(head, score, chunk);
    }
    const int n = tk.finish();
    gr_write_topk(b_s, b_id, n, q, k, chunk_base, overflow ? THR_FLAG_OVERFLOW : THR_FLAG_CERTIFIED, out_s,
                  out_id, out_cnt, out_flags);
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
