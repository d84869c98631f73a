// Graph channel inside a scope: thr_graph_topk with a per-query row filter (gfx950).
//
// The reference's graph search filters every entity and relation query by tenant
// (.eq("org_id", org_id), src/voice_agent/rag2/graph_search.py:154-230), so a tenant's graph list
// holds its own chunks only.  Here the walk is the unfiltered one -- entities carry no attributes,
// BFS distances are thr_graph_topk's -- and the filter sits where a mention becomes a contribution:
// chunk c of query q counts only if query_label[q] < 0 or doc_label[c] == query_label[q] (the
// doc_coll / query_coll convention of the dense and BM25 kernels, the labels thr_scope_resolve
// writes).  An in-scope chunk's score has thr_graph_topk's bits: the same mentions in the same
// (entity ascending, mention) order, summed left to right in float64.
//
// Cost follows the scope.  graph_topk_kernel reserves a contribution slot for every mention of every
// reached entity (thread i loops over entity i's mentions); here a mention that is out of scope or
// out of the shard takes none.  Every reached entity goes to a group of GR_GROUP lanes of a wave, lanes
// over its mentions:
//   count   kept mentions per entity: popcount of the group's bits of the wave's ballot, summed over
//           its trips of GR_GROUP mentions;
//   scan    exclusive scan of the counts over the sorted entities (block-wide);
//   emit    the same walk again; a kept mention lands at  offset(entity) + kept before it in the
//           entity  (trips done + the group's ballot bits below the lane).
// Position order is therefore (entity asc, mention order) among the kept mentions, which is all the
// sort and the segmented sum need.  The label is gathered twice per mention (4 bytes each time)
// against fewer sort keys; a thin tenant's query seeded at a hub entity stays on chip where the
// unfiltered call goes to the global-memory tier.  Entity capacities are the unfiltered ones.
// The per-entity counts live in the top-k buffers' bytes (unused until the sums): no LDS is added.
//
// Same workspace as thr_graph_topk (thr_graph_workspace_bytes), same three tiers, flags, padding.
#include "graph_common.hpp"

namespace thr {

// is mention j of the CSR a contribution of this query?  -> its LOCAL chunk through `c`
__device__ __forceinline__ bool gr_kept(const int32_t* __restrict__ men_chunk, int64_t j,
                                        int64_t chunk_base, int64_t n_chunks,
                                        const int32_t* __restrict__ doc_label, int32_t ql, int64_t& c) {
    c = (int64_t)men_chunk[j] - chunk_base;
    if (c < 0 || c >= n_chunks) return false;
    return ql < 0 || doc_label[c] == ql;
}

// Lanes per reached entity in the count and emit walks.  A whole wave per entity was measured first
// (1M chunks, 2048 queries, ~220 reached entities of ~4 mentions each): the 55 entities a wave then
// takes one after the other are 55 dependent-load latencies in a row, twice, and the call took 0.46 ms
// against the unfiltered 0.20.  Sixteen lanes still cover a typical entity in one trip, a wave has four
// entities' loads in flight, and a hub's mentions are walked 16 at a time.
constexpr int GR_GROUP = 16;
static_assert(WAVE % GR_GROUP == 0 && GR_GROUP <= 32, "groups tile a wave; a group's ballot bits fit 32");

// the ballot bits of group `sub` of the wave
__device__ __forceinline__ uint32_t gr_group_bits(uint64_t ballot, int sub) {
    return (uint32_t)(ballot >> (sub * GR_GROUP)) & ((1u << GR_GROUP) - 1u);
}

// trips of GR_GROUP mentions the longest entity of this WAVE needs (the same value in every lane)
__device__ __forceinline__ int gr_wave_trips(int64_t mentions) {
    int trips = (int)((mentions + GR_GROUP - 1) / GR_GROUP);
    for (int off = GR_GROUP; off < WAVE; off <<= 1) trips = max(trips, __shfl_xor(trips, off));
    return trips;
}

template <typename C, bool ONLY_OVERFLOWED>
__global__ __launch_bounds__(GR_THREADS) void graph_scoped_kernel(
    const int64_t* __restrict__ ent_rowptr, const int32_t* __restrict__ ent_col, int64_t n_entities,
    const int64_t* __restrict__ men_rowptr, const int32_t* __restrict__ men_chunk,
    const float* __restrict__ men_conf, int64_t chunk_base, int64_t n_chunks,
    const int32_t* __restrict__ doc_label, const int32_t* __restrict__ query_label,
    const int32_t* __restrict__ query_seeds, int max_seeds, int hops, int k,
    double* __restrict__ con_val_ws,  // [nq][GR_MAX_CON]
    double* __restrict__ out_s, int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt,
    uint32_t* __restrict__ out_flags) {
    constexpr int GR_SLOTS = C::SLOTS, GR_MAX_ENT = C::MAX_ENT, GR_MAX_CON = C::MAX_CON,
                  GR_CAP = C::CAP;
    static_assert(GR_SLOTS * 5 <= GR_MAX_CON * 8, "hash set must fit the sort-key bytes");
    static_assert(GR_MAX_ENT * 4 <= GR_CAP * 16, "entity offsets must fit the top-k buffers' bytes");
    // LDS: phase A (BFS) uses keys/dist/frontiers; phase B reuses the same bytes for sort keys
    __shared__ uint64_t big[GR_MAX_CON];            // hash set + lists, later sort keys
    __shared__ uint32_t reached[GR_MAX_ENT];         // (entity) list, later sorted
    __shared__ uint8_t reached_dist[GR_MAX_ENT];
    __shared__ int scan_tmp[GR_THREADS];
    __shared__ uint64_t tk_buf[2 * GR_CAP];          // kept-mention offsets per entity, later top-k
    __shared__ int b_cnt;
    __shared__ double th_s;
    __shared__ int64_t th_id;
    __shared__ int n_reached, lvl_begin, lvl_end, overflow;

    uint32_t* keys = reinterpret_cast<uint32_t*>(big);            // [GR_SLOTS]
    uint8_t* hdist = reinterpret_cast<uint8_t*>(keys + GR_SLOTS);  // [GR_SLOTS]
    double* b_s = reinterpret_cast<double*>(tk_buf);               // [GR_CAP]
    int64_t* b_id = reinterpret_cast<int64_t*>(tk_buf + GR_CAP);   // [GR_CAP]
    int* ent_off = reinterpret_cast<int*>(tk_buf);                 // [GR_MAX_ENT]

    const int q = blockIdx.x;
    if (ONLY_OVERFLOWED && !(out_flags[q] & THR_FLAG_OVERFLOW)) return;
    const int32_t ql = query_label[q];
    double* con_val = con_val_ws + (int64_t)q * thr::GR_MAX_CON;
    for (int i = threadIdx.x; i < GR_SLOTS; i += GR_THREADS) keys[i] = GR_EMPTY;
    if (threadIdx.x == 0) {
        n_reached = 0;
        overflow = 0;
    }
    __syncthreads();

    // ---- the walk of graph_topk_kernel, unfiltered, and the sorted reached entities ----
    const int nr = gr_walk_onchip<C>(keys, hdist, big, reached, reached_dist, n_reached, lvl_begin, lvl_end,
                                     overflow, ent_rowptr, ent_col, n_entities, query_seeds, q, max_seeds, hops);
    const int lane = threadIdx.x & 63;

    // ---- count: GR_GROUP lanes per entity, lanes over its mentions; kept = in the shard and in scope ----
    const int sub = lane / GR_GROUP, sl = lane % GR_GROUP;   // the lane's group in its wave, its place in the group
    for (int base = 0; base < nr; base += GR_THREADS / GR_GROUP) {
        const int i = base + (int)threadIdx.x / GR_GROUP;
        int64_t mlo = 0, mhi = 0;
        if (i < nr) {
            mlo = men_rowptr[reached[i]];
            mhi = men_rowptr[reached[i] + 1];
        }
        const int trips = gr_wave_trips(mhi - mlo);          // (wave-uniform: every lane ballots)
        int kept = 0;
        for (int t = 0; t < trips; ++t) {
            const int64_t j = mlo + (int64_t)t * GR_GROUP + sl;
            int64_t c;
            const bool keep = j < mhi && gr_kept(men_chunk, j, chunk_base, n_chunks, doc_label, ql, c);
            kept += __popc(gr_group_bits(__ballot(keep), sub));
        }
        if (sl == 0 && i < nr) ent_off[i] = kept;
    }
    __syncthreads();

    // ---- scan: thread t owns a run of consecutive entities; exclusive offsets in place ----
    const int per = (nr + GR_THREADS - 1) / GR_THREADS;
    const int r0 = threadIdx.x * per, r1 = r0 + per < nr ? r0 + per : nr;
    int mine = 0;
    for (int i = r0; i < r1; ++i) mine += ent_off[i];
    scan_tmp[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < GR_THREADS; off <<= 1) {  // Hillis-Steele inclusive scan
        int v = threadIdx.x >= off ? scan_tmp[threadIdx.x - off] : 0;
        __syncthreads();
        scan_tmp[threadIdx.x] += v;
        __syncthreads();
    }
    const int total = scan_tmp[GR_THREADS - 1];
    {
        int run = scan_tmp[threadIdx.x] - mine;
        for (int i = r0; i < r1; ++i) {
            const int c = ent_off[i];
            ent_off[i] = run;
            run += c;
        }
    }
    if (threadIdx.x == 0 && total > GR_MAX_CON) overflow = 1;
    __syncthreads();

    // ---- emit: the same walk; a kept mention goes to offset + kept before it in its entity.  A query
    // whose kept mentions exceed the capacity emits nothing: it is redone by the next tier ----
    const int nc = total <= GR_MAX_CON ? total : 0;
    for (int base = 0; nc > 0 && base < nr; base += GR_THREADS / GR_GROUP) {
        const int i = base + (int)threadIdx.x / GR_GROUP;
        int64_t mlo = 0, mhi = 0;
        int at = 0;
        double w = 1.0;
        if (i < nr) {
            mlo = men_rowptr[reached[i]];
            mhi = men_rowptr[reached[i] + 1];
            at = ent_off[i];
            w = __dadd_rn(1.0, (double)reached_dist[i]);
        }
        const int trips = gr_wave_trips(mhi - mlo);
        for (int t = 0; t < trips; ++t) {
            const int64_t j = mlo + (int64_t)t * GR_GROUP + sl;
            int64_t c = 0;
            const bool keep = j < mhi && gr_kept(men_chunk, j, chunk_base, n_chunks, doc_label, ql, c);
            const uint32_t m = gr_group_bits(__ballot(keep), sub);
            const int pos = at + __popc(m & ((1u << sl) - 1u));
            if (keep && pos < GR_MAX_CON) {   // (pos < total <= GR_MAX_CON: the bound is checked all the same)
                big[pos] = ((uint64_t)c << 32) | (uint32_t)pos;
                con_val[pos] = __ddiv_rn((double)men_conf[j], w);
            }
            at += __popc(m);
        }
    }
    const int ncp = next_pow2(nc > 1 ? nc : 2);
    for (int i = nc + threadIdx.x; i < ncp; i += GR_THREADS) big[i] = ~0ull;
    __syncthreads();
    sort_u64_asc(big, ncp);
    __threadfence_block();

    // ---- segmented left-to-right sums + top-k (ent_off's bytes become the top-k buffers) ----
    BlockTopK<GR_CAP, GR_THREADS> tk;
    tk.init(b_s, b_id, &b_cnt, &th_s, &th_id, k);
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
    for (int i = threadIdx.x; i < k; i += GR_THREADS) {
        out_s[(int64_t)q * k + i] = i < n ? b_s[i] : -INFINITY;
        out_id[(int64_t)q * k + i] = i < n ? b_id[i] + chunk_base : -1;
    }
    if (threadIdx.x == 0) {
        out_cnt[q] = n;
        out_flags[q] = overflow ? THR_FLAG_OVERFLOW : THR_FLAG_CERTIFIED;
    }
}

// Third tier: graph_fallback_kernel's walk in global memory (see graph.hip), scoring the chunks of
// the query's scope only -- a thread skips its chunk when the label does not match.
__global__ __launch_bounds__(GR_THREADS) void graph_fallback_scoped_kernel(
    const int64_t* __restrict__ ent_rowptr, const int32_t* __restrict__ ent_col, int64_t n_entities,
    const int64_t* __restrict__ tmen_rowptr, const int32_t* __restrict__ tmen_ent,
    const float* __restrict__ tmen_conf, int64_t chunk_base, int64_t n_chunks,
    const int32_t* __restrict__ doc_label, const int32_t* __restrict__ query_label,
    const int32_t* __restrict__ query_seeds, int n_queries, int max_seeds, int hops, int k,
    uint8_t* __restrict__ dist_ws, int64_t e_pad, double* __restrict__ out_s,
    int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt, uint32_t* __restrict__ out_flags) {
    __shared__ double b_s[GrFull::CAP];
    __shared__ int64_t b_id[GrFull::CAP];
    __shared__ int b_cnt;
    __shared__ double th_s;
    __shared__ int64_t th_id;
    uint8_t* dist = dist_ws + (int64_t)blockIdx.x * e_pad;
    for (int q = blockIdx.x; q < n_queries; q += gridDim.x) {
        if (!(out_flags[q] & THR_FLAG_OVERFLOW)) continue;   // same answer in every thread
        const int32_t ql = query_label[q];
        gr_walk_global(dist, e_pad, ent_rowptr, ent_col, n_entities, query_seeds, q, max_seeds, hops);
        BlockTopK<GrFull::CAP, GR_THREADS> tk;
        tk.init(b_s, b_id, &b_cnt, &th_s, &th_id, k);
        for (int64_t base = 0; base < n_chunks; base += GR_THREADS) {
            const int64_t c = base + threadIdx.x;
            bool any = false;
            double score = 0.0;
            if (c < n_chunks && (ql < 0 || doc_label[c] == ql)) {
                const int64_t lo = tmen_rowptr[c], hi = tmen_rowptr[c + 1];
                for (int64_t j = lo; j < hi; ++j) {
                    const uint32_t d = gr_dist(dist, (uint32_t)tmen_ent[j]);
                    if (d != 0xffu) {
                        score = __dadd_rn(score, __ddiv_rn((double)tmen_conf[j], __dadd_rn(1.0, (double)d)));
                        any = true;
                    }
                }
            }
            tk.push(any, score, c);
        }
        const int n = tk.finish();
        for (int i = threadIdx.x; i < k; i += GR_THREADS) {
            out_s[(int64_t)q * k + i] = i < n ? b_s[i] : -INFINITY;
            out_id[(int64_t)q * k + i] = i < n ? b_id[i] + chunk_base : -1;
        }
        if (threadIdx.x == 0) {
            out_cnt[q] = n;
            out_flags[q] = THR_FLAG_CERTIFIED | THR_FLAG_EXACT;
        }
    }
}

}  // namespace thr

using namespace thr;

extern "C" int thr_graph_topk_scoped(
    const int64_t* ent_rowptr, const int32_t* ent_col, int64_t n_entities, const int64_t* men_rowptr,
    const int32_t* men_chunk, const float* men_conf, const int64_t* tmen_rowptr,
    const int32_t* tmen_ent, const float* tmen_conf, int64_t chunk_base, int64_t n_chunks,
    const int32_t* doc_label, const int32_t* query_label, const int32_t* query_seeds, int n_queries,
    int max_seeds, int hops, int k, double* out_scores, int64_t* out_ids, int32_t* out_counts,
    uint32_t* out_flags, void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!ent_rowptr || !ent_col || !men_rowptr || !men_chunk || !men_conf ||
                      !doc_label || !query_label || !query_seeds || !out_scores || !out_ids ||
                      !out_counts || !out_flags || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_entities <= 0 || n_entities >= 0xffffffffll || n_chunks <= 0 ||
                      n_chunks >= 0xffffffffll || n_queries <= 0 || max_seeds <= 0 ||
                      max_seeds > THR_GRAPH_MAX_SEEDS || hops < 0 || hops > 8 || k <= 0 ||
                      k > THR_TOPK_MAX,
                  THR_ERR_INVALID);
    const bool fallback = tmen_rowptr && tmen_ent && tmen_conf;
    THR_RETURN_IF(workspace_bytes < thr_graph_workspace_bytes(n_queries, fallback ? n_entities : 0),
                  THR_ERR_WORKSPACE);
    hipLaunchKernelGGL((graph_scoped_kernel<GrSmall, false>), dim3(n_queries), dim3(GR_THREADS), 0,
                       (hipStream_t)stream, ent_rowptr, ent_col, n_entities, men_rowptr, men_chunk,
                       men_conf, chunk_base, n_chunks, doc_label, query_label, query_seeds, max_seeds,
                       hops, k, (double*)workspace, out_scores, out_ids, out_counts, out_flags);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL((graph_scoped_kernel<GrFull, true>), dim3(n_queries), dim3(GR_THREADS), 0,
                       (hipStream_t)stream, ent_rowptr, ent_col, n_entities, men_rowptr, men_chunk,
                       men_conf, chunk_base, n_chunks, doc_label, query_label, query_seeds, max_seeds,
                       hops, k, (double*)workspace, out_scores, out_ids, out_counts, out_flags);
    rc = launch_status();
    if (rc || !fallback) return rc;
    uint8_t* dist_ws = (uint8_t*)workspace + (size_t)n_queries * GR_MAX_CON * sizeof(double);
    hipLaunchKernelGGL(graph_fallback_scoped_kernel, dim3(GR_FB_BLOCKS), dim3(GR_THREADS), 0,
                       (hipStream_t)stream, ent_rowptr, ent_col, n_entities, tmen_rowptr, tmen_ent,
                       tmen_conf, chunk_base, n_chunks, doc_label, query_label, query_seeds,
                       n_queries, max_seeds, hops, k, dist_ws, (int64_t)graph_dist_pad(n_entities),
                       out_scores, out_ids, out_counts, out_flags);
    return launch_status();
}
