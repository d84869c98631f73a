// Graph channel: bounded BFS over the entity CSR + mention scoring (gfx950).
//
// Stands where the reference calls GraphSearcher.search
// (src/voice_agent/rag2/retrieval.py:316-356 ->
// src/voice_agent/rag2/graph_search.py:290-418).  The reference returns an
// unordered set of chunk ids from PuppyGraph / SQL; the only score forms it
// holds are the standalone package's Cypher, 1/(1+distance) over 1..N hops and
// 1.0 for a direct mention (triple-hybrid-rag/src/triple_hybrid_rag/graph/
// puppygraph.py:152-167, 203-221).  The contract implemented here is the
// oracle's (oracle/thr_oracle.py graph_scores):
//     score(c) = sum over reached entities e, ascending e, mentions in CSR order,
//                of float64(conf(e,c)) / (1 + dist(e)),   dist(e) <= hops.
//
// One workgroup per query, everything on-chip except the contribution values:
//   1. level-synchronous BFS with an LDS open-addressing set (entity -> dist)
//   2. reached entities sorted ascending (LDS bitonic)
//   3. one contribution per (entity, mention) at an exclusive-scan position, so
//      position order == (entity asc, mention order)
//   4. keys (local chunk << 32 | position) sorted in LDS; each chunk's segment is
//      summed left to right in float64 by the thread that owns its head
//   5. streaming block top-k under (score desc, chunk asc)
// Algorithmic bytes per query: S*8 + sum_hops frontier*deg*4 + reached*(16 + mentions*8).
//
// Two launches, no host round trip: every query first runs with SMALL on-chip capacities
// (1024 entities / 2048 contributions: 5 workgroups per CU instead of 1), and only the queries
// that report an overflow there are redone by the second launch with the full capacities
// (its other workgroups exit at once).  Capacities never truncate silently: a query that
// overflows the full ones too keeps THR_FLAG_OVERFLOW until the third tier (below) redoes it.
//
// thr_graph_topk_scoped is the same call with a per-query row filter.  The reference's graph search
// filters every entity and relation query by tenant (.eq("org_id", org_id),
// src/voice_agent/rag2/graph_search.py:154-230), so a tenant's graph list holds its own chunks only.
// Here the walk is the unfiltered one -- entities carry no attributes, BFS distances are
// thr_graph_topk's -- and the filter sits where a mention becomes a contribution: chunk c of query q
// counts only if query_label[q] < 0 or doc_label[c] == query_label[q] (the doc_coll / query_coll
// convention of the dense and BM25 kernels, the labels thr_scope_resolve writes).  An in-scope chunk's
// score has thr_graph_topk's bits: the same mentions in the same (entity ascending, mention) order,
// summed left to right in float64.  Same workspace (thr_graph_workspace_bytes), tiers, flags, padding.
//
// Both entry points run ONE kernel template per tier and one host driver, both below; the walks and the
// ranking tail are device functions in graph_common.hpp.  Only step 3 differs -- gr_emit_all /
// gr_emit_kept below.
#include "graph_common.hpp"

namespace thr {

// ---- step 3, unscoped: thread i walks entity i's mentions and reserves a slot for EVERY one of them
// (an out-of-shard mention gets the key ~0) at the exclusive scan of the mention counts over the sorted
// entities.  Positions at or past MAX_CON set `overflow`; the first MAX_CON contributions are ranked.
// -> the number of contributions placed
template <typename C>
__device__ __forceinline__ int gr_emit_all(
    int nr, const uint32_t* reached, const uint8_t* reached_dist, int* scan_tmp, uint64_t* big,
    double* __restrict__ con_val, int& overflow, const int64_t* __restrict__ men_rowptr,
    const int32_t* __restrict__ men_chunk, const float* __restrict__ men_conf, int64_t chunk_base,
    int64_t n_chunks) {
    constexpr int GR_MAX_CON = C::MAX_CON;
    int running = 0;  // same in every thread
    for (int base = 0; base < nr; base += GR_THREADS) {
        const int i = base + threadIdx.x;
        int cntm = 0;
        int64_t mlo = 0;
        if (i < nr) {
            mlo = men_rowptr[reached[i]];
            cntm = (int)(men_rowptr[reached[i] + 1] - mlo);
        }
        scan_tmp[threadIdx.x] = cntm;
        block_inclusive_scan<GR_THREADS>(scan_tmp);
        const int excl = running + scan_tmp[threadIdx.x] - cntm;
        const int chunk_total = scan_tmp[GR_THREADS - 1];
        if (i < nr) {
            const double w = __dadd_rn(1.0, (double)reached_dist[i]);
            for (int m = 0; m < cntm; ++m) {
                const int pos = excl + m;
                if (pos < GR_MAX_CON) {
                    const int64_t c = (int64_t)men_chunk[mlo + m] - chunk_base;
                    const bool mine = c >= 0 && c < n_chunks;
                    big[pos] = mine ? ((uint64_t)c << 32) | (uint32_t)pos : ~0ull;
                    con_val[pos] = __ddiv_rn((double)men_conf[mlo + m], w);
                } else {
                    overflow = 1;
                }
            }
        }
        running += chunk_total;
        __syncthreads();
    }
    return running < GR_MAX_CON ? running : GR_MAX_CON;
}

// ---- step 3, scoped: a contribution slot only for the mentions the query keeps.
// gr_emit_all reserves a slot for every mention of every reached entity; here a mention that is out of
// scope or out of the shard takes none, so cost follows the scope.  Every reached entity goes to a
// group of GR_GROUP lanes of a wave, lanes over its mentions:
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

// -> the number of contributions placed: 0 when the kept mentions exceed the capacity (`overflow` is
// set and the query is redone by the next tier)
template <typename C>
__device__ __forceinline__ int gr_emit_kept(
    int nr, const uint32_t* reached, const uint8_t* reached_dist, int* scan_tmp, int* ent_off, uint64_t* big,
    double* __restrict__ con_val, int& overflow, const int64_t* __restrict__ men_rowptr,
    const int32_t* __restrict__ men_chunk, const float* __restrict__ men_conf, int64_t chunk_base,
    int64_t n_chunks, const int32_t* __restrict__ doc_label, int32_t ql) {
    constexpr int GR_MAX_CON = C::MAX_CON;
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
    block_inclusive_scan<GR_THREADS>(scan_tmp);
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
    return nc;
}

// One workgroup per query, one on-chip tier (C: its capacities; ONLY_OVERFLOWED: the second launch).
// doc_label / query_label are read by the SCOPED flavour only.
template <typename C, bool ONLY_OVERFLOWED, bool SCOPED>
__global__ __launch_bounds__(GR_THREADS) void graph_topk_kernel(
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
    int32_t ql = -1;
    if constexpr (SCOPED) ql = query_label[q];
    double* con_val = con_val_ws + (int64_t)q * thr::GR_MAX_CON;
    for (int i = threadIdx.x; i < GR_SLOTS; i += GR_THREADS) keys[i] = GR_EMPTY;
    if (threadIdx.x == 0) {
        n_reached = 0;
        overflow = 0;
    }
    __syncthreads();

    // ---- walk: seeds, BFS levels 1..hops, reached entities sorted ascending (graph_common.hpp) ----
    const int nr = gr_walk_onchip<C>(keys, hdist, big, reached, reached_dist, n_reached, lvl_begin, lvl_end,
                                     overflow, ent_rowptr, ent_col, n_entities, query_seeds, q, max_seeds, hops);

    // ---- contributions -> big[0 .. nc) / con_val, position order == (entity asc, mention order) ----
    int nc;
    if constexpr (SCOPED)
        nc = gr_emit_kept<C>(nr, reached, reached_dist, scan_tmp, ent_off, big, con_val, overflow, men_rowptr,
                             men_chunk, men_conf, chunk_base, n_chunks, doc_label, ql);
    else
        nc = gr_emit_all<C>(nr, reached, reached_dist, scan_tmp, big, con_val, overflow, men_rowptr, men_chunk,
                            men_conf, chunk_base, n_chunks);

    // ---- sort, segmented sums, top-k, write (ent_off's bytes become the top-k buffers) ----
    gr_rank_and_write<C>(big, nc, con_val, b_s, b_id, &b_cnt, &th_s, &th_id, overflow, q, k, chunk_base, out_s,
                         out_id, out_cnt, out_flags);
}

// ---------------------------------------------------------------------------------------------
// Third tier: queries that overflow the full on-chip capacities too (a hub entity with tens of
// thousands of edges) are walked in GLOBAL memory -- no capacity left to overflow, so
// THR_FLAG_OVERFLOW never reaches the caller and nothing in a batch pipeline has to raise.
// GR_FB_BLOCKS workgroups share the overflowed queries of the batch; each owns one distance
// array (1 byte per entity, 0xFF = not reached) and
//   1. BFS, level-synchronous, by SCANNING the distance array for the entities of the previous
//      level (no frontier lists); a wave expands one frontier entity at a time, lanes over its
//      edges.  The distance bytes are written and read with agent-scope relaxed atomics (the
//      array is rewritten level after level by the same CU), fenced at every level barrier, and
//      only ever change 0xFF -> level, so racing writers agree;
//   2. scores every chunk of the shard from the TRANSPOSED mention CSR (chunk -> (entity, conf),
//      in (entity asc, mention) order -- built once at index set-up): one thread per chunk sums
//      conf/(1+dist) left to right in float64, which is the oracle's order, then the streaming
//      block top-k.  O(E + mentions) per query instead of O(reached): a rare, slow, exact path.
// ---------------------------------------------------------------------------------------------
// The SCOPED flavour scores the chunks of the query's scope only: a thread skips its chunk when the
// label does not match.
// (GR_FB_BLOCKS workgroups and the distance accessors: graph_common.hpp)
template <bool SCOPED>
__global__ __launch_bounds__(GR_THREADS) void graph_fallback_kernel(
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
        int32_t ql = -1;
        if constexpr (SCOPED) ql = query_label[q];
        gr_walk_global(dist, e_pad, ent_rowptr, ent_col, n_entities, query_seeds, q, max_seeds, hops);
        BlockTopK<GrFull::CAP, GR_THREADS> tk;
        tk.init(b_s, b_id, &b_cnt, &th_s, &th_id, k);
        for (int64_t base = 0; base < n_chunks; base += GR_THREADS) {
            const int64_t c = base + threadIdx.x;
            bool any = false;
            double score = 0.0;
            bool mine = c < n_chunks;
            if constexpr (SCOPED) mine = mine && (ql < 0 || doc_label[c] == ql);
            if (mine) {
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
        gr_write_topk(b_s, b_id, n, q, k, chunk_base, THR_FLAG_CERTIFIED | THR_FLAG_EXACT, out_s, out_id, out_cnt,
                      out_flags);
    }
}

}  // namespace thr

using namespace thr;

extern "C" size_t thr_graph_workspace_bytes(int n_queries, int64_t n_entities) {
    if (n_queries <= 0) return 0;
    return (size_t)n_queries * GR_MAX_CON * sizeof(double) +
           (n_entities > 0 ? (size_t)GR_FB_BLOCKS * graph_dist_pad(n_entities) : 0);
}

// Both entry points: the argument checks (the scoped call's two labels among them), the workspace check
// and the three launches (small tier for every query, full tier and global-memory tier for the queries
// that still carry THR_FLAG_OVERFLOW).
template <bool SCOPED>
static int graph_topk(const int64_t* ent_rowptr, const int32_t* ent_col, int64_t n_entities,
                      const int64_t* men_rowptr, const int32_t* men_chunk, const float* men_conf,
                      const int64_t* tmen_rowptr, const int32_t* tmen_ent, const float* tmen_conf,
                      int64_t chunk_base, int64_t n_chunks, const int32_t* doc_label,
                      const int32_t* query_label, const int32_t* query_seeds, int n_queries, int max_seeds,
                      int hops, int k, double* out_scores, int64_t* out_ids, int32_t* out_counts,
                      uint32_t* out_flags, void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!ent_rowptr || !ent_col || !men_rowptr || !men_chunk || !men_conf ||
                      !query_seeds || !out_scores || !out_ids || !out_counts || !out_flags ||
                      !workspace,
                  THR_ERR_INVALID);
    if constexpr (SCOPED) THR_RETURN_IF(!doc_label || !query_label, THR_ERR_INVALID);
    THR_RETURN_IF(n_entities <= 0 || n_entities >= 0xffffffffll || n_chunks <= 0 ||
                      n_chunks >= 0xffffffffll || n_queries <= 0 || max_seeds <= 0 ||
                      max_seeds > THR_GRAPH_MAX_SEEDS || hops < 0 || hops > 8 || k <= 0 ||
                      k > THR_TOPK_MAX,
                  THR_ERR_INVALID);
    const bool fallback = tmen_rowptr && tmen_ent && tmen_conf;
    THR_RETURN_IF(workspace_bytes < thr_graph_workspace_bytes(n_queries, fallback ? n_entities : 0),
                  THR_ERR_WORKSPACE);
    hipLaunchKernelGGL((graph_topk_kernel<GrSmall, false, SCOPED>), dim3(n_queries), dim3(GR_THREADS), 0,
                       (hipStream_t)stream, ent_rowptr, ent_col, n_entities, men_rowptr, men_chunk,
                       men_conf, chunk_base, n_chunks, doc_label, query_label, query_seeds, max_seeds,
                       hops, k, (double*)workspace, out_scores, out_ids, out_counts, out_flags);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL((graph_topk_kernel<GrFull, true, SCOPED>), dim3(n_queries), dim3(GR_THREADS), 0,
                       (hipStream_t)stream, ent_rowptr, ent_col, n_entities, men_rowptr, men_chunk,
                       men_conf, chunk_base, n_chunks, doc_label, query_label, query_seeds, max_seeds,
                       hops, k, (double*)workspace, out_scores, out_ids, out_counts, out_flags);
    rc = launch_status();
    if (rc || !fallback) return rc;
    uint8_t* dist_ws = (uint8_t*)workspace + (size_t)n_queries * GR_MAX_CON * sizeof(double);
    hipLaunchKernelGGL(graph_fallback_kernel<SCOPED>, dim3(GR_FB_BLOCKS), dim3(GR_THREADS), 0,
                       (hipStream_t)stream, ent_rowptr, ent_col, n_entities, tmen_rowptr, tmen_ent,
                       tmen_conf, chunk_base, n_chunks, doc_label, query_label, query_seeds,
                       n_queries, max_seeds, hops, k, dist_ws, (int64_t)graph_dist_pad(n_entities),
                       out_scores, out_ids, out_counts, out_flags);
    return launch_status();
}

extern "C" int thr_graph_topk(const int64_t* ent_rowptr, const int32_t* ent_col, int64_t n_entities,
                              const int64_t* men_rowptr, const int32_t* men_chunk,
                              const float* men_conf, const int64_t* tmen_rowptr,
                              const int32_t* tmen_ent, const float* tmen_conf, int64_t chunk_base,
                              int64_t n_chunks, const int32_t* query_seeds, int n_queries,
                              int max_seeds, int hops, int k, double* out_scores, int64_t* out_ids,
                              int32_t* out_counts, uint32_t* out_flags, void* workspace,
                              size_t workspace_bytes, thr_stream_t stream) {
    return graph_topk<false>(ent_rowptr, ent_col, n_entities, men_rowptr, men_chunk, men_conf, tmen_rowptr,
                             tmen_ent, tmen_conf, chunk_base, n_chunks, nullptr, nullptr, query_seeds,
                             n_queries, max_seeds, hops, k, out_scores, out_ids, out_counts, out_flags,
                             workspace, workspace_bytes, stream);
}

extern "C" int thr_graph_topk_scoped(
    const int64_t* ent_rowptr, const int32_t* ent_col, int64_t n_entities, const int64_t* men_rowptr,
    const int32_t* men_chunk, const float* men_conf, const int64_t* tmen_rowptr,
    const int32_t* tmen_ent, const float* tmen_conf, int64_t chunk_base, int64_t n_chunks,
    const int32_t* doc_label, const int32_t* query_label, const int32_t* query_seeds, int n_queries,
    int max_seeds, int hops, int k, double* out_scores, int64_t* out_ids, int32_t* out_counts,
    uint32_t* out_flags, void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    return graph_topk<true>(ent_rowptr, ent_col, n_entities, men_rowptr, men_chunk, men_conf, tmen_rowptr,
                            tmen_ent, tmen_conf, chunk_base, n_chunks, doc_label, query_label, query_seeds,
                            n_queries, max_seeds, hops, k, out_scores, out_ids, out_counts, out_flags,
                            workspace, workspace_bytes, stream);
}
