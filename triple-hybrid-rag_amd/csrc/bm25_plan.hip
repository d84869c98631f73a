// BM25 work decomposition and its tail: the plan and the slice edges before the walks, the sweep
// filter between stage A and stage B, the merge of the slices' lists.
#include "bm25_common.hpp"

namespace thr {

// ---------------------------------------------------------------------------------------------
// Work decomposition (one launch each, no host round trip):
//   bm25_plan_kernel   per query: the valid term ids in query order, the total posting count,
//                      the number of doc-range slices S_q (1 up to one slice's postings, else
//                      ~total / target, <= BM_MAX_SLICES; the target doubles until all items
//                      fit the item list), the item list (query, slice);
//   bm25_edges_kernel  per (item, term): the first posting of the slice in the term's list
//                      (slice s of S starts at doc B_s = the (len * s / S)-th doc of the
//                      query's longest list: equal shares of the dominant list whatever the
//                      distribution of its docs; the other lists are cut by binary search);
//   bm25_topk_kernel   persistent workgroups pull items from ctl[CTL_NEXT_BLOCK];
//   bm25_merge_kernel  per query with S_q > 1: the best k of its slices' lists.
constexpr int BM_MAX_SLICES = 128;
constexpr int WW_TARGET_MIN = 640, WW_TARGET_MAX = 1536;   // postings per slice of the wave walk (bm25_walk_wave_kernel)
constexpr int BM_TARGET0 = 24576;      // postings per slice aimed at when the batch fills the grid (3 passes)
constexpr int BM_TARGET_MIN = 8192;    // ... and at least (one pass), when it does not: a one-query
                                       // call spreads its 75 K postings over nine workgroups
constexpr int PLAN_THREADS = 256;       // bm25_plan_kernel: one query per thread in as many workgroups as that takes (<= 64);
constexpr int PLAN_MAX_BLOCKS = 64;     // the workgroup that finishes last cuts the slices and writes the item list
// bm25_plan_kernel's fit loop doubles a slice size whose items do not fit, up to BM_TARGET_OPEN -- a size no query
// reaches (at most 32 lists of < 2^31 postings, < 2^31 docs): every query is then its fewest items, which the
// item list always holds (bm_layout) -- and at most BM_FIT_PASSES times (both sizes are there after 58 doublings)
constexpr int BM_FIT_PASSES = 64;
constexpr long long BM_TARGET_OPEN = 1ll << 40;

__device__ __forceinline__ int bm_slices(long long tot, long long target);
// stage-A slices of a query with dense terms: none when its other terms have no posting
__device__ __forceinline__ int bm_slices_a(long long sparse, long long target) {
    return sparse > 0 ? bm_slices(sparse, target) : 0;
}
__device__ __forceinline__ int bm_slices(long long tot, long long target) {
    if (tot <= target) return 1;   // (a query of at most one slice's postings is one work item)
    const long long s = (tot + target - 1) / target;
    return s < 1 ? 1 : s > BM_MAX_SLICES ? BM_MAX_SLICES : (int)s;
}

__global__ __launch_bounds__(PLAN_THREADS) void bm25_plan_kernel(
    const int64_t* __restrict__ rowptr, int64_t n_vocab, const int32_t* __restrict__ query_terms,
    int nq, int mt, int cap, int cap_wave, int conjunctive, int n_slots, int target_max, int target_a0, int wave_mode, int walk_div,
    const int32_t* __restrict__ dense_slot, const double* __restrict__ term_ub, int64_t n_docs,
    int32_t* __restrict__ ctl, int64_t* __restrict__ q_tot, double* __restrict__ q_dub,
    int32_t* __restrict__ q_nt, int32_t* __restrict__ q_S, int32_t* __restrict__ q_SA,
    int32_t* __restrict__ q_pmask, int32_t* __restrict__ q_item0,
    int32_t* __restrict__ q_long, int32_t* __restrict__ q_terms, int2* __restrict__ items) {
    // Part 1, every workgroup: what a query is made of (its own load chains -- term ids, then list
    // lengths / bounds / row slots -- are the kernel's time: one query per thread, the workgroups of
    // the grid on different CUs; round 3 ran this on ONE workgroup, two queries per thread: 62 us)
    __shared__ int red[PLAN_THREADS];
    int n_dp = 0, n_blk = 0;
    for (int q = blockIdx.x * PLAN_THREADS + threadIdx.x; q < nq; q += gridDim.x * PLAN_THREADS) {
        int nt = 0, lng = 0;
        long long tot = 0, best = -1;
        bool dead = false;   // AND mode: a term outside the vocabulary is held by no doc
#pragma unroll 4
        for (int j = 0; j < mt; ++j) {
            const int term = query_terms[(int64_t)q * mt + j];
            if (term >= n_vocab && conjunctive) dead = true;
            if (term < 0 || term >= n_vocab) continue;   // padding / unknown term: no postings
            q_terms[(int64_t)q * mt + nt++] = term;
        }
        if (dead) nt = 0;   // (nothing to score: the item writes an empty list)
        // A query with dense terms (OR form, <= 8 terms) is split the MaxScore way.  Some of its
        // terms are PROBED -- never walked, read from their per-doc rows where a doc is scored --,
        // the others are WALKED.  Stage A walks the walked terms' postings (slices of those lists,
        // bm25_topk_kernel<.., true>); stage B sweeps the shard's docs that hold none of the walked
        // terms in doc windows (bm25_window_kernel) -- and is skipped when the probed terms' bounds
        // together cannot reach stage A's threshold.  Which terms are probed only decides the
        // cost, never the result: a term held by 1/64 of the docs always is (walking a posting costs
        // ~20x what a sweep spends on a doc); rarer terms with rows are walked, rarest first, until
        // the bounds of what is left sum to half the largest bound of a walked term held by >= 200
        // docs (a guess of stage A's threshold from below: then the sweep is very likely skipped).
        // q_SA = -1: not such a query; else the number of stage-A slices (the first q_SA of q_S).
        uint32_t pmask = 0;
        double dub = 0.0;
        long long walked = 0;
        if (nt <= 8) {
            // everything about the (up to eight) terms in registers, the loads of all of them in flight
            // together: this kernel is one workgroup, its time is the length of its load chains
            long long len_[8];
            double ub_[8];
            uint32_t cap_mask = 0;   // terms that have per-doc rows
            const bool rows = dense_slot && !conjunctive;
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const bool on = t < nt;
                const int term = on ? q_terms[(int64_t)q * mt + t] : 0;
                len_[t] = on ? rowptr[term + 1] - rowptr[term] : 0;
                ub_[t] = on && rows ? term_ub[term] : 0.0;
                if (on && rows && dense_slot[term] >= 0) cap_mask |= 1u << t;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                tot += len_[t];
                if (t < nt && len_[t] > best) { best = len_[t]; lng = t; }
            }
            walked = tot;
            if (cap_mask) {
                double walk_ub = 0.0;
                pmask = cap_mask;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    if ((cap_mask >> t) & 1u) dub += ub_[t];
                    else if (t < nt && len_[t] >= 200 && ub_[t] > walk_ub) walk_ub = ub_[t];
                }
                for (;;) {
                    if (!(dub > 0.5 * walk_ub)) break;
                    int pick = -1;
                    long long pick_len = 0;
                    double pick_ub = 0.0;
#pragma unroll
                    for (int t = 0; t < 8; ++t) {   // the rarest probed term that may be walked
                        if (!((pmask >> t) & 1u)) continue;
                        if (len_[t] * walk_div >= n_docs) continue;   // (walking costs ~20x a sweep's per-doc work)
                        if (pick < 0 || len_[t] < pick_len) { pick = t; pick_len = len_[t]; pick_ub = ub_[t]; }
                    }
                    if (pick < 0) break;
                    pmask &= ~(1u << pick);
                    dub -= pick_ub;
                    if (pick_len >= 200 && pick_ub > walk_ub) walk_ub = pick_ub;
                }
                dub = 0.0;   // (summed again: no cancellation left over from the subtractions)
                walked = 0;
                best = -1;
#pragma unroll
                for (int t = 0; t < 8; ++t) {
                    if (t >= nt) continue;
                    if ((pmask >> t) & 1u) {
                        dub += ub_[t];
                    } else {
                        walked += len_[t];
                        if (len_[t] > best) { best = len_[t]; lng = t; }   // (the longest WALKED list cuts the stage-A slices)
                    }
                }
                if (pmask) ++n_dp;
            }
        } else {
            for (int t = 0; t < nt; ++t) {
                const int term = q_terms[(int64_t)q * mt + t];
                const long long len = rowptr[term + 1] - rowptr[term];
                if (len > best) { best = len; lng = t; }
                tot += len;
            }
        }
        // Wave mode (bm25_walk_wave_kernel): an OR query of <= 8 terms WITHOUT probed terms is walked by
        // waves too -- it is a stage A with nothing probed and no stage B: bit 30 marks it, all its
        // slices are stage-A slices (q_SA == q_S), cut with the waves' slice size.
        const bool wave_q = wave_mode && !conjunctive && nt >= 1 && nt <= 8 && !pmask;
        q_SA[q] = (pmask || wave_q) ? 0 : -1;      // (slice counts: below, once the target is known)
        if (!(pmask || wave_q)) ++n_blk;           // (left to the workgroup walk)
        q_pmask[q] = (int32_t)pmask | (wave_q ? (1 << 30) : 0);
        q_dub[q] = dub;
        q_tot[q] = pmask ? -(walked + 1) : tot;    // dense terms: -(postings of the walked terms + 1)
        q_nt[q] = nt;
        q_long[q] = lng;
    }
    {   // queries with probed terms: one atomic per wave
        for (int o = WAVE / 2; o > 0; o >>= 1) {
            n_dp += __shfl_down(n_dp, o, WAVE);
            n_blk += __shfl_down(n_blk, o, WAVE);
        }
        if ((threadIdx.x & (WAVE - 1)) == 0 && n_dp) atomicAdd(&ctl[CTL_DENSE_Q], n_dp);
        if ((threadIdx.x & (WAVE - 1)) == 0 && n_blk) atomicAdd(&ctl[CTL_BLOCK_Q], n_blk);   // queries the workgroup walk takes
    }
    // Part 2, the workgroup that finishes last: slice size, item list.  (Its reads of the other
    // workgroups' per-query words go to L2: agent-scope atomic loads.)
    __shared__ int is_last;
    __threadfence();
    __syncthreads();
    if (threadIdx.x == 0) is_last = atomicAdd(&ctl[CTL_PLAN_DONE], 1) == (int)gridDim.x - 1;
    __syncthreads();
    if (!is_last) return;
    __threadfence();
    auto tot_of = [&](int q) -> long long {
        return (long long)__hip_atomic_load(&q_tot[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    auto wave_q_of = [&](int q) -> bool {   // an ordinary query the waves walk (bit 30 of its probe mask)
        return (__hip_atomic_load(&q_pmask[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 30) & 1;
    };
    const int per = (nq + PLAN_THREADS - 1) / PLAN_THREADS;
    const int q0 = threadIdx.x * per < nq ? threadIdx.x * per : nq;
    const int q1 = q0 + per < nq ? q0 + per : nq;
    // slice size: what gives every workgroup slot of the grid an item, between one pass and three
    __shared__ long long red64[PLAN_THREADS], red64w[PLAN_THREADS];
    {
        long long t = 0, tw = 0;   // (a stage-B sweep counts one unit per doc)
        for (int q = q0; q < q1; ++q) {
            const long long v = tot_of(q);
            t += v >= 0 ? v : -v - 1 + n_docs;
            tw += v >= 0 ? (wave_q_of(q) ? v : 0) : -v - 1;   // postings the waves will walk
        }
        red64[threadIdx.x] = t;
        red64w[threadIdx.x] = tw;
        __syncthreads();
        for (int o = PLAN_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                red64[threadIdx.x] += red64[threadIdx.x + o];
                red64w[threadIdx.x] += red64w[threadIdx.x + o];
            }
            __syncthreads();
        }
    }
    long long target = red64[0] / (n_slots > 0 ? n_slots : 1);
    target = target < BM_TARGET_MIN ? BM_TARGET_MIN : target > target_max ? target_max : target;
    // The waves' slices have their own size (bm25_walk_wave_kernel): what gives each of the ``target_a0``
    // wave slots of the chip an item, between WW_TARGET_MIN (a small batch spreads over many waves: 256
    // survey queries 0.46 -> 0.43 ms) and WW_TARGET_MAX (a full batch pays the per-item set-up less
    // often: 2048 survey queries 0.89 -> 0.87 ms); 0: no wave walk, stage A takes the shared size.
    long long target_a = target;
    if (target_a0 > 0) {
        target_a = red64w[0] / target_a0;
        target_a = target_a < WW_TARGET_MIN ? WW_TARGET_MIN : target_a > WW_TARGET_MAX ? WW_TARGET_MAX : target_a;
    }
    // ``cap`` items for the sweeps and the workgroup walk's items (the slice size that budget gives them
    // was tuned with it), ``cap_wave`` more for the waves' ~1 K-posting slices.  A slice size that does not
    // fit is doubled, up to BM_TARGET_OPEN and at most BM_FIT_PASSES times: the last pass counts every query
    // at BM_TARGET_OPEN -- one item of the waves, or one of the workgroup walk, or a stage A and one sweep --,
    // and cap >= 2 nq, cap_wave >= nq hold that (bm_layout).  The loop ends whatever the batch.
    __shared__ int red_w[PLAN_THREADS];
    int total = 0, mine = 0;
    for (int pass = 0;; ++pass) {
        if (pass == BM_FIT_PASSES) target = target_a = BM_TARGET_OPEN;
        mine = 0;
        int mine_w = 0;
        for (int q = q0; q < q1; ++q) {
            const long long v = tot_of(q);
            if (v >= 0) {
                if (wave_q_of(q)) mine_w += bm_slices(v, target_a);
                else mine += bm_slices(v, target);
            } else {
                const int sa = bm_slices_a(-v - 1, target_a);
                if (wave_mode) mine_w += sa; else mine += sa;
                mine += bm_slices(n_docs, target);
            }
        }
        red[threadIdx.x] = mine;
        red_w[threadIdx.x] = mine_w;
        __syncthreads();
        for (int o = PLAN_THREADS / 2; o > 0; o >>= 1) {
            if ((int)threadIdx.x < o) {
                red[threadIdx.x] += red[threadIdx.x + o];
                red_w[threadIdx.x] += red_w[threadIdx.x + o];
            }
            __syncthreads();
        }
        total = red[0] + red_w[0];
        const bool fits = red[0] <= cap && red_w[0] <= cap_wave;
        const bool grow_w = red_w[0] > cap_wave;
        __syncthreads();
        mine += mine_w;
        if (fits || pass == BM_FIT_PASSES) break;
        if (grow_w) {
            target_a = target_a < BM_TARGET_OPEN / 2 ? target_a * 2 : BM_TARGET_OPEN;
            continue;
        }
        target = target < BM_TARGET_OPEN / 2 ? target * 2 : BM_TARGET_OPEN;
        if (!wave_mode) target_a = target;   // (stage A on the workgroup walk: its slices are in ``cap`` and grow with the others)
    }
    // exclusive prefix of the per-thread item counts
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < PLAN_THREADS; o <<= 1) {
        const int v = (int)threadIdx.x >= o ? red[threadIdx.x - o] : 0;
        __syncthreads();
        red[threadIdx.x] += v;
        __syncthreads();
    }
    // Item order: slice 0 of EVERY query first (item q), then the other slices query by query
    // (item q_item0[q] + s, s >= 1).  The slices of a query that are started together all begin
    // without a threshold and score every doc of their first pass in full; with this order a
    // query's first slice has published its threshold (theta_glob) long before most of its other
    // slices are taken, and those start with the pruning already in force.
    int rest = (red[threadIdx.x] - mine) - q0;   // slices s >= 1 of the queries before this thread's
    for (int q = q0; q < q1; ++q) {
        int S = 0;
        const long long v = tot_of(q);
        if (v >= 0) {
            const bool wq = wave_q_of(q);
            S = bm_slices(v, wq ? target_a : target);
            if (wq) q_SA[q] = S;
        } else {
            const int SA = bm_slices_a(-v - 1, target_a);
            q_SA[q] = SA;
            S = SA + bm_slices(n_docs, target);
        }
        q_S[q] = S;
        q_item0[q] = nq + rest - 1;
        items[q] = make_int2(q, 0);
        for (int s = 1; s < S; ++s) items[nq + rest + s - 1] = make_int2(q, s);
        rest += S - 1;
    }
    if (threadIdx.x == 0) {
        ctl[CTL_ITEMS] = total;
        ctl[CTL_TARGET_A] = (int)(target_a > 0x7fffffff ? 0x7fffffff : target_a);   // (what a stage-A slice was aimed at)
    }
}

__global__ __launch_bounds__(256) void bm25_edges_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ post_doc,
    const int32_t* __restrict__ ctl, const int32_t* __restrict__ q_nt,
    const int32_t* __restrict__ q_S, const int32_t* __restrict__ q_SA, const int32_t* __restrict__ q_long,
    const int32_t* __restrict__ q_terms, const int2* __restrict__ items, int mt,
    const int32_t* __restrict__ q_pmask, int64_t n_docs, int32_t* __restrict__ ipos,
    const double* __restrict__ idf, const double* __restrict__ term_ub, const int32_t* __restrict__ dense_slot,
    int64_t dense_stride, const int32_t* __restrict__ query_coll, WwItem* __restrict__ wrec,
    WwTerm* __restrict__ wterm) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int item = (int)(g / mt), slot = (int)(g % mt);
    if (item >= ctl[CTL_ITEMS]) return;
    const int2 it = items[item];
    const int q = it.x;
    if (wrec && slot == 0) {
        WwItem r;
        r.q = q; r.sl = it.y; r.SA = q_SA[q]; r.S = q_S[q]; r.nt = q_nt[q]; r.pm = q_pmask[q] & 0xFF;
        r.qc = query_coll ? query_coll[q] : -1; r.pad = 0;
        wrec[item] = r;
    }
    if (slot >= q_nt[q]) return;
    const int term = q_terms[(int64_t)q * mt + slot];
    const int64_t lo = rowptr[term];
    const int full = (int)(rowptr[term + 1] - lo);
    int start = 0, end = full;
    const int SA = q_SA[q];      // -1: an ordinary query; else its first SA slices are stage A
    int S = q_S[q], s = it.y;
    const bool sweep = SA >= 0 && s >= SA;
    if (SA >= 0) {
        if (sweep) s -= SA, S -= SA; else S = SA;
    }
    if (SA >= 0 && ((q_pmask[q] >> slot) & 1)) {
        start = end = 0;         // a probed term is read from its per-doc rows
    } else if (sweep) {
        // stage B: slice s is the doc range [bm_window_edge(s), bm_window_edge(s + 1))
        if (S > 1) {
            start = count_below(post_doc + lo, full, bm_window_edge(n_docs, s, S));
            end = count_below(post_doc + lo, full, bm_window_edge(n_docs, s + 1, S));
        }
    } else if (S > 1) {
        const int L = q_long[q];   // (stage A: the longest of the other terms' lists)
        const int tl = q_terms[(int64_t)q * mt + L];
        const int64_t lo_l = rowptr[tl], len_l = rowptr[tl + 1] - lo_l;
        // edge e of S: the (len * e / S)-th doc of the longest list (S > 1 only with > BM_TARGET_MIN
        // postings: len_l >= 256 > S, the edges are distinct)
        auto edge = [&](int e) -> int {
            if (e == 0) return 0;
            if (e == S) return full;
            const int64_t p = len_l * e / S;
            return slot == L ? (int)p : count_below(post_doc + lo, full, (int64_t)post_doc[lo_l + p]);
        };
        start = edge(s);
        end = edge(s + 1);
    }
    ipos[((int64_t)item * mt + slot) * 2] = start;
    ipos[((int64_t)item * mt + slot) * 2 + 1] = end;
    if (wterm && slot < 8 && SA >= 0 && !sweep) {
        const bool probed = (q_pmask[q] >> slot) & 1;
        WwTerm t;
        t.lo = lo + start;
        t.idf = idf[term];
        t.ub = term_ub[term];
        t.row = probed ? (int64_t)dense_slot[term] * dense_stride : -1;
        t.len = probed ? 0 : end - start;
        t.pad = 0;
        wterm[(int64_t)item * 8 + slot] = t;
    }
}

// Between stage A and stage B: the sweeps that are still needed.  The docs of a sweep hold none of
// the query's other terms, so a score there is at most the sum of the dense terms' bounds (added
// out of order: hence the margin); stage A is complete, and when that sum stays below its
// threshold no doc of the sweep can enter the top-k -- the query's sweep slices are closed with
// empty lists.  The others are listed for bm25_window_kernel SLICE-MAJOR: the first slice of every
// sweeping query, then the second of every one, ... -- the workgroups of the persistent grid then
// start on different queries, and a query's later slices find the threshold its first one has
// published (query-major, the first 512 items were the six slices of 85 queries, all started
// together and all without a threshold: every doc of their first windows scored in full).
// One workgroup: rank of a query among the sweeping ones by a block scan, no atomics, a
// deterministic list.
constexpr int FILTER_THREADS = 1024;
__global__ __launch_bounds__(FILTER_THREADS) void bm25_sweep_filter_kernel(
    int32_t* __restrict__ ctl, int nq, const int32_t* __restrict__ q_S, const int32_t* __restrict__ q_SA,
    const int32_t* __restrict__ q_item0, const double* __restrict__ q_dub,
    const unsigned long long* __restrict__ theta_glob, int32_t* __restrict__ slice_cnt,
    int32_t* __restrict__ sweep_items) {
    __shared__ int red[FILTER_THREADS];
    const int per = (nq + FILTER_THREADS - 1) / FILTER_THREADS;
    const int q0 = (int)threadIdx.x * per < nq ? (int)threadIdx.x * per : nq;
    const int q1 = q0 + per < nq ? q0 + per : nq;
    auto item_of = [&](int q, int s) -> int { return s == 0 ? q : q_item0[q] + s; };
    auto sweeps = [&](int q) -> bool {   // (and closes the slices of a sweep that is ruled out)
        const int SA = q_SA[q];
        if (SA < 0 || SA == q_S[q]) return false;   // not split / walked by waves without a stage B
        const unsigned long long g = theta_glob[q];
        if (g && q_dub[q] * (1.0 + 1e-12) < dkey_inv(g)) {
            // (a threshold exists: the query has stage-A slices, the lists are merged)
            for (int s = SA; s < q_S[q]; ++s) slice_cnt[item_of(q, s)] = 0;
            return false;
        }
        return true;
    };
    int mine = 0;
    unsigned long long live = 0ull;   // (per <= 64 for batches of up to 65536 queries; beyond, recomputed)
    for (int q = q0; q < q1; ++q)
        if (sweeps(q)) {
            ++mine;
            if (q - q0 < 64) live |= 1ull << (q - q0);
        }
    red[threadIdx.x] = mine;
    __syncthreads();
    for (int o = 1; o < FILTER_THREADS; o <<= 1) {
        const int v = (int)threadIdx.x >= o ? red[threadIdx.x - o] : 0;
        __syncthreads();
        red[threadIdx.x] += v;
        __syncthreads();
    }
    const int n_sw = red[FILTER_THREADS - 1];
    int rank = red[threadIdx.x] - mine;
    int n_items = 0;
    for (int q = q0; q < q1; ++q) {
        const bool on = q - q0 < 64 ? ((live >> (q - q0)) & 1ull) != 0ull : sweeps(q);
        if (!on) continue;
        const int SA = q_SA[q], SB = q_S[q] - SA;   // (SB is the same for every query of a batch)
        for (int s = 0; s < SB; ++s) sweep_items[(int64_t)s * n_sw + rank] = item_of(q, SA + s);
        n_items = SB;
        ++rank;
    }
    // the number of sweep items: n_sw * SB (any thread with a sweeping query knows SB)
    if (n_items && red[threadIdx.x] == n_sw && mine > 0) ctl[CTL_SWEEPS] = n_sw * n_items;   // (the last thread that holds one)
}

// The best k of a sliced query's per-slice lists (order: score desc, id asc -- the slices hold
// disjoint docs, so there are no duplicates to resolve).
constexpr int BMM_THREADS = 256, BMM_CAP = 512;
__global__ __launch_bounds__(BMM_THREADS) void bm25_merge_kernel(
    const int32_t* __restrict__ q_S, const int32_t* __restrict__ q_item0,
    const double* __restrict__ slice_s, const int64_t* __restrict__ slice_id,
    const int32_t* __restrict__ slice_cnt, int k, double* __restrict__ out_s,
    int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt) {
    static_assert(BMM_CAP >= THR_TOPK_MAX + BMM_THREADS, "merge buffer");
    __shared__ double b_s[BMM_CAP];
    __shared__ int64_t b_id[BMM_CAP];
    __shared__ int b_cnt;
    __shared__ double th_s;
    __shared__ int64_t th_id;
    const int q = blockIdx.x;
    const int S = q_S[q];
    if (S == 1) return;   // written by the item itself
    const int item0 = q_item0[q];
    BlockTopK<BMM_CAP, BMM_THREADS> tk;
    tk.init(b_s, b_id, &b_cnt, &th_s, &th_id, k);
    for (int base = 0; base < S * k; base += BMM_THREADS) {
        const int idx = base + threadIdx.x;
        const int sl = idx / k, j = idx - sl * k;
        const int item = sl == 0 ? q : item0 + sl;   // (slice 0 is item q: bm25_plan_kernel)
        const bool ok = sl < S && j < slice_cnt[item];
        double sc = 0.0;
        int64_t id = 0;
        if (ok) {
            sc = slice_s[(int64_t)item * k + j];
            id = slice_id[(int64_t)item * k + j];
        }
        tk.push(ok, sc, id);
    }
    const int n = tk.finish();
    for (int i = threadIdx.x; i < k; i += BMM_THREADS) {
        out_s[(int64_t)q * k + i] = i < n ? b_s[i] : -INFINITY;
        out_id[(int64_t)q * k + i] = i < n ? b_id[i] : -1;
    }
    if (threadIdx.x == 0) out_cnt[q] = n;
}

void bm_launch_plan(const BmIndex& X, const BmBatch& B, const BmLayout& L, int n_slots, int wave_slots) {
    int plan_blocks = (B.n_queries + PLAN_THREADS - 1) / PLAN_THREADS;
    plan_blocks = plan_blocks > PLAN_MAX_BLOCKS ? PLAN_MAX_BLOCKS : plan_blocks;
    hipLaunchKernelGGL(bm25_plan_kernel, dim3(plan_blocks), dim3(PLAN_THREADS), 0, B.st, X.rowptr, X.n_vocab,
                       B.query_terms, B.n_queries, B.max_terms, L.cap_base, L.cap_wave, B.conjunctive, n_slots,
                       BM_TARGET0, wave_slots, B.wave ? 1 : 0, B.walk_div, X.dense_slot, X.term_ub, X.n_docs, L.ctl,
                       L.q_tot, L.q_dub, L.q_nt, L.q_S, L.q_SA, L.q_pmask, L.q_item0, L.q_long, L.q_terms, L.items);
    const int64_t edge_threads = (int64_t)L.cap * B.max_terms;
    hipLaunchKernelGGL(bm25_edges_kernel, dim3((unsigned)((edge_threads + 255) / 256)), dim3(256), 0, B.st,
                       X.rowptr, X.post_doc, L.ctl, L.q_nt, L.q_S, L.q_SA, L.q_long, L.q_terms, L.items, B.max_terms,
                       L.q_pmask, X.n_docs, L.ipos, X.idf, X.term_ub, X.dense_slot, X.dense_stride, B.query_coll,
                       B.wave ? L.wrec : (WwItem*)nullptr, B.wave ? L.wterm : (WwTerm*)nullptr);
}

void bm_launch_sweep_filter(const BmBatch& B, const BmLayout& L) {
    hipLaunchKernelGGL(bm25_sweep_filter_kernel, dim3(1), dim3(FILTER_THREADS), 0, B.st, L.ctl, B.n_queries, L.q_S,
                       L.q_SA, L.q_item0, L.q_dub, L.theta, L.slice_cnt, L.sweep_items);
}

void bm_launch_merge(const BmBatch& B, const BmLayout& L) {
    hipLaunchKernelGGL(bm25_merge_kernel, dim3(B.n_queries), dim3(BMM_THREADS), 0, B.st, L.q_S, L.q_item0,
                       L.slice_s, L.slice_id, L.slice_cnt, B.k, B.out_s, B.out_id, B.out_cnt);
}

}  // namespace thr
