// BM25 workgroup walk: bm25_topk_kernel, a workgroup per work item -- ordinary items, and stage A of
// the queries with dense terms when the wave walk does not take it.
#include "bm25_common.hpp"

namespace thr {

// Block shapes (template arguments of bm25_topk_kernel):
//   BM_THREADS  threads per query
//   BM_STAGE    doc ids staged in LDS per doc-range pass
//   BM_WINDOW   doc slots of the mask path (BM_STAGE <= 3 * BM_WINDOW: the survivor list shares it)
//   BM_CAP      BlockTopK buffer (>= k + BM_THREADS)

// An item's postings are consumed in DOC-RANGE passes.  A pass stages, from every term's list,
// the next quota_t postings (quotas proportional to what is left of each list, together one LDS
// stage), then takes d_hi = the smallest "last staged doc + 1" among the lists that have more
// postings behind their quota: every posting with doc < d_hi of EVERY list is then on chip, so a
// doc's postings all fall into the same pass and the owner search never leaves LDS, whatever
// the length of the lists.  The postings with doc >= d_hi stay for the next pass and are staged
// again.
//
// WAND-style pruning (exact): passes visit the docs in ascending id order, so once k docs have
// been scored every later doc of the item has to BEAT the item's k-th best score theta (a tie
// loses on the id); against the threshold shared by the query's other slices (th_glob, whose
// docs may have larger ids) a doc is dropped only when its bound is strictly BELOW it.  Phase 1
// of a pass is LDS-only: it learns from the staged doc ids which query terms hold a doc and sums
// their term_ub in query-term order; rounding is monotone, so fl(sum of bounds) >= fl(sum of
// contributions).  The survivors are compacted into an LDS list; phase 2 walks that list a
// workgroup's width at a time: tighter block_ub check, collection filter, term-frequency /
// doc-length gathers, float64 score, top-k push.
//
// Phase 1 has three forms.  DENSE lists: every staged posting ORs its term's bit into the
// doc's slot of a mask array -- O(1) per posting -- and the non-empty slots are the candidate
// docs.  The mask holds 8 bits per doc for queries of <= 8 terms (4 BM_WINDOW docs), 32 bits
// otherwise; a pass whose staged range is wider than the mask is CUT to the mask's width when
// that still consumes at least an eighth of the staged postings (so stop-word lists always
// take this path).  SPARSE lists: a Bloom bit per (list, doc) answers "is this doc in another
// list" with one LDS read; singletons are scored (or dropped on term_ub) at once, the others
// are searched from a dense work list.  In between, with a threshold: owners and bounds by
// binary search in LDS.

// DPM: 0 = ordinary queries only, 1 = stage-A slices only, 2 = both kinds in one launch (decided per item)
template <int BM_THREADS, int BM_STAGE, int BM_WINDOW, int BM_CAP, int DPM>
__global__ __launch_bounds__(BM_THREADS, 4) void bm25_topk_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ post_doc,
    const int32_t* __restrict__ post_tf, const float* __restrict__ doclen,
    const double* __restrict__ idf, const double* __restrict__ term_ub,
    const double* __restrict__ block_ub, const uint8_t* __restrict__ post_imp,
    const int32_t* __restrict__ dense_slot, const uint16_t* __restrict__ dense_tf, int64_t dense_stride,
    double avgdl, double k1, double b,
    double imp_unit /* (k1 + 1) / 255 */, double imp_per_unit /* 255 / (k1 + 1): the host's divisions, same bits */,
    int64_t id_base, int max_terms, int k, int conjunctive, const int32_t* __restrict__ doc_coll,
    const int32_t* __restrict__ query_coll, int n_queries, int fuse_div, int32_t* __restrict__ ctl,
    const int32_t* __restrict__ q_nt, const int32_t* __restrict__ q_S, const int32_t* __restrict__ q_SA,
    const int32_t* __restrict__ q_pmask,
    const int32_t* __restrict__ q_terms, const int2* __restrict__ items,
    const int32_t* __restrict__ ipos, unsigned long long* __restrict__ theta_glob,
    double* __restrict__ slice_s, int64_t* __restrict__ slice_id, int32_t* __restrict__ slice_cnt,
    double* __restrict__ out_s, int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt
#ifdef BM_STAMPS
    , unsigned long long* __restrict__ stamps, unsigned long long* __restrict__ walk_log
#endif
    ) {
#ifdef BM_STAMPS
    unsigned long long stamp_acc[BM_NSTAMP] = {0};
    unsigned long long stamp_last = __builtin_readcyclecounter(), stamp_items = 0;
#endif
    __shared__ TermRange tr[THR_BM25_MAX_TERMS];   // .sub = postings of this pass, .lds_off = where staged
    __shared__ double t_idf[THR_BM25_MAX_TERMS], t_ub[THR_BM25_MAX_TERMS];
    __shared__ int t_staged[THR_BM25_MAX_TERMS];   // postings of the term staged in this pass
    __shared__ int t_subwin[THR_BM25_MAX_TERMS];   // ... of them inside the mask window
    __shared__ int t_prefix[THR_BM25_MAX_TERMS + 1];
    // DP (stage A of a query with dense terms): those terms have no postings here; their per-doc
    // rows are probed when a doc is scored, their bounds are added to every doc's bound
    __shared__ int64_t t_row[8];    // dense term: offset of its per-doc row; else -1
    __shared__ double p_dub;        // sum of the dense terms' term_ub
    __shared__ int p_dmaxq;         // ... of their largest quantised impacts, in accumulator units
    __shared__ int t_w[8];          // accumulator path: integer weight of a term's quantised impacts
    __shared__ double acc_scale;    // ... accumulated bound = acc_scale * (real bound), rounded up
    __shared__ int p_acc, p_thq;    // this pass takes the accumulator path; its threshold in acc units
    __shared__ int remaining, last_compact, n_surv, n_single, p_boot_q, cur_item;
    __shared__ int t_order[THR_BM25_MAX_TERMS];   // terms by descending term_ub
    __shared__ int64_t d_hi, d_lo, p_last;
    __shared__ double th_glob;
    __shared__ double b_s[BM_CAP];
    __shared__ int64_t b_id[BM_CAP];
    __shared__ int b_cnt;
    __shared__ double th_s;
    __shared__ int64_t th_id;
    __shared__ int32_t st_doc[BM_STAGE];
    // mask path: BM_WINDOW mask words (which query terms hold doc d_lo + slot; 1 or 4 slots per
    // word) + up to BM_WINDOW surviving slots behind them; search path: up to BM_STAGE surviving
    // staged indices; Bloom path: the bits + a work list.  One 24 KiB buffer.
    // accumulator path: ACC_WORDS words of two 16-bit doc accumulators, the survivor slots behind them
    constexpr int ACC_WORDS = BM_WINDOW, ACC_SLOTS = 2 * ACC_WORDS;   // (a wider window was measured: no gain)
    // survivor slots of a scan: SURV_CAP 16-bit entries behind the masks / accumulators (with a
    // threshold a window has ~100 survivors; a scan that finds more is redone SURV_CAP slots at a time)
    constexpr int SURV_CAP = BM_WINDOW;
    constexpr int SCR_WORDS = ACC_WORDS + SURV_CAP / 2;
    __shared__ uint32_t scratch[SCR_WORDS];
    static_assert(sizeof(uint32_t) * SCR_WORDS >= sizeof(uint16_t) * BM_STAGE, "survivor list of the search path must fit");
    static_assert(BM_CAP >= THR_TOPK_MAX + BM_THREADS && BM_STAGE <= 65536, "top-k buffer / 16-bit staged indices");
    static_assert(4 * BM_WINDOW <= 65536, "16-bit slot indices");
    uint32_t* mask = scratch;

    const int n_items = ctl[CTL_ITEMS];
    {   // Which launches work is decided on the device (no host round trip): when at least 1/fuse_div of
        // the batch's queries hold dense terms, ONE launch (DPM 2) takes the ordinary items and the
        // stage-A slices together -- two half-empty persistent grids, each with its own tail, cost
        // more than the row probes' registers cost the ordinary items (256 / 2048 survey queries:
        // 0.85 -> 0.60 / 1.83 -> 1.55 ms; a batch without dense terms: 0.49 -> 0.55 ms, hence the switch).
        // (fuse_div < 0: wave mode -- the waves took every OR query of <= 8 terms; this launch has the
        // rest, and nothing to do at all when the plan counted none)
        if (fuse_div < 0 && ctl[CTL_BLOCK_Q] == 0) return;
        const int nd = ctl[CTL_DENSE_Q];
        const bool fuse = fuse_div > 0 && nd > 0 && (long long)nd * fuse_div >= n_queries;
        if (DPM == 2 ? !fuse : DPM == 1 ? (fuse || nd == 0) : fuse) return;
    }
    BlockTopK<BM_CAP, BM_THREADS> tk;
    for (;;) {
        __syncthreads();   // the previous item's LDS state is no longer read
        if (threadIdx.x == 0) cur_item = atomicAdd(&ctl[DPM == 1 ? CTL_NEXT_A : CTL_NEXT_BLOCK], 1);
        __syncthreads();
        const int item = cur_item;
        if (item >= n_items) break;   // (uniform: every workgroup of the grid ends here)
#ifdef BM_STAMPS
        const unsigned long long item_t0 = __builtin_readcyclecounter();
        int item_passes = 0;
#endif
        const int2 it = items[item];
        const int q = it.x, sl = it.y;
        // a query with dense terms: its first q_SA slices are stage A's (DP), the rest bm25_window_kernel's
        const int SA_ = q_SA[q];
        if (DPM == 0 ? SA_ >= 0 : DPM == 1 ? !(SA_ >= 0 && sl < SA_) : (SA_ >= 0 && sl >= SA_)) continue;
        const bool DP = DPM == 1 || (DPM == 2 && SA_ >= 0);
        const int S = q_S[q];
        const int nt = q_nt[q];
        const int qc = query_coll ? query_coll[q] : -1;   // -1: no collection filter
        // 8 mask bits per doc for queries of <= 8 terms: 4 docs per mask word
        const int ms = nt <= 8 ? 2 : 0;
        const int spw = 1 << ms;
        const int64_t WIN = (int64_t)BM_WINDOW << ms;
        if ((int)threadIdx.x < nt) {
            const int slot = threadIdx.x;
            const int term = q_terms[(int64_t)q * max_terms + slot];
            const int64_t lo = rowptr[term];
            const int full = (int)(rowptr[term + 1] - lo);
            const int start = ipos[((int64_t)item * max_terms + slot) * 2];
            const int end = ipos[((int64_t)item * max_terms + slot) * 2 + 1];
            tr[slot].lo = lo + start;
            tr[slot].len = end - start;
            tr[slot].cur = 0;
            t_idf[slot] = idf[term];
            t_ub[slot] = term_ub ? term_ub[term] : INFINITY;
            if (DP && slot < 8) {
                const bool probed = (q_pmask[q] >> slot) & 1;
                t_row[slot] = probed ? (int64_t)dense_slot[term] * dense_stride : -1;   // (its slice is empty: bm25_edges_kernel)
            }
        }
        BM_STAMP(0);
        if (threadIdx.x == 0) {
            last_compact = 0;
            const unsigned long long g0 = S > 1 ? __hip_atomic_load(&theta_glob[q], __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            th_glob = g0 ? dkey_inv(g0) : -INFINITY;
        }
        tk.init(b_s, b_id, &b_cnt, &th_s, &th_id, k);  // includes a barrier
        // Accumulator path (queries of <= 8 terms, OR form, impacts given): a doc's bound is the
        // sum over its postings of idf_t * impact_q * (k1+1)/255, accumulated in 16 bits per doc
        // slot as integers imp_q * w_t with w_t = ceil(idf_t * (k1+1)/255 * scale), scale chosen so
        // that the weights add up to <= 256 (255 * 256 < 2^16: a slot cannot overflow into its
        // neighbour).  It is an upper bound of the doc's score to within 1e-15, far tighter than
        // the sum of the per-term maxima: ~1 % of the docs of a stop-word query survive it
        // instead of ~16 %.
        const bool acc_ok = post_imp != nullptr && !conjunctive && nt >= 1 && nt <= 8;
        if (threadIdx.x == 0) {
            int total = 0;
            for (int t = 0; t < nt; ++t) total += tr[t].len;
            remaining = total;
            for (int t = 0; t < nt; ++t) t_order[t] = t;
            for (int a = 1; a < nt; ++a) {   // (insertion sort, <= 32 terms)
                const int ta = t_order[a];
                int c = a;
                for (; c > 0 && t_ub[t_order[c - 1]] < t_ub[ta]; --c) t_order[c] = t_order[c - 1];
                t_order[c] = ta;
            }
            if (acc_ok) {
                const double c = imp_unit;
                double sum = 0.0;
                for (int t = 0; t < nt; ++t) sum += t_idf[t] * c;
                const double scale = 248.0 / sum;
                for (int t = 0; t < nt; ++t) {
                    int w = (int)ceil(t_idf[t] * c * scale);
                    t_w[t] = w < 1 ? 1 : w;
                }
                acc_scale = scale;
            }
            if (DP) {
                double dub = 0.0;
                int dmaxq = 0;
                for (int t = 0; t < nt; ++t) {
                    if (t_row[t] < 0) continue;
                    dub += t_ub[t];
                    // the term's largest quantised impact: its bound / idf in steps of (k1+1)/255, as bm25_bounds_kernel rounds
                    const double im = t_idf[t] > 0.0 ? ceil(t_ub[t] / t_idf[t] * imp_per_unit) + 1.0 : 255.0;
                    dmaxq += t_w[t] * (im > 255.0 || !(im >= 0.0) ? 255 : (int)im);
                }
                p_dub = dub;
                p_dmaxq = dmaxq;
            }
        }
        __syncthreads();
        BM_STAMP(1);

        while (remaining > 0) {
#ifdef BM_STAMPS
            ++item_passes;
#endif
            // ---- quotas: the stage is shared out in proportion to what is left of each list ----
            if (threadIdx.x == 0) {
                // (th_glob: read at the item's start and again in every staging interval -- the load
                // of the other slices' threshold travels WITH the staging loads, it is never a round
                // trip of its own on the pass's critical path)
                const unsigned long long g = th_glob > -INFINITY ? 1ull : 0ull;
                // no threshold anywhere yet and a long way to go: a short first pass gets one cheaply
                // (without a threshold every staged doc is scored in full)
                // (sliced items only: an unsliced query is at most three passes long)
                const bool warm = g != 0ull || (b_cnt >= k && th_s > -INFINITY) || remaining <= BM_STAGE || S == 1;
                // with a threshold to hold them against, the pass accumulates per-doc impact bounds
                // (2 * BM_WINDOW 16-bit slots); without one every doc is scored anyway: the mask
                const bool have_th = g != 0ull || (b_cnt >= k && th_s > -INFINITY);
                p_acc = acc_ok && have_th ? 1 : 0;
                if (p_acc) {
                    double th = (b_cnt >= k && th_s > -INFINITY) ? th_s : -INFINITY;
                    th = th_glob > th ? th_glob : th;
                    // prune only what is below the threshold by more than the arithmetic's slack
                    const double tq = floor(th * acc_scale * (1.0 - 1e-12));
                    p_thq = tq < 0.0 ? 0 : tq > 70000.0 ? 70000 : (int)tq;
                }
                const int stage = warm ? BM_STAGE : BM_STAGE / 4;
                int off = 0;
                const int spare = stage - 32 * nt;   // every list gets at least 32 slots
                for (int t = 0; t < nt; ++t) {
                    const int rem = tr[t].len - tr[t].cur;
                    int quota = 32 + (int)((int64_t)spare * rem / remaining);
                    quota = quota < rem ? quota : rem;
                    tr[t].lds_off = off;
                    t_staged[t] = quota;
                    off += quota;
                }
                d_hi = INT64_MAX;
                d_lo = INT64_MAX;
            }
            __syncthreads();
            BM_STAMP(2);
            unsigned long long gth = 0ull;
            if (threadIdx.x == 0 && S > 1)
                gth = __hip_atomic_load(&theta_glob[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int t = 0; t < nt; ++t) {
                const int32_t* src = post_doc + tr[t].lo + tr[t].cur;
                int32_t* dst = st_doc + tr[t].lds_off;
                // (a variant that puts a term's 16 loads per thread in flight before the first LDS
                // store was A/B-measured on one box: 5 % slower -- the registers it holds cost more)
                for (int i = threadIdx.x; i < t_staged[t]; i += BM_THREADS) dst[i] = src[i];
            }
            if (threadIdx.x == 0 && S > 1) th_glob = gth ? dkey_inv(gth) : -INFINITY;
            __syncthreads();
            BM_STAMP(3);
            if ((int)threadIdx.x < nt) {
                const int t = threadIdx.x;
                if (t_staged[t] > 0 && tr[t].cur + t_staged[t] < tr[t].len)   // more postings behind the quota
                    atomicMin((unsigned long long*)&d_hi,
                              (unsigned long long)((int64_t)st_doc[tr[t].lds_off + t_staged[t] - 1] + 1));
                if (t_staged[t] > 0)
                    atomicMin((unsigned long long*)&d_lo, (unsigned long long)st_doc[tr[t].lds_off]);
            }
            __syncthreads();
            if ((int)threadIdx.x < nt) {
                TermRange& r = tr[threadIdx.x];
                const int stg = t_staged[threadIdx.x];
                r.sub = d_hi == INT64_MAX ? stg : count_below(st_doc + r.lds_off, stg, d_hi);
                const int64_t win = p_acc ? (int64_t)ACC_SLOTS : WIN;
                const int64_t dw = d_lo + win < d_hi ? d_lo + win : d_hi;
                t_subwin[threadIdx.x] = dw == INT64_MAX ? stg : count_below(st_doc + r.lds_off, stg, dw);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int total = 0, totw = 0;
                int64_t last = 0;
                for (int t = 0; t < nt; ++t) {
                    total += tr[t].sub;
                    totw += t_subwin[t];
                    if (tr[t].sub > 0) {
                        const int64_t e = (int64_t)st_doc[tr[t].lds_off + tr[t].sub - 1] + 1;
                        last = e > last ? e : last;
                    }
                }
                // wider than the mask, but the mask's width holds a fair share of the staged
                // postings: cut the pass to that width (the rest is staged again)
                if (total > 0 && last - d_lo > (p_acc ? (int64_t)ACC_SLOTS : WIN) && (int64_t)totw * 8 >= total) {
                    total = 0;
                    last = 0;
                    for (int t = 0; t < nt; ++t) {
                        tr[t].sub = t_subwin[t];
                        total += tr[t].sub;
                        if (tr[t].sub > 0) {
                            const int64_t e = (int64_t)st_doc[tr[t].lds_off + tr[t].sub - 1] + 1;
                            last = e > last ? e : last;
                        }
                    }
                }
                int acc = 0;
                for (int t = 0; t < nt; ++t) {
                    t_prefix[t] = acc;
                    acc += tr[t].sub;
                }
                t_prefix[nt] = acc;
                p_last = last;   // one past the last doc of the pass
                n_surv = 0;
                n_single = 0;
                p_boot_q = 0;
            }
            __syncthreads();
            BM_STAMP(4);
            const int total = t_prefix[nt];
            const double thg = th_glob;                 // the query's other slices' threshold (or -inf)
            const bool have_local = b_cnt >= k && th_s > -INFINITY;
            const double theta = have_local ? th_s : -INFINITY;
            const bool have_theta = have_local || thg > -INFINITY;
            // (a bound ub cannot make the top-k: it does not beat this item's threshold, or it is
            // below the threshold of the query's other slices)
            // (DP: plus the dense terms' bounds -- added out of query-term order, so with a margin far
            // above the rounding of an 8-term sum and far below anything that matters for pruning)
            const double dub = DP ? p_dub : 0.0;
            auto pruned = [&](double ub) -> bool {
                if (DP) ub = (ub + dub) * (1.0 + 1e-12);
                return !(ub > theta) || ub < thg;
            };
            // a dense term's contribution to doc d (DP), 0 when the doc does not hold it
            auto dense_add = [&](int e, int32_t d, double dl, double& score) {
                const int tfd = (int)dense_tf[t_row[e] + d];
                if (tfd > 0) score = __dadd_rn(score, bm25_contrib(t_idf[e], (double)tfd, dl, avgdl, k1, b));
            };
            auto push = [&](bool ok, double sc, int64_t d) { tk.push(ok && !(sc < thg), sc, d); };
            const int64_t last = p_last;
            const int64_t first = d_lo;
            const bool use_acc = p_acc != 0;
            const bool masked = total > 0 && last - first <= (use_acc ? (int64_t)ACC_SLOTS : WIN);
            const uint32_t thq = (uint32_t)p_thq;
            const uint32_t dmaxq = DP ? (uint32_t)p_dmaxq : 0u;
            uint16_t* surv = reinterpret_cast<uint16_t*>(masked ? scratch + ACC_WORDS : scratch);   // (ACC_WORDS == BM_WINDOW)
            auto slot_mask = [&](int slot) -> uint32_t {
                const uint32_t v = mask[slot >> ms];
                return ms ? (v >> ((slot & 3) << 3)) & 0xFFu : v;
            };

            // ---- phase 2: the survivors, densely ----
            // survivors are staged indices of owner postings (mode 0), doc slots of the mask (1) or doc
            // slots of the accumulators (2: which terms hold the doc is not known, every list is searched)
            auto phase2 = [&](int mode, int ns) {
                for (int base = 0; base < ns; base += BM_THREADS) {
                    const int j = base + threadIdx.x;
                    bool keep = j < ns;
                    double score = 0.0;
                    int32_t d = 0;
                    if (keep) {
                        int t = 0, at;
                        uint32_t has = 0xFFFFFFFFu;   // terms that may hold the doc
                        if (mode == 2) {
                            d = (int32_t)(first + surv[j]);
                            at = 0;
                        } else if (mode == 1) {   // survivor = doc slot: owner = lowest term bit, position searched
                            d = (int32_t)(first + surv[j]);
                            has = slot_mask(surv[j]);
                            t = __ffs((int)has) - 1;
                            at = tr[t].lds_off + find_doc(st_doc + tr[t].lds_off, tr[t].sub, d);
                        } else {        // survivor = staged index of the owner posting
                            at = surv[j];
                            while (t + 1 < nt && at >= tr[t + 1].lds_off) ++t;   // lds_off ascends with t
                            d = st_doc[at];
                        }
                        // staged position of the doc in every term that holds it (first 8 terms in
                        // registers -- static indexing only --, the rest searched again when needed)
                        int wf[8];
                        if (mode == 2 && nt <= 4) {
                            // the (up to four) lower-bound searches advance in lockstep, branch-free: four
                            // independent LDS reads per step instead of four chains one after the other
                            int lo_[4], hi_[4], base_[4];
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                lo_[e] = 0;
                                hi_[e] = e < nt ? tr[e].sub : 0;
                                base_[e] = e < nt ? tr[e].lds_off : 0;
                            }
                            int span = 0;
#pragma unroll
                            for (int e = 0; e < 4; ++e) span = hi_[e] > span ? hi_[e] : span;
#pragma unroll 1
                            for (; span > 0; span >>= 1) {
                                int mid[4];
                                int32_t v[4];
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    mid[e] = (lo_[e] + hi_[e]) >> 1;
                                    v[e] = st_doc[base_[e] + (lo_[e] < hi_[e] ? mid[e] : 0)];
                                }
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    const bool live = lo_[e] < hi_[e], right = v[e] < d;
                                    lo_[e] = live && right ? mid[e] + 1 : lo_[e];
                                    hi_[e] = live && !right ? mid[e] : hi_[e];
                                }
                            }
#pragma unroll
                            for (int e = 0; e < 8; ++e) wf[e] = -1;
#pragma unroll
                            for (int e = 0; e < 4; ++e)   // lo = the lower bound: the doc is there iff it equals d
                                if (e < nt && lo_[e] < tr[e].sub && st_doc[base_[e] + lo_[e]] == d) wf[e] = lo_[e];
                        } else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            wf[e] = -1;
                            if (e >= t && e < nt && ((has >> e) & 1u))
                                wf[e] = (mode != 2 && e == t) ? at - tr[e].lds_off : find_doc(st_doc + tr[e].lds_off, tr[e].sub, d);
                        }
                        }
                        auto where_far = [&](int e) -> int64_t {   // e >= 8
                            if (!((has >> e) & 1u)) return -1;
                            const int f = e == t ? at - tr[e].lds_off : find_doc(st_doc + tr[e].lds_off, tr[e].sub, d);
                            return f >= 0 ? tr[e].lo + tr[e].cur + f : -1;
                        };
                        if (have_theta && block_ub && mode != 2) {   // (the impact bound is the tighter one)
                            double ub2 = 0.0;
#pragma unroll
                            for (int e = 0; e < 8; ++e)
                                if (wf[e] >= 0) ub2 = __dadd_rn(ub2, block_ub[(tr[e].lo + tr[e].cur + wf[e]) / BM_BLOCK]);
                            for (int e = 8 > t ? 8 : t; e < nt; ++e) {
                                const int64_t w = where_far(e);
                                if (w >= 0) ub2 = __dadd_rn(ub2, block_ub[w / BM_BLOCK]);
                            }
                            if (pruned(ub2)) keep = false;
                        }
                        if (keep && qc != -1 && doc_coll[d] != qc) keep = false;
                        if (keep) {
                            const double dl = (double)doclen[d];
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                if (DP && e < nt && t_row[e] >= 0) dense_add(e, d, dl, score);
                                else if (wf[e] >= 0)
                                    score = __dadd_rn(score, bm25_contrib(t_idf[e], (double)post_tf[tr[e].lo + tr[e].cur + wf[e]], dl, avgdl, k1, b));
                            }
                            for (int e = 8 > t ? 8 : t; e < nt; ++e) {
                                const int64_t w = where_far(e);
                                if (w >= 0)
                                    score = __dadd_rn(score, bm25_contrib(t_idf[e], (double)post_tf[w], dl, avgdl, k1, b));
                            }
                        }
                    }
                    push(keep, score, (int64_t)d);
                }
            };

            // ---- phase 1 (LDS only): owners, which terms hold the doc, bound against theta ----
            const bool middle = !masked && have_theta && (last - first) < 32 * (int64_t)total;
            if (masked || middle) {
                const int w = masked ? (int)(last - first) : 1;
                if (masked && use_acc) {
                    const int words = (w + 1) >> 1;   // two 16-bit accumulators per word
                    for (int i = threadIdx.x; i < words; i += BM_THREADS) mask[i] = 0u;
                    __syncthreads();
                    // term by term: everything that depends on the term is uniform (scalar registers),
                    // a posting costs one LDS read, one byte from global memory and one LDS atomic
                    for (int t = 0; t < nt; ++t) {
                        const int sub = __builtin_amdgcn_readfirstlane(tr[t].sub);
                        const int off0 = __builtin_amdgcn_readfirstlane(tr[t].lds_off);
                        const uint32_t wt = (uint32_t)__builtin_amdgcn_readfirstlane(t_w[t]);
                        // (staging the impacts in LDS with the ids -- bytes, or aligned words -- was measured:
                        // what the fill gains the staging loses)
                        const uint8_t* imp_t = post_imp + tr[t].lo + tr[t].cur;
                        for (int i0 = threadIdx.x; i0 < sub; i0 += 4 * BM_THREADS) {
                            int slot[4];
                            uint32_t val[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const int i = i0 + u * BM_THREADS;
                                slot[u] = -1;
                                if (i < sub) {
                                    slot[u] = (int)(st_doc[off0 + i] - first);
                                    val[u] = (uint32_t)imp_t[i] * wt;
                                }
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (slot[u] >= 0) atomicAdd(&mask[slot[u] >> 1], val[u] << ((slot[u] & 1) << 4));
                        }
                    }
                    __syncthreads();
                    BM_STAMP(12);
                    BM_COUNT(14, 1);
                    BM_COUNT(16, total);
                } else if (masked) {
                    const int words = (w + spw - 1) >> ms;
                    for (int i = threadIdx.x; i < words; i += BM_THREADS) mask[i] = 0u;
                    __syncthreads();
                    for (int i = threadIdx.x; i < total; i += BM_THREADS) {
                        int t = 0;
                        while (i >= t_prefix[t + 1]) ++t;
                        const int slot = (int)(st_doc[tr[t].lds_off + (i - t_prefix[t])] - first);
                        atomicOr(&mask[slot >> ms], 1u << (((slot & (spw - 1)) << 3) + t));
                    }
                    __syncthreads();
                    BM_STAMP(12);
                    BM_COUNT(15, 1);
                    BM_COUNT(16, total);
                }
                // masked: the candidate slots, BM_WINDOW slots (= the survivor list's capacity) at a
                // time; else one round over the staged postings
                // the whole window at once when its survivors fit the list (BM_WINDOW slots: they do
                // once a threshold prunes), else BM_WINDOW slots at a time
                int c_step = masked ? w : SURV_CAP;
                for (int c0 = 0; c0 < w;) {
                    const int c_next = c0 + c_step < w ? c0 + c_step : w;
                    if (masked && use_acc) {
                        const int cend = c_next;
                        for (int wd = (c0 >> 1) + (int)threadIdx.x; wd < ((cend + 1) >> 1); wd += BM_THREADS) {
                            const uint32_t v = mask[wd];
                            if (!v) continue;
#pragma unroll
                            for (int u = 0; u < 2; ++u) {
                                const uint32_t a = (v >> (u << 4)) & 0xFFFFu;
                                if (a != 0u && a + dmaxq >= thq) {
                                    const int at = atomicAdd(&n_surv, 1);
                                    if (at < SURV_CAP) surv[at] = (uint16_t)((wd << 1) + u);
                                }
                            }
                        }
                    } else if (masked) {
                        const int cend = c_next;
                        for (int wd = (c0 >> ms) + (int)threadIdx.x; wd < ((cend + spw - 1) >> ms); wd += BM_THREADS) {
                            const uint32_t v = mask[wd];
                            if (!v) continue;
                            for (int u = 0; u < spw; ++u) {
                                const uint32_t m = ms ? (v >> (u << 3)) & 0xFFu : v;
                                if (!m) continue;
                                if (conjunctive && __popc(m) < nt) continue;
                                if (have_theta) {
                                    double ub = 0.0;
                                    for (uint32_t r = m; r; r &= r - 1) ub = __dadd_rn(ub, t_ub[__ffs((int)r) - 1]);
                                    if (pruned(ub)) continue;
                                }
                                const int at = atomicAdd(&n_surv, 1);
                                if (at < SURV_CAP) surv[at] = (uint16_t)((wd << ms) + u);
                            }
                        }
                    } else {
                        // moderately dense lists and a threshold to prune with: LDS-only owner / bound
                        // search (a doc is dropped on the sum of its terms' bounds before any gather;
                        // the sweep below would find most docs shared and score them all)
                        for (int i = threadIdx.x; i < total; i += BM_THREADS) {
                            int t = 0;
                            while (i >= t_prefix[t + 1]) ++t;
                            const int off = i - t_prefix[t];
                            const int32_t d = st_doc[tr[t].lds_off + off];
                            bool owner = true;
                            for (int e = 0; e < t && owner; ++e)
                                if (find_doc(st_doc + tr[e].lds_off, tr[e].sub, d) >= 0) owner = false;
                            if (!owner) continue;
                            int present = 1;
                            double ub = __dadd_rn(0.0, t_ub[t]);
                            for (int e = t + 1; e < nt; ++e)
                                if (find_doc(st_doc + tr[e].lds_off, tr[e].sub, d) >= 0) {
                                    ++present;
                                    ub = __dadd_rn(ub, t_ub[e]);
                                }
                            if (conjunctive && present < nt) continue;
                            if (pruned(ub)) continue;
                            surv[atomicAdd(&n_surv, 1)] = (uint16_t)(tr[t].lds_off + off);
                        }
                    }
                    __syncthreads();
                    BM_STAMP(13);
                    const int ns = n_surv;
                    if (masked && ns > SURV_CAP) {   // (only with c_step == w) too many: again, chunk by chunk
                        __syncthreads();
                        if (threadIdx.x == 0) n_surv = 0;
                        __syncthreads();
                        c_step = SURV_CAP;
                        continue;
                    }
                    BM_COUNT(17, ns);
                    BM_COUNT(18, (ns + BM_THREADS - 1) / BM_THREADS);
                    phase2(masked ? (use_acc ? 2 : 1) : 0, ns);
                    __syncthreads();
                    if (threadIdx.x == 0) n_surv = 0;
                    __syncthreads();
                    BM_STAMP(5);
                    c0 = c_next;
                }
            } else {
                // sparse lists (or no threshold yet): every owner is scored in the same sweep that finds it.
                // Sparse lists share few docs, so nearly every "is this doc in list e" question is
                // answered NO: a Bloom bit per (list, doc hash) in the idle scratch buffer answers
                // those with one LDS read instead of a binary search (a chain of ~11); a set bit is
                // confirmed by the search, so the result is exact.  The doc-length and own-tf gathers
                // of the NEXT sweep step are requested before the current one is worked on.
                // bits per list: the largest power of two (<= 32768) that fits the buffer nt times next
                // to a work list that could take every posting of the pass (16 bits each)
                int bwords = 1024;
                while (bwords >= 128 && nt * bwords + (total + 1) / 2 > SCR_WORDS) bwords >>= 1;
                const bool bloom = bwords >= 128;
                const int bl2 = 31 - __clz(bwords * 32);
                if (bloom) {
                    for (int i = threadIdx.x; i < nt * bwords; i += BM_THREADS) scratch[i] = 0u;
                    __syncthreads();
                    for (int i = threadIdx.x; i < total; i += BM_THREADS) {
                        int t = 0;
                        while (i >= t_prefix[t + 1]) ++t;
                        const uint32_t h = ((uint32_t)st_doc[tr[t].lds_off + (i - t_prefix[t])] * 2654435761u) >> (32 - bl2);
                        atomicOr(&scratch[t * bwords + (h >> 5)], 1u << (h & 31));
                    }
                    __syncthreads();
                }
                BM_STAMP(6);
                auto lookup = [&](int e, int32_t d) -> int {   // index of d in list e's staged ids, or -1
                    if (bloom) {
                        const uint32_t h = ((uint32_t)d * 2654435761u) >> (32 - bl2);
                        if (!((scratch[e * bwords + (h >> 5)] >> (h & 31)) & 1u)) return -1;
                    }
                    return find_doc(st_doc + tr[e].lds_off, tr[e].sub, d);
                };
                // the searching version of "score posting (t, off) if it owns doc d"
                auto score_full = [&](int t, int off, int32_t d, float dl_own, int32_t tf_own, double& score) -> bool {
                    for (int e = 0; e < t; ++e)
                        if (lookup(e, d) >= 0) return false;
                    int present = 0;
                    int wf[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        wf[e] = -1;
                        if (e >= t && e < nt) {
                            wf[e] = e == t ? off : lookup(e, d);
                            if (wf[e] >= 0) ++present;
                        }
                    }
                    auto far = [&](int e) -> int64_t {   // terms beyond the 8th: searched when needed
                        const int f = e < t ? -1 : (e == t ? off : lookup(e, d));
                        return f >= 0 ? tr[e].lo + tr[e].cur + f : -1;
                    };
                    for (int e = 8; e < nt; ++e) present += far(e) >= 0 ? 1 : 0;
                    if (conjunctive && present < nt) return false;
                    if (qc != -1 && doc_coll[d] != qc) return false;
                    const double dl = (double)dl_own;
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        if (DP && e < nt && t_row[e] >= 0) dense_add(e, d, dl, score);
                        else if (wf[e] >= 0)
                            score = __dadd_rn(score, bm25_contrib(t_idf[e], (double)(e == t ? tf_own : post_tf[tr[e].lo + tr[e].cur + wf[e]]), dl, avgdl, k1, b));
                    }
                    for (int e = 8; e < nt; ++e) {
                        const int64_t w = far(e);
                        if (w >= 0)
                            score = __dadd_rn(score, bm25_contrib(t_idf[e], (double)(e == t ? tf_own : post_tf[w]), dl, avgdl, k1, b));
                    }
                    return true;
                };
                int n_t = 0, n_off = 0;
                int32_t n_d = 0, n_tf = 0;
                float n_dl = 0.f;
                auto fetch = [&](int i) {
                    if (i >= 0 && i < total) {
                        n_t = 0;
                        while (i >= t_prefix[n_t + 1]) ++n_t;
                        n_off = i - t_prefix[n_t];
                        n_d = st_doc[tr[n_t].lds_off + n_off];
                        n_dl = doclen[n_d];
                        n_tf = post_tf[tr[n_t].lo + tr[n_t].cur + n_off];
                    }
                };
                // With the filter, sweep 1 never searches: a posting whose doc shows in no other list's
                // bits is the doc's only posting (owner, one contribution) and is scored at once; the
                // few with a set bit -- which a wave would otherwise wait for, lane by lane -- go to a
                // work list (behind the bits in the same buffer) that sweep 2 walks densely.
                static_assert(2 * SCR_WORDS >= BM_STAGE, "work list of a pass without the filter");
                uint16_t* work = reinterpret_cast<uint16_t*>(bloom ? scratch + nt * bwords : scratch);
                // (n_surv is 0 here: it counts the work list now)
                if (bloom) {
                    // list by list: everything that depends on the term is uniform (scalar registers).
                    // Nothing is scored in this sweep: a posting that is its doc's only one is held
                    // against the threshold with its own quantised impact (plus, DP, the dense terms'
                    // largest) and, when it may enter, listed -- from the BACK of the work list's
                    // buffer, the postings to be searched from the front (together at most ``total``).
                    auto list_term = [&](int t, bool use_q, uint32_t thq_now) {
                        const int sub = __builtin_amdgcn_readfirstlane(tr[t].sub);
                        const int off0 = __builtin_amdgcn_readfirstlane(tr[t].lds_off);
                        const int pre = __builtin_amdgcn_readfirstlane(t_prefix[t]);
                        const uint32_t wt = use_q ? (uint32_t)__builtin_amdgcn_readfirstlane(t_w[t]) : 0u;
                        const uint8_t* imp_t = post_imp + tr[t].lo + tr[t].cur;
                        const double ub_t = t_ub[t];
                        const double ubx_t = DP ? (ub_t + dub) * (1.0 + 1e-12) : ub_t;
                        // (ub_t < threshold: no posting of this list can enter on its own)
                        const bool single_ok = !(conjunctive && nt > 1) && !(ubx_t < th_s) && !(ubx_t < thg);
                        for (int base = 0; base < sub; base += BM_THREADS) {
                            const int i = base + (int)threadIdx.x;
                            if (i < sub) {
                                const int32_t d = st_doc[off0 + i];
                                const uint32_t h = ((uint32_t)d * 2654435761u) >> (32 - bl2);
                                const uint32_t w = h >> 5, bit = 1u << (h & 31);
                                bool alone = true;
                                for (int e = 0; e < nt; ++e)
                                    if (e != t && (scratch[e * bwords + w] & bit)) alone = false;
                                if (!alone) {
                                    work[atomicAdd(&n_surv, 1)] = (uint16_t)(pre + i);
                                } else if (single_ok && (!use_q || (uint32_t)imp_t[i] * wt + dmaxq >= thq_now)) {
                                    work[total - 1 - atomicAdd(&n_single, 1)] = (uint16_t)(pre + i);
                                }
                            }
                        }
                    };
                    // the listed singles [from, to), densely: collection filter, gathers, score, push
                    auto score_singles = [&](int from, int to) {
                        for (int base = from; base < to; base += BM_THREADS) {
                            const int j = base + (int)threadIdx.x;
                            bool owner = j < to;
                            double score = 0.0;
                            int32_t d = 0;
                            if (owner) {
                                const int idx = work[total - 1 - j];
                                int t = 0;
                                while (idx >= t_prefix[t + 1]) ++t;
                                const int off = idx - t_prefix[t];
                                d = st_doc[tr[t].lds_off + off];
                                if (qc != -1 && doc_coll[d] != qc) owner = false;
                                if (owner) {
                                    const double dl = (double)doclen[d];
                                    const double tf_own = (double)post_tf[tr[t].lo + tr[t].cur + off];
                                    if (DP) {   // its own posting and the dense terms, in query-term order
#pragma unroll
                                        for (int e = 0; e < 8; ++e) {
                                            if (e >= nt) continue;
                                            if (t_row[e] >= 0) dense_add(e, d, dl, score);
                                            else if (e == t) score = __dadd_rn(score, bm25_contrib(t_idf[e], tf_own, dl, avgdl, k1, b));
                                        }
                                    } else {
                                        score = __dadd_rn(score, bm25_contrib(t_idf[t], tf_own, dl, avgdl, k1, b));
                                    }
                                }
                            }
                            push(owner, score, (int64_t)d);
                        }
                    };
#if defined(BM_BOOT_NONE)
                    const bool boot = false;
#elif defined(BM_BOOT_ALL)
                    const bool boot = acc_ok && !have_theta && nt > 1;
#else
                    const bool boot = !DP && acc_ok && !have_theta && nt > 1;
#endif
                    if (!boot) {
                        // (use_acc: a threshold in accumulator units exists, p_thq)
                        for (int t = 0; t < nt; ++t) list_term(t, use_acc, thq);
                        __syncthreads();
                        BM_STAMP(7);
                        BM_COUNT(19, n_single);
                        score_singles(0, n_single);
                        BM_STAMP(8);
                    } else {
                        // No threshold yet (an item's first pass -- the only one of a short query): list by
                        // list, the largest bound first, and a select after each, so that the later lists
                        // (smaller bounds: the longer ones) are held against a threshold already.
                        int done = 0;
                        for (int oi = 0; oi < nt; ++oi) {
                            list_term(t_order[oi], p_boot_q != 0, (uint32_t)p_thq);
                            __syncthreads();
                            BM_STAMP(7);
                            const int upto = n_single;
                            BM_COUNT(19, upto - done);
                            score_singles(done, upto);
                            done = upto;
                            __syncthreads();
                            BM_STAMP(8);
                            if (b_cnt >= k && b_cnt - last_compact >= 64) {
                                tk.compact();
                                if (threadIdx.x == 0) {
                                    last_compact = b_cnt;
                                    if (S > 1 && th_s > -INFINITY) atomicMax(&theta_glob[q], (unsigned long long)dkey(th_s));
                                }
                            }
                            if (threadIdx.x == 0 && b_cnt >= k && th_s > -INFINITY) {
                                const double th = th_glob > th_s ? th_glob : th_s;
                                const double tq = floor(th * acc_scale * (1.0 - 1e-12));
                                p_thq = tq < 0.0 ? 0 : tq > 70000.0 ? 70000 : (int)tq;
                                p_boot_q = 1;
                            }
                            __syncthreads();
                        }
                    }
                } else {   // no room for the bits (many terms): every posting takes the searching sweep
                    for (int i = threadIdx.x; i < total; i += BM_THREADS) work[i] = (uint16_t)i;
                    if (threadIdx.x == 0) n_surv = total;
                }
                __syncthreads();
                const int n_work = n_surv;
                fetch((int)threadIdx.x < n_work ? (int)work[threadIdx.x] : -1);
                for (int base = 0; base < n_work; base += BM_THREADS) {
                    const int j = base + threadIdx.x;
                    const int t = n_t, off = n_off;
                    const int32_t d = n_d, tf_own = n_tf;
                    const float dl_own = n_dl;
                    fetch(j + BM_THREADS < n_work ? (int)work[j + BM_THREADS] : -1);
                    bool owner = false;
                    double score = 0.0;
                    if (j < n_work) owner = score_full(t, off, d, dl_own, tf_own, score);
                    push(owner, score, (int64_t)d);
                }
            }
            BM_STAMP(9);
            __syncthreads();
            // a fresh theta pays for the select once enough docs have entered since the last one
            if (b_cnt >= k && b_cnt - last_compact >= 64) {
                tk.compact();
                if (threadIdx.x == 0) {
                    last_compact = b_cnt;
                    // a lower bound of this slice's k-th best bounds the query's k-th best from below
                    if (S > 1 && th_s > -INFINITY) atomicMax(&theta_glob[q], (unsigned long long)dkey(th_s));
                }
            }
            if (threadIdx.x == 0) {
                for (int t = 0; t < nt; ++t) tr[t].cur += tr[t].sub;
                remaining -= total;
            }
            __syncthreads();
            BM_STAMP(10);
        }
        const int n = tk.finish();
        if (S == 1) {
            for (int i = threadIdx.x; i < k; i += BM_THREADS) {
                out_s[(int64_t)q * k + i] = i < n ? b_s[i] : -INFINITY;
                out_id[(int64_t)q * k + i] = i < n ? b_id[i] + id_base : -1;
            }
            if (threadIdx.x == 0) out_cnt[q] = n;
        } else {
            for (int i = threadIdx.x; i < n; i += BM_THREADS) {
                slice_s[(int64_t)item * k + i] = b_s[i];
                slice_id[(int64_t)item * k + i] = b_id[i] + id_base;
            }
            if (threadIdx.x == 0) {
                slice_cnt[item] = n;
                if (n >= k) atomicMax(&theta_glob[q], (unsigned long long)dkey(b_s[k - 1]));
            }
        }
        BM_STAMP(11);
#ifdef BM_STAMPS
        ++stamp_items;
        if (threadIdx.x == 0 && walk_log) {
            int tot_ = 0;
            for (int t = 0; t < nt; ++t) tot_ += tr[t].len;
            walk_log[4 * (size_t)item] = ((unsigned long long)q << 32) | (unsigned)((sl << 16) | ((DP ? 1 : 0) << 8) | nt);
            walk_log[4 * (size_t)item + 1] = (unsigned long long)tot_;
            walk_log[4 * (size_t)item + 2] = __builtin_readcyclecounter() - item_t0;
            walk_log[4 * (size_t)item + 3] = (unsigned long long)item_passes;
        }
#endif
    }
#ifdef BM_STAMPS
    if (threadIdx.x == 0) {
        for (int i = 0; i < BM_NSTAMP; ++i) stamps[(int64_t)blockIdx.x * (BM_NSTAMP + 1) + i] = stamp_acc[i];
        stamps[(int64_t)blockIdx.x * (BM_NSTAMP + 1) + BM_NSTAMP] = stamp_items;
    }
#endif
}

// Block shape: 512 threads / 8192 staged ids per pass / 75 KiB of LDS, two workgroups per CU --
// a four-term query of the bench (6.7 K postings) is one pass.  THR_BM25_SHAPE=small selects
// 256 threads / 4096 ids / 39 KiB, four per CU: the fixed cost of an item (set-up, staging, the
// final sort) overlaps four ways, which wins when every list is short (2048 queries over lists
// of <= 200 postings: 0.075 ms against 0.124 ms) and loses otherwise.
using WalkKernel = decltype(&bm25_topk_kernel<512, 8192, 4096, 1024, 0>);
struct WalkShape {
    WalkKernel kernel;
    int threads;
};
template <int T, int S, int W, int C>
static WalkShape walk_shape(int dpm) {
    return {dpm == 2   ? bm25_topk_kernel<T, S, W, C, 2>
            : dpm == 1 ? bm25_topk_kernel<T, S, W, C, 1>
                       : bm25_topk_kernel<T, S, W, C, 0>,
            T};
}

void bm_launch_walk_block(const BmIndex& X, const BmBatch& B, const BmLayout& L, BmShape shape, int dpm, int grid
                          BM_STAMPS_ONLY(, unsigned long long* stamps, unsigned long long* walk_log)) {
    const WalkShape w = shape == BM_SHAPE_HUGE  ? walk_shape<1024, 16384, 8192, 2048>(dpm)   // one 16-wave workgroup per CU
                        : shape == BM_SHAPE_BIG ? walk_shape<512, 8192, 4096, 1024>(dpm)
                                                : walk_shape<256, 4096, 2048, 512>(dpm);
    hipLaunchKernelGGL(w.kernel, dim3(grid), dim3(w.threads), 0, B.st, X.rowptr, X.post_doc, X.post_tf, X.doclen,
                       X.idf, X.term_ub, X.block_ub, X.post_imp, X.dense_slot, X.dense_tf, X.dense_stride, X.avgdl,
                       X.k1, X.b, X.imp_unit, X.imp_per_unit, X.id_base, B.max_terms, B.k, B.conjunctive, B.doc_coll,
                       B.query_coll, B.n_queries, B.fuse_div, L.ctl, L.q_nt, L.q_S, L.q_SA, L.q_pmask, L.q_terms,
                       L.items, L.ipos, L.theta, L.slice_s, L.slice_id, L.slice_cnt, B.out_s, B.out_id, B.out_cnt
                       BM_STAMPS_ONLY(, stamps, walk_log));
}

}  // namespace thr
