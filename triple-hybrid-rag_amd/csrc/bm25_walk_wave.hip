// BM25 wave walk: bm25_walk_wave_kernel, a wave per work item.
#include "bm25_common.hpp"

namespace thr {

// ---------------------------------------------------------------------------------------------
// bm25_walk_wave_kernel: stage A (the walked terms of a query with probed terms) with a WAVE, not a
// workgroup, per work item.
//
// Why (round 4): the block walk above gives an item to 512 threads that run a chain of
// barrier-separated phases, each a dependent memory round trip; a stage-A item is ~3 K postings,
// its fixed latency ~60 us, two workgroups fit a CU -- the kernel's waves wait 82 % of their life
// and 40 % of its cycles are per-item latency.  The work itself is embarrassingly parallel over
// items, so the way to hide a latency chain is MORE CHAINS PER CU, not more threads per chain:
// here an item is a doc-range slice of ~1 K walked postings (the plan cuts stage A with its own,
// smaller target), ONE wave walks it without a single workgroup barrier, and sixteen waves --
// sixteen independent chains -- share a CU (10 KiB of LDS and <= 128 VGPRs per wave).
//
// Per pass (an item is one pass unless a doc-range slice came out longer than the stage):
//   stage     the next ids of every walked list into the wave's LDS (equal quotas; d_hi = the
//             smallest "last staged doc + 1" among lists with more behind: every posting below
//             d_hi of every list is on chip);
//   bits      a Bloom bit per (list, doc) when more than one list has postings;
//   classify  a posting whose doc shows in no other list's bits is its doc's only one: held against
//             the threshold with its own quantised impact + the probed terms' largest, listed when it
//             may enter; the others go to a work list;
//   score     listed singles 64 at a time: doc length, own tf, the probed terms' frequencies from
//             their rows, float64 in query-term order, wave-level top-k (128 slots, bitonic cut);
//             as soon as k docs are in, the cut gives a threshold and the classification goes on
//             with it; work-list postings find their owner and the other lists' positions by
//             binary search in LDS.
// Same arithmetic, same bounds (bm25_topk_kernel's accumulator units), same threshold sharing
// (theta_glob) and slice lists as the block walk: results are the same bits.  k <= 64.
// ---------------------------------------------------------------------------------------------
constexpr int WW_STAGE = 1024;     // doc ids a wave stages per pass
constexpr int WW_CAP = 128;        // top-k slots of a wave (k <= 64: a batch of 64 always fits after a cut)
constexpr int WW_BLOOM = 256;      // words of Bloom bits per wave, shared out among the lists with postings

struct WwLds {
    int32_t st_doc[WW_STAGE];
    uint8_t st_imp[WW_STAGE];      // the staged postings' quantised impacts (the bound test never leaves LDS)
    uint16_t list[WW_STAGE];       // singles to score from the front, postings to search from the back
    double b_s[WW_CAP];
    int32_t b_id[WW_CAP];
    uint32_t bloom[WW_BLOOM];
    int64_t t_lo[8];               // first posting of the term's slice
    int64_t t_row[8];              // probed term: offset of its per-doc row; else -1
    double t_idf[8];
    int t_len[8], t_cur[8], t_sub[8], t_off[8], t_w[8], t_stg[8], t_bs[8];
};

__device__ __forceinline__ void ww_sync() {
    // lanes of ONE wave exchange data through LDS: the hardware keeps a wave's LDS accesses in
    // order; this keeps the compiler from moving or caching them
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// descending (score, then ascending id) bitonic sort of the WW_CAP slots by one wave: two slots per lane
__device__ __forceinline__ void ww_sort(double* s, int32_t* id, int lane) {
    for (int k2 = 2; k2 <= WW_CAP; k2 <<= 1)
        for (int j = k2 >> 1; j > 0; j >>= 1) {
            const int i = ((lane & ~(j - 1)) << 1) | (lane & (j - 1)), p = i | j;
            const bool up = (i & k2) == 0;
            const double sa = s[i], sb = s[p];
            const int32_t ia = id[i], ib = id[p];
            const bool swap = up ? better(sb, (int64_t)ib, sa, (int64_t)ia) : better(sa, (int64_t)ia, sb, (int64_t)ib);
            if (swap) {
                s[i] = sb; s[p] = sa;
                id[i] = ib; id[p] = ia;
            }
            ww_sync();
        }
}

__global__ __launch_bounds__(WW_WAVES * 64, 4) void bm25_walk_wave_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ post_doc,
    const int32_t* __restrict__ post_tf, const float* __restrict__ doclen,
    const double* __restrict__ idf, const double* __restrict__ term_ub,
    const uint8_t* __restrict__ post_imp, const int32_t* __restrict__ dense_slot,
    const uint16_t* __restrict__ dense_tf, int64_t dense_stride, double avgdl, double k1, double b,
    double imp_unit /* (k1 + 1) / 255 */, double imp_per_unit /* 255 / (k1 + 1): the host's divisions, same bits */,
    int64_t id_base, int max_terms, int k, const int32_t* __restrict__ doc_coll,
    const int32_t* __restrict__ query_coll, int32_t* __restrict__ ctl,
    const int32_t* __restrict__ q_nt, const int32_t* __restrict__ q_S, const int32_t* __restrict__ q_SA,
    const int32_t* __restrict__ q_pmask, const int32_t* __restrict__ q_terms,
    const int2* __restrict__ items, const int32_t* __restrict__ ipos, const WwItem* __restrict__ wrec,
    const WwTerm* __restrict__ wterm,
    unsigned long long* __restrict__ theta_glob, double* __restrict__ slice_s,
    int64_t* __restrict__ slice_id, int32_t* __restrict__ slice_cnt, double* __restrict__ out_s,
    int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt
#ifdef BM_STAMPS
    , unsigned long long* __restrict__ wstamps
#endif
    ) {
#ifdef BM_STAMPS
    unsigned long long ws_acc[16] = {0};
    unsigned long long ws_last = __builtin_readcyclecounter();
#define WW_T(i) do { const unsigned long long now_ = __builtin_readcyclecounter(); ws_acc[i] += now_ - ws_last; ws_last = now_; } while (0)
#define WW_C(i, v) do { ws_acc[i] += (unsigned long long)(v); } while (0)
#else
#define WW_T(i)
#define WW_C(i, v)
#endif
    __shared__ WwLds lds_all[WW_WAVES];
    const int lane = threadIdx.x & 63;
    WwLds& L = lds_all[threadIdx.x >> 6];
    const int n_items = ctl[CTL_ITEMS];
    const unsigned long long lt_mask = (1ull << lane) - 1ull;
        // a wave's first item is its own number (thousands of waves bumping one counter at launch spend
    // tens of microseconds in the L2's atomic unit: an EMPTY launch took 72 us that way); the counter
    // hands out the items behind those
    const int n_waves = (int)gridDim.x * WW_WAVES;
    int item = (int)blockIdx.x * WW_WAVES + (int)(threadIdx.x >> 6);
    bool first = true;
    for (;; first = false) {
        if (!first) {
            if (lane == 0) item = atomicAdd(&ctl[CTL_NEXT_A], 1) + n_waves;
            item = __builtin_amdgcn_readfirstlane(item);
        }
        if (item >= n_items) break;
        const WwItem rec = wrec[item];
        const int q = rec.q, sl = rec.sl, SA = rec.SA;
        if (!(SA >= 0 && sl < SA)) {                    // not a stage-A slice: another kernel's item
            WW_T(7);
            continue;
        }
        const int S = rec.S, nt = rec.nt, pm = rec.pm, qc = rec.qc;
        // ---- the terms (lane t < 8), then everything uniform the passes need ----
        double scale_l = 0.0;
        int dm_l = 0;
        {
            const bool on = lane < nt && lane < 8;
            WwTerm tr_;
            tr_.lo = 0; tr_.idf = 0.0; tr_.ub = 0.0; tr_.row = -1; tr_.len = 0; tr_.pad = 0;
            if (on) tr_ = wterm[(int64_t)item * 8 + lane];
            const bool probed = on && ((pm >> lane) & 1);
            const int64_t lo = tr_.lo;
            const int start = 0, end = tr_.len;
            const double idf_l = tr_.idf;
            const double ubt = tr_.ub;
            const int64_t row_l = tr_.row;
            // integer weights of the quantised impacts, as bm25_topk_kernel computes them
            const double c = imp_unit;
            double sum = idf_l * c;
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) sum += __shfl_xor(sum, o, WAVE);   // (lanes 0..7 hold the terms; 8.. hold zeros)
            scale_l = 248.0 / sum;
            int w = on ? (int)ceil(idf_l * c * scale_l) : 0;
            w = on && w < 1 ? 1 : w;
            // the probed terms' largest quantised impacts in accumulator units (their bound / idf in
            // steps of (k1+1)/255, as bm25_bounds_kernel rounds)
            const double im = probed ? (idf_l > 0.0 ? ceil(ubt / idf_l * imp_per_unit) + 1.0 : 255.0) : 0.0;
            dm_l = probed ? w * (im > 255.0 || !(im >= 0.0) ? 255 : (int)im) : 0;
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) dm_l += __shfl_xor(dm_l, o, WAVE);
            if (lane < 8) {
                L.t_lo[lane] = lo + start;
                L.t_len[lane] = (on && !probed) ? end - start : 0;
                L.t_cur[lane] = 0;
                L.t_idf[lane] = idf_l;
                L.t_row[lane] = row_l;
                L.t_w[lane] = w;
            }
        }
        const double acc_scale = __shfl(scale_l, 0, WAVE);
        const uint32_t dmaxq = (uint32_t)__shfl(dm_l, 0, WAVE);
        ww_sync();
        WW_T(0);
        WW_C(10, 1);
        // the wave's top-k
        for (int i = lane; i < WW_CAP; i += 64) {
            L.b_s[i] = -INFINITY;
            L.b_id[i] = INT32_MAX;
        }
        int b_cnt = 0;                 // (uniform)
        double th_s = -INFINITY;       // this item's k-th best so far (exact after a cut)
        int32_t th_id = INT32_MAX;
        double thg = -INFINITY;        // the query's other slices' threshold
        {
            const unsigned long long g0 = __hip_atomic_load(&theta_glob[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (g0) thg = dkey_inv(g0);
        }
        int remaining = 0;
        for (int t = 0; t < nt; ++t) remaining += L.t_len[t];
        ww_sync();
        auto thq_now = [&]() -> uint32_t {   // the threshold in accumulator units (0: none yet)
            double th = th_s > thg ? th_s : thg;
            if (!(th > -INFINITY)) return 0u;
            const double tq = floor(th * acc_scale * (1.0 - 1e-12));
            return tq < 0.0 ? 0u : tq > 70000.0 ? 70000u : (uint32_t)tq;
        };
        // cut the buffer back to the best k: exact sort, so the threshold is the k-th best itself
        auto cut = [&]() {
            WW_C(12, 1);
            ww_sync();
            ww_sort(L.b_s, L.b_id, lane);
            if (b_cnt > k) {
                for (int i = k + lane; i < WW_CAP; i += 64) {
                    L.b_s[i] = -INFINITY;
                    L.b_id[i] = INT32_MAX;
                }
                b_cnt = k;
            }
            ww_sync();
            if (b_cnt >= k) {
                th_s = L.b_s[k - 1];
                th_id = L.b_id[k - 1];
                if (lane == 0 && th_s > -INFINITY) atomicMax(&theta_glob[q], (unsigned long long)dkey(th_s));
            }
        };
        auto push = [&](bool ok, double sc, int32_t d) {
            // (precondition: b_cnt <= 64)
            ok = ok && !(sc < thg) && better(sc, (int64_t)d, th_s, (int64_t)th_id);
            const unsigned long long m = __ballot(ok);
            if (ok) {
                const int p = b_cnt + __popcll(m & lt_mask);
                L.b_s[p] = sc;
                L.b_id[p] = d;
            }
            b_cnt += __popcll(m);
            if (b_cnt > 64) cut();
        };
        // a probed term's contribution to doc d, 0 when the doc does not hold it
        auto probe_add = [&](int e, int32_t d, double dl, double& score) {
            const int tfd = (int)dense_tf[L.t_row[e] + d];
            if (tfd > 0) score = __dadd_rn(score, bm25_contrib(L.t_idf[e], (double)tfd, dl, avgdl, k1, b));
        };

        while (remaining > 0) {
            // ---- stage: the stage is shared out in proportion to what is left of each list (a slice is
            // cut at docs of its longest list: equal quotas would take a 900 + 100 slice in two passes) ----
            if (lane == 0) {
                int n_live = 0;
                for (int t = 0; t < nt; ++t) n_live += L.t_len[t] - L.t_cur[t] > 0 ? 1 : 0;
                const int spare = WW_STAGE - 16 * n_live;   // every list with postings left gets at least 16 slots
                int off = 0;
                for (int t = 0; t < nt; ++t) {
                    const int rem = L.t_len[t] - L.t_cur[t];
                    int stg = rem > 0 ? 16 + (int)((int64_t)spare * rem / remaining) : 0;
                    stg = stg < rem ? stg : rem;
                    L.t_off[t] = off;
                    L.t_stg[t] = stg;
                    off += stg;
                }
            }
            ww_sync();
            for (int t = 0; t < nt; ++t) {
                const int stg = L.t_stg[t];
                const int32_t* src = post_doc + L.t_lo[t] + L.t_cur[t];
                const uint8_t* srci = post_imp + L.t_lo[t] + L.t_cur[t];
                int32_t* dst = L.st_doc + L.t_off[t];
                uint8_t* dsti = L.st_imp + L.t_off[t];
                for (int i = lane; i < stg; i += 64) {
                    dst[i] = src[i];
                    dsti[i] = srci[i];
                }
            }
            // the other slices' threshold travels with the staging loads
            {
                const unsigned long long g1 = __hip_atomic_load(&theta_glob[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (g1) {
                    const double g = dkey_inv(g1);
                    thg = g > thg ? g : thg;
                }
            }
            ww_sync();
            // d_hi: one past the last doc every list has fully staged
            int64_t d_hi = INT64_MAX;
            for (int t = 0; t < nt; ++t) {
                const int stg = L.t_stg[t];
                if (stg > 0 && L.t_cur[t] + stg < L.t_len[t]) {
                    const int64_t e = (int64_t)L.st_doc[L.t_off[t] + stg - 1] + 1;
                    d_hi = e < d_hi ? e : d_hi;
                }
            }
            if (lane < nt) {
                const int stg = L.t_stg[lane];
                L.t_sub[lane] = d_hi == INT64_MAX ? stg : count_below(L.st_doc + L.t_off[lane], stg, d_hi);
            }
            ww_sync();
            int total = 0, live = 0;
            for (int t = 0; t < nt; ++t) {
                total += L.t_sub[t];
                live += L.t_sub[t] > 0 ? 1 : 0;
            }
            WW_T(1);
            WW_C(11, 1);
            WW_C(14, total);
            // ---- Bloom bits (only with postings from more than one list) ----
            const bool bits = live > 1;
            int bwords = WW_BLOOM;   // per list: the largest power of two that fits `live` times
            while (bits && bwords * live > WW_BLOOM) bwords >>= 1;
            const int bl2 = 31 - __clz(bwords * 32);
            if (bits) {
                if (lane == 0) {
                    int s_ = 0;
                    for (int t = 0; t < nt; ++t) L.t_bs[t] = L.t_sub[t] > 0 ? s_++ : -1;
                }
                for (int i = lane; i < WW_BLOOM; i += 64) L.bloom[i] = 0u;
                ww_sync();
                for (int t = 0; t < nt; ++t) {
                    const int sub = L.t_sub[t], off = L.t_off[t], bs = L.t_bs[t];
                    for (int i = lane; i < sub; i += 64) {
                        const uint32_t dd = (uint32_t)L.st_doc[off + i];
                        const uint32_t h = (dd * 2654435761u) >> (32 - bl2), h2 = (dd * 0x85EBCA6Bu + 0x9E3779B9u) >> (32 - bl2);
                        atomicOr(&L.bloom[bs * bwords + (h >> 5)], 1u << (h & 31));
                        atomicOr(&L.bloom[bs * bwords + (h2 >> 5)], 1u << (h2 & 31));
                    }
                }
                ww_sync();
            }
            WW_T(2);
            // ---- classify and score ----
            int n_list = 0, n_work = 0;   // (uniform) singles from the front, postings to search from the back
            // the listed singles [0, n_list): gathers, float64 score, push -- 64 at a time
            auto score_listed = [&]() {
                WW_T(3);
                WW_C(13, (n_list + 63) / 64);
                WW_C(15, n_list);
                for (int base = 0; base < n_list; base += 64) {
                    const int j = base + lane;
                    bool ok = j < n_list;
                    double score = 0.0;
                    int32_t d = 0;
                    if (ok) {
                        const int idx = L.list[j];
                        int t = 0;
                        while (t + 1 < nt && idx >= L.t_off[t + 1]) ++t;   // (offsets ascend with t; an empty list shares the next one's)
                        d = L.st_doc[idx];
                        if (qc != -1 && doc_coll[d] != qc) ok = false;
                        if (ok) {
                            const double dl = (double)doclen[d];
                            const double tf_own = (double)post_tf[L.t_lo[t] + L.t_cur[t] + (idx - L.t_off[t])];
#pragma unroll
                            for (int e = 0; e < 8; ++e) {
                                if (e >= nt) continue;
                                if (L.t_row[e] >= 0) probe_add(e, d, dl, score);
                                else if (e == t) score = __dadd_rn(score, bm25_contrib(L.t_idf[e], tf_own, dl, avgdl, k1, b));
                            }
                        }
                    }
                    push(ok, score, d);
                }
                n_list = 0;
                WW_T(4);
            };
            for (int t = 0; t < nt; ++t) {
                const int sub = L.t_sub[t];
                if (sub == 0) continue;
                const int off = L.t_off[t];
                const uint32_t wt = (uint32_t)L.t_w[t];
                const uint8_t* imp_t = L.st_imp + off;
                for (int base = 0; base < sub; base += 64) {
                    const int i = base + lane;
                    const uint32_t thq = thq_now();
                    bool alone = i < sub, search = false;
                    if (alone) {
                        const int32_t d = L.st_doc[off + i];
                        if (bits) {   // two bits per (list, doc): ~5 % false positives where one bit gave 12 %
                            const uint32_t dd = (uint32_t)d;
                            const uint32_t h = (dd * 2654435761u) >> (32 - bl2), h2 = (dd * 0x85EBCA6Bu + 0x9E3779B9u) >> (32 - bl2);
                            const uint32_t w = h >> 5, bit = 1u << (h & 31), w2 = h2 >> 5, bit2 = 1u << (h2 & 31);
                            for (int e = 0; e < nt; ++e) {
                                const int bs = L.t_bs[e];
                                if (e != t && bs >= 0 && (L.bloom[bs * bwords + w] & bit) && (L.bloom[bs * bwords + w2] & bit2)) search = true;
                            }
                        }
                        alone = !search;
                        if (alone && thq != 0u && (uint32_t)imp_t[i] * wt + dmaxq < thq) alone = false;   // cannot enter
                    }
                    const unsigned long long ma = __ballot(alone), ms = __ballot(search);
                    if (alone) L.list[n_list + __popcll(ma & lt_mask)] = (uint16_t)(off + i);
                    if (search) L.list[WW_STAGE - 1 - (n_work + __popcll(ms & lt_mask))] = (uint16_t)(off + i);
                    n_list += __popcll(ma);
                    n_work += __popcll(ms);
                    // no threshold yet: score what is listed as soon as it can fill the top-k, so that
                    // the rest of the pass is classified against a threshold
                    ww_sync();
                    if (n_list >= 64 && (thq_now() == 0u || n_list + n_work + 64 > WW_STAGE)) score_listed();
                }
            }
            ww_sync();
            score_listed();
            WW_T(3);
            // the postings whose doc may be in another list: owner and positions by search
            for (int base = 0; base < n_work; base += 64) {
                const int j = base + lane;
                bool ok = j < n_work;
                double score = 0.0;
                int32_t d = 0;
                if (ok) {
                    const int idx = L.list[WW_STAGE - 1 - j];
                    int t = 0;
                    while (t + 1 < nt && idx >= L.t_off[t + 1]) ++t;
                    d = L.st_doc[idx];
                    int wf[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        wf[e] = -1;
                        if (e < nt && L.t_sub[e] > 0)
                            wf[e] = e == t ? idx - L.t_off[e] : find_doc(L.st_doc + L.t_off[e], L.t_sub[e], d);
                    }
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (e < t && wf[e] >= 0) ok = false;             // an earlier list owns the doc
                    if (ok && qc != -1 && doc_coll[d] != qc) ok = false;
                    if (ok) {
                        const double dl = (double)doclen[d];
#pragma unroll
                        for (int e = 0; e < 8; ++e) {
                            if (e >= nt) continue;
                            if (L.t_row[e] >= 0) probe_add(e, d, dl, score);
                            else if (wf[e] >= 0)
                                score = __dadd_rn(score, bm25_contrib(L.t_idf[e], (double)post_tf[L.t_lo[e] + L.t_cur[e] + wf[e]], dl, avgdl, k1, b));
                        }
                    }
                }
                push(ok, score, d);
            }
            ww_sync();
            if (lane == 0)
                for (int t = 0; t < nt; ++t) L.t_cur[t] += L.t_sub[t];
            remaining -= total;
            ww_sync();
            WW_T(5);
        }
        // ---- the item's list: sorted best first ----
        ww_sync();
        ww_sort(L.b_s, L.b_id, lane);
        const int n = b_cnt < k ? b_cnt : k;
        // (the output addresses are formed HERE: formed at the top of the item, as the compiler
        // would, they are four registers carried -- spilled -- through the whole walk)
        int q_w = __builtin_amdgcn_readfirstlane(q), item_w = __builtin_amdgcn_readfirstlane(item);
        asm volatile("" : "+s"(q_w), "+s"(item_w));
        if (S == 1) {   // the query's only item: its list is the result
            for (int i = lane; i < k; i += 64) {
                out_s[(int64_t)q_w * k + i] = i < n ? L.b_s[i] : -INFINITY;
                out_id[(int64_t)q_w * k + i] = i < n ? (int64_t)L.b_id[i] + id_base : -1;
            }
            if (lane == 0) out_cnt[q_w] = n;
        } else {
            for (int i = lane; i < n; i += 64) {
                slice_s[(int64_t)item_w * k + i] = L.b_s[i];
                slice_id[(int64_t)item_w * k + i] = (int64_t)L.b_id[i] + id_base;
            }
            if (lane == 0) {
                slice_cnt[item_w] = n;
                if (n >= k) atomicMax(&theta_glob[q], (unsigned long long)dkey(L.b_s[k - 1]));
            }
        }
        ww_sync();
        WW_T(6);
    }
#ifdef BM_STAMPS
    WW_T(8);
    if (lane == 0) {
        const int w = blockIdx.x * WW_WAVES + (threadIdx.x >> 6);
        for (int i = 0; i < 16; ++i) wstamps[(size_t)w * 16 + i] = ws_acc[i];
    }
#endif
#undef WW_T
#undef WW_C
}

void bm_launch_walk_wave(const BmIndex& X, const BmBatch& B, const BmLayout& L, int grid) {
    hipLaunchKernelGGL(bm25_walk_wave_kernel, dim3(grid), dim3(WW_WAVES * 64), 0, B.st, X.rowptr, X.post_doc,
                       X.post_tf, X.doclen, X.idf, X.term_ub, X.post_imp, X.dense_slot, X.dense_tf, X.dense_stride,
                       X.avgdl, X.k1, X.b, X.imp_unit, X.imp_per_unit, X.id_base, B.max_terms, B.k, B.doc_coll,
                       B.query_coll, L.ctl, L.q_nt, L.q_S, L.q_SA, L.q_pmask, L.q_terms, L.items, L.ipos, L.wrec,
                       L.wterm, L.theta, L.slice_s, L.slice_id, L.slice_cnt, B.out_s, B.out_id, B.out_cnt
                       BM_STAMPS_ONLY(, L.stamps));
}

}  // namespace thr
