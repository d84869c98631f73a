// BM25 stage B: bm25_window_kernel, the doc-window sweep over the dense terms' rows.
#include "bm25_common.hpp"

namespace thr {

typedef unsigned short bm_u16x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------
// bm25_window_kernel: stage B of a query with dense (probed) terms -- the docs of a doc range that
// hold none of the query's walked terms (those were scored by stage A).
// The range is taken in SEGMENTS of up to 256 K docs.  Per segment the walked terms' postings set
// one bit per doc in an LDS bitmap (32 KiB): the docs to leave out.  The segment is then swept in
// windows of up to 64 K docs: the probed terms add their quantised impacts straight from their
// per-doc rows into per-thread registers (coalesced dword loads: 4 docs each, v_perm_b32 +
// v_pk_mad_u16 into two 16-bit sums per word), BW_SCAN docs at a time; a doc whose summed bound
// reaches the threshold survives; phase 2 drops the survivors whose bit is set, reads the others'
// term frequencies from the rows and scores them with the oracle's arithmetic in query-term order.
// Nothing is staged per window and no accumulator is kept in LDS: a pass is the row loads, the
// scan, the (few) survivors and the select.  Same exactness argument as the accumulator path (the
// bound is >= acc_scale * score), same top-k / threshold sharing / slice merge as bm25_topk_kernel.
template <int BW_THREADS, int BW_SCAN, int BW_CAP>
__global__ __launch_bounds__(BW_THREADS, 4) void bm25_window_kernel(
    const int64_t* __restrict__ rowptr, const int32_t* __restrict__ post_doc,
    const float* __restrict__ doclen, const double* __restrict__ idf,
    const int32_t* __restrict__ dense_slot, const uint8_t* __restrict__ dense_imp,
    const uint16_t* __restrict__ dense_tf, int64_t dense_stride, double avgdl, double k1, double b,
    int64_t n_docs, int64_t id_base, int max_terms, int k, const int32_t* __restrict__ doc_coll,
    const int32_t* __restrict__ query_coll, int32_t* __restrict__ ctl,
    const int32_t* __restrict__ q_nt, const int32_t* __restrict__ q_S, const int32_t* __restrict__ q_SA,
    const int32_t* __restrict__ q_pmask,
    const int32_t* __restrict__ q_terms, const int2* __restrict__ items, const int32_t* __restrict__ sweep_items,
    const int32_t* __restrict__ ipos, unsigned long long* __restrict__ theta_glob,
    double* __restrict__ slice_s, int64_t* __restrict__ slice_id, int32_t* __restrict__ slice_cnt,
    double* __restrict__ out_s, int64_t* __restrict__ out_id, int32_t* __restrict__ out_cnt
#ifdef BM_STAMPS
    , unsigned long long* __restrict__ stamps
#endif
    ) {
#ifdef BM_STAMPS
    unsigned long long stamp_acc[BM_NSTAMP] = {0};
    unsigned long long stamp_last = __builtin_readcyclecounter(), stamp_items = 0;
    unsigned long long* item_log = stamps + (size_t)2 * 4096 * (BM_NSTAMP + 1);   // behind the three stamp areas: 4 words per sweep item
#endif
    constexpr int BIT_WORDS = 8192;                   // the segment's bitmap: 256 K docs
    constexpr int SEG_DOCS = BIT_WORDS * 32;
    constexpr int QPT = BW_SCAN / 4 / BW_THREADS;     // dwords of a dense row per thread and scan step (4 docs each)
    constexpr int SURV_CAP = 4096;
    constexpr int CHUNK = 4 * BW_THREADS;             // walked postings looked at per step of the bitmap fill
    static_assert(QPT * 4 * BW_THREADS == BW_SCAN && BW_PAD % BW_SCAN == 0 && BW_SCAN % SURV_CAP == 0 &&
                  BW_PAD <= 65536 && SEG_DOCS % BW_PAD == 0, "window shape");
    static_assert(BW_CAP >= THR_TOPK_MAX + BW_THREADS, "top-k buffer");
    __shared__ TermRange tr[8];      // walked terms: .lo / .len = the slice's postings, .cur = consumed by earlier segments
    __shared__ double t_idf[8];
    __shared__ int64_t t_row[8];     // probed term: offset of its per-doc row; else -1
    __shared__ int t_w[8], p_w[8];
    __shared__ int64_t p_row[8];     // the probed terms' rows and weights, compactly
    __shared__ double acc_scale, th_glob;
    __shared__ int p_thq, p_wmax, n_surv, cur_item, last_compact, chunk_cnt;
    __shared__ double b_s[BW_CAP];
    __shared__ int64_t b_id[BW_CAP];
    __shared__ int b_cnt;
    __shared__ double th_s;
    __shared__ int64_t th_id;
    __shared__ uint32_t bits[BIT_WORDS];
    __shared__ uint16_t surv[SURV_CAP];

    const int n_sweeps = ctl[CTL_SWEEPS];   // (bm25_sweep_filter_kernel)
    BlockTopK<BW_CAP, BW_THREADS> tk;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) cur_item = atomicAdd(&ctl[CTL_NEXT_SWEEP], 1);
        __syncthreads();
        if (cur_item >= n_sweeps) break;
#ifdef BM_STAMPS
        const unsigned long long item_t0 = __builtin_readcyclecounter();
        int item_passes = 0, item_surv = 0;
#endif
        const int item = sweep_items[cur_item];
        const int2 it = items[item];
        const int q = it.x, sl = it.y;
        const int SA = q_SA[q];
        const int S = q_S[q];              // (> 1: the item writes a slice list and shares the threshold)
        const int nt = q_nt[q];
        const int qc = query_coll ? query_coll[q] : -1;
        const int64_t D0 = bm_window_edge(n_docs, sl - SA, S - SA), D1 = bm_window_edge(n_docs, sl - SA + 1, S - SA);
        if ((int)threadIdx.x < nt) {
            const int slot = threadIdx.x;
            const int term = q_terms[(int64_t)q * max_terms + slot];
            const int64_t lo = rowptr[term];
            const int ds = ((q_pmask[q] >> slot) & 1) ? dense_slot[term] : -1;   // a walked term: its docs are left out
            const int start = ipos[((int64_t)item * max_terms + slot) * 2];
            const int end = ipos[((int64_t)item * max_terms + slot) * 2 + 1];
            tr[slot].lo = lo + start;
            tr[slot].len = ds >= 0 ? 0 : end - start;
            tr[slot].cur = 0;
            t_row[slot] = ds >= 0 ? (int64_t)ds * dense_stride : -1;
            t_idf[slot] = idf[term];
        }
        if (threadIdx.x == 0) {
            last_compact = 0;
            chunk_cnt = 0;
            const unsigned long long g0 = S > 1 ? __hip_atomic_load(&theta_glob[q], __ATOMIC_RELAXED,
                                                                    __HIP_MEMORY_SCOPE_AGENT) : 0ull;
            th_glob = g0 ? dkey_inv(g0) : -INFINITY;
        }
        BM_STAMP(0);
        tk.init(b_s, b_id, &b_cnt, &th_s, &th_id, k);   // includes a barrier
        int n_walked = 0, np = 0;
        for (int t = 0; t < nt; ++t) {
            n_walked += t_row[t] < 0 && tr[t].len > 0 ? 1 : 0;
            np += t_row[t] >= 0 ? 1 : 0;
        }
        if (threadIdx.x == 0) {
            // integer weights of the quantised impacts (see bm25_topk_kernel) -- of the PROBED terms
            // only: a doc of the sweep holds no walked term, so its score is the probed terms' alone,
            // and the 248 units go to them.  (Shared out over all the query's terms -- round 3 -- a lone
            // stop word beside three rare walked terms got a weight of ceil(1.6) = 2: a bound 22 % above
            // the score, every doc of the shard "survived" and was scored in full: six items of 1.3 M
            // cycles each in a kernel whose workgroups average 0.64 M -- the sweep kernel's length.)
            const double c = (k1 + 1.0) / 255.0;
            double sum = 0.0;
            for (int t = 0; t < nt; ++t)
                if (t_row[t] >= 0) sum += t_idf[t] * c;
            const double scale = sum > 0.0 ? 248.0 / sum : 1.0;
            for (int t = 0; t < nt; ++t) {
                const int w = t_row[t] >= 0 ? (int)ceil(t_idf[t] * c * scale) : 0;
                t_w[t] = w < 1 ? 1 : w;
            }
            acc_scale = scale;
            int i = 0;   // the probed terms, compactly: row and weight
            for (int t = 0; t < nt; ++t)
                if (t_row[t] >= 0) {
                    p_row[i] = t_row[t];
                    p_w[i++] = t_w[t];
                }
        }
        __syncthreads();
        // what the coming pass needs: its window and its threshold in accumulator units
        auto prepare = [&](int last_w, int last_ns) {
            if (threadIdx.x == 0) {
                const bool have_local = b_cnt >= k && th_s > -INFINITY;
                const bool have_th = have_local || th_glob > -INFINITY;
                double th = have_local ? th_s : -INFINITY;
                th = th_glob > th ? th_glob : th;
                const double tq = have_th ? floor(th * acc_scale * (1.0 - 1e-12)) : 0.0;
                p_thq = tq < 0.0 ? 0 : tq > 70000.0 ? 70000 : (int)tq;
                // without a threshold every doc that holds a term is scored in full: a short window gets
                // one; and a threshold that let more than 1/16 of the last window through is still a poor
                // one (the k docs seen so far need not hold the term that decides the ranking: a stop
                // word with idf 0.01 beside a 2 % term with idf 3.8 had 35 K survivors in the 64 K window
                // that followed the first 2 K one): the window then grows fourfold per pass, not at once
                p_wmax = !(have_th || S == 1) ? 2048
                         : (last_w > 0 && last_ns * 16 > last_w && last_w * 4 < BW_PAD) ? (last_w * 4 > 2048 ? last_w * 4 : 2048)
                                                                                       : BW_PAD;
                n_surv = 0;
            }
        };
        BM_STAMP(1);
        for (int64_t g0 = D0; g0 < D1; g0 += SEG_DOCS) {
            const int64_t g1 = g0 + SEG_DOCS < D1 ? g0 + SEG_DOCS : D1;
            // ---- the segment's docs that hold a walked term: one bit each ----
            if (n_walked > 0) {
                const int nw = (int)((g1 - g0 + 31) >> 5);
                for (int i = threadIdx.x; i < nw; i += BW_THREADS) bits[i] = 0u;
                __syncthreads();
                for (int t = 0; t < nt; ++t) {
                    if (t_row[t] >= 0) continue;
                    for (;;) {   // the list's next postings, CHUNK at a time, up to the segment's end (the list is doc-sorted)
                        const int base = tr[t].cur, rem = tr[t].len - base;
                        if (rem <= 0) break;
                        const int n = rem < CHUNK ? rem : CHUNK;
                        const int32_t* src = post_doc + tr[t].lo + base;
                        int mine = 0;
#pragma unroll
                        for (int u = 0; u < CHUNK / BW_THREADS; ++u) {
                            const int i = u * BW_THREADS + (int)threadIdx.x;
                            if (i < n) {
                                const int64_t d = src[i];
                                if (d < g1) {
                                    const uint32_t bit = (uint32_t)(d - g0);
                                    atomicOr(&bits[bit >> 5], 1u << (bit & 31));
                                    ++mine;
                                }
                            }
                        }
                        if (mine) atomicAdd(&chunk_cnt, mine);
                        __syncthreads();
                        const int c = chunk_cnt;
                        __syncthreads();
                        if (threadIdx.x == 0) {
                            tr[t].cur = base + c;
                            chunk_cnt = 0;
                        }
                        __syncthreads();
                        if (c < n) break;   // the rest of the list belongs to later segments
                    }
                }
            }
            prepare(0, 0);
            __syncthreads();
            BM_STAMP(3);
            int64_t cursor = g0;
            while (cursor < g1) {
                const int wmax = p_wmax;
                const int64_t end = cursor + wmax < g1 ? cursor + wmax : g1;   // (g0, the window widths: multiples of 4)
                const int w = (int)(end - cursor);
                const double thg = th_glob;
                auto push = [&](bool ok, double sc, int64_t d) { tk.push(ok && !(sc < thg), sc, d); };
                // (the other slices' threshold for the NEXT pass: requested now, read in the tail)
                unsigned long long gth = 0ull;
                if (threadIdx.x == 0 && S > 1)
                    gth = __hip_atomic_load(&theta_glob[q], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                // ---- probed terms: 4 docs per load, straight into registers ----
                auto load_rows = [&](uint32_t (&v)[QPT], int i, int h0) {   // row i, docs [h0, h0 + BW_SCAN) of the window
                    const uint32_t* src = reinterpret_cast<const uint32_t*>(dense_imp + p_row[i] + cursor + h0);   // a multiple of 4
#pragma unroll
                    for (int j = 0; j < QPT; ++j) {
                        const int dw = j * BW_THREADS + (int)threadIdx.x;
                        v[j] = h0 + 4 * dw < w ? src[dw] : 0u;
                    }
                };
                // four impact bytes -> two words of two 16-bit sums: v_perm_b32 spreads the bytes,
                // v_pk_mad_u16 multiplies both lanes by the weight and adds (a sum stays below 2^16)
                auto add_rows = [&](uint32_t (&dsum)[2 * QPT], const uint32_t (&v)[QPT], int i) {
                    const unsigned short wt = (unsigned short)p_w[i];
                    const bm_u16x2 w2 = {wt, wt};
#pragma unroll
                    for (int j = 0; j < QPT; ++j) {
                        const bm_u16x2 lo = __builtin_bit_cast(bm_u16x2, __builtin_amdgcn_perm(0u, v[j], 0x0c010c00u));
                        const bm_u16x2 hi = __builtin_bit_cast(bm_u16x2, __builtin_amdgcn_perm(0u, v[j], 0x0c030c02u));
                        dsum[2 * j] = __builtin_bit_cast(uint32_t, (bm_u16x2)(lo * w2 + __builtin_bit_cast(bm_u16x2, dsum[2 * j])));
                        dsum[2 * j + 1] = __builtin_bit_cast(uint32_t, (bm_u16x2)(hi * w2 + __builtin_bit_cast(bm_u16x2, dsum[2 * j + 1])));
                    }
                };
                auto dense_sums = [&](uint32_t (&dsum)[2 * QPT], int h0) {
#pragma unroll
                    for (int j = 0; j < 2 * QPT; ++j) dsum[j] = 0u;
                    for (int i = 0; i < np; ++i) {
                        uint32_t v[QPT];
                        load_rows(v, i, h0);
                        add_rows(dsum, v, i);
                    }
                };
                // ---- scan: the docs whose bound reaches the threshold ----
                const uint32_t thq = (uint32_t)p_thq;
                auto scan = [&](int c0, int c1, const uint32_t (&dsum)[2 * QPT], int h0) {
#pragma unroll
                    for (int j = 0; j < 2 * QPT; ++j) {
                        const int s0 = h0 + 4 * ((j >> 1) * BW_THREADS + (int)threadIdx.x) + 2 * (j & 1);
                        if (s0 >= c1 || s0 + 1 < c0 || s0 >= w) continue;
                        const uint32_t v = dsum[j];
                        if ((v & 0xFFFFu) < thq && (v >> 16) < thq) continue;   // (nearly every word)
#pragma unroll
                        for (int u = 0; u < 2; ++u) {
                            const uint32_t a = (v >> (u << 4)) & 0xFFFFu;
                            const int slot = s0 + u;
                            if (a != 0u && a >= thq && slot >= c0 && slot < c1 && slot < w) {
                                const int at = atomicAdd(&n_surv, 1);
                                if (at < SURV_CAP) surv[at] = (uint16_t)slot;
                            }
                        }
                    }
                };
                auto phase2 = [&](int ns) {
                    for (int base = 0; base < ns; base += BW_THREADS) {
                        const int j = base + threadIdx.x;
                        bool keep = j < ns;
                        double score = 0.0;
                        int32_t d = 0;
                        if (keep) {
                            d = (int32_t)(cursor + surv[j]);
                            if (n_walked > 0) {   // (a doc that holds a walked term was scored by stage A)
                                const uint32_t bit = (uint32_t)(d - g0);
                                if ((bits[bit >> 5] >> (bit & 31)) & 1u) keep = false;
                            }
                            if (keep && qc != -1 && doc_coll[d] != qc) keep = false;
                            if (keep) {
                                const double dl = (double)doclen[d];
                                int tfv[8];
#pragma unroll
                                for (int e = 0; e < 8; ++e) {
                                    tfv[e] = 0;
                                    if (e < nt) {
                                        const int64_t row = t_row[e];
                                        if (row >= 0) tfv[e] = (int)dense_tf[row + d];
                                    }
                                }
#pragma unroll
                                for (int e = 0; e < 8; ++e)
                                    if (tfv[e] > 0)
                                        score = __dadd_rn(score, bm25_contrib(t_idf[e], (double)tfv[e], dl, avgdl, k1, b));
                            }
                        }
                        push(keep, score, (int64_t)d);
                    }
                };
                BM_COUNT(14, 1);
                BM_COUNT(16, w);
                // BW_SCAN docs per step; the rows of the first PF probed terms for the NEXT step are
                // requested before this step's sums and scan (a step is otherwise one round trip long)
                constexpr int PF = 4;
                uint32_t nxt[PF][QPT];
#pragma unroll
                for (int i = 0; i < PF; ++i)
                    if (i < np) load_rows(nxt[i], i, 0);
#pragma unroll 1
                for (int h0 = 0; h0 < w; h0 += BW_SCAN) {
                    uint32_t cur[PF][QPT];
#pragma unroll
                    for (int i = 0; i < PF; ++i)
#pragma unroll
                        for (int j = 0; j < QPT; ++j) cur[i][j] = nxt[i][j];
                    if (h0 + BW_SCAN < w) {
#pragma unroll
                        for (int i = 0; i < PF; ++i)
                            if (i < np) load_rows(nxt[i], i, h0 + BW_SCAN);
                    }
                    uint32_t dsum[2 * QPT];
#pragma unroll
                    for (int j = 0; j < 2 * QPT; ++j) dsum[j] = 0u;
#pragma unroll
                    for (int i = 0; i < PF; ++i)
                        if (i < np) add_rows(dsum, cur[i], i);
                    for (int i = PF; i < np; ++i) {
                        uint32_t v[QPT];
                        load_rows(v, i, h0);
                        add_rows(dsum, v, i);
                    }
                    scan(0, w, dsum, h0);
                }
                __syncthreads();
                BM_STAMP(13);
                const int ns = n_surv;
                BM_COUNT(17, ns);
                BM_COUNT(18, (ns + BW_THREADS - 1) / BW_THREADS);
#ifdef BM_STAMPS
                ++item_passes;
                item_surv += ns;
#endif
                if (ns <= SURV_CAP) {
                    phase2(ns);
                } else {   // (passes without a threshold) SURV_CAP slots at a time
                    for (int c0 = 0; c0 < w; c0 += SURV_CAP) {
                        __syncthreads();
                        if (threadIdx.x == 0) n_surv = 0;
                        __syncthreads();
                        {   // (the sums again: they are not kept across phase 2)
                            const int h0 = c0 / BW_SCAN * BW_SCAN;
                            uint32_t dsum[2 * QPT];
                            dense_sums(dsum, h0);
                            scan(c0, c0 + SURV_CAP, dsum, h0);
                        }
                        __syncthreads();
                        phase2(n_surv);
                    }
                }
                __syncthreads();
                BM_STAMP(5);
                if (b_cnt >= k && b_cnt - last_compact >= 64) {
                    BM_COUNT(15, 1);
                    tk.compact();
                    if (threadIdx.x == 0) {
                        last_compact = b_cnt;
                        if (S > 1 && th_s > -INFINITY) atomicMax(&theta_glob[q], (unsigned long long)dkey(th_s));
                    }
                }
                if (threadIdx.x == 0 && S > 1 && gth) {
                    const double g = dkey_inv(gth);
                    if (g > th_glob) th_glob = g;
                }
                cursor = end;
                prepare(w, ns);
                __syncthreads();
                BM_STAMP(10);
            }
        }
        const int n = tk.finish();
#ifdef BM_STAMPS
        if (threadIdx.x == 0) {
            item_log[4 * (size_t)cur_item] = ((unsigned long long)q << 32) | (unsigned)(((sl - SA) << 16) | (np << 8) | n_walked);
            item_log[4 * (size_t)cur_item + 1] = item_t0;
            item_log[4 * (size_t)cur_item + 2] = __builtin_readcyclecounter();
            item_log[4 * (size_t)cur_item + 3] = ((unsigned long long)item_passes << 32) | (unsigned)item_surv;
        }
#endif
        if (S == 1) {
            for (int i = threadIdx.x; i < k; i += BW_THREADS) {
                out_s[(int64_t)q * k + i] = i < n ? b_s[i] : -INFINITY;
                out_id[(int64_t)q * k + i] = i < n ? b_id[i] + id_base : -1;
            }
            if (threadIdx.x == 0) out_cnt[q] = n;
        } else {
            for (int i = threadIdx.x; i < n; i += BW_THREADS) {
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
#endif
    }
#ifdef BM_STAMPS
    if (threadIdx.x == 0) {
        for (int i = 0; i < BM_NSTAMP; ++i) stamps[(int64_t)blockIdx.x * (BM_NSTAMP + 1) + i] = stamp_acc[i];
        stamps[(int64_t)blockIdx.x * (BM_NSTAMP + 1) + BM_NSTAMP] = stamp_items;
    }
#endif
}

void bm_launch_window(const BmIndex& X, const BmBatch& B, const BmLayout& L, int grid
                      BM_STAMPS_ONLY(, unsigned long long* stamps)) {
    hipLaunchKernelGGL((bm25_window_kernel<512, 8192, 1024>), dim3(grid), dim3(512), 0, B.st, X.rowptr, X.post_doc,
                       X.doclen, X.idf, X.dense_slot, X.dense_imp, X.dense_tf, X.dense_stride, X.avgdl, X.k1, X.b,
                       X.n_docs, X.id_base, B.max_terms, B.k, B.doc_coll, B.query_coll, L.ctl, L.q_nt, L.q_S, L.q_SA,
                       L.q_pmask, L.q_terms, L.items, L.sweep_items, L.ipos, L.theta, L.slice_s, L.slice_id,
                       L.slice_cnt, B.out_s, B.out_id, B.out_cnt BM_STAMPS_ONLY(, stamps));
}

}  // namespace thr
