// Host side of the BM_STAMPS diagnostic build (_build.build_variant("stamps", ["BM_STAMPS"]);
// scripts/bm25_stamps.py, scripts/bm25_items.py): the stamp buffer behind the workspace, and the
// reports thr_bm25_topk prints to stderr after waiting for its launches.  Included by bm25.hip
// (behind BmLayout), and called, only under #ifdef BM_STAMPS.
//
// The buffer: three areas of 4096 workgroups x (BM_NSTAMP + 1) words -- [0] the workgroup walk (its
// ordinary or fused launch; the wave walk's 16 words per wave before it), [1] the window kernel,
// [2] the workgroup walk's stage-A launch -- then 4 words per sweep item, then 4 per walked item.
#pragma once
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace thr {

constexpr size_t BM_STAMP_AREA = (size_t)4096 * (BM_NSTAMP + 1);

inline size_t bm_stamps_words(int cap) { return 3 * BM_STAMP_AREA + 8 * (size_t)cap; }
inline unsigned long long* bm_stamps_area(const BmLayout& L, int area) { return L.stamps + area * BM_STAMP_AREA; }
inline unsigned long long* bm_stamps_sweep_log(const BmLayout& L) { return L.stamps + 3 * BM_STAMP_AREA; }
inline unsigned long long* bm_stamps_walk_log(const BmLayout& L) { return bm_stamps_sweep_log(L) + 4 * (size_t)L.cap; }

inline void bm_stamps_begin(const BmLayout& L, hipStream_t st) {
    (void)hipMemsetAsync(L.stamps, 0, sizeof(unsigned long long) * bm_stamps_words(L.cap), st);
}

inline void bm_stamps_report_waves(const BmLayout& L, hipStream_t st, int nw) {
    (void)hipStreamSynchronize(st);
    std::vector<unsigned long long> h((size_t)nw * 16);
    (void)hipMemcpy(h.data(), L.stamps, h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    double tot[16] = {0};
    double mx = 0;
    for (int w = 0; w < nw; ++w) {
        double all = 0;
        for (int i = 0; i < 16; ++i) tot[i] += (double)h[(size_t)w * 16 + i];
        for (int i = 0; i < 9; ++i) all += (double)h[(size_t)w * 16 + i];
        mx = all > mx ? all : mx;
    }
    static const char* nm[9] = {"set-up", "stage+d_hi", "bloom", "classify", "score listed", "work list+advance", "finish", "skipped items", "idle tail"};
    double all = 0;
    for (int i = 0; i < 9; ++i) all += tot[i];
    fprintf(stderr, "[bm25 wave walk] %d waves, %.0f cycles per wave (max %.0f):", nw, all / nw, mx);
    for (int i = 0; i < 9; ++i) fprintf(stderr, " %s %.1f%%", nm[i], 100.0 * tot[i] / all);
    fprintf(stderr, " | items %.0f passes %.0f cuts %.0f batches %.0f postings %.0f listed %.0f\n", tot[10], tot[11], tot[12], tot[13], tot[14], tot[15]);
}

// (grid: of the workgroup walk; dense: stage A and stage B ran)
inline void bm_stamps_report(const BmLayout& L, hipStream_t st, int n_queries, int grid, bool dense) {
    static const char* names[BM_NSTAMP] = {"item set-up", "init", "quotas", "staging", "edges/prefix", "phase 2 (+ chunk reset)",
                                           "bloom build", "singles listed", "singles scored", "work list / boot select", "compact/advance", "finish",
                                           "mask / acc fill", "slot scan / middle search", "#acc passes", "#mask passes",
                                           "#postings masked", "#survivors", "#phase2 rounds", ""};
    (void)hipStreamSynchronize(st);
    for (int pass = 0; pass < (dense ? 3 : 1); ++pass) {
        const int g_n = pass == 1 ? num_cus() * 2 : grid;
        std::vector<unsigned long long> h((size_t)g_n * (BM_NSTAMP + 1));
        (void)hipMemcpy(h.data(), bm_stamps_area(L, pass), h.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        double tot[BM_NSTAMP + 1] = {0};
        for (int g = 0; g < g_n; ++g)
            for (int i = 0; i <= BM_NSTAMP; ++i) tot[i] += (double)h[(size_t)g * (BM_NSTAMP + 1) + i];
        double all = 0;
        for (int i = 0; i < 14; ++i) all += tot[i];
        fprintf(stderr, "[bm25 stamps%s] %d queries, %d workgroups, %.0f items, %.0f cycles per workgroup:", pass == 1 ? " window kernel (stage B)" : pass == 2 ? " stage A" : "", n_queries, g_n,
                tot[BM_NSTAMP], all / g_n);
        for (int i = 0; i < 14; ++i)
            if (names[i][0]) fprintf(stderr, " %s %.1f%%", names[i], 100.0 * tot[i] / all);
        for (int i = 14; i < 20; ++i) fprintf(stderr, " %s %.0f", names[i][0] ? names[i] : "#wmax|#singles", tot[i]);
        fprintf(stderr, "\n");
    }
    if (!dense) return;
    // the sweep items one by one: when each started and ended (cycles since the first), its passes and survivors
    int h_ctl[8];
    (void)hipMemcpy(h_ctl, L.ctl, sizeof(h_ctl), hipMemcpyDeviceToHost);
    const int ns = h_ctl[CTL_SWEEPS];
    std::vector<unsigned long long> lg((size_t)4 * (ns > 0 ? ns : 1));
    (void)hipMemcpy(lg.data(), bm_stamps_sweep_log(L), lg.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    unsigned long long t0 = ~0ull, t1 = 0;
    for (int i = 0; i < ns; ++i) {
        if (lg[4 * i + 1] < t0) t0 = lg[4 * i + 1];
        if (lg[4 * i + 2] > t1) t1 = lg[4 * i + 2];
    }
    fprintf(stderr, "[bm25 sweep items] %d items, %llu cycles from the first start to the last end\n", ns, ns ? t1 - t0 : 0ull);
    if (!getenv("THR_BM25_ITEM_LOG")) return;
    const int ni = h_ctl[CTL_ITEMS];
    std::vector<unsigned long long> wl((size_t)4 * (ni > 0 ? ni : 1));
    (void)hipMemcpy(wl.data(), bm_stamps_walk_log(L), wl.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    for (int i = 0; i < ni; ++i)
        if (wl[4 * i + 2])
            fprintf(stderr, "[walk] %d q %llu slice %llu dp %llu nt %llu postings %llu cycles %llu passes %llu\n", i, wl[4 * i] >> 32,
                    (wl[4 * i] >> 16) & 0xFFFF, (wl[4 * i] >> 8) & 0xFF, wl[4 * i] & 0xFF, wl[4 * i + 1], wl[4 * i + 2], wl[4 * i + 3]);
    for (int i = 0; i < ns; ++i)
        fprintf(stderr, "[item] %d q %llu slice %llu np %llu walked %llu start %llu cycles %llu passes %llu survivors %llu\n", i,
                lg[4 * i] >> 32, (lg[4 * i] >> 16) & 0xFFFF, (lg[4 * i] >> 8) & 0xFF, lg[4 * i] & 0xFF, lg[4 * i + 1] - t0,
                lg[4 * i + 2] - lg[4 * i + 1], lg[4 * i + 3] >> 32, lg[4 * i + 3] & 0xFFFFFFFFull);
}

}  // namespace thr
