// Dense scan over the float32 rows on the fp32-input matrix cores: dense_scan_mfma and
// dense_scan_mfma2 (dense_scan_mfma.hpp), every dim x MODE_ALL / MODE_FILTER, and their launcher.
#include "dense_scan_mfma.hpp"

namespace thr {

template <int MODE>
int launch_scan_mfma(int dim, const float* docs, const float* inv_norm, int64_t n_docs,
                            const float* queries, int n_queries, int ntiles, int64_t n_row_tiles,
                            int64_t tile_stride, const float* tau, int* tile_cnt, Cand* tile_list,
                            int tile_cap, float* sample, int64_t sample_ld, hipStream_t st,
                            const int32_t* doc_coll, const int32_t* query_coll) {
    const size_t lds1 = sizeof(float) * MF_QT * (size_t)dim + sizeof(Cand) * MF_WAVES * WBUF;
    auto lds2_for = [&](int nw) {
        return sizeof(float) * MF_QT * (size_t)dim + (sizeof(Cand) * WBUF + sizeof(float4) * MF2_STAGE_F4) * nw;
    };
    // v2 adds a 4 KiB transpose tile per wave on top of the query tile: 8 waves fit up to dim
    // 768.  At dim 1024 only 4 waves (one per SIMD) would fit, and that measured slower than
    // the fragment-load variant with 8 waves (4.30 vs 4.93 TB/s), which therefore runs there.
    int nw = 0;
    if (dim % 128 == 0 && dim >= 256)
        nw = lds2_for(8) <= 160 * 1024 ? 8 : 0;
    const bool v2 = nw != 0;
    const size_t lds = v2 ? lds2_for(nw) : lds1;
    const int waves = v2 ? nw : MF_WAVES;
    bool shared_rows = false;
    const dim3 grid = scan_grid(ntiles, n_row_tiles, waves, &shared_rows);
    const bool nt = scan_nt(shared_rows);
#define THR_MF_LAUNCH(KERN, THREADS)                                                              \
    return launch_lds(KERN, grid, dim3(THREADS), lds, st, docs, inv_norm, n_docs, queries,        \
                      n_queries, n_row_tiles, tile_stride, tau, tile_cnt, tile_list, tile_cap,    \
                      sample, sample_ld, doc_coll, query_coll);
#define THR_MF_CASE(D8)                                                                           \
    case D8:                                                                                      \
        if (!v2) THR_MF_LAUNCH((dense_scan_mfma<D8, MODE>), MF_THREADS)                           \
        if (nt) THR_MF_LAUNCH((dense_scan_mfma2<D8, MODE, true, 8>), 512)                         \
        THR_MF_LAUNCH((dense_scan_mfma2<D8, MODE, false, 8>), 512)
    switch (dim / 8) {
        THR_MF_CASE(32)
        THR_MF_CASE(64)
        THR_MF_CASE(96)
        THR_MF_CASE(128)
        default:
            return THR_ERR_UNSUPPORTED;
    }
#undef THR_MF_CASE
#undef THR_MF_LAUNCH
}

#define THR_INSTANTIATE(MODE)                                                                          \
    template int launch_scan_mfma<MODE>(int, const float*, const float*, int64_t, const float*, int, int, \
                                        int64_t, int64_t, const float*, int*, Cand*, int, float*, int64_t, \
                                        hipStream_t, const int32_t*, const int32_t*);
THR_INSTANTIATE(MODE_ALL)
THR_INSTANTIATE(MODE_FILTER)
#undef THR_INSTANTIATE

}  // namespace thr
