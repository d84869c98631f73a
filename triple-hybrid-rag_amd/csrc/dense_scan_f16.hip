// Dense scan on the f16 matrix cores over the float32 rows, rounded in flight: dense_scan_f16
// (dense_scan_f16.hpp), every dim x MODE_ALL / MODE_FILTER, and its launcher.
#include "dense_scan_f16.hpp"

namespace thr {

// the in-flight-rounding f16 scan: streams the float32 rows and rounds them in registers
template <int MODE>
int launch_scan_f16(int dim, int nq, const float* rows32, const float* inv_norm,
                           int64_t n_docs, const float* queries, int n_queries, int ntiles,
                           int64_t n_row_tiles, int64_t tile_stride, const float* tau, int* tile_cnt,
                           Cand* tile_list, int tile_cap, float* sample, int64_t sample_ld,
                           hipStream_t st, const int32_t* doc_coll,
                           const int32_t* query_coll) {
    const size_t lds = f16_lds_bytes(dim, nq);
    THR_RETURN_IF(lds > 160 * 1024, THR_ERR_UNSUPPORTED);
    bool shared_rows = false;
    const dim3 grid = scan_grid(ntiles, n_row_tiles, H_WAVES, &shared_rows);
    const bool nt = scan_nt(shared_rows);
#define THR_H_LAUNCH(DIM, NQV)                                                                    \
    return nt ? launch_lds(dense_scan_f16<DIM, MODE, true, NQV>, THR_H_ARGS)                      \
              : launch_lds(dense_scan_f16<DIM, MODE, false, NQV>, THR_H_ARGS);
#define THR_H_ARGS                                                                                \
    grid, dim3(H_THREADS), lds, st, rows32, inv_norm, n_docs, queries, n_queries, n_row_tiles,    \
        tile_stride, tau, tile_cnt, tile_list, tile_cap, sample, sample_ld, doc_coll, query_coll
    switch (dim * 10 + nq) {
        case 5122: THR_H_LAUNCH(512, 2)
        case 7682: THR_H_LAUNCH(768, 2)
        case 10241: THR_H_LAUNCH(1024, 1)
        default: return THR_ERR_UNSUPPORTED;
    }
#undef THR_H_ARGS
#undef THR_H_LAUNCH
}

#define THR_INSTANTIATE(MODE)                                                                          \
    template int launch_scan_f16<MODE>(int, int, const float*, const float*, int64_t, const float*, int, \
                                       int, int64_t, int64_t, const float*, int*, Cand*, int, float*,  \
                                       int64_t, hipStream_t, const int32_t*, const int32_t*);
THR_INSTANTIATE(MODE_ALL)
THR_INSTANTIATE(MODE_FILTER)
#undef THR_INSTANTIATE

}  // namespace thr
