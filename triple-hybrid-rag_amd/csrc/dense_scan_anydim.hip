// Dense scan on the f16 matrix cores at a row length given at run time (a multiple of 32 up to 4096):
// dense_scan_anydim (dense_scan_anydim.hpp), MODE_ALL / MODE_FILTER x the three query-tile sizes, and
// its launcher.
#include "dense_scan_anydim.hpp"

namespace thr {

template <int MODE>
int launch_scan_anydim(int dim, const float* rows32, const float* inv_norm, int64_t n_docs,
                       const float* queries, int n_queries, int ntiles, int64_t n_row_tiles,
                       int64_t tile_stride, const float* tau, int* tile_cnt, Cand* tile_list,
                       int tile_cap, float* sample, int64_t sample_ld, hipStream_t st,
                       const int32_t* doc_coll, const int32_t* query_coll) {
    THR_RETURN_IF(!anydim_ok(dim), THR_ERR_UNSUPPORTED);
    const size_t lds = anydim_lds_bytes(dim);
    THR_RETURN_IF(lds > 160 * 1024, THR_ERR_UNSUPPORTED);
    bool shared_rows = false;
    const dim3 grid = scan_grid(ntiles, n_row_tiles, AD_WAVES, &shared_rows);
    const bool nt = scan_nt(shared_rows);
#define THR_AD_LAUNCH(NB)                                                                         \
    return nt ? launch_lds(dense_scan_anydim<MODE, true, NB>, THR_AD_ARGS)                        \
              : launch_lds(dense_scan_anydim<MODE, false, NB>, THR_AD_ARGS);
#define THR_AD_ARGS                                                                               \
    grid, dim3(AD_THREADS), lds, st, rows32, inv_norm, n_docs, dim, queries, n_queries,           \
        n_row_tiles, tile_stride, tau, tile_cnt, tile_list, tile_cap, sample, sample_ld, doc_coll, \
        query_coll
    switch (anydim_qt(dim)) {
        case 64: THR_AD_LAUNCH(4)
        case 32: THR_AD_LAUNCH(2)
        case 16: THR_AD_LAUNCH(1)
        default: return THR_ERR_UNSUPPORTED;
    }
#undef THR_AD_ARGS
#undef THR_AD_LAUNCH
}

#define THR_INSTANTIATE(MODE)                                                                          \
    template int launch_scan_anydim<MODE>(int, const float*, const float*, int64_t, const float*, int, \
                                          int, int64_t, int64_t, const float*, int*, Cand*, int,       \
                                          float*, int64_t, hipStream_t, const int32_t*, const int32_t*);
THR_INSTANTIATE(MODE_ALL)
THR_INSTANTIATE(MODE_FILTER)
#undef THR_INSTANTIATE

}  // namespace thr
