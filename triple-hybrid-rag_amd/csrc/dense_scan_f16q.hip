// Dense scan over the normalised float16 copy, queries in registers (the default): dense_scan_f16qs
// and dense_scan_f16q (dense_scan_f16q.hpp) with their launcher, and the kernels that write what
// they read (dense_f16_image.hpp) -- pack_queries_f16 (the query image), quantize_f16_norm /
// measure_f16_error (the copy and its rounding error).
#include "dense_f16_image.hpp"
#include "dense_scan_f16q.hpp"

namespace thr {

template <int MODE, bool PROF>
int launch_scan_f16q(int dim, const _Float16* rows16, const _Float16* qfrag, int n_qtiles,
                            int64_t n_row_tiles, int64_t tile_stride, const float* tau, int* seg_cnt,
                            Cand* cand, float* sample, hipStream_t st,
                            int* nseg_out, const int32_t* doc_coll,
                            const int32_t* query_coll, int n_queries,
                            unsigned long long* stamps, int* n_blocks) {
    bool shared_rows = false;
    const bool stag = qreg_staggered(dim);
    // a lane's candidate segment is (row slice, row half): at most 256 slices (512 segments, two
    // per thread of select_band) -- enough for one block per CU when the batch is a single
    // workgroup tile of queries
    const dim3 grid = scan_grid(n_qtiles, n_row_tiles, 1, &shared_rows, (!stag && dim <= 768) ? 2 : 1, 32);
    const int shape = qreg_shape(dim);
    const int nseg = (shape == 16 ? 4 : 2) * (int)(grid.x / n_qtiles);
    if (nseg_out) *nseg_out = nseg;
    if (n_blocks) *n_blocks = (int)grid.x;
    if (PROF && !stamps) return THR_OK;   // size query
    // a batch without a collection filter (no collections in the index, or none asked for) runs the
    // instantiation that has no gather and no test for one compiled in
    const bool coll = doc_coll != nullptr && query_coll != nullptr;
#define THR_QS_LAUNCH_(DIM, SHAPE, COLL)                                                          \
    {if constexpr (PROF)                                                                          \
        return launch_lds(dense_scan_f16qs_stamps<DIM, SHAPE, COLL>, grid, dim3(QS_NW * 64),      \
                          QStag<DIM>::LDS_BYTES, st, (const f32x4*)rows16, (const f32x4*)qfrag,   \
                          n_qtiles, n_row_tiles, tile_stride, tau, seg_cnt, cand, CAND_CAP / nseg,\
                          doc_coll, query_coll, n_queries, stamps);                               \
    else                                                                                          \
        return launch_lds(dense_scan_f16qs<DIM, MODE, SHAPE, COLL>, grid, dim3(QS_NW * 64),       \
                          QStag<DIM>::LDS_BYTES, st, (const f32x4*)rows16, (const f32x4*)qfrag,   \
                          n_qtiles, n_row_tiles, tile_stride, tau, seg_cnt, cand, CAND_CAP / nseg,\
                          sample, doc_coll, query_coll, n_queries);}
#define THR_QS_LAUNCH(DIM, SHAPE)                                                                 \
    {                                                                                             \
        if (coll) THR_QS_LAUNCH_(DIM, SHAPE, true)                                                \
        THR_QS_LAUNCH_(DIM, SHAPE, false)                                                         \
    }
    if (stag) {
        if (dim == 512 && shape == 32) THR_QS_LAUNCH(512, 32)
        if (dim == 512) THR_QS_LAUNCH(512, 16)
        if (shape == 32) THR_QS_LAUNCH(768, 32)
        THR_QS_LAUNCH(768, 16)
    }
#undef THR_QS_LAUNCH
#undef THR_QS_LAUNCH_
#define THR_Q_LAUNCH_(DIM, SHAPE, COLL)                                                           \
    return launch_lds(dense_scan_f16q<DIM, MODE, PROF, SHAPE, COLL>, grid, dim3(Q_NW * 64),       \
                      QScan<DIM>::LDS_BYTES, st, (const f32x4*)rows16, (const f32x4*)qfrag,       \
                      n_qtiles, n_row_tiles, tile_stride, tau, seg_cnt, cand, CAND_CAP / nseg,    \
                      sample, doc_coll, query_coll, n_queries, stamps);
#define THR_Q_LAUNCH(DIM, SHAPE)                                                                  \
    {                                                                                             \
        if (coll) THR_Q_LAUNCH_(DIM, SHAPE, true)                                                 \
        THR_Q_LAUNCH_(DIM, SHAPE, false)                                                          \
    }
    switch (dim) {
        case 512: if (shape == 16) THR_Q_LAUNCH(512, 16) THR_Q_LAUNCH(512, 32)
        case 768: if (shape == 16) THR_Q_LAUNCH(768, 16) THR_Q_LAUNCH(768, 32)
        case 1024:
            if (shape == 16 && qreg_qw(dim) == 48) THR_Q_LAUNCH(1024, 48)
            if (shape == 16) THR_Q_LAUNCH(1024, 16)
            THR_Q_LAUNCH(1024, 32)
        default: return THR_ERR_UNSUPPORTED;
    }
#undef THR_Q_LAUNCH
#undef THR_Q_LAUNCH_
}

int launch_pack_queries(int dim, const float* queries, int n_queries, int qpad,
                               _Float16* qfrag, float* qerr, hipStream_t st) {
    const dim3 grid((unsigned)(qpad / 32));
    const bool s16 = qreg_shape(dim) == 16;
#define THR_PACK(DIM, SHAPE) \
    hipLaunchKernelGGL((pack_queries_f16<DIM, SHAPE>), grid, dim3(256), 0, st, queries, n_queries, (f32x4*)qfrag, qerr)
    switch (dim) {
        case 512: if (s16) THR_PACK(512, 16); else THR_PACK(512, 32); break;
        case 768: if (s16) THR_PACK(768, 16); else THR_PACK(768, 32); break;
        case 1024: if (s16) THR_PACK(1024, 16); else THR_PACK(1024, 32); break;
        default: return THR_ERR_UNSUPPORTED;
    }
#undef THR_PACK
    return launch_status();
}

int launch_quantize_f16(const float* docs, int64_t n_docs, int dim, _Float16* docs16,
                        unsigned int* max_rel_err, hipStream_t st) {
    if (docs16) {
        // normalised rows, NaN for rows without an embedding and for the padding of the last tile
        THR_RETURN_IF(dim % 16 != 0, THR_ERR_UNSUPPORTED);
        const int64_t n_pad = (n_docs + 31) / 32 * 32;
        hipLaunchKernelGGL(quantize_f16_norm, dim3((unsigned)((n_pad + 3) / 4)), dim3(256), 0, st,
                           docs, n_docs, dim, qreg_shape(dim), docs16, max_rel_err);
        return launch_status();
    }
    // measure only: the in-flight-rounding scan rounds the rows as they are
    hipLaunchKernelGGL(measure_f16_error, dim3((unsigned)((n_docs + 3) / 4)), dim3(256), 0, st, docs,
                       n_docs, dim, max_rel_err);
    return launch_status();
}

#define THR_INSTANTIATE(MODE, PROF)                                                                    \
    template int launch_scan_f16q<MODE, PROF>(int, const _Float16*, const _Float16*, int, int64_t, int64_t, \
                                              const float*, int*, Cand*, float*, hipStream_t, int*, \
                                              const int32_t*, const int32_t*, int, unsigned long long*, int*);
THR_INSTANTIATE(MODE_ALL, false)
THR_INSTANTIATE(MODE_FILTER, false)
THR_INSTANTIATE(MODE_FILTER, true)
#undef THR_INSTANTIATE

}  // namespace thr
