// What the dense translation units share: the sizes and records of the pipeline, the device helpers
// and tile sizes more than one scan flavour uses, and the host functions the units call each other
// through -- the knobs and the scan grid of dense.hip; the launch functions of the scans, of the
// selection and of the rescoring, each defined beside its kernels, which take the records dense.hip
// fills once per call (DensePlan, DenseIndex, DenseBatch, DensePhase).
#pragma once
#include <type_traits>

#include "thr_common.hpp"

namespace thr {

constexpr int CHUNK = 256;                 // floats per wave-wide float4 load (1 KiB)
constexpr int MODE_ALL = 0, MODE_FILTER = 1;
constexpr int CAND_CAP = 16384;            // candidates kept per query between K3 and K4
constexpr int SAMPLE_MAX = 1 << 20;        // upper bound of the sample (rows) for the tau estimate
constexpr int WBUF = 256;                  // per-wave LDS staging slots for passing rows
constexpr int ROW_BITS = 27;               // tile-list entries pack (query-in-tile << 27 | row)
constexpr uint32_t ROW_MASK = (1u << ROW_BITS) - 1;
constexpr int ROW_BITS_F16 = 25;           // f16 shortlist scans: up to 96 queries per tile -> 7 bits
constexpr int SEL_BIG_BAND = 1024;         // rows a query's shortlist may hold (K4a -> K4b): the row stride of sel_rows
constexpr int QREG_MAX_SEG = 1024;         // most candidate / sample segments per query of the register-resident scans
constexpr int SAMPLE_TOP = 4;              // sample scores a lane of the register-resident scans keeps per query and segment
constexpr int CS_BINS = 4096;              // histogram bins of the coarse selects = most values select_band ranks in their place

struct Cand {
    float score;
    uint32_t doc;
};

}  // namespace thr
// ---------------------------------------------------------------------------
// Block -> (row slice, query tile) for the MFMA scans.
// Every query tile streams the same rows, so the launch is laid out for the 8 private L2s:
// workgroups are dealt round-robin over the XCDs (b and b+8 share one), and a 1-D grid of
// 8 * m * n_qtiles blocks is decoded so that the blocks resident together on one XCD are the
// n_qtiles query tiles of the SAME row slice.  They walk identical addresses in step: the
// first one to ask for a line pulls it from HBM, the others hit it in that XCD's L2.
// Placement is a speed matter only: any dispatch order gives the same result.
// ---------------------------------------------------------------------------
struct ScanSlot {
    int qtile, slice, nslices;
};
__device__ __forceinline__ ScanSlot scan_slot(int n_qtiles) {
    ScanSlot s;
    const int b = blockIdx.x, xcd = b & 7, j = b >> 3;
    s.qtile = j % n_qtiles;
    s.slice = xcd + 8 * (j / n_qtiles);
    s.nslices = gridDim.x / n_qtiles;
    return s;
}

namespace thr {

// ---- device helpers and tile sizes shared by the scan flavours ----
// compile-time loop: the body sees its index as a constant expression, so register arrays
// indexed with it stay in registers (a "#pragma unroll" the compiler declines would demote
// them to scratch)
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));  // native vector: plain SSA loads/stores
typedef _Float16 half8 __attribute__((ext_vector_type(8)));

constexpr int MF_ROWS = 32;   // rows per wave tile
constexpr int MF_QT = 32;     // queries per tile pass
constexpr int MF2_STAGE_F4 = MF_ROWS * 8;  // float4 slots per stage tile (32 rows x 8 chunks)
constexpr int H_WAVES = 8;     // waves per workgroup of dense_scan_f16

// swizzled float4 index of 16-byte chunk `cidx` of query row q (row length D8*2 chunks)
__device__ __forceinline__ int mf_qslot(int q, int cidx, int chunks_per_row) {
    return q * chunks_per_row + ((cidx & ~15) | ((cidx ^ q) & 15));
}

// float4 slot of (row, chunk) inside a stage tile: chunk ^ ((row >> 1) & 7)
__device__ __forceinline__ int mf2_slot(int row, int chunk) {
    return row * 8 + (chunk ^ ((row >> 1) & 7));
}

// round 8 floats to nearest-even float16 (same rounding as quantize_f16, whose error bound covers
// both flavours)
__device__ __forceinline__ f32x4 pack_f16x8(f32x4 lo, f32x4 hi) {
    typedef _Float16 half4 __attribute__((ext_vector_type(4)));
    const half4 a = __builtin_convertvector(lo, half4), b = __builtin_convertvector(hi, half4);
    half8 v = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(f32x4, v);
}

// ---- host side ----
// in-flight-rounding f16 scan (dense_scan_f16): query sub-tiles of 32 per pass -- 2 (64 queries,
// 96 KiB of LDS at dim 768) when the tile fits next to the transpose tiles, else 1
inline size_t f16_lds_bytes(int dim, int nq) {
    return sizeof(_Float16) * 32 * nq * (size_t)dim +
           (sizeof(Cand) * WBUF + sizeof(float4) * MF2_STAGE_F4) * H_WAVES;
}
inline int f16_pick_nq(int dim) { return f16_lds_bytes(dim, 2) <= 160 * 1024 ? 2 : 1; }

// runtime-dim f16 scan (dense_scan_anydim): any row length that is a multiple of THR_DENSE_ANYDIM_STEP up to
// THR_DENSE_ANYDIM_MAX; queries per tile by row length -- the tile ([QT][dim] float16) stays in LDS beside
// the waves' candidate buffers within the CU's 160 KiB (16 x 4096 x 2 B = 128 KiB + 16 KiB)
inline bool anydim_ok(int dim) {
    return dim >= THR_DENSE_ANYDIM_STEP && dim <= THR_DENSE_ANYDIM_MAX && dim % THR_DENSE_ANYDIM_STEP == 0;
}
// (at 512 / 768 / 1024, where thr_dense_f16_select lets either scan of float32 rows serve a call, this is
// 32 * f16_pick_nq(dim): a plan, its workspace and the candidate lists a shortlist call leaves for its
// finish call do not depend on the selection -- asserted below)
inline int anydim_qt(int dim) { return dim <= 768 ? 64 : dim <= 1536 ? 32 : 16; }
inline size_t anydim_lds_bytes(int dim) {
    return sizeof(_Float16) * (size_t)anydim_qt(dim) * (size_t)dim + sizeof(Cand) * WBUF * H_WAVES;
}

inline bool f16_tiles_agree() {
    for (int dim : {512, 768, 1024})
        if (anydim_qt(dim) != 32 * f16_pick_nq(dim)) return false;
    return true;
}

// fp32 error bound of the MFMA scans, relative to ||q||*||d||, in units of 2^-24: a dim-long fma chain
inline double scan_eps(int dim) {
    const double u = 5.9604644775390625e-08;
    return ((double)dim + 16.0) * u;
}

// ---- what the launch functions take: filled once per entry point (dense.hip) ----
// The work plan of a batch and its workspace, carved by make_plan.
constexpr int KIND_F32 = 0, KIND_F16 = 1;
struct DensePlan {
    int kind;      // KIND_F32: float32 MFMA scan; KIND_F16: an f16 MFMA scan
    bool anydim;   // KIND_F16, not packed: dense_scan_anydim (row length at run time) in the place of dense_scan_f16
    bool packed;   // KIND_F16 only: dense_scan_f16q[s] over the fragment-major copy (queries in registers,
                   // rows through LDS; the candidate area is written in per-lane segments), else float32
                   // rows rounded in flight
    int nq, qtile, ntiles, qpad, row_bits, ksample, tile_cap;
    bool sampled;
    int64_t groups, sample_groups, sample_stride, sample_docs;
    float* tau;
    float* qerr;         // null for KIND_F32 (no quantisation term)
    int* cnt;            // } zeroed per call
    int* tcnt;           // } by one memset
    Cand *cand, *tlist;
    float* sample;
    _Float16* qfrag;
    int32_t *sel_rows, *sel_meta;   // K4a -> K4b shortlists
    size_t total;
};
// The index as the caller holds it.
struct DenseIndex {
    const float *docs, *inv_norm;
    int64_t n_docs;
    int dim;
    const double* dnorm = nullptr;
    int64_t id_base = 0;
    const int32_t* doc_coll = nullptr;
    const _Float16* docs16 = nullptr;   // the normalised f16 copy (null: float32 rows)
    double doc_rel_err = 0.0;
};
// The batch of one call (no outputs before the shards' exchange).
struct DenseBatch {
    const float* queries;
    int n_queries, k, kprime;
    const int32_t* query_coll;
    hipStream_t st;
    double* out_scores = nullptr;
    int64_t* out_ids = nullptr;
    int32_t* out_counts = nullptr;
    uint32_t* out_flags = nullptr;
};
// What only document shards use.  PIPE_ALL = one call; PIPE_SHORTLIST = K1..K3 + the top_m lower
// bounds (the candidate lists stay in the workspace); PIPE_FINISH = K4 on those lists with the
// shards' common floor.
enum { PIPE_ALL = 0, PIPE_SHORTLIST = 1, PIPE_FINISH = 2 };
struct DensePhase {
    int phase = PIPE_ALL;
    float* top_lb = nullptr;         // SHORTLIST: this shard's lower bounds [nq, top_m]
    int top_m = 0;
    const float* gfloor = nullptr;   // FINISH: the common floor, or
    const float* lb_all = nullptr;   //   the shards' gathered lower bounds [n_shards, nq, top_m]
    int n_shards = 0;
};

// dense.hip: the knobs (read once, there), the grid of a scan
bool qreg_staggered(int dim);
int qreg_waves(int dim);
int qreg_shape(int dim);
int qreg_qw(int dim);
int qreg_max_queries(int dim);
dim3 scan_grid(int ntiles, int64_t n_row_tiles, int waves, bool* shared_rows, int blocks_per_cu = 1,
               int m_cap = 64);
bool scan_nt(bool shared_rows);

// dense_scan_mfma.hip, dense_scan_f16.hip, dense_scan_anydim.hip, dense_scan_f16q.hip: MODE_ALL and
// MODE_FILTER of each
template <int MODE>
int launch_scan_mfma(int dim, const float* docs, const float* inv_norm, int64_t n_docs,
                     const float* queries, int n_queries, int ntiles, int64_t n_row_tiles,
                     int64_t tile_stride, const float* tau, int* tile_cnt, Cand* tile_list,
                     int tile_cap, float* sample, int64_t sample_ld, hipStream_t st,
                     const int32_t* doc_coll = nullptr, const int32_t* query_coll = nullptr);
template <int MODE>
int launch_scan_f16(int dim, int nq, const float* rows32, const float* inv_norm, int64_t n_docs,
                    const float* queries, int n_queries, int ntiles, int64_t n_row_tiles,
                    int64_t tile_stride, const float* tau, int* tile_cnt, Cand* tile_list,
                    int tile_cap, float* sample, int64_t sample_ld, hipStream_t st,
                    const int32_t* doc_coll = nullptr, const int32_t* query_coll = nullptr);
template <int MODE>
int launch_scan_anydim(int dim, const float* rows32, const float* inv_norm, int64_t n_docs,
                       const float* queries, int n_queries, int ntiles, int64_t n_row_tiles,
                       int64_t tile_stride, const float* tau, int* tile_cnt, Cand* tile_list,
                       int tile_cap, float* sample, int64_t sample_ld, hipStream_t st,
                       const int32_t* doc_coll = nullptr, const int32_t* query_coll = nullptr);
// (PROF: the stamped kernel, MODE_FILTER only; without `stamps` a size query)
template <int MODE, bool PROF = false>
int launch_scan_f16q(int dim, const _Float16* rows16, const _Float16* qfrag, int n_qtiles,
                     int64_t n_row_tiles, int64_t tile_stride, const float* tau, int* seg_cnt,
                     Cand* cand, float* sample, hipStream_t st,
                     int* nseg_out = nullptr, const int32_t* doc_coll = nullptr,
                     const int32_t* query_coll = nullptr, int n_queries = 1 << 30,
                     unsigned long long* stamps = nullptr, int* n_blocks = nullptr);
int launch_pack_queries(int dim, const float* queries, int n_queries, int qpad, _Float16* qfrag,
                        float* qerr, hipStream_t st);
// docs16 == null: the rounding error alone (measure_f16_error)
int launch_quantize_f16(const float* docs, int64_t n_docs, int dim, _Float16* docs16,
                        unsigned int* max_rel_err, hipStream_t st);
// dense_select.hip: K2 (the sampled and the unsampled form; sample_nseg: segments per query of the
// register-resident sample pass, else 0), K3b, K4a (nseg: segments per query of the candidate area as
// the register-resident scan left it, else 0); dense_rescore.hip: K4b, both sizes
int launch_threshold(const DensePlan& P, const DenseIndex& X, const DenseBatch& B, int sample_nseg);
int launch_bucket(const DensePlan& P, hipStream_t st);
int launch_band(const DensePlan& P, const DenseIndex& X, const DenseBatch& B, const DensePhase& S, int nseg);
int launch_rescore(const DensePlan& P, const DenseIndex& X, const DenseBatch& B);
// dense_exact.hip, for dense_rows.hip: the [q][slab][k] lists of every query -> its top k (ids + id_base,
// flags CERTIFIED|EXACT); a query whose scope is outside [0, n_scopes) gets the empty list
int launch_merge_scoped(const double* slab_s, const int64_t* slab_id, int n_queries, int n_slabs, int k,
                        int64_t id_base, const int32_t* query_scope, int n_scopes, double* out_scores,
                        int64_t* out_ids, int32_t* out_counts, uint32_t* out_flags, hipStream_t st);

}  // namespace thr
