// Dense channel: exact brute-force cosine top-k on gfx950 (MI355X).
//
// Stands where the reference calls SQL rag2_semantic_search
// (database/migrations/20260114_rag2_schema.sql:377-410, from
// src/voice_agent/rag2/retrieval.py:304-312): `1 - (embedding <=> q)`
// ORDER BY distance LIMIT k.  The reference answers it from an approximate
// HNSW index inside PostgreSQL; this is the exact scan that index approximates.
//
// Pipeline per batch of queries (all kernels on one stream, no host sync):
//   K0 pack_queries_f16         [dense_scan_f16q.hip] (default scan) queries -> fragment-major f16 register image
//   K1 scan<MODE_ALL>           score a strided SAMPLE of row groups for every query tile.  The
//                               register-resident scans keep each lane's SAMPLE_TOP best per query in
//                               registers and write only those; the other flavours write every score
//   K2 kth_select[_top]         [dense_select.hip] tau[q] ~ the ks-th largest sample score (of the
//                               lanes' kept values: never above it): about `aim` rows of the corpus
//                               will pass it
//   K3 scan<MODE_FILTER>        THE dominant kernel: stream the corpus once per query tile,
//                               emit (score, row) >= tau[q].  Default: dense_scan_f16qs (f16
//                               MFMA over the normalised f16 copy, queries in registers);
//                               dense_scan_f16 / dense_scan_mfma2 (dense_scan_mfma at dim 1024)
//                               are the other flavours [dense_scan_f16q.hip, dense_scan_f16.hip,
//                               dense_scan_mfma.hip: a unit per flavour]
//   K3b bucket_candidates       [dense_select.hip] (the scans with tile lists) a tile's candidates
//                               split by query
//   K4a select_band             [dense_select.hip] per query: the band of candidates that can still
//                               reach the top-k -> a shortlist of rows
//   K4b rescore_rank            [dense_rescore.hip] shortlist re-scored in float64 with sequential
//                               accumulation (the oracle's contract), sorted (score desc, row asc),
//                               certified with the scan's error bound
//   K5 thr_dense_rescue         [dense_exact.hip] uncertified queries redone exhaustively
// Beside the pipeline, the same float64 arithmetic without a shortlist: thr_dense_topk_exact over every row
// [dense_exact.hip] and thr_dense_topk_rows over a scope's row list [dense_rows.hip], both merged by
// merge_lists [dense_exact.hip].
// Algorithmic HBM bytes of K3 = n_docs * dim * 4 per tile pass.
//
// This unit is the host side of a batch: the knobs, the work plan and its workspace, the grid of a
// scan, the pipeline and the entry points that drive it.  The kernels live with their families and
// are launched through dense_common.hpp.
#include <stdlib.h>

#include "dense_common.hpp"

namespace thr {

constexpr double QREG_AIM_1M = 1448.0;   // see make_plan
constexpr int QREG_KS = 32;
// The A/B knobs, each read once per process (the layout of the f16 copy depends on them).
struct DenseKnobs {
    bool forced_q;   // THR_DENSE_F16=q: dense_scan_f16q (4-wave blocks) at every dim
    int shape;       // THR_DENSE_MFMA=32: the 32x32x16 MFMA shape, else 16 (16x16x32)
    bool forced32;   // THR_DENSE_QW=32: 32 queries per wave at dim 1024 too
    double aim_1m;   // THR_DENSE_AIM: candidates per query the register-resident scans aim at on 1M rows
    int ks;          // THR_DENSE_KS: their sample rank (both: the sweep of profiles/dense_threshold_pass.md)
};
static const DenseKnobs& dense_knobs() {
    static const DenseKnobs knobs = [] {
        DenseKnobs K;
        const char* e = getenv("THR_DENSE_F16");
        K.forced_q = e && e[0] == 'q';
        e = getenv("THR_DENSE_MFMA");
        K.shape = (e && atoi(e) == 32) ? 32 : 16;
        e = getenv("THR_DENSE_QW");
        K.forced32 = e && atoi(e) == 32;
        e = getenv("THR_DENSE_AIM");
        K.aim_1m = (e && atof(e) >= 64.0) ? atof(e) : QREG_AIM_1M;
        e = getenv("THR_DENSE_KS");
        K.ks = (e && atoi(e) >= 4 && atoi(e) <= 64) ? atoi(e) : QREG_KS;
        return K;
    }();
    return knobs;
}

// The scan over the float16 copy (queries in registers, rows through LDS): dense_scan_f16qs
// (staggered 8-wave block) where 8 x 32 queries' B operands fit the registers of two waves per
// SIMD, else dense_scan_f16q (4-wave blocks); THR_DENSE_F16=q forces the latter (it has the
// stamped diagnostic build).
bool qreg_staggered(int dim) { return !dense_knobs().forced_q && dim <= 768; }
int qreg_waves(int dim) { return qreg_staggered(dim) ? 8 : 4; }   // qreg_qw queries per wave
// MFMA shape of the staggered scan and therefore of the copy / query images: 16 (16x16x32, the
// default: 2.50 ms against 2.67 ms per 2048 x 1M x 768 launch) or 32 (32x32x16,
// THR_DENSE_MFMA=32).  (both register-resident kernels take either shape at every dim)
int qreg_shape(int) { return dense_knobs().shape; }
// queries per wave: 32, or 48 at dim 1024 with the 16x16x32 shape (dense_scan_f16q<1024, .., 48>:
// three 16-query blocks per wave, 192 queries per CU; THR_DENSE_QW=32 keeps the 32-query kernel for A/B)
int qreg_qw(int dim) {
    return (dim == 1024 && !qreg_staggered(dim) && qreg_shape(dim) == 16 && !dense_knobs().forced32) ? 48 : 32;
}
// The register-resident scans address a lane's candidate segment with a 32-bit byte offset from
// the start of the candidate area ((q * CAND_CAP + segment start) * sizeof(Cand)): a batch may
// hold as many (padded) queries as keep every offset below 2^32.
int qreg_max_queries(int dim) {
    const int qt = qreg_qw(dim) * qreg_waves(dim);
    const int64_t m = (int64_t)UINT32_MAX / ((int64_t)CAND_CAP * (int64_t)sizeof(Cand));
    return (int)(m / qt * qt);
}


// Which scan streams the float32 rows of an f16 call without a copy: the tuned dense_scan_f16 at the row
// lengths it is instantiated for, dense_scan_anydim at every other one it takes -- and at those three too
// while the calling thread has selected it (thr_dense_f16_select: the A/B of both kernels at one shape).
static thread_local int f16_selected = THR_DENSE_F16_BY_DIM;
static bool f16_tuned_dim(int dim) { return dim == 512 || dim == 768 || dim == 1024; }
static bool f16_dim_ok(int dim, bool packed) { return f16_tuned_dim(dim) || (!packed && anydim_ok(dim)); }
static bool f16_anydim(int dim, bool packed) {
    return !packed && anydim_ok(dim) && (!f16_tuned_dim(dim) || f16_selected == THR_DENSE_F16_ANYDIM);
}

// The work plan of a batch and its workspace carved from `ws`; from null, the plan and the size alone.
static DensePlan make_plan(void* ws, int64_t n_docs, int n_queries, int kprime, int kind, int dim,
                           bool packed) {
    DensePlan p;
    p.kind = kind;
    p.packed = kind == KIND_F16 && packed;
    p.anydim = kind == KIND_F16 && f16_anydim(dim, p.packed);
    p.nq = (kind == KIND_F16 && !p.packed && !p.anydim) ? f16_pick_nq(dim) : 1;
    p.row_bits = (kind == KIND_F16 && !p.packed) ? ROW_BITS_F16 : ROW_BITS;
    p.qtile = p.packed ? qreg_qw(dim) * qreg_waves(dim)
              : p.anydim ? anydim_qt(dim)
              : kind == KIND_F16 ? 32 * p.nq : MF_QT;
    p.ntiles = (n_queries + p.qtile - 1) / p.qtile;
    p.qpad = p.ntiles * p.qtile;
    const int64_t groups = (n_docs + MF_ROWS - 1) / MF_ROWS;
    // sample only when the corpus is larger than what the candidate list can hold anyway
    p.sampled = n_docs > CAND_CAP / 2;
    // tau = the ks-th best score of a sample of S rows lets (n / S) * ks rows per query through
    // on average; aim at 4096 (a quarter of CAND_CAP, half of a tile list's share).  ks is capped
    // at 64: the count of passing rows then spreads by ~1/8 of its mean (the tile share is 8
    // sigma away), and the sample pass + select cost a third of what ks = k' = 192 did.
    // The register-resident scan keeps one candidate segment per lane (no shared tile list), so
    // only the cost matters there: ks = 32 (spread ~1/6) halves the sample pass and the select.
    const int ks_cap = p.packed ? dense_knobs().ks : 64;
    p.ksample = kprime < ks_cap ? kprime : ks_cap;
    // (the sample must grow with the corpus: a capped sample lets n / S * ks rows through, which
    // overflows the candidate lists of every query on a 10M-row shard)
    // The sample pass costs ~ n * ks / aim, the scan's emit + K4's candidate read ~ aim: for the scans
    // that write every sample score the two meet at aim = 4096 at 1M rows
    // (profiles/r2_scan_tau_experiment.json), so aim follows sqrt(n) below that; never under 8 k'
    // (k' = 128: 1024 = k' + 7 sigma of the passing count at ks = 64).
    // The register-resident scans' sample pass writes a lane's SAMPLE_TOP best only, so it costs its
    // flops alone (~2.4 ns per sample row and 2048 queries) and the optimum sits lower: measured at
    // 1M x 768 x 2048, k' = 192 (profiles/dense_threshold_pass.md), aim 2896 -> 1536 takes 75 us off the
    // filter scan's emit and 5 off select_band for 31 more in the sample pass, and the 8 k' floor is
    // what holds it there: 1448 sqrt(n / 1M), i.e. the floor up to 1.1M rows at k' = 192.  ks stays 32:
    // 24 and 16 sample fewer rows (-15 / -31 us) but sit within the spread of the sum, and the
    // passing count's spread grows to 1/5 and 1/4 of its mean.
    double aim = (p.packed ? dense_knobs().aim_1m : 4096.0) * sqrt((double)n_docs / 1.0e6);   // (ks / 64 under the root)
    const double aim_lo = 8.0 * kprime < 4096.0 ? 8.0 * kprime : 4096.0;
    aim = aim < aim_lo ? aim_lo : aim > 4096.0 ? 4096.0 : aim;
    int64_t target = (int64_t)((double)n_docs * (double)p.ksample / aim);
    if (target > SAMPLE_MAX) target = SAMPLE_MAX;
    if (target < 4 * (int64_t)p.ksample) target = 4 * (int64_t)p.ksample;
    int64_t sg = (target + MF_ROWS - 1) / MF_ROWS;
    if (sg > groups) sg = groups;
    p.sample_stride = sg > 0 ? groups / sg : 1;
    if (p.sample_stride < 1) p.sample_stride = 1;
    p.sample_groups = p.sampled ? sg : 0;
    p.sample_docs = p.sample_groups * MF_ROWS;
    p.groups = groups;
    p.tile_cap = p.packed ? 1 : p.qtile * (CAND_CAP / 2);   // (no tile lists in the register-resident scan)
    const size_t qpad = (size_t)p.qpad;
    Arena A{(char*)ws};
    p.tau = A.take<float>(qpad);
    p.qerr = A.take<float>(qpad);
    if (kind != KIND_F16) p.qerr = nullptr;
    // (cnt and tcnt are zeroed by one memset; the register-resident scan keeps one count per segment
    // and writes every one of them itself)
    p.cnt = A.take<int>(qpad * (p.packed ? QREG_MAX_SEG : 1));
    p.tcnt = A.take<int>(p.ntiles);
    p.cand = A.take<Cand>(qpad * CAND_CAP);
    p.tlist = A.take<Cand>((size_t)p.ntiles * p.tile_cap);
    // the sample pass's output: every score (row-major), or the lanes' SAMPLE_TOP best per segment
    p.sample = A.take<float>(p.packed ? qpad * (size_t)QREG_MAX_SEG * SAMPLE_TOP : qpad * (size_t)p.sample_docs);
    p.qfrag = A.take<_Float16>(p.packed ? qpad * (size_t)dim : 0);
    p.sel_rows = A.take<int32_t>(qpad * SEL_BIG_BAND);
    p.sel_meta = A.take<int32_t>(4 * qpad);
    p.total = A.total;
    return p;
}

// Grid of an MFMA scan (see scan_slot): 1-D, 8 * m * n_qtiles blocks, one block per CU.  m is
// chosen for the fullest last round of blocks, the smallest such m first (fewer, longer row
// slices; at 32 query tiles m = 1 and the whole launch is a single round).
dim3 scan_grid(int ntiles, int64_t n_row_tiles, int waves, bool* shared_rows, int blocks_per_cu,
               int m_cap) {
    const int cus = num_cus() * blocks_per_cu;   // block slots
    int64_t m_max = n_row_tiles / (8 * (int64_t)waves);  // every wave gets at least one row tile
    if (m_max < 1) m_max = 1;
    if (m_max > m_cap) m_max = m_cap;
    int best_m = 1;
    double best_eff = 0.0;
    for (int m = 1; m <= (int)m_max; ++m) {
        const int64_t g = 8 * (int64_t)m * ntiles;
        const int64_t rounds = (g + cus - 1) / cus;
        const double eff = (double)g / (double)(rounds * cus);
        if (eff > best_eff + 1e-9) {
            best_eff = eff;
            best_m = m;
        }
    }
    *shared_rows = ntiles > 1;
    return dim3((unsigned)(8 * best_m * ntiles), 1u);
}

// row loads: non-temporal when no other query tile will ask for the same lines, plain when the
// query tiles of a slice share them through L2
bool scan_nt(bool shared_rows) { return !shared_rows; }


// K1 / K3: the scan of the plan's flavour in one mode.  MODE_ALL scores the sample rows for every
// query; MODE_FILTER streams the corpus and emits the candidates (*nseg: the segments per query of
// the register-resident scan's candidate area, or of its sample area; the other scans fill tile lists).
template <int MODE>
static int launch_scan(const DensePlan& P, const DenseIndex& X, const DenseBatch& B, int* nseg = nullptr) {
    constexpr bool all = MODE == MODE_ALL;
    const int64_t units = all ? P.sample_groups : P.groups, stride = all ? P.sample_stride : 1;
    const float* tau = all ? nullptr : P.tau;
    float* smp = all ? P.sample : nullptr;
    const int64_t ld = all ? P.sample_docs : 0;
    // (the register-resident sample pass applies the collection filter itself: it keeps no row identity)
    if (P.packed)
        return launch_scan_f16q<MODE>(X.dim, X.docs16, P.qfrag, P.ntiles, units, stride, tau,
                                      all ? nullptr : P.cnt, all ? nullptr : P.cand, smp, B.st,
                                      nseg, X.doc_coll, B.query_coll, B.n_queries);
    const int32_t* doc_coll = all ? nullptr : X.doc_coll;
    const int32_t* query_coll = all ? nullptr : B.query_coll;
    int* tcnt = all ? nullptr : P.tcnt;
    Cand* tlist = all ? nullptr : P.tlist;
    const int tile_cap = all ? 0 : P.tile_cap;
    if (P.anydim)
        return launch_scan_anydim<MODE>(X.dim, X.docs, X.inv_norm, X.n_docs, B.queries, B.n_queries, P.ntiles,
                                        units, stride, tau, tcnt, tlist, tile_cap, smp, ld, B.st, doc_coll,
                                        query_coll);
    if (P.kind == KIND_F16)
        return launch_scan_f16<MODE>(X.dim, P.nq, X.docs, X.inv_norm, X.n_docs, B.queries, B.n_queries,
                                     P.ntiles, units, stride, tau, tcnt, tlist, tile_cap, smp, ld, B.st,
                                     doc_coll, query_coll);
    return launch_scan_mfma<MODE>(X.dim, X.docs, X.inv_norm, X.n_docs, B.queries, B.n_queries, P.ntiles,
                                  units, stride, tau, tcnt, tlist, tile_cap, smp, ld, B.st, doc_coll,
                                  query_coll);
}

// K0..K4 for every scan flavour (S.phase: all of it, or one side of the shards' exchange).
static int dense_pipeline(const DensePlan& P, const DenseIndex& X, const DenseBatch& B,
                          const DensePhase& S) {
    int rc, nseg = 0, sample_nseg = 0;   // see launch_scan
    if (S.phase != PIPE_FINISH) {
        // cnt + tcnt.  Not for the register-resident scan: every block of it, the waves of padding
        // queries included, ends by writing the count of each (query, segment) it owns, the blocks
        // of a launch own all qpad x nseg of them, select_band reads no other, and tcnt is unused.
        if (!P.packed) {
            hipError_t e = hipMemsetAsync(P.cnt, 0, (char*)P.cand - (char*)P.cnt, B.st);
            if (e != hipSuccess) return (int)e;
        }
        if (P.packed && (rc = launch_pack_queries(X.dim, B.queries, B.n_queries, P.qpad, P.qfrag, P.qerr, B.st)))
            return rc;
        if (P.sampled && (rc = launch_scan<MODE_ALL>(P, X, B, &sample_nseg))) return rc;
        if ((rc = launch_threshold(P, X, B, P.packed ? sample_nseg : 0))) return rc;
        if ((rc = launch_scan<MODE_FILTER>(P, X, B, &nseg))) return rc;
        // (the register-resident scan writes the per-query lists itself)
        if (!P.packed && (rc = launch_bucket(P, B.st))) return rc;
    } else if (P.packed) {
        // the candidate area's layout as the filter scan of the shortlist call left it (a size query)
        if ((rc = launch_scan_f16q<MODE_FILTER, true>(X.dim, X.docs16, P.qfrag, P.ntiles, P.groups, 1,
                                                      nullptr, nullptr, nullptr, nullptr, B.st, &nseg)))
            return rc;
    }
    if ((rc = launch_band(P, X, B, S, nseg))) return rc;
    if (S.phase == PIPE_SHORTLIST) return THR_OK;   // (the top_m lower bounds are all of that call)
    return launch_rescore(P, X, B);
}

}  // namespace thr

using namespace thr;

extern "C" size_t thr_dense_workspace_bytes(int64_t n_docs, int dim, int n_queries, int kprime) {
    if (n_docs <= 0 || n_queries <= 0) return 0;
    return make_plan(nullptr, n_docs, n_queries, kprime, KIND_F32, dim, false).total;
}

static int dense_args_ok(const void* docs, const void* dnorm, const void* inv_norm,
                         const void* queries, const void* a, const void* b, const void* c,
                         const void* d, const void* ws, int64_t n_docs, int n_queries, int k,
                         int kprime) {
    THR_RETURN_IF(!docs || !dnorm || !inv_norm || !queries || !a || !b || !c || !d || !ws,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_docs <= 0 || n_queries <= 0 || k <= 0 || kprime < k ||
                      kprime > THR_DENSE_MAX_K,
                  THR_ERR_INVALID);
    return THR_OK;
}

extern "C" int thr_dense_topk(const float* docs, const double* dnorm, const float* inv_norm,
                              int64_t n_docs, int dim, int64_t id_base, const float* queries,
                              int n_queries, int k, int kprime, const int32_t* doc_coll,
                              const int32_t* query_coll, double* out_scores,
                              int64_t* out_ids, int32_t* out_counts, uint32_t* out_flags,
                              void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    int rc = dense_args_ok(docs, dnorm, inv_norm, queries, out_scores, out_ids, out_counts,
                           out_flags, workspace, n_docs, n_queries, k, kprime);
    if (rc) return rc;
    THR_RETURN_IF((query_coll != nullptr) != (doc_coll != nullptr), THR_ERR_INVALID);
    THR_RETURN_IF(dim <= 0 || dim % CHUNK != 0 || dim / CHUNK > 4, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n_docs >= (int64_t)1 << ROW_BITS, THR_ERR_UNSUPPORTED);
    const DensePlan P = make_plan(workspace, n_docs, n_queries, kprime, KIND_F32, dim, false);
    THR_RETURN_IF(workspace_bytes < P.total, THR_ERR_WORKSPACE);
    const DenseIndex X{docs, inv_norm, n_docs, dim, dnorm, id_base, doc_coll};
    const DenseBatch B{queries, n_queries, k, kprime, query_coll, (hipStream_t)stream,
                       out_scores, out_ids, out_counts, out_flags};
    return dense_pipeline(P, X, B, DensePhase{});
}

extern "C" size_t thr_dense_f16_workspace_bytes(int64_t n_docs, int dim, int n_queries,
                                                int kprime) {
    if (n_docs <= 0 || n_queries <= 0) return 0;
    // (the two scans of float32 rows have the same query tile where both exist: one size serves either)
    const size_t a = make_plan(nullptr, n_docs, n_queries, kprime, KIND_F16, dim, false).total;
    if (anydim_ok(dim) && !f16_tuned_dim(dim)) return a;   // (no copy scan at such a length)
    const size_t b = make_plan(nullptr, n_docs, n_queries, kprime, KIND_F16, dim, true).total;
    return a > b ? a : b;
}

extern "C" int thr_dense_f16_select(int flavour) {
    const int before = f16_selected;
    // both scans must plan the same query tile where the selection chooses between them
    if (!f16_tiles_agree()) return before;
    if (flavour == THR_DENSE_F16_BY_DIM || flavour == THR_DENSE_F16_ANYDIM) f16_selected = flavour;
    return before;
}

extern "C" int thr_dense_f16_max_queries(int dim, int packed) {
    if (!f16_dim_ok(dim, packed != 0)) return 0;
    return packed ? qreg_max_queries(dim) : INT32_MAX;
}

extern "C" int thr_dense_f16_query_tile(int dim, int packed, int n_queries) {
    if (!f16_dim_ok(dim, packed != 0)) return 0;
    (void)n_queries;
    if (f16_anydim(dim, packed != 0)) return anydim_qt(dim);
    return packed ? qreg_qw(dim) * qreg_waves(dim) : 32 * f16_pick_nq(dim);
}

extern "C" size_t thr_dense_f16_copy_bytes(int64_t n_docs, int dim) {
    if (n_docs <= 0 || dim <= 0) return 0;
    return sizeof(_Float16) * (size_t)((n_docs + 31) / 32 * 32) * (size_t)dim;
}

extern "C" int thr_dense_quantize_f16(const float* docs, int64_t n_docs, int dim, uint16_t* docs16,
                                      float* max_rel_err, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!docs || !max_rel_err || n_docs <= 0 || dim <= 0, THR_ERR_INVALID);
    // (the copy is written in 64-dim stages; measuring alone takes what dense_scan_anydim takes)
    THR_RETURN_IF(docs16 ? dim % 64 != 0 : dim % THR_DENSE_ANYDIM_STEP != 0, THR_ERR_UNSUPPORTED);
    hipStream_t st = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(max_rel_err, 0, sizeof(float), st);
    if (e != hipSuccess) return (int)e;
    return launch_quantize_f16(docs, n_docs, dim, reinterpret_cast<_Float16*>(docs16),
                               reinterpret_cast<unsigned int*>(max_rel_err), st);
}

static int f16_args_ok(const float* docs, const uint16_t* docs16, double doc_rel_err, int64_t n_docs,
                       int dim, int n_queries, const int32_t* doc_coll, const int32_t* query_coll) {
    (void)docs;
    THR_RETURN_IF((query_coll != nullptr) != (doc_coll != nullptr), THR_ERR_INVALID);
    THR_RETURN_IF(!(doc_rel_err >= 0.0) || !(doc_rel_err < 1.0), THR_ERR_INVALID);
    THR_RETURN_IF(!f16_dim_ok(dim, docs16 != nullptr), THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n_docs >= (int64_t)1 << ROW_BITS_F16, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(docs16 != nullptr && n_queries > qreg_max_queries(dim), THR_ERR_UNSUPPORTED);
    return THR_OK;
}


extern "C" int thr_dense_topk_f16(const float* docs, const uint16_t* docs16, double doc_rel_err,
                                  const double* dnorm, const float* inv_norm, int64_t n_docs,
                                  int dim, int64_t id_base, const float* queries, int n_queries,
                                  int k, int kprime, const int32_t* doc_coll,
                                  const int32_t* query_coll, double* out_scores, int64_t* out_ids,
                                  int32_t* out_counts, uint32_t* out_flags, void* workspace,
                                  size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    int rc = dense_args_ok(docs, dnorm, inv_norm, queries, out_scores, out_ids, out_counts,
                           out_flags, workspace, n_docs, n_queries, k, kprime);
    if (rc) return rc;
    if ((rc = f16_args_ok(docs, docs16, doc_rel_err, n_docs, dim, n_queries, doc_coll, query_coll))) return rc;
    const DensePlan P = make_plan(workspace, n_docs, n_queries, kprime, KIND_F16, dim, docs16 != nullptr);
    THR_RETURN_IF(workspace_bytes < P.total, THR_ERR_WORKSPACE);
    const DenseIndex X{docs, inv_norm, n_docs, dim, dnorm, id_base, doc_coll,
                       reinterpret_cast<const _Float16*>(docs16), doc_rel_err};
    const DenseBatch B{queries, n_queries, k, kprime, query_coll, (hipStream_t)stream,
                       out_scores, out_ids, out_counts, out_flags};
    return dense_pipeline(P, X, B, DensePhase{});
}

extern "C" int thr_dense_shortlist_f16(const float* docs, const uint16_t* docs16, double doc_rel_err,
                                       const float* inv_norm, int64_t n_docs, int dim,
                                       const float* queries, int n_queries, int kprime,
                                       const int32_t* doc_coll, const int32_t* query_coll, int m,
                                       float* top_lb, void* workspace, size_t workspace_bytes,
                                       thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!docs || !inv_norm || !queries || !top_lb || !workspace, THR_ERR_INVALID);
    THR_RETURN_IF(n_docs <= 0 || n_queries <= 0 || kprime <= 0 || kprime > THR_DENSE_MAX_K || m <= 0 ||
                      m > THR_DENSE_MAX_K,
                  THR_ERR_INVALID);
    int rc = f16_args_ok(docs, docs16, doc_rel_err, n_docs, dim, n_queries, doc_coll, query_coll);
    if (rc) return rc;
    const DensePlan P = make_plan(workspace, n_docs, n_queries, kprime, KIND_F16, dim, docs16 != nullptr);
    THR_RETURN_IF(workspace_bytes < P.total, THR_ERR_WORKSPACE);
    // (nothing is rescored: no norms, no id base, no k, no outputs)
    const DenseIndex X{docs, inv_norm, n_docs, dim, nullptr, 0, doc_coll,
                       reinterpret_cast<const _Float16*>(docs16), doc_rel_err};
    const DenseBatch B{queries, n_queries, 0, kprime, query_coll, (hipStream_t)stream};
    return dense_pipeline(P, X, B, DensePhase{PIPE_SHORTLIST, top_lb, m});
}

extern "C" int thr_dense_finish_f16(const float* docs, const uint16_t* docs16, double doc_rel_err,
                                    const double* dnorm, const float* inv_norm, int64_t n_docs,
                                    int dim, int64_t id_base, const float* queries, int n_queries,
                                    int k, int kprime, const int32_t* doc_coll,
                                    const int32_t* query_coll, const float* gfloor,
                                    const float* top_lb_all, int n_shards, int m,
                                    double* out_scores, int64_t* out_ids, int32_t* out_counts,
                                    uint32_t* out_flags, void* workspace, size_t workspace_bytes,
                                    thr_stream_t stream) {
    clear_status();
    int rc = dense_args_ok(docs, dnorm, inv_norm, queries, out_scores, out_ids, out_counts,
                           out_flags, workspace, n_docs, n_queries, k, kprime);
    if (rc) return rc;
    if ((rc = f16_args_ok(docs, docs16, doc_rel_err, n_docs, dim, n_queries, doc_coll, query_coll))) return rc;
    THR_RETURN_IF(gfloor && top_lb_all, THR_ERR_INVALID);
    THR_RETURN_IF(top_lb_all && (n_shards <= 0 || m <= 0), THR_ERR_INVALID);
    THR_RETURN_IF(top_lb_all && (int64_t)n_shards * m > CS_BINS, THR_ERR_CAPACITY);
    const DensePlan P = make_plan(workspace, n_docs, n_queries, kprime, KIND_F16, dim, docs16 != nullptr);
    THR_RETURN_IF(workspace_bytes < P.total, THR_ERR_WORKSPACE);
    const DenseIndex X{docs, inv_norm, n_docs, dim, dnorm, id_base, doc_coll,
                       reinterpret_cast<const _Float16*>(docs16), doc_rel_err};
    const DenseBatch B{queries, n_queries, k, kprime, query_coll, (hipStream_t)stream,
                       out_scores, out_ids, out_counts, out_flags};
    return dense_pipeline(P, X, B, DensePhase{PIPE_FINISH, nullptr, m, gfloor, top_lb_all, n_shards});
}

// The filter scan alone, for timing.  tau (and the register-resident scan's query image) is whatever
// the last thr_dense_topk[_f16] on this workspace left (a realistic filter rate); the tile counters
// are reset so the lists never overflow across repeats.
static int scan_probe(const DensePlan& P, const DenseIndex& X, const DenseBatch& B) {
    if (!P.packed) {
        hipError_t e = hipMemsetAsync(P.tcnt, 0, sizeof(int) * P.ntiles, B.st);
        if (e != hipSuccess) return (int)e;
    }
    return launch_scan<MODE_FILTER>(P, X, B);
}

extern "C" int thr_dense_scan_probe(const float* docs, const float* inv_norm, int64_t n_docs,
                                    int dim, const float* queries, int n_queries, void* workspace,
                                    size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!docs || !inv_norm || !queries || !workspace, THR_ERR_INVALID);
    THR_RETURN_IF(dim <= 0 || dim % CHUNK != 0 || dim / CHUNK > 4, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n_docs <= 0 || n_docs >= (int64_t)1 << ROW_BITS || n_queries <= 0,
                  THR_ERR_INVALID);
    const DensePlan P = make_plan(workspace, n_docs, n_queries, 128, KIND_F32, dim, false);
    THR_RETURN_IF(workspace_bytes < P.total, THR_ERR_WORKSPACE);
    return scan_probe(P, DenseIndex{docs, inv_norm, n_docs, dim},
                      DenseBatch{queries, n_queries, 0, 128, nullptr, (hipStream_t)stream});
}

extern "C" int thr_dense_scan_probe_f16(const float* docs, const uint16_t* docs16,
                                        const float* inv_norm,
                                        int64_t n_docs, int dim, const float* queries,
                                        int n_queries, void* workspace, size_t workspace_bytes,
                                        thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF((!docs16 && !docs) || !inv_norm || !queries || !workspace, THR_ERR_INVALID);
    THR_RETURN_IF(!f16_dim_ok(dim, docs16 != nullptr), THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n_docs <= 0 || n_docs >= (int64_t)1 << ROW_BITS_F16 || n_queries <= 0,
                  THR_ERR_INVALID);
    THR_RETURN_IF(docs16 != nullptr && n_queries > qreg_max_queries(dim), THR_ERR_UNSUPPORTED);
    const DensePlan P = make_plan(workspace, n_docs, n_queries, 128, KIND_F16, dim, docs16 != nullptr);
    THR_RETURN_IF(workspace_bytes < P.total, THR_ERR_WORKSPACE);
    DenseIndex X{docs, inv_norm, n_docs, dim};
    X.docs16 = reinterpret_cast<const _Float16*>(docs16);
    return scan_probe(P, X, DenseBatch{queries, n_queries, 0, 128, nullptr, (hipStream_t)stream});
}

extern "C" int thr_dense_scan_stamps_f16(const uint16_t* docs16, int64_t n_docs, int dim,
                                         int n_queries, void* workspace, size_t workspace_bytes,
                                         unsigned long long* stamps, int* h_n_waves,
                                         thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!docs16 || !workspace || !h_n_waves, THR_ERR_INVALID);
    THR_RETURN_IF(dim != 512 && dim != 768 && dim != 1024, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n_docs <= 0 || n_queries <= 0, THR_ERR_INVALID);
    THR_RETURN_IF(n_queries > qreg_max_queries(dim), THR_ERR_UNSUPPORTED);
    const DensePlan P = make_plan(workspace, n_docs, n_queries, 128, KIND_F16, dim, true);
    THR_RETURN_IF(workspace_bytes < P.total, THR_ERR_WORKSPACE);
    int blocks = 0;
    int rc = launch_scan_f16q<MODE_FILTER, true>(
        dim, reinterpret_cast<const _Float16*>(docs16), P.qfrag, P.ntiles, P.groups, 1, P.tau, P.cnt,
        P.cand, nullptr, (hipStream_t)stream, nullptr, nullptr, nullptr, n_queries, stamps, &blocks);
    // rows of 8 words: one per wave of the 4-wave-block kernel, two per wave of the staggered one
    *h_n_waves = blocks * qreg_waves(dim) * (qreg_staggered(dim) ? 2 : 1);
    return rc;
}
