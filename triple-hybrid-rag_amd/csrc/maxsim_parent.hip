// Child -> parent expansion of the funnel on the device (include/thr_hip_parent.h holds the contract):
// the groups of a fused list, and MaxSim of a query against the PARENT of a candidate -- the concatenation
// of the token blocks of every row that names the same parent -- over the float16 packed store and over the
// FP8 store.
//
// Stands where the reference expands children to parents and reranks ``c.parent_text or c.text``
// (src/voice_agent/rag2/retrieval.py:118-201, :419): what is scored is the parent passage, two children
// of one parent get one score.
//
// Groups.  One workgroup per query, one thread per position of the fused row (at most 512).  The keys go
// to LDS; a thread finds its leader by a forward scan over the lower positions (n^2 / 2 LDS reads of a row
// of at most 512: set-up cost next to the scorer), the leaders are numbered by a ballot prefix count.  No
// atomics: every output word has one writer, the same bits every run.
//
// Scorer.  csrc/maxsim.hip's and csrc/maxsim_fp8.hip's kernels with another walk: one wave per (query,
// candidate), product formed transposed with v_mfma_f32_32x32x16_f16 (A = 32 doc tokens x 16 dims from the
// fragment-major image, B = 16 dims x 32 query tokens), per-lane max over doc tokens.  The wave walks the
// 32-token tiles of every child of the candidate's parent (par_rowptr / par_child, ascending rows) instead of
// the tiles of one document.  LOOP ORDER: query tile OUTER, as in the plain scorers -- the B fragments of
// one 32-query-token tile stay in registers while the family's tiles stream through; a query of q_tokens
// tokens reads the family q_tokens / 32 times, the first time from HBM, the rest from L2 (a family of 4 x
// 128 x 128 float16 tokens is 128 KiB).  The max over a family is a max over its tiles in any order, each
// tile's accumulator is the plain kernel's, so a family of one row gives the plain kernel's bits.
// The FP8 walk pairs tiles ACROSS children (the loads of two tiles go out before the first MFMA of the
// pair, whichever children they belong to); an odd total ends with a single tile.
// The kernel has no barrier and no LDS: waves of a workgroup have different trip counts and leave early.
// Every index is checked: a candidate outside the shard scores -inf, a parent number outside
// [0, n_parents) is a row on its own, a row pointer is clamped to [0, nnz], a child outside [0, n_docs)
// is skipped and never dereferenced.
// Algorithmic bytes per (q, c) at fan-out f: f * d_tokens * tok_dim * 2 (float16), f * d_tokens *
// (tok_dim + 4) (FP8), + 4 (parent_of) + 16 (two row pointers) + 4 f (children).
#include "thr_common.hpp"

#include "../../include/thr_hip_parent.h"

namespace thr {

typedef _Float16 mp_half2 __attribute__((ext_vector_type(2)));
typedef _Float16 mp_half8 __attribute__((ext_vector_type(8)));
typedef float mp_f32x4 __attribute__((ext_vector_type(4)));
typedef float mp_f32x16 __attribute__((ext_vector_type(16)));
typedef uint32_t mp_u32x4 __attribute__((ext_vector_type(4)));

constexpr int MP_THREADS = 256;
constexpr int MP_WAVES = MP_THREADS / WAVE;
constexpr int PG_THREADS = THR_RRF_MAX_TOP_K;   // one thread per position of a fused row
constexpr int PG_WAVES = PG_THREADS / WAVE;

// ------------------------------------------------------------------------------------------- groups
__global__ __launch_bounds__(PG_THREADS) void parent_groups_kernel(
    const int64_t* __restrict__ ids, const int32_t* __restrict__ counts, const int32_t* __restrict__ parent_of,
    int64_t n_docs, int64_t id_base, int n, int32_t* __restrict__ leader, int32_t* __restrict__ slot,
    int64_t* __restrict__ uniq_ids, int32_t* __restrict__ n_uniq) {
    __shared__ int32_t key[PG_THREADS];     // parent number, or -1 - p: a key of position p's own
    __shared__ int32_t rank[PG_THREADS];    // of a leader: its place in the unique list
    __shared__ int32_t wave_sum[PG_WAVES];
    const int64_t q = blockIdx.x;
    const int p = threadIdx.x;
    const int lane = p & 63, wave = p >> 6;
    int cnt = n;
    if (counts) {
        cnt = counts[q];
        cnt = cnt < 0 ? 0 : (cnt > n ? n : cnt);
    }
    const bool live = p < cnt;
    int64_t id = -1;
    int32_t k = -1 - p;
    if (live) {
        id = ids[q * n + p];
        const int64_t row = id >= 0 ? id - id_base : -1;
        if (row >= 0 && row < n_docs) {
            const int32_t par = parent_of[row];
            if (par >= 0) k = par;
        }
    }
    key[p] = k;
    __syncthreads();
    int l = -1;
    if (live) {
        l = p;
        if (k >= 0) {
            for (int j = 0; j < p; ++j) {
                if (key[j] == k) {
                    l = j;
                    break;
                }
            }
        }
    }
    const bool is_leader = live && l == p;
    // exclusive prefix count of the leaders: inside the wave by ballot, across the waves through LDS
    const unsigned long long bal = __ballot(is_leader);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wave_sum[wave] = __popcll(bal);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < PG_WAVES; ++w) {
        const int s = wave_sum[w];
        if (w < wave) base += s;
        total += s;
    }
    rank[p] = is_leader ? base + before : -1;
    __syncthreads();
    if (p < n) {
        leader[q * n + p] = l;
        slot[q * n + p] = l >= 0 ? rank[l] : -1;
        if (p >= total) uniq_ids[q * n + p] = -1;      // padding behind the unique list
    }
    if (is_leader) uniq_ids[q * n + base + before] = id;
    if (p == 0) n_uniq[q] = total;
}

// ------------------------------------------------------------------------------------------- the walk
// The tiles of a candidate's family in row order, wave-uniform: children par_child[i], i in [lo, hi), or the
// candidate row alone; a child outside [0, n_docs) is skipped.
struct FamilyWalk {
    const int32_t* child_list;   // nullptr: the candidate row alone
    int64_t i, hi;
    int32_t self;
    int32_t n_docs;
    int tiles;
    int32_t child;
    int t;

    __device__ __forceinline__ void start(int64_t lo) {
        i = lo;
        t = 0;
        child = -1;
    }
    // -> is there a tile?  (child, t) names it; step() moves on
    __device__ __forceinline__ bool more() {
        while (i < hi) {
            if (t > 0) return true;
            child = child_list ? child_list[i] : self;
            if (child >= 0 && child < n_docs) return true;
            ++i;
        }
        return false;
    }
    __device__ __forceinline__ void step() {
        if (++t == tiles) {
            t = 0;
            ++i;
        }
    }
};

// the candidate -> its local row, or -1 (negative id, another shard, out of range)
__device__ __forceinline__ int64_t candidate_row(const int64_t* __restrict__ cand_ids, int64_t at, int64_t id_base,
                                                 int64_t n_docs) {
    const int64_t g = cand_ids[at];
    const int64_t row = g >= 0 ? g - id_base : -1;
    return row >= 0 && row < n_docs ? row : -1;
}

__device__ __forceinline__ void family_of(FamilyWalk& w, int64_t& lo, int64_t row, const int32_t* __restrict__ parent_of,
                                          const int64_t* __restrict__ par_rowptr, const int32_t* __restrict__ par_child,
                                          int n_parents, int64_t nnz, int64_t n_docs, int tiles) {
    w.n_docs = (int32_t)n_docs;
    w.tiles = tiles;
    w.self = (int32_t)row;
    w.child_list = nullptr;
    lo = 0;
    w.hi = 1;
    const int32_t par = parent_of[row];
    if (par >= 0 && par < n_parents) {
        int64_t a = par_rowptr[par], b = par_rowptr[par + 1];
        a = a < 0 ? 0 : (a > nnz ? nnz : a);
        b = b < a ? a : (b > nnz ? nnz : b);
        w.child_list = par_child;
        lo = a;
        w.hi = b;
    }
}

__device__ __forceinline__ float sum_of_maxima(float mx) {
    mx = fmaxf(mx, __shfl_xor(mx, 32, WAVE));  // the two 16-row halves of every tile
    float s = mx;
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) s += __shfl_xor(s, m, WAVE);
    return s;
}

// ------------------------------------------------------------------------------------------- float16
template <int KSTEPS>
__global__ __launch_bounds__(MP_THREADS) void maxsim_parent_kernel(
    const _Float16* __restrict__ qtok, int q_tokens, const _Float16* __restrict__ dtok, int64_t n_docs,
    int d_tokens, const int64_t* __restrict__ cand_ids, int64_t id_base, int n_cand,
    const int32_t* __restrict__ parent_of, const int64_t* __restrict__ par_rowptr,
    const int32_t* __restrict__ par_child, int n_parents, int64_t nnz, float* __restrict__ out) {
    constexpr int TD = KSTEPS * 16;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = blockIdx.y;
    const int c = blockIdx.x * MP_WAVES + wave;
    if (c >= n_cand) return;
    const int64_t at = (int64_t)q * n_cand + c;
    const int64_t row = candidate_row(cand_ids, at, id_base, n_docs);
    if (row < 0) {
        if (lane == 0) out[at] = -INFINITY;
        return;
    }
    const int tiles = d_tokens / 32;
    FamilyWalk w;
    int64_t lo;
    family_of(w, lo, row, parent_of, par_rowptr, par_child, n_parents, nnz, n_docs, tiles);
    const int r = lane & 31, h = lane >> 5;
    float total = 0.f;
    for (int n0 = 0; n0 < q_tokens; n0 += 32) {
        // B fragments of this 32-query-token tile: lane holds Q[n0 + r][16*ks + 8*h + j]
        mp_half8 bq[KSTEPS];
        const _Float16* Q = qtok + ((int64_t)q * q_tokens + n0 + r) * TD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) bq[ks] = *reinterpret_cast<const mp_half8*>(Q + 16 * ks);
        float mx = -INFINITY;
        for (w.start(lo); w.more(); w.step()) {
            const mp_half8* tile = reinterpret_cast<const mp_half8*>(dtok + (int64_t)w.child * d_tokens * TD) +
                                   (int64_t)w.t * KSTEPS * 64 + lane;
            mp_half8 a[KSTEPS];
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks) a[ks] = __builtin_nontemporal_load(tile + ks * 64);
            mp_f32x16 acc;
#pragma unroll
            for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
            for (int ks = 0; ks < KSTEPS; ++ks)
                acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a[ks], bq[ks], acc, 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 16; ++i) mx = fmaxf(mx, acc[i]);
        }
        total += sum_of_maxima(mx);
    }
    if (lane == 0) out[at] = total;
}

// ------------------------------------------------------------------------------------------- FP8
template <int KPAIRS>
struct ParTile8 {
    mp_u32x4 c[KPAIRS];
    mp_f32x4 s[4];
};

template <int KPAIRS>
__device__ __forceinline__ void par_tile8_load(ParTile8<KPAIRS>& t, const uint8_t* __restrict__ codes,
                                               const float* __restrict__ scales, int64_t child, int d_tokens,
                                               int tile, int lane) {
    const mp_u32x4* p = reinterpret_cast<const mp_u32x4*>(codes + child * (int64_t)d_tokens * (KPAIRS * 32)) +
                        (int64_t)tile * KPAIRS * 64 + lane;
#pragma unroll
    for (int kp = 0; kp < KPAIRS; ++kp) t.c[kp] = __builtin_nontemporal_load(p + kp * 64);
    const float* sc = scales + child * (int64_t)d_tokens + tile * 32 + 4 * (lane >> 5);
#pragma unroll
    for (int g = 0; g < 4; ++g) t.s[g] = *reinterpret_cast<const mp_f32x4*>(sc + 8 * g);
}

// eight codes (two words) -> the float16 A fragment of one k-step; byte 0 of a word is the lower dim
__device__ __forceinline__ mp_half8 par_dequant8(uint32_t w0, uint32_t w1) {
    const mp_half2 a = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, false);
    const mp_half2 b = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w0, 1.0f, true);
    const mp_half2 c = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, false);
    const mp_half2 d = __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w1, 1.0f, true);
    mp_half8 o;
    o[0] = a[0]; o[1] = a[1]; o[2] = b[0]; o[3] = b[1];
    o[4] = c[0]; o[5] = c[1]; o[6] = d[0]; o[7] = d[1];
    return o;
}

template <int KPAIRS>
__device__ __forceinline__ float par_tile8_max(const ParTile8<KPAIRS>& t, const mp_half8 (&bq)[2 * KPAIRS], float mx) {
    mp_f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[i] = 0.f;
#pragma unroll
    for (int kp = 0; kp < KPAIRS; ++kp) {
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(par_dequant8(t.c[kp][0], t.c[kp][1]), bq[2 * kp], acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(par_dequant8(t.c[kp][2], t.c[kp][3]), bq[2 * kp + 1], acc, 0, 0, 0);
    }
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, acc[i] * t.s[i >> 2][i & 3]);
    return mx;
}

template <int KPAIRS>
__global__ __launch_bounds__(MP_THREADS) void maxsim_parent_fp8_kernel(
    const _Float16* __restrict__ qtok, int q_tokens, const uint8_t* __restrict__ codes,
    const float* __restrict__ scales, int64_t n_docs, int d_tokens, const int64_t* __restrict__ cand_ids,
    int64_t id_base, int n_cand, const int32_t* __restrict__ parent_of, const int64_t* __restrict__ par_rowptr,
    const int32_t* __restrict__ par_child, int n_parents, int64_t nnz, float* __restrict__ out) {
    constexpr int TD = KPAIRS * 32;
    constexpr int KSTEPS = KPAIRS * 2;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q = blockIdx.y;
    const int c = blockIdx.x * MP_WAVES + wave;
    if (c >= n_cand) return;
    const int64_t at = (int64_t)q * n_cand + c;
    const int64_t row = candidate_row(cand_ids, at, id_base, n_docs);
    if (row < 0) {
        if (lane == 0) out[at] = -INFINITY;
        return;
    }
    const int tiles = d_tokens / 32;
    FamilyWalk w;
    int64_t lo;
    family_of(w, lo, row, parent_of, par_rowptr, par_child, n_parents, nnz, n_docs, tiles);
    const int r = lane & 31, h = lane >> 5;
    float total = 0.f;
    for (int n0 = 0; n0 < q_tokens; n0 += 32) {
        // B fragments of this 32-query-token tile: lane holds Q[n0 + r][16*ks + 8*h + j]
        mp_half8 bq[KSTEPS];
        const _Float16* Q = qtok + ((int64_t)q * q_tokens + n0 + r) * TD + 8 * h;
#pragma unroll
        for (int ks = 0; ks < KSTEPS; ++ks) bq[ks] = *reinterpret_cast<const mp_half8*>(Q + 16 * ks);
        float mx = -INFINITY;
        w.start(lo);
        while (w.more()) {
            ParTile8<KPAIRS> t0;
            par_tile8_load<KPAIRS>(t0, codes, scales, w.child, d_tokens, w.t, lane);
            w.step();
            if (w.more()) {     // the loads of both tiles go out before the first MFMA
                ParTile8<KPAIRS> t1;
                par_tile8_load<KPAIRS>(t1, codes, scales, w.child, d_tokens, w.t, lane);
                w.step();
                __builtin_amdgcn_sched_barrier(0);
                mx = par_tile8_max<KPAIRS>(t0, bq, mx);
                mx = par_tile8_max<KPAIRS>(t1, bq, mx);
            } else {
                mx = par_tile8_max<KPAIRS>(t0, bq, mx);
            }
        }
        total += sum_of_maxima(mx);
    }
    if (lane == 0) out[at] = total;
}

}  // namespace thr

using namespace thr;

// tok_dim / 16 of the float16 scorer's instantiations and tok_dim / 32 of the FP8 scorer's: the lists of
// csrc/maxsim.hip (THR_MS_KSTEPS) and csrc/maxsim_fp8.hip (THR_M8_KPAIRS), restated, not shared -- those
// files stay as they are, to the byte of their object code; tests/test_parent_host.py holds the entry points
// here to _native.MAXSIM_TOK_DIMS / MAXSIM_FP8_TOK_DIMS dim by dim.
#define THR_MP_KSTEPS(X) X(1) X(2) X(4) X(6) X(8) X(12) X(16)
#define THR_MP_KPAIRS(X) X(1) X(2) X(3) X(4) X(6) X(8)

static bool mp_tok_dim_supported(int tok_dim, bool fp8) {
    const int unit = fp8 ? 32 : 16;
    if (tok_dim <= 0 || tok_dim % unit) return false;
    if (fp8) {
        switch (tok_dim / 32) {
#define THR_MP_LABEL(K) case K:
            THR_MP_KPAIRS(THR_MP_LABEL)
            return true;
            default:
                return false;
        }
    }
    switch (tok_dim / 16) {
        THR_MP_KSTEPS(THR_MP_LABEL)
#undef THR_MP_LABEL
        return true;
        default:
            return false;
    }
}

// Shapes are refused before any pointer is looked at (host arithmetic: no GPU needed to ask).
static bool mp_tokens_supported(int n_tokens, int tok_dim, bool fp8) {
    return n_tokens > 0 && n_tokens % 32 == 0 && mp_tok_dim_supported(tok_dim, fp8);
}

// Largest gridDim.x / gridDim.y of the current device (2^31 - 1 / 65535 when it cannot be asked)
static void mp_max_grid(int* gx, int* gy) {
    static int x = 0, y = 0;
    if (!x) {
        int dev = 0;
        hipDeviceProp_t prop;
        int px = 0, py = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) {
            px = prop.maxGridSize[0];
            py = prop.maxGridSize[1];
        }
        y = py > 0 ? py : 65535;
        x = px > 0 ? px : 0x7fffffff;
    }
    *gx = x;
    *gy = y;
}

extern "C" int thr_parent_groups(const int64_t* ids, const int32_t* counts, int n_queries, int n,
                                 const int32_t* parent_of, int64_t n_docs, int64_t id_base, int32_t* out_leader,
                                 int32_t* out_slot, int64_t* out_uniq_ids, int32_t* out_n_uniq,
                                 thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(n < 1 || n > THR_RRF_MAX_TOP_K, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!ids || !parent_of || !out_leader || !out_slot || !out_uniq_ids || !out_n_uniq, THR_ERR_INVALID);
    THR_RETURN_IF(n_queries <= 0 || n_docs <= 0, THR_ERR_INVALID);
    int gx, gy;
    mp_max_grid(&gx, &gy);
    // queries sit on gridDim.x: a batch above the device's limit goes out in slices of at most that many
    for (int q0 = 0; q0 < n_queries; q0 += gx) {
        const int nq = n_queries - q0 < gx ? n_queries - q0 : gx;
        const int64_t off = (int64_t)q0 * n;
        hipLaunchKernelGGL(parent_groups_kernel, dim3((unsigned)nq), dim3(PG_THREADS), 0, (hipStream_t)stream,
                           ids + off, counts ? counts + q0 : nullptr, parent_of, n_docs, id_base, n,
                           out_leader + off, out_slot + off, out_uniq_ids + off, out_n_uniq + q0);
        if (n_queries - q0 <= gx) break;      // (q0 + gx may not fit an int)
    }
    return launch_status();
}

// the checks the two scorers share, in the order of the contract: shapes, then pointers, then counts
static int mp_check(bool fp8, const void* qtok, int n_queries, int q_tokens, const void* store, const void* scales,
                    int64_t n_docs, int d_tokens, int tok_dim, const void* cand_ids, int n_cand,
                    const void* parent_of, const void* par_rowptr, const void* par_child, int n_parents,
                    int64_t nnz, const void* out_scores) {
    THR_RETURN_IF(!mp_tokens_supported(q_tokens, tok_dim, fp8) || !mp_tokens_supported(d_tokens, tok_dim, fp8),
                  THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(n_docs > 0x7fffffffll, THR_ERR_UNSUPPORTED);      // children are int32 rows
    THR_RETURN_IF(!qtok || !store || (fp8 && !scales) || !cand_ids || !out_scores, THR_ERR_INVALID);
    THR_RETURN_IF(!parent_of || !par_rowptr || !par_child, THR_ERR_INVALID);
    THR_RETURN_IF(n_queries <= 0 || n_docs <= 0 || n_cand <= 0 || n_parents <= 0 || nnz <= 0, THR_ERR_INVALID);
    return THR_OK;
}

extern "C" int thr_maxsim_parent_ids(const uint16_t* qtok, int n_queries, int q_tokens, const uint16_t* dtok,
                                     int64_t n_docs, int d_tokens, int tok_dim, const int64_t* cand_ids,
                                     int64_t id_base, int n_cand, const int32_t* parent_of,
                                     const int64_t* par_rowptr, const int32_t* par_child, int n_parents,
                                     int64_t nnz, float* out_scores, thr_stream_t stream) {
    clear_status();
    const int rc = mp_check(false, qtok, n_queries, q_tokens, dtok, nullptr, n_docs, d_tokens, tok_dim, cand_ids,
                            n_cand, parent_of, par_rowptr, par_child, n_parents, nnz, out_scores);
    THR_RETURN_IF(rc != THR_OK, rc);
    const _Float16* Dk = reinterpret_cast<const _Float16*>(dtok);
    hipStream_t st = (hipStream_t)stream;
    int gx, slice;
    mp_max_grid(&gx, &slice);
    // queries sit on gridDim.y: a batch above the device's limit goes out in slices of at most
    // that many queries, each a launch of its own over its rows of qtok, cand_ids and out
    for (int q0 = 0; q0 < n_queries; q0 += slice) {
        dim3 grid((n_cand + MP_WAVES - 1) / MP_WAVES, n_queries - q0 < slice ? n_queries - q0 : slice);
        const _Float16* Q = reinterpret_cast<const _Float16*>(qtok) + (int64_t)q0 * q_tokens * tok_dim;
        const int64_t* G = cand_ids + (int64_t)q0 * n_cand;
        float* out = out_scores + (int64_t)q0 * n_cand;
#define THR_MP_CASE(KS)                                                                                     \
    case KS:                                                                                                \
        hipLaunchKernelGGL((maxsim_parent_kernel<KS>), grid, dim3(MP_THREADS), 0, st, Q, q_tokens, Dk,      \
                           n_docs, d_tokens, G, id_base, n_cand, parent_of, par_rowptr, par_child,          \
                           n_parents, nnz, out);                                                            \
        break;
        switch (tok_dim / 16) {
            THR_MP_KSTEPS(THR_MP_CASE)
            default:
                return THR_ERR_UNSUPPORTED;
        }
#undef THR_MP_CASE
    }
    return launch_status();
}

extern "C" int thr_maxsim_parent_fp8_ids(const uint16_t* qtok, int n_queries, int q_tokens, const uint8_t* codes,
                                         const float* scales, int64_t n_docs, int d_tokens, int tok_dim,
                                         const int64_t* cand_ids, int64_t id_base, int n_cand,
                                         const int32_t* parent_of, const int64_t* par_rowptr,
                                         const int32_t* par_child, int n_parents, int64_t nnz,
                                         float* out_scores, thr_stream_t stream) {
    clear_status();
    const int rc = mp_check(true, qtok, n_queries, q_tokens, codes, scales, n_docs, d_tokens, tok_dim, cand_ids,
                            n_cand, parent_of, par_rowptr, par_child, n_parents, nnz, out_scores);
    THR_RETURN_IF(rc != THR_OK, rc);
    hipStream_t st = (hipStream_t)stream;
    int gx, slice;
    mp_max_grid(&gx, &slice);
    for (int q0 = 0; q0 < n_queries; q0 += slice) {
        dim3 grid((n_cand + MP_WAVES - 1) / MP_WAVES, n_queries - q0 < slice ? n_queries - q0 : slice);
        const _Float16* Q = reinterpret_cast<const _Float16*>(qtok) + (int64_t)q0 * q_tokens * tok_dim;
        const int64_t* G = cand_ids + (int64_t)q0 * n_cand;
        float* out = out_scores + (int64_t)q0 * n_cand;
#define THR_MP_CASE(KP)                                                                                     \
    case KP:                                                                                                \
        hipLaunchKernelGGL((maxsim_parent_fp8_kernel<KP>), grid, dim3(MP_THREADS), 0, st, Q, q_tokens,      \
                           codes, scales, n_docs, d_tokens, G, id_base, n_cand, parent_of, par_rowptr,      \
                           par_child, n_parents, nnz, out);                                                 \
        break;
        switch (tok_dim / 32) {
            THR_MP_KPAIRS(THR_MP_CASE)
            default:
                return THR_ERR_UNSUPPORTED;
        }
#undef THR_MP_CASE
    }
    return launch_status();
}
