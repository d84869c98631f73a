// Typo-tolerant lexical queries (include/thr_hip_fuzzy.h holds the contract): for each unknown token of a batch
// the vocabulary terms within a small edit distance, and the query table with those corrections folded in.
//
// fz_needles     one thread per unknown token: its bytes lowered through the character table into uint16 code
//                points (a row of the needle table) and its length (0: no correction is sought); its best slots
//                set to FZ_EMPTY.
// fz_rank        one workgroup: the place of every needle in the order by length (a counting sort made of block
//                scans, one per length: deterministic, no atomics) and where each length begins.
// fz_scatter     one thread per needle: its row to its place, so that the needles of one length lie together.
// fz_scan_keys   ONE pass over the key store.  A workgroup stages a slice of THR_FUZZY_SLICE_BYTES key bytes in
//                LDS, with the halo the longest key that can still match needs behind it; a lane owns one key that
//                BEGINS in the slice, decodes it once into a column of LDS, and meets only the needles of L - d ..
//                L + d code points, which the workgroup stages in LDS in batches.  Per pair the banded edit
//                distance of fuzzy_common.hpp; a match goes into the needle's slots by the chain of 64-bit minima.
// fz_write       one thread per needle: the slots unpacked into near_term / near_dist.
// fz_unknowns    one wave per query: its token rows with term -1, counted (their scan names unknown u of a row).
// fz_query_terms one wave per query over its token rows, 64 at a time, each with up to n_use candidates: the
//                distinct ids in order of first appearance, a known token's id and an unknown token's corrections
//                at the token's place.
// Nothing waits for another workgroup, nothing is read back, every output is the same bits every run whatever
// the workspace held.
#include "fuzzy_common.hpp"

namespace thr {

constexpr int FZ_THREADS = 256;
constexpr int FZ_WAVES = FZ_THREADS / WAVE;
constexpr int FZ_SLICE = THR_FUZZY_SLICE_BYTES;
constexpr int FZ_HALO = 112;                           // >= FZ_MAX_KEY_BYTES, in 16-byte pieces
constexpr int FZ_LDS = FZ_SLICE + FZ_HALO;
constexpr int FZ_BATCH = 64;                           // needles staged at a time
constexpr int FZ_ROW = FZ_MAX_LEN;                     // uint16 per needle in the tables
constexpr int FZ_ROW_LDS = FZ_MAX_LEN + 2;             // 17 words: needles of one column on different banks
constexpr int FZ_LENGTHS = FZ_MAX_LEN + 2;             // start[n], n = 0 .. FZ_MAX_LEN + 1
constexpr int FZ_SCAN_THREADS = 1024;
static_assert(FZ_HALO >= FZ_MAX_KEY_BYTES && FZ_HALO % 16 == 0 && FZ_SLICE % 16 == 0, "slices are staged in 16-byte pieces");
static_assert(FZ_BATCH * FZ_ROW / 2 == 4 * FZ_THREADS, "a batch is staged four words a thread");

__device__ __forceinline__ int64_t fz_count(const int32_t* n_unknown, int64_t capacity) {
    const int64_t n = *n_unknown;
    return n < 0 ? 0 : n < capacity ? n : capacity;
}

__global__ __launch_bounds__(FZ_THREADS) void fz_needles(const uint8_t* __restrict__ text, int64_t n_bytes,
                                                         const uint32_t* __restrict__ table,
                                                         const int64_t* __restrict__ unknown_off,
                                                         const int32_t* __restrict__ unknown_len,
                                                         const int32_t* __restrict__ n_unknown, int64_t capacity,
                                                         int max_edits, int n_best, uint16_t* __restrict__ cps,
                                                         int32_t* __restrict__ nlen, unsigned long long* __restrict__ slots) {
    const int64_t u = (int64_t)blockIdx.x * FZ_THREADS + threadIdx.x;
    if (u >= fz_count(n_unknown, capacity)) return;
    int64_t a = unknown_off[u];
    a = a < 0 ? 0 : a < n_bytes ? a : n_bytes;
    int64_t l = unknown_len[u];
    l = l < 0 ? 0 : l < n_bytes - a ? l : n_bytes - a;
    const int n = fz_lower_needle(text, a, a + l, table, cps + u * FZ_ROW);
    nlen[u] = n >= FZ_MIN_LEN && fz_edits(n, max_edits) > 0 ? n : 0;
    for (int j = 0; j < n_best; ++j) slots[u * n_best + j] = FZ_EMPTY;
}

// rank[u]: the place of needle u among the needles ordered by (length, u); start[n]: the needles shorter than n.
__global__ __launch_bounds__(FZ_SCAN_THREADS) void fz_rank(const int32_t* __restrict__ nlen,
                                                           const int32_t* __restrict__ n_unknown, int64_t capacity,
                                                           int32_t* __restrict__ rank, int32_t* __restrict__ start) {
    __shared__ int32_t tmp[FZ_SCAN_THREADS];
    const int64_t nu = fz_count(n_unknown, capacity);
    const int64_t per = (nu + FZ_SCAN_THREADS - 1) / FZ_SCAN_THREADS;
    const int64_t a = per * threadIdx.x < nu ? per * threadIdx.x : nu, b = a + per < nu ? a + per : nu;
    int32_t base = 0;
    for (int n = 0; n < FZ_MIN_LEN; ++n)
        if (threadIdx.x == 0) start[n] = 0;
#pragma unroll 1
    for (int n = FZ_MIN_LEN; n <= FZ_MAX_LEN; ++n) {
        int32_t c = 0;
        for (int64_t i = a; i < b; ++i) c += nlen[i] == n;
        tmp[threadIdx.x] = c;
        block_inclusive_scan<FZ_SCAN_THREADS>(tmp);
        int32_t run = base + tmp[threadIdx.x] - c;
        const int32_t total = tmp[FZ_SCAN_THREADS - 1];
        __syncthreads();                       // (tmp is written again in the next round)
        for (int64_t i = a; i < b; ++i)
            if (nlen[i] == n) rank[i] = run++;
        if (threadIdx.x == 0) start[n] = base;
        base += total;
    }
    if (threadIdx.x == 0) start[FZ_MAX_LEN + 1] = base;
}

__global__ __launch_bounds__(FZ_THREADS) void fz_scatter(const uint16_t* __restrict__ cps, const int32_t* __restrict__ nlen,
                                                         const int32_t* __restrict__ rank,
                                                         const int32_t* __restrict__ n_unknown, int64_t capacity,
                                                         uint16_t* __restrict__ s_cps, int32_t* __restrict__ s_len,
                                                         int32_t* __restrict__ s_u) {
    const int64_t u = (int64_t)blockIdx.x * FZ_THREADS + threadIdx.x;
    if (u >= fz_count(n_unknown, capacity)) return;
    const int n = nlen[u];
    if (n < FZ_MIN_LEN) return;
    const int64_t r = rank[u];
    const uint4* src = reinterpret_cast<const uint4*>(cps + u * FZ_ROW);
    uint4* dst = reinterpret_cast<uint4*>(s_cps + r * FZ_ROW);
#pragma unroll
    for (int j = 0; j < FZ_ROW * 2 / 16; ++j) dst[j] = src[j];
    s_len[r] = n;
    s_u[r] = (int32_t)u;
}

struct KeyStore {
    const uint8_t* bytes;      // as handed in; ``shift`` = its address mod 16
    const int64_t* ptr;        // [n + 1]
    const int64_t* rowptr;     // [n + 1] or null
    int64_t n, n_bytes;
    int shift;
};

// W: the half width of the band = max_edits.
template <int W>
__global__ __launch_bounds__(FZ_THREADS) void fz_scan_keys(KeyStore K, const uint16_t* __restrict__ s_cps,
                                                           const int32_t* __restrict__ s_len,
                                                           const int32_t* __restrict__ s_u,
                                                           const int32_t* __restrict__ start, int n_best,
                                                           unsigned long long* __restrict__ slots) {
    __shared__ __attribute__((aligned(16))) uint8_t text[FZ_LDS];
    __shared__ uint16_t key[FZ_MAX_KEY_CPS * FZ_THREADS];          // key[i * FZ_THREADS + thread]: its key's i-th code point
    __shared__ __attribute__((aligned(16))) uint16_t needle[FZ_BATCH * FZ_ROW_LDS];
    __shared__ int32_t needle_len[FZ_BATCH], needle_u[FZ_BATCH];
    __shared__ int32_t begin[FZ_LENGTHS];
    __shared__ int64_t keys[2];
    __shared__ int32_t span[2];
    if (threadIdx.x < FZ_LENGTHS) begin[threadIdx.x] = start[threadIdx.x];
    // the slice in the coordinates of the 16-byte aligned address below ``bytes``: LDS byte i is key-store byte v0 + i
    const int64_t v0 = (int64_t)blockIdx.x * FZ_SLICE - K.shift;
    const uint8_t* aligned = K.bytes - K.shift;
    for (int i = threadIdx.x * 16; i < FZ_LDS; i += FZ_THREADS * 16) {
        const int64_t g = v0 + i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g >= 0 && g + 16 <= K.n_bytes) {
            v = *reinterpret_cast<const uint4*>(aligned + (g + K.shift));
        } else if (g + 16 > 0 && g < K.n_bytes) {
            uint8_t* b = reinterpret_cast<uint8_t*>(&v);
            for (int j = 0; j < 16; ++j)
                if (g + j >= 0 && g + j < K.n_bytes) b[j] = K.bytes[g + j];
        }
        *reinterpret_cast<uint4*>(text + i) = v;
    }
    // the keys that begin in the slice: ptr ascends
    if (threadIdx.x == 0) keys[0] = tx_upper(K.ptr, 0, K.n, v0 - 1);
    if (threadIdx.x == 64) keys[1] = tx_upper(K.ptr, 0, K.n, v0 + FZ_SLICE - 1);
    __syncthreads();
    if (begin[FZ_MAX_LEN + 1] == 0) return;                        // no needle at all
    const int64_t t_lo = keys[0], t_hi = keys[1];
    uint16_t* mine = key + threadIdx.x;
#pragma unroll 1
    for (int64_t t0 = t_lo; t0 < t_hi; t0 += FZ_THREADS) {
        __syncthreads();                                           // the round before is done: its span read, its last batch used
        if (threadIdx.x == 0) {
            span[0] = INT32_MAX;
            span[1] = 0;
        }
        __syncthreads();
        // ---- this lane's key: code points into its column, frequency, the needles it can meet
        const int64_t t = t0 + threadIdx.x;
        int L = 0;
        int64_t df = 0;
        if (t < t_hi) {
            const int64_t ka = K.ptr[t];
            int64_t kb = K.ptr[t + 1];
            kb = kb < K.n_bytes ? kb : K.n_bytes;
            const int64_t bytes = kb - ka;
            bool ok = ka >= v0 && ka >= 0 && ka < v0 + FZ_SLICE && bytes >= 1 && bytes <= FZ_MAX_KEY_BYTES;
            if (ok && K.rowptr) {
                df = K.rowptr[t + 1] - K.rowptr[t];
                ok = df > 0;                                       // a term without postings corrects nothing
            }
            if (ok) {
                const uint8_t* p = text + (ka - v0);               // [0, FZ_SLICE) + at most FZ_MAX_KEY_BYTES: staged
                int at = 0, n = 0;
                while (at < (int)bytes && ok) {
                    const int avail = (int)bytes - at;
                    int len;
                    const int cp = fz_key_cp(p[at], avail > 1 ? p[at + 1] : 0, avail > 2 ? p[at + 2] : 0, avail, len);
                    if (cp < 0 || n == FZ_MAX_KEY_CPS) {
                        ok = false;
                    } else {
                        mine[n++ * FZ_THREADS] = (uint16_t)cp;
                        at += len;
                    }
                }
                L = ok ? n : 0;
            }
        }
        int lo = 0, hi = 0;                                        // its needles: places lo .. hi - 1 of the order by length
        if (L > 0) {
            const int n_lo = L - W > FZ_MIN_LEN ? L - W : FZ_MIN_LEN, n_hi = L + W < FZ_MAX_LEN ? L + W : FZ_MAX_LEN;
            if (n_lo <= n_hi) {
                lo = begin[n_lo];
                hi = begin[n_hi + 1];
            }
        }
        if (lo < hi) {
            atomicMin(&span[0], lo);
            atomicMax(&span[1], hi);
        }
        __syncthreads();
        const int s_lo = span[0], s_hi = span[1];
#pragma unroll 1
        for (int r0 = s_lo; r0 < s_hi; r0 += FZ_BATCH) {           // (s_lo >= s_hi: no lane has a needle to meet)
            __syncthreads();                                       // span is read, the batch before is done with
            {
                // FZ_BATCH rows of FZ_ROW uint16 = 16 words each, four words a thread; rows behind s_hi stay unread
                const int row = threadIdx.x / 4, w0 = (threadIdx.x % 4) * 4;
                if (r0 + row < s_hi) {
                    const uint4 v = *reinterpret_cast<const uint4*>(s_cps + (int64_t)(r0 + row) * FZ_ROW + w0 * 2);
                    uint32_t* dst = reinterpret_cast<uint32_t*>(needle + row * FZ_ROW_LDS) + w0;
                    dst[0] = v.x;
                    dst[1] = v.y;
                    dst[2] = v.z;
                    dst[3] = v.w;
                }
                if (threadIdx.x < FZ_BATCH && r0 + (int)threadIdx.x < s_hi) {
                    needle_len[threadIdx.x] = s_len[r0 + threadIdx.x];
                    needle_u[threadIdx.x] = s_u[r0 + threadIdx.x];
                }
            }
            __syncthreads();
            const int a = lo > r0 ? lo : r0, b = hi < r0 + FZ_BATCH ? hi : r0 + FZ_BATCH;
            for (int r = a; r < b; ++r) {
                const int n = needle_len[r - r0];
                const int d = fz_edits(n, W);
                const int gap = L > n ? L - n : n - L;
                if (gap > d) continue;
                const int dist = fz_banded<W>(needle + (r - r0) * FZ_ROW_LDS, n, mine, FZ_THREADS, L, d);
                if (dist <= d)
                    fz_insert(slots + (int64_t)needle_u[r - r0] * n_best, n_best, fz_pack(dist, df, (int32_t)t));
            }
        }
    }
}

__global__ __launch_bounds__(FZ_THREADS) void fz_write(const unsigned long long* __restrict__ slots,
                                                       const int32_t* __restrict__ n_unknown, int64_t capacity,
                                                       int n_best, int32_t* __restrict__ near_term,
                                                       int32_t* __restrict__ near_dist) {
    const int64_t u = (int64_t)blockIdx.x * FZ_THREADS + threadIdx.x;
    if (u >= fz_count(n_unknown, capacity)) return;
    for (int j = 0; j < n_best; ++j) {
        const unsigned long long x = slots[u * n_best + j];
        near_term[u * n_best + j] = x == FZ_EMPTY ? -1 : (int32_t)(x & 0x7FFFFFFFull);
        near_dist[u * n_best + j] = x == FZ_EMPTY ? -1 : (int32_t)(x >> 62);
    }
}

// out[i] = in[0] + .. + in[i - 1] for i in 0 .. n (n + 1 values); one workgroup.  (text.hip's scan.)
__global__ __launch_bounds__(FZ_SCAN_THREADS) void fz_scan(const int32_t* in, int64_t n, int32_t* out) {
    __shared__ int32_t tmp[FZ_SCAN_THREADS];
    const int64_t per = (n + FZ_SCAN_THREADS - 1) / FZ_SCAN_THREADS;
    const int64_t a = per * threadIdx.x < n ? per * threadIdx.x : n, b = a + per < n ? a + per : n;
    int32_t s = 0;
    for (int64_t i = a; i < b; ++i) s += in[i];
    tmp[threadIdx.x] = s;
    block_inclusive_scan<FZ_SCAN_THREADS>(tmp);
    int32_t run = tmp[threadIdx.x] - s;
    for (int64_t i = a; i < b; ++i) {
        const int32_t v = in[i];     // (read before written: in and out may be one array)
        out[i] = run;
        run += v;
    }
    if (threadIdx.x == FZ_SCAN_THREADS - 1) out[n] = tmp[FZ_SCAN_THREADS - 1];
}

// The token rows of query q, clamped as thr_query_terms clamps them.
__device__ __forceinline__ void fz_rows(const int32_t* row_of, const int32_t* n_total, int64_t capacity, int64_t q,
                                        int64_t& a, int64_t& b) {
    int64_t limit = *n_total;
    limit = limit < capacity ? limit : capacity;
    limit = limit < 0 ? 0 : limit;
    a = row_of[q];
    b = row_of[q + 1];
    a = a < limit ? a : limit;
    b = b < limit ? b : limit;
}

__global__ __launch_bounds__(FZ_THREADS) void fz_unknowns(const int32_t* __restrict__ tok_term,
                                                          const int32_t* __restrict__ row_of,
                                                          const int32_t* __restrict__ n_total, int64_t capacity, int nq,
                                                          int32_t* __restrict__ unk_count) {
    const int lane = threadIdx.x % WAVE;
    const int64_t q = (int64_t)blockIdx.x * FZ_WAVES + threadIdx.x / WAVE;
    if (q >= nq) return;
    int64_t a, b;
    fz_rows(row_of, n_total, capacity, q, a, b);
    int c = 0;
    for (; a < b; a += WAVE) c += __popcll(__ballot(a + lane < b && tok_term[a + lane] < 0));
    if (lane == 0) unk_count[q] = c;
}

__global__ __launch_bounds__(FZ_THREADS) void fz_query_terms(const int32_t* __restrict__ tok_term,
                                                             const int32_t* __restrict__ row_of,    // [nq + 1]
                                                             const int32_t* __restrict__ unk_of,    // [nq + 1]
                                                             const int32_t* __restrict__ n_total, int64_t capacity,
                                                             const int32_t* __restrict__ text_flags, int nq,
                                                             const int32_t* __restrict__ near_term, int64_t near_capacity,
                                                             int n_best, int n_use, int32_t* __restrict__ out_terms,
                                                             int32_t* __restrict__ n_distinct, int32_t* __restrict__ out_flags) {
    constexpr int CAP = THR_BM25_MAX_TERMS + 1, C = THR_FUZZY_MAX_BEST;
    __shared__ int32_t list_all[FZ_WAVES][CAP];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t q = (int64_t)blockIdx.x * FZ_WAVES + wave;
    if (q >= nq) return;
    int32_t* list = list_all[wave];
    int64_t a, b;
    fz_rows(row_of, n_total, capacity, q, a, b);
    int64_t u0 = unk_of[q];                       // unknown u of this query's first -1 row
    int cnt = 0;
    bool unknown = false, corrected = false;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (; a < b; a += WAVE) {
        const bool have = a + lane < b;
        const int32_t t = have ? tok_term[a + lane] : 0;
        const uint64_t miss = __ballot(have && t < 0);
        // this token's candidates, in order: its id, or its corrections best first
        int32_t c[C];
#pragma unroll
        for (int s = 0; s < C; ++s) c[s] = -1;
        if (have && t >= 0) c[0] = t;
        bool none = false;
        if (have && t < 0) {
            const int64_t u = u0 + __popcll(miss & below);
            none = true;
            if (u < near_capacity) {
#pragma unroll
                for (int s = 0; s < C; ++s)
                    if (s < n_use) {
                        c[s] = near_term[u * n_best + s];
                        if (c[s] < 0) c[s] = -1; else none = false;
                    }
            }
        }
        unknown = unknown || __ballot(none) != 0;
        corrected = corrected || __ballot(have && t < 0 && !none) != 0;
        u0 += __popcll(miss);
        // fresh: not in the list, not earlier in this round (an earlier lane, or an earlier place of this lane)
        bool fresh[C];
#pragma unroll
        for (int s = 0; s < C; ++s) {
            fresh[s] = c[s] >= 0;
#pragma unroll
            for (int s2 = 0; s2 < s; ++s2)
                if (c[s2] == c[s]) fresh[s] = false;
        }
        for (int j = 0; j < WAVE; ++j) {
#pragma unroll
            for (int s2 = 0; s2 < C; ++s2) {
                const int32_t v = __shfl(c[s2], j, WAVE);
#pragma unroll
                for (int s = 0; s < C; ++s)
                    if (j < lane && v == c[s]) fresh[s] = false;
            }
        }
        for (int j = 0; j < cnt; ++j) {
            const int32_t v = list[j];
#pragma unroll
            for (int s = 0; s < C; ++s)
                if (v == c[s]) fresh[s] = false;
        }
        int mine = 0;
#pragma unroll
        for (int s = 0; s < C; ++s) mine += fresh[s];
        int incl = mine;
#pragma unroll
        for (int o = 1; o < WAVE; o <<= 1) {
            const int v = __shfl_up(incl, o, WAVE);
            if (lane >= o) incl += v;
        }
        int at = cnt + incl - mine;
#pragma unroll
        for (int s = 0; s < C; ++s)
            if (fresh[s]) {
                if (at < CAP) list[at] = c[s];
                ++at;
            }
        cnt += __shfl(incl, WAVE - 1, WAVE);
        cnt = cnt < CAP ? cnt : CAP;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < THR_BM25_MAX_TERMS) out_terms[q * THR_BM25_MAX_TERMS + lane] = lane < cnt ? list[lane] : -1;
    if (lane == 0) {
        n_distinct[q] = cnt;
        out_flags[q] = (text_flags[q] & THR_TEXT_EXCEPTIONAL) | (unknown ? THR_TEXT_UNKNOWN : 0) |
                       (cnt > THR_BM25_MAX_TERMS ? THR_TEXT_TOO_MANY : 0) | (corrected ? THR_TEXT_CORRECTED : 0);
    }
}

}  // namespace thr

using namespace thr;

struct FuzzyPlan {
    uint16_t* needle_cps;          // [capacity, FZ_ROW]: the needles in list order
    uint16_t* sorted_cps;          // the same rows in the order by length
    int32_t *needle_len, *needle_rank, *sorted_len, *sorted_of;   // [capacity]
    int32_t* length_start;         // [FZ_LENGTHS]
    unsigned long long* best_slots;   // [capacity, n_best]
};

static FuzzyPlan fuzzy_plan(Arena& A, int64_t capacity, int n_best) {
    FuzzyPlan plan;
    plan.needle_cps = A.take<uint16_t>((size_t)capacity * FZ_ROW);
    plan.sorted_cps = A.take<uint16_t>((size_t)capacity * FZ_ROW);
    plan.needle_len = A.take<int32_t>((size_t)capacity);
    plan.needle_rank = A.take<int32_t>((size_t)capacity);
    plan.sorted_len = A.take<int32_t>((size_t)capacity);
    plan.sorted_of = A.take<int32_t>((size_t)capacity);
    plan.length_start = A.take<int32_t>(FZ_LENGTHS);
    plan.best_slots = A.take<unsigned long long>((size_t)capacity * n_best);
    return plan;
}

static bool fuzzy_shape_ok(int64_t n_bytes, int64_t unknown_capacity, int64_t n_vocab, int64_t n_term_bytes) {
    return n_bytes >= 0 && n_bytes <= THR_TEXT_MAX_BYTES && unknown_capacity >= 1 && unknown_capacity <= THR_TEXT_MAX_BYTES &&
           n_vocab <= INT32_MAX && n_term_bytes <= ((int64_t)1 << 43);
}

extern "C" size_t thr_vocab_nearest_workspace_bytes(int64_t n_bytes, int64_t unknown_capacity, int64_t n_vocab,
                                                    int64_t n_term_bytes, int n_best) {
    if (!fuzzy_shape_ok(n_bytes, unknown_capacity, n_vocab, n_term_bytes)) return 0;
    if (n_vocab < 0 || n_term_bytes < 0 || n_best < 1 || n_best > THR_FUZZY_MAX_BEST) return 0;
    Arena A;
    fuzzy_plan(A, unknown_capacity, n_best);
    return A.total;
}

extern "C" int thr_vocab_nearest(const uint8_t* text_bytes, int64_t n_bytes, const uint32_t* table,
                                 const int64_t* unknown_off, const int32_t* unknown_len, const int32_t* n_unknown,
                                 int64_t unknown_capacity, const uint8_t* term_bytes, const int64_t* term_ptr,
                                 int64_t n_vocab, int64_t n_term_bytes, const int64_t* term_rowptr, int max_edits,
                                 int n_best, int32_t* near_term, int32_t* near_dist, void* workspace,
                                 size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!fuzzy_shape_ok(n_bytes, unknown_capacity, n_vocab, n_term_bytes), THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!text_bytes || !table || !unknown_off || !unknown_len || !n_unknown || !term_bytes || !term_ptr ||
                      !near_term || !near_dist || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(n_vocab < 0 || n_term_bytes < 0, THR_ERR_INVALID);
    THR_RETURN_IF(max_edits < 1 || max_edits > FZ_MAX_EDITS || n_best < 1 || n_best > THR_FUZZY_MAX_BEST, THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)unknown_off & 7) != 0 || ((uintptr_t)term_ptr & 7) != 0 || ((uintptr_t)term_rowptr & 7) != 0,
                  THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)table & 3) != 0 || ((uintptr_t)unknown_len & 3) != 0 || ((uintptr_t)n_unknown & 3) != 0 ||
                      ((uintptr_t)near_term & 3) != 0 || ((uintptr_t)near_dist & 3) != 0 || ((uintptr_t)workspace & 15) != 0,
                  THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_vocab_nearest_workspace_bytes(n_bytes, unknown_capacity, n_vocab, n_term_bytes, n_best),
                  THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    const FuzzyPlan P = fuzzy_plan(A, unknown_capacity, n_best);
    const dim3 per_needle((unsigned)((unknown_capacity + FZ_THREADS - 1) / FZ_THREADS));
    hipLaunchKernelGGL(fz_needles, per_needle, dim3(FZ_THREADS), 0, st, text_bytes, n_bytes, table, unknown_off, unknown_len,
                       n_unknown, unknown_capacity, max_edits, n_best, P.needle_cps, P.needle_len, P.best_slots);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(fz_rank, dim3(1), dim3(FZ_SCAN_THREADS), 0, st, (const int32_t*)P.needle_len, n_unknown, unknown_capacity,
                       P.needle_rank, P.length_start);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(fz_scatter, per_needle, dim3(FZ_THREADS), 0, st, (const uint16_t*)P.needle_cps, (const int32_t*)P.needle_len,
                       (const int32_t*)P.needle_rank, n_unknown, unknown_capacity, P.sorted_cps, P.sorted_len, P.sorted_of);
    rc = launch_status();
    if (rc) return rc;
    if (n_vocab > 0) {
        const int shift = (int)((uintptr_t)term_bytes & 15);
        const KeyStore K = {term_bytes, term_ptr, term_rowptr, n_vocab, n_term_bytes, shift};
        const int64_t n_slices = (n_term_bytes + shift + FZ_SLICE - 1) / FZ_SLICE;
        const dim3 slices((unsigned)(n_slices > 0 ? n_slices : 1));
        if (max_edits == 1)
            hipLaunchKernelGGL(fz_scan_keys<1>, slices, dim3(FZ_THREADS), 0, st, K, (const uint16_t*)P.sorted_cps,
                               (const int32_t*)P.sorted_len, (const int32_t*)P.sorted_of, (const int32_t*)P.length_start, n_best, P.best_slots);
        else
            hipLaunchKernelGGL(fz_scan_keys<2>, slices, dim3(FZ_THREADS), 0, st, K, (const uint16_t*)P.sorted_cps,
                               (const int32_t*)P.sorted_len, (const int32_t*)P.sorted_of, (const int32_t*)P.length_start, n_best, P.best_slots);
        rc = launch_status();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(fz_write, per_needle, dim3(FZ_THREADS), 0, st, (const unsigned long long*)P.best_slots, n_unknown,
                       unknown_capacity, n_best, near_term, near_dist);
    return launch_status();
}

extern "C" size_t thr_query_terms_fuzzy_workspace_bytes(int n_queries) {
    if (n_queries < 1 || n_queries > THR_TEXT_MAX_TEXTS) return 0;
    Arena A;
    A.take<int32_t>((size_t)n_queries + 1);
    A.take<int32_t>((size_t)n_queries + 1);
    return A.total;
}

extern "C" int thr_query_terms_fuzzy(const int32_t* tok_term, const int32_t* n_tokens, const int32_t* text_flags,
                                     const int32_t* n_total, int64_t token_capacity, int n_queries,
                                     const int32_t* near_term, int64_t near_capacity, int n_best, int n_use,
                                     int32_t* out_terms, int32_t* n_distinct, int32_t* out_flags, void* workspace,
                                     size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(n_queries < 1 || n_queries > THR_TEXT_MAX_TEXTS, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(token_capacity < 1 || token_capacity > THR_TEXT_MAX_BYTES, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!tok_term || !n_tokens || !text_flags || !n_total || !near_term || !out_terms || !n_distinct ||
                      !out_flags || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(near_capacity < 1 || n_best < 1 || n_best > THR_FUZZY_MAX_BEST || n_use < 1 || n_use > n_best,
                  THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)workspace & 3) != 0, THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_query_terms_fuzzy_workspace_bytes(n_queries), THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    int32_t* row_of = A.take<int32_t>((size_t)n_queries + 1);     // the first token row of each query
    int32_t* unknown_of = A.take<int32_t>((size_t)n_queries + 1);  // its first unknown token
    const dim3 per_query((unsigned)((n_queries + FZ_WAVES - 1) / FZ_WAVES));
    hipLaunchKernelGGL(fz_scan, dim3(1), dim3(FZ_SCAN_THREADS), 0, st, n_tokens, (int64_t)n_queries, row_of);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(fz_unknowns, per_query, dim3(FZ_THREADS), 0, st, tok_term, (const int32_t*)row_of, n_total,
                       token_capacity, n_queries, unknown_of);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(fz_scan, dim3(1), dim3(FZ_SCAN_THREADS), 0, st, (const int32_t*)unknown_of, (int64_t)n_queries,
                       unknown_of);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(fz_query_terms, per_query, dim3(FZ_THREADS), 0, st, tok_term, (const int32_t*)row_of,
                       (const int32_t*)unknown_of, n_total, token_capacity, text_flags, n_queries, near_term, near_capacity,
                       n_best, n_use, out_terms, n_distinct, out_flags);
    return launch_status();
}
