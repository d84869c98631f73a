// Shortlist scan with the QUERIES in registers and the ROWS shared through LDS
// (thr_dense_topk_f16 over the fragment-major float16 copy; the default f16 scan since round 2).
// Two kernels share the pieces below (QAcc / qs_steps / QEmit / QTop / QS_WAVE_*: the MFMA shape, the
// k-loop, the per-lane segment emit, the sample keep, the wave's set-up and write-out):
// dense_scan_f16q, described first -- 4-wave blocks, the kernel of dim 1024 -- and
// dense_scan_f16qs further down, the staggered 8-wave block that is the default at dim <= 768.
//
// Why (profiles/README.md, round 2): the round-1 kernel (dense_scan_f16p) kept 96 queries in
// LDS and let every wave stream its own rows from L2 -- 8 KiB of row fragments per 24 MFMAs and
// wave, 42.7 B/clk/CU at the full matrix rate against an L1 path of 64 B/clk.  Its waves sat in
// s_waitcnt 44 % of the time and the matrix pipe was 52 % busy.  Here the operand roles are
// swapped, which takes the row loads off the waves' critical path altogether:
//
//   * a wave owns 32 queries for the whole launch and keeps their float16 image as the B operands
//     of all DIM/16 k-steps in registers (192 VGPRs at dim 768) -- loaded once, coalesced, from
//     the fragment-major query image pack_queries_f16 writes;
//   * rows reach LDS by LDS-DMA (global_load_lds_dwordx4: no VGPRs, no LDS store instructions) in
//     HALF tiles (32 rows x DIM/2: 24 KiB at dim 768): the copy is fragment-major, so each 1 KiB
//     piece IS the A operand of one k-step and lands lane-linear; one conflict-free ds_read_b128
//     per MFMA and wave;
//   * a block is 4 waves (one per SIMD, 128 queries) and TWO blocks share a CU (2 x 76 KiB of
//     LDS at dim 768).  The first version of this kernel ran ONE 8-wave block per CU and its phase
//     stamps (profiles/r2_scan_stamps_v1.json) showed why that is wrong: the older wave of a SIMD
//     takes the matrix pipe for its whole k-loop, the younger runs after it, and the block-wide
//     barrier then holds everybody until the last wave has emitted -- the pipe idled 40 % of
//     every tile.  Two independent blocks have independent barriers, so one block's DMA issue,
//     emit and barrier wait run under the other block's MFMAs;
//   * ring of NB half-tile buffers, ONE workgroup barrier per half tile: wait for the own pieces
//     of half-tile j (counted vmcnt: the next half-tile's pieces stay in flight), barrier
//     (everybody's pieces of j have landed, everybody is done reading j-1), then the pieces of
//     j+NB-1 are issued into j-1's buffer BETWEEN the MFMAs of j.
//
// The copy holds the rows NORMALISED (d/||d|| rounded to float16, thr_dense_quantize_f16) with
// NaN for rows without an embedding and for the padding rows of the last tile: an accumulator
// is then the scan score itself (no 1/||d|| gather) and `acc >= tau` is false for every row that
// must not be emitted -- the fast path of the epilogue is one compare + branch per accumulator
// register.  A lane that passes writes (score, row) straight to global memory at its OWN cursor:
// lane (query c, row group g) of the block working on row slice `slice` owns segment
// SEGS * slice + g of query c's candidate area (SEGS = 2 row halves with the 32x32x16 MFMA shape,
// 4 row groups with 16x16x32), so there is no staging, no atomic and no flush -- the 1400 cycles
// per tile the LDS-staged, atomically flushed emit of the first version took (the returning
// atomics also drained the DMA queue).  select_band reads the segments in place
// (cand_cnt[q * nseg + s] entries each).
#pragma once
#include "dense_common.hpp"
#include "dense_tile_schedule.hpp"

namespace thr {

constexpr int Q_RING = 4;  // A fragments in flight per wave
constexpr int Q_NW = 4;    // waves per block, 32 queries each

template <int DIM>
struct QScan {
    static constexpr int KS = DIM / 16;             // k-steps = 1 KiB pieces per row tile
    static constexpr int HS = KS / 2;               // ... per half tile
    static constexpr int HALF_BYTES = HS * 1024;
    static constexpr int PER_CU = DIM <= 768 ? 2 : 1;   // blocks per CU (256 B-operand VGPRs at 1024)
    static constexpr int NB = (160 * 1024 / PER_CU) / HALF_BYTES > 4 ? 4 : (160 * 1024 / PER_CU) / HALF_BYTES;
    static constexpr int PER = HS / Q_NW;           // pieces a wave issues per half tile
#ifndef THR_Q_RING_1024
#define THR_Q_RING_1024 8
#endif
    // A fragments in flight per wave: a block that is alone on its CU (dim 1024) has one wave per
    // SIMD, nobody else's MFMAs cover an LDS read that returns late
    static constexpr int RING = PER_CU == 1 ? THR_Q_RING_1024 : Q_RING;
#ifdef Q_PROBE_EXTRA
    static constexpr int VM_PER_PIECE = 2, LDS_BYTES = NB * HALF_BYTES + 32 * 1024;   // (diagnostic: dma())
#else
    static constexpr int VM_PER_PIECE = 1, LDS_BYTES = NB * HALF_BYTES;
#endif
    static_assert(HS % Q_NW == 0 && NB >= 3, "half tile must split evenly over the waves; >= 3 buffers");
};

// The k-loop of one half tile, fully unrolled: wait for the A fragment of step S (the Q_RING - 1
// younger reads stay in flight), multiply, refill the ring slot with step S + Q_RING, and after
// every fourth MFMA issue one DMA piece of the half tile NB-1 ahead.  The LDS reads are inline
// asm (hipcc would wait vmcnt(0) before an LDS read that may alias an LDS-DMA in flight); the
// "+v" on the waited fragment orders the MFMA behind the wait.  (Plain functions, not lambdas:
// asm operands do not capture.)
#define QS_RD(dst, ks) \
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(abase), "n"((ks) * 1024) : "memory")
template <int S, int HS, int RING>
__device__ __forceinline__ void qs_fill(f32x4 (&a)[RING], uint32_t abase) {
    if constexpr (S < RING && S < HS) {
        QS_RD(a[S], S);
        qs_fill<S + 1, HS>(a, abase);
    }
}
// SHAPE = 32: v_mfma_f32_32x32x16_f16, one MFMA per 1 KiB piece (piece = 32 rows x 16 dims).
// SHAPE = 16: v_mfma_f32_16x16x32_f16, two MFMAs per piece (piece = 16 rows x 32 dims, against the
//             wave's two 16-query halves).  Same bytes, same cadence (a piece per 32 matrix-pipe
//             cycles); the micro-architecture guide measures the 16x16x32 shape at ~1.15x the
//             FLOP/s of 32x32x16 once the chip is power-limited, which this kernel is.  The
//             fragment-major images differ (quantize_f16_norm / pack_queries_f16 take the shape).
// The accumulators are 16 registers either way; QAcc maps register x to (row, query half).
template <int SHAPE>
struct QAcc;
// SHAPE = 48 (round 4, dim 1024): the 16x16x32 MFMA against THREE 16-query blocks -- 48 queries
//             per wave, 192 per CU: three MFMAs per LDS fragment, and every row tile that is
//             brought into LDS serves half again as many queries (the query image is a sequence of
//             16-query blocks either way: block B's fragments sit at [B * KS/2 + k32]).
// QW = queries per wave, NQB = 16-query blocks, NREG = accumulator registers.
template <>
struct QAcc<32> {
    static constexpr int NQL = 1, SEGS = 2;   // queries per lane; candidate segments per row slice
    static constexpr int QW = 32, NQB = 2, NREG = 16;
    f32x16 v;
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int x = 0; x < 16; ++x) v[x] = 0.f;
    }
    template <int X> __device__ __forceinline__ float get() const { return v[X]; }
    // lane (c = lane & 31, h = lane >> 5): register x is row (x&3) + 8 (x>>2) + 4 h of query c
    template <int X> static __device__ __forceinline__ int row(int lane) { return (X & 3) + 8 * (X >> 2) + 4 * (lane >> 5); }
    template <int X> static constexpr int qsel() { return 0; }
    static __device__ __forceinline__ int query(int lane, int) { return lane & 31; }
    static __device__ __forceinline__ int seg(int lane) { return lane >> 5; }
};
template <>
struct QAcc<48> {
    static constexpr int NQL = 3, SEGS = 4;
    static constexpr int QW = 48, NQB = 3, NREG = 24;
    f32x4 t[6];   // tile [row half ra][query block qb] at 3 ra + qb
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int x = 0; x < 6; ++x) t[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    template <int X> __device__ __forceinline__ float get() const { return t[X >> 2][X & 3]; }
    // lane (c = lane & 15, g = lane >> 4): register x = 4 (3 ra + qb) + j is row 16 ra + 4 g + j
    // of query 16 qb + c
    template <int X> static __device__ __forceinline__ int row(int lane) { return 16 * ((X >> 2) / 3) + 4 * (lane >> 4) + (X & 3); }
    template <int X> static constexpr int qsel() { return (X >> 2) % 3; }
    static __device__ __forceinline__ int query(int lane, int qb) { return 16 * qb + (lane & 15); }
    static __device__ __forceinline__ int seg(int lane) { return lane >> 4; }
};
template <>
struct QAcc<16> {
    static constexpr int NQL = 2, SEGS = 4;
    static constexpr int QW = 32, NQB = 2, NREG = 16;
    f32x4 t[4];   // tile [row half ra][query half qb] at 2 ra + qb
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int x = 0; x < 4; ++x) t[x] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    template <int X> __device__ __forceinline__ float get() const { return t[X >> 2][X & 3]; }
    // lane (c = lane & 15, g = lane >> 4): register x = 4 (2 ra + qb) + j is row 16 ra + 4 g + j
    // of query 16 qb + c
    template <int X> static __device__ __forceinline__ int row(int lane) { return 16 * (X >> 3) + 4 * (lane >> 4) + (X & 3); }
    template <int X> static constexpr int qsel() { return (X >> 2) & 1; }
    static __device__ __forceinline__ int query(int lane, int qb) { return 16 * qb + (lane & 15); }
    static __device__ __forceinline__ int seg(int lane) { return lane >> 4; }
};

// piece S of a half tile (HS pieces): SHAPE 32 -> k-step K0 + S; SHAPE 16 -> row half S & 1 of
// k32-step (K0 + S) / 2, B operands bq[qb * KS/2 + k32]
// the MFMAs of piece S: SHAPE 32 one, else one per 16-query block of the wave
template <int S, int K0, int KS, int SHAPE, int NBQ>
__device__ __forceinline__ void qsx_mfma(const f32x4& a, const f32x4 (&bq)[NBQ], QAcc<SHAPE>& acc) {
    if constexpr (SHAPE == 32) {
        acc.v = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a),
                                                       __builtin_bit_cast(half8, bq[K0 + S]), acc.v, 0, 0, 0);
    } else {
        constexpr int k32 = (K0 + S) / 2, ra = S & 1, NQB = QAcc<SHAPE>::NQB;
        static_assert(NBQ == NQB * KS / 2, "one B fragment per 16-query block and 32-dim step");
        static_for<0, NQB>([&](auto qb) {
            acc.t[NQB * ra + qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                __builtin_bit_cast(half8, a), __builtin_bit_cast(half8, bq[qb * (KS / 2) + k32]),
                acc.t[NQB * ra + qb], 0, 0, 0);
        });
    }
}
// THE k-loop: steps S .. N - 1 of a buffer of N pieces (a half tile: N = HS, its first k-step K0; a
// whole tile: N = KS, K0 = 0).  What a kernel threads between the MFMAs is Hook::after<S>(args...),
// called once the ring slot of step S is refilled.  (A stateless policy and plain arguments, not a
// closure: one that holds the emit state by reference keeps it in memory a pass longer, and hipcc
// then numbers the B-operand registers differently.)
template <int S, int N, int K0, int KS, typename Hook, int SHAPE, int RING, int NBQ, typename... Args>
__device__ __forceinline__ void qs_steps(f32x4 (&a)[RING], const f32x4 (&bq)[NBQ], QAcc<SHAPE>& acc,
                                         uint32_t abase, Args&... args) {
    if constexpr (S < N) {
        constexpr int left = N - S - 1 < RING - 1 ? N - S - 1 : RING - 1;
        asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a[S % RING]) : "n"(left) : "memory");
        qsx_mfma<S, K0, KS, SHAPE>(a[S % RING], bq, acc);
        if constexpr (S + RING < N) QS_RD(a[S % RING], S + RING);
        Hook::template after<S>(args...);
        qs_steps<S + 1, N, K0, KS, Hook>(a, bq, acc, abase, args...);
    }
}
// The k-loop of dense_scan_f16qs.  A wave that has its SIMD's matrix pipe to itself (the other group
// is in its emit or at the barrier: most of an interval) paced 41 cycles per step through qs_steps
// against the 32 its MFMAs take -- with four and with six reads in flight (the stamp tables of
// profiles/dense_scan_ring.md): what does not
// overlap is the wave's own issue of refill, wait and the next MFMA, all of them between the LAST MFMA of
// one step and the first of the next.  Here they sit between the two MFMAs of ONE step (SHAPE 16), under
// the first one's 16 pipe cycles, and the next step's first MFMA follows the second back to back:
//     mfma(S, query block 0) | refill the slot of step S - 1 | wait for step S + 1 | mfma(S, block 1)
// The slot refilled is the one read a step ago, so RING slots keep RING - 1 reads in flight.  Same
// MFMAs in the same order per accumulator as qs_steps: same bits.
template <int S, int N, int KS, typename Hook, int SHAPE, int RING, int NBQ, typename... Args>
__device__ __forceinline__ void qs_steps_il(f32x4 (&a)[RING], const f32x4 (&bq)[NBQ], QAcc<SHAPE>& acc,
                                            uint32_t abase, Args&... args) {
    if constexpr (S < N) {
        constexpr int NQB = QAcc<SHAPE>::NQB, k32 = S / 2, ra = S & 1;
        if constexpr (S == 0) {
            constexpr int left0 = N - 1 < RING - 1 ? N - 1 : RING - 1;
            asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a[0]) : "n"(left0) : "memory");
        }
        if constexpr (SHAPE == 32) {
            acc.v = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(half8, a[S % RING]),
                                                           __builtin_bit_cast(half8, bq[S]), acc.v, 0, 0, 0);
        } else {
            acc.t[NQB * ra] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                __builtin_bit_cast(half8, a[S % RING]), __builtin_bit_cast(half8, bq[k32]), acc.t[NQB * ra], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (S >= 1 && S - 1 + RING < N) QS_RD(a[(S - 1) % RING], S - 1 + RING);
        if constexpr (S + 1 < N) {
            // reads issued after the one of step S + 1: up to step min(S - 1 + RING, N - 1)
            constexpr int left = N - 2 - S < RING - 2 ? N - 2 - S : RING - 2;
            asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a[(S + 1) % RING]) : "n"(left) : "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (SHAPE != 32) {
            static_for<1, NQB>([&](auto qb) {
                acc.t[NQB * ra + qb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                    __builtin_bit_cast(half8, a[S % RING]), __builtin_bit_cast(half8, bq[qb * (KS / 2) + k32]),
                    acc.t[NQB * ra + qb], 0, 0, 0);
            });
        }
        Hook::template after<S>(args...);
        __builtin_amdgcn_sched_barrier(0);
        qs_steps_il<S + 1, N, KS, Hook>(a, bq, acc, abase, args...);
    }
}
#undef QS_RD
// after step S of a WHOLE row tile (dense_scan_f16qs): the PB row pieces an issuing wave sends go
// into its first steps (tsched::issue_step; PB = 0: none)
template <int PB>
struct QTileHook {
    template <int S, typename Issue>
    static __device__ __forceinline__ void after(Issue& issue_piece) {
        constexpr int p = (S - 1) / 2;
        if constexpr (S >= 1 && p < PB && tsched::issue_step(p) == S) issue_piece(std::integral_constant<int, p>{});
    }
};

// the emit of one accumulator register (a struct member, not a lambda: its store is inline asm).
// A lane's candidate segment is addressed as a 32-bit byte offset from `cand` (one SGPR pair for
// the base instead of a 64-bit pointer per lane): slot = next free entry, end = one past the last.
//
// COLL: whether the batch carries a collection filter.  The COLL = false instantiation (what
// launch_scan_f16q picks when the index or the batch has no collections) has no qc[], no doc_coll
// pointer, no gather and no exec region for it: an unfiltered batch used to carry all that and
// branch around it on every hit (53 us of the 2.74 ms headline step, profiles/dense_emit.md).
template <int NQL, bool COLL>
struct QColl {   // the collection filter of a lane's queries (-1: none)
    const int32_t* doc_coll;
    int qc[NQL];
};
template <int NQL>
struct QColl<NQL, false> {};

template <int SHAPE, bool COLL>
struct QEmit : QColl<QAcc<SHAPE>::NQL, COLL> {
    static constexpr int NQL = QAcc<SHAPE>::NQL;
    const Cand* cand;
    float tau[NQL];
    uint32_t slot[NQL], end[NQL];
    template <int X>
    __device__ __forceinline__ void one(const QAcc<SHAPE>& acc, uint32_t row0, int lane) {
        constexpr int qs = QAcc<SHAPE>::template qsel<X>();
        const float v = acc.template get<X>();
        if (v >= tau[qs]) {   // false for NaN
            const uint32_t row = row0 + (uint32_t)QAcc<SHAPE>::template row<X>(lane);
            if constexpr (COLL) {
                // (a filtered query pays a dependent gather here, and its wait drains the DMA queue)
                if (this->qc[qs] != -1 && this->doc_coll[row] != this->qc[qs]) return;
            }
            if (slot[qs] < end[qs]) {
                const uint64_t word = (uint64_t)__float_as_uint(v) | ((uint64_t)row << 32);
                // (inline asm: a store hipcc can see would make it wait vmcnt(0) -- DMA included --
                // at the loop's back edge)
                asm volatile("global_store_dwordx2 %0, %1, %2" ::"v"(slot[qs]), "v"(word), "s"(cand) : "memory");
            }
            slot[qs] += 8;
        }
    }
};
// every accumulator register of a row tile through `one` of a QEmit or a QTop, in register order
template <int SHAPE, typename Keep>
__device__ __forceinline__ void q_all(Keep& keep, const QAcc<SHAPE>& acc, uint32_t row0, int lane) {
    static_for<0, QAcc<SHAPE>::NREG>([&](auto x) { keep.template one<decltype(x)::value>(acc, row0, lane); });
}

// MODE_ALL (the sample pass): what a lane keeps of the sample rows it scores -- for each of its NQL
// queries the SAMPLE_TOP largest finite scores, in registers, sorted descending (a max / min pair per
// kept value and accumulator register; NaN -- no such row, no embedding -- counts as -inf).  No score
// goes to memory before the end of the launch, where the lane writes its SAMPLE_TOP values per query
// to sample[q][segment][0..SAMPLE_TOP), segment = the (row slice, lane group) index of the filter
// scan's candidate segments.  kth_select_top takes the ks-th largest of a query's values.
// With a collection filter (qc != -1) only the sample rows of the query's collection count: the
// row's collection is gathered for every finite score (the padding rows of the last tile are NaN,
// so the gather never leaves doc_coll).  That is a dependent load per finite score of a filtered
// query, and its wait drains the DMA queue as the filter scan's gather does: paid by filtered batches
// in the sample pass only (~1 % of the rows), and NOT measured -- no filtered batch was profiled.
// COLL = false (no collections in the index or the batch) compiles the gather and its test out.
template <int SHAPE, bool COLL>
struct QTop : QColl<QAcc<SHAPE>::NQL, COLL> {
    static constexpr int NQL = QAcc<SHAPE>::NQL;
    float t[NQL][SAMPLE_TOP];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int u = 0; u < NQL; ++u)
#pragma unroll
            for (int j = 0; j < SAMPLE_TOP; ++j) t[u][j] = -INFINITY;
    }
    template <int X>
    __device__ __forceinline__ void one(const QAcc<SHAPE>& acc, uint32_t row0, int lane) {
        constexpr int qs = QAcc<SHAPE>::template qsel<X>();
        float x = acc.template get<X>();
        x = x == x ? x : -INFINITY;
        if constexpr (COLL) {
            if (this->doc_coll && this->qc[qs] != -1 && x > -INFINITY) {
                const uint32_t row = row0 + (uint32_t)QAcc<SHAPE>::template row<X>(lane);
                if (this->doc_coll[row] != this->qc[qs]) x = -INFINITY;
            }
        }
#pragma unroll
        for (int j = 0; j < SAMPLE_TOP; ++j) {   // t[qs] stays sorted; x carries the displaced value down
            const float hi = fmaxf(t[qs][j], x);
            x = fminf(t[qs][j], x);
            t[qs][j] = hi;
        }
    }
    // the lane's values of query q (u-th of the lane), segment seg of nseg
    __device__ __forceinline__ void store(float* __restrict__ sample, int u, int64_t q, int nseg, int seg) const {
        float* dst = sample + (q * nseg + seg) * SAMPLE_TOP;
#pragma unroll
        for (int j = 0; j < SAMPLE_TOP; ++j) dst[j] = t[u][j];
    }
};

// after step S of half HF of a row tile, HS pieces (dense_scan_f16q): one of the wave's PER pieces
// after every (HS / PER)-th MFMA.
// With an emit state, also the emit of the PREVIOUS row tile's accumulators (MODE_FILTER at dim 1024):
// a block of that kernel has ONE wave per SIMD, so while a wave runs its epilogue nothing feeds the
// SIMD's matrix pipe -- the stamps put that at a quarter of a half tile.  Here the 16 accumulator
// registers of tile i - 1 are compared / stored one at a time between the MFMAs of tile i (8 per
// half tile, evenly spaced): an MFMA occupies the pipe for 16 cycles after it issues, which is what
// one register's compare-and-branch takes to issue.
template <int HS, int PER, int HF>
struct QHalfHook {
    template <int S, typename Issue>
    static __device__ __forceinline__ void after(Issue& issue_piece) {
        constexpr int every = HS / PER;
        if constexpr (S % every == 1 && S / every < PER) issue_piece(std::integral_constant<int, S / every>{});
    }
    template <int S, typename Issue, int SHAPE, bool COLL>
    static __device__ __forceinline__ void after(Issue& issue_piece, QEmit<SHAPE, COLL>& em,
                                                 const QAcc<SHAPE>& prv, uint32_t row_prv, int lane) {
        after<S>(issue_piece);
        // half the registers of the previous tile per half tile, evenly spaced: register j after the
        // step at which j = floor(S * NRH / HS) is about to change
        constexpr int NRH = QAcc<SHAPE>::NREG / 2, j = S * NRH / HS;
        if constexpr ((S + 1) * NRH / HS > j) em.template one<NRH * HF + j>(prv, row_prv, lane);
    }
};

// What a wave holds for the whole launch besides its accumulators, and what it leaves behind, for
// both kernels.  (Macros over the kernel's own names -- A, MODE, SHAPE, COLL, slot, lane, q32 = the
// wave's tile of A::QW queries, and the kernel's arguments -- not functions: as functions over em /
// top / start, or as one struct that holds them, hipcc numbers the kernels' registers differently,
// DESIGN.md 4.1.)
// QS_WAVE_SETUP: the B operands of the wave's queries, all k-steps, in registers for the whole launch
// (bq: NBQ fragments of 1 KiB, image [tile of QW queries][NBQ][64 lanes]; a wave whose queries are all
// padding only moves row pieces: no operands); the lane's private candidate segments (MODE_FILTER:
// query q, segment my_seg = SEGS * slice + seg(lane) of nseg; start[u] = byte offset of the segment of
// the lane's u-th query) and its sample keep (MODE_ALL).
#define QS_WAVE_SETUP(NBQ_)                                                                             \
    f32x4 bq[NBQ_];                                                                                     \
    if ((int64_t)q32 * A::QW < n_queries)                                                               \
        static_for<0, NBQ_>([&](auto s) {                                                               \
            bq[s] = qfrag[((int64_t)q32 * NBQ_ + s) * 64 + lane];                                       \
        });                                                                                             \
    const int nseg = A::SEGS * slot.nslices;                                                            \
    const int my_seg = A::SEGS * slot.slice + A::seg(lane);                                             \
    QEmit<SHAPE, COLL> em;                                                                              \
    em.cand = cand;                                                                                     \
    QTop<SHAPE, COLL> top; /* MODE_ALL */                                                               \
    if constexpr (COLL) em.doc_coll = top.doc_coll = doc_coll;                                          \
    top.init();                                                                                         \
    uint32_t start[A::NQL];                                                                             \
    _Pragma("unroll")                                                                                   \
    for (int u = 0; u < A::NQL; ++u) {                                                                  \
        const int q = q32 * A::QW + A::query(lane, u);                                                  \
        em.tau[u] = MODE == MODE_FILTER ? tau[q] : 0.f;                                                 \
        /* collection filter of this lane's query (-1: none): checked only for rows that pass tau      \
           (MODE_ALL: for the sample rows with a finite score) */                                       \
        if constexpr (COLL) em.qc[u] = top.qc[u] = (query_coll && q < n_queries) ? query_coll[q] : -1;  \
        start[u] = (uint32_t)(((int64_t)q * CAND_CAP + (int64_t)my_seg * seg_cap) * sizeof(Cand));      \
        em.slot[u] = start[u];                                                                          \
        em.end[u] = start[u] + (uint32_t)(seg_cap * sizeof(Cand));                                      \
    }                                                                                                   \
    /* Retire these loads HERE, visibly to hipcc: left pending, their first use (the first MFMA of     \
       the tile loop) gets an s_waitcnt vmcnt(0) on every trip, which would drain the DMA of the       \
       next (half) tiles each time. */                                                                  \
    __builtin_amdgcn_s_waitcnt(0x0F70);
// QS_WAVE_TILE: a row tile's accumulators into the candidate segments, or into the sample keep
#define QS_WAVE_TILE(acc_, row0_)                                \
    if constexpr (MODE == MODE_ALL) {                            \
        q_all(top, acc_, row0_, lane);                           \
    } else {                                                     \
        q_all(em, acc_, row0_, lane);                            \
    }
// QS_WAVE_WRITE_OUT, the end of the launch: the fill of the lane's segments, or its kept sample scores
// (the waves of padding queries too: -inf)
#define QS_WAVE_WRITE_OUT()                                                                             \
    if constexpr (MODE == MODE_FILTER) {                                                                \
        _Pragma("unroll")                                                                               \
        for (int u = 0; u < A::NQL; ++u)                                                                \
            seg_cnt[(int64_t)(q32 * A::QW + A::query(lane, u)) * nseg + my_seg] =                       \
                (int)((em.slot[u] - start[u]) / sizeof(Cand));                                          \
    } else {                                                                                            \
        _Pragma("unroll")                                                                               \
        for (int u = 0; u < A::NQL; ++u)                                                                \
            top.store(sample, u, (int64_t)q32 * A::QW + A::query(lane, u), nseg, my_seg);               \
    }

// PROF: diagnostic build (thr_dense_scan_stamps_f16): s_memtime stamps around the phases of the
// half-tile loop, summed per wave into stamps[(block * 4 + wave) * 8 + {0: wait for the own DMA
// pieces, 1: barrier, 2: ring fill, 3: k-loop (with the DMA issue), 4: emit, 5: half tiles,
// 6: whole loop, 7: HW_ID}].  Each stamp drains the wave's LDS/SMEM queue, so the build is slower
// than the real one; it only says where the time goes.
// COLL: the batch carries a collection filter (QEmit / QTop).
template <int DIM, int MODE, bool PROF = false, int SHAPE = 32, bool COLL = true>
__global__ __launch_bounds__(Q_NW * 64, QScan<DIM>::PER_CU) void dense_scan_f16q(
    const f32x4* __restrict__ packed, const f32x4* __restrict__ qfrag, int n_qtiles,
    int64_t n_tiles, int64_t tile_stride, const float* __restrict__ tau,
    int* __restrict__ seg_cnt, Cand* __restrict__ cand, int seg_cap,
    float* __restrict__ sample,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll, int n_queries,
    unsigned long long* __restrict__ stamps = nullptr) {
    using C = QScan<DIM>;
    using A = QAcc<SHAPE>;
    constexpr int KS = C::KS, HS = C::HS, NB = C::NB, PER = C::PER, QW = A::QW;
    constexpr int NBQ = SHAPE == 32 ? KS : A::NQB * KS / 2;   // B fragments of the wave's queries
    extern __shared__ f32x4 lds_rows[];  // NB half-tile buffers

    const ScanSlot slot = scan_slot(n_qtiles);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q32 = slot.qtile * Q_NW + wave;  // this wave's tile of QW (32, or 48) queries
    const bool idle = (int64_t)q32 * QW >= n_queries;   // all padding: only moves row pieces

    QS_WAVE_SETUP(NBQ)

    // this block's row tiles: slice, slice + nslices, ...; half tile j = (tile j/2, dims half j&1)
    const int64_t first = slot.slice, step = slot.nslices;
    const int64_t n_mine = first < n_tiles ? (n_tiles - first + step - 1) / step : 0;
    const int64_t n_half = 2 * n_mine;
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)lds_rows;
    // piece p (wave + 4 p) of the block's j-th half tile -> buffer buf; past the end the last
    // half tile is requested again (never read): the count of pieces in flight stays what the
    // vmcnt waits assume
    auto piece_src = [&](int64_t j) -> const f32x4* {
        const int64_t jc = j < n_half ? j : n_half - 1;
        const int64_t t = first + (jc >> 1) * step;
        return packed + ((t * tile_stride * KS + (jc & 1) * HS + wave) * 64 + lane);
    };
#ifdef Q_PROBE_EXTRA
    f32x4 probe_reg = {0.f, 0.f, 0.f, 0.f};   // (diagnostic builds only: see below)
#endif
    auto dma = [&](const f32x4* src, int buf, int p) {
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(src + p * Q_NW * 64),
            (__attribute__((address_space(3))) void*)(size_t)(lds_base + buf * C::HALF_BYTES +
                                                              (wave + p * Q_NW) * 1024),
            16, 0, 0);
#ifdef Q_PROBE_EXTRA
        // Diagnostic builds (_build.build_variant(name, ["Q_PROBE_EXTRA=1|2"]), dim 1024): is the
        // wave's instruction issue what bounds the k-loop?  Every row piece is issued a SECOND time
        // into 32 KiB of LDS nobody reads -- 1: as another LDS-DMA piece, 2: as a plain load into a
        // register plus a ds_write_b128 of that register (stale data: only the issue slots
        // matter).  Results are unchanged.  Measured (THR_DENSE_QW=32 scripts/probe_dim1024.py
        // 1000000 2048, one box): 4.201 ms plain, 4.180 with the pieces doubled, 4.160 with the load
        // + write added -- the extra instructions are free: not issue-bound.
        const uint32_t scratch = lds_base + NB * C::HALF_BYTES + (wave + (p & 7) * Q_NW) * 1024;
        if constexpr (Q_PROBE_EXTRA == 1) {
            __builtin_amdgcn_global_load_lds(
                (const __attribute__((address_space(1))) void*)(src + p * Q_NW * 64),
                (__attribute__((address_space(3))) void*)(size_t)scratch, 16, 0, 0);
        } else {
            asm volatile("ds_write_b128 %0, %1" ::"v"(scratch + lane * 16), "v"(probe_reg) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(probe_reg) : "v"(src + p * Q_NW * 64) : "memory");
        }
#endif
    };
    if (n_half > 0) {
#pragma unroll
        for (int b = 0; b < NB - 1; ++b) {
            const f32x4* src = piece_src(b);
#pragma unroll
            for (int p = 0; p < PER; ++p) dma(src, b, p);
        }
    }

    unsigned long long ph[5] = {0, 0, 0, 0, 0}, t_loop = 0, t_prev = 0;
    auto stamp = [&](int j) {
        if constexpr (PROF) {
            const unsigned long long t = __builtin_amdgcn_s_memtime();
            if (j >= 0) ph[j] += t - t_prev;
            t_prev = t;
        }
    };
    if constexpr (PROF) t_loop = __builtin_amdgcn_s_memtime();

    A acc;
    int buf = 0;
    if (idle) {
        // same barriers, same DMA order and wait counts as a working wave; no LDS reads, no
        // MFMAs, nothing to emit (see dense_scan_f16qs below)
#pragma unroll 1
        for (int64_t j = 0; j < n_half; ++j) {
            asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NB - 2) * PER * C::VM_PER_PIECE) : "memory");
            __builtin_amdgcn_s_barrier();
            const int nbuf = buf == 0 ? NB - 1 : buf - 1;
            const f32x4* src = piece_src(j + NB - 1);
#pragma unroll
            for (int p = 0; p < PER; ++p) dma(src, nbuf, p);
            buf = buf + 1 == NB ? 0 : buf + 1;
        }
    }
    // One half tile, hf of row tile i, into the accumulators ACC (a macro, not a lambda: asm operands
    // do not capture).  After ACC come the arguments of QHalfHook::after: issue_piece (defined in
    // here), then nothing or the emit state.
#define QS_HALF(hf, ACC, ...)                                                                      \
    {                                                                                              \
        stamp(-1);                                                                                 \
        /* own pieces of half tile 2i+hf done (the NB-2 younger half tiles' pieces -- and the      \
           emit's few stores among them, which are over-waited for -- may stay in flight) */       \
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NB - 2) * PER * C::VM_PER_PIECE) : "memory");    \
        stamp(0);                                                                                  \
        __builtin_amdgcn_s_barrier();                                                              \
        stamp(1);                                                                                  \
        const int nbuf = buf == 0 ? NB - 1 : buf - 1; /* half tile j-1's buffer */                 \
        const f32x4* src = piece_src(2 * i + (hf) + NB - 1);                                       \
        auto issue_piece = [&](auto P) { dma(src, nbuf, decltype(P)::value); };                    \
        const uint32_t abase = lds_base + buf * C::HALF_BYTES + lane * 16;                         \
        f32x4 a[C::RING];                                                                          \
        qs_fill<0, HS>(a, abase);                                                                  \
        stamp(2);                                                                                  \
        qs_steps<0, HS, (hf) * HS, KS, QHalfHook<HS, PER, (hf)>>(a, bq, ACC, abase, __VA_ARGS__);  \
        if constexpr (PROF) {                                                                      \
            if constexpr (SHAPE == 32) asm volatile("" : "+v"(ACC.v));                             \
            else {                                                                                 \
                asm volatile("" : "+v"(ACC.t[0]), "+v"(ACC.t[1]), "+v"(ACC.t[2]), "+v"(ACC.t[3])); \
                if constexpr (A::NQB == 3) asm volatile("" : "+v"(ACC.t[4]), "+v"(ACC.t[5]));      \
            }                                                                                      \
        }                                                                                          \
        stamp(3);                                                                                  \
        buf = buf + 1 == NB ? 0 : buf + 1;                                                         \
    }
    // MODE_FILTER: the emit of a row tile runs between the MFMAs of the NEXT one (QHalfHook), out
    // of the other of two accumulator sets; the first tile "emits" a set of -inf (a compare and a
    // branch per register), the last tile's set is emitted after the loop.  Same barriers, same
    // DMA order and wait counts per half tile as below.
    // (Only where a block is alone on its CU -- dim 1024, one wave per SIMD: with two blocks per CU
    // the other block's MFMAs already cover an epilogue, and the second accumulator set does not fit
    // the 256-register budget there.)
    // (And not with 48 queries per wave: 384 B-operand registers leave no room for a second set.)
#ifdef Q_NO_PIPE_EMIT   // (A/B builds: the round-3 loop, the emit after its own tile)
    constexpr bool PIPE_EMIT = false;
#else
    constexpr bool PIPE_EMIT = true;
#endif
    if constexpr (PIPE_EMIT && MODE == MODE_FILTER && !PROF && C::PER_CU == 1 && SHAPE != 48) {
        A acc2[2];
#pragma unroll
        for (int x = 0; x < A::NREG; ++x) {
            if constexpr (SHAPE == 32) acc2[1].v[x] = -INFINITY;
            else acc2[1].t[x >> 2][x & 3] = -INFINITY;
        }
        uint32_t row_of[2] = {0u, 0u};
#define QS_HALF_PE(hf, CUR, PRV) QS_HALF(hf, acc2[CUR], issue_piece, em, acc2[PRV], row_of[PRV], lane)
        const int64_t n_it = idle ? 0 : n_mine;
        int64_t i = 0;
#pragma unroll 1
        for (; i + 1 < n_it; i += 2) {
            acc2[0].zero();
            QS_HALF_PE(0, 0, 1)
            QS_HALF_PE(1, 0, 1)
            row_of[0] = (uint32_t)((first + i * step) * tile_stride * 32);
            ++i;
            acc2[1].zero();
            QS_HALF_PE(0, 1, 0)
            QS_HALF_PE(1, 1, 0)
            row_of[1] = (uint32_t)((first + i * step) * tile_stride * 32);
            --i;
        }
        if (i < n_it) {   // an odd tile left: into set 0, emitting set 1; then set 0 itself
            acc2[0].zero();
            QS_HALF_PE(0, 0, 1)
            QS_HALF_PE(1, 0, 1)
            QS_WAVE_TILE(acc2[0], (uint32_t)((first + i * step) * tile_stride * 32))
        } else if (n_it > 0) {
            QS_WAVE_TILE(acc2[1], row_of[1])
        }
#undef QS_HALF_PE
    } else {
    // one trip = one row tile = two half tiles (the accumulators run through both)
#pragma unroll 1
    for (int64_t i = 0; i < (idle ? 0 : n_mine); ++i) {
        acc.zero();
        QS_HALF(0, acc, issue_piece)
        QS_HALF(1, acc, issue_piece)

        const int64_t t = first + i * step;
        QS_WAVE_TILE(acc, (uint32_t)(t * tile_stride * 32))
        stamp(4);
    }
    }
#undef QS_HALF
    // nothing may still be landing in LDS when the block retires
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    QS_WAVE_WRITE_OUT()
    if constexpr (PROF) {
        if (lane == 0) {
            unsigned long long* o = stamps + ((int64_t)blockIdx.x * Q_NW + wave) * 8;
            for (int j = 0; j < 5; ++j) o[j] = ph[j];
            o[5] = (unsigned long long)n_half;
            o[6] = __builtin_amdgcn_s_memtime() - t_loop;
            o[7] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));  // HW_REG_HW_ID
        }
    }
}

// ---------------------------------------------------------------------------------------------
// dense_scan_f16qs: the same scan with ONE 8-wave block per CU (256 queries) whose two wave groups
// run STAGGERED inside one interval per row tile -- the default at dim <= 768.
//
// What the counters of the two-blocks-per-CU kernel above said (profiles/r2_scan_v2_*.json): pipe
// 64 % busy; the older block of a CU wins the matrix pipe and retires when 3/4 of the launch is
// over, so the pipe is half empty for the last quarter; every CU pulls each tile twice; and the
// chip drops its clock to 1.5-1.7 GHz under the load.  Here the 8 waves share each row tile
// (half the DMA pieces and L2 bytes per flop) and are kept in step by ONE barrier per tile; both
// groups multiply the same tile, and the stagger is the order inside the interval:
//
//     interval t       A (waves 0-3)                        B (waves 4-7)
//                      MFMA tile t, then EMIT tile t        EMIT tile t-1, then MFMA tile t
//
// so an emit always runs under the other group's MFMAs (A is the older wave of the SIMD and gets
// the pipe first: its MFMAs cover B's emit at the start of the interval, B's cover A's at the
// end).  B keeps tile t-1's accumulators across the barrier: there is one accumulator set.
// The index arithmetic -- ring of whole-tile buffers, who issues what into which buffer, what the
// counted wait leaves in flight, barriers per role -- is tsched:: (dense_tile_schedule.hpp), which
// tests/native/dense_tile_schedule_host_check.cpp replays on the host.
//
// Only group B issues row pieces, and only group B waits before a barrier.  vmcnt counts loads,
// stores and LDS-DMA in issue order.  B's emit stores of interval t are issued BEFORE its pieces
// of interval t, so at the wait before barrier t+1 -- s_waitcnt vmcnt((nbuf-2) * PB) -- the PB
// youngest operations per tile left in flight are pieces, never that interval's stores: the wait
// retires tile t+1's pieces (older than the stores) and the stores themselves, which were issued
// a whole multiply earlier.  A's stores are never waited for inside the loop: A issues no piece,
// so it has nothing to wait for, and its LDS reads have all returned into its MFMAs by then.
// ---------------------------------------------------------------------------------------------
constexpr int QS_NW = tsched::N_WAVES;

template <int DIM>
struct QStag {
    static constexpr int KS = tsched::pieces_per_tile(DIM), TILE_BYTES = tsched::tile_bytes(DIM);
    static constexpr int NBUF = tsched::nbuf(DIM);
    static constexpr int PB = tsched::pieces_issued(tsched::ROLE_B, DIM);   // pieces an issuing wave sends per tile
    static constexpr int LDS_BYTES = NBUF * TILE_BYTES;
    static_assert(KS % tsched::N_ISSUERS == 0 && NBUF >= 3 && LDS_BYTES <= tsched::LDS_BUDGET, "dim 512 / 768 only");
    static_assert(tsched::wait_leaves(tsched::ROLE_B, DIM) < 64 && tsched::issue_step(PB - 1) < KS, "vmcnt is 6 bits");
    // Slots of the wave's ring of A fragments (qs_steps_il keeps RING - 1 reads in flight).  Measured
    // (profiles/dense_scan_ring.md): with the old k-loop four and six reads in flight gave the same step
    // time and the same pace of a wave that runs alone, so depth is not what the k-loop waits for; 5 / 6
    // slots keep the four reads in flight the kernel had, and one more at dim 512 where registers are free.
    // Every instantiation of a row length compiles without scratch at this depth (<768, *, 16, true>: 254
    // VGPRs); deeper rings under qs_steps_il were not measured.
    static constexpr int RING = DIM == 512 ? 6 : 5;
};

// The stamped build of dense_scan_f16qs (PROF; thr_dense_scan_stamps_f16 without THR_DENSE_F16=q at
// dim <= 768): every wave takes s_memtime at the points QS_T_* of each interval and folds the
// differences at the interval's end into sums, written as 16 words per wave to
// stamps[(block * 8 + wave) * 16 + QS_PH_*].  The values are consumed only at the fold, so no stamp
// drains the fragment ring inside the interval (a pending s_memtime makes a counted lgkmcnt wait reach
// one slot further at the most).  Group A has no counted wait (0); group B's emit of the previous
// tile is QS_PH_EMIT and its fill latency -- what of barrier release .. first fragment in a register
// is not its emit -- QS_PH_FILL; the emit of B's last tile, after the loop, is not counted.
enum { QS_T_START, QS_T_WAIT, QS_T_BAR, QS_T_EMIT_B, QS_T_FILL, QS_T_Q1, QS_T_Q2, QS_T_Q3, QS_T_K, QS_T_END, QS_T_N };
enum { QS_PH_WAIT = 0,    // counted vmcnt wait for the wave's own pieces (B)
       QS_PH_BARRIER = 1, // s_barrier, arrival to release
       QS_PH_FILL = 2,    // release (B: end of its emit) to the first A fragment in a register
       QS_PH_Q0 = 3,      // k-loop, quarters of KS steps: QS_PH_Q0 .. QS_PH_Q0 + 3
       QS_PH_EMIT = 7,
       QS_PH_INTERVALS = 8, QS_PH_LOOP = 9, QS_PH_HW_ID = 10, QS_PH_N = 16 };
template <bool PROF>
struct QsClock {
    __device__ __forceinline__ void init() {}
    template <int J> __device__ __forceinline__ void at() {}
    template <int J, int K> __device__ __forceinline__ void same() {}
    __device__ __forceinline__ void fold() {}
    __device__ __forceinline__ void write(unsigned long long*, int, int64_t) const {}
};
template <>
struct QsClock<true> {
    unsigned long long t[QS_T_N], sum[QS_PH_INTERVALS], t0;
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int j = 0; j < QS_PH_INTERVALS; ++j) sum[j] = 0;
        t[QS_T_END] = t0 = __builtin_amdgcn_s_memtime();
    }
    template <int J> __device__ __forceinline__ void at() { t[J] = __builtin_amdgcn_s_memtime(); }
    template <int J, int K> __device__ __forceinline__ void same() { t[J] = t[K]; }   // point J not taken: = K
    // end of an interval (t[QS_T_END] taken): the phases, and the next interval's start
    __device__ __forceinline__ void fold() {
        sum[QS_PH_WAIT] += t[QS_T_WAIT] - t[QS_T_START];
        sum[QS_PH_BARRIER] += t[QS_T_BAR] - t[QS_T_WAIT];
        sum[QS_PH_FILL] += t[QS_T_FILL] - t[QS_T_EMIT_B];
        sum[QS_PH_Q0 + 0] += t[QS_T_Q1] - t[QS_T_FILL];
        sum[QS_PH_Q0 + 1] += t[QS_T_Q2] - t[QS_T_Q1];
        sum[QS_PH_Q0 + 2] += t[QS_T_Q3] - t[QS_T_Q2];
        sum[QS_PH_Q0 + 3] += t[QS_T_K] - t[QS_T_Q3];
        sum[QS_PH_EMIT] += (t[QS_T_EMIT_B] - t[QS_T_BAR]) + (t[QS_T_END] - t[QS_T_K]);
    }
    // one lane of the wave, at the end of the launch
    __device__ __forceinline__ void write(unsigned long long* stamps, int wave_of_launch, int64_t intervals) const {
        unsigned long long* o = stamps + (int64_t)wave_of_launch * QS_PH_N;
        for (int j = 0; j < QS_PH_INTERVALS; ++j) o[j] = sum[j];
        o[QS_PH_INTERVALS] = (unsigned long long)intervals;
        o[QS_PH_LOOP] = __builtin_amdgcn_s_memtime() - t0;
        o[QS_PH_HW_ID] = (unsigned long long)__builtin_amdgcn_s_getreg((4 << 0) | (0 << 6) | (31 << 11));  // HW_REG_HW_ID
        for (int j = QS_PH_HW_ID + 1; j < QS_PH_N; ++j) o[j] = 0;
    }
};
// every MFMA issued so far stays in front of what follows (a stamp)
template <int SHAPE>
__device__ __forceinline__ void qs_pin(QAcc<SHAPE>& acc) {
    if constexpr (SHAPE == 32) asm volatile("" : "+v"(acc.v));
    else asm volatile("" : "+v"(acc.t[0]), "+v"(acc.t[1]), "+v"(acc.t[2]), "+v"(acc.t[3]));
}
// QTileHook with the quarter stamps of the stamped build
template <int PB, int KS>
struct QTileStampHook {
    template <int S, typename Issue, int SHAPE>
    static __device__ __forceinline__ void after(Issue& issue_piece, QAcc<SHAPE>& acc, QsClock<true>& clk) {
        QTileHook<PB>::template after<S>(issue_piece);
        if constexpr ((S + 1) % (KS / 4) == 0 && S + 1 < KS) {
            qs_pin(acc);
            clk.template at<QS_T_Q1 + (S + 1) / (KS / 4) - 1>();
        }
    }
};

// The two kernels -- the product one and its stamped build (PROF; MODE_FILTER; see QsClock) -- are
// defined behind their common body, qs_scan.
template <int DIM, int MODE, int SHAPE = 32, bool COLL = true>
__global__ __launch_bounds__(QS_NW * 64) void dense_scan_f16qs(
    const f32x4* __restrict__ packed, const f32x4* __restrict__ qfrag, int n_qtiles,
    int64_t n_tiles, int64_t tile_stride, const float* __restrict__ tau,
    int* __restrict__ seg_cnt, Cand* __restrict__ cand, int seg_cap,
    float* __restrict__ sample,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll, int n_queries);

template <int DIM, int MODE, int SHAPE, bool COLL, bool PROF>
__device__ __forceinline__ void qs_scan(
    const f32x4* __restrict__ packed, const f32x4* __restrict__ qfrag, int n_qtiles,
    int64_t n_tiles, int64_t tile_stride, const float* __restrict__ tau,
    int* __restrict__ seg_cnt, Cand* __restrict__ cand, int seg_cap,
    float* __restrict__ sample,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll, int n_queries,
    unsigned long long* __restrict__ stamps) {
    static_assert(!PROF || MODE == MODE_FILTER, "the stamped build is the filter scan");
    using C = QStag<DIM>;
    using A = QAcc<SHAPE>;
    constexpr int KS = C::KS, PB = C::PB, RING = C::RING;
    static_assert(KS % 4 == 0 && RING >= 3 && RING <= KS, "quarter stamps; qs_steps_il refills the slot read a step ago");
    static_assert(A::QW == 32 && A::NQB * KS / 2 == KS, "32 queries per wave: KS fragments in both shapes");
    extern __shared__ f32x4 lds_rows[];  // NBUF whole-tile buffers

    const ScanSlot slot = scan_slot(n_qtiles);
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int q32 = slot.qtile * QS_NW + wave;   // this wave's 32 queries

    QS_WAVE_SETUP(KS)   // (both shapes: KS fragments)

    namespace ts = tsched;
    const int64_t first = slot.slice, step = slot.nslices;
    const int64_t n_mine = first < n_tiles ? (n_tiles - first + step - 1) / step : 0;
    const uint32_t lds_base = (uint32_t)(size_t)(__attribute__((address_space(3))) void*)lds_rows;
    const ts::Role role = ts::role_of(wave, (int64_t)q32 * 32 >= n_queries);
    const int iw = wave & (ts::N_ISSUERS - 1);   // an issuing wave's place among the issuers
    // this wave's pieces of the block's j-th tile (past the end: the last tile again, never read)
    auto piece_src = [&](int64_t j) -> const f32x4* {
        const int64_t t = first + ts::source_tile(j, n_mine) * step;
        return packed + ((t * tile_stride * KS + iw) * 64 + lane);
    };
    auto dma = [&](const f32x4* src, int buf, int p) {
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(src + (ts::piece_index(iw, p) - iw) * 64),
            (__attribute__((address_space(3))) void*)(size_t)(lds_base + buf * C::TILE_BYTES +
                                                              ts::piece_index(iw, p) * 1024),
            16, 0, 0);
    };
#define QS_EMIT(i_) QS_WAVE_TILE(acc, (uint32_t)((first + (i_) * step) * tile_stride * 32))
    // barrier t of an issuing wave: its own pieces of tile t have landed; the pieces of the
    // nbuf - 2 younger tiles stay in flight, and the emit stores of the interval that ends here
    // are older than the youngest of them (see above), so they are not what the count leaves out
    constexpr int WAIT_B = ts::wait_leaves(ts::ROLE_B, DIM);
    static_assert(WAIT_B == ts::wait_leaves(ts::ROLE_PAD_B, DIM) && ts::pieces_issued(ts::ROLE_PAD_B, DIM) == PB &&
                  ts::pieces_issued(ts::ROLE_A, DIM) == 0 && ts::pieces_issued(ts::ROLE_PAD_A, DIM) == 0,
                  "a padding wave moves what a working wave of its group moves");
#define QS_SYNC_B()                                                    \
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT_B) : "memory");      \
    __builtin_amdgcn_s_barrier();

    if (ts::issues(role) && n_mine > 0) {
#pragma unroll
        for (int b = 0; b < ts::prologue_tiles(DIM); ++b) {
            const f32x4* src = piece_src(b);
#pragma unroll
            for (int p = 0; p < PB; ++p) dma(src, ts::buffer_of(b, DIM), p);
        }
    }
    A acc;
    f32x4 a[RING];
    auto no_piece = [](auto) {};
    QsClock<PROF> clk;
    clk.init();
    // the first A fragment is in a register (the stamped build only: the k-loop waits for it anyway)
#define QS_STAMP_FILL()                                                             \
    if constexpr (PROF) {                                                           \
        asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(RING - 1) : "memory");          \
        clk.template at<QS_T_FILL>();                                               \
    }
    if (!ts::multiplies(role)) {
        // ---- a wave whose 32 queries are all padding (small batches: one query keeps 7 of the 8
        // waves here): same barriers as a working wave of its group, and for an issuer the same
        // DMA order and wait counts; no LDS reads, no MFMAs, nothing to emit.  A launch with one
        // live wave per CU is bound by the row stream alone. ----
        if (ts::issues(role)) {
            int ibuf = ts::buffer_of(ts::issue_tile(0, DIM), DIM);
#pragma unroll 1
            for (int64_t t = 0; t < ts::barriers(ts::ROLE_PAD_B, n_mine); ++t) {
                QS_SYNC_B()   // barrier t, then tile t + nbuf - 1 into tile t - 1's buffer
                const f32x4* src = piece_src(ts::issue_tile(t, DIM));
#pragma unroll
                for (int p = 0; p < PB; ++p) dma(src, ibuf, p);
                ibuf = ts::next_buffer(ibuf, DIM);
            }
        } else {
#pragma unroll 1
            for (int64_t t = 0; t < ts::barriers(ts::ROLE_PAD_A, n_mine); ++t) __builtin_amdgcn_s_barrier();
        }
    } else if (role == ts::ROLE_A) {
        // ---- group A: multiply tile t, then emit it (under B's MFMAs) ----
        int buf = 0;   // buffer of tile i
#pragma unroll 1
        for (int64_t i = 0; i < ts::barriers(ts::ROLE_A, n_mine); ++i) {
            clk.template same<QS_T_START, QS_T_END>();
            clk.template same<QS_T_WAIT, QS_T_END>();
            __builtin_amdgcn_s_barrier();   // barrier i
            clk.template at<QS_T_BAR>();
            clk.template same<QS_T_EMIT_B, QS_T_BAR>();
            const uint32_t abase = lds_base + buf * C::TILE_BYTES + lane * 16;
            qs_fill<0, KS>(a, abase);
            acc.zero();
            QS_STAMP_FILL()
            if constexpr (PROF) {
                qs_steps_il<0, KS, KS, QTileStampHook<0, KS>>(a, bq, acc, abase, no_piece, acc, clk);
                qs_pin(acc);
            } else {
                qs_steps_il<0, KS, KS, QTileHook<0>>(a, bq, acc, abase, no_piece);
            }
            clk.template at<QS_T_K>();
            buf = ts::next_buffer(buf, DIM);
            QS_EMIT(i)
            clk.template at<QS_T_END>();
            clk.fold();
        }
    } else {
        // ---- group B: emit tile t - 1 (under A's MFMAs), then multiply tile t and request tile
        // t + nbuf - 1 in the first steps of it ----
        int buf = 0;   // buffer of tile i
#pragma unroll 1
        for (int64_t i = 0; i < ts::barriers(ts::ROLE_B, n_mine); ++i) {
            clk.template same<QS_T_START, QS_T_END>();
            if constexpr (PROF) {
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT_B) : "memory");
                clk.template at<QS_T_WAIT>();
            }
            QS_SYNC_B()   // barrier i
            clk.template at<QS_T_BAR>();
            if (i > 0) {
                QS_EMIT(i - 1)
            }
            clk.template at<QS_T_EMIT_B>();
            const int ibuf = ts::prev_buffer(buf, DIM);   // tile i - 1's buffer
            const f32x4* src = piece_src(ts::issue_tile(i, DIM));
            auto issue_piece = [&](auto P) { dma(src, ibuf, decltype(P)::value); };
            const uint32_t abase = lds_base + buf * C::TILE_BYTES + lane * 16;
            qs_fill<0, KS>(a, abase);
            acc.zero();
            QS_STAMP_FILL()
            if constexpr (PROF) {
                qs_steps_il<0, KS, KS, QTileStampHook<PB, KS>>(a, bq, acc, abase, issue_piece, acc, clk);
                qs_pin(acc);
            } else {
                qs_steps_il<0, KS, KS, QTileHook<PB>>(a, bq, acc, abase, issue_piece);
            }
            clk.template at<QS_T_K>();
            clk.template same<QS_T_END, QS_T_K>();
            clk.fold();
            buf = ts::next_buffer(buf, DIM);
        }
        if (n_mine > 0) {
            QS_EMIT(n_mine - 1)
        }
    }
#undef QS_STAMP_FILL
#undef QS_SYNC_B
#undef QS_EMIT
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // nothing may still be landing in LDS
    QS_WAVE_WRITE_OUT()
    if (lane == 0) clk.write(stamps, blockIdx.x * QS_NW + wave, n_mine);
}

template <int DIM, int MODE, int SHAPE, bool COLL>
__global__ __launch_bounds__(QS_NW * 64) void dense_scan_f16qs(
    const f32x4* __restrict__ packed, const f32x4* __restrict__ qfrag, int n_qtiles,
    int64_t n_tiles, int64_t tile_stride, const float* __restrict__ tau,
    int* __restrict__ seg_cnt, Cand* __restrict__ cand, int seg_cap,
    float* __restrict__ sample,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll, int n_queries) {
    qs_scan<DIM, MODE, SHAPE, COLL, false>(packed, qfrag, n_qtiles, n_tiles, tile_stride, tau, seg_cnt, cand, seg_cap,
                                           sample, doc_coll, query_coll, n_queries, nullptr);
}
template <int DIM, int SHAPE, bool COLL>
__global__ __launch_bounds__(QS_NW * 64) void dense_scan_f16qs_stamps(
    const f32x4* __restrict__ packed, const f32x4* __restrict__ qfrag, int n_qtiles,
    int64_t n_tiles, int64_t tile_stride, const float* __restrict__ tau,
    int* __restrict__ seg_cnt, Cand* __restrict__ cand, int seg_cap,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll, int n_queries,
    unsigned long long* __restrict__ stamps) {
    qs_scan<DIM, MODE_FILTER, SHAPE, COLL, true>(packed, qfrag, n_qtiles, n_tiles, tile_stride, tau, seg_cnt, cand, seg_cap,
                                                 nullptr, doc_coll, query_coll, n_queries, stamps);
}

#undef QS_WAVE_WRITE_OUT
#undef QS_WAVE_TILE
#undef QS_WAVE_SETUP

}  // namespace thr
