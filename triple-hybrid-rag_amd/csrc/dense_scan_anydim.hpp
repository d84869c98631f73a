// Shortlist scan on the f16 matrix cores for ANY row length that is a multiple of 32, up to 4096
// (thr_dense_topk_f16 with docs16 == NULL at a dim the tuned kernels are not built for, or everywhere
// under thr_dense_f16_select(THR_DENSE_F16_ANYDIM)).  The interface of dense_scan_f16: the float32
// rows are streamed and rounded to float16 in registers, no second copy of the corpus, MODE_ALL writes
// the sample scores row-major, MODE_FILTER emits Cand{score, (query-in-tile << ROW_BITS_F16) | row}
// into the tile lists.  The certificate's bound is dense_scan_f16.hpp's: ea*(1+eq) + eq + eps32.
//
// dim is a kernel ARGUMENT: the K loop is a runtime loop of dim / 32 steps, one
// v_mfma_f32_16x16x32_f16 per (16 rows, 16 queries, step).  What is compiled per shape is only the
// query tile, NB blocks of 16 queries (the accumulators must be registers): 64 queries up to dim 768,
// 32 up to 1536, 16 beyond (anydim_qt) -- the tile stays in LDS as float16 for the whole launch and
// has to fit the CU's 160 KiB next to the waves' candidate buffers.
//
// A wave owns row tiles of 32 rows (MF_ROWS: the unit of the sample and of the row slices) = two A
// fragments.  No LDS transpose: the A operand of the 16x16x32 MFMA is 8 consecutive k of ONE row per
// lane, so a lane loads its fragment straight from the row -- float4 #g and #(4+g) of the step's 8
// (g = lane >> 4), i.e. the 4 lanes of a row read 64 contiguous bytes per instruction and the two
// instructions of a step cover the 128-byte line.  k is only a summation index: the query tile is
// laid out with the same permutation.  Three steps of a wave's rows are in flight in registers
// (12 KiB per wave, 96 KiB per CU); the load cursor runs ahead of the MFMAs ACROSS row tiles, so a
// short row (dim 32: one step per tile) streams like a long one.
//
// Query tile in LDS: 16-byte chunk c (8 halves: k-step c >> 2, lane group c & 3) of query q sits at
// chunk index c * QT + q.  A b128 fragment read takes the 16 queries of one (step, group) per
// 16-lane group: 256 contiguous bytes = every bank once, for each of the four lane groups the
// hardware serves a ds_read_b128 in ({0-3,12-15,20-27}, ...: 16 distinct queries each).
// Each B fragment feeds two MFMAs (the wave's two row blocks): LDS 1 KiB per 2 x 16 cycles of MFMA.
//
// Accumulation: one fp32 accumulator per (row, query) through all dim / 32 steps -- a dim-long fp32
// chain and nothing narrower, which is what scan_eps(dim) bounds.
#pragma once
#include "dense_scan_tilelist.hpp"

namespace thr {

constexpr int AD_WAVES = H_WAVES;            // 8 waves: two per SIMD, one workgroup per CU
constexpr int AD_THREADS = AD_WAVES * WAVE;

template <int MODE, bool nt_loads, int NB>
__global__ __launch_bounds__(AD_THREADS) void dense_scan_anydim(
    const float* __restrict__ docs, const float* __restrict__ inv_norm, int64_t n_docs, int dim,
    const float* __restrict__ queries, int n_queries, int64_t n_tiles, int64_t tile_stride,
    const float* __restrict__ tau, int* __restrict__ tile_cnt, Cand* __restrict__ tile_list,
    int tile_cap, float* __restrict__ sample_scores, int64_t sample_ld,
    const int32_t* __restrict__ doc_coll, const int32_t* __restrict__ query_coll) {
    constexpr int QT = 16 * NB;
    constexpr int QBITS = 32 - ROW_BITS_F16;
    static_assert(QT <= (1 << QBITS), "query-in-tile index must fit the packed candidate word");
    extern __shared__ float4 lds_q[];  // [dim / 8][QT] f16 query chunks | AD_WAVES wbufs

    const ScanSlot slot = scan_slot((n_queries + QT - 1) / QT);
    const int qtile = slot.qtile;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int fr = lane & 15, g = lane >> 4;   // fragment row / query, lane group (k sub-block)
    const int cpr = dim / 8;       // 16-byte f16 chunks per query
    const int nsteps = dim / 32;   // K steps
    const int64_t gpr = dim / 4;   // float4 per float32 row
    f32x4* lds_v = reinterpret_cast<f32x4*>(lds_q);
    Cand* wbuf = reinterpret_cast<Cand*>(lds_q + (size_t)cpr * QT) + wave * WBUF;
    int wcnt = 0;
    // (tilelist_flush<false> of dense_scan_tilelist.hpp written out: through the function the
    // MODE_FILTER kernels gain two instructions.  No drain after the copy: see there.)
    auto flush = [&]() {
        int base = 0;
        if (lane == 0) base = atomicAdd(&tile_cnt[qtile], wcnt);
        base = __shfl(base, 0, WAVE);
        for (int i = lane; i < wcnt; i += WAVE)
            if (base + i < tile_cap) tile_list[(int64_t)qtile * tile_cap + base + i] = wbuf[i];
        wcnt = 0;
    };

    // query tile: float32 -> float16 (round to nearest even); padding queries of the last tile are zero
    for (int i = threadIdx.x; i < QT * cpr; i += AD_THREADS) {
        const int q = i % QT, c = i / QT;   // q fastest: a wave's b128 stores are contiguous in LDS
        const int qg = qtile * QT + q;
        f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = lo;
        if (qg < n_queries) {
            // dims of chunk c: the two float4 a lane of group c & 3 pairs up in step c >> 2
            const float* qsrc = queries + (int64_t)qg * dim + 32 * (c >> 2) + 4 * (c & 3);
            lo = *reinterpret_cast<const f32x4*>(qsrc);
            hi = *reinterpret_cast<const f32x4*>(qsrc + 16);
        }
        lds_v[c * QT + q] = pack_f16x8(lo, hi);
    }
    __syncthreads();

    const int64_t wave_id = (int64_t)slot.slice * AD_WAVES + wave;
    const int64_t wave_stride = (int64_t)slot.nslices * AD_WAVES;
    if (wave_id >= n_tiles) return;   // (wave-uniform; no barrier follows)

    float my_tau[NB];
    int my_qc[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int qg = qtile * QT + 16 * nb + fr;
        my_tau[nb] = lane_tau<MODE>(tau, qg);
        my_qc[nb] = lane_coll<MODE>(query_coll, qg, n_queries);
    }

    const f32x4* docs4 = reinterpret_cast<const f32x4*>(docs);
    // ---- the load cursor: (row tile pt, step ps) of the next fragment pair to request.  The row index
    // is clamped to the last row (a clamped row is never emitted) and past the wave's last tile the
    // cursor stays on it: every address is below docs + n_docs * dim.
    int64_t pt = wave_id;
    int ps = 0;
    int64_t p0 = 0, p1 = 0;   // float4 offsets of this lane's next loads, row blocks 0 and 1
    auto set_tile = [&]() {
        int64_t r0 = pt * tile_stride * MF_ROWS + fr, r1 = r0 + 16;
        r0 = r0 < n_docs ? r0 : n_docs - 1;
        r1 = r1 < n_docs ? r1 : n_docs - 1;
        p0 = r0 * gpr + g;
        p1 = r1 * gpr + g;
    };
    auto ld = [&](int64_t p) -> f32x4 {
        return nt_loads ? __builtin_nontemporal_load(&docs4[p]) : docs4[p];
    };
    auto load = [&](f32x4(&a)[4]) {
        a[0] = ld(p0);
        a[1] = ld(p0 + 4);
        a[2] = ld(p1);
        a[3] = ld(p1 + 4);
        p0 += 8;
        p1 += 8;
        if (++ps == nsteps) {   // (wave-uniform)
            ps = 0;
            if (pt + wave_stride < n_tiles) pt += wave_stride;
            set_tile();
        }
    };

    // ---- the compute cursor: (row tile t, step s)
    int64_t t = wave_id;
    int s = 0;
    f32x4 acc[2][NB];
    auto clear = [&]() {
#pragma unroll
        for (int af = 0; af < 2; ++af)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[af][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    auto tile_inv = [&](int64_t tt) -> float {   // 1 / ||row|| of row (lane & 31) of the tile, clamped
        const int64_t row0 = tt * tile_stride * MF_ROWS;
        int64_t row = row0 + (lane & 31);
        row = row < n_docs ? row : n_docs - 1;
        return inv_norm[row];
    };
    float my_inv = tile_inv(t);

    // the tile's 32 x QT scores are complete: write or filter them.  The accumulator of lane (fr, g),
    // row block af, query block nb, register j is (row 16 af + 4 g + j, query 16 nb + fr).
    auto finish_tile = [&]() {
        const int64_t row0 = t * tile_stride * MF_ROWS;
#pragma unroll
        for (int af = 0; af < 2; ++af) {
            float inv[4];
            bool ok[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = 16 * af + 4 * g + j;
                inv[j] = __shfl(my_inv, row, WAVE);
                ok[j] = row0 + row < n_docs && inv[j] > 0.f;
            }
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                if constexpr (MODE == MODE_ALL) {
                    // registers 0..3 are 4 consecutive rows: one 16-byte store
                    f32x4 v;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = ok[j] ? acc[af][nb][j] * inv[j] : -INFINITY;
                    const int qg = qtile * QT + 16 * nb + fr;
                    *reinterpret_cast<f32x4*>(sample_scores + (int64_t)qg * sample_ld + t * MF_ROWS +
                                              16 * af + 4 * g) = v;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int row = 16 * af + 4 * g + j;
                        const float sc = acc[af][nb][j] * inv[j];
                        bool pass = ok[j] && sc >= my_tau[nb];
                        if (pass && my_qc[nb] != -1 && doc_coll[row0 + row] != my_qc[nb]) pass = false;
                        THR_TILELIST_PUSH(pass, sc, ((uint32_t)(16 * nb + fr) << ROW_BITS_F16) | (uint32_t)(row0 + row))
                    }
                }
            }
        }
    };

    // one K step: request the fragments three steps ahead, then 2 NB MFMAs on the oldest.  Behind the
    // wave's last tile a step only loads (the cursor stays on that tile): the loop below then has no
    // exit between its steps, and every wait inside it counts loads the same way on every path.
    auto step = [&](f32x4(&cur)[4], f32x4(&nxt)[4]) {
        load(nxt);
        if (t >= n_tiles) return;   // (wave-uniform)
        const half8 a0 = __builtin_bit_cast(half8, pack_f16x8(cur[0], cur[1]));
        const half8 a1 = __builtin_bit_cast(half8, pack_f16x8(cur[2], cur[3]));
        const f32x4* qb = lds_v + (4 * s + g) * QT + fr;
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
            const half8 b = __builtin_bit_cast(half8, qb[16 * nb]);
            acc[0][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a0, b, acc[0][nb], 0, 0, 0);
            acc[1][nb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a1, b, acc[1][nb], 0, 0, 0);
        }
        if (++s == nsteps) {   // (wave-uniform)
            finish_tile();
            clear();
            s = 0;
            t += wave_stride;
            if (t < n_tiles) my_inv = tile_inv(t);
        }
    };

    // ring of three register sets, rotated by name (a copy would wait for the load it moves)
    f32x4 r0[4], r1[4], r2[4];
    set_tile();
    clear();
    load(r0);
    load(r1);
    do {
        step(r0, r2);
        step(r1, r0);
        step(r2, r1);
    } while (t < n_tiles);
    if constexpr (MODE == MODE_FILTER) {
        if (wcnt > 0) flush();
    }
}

}  // namespace thr
