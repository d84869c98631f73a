// What a fuzzy match over UTF-8 keys needs (fuzzy.hip: the vocabulary's nearest terms; written to be shared with a
// later fuzzy entity match): the edit budget of a needle, the lowering of a needle into uint16 code points, the
// decoder of a key as it stands, the banded edit distance and the insertion into a needle's best slots.
#pragma once
#include "../../include/thr_hip_fuzzy.h"
#include "text_common.hpp"

namespace thr {

constexpr int FZ_MAX_LEN = THR_FUZZY_MAX_LEN;      // code points of a needle
constexpr int FZ_MAX_EDITS = 2;
constexpr int FZ_MIN_LEN = 3;                      // a shorter needle has no edit budget
constexpr int FZ_MAX_KEY_CPS = FZ_MAX_LEN + FZ_MAX_EDITS;
constexpr int FZ_MAX_KEY_BYTES = 3 * FZ_MAX_KEY_CPS;   // a longer key holds more code points than any needle reaches
constexpr unsigned long long FZ_EMPTY = ~0ull;     // a best slot nobody took (distance field 3: never a match)

// Lucene's AUTO rule, capped.
__host__ __device__ __forceinline__ int fz_edits(int n, int max_edits) {
    const int d = n < 3 ? 0 : n < 6 ? 1 : 2;
    return d < max_edits ? d : max_edits;
}

// The needle bytes [p, end) of B, lowered through the table, to out[0 .. FZ_MAX_LEN) (zero behind the needle)
// -> its code points, or -1: malformed UTF-8, an exceptional code point, a code point above U+FFFF, more than
// FZ_MAX_LEN code points.  Reads nothing outside [p, end).
__device__ __forceinline__ int fz_lower_needle(const uint8_t* __restrict__ B, int64_t p, int64_t end,
                                               const uint32_t* __restrict__ table, uint16_t* __restrict__ out) {
    int n = 0;
    bool ok = true;
    while (p < end && ok) {
        const int avail = end - p < 4 ? (int)(end - p) : 4;
        int len;
        const uint32_t e = tx_decode(B[p], avail > 1 ? B[p + 1] : 0, avail > 2 ? B[p + 2] : 0, avail, table, len);
        if ((e & (TX_BAD | TX_EXC)) || n == FZ_MAX_LEN) {
            ok = false;
        } else {
            out[n++] = (uint16_t)(e & 0xFFFF);
            p += len;
        }
    }
    if (!ok) n = 0;
    for (int j = n; j < FZ_MAX_LEN; ++j) out[j] = 0;
    return ok ? n : -1;
}

// One character of a key as it stands, ``avail`` (>= 1) bytes of the key left: its code point and encoded length,
// or -1 (not one of the one- to three-byte forms, cut off by the key's end, overlong).  The three-byte form of a
// surrogate is its code point: the project's encoder ("surrogatepass") writes it.
__device__ __forceinline__ int fz_key_cp(uint32_t b0, uint32_t b1, uint32_t b2, int avail, int& len) {
    len = 1;
    if (b0 < 0x80) return (int)b0;
    if (b0 >= 0xC2 && b0 <= 0xDF) {
        if (avail < 2 || !tx_cont(b1)) return -1;
        len = 2;
        return (int)(((b0 & 0x1F) << 6) | (b1 & 0x3F));
    }
    if (b0 >= 0xE0 && b0 <= 0xEF) {
        if (avail < 3 || !tx_cont(b1) || !tx_cont(b2)) return -1;
        const uint32_t cp = ((b0 & 0x0F) << 12) | ((b1 & 0x3F) << 6) | (b2 & 0x3F);
        if (cp < 0x800) return -1;
        len = 3;
        return (int)cp;
    }
    return -1;
}

// Edit distance (insert / delete / substitute, unit cost) between the needle a[0 .. n) and the key b[0], b[bs],
// .. b[(L - 1) bs], for | L - n | <= d <= W: the cells within W of the diagonal only (a path of cost <= d never
// leaves them), one row of 2 W + 1 cells per key character, ended as soon as every cell of a row exceeds d.
// -> the distance when it is <= d, else d + 1.
template <int W>
__device__ __forceinline__ int fz_banded(const uint16_t* a, int n, const uint16_t* b, int bs, int L, int d) {
    constexpr int BW = 2 * W + 1, INF = 64;
    constexpr uint32_t NONE = 0x10000;          // no code point: beside the needle
    int prev[BW], cur[BW];
    uint32_t win[BW];                           // in row i: win[k] = a[i - W + k - 1], the needle character of cell k
#pragma unroll
    for (int k = 0; k < BW; ++k) {
        const int j = k - W;
        prev[k] = j >= 0 && j <= n ? j : INF;   // row 0: D[0][j] = j
        win[k] = j >= 0 && j < n ? a[j] : NONE;
    }
    for (int i = 1; i <= L; ++i) {
        const uint32_t bc = b[(i - 1) * bs];
        int best = INF;
#pragma unroll
        for (int k = 0; k < BW; ++k) {
            const int j = i - W + k;
            int v = INF;
            if (j == 0) {
                v = i;
            } else if (j > 0 && j <= n) {
                v = prev[k] + (win[k] != bc ? 1 : 0);
                if (k + 1 < BW) v = min(v, prev[k + 1] + 1);
                if (k > 0) v = min(v, cur[k - 1] + 1);
            }
            cur[k] = v;
            best = min(best, v);
        }
        if (best > d) return d + 1;
#pragma unroll
        for (int k = 0; k < BW; ++k) {
            prev[k] = cur[k];
            if (k + 1 < BW) win[k] = win[k + 1];
        }
        const int nx = i + W;                   // row i + 1, cell BW - 1
        win[BW - 1] = nx < n ? a[nx] : NONE;
    }
    int out = INF;
#pragma unroll
    for (int k = 0; k < BW; ++k)
        if (k == n - L + W) out = prev[k];
    return out <= d ? out : d + 1;
}

// (distance, frequency descending, id ascending) as one ascending 64-bit key.
__device__ __forceinline__ unsigned long long fz_pack(int dist, int64_t df, int32_t id) {
    const uint64_t f = df > 0x7FFFFFFFll ? 0x7FFFFFFFull : df < 0 ? 0ull : (uint64_t)df;
    return ((unsigned long long)dist << 62) | ((0x7FFFFFFFull - f) << 31) | (unsigned long long)(uint32_t)id;
}

// x into the n_best ascending slots: every step keeps the smaller value and forwards the larger, so slot j ends as
// the (j + 1)-th smallest of everything inserted, whatever the interleaving of the inserters.
__device__ __forceinline__ void fz_insert(unsigned long long* slot, int n_best, unsigned long long x) {
    for (int j = 0; j < n_best && x != FZ_EMPTY; ++j) {
        const unsigned long long old = atomicMin(&slot[j], x);
        x = old > x ? old : x;
    }
}

}  // namespace thr
