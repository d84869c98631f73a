// What the text kernels share (text.hip: tokens and lookups; vocab_grow.hip: numbering new terms): the bits
// of a table entry, the vocabulary hash of thr_hip.h and the decoder of one UTF-8 character.
#pragma once
#include "thr_common.hpp"

namespace thr {

constexpr uint32_t TX_WORD = 1u << 16, TX_EXC = 1u << 17, TX_BAD = 1u << 18;   // (TX_BAD: never in a table)
constexpr uint64_t TX_FNV_BASIS = 0xCBF29CE484222325ull, TX_FNV_PRIME = 0x100000001B3ull;

__device__ __forceinline__ uint64_t tx_fnv(uint64_t h, uint32_t byte) { return (h ^ byte) * TX_FNV_PRIME; }
__device__ __forceinline__ uint64_t tx_fnv_end(uint64_t h) { return h ? h : 1; }
__device__ __forceinline__ uint32_t tx_home(uint64_t h, uint32_t mask) { return (uint32_t)(h ^ (h >> 32)) & mask; }

// FNV-1a over the UTF-8 encoding of one BMP code point.
__device__ __forceinline__ uint64_t tx_fnv_cp(uint64_t h, uint32_t cp) {
    if (cp < 0x80) return tx_fnv(h, cp);
    if (cp < 0x800) return tx_fnv(tx_fnv(h, 0xC0 | (cp >> 6)), 0x80 | (cp & 63));
    return tx_fnv(tx_fnv(tx_fnv(h, 0xE0 | (cp >> 12)), 0x80 | ((cp >> 6) & 63)), 0x80 | (cp & 63));
}

__device__ __forceinline__ bool tx_cont(uint32_t b) { return (b & 0xC0) == 0x80; }

// The character whose lead byte is b0, of which ``avail`` (>= 1) bytes lie inside its text: its table entry
// (TX_BAD alone: malformed, truncated, overlong, or above U+FFFF) and its encoded length (1 when bad).
__device__ __forceinline__ uint32_t tx_decode(uint32_t b0, uint32_t b1, uint32_t b2, int avail,
                                              const uint32_t* __restrict__ table, int& len) {
    len = 1;
    if (b0 < 0x80) return table[b0];
    if (b0 >= 0xC2 && b0 <= 0xDF) {
        if (avail < 2 || !tx_cont(b1)) return TX_BAD;
        len = 2;
        return table[((b0 & 0x1F) << 6) | (b1 & 0x3F)];
    }
    if (b0 >= 0xE0 && b0 <= 0xEF) {
        if (avail < 3 || !tx_cont(b1) || !tx_cont(b2)) return TX_BAD;
        const uint32_t cp = ((b0 & 0x0F) << 12) | ((b1 & 0x3F) << 6) | (b2 & 0x3F);
        if (cp < 0x800) return TX_BAD;   // overlong
        len = 3;
        return table[cp];                // (a surrogate's entry carries TX_EXC)
    }
    return TX_BAD;                       // a continuation byte, 0xC0, 0xC1, a four-byte lead, 0xF5 ..
}

// first index in [lo, hi) whose ptr is above x, else hi
__device__ __forceinline__ int64_t tx_upper(const int64_t* __restrict__ ptr, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (ptr[mid] <= x) lo = mid + 1; else hi = mid;
    }
    return lo;
}

}  // namespace thr
