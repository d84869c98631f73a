// Query and chunk text to BM25 term ids, for a whole batch, on the device.
//
// The reference hands text to PostgreSQL: plainto_tsquery(p_query) inside rag2_lexical_search for a
// query (rag2_schema.sql:365), and the child-chunk insert of ingest.py for a row, whose text column
// the database tokenises.  The host restatement is backend.tokenize (\w+ over text.lower()), a lookup
// in store.vocab and GpuIndexClient._query_terms.  Here the same three steps run on UTF-8 bytes.
//
// The analysis is DATA: a uint32 [65536] table with one entry per BMP code point (index_text.TextTable):
// bits 0..15 the lowered code point, bit 16 "the lowered character is a word character", bit 17
// "exceptional" (the per-character model does not hold for it).  A text that holds an exceptional code
// point, a code point above U+FFFF, a surrogate or malformed UTF-8 gets bit 0 of its flags and is redone
// by the caller on the host; its neighbours are not affected.
//
// The vocabulary is an open-addressing table of 16-byte slots {uint64 hash, int32 term_id, int32 pad}
// (hash 0 = empty; see thr_hip.h for the hash) beside the key store term_bytes / term_ptr.
//
// vocab_insert   one thread per key: hash, then claim the first free slot from the home slot on by a
//                64-bit compare-and-swap on the hash word, then write the id.
// text_count     a workgroup stages one slice of THR_TEXT_SLICE_BYTES bytes in LDS (3 bytes of halo in
//                front, 4 behind) with a bitmap of the text boundaries inside it; a lane classifies one
//                byte; a wave owns a quarter of the slice (a UNIT) and counts its token starts.
// text_scan      exclusive scan of the unit counts (one workgroup): where each unit's token rows begin.
// text_emit      the same classification; a token-start lane finds its text (binary search over the
//                texts of the slice), walks the token in global memory lowering and hashing as it goes,
//                probes the vocabulary, verifies the hit byte for byte and writes its row.  Flags and
//                per-text counts are commuting atomics (or / add).  Unknown tokens are counted per unit.
// text_unknown   after a second scan: per unit the rows with term -1, compacted in order.
// query_terms    one wave per query over its token rows, 64 at a time: the distinct known ids in order of
//                first appearance.
// Nothing waits for another workgroup, nothing is read back, every output is the same bits every run.
//
// thr_text_tokens_analyzed (thr_hip_text.h) is the same three kernels with the token-level analysis switched on
// by a template parameter: a stop set (the vocabulary's layout, the vocabulary's probe) and suffix rules.  A stop
// token gets no row, so the count pass must know it: it walks each token and probes the stop set there (only when
// there is a stop list), and the emit pass decides again, from the same bytes, the same way.  The emit pass keeps
// the token's last 32 lowered code points in eight 64-bit shift registers while it walks, matches the rules of
// each step against them (staged in LDS once per workgroup) and, when something was stripped, walks the kept
// prefix again for its hash.
#include "../../include/thr_hip_text.h"
#include "text_common.hpp"

namespace thr {

constexpr int TX_THREADS = 256;
constexpr int TX_WAVES = TX_THREADS / WAVE;
constexpr int TX_SLICE = THR_TEXT_SLICE_BYTES;
constexpr int TX_UNIT = TX_SLICE / TX_WAVES;          // consecutive bytes per wave
constexpr int TX_ROUNDS = TX_UNIT / WAVE;
constexpr int TX_FRONT = 3, TX_BACK = 4;              // halo bytes staged around a slice
constexpr int TX_LDS = 16 + TX_SLICE + 16;            // the slice starts at byte 16 of the buffer (aligned copies)
constexpr int TX_BIT0 = 32;                           // boundary bits: 32 positions of halo on either side
constexpr int TX_BITS = TX_BIT0 + TX_SLICE + 32;
constexpr int TX_SCAN_THREADS = 1024;
constexpr int TX_TAIL_CPS = THR_STEM_MAX_STEPS * THR_STEM_MAX_SUFFIX;   // what the steps can strip between them
constexpr int TX_TAIL_WORDS = TX_TAIL_CPS / 4;
constexpr int TX_RULE_WORDS = 6;                      // a 24-byte rule as uint32 words
static_assert(TX_TAIL_CPS % 4 == 0 && THR_STEM_MAX_SUFFIX == 8, "a rule's suffix is two 64-bit words of code points");
static_assert(TX_SLICE % (TX_THREADS * 16) == 0, "slices are staged in 16-byte pieces");
static_assert(TX_UNIT % WAVE == 0, "a wave takes whole rounds");

struct VocabSlot {
    uint64_t hash;
    int32_t term_id;
    int32_t pad;
};
static_assert(sizeof(VocabSlot) == 16, "the slot layout is part of the ABI");

__global__ __launch_bounds__(TX_THREADS) void vocab_insert(VocabSlot* __restrict__ slots, uint32_t mask,
                                                           const uint8_t* __restrict__ term_bytes,
                                                           const int64_t* __restrict__ term_ptr, int32_t first_id,
                                                           int32_t count) {
    const int i = blockIdx.x * TX_THREADS + threadIdx.x;
    if (i >= count) return;
    const int32_t id = first_id + i;
    const int64_t a = term_ptr[id], b = term_ptr[id + 1];
    uint64_t h = TX_FNV_BASIS;
    for (int64_t p = a; p < b; ++p) h = tx_fnv(h, term_bytes[p]);
    h = tx_fnv_end(h);
    uint32_t s = tx_home(h, mask);
    for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {   // (load <= 1/2: a free one exists)
        const unsigned long long old =
            atomicCAS(reinterpret_cast<unsigned long long*>(&slots[s].hash), 0ull, (unsigned long long)h);
        if (old == 0ull) {
            slots[s].term_id = id;
            return;
        }
    }
}

struct TextArgs {
    const uint8_t* bytes;
    const int64_t* ptr;        // [n + 1]
    int64_t n, n_bytes;
    const uint32_t* table;
};

struct Vocab {
    const VocabSlot* slots;
    uint32_t mask;
    const uint8_t* term_bytes;
    const int64_t* term_ptr;
    int64_t n_vocab;
};

struct Slice {
    uint8_t* text;             // text[16 + i] = byte g0 + i, i in [-TX_FRONT, TX_SLICE + TX_BACK)
    uint32_t* bits;            // bit TX_BIT0 + i: a text begins (or the data ends) at byte g0 + i
    int64_t g0, d_lo, d_hi;    // texts d_lo .. d_hi: those with ptr[d] <= a byte of the slice or of its front halo
};

__device__ __forceinline__ bool tx_bit(const uint32_t* bits, int i) {
    return (bits[(i + TX_BIT0) >> 5] >> ((i + TX_BIT0) & 31)) & 1u;
}

// Stage slice ``sl``.  Bytes outside [0, n_bytes) are staged as zero (a continuation byte is never zero:
// a character cut off by the end of the data is malformed).  Ends behind a barrier.
__device__ __forceinline__ void tx_stage(const TextArgs& T, int64_t sl, Slice& S, int64_t* range) {
    S.g0 = sl * TX_SLICE;
    for (int i = threadIdx.x; i < TX_BITS / 32; i += TX_THREADS) S.bits[i] = 0;
    for (int i = threadIdx.x * 16; i < TX_LDS; i += TX_THREADS * 16) {
        const int64_t g = S.g0 - 16 + i;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g >= 0 && g + 16 <= T.n_bytes) {
            v = *reinterpret_cast<const uint4*>(T.bytes + g);
        } else if (g + 16 > 0 && g < T.n_bytes) {
            uint8_t* b = reinterpret_cast<uint8_t*>(&v);
            for (int j = 0; j < 16; ++j)
                if (g + j >= 0 && g + j < T.n_bytes) b[j] = T.bytes[g + j];
        }
        *reinterpret_cast<uint4*>(S.text + i) = v;
    }
    if (threadIdx.x == 0) range[0] = tx_upper(T.ptr, 0, T.n + 1, S.g0 - TX_BIT0) - 1;        // may be -1
    if (threadIdx.x == 64) range[1] = tx_upper(T.ptr, 0, T.n + 1, S.g0 + TX_SLICE - 1) - 1;
    __syncthreads();
    S.d_lo = range[0];
    S.d_hi = range[1];
    // the boundaries in [g0 - TX_BIT0, g0 + TX_SLICE + 32): ptr is ascending, so the run ends at the first above it
    for (int64_t d = (S.d_lo < 0 ? 0 : S.d_lo) + threadIdx.x; d <= T.n; d += TX_THREADS) {
        const int64_t v = T.ptr[d];
        const int64_t i = v - S.g0 + TX_BIT0;
        if (i >= TX_BITS) break;
        if (i >= 0) atomicOr(&S.bits[i >> 5], 1u << (i & 31));
    }
    __syncthreads();
}

// What the byte at slice position lp is.  start: a token begins here; bad: the byte makes its text exceptional.
__device__ __forceinline__ void tx_classify(const TextArgs& T, const Slice& S, int lp, bool& start, bool& bad) {
    start = bad = false;
    if (S.g0 + lp >= T.n_bytes) return;
    const uint8_t* t = S.text + 16 + lp;
    const uint32_t b0 = t[0];
    const bool first = tx_bit(S.bits, lp);
    if (tx_cont(b0)) {
        // valid iff it continues a lead 1 .. 3 bytes back with no text boundary in between
        bool ok = false;
        if (!first) {
            const uint32_t m1 = t[-1];
            if (m1 >= 0xC2 && m1 <= 0xF4) ok = true;
            else if (tx_cont(m1) && !tx_bit(S.bits, lp - 1)) {
                const uint32_t m2 = t[-2];
                if (m2 >= 0xE0 && m2 <= 0xF4) ok = true;
                else if (tx_cont(m2) && !tx_bit(S.bits, lp - 2)) ok = t[-3] >= 0xF0 && t[-3] <= 0xF4;
            }
        }
        bad = !ok;
        return;
    }
    int avail = 1;
    while (avail < 4 && !tx_bit(S.bits, lp + avail)) ++avail;     // (the end of the data is a boundary)
    int len;
    const uint32_t e = tx_decode(b0, t[1], t[2], avail, T.table, len);
    bad = (e & (TX_EXC | TX_BAD)) != 0;
    if (!(e & TX_WORD) || (e & TX_BAD)) return;
    if (first) {
        start = true;
        return;
    }
    // the character in front (same text): a word character continues its token
    const uint32_t m1 = t[-1];
    uint32_t pe = 0;
    if (m1 < 0x80) {
        pe = T.table[m1];
    } else if (tx_cont(m1)) {
        const uint32_t m2 = t[-2];
        if (m2 >= 0xC2 && m2 <= 0xDF) {
            pe = T.table[((m2 & 0x1F) << 6) | (m1 & 0x3F)];
        } else if (tx_cont(m2)) {
            const uint32_t m3 = t[-3];
            if (m3 >= 0xE0 && m3 <= 0xEF) {
                const uint32_t cp = ((m3 & 0x0F) << 12) | ((m2 & 0x3F) << 6) | (m1 & 0x3F);
                pe = cp < 0x800 ? 0 : T.table[cp];
            }
        }
    }
    start = !(pe & TX_WORD);
}

// out[i] = in[0] + .. + in[i - 1] for i in 0 .. n (n + 1 values); one workgroup.
__global__ __launch_bounds__(TX_SCAN_THREADS) void text_scan(const int32_t* in, int64_t n, int32_t* out,
                                                             int32_t* total) {
    __shared__ int32_t tmp[TX_SCAN_THREADS];
    const int64_t per = (n + TX_SCAN_THREADS - 1) / TX_SCAN_THREADS;
    const int64_t a = per * threadIdx.x, b = a + per < n ? a + per : n;
    int32_t s = 0;
    for (int64_t i = a; i < b; ++i) s += in[i];
    tmp[threadIdx.x] = s;
    block_inclusive_scan<TX_SCAN_THREADS>(tmp);
    int32_t run = tmp[threadIdx.x] - s;
    for (int64_t i = a; i < b; ++i) {
        const int32_t v = in[i];     // (read before written: in and out may be one array)
        out[i] = run;
        run += v;
    }
    if (threadIdx.x == TX_SCAN_THREADS - 1) {
        out[n] = tmp[TX_SCAN_THREADS - 1];
        if (total) *total = tmp[TX_SCAN_THREADS - 1];
    }
}

// The last THR_STEM_MAX_STEPS * THR_STEM_MAX_SUFFIX lowered code points of a token, 16 bits each, the last one in
// the low bits of w[0].  Only ever indexed by constants (unrolled): it lives in registers.
struct Tail {
    uint64_t w[TX_TAIL_WORDS];
};

// Walk the token that starts at byte p of a text that ends at ``end``, at most max_cp characters of it:
// -> the byte behind the last character taken; the FNV state over the lowered characters (before tx_fnv_end),
// their encoded length and their number; with TAIL the last lowered code points.
template <bool TAIL>
__device__ __forceinline__ int64_t tx_walk(const TextArgs& T, int64_t p, int64_t end, int64_t max_cp, uint64_t& h_out,
                                           int64_t& low_len_out, int64_t& n_cp_out, Tail& tail) {
    const uint8_t* B = T.bytes;
    uint64_t h = TX_FNV_BASIS;
    int64_t q = p;
    int64_t low_len = 0, n_cp = 0;     // bytes and characters of the lowered token
    if (TAIL) {
#pragma unroll
        for (int j = 0; j < TX_TAIL_WORDS; ++j) tail.w[j] = 0;
    }
    while (q < end && n_cp < max_cp) {
        const int avail = end - q < 4 ? (int)(end - q) : 4;
        int len;
        const uint32_t e = tx_decode(B[q], avail > 1 ? B[q + 1] : 0, avail > 2 ? B[q + 2] : 0, avail, T.table, len);
        if ((e & TX_BAD) || !(e & TX_WORD)) break;
        const uint32_t cp = e & 0xFFFF;
        h = tx_fnv_cp(h, cp);
        low_len += cp < 0x80 ? 1 : cp < 0x800 ? 2 : 3;
        ++n_cp;
        if (TAIL) {
#pragma unroll
            for (int j = TX_TAIL_WORDS - 1; j > 0; --j) tail.w[j] = (tail.w[j] << 16) | (tail.w[j - 1] >> 48);
            tail.w[0] = (tail.w[0] << 16) | cp;
        }
        q += len;
    }
    h_out = h;
    low_len_out = low_len;
    n_cp_out = n_cp;
    return q;
}

// Probe table V for the lowered bytes [p, q) of a text that ends at ``end`` (h: their FNV state, low_len: their
// lowered length) -> the id of the key that equals them byte for byte, or -1.  The vocabulary's lookup and the
// stop set's: one function.
__device__ __forceinline__ int32_t tx_probe(const TextArgs& T, const Vocab& V, int64_t p, int64_t q, int64_t end,
                                            uint64_t h, int64_t low_len) {
    const uint8_t* B = T.bytes;
    h = tx_fnv_end(h);
    uint32_t s = tx_home(h, V.mask);
    for (uint32_t probe = 0; probe <= V.mask; ++probe, s = (s + 1) & V.mask) {
        const VocabSlot slot = V.slots[s];
        if (slot.hash == 0) return -1;
        if (slot.hash != h) continue;
        const int32_t id = slot.term_id;
        if (id < 0 || id >= V.n_vocab) continue;
        const int64_t ka = V.term_ptr[id], kb = V.term_ptr[id + 1];
        if (kb - ka != low_len) continue;
        // byte for byte: the token lowered again against the key as it stands
        bool same = true;
        int64_t k = ka;
        for (int64_t r = p; r < q && same;) {
            const int avail = end - r < 4 ? (int)(end - r) : 4;
            int len;
            const uint32_t cp =
                tx_decode(B[r], avail > 1 ? B[r + 1] : 0, avail > 2 ? B[r + 2] : 0, avail, T.table, len) & 0xFFFF;
            if (cp < 0x80) {
                same = V.term_bytes[k] == cp;
                k += 1;
            } else if (cp < 0x800) {
                same = V.term_bytes[k] == (0xC0 | (cp >> 6)) && V.term_bytes[k + 1] == (0x80 | (cp & 63));
                k += 2;
            } else {
                same = V.term_bytes[k] == (0xE0 | (cp >> 12)) && V.term_bytes[k + 1] == (0x80 | ((cp >> 6) & 63)) &&
                       V.term_bytes[k + 2] == (0x80 | (cp & 63));
                k += 3;
            }
            r += len;
        }
        if (same) return id;
    }
    return -1;
}

constexpr int64_t TX_NO_LIMIT = INT64_MAX;

// The token that starts at byte p of a text that ends at ``end``: its byte length and its term id (-1: none).
__device__ __forceinline__ int32_t tx_lookup(const TextArgs& T, const Vocab& V, int64_t p, int64_t end, int32_t& tok_len) {
    uint64_t h;
    int64_t low_len, n_cp;
    Tail none;
    const int64_t q = tx_walk<false>(T, p, end, TX_NO_LIMIT, h, low_len, n_cp, none);
    tok_len = (int32_t)(q - p);
    return tx_probe(T, V, p, q, end, h, low_len);
}

// ---- the token-level analysis (thr_hip_text.h): a stop set in the vocabulary's layout and a table of suffix rules
struct Analysis {
    Vocab stop;                              // slots null: no stop list
    const uint32_t* rules;                   // TX_RULE_WORDS uint32 per rule: tail[8] as four words, len, min_stem
    int32_t step[THR_STEM_MAX_STEPS + 1];    // rules step[s] .. step[s + 1] - 1 are step s; checked on the host
    int32_t n_steps;
};

// Rules to LDS, once per workgroup, with len clamped to 1 .. THR_STEM_MAX_SUFFIX and min_stem to >= 1: the table is
// device memory, which the host cannot check.  The caller's next barrier publishes them.
__device__ __forceinline__ void tx_stage_rules(const Analysis& A, uint32_t* rules) {
    const int words = A.step[A.n_steps] * TX_RULE_WORDS;
    for (int i = threadIdx.x; i < words; i += TX_THREADS) {
        uint32_t v = A.rules[i];
        const int field = i % TX_RULE_WORDS;
        if (field == 4) v = (int32_t)v < 1 ? 1u : v > (uint32_t)THR_STEM_MAX_SUFFIX ? (uint32_t)THR_STEM_MAX_SUFFIX : v;
        if (field == 5) v = (int32_t)v < 1 ? 1u : v;
        rules[i] = v;
    }
}

// Code points s .. s + 7 from the end of the token (s <= TX_TAIL_CPS - THR_STEM_MAX_SUFFIX), 16 bits each.
__device__ __forceinline__ void tx_tail_window(const Tail& t, int s, uint64_t& lo, uint64_t& hi) {
    const int word = s >> 2, sh = (s & 3) * 16;
    uint64_t a = 0, b = 0, c = 0;
#pragma unroll
    for (int j = 0; j < TX_TAIL_WORDS; ++j) {
        if (j == word) a = t.w[j];
        if (j == word + 1) b = t.w[j];
        if (j == word + 2) c = t.w[j];
    }
    lo = sh ? (a >> sh) | (b << (64 - sh)) : a;
    hi = sh ? (b >> sh) | (c << (64 - sh)) : b;
}

// The code points the steps strip from a token of n_cp characters: per step the FIRST rule in table order whose
// suffix ends the token as it stands and leaves at least its min_stem characters.
__device__ __forceinline__ int tx_stem(const Analysis& A, const uint32_t* rules, const Tail& tail, int64_t n_cp) {
    int s = 0;
    for (int st = 0; st < A.n_steps; ++st) {
        uint64_t lo, hi;
        tx_tail_window(tail, s, lo, hi);
        for (int r = A.step[st]; r < A.step[st + 1]; ++r) {
            const uint32_t* R = rules + r * TX_RULE_WORDS;
            const int L = (int)R[4];
            if (n_cp - s - L < (int64_t)(int32_t)R[5]) continue;
            const uint64_t rlo = R[0] | ((uint64_t)R[1] << 32), rhi = R[2] | ((uint64_t)R[3] << 32);
            const uint64_t mlo = L >= 4 ? ~0ull : (1ull << (16 * L)) - 1;
            const uint64_t mhi = L <= 4 ? 0ull : L >= 8 ? ~0ull : (1ull << (16 * (L - 4))) - 1;
            if ((((lo ^ rlo) & mlo) | ((hi ^ rhi) & mhi)) == 0) {
                s += L;
                break;
            }
        }
    }
    return s;
}

// Is the token at byte p a stop word?  The whole lowered token, before any stemming.  (The count pass.)
__device__ __forceinline__ bool tx_is_stop(const TextArgs& T, const Analysis& A, int64_t p, int64_t end) {
    uint64_t h;
    int64_t low_len, n_cp;
    Tail none;
    const int64_t q = tx_walk<false>(T, p, end, TX_NO_LIMIT, h, low_len, n_cp, none);
    return tx_probe(T, A.stop, p, q, end, h, low_len) >= 0;
}

// The analysed token at byte p -> kept (false: a stop word, no row); its term is the STEM's id and tok_len the
// bytes of the kept prefix in the text.  A stem shorter than the token is walked again for its hash.
__device__ __forceinline__ bool tx_lookup_analyzed(const TextArgs& T, const Vocab& V, const Analysis& A,
                                                   const uint32_t* rules, int64_t p, int64_t end, int32_t& term,
                                                   int32_t& tok_len) {
    uint64_t h;
    int64_t low_len, n_cp;
    Tail tail;
    int64_t q = tx_walk<true>(T, p, end, TX_NO_LIMIT, h, low_len, n_cp, tail);
    if (A.stop.slots && tx_probe(T, A.stop, p, q, end, h, low_len) >= 0) return false;
    const int strip = tx_stem(A, rules, tail, n_cp);
    if (strip > 0) {
        Tail none;
        int64_t kept;
        q = tx_walk<false>(T, p, end, n_cp - strip, h, low_len, kept, none);
    }
    tok_len = (int32_t)(q - p);
    term = tx_probe(T, V, p, q, end, h, low_len);
    return true;
}

// The text of byte gp among texts d_lo .. d_hi of the slice, or -1 (a byte in front of ptr[0] or behind ptr[n]).
__device__ __forceinline__ int64_t tx_doc(const TextArgs& T, const Slice& S, int64_t gp) {
    const int64_t lo = S.d_lo < 0 ? 0 : S.d_lo;
    const int64_t hi = S.d_hi + 1 < T.n ? S.d_hi + 1 : T.n;      // texts only: ptr[n] is the end
    const int64_t d = tx_upper(T.ptr, lo, hi, gp) - 1;
    if (d < 0 || d >= T.n || T.ptr[d] > gp || T.ptr[d + 1] <= gp) return -1;
    return d;
}

// The end of text d for a token that starts at byte gp (d < 0: the byte belongs to no text).
__device__ __forceinline__ int64_t tx_text_end(const TextArgs& T, int64_t d, int64_t gp) {
    const int64_t end = d >= 0 ? T.ptr[d + 1] : gp + 1;
    return end < T.n_bytes ? end : T.n_bytes;
}

// ANALYZED: a token start that is a stop word is not counted (a token of no text is never one).
template <bool ANALYZED>
__global__ __launch_bounds__(TX_THREADS) void text_count(TextArgs T, Analysis A, int32_t* __restrict__ unit_count) {
    __shared__ __attribute__((aligned(16))) uint8_t text[TX_LDS];
    __shared__ uint32_t bits[TX_BITS / 32];
    __shared__ int64_t range[2];
    Slice S;
    S.text = text;
    S.bits = bits;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    tx_stage(T, blockIdx.x, S, range);
    int c = 0;
#pragma unroll 1
    for (int r = 0; r < TX_ROUNDS; ++r) {
        const int lp = wave * TX_UNIT + r * WAVE + lane;
        bool start, bad;
        tx_classify(T, S, lp, start, bad);
        if (ANALYZED && start && A.stop.slots) {
            const int64_t gp = S.g0 + lp;
            const int64_t d = tx_doc(T, S, gp);
            if (d >= 0 && tx_is_stop(T, A, gp, tx_text_end(T, d, gp))) start = false;
        }
        c += __popcll(__ballot(start));
    }
    if (lane == 0) unit_count[(int64_t)blockIdx.x * TX_WAVES + wave] = c;
}

template <bool ANALYZED>
__global__ __launch_bounds__(TX_THREADS) void text_emit(TextArgs T, Vocab V, Analysis A,
                                                        const int32_t* __restrict__ unit_off, int64_t capacity,
                                                        int32_t* __restrict__ tok_doc, int32_t* __restrict__ tok_term,
                                                        int64_t* __restrict__ tok_off, int32_t* __restrict__ tok_len,
                                                        int32_t* __restrict__ n_tokens, int32_t* __restrict__ flags,
                                                        int32_t* __restrict__ unit_unknown) {
    __shared__ __attribute__((aligned(16))) uint8_t text[TX_LDS];
    __shared__ uint32_t bits[TX_BITS / 32];
    __shared__ int64_t range[2];
    __shared__ uint32_t rules[ANALYZED ? THR_STEM_MAX_RULES * TX_RULE_WORDS : 1];
    Slice S;
    S.text = text;
    S.bits = bits;
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (ANALYZED) tx_stage_rules(A, rules);       // (tx_stage's barriers stand between this and the first use)
    tx_stage(T, blockIdx.x, S, range);
    const int64_t unit = (int64_t)blockIdx.x * TX_WAVES + wave;
    int64_t row = unit_off[unit];
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    int unknown = 0;
#pragma unroll 1
    for (int r = 0; r < TX_ROUNDS; ++r) {
        const int lp = wave * TX_UNIT + r * WAVE + lane;
        bool start, bad;
        tx_classify(T, S, lp, start, bad);
        const int64_t gp = S.g0 + lp;
        int64_t d = -1;
        int32_t term = -1, len = 0;
        bool kept = start;                        // a row is written for it
        if (start || bad) {
            d = tx_doc(T, S, gp);
            if (d >= 0 && bad) atomicOr(&flags[d], 1);
            if (start && d >= 0) {
                const int64_t end = tx_text_end(T, d, gp);
                if (ANALYZED) kept = tx_lookup_analyzed(T, V, A, rules, gp, end, term, len);
                else term = tx_lookup(T, V, gp, end, len);
                if (kept) atomicAdd(&n_tokens[d], 1);
            }
        }
        const uint64_t keeps = __ballot(kept);
        if (kept) {
            const int64_t at = row + __popcll(keeps & below);
            if (at < capacity) {
                tok_doc[at] = (int32_t)d;
                tok_term[at] = term;
                tok_off[at] = gp;
                tok_len[at] = len;
            }
        }
        unknown += __popcll(__ballot(kept && term < 0));
        row += __popcll(keeps);
    }
    if (lane == 0) unit_unknown[unit] = unknown;
}

// One wave per unit: its rows with term -1, in order, to the compacted list.
__global__ __launch_bounds__(TX_THREADS) void text_unknown(const int32_t* __restrict__ unit_off,
                                                           const int32_t* __restrict__ unk_off_of, int64_t n_units,
                                                           int64_t capacity, const int32_t* __restrict__ tok_term,
                                                           const int64_t* __restrict__ tok_off,
                                                           const int32_t* __restrict__ tok_len,
                                                           int64_t* __restrict__ unk_off, int32_t* __restrict__ unk_len) {
    const int64_t unit = (int64_t)blockIdx.x * TX_WAVES + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (unit >= n_units) return;
    int64_t a = unit_off[unit], b = unit_off[unit + 1];
    b = b < capacity ? b : capacity;
    int64_t out = unk_off_of[unit];
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (; a < b; a += WAVE) {
        const bool mine = a + lane < b && tok_term[a + lane] < 0;
        const uint64_t m = __ballot(mine);
        if (mine) {
            const int64_t at = out + __popcll(m & below);
            if (at < capacity) {
                unk_off[at] = tok_off[a + lane];
                unk_len[at] = tok_len[a + lane];
            }
        }
        out += __popcll(m);
    }
}

__global__ __launch_bounds__(TX_THREADS) void query_terms(const int32_t* __restrict__ tok_term,
                                                          const int32_t* __restrict__ row_of,   // [nq + 1]
                                                          const int32_t* __restrict__ n_total, int64_t capacity,
                                                          const int32_t* __restrict__ text_flags, int nq,
                                                          int32_t* __restrict__ out_terms, int32_t* __restrict__ n_distinct,
                                                          int32_t* __restrict__ out_flags) {
    __shared__ int32_t list_all[TX_WAVES][THR_BM25_MAX_TERMS + 1];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t q = (int64_t)blockIdx.x * TX_WAVES + wave;
    if (q >= nq) return;
    int32_t* list = list_all[wave];
    int64_t a = row_of[q], b = row_of[q + 1];
    int64_t limit = *n_total;
    limit = limit < capacity ? limit : capacity;
    a = a < limit ? a : limit;
    b = b < limit ? b : limit;
    int cnt = 0;
    bool unknown = false;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (; a < b; a += WAVE) {
        const bool have = a + lane < b;
        const int32_t t = have ? tok_term[a + lane] : -1;
        unknown = unknown || __ballot(have && t < 0) != 0;
        bool fresh = have && t >= 0;
        for (int j = 0; j < WAVE; ++j) {              // an earlier lane of this round with the same term
            const int32_t tj = __shfl(t, j, WAVE);
            if (j < lane && tj == t) fresh = false;
        }
        const int known = cnt < THR_BM25_MAX_TERMS + 1 ? cnt : THR_BM25_MAX_TERMS + 1;
        for (int j = 0; j < known; ++j)
            if (list[j] == t) fresh = false;
        const uint64_t m = __ballot(fresh);
        if (fresh) {
            const int at = cnt + __popcll(m & below);
            if (at < THR_BM25_MAX_TERMS + 1) list[at] = t;
        }
        cnt += __popcll(m);
        cnt = cnt < THR_BM25_MAX_TERMS + 1 ? cnt : THR_BM25_MAX_TERMS + 1;
        __builtin_amdgcn_wave_barrier();
    }
    if (lane < THR_BM25_MAX_TERMS)
        out_terms[q * THR_BM25_MAX_TERMS + lane] = lane < cnt ? list[lane] : -1;
    if (lane == 0) {
        n_distinct[q] = cnt;
        out_flags[q] = (text_flags[q] & 1) | (unknown ? 2 : 0) | (cnt > THR_BM25_MAX_TERMS ? 4 : 0);
    }
}

}  // namespace thr

using namespace thr;

static bool pow2(int64_t v) { return v > 0 && (v & (v - 1)) == 0; }

extern "C" size_t thr_vocab_table_bytes(int64_t capacity) {
    if (!pow2(capacity) || capacity < THR_VOCAB_MIN_SLOTS || capacity > THR_VOCAB_MAX_SLOTS) return 0;
    return (size_t)capacity * sizeof(VocabSlot);
}

extern "C" int thr_vocab_insert(void* slots, int64_t capacity, const uint8_t* term_bytes, const int64_t* term_ptr,
                                int64_t first_id, int64_t count, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!slots || !term_bytes || !term_ptr, THR_ERR_INVALID);
    THR_RETURN_IF(thr_vocab_table_bytes(capacity) == 0, THR_ERR_INVALID);
    THR_RETURN_IF(first_id < 0 || count < 1 || first_id > capacity / 2 || count > capacity / 2 - first_id,
                  THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)slots & 15) != 0 || ((uintptr_t)term_ptr & 7) != 0, THR_ERR_INVALID);
    hipLaunchKernelGGL(vocab_insert, dim3((unsigned)((count + TX_THREADS - 1) / TX_THREADS)), dim3(TX_THREADS), 0,
                       (hipStream_t)stream, (VocabSlot*)slots, (uint32_t)(capacity - 1), term_bytes, term_ptr,
                       (int32_t)first_id, (int32_t)count);
    return launch_status();
}

static bool text_shape_ok(int64_t n_texts, int64_t n_bytes) {
    return n_texts >= 1 && n_texts <= THR_TEXT_MAX_TEXTS && n_bytes >= 0 && n_bytes <= THR_TEXT_MAX_BYTES;
}

static int64_t text_slices(int64_t n_bytes) { return n_bytes > 0 ? (n_bytes + TX_SLICE - 1) / TX_SLICE : 1; }

struct TextPlan {
    int32_t* unit_off;       // [units + 1]: counts, then their exclusive scan
    int32_t* unit_unknown;   // [units + 1]: the same for the unknown tokens
    int64_t* tok_off;        // [capacity]
    int32_t* tok_len;        // [capacity]
};

static TextPlan text_plan(Arena& A, int64_t n_bytes, int64_t capacity) {
    TextPlan P;
    const size_t units = (size_t)text_slices(n_bytes) * TX_WAVES;
    P.unit_off = A.take<int32_t>(units + 1);
    P.unit_unknown = A.take<int32_t>(units + 1);
    P.tok_off = A.take<int64_t>((size_t)capacity);
    P.tok_len = A.take<int32_t>((size_t)capacity);
    return P;
}

extern "C" size_t thr_text_tokens_workspace_bytes(int64_t n_texts, int64_t n_bytes, int64_t token_capacity) {
    if (!text_shape_ok(n_texts, n_bytes) || token_capacity < 1 || token_capacity > THR_TEXT_MAX_BYTES) return 0;
    Arena A;
    text_plan(A, n_bytes, token_capacity);
    return A.total;
}

// thr_text_tokens' refusals and launches; ANALYZED: with the analysis ``A`` (checked by the caller).
template <bool ANALYZED>
static int text_tokens_run(const uint8_t* text_bytes, const int64_t* text_ptr, int64_t n_texts, int64_t n_bytes,
                           const uint32_t* table, const void* slots, int64_t capacity, const uint8_t* term_bytes,
                           const int64_t* term_ptr, int64_t n_vocab, const Analysis& An, int64_t token_capacity,
                           int32_t* tok_doc, int32_t* tok_term, int32_t* n_tokens, int32_t* flags, int32_t* n_total,
                           int64_t* unknown_off, int32_t* unknown_len, int32_t* n_unknown, void* workspace,
                           size_t workspace_bytes, thr_stream_t stream) {
    THR_RETURN_IF(!text_shape_ok(n_texts, n_bytes), THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(token_capacity < 1 || token_capacity > THR_TEXT_MAX_BYTES, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!text_bytes || !text_ptr || !table || !slots || !term_bytes || !term_ptr || !tok_doc || !tok_term ||
                      !n_tokens || !flags || !n_total || !unknown_off || !unknown_len || !n_unknown || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(thr_vocab_table_bytes(capacity) == 0 || n_vocab < 0 || n_vocab > capacity / 2, THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)text_bytes & 15) != 0 || ((uintptr_t)slots & 15) != 0, THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)text_ptr & 7) != 0 || ((uintptr_t)term_ptr & 7) != 0 || ((uintptr_t)unknown_off & 7) != 0 ||
                      ((uintptr_t)workspace & 7) != 0 || ((uintptr_t)table & 3) != 0,
                  THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_text_tokens_workspace_bytes(n_texts, n_bytes, token_capacity), THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    const TextPlan P = text_plan(A, n_bytes, token_capacity);
    const int64_t slices = text_slices(n_bytes), units = slices * TX_WAVES;
    hipError_t e = hipMemsetAsync(n_tokens, 0, sizeof(int32_t) * n_texts, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(flags, 0, sizeof(int32_t) * n_texts, st);
    if (e != hipSuccess) return (int)e;
    const TextArgs T = {text_bytes, text_ptr, n_texts, n_bytes, table};
    const Vocab V = {(const VocabSlot*)slots, (uint32_t)(capacity - 1), term_bytes, term_ptr, n_vocab};
    hipLaunchKernelGGL(text_count<ANALYZED>, dim3((unsigned)slices), dim3(TX_THREADS), 0, st, T, An, P.unit_off);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(text_scan, dim3(1), dim3(TX_SCAN_THREADS), 0, st, (const int32_t*)P.unit_off, units, P.unit_off,
                       n_total);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(text_emit<ANALYZED>, dim3((unsigned)slices), dim3(TX_THREADS), 0, st, T, V, An,
                       (const int32_t*)P.unit_off, token_capacity, tok_doc, tok_term, P.tok_off, P.tok_len, n_tokens, flags,
                       P.unit_unknown);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(text_scan, dim3(1), dim3(TX_SCAN_THREADS), 0, st, (const int32_t*)P.unit_unknown, units,
                       P.unit_unknown, n_unknown);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(text_unknown, dim3((unsigned)slices), dim3(TX_THREADS), 0, st, (const int32_t*)P.unit_off,
                       (const int32_t*)P.unit_unknown, units, token_capacity, (const int32_t*)tok_term,
                       (const int64_t*)P.tok_off, (const int32_t*)P.tok_len, unknown_off, unknown_len);
    return launch_status();
}

extern "C" int thr_text_tokens(const uint8_t* text_bytes, const int64_t* text_ptr, int64_t n_texts, int64_t n_bytes,
                               const uint32_t* table, const void* slots, int64_t capacity, const uint8_t* term_bytes,
                               const int64_t* term_ptr, int64_t n_vocab, int64_t token_capacity, int32_t* tok_doc,
                               int32_t* tok_term, int32_t* n_tokens, int32_t* flags, int32_t* n_total,
                               int64_t* unknown_off, int32_t* unknown_len, int32_t* n_unknown, void* workspace,
                               size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    return text_tokens_run<false>(text_bytes, text_ptr, n_texts, n_bytes, table, slots, capacity, term_bytes, term_ptr,
                                  n_vocab, Analysis{}, token_capacity, tok_doc, tok_term, n_tokens, flags, n_total,
                                  unknown_off, unknown_len, n_unknown, workspace, workspace_bytes, stream);
}

extern "C" size_t thr_text_tokens_analyzed_workspace_bytes(int64_t n_texts, int64_t n_bytes, int64_t token_capacity) {
    return thr_text_tokens_workspace_bytes(n_texts, n_bytes, token_capacity);
}

extern "C" int thr_text_tokens_analyzed(const uint8_t* text_bytes, const int64_t* text_ptr, int64_t n_texts,
                                        int64_t n_bytes, const uint32_t* table, const void* slots, int64_t capacity,
                                        const uint8_t* term_bytes, const int64_t* term_ptr, int64_t n_vocab,
                                        const void* stop_slots, int64_t stop_capacity, const uint8_t* stop_bytes,
                                        const int64_t* stop_ptr, int64_t n_stop, const int32_t* h_step_ptr, int n_steps,
                                        const void* rules, int64_t token_capacity, int32_t* tok_doc, int32_t* tok_term,
                                        int32_t* n_tokens, int32_t* flags, int32_t* n_total, int64_t* unknown_off,
                                        int32_t* unknown_len, int32_t* n_unknown, void* workspace, size_t workspace_bytes,
                                        thr_stream_t stream) {
    clear_status();
    Analysis A = {};
    // the rule table: the step pointers are HOST memory (five numbers at the most) and checked here
    THR_RETURN_IF(n_steps < 0 || n_steps > THR_STEM_MAX_STEPS, THR_ERR_INVALID);
    THR_RETURN_IF(n_steps > 0 && !h_step_ptr, THR_ERR_INVALID);
    A.n_steps = n_steps;
    for (int s = 0; s <= n_steps && n_steps > 0; ++s) {
        const int32_t v = h_step_ptr[s];
        THR_RETURN_IF(s == 0 ? v != 0 : v < A.step[s - 1], THR_ERR_INVALID);
        THR_RETURN_IF(v > THR_STEM_MAX_RULES, THR_ERR_INVALID);
        A.step[s] = v;
    }
    const int n_rules = A.step[n_steps];
    THR_RETURN_IF(n_rules > 0 && (!rules || ((uintptr_t)rules & 7) != 0), THR_ERR_INVALID);
    A.rules = (const uint32_t*)rules;
    // the stop set: capacity 0 with null pointers is no stop list, anything else a whole vocabulary
    if (stop_capacity == 0) {
        THR_RETURN_IF(stop_slots || stop_bytes || stop_ptr || n_stop != 0, THR_ERR_INVALID);
    } else {
        THR_RETURN_IF(!stop_slots || !stop_bytes || !stop_ptr, THR_ERR_INVALID);
        THR_RETURN_IF(thr_vocab_table_bytes(stop_capacity) == 0 || n_stop < 0 || n_stop > stop_capacity / 2,
                      THR_ERR_INVALID);
        THR_RETURN_IF(((uintptr_t)stop_slots & 15) != 0 || ((uintptr_t)stop_ptr & 7) != 0, THR_ERR_INVALID);
        A.stop = {(const VocabSlot*)stop_slots, (uint32_t)(stop_capacity - 1), stop_bytes, stop_ptr, n_stop};
    }
    return text_tokens_run<true>(text_bytes, text_ptr, n_texts, n_bytes, table, slots, capacity, term_bytes, term_ptr,
                                 n_vocab, A, token_capacity, tok_doc, tok_term, n_tokens, flags, n_total, unknown_off,
                                 unknown_len, n_unknown, workspace, workspace_bytes, stream);
}

extern "C" size_t thr_query_terms_workspace_bytes(int n_queries) {
    if (n_queries < 1 || n_queries > THR_TEXT_MAX_TEXTS) return 0;
    Arena A;
    A.take<int32_t>((size_t)n_queries + 1);
    return A.total;
}

extern "C" int thr_query_terms(const int32_t* tok_term, const int32_t* n_tokens, const int32_t* text_flags,
                               const int32_t* n_total, int64_t token_capacity, int n_queries, int32_t* out_terms,
                               int32_t* n_distinct, int32_t* out_flags, void* workspace, size_t workspace_bytes,
                               thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(n_queries < 1 || n_queries > THR_TEXT_MAX_TEXTS, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(token_capacity < 1 || token_capacity > THR_TEXT_MAX_BYTES, THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!tok_term || !n_tokens || !text_flags || !n_total || !out_terms || !n_distinct || !out_flags ||
                      !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)workspace & 3) != 0, THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_query_terms_workspace_bytes(n_queries), THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    int32_t* row_of = (int32_t*)workspace;
    hipLaunchKernelGGL(text_scan, dim3(1), dim3(TX_SCAN_THREADS), 0, st, n_tokens, (int64_t)n_queries, row_of,
                       (int32_t*)nullptr);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(query_terms, dim3((unsigned)((n_queries + TX_WAVES - 1) / TX_WAVES)), dim3(TX_THREADS), 0, st,
                       tok_term, (const int32_t*)row_of, n_total, token_capacity, text_flags, n_queries, out_terms,
                       n_distinct, out_flags);
    return launch_status();
}
