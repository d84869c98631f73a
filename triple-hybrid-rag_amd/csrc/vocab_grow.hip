// Numbering the new terms of a batch on the device: the step behind thr_text_tokens on the ingest side.
//
// thr_text_tokens leaves the tokens the vocabulary does not hold as a list of (byte offset, byte length) in
// text order.  The host restatement numbers them in a dict loop (GpuIndexClient.insert_children,
// TextSearch.text_rows' first.setdefault, index_build.lexical_rows): a token not seen before gets the next
// id, in order of first appearance.  Here the same numbering is count / scan / scatter over the list:
//
// vg_claim    one lane per occurrence u: lowers and hashes its token (tx_fnv_cp, as tx_lookup), masks the
//             hash, and probes a scratch table of 16-byte slots {uint64 hash, int32 INT_MAX - first, int32 id}
//             from the home slot with a 64-bit compare-and-swap on the hash word until it claims a slot or
//             meets its own hash.  It records slot[u] and folds u into the slot with one atomicMax of
//             INT_MAX - u (over zeroed memory: the minimum u wins).  The hash word is read only through the
//             CAS's return value; everything else of a slot is read in a later kernel.
// vg_verify   each occurrence compares its lowered characters with those of its slot's first occurrence: a
//             difference is two tokens under one (masked) hash -> THR_VOCAB_GROW_COLLISION.  The heads (u ==
//             first of its slot) put down 1 and their lowered byte length for the scan.
// vg_scan     exclusive scans of both (one workgroup, text_scan's scheme): the rank r of every head and where
//             its key begins; the totals, new_ptr's end and THR_VOCAB_GROW_OVERFLOW.
// vg_emit     heads write new_ptr[r], their lowered key bytes and their id n_vocab + r into the slot.
// vg_patch    every occurrence reads its id from its slot into unknown_term.
// vg_tok_*    optional: the rows of tok_term below 0 are, in row order, the list; count per unit, scan, patch.
//
// Integer atomics that commute (CAS on a hash word whose winner does not matter, max, or), kernel boundaries
// as the only ordering, no workgroup waits for another, nothing is read back: the same bits every run.
#include <limits.h>

#include "text_common.hpp"

namespace thr {

constexpr int VG_THREADS = 256;
constexpr int VG_WAVES = VG_THREADS / WAVE;
constexpr int VG_SCAN_THREADS = 1024;
constexpr int64_t VG_TOK_UNITS = 16384;        // waves of the tok_term patch at most (their counts are workspace)

struct GrowSlot {
    uint64_t hash;          // the masked hash; 0 = empty
    int32_t first_inv;      // INT_MAX - (the lowest occurrence that landed here)
    int32_t id;             // n_vocab + rank, written by the head
};
static_assert(sizeof(GrowSlot) == 16, "16-byte slots");

struct GrowIn {
    const uint8_t* bytes;
    const int64_t* ptr;         // [n_texts + 1]
    int64_t n_texts, n_bytes;
    const uint32_t* table;
    const int32_t* flags;       // [n_texts]
    const int64_t* unk_off;
    const int32_t* unk_len;
    const int32_t* n_unknown;
    int64_t capacity;           // of the list
};

__device__ __forceinline__ int64_t vg_count(const GrowIn& G) {
    const int64_t n = *G.n_unknown;
    return n < 0 ? 0 : n < G.capacity ? n : G.capacity;
}

// Occurrence u as a byte range inside [0, n_bytes) and inside its text; false: its text is flagged.
__device__ __forceinline__ bool vg_span(const GrowIn& G, int64_t u, int64_t& p, int64_t& end) {
    int64_t off = G.unk_off[u], len = G.unk_len[u];
    off = off < 0 ? 0 : off < G.n_bytes ? off : G.n_bytes;
    len = len < 0 ? 0 : len < G.n_bytes - off ? len : G.n_bytes - off;
    int64_t d = tx_upper(G.ptr, 0, G.n_texts, off) - 1;
    d = d < 0 ? 0 : d;
    const int64_t stop = G.ptr[d + 1];
    p = off;
    end = off + len;
    if (stop >= off && stop < end) end = stop;
    return !(G.flags[d] & THR_TEXT_EXCEPTIONAL);
}

// The lowered characters of [q, end), one per call; the walk ends at the range's end (or at a character that
// is no word character: never in a list thr_text_tokens left).
__device__ __forceinline__ bool vg_next(const GrowIn& G, int64_t& q, int64_t end, uint32_t& cp) {
    if (q >= end) return false;
    const int avail = end - q < 4 ? (int)(end - q) : 4;
    int len;
    const uint32_t e =
        tx_decode(G.bytes[q], avail > 1 ? G.bytes[q + 1] : 0, avail > 2 ? G.bytes[q + 2] : 0, avail, G.table, len);
    if ((e & TX_BAD) || !(e & TX_WORD)) {
        q = end;
        return false;
    }
    cp = e & 0xFFFF;
    q += len;
    return true;
}

__global__ __launch_bounds__(VG_THREADS) void vg_claim(GrowIn G, uint64_t hash_mask, GrowSlot* __restrict__ slots,
                                                       uint32_t mask, uint32_t* __restrict__ slot_of,
                                                       int32_t* __restrict__ low_len) {
    const int64_t u = (int64_t)blockIdx.x * VG_THREADS + threadIdx.x;
    if (u >= vg_count(G)) return;
    int64_t q, end;
    if (!vg_span(G, u, q, end)) {
        low_len[u] = -1;            // a flagged text's rows may hold anything: not numbered
        slot_of[u] = 0;
        return;
    }
    uint64_t h = TX_FNV_BASIS;
    int32_t bytes = 0;
    uint32_t cp;
    while (vg_next(G, q, end, cp)) {
        h = tx_fnv_cp(h, cp);
        bytes += cp < 0x80 ? 1 : cp < 0x800 ? 2 : 3;
    }
    h = tx_fnv_end(h) & hash_mask;
    h = h ? h : 1;
    uint32_t s = tx_home(h, mask);
    for (uint64_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {     // (load <= 1/2: a free one exists)
        const unsigned long long old =
            atomicCAS(reinterpret_cast<unsigned long long*>(&slots[s].hash), 0ull, (unsigned long long)h);
        if (old == 0ull || old == (unsigned long long)h) break;
    }
    slot_of[u] = s;
    low_len[u] = bytes;
    atomicMax(&slots[s].first_inv, INT_MAX - (int32_t)u);
}

__global__ __launch_bounds__(VG_THREADS) void vg_verify(GrowIn G, const GrowSlot* __restrict__ slots,
                                                        const uint32_t* __restrict__ slot_of,
                                                        const int32_t* __restrict__ low_len, int32_t* __restrict__ rank,
                                                        int64_t* __restrict__ byte_at, int32_t* __restrict__ status) {
    const int64_t u = (int64_t)blockIdx.x * VG_THREADS + threadIdx.x;
    if (u >= vg_count(G)) return;
    int32_t head = 0;
    if (low_len[u] >= 0) {
        const int64_t f = INT_MAX - slots[slot_of[u]].first_inv;
        head = f == u;
        if (!head) {
            int64_t qa, ea, qb, eb;
            vg_span(G, u, qa, ea);
            vg_span(G, f, qb, eb);
            bool same = low_len[f] == low_len[u];
            while (same) {
                uint32_t ca = 0, cb = 0;
                const bool ha = vg_next(G, qa, ea, ca), hb = vg_next(G, qb, eb, cb);
                if (!ha || !hb) {
                    same = ha == hb;
                    break;
                }
                same = ca == cb;
            }
            if (!same) atomicOr(status, THR_VOCAB_GROW_COLLISION);
        }
    }
    rank[u] = head;
    byte_at[u] = head ? low_len[u] : 0;
}

// a[i] = a[0] + .. + a[i - 1] for i in 0 .. n (n + 1 values), in place, by the whole workgroup -> a[n]
template <typename T>
__device__ __forceinline__ T vg_scan_in_place(T* a, int64_t n, T* tmp) {
    const int64_t per = (n + VG_SCAN_THREADS - 1) / VG_SCAN_THREADS;
    const int64_t lo = per * threadIdx.x < n ? per * threadIdx.x : n, hi = lo + per < n ? lo + per : n;
    T s = 0;
    for (int64_t i = lo; i < hi; ++i) s += a[i];
    tmp[threadIdx.x] = s;
    block_inclusive_scan<VG_SCAN_THREADS>(tmp);
    T run = tmp[threadIdx.x] - s;
    for (int64_t i = lo; i < hi; ++i) {
        const T v = a[i];
        a[i] = run;
        run += v;
    }
    const T total = tmp[VG_SCAN_THREADS - 1];
    if (threadIdx.x == 0) a[n] = total;
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(VG_SCAN_THREADS) void vg_scan(GrowIn G, int32_t* __restrict__ rank,
                                                           int64_t* __restrict__ byte_at, int64_t new_bytes_capacity,
                                                           int64_t* __restrict__ new_ptr, int32_t* __restrict__ n_new,
                                                           int64_t* __restrict__ n_new_bytes, int32_t* __restrict__ status) {
    __shared__ int64_t tmp[VG_SCAN_THREADS];
    const int64_t n = vg_count(G);
    const int32_t heads = vg_scan_in_place(rank, n, reinterpret_cast<int32_t*>(tmp));
    const int64_t bytes = vg_scan_in_place(byte_at, n, tmp);
    if (threadIdx.x == 0) {
        *n_new = heads;
        *n_new_bytes = bytes;
        new_ptr[heads] = bytes;         // (heads <= n <= the list's capacity: new_ptr holds capacity + 1)
        if (bytes > new_bytes_capacity) atomicOr(status, THR_VOCAB_GROW_OVERFLOW);
    }
}

__global__ __launch_bounds__(VG_THREADS) void vg_emit(GrowIn G, GrowSlot* __restrict__ slots,
                                                      const uint32_t* __restrict__ slot_of,
                                                      const int32_t* __restrict__ low_len, const int32_t* __restrict__ rank,
                                                      const int64_t* __restrict__ byte_at, int64_t n_vocab,
                                                      int64_t new_bytes_capacity, uint8_t* __restrict__ new_bytes,
                                                      int64_t* __restrict__ new_ptr) {
    const int64_t u = (int64_t)blockIdx.x * VG_THREADS + threadIdx.x;
    if (u >= vg_count(G) || low_len[u] < 0) return;
    GrowSlot& S = slots[slot_of[u]];
    if ((int64_t)(INT_MAX - S.first_inv) != u) return;
    const int32_t r = rank[u];
    S.id = (int32_t)(n_vocab + r);
    int64_t k = byte_at[u];
    new_ptr[r] = k;
    int64_t q, end;
    vg_span(G, u, q, end);
    uint32_t cp;
    while (vg_next(G, q, end, cp)) {
        uint8_t b[3];
        int nb;
        if (cp < 0x80) {
            b[0] = (uint8_t)cp;
            nb = 1;
        } else if (cp < 0x800) {
            b[0] = (uint8_t)(0xC0 | (cp >> 6));
            b[1] = (uint8_t)(0x80 | (cp & 63));
            nb = 2;
        } else {
            b[0] = (uint8_t)(0xE0 | (cp >> 12));
            b[1] = (uint8_t)(0x80 | ((cp >> 6) & 63));
            b[2] = (uint8_t)(0x80 | (cp & 63));
            nb = 3;
        }
        for (int j = 0; j < nb; ++j, ++k)
            if (k < new_bytes_capacity) new_bytes[k] = b[j];
    }
}

__global__ __launch_bounds__(VG_THREADS) void vg_patch(GrowIn G, const GrowSlot* __restrict__ slots,
                                                       const uint32_t* __restrict__ slot_of,
                                                       const int32_t* __restrict__ low_len,
                                                       int32_t* __restrict__ unknown_term) {
    const int64_t u = (int64_t)blockIdx.x * VG_THREADS + threadIdx.x;
    if (u >= vg_count(G)) return;
    unknown_term[u] = low_len[u] >= 0 ? slots[slot_of[u]].id : -1;
}

// One wave per unit of ``per`` (a multiple of 64) rows: its rows below 0.
__global__ __launch_bounds__(VG_THREADS) void vg_tok_count(const int32_t* __restrict__ tok_term,
                                                           const int32_t* __restrict__ n_total, int64_t token_capacity,
                                                           int64_t per, int64_t units, int32_t* __restrict__ unit_neg) {
    const int64_t unit = (int64_t)blockIdx.x * VG_WAVES + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (unit >= units) return;
    int64_t limit = *n_total;
    limit = limit < 0 ? 0 : limit < token_capacity ? limit : token_capacity;
    int64_t a = unit * per, b = a + per < limit ? a + per : limit;
    int c = 0;
    for (; a < b; a += WAVE) c += __popcll(__ballot(a + lane < b && tok_term[a + lane] < 0));
    if (lane == 0) unit_neg[unit] = c;
}

__global__ __launch_bounds__(VG_SCAN_THREADS) void vg_tok_scan(int32_t* __restrict__ unit_neg, int64_t units) {
    __shared__ int32_t tmp[VG_SCAN_THREADS];
    vg_scan_in_place(unit_neg, units, tmp);
}

__global__ __launch_bounds__(VG_THREADS) void vg_tok_patch(GrowIn G, int32_t* __restrict__ tok_term,
                                                           const int32_t* __restrict__ n_total, int64_t token_capacity,
                                                           int64_t per, int64_t units, const int32_t* __restrict__ unit_neg,
                                                           const int32_t* __restrict__ unknown_term) {
    const int64_t unit = (int64_t)blockIdx.x * VG_WAVES + threadIdx.x / WAVE;
    const int lane = threadIdx.x % WAVE;
    if (unit >= units) return;
    const int64_t n = vg_count(G);
    int64_t limit = *n_total;
    limit = limit < 0 ? 0 : limit < token_capacity ? limit : token_capacity;
    int64_t a = unit * per, b = a + per < limit ? a + per : limit;
    int64_t at = unit_neg[unit];
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (; a < b; a += WAVE) {
        const bool mine = a + lane < b && tok_term[a + lane] < 0;
        const uint64_t m = __ballot(mine);
        if (mine) {
            const int64_t j = at + __popcll(m & below);
            if (j < n) {
                const int32_t t = unknown_term[j];
                if (t >= 0) tok_term[a + lane] = t;
            }
        }
        at += __popcll(m);
    }
}

}  // namespace thr

using namespace thr;

static bool grow_capacity_ok(int64_t unknown_capacity) {
    return unknown_capacity >= 1 && unknown_capacity <= THR_TEXT_MAX_BYTES;
}

// the smallest power of two >= 2 * unknown_capacity (at least 16)
static uint64_t grow_slots(int64_t unknown_capacity) {
    uint64_t cap = 16;
    while (cap < 2 * (uint64_t)unknown_capacity) cap <<= 1;
    return cap;
}

struct GrowPlan {
    GrowSlot* slots;
    uint32_t* slot_of;      // [capacity]
    int32_t* low_len;       // [capacity]: bytes of the lowered token, -1: not numbered
    int32_t* rank;          // [capacity + 1]
    int64_t* byte_at;       // [capacity + 1]
    int32_t* unit_neg;      // [VG_TOK_UNITS + 1]
};

static GrowPlan grow_plan(Arena& A, int64_t unknown_capacity) {
    GrowPlan P;
    const size_t n = (size_t)unknown_capacity;
    P.slots = A.take<GrowSlot>((size_t)grow_slots(unknown_capacity));
    P.slot_of = A.take<uint32_t>(n);
    P.low_len = A.take<int32_t>(n);
    P.rank = A.take<int32_t>(n + 1);
    P.byte_at = A.take<int64_t>(n + 1);
    P.unit_neg = A.take<int32_t>((size_t)VG_TOK_UNITS + 1);
    return P;
}

extern "C" size_t thr_vocab_grow_workspace_bytes(int64_t unknown_capacity) {
    if (!grow_capacity_ok(unknown_capacity)) return 0;
    Arena A;
    grow_plan(A, unknown_capacity);
    return A.total;
}

extern "C" int thr_vocab_grow(const uint8_t* text_bytes, const int64_t* text_ptr, int64_t n_texts, int64_t n_bytes,
                              const uint32_t* table, const int32_t* flags, const int64_t* unknown_off,
                              const int32_t* unknown_len, const int32_t* n_unknown, int64_t unknown_capacity,
                              int64_t n_vocab, uint64_t hash_mask, int32_t* tok_term, const int32_t* n_total,
                              int64_t token_capacity, int32_t* unknown_term, uint8_t* new_bytes,
                              int64_t new_bytes_capacity, int64_t* new_ptr, int32_t* n_new, int64_t* n_new_bytes,
                              int32_t* status, void* workspace, size_t workspace_bytes, thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(n_texts < 1 || n_texts > THR_TEXT_MAX_TEXTS || n_bytes < 0 || n_bytes > THR_TEXT_MAX_BYTES,
                  THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!grow_capacity_ok(unknown_capacity), THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(tok_term && (token_capacity < 1 || token_capacity > THR_TEXT_MAX_BYTES), THR_ERR_UNSUPPORTED);
    THR_RETURN_IF(!text_bytes || !text_ptr || !table || !flags || !unknown_off || !unknown_len || !n_unknown ||
                      !unknown_term || !new_bytes || !new_ptr || !n_new || !n_new_bytes || !status || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(tok_term && !n_total, THR_ERR_INVALID);
    THR_RETURN_IF(n_vocab < 0 || n_vocab > (int64_t)INT32_MAX - unknown_capacity, THR_ERR_INVALID);
    THR_RETURN_IF(hash_mask == 0 || new_bytes_capacity < 0, THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)text_bytes & 15) != 0 || ((uintptr_t)workspace & 15) != 0, THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)text_ptr & 7) != 0 || ((uintptr_t)unknown_off & 7) != 0 || ((uintptr_t)new_ptr & 7) != 0 ||
                      ((uintptr_t)n_new_bytes & 7) != 0 || ((uintptr_t)table & 3) != 0,
                  THR_ERR_INVALID);
    THR_RETURN_IF(workspace_bytes < thr_vocab_grow_workspace_bytes(unknown_capacity), THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    const GrowPlan P = grow_plan(A, unknown_capacity);
    const uint64_t cap = grow_slots(unknown_capacity);
    hipError_t e = hipMemsetAsync(P.slots, 0, (size_t)cap * sizeof(GrowSlot), st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(status, 0, sizeof(int32_t), st);
    if (e != hipSuccess) return (int)e;
    const GrowIn G = {text_bytes, text_ptr, n_texts, n_bytes, table, flags, unknown_off, unknown_len, n_unknown,
                      unknown_capacity};
    const dim3 grid((unsigned)((unknown_capacity + VG_THREADS - 1) / VG_THREADS)), block(VG_THREADS);
    hipLaunchKernelGGL(vg_claim, grid, block, 0, st, G, hash_mask, P.slots, (uint32_t)(cap - 1), P.slot_of, P.low_len);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(vg_verify, grid, block, 0, st, G, (const GrowSlot*)P.slots, (const uint32_t*)P.slot_of,
                       (const int32_t*)P.low_len, P.rank, P.byte_at, status);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(vg_scan, dim3(1), dim3(VG_SCAN_THREADS), 0, st, G, P.rank, P.byte_at, new_bytes_capacity, new_ptr,
                       n_new, n_new_bytes, status);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(vg_emit, grid, block, 0, st, G, P.slots, (const uint32_t*)P.slot_of, (const int32_t*)P.low_len,
                       (const int32_t*)P.rank, (const int64_t*)P.byte_at, n_vocab, new_bytes_capacity, new_bytes, new_ptr);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(vg_patch, grid, block, 0, st, G, (const GrowSlot*)P.slots, (const uint32_t*)P.slot_of,
                       (const int32_t*)P.low_len, unknown_term);
    rc = launch_status();
    if (rc || !tok_term) return rc;
    // the rows of tok_term in at most VG_TOK_UNITS units of whole wave rounds
    int64_t per = (token_capacity + VG_TOK_UNITS - 1) / VG_TOK_UNITS;
    per = (per + WAVE - 1) / WAVE * WAVE;
    const int64_t units = (token_capacity + per - 1) / per;
    const dim3 tgrid((unsigned)((units + VG_WAVES - 1) / VG_WAVES));
    hipLaunchKernelGGL(vg_tok_count, tgrid, block, 0, st, (const int32_t*)tok_term, n_total, token_capacity, per, units,
                       P.unit_neg);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(vg_tok_scan, dim3(1), dim3(VG_SCAN_THREADS), 0, st, P.unit_neg, units);
    rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(vg_tok_patch, tgrid, block, 0, st, G, tok_term, n_total, token_capacity, per, units,
                       (const int32_t*)P.unit_neg, (const int32_t*)unknown_term);
    return launch_status();
}
