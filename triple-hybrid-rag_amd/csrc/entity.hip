// Seed entities of the graph channel from query keywords, for a whole batch, on the device.
//
// The reference resolves a query's keywords one at a time in SQL: rag_entities ... ILIKE '%kw%' LIMIT
// limit // len(keywords), first 5 keywords (src/voice_agent/rag2/graph_search.py:151-176); the host
// restatement is GpuIndexClient.find_entities.  Here the batch's DISTINCT lowered keywords (the NEEDLES)
// are matched against the lowered entity names in ONE pass over the name bytes, whatever their number.
//
// Two facts make this a byte-level device job:
//   1. Byte matching equals code-point matching.  Case folding stays on the host (str.lower() of names at
//      set-up, of keywords per call); on the lowered strings a code-point substring match is a byte
//      substring match of the UTF-8 encodings, because UTF-8 is self-synchronising: a valid needle can only
//      match at a character boundary.  The kernels compare bytes and know nothing about characters.
//   2. min(per, 16) matches per keyword are enough.  Only the first min(per, 16) matches of a keyword (in
//      ascending entity id) can reach the output: if the earlier keywords contributed m < 16 entities, at
//      most m of this keyword's first 16 matches are duplicates, so the 16 - m new ones the output still
//      has room for are among them.  Pass 1 therefore keeps, per needle, its 16 smallest matching ids.
//
// Name store: name_bytes = the names' UTF-8, each followed by ONE 0xFF separator (a byte UTF-8 never
// holds: no needle straddles two names, a match ends inside its name for free), name_ptr int64 [E + 1]
// (name_ptr[0] = 0; name e is [name_ptr[e], name_ptr[e + 1] - 1)), and behind name_ptr[E] at least
// THR_ENTITY_MAX_NEEDLE further 0xFF bytes, so that a window read at the last position stays inside the
// allocation.
//
// entity_table    one thread per needle: its 16 best slots := INT32_MAX, and the needle into an
//                 open-addressed hash table in global memory keyed by (min(len, 3), its first min(len, 3)
//                 bytes); a slot is (key, first needle), the needles of one key are a chain (rec[n] = next,
//                 length).  A 64 Kbit filter of the keys' hashes goes with it.  Needles of length 0 (they
//                 match every entity: pass 2 knows), above THR_ENTITY_MAX_NEEDLE or holding 0xFF are left
//                 out: they match nothing here.
// entity_scan     pass 1.  A workgroup owns a run of consecutive EN_SLICE-byte slices; a slice and a halo of
//                 THR_ENTITY_MAX_NEEDLE bytes are staged in LDS with the filter.  A lane takes a text position,
//                 forms the 1-, 2- and 3-byte keys there, tests each against the filter (LDS) and only on a
//                 set bit probes the table (L2), walks the key's chain and verifies the needle's remaining
//                 bytes against the LDS window.  The work per position does not depend on the needle count
//                 (beyond the filter's fill), so the pass costs one read of the store plus the verifications.
//                 The entity of a position is the number of separators in front of it: one binary search per
//                 workgroup, then counted (ballots) as the slices go by.
//                 A match inserts its entity into best[needle][0..16) by walking the slots with
//                 old = atomicMin(slot, v), stopping at old == v and carrying max(old, v): the operations
//                 commute, so the final content is the 16 smallest distinct ids whatever the interleaving --
//                 the same bits every run, and no workgroup waits for another.  A plain load in front of each
//                 atomic (and of slot 15 before anything else) rejects most matches: slot values only fall, so
//                 a stale value is only ever larger than the current one and can cost an atomic, never lose one.
//                 A wave meets its entities in ascending order (its quarter of each slice, the slices in
//                 order), so a needle whose slot 15 is below the FIRST entity of the wave's current round is
//                 rejected for every lane of that round and for the rest of the wave's run: a bit per wave and
//                 needle in LDS (the first EN_DEAD_BITS needles) remembers that and spares the look at slot 15.
//                 Launched three times, over the first 8 slices, the next 128 and the rest: when every
//                 workgroup starts at once, slot 15 of a needle found in most names is still INT32_MAX for all
//                 of them and each sends its first matches down the same 16 slots; after the small stages
//                 such a needle is full before the wide one starts, and a needle that is not is rare enough
//                 for the burst to be small.  The stages order work by kernel boundaries: nobody waits.
// entity_resolve  pass 2, one thread per query: its needles in order, from each the first min(per, 16)
//                 entries of best, those already present skipped, until 16 -> seeds (-1 padded), counts.
#include "thr_common.hpp"

namespace thr {

constexpr int EN_THREADS = 256;
constexpr int EN_WAVES = EN_THREADS / WAVE;
constexpr int EN_SLICE = THR_ENTITY_SLICE_BYTES;       // text positions per staged slice
constexpr int EN_HALO = THR_ENTITY_MAX_NEEDLE;         // bytes staged behind it (a window is at most this long)
constexpr int EN_WSLICE = EN_SLICE / EN_WAVES;         // consecutive positions per wave
constexpr int EN_ROUNDS = EN_WSLICE / WAVE;
constexpr int EN_BEST = THR_GRAPH_MAX_SEEDS;           // ids kept per needle
constexpr int EN_FILTER_BITS = 1 << 16;
constexpr int EN_FILTER_WORDS = EN_FILTER_BITS / 32;
constexpr uint32_t EN_EMPTY = 0xFFFFFFFFu;             // (a key's top byte is 1, 2 or 3)
constexpr int EN_MIN_SLOTS = 1024;
constexpr int EN_DEAD_BITS = 1 << 14;                  // needles whose rejection a wave remembers (2 KiB of LDS each)
constexpr int EN_STAGE_A = 8, EN_STAGE_B = 128;        // slices of the two small stages in front of the wide one
static_assert(EN_SLICE % (EN_THREADS * 16) == 0 && EN_HALO % 16 == 0, "slices are staged in 16-byte pieces");

__device__ __forceinline__ uint32_t en_slot_hash(uint32_t key) { return key * 2654435761u; }
__device__ __forceinline__ uint32_t en_filter_bit(uint32_t key) { return (key * 0x9E3779B1u) >> 16; }

__global__ __launch_bounds__(EN_THREADS) void entity_table(const uint8_t* __restrict__ needles,
                                                           const int32_t* __restrict__ needle_len, int M,
                                                           uint32_t* __restrict__ filter, uint32_t* __restrict__ slots,
                                                           int log_slots, int32_t* __restrict__ rec,
                                                           int32_t* __restrict__ best) {
    const int n = blockIdx.x * EN_THREADS + threadIdx.x;
    if (n >= M) return;
#pragma unroll
    for (int i = 0; i < EN_BEST; ++i) best[(int64_t)n * EN_BEST + i] = INT32_MAX;
    rec[2 * n] = -1;        // next
    rec[2 * n + 1] = 0;     // length (0: not in the table)
    const int L = needle_len[n];
    if (L < 1 || L > THR_ENTITY_MAX_NEEDLE) return;
    const uint8_t* nd = needles + (int64_t)n * THR_ENTITY_MAX_NEEDLE;
    for (int i = 0; i < L; ++i)
        if (nd[i] == 0xFF) return;
    const int kl = L < 3 ? L : 3;
    uint32_t key = (uint32_t)kl << 24;
    for (int i = 0; i < kl; ++i) key |= (uint32_t)nd[i] << (8 * i);
    const uint32_t fb = en_filter_bit(key);
    atomicOr(&filter[fb >> 5], 1u << (fb & 31));
    const uint32_t mask = (1u << log_slots) - 1;
    uint32_t s = en_slot_hash(key) >> (32 - log_slots);
    for (uint32_t probe = 0; probe <= mask; ++probe, s = (s + 1) & mask) {   // (slots >= 2 M: a free one exists)
        const uint32_t old = atomicCAS(&slots[2 * s], EN_EMPTY, key);
        if (old == EN_EMPTY || old == key) {
            rec[2 * n + 1] = L;
            rec[2 * n] = (int32_t)atomicExch(&slots[2 * s + 1], (uint32_t)n);   // (chain order varies from run to run; no result depends on it)
            return;
        }
    }
}

struct EntityTable {
    const uint32_t* needles;     // [M, THR_ENTITY_MAX_NEEDLE / 4]: the needle bytes, a dword at a time
    const uint2* slots;          // (key, first needle of the key or -1)
    const int2* rec;             // per needle (next of its chain or -1, length)
    int32_t* best;
    int M, log_slots;
};

__device__ __forceinline__ int32_t en_peek(const int32_t* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// e into the 16 smallest distinct ids of one needle (see the head of the file).  All 16 slots are looked at
// first, in one go (independent loads: one round trip, not sixteen dependent ones); the looks may be stale by
// the time they are used, which only ever makes them too large.
__device__ __forceinline__ void en_insert(int32_t* slots, int32_t e) {
    int32_t cur[EN_BEST];    // (constant indices: registers)
#pragma unroll
    for (int i = 0; i < EN_BEST; ++i) cur[i] = en_peek(&slots[i]);
    int32_t v = e;
#pragma unroll
    for (int i = 0; i < EN_BEST; ++i) {
        if (cur[i] == v) return;
        if (cur[i] < v) continue;     // (it only falls: the atomic would change nothing and hand v on)
        const int32_t old = atomicMin(&slots[i], v);
        if (old == v) return;
        v = old > v ? old : v;
        if (v == INT32_MAX) return;
    }
}

// The 4 text bytes at byte offset o of the staged slice (any alignment): two aligned LDS dwords.
__device__ __forceinline__ uint32_t en_text4(const uint8_t* text, int o) {
    const uint32_t* w = reinterpret_cast<const uint32_t*>(text + (o & ~3));
    return (uint32_t)((((uint64_t)w[1] << 32) | w[0]) >> (8 * (o & 3)));
}

// The needles whose key is ``key``, at the text position lp of the staged slice, whose name is ent.
// dead: this wave's remembered rejections; round_min: the entity of the round's first lane (<= ent).
__device__ __forceinline__ void en_lookup(const EntityTable& T, const uint32_t* filter, uint32_t* dead, uint32_t key,
                                          const uint8_t* text, int lp, int32_t ent, int32_t round_min) {
    const uint32_t fb = en_filter_bit(key);
    if (!((filter[fb >> 5] >> (fb & 31)) & 1u)) return;
    const uint32_t mask = (1u << T.log_slots) - 1;
    uint32_t s = en_slot_hash(key) >> (32 - T.log_slots);
    uint32_t probe = 0;
    uint2 slot;
    for (;; ++probe, s = (s + 1) & mask) {
        slot = T.slots[s];
        if (slot.x == EN_EMPTY || probe > mask) return;
        if (slot.x == key) break;
    }
    int32_t n = (int32_t)slot.y;
    for (int walked = 0; n >= 0 && n < T.M && walked < T.M; ++walked) {
        const int2 r = T.rec[n];
        const int32_t cur = n;
        n = r.x;
        const bool remembered = cur < EN_DEAD_BITS;
        if (remembered && ((dead[cur >> 5] >> (cur & 31)) & 1u)) continue;
        int32_t* slots = T.best + (int64_t)cur * EN_BEST;
        const int32_t b15 = en_peek(&slots[EN_BEST - 1]);
        if (ent >= b15) {   // (equal: it is in the list already)
            // every entity this wave has in hand or will meet is above the slot, and the slot only falls
            if (remembered && round_min > b15) atomicOr(&dead[cur >> 5], 1u << (cur & 31));
            continue;
        }
        const int L = r.y;
        const uint32_t* nd = T.needles + (int64_t)cur * (THR_ENTITY_MAX_NEEDLE / 4);
        bool same = true;
        // a separator in the window differs from every needle byte, so a match never runs past the end
        // of its name (the key's bytes are compared again: whole dwords)
        for (int i = 0; i < L && same; i += 4) {
            const uint32_t m = L - i >= 4 ? ~0u : (1u << (8 * (L - i))) - 1;
            same = ((en_text4(text, lp + i) ^ nd[i >> 2]) & m) == 0;
        }
        if (same) en_insert(slots, ent);
    }
}

__global__ __launch_bounds__(EN_THREADS) void entity_scan(const uint8_t* __restrict__ name_bytes,
                                                          const int64_t* __restrict__ name_ptr, int64_t E,
                                                          const uint32_t* __restrict__ g_filter, EntityTable T,
                                                          int64_t stage_lo, int64_t stage_hi) {
    __shared__ __attribute__((aligned(16))) uint8_t text[EN_SLICE + EN_HALO + 16];   // (a window's last dword pair)
    __shared__ uint32_t filter[EN_FILTER_WORDS];
    __shared__ uint32_t dead_all[EN_WAVES][EN_DEAD_BITS / 32];
    __shared__ int wave_seps[EN_WAVES];
    const int wave = threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    const int64_t total = name_ptr[E];                   // bytes of names and separators
    const int64_t readable = total + EN_HALO;            // the caller's padding
    const int64_t n_slices = (total + EN_SLICE - 1) / EN_SLICE;
    const int64_t lo_s = stage_lo < n_slices ? stage_lo : n_slices;      // this launch's slices
    const int64_t hi_s = stage_hi < n_slices ? stage_hi : n_slices;
    const int64_t per_block = (hi_s - lo_s + gridDim.x - 1) / gridDim.x;
    const int64_t first = lo_s + per_block * blockIdx.x;
    const int64_t last = first + per_block < hi_s ? first + per_block : hi_s;
    if (first >= last) return;
    for (int i = threadIdx.x; i < EN_FILTER_WORDS; i += EN_THREADS) filter[i] = g_filter[i];
    for (int i = threadIdx.x; i < EN_WAVES * EN_DEAD_BITS / 32; i += EN_THREADS) (&dead_all[0][0])[i] = 0;
    uint32_t* dead = dead_all[threadIdx.x / WAVE];
    if (threadIdx.x < 4) reinterpret_cast<uint32_t*>(text + EN_SLICE + EN_HALO)[threadIdx.x] = ~0u;
    // names that end in front of the first slice = separators in front of it: the first e with
    // name_ptr[e + 1] > first * EN_SLICE
    int64_t lo = 0, hi = E;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (name_ptr[mid + 1] <= first * EN_SLICE) lo = mid + 1; else hi = mid;
    }
    int64_t ent0 = lo;
    const uint64_t below = ((uint64_t)1 << lane) - 1;
    for (int64_t sl = first; sl < last; ++sl) {
        const int64_t g0 = sl * EN_SLICE;
        __syncthreads();   // (the previous slice has been read)
        for (int i = threadIdx.x * 16; i < EN_SLICE + EN_HALO; i += EN_THREADS * 16) {
            uint4 v = make_uint4(~0u, ~0u, ~0u, ~0u);    // behind the padding: separators
            if (g0 + i + 16 <= readable) {
                v = *reinterpret_cast<const uint4*>(name_bytes + g0 + i);
            } else {
                uint8_t* b = reinterpret_cast<uint8_t*>(&v);
                for (int j = 0; j < 16; ++j)
                    if (g0 + i + j < readable) b[j] = name_bytes[g0 + i + j];
            }
            *reinterpret_cast<uint4*>(text + i) = v;
        }
        __syncthreads();
        // separators of each wave's positions (lane l: 32 consecutive bytes of them)
        {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(text + wave * EN_WSLICE + lane * (EN_WSLICE / WAVE));
            int c = 0;
#pragma unroll
            for (int j = 0; j < EN_WSLICE / WAVE / 4; ++j) {
                const uint32_t z = ~w[j];    // a zero byte of z is a separator
                c += __popc(~(((z & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | z) & 0x80808080u);
            }
#pragma unroll
            for (int o = WAVE / 2; o > 0; o >>= 1) c += __shfl_xor(c, o, WAVE);
            if (lane == 0) wave_seps[wave] = c;
        }
        __syncthreads();
        int64_t run = ent0;
        int all = 0;
#pragma unroll
        for (int w = 0; w < EN_WAVES; ++w) {
            if (w < wave) run += wave_seps[w];
            all += wave_seps[w];
        }
        ent0 += all;
#pragma unroll 1
        for (int r = 0; r < EN_ROUNDS; ++r) {
            const int lp = wave * EN_WSLICE + r * WAVE + lane;
            const uint32_t* w = reinterpret_cast<const uint32_t*>(text + (lp & ~3));
            const uint64_t win = (((uint64_t)w[1] << 32) | w[0]) >> (8 * (lp & 3));
            const uint32_t b0 = win & 0xFF, b1 = (win >> 8) & 0xFF, b2 = (win >> 16) & 0xFF;
            const uint64_t seps = __ballot(b0 == 0xFF);
            const int64_t ent = run + __popcll(seps & below);
            const int32_t round_min = (int32_t)(run < INT32_MAX ? run : INT32_MAX);
            run += __popcll(seps);
            if (b0 == 0xFF || g0 + lp >= total || ent >= E) continue;
            en_lookup(T, filter, dead, (1u << 24) | b0, text, lp, (int32_t)ent, round_min);
            if (b1 == 0xFF) continue;
            en_lookup(T, filter, dead, (2u << 24) | (b1 << 8) | b0, text, lp, (int32_t)ent, round_min);
            if (b2 == 0xFF) continue;
            en_lookup(T, filter, dead, (3u << 24) | (b2 << 16) | (b1 << 8) | b0, text, lp, (int32_t)ent, round_min);
        }
    }
}

__global__ __launch_bounds__(EN_THREADS) void entity_resolve(const int32_t* __restrict__ needle_len, int M, int64_t E,
                                                             const int32_t* __restrict__ best,
                                                             const int32_t* __restrict__ query_needles,
                                                             const int32_t* __restrict__ query_per, int nq,
                                                             int32_t* __restrict__ seeds, int32_t* __restrict__ counts) {
    const int q = blockIdx.x * EN_THREADS + threadIdx.x;
    if (q >= nq) return;
    int32_t out[EN_BEST];    // (every index below is a compile-time constant: registers)
#pragma unroll
    for (int c = 0; c < EN_BEST; ++c) out[c] = -1;
    int cnt = 0;
    int per = query_per[q];
    per = per < 0 ? 0 : per > EN_BEST ? EN_BEST : per;   // fact 2 of the head of the file
    for (int j = 0; j < THR_ENTITY_MAX_KEYWORDS && cnt < EN_BEST; ++j) {
        const int n = query_needles[(int64_t)q * THR_ENTITY_MAX_KEYWORDS + j];
        if (n < 0 || n >= M) continue;
        const bool every = needle_len[n] == 0;           // the empty needle: entities 0, 1, 2, ...
        for (int i = 0; i < per && cnt < EN_BEST; ++i) {
            const int32_t e = every ? (i < E ? i : INT32_MAX) : best[(int64_t)n * EN_BEST + i];
            if (e == INT32_MAX) break;
            bool dup = false;
#pragma unroll
            for (int c = 0; c < EN_BEST; ++c) dup = dup || out[c] == e;   // (free slots hold -1, e >= 0)
            if (dup) continue;
#pragma unroll
            for (int c = 0; c < EN_BEST; ++c)
                if (c == cnt) out[c] = e;
            ++cnt;
        }
    }
#pragma unroll
    for (int c = 0; c < EN_BEST; ++c) seeds[(int64_t)q * EN_BEST + c] = out[c];
    counts[q] = cnt;
}

}  // namespace thr

using namespace thr;

static int entity_log_slots(int n_needles) {
    int lg = 10;
    while (((int64_t)1 << lg) < 2 * (int64_t)n_needles) ++lg;
    return lg;
}
static_assert((1 << 10) == EN_MIN_SLOTS, "entity_log_slots starts at the smallest table");

struct EntityPlan {
    uint32_t* filter;
    uint32_t* slots;     // (key, head) pairs
    int32_t* rec;        // (next, length) pairs
    int32_t* best;
    size_t slot_bytes;   // set to 0xFF: keys EN_EMPTY, heads -1
};

static EntityPlan entity_plan(Arena& A, int n_needles) {
    EntityPlan P;
    const size_t slots = (size_t)1 << entity_log_slots(n_needles);
    P.filter = A.take<uint32_t>(EN_FILTER_WORDS);
    P.slot_bytes = 2 * slots * sizeof(uint32_t);
    P.slots = A.take<uint32_t>(2 * slots);
    P.rec = A.take<int32_t>(2 * (size_t)n_needles);
    P.best = A.take<int32_t>((size_t)n_needles * EN_BEST);
    return P;
}

static bool entity_shape_ok(int64_t n_entities, int n_needles, int n_queries) {
    return n_entities > 0 && n_entities <= INT32_MAX && n_queries >= 1 && n_queries <= THR_ENTITY_MAX_QUERIES &&
           n_needles >= 1 && (int64_t)n_needles <= (int64_t)THR_ENTITY_MAX_KEYWORDS * n_queries;
}

extern "C" size_t thr_entity_match_workspace_bytes(int64_t n_entities, int n_needles, int n_queries) {
    if (!entity_shape_ok(n_entities, n_needles, n_queries)) return 0;
    Arena A;
    entity_plan(A, n_needles);
    return A.total;
}

extern "C" int thr_entity_match(const uint8_t* name_bytes, const int64_t* name_ptr, int64_t n_entities,
                                const uint8_t* needles, const int32_t* needle_len, int n_needles,
                                const int32_t* query_needles, const int32_t* query_per, int n_queries,
                                int32_t* seeds, int32_t* counts, void* workspace, size_t workspace_bytes,
                                thr_stream_t stream) {
    clear_status();
    THR_RETURN_IF(!name_bytes || !name_ptr || !needles || !needle_len || !query_needles || !query_per || !seeds ||
                      !counts || !workspace,
                  THR_ERR_INVALID);
    THR_RETURN_IF(!entity_shape_ok(n_entities, n_needles, n_queries), THR_ERR_INVALID);
    THR_RETURN_IF(((uintptr_t)name_bytes & 15) != 0, THR_ERR_INVALID);   // slices are read 16 bytes at a time,
    THR_RETURN_IF(((uintptr_t)needles & 3) != 0, THR_ERR_INVALID);       // needles 4,
    THR_RETURN_IF(((uintptr_t)workspace & 7) != 0, THR_ERR_INVALID);     // the table's slots and records 8
    THR_RETURN_IF(workspace_bytes < thr_entity_match_workspace_bytes(n_entities, n_needles, n_queries),
                  THR_ERR_WORKSPACE);
    hipStream_t st = (hipStream_t)stream;
    Arena A;
    A.base = (char*)workspace;
    const EntityPlan P = entity_plan(A, n_needles);
    const int log_slots = entity_log_slots(n_needles);
    hipError_t e = hipMemsetAsync(P.filter, 0, sizeof(uint32_t) * EN_FILTER_WORDS, st);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(P.slots, 0xFF, P.slot_bytes, st);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(entity_table, dim3((unsigned)((n_needles + EN_THREADS - 1) / EN_THREADS)), dim3(EN_THREADS), 0,
                       st, needles, needle_len, n_needles, P.filter, P.slots, log_slots, P.rec, P.best);
    int rc = launch_status();
    if (rc) return rc;
    EntityTable T = {reinterpret_cast<const uint32_t*>(needles), reinterpret_cast<const uint2*>(P.slots),
                     reinterpret_cast<const int2*>(P.rec), P.best, n_needles, log_slots};
    // the store's byte count is on the device (name_ptr[n_entities]) and nothing is read back: grids of a
    // fixed size, each workgroup a run of consecutive slices of its stage (none: it returns at once)
    const int64_t stage[4] = {0, EN_STAGE_A, EN_STAGE_A + EN_STAGE_B, INT64_MAX};
    const unsigned grid[3] = {EN_STAGE_A, EN_STAGE_B, (unsigned)(num_cus() * 8)};
    for (int g = 0; g < 3; ++g) {
        hipLaunchKernelGGL(entity_scan, dim3(grid[g]), dim3(EN_THREADS), 0, st, name_bytes, name_ptr, n_entities,
                           (const uint32_t*)P.filter, T, stage[g], stage[g + 1]);
        rc = launch_status();
        if (rc) return rc;
    }
    hipLaunchKernelGGL(entity_resolve, dim3((unsigned)((n_queries + EN_THREADS - 1) / EN_THREADS)), dim3(EN_THREADS),
                       0, st, needle_len, n_needles, n_entities, (const int32_t*)P.best, query_needles, query_per,
                       n_queries, seeds, counts);
    return launch_status();
}
