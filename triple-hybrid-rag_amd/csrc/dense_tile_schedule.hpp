// The bookkeeping of dense_scan_f16qs' whole-tile schedule (dense_scan_f16q.hpp), as constexpr
// functions the host can replay (tests/native/dense_tile_schedule_host_check.cpp): which tile goes
// into which buffer and when, which buffer a role reads, how many pieces it issues, what its
// counted wait leaves in flight and how many barriers it executes.  No device code, no HIP types.
//
// One interval per 32-row tile, one barrier per interval, a ring of nbuf(dim) whole-tile buffers.
// Tile j lives in buffer j % nbuf.  Barrier t publishes tile t (every issuing wave has waited for
// its own pieces of it) and retires tile t - 1 (both groups multiplied it in interval t - 1), so
// in interval t the buffer of tile t - 1 takes the pieces of tile t + nbuf - 1.
//
//     role        in interval t (after barrier t)
//     A           multiply tile t, then emit tile t            issues nothing, waits for nothing
//     B           emit tile t - 1, then multiply tile t        issues tile t + nbuf - 1 (all pieces)
//     padding A   nothing                                      as A
//     padding B   nothing                                      as B
//
// Only group B issues row pieces: its emit stores come FIRST in its interval, its pieces after
// them, so in the issue order that vmcnt counts a tile's stores are older than the pieces issued
// in the same interval (wait_leaves below).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define THR_TS_FN constexpr __host__ __device__ inline
#else
#define THR_TS_FN constexpr inline
#endif

namespace thr {
namespace tsched {

enum Role { ROLE_A = 0, ROLE_B = 1, ROLE_PAD_A = 2, ROLE_PAD_B = 3 };
constexpr int N_ROLES = 4;
constexpr int N_WAVES = 8, N_ISSUERS = 4;     // waves per block; waves 4-7 issue the row pieces
constexpr int LDS_BUDGET = 160 * 1024, MAX_BUF = 4;

THR_TS_FN Role role_of(int wave, bool padding) {
    return wave < N_WAVES - N_ISSUERS ? (padding ? ROLE_PAD_A : ROLE_A) : (padding ? ROLE_PAD_B : ROLE_B);
}
THR_TS_FN int pieces_per_tile(int dim) { return dim / 16; }            // 1 KiB each
THR_TS_FN int tile_bytes(int dim) { return pieces_per_tile(dim) * 1024; }
// tile buffers in the ring: 3 at dim 768 (144 KiB), 4 at dim 512 (128 KiB)
THR_TS_FN int nbuf(int dim) {
    return LDS_BUDGET / tile_bytes(dim) > MAX_BUF ? MAX_BUF : LDS_BUDGET / tile_bytes(dim);
}
THR_TS_FN bool issues(Role r) { return r == ROLE_B || r == ROLE_PAD_B; }
THR_TS_FN bool multiplies(Role r) { return r == ROLE_A || r == ROLE_B; }
THR_TS_FN bool emits_first(Role r) { return r == ROLE_B; }             // tile t - 1, before multiplying tile t
// pieces one wave of the role issues per tile
THR_TS_FN int pieces_issued(Role r, int dim) { return issues(r) ? pieces_per_tile(dim) / N_ISSUERS : 0; }
// piece p of issuing wave iw (0..3) -> piece of the tile
THR_TS_FN int piece_index(int iw, int p) { return iw + N_ISSUERS * p; }
// the k-step after whose MFMAs a multiplying issuer sends piece p: every other step from step 1,
// the first half of its multiply
THR_TS_FN int issue_step(int p) { return 1 + 2 * p; }

THR_TS_FN int buffer_of(int64_t tile, int dim) { return (int)(tile % nbuf(dim)); }
THR_TS_FN int next_buffer(int buf, int dim) { return buf + 1 == nbuf(dim) ? 0 : buf + 1; }
THR_TS_FN int prev_buffer(int buf, int dim) { return buf == 0 ? nbuf(dim) - 1 : buf - 1; }
// tiles requested before the first barrier: 0 .. prologue_tiles - 1, tile j into buffer j
THR_TS_FN int prologue_tiles(int dim) { return nbuf(dim) - 1; }
// the tile requested in interval t, into the buffer of tile t - 1
THR_TS_FN int64_t issue_tile(int64_t t, int dim) { return t + nbuf(dim) - 1; }
// its source: past the block's last tile the last one is requested again (never read), so that the
// number of pieces in flight at every wait is the same
THR_TS_FN int64_t source_tile(int64_t j, int64_t n_mine) { return j < n_mine ? j : n_mine - 1; }
// the tile a multiplying role reads in interval t
THR_TS_FN int64_t read_tile(Role, int64_t t) { return t; }
// s_waitcnt vmcnt(N) before barrier t: an issuer's operations, oldest first, are then
//     ... pieces(t) | stores(t-nbuf+2) pieces(t+1) | ... | stores(t-1) pieces(t+nbuf-2)
// (stores(i): the emit stores of interval i, which precede the pieces of tile i + nbuf - 1 issued
// in interval i).  Leaving the (nbuf - 2) * pieces youngest in flight therefore retires pieces(t)
// whatever the number of stores: a store is never younger than the pieces it would have to out-wait,
// it only makes the wait reach a little further (into pieces(t+1), requested an interval ago).
THR_TS_FN int wait_leaves(Role r, int dim) { return (nbuf(dim) - 2) * pieces_issued(r, dim); }
THR_TS_FN bool waits(Role r) { return issues(r); }
// barriers a role executes: one per tile of the block, for every role
THR_TS_FN int64_t barriers(Role, int64_t n_mine) { return n_mine; }

}  // namespace tsched
}  // namespace thr
