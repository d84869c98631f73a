// Host replay of dense_scan_f16qs' whole-tile schedule (csrc/dense_tile_schedule.hpp): the eight
// waves of a block, every mix of working and padding waves, n_mine = 0 .. 9 tiles, dims 512 and
// 768, 0 / 1 / 16 emit stores per interval.  Each wave runs the steps the kernel runs, built from
// the same tsched:: functions; the replay keeps a wave's vmcnt queue (issue order, retired oldest
// first) and the state of every 1 KiB piece slot of the LDS ring, and asserts
//   * every role executes the same number of barriers,
//   * every piece a wave reads was issued, waited for by its issuer and published by a barrier,
//   * no buffer is rewritten between its publication and the barrier after its last reader, nor
//     while a request into it is still in flight, nor in the interval in which it is read,
//   * what a counted wait leaves in flight never includes a piece of the tile being published.
// Built with ASan + UBSan by tests/test_dense_tile_schedule_host.py and run on the CPU.
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <vector>

#include "../../triple-hybrid-rag_amd/csrc/dense_tile_schedule.hpp"

namespace ts = thr::tsched;

#define CHECK(cond, ...)                                                   \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "FAILED %s (line %d): ", #cond, __LINE__); \
            std::fprintf(stderr, __VA_ARGS__);                             \
            std::fprintf(stderr, "\n");                                    \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

struct Op {          // one entry of a wave's vmcnt queue
    bool piece;      // a row piece (LDS-DMA) or an emit store
    int64_t tile;    // the block's j-th tile, as requested (not clamped)
    int buf, index;  // ring buffer and piece of the tile
};
struct Slot {        // one 1 KiB piece slot of the ring
    int64_t tile = -1, src = -1;   // requested tile and the tile its bytes come from
    bool landed = false;           // its issuer has waited for it
    int64_t published = -1;        // the barrier that published it (-1: not yet)
    int64_t last_read = -1;        // the last interval in which a wave read it
};
struct Wave {
    ts::Role role;
    int iw;                      // place among the issuers
    std::deque<Op> vm;           // in flight, oldest first
    int buf = 0, ibuf = 0;       // the kernel's running buffer counters
    int64_t barriers = 0, issued = 0, reads = 0;
};

struct Block {
    int dim, nbuf, ks, stores;
    int64_t n_mine;
    std::vector<Slot> slot;      // [nbuf][ks]
    std::vector<Wave> wave;
    std::vector<int> read_in, written_in;   // per buffer: read / written in the current interval

    Slot& at(int buf, int index) { return slot[(size_t)buf * ks + index]; }

    void issue(Wave& w, int64_t tile, int buf, int64_t t_now) {
        CHECK(buf >= 0 && buf < nbuf, "buffer %d", buf);
        CHECK(buf == ts::buffer_of(tile, dim), "tile %lld goes into buffer %d, not %d", (long long)tile,
              ts::buffer_of(tile, dim), buf);
        for (int p = 0; p < ts::pieces_issued(w.role, dim); ++p) {
            const int index = ts::piece_index(w.iw, p);
            CHECK(index >= 0 && index < ks, "piece %d", index);
            Slot& s = at(buf, index);
            if (s.tile >= 0) {
                CHECK(s.landed, "request into buffer %d while tile %lld is still landing there", buf, (long long)s.tile);
                // published at barrier s.tile (earlier where emit stores made a wait reach further),
                // read in interval s.tile: free after barrier s.tile + 1
                if (s.tile < n_mine) {
                    CHECK(s.published >= 0 && s.published <= s.tile, "tile %lld rewritten before it was published",
                          (long long)s.tile);
                    CHECK(t_now >= s.tile + 1, "tile %lld rewritten in interval %lld, before the barrier after its readers",
                          (long long)s.tile, (long long)t_now);
                    CHECK(s.last_read <= t_now - 1, "tile %lld read in interval %lld, rewritten in %lld", (long long)s.tile,
                          (long long)s.last_read, (long long)t_now);
                }
            }
            s = Slot();
            s.tile = tile;
            s.src = ts::source_tile(tile, n_mine);
            CHECK(s.src >= 0 && s.src < n_mine && (tile >= n_mine || s.src == tile), "source of tile %lld", (long long)tile);
            w.vm.push_back(Op{true, tile, buf, index});
            ++w.issued;
        }
        if (t_now >= 0) written_in[buf] = 1;
    }
    // s_waitcnt vmcnt(leave): retire, oldest first, until `leave` operations are in flight
    void wait(Wave& w, int leave, int64_t publishing) {
        while ((int)w.vm.size() > leave) {
            const Op op = w.vm.front();
            w.vm.pop_front();
            if (op.piece) at(op.buf, op.index).landed = true;
        }
        for (const Op& op : w.vm)
            CHECK(!(op.piece && op.tile == publishing), "the wait before barrier %lld leaves a piece of tile %lld in flight",
                  (long long)publishing, (long long)publishing);
    }
    void read(Wave& w, int64_t t) {
        const int64_t tile = ts::read_tile(w.role, t);
        CHECK(tile >= 0 && tile < n_mine, "read of tile %lld", (long long)tile);
        CHECK(w.buf == ts::buffer_of(tile, dim), "the running buffer of tile %lld", (long long)tile);
        for (int index = 0; index < ks; ++index) {
            Slot& s = at(w.buf, index);
            CHECK(s.tile == tile && s.src == tile, "buffer %d piece %d holds tile %lld, not %lld", w.buf, index,
                  (long long)s.tile, (long long)tile);
            CHECK(s.landed, "tile %lld piece %d read before its issuer waited for it", (long long)tile, index);
            CHECK(s.published >= 0 && s.published <= t, "tile %lld piece %d read before a barrier published it",
                  (long long)tile, index);
            s.last_read = t;
        }
        read_in[w.buf] = 1;
        ++w.reads;
    }
    void emit(Wave& w) {
        for (int i = 0; i < stores; ++i) w.vm.push_back(Op{false, -1, -1, -1});
    }

    // the part of interval t after barrier t, as the kernel's loops order it
    void after_barrier(Wave& w, int64_t t) {
        if (ts::emits_first(w.role) && t > 0) emit(w);                      // B: tile t - 1
        if (ts::issues(w.role)) {
            if (ts::multiplies(w.role)) w.ibuf = ts::prev_buffer(w.buf, dim);
            issue(w, ts::issue_tile(t, dim), w.ibuf, t);
            if (!ts::multiplies(w.role)) w.ibuf = ts::next_buffer(w.ibuf, dim);
        }
        if (ts::multiplies(w.role)) {
            read(w, t);
            w.buf = ts::next_buffer(w.buf, dim);
            if (!ts::emits_first(w.role)) emit(w);                          // A: tile t
        }
    }

    void run(int order) {
        for (Wave& w : wave) {
            if (ts::issues(w.role) && n_mine > 0)
                for (int b = 0; b < ts::prologue_tiles(dim); ++b) issue(w, b, ts::buffer_of(b, dim), -1);
            w.ibuf = ts::buffer_of(ts::issue_tile(0, dim), dim);
        }
        int64_t n_bar = ts::barriers(wave[0].role, n_mine);
        for (const Wave& w : wave)
            CHECK(ts::barriers(w.role, n_mine) == n_bar, "role %d executes %lld barriers, role %d %lld", (int)w.role,
                  (long long)ts::barriers(w.role, n_mine), (int)wave[0].role, (long long)n_bar);
        for (int64_t t = 0; t < n_bar; ++t) {
            for (Wave& w : wave)
                if (ts::waits(w.role)) wait(w, ts::wait_leaves(w.role, dim), t);
            // barrier t: what has landed is published
            for (Wave& w : wave) ++w.barriers;
            for (Slot& s : slot)
                if (s.landed && s.published < 0) s.published = t;
            read_in.assign(nbuf, 0);
            written_in.assign(nbuf, 0);
            if (order == 0)
                for (size_t i = 0; i < wave.size(); ++i) after_barrier(wave[i], t);
            else
                for (size_t i = wave.size(); i-- > 0;) after_barrier(wave[i], t);
            for (int b = 0; b < nbuf; ++b)
                CHECK(!(read_in[b] && written_in[b]), "buffer %d is read and rewritten in interval %lld", b, (long long)t);
        }
        for (Wave& w : wave) {
            wait(w, 0, -1);   // the vmcnt(0) before the block retires
            CHECK(w.barriers == n_bar, "barriers");
            CHECK(w.reads == (ts::multiplies(w.role) ? n_mine : 0), "tiles read");
            const int64_t tiles = n_mine > 0 ? ts::prologue_tiles(dim) + n_mine : 0;
            CHECK(w.issued == tiles * ts::pieces_issued(w.role, dim), "pieces issued");
        }
    }
};

static long replay(int dim) {
    long cases = 0;
    const int ks = ts::pieces_per_tile(dim), nbuf = ts::nbuf(dim);
    CHECK(nbuf >= 3 && nbuf * ts::tile_bytes(dim) <= ts::LDS_BUDGET, "ring of %d buffers", nbuf);
    CHECK(ts::wait_leaves(ts::ROLE_B, dim) < 64 && ts::wait_leaves(ts::ROLE_B, dim) == ts::wait_leaves(ts::ROLE_PAD_B, dim),
          "counted wait");
    CHECK(ts::pieces_issued(ts::ROLE_B, dim) * ts::N_ISSUERS == ks, "the issuers cover a tile");
    CHECK(ts::issue_step(ts::pieces_issued(ts::ROLE_B, dim) - 1) < ks, "pieces are issued within the multiply");
    // every piece of a tile belongs to exactly one issuer
    std::vector<int> owner(ks, 0);
    for (int iw = 0; iw < ts::N_ISSUERS; ++iw)
        for (int p = 0; p < ts::pieces_issued(ts::ROLE_B, dim); ++p) ++owner[ts::piece_index(iw, p)];
    for (int i = 0; i < ks; ++i) CHECK(owner[i] == 1, "piece %d has %d issuers", i, owner[i]);
    for (int buf = 0; buf < nbuf; ++buf) {
        CHECK(ts::prev_buffer(ts::next_buffer(buf, dim), dim) == buf, "ring");
        CHECK(ts::next_buffer(buf, dim) == ts::buffer_of(buf + 1, dim), "ring");
    }
    const int store_counts[] = {0, 1, 16};
    for (int64_t n_mine = 0; n_mine <= 9; ++n_mine)
        for (int live = 0; live <= ts::N_WAVES; ++live)      // waves 0 .. live - 1 work, the rest are padding
            for (int stores : store_counts)
                for (int order = 0; order < 2; ++order) {
                    Block b;
                    b.dim = dim, b.nbuf = nbuf, b.ks = ks, b.stores = stores, b.n_mine = n_mine;
                    b.slot.assign((size_t)nbuf * ks, Slot());
                    for (int w = 0; w < ts::N_WAVES; ++w) {
                        Wave wv;
                        wv.role = ts::role_of(w, w >= live);
                        wv.iw = w & (ts::N_ISSUERS - 1);
                        b.wave.push_back(wv);
                    }
                    b.run(order);
                    ++cases;
                }
    return cases;
}

int main() {
    // the three roles of the issue plus the padding wave of either group, by wave number
    CHECK(ts::role_of(0, false) == ts::ROLE_A && ts::role_of(3, true) == ts::ROLE_PAD_A, "roles");
    CHECK(ts::role_of(4, false) == ts::ROLE_B && ts::role_of(7, true) == ts::ROLE_PAD_B, "roles");
    CHECK(ts::nbuf(768) == 3 && ts::nbuf(512) >= 3 && ts::nbuf(512) <= 5, "ring sizes");
    long cases = 0;
    for (int dim : {512, 768}) cases += replay(dim);
    std::printf("dense tile schedule host check: ok (%ld replays)\n", cases);
    return 0;
}
