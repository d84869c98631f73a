"""What the builders of tests/graph_cases.py promise, checked with the oracle alone (no GPU): each
tier variant lies in its range of reached entities / contributions and has the unballasted case's
expected output, each boundary case has exactly the stated count, the long sums are order-sensitive,
the tie cases tie across the k boundary, the flood shares the 32-bit key prefix, and every workgroup
of the global-memory tier gets at least two queries.  These are conditions on the inputs: until they
hold, tests/test_gpu_graph.py means nothing."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_cases as GC  # noqa: E402

from oracle import thr_oracle as O  # noqa: E402


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def check_tier_and_output(case, wname):
    """The queries the variant is about lie in its tier; the output is the unballasted one, bit for bit."""
    for q in range(case.nq):
        nr, slots, _ = GC.reach_counts(case, q)
        if case.ballasted[q]:
            assert GC.tier_of(nr, slots) == case.intended_tier, \
                f"{case.name}/{case.tier}/{wname} q{q}: {nr} entities, {slots} slots is not the {case.intended_tier} tier"
        elif case.tier == "asbuilt" and case.name not in GC.EDGES:
            assert GC.tier_of(nr, slots) == "small"
    if case.tier == "asbuilt":
        return                       # (GC.scores is the oracle over this very case)
    base = GC.scores(case.name, wname)
    got = GC.oracle_scores(case)
    assert len(base) == len(got) == case.nq
    for q in range(case.nq):
        assert same_bits(base[q], got[q]), f"{case.name}/{case.tier}/{wname} q{q}: the ballast changes the answer"


def boundary_ties(s, k):
    """-> (chunks that tie with the k-th best score, how many of them the top-k holds)"""
    ts, _ = O.topk_desc(s, k)
    return int((s == ts[-1]).sum()), int((ts == ts[-1]).sum())


def check_distances(case, wname):
    hops = case.hops
    dist = [GC.oracle_dist(case, q) for q in range(case.nq)]
    assert list(np.flatnonzero(dist[0][:10] >= 0)) == list(range(hops + 1))           # the path, one more per hop
    assert all(dist[0][e] == e for e in range(hops + 1))
    if hops >= 3:
        assert dist[0][3] == 3 and dist[1][3] == 1 and dist[2][3] == 1 and dist[2][2] == 2   # the shortcut
    if hops >= 1:
        assert dist[6][41] == 1 and dist[7][40] == -1                                 # one direction only
        assert dist[8][43] == 1 and dist[9][42] == 1
        assert dist[4][31] == 1 and dist[4][33] == 1 and dist[4][32] == (2 if hops >= 2 else -1)   # the cycle
    g = case.g
    assert -1 in g[1] and case.n_entities in g[1] and -1 not in case.clean_g[1]
    assert case.clean_g[1].max() < case.n_entities
    # every term is exact: conf / (1 + d) * (1 + d) == conf for every d the ABI allows
    conf = g[4][g[4] != np.float32(0.75)].astype(np.float64)
    for d in range(GC.MAX_HOPS + 1):
        assert np.all(conf / (1.0 + d) * (1.0 + d) == conf) and np.all(conf / (1.0 + d) == np.rint(conf / (1.0 + d)))
    assert len({c / (1.0 + d) for c in conf[:1] for d in range(9)}) == 9


def check_sum_order(case, wname):
    chunks, segs = case.hits["chunks"], case.hits["segments"]
    where = GC.sorted_positions(case, 0)
    base_scores = GC.scores(case.name, wname)[0]
    for chunk, L in zip(chunks, segs):
        terms = GC.contributions(case, 0, chunk)
        assert len(terms) == L and where[chunk][1] - where[chunk][0] == L
        s = GC.sum_in_order(terms)
        assert same_bits(s, base_scores[chunk - case.window[0]])
        if L > 2:      # (a sum of two terms is the same in either order: that segment is there for its position)
            assert not same_bits(s, GC.sum_in_order(terms[::-1])), f"segment {L}: the reverse order gives the same bits"
            assert not same_bits(s, GC.sum_in_order(sorted(terms))), f"segment {L}: the sorted order gives the same bits"
        assert len({float(t) for t in terms}) > 1
    spans = [where[c] for c in chunks]
    assert any(lo < 256 < hi for lo, hi in spans), "no segment straddles position 256"
    if case.name == "sum_order_long":
        assert any(lo < 2048 < hi for lo, hi in spans), "no segment straddles position 2048"
    dist = GC.oracle_dist(case, 0)
    assert {0, 1, 2} <= set(dist[dist >= 0])


def check_ties(case, wname):
    k = case.k
    s = dict(zip(GC.TIE_QUERIES, GC.scores(case.name, wname)))
    n_in = case.window[1]
    for name in ("plain", "ids_descending", "flood"):
        tied, taken = boundary_ties(s[name], k)
        assert tied > taken and tied > k, f"{name} k={k}: {tied} chunks tie at the boundary, {taken} are taken"
    assert np.isfinite(s["plain"]).sum() > 512                     # more hits than the small tier's buffer holds
    assert len(np.unique(s["plain"][np.isfinite(s["plain"])])) == 1
    _, ti = O.topk_desc(s["plain"], k)
    assert list(ti) == list(np.flatnonzero(np.isfinite(s["plain"]))[:k])        # the k lowest ids
    _, ti = O.topk_desc(s["ids_descending"], k)
    hit = np.flatnonzero(np.isfinite(s["ids_descending"]))
    assert ti.min() > hit[len(hit) // 2]                           # the best sit on the highest ids
    flood = s["flood"][np.isfinite(s["flood"])]
    assert len(np.unique(flood)) == 8 and len(np.unique(GC.dkey_prefix(flood))) == 1
    mags = s["magnitudes"][np.isfinite(s["magnitudes"])]
    assert len(np.unique(np.frexp(mags)[1])) > 64
    assert len(np.unique(GC.dkey_prefix(mags) >> 24)) > 4          # the radix select's first digit varies
    z = s["zeros"]
    assert (z == 0.0).sum() > GC.TOPK_MAX and 0 < (z > 0.0).sum() < 50
    if k == 50:
        ts, _ = O.topk_desc(z, k)
        assert ts[0] > 0.0 and ts[-1] == 0.0 and not np.signbit(ts[-1])
        tied, taken = boundary_ties(z, k)
        assert tied > taken
    assert 0 < np.isfinite(s["short"]).sum() < 50
    assert n_in >= 1500


def check_seeds(case, wname):
    n = case.n_entities
    if case.name == "seeds_one":
        assert case.seeds.shape[1] == (1 if case.tier == "asbuilt" else 2)
        lonely = 17
        assert case.g[0][lonely] == case.g[0][lonely + 1] and case.g[2][lonely] == case.g[2][lonely + 1]
        assert lonely not in case.g[1]
        assert case.seeds[2, 0] == n and case.seeds[3, 0] == 2 ** 31 - 1 and case.seeds[4, 0] == -1
        for q in (1, 2, 3, 4):
            assert not np.isfinite(GC.scores(case.name, wname)[q]).any()          # count 0
    else:
        assert case.seeds.shape[1] == GC.MAX_SEEDS
        assert len(set(case.seeds[0])) == 16 and np.all((case.seeds[0] >= 0) & (case.seeds[0] < n))
        assert len(set(case.seeds[1])) < 16 and np.all(case.seeds[1] >= 0)
        assert np.all(case.seeds[2] == -1) and not case.ballasted[2]
        assert np.any(case.seeds[3] >= n) and n in case.seeds[3] and np.any(case.seeds[3] < -1)
        assert np.any(case.clean_seeds[3] >= 0) and np.all(case.clean_seeds[3] < n)
        assert not np.isfinite(GC.scores(case.name, wname)[2]).any()


def check_star(case, wname):
    nr, slots, _ = GC.reach_counts(case, 0)
    assert nr == case.hits["reached"] and slots <= 2 * nr
    assert case.hops == 1


def check_mentions(case, wname):
    nr, slots, kept = GC.reach_counts(case, 0)
    assert nr == 1 and slots == kept == case.hits["mentions"] and case.hops == 0


def check_scoped_mentions(case, wname):
    nr, slots, kept = GC.reach_counts(case, 0, 0, case.doc_label)
    assert nr == 1 and slots == GC.SCOPED_TOTAL and kept == case.hits["kept"]
    assert GC.reach_counts(case, 2)[2] > GC.FULL_CON         # the same entity without a label


def check_fallback_reuse(case, wname):
    hub = case.hits["hub"]
    over = [q for q in range(case.nq) if GC.tier_of(*GC.reach_counts(case, q)[:2]) == "global"]
    assert over == list(np.flatnonzero(hub >= 0)) and len(over) >= 150
    assert case.n_entities % 4 != 0
    reached = {}
    for b in range(GC.FB_BLOCKS):
        mine = [q for q in over if q % GC.FB_BLOCKS == b]
        assert 2 <= len(mine) <= 3, f"workgroup {b} takes {len(mine)} third-tier queries"
        for q in mine:
            reached[q] = frozenset(np.flatnonzero(GC.oracle_dist(case, q) >= 0))
        for a, c in zip(mine, mine[1:]):
            assert hub[a] != hub[c]
            assert max(reached[a] & reached[c], default=0) < 62 and reached[a] != reached[c]   # disjoint neighbourhoods
        assert len({reached[q] for q in mine}) == len(mine)      # the other seeds: the same hub again is another set
        assert len({int(case.seeds[q, 0]) for q in mine}) == len(mine)
    assert any(case.n_entities - 1 in r for r in reached.values())
    on_chip = [q for q in range(case.nq) if hub[q] < 0]
    assert len(on_chip) >= 30 and all(hub[q - 1] >= 0 for q in on_chip)           # interleaved


CHECKS = (("distances", check_distances), ("sum_order", check_sum_order), ("ties", check_ties),
          ("seeds", check_seeds), ("star", check_star), ("mentions", check_mentions),
          ("scoped_mentions", check_scoped_mentions), ("fallback_reuse", check_fallback_reuse))


@pytest.mark.parametrize("name", list(GC.BUILDERS))
def test_the_case_is_what_it_says(name):
    check = next(fn for prefix, fn in CHECKS if name.startswith(prefix))
    for wname in GC.WINDOWS:
        for tier in (GC.TIERS if name in GC.CONTENT else GC.TIERS[:1]):
            case = GC.build(name, wname, tier)
            assert case.window == GC.WINDOWS[wname] and case.tier == tier
            assert 1 <= case.seeds.shape[1] <= GC.MAX_SEEDS and 1 <= case.k <= GC.TOPK_MAX
            assert case.n_entities <= 15000
            check_tier_and_output(case, wname)
            check(case, wname)
    # on the shard some mentions lie below the base and some at or beyond its end
    case = GC.build(name, "shard", GC.TIERS[-1] if name in GC.CONTENT else "asbuilt")
    base, n = case.window
    if not name.startswith(("star", "mentions", "scoped_mentions")):
        assert (case.g[3] < base).any() and (case.g[3] >= base + n).any()


def test_outside_chunks_lie_on_both_sides():
    base, n = GC.SHARD
    out = GC.outside_chunks(GC.SHARD, 5000)
    assert len(set(out)) == 5000 and not ((out >= base) & (out < base + n)).any()
    assert (out < base).sum() == base and base + n in out and out.min() == 0
    out = GC.outside_chunks(GC.WHOLE, 100)
    assert np.all(out >= GC.N_CORPUS)


def test_dkey_prefix_orders_like_the_scores():
    x = np.array([-np.inf, -2.0, -0.0, 0.0, 2.0 ** -40, 1.0, 1.0 + 2.0 ** -23, 1.5, 3.0e10, np.inf])
    p = GC.dkey_prefix(x).astype(np.int64)
    assert np.all(np.diff(p) >= 0) and p[5] == p[6] and p[4] < p[5] < p[7]
