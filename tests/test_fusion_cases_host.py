"""What the builders of tests/fusion_cases.py promise, and what the fusion references of
oracle/thr_oracle.py are pinned to, checked on the CPU alone:

* the new oracle functions against the reference's recorded outputs (standalone_fusion.json: all
  16 ``fuse``, 16 ``two`` and 16 ``normalize`` records; merge_candidates.json for the ranks) and
  against the package's own CPU RRFFusion on the built cases;
* every builder reaches the branch it names (384 sightings, first sightings on one side of the wave
  boundary, probe chain of 128 that wraps, tie groups, interpolation weights on both sides of 0.5,
  plateau rows equal to the cut, 1024 / 1025 merge candidates, ...);
* the cases discriminate: each deliberately wrong variant of the reference changes the output of a
  named case.  That says nothing about the kernels; it shows that a kernel with the same mistake
  could not pass tests/test_gpu_fusion.py.

Scores are compared bit for bit through their int64 view unless a line says otherwise."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_cases as F  # noqa: E402

from oracle import thr_oracle as O  # noqa: E402


def bits(x):
    return np.asarray(list(x), dtype=np.float64).view(np.int64).tolist()


# ------------------------------------------------------------------- pins to the recorded outputs
def _id_table(*row_lists):
    t = {}
    for rows in row_lists:
        for r in rows:
            t.setdefault(r["chunk_id"], len(t) + 100)
    return t


def test_standalone_references_match_the_recorded_outputs(golden):
    g = golden("standalone_fusion.json")
    assert len(g["fuse"]) == 16 and len(g["two"]) == 16 and len(g["normalize"]) == 16
    for c in g["fuse"]:
        t = _id_table(c["lexical"], c["semantic"], c["graph"])
        back = {v: k for k, v in t.items()}
        chans = [[t[r["chunk_id"]] for r in c[k]] for k in ("lexical", "semantic", "graph")]
        cs = [[float(r.get(k + "_score", 0.0)) for r in c[k]] for k in ("lexical", "semantic", "graph")]
        ids, sc, rk = O.standalone_fuse_ids(*chans, weights=c["weights"])
        # up to the sort: the pinned whole-row reference with its tail switched off
        full = O.standalone_fuse(c["lexical"], c["semantic"], c["graph"], c["weights"], None, 0.0, False)
        assert [back[i] for i in ids] == [r["chunk_id"] for r in full]
        assert bits(sc) == bits(r["rrf_score"] for r in full)
        for i, r in zip(ids, rk):
            for ch in range(3):
                assert r[ch] == max([p + 1 for p, x in enumerate(chans[ch]) if x == i], default=0)
        # the tail, against the reference's own output
        oi, os_ = O.fuse_post_rows(ids, sc, rk, cs, c["safety_threshold"],
                                   c["denoise_alpha"] if c["denoise_enabled"] else None, c["top_k"])
        assert [back[i] for i in oi] == [r["chunk_id"] for r in c["out"]]
        assert bits(os_) == bits(r["rrf_score"] for r in c["out"])
    for c in g["two"]:
        t = _id_table(c["a"], c["b"])
        back = {v: k for k, v in t.items()}
        ids, sc, _ = O.standalone_fuse_two_ids([t[r["chunk_id"]] for r in c["a"]],
                                               [t[r["chunk_id"]] for r in c["b"]], c["wa"], c["wb"])
        k = c["top_k"] or len(ids)
        assert [back[i] for i in ids[:k]] == [r["chunk_id"] for r in c["out"]]
        assert bits(sc[:k]) == bits(r["rrf_score"] for r in c["out"])
    for c in g["normalize"]:
        assert bits(O.normalize_scores(c["in"])) == bits(c["out"])
        n = len(c["in"])
        assert bits(O.fuse_post_rows(range(n), c["in"], normalize=True)[1]) == bits(c["out"])


def test_rag2_ranks_match_the_recorded_merge(golden):
    seen = 0
    for c in golden("merge_candidates.json"):
        t = {}
        for rows in (c["lexical"] or [], c["semantic"], c["graph"] or []):
            for r in rows:
                t.setdefault(r["child_id"], len(t))
        chan = lambda rows: None if rows is None else [t[r["child_id"]] for r in rows]
        ids, _, rk = O.fused_topk_ranks(chan(c["lexical"]), chan(c["semantic"]), chan(c["graph"]), 10 ** 6)
        got = {i: r for i, r in zip(ids, rk)}
        assert len(got) == len(c["out"])
        for e in c["out"]:
            assert got[t[e["child_id"]]] == (e["lexical_rank"] or 0, e["semantic_rank"] or 0, e["graph_rank"] or 0)
            seen += 1
    assert seen > 100


def _hits(ids, scores=None, field=None):
    from triple_hybrid_rag_amd.core.types import SearchResult
    return [SearchResult(chunk_id=i, **({field: scores[p]} if scores is not None else {}))
            for p, i in enumerate(ids)]


def test_cpu_rrffusion_agrees_with_the_new_references_on_the_built_cases():
    from triple_hybrid_rag_amd.config import RAGConfig
    from triple_hybrid_rag_amd.core.fusion import RRFFusion
    from triple_hybrid_rag_amd.core.types import QueryPlan, SearchResult
    rows = F.rrf_rows()
    plain = RRFFusion(RAGConfig(rag_safety_threshold=0.0, rag_denoise_enabled=False))
    tail = RRFFusion(RAGConfig(rag_safety_threshold=F.SAFETY, rag_denoise_enabled=True, rag_denoise_alpha=0.6))
    for wname, w in F.WEIGHT_SETS.items():
        wd = dict(zip(F.NAMES, w))
        for nm, row in rows.items():
            lex, sem, gra = (F.cut(c) for c in row)
            out = plain.fuse(_hits(lex), _hits(sem), _hits(gra), QueryPlan(weights=wd))
            ids, sc, _ = O.standalone_fuse_ids(lex, sem, gra, wd)
            assert [h.chunk_id for h in out] == ids, (wname, nm)
            assert bits(h.rrf_score for h in out) == bits(sc), (wname, nm)
            out = plain.fuse_two_channels(_hits(lex), _hits(sem), w[0], w[1])
            ids2, sc2, _ = O.standalone_fuse_two_ids(lex, sem, w[0], w[1])
            assert [h.chunk_id for h in out] == ids2 and bits(h.rrf_score for h in out) == bits(sc2), (wname, nm)
            # the tail, with synthetic channel scores
            cs = [[((p * 7 + c) % 8) / 8.0 for p in range(len(ch))] for c, ch in enumerate((lex, sem, gra))]
            out = tail.fuse(_hits(lex, cs[0], "lexical_score"), _hits(sem, cs[1], "semantic_score"),
                            _hits(gra, cs[2], "graph_score"), QueryPlan(weights=wd), top_k=10)
            ids, sc, rk = O.standalone_fuse_ids(lex, sem, gra, wd)
            ei, es = O.fuse_post_rows(ids, sc, rk, cs, F.SAFETY, 0.6, 10)
            assert [h.chunk_id for h in out] == ei and bits(h.rrf_score for h in out) == bits(es), (wname, nm)
            normed = plain.normalize_scores([SearchResult(final_score=v) for v in sc])
            assert bits(h.final_score for h in normed) == bits(O.normalize_scores(sc))


def test_native_wrappers_refuse_top_k_above_the_table():
    """_native.rrf_fuse / rrf_fuse_standalone name the limit instead of handing top_k > 512 to the library."""
    torch = pytest.importorskip("torch")
    from triple_hybrid_rag_amd import _native as N
    ids = torch.zeros((1, 4), dtype=torch.int64)
    for fn in (N.rrf_fuse, N.rrf_fuse_standalone):
        for top_k in (F.SLOTS + 1, 0):
            with pytest.raises(N.NativeError, match=str(F.SLOTS)):
                fn(None, ids, None, top_k)
    assert N.THR_RRF_MAX_TOP_K == F.SLOTS


# ------------------------------------------------------------------------ the builders' promises
def test_rrf_rows_reach_their_branches():
    R = F.rrf_rows()
    for nm, row in R.items():
        assert all(len(c) <= F.MAXC for c in row), nm
    n_sight = lambda nm: len(F.sighting_order(*R[nm]))
    assert n_sight("cap_disjoint") == 3 * F.MAXC == 384
    for nm in ("overlap_same", "overlap_sem_reversed", "overlap_gra_rot1"):
        assert n_sight(nm) == F.MAXC and all(len(c) == F.MAXC for c in R[nm])
    fs = lambda nm: F.first_sighting_positions(*R[nm])
    assert all(p and max(p) < F.WAVE for p in fs("wave_low")[1:])
    assert all(p and min(p) >= F.WAVE for p in fs("wave_high")[1:])
    assert fs("wave_63_64")[1] == [63, 64] and fs("wave_63_64")[2] == [63, 64]
    assert fs("wave_no_new")[1] == [] and fs("wave_no_new")[2] != [] and len(fs("wave_no_new")[0]) == F.MAXC
    assert fs("wave_no_new_gra")[2] == [] and fs("wave_no_new_gra")[1] != []
    lex, sem, gra = R["dup_ends"]
    assert [p for p, i in enumerate(lex) if i == 7] == [0, 127] and sem.count(8) == 2 and sem.index(8) == 0
    assert R["dup_128"][0] == [5] * 128 and R["dup_128"][1] == [5] * 128
    # 128 sequential adds of one value are not the single product: the order of summation shows
    v = 0.7 * (1.0 / (60 + 128))
    acc = 0.0
    for _ in range(128):
        acc += v
    assert acc != 128 * v
    lex, sem, _ = R["b_only_twice"]
    assert sem.count(9) == 2 and 9 not in lex
    assert -1 in R["interior_minus1"][0][1:-1] and R["interior_minus1"][0][-1] >= 0
    assert R["minus1_first"][0][0] == -1 and R["minus1_first"][1][0] >= 0
    assert any(i < -1 for i in R["negative_other"][1])
    assert 0 in R["ids_extreme"][0] and 2 ** 62 in R["ids_extreme"][0]
    # exact ties: groups of three that straddle sighting position 128 (equal weights), pairs, and a
    # group of 128 at 0.0 under the zero semantic weight
    for flavour in ("rag2", "standalone"):
        ids, sc, _, _ = F.rrf_expect(flavour, *R["tie_cycles"], F.W_EQUAL, F.SLOTS)
        order = F.sighting_order(*R["tie_cycles"])
        b = bits(sc)
        for g in range(0, 192, 3):
            assert b[g] == b[g + 1] == b[g + 2]
            pos = [order.index(i) for i in ids[g:g + 3]]
            assert pos == sorted(pos) and pos[0] < 128 <= pos[2]
        ids, sc, _, _ = F.rrf_expect(flavour, *R["tie_pairs"], F.W_EQUAL, F.SLOTS)
        by = dict(zip(ids, bits(sc)))
        A = R["tie_pairs"][0]
        assert all(by[A[p]] == by[A[p ^ 1]] for p in range(F.MAXC))
        assert all(ids.index(A[p]) + 1 == ids.index(A[p + 1]) for p in range(0, F.MAXC, 2))   # sighting order
        ids, sc, _, _ = F.rrf_expect(flavour, *R["zero_group"], F.W_ZERO_SEM, F.SLOTS)
        order = F.sighting_order(*R["zero_group"])
        zero = [i for i, s in zip(ids, sc) if s == 0.0]
        assert len(zero) == 128 and zero == order[100:228]      # at least 4 members, across position 128
    ids, sc, _, n = F.rrf_expect("standalone", *R["cap_disjoint"], F.W_ALL_ZERO, F.SLOTS)
    assert n == 384 and ids == F.sighting_order(*R["cap_disjoint"]) and set(sc) == {0.0}
    ids, sc, _, _ = F.rrf_expect("rag2", *R["cap_disjoint"], F.W_NEGATIVE, F.SLOTS)
    assert min(sc) < 0.0
    # the largest rrf_k: k + 128 == INT_MAX exactly, one more would overflow an int
    assert F.RRF_K_MAX + F.MAXC == 2 ** 31 - 1


def test_shortcut_rows_build_a_probe_chain_that_wraps():
    rows, slot = F.shortcut_rows()
    assert rows.shape == (3, F.MAXC) and slot >= 500 and slot + F.MAXC > F.SLOTS      # wraps past 511
    assert {F.hash_slot(int(i)) for i in rows.ravel()} == {slot}                      # one chain
    assert len(set(rows[0].tolist())) == F.MAXC
    assert rows[1, -1] == rows[1, 0] and len(set(rows[1].tolist())) == F.MAXC - 1
    assert rows[2, 63] == rows[2, 64] and len(set(rows[2].tolist())) == F.MAXC - 1
    # the formula, on a value worked by hand: 1 * C >> 40 = 0x9E3779, & 511 = 0x179
    assert F.hash_slot(1) == 0x9E3779 & 511


def test_post_calls_reach_their_branches():
    calls = {c.name: c for c in F.post_safety_calls()}
    c = calls["safety_no_denoise"]
    kept = {nm: c.expect(q)[0] for q, nm in enumerate(c.row_names)}
    n = c.ids.shape[1]
    assert n == 384 and len(kept["all_kept"]) == n and kept["none_kept"] == []
    pos = lambda nm: [list(c.ids[c.row_names.index(nm)]).index(i) for i in kept[nm]]
    assert pos("straddle_127_128") == [127, 128] and pos("straddle_255_256") == [3, 255, 256, 300]
    assert pos("trips") == [0, 127, 128, 255, 256, 383]
    assert len(kept["two_survivors"]) == 2 and len(kept["three_survivors"]) == 3
    assert len(kept["at_threshold"]) == 3
    assert kept["dup_last_rank_low"] == [] and kept["dup_last_rank_high"] == [7]
    d = calls["safety"]
    q2, q3 = d.row_names.index("two_survivors"), d.row_names.index("three_survivors")
    assert len(d.expect(q2)[0]) == 2 and len(d.expect(q3)[0]) < 3      # denoise skipped at 2, runs at 3
    g = calls["safety_graph_scores_absent"]
    qa = g.row_names.index("all_kept")
    assert (g.ranks[qa, :, 2] > 0).sum() == 128 and len(g.expect(qa)[0]) < len(d.expect(qa)[0])
    sizes = F.post_size_calls()
    assert {c.ids.shape[1] for c in sizes} == set(F.POST_SIZES)
    assert any(c.counts is None for c in sizes)
    for c in sizes:
        if c.counts is not None:
            n = c.ids.shape[1]
            assert list(c.counts) == [0, 1, 2, 3, n - 1, n, n + 5] and c.row_count(6) == n
    pool = F.score_pool()
    assert len(pool) == 512 and all(a > b for a, b in zip(pool, pool[1:]))


def test_percentile_sweep_covers_both_lerp_branches_and_the_plateau_cut():
    assert len(F.ALPHAS) == 21 + 4          # (0.3, 0.6 and 0.9 are 6/20, 12/20 and 18/20, the same doubles)
    assert {0.0, 1.0, 0.5, 1 / 3, 2 / 3, 1e-9, 1 - 1e-9} <= set(F.ALPHAS)
    assert set(range(3, 41)) | {127, 128, 129, 384, 512} == set(F.SWEEP_M)
    g = [F.lerp_weight(m, a) for a in F.ALPHAS for m in F.SWEEP_M]
    assert any(0 < x < 0.5 for x in g) and any(x >= 0.5 for x in g) and any(x == 0.0 for x in g)
    on_cut = total = 0
    for a in F.ALPHAS:
        c = F.post_sweep_call(a)
        assert c.ids.shape == (3 * len(F.SWEEP_M), F.SLOTS)
        for q, nm in enumerate(c.row_names):
            m = c.row_count(q)
            thr = np.percentile(c.scores[q, :m], (1 - a) * 100)
            ids, sc = c.expect(q)
            total += 1
            if nm.startswith("plateau"):
                eq = int((c.scores[q, :m].view(np.int64) == np.float64(thr).view(np.int64)).sum())
                if eq >= 2:
                    on_cut += 1
                    assert sc[-eq:] == [float(thr)] * eq      # every row equal to the cut stays
    assert on_cut > 100, (on_cut, total)


def test_rerank_cases_reach_their_branches():
    assert F.F32_DENORM > 0 and F.F32_DENORM < np.finfo(np.float32).tiny
    assert float(np.float32(F.F32_DENORM)) == F.F32_DENORM
    R = F.rerank_rows(512)
    assert max(R["tie_group"].count(v) for v in set(R["tie_group"])) >= 300
    assert R["all_unscored"] == [None] * 512
    z = R["zeros_next_to_unscored"]
    assert any(v is None for v in z) and any(v == 0.0 and np.signbit(v) for v in z if v is not None)
    ids = list(range(512))
    assert F.rerank_expect(z, ids, 512, 512)[0] == ids                      # all tie: order unchanged
    assert F.rerank_expect(R["all_unscored"], ids, 512, 512)[0] == ids
    neg = F.rerank_expect(R["negatives_below_unscored"], ids, 512, 512)
    assert neg[1] == sorted(neg[1], reverse=True) and neg[1][-1] < 0.0 and 0.0 in neg[1]
    assert F.rerank_expect(R["plus_inf"], ids, 512, 1)[1] == [float("inf")]
    for nl in F.RERANK_LISTS:
        sc, ids_a, vals, names = F.rerank_case(129, nl)
        assert sc.shape == (nl, len(names), 129) and sc.dtype == np.float32
        q = names.index("two_lists_finite")
        both = (np.isfinite(sc[:, q, :]).sum(axis=0) >= 2).sum()
        assert both > 100 if nl > 1 else both == 0
        best = sc[:, q, :].max(axis=0)
        assert [float(x) for x in best] == vals[q]                        # the maximum is the value
    assert set(F.rerank_counts(128, 10)) == {0, 128, 131, 64, 127}


def test_merge_cases_reach_their_branches():
    assert [g * k for g, k in F.MERGE_SHAPES] == [F.MERGE_CAP, F.MERGE_CAP + 1, 1]
    better = lambda s1, i1, s0, i0: s1 > s0 or (s1 == s0 and i1 < i0)
    for G, k in F.MERGE_SHAPES[:2]:
        R = F.merge_rows(G, k)

        def ranked(nm, l):
            s, i = R[nm][0][l].copy(), R[nm][1][l].copy()
            bad = ~(s > -np.inf) | (i < 0)
            s[bad], i[bad] = -np.inf, np.iinfo(np.int64).max
            return not any(better(s[p + 1], i[p + 1], s[p], i[p]) for p in range(k - 1))
        for nm in ("random", "cross_ties", "all_tied", "few_valid", "plus_inf", "signed_zeros", "duplicate_pairs"):
            assert all(ranked(nm, l) for l in range(G)), nm
        assert not any(ranked("tied_ids_descend", l) for l in range(G))
        s, i = R["tied_ids_descend"]
        assert all(np.all(np.diff(s[l]) <= 0) for l in range(G))              # ranked by score alone
        s, i = R["invalid_entries"]
        assert (i[0] == -1).sum() == 1 and np.isfinite(s[0][i[0] == -1]).all()
        assert np.isnan(s).sum() == 1 and (np.isneginf(s) & (i >= 0)).sum() == 1
        assert np.all(i[1] == -1) and not ranked("invalid_entries", 0)        # valid after invalid
        s, i = R["few_valid"]
        assert 0 < (i >= 0).sum() < 512
        s, i = R["cross_ties"]
        es, ei = F.merge_expect(s, i, 512)
        assert len(set(es.tolist())) <= 6 and len(set(s[0]) & set(s[1])) >= 2
        s, i = R["signed_zeros"]
        assert np.signbit(s[0][s[0] == 0]).all() and not np.signbit(s[1][s[1] == 0]).any()
        es, ei = F.merge_expect(s, i, 512)
        z = np.signbit(es[es == 0])
        assert z.any() and not z.all() and (i >= 0).all() and (s > 0).sum() < 512
        s, i = R["duplicate_pairs"]
        pairs = list(zip(s.ravel().tolist(), i.ravel().tolist()))
        assert len(pairs) - len(set(pairs)) >= k // 2
        es, ei = F.merge_expect(s, i, 512)
        assert len(ei) == 512 and len(set(ei.tolist())) < 512                 # both copies come out
        assert np.isinf(R["plus_inf"][0]).any() and np.isinf(F.merge_expect(*R["plus_inf"], 10)[0]).all()


# ---------------------------------------------------------------- the cases discriminate (mutants)
def fuse_variant(flavour, lex, sem, gra, weights, rrf_k=60, rank="last", once=False, by_id=False):
    """The fusion arithmetic with switches for the classic mistakes.  All switches off: the oracle."""
    chans = [F.cut(lex) or [], F.cut(sem) or [], [] if flavour == "two" else (F.cut(gra) or [])]
    rk = lambda c, i: (chans[c].index(i) + 1 if rank == "first"
                       else max(p + 1 for p, x in enumerate(chans[c]) if x == i)) if i in chans[c] else 0
    out = []
    for i in F.sighting_order(*chans):
        r = [rk(c, i) for c in range(3)]
        s = 0.0
        for c in range(3):
            if not r[c]:
                continue
            if flavour == "rag2":
                s += weights[c] / (rrf_k + r[c])
            else:
                v = weights[c] * (1.0 / (60 + r[c]))
                reps = 1 if once or (flavour == "two" and c == 0) else chans[c].count(i)
                for _ in range(reps):
                    s += v
        out.append((i, s, tuple(r)))
    key = (lambda t: (-t[1], t[0])) if by_id else (lambda t: -t[1])
    out.sort(key=key)
    return [t[0] for t in out], [t[1] for t in out], [t[2] for t in out]


def _rrf_changed(**mut):
    """(flavour, weight set, row) of every built case whose ids, scores or ranks the variant changes."""
    R = F.rrf_rows()
    changed = set()
    for flavour in ("rag2", "standalone", "two"):
        for wname, w in F.WEIGHT_SETS.items():
            for nm, row in R.items():
                ei, es, er, _ = F.rrf_expect(flavour, *row, w, F.SLOTS)
                gi, gs, gr = fuse_variant(flavour, *row, w, **mut)
                if (gi, bits(gs), gr) != (ei, bits(es), er):
                    changed.add((flavour, wname, nm))
    return changed


def test_variant_without_a_mistake_is_the_oracle():
    assert _rrf_changed() == set()
    rows, _ = F.shortcut_rows()
    for row in rows:
        for flavour in ("rag2", "standalone", "two"):
            ei, es, er, _ = F.rrf_expect(flavour, None, row, None, F.W_DEFAULT, F.SLOTS)
            assert (ei, bits(es), er) == tuple(x if j != 1 else bits(x) for j, x in
                                               enumerate(fuse_variant(flavour, None, row, None, F.W_DEFAULT)))


def test_cases_catch_first_rank_used_instead_of_last():
    ch = _rrf_changed(rank="first")
    assert ("rag2", "default", "dup_ends") in ch and ("standalone", "default", "dup_ends") in ch
    assert ("two", "default", "dup_ends") in ch


def test_cases_catch_occurrences_counted_once():
    ch = _rrf_changed(once=True)
    assert {("standalone", "default", nm) for nm in ("dup_ends", "dup_128", "b_only_twice")} <= ch
    assert {("two", "default", nm) for nm in ("dup_ends", "dup_128", "b_only_twice")} <= ch
    assert not any(f == "rag2" for f, _, _ in ch)        # the RAG2 flavour has no occurrence counts


def test_cases_catch_an_unstable_sort_with_ties_ordered_by_id():
    ch = _rrf_changed(by_id=True)
    for flavour in ("rag2", "standalone"):
        assert (flavour, "equal", "tie_cycles") in ch and (flavour, "zero_sem", "zero_group") in ch
        assert (flavour, "all_zero", "overlap_sem_reversed") not in ch      # (sighting order is id order there)
        assert (flavour, "all_zero", "tie_cycles") in ch
    assert ("two", "all_zero", "tie_cycles") in ch


def post_variant(ids, scores, ranks, channel_scores, safety, alpha, top_k, normalize, safety_gt=False,
                 cut_gt=False, own_lerp=False, no_half_branch=False, minmax_first=False):
    """fuse_post_rows with switches.  ``own_lerp`` restates numpy's interpolation (so that its
    ``t >= 0.5`` branch can be dropped); with every switch off it is the oracle."""
    rows = list(zip(ids, scores))
    if safety > 0:
        def best(j):
            v = [float(channel_scores[c][ranks[j][c] - 1]) if ranks[j][c] > 0 and channel_scores[c] is not None
                 else 0.0 for c in range(3)]
            return max(v)
        rows = [r for j, r in enumerate(rows) if (best(j) > safety if safety_gt else best(j) >= safety)]
    if alpha is not None and len(rows) >= 3:
        sc = np.array([s for _, s in rows])
        if own_lerp or no_half_branch:
            asc = np.sort(sc)
            v = (len(asc) - 1) * F.quantile_of(alpha)
            lo = int(np.floor(v))
            hi = min(lo + 1, len(asc) - 1)
            t = v - lo
            a, b = float(asc[lo]), float(asc[hi])
            thr = b - (b - a) * (1 - t) if (t >= 0.5 and not no_half_branch) else a + (b - a) * t
        else:
            thr = np.percentile(sc, (1 - alpha) * 100)
        rows = [r for r in rows if (r[1] > thr if cut_gt else r[1] >= thr)]
    lo_hi = (min(s for _, s in rows), max(s for _, s in rows)) if rows else None
    if top_k:
        rows = rows[:top_k]
    out = [s for _, s in rows]
    if normalize and out:
        lo, hi = lo_hi if minmax_first else (min(out), max(out))
        out = [1.0 if hi == lo else (v - lo) / (hi - lo) for v in out]
    return [i for i, _ in rows], out


def _all_post_calls():
    return (F.post_size_calls() + F.post_safety_calls() + F.post_topk_norm_calls()
            + [F.post_sweep_call(a) for a in F.ALPHAS])


def _post_changed(**mut):
    changed = set()
    for c in _all_post_calls():
        for q, nm in enumerate(c.row_names):
            ei, es = c.expect(q)
            gi, gs = c.expect(q, lambda *a: post_variant(*a, **mut))
            if (gi, bits(gs)) != (ei, bits(es)):
                changed.add((c.name, nm))
    return changed


def test_post_variant_without_a_mistake_is_the_oracle_and_restates_numpy_exactly():
    assert _post_changed() == set()
    assert _post_changed(own_lerp=True) == set()       # the restated interpolation is numpy's, bit for bit


def test_cases_catch_strict_comparisons_at_the_threshold_and_the_cut():
    assert ("safety_no_denoise", "at_threshold") in _post_changed(safety_gt=True)
    ch = _post_changed(cut_gt=True)
    assert any(name.startswith("sweep") and nm.startswith("plateau") for name, nm in ch)
    assert any(name.startswith("sweep") and nm.startswith("strict") for name, nm in ch)   # weight exactly 0


def _cut(scores, alpha, no_half_branch):
    asc = np.sort(np.asarray(scores))
    v = (len(asc) - 1) * F.quantile_of(alpha)
    lo = int(np.floor(v))
    t, a, b = v - lo, float(asc[lo]), float(asc[min(lo + 1, len(asc) - 1)])
    return b - (b - a) * (1 - t) if (t >= 0.5 and not no_half_branch) else a + (b - a) * t


def test_cases_reach_the_upper_lerp_branch_where_its_value_differs():
    """The ``t >= 0.5`` form of numpy's lerp dropped.  What the sweep can and does show is the CUT: on
    named rows (the widely spaced family; where neighbours lie within a few percent of each other the
    two forms round to the same double) the one-form cut has other bits than numpy's.  The rows thr_fuse_post keeps cannot show
    it, on any input: with a < b adjacent in the sorted scores both forms give a value in (a, b] for
    t >= 0.5 (a + fl((b - a) t) <= fl(a + fl(b - a)) never passes b for t <= 1 - 2^-53, and t here is
    a difference of doubles >= 2, so 1 - t >= 2^-52), so b and everything above stays and a goes either
    way; with a == b both forms give a.  The assertion on the outputs therefore reads: no case
    changes -- if one ever did, the argument above would be wrong and the case belongs in the sweep."""
    differ = []
    for alpha in F.ALPHAS:
        c = F.post_sweep_call(alpha)
        for q, nm in enumerate(c.row_names):
            sc = c.scores[q, :c.row_count(q)]
            ref = float(np.percentile(sc, (1 - alpha) * 100))
            assert bits([_cut(sc, alpha, False)]) == bits([ref]), (alpha, nm)
            if bits([_cut(sc, alpha, True)]) != bits([ref]):
                differ.append((c.name, nm))
    assert len(differ) > 20 and all(nm.startswith("wide") for _, nm in differ), len(differ)
    assert _post_changed(no_half_branch=True) == set()


def test_cases_catch_min_and_max_taken_before_top_k():
    ch = _post_changed(minmax_first=True)
    assert ("normalize_after_topk", "decreasing") in ch and ("normalize_after_topk", "negatives_and_zero") in ch
    assert ("normalize_after_denoise_topk", "decreasing") in ch


def test_cases_catch_a_merge_tie_break_of_id_descending():
    def id_desc(scores, k, ids):
        keep = scores > -np.inf
        s, i = scores[keep], ids[keep]
        o = np.lexsort((-i, -s))[:k]
        return s[o], i[o]
    for G, k in F.MERGE_SHAPES[:2]:
        S, I, names = F.merge_case(G, k)
        changed = {nm for q, nm in enumerate(names)
                   if not np.array_equal(F.merge_expect(S[:, q], I[:, q], 512)[1],
                                         F.merge_expect(S[:, q], I[:, q], 512, id_desc)[1])}
        assert {"cross_ties", "all_tied", "signed_zeros"} <= changed and "random" not in changed
