"""What the builders of tests/bm25_cases.py promise, checked with the oracle and float64 numpy alone
(no GPU): the quantiser clips where a case says it does, the tie cases tie across the k boundary and
list the lowest ids, the stage-B cases take their top-k from the side they are named for, the ladder
terms stand on the stated sides of the row edges, the sliced queries exceed one slice.  These are
conditions on the inputs: until they hold, tests/test_gpu_bm25_values.py means nothing.  Every case
runs; none is skipped.

Also here, on CPU tensors: _native.bm25_check_params, the input contract of the pruning bounds."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm25_cases as BC  # noqa: E402

from oracle import thr_oracle as O  # noqa: E402


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def holds(c, name):
    m = np.zeros(c.n, dtype=bool)
    m[c.docs_of(name)] = True
    return m


def boundary(c, p, k, k1=BC.DEFAULT[0], b=BC.DEFAULT[1]):
    """-> (docs bit-equal to the k-th score, how many of them the top-k holds, are those the lowest ids)"""
    s = BC.all_scores(c, p, k1, b)
    ts, ti = O.topk_desc(s, k)
    assert len(ts) == k, f"{c.name}/{c.qname[p]}: only {len(ts)} results at k = {k}"
    tied = np.flatnonzero(bits(np.where(np.isfinite(s), s, -1.0)) == bits(ts[-1]))
    listed = ti[bits(ts) == bits(ts[-1])]
    return len(tied), len(listed), np.array_equal(listed, tied[:len(listed)])


# ------------------------------------------------------------------------------------------- every case
def test_every_case_is_registered_and_non_empty():
    want = {"saturate", "tf_ladder", "idf_spread", "conj_values", "stage_b_wins", "stage_b_skipped", "stage_b_tie",
            "slice_ties", "slice_saturate"} | {f"k1b-{k1}-{b}" for k1, b in BC.K1B}
    assert set(BC.CASES) == want
    for case in BC.CASES.values():
        c = case.corpus
        assert len(case.rows) >= 2, case.name
        S, I, cnt = case.expected()
        assert S.shape == (len(c.queries), BC.K_MAX) and not S.flags.writeable and not I.flags.writeable
        # every list is sorted (score desc, id asc) and padded with -1
        for p in case.rows:
            n = cnt[p]
            assert np.all(I[p, n:] == -1) and np.all(I[p, :n] >= 0)
            s, i = S[p, :n], I[p, :n]
            assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (i[:-1] < i[1:])))


def test_corpus_sizes_and_probed_terms():
    for name in BC.BUILDERS:
        c = BC.corpus(name)
        assert c.n == (BC.N_SLICED if name == "sliced" else BC.N_SMALL)
        assert c.has_row.any() and ((~c.has_row).any() or name == "sliced")   # (sliced: every term has rows)
        # a term with rows is probed for certain (bm25_plan_kernel may walk one held by < 1/64 of the docs)
        assert np.all(c.df[c.has_row] * 64 >= c.n), name
        tot = np.array([c.df[c.terms_of(p)].sum() for p in range(len(c.queries))])
        if name == "sliced":
            assert np.all(tot > BC.BM_TARGET0), "every sliced query has more than one slice's postings"
            assert c.n / BC.WW_TARGET_MAX > 8, "the waves cut a list into many slices"
        else:
            assert np.all(tot <= 8192), "a query of the small corpora is at most one slice (BM_TARGET_MIN)"


# --------------------------------------------------------------------------------------------- saturate
def test_saturate_clips_the_quantiser():
    c = BC.corpus("values")
    _, _, x = BC.impacts(c, *BC.DEFAULT)
    sat_terms = [c.term[f"{g}{j}"] for g in "SP" for j in range(8)]
    of_sat = np.isin(c.post_term, sat_terms)
    clip = BC.clipped(x)
    assert (clip & of_sat).sum() > 500, "saturated postings"
    # the last unclipped steps and the near-zero end stand beside them, in the same lists
    assert ((x > 253.0) & (x < 254.0) & of_sat).sum() > 100 and ((x > 252.0) & (x < 253.0) & of_sat).sum() > 100
    assert ((x < 0.05) & of_sat).sum() > 300
    for t in sat_terms:
        xs = x[c.rowptr[t]:c.rowptr[t + 1]]
        assert (xs > 254).any() and ((xs > 252) & (xs < 254)).any() and (xs < 0.05).any(), t
    q = BC.quantised(x)
    assert q[clip].min() == 255 and q[x < 0.05].max() == 2
    # eight saturated terms in one doc: the largest sum an accumulator takes
    for group in "SP":
        m = np.ones(c.n, dtype=bool)
        for j in range(8):
            t = c.term[f"{group}{j}"]
            sat = np.zeros(c.n, dtype=bool)
            lo, hi = c.rowptr[t], c.rowptr[t + 1]
            sat[c.post_doc[lo:hi][clip[lo:hi]]] = True
            m &= sat
        assert m.sum() >= 30, f"docs that hold all eight {group} terms clipped"
    # the saturated scores differ in their low bits: the top of a list is decided by the arithmetic, not by ids alone
    S, _, cnt = BC.CASES["saturate"].expected()
    for p in c.rows("saturate"):
        top = S[p, :10]
        assert cnt[p] >= 128 and len(np.unique(top)) >= 5, c.qname[p]


def test_k1_zero_clips_every_posting():
    c = BC.corpus("values")
    imp, con, x = BC.impacts(c, 0.0, 0.75)
    assert np.all(BC.clipped(x)) and np.all(imp == 1.0)
    assert np.array_equal(bits(con), bits(c.idf[c.post_term])), "at k1 = 0 every contribution is the idf itself"
    for k1, b in BC.K1B[2:]:
        _, _, x = BC.impacts(c, k1, b)
        assert BC.clipped(x).any() and (~BC.clipped(x)).any()


# -------------------------------------------------------------------------------------------------- k1b
def test_k1b_ties_at_k1_zero():
    c = BC.corpus("values")
    p = c.row("W")
    s = BC.all_scores(c, p, 0.0, 0.75)
    w = c.term["W"]
    assert c.df[w] > c.n / 2
    assert np.all(bits(s[np.isfinite(s)]) == bits(c.idf[w])) and np.isfinite(s).sum() == c.df[w]
    for k in BC.KS:
        tied, listed, lowest = boundary(c, p, k, 0.0, 0.75)
        assert tied == c.df[w] > c.n / 2 and listed == k and lowest
    # the four parameter sets give four different rankings of the same rows
    lists = {BC.expected("values", k1, b)[1][c.row("S8"), :10].tobytes() for k1, b in BC.K1B}
    assert len(lists) >= 3


# -------------------------------------------------------------------------------------------- tf_ladder
def test_tf_ladder_terms():
    c = BC.corpus("values")
    L, L2, L3 = c.term["L"], c.term["L2"], c.term["L3"]
    need = c.share * c.n
    assert c.df[L] >= need and c.max_tf[L] == 65535 and c.has_row[L]
    assert c.df[L2] >= need and c.max_tf[L2] == 65536 and not c.has_row[L2]
    assert c.max_tf[L3] == 2 ** 31 - 1 and not c.has_row[L3] and 2 ** 24 in c.tf_of("L3")
    ladder = np.arange(BC.LADDER0, BC.LADDER0 + len(BC.LADDER_TF))
    at = np.searchsorted(c.docs_of("L"), ladder)
    assert np.array_equal(c.docs_of("L")[at], ladder) and tuple(c.tf_of("L")[at]) == BC.LADDER_TF
    assert np.array_equal(c.docs_of("L"), c.docs_of("L2")) and (c.tf_of("L") != c.tf_of("L2")).sum() == 1
    # the ladder docs ARE the top of the list, each with its own score: a frequency read with the wrong
    # sign or width changes the result
    S, I, _ = BC.CASES["tf_ladder"].expected()
    for name in ("L", "L2"):
        p = c.row(name)
        assert set(ladder) <= set(I[p, :10]) and len(np.unique(S[p, :8])) == 8, name
    assert {BC.LADDER0 + 10, BC.LADDER0 + 11} <= set(I[c.row("L3"), :10])
    # queried with a rare term, the row term is probed in stage A on docs of the ladder's upper half
    rare = set(c.docs_of("RARE"))
    assert {BC.LADDER0 + 3, BC.LADDER0 + 5, BC.LADDER0 + 6} <= rare and not c.has_row[c.term["RARE"]]
    assert set(I[c.row("RARE+L"), :3]) <= rare


# ------------------------------------------------------------------------------------------- idf_spread
def test_idf_spread_values():
    c = BC.corpus("values")
    assert 2.3e-10 < BC.IDF_TINY < 2.4e-10 and BC.IDF_TINY == np.log(1.0 + 0.5 / (2.0 ** 31 + 0.5))
    idf = {name: c.idf[t] for name, t in c.term.items()}
    assert idf["T_TINY"] == idf["PT_TINY"] == BC.IDF_TINY and idf["T_ZERO"] == idf["PT_ZERO"] == 0.0
    assert idf["T_HUGE"] == idf["PT_HUGE"] == 30.0 and idf["T_MIN"] == idf["PT_MIN"] == BC.IDF_MIN == 1e-300
    for name in ("TINY", "ZERO", "HUGE", "MIN"):
        assert c.has_row[c.term["PT_" + name]] and not c.has_row[c.term["T_" + name]]
    assert len({idf[f"E{j}"] for j in range(8)}) == 1
    assert len(set(c.terms_of(c.row("same8")))) == 1 and len(c.terms_of(c.row("same8"))) == 8
    S, I, cnt = BC.CASES["idf_spread"].expected()
    # all-zero idfs: every doc that holds a term is a result with score +0.0, and the lowest ids hold
    # only the term with rows -- the sweep supplies them although its bound equals the threshold, 0.0 == 0.0
    p = c.row("all_zero")
    assert np.all(bits(S[p]) == 0) and cnt[p] == BC.K_MAX
    walked, probed = np.isin(I[p, :10], c.docs_of("T_ZERO")), np.isin(I[p, :10], c.docs_of("PT_ZERO"))
    assert probed[0] and not walked[0] and walked.any() and (probed & ~walked).sum() >= 3
    assert len(c.docs_of("T_ZERO")) >= 100        # (stage A alone fills a list of 10 or 65: it has a threshold)
    # the smallest allowed idf still separates docs: the scores are not all equal
    for name in ("min", "row_min"):
        assert len(np.unique(S[c.row(name), :20])) >= 2 and 0.0 < S[c.row(name), 0] < 3e-300
    assert cnt[c.row("empty")] == 0
    # 248 / (idf * (k1 + 1) / 255) is finite at the bound for every k1 >= 0 (the unit is smallest at k1 = 0)
    with np.errstate(over="raise"):
        assert np.isfinite(248.0 / (BC.IDF_MIN * (1.0 / 255.0)))


# ---------------------------------------------------------------------------------------------- stage B
def test_stage_b_cases():
    c = BC.corpus("stageb")
    S, I, cnt = BC.expected("stageb")
    tub, _ = BC.bounds(c, *BC.DEFAULT)
    for t in ("D", "D2", "PZ"):
        assert c.has_row[c.term[t]]
    for t in ("R", "R2", "R0"):
        assert not c.has_row[c.term[t]] and c.df[c.term[t]] >= 100
    R, R2 = holds(c, "R"), holds(c, "R2")
    for p in c.rows("stage_b_wins"):
        for k in BC.KS:
            assert cnt[p] >= k and not R[I[p, :k]].any(), "the sweep supplies every result"
        # ... and stage A, on its own, has a k-th score far below the probed bound: the sweep cannot be skipped
        s = BC.all_scores(c, p)
        assert np.sort(s[R])[-10] * 1000 < tub[c.term["D"]]
    for p in c.rows("stage_b_skipped"):
        for k in (10, 65):
            assert R2[I[p, :k]].all()
            assert tub[c.term["D"]] * 1.01 < S[p, k - 1], "D's bound lies clearly below stage A's k-th score"
    for name, probed in (("R0+D2", "D2"), ("D2+R0", "D2"), ("R0+PZ", "PZ")):
        p = c.row(name)
        stage_a = holds(c, "R0")
        for k in BC.KS:
            # stage A (the docs of R0) has k docs at the k-th score -- for k up to 100 --, which is the probed
            # term's bound to the bit
            s = BC.all_scores(c, p)
            a = np.sort(s[stage_a])[::-1]
            assert bits(tub[c.term[probed]]) == bits(S[p, k - 1])
            assert k > 100 or bits(a[k - 1]) == bits(S[p, k - 1])
            tied, listed, lowest = boundary(c, p, k)
            assert tied > listed and lowest
        # the lower ids hold the probed term alone: the sweep supplies the first hundred
        assert not stage_a[I[p, :100]].any() and (bits(s[stage_a]) == bits(S[p, 0])).sum() >= 100 and I[p, 0] < BC.TIE_LOW[1]


# ------------------------------------------------------------------------------------------- slice_ties
def test_slice_ties():
    c = BC.corpus("sliced")
    S, I, cnt = BC.expected("sliced")
    assert len(c.rows("slice_ties")) == 10
    for p in c.rows("slice_ties"):
        for k in BC.SLICE_KS:
            tied, listed, lowest = boundary(c, p, k)
            assert tied > listed >= 1 and lowest, f"{c.qname[p]} k={k}: {tied} tied, {listed} listed"
        if c.qcoll[p] == 1:
            assert np.all(I[p] % BC.KEEP_EVERY == 0)
    assert np.array_equal(I[c.row("all")], np.arange(BC.K_MAX))
    assert np.array_equal(I[c.row("all/filtered")], np.arange(BC.K_MAX) * BC.KEEP_EVERY)
    assert np.array_equal(I[c.row("last")], BC.LAST_FROM + np.arange(BC.K_MAX))       # only the last slice's docs
    assert np.array_equal(I[c.row("spread")], np.arange(BC.K_MAX) * BC.SPREAD_EVERY)  # one per 250 docs
    # LAST_FROM lies in the last slice of every cut: 128 slices (the most) of 40000 docs are 312 docs each
    assert c.n - BC.LAST_FROM < c.n // 128 and c.n - BC.LAST_FROM > BC.K_MAX
    assert BC.SPREAD_EVERY < c.n // 128 and c.n // BC.SPREAD_EVERY > BC.K_MAX


def test_slice_saturate():
    c = BC.corpus("sliced")
    _, _, x = BC.impacts(c, *BC.DEFAULT)
    S, I, cnt = BC.expected("sliced")
    for j in range(8):
        t = c.term[f"SAT{j}"]
        assert c.df[t] == c.n and c.has_row[t] and np.all(BC.clipped(x[c.rowptr[t]:c.rowptr[t + 1]]))
    assert len(c.rows("slice_saturate")) == 4
    for p in c.rows("slice_saturate"):
        assert cnt[p] == BC.K_MAX and len(np.unique(S[p, :65])) >= 30, c.qname[p]   # decided by the arithmetic (and pairs of equal tf by the id)
    assert len(set(I[c.row("sat8"), :65] // 8192)) >= 4, "the best docs lie in several slices"


# ------------------------------------------------------------------------------------------ conj_values
def test_conj_values():
    c = BC.corpus("values")
    S, I, cnt = BC.CASES["conj_values"].expected()
    So, Io, _ = BC.expected("values")
    differ = 0
    for p in BC.CASES["conj_values"].rows:
        t = c.terms_of(p)
        every = np.ones(c.n, dtype=bool)
        for name, tid in c.term.items():
            if tid in t:
                every &= holds(c, name)
        assert cnt[p] == min(BC.K_MAX, every.sum()) and every[I[p, :cnt[p]]].all(), c.qname[p]
        differ += not np.array_equal(I[p], Io[p])
    assert differ >= 6, "the AND form changes most multi-term lists"
    assert cnt[c.row("S8")] >= 100 and cnt[c.row("P8")] == BC.K_MAX


# ------------------------------------------------------------------------------ the input contract (a3)
def test_check_params():
    torch = pytest.importorskip("torch")
    from triple_hybrid_rag_amd import _native as N
    good = torch.tensor([0.0, BC.IDF_MIN, BC.IDF_TINY, 1.0, 30.0], dtype=torch.float64)
    N.bm25_check_params(good, 100.0, 1.2, 0.75)
    N.bm25_check_params(good, 1e-3, 0.0, 0.0)
    N.bm25_check_params(good.numpy(), 2000.0, 100.0, 1.0)
    N.bm25_check_params(BC.corpus("values").idf, 2000.0)          # (a read-only numpy array)
    assert N.BM25_IDF_MIN == BC.IDF_MIN

    def refused(idf, avgdl=100.0, k1=1.2, b=0.75):
        with pytest.raises(N.NativeError) as e:
            N.bm25_check_params(torch.tensor(idf, dtype=torch.float64), avgdl, k1, b)
        return str(e.value)

    assert "idf[1] = -0.125" in refused([1.0, -0.125, 2.0])        # Robertson's idf above df = N / 2
    assert "idf[2] = nan" in refused([1.0, 2.0, float("nan")])
    assert "idf[0] = inf" in refused([float("inf"), 2.0])
    assert "idf[3] = 1e-301" in refused([0.0, 1.0, 1e-300, 1e-301])
    assert "idf[0] = 5e-324" in refused([5e-324])
    assert "k1 = -0.5" in refused([1.0], k1=-0.5)
    assert "b = 1.5" in refused([1.0], b=1.5)
    assert "b = -0.1" in refused([1.0], b=-0.1)
    assert "avgdl = 0.0" in refused([1.0], avgdl=0.0)
    assert "avgdl = nan" in refused([1.0], avgdl=float("nan"))
    assert "k1 = inf" in refused([1.0], k1=float("inf"))
