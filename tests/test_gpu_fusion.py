"""The fusion tail on the device against the CPU oracle, on the built cases of tests/fusion_cases.py
(what each case is aimed at is asserted on the CPU by tests/test_fusion_cases_host.py):
thr_rrf_fuse, thr_rrf_fuse_standalone (``fuse`` and ``fuse_two_channels``), thr_fuse_post,
thr_rerank_order and both kernels of thr_merge_topk.

Every comparison is bit for bit: ids, ranks and counts as integers, float64 scores through their
int64 view.  The one exception is thr_rerank_order's score output, compared with ``==`` on Python
floats: the reference sorts on ``rerank_score or 0``, which yields the int 0 for -0.0, so the sign
of a zero has no counterpart there.  No tolerances.  NaN is left out (as a fusion score and as a
rerank score: the reference's sort on NaN is not an order); nothing else is."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fusion_cases as F  # noqa: E402

from oracle import thr_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def N():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T._native


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def same(a, b):
    """Two device outputs (or rows of them) equal, float64 by bits."""
    return np.array_equal(bits(a), bits(b)) if a.dtype == np.float64 else np.array_equal(a, b)


# ------------------------------------------------------------------------------------------ RRF
def run_rrf(N, flavour, chans, w, top_k, rrf_k=60):
    """chans: three numpy arrays or None -> numpy (ids, scores, ranks, counts)."""
    lex, sem, gra = (dev(c) for c in chans)
    if flavour == "rag2":
        out = N.rrf_fuse(lex, sem, gra, top_k, w[0], w[1], w[2], rrf_k, want_ranks=True)
    else:
        two = flavour == "two"
        out = N.rrf_fuse_standalone(lex, sem, None if two else gra, top_k, w[0], w[1], w[2],
                                    two_channels=two, want_ranks=True)
    return [o.cpu().numpy() for o in out]


def check_rrf_row(got, q, exp, what):
    """Row q of a device result against the oracle's (ids, scores, ranks, count): everything inside
    the count, and the padding past it."""
    ids, sc, rk, cnt = got
    ei, es, er, n = exp
    assert int(cnt[q]) == n, f"{what}: count {cnt[q]} != {n}"
    assert ids[q, :n].tolist() == ei, f"{what}: ids"
    assert np.array_equal(bits(sc[q, :n]), bits(es)), f"{what}: scores (bits)"
    assert rk[q, :n].tolist() == [list(r) for r in er], f"{what}: ranks"
    assert np.all(ids[q, n:] == -1) and np.all(np.isneginf(sc[q, n:])) and not rk[q, n:].any(), f"{what}: padding"


def row_chans(rows, nm, flavour):
    lex, sem, gra = rows[nm]
    return lex, sem, (None if flavour == "two" else gra)


@pytest.mark.parametrize("flavour,wname,rrf_k,top_k", F.rrf_calls())
def test_rrf_built_rows_match_the_oracle(N, flavour, wname, rrf_k, top_k):
    """All built rows in ONE call; the same rows shuffled; a sample of them as nq = 1 calls."""
    rows = F.rrf_rows()
    names = list(rows)
    w = F.WEIGHT_SETS[wname]
    got = run_rrf(N, flavour, F.rrf_batch(rows, names), w, top_k, rrf_k)
    for q, nm in enumerate(names):
        check_rrf_row(got, q, F.rrf_expect(flavour, *row_chans(rows, nm, flavour), w, top_k, rrf_k),
                      f"{flavour}/{wname}/k={rrf_k}/top_k={top_k}/{nm}")
    perm = np.random.default_rng(5).permutation(len(names))
    shuf = run_rrf(N, flavour, F.rrf_batch(rows, [names[p] for p in perm]), w, top_k, rrf_k)
    for j, p in enumerate(perm):
        assert all(same(a[p], b[j]) for a, b in zip(got, shuf)), f"shuffled: {names[p]}"
    for nm in ("cap_disjoint", "wave_63_64", "dup_128", "tie_cycles", "all_empty", "ids_extreme"):
        one = run_rrf(N, flavour, F.rrf_batch(rows, [nm]), w, top_k, rrf_k)
        q = names.index(nm)
        assert all(same(a[q], b[0]) for a, b in zip(got, one)), f"nq=1: {nm}"


@pytest.mark.parametrize("flavour", ["rag2", "standalone", "two"])
def test_rrf_widths_and_absent_channels(N, flavour):
    """Channel widths 1, 37 and 128, and a channel passed as None against the same channel passed
    with width 1 holding only -1."""
    rows = F.rrf_rows()
    w = F.W_DEFAULT
    for width, names in ((1, ["width_1", "all_empty"]), (37, ["width_37", "width_1", "interior_minus1"]),
                         (128, ["cap_disjoint", "width_37"])):
        got = run_rrf(N, flavour, F.rrf_batch(rows, names, width), w, F.SLOTS)
        for q, nm in enumerate(names):
            check_rrf_row(got, q, F.rrf_expect(flavour, *row_chans(rows, nm, flavour), w, F.SLOTS), f"{flavour}/w{width}/{nm}")
    names = ["cap_disjoint", "dup_ends", "tie_pairs", "minus1_first"]
    lex, sem, gra = F.rrf_batch(rows, names)
    empty = np.full((len(names), 1), -1, dtype=np.int64)
    slots = (0, 1) if flavour == "two" else (0, 1, 2)
    for absent in slots:
        with_none, with_empty = [lex, sem, gra], [lex, sem, gra]
        with_none[absent], with_empty[absent] = None, empty
        a = run_rrf(N, flavour, with_none, w, F.SLOTS)
        b = run_rrf(N, flavour, with_empty, w, F.SLOTS)
        assert all(same(x, y) for x, y in zip(a, b)), f"{flavour}: None against an empty channel {absent}"
        for q, nm in enumerate(names):
            ch = list(row_chans(rows, nm, flavour))
            ch[absent] = None
            check_rrf_row(a, q, F.rrf_expect(flavour, *ch, w, F.SLOTS), f"{flavour}/absent{absent}/{nm}")


@pytest.mark.parametrize("flavour", ["rag2", "standalone", "two"])
@pytest.mark.parametrize("weight", [0.8, 0.0, -0.5])
def test_one_channel_shortcut_on_a_probe_chain_that_wraps(N, flavour, weight):
    """128 ids that start at one table slot >= 500 (the chain wraps past 511): no duplicate -> the
    list is written straight out; a duplicate of the first id at the end, and an adjacent pair in the
    middle -> the general path merges the occurrences.  Every slot the flavour has."""
    chain, _ = F.shortcut_rows()
    for slot in ((0, 1) if flavour == "two" else (0, 1, 2)):
        w = [0.7, 0.9, 1.1]
        w[slot] = weight
        chans = [None, None, None]
        chans[slot] = chain
        got = run_rrf(N, flavour, chans, w, F.SLOTS)
        for q in range(chain.shape[0]):
            ch = [None, None, None]
            ch[slot] = chain[q].tolist()
            check_rrf_row(got, q, F.rrf_expect(flavour, *ch, w, F.SLOTS), f"{flavour}/slot{slot}/w={weight}/row{q}")


def test_rrf_k_is_refused_where_k_plus_rank_would_overflow(N):
    """rrf_k = INT_MAX - 128 is the last value taken (and is right: see rrf_calls); one more is
    THR_ERR_INVALID, as is a negative one.  top_k above the 512 rows is refused by the wrapper."""
    ids = dev(np.arange(8, dtype=np.int64)[None])
    out = N.rrf_fuse(None, ids, None, 8, rrf_k=F.RRF_K_MAX, want_ranks=True)
    assert out[0].cpu().numpy()[0].tolist() == list(range(8))
    assert out[1].cpu().numpy()[0].tolist() == [0.0 + 0.8 / (F.RRF_K_MAX + r) for r in range(1, 9)]
    for bad in (F.RRF_K_MAX + 1, 2 ** 31 - 1, -1):
        with pytest.raises(N.NativeError, match="invalid"):
            N.rrf_fuse(None, ids, None, 8, rrf_k=bad)
    with pytest.raises(N.NativeError, match="512"):
        N.rrf_fuse(None, ids, None, 513)


# ------------------------------------------------------------------------------------- fuse_post
def run_post(N, c):
    oi, os_, oc = N.fuse_post(dev(c.ids), dev(c.scores), dev(c.ranks), dev(c.counts),
                              tuple(dev(x) for x in c.channel_scores), c.safety, c.quantile,
                              c.normalize, c.top_k)
    return oi.cpu().numpy(), os_.cpu().numpy(), oc.cpu().numpy()


def check_post(N, c):
    oi, os_, oc = run_post(N, c)
    for q, nm in enumerate(c.row_names):
        ei, es = c.expect(q)
        m = len(ei)
        what = f"{c.name}/{nm}"
        assert int(oc[q]) == m, f"{what}: count {oc[q]} != {m}"
        assert oi[q, :m].tolist() == ei, f"{what}: ids"
        assert np.array_equal(bits(os_[q, :m]), bits(es)), f"{what}: scores (bits)"
        assert np.all(oi[q, m:] == -1) and np.all(np.isneginf(os_[q, m:])), f"{what}: padding"


def test_fuse_post_sizes_and_counts(N):
    for c in F.post_size_calls():
        check_post(N, c)


def test_fuse_post_safety_threshold(N):
    for c in F.post_safety_calls():
        check_post(N, c)


def test_fuse_post_top_k_and_normalise(N):
    for c in F.post_topk_norm_calls():
        check_post(N, c)


def test_fuse_post_percentile_sweep(N):
    """One launch per alpha; every m through ``counts``; strict, plateau and widely spaced scores."""
    for alpha in F.ALPHAS:
        check_post(N, F.post_sweep_call(alpha))


@pytest.mark.parametrize("safety,alpha,top_k,normalize", [(F.SAFETY, 0.6, 10, False), (0.0, None, None, True),
                                                          (0.25, 0.9, None, True)])
def test_fuse_batch_end_to_end(N, safety, alpha, top_k, normalize):
    """RRFFusion.fuse_batch over the RRF rows with synthetic channel scores against
    standalone_fuse_ids followed by fuse_post_rows."""
    from triple_hybrid_rag_amd.config import RAGConfig
    from triple_hybrid_rag_amd.core.fusion import RRFFusion
    rows = F.rrf_rows()
    names = list(rows)
    chans = F.rrf_batch(rows, names)
    cs = F.channel_scores_for(chans)
    fus = RRFFusion(RAGConfig(rag_safety_threshold=safety, rag_denoise_enabled=alpha is not None,
                              rag_denoise_alpha=alpha if alpha is not None else 0.6))
    for wname, w in F.WEIGHT_SETS.items():
        wd = dict(zip(F.NAMES, w))
        oi, os_, oc = fus.fuse_batch(*(dev(c) for c in chans), *(dev(c) for c in cs), weights=wd, top_k=top_k,
                                     normalize=normalize)
        oi, os_, oc = oi.cpu().numpy(), os_.cpu().numpy(), oc.cpu().numpy()
        for q, nm in enumerate(names):
            ids, sc, rk = O.standalone_fuse_ids(*(F.cut(c) for c in rows[nm]), wd)
            ei, es = O.fuse_post_rows(ids, sc, rk, [c[q].tolist() for c in cs], safety, alpha, top_k, normalize)
            m = len(ei)
            what = f"{wname}/{nm}"
            assert int(oc[q]) == m and oi[q, :m].tolist() == ei, f"{what}: ids"
            assert np.array_equal(bits(os_[q, :m]), bits(es)), f"{what}: scores (bits)"
            assert np.all(oi[q, m:] == -1) and np.all(np.isneginf(os_[q, m:])), f"{what}: padding"


# ---------------------------------------------------------------------------------- rerank_order
@pytest.mark.parametrize("n", F.RERANK_SIZES)
def test_rerank_order_built_rows(N, n):
    for n_lists in F.RERANK_LISTS:
        sc, ids, vals, names = F.rerank_case(n, n_lists)
        for counts in (None, F.rerank_counts(n, len(names)), np.full(len(names), n, dtype=np.int32),
                       np.zeros(len(names), dtype=np.int32), np.full(len(names), n + 7, dtype=np.int32)):
            for top_k in sorted({1, n}):
                oi, os_, oc = (o.cpu().numpy() for o in N.rerank_order(dev(sc), dev(ids), dev(counts), top_k))
                for q, nm in enumerate(names):
                    ei, es = F.rerank_expect(vals[q], ids[q], n if counts is None else int(counts[q]), top_k)
                    m = len(ei)
                    what = f"n={n}/lists={n_lists}/top_k={top_k}/{nm}"
                    assert int(oc[q]) == m and oi[q, :m].tolist() == ei, f"{what}: ids"
                    assert os_[q, :m].tolist() == es, f"{what}: scores"     # ==: the sign of a zero is not compared
                    assert np.all(oi[q, m:] == -1) and np.all(np.isneginf(os_[q, m:])), f"{what}: padding"


# ------------------------------------------------------------------------------------ merge_topk
def check_merge(S, I, names, out, k_out, what):
    s, i, cnt = (o.cpu().numpy() for o in out)
    for q, nm in enumerate(names):
        es, ei = F.merge_expect(S[:, q], I[:, q], k_out)
        m = len(es)
        assert int(cnt[q]) == m, f"{what}/{nm}: count {cnt[q]} != {m}"
        assert np.array_equal(i[q, :m], ei), f"{what}/{nm}: ids"
        assert np.array_equal(bits(s[q, :m]), bits(es)), f"{what}/{nm}: scores (bits)"
        assert np.all(i[q, m:] == -1) and np.all(np.isneginf(s[q, m:])), f"{what}/{nm}: padding"


@pytest.mark.parametrize("G,k", F.MERGE_SHAPES)
@pytest.mark.parametrize("k_out", F.MERGE_K_OUT)
def test_merge_topk_built_rows(N, G, k, k_out):
    """The same value families at 1024 candidates (the ranked-lists kernel) and at 1025 (the general
    one): each must agree with topk_desc, duplicates and signed zeros included."""
    S, I, names = F.merge_case(G, k)
    check_merge(S, I, names, N.merge_topk(dev(S), dev(I), k_out), k_out, f"{G}x{k}/k_out={k_out}")


@pytest.mark.parametrize("G,k", F.MERGE_SHAPES[:2])
def test_merge_topk_reads_a_gathered_tile_in_place(N, G, k):
    S, I, names = F.merge_case(G, k)
    tile = torch.stack([dev(S).view(torch.int64), dev(I)], dim=1).contiguous()       # [G, 2, nq, k]
    out = N.merge_topk(tile[:, 0].view(torch.float64), tile[:, 1], 10)
    check_merge(S, I, names, out, 10, f"tile {G}x{k}")


def test_merge_topk_refuses_k_out_above_512(N):
    S, I, _ = F.merge_case(8, 128)
    with pytest.raises(N.NativeError, match="invalid"):
        N.merge_topk(dev(S), dev(I), 513)
    assert int(N.merge_topk(dev(S), dev(I), 512)[2][0]) == 512
