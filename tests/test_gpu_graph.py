"""The graph channel against the oracle, case by case (tests/graph_cases.py; what each case promises
is proven without a GPU by tests/test_graph_cases_host.py): thr_graph_topk with and without the
transposed mention CSR, GpuIndex.graph_search and thr_graph_topk_scoped, in all three capacity tiers,
on the whole corpus and on an interior shard.  Every comparison is bit for bit: ids, scores, counts
and the (-inf, -1) padding."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import graph_cases as GC  # noqa: E402

CERTIFIED, OVERFLOW, EXACT = 1, 2, 4


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_rows(res, expected, what, only=None):
    S, I, cnt = (t.cpu().numpy() for t in res[:3])
    for q, (es, ei) in enumerate(expected):
        if only is not None and not only[q]:
            continue
        m = len(ei)
        assert cnt[q] == m, f"{what} q{q}: count {cnt[q]} != {m}"
        assert np.array_equal(I[q, :m], ei), f"{what} q{q}: ids differ: {I[q, :m]} != {ei}"
        assert np.array_equal(S[q, :m].view(np.uint64), es.view(np.uint64)), f"{what} q{q}: scores differ (bits)"
        assert np.all(I[q, m:] == -1) and np.all(np.isneginf(S[q, m:])), f"{what} q{q}: padding"


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{what} differs"


def labellings(case):
    """The scoped runs of a case -> [(what, doc_label, query_label)]: real labels with one that no
    chunk carries, -1 and real labels mixed in one batch, and nothing but the absent label."""
    doc = case.doc_label if case.doc_label is not None else GC.chunk_labels(case.window)
    q = np.arange(case.nq)
    real = (q % 3).astype(np.int32) if case.query_label is None else case.query_label.copy()
    absent = real.copy()
    absent[-1] = 99
    mixed = np.where(q % 2 == 0, -1, real).astype(np.int32)
    if case.nq > 2:
        mixed[-2] = 99
    return [("labels", doc, real), ("labels+absent", doc, absent), ("mixed", doc, mixed),
            ("absent", doc, np.full(case.nq, 99, dtype=np.int32))]


@pytest.mark.parametrize("name,tier,wname", GC.variants(), ids=["/".join(v) for v in GC.variants()])
def test_graph_case_equals_the_oracle(T, name, tier, wname):
    N = T._native
    case = GC.build(name, wname, tier)
    what = f"{name}/{tier}/{wname}"
    base, n = case.window
    k, hops = case.k, case.hops
    exp = GC.expected(case, wname)
    beyond = GC.beyond_full(case)
    idx = T.GpuIndex(doc_base=base)
    idx.n_docs = n
    idx.set_graph(*case.g)
    G = idx.graph
    args = (G["ent_rowptr"], G["ent_col"], G["men_rowptr"], G["men_chunk"], G["men_conf"], dev(case.seeds))

    # 1. without the transposed CSR: the flags name the queries beyond the full capacities, the rest is exact
    res = N.graph_topk(*args, hops, k, base, n)
    flg = res[3].cpu().numpy()
    assert list(flg) == [OVERFLOW if b else CERTIFIED for b in beyond], f"{what}: flags {flg} vs beyond-full {beyond}"
    assert_rows(res, exp, f"{what} on chip", only=~beyond)

    # 2. with it, and through GpuIndex: no overflow comes back, every query is the oracle's
    tr = idx._graph_transposed()
    full = N.graph_topk(*args, hops, k, base, n, transposed=tr)
    flg = full[3].cpu().numpy()
    assert not (flg & OVERFLOW).any(), f"{what}: overflow with the transposed CSR: {flg}"
    assert list(flg) == [CERTIFIED | EXACT if b else CERTIFIED for b in beyond], f"{what}: flags {flg}"
    assert_rows(full, exp, f"{what} three tiers")
    assert_rows(idx.graph_search(dev(case.seeds), k, hops), exp, f"{what} graph_search")

    # 3. scoped: no label is the unscoped call; labels are the masked oracle
    free = N.graph_topk_scoped(*args, hops, k, base, n, dev(GC.chunk_labels(case.window)),
                               dev(np.full(case.nq, -1, dtype=np.int32)), transposed=tr)
    assert not (free[3].cpu().numpy() & OVERFLOW).any()
    for j in range(3):
        same(free[j], full[j], f"{what} scoped without labels [{j}]")
    for lname, doc, ql in labellings(case):
        got = N.graph_topk_scoped(*args, hops, k, base, n, dev(doc), dev(ql), transposed=tr)
        assert not (got[3].cpu().numpy() & OVERFLOW).any(), f"{what} {lname}: overflow"
        e = GC.expected(case, wname, ql, doc)
        if lname == "absent":
            assert all(len(ei) == 0 for _, ei in e)
        assert_rows(got, e, f"{what} scoped {lname}")


@pytest.mark.parametrize("wname", list(GC.WINDOWS))
@pytest.mark.parametrize("kept", [GC.FULL_CON, GC.FULL_CON + 1])
def test_a_scope_that_keeps_exactly_the_capacity_stays_on_chip(T, kept, wname):
    """16 384 mentions of one entity: thr_graph_topk overflows; thr_graph_topk_scoped with a label that
    keeps 8192 of them is certified on chip, with 8193 it overflows (no transposed CSR in either call)."""
    N = T._native
    case = GC.build(f"scoped_mentions-{kept}", wname)
    base, n = case.window
    args = tuple(dev(a) for a in case.g) + (dev(case.seeds),)
    flg0 = N.graph_topk(*args, case.hops, case.k, base, n)[3].cpu().numpy()
    assert list(flg0) == [OVERFLOW, CERTIFIED, OVERFLOW]
    res = N.graph_topk_scoped(*args, case.hops, case.k, base, n, dev(case.doc_label), dev(case.query_label))
    flg = res[3].cpu().numpy()
    on_chip = kept <= GC.FULL_CON
    assert list(flg) == [CERTIFIED if on_chip else OVERFLOW, CERTIFIED, OVERFLOW]     # (query 2 has no label)
    exp = GC.expected(case, wname, case.query_label, case.doc_label)
    assert_rows(res, exp, f"scoped_mentions-{kept}/{wname}", only=np.array([on_chip, True, False]))


def test_refusals_before_any_result(T):
    """hops 9 is THR_ERR_INVALID; 17 seeds per query and k = 129 are refused by the host wrapper."""
    N = T._native
    case = GC.build("seeds_one", "whole")
    base, n = case.window
    g = tuple(dev(a) for a in case.g)
    labels = (dev(GC.chunk_labels(case.window)), dev(np.zeros(case.nq, dtype=np.int32)))
    seeds = dev(case.seeds)
    wide = dev(np.full((case.nq, GC.MAX_SEEDS + 1), 4, dtype=np.int32))
    for call, extra in ((N.graph_topk, ()), (N.graph_topk_scoped, labels)):
        with pytest.raises(N.NativeError, match=r"\(code -1\)"):
            call(*g, seeds, GC.MAX_HOPS + 1, 50, base, n, *extra)
        with pytest.raises(N.NativeError, match="too many seeds per query or k too large"):
            call(*g, wide, 2, 50, base, n, *extra)
        with pytest.raises(N.NativeError, match="too many seeds per query or k too large"):
            call(*g, seeds, 2, GC.TOPK_MAX + 1, base, n, *extra)
        ok = call(*g, seeds, GC.MAX_HOPS, GC.TOPK_MAX, base, n, *extra)      # the limits themselves are served
        assert ok[0].shape == (case.nq, GC.TOPK_MAX)
