"""The graph channel inside a scope: thr_graph_topk_scoped against the oracle's scores with the
out-of-scope chunks masked, GpuIndex.graph_search(scopes=) over groups of scopes, the three capacity
tiers, retrieve_batch(scope_graph=) and a mutated index -- every comparison bit for bit."""
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import thr_oracle as O  # noqa: E402


def _scope_tests():
    """tests/test_gpu_scope.py as a module: its make_index and MIXED are this file's fixture too."""
    spec = importlib.util.spec_from_file_location(
        "_thr_test_gpu_scope", os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_scope.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SC = _scope_tests()
MIXED, make_index, dev, same = SC.MIXED, SC.make_index, SC.dev, SC.same


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def scope_mask(cols, sc, n):
    m = np.ones(n, dtype=bool)
    for name, v in (sc or {}).items():
        m &= cols[name] == v
    return m


def masked_topk(g, seeds, hops, n_chunks, k, mask, base=0):
    """The oracle's graph scores with the chunks outside ``mask`` (None = no filter) at -inf."""
    s = O.graph_scores(g[0], g[1], g[2], g[3], g[4], [int(x) for x in seeds], hops, n_chunks, base)
    if mask is not None:
        s = np.where(mask, s, -np.inf)
    ts, ti = O.topk_desc(s, k)
    return ts, ti + base


def assert_rows(res, expected, what):
    S, I, cnt = (t.cpu().numpy() for t in res[:3])
    for q, (es, ei) in enumerate(expected):
        m = len(ei)
        assert cnt[q] == m, f"{what} q{q}: count {cnt[q]} != {m}"
        assert np.array_equal(I[q, :m], ei), f"{what} q{q}: ids differ"
        assert np.array_equal(S[q, :m], es), f"{what} q{q}: scores differ (bits)"
        assert np.all(I[q, m:] == -1) and np.all(np.isneginf(S[q, m:])), f"{what} q{q}: padding"


def test_graph_search_scopes_equal_the_masked_oracle(T):
    from triple_hybrid_rag_amd import synth
    n, k, nq = 20000, 50, 24
    idx, _, cols, _ = make_index(T, n, 256, "exact")
    gs = synth.build_graph(n, 0, n)
    g = (gs.ent_rowptr, gs.ent_col, gs.men_rowptr, gs.men_chunk, gs.men_conf)
    idx.set_graph(*g)
    seeds = synth.graph_queries(nq, n, 3)
    scopes = [MIXED[i % len(MIXED)] for i in range(nq)]
    plan = idx.scope_plan(scopes, nq)
    assert len(plan.groups) >= 2          # overlapping scopes: more than one labelled call
    for hops in (0, 1, 2):
        exp = [masked_topk(g, seeds[i], hops, n, k, scope_mask(cols, scopes[i], n)) for i in range(nq)]
        free = [masked_topk(g, seeds[i], hops, n, k, None) for i in range(nq)]
        # a filter that does nothing fails here: some scoped list is not the unscoped one
        assert any(not np.array_equal(a[1], b[1]) for a, b in zip(exp, free))
        res = idx.graph_search(dev(seeds), k, hops, scopes=scopes)
        assert_rows(res, exp, f"scoped graph hops={hops}")
        by_plan = idx.graph_search(dev(seeds), k, hops, scopes=plan)
        plain = idx.graph_search(dev(seeds), k, hops)
        for j in range(3):
            same(res[j], by_plan[j], f"scopes vs plan [{j}]")
        for i, sc in enumerate(scopes):
            if not sc:                    # None and {}: the unscoped search's row
                for j in range(3):
                    same(res[j][i:i + 1], plain[j][i:i + 1], f"unscoped query {i} [{j}]")
        for i in range(nq):
            alone = idx.graph_search(dev(seeds[i:i + 1]), k, hops, scopes=[scopes[i]])
            for j in range(3):
                same(alone[j], res[j][i:i + 1].contiguous(), f"query {i} alone [{j}]")
    # one group of disjoint scopes: one call, the same rows
    tenants = [{"org": i % 4} for i in range(nq)]
    assert len(idx.scope_plan(tenants, nq).groups) == 1
    exp = [masked_topk(g, seeds[i], 2, n, k, scope_mask(cols, tenants[i], n)) for i in range(nq)]
    assert all(len(e[1]) for e in exp)    # every tenant's list is non-empty
    assert_rows(idx.graph_search(dev(seeds), k, 2, scopes=tenants), exp, "tenants")
    with pytest.raises(ValueError, match="unknown attribute"):
        idx.graph_search(dev(seeds[:1]), k, 2, scopes=[{"tenant": 1}])
    bare = T.GpuIndex()
    bare.n_docs = n
    bare.set_graph(*g)
    with pytest.raises(ValueError, match="unknown attribute"):     # (it has none)
        bare.graph_search(dev(seeds[:1]), k, 2, scopes=[{"org": 1}])


def hub_graph():
    """The graph of test_gpu_parity.py::test_graph_capacity_tiers, built with its seed."""
    rng = np.random.default_rng(9)
    n_ent, n_chunks = 20000, 50000
    deg = np.full(n_ent, 2, dtype=np.int64)
    deg[0], deg[1], deg[2] = 1200, 40, 6000           # hubs: medium, small-but-many-mentions, huge
    ent_rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ent_col = rng.integers(3, n_ent, ent_rowptr[-1]).astype(np.int32)
    ent_col[ent_rowptr[0]:ent_rowptr[1]] = rng.choice(np.arange(3, n_ent), 1200, replace=False)
    ent_col[ent_rowptr[2]:ent_rowptr[3]] = rng.choice(np.arange(3, n_ent), 6000, replace=False)
    men = np.full(n_ent, 1, dtype=np.int64)
    men[1] = 3000                                      # > 2048 contributions from one entity
    men[3] = 9000                                      # > 8192 contributions: beyond the full capacities
    men_rowptr = np.concatenate([[0], np.cumsum(men)]).astype(np.int64)
    men_chunk = rng.integers(0, n_chunks, men_rowptr[-1]).astype(np.int32)
    men_conf = rng.uniform(0.5, 1.0, men_rowptr[-1]).astype(np.float32)
    return (ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf), n_chunks


def test_scoped_graph_capacity_tiers(T):
    """A thin scope keeps a hub-seeded query on chip: of entity 3's 9000 mentions fewer than 2048 are
    in scope, so the filtered call reports no overflow where thr_graph_topk does; a query that reaches
    more than 4096 entities still takes the third tier.  Every tier gives the masked oracle's bits."""
    N = T._native
    g, n_chunks = hub_graph()
    label_of = (np.arange(n_chunks) % 8).astype(np.int32)          # eight tenants, chunk by chunk
    hub3 = g[3][g[2][3]:g[2][4]]
    assert (label_of[hub3] == 0).sum() < 2048 < 8192 < len(hub3)
    seeds = np.array([[0, -1, -1], [1, -1, -1], [2, -1, -1], [7, 8, 9], [3, 2, 5], [3, -1, -1], [3, -1, -1],
                      [1, -1, -1]], dtype=np.int32)
    qlabel = np.array([0, 1, 0, -1, 0, 0, 99, -1], dtype=np.int32)
    for lo, hi in ((0, n_chunks), (20000, 45000)):     # whole corpus / a document shard
        idx = T.GpuIndex(doc_base=lo)
        idx.n_docs = hi - lo
        idx.set_graph(*g)
        G = idx.graph
        labels = label_of[lo:hi]
        args = (G["ent_rowptr"], G["ent_col"], G["men_rowptr"], G["men_chunk"], G["men_conf"], dev(seeds))
        for hops in (0, 1, 2):
            exp = [masked_topk(g, seeds[q], hops, hi - lo, 50, None if qlabel[q] < 0 else labels == qlabel[q], lo)
                   for q in range(len(seeds))]
            assert len(exp[6][1]) == 0 and len(exp[5][1]) == 50
            # without the transposed CSR: the flags say which tier answered
            S, I, cnt, flg = N.graph_topk_scoped(*args, hops, 50, lo, hi - lo, dev(labels), dev(qlabel))
            _, _, _, flg0 = N.graph_topk(*args, hops, 50, lo, hi - lo)
            flg, flg0 = flg.cpu().numpy(), flg0.cpu().numpy()
            assert flg0[5] & 2 and flg0[6] & 2 and flg[5] == 1 and flg[6] == 1    # entity 3 alone: on chip in scope
            big = [2, 4] if hops >= 1 else []          # the 6000-edge hub: > 4096 entities
            assert all(flg[q] & 2 for q in big)
            if hops == 0:
                assert flg0[4] & 2 and flg[4] == 1     # (3, 2, 5) without a hop: entity 3's mentions only
            ok = [q for q in range(len(seeds)) if q not in big]
            assert all(flg[q] == 1 for q in ok)
            assert_rows((S[ok], I[ok], cnt[ok]), [exp[q] for q in ok], f"scoped tiers hops={hops} base={lo}")
            # with it (GpuIndex): the third tier answers the rest, no overflow comes back
            S, I, cnt, flg = N.graph_topk_scoped(*args, hops, 50, lo, hi - lo, dev(labels), dev(qlabel),
                                                 transposed=idx._graph_transposed())
            assert not (flg.cpu().numpy() & 2).any()
            assert all(int(flg[q]) == 5 for q in big)  # CERTIFIED | EXACT: the global-memory walk
            assert_rows((S, I, cnt), exp, f"scoped fallback hops={hops} base={lo}")


def test_retrieve_batch_scope_graph_isolates_every_channel(T):
    from triple_hybrid_rag_amd import synth
    n, k, nq = 20000, 10, 12
    idx, _, cols, csr = make_index(T, n, 768, "f16", lexical=True)
    gs = synth.build_graph(n, 0, n)
    idx.set_graph(gs.ent_rowptr, gs.ent_col, gs.men_rowptr, gs.men_chunk, gs.men_conf)
    q = dev(synth.dense_queries(nq, 768, n))
    qt = dev(synth.lexical_queries(nq, csr.df_local, 4))
    seeds = dev(synth.graph_queries(nq, n, 3))
    scopes = [{"org": i % 4} for i in range(nq)]
    res = idx.retrieve_batch(q, qt, seeds, top_k=k, scopes=scopes, scope_graph=True)
    ids = res.ids.cpu().numpy()
    for i in range(nq):
        for name in ("semantic", "lexical", "graph"):
            ch = res.channels[name][1][i].cpu().numpy()
            ch = ch[ch >= 0]
            assert ch.size and np.all(cols["org"][ch] == i % 4), f"{name} list of query {i} leaves its tenant"
        got = ids[i][ids[i] >= 0]
        assert got.size and np.all(cols["org"][got] == i % 4)
        exp, _ = O.fused_topk_ids(list(res.channels["lexical"][1][i].cpu().numpy()),
                                  list(res.channels["semantic"][1][i].cpu().numpy()),
                                  list(res.channels["graph"][1][i].cpu().numpy()), k)
        assert list(ids[i]) == exp
    scoped = idx.graph_search(seeds, 50, 2, scopes=scopes)
    for j in range(3):
        same(res.channels["graph"][j], scoped[j], f"graph channel vs graph_search(scopes=) [{j}]")
    # scope_graph=False: the documented default, the graph list of the whole shard
    loose = idx.retrieve_batch(q, qt, seeds, top_k=k, scopes=scopes)
    plain = idx.graph_search(seeds, 50, 2)
    for j in range(3):
        same(loose.channels["graph"][j], plain[j], f"unfiltered graph channel [{j}]")
    leak = loose.channels["graph"][1].cpu().numpy()
    assert any(np.any(cols["org"][r[r >= 0]] != i % 4) for i, r in enumerate(leak))   # what the flag is for
    # without scopes the flag changes nothing
    a = idx.retrieve_batch(q, qt, seeds, top_k=k, scope_graph=True)
    b = idx.retrieve_batch(q, qt, seeds, top_k=k)
    same(a.ids, b.ids, "scope_graph without scopes")
    same(a.scores, b.scores, "scope_graph without scopes: scores")


def _men_csr(me, mc, mw, n_ent):
    order = np.lexsort((mc, me))
    rp = np.concatenate([[0], np.cumsum(np.bincount(me, minlength=n_ent))]).astype(np.int64)
    return rp, mc[order].astype(np.int32), mw[order]


def test_scoped_graph_after_append_and_delete_equals_a_fresh_build(T):
    from triple_hybrid_rag_amd import synth
    n0, m, dim, n_ent, k, base = 5000, 1200, 256, 3000, 50, 700
    n = n0 + m
    rng = np.random.default_rng(23)
    x = synth.dense_rows(5, n, dim)
    org = rng.integers(0, 5, n).astype(np.int32)
    coll = rng.integers(0, 2, n).astype(np.int32)
    deg = rng.integers(1, 6, n_ent)
    ent_rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ent_col = rng.integers(0, n_ent, ent_rowptr[-1]).astype(np.int32)
    me = rng.integers(0, n_ent, 2 * n).astype(np.int64)
    me[: n // 2] = 3                                  # a hub entity
    mc = rng.integers(0, n, 2 * n).astype(np.int64)
    mw = rng.uniform(0.5, 1.0, 2 * n).astype(np.float32)

    def build(keep):
        rm = np.cumsum(keep) - 1
        sel = keep[mc]
        rp, c, w = _men_csr(me[sel], rm[mc[sel]].astype(np.int64) + base, mw[sel], n_ent)
        idx = T.GpuIndex(doc_base=base).set_dense(x[keep], shortlist="exact").set_collections(coll[keep])
        idx.set_attributes({"org": org[keep]})
        return idx.set_graph(ent_rowptr, ent_col, rp, c, w)

    first = np.arange(n) < n0
    idx = build(first)
    seeds = rng.integers(0, n_ent, (10, 3)).astype(np.int32)
    seeds[0] = [3, -1, -1]
    scopes = [{"org": i % 5, "collection": i % 2} if i % 3 else {"org": i % 5} for i in range(10)]
    scopes[4] = None
    stale = idx.scope_plan(scopes, 10)
    msel = mc >= n0
    idx.append_rows(x[n0:], collections=coll[n0:], attributes={"org": org[n0:]},
                    mentions=(me[msel], mc[msel] - n0, mw[msel]))
    gone = rng.choice(n, 600, replace=False)
    idx.delete_rows(gone)
    alive = np.ones(n, dtype=bool)
    alive[gone] = False
    fresh = build(alive)
    with pytest.raises(ValueError, match="ScopePlan"):
        idx.graph_search(dev(seeds), k, 2, scopes=stale)
    g = tuple(t.cpu().numpy() for t in (fresh.graph[key] for key in
                                        ("ent_rowptr", "ent_col", "men_rowptr", "men_chunk", "men_conf")))
    cols = dict(org=org[alive], collection=coll[alive])
    for hops in (0, 1, 2):
        a = idx.graph_search(dev(seeds), k, hops, scopes=scopes)
        b = fresh.graph_search(dev(seeds), k, hops, scopes=scopes)
        for j in range(3):
            same(a[j], b[j], f"scoped graph after append + delete, hops={hops} [{j}]")
        exp = [masked_topk(g, seeds[i], hops, int(alive.sum()), k,
                           scope_mask(cols, scopes[i], int(alive.sum())) if scopes[i] else None, base)
               for i in range(10)]
        assert_rows(a, exp, f"mutated index vs masked oracle hops={hops}")
