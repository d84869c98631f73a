"""Scope clauses on the device: thr_scope_resolve_clauses against the numpy restatement of the clause
table (tests/scope_clause_cases.py), array for array, and sets, ranges and negations through every
channel -- dense (both routes, every shortlist), BM25, the graph channel, retrieve_batch, a mutated
index and the drop-in client's p_collection=[...] -- against the oracle over the rows the restated
clauses accept.  Every comparison is bit for bit."""
import importlib.util
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scope_clause_cases as SC  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402


def _module(name):
    """Another test file of this directory as a module: its builders are this file's too."""
    spec = importlib.util.spec_from_file_location(
        "_thr_" + name, os.path.join(os.path.dirname(os.path.abspath(__file__)), name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SCOPE = _module("test_gpu_scope")
GRAPH = _module("test_gpu_scope_graph")
CLIENT = _module("test_gpu_scope_client")
make_index, dev, same, oracle_rows = SCOPE.make_index, SCOPE.dev, SCOPE.same, SCOPE.oracle_rows


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def check_resolve(N, dcols, tab, sv, masks, what):
    """rowptr, rows at full, exact and one-third cap, labels and overlap against the match matrix."""
    e_rowptr, e_rows, e_labels, e_ov = SC.np_resolve_masks(masks)
    n, total = masks.shape[1], int(e_rowptr[-1])
    rowptr, rows, labels, overlap = N.scope_resolve_clauses(dcols, tab, sv)            # cap = n
    assert np.array_equal(rowptr.cpu().numpy(), e_rowptr), f"{what}: rowptr"
    assert np.array_equal(rows.cpu().numpy()[:min(n, total)], e_rows[:n]), f"{what}: rows at cap = n"
    assert np.array_equal(labels.cpu().numpy(), e_labels), f"{what}: labels"
    assert int(overlap.item()) == e_ov, f"{what}: overlap"
    for cap in sorted({max(total, 1), max(1, total // 3), total + 5}):
        rp, r, lab, ov = N.scope_resolve_clauses(dcols, tab, sv, cap=cap)
        assert np.array_equal(rp.cpu().numpy(), e_rowptr), f"{what}: rowptr at cap {cap}"
        assert np.array_equal(r.cpu().numpy()[:min(cap, total)], e_rows[:cap]), f"{what}: rows at cap {cap}"
        assert np.array_equal(lab.cpu().numpy(), e_labels) and int(ov.item()) == e_ov
    rp, r, lab, ov = N.scope_resolve_clauses(dcols, tab, sv, cap=0, want_labels=False)  # counts only
    assert np.array_equal(rp.cpu().numpy(), e_rowptr) and r.numel() == 0 and lab is None and ov is None
    return e_rowptr, e_rows, e_labels, e_ov


@pytest.mark.parametrize("n_cols", [1, 3, 8])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049, 10007])
def test_resolve_clauses_equals_numpy(T, n, n_cols):
    from triple_hybrid_rag_amd import index_scope as IS
    N = T._native
    names = [f"a{c}" for c in range(n_cols)]
    cols = SC.resolve_columns(n, n_cols, seed=n * 10 + n_cols)
    cols[0][0] = -1 if n > 1 else cols[0][0]              # (a row without a value in the negated column)
    if n_cols > 1:
        cols[1][0], cols[1][n - 1] = SC.INT32_MAX, 0 if n > 1 else SC.INT32_MAX
    by_name = dict(zip(names, cols))
    scopes = SC.resolve_scopes(T, n_cols, names)
    masks = np.stack([SC.scope_mask(sc, by_name, T) for sc in scopes])
    keys = [tuple(IS.canonical_clause(sc[nm]) if nm in sc else None for nm in names) for sc in scopes]
    tab, sv = IS.encode_clauses(keys, n_cols)
    kinds = set(tab[..., 0].reshape(-1).tolist())
    assert {1, 2, 3, 6, 7} <= kinds                       # every kind in one call
    dcols = [dev(c) for c in cols]
    e_rowptr, e_rows, e_labels, e_ov = check_resolve(N, dcols, tab, sv, masks, f"n={n} C={n_cols}")
    # a row whose value is -1 is in no list of a predicate that tests that column, negated ones included
    for p, sc in enumerate(scopes):
        lst = e_rows[e_rowptr[p]:e_rowptr[p + 1]]
        for nm in sc:
            assert not np.any(by_name[nm][lst] == -1), (p, sc)
    assert e_ov == 1 or n == 1                             # these predicates overlap
    # two runs are byte-identical
    a = N.scope_resolve_clauses(dcols, tab, sv, cap=max(int(e_rowptr[-1]), 1))
    b = N.scope_resolve_clauses(dcols, tab, sv, cap=max(int(e_rowptr[-1]), 1))
    used = int(e_rowptr[-1])
    for x, y in zip(a, b):
        same(x[:used] if x is a[1] else x, y[:used] if y is b[1] else y, "scope_resolve_clauses run to run")
    # disjoint predicates leave the flag clear
    dis = [{names[0]: [0, 1, 2]}, {names[0]: T.Between(3, 9)}, {names[0]: T.Not(T.Between(0, 9))}]
    dkeys = [tuple(IS.canonical_clause(sc[nm]) if nm in sc else None for nm in names) for sc in dis]
    dtab, dsv = IS.encode_clauses(dkeys, n_cols)
    dmasks = np.stack([SC.scope_mask(sc, by_name, T) for sc in dis])
    assert check_resolve(N, dcols, dtab, dsv, dmasks, "disjoint")[3] == 0


@pytest.mark.parametrize("n", [1, 777, 2048, 10007])
def test_an_equality_only_table_equals_thr_scope_resolve(T, n):
    N = T._native
    rng = np.random.default_rng(n)
    cols = [rng.integers(0, 5, n).astype(np.int32), rng.integers(-1, 40, n).astype(np.int32),
            rng.integers(0, 3, n).astype(np.int32)]
    preds = np.array([[0, -1, -1], [1, 7, -1], [-1, -1, -1], [2, -1, 1], [4, 39, 2], [3, -2, -1], [9, -1, -1],
                      [-1, 7, -1]], dtype=np.int32)
    tab = np.zeros((len(preds), 3, 4), dtype=np.int32)
    tab[..., 0] = np.where(preds == -1, 0, np.where(preds < -1, 1, 2))
    tab[..., 1] = tab[..., 2] = np.maximum(preds, 0)
    dcols = [dev(c) for c in cols]
    total = int(N.scope_resolve(dcols, dev(preds), cap=0)[0][-1].item())
    for cap in (n, max(total, 1), max(1, total // 3)):
        old = N.scope_resolve(dcols, dev(preds), cap=cap)
        new = N.scope_resolve_clauses(dcols, tab, None, cap=cap)
        used = min(cap, total)
        for x, y, what in zip(old, new, ("rowptr", "rows", "labels", "overlap")):
            same(x[:used] if what == "rows" else x, y[:used] if what == "rows" else y, f"{what} at cap {cap}")


def test_any_table_is_safe_unknown_kinds_and_windows_past_the_set_values(T):
    """The table is device memory the host entry cannot read: a kind the kernel does not know matches no
    row, and a set's window is clamped into [0, n_set_values] before anything is read.  The C entry is
    called directly (the Python wrapper refuses these tables), with ``set_values`` allocated LARGER than
    n_set_values declares and filled with values rows carry: a kernel that read behind the declared
    end would read allocated memory and give the wrong lists here, not a fault."""
    import ctypes as C
    N = T._native
    lib = N.load()
    n, n_set = 5000, 6
    cols = [np.random.default_rng(3).integers(-1, 12, n).astype(np.int32), (np.arange(n) % 9).astype(np.int32)]
    sv = np.array([1, 3, 5, 7, 9, 11] + [0, 2, 4, 6, 8, 10] * 20, dtype=np.int32)          # declared: the first 6
    tab = np.zeros((12, 2, 4), dtype=np.int32)
    tab[0, 0] = (3, 0, 6, 0)              # the whole declared set
    tab[1, 0] = (3, 4, 100, 0)            # reaches past the end: clamped to [4, 6)
    tab[2, 0] = (7, 4, 100, 0)            # negated, clamped the same way
    tab[3, 0] = (3, 6, 3, 0)              # starts at the end: empty
    tab[4, 0] = (3, 1000, 5, 0)           # starts far behind it: empty
    tab[5, 0] = (3, -4, 3, 0)             # negative offset: clamped to 0
    tab[6, 0] = (3, 2, -7, 0)             # negative length: empty
    tab[7, 0] = (3, 2, 2 ** 31 - 1, 0)    # a + b overflows an int32
    tab[8, 0] = (9, 0, 5, 0)              # unknown kinds: no row
    tab[9, 1] = (-1, 0, 5, 0)
    tab[10, 0] = (4, 0, 5, 0)             # "negated any" and "negated none" are no kinds
    tab[11] = ((5, 0, 5, 0), (2, 0, 8, 0))
    masks = SC.table_masks(tab, sv, n_set, cols)
    assert masks[1].any() and masks[2].any() and not masks[[3, 4, 6, 8, 9, 10, 11]].any() and masks[7].any()
    e_rowptr, e_rows, e_labels, e_ov = SC.np_resolve_masks(masks)
    dcols = [dev(c) for c in cols]
    ptrs = (C.c_void_p * 2)(*[c.data_ptr() for c in dcols])
    dtab, dsv = dev(tab), dev(sv)
    cap = int(e_rowptr[-1])
    rowptr = torch.empty(13, dtype=torch.int64, device="cuda")
    rows = torch.full((cap,), -7, dtype=torch.int32, device="cuda")
    labels = torch.empty(n, dtype=torch.int32, device="cuda")
    overlap = torch.empty(1, dtype=torch.int32, device="cuda")
    need = lib.thr_scope_resolve_clauses_workspace_bytes(n, 12)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.thr_scope_resolve_clauses(ptrs, 2, n, dtab.data_ptr(), 12, dsv.data_ptr(), n_set, rowptr.data_ptr(),
                                       rows.data_ptr(), cap, labels.data_ptr(), overlap.data_ptr(), ws.data_ptr(), need,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    assert np.array_equal(rowptr.cpu().numpy(), e_rowptr)
    assert np.array_equal(rows.cpu().numpy(), e_rows)
    assert np.array_equal(labels.cpu().numpy(), e_labels) and int(overlap.item()) == e_ov


def expected_dense(x, dn, q, scopes, cols, T, k):
    out = []
    for i, sc in enumerate(scopes):
        r = np.nonzero(SC.scope_mask(sc, cols, T))[0]
        out.append(oracle_rows(x, dn, q[i], r, k, 0))
    return out


@pytest.mark.parametrize("shortlist", ["f16", "f16-inline", "f32", "exact"])
def test_dense_clause_scopes_both_routes_equal_the_oracle(T, shortlist):
    from triple_hybrid_rag_amd import synth
    n, dim, k = 20000, 768, 10
    idx, x, cols, _ = make_index(T, n, dim, shortlist)
    scopes = SC.index_scopes(T) * 2
    nq = len(scopes)
    counts = [int(SC.scope_mask(sc, cols, T).sum()) for sc in scopes]
    assert 0 in counts and any(0 < c < k for c in counts) and any(c > 6000 for c in counts)
    q = dev(synth.dense_queries(nq, dim, n))
    scan = idx.dense_search(q, k, scopes=scopes, scope_rows_max=0)
    rows = idx.dense_search(q, k, scopes=scopes, scope_rows_max=n)
    auto = idx.dense_search(q, k, scopes=scopes, scope_rows_max=6000)
    for j in range(3):
        same(scan[j], rows[j], f"scan vs rows route [{j}]")
        same(scan[j], auto[j], f"scan vs mixed route [{j}]")
    S, I, cnt = (t.cpu().numpy() for t in rows[:3])
    exp = expected_dense(x, O.doc_norms_f64(x), q.cpu().numpy(), scopes, cols, T, k)
    for i, (es, ei) in enumerate(exp):
        assert cnt[i] == len(ei) and np.array_equal(I[i, :len(ei)], ei) and np.array_equal(S[i, :len(ei)], es), (i, scopes[i])
    for i in (0, 3, 4, 6, 8, 11, 12):
        alone = idx.dense_search(q[i:i + 1], k, scopes=[scopes[i]])
        for j in range(3):
            same(alone[j], auto[j][i:i + 1], f"query {i} alone [{j}]")
    plan = idx.scope_plan(scopes, nq)
    assert plan.clauses is not None and len(plan.groups) >= 2      # Between(0, 10) beside Between(5, 15)
    again = idx.dense_search(q, k, scopes=plan, scope_rows_max=6000)
    for j in range(3):
        same(again[j], auto[j], f"plan passed back [{j}]")


@pytest.mark.parametrize("conjunctive", [False, True])
def test_bm25_clause_scopes_equal_the_oracle_with_the_host_mask(T, conjunctive):
    from triple_hybrid_rag_amd import synth
    n, k = 20000, 10
    idx, x, cols, csr = make_index(T, n, 256, "exact", lexical=True)
    scopes = SC.index_scopes(T) * 2
    nq = len(scopes)
    assert len(idx.scope_plan(scopes, nq).groups) >= 2
    qt = synth.lexical_queries(nq, csr.df_local, 3 if conjunctive else 4)
    S, I, cnt = idx.bm25_search(dev(qt), k, scopes=scopes, conjunctive=conjunctive)
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    idf = O.bm25_idf(n, csr.df_local)
    for i, sc in enumerate(scopes):
        m = SC.scope_mask(sc, cols, T).astype(np.int32)
        es, ei = O.bm25_topk(csr.rowptr, csr.post_doc, csr.post_tf, csr.doclen, idf, csr.sum_dl_local / n,
                             qt[i:i + 1], n, k, conjunctive=conjunctive, doc_coll=m, query_coll=[1])
        es, ei = np.asarray(es[0]), np.asarray(ei[0])
        assert cnt[i] == len(ei) and np.array_equal(I[i, :len(ei)], ei) and np.array_equal(S[i, :len(ei)], es), (i, sc)


def test_graph_clause_scopes_equal_the_masked_oracle(T):
    from triple_hybrid_rag_amd import synth
    n, k = 20000, 50
    idx, _, cols, _ = make_index(T, n, 256, "exact")
    gs = synth.build_graph(n, 0, n)
    g = (gs.ent_rowptr, gs.ent_col, gs.men_rowptr, gs.men_chunk, gs.men_conf)
    idx.set_graph(*g)
    scopes = SC.index_scopes(T) * 2
    nq = len(scopes)
    seeds = synth.graph_queries(nq, n, 3)
    assert len(idx.scope_plan(scopes, nq).groups) >= 2
    for hops in (0, 2):
        exp = [GRAPH.masked_topk(g, seeds[i], hops, n, k, SC.scope_mask(scopes[i], cols, T) if scopes[i] else None)
               for i in range(nq)]
        free = [GRAPH.masked_topk(g, seeds[i], hops, n, k, None) for i in range(nq)]
        assert any(not np.array_equal(a[1], b[1]) for a, b in zip(exp, free))
        GRAPH.assert_rows(idx.graph_search(dev(seeds), k, hops, scopes=scopes), exp, f"clause scopes, hops={hops}")


def test_retrieve_batch_clause_scopes_isolate_every_channel(T):
    from triple_hybrid_rag_amd import synth
    n, k = 20000, 10
    idx, x, cols, csr = make_index(T, n, 768, "f16", lexical=True)
    gs = synth.build_graph(n, 0, n)
    idx.set_graph(gs.ent_rowptr, gs.ent_col, gs.men_rowptr, gs.men_chunk, gs.men_conf)
    scopes = [sc for sc in SC.index_scopes(T) if sc]
    nq = len(scopes)
    q = dev(synth.dense_queries(nq, 768, n))
    qt = dev(synth.lexical_queries(nq, csr.df_local, 4))
    seeds = dev(synth.graph_queries(nq, n, 3))
    res = idx.retrieve_batch(q, qt, seeds, top_k=k, scopes=scopes, scope_graph=True)
    ids = res.ids.cpu().numpy()
    seen = 0
    for i, sc in enumerate(scopes):
        inside = SC.scope_mask(sc, cols, T)
        for name in ("semantic", "lexical", "graph"):
            ch = res.channels[name][1][i].cpu().numpy()
            ch = ch[ch >= 0]
            seen += ch.size
            assert np.all(inside[ch]), f"{name} list of query {i} leaves its scope {sc}"
        got = ids[i][ids[i] >= 0]
        assert np.all(inside[got]), f"fused ids of query {i} leave its scope {sc}"
        lists = [[int(v) for v in res.channels[name][1][i].cpu().numpy() if v >= 0] for name in ("lexical", "semantic", "graph")]
        exp, _ = O.fused_topk_ids(lists[0], lists[1], lists[2], k)       # (a thin or empty scope: short lists)
        assert list(ids[i][:len(exp)]) == exp and np.all(ids[i][len(exp):] == -1), (i, sc)
    assert seen > nq * k


def test_append_and_delete_under_clause_scopes_equal_a_fresh_build(T):
    from triple_hybrid_rag_amd import synth
    n, m, dim, k = 6000, 1000, 768, 10
    x = synth.dense_rows(3, n + m, dim)
    rng = np.random.default_rng(5)
    org = rng.integers(0, 8, n + m).astype(np.int32)          # appended rows inside and outside [2, 4] and {1, 6}
    day = np.concatenate([rng.integers(100, 200, n), rng.integers(195, 260, m)]).astype(np.int32)
    idx = T.GpuIndex().set_dense(x[:n], shortlist="f32").set_attributes({"org": org[:n], "day": day[:n]})
    scopes = [{"org": [1, 6]}, {"org": T.Between(2, 4)}, {"day": T.Between(199, None)}, {"day": T.Not(range(150, 230))},
              {"org": T.Not([1, 6]), "day": range(190, 210)}, {"org": [1, 6, 7], "day": T.Between(None, 120)}]
    q = dev(synth.dense_queries(len(scopes), dim, n))
    stale = idx.scope_plan(scopes, len(scopes))
    before = idx.dense_search(q, k, scopes=stale)
    idx.append_rows(x[n:], attributes={"org": org[n:], "day": day[n:]})
    with pytest.raises(ValueError, match="ScopePlan"):
        idx.dense_search(q, k, scopes=stale)
    gone = rng.choice(n + m, 700, replace=False)
    idx.delete_rows(gone)
    keep = np.setdiff1d(np.arange(n + m), gone)
    fresh = T.GpuIndex().set_dense(x[keep], shortlist="f32").set_attributes({"org": org[keep], "day": day[keep]})
    cols = dict(org=org[keep], day=day[keep])
    exp = expected_dense(x[keep], O.doc_norms_f64(x[keep]), q.cpu().numpy(), scopes, cols, T, k)
    changed = False
    for rmax in (0, n + m):
        a = idx.dense_search(q, k, scopes=scopes, scope_rows_max=rmax)
        b = fresh.dense_search(q, k, scopes=scopes, scope_rows_max=rmax)
        for j in range(3):
            same(a[j], b[j], f"clause scopes after append + delete [{j}]")
        S, I, cnt = (t.cpu().numpy() for t in a[:3])
        for i, (es, ei) in enumerate(exp):
            assert cnt[i] == len(ei) and np.array_equal(I[i, :len(ei)], ei) and np.array_equal(S[i, :len(ei)], es), (i, scopes[i])
        changed |= not torch.equal(a[1], before[1])
    assert changed


def _rows_of(store, x, q, mask, k):
    ts, ti = O.topk_desc(np.where(mask, O.cosine_scores_f64(x, q), -np.inf), k)
    return [f"c{j}" for j in ti], list(ts)


@pytest.mark.parametrize("tenants", [False, True])
def test_p_collection_as_a_list_ranks_inside_the_union(T, tenants):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    if tenants:
        client, hi, idx, rng, words, zipf = CLIENT.build(T, image=False)
        org, p = "acme", {"p_org_id": "acme"}
    else:
        rng, words, zipf, emb, children, parents, ents, rels, mens = CLIENT.corpus()
        hi = IB.from_rows([dict(c, org_id="solo") for c in children], parents, ents, rels, mens)
        client = GpuIndexClient(hi.to_gpu(), hi.store, org_id="solo")
        org, p = None, {"p_org_id": "solo"}
    assert client.multi_tenant == tenants
    st = hi.store
    x = np.asarray(hi.docs)
    colls = np.array(st.collections)
    mine = np.ones(len(colls), dtype=bool) if org is None else np.array(st.org_ids) == org
    q = (x[17] + 0.7 * rng.standard_normal(CLIENT.DIM)).astype(np.float32)
    text = f"{words[3]} {words[11]} {words[40]}"
    tids = np.array([[st.vocab[w] for w in text.split()]], dtype=np.int32)

    def sem(coll, limit=20):
        return client.rpc("rag2_semantic_search", dict(p, p_embedding=q.tolist(), p_limit=limit, p_collection=coll)).execute().data

    def lex(coll, limit=15, **kw):
        return list(client.rpc("rag2_lexical_search", dict(p, p_query=text, p_limit=limit, p_collection=coll, **kw)).execute().data)

    def hyb(coll):
        return client.rpc("rag2_hybrid_rrf_search", dict(p, p_query=text, p_embedding=q.tolist(), p_limit=10,
                                                         p_collection=coll)).execute().data

    union = mine & np.isin(colls, ["col0", "col2"])
    for names in (["col0", "col2"], ("col2", "col0"), ["col0", "nowhere", "col2", "col0"]):
        got = sem(names)
        ids, scores = _rows_of(st, x, q, union, 20)
        assert [r["child_id"] for r in got] == ids and [r["similarity"] for r in got] == scores
        Sl, Il = O.bm25_topk(hi.rowptr, hi.post_doc, hi.post_tf, hi.doclen, hi.idf, hi.avgdl, tids, CLIENT.N_ROWS, 15,
                             doc_coll=union.astype(np.int32), query_coll=[1])
        for rows in (lex(names), lex(names, _defer=True)):
            assert [r["child_id"] for r in rows] == [f"c{j}" for j in Il[0]] and [r["rank"] for r in rows] == list(Sl[0])
            assert rows
        lex_ids = [int(r["child_id"][1:]) for r in lex(names, 20)]
        sem_ids = [int(r["child_id"][1:]) for r in sem(names, 20)]
        fused, fused_sc = O.fused_topk_ids(lex_ids, sem_ids, None, 10)
        h = hyb(names)
        assert [r["child_id"] for r in h] == [f"c{j}" for j in fused]
        assert [r["rrf_score"] for r in h] == [float(np.float32(v)) for v in fused_sc]
        assert all(union[int(r["child_id"][1:])] for r in h)
    # the union is no single collection's answer, and a list of one name is the string form row for row
    assert sem(["col0", "col2"]) != sem("col0") and sem(["col0", "col2"]) != sem("col2")
    assert sem(["col1"]) == sem("col1") and sem(["col1"])
    assert lex(["col1"]) == lex("col1") and hyb(("col1",)) == hyb("col1")
    # names no row carries are ignored; none left: no rows
    assert sem(["nowhere", "col1"]) == sem("col1")
    assert sem([]) == [] and lex([]) == [] and hyb([]) == [] and sem(["nowhere"]) == [] and lex(("nowhere",), _defer=True) == []
    # the plan of a list is kept under its sorted names: a second request resolves nothing
    N = T._native
    keys = [k for k in client._plans if isinstance(k[2], tuple)]
    assert sorted(k[2] for k in keys) == [("col0", "col2"), ("col1",)]
    saved = N.scope_resolve_clauses, N.scope_resolve

    def boom(*_a, **_kw):
        raise AssertionError("a scope was resolved for a list of collections seen before")
    N.scope_resolve_clauses = N.scope_resolve = boom
    try:
        assert sem(("col2", "col0", "col2")) == sem(["col0", "col2"])
    finally:
        N.scope_resolve_clauses, N.scope_resolve = saved
