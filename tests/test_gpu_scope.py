"""Scoped queries on the device: thr_scope_resolve against numpy, thr_dense_topk_rows against the
oracle, and GpuIndex's two routes (row lists / scan with scope labels) against each other, against
``collections=`` and against a fresh index over the scope's rows -- every comparison bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import thr_oracle as O  # noqa: E402


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{what} differs"


def np_resolve(cols, preds):
    n = len(cols[0])
    match = np.ones((len(preds), n), dtype=bool)
    for p, pred in enumerate(preds):
        for c, v in enumerate(pred):
            if v == -1:
                continue
            match[p] &= (cols[c] == v) if v >= 0 else False
    lists = [np.nonzero(m)[0].astype(np.int32) for m in match]
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    hit = match.any(axis=0)
    labels = np.where(hit, match.argmax(axis=0), -2).astype(np.int32)
    return rowptr, (np.concatenate(lists) if lists else np.zeros(0, np.int32)), labels, int((match.sum(axis=0) > 1).any())


@pytest.mark.parametrize("n", [1, 777, 2048, 10007])
def test_scope_resolve_equals_numpy(T, n):
    N = T._native
    rng = np.random.default_rng(n)
    cols = [rng.integers(0, 5, n).astype(np.int32), rng.integers(-1, 40, n).astype(np.int32),
            rng.integers(0, 3, n).astype(np.int32)]
    preds = np.array([[0, -1, -1], [1, 7, -1], [-1, -1, -1], [2, -1, 1], [4, 39, 2], [3, -2, -1], [9, -1, -1],
                      [-1, 7, -1]], dtype=np.int32)
    rowptr, rows, labels, overlap = N.scope_resolve([dev(c) for c in cols], dev(preds))
    e_rowptr, e_rows, e_labels, e_ov = np_resolve(cols, preds)
    assert np.array_equal(rowptr.cpu().numpy(), e_rowptr)
    total = int(e_rowptr[-1])
    assert (total > n or n == 1) and np.array_equal(rows.cpu().numpy()[:min(n, total)], e_rows[:n])   # (cap = n < the matches)
    assert np.array_equal(labels.cpu().numpy(), e_labels) and int(overlap.item()) == e_ov == int(n > 1)
    # room for everything: the whole lists; nothing is written behind the capacity
    ptrs = [dev(c) for c in cols]
    rowptr2, rows2, _, _ = N.scope_resolve(ptrs, dev(preds), cap=total)
    assert np.array_equal(rows2.cpu().numpy(), e_rows) and np.array_equal(rowptr2.cpu().numpy(), e_rowptr)
    small = max(1, total // 3)
    rp3, rows3, _, _ = N.scope_resolve(ptrs, dev(preds), cap=small)
    assert np.array_equal(rp3.cpu().numpy(), e_rowptr) and np.array_equal(rows3.cpu().numpy(), e_rows[:small])
    # disjoint predicates: the flag stays clear, run to run identical
    dis = np.array([[0, -1, -1], [1, -1, -1], [3, -1, 0]], dtype=np.int32)
    a = N.scope_resolve(ptrs, dev(dis))
    b = N.scope_resolve(ptrs, dev(dis))
    assert int(a[3].item()) == 0
    used = int(a[0][-1].item())
    for x, y in zip(a, b):
        same(x[:used] if x is a[1] else x, y[:used] if y is b[1] else y, "scope_resolve run to run")


def oracle_rows(x, dn, q, rows, k, id_base):
    s = O.cosine_scores_f64(x[rows], q, dn[rows])
    ts, ti = O.topk_desc(s, k, np.asarray(rows, dtype=np.int64) + id_base)
    return ts, ti


@pytest.mark.parametrize("dim,k", [(256, 1), (768, 10), (1024, 100), (4000, 10), (768, 256)])
def test_dense_topk_rows_equals_oracle(T, dim, k):
    N = T._native
    rng = np.random.default_rng(dim + k)
    n = 6000 if dim < 4000 else 1500
    x = rng.standard_normal((n, dim)).astype(np.float32)
    x[5] = 0.0
    x[17] = 0.0
    x[100:140] = x[99]                      # duplicates: ties broken by id
    dn = O.doc_norms_f64(x)
    sizes = [0, 1, max(k - 1, 1), k, k + 1, 3000 if dim < 4000 else 900, 50]
    lists = [np.sort(rng.choice(n, s, replace=False)).astype(np.int32) for s in sizes]
    lists[5] = np.union1d(lists[5], np.arange(95, 145)).astype(np.int32)
    lists[6] = np.union1d(lists[6], [5, 17]).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    rows = np.concatenate(lists).astype(np.int32)
    P = len(lists)
    # many queries on one scope, the others one or two each, one query without a scope
    qscope = np.array([5] * 19 + list(range(P)) + [6, 4, -1, P + 3], dtype=np.int32)
    nq = len(qscope)
    q = rng.standard_normal((nq, dim)).astype(np.float32)
    q[3] = 0.0                              # a zero query scores 0.0
    q[1] = x[99]
    id_base = 1000
    S, I, cnt, flg = N.dense_topk_rows(dev(x), dev(dn), dev(q), k, dev(rowptr), dev(rows), dev(qscope), id_base)
    S, I, cnt, flg = (t.cpu().numpy() for t in (S, I, cnt, flg))
    for i in range(nq):
        p = int(qscope[i])
        if 0 <= p < P:
            es, ei = oracle_rows(x, dn, q[i], lists[p], k, id_base)
        else:
            es, ei = np.zeros(0), np.zeros(0, np.int64)
        m = len(ei)
        assert cnt[i] == m, (i, p, cnt[i], m)
        assert np.array_equal(I[i, :m], ei), f"ids of query {i} (scope {p})"
        assert np.array_equal(S[i, :m], es), f"scores of query {i} (scope {p})"
        assert np.all(I[i, m:] == -1) and np.all(np.isneginf(S[i, m:]))
        assert flg[i] == (N.THR_FLAG_CERTIFIED | N.THR_FLAG_EXACT)


def make_index(T, n, dim, shortlist, seed=0, lexical=False):
    from triple_hybrid_rag_amd import synth
    x = synth.dense_rows(seed, n, dim)
    rng = np.random.default_rng(seed + 1)
    org = rng.integers(0, 4, n).astype(np.int32)
    org[: n // 2] = 0                        # a wide tenant, three thin ones
    coll = rng.integers(0, 3, n).astype(np.int32)
    docu = (np.arange(n) // 50).astype(np.int32)
    idx = T.GpuIndex().set_dense(x, shortlist=shortlist).set_collections(coll)
    idx.set_attributes({"org": org, "document": docu})
    csr = None
    if lexical:
        doc, term, tf = synth.lexical_rows(seed, n, n)
        csr = synth.build_lexical_csr(doc, term, tf, n, synth.vocab_size(n))
        idf = O.bm25_idf(n, csr.df_local)
        idx.set_lexical(csr.rowptr, csr.post_doc, csr.post_tf, csr.doclen, idf, csr.sum_dl_local / n)
    return idx, x, dict(collection=coll, org=org, document=docu), csr


MIXED = [None, {"org": 1}, {"org": 0}, {"org": 77}, {"collection": 2}, {"org": 0, "collection": 1},
         {"document": 3}, {}, {"org": 2, "document": 9999}, {"org": 1}, {"collection": 2, "org": 3}]


@pytest.mark.parametrize("shortlist", ["f16", "f16-inline", "f32", "exact"])
def test_both_routes_agree_and_equal_the_oracle(T, shortlist):
    from triple_hybrid_rag_amd import synth
    n, dim, k = 20000, 768, 10
    idx, x, cols, _ = make_index(T, n, dim, shortlist)
    nq = len(MIXED) * 3
    scopes = MIXED * 3
    q = dev(synth.dense_queries(nq, dim, n))
    scan = idx.dense_search(q, k, scopes=scopes, scope_rows_max=0)
    rows = idx.dense_search(q, k, scopes=scopes, scope_rows_max=n)
    auto = idx.dense_search(q, k, scopes=scopes, scope_rows_max=6000)
    for j in range(3):
        same(scan[j], rows[j], f"scan vs rows route [{j}]")
        same(scan[j], auto[j], f"scan vs mixed route [{j}]")
    # the oracle over each scope's rows, and each query run alone
    dn = O.doc_norms_f64(x)
    S, I, cnt = (t.cpu().numpy() for t in rows[:3])
    for i, sc in enumerate(scopes):
        m = np.ones(n, dtype=bool)
        for name, v in (sc or {}).items():
            m &= cols[name] == v
        r = np.nonzero(m)[0]
        es, ei = oracle_rows(x, dn, q[i].cpu().numpy(), r, k, 0)
        assert cnt[i] == len(ei) and np.array_equal(I[i, :len(ei)], ei) and np.array_equal(S[i, :len(ei)], es), (i, sc)
    for i in (0, 1, 2, 3, 5):
        alone = idx.dense_search(q[i:i + 1], k, scopes=[scopes[i]])
        for j in range(3):
            same(alone[j], auto[j][i:i + 1], f"query {i} alone [{j}]")
    # a scope that is a collection alone equals collections=
    qc = np.array([2, -1, 0, 1] * 2, dtype=np.int32)
    by_coll = idx.dense_search(q[:8], k, collections=dev(qc))
    by_scope = idx.dense_search(q[:8], k, scopes=[{"collection": int(c)} if c >= 0 else None for c in qc])
    tab = np.full((8, 3), -1, dtype=np.int32)
    tab[:, 0] = qc
    by_table = idx.dense_search(q[:8], k, scopes=dev(tab), scope_rows_max=0)
    for j in range(3):
        same(by_coll[j], by_scope[j], f"collections= vs scopes= [{j}]")
        same(by_coll[j], by_table[j], f"collections= vs scope table [{j}]")
    with pytest.raises(ValueError, match="not both"):
        idx.dense_search(q[:8], k, collections=dev(qc), scopes=[None] * 8)
    with pytest.raises(ValueError, match="unknown attribute"):
        idx.dense_search(q[:1], k, scopes=[{"tenant": 1}])


@pytest.mark.parametrize("conjunctive", [False, True])
def test_bm25_scopes_equal_the_oracle_with_composite_labels(T, conjunctive):
    from triple_hybrid_rag_amd import synth
    n, k = 20000, 10
    idx, x, cols, csr = make_index(T, n, 256, "exact", lexical=True)
    scopes = MIXED * 2
    nq = len(scopes)
    qt = synth.lexical_queries(nq, csr.df_local, 3 if conjunctive else 4)
    S, I, cnt = idx.bm25_search(dev(qt), k, scopes=scopes, conjunctive=conjunctive)
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    idf = O.bm25_idf(n, csr.df_local)
    for i, sc in enumerate(scopes):
        m = np.ones(n, dtype=np.int32)
        for name, v in (sc or {}).items():
            m &= (cols[name] == v).astype(np.int32)
        es, ei = O.bm25_topk(csr.rowptr, csr.post_doc, csr.post_tf, csr.doclen, idf, csr.sum_dl_local / n,
                             qt[i:i + 1], n, k, conjunctive=conjunctive, doc_coll=m, query_coll=[1])
        es, ei = np.asarray(es[0]), np.asarray(ei[0])
        assert cnt[i] == len(ei) and np.array_equal(I[i, :len(ei)], ei) and np.array_equal(S[i, :len(ei)], es), (i, sc)


def test_retrieve_batch_scopes_isolate_tenants(T):
    from triple_hybrid_rag_amd import synth
    n, k = 20000, 10
    idx, x, cols, csr = make_index(T, n, 768, "f16", lexical=True)
    nq = 12
    q = dev(synth.dense_queries(nq, 768, n))
    qt = dev(synth.lexical_queries(nq, csr.df_local, 4))
    scopes = [{"org": i % 4} for i in range(nq)]
    res = idx.retrieve_batch(q, qt, top_k=k, scopes=scopes)
    plan = idx.scope_plan(scopes, nq)
    again = idx.retrieve_batch(q, qt, top_k=k, scopes=plan, scope_rows_max=0)
    same(res.ids, again.ids, "fused ids, plan passed in and scan route")
    same(res.scores, again.scores, "fused scores")
    ids = res.ids.cpu().numpy()
    for i in range(nq):
        for name in ("semantic", "lexical"):
            ch = res.channels[name][1][i].cpu().numpy()
            ch = ch[ch >= 0]
            assert ch.size and np.all(cols["org"][ch] == i % 4), f"{name} list of query {i} leaves its tenant"
        got = ids[i][ids[i] >= 0]
        assert got.size and np.all(cols["org"][got] == i % 4)
        exp, _ = O.fused_topk_ids(list(res.channels["lexical"][1][i].cpu().numpy()),
                                  list(res.channels["semantic"][1][i].cpu().numpy()), None, k)
        assert list(ids[i]) == exp


def test_append_and_delete_keep_attributes_and_scoped_results_equal_to_a_fresh_build(T, tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd import synth
    n, m, dim, k = 6000, 1000, 768, 10
    x = synth.dense_rows(3, n + m, dim)
    rng = np.random.default_rng(5)
    org = rng.integers(0, 5, n + m).astype(np.int32)
    coll = rng.integers(0, 2, n + m).astype(np.int32)
    idx = T.GpuIndex().set_dense(x[:n], shortlist="f32").set_collections(coll[:n]).set_attributes({"org": org[:n]})
    with pytest.raises(T._native.NativeError, match="attributes"):
        idx.append_rows(x[n:], collections=coll[n:])
    with pytest.raises(T._native.NativeError, match="one value per appended row"):
        idx.append_rows(x[n:], collections=coll[n:], attributes={"org": org[n:n + 5]})
    assert idx.n_docs == n
    idx.append_rows(x[n:], collections=coll[n:], attributes={"org": org[n:]})
    gone = rng.choice(n + m, 700, replace=False)
    idx.delete_rows(gone)
    keep = np.setdiff1d(np.arange(n + m), gone)
    fresh = T.GpuIndex().set_dense(x[keep], shortlist="f32").set_collections(coll[keep]).set_attributes({"org": org[keep]})
    same(idx.attribute("org"), fresh.attribute("org"), "org column")
    same(idx.attribute("collection"), fresh.attribute("collection"), "collection column")
    q = dev(synth.dense_queries(10, dim, n))
    scopes = [{"org": i % 5, "collection": i % 2} for i in range(10)]
    for rmax in (0, n + m):
        a = idx.dense_search(q, k, scopes=scopes, scope_rows_max=rmax)
        b = fresh.dense_search(q, k, scopes=scopes, scope_rows_max=rmax)
        for j in range(3):
            same(a[j], b[j], f"scoped search after append + delete [{j}]")
    # save -> load keeps the columns
    hi = IB.HostIndex(docs=x[:n].copy(), attributes={"org": org[:n], "collection": coll[:n]})
    IB.save(hi, str(tmp_path / "ix"), idx)
    back = IB.load(str(tmp_path / "ix")).to_gpu()
    same(back.attribute("org"), fresh.attribute("org"), "org column after save / load")
    same(back.attribute("collection"), fresh.attribute("collection"), "collection column after save / load")
    c = back.dense_search(q, k, scopes=scopes)
    for j in range(3):
        same(c[j], b[j], f"scoped search after save / load [{j}]")
