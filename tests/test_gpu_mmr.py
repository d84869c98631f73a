"""Diversified top-k on the GPU (include/thr_hip_diversify.h): thr_mmr_select on every built case of
tests/mmr_cases.py against the numpy restatement, array for array and bit for bit (float64 outputs through their
int64 view, padding included, outputs pre-filled with garbage, with out_mmr and with NULL), then the route through
GpuIndex.retrieve_batch(diversify=) -- dense only, dense + BM25, with qtok, parents="collapse", scopes, after an
append and a delete -- and through the drop-in client's final cut."""
import asyncio
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxsim_cases as MC  # noqa: E402
import mmr_cases as MM  # noqa: E402


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def on_device(name):
    """The inputs of a built case on the device, uploaded once for the runs that share them."""
    c = MM.case(name)
    return (dev(c.ids), dev(c.scores), None if c.counts is None else dev(c.counts), dev(c.docs), dev(c.dnorm))


def run_entry(T, c, want_mmr, lam=None, tensors=None):
    """thr_mmr_select itself, over outputs pre-filled with garbage -> (ids, scores, pos, mmr or None, counts)."""
    ids, scores, counts, docs, dnorm = tensors or on_device(c.name)
    nq, n = c.ids.shape
    out_ids = torch.full((nq, c.top_k), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    out_sc = torch.full((nq, c.top_k), float("nan"), dtype=torch.float64, device="cuda")
    out_pos = torch.full((nq, c.top_k), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out_mmr = torch.full((nq, c.top_k), 12345.678, dtype=torch.float64, device="cuda") if want_mmr else None
    out_cnt = torch.full((nq,), -77, dtype=torch.int32, device="cuda")
    rc = T._native.load().thr_mmr_select(
        ids.data_ptr(), scores.data_ptr(), None if counts is None else counts.data_ptr(), nq, n, docs.data_ptr(),
        dnorm.data_ptr(), docs.shape[0], docs.shape[1], c.id_base, c.lam if lam is None else lam, c.top_k,
        out_ids.data_ptr(), out_sc.data_ptr(), out_pos.data_ptr(), None if out_mmr is None else out_mmr.data_ptr(),
        out_cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, f"{c.name}: thr_mmr_select returned {rc}"
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in (out_ids, out_sc, out_pos, out_mmr, out_cnt)]


def assert_selection(got, want: MM.Selection, what):
    ids, sc, pos, mmr, cnt = got
    assert np.array_equal(cnt, want.counts), f"{what}: counts differ at queries {np.argwhere(cnt != want.counts)[:4].ravel().tolist()}"
    for name, g, w in (("out_pos", pos, want.pos), ("out_ids", ids, want.ids), ("out_scores", bits(sc), bits(want.scores))) + \
            ((("out_mmr", bits(mmr), bits(want.mmr)),) if mmr is not None else ()):
        assert g.shape == w.shape and np.array_equal(g, w), \
            f"{what}: {name} differs in {int((g != w).sum())} of {w.size} places, first at {np.argwhere(g != w)[0].tolist()}: " \
            f"got {g[g != w][0]!r}, want {w[g != w][0]!r}"


# ------------------------------------------------------------------------------------------ the entry point
@pytest.mark.parametrize("want_mmr", (True, False), ids=("mmr", "null"))
@pytest.mark.parametrize("name", MM.NAMES)
def test_every_built_case_equals_the_restatement(T, name, want_mmr):
    c = MM.case(name)
    assert_selection(run_entry(T, c, want_mmr), MM.expected(name), f"{name} ({'with' if want_mmr else 'without'} out_mmr)")


def test_the_same_bits_every_run_and_minus_zero_lambda(T):
    c = MM.case("real")
    a, b = run_entry(T, c, True), run_entry(T, c, True)
    for x, y in zip(a, b):
        assert np.array_equal(x.view(np.uint8), y.view(np.uint8))
    c = MM.case("lam-0.0")
    want = MM.mmr_reference(c.ids, c.scores, c.counts, c.docs, c.dnorm, c.id_base, -0.0, c.top_k)
    assert_selection(run_entry(T, c, True, lam=-0.0), want, "lam = -0.0")


def test_the_binding_returns_the_selection_and_refuses_bad_operands(T):
    N = T._native
    c, want = MM.case("duplicates"), MM.expected("duplicates")
    ids, scores, counts, docs, dnorm = on_device("duplicates")
    out = N.mmr_select(ids, scores, counts, docs, dnorm, c.id_base, c.top_k, c.lam)
    assert [t.dtype for t in out] == [torch.int64, torch.float64, torch.int32, torch.int32, torch.float64]
    o_ids, o_sc, o_cnt, o_pos, o_mmr = (t.cpu().numpy() for t in out)
    assert_selection((o_ids, o_sc, o_pos, o_mmr, o_cnt), want, "mmr_select")
    assert N.mmr_select(ids, scores, counts, docs, dnorm, c.id_base, c.top_k, c.lam, want_mmr=False)[4] is None
    n = c.ids.shape[1]
    for call, msg in (
            (lambda: N.mmr_select(ids, scores, counts, docs, dnorm, c.id_base, n + 1, 0.5), rf"top_k must be in 1 \.\. {n}"),
            (lambda: N.mmr_select(ids, scores, counts, docs, dnorm, c.id_base, 0, 0.5), rf"top_k must be in 1 \.\. {n}"),
            (lambda: N.mmr_select(ids, scores, counts, docs, dnorm, c.id_base, 2, 1.5), r"lam must be in \[0, 1\]"),
            (lambda: N.mmr_select(ids, scores, counts, docs, dnorm, c.id_base, 2, float("nan")), r"lam must be in \[0, 1\]"),
            (lambda: N.mmr_select(ids, scores.float(), counts, docs, dnorm, c.id_base, 2, 0.5), "scores: expected dtype"),
            (lambda: N.mmr_select(ids, scores[:, :-1].contiguous(), counts, docs, dnorm, c.id_base, 2, 0.5), "one score per id"),
            (lambda: N.mmr_select(ids, scores, counts, docs, dnorm[:-1], c.id_base, 2, 0.5), "dnorm length"),
            (lambda: N.mmr_select(ids, scores, counts, docs[:, :34].contiguous(), dnorm, c.id_base, 2, 0.5), "multiple of 4"),
            (lambda: N.mmr_select(ids, scores, counts, docs.t(), dnorm, c.id_base, 2, 0.5), "must be contiguous"),
            (lambda: N.mmr_select(ids, scores, counts, docs.double(), dnorm, c.id_base, 2, 0.5), "docs: expected dtype"),
            (lambda: N.mmr_select(torch.zeros((1, 513), dtype=torch.int64, device="cuda"),
                                  torch.zeros((1, 513), dtype=torch.float64, device="cuda"), None, docs, dnorm, 0, 2, 0.5),
             r"top_k must be in 1 \.\. 512")):
        with pytest.raises(N.NativeError, match=msg):
            call()


# ------------------------------------------------------------------------------------------ through the index
def _lex_rows(rng, n, v, per=12):
    term = np.minimum((v * rng.random((n, per)) ** 3).astype(np.int32), v - 1).reshape(-1)
    doc = np.repeat(np.arange(n, dtype=np.int32), per)
    tf = rng.geometric(0.5, n * per).astype(np.int32)
    return doc, term, tf


@functools.lru_cache(maxsize=None)
def corpus():
    """3 000 rows in clusters of five near-duplicates (the cluster's first row plus noise of 5 %); in every other
    cluster the second row is the first one's bytes.  Queries sit next to a row, so a fused list opens with a
    whole cluster."""
    rng = np.random.default_rng(77)
    n, d, v, nq = 3000, 768, 500, 8
    x = rng.standard_normal((n, d)).astype(np.float32)
    x = (x[(np.arange(n) // 5) * 5] + np.float32(0.05) * x * (np.arange(n) % 5 != 0)[:, None]).astype(np.float32)
    x[1::10] = x[0::10]
    doc, term, tf = _lex_rows(rng, n, v)
    dtok = MC.exact_tokens(rng, (n, 32, 64))
    qtok = MC.exact_tokens(rng, (nq, 32, 64))
    P = (np.arange(n) // 3).astype(np.int32)             # parents cut across the clusters
    org = (np.arange(n) % 3).astype(np.int32)
    q = x[rng.integers(0, 2400, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qt = rng.integers(0, v, (nq, 4)).astype(np.int32)
    return dict(n=n, v=v, x=x, doc=doc, term=term, tf=tf, dtok=dtok, qtok=qtok, q=q, qt=qt, P=P, org=org)


def _lex_of(C, rows):
    pos = np.full(C["n"], -1, dtype=np.int64)
    pos[rows] = np.arange(len(rows))
    sel = pos[C["doc"]] >= 0
    return pos[C["doc"][sel]].astype(np.int32), C["term"][sel], C["tf"][sel]


def _build(T, C, rows):
    rows = np.asarray(rows)
    idx = T.GpuIndex().set_dense(C["x"][rows])
    idx.set_lexical_rows(*_lex_of(C, rows), C["v"], n_docs=len(rows))
    idx.set_tokens(C["dtok"][rows])
    return idx.set_attributes({"parent": C["P"][rows], "org": C["org"][rows]})


def _same_bits(a, b, what):
    for name in ("ids", "scores", "counts"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.shape == y.shape and x.dtype == y.dtype and \
            torch.equal(x.contiguous().view(torch.uint8).cpu(), y.contiguous().view(torch.uint8).cpu()), f"{what}: {name}"


def _check_surface(T, idx, C, rows, what):
    rows = np.asarray(rows)
    qd, qtd, tokd = dev(C["q"]), dev(C["qt"]), dev(C["qtok"])
    nq = len(C["q"])
    docs, dnorm = idx.docs.cpu().numpy(), idx.dnorm.cpu().numpy()
    assert np.array_equal(docs, C["x"][rows]), what
    scopes = [{"org": i % 3} for i in range(nq)]
    configs = (("dense only", dict(query_terms=None)), ("dense + bm25", dict(query_terms=qtd)),
               ("qtok", dict(query_terms=qtd, qtok=tokd)), ("collapse", dict(query_terms=qtd, parents="collapse")),
               ("collapse + qtok", dict(query_terms=qtd, qtok=tokd, parents="collapse")),
               ("scopes", dict(query_terms=qtd, scopes=scopes)), ("scopes + qtok", dict(query_terms=qtd, qtok=tokd, scopes=scopes)))
    changed = 0
    for tag, kw in configs:
        for top_k, rerank_top_k, lam in ((10, 100, 0.5), (12, 8, 0.5), (10, 100, 1.0)):
            n_all = max(rerank_top_k, top_k)
            base = idx.retrieve_batch(qd, top_k=n_all, rerank_top_k=rerank_top_k, **kw)
            got = idx.retrieve_batch(qd, top_k=top_k, rerank_top_k=rerank_top_k, diversify=lam, **kw)
            b_ids, b_sc, b_cnt = (t.cpu().numpy() for t in (base.ids, base.scores, base.counts))
            assert b_ids.shape == (nq, n_all)
            want = MM.mmr_reference(b_ids, b_sc, b_cnt, docs, dnorm, idx.doc_base, lam, top_k)
            where = f"{what}, {tag}, top_k {top_k}, rerank_top_k {rerank_top_k}, lam {lam}"
            assert got.ids.dtype == torch.int64 and got.scores.dtype == torch.float64 and got.counts.dtype == torch.int32
            assert_selection((got.ids.cpu().numpy(), got.scores.cpu().numpy(), want.pos, None, got.counts.cpu().numpy()),
                             want, where)
            if lam == 1.0:      # relevance alone: the plain cut (the lists are descending and their scores usable)
                assert np.array_equal(got.ids.cpu().numpy(), b_ids[:, :top_k]), where
            else:
                changed += int(not np.array_equal(got.ids.cpu().numpy(), b_ids[:, :top_k]))
            if "parents" in kw:
                par = got.parents.cpu().numpy()
                ids = got.ids.cpu().numpy()
                assert np.array_equal(par, np.where(ids >= 0, C["P"][rows][np.maximum(ids, 0)], -1)), where
            else:
                assert got.parents is None
            if "scopes" in kw:
                ids, cnt = got.ids.cpu().numpy(), got.counts.cpu().numpy()
                for i in range(nq):
                    assert np.all(C["org"][rows][ids[i, :cnt[i]]] == i % 3), where
        # None is today's path: the same bits as the call without the argument
        _same_bits(idx.retrieve_batch(qd, top_k=10, rerank_top_k=100, diversify=None, **kw),
                   idx.retrieve_batch(qd, top_k=10, rerank_top_k=100, **kw), f"{what}, {tag}: diversify=None")
    assert changed >= len(configs), f"{what}: the selection hardly ever differs from the plain cut"
    # the look-alikes: the plain top 10 of the dense channel is crowded with the query's cluster, the selection is not
    plain = idx.retrieve_batch(qd, top_k=10).ids.cpu().numpy()
    div = idx.retrieve_batch(qd, top_k=10, diversify=0.5).ids.cpu().numpy()
    def crowd(lists):       # the most hits one cluster has in one query's list
        return max(np.bincount(rows[one[one >= 0]] // 5).max() for one in lists)
    assert crowd(plain) >= 3 and crowd(div) < crowd(plain), (what, crowd(plain), crowd(div))
    # the method itself, on a hand-made list with a foreign id and a count
    ids = np.array([[5, 6, -1, len(rows) + 3, 7, 40, 41, 0]], np.int64)
    sc = np.linspace(1.0, 0.3, 8)[None, :]
    out = idx.diversify(ids, sc, np.array([7], np.int32), top_k=4, lam=0.3)
    want = MM.mmr_reference(ids, sc, [7], docs, dnorm, idx.doc_base, 0.3, 4)
    assert_selection((out[0].cpu().numpy(), out[1].cpu().numpy(), out[3].cpu().numpy(), out[4].cpu().numpy(), out[2].cpu().numpy()),
                     want, f"{what}: GpuIndex.diversify")


def test_retrieve_batch_diversify_fresh_appended_deleted(T):
    C = corpus()
    n, n0 = C["n"], 2600
    idx = _build(T, C, np.arange(n0))
    _check_surface(T, idx, C, np.arange(n0), "fresh")
    new = np.arange(n0, n)
    idx.append_rows(C["x"][new], lex=(*_lex_of(C, new), C["v"]), tokens=C["dtok"][new],
                    attributes={"parent": C["P"][new], "org": C["org"][new]})
    _check_surface(T, idx, C, np.arange(n), "append")
    gone = np.unique(np.concatenate([np.arange(0, 2400, 5)[::7], [n - 1], np.arange(700, 716)]))      # cluster heads too
    idx.delete_rows(gone)
    _check_surface(T, idx, C, np.setdiff1d(np.arange(n), gone), "delete")
    with pytest.raises(ValueError, match=r"diversify is None or a float in \[0, 1\]"):
        idx.retrieve_batch(dev(C["q"]), diversify=1.5)
    bare = T.GpuIndex()
    bare.set_lexical_rows(*_lex_of(C, np.arange(50)), C["v"], n_docs=50)
    with pytest.raises(ValueError, match="no dense rows"):
        bare.diversify(np.zeros((1, 4), np.int64), np.zeros((1, 4)), top_k=2)


# ------------------------------------------------------------------------------------------ the drop-in client
def test_drop_in_client_diversifies_the_final_cut(T):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.config import SETTINGS
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever, _effective_score

    rng = np.random.default_rng(5)
    n, d = 400, 1024
    base = rng.standard_normal((n // 4, d)).astype(np.float32)
    words = [f"w{i}" for i in range(200)]
    rows = []
    for i in range(n):      # clusters of four near-identical embeddings under distinct ids and texts; one row without
        emb = base[i // 4] + np.float32(0.02) * rng.standard_normal(d).astype(np.float32)
        rows.append({"id": f"c{i}", "parent_id": f"p{i // 4}", "document_id": f"d{i // 50}",
                     "text": " ".join(rng.choice(words, 10)) + f" doc{i}", "page": 1, "modality": "text",
                     "embedding_1024": None if i == 2 else emb.tolist(), "content_hash": f"h{i}", "org_id": "org"})
    parents = [{"id": f"p{j}", "text": f"parent text {j}", "section_heading": None} for j in range(n // 4)]
    hi = IB.from_rows(rows, parents)
    idx = hi.to_gpu()
    plain = GpuIndexClient(idx, hi.store, org_id="org")
    div = GpuIndexClient(idx, hi.store, org_id="org", diversify=0.5)
    docs, dnorm = idx.docs.cpu().numpy(), idx.dnorm.cpu().numpy()
    saved = dict(SETTINGS.__dict__)
    SETTINGS.rag2_safety_threshold = 0.0
    SETTINGS.rag2_denoise_alpha = 0.0
    try:
        differs = 0
        for target in (rows[0], rows[41], rows[203]):
            e = PrecomputedEmbedder(store_dim=d)
            e.register(target["text"], base[int(target["id"][1:]) // 4].tolist())

            def retrieve(client, top_k):
                r = RAG2Retriever(org_id="org", embedder=e, query_planner=QueryPlanner())
                r._supabase = client
                res = asyncio.run(r.retrieve(target["text"], top_k=top_k, skip_rerank=True))
                assert res.success and not res.refused
                return res

            kept = retrieve(plain, 10 ** 6).contexts                  # everything the safety pass keeps, in order
            got = retrieve(div, 5)
            assert len(kept) > 5 and retrieve(plain, 5).contexts == kept[:5]
            ids = np.array([[idx.doc_base + hi.store.row_index(c.child_id) for c in kept]], np.int64)
            sc = np.array([[_effective_score(c) for c in kept]], np.float64)
            want = MM.mmr_reference(ids, sc, None, docs, dnorm, idx.doc_base, 0.5, 5)
            assert [c.child_id for c in got.contexts] == [kept[p].child_id for p in want.pos[0]]
            assert got.contexts == [kept[p] for p in want.pos[0]]     # the candidates themselves, untouched
            assert got.max_rerank_score == retrieve(plain, 5).max_rerank_score
            assert div.mmr_order([c.child_id for c in kept], sc[0].tolist(), 5) == want.pos[0].tolist()
            differs += [c.child_id for c in got.contexts] != [c.child_id for c in kept[:5]]
        assert differs > 0
        # an id the store does not know goes in as -1: selectable, similar to nothing
        order = div.mmr_order(["c0", "nobody", "c1", "c3"], [0.9, 0.8, 0.7, 0.6], 3)
        want = MM.mmr_reference(np.array([[0, -1, 1, 3]]) + np.array([[idx.doc_base, 0, idx.doc_base, idx.doc_base]]),
                                np.array([[0.9, 0.8, 0.7, 0.6]]), None, docs, dnorm, idx.doc_base, 0.5, 3)
        assert order == want.pos[0].tolist() and 1 in order
    finally:
        SETTINGS.__dict__.update(saved)
