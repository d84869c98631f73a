"""Incremental ingest on the GPU: an index built from rows [0, N - m) and appended to must equal,
array for array and result for result, a fresh index built from all N rows -- and the oracle
over the N rows."""
import asyncio

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO  # noqa: E402
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
    """Bit equality of two device arrays (NaN-aware: compared as raw bytes)."""
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8)), f"{what} differs"


def same_results(r1, r2, what):
    for j, (a, b) in enumerate(zip(r1, r2)):
        if isinstance(a, torch.Tensor):
            same(a, b, f"{what}[{j}]")
        else:
            assert a == b, f"{what}[{j}]: {a} != {b}"


# --------------------------------------------------------------------------- thr_csr_append alone
def _random_csr(rng, rows, lens, lo, hi):
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    assert len(lens) == rows
    return rowptr, rng.integers(lo, hi, nnz).astype(np.int32), rng.random(nnz).astype(np.float32)


def _concat(ra, a0, a1, rb, b0, b1):
    rows_a, rows_b = len(ra) - 1, len(rb) - 1
    o0, o1, rp = [], [], [0]
    for t in range(rows_b):
        if t < rows_a:
            o0.append(a0[ra[t]:ra[t + 1]])
            o1.append(a1[ra[t]:ra[t + 1]])
        o0.append(b0[rb[t]:rb[t + 1]])
        o1.append(b1[rb[t]:rb[t + 1]])
        rp.append(rp[-1] + sum(len(x) for x in o0[-2 if t < rows_a else -1:]))
    return (np.asarray(rp, dtype=np.int64), np.concatenate(o0) if o0 else a0[:0],
            np.concatenate(o1) if o1 else a1[:0])


@pytest.mark.parametrize("case", ["random", "grown", "empty_a", "empty_b", "long_row", "no_a"])
def test_csr_append_equals_numpy_concatenation(T, case):
    rng = np.random.default_rng(5)
    rows_a = rows_b = 3000
    la = rng.integers(0, 6, rows_a) * (rng.random(rows_a) < 0.6)     # many empty rows
    lb = rng.integers(0, 4, rows_b) * (rng.random(rows_b) < 0.5)
    if case == "grown":
        rows_b = 4500
        lb = rng.integers(0, 4, rows_b) * (rng.random(rows_b) < 0.5)
    elif case == "empty_a":
        la = np.zeros(rows_a, dtype=np.int64)
    elif case == "empty_b":
        lb = np.zeros(rows_b, dtype=np.int64)
    elif case == "long_row":          # one row of ~1e6 entries among singletons: many workgroup slices
        la = np.ones(rows_a, dtype=np.int64)
        lb = np.ones(rows_b, dtype=np.int64)
        la[1717], lb[1717] = 1_000_003, 70_001
        lb[5] = 0
    elif case == "no_a":
        rows_a, la = 0, np.zeros(0, dtype=np.int64)
    ra, a0, a1 = _random_csr(rng, rows_a, la, 0, 1 << 30)
    rb, b0, b1 = _random_csr(rng, rows_b, lb, 0, 1 << 30)
    exp_rp, exp0, exp1 = _concat(ra, a0, a1, rb, b0, b1)
    N = T._native
    A = (None, None, None) if case == "no_a" else (dev(ra), dev(a0), dev(a1))
    for two in (True, False):
        for extra in (0, 37):                      # into a capacity-reserved destination
            nnz = len(a0) + len(b0)
            out0 = torch.full((nnz + extra,), -7, dtype=torch.int32, device="cuda")
            out1 = torch.full((nnz + extra,), -7.0, dtype=torch.float32, device="cuda") if two else None
            rp, o0, o1, got_nnz = N.csr_append(A[0], A[1], A[2] if two else None, dev(rb), dev(b0),
                                               dev(b1) if two else None, out0, out1)
            assert got_nnz == nnz
            assert np.array_equal(rp.cpu().numpy(), exp_rp)
            assert np.array_equal(o0[:nnz].cpu().numpy(), exp0)
            assert np.all(o0[nnz:].cpu().numpy() == -7)          # nothing written behind the end
            if two:
                assert np.array_equal(o1[:nnz].cpu().numpy(), exp1)
                assert np.all(o1[nnz:].cpu().numpy() == -7.0)
    # an unaligned destination and source (views one element in): the element path
    if case == "long_row":
        pad = lambda a: torch.cat([a[:1], a])[1:]
        nnz = len(a0) + len(b0)
        out0 = torch.empty(nnz + 1, dtype=torch.int32, device="cuda")[1:]
        rp, o0, _, _ = N.csr_append(dev(ra), pad(dev(a0)), None, dev(rb), pad(dev(b0)), None, out0, None)
        assert np.array_equal(o0.cpu().numpy(), exp0)


# --------------------------------------------------------------------------- dense
def _dense_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    x[11] = 0                                   # a row without an embedding
    x[n - 3] = 0                                # ... among the appended ones too
    return x, rng


@pytest.mark.parametrize("shortlist", ["f16", "f16-inline", "f32", "exact"])
@pytest.mark.parametrize("d", [768, 1024])
def test_dense_append_equals_fresh_build(T, shortlist, d):
    n, nq, k = 9000 + 13, 24, 50
    x, rng = _dense_rows(n, d, 21)
    coll = rng.integers(0, 3, n).astype(np.int32)
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    q[0] = x[n - 1] * 2.0                       # its true top-1 is an appended row
    qc = np.array([-1, 0, 1, 2] * (nq // 4), dtype=np.int32)
    fresh = T.GpuIndex().set_dense(x, shortlist=shortlist).set_collections(coll)
    Se, Ie, cnte = CO.dense_topk_exact(x, q, k)
    for batches, reserve in (([n - 7000], None), ([1, 31, 33, 1000, n - 7000 - 1065], None),
                             ([1000, n - 8000], n + 50)):
        n0 = n - sum(batches)
        assert n0 % 32 != 0
        idx = T.GpuIndex().set_dense(x[:n0], shortlist=shortlist).set_collections(coll[:n0])
        assert idx.capacity_rows() == n0        # nothing reserved until asked
        if reserve:
            idx.reserve_rows(reserve)
            assert idx.capacity_rows() == reserve and idx.n_docs == n0
            ptr = idx.docs.data_ptr()
        lo = n0
        for m in batches:
            r = idx.append_rows(x[lo:lo + m], collections=coll[lo:lo + m])
            assert r == range(lo, lo + m)
            lo += m
        if reserve:
            assert idx.docs.data_ptr() == ptr   # the appends fitted the reservation: nothing moved
        assert idx.n_docs == n and idx.shortlist == fresh.shortlist == shortlist
        same(idx.docs, fresh.docs, "docs")
        same(idx.dnorm, fresh.dnorm, "dnorm")
        same(idx.inv_norm, fresh.inv_norm, "inv_norm")
        same(idx.doc_coll, fresh.doc_coll, "doc_coll")
        assert idx.doc_rel_err == fresh.doc_rel_err
        assert (idx.docs16 is None) == (fresh.docs16 is None)
        if fresh.docs16 is not None:
            same(idx.docs16, fresh.docs16, "docs16")
        for c in (None, qc):
            got, exp = idx.dense_search(dev(q), k, collections=c), fresh.dense_search(dev(q), k, collections=c)
            same_results(got, exp, f"dense_search {shortlist} collections={c is not None}")
        S, I, cnt, _ = idx.dense_search(dev(q), k)
        assert int(I[0, 0]) == n - 1
        S, I = S.cpu().numpy(), I.cpu().numpy()
        for i in range(nq):
            assert np.array_equal(I[i], Ie[i]) and np.array_equal(S[i], Se[i])
        # an empty batch is a no-op
        assert idx.append_rows(x[:0], collections=coll[:0]) == range(n, n)
        assert idx.n_docs == n


def test_dense_append_refuses_rows_float16_cannot_hold(T):
    x, _ = _dense_rows(3000, 768, 4)
    bad = x[:5].copy()
    bad[2] *= 1e6                               # values beyond 65504: the in-flight rounding cannot hold them
    idx = T.GpuIndex().set_dense(x, shortlist="f16-inline")
    with pytest.raises(T.NativeError, match="float16"):
        idx.append_rows(bad)
    assert idx.n_docs == 3000 and idx.docs.shape[0] == 3000      # nothing was changed
    auto = T.GpuIndex().set_dense(x, shortlist="auto")
    assert auto.shortlist == "f16"
    tiny = (x[:4] * 1e-7).astype(np.float32)
    auto.append_rows(np.concatenate([bad, tiny]))
    ref = T.GpuIndex().set_dense(np.concatenate([x, bad, tiny]), shortlist="auto")
    assert auto.shortlist == ref.shortlist and auto.doc_rel_err == ref.doc_rel_err
    assert (auto.docs16 is None) == (ref.docs16 is None)


# --------------------------------------------------------------------------- lexical
def _lex_rows(n, v, seed, everywhere=None):
    """(doc, term, tf) of n docs over v terms, Zipf-ish; ``everywhere``: a term every doc holds."""
    rng = np.random.default_rng(seed)
    per = 12
    term = np.minimum((v * rng.random((n, per)) ** 3).astype(np.int32), v - 1)
    doc = np.repeat(np.arange(n, dtype=np.int32), per)
    tf = rng.geometric(0.5, n * per).astype(np.int32)
    term = term.reshape(-1)
    if everywhere is not None:
        doc = np.concatenate([doc, np.arange(n, dtype=np.int32)])
        term = np.concatenate([term, np.full(n, everywhere, dtype=np.int32)])
        tf = np.concatenate([tf, np.ones(n, dtype=np.int32)])
    return doc, term, tf


def _assert_lex_equal(idx, fresh):
    L, F = idx.lex, fresh.lex
    for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"):
        same(L[k], F[k], k)
    assert L["avgdl"] == F["avgdl"]
    for j, name in enumerate(("term_ub", "block_ub", "post_imp")):
        same(L["bounds"][j], F["bounds"][j], name)
    assert (L["dense"] is None) == (F["dense"] is None)
    if F["dense"] is not None:
        for j, name in enumerate(("dense_slot", "dense_imp", "dense_tf")):
            same(L["dense"][j], F["dense"][j], name)
        assert L["dense"][3] == F["dense"][3]
    same(idx.df_local, fresh.df_local, "df_local")


def test_lexical_append_equals_fresh_build(T):
    n, v0, v1 = 20011, 3000, 3400
    doc, term, tf = _lex_rows(n, v0, 31, everywhere=7)            # skewed: term 7 is in every doc
    n0 = n - 4000
    old = doc < n0
    # the batch: new vocabulary (ids >= v0), and a term that only the new rows make dense
    rng = np.random.default_rng(32)
    nd = np.arange(n0, n, dtype=np.int32)
    doc = np.concatenate([doc, nd[::3], nd])
    term = np.concatenate([term, rng.integers(v0, v1, len(nd[::3])).astype(np.int32),
                           np.full(len(nd), 2999, dtype=np.int32)])
    tf = np.concatenate([tf, np.ones(len(nd[::3]) + len(nd), dtype=np.int32)])
    old = np.concatenate([old, np.zeros(len(nd[::3]) + len(nd), dtype=bool)])
    fresh = T.GpuIndex()
    fresh.set_lexical_rows(doc, term, tf, v1, n_docs=n, dense_share=0.05)
    idx = T.GpuIndex()
    idx.set_lexical_rows(doc[old], term[old], tf[old], v0, n_docs=n0, dense_share=0.05)
    slot_before = idx.lex["dense"][0].cpu().numpy()
    assert slot_before[7] >= 0 and slot_before[2999] < 0
    cut = n0 + 1500                                                # two uneven batches
    for lo, hi in ((n0, cut), (cut, n)):
        sel = (doc >= lo) & (doc < hi)
        r = idx.append_rows(None, lex=(doc[sel] - lo, term[sel], tf[sel], v1), n_rows=hi - lo)
        assert r == range(lo, hi)
    assert fresh.lex["dense"][0].cpu().numpy()[2999] >= 0          # the batch turned term 2999 dense
    _assert_lex_equal(idx, fresh)
    # searches: OR and conjunctive, with the oracle over all N rows
    csr_rowptr, pd, ptf, dl = (fresh.lex[k].cpu().numpy() for k in ("rowptr", "post_doc", "post_tf", "doclen"))
    idf = fresh.lex["idf"].cpu().numpy()
    qt = np.full((12, 4), -1, dtype=np.int32)
    qt[:, :3] = rng.integers(0, v1, (12, 3))
    qt[0] = [7, 2999, 3, -1]
    qt[1, :2] = [v0 + 5, 2999]
    for conj in (False, True):
        got = idx.bm25_search(dev(qt), 50, conjunctive=conj)
        same_results(got, fresh.bm25_search(dev(qt), 50, conjunctive=conj), f"bm25 conjunctive={conj}")
    Se, Ie = O.bm25_topk(csr_rowptr, pd, ptf, dl, idf, fresh.lex["avgdl"], qt, n, 50)
    S, I, cnt = idx.bm25_search(dev(qt), 50)
    for i in range(len(qt)):
        c = int(cnt[i])
        assert c == len(Ie[i]) and np.array_equal(I[i, :c].cpu().numpy(), Ie[i]) \
            and np.array_equal(S[i, :c].cpu().numpy(), Se[i])
    # filtered
    coll = rng.integers(0, 3, n).astype(np.int32)
    idx.set_collections(coll)
    fresh.set_collections(coll)
    qc = np.arange(12, dtype=np.int32) % 4 - 1
    for conj in (False, True):
        same_results(idx.bm25_search(dev(qt), 20, collections=qc, conjunctive=conj),
                     fresh.bm25_search(dev(qt), 20, collections=qc, conjunctive=conj), "bm25 filtered")


# --------------------------------------------------------------------------- everything together
def _graph(rng, n_ent, n, per=2):
    deg = rng.integers(1, 6, n_ent)
    ent_rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ent_col = rng.integers(0, n_ent, ent_rowptr[-1]).astype(np.int32)
    me = rng.integers(0, n_ent, n * per).astype(np.int64)
    me[: n // 2] = 3                                              # a hub entity: > 2048 contributions
    mc = rng.integers(0, n, n * per).astype(np.int64)
    mw = rng.uniform(0.5, 1.0, n * per).astype(np.float32)
    return ent_rowptr, ent_col, me, mc, mw


def _men_csr(me, mc, mw, n_ent):
    order = np.lexsort((mc, me))
    rp = np.concatenate([[0], np.cumsum(np.bincount(me, minlength=n_ent))]).astype(np.int64)
    return rp, mc[order].astype(np.int32), mw[order]


def test_triple_hybrid_append_equals_fresh_build(T):
    from triple_hybrid_rag_amd import synth
    n, d, v, n_ent, base = 12000 + 5, 768, 2000, 6000, 1000
    n0 = n - 2500
    x, rng = _dense_rows(n, d, 41)
    doc, term, tf = _lex_rows(n, v, 42)
    ent_rowptr, ent_col, me, mc, mw = _graph(rng, n_ent, n)
    dtok = synth.doc_tokens(0, n, 32, 64)

    def build(rows):
        sel, msel = doc < rows, mc < rows
        rp, c, w = _men_csr(me[msel], mc[msel] + base, mw[msel], n_ent)
        idx = T.GpuIndex(doc_base=base).set_dense(x[:rows], shortlist="f16")
        idx.set_lexical_rows(doc[sel], term[sel], tf[sel], v, n_docs=rows)
        return idx.set_graph(ent_rowptr, ent_col, rp, c, w).set_tokens(dtok[:rows])

    fresh, idx = build(n), build(n0)
    nq = 16
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qt = rng.integers(0, v, (nq, 4)).astype(np.int32)
    seeds = rng.integers(0, n_ent, (nq, 3)).astype(np.int32)
    seeds[0] = [3, -1, -1]
    qtok = synth.query_tokens(nq, 32, 64)
    idx.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok))     # (caches sized for n0 exist)
    cut = n0 + 700
    for lo, hi in ((n0, cut), (cut, n)):
        sel, msel = (doc >= lo) & (doc < hi), (mc >= lo) & (mc < hi)
        # mentions as the rows list them (not sorted; a pair listed twice keeps its order, as in the build)
        idx.append_rows(x[lo:hi], lex=(doc[sel] - lo, term[sel], tf[sel], v), tokens=dtok[lo:hi],
                        mentions=(me[msel], mc[msel] - lo, mw[msel]))
    for k in ("men_rowptr", "men_chunk", "men_conf", "ent_rowptr", "ent_col"):
        same(idx.graph[k], fresh.graph[k], k)
    same(idx.tokens, fresh.tokens, "tokens")
    same(idx.docs16, fresh.docs16, "docs16")
    _assert_lex_equal(idx, fresh)
    for hops in (0, 1, 2):
        same_results(idx.graph_search(dev(seeds), 50, hops), fresh.graph_search(dev(seeds), 50, hops), "graph")
    for a, b in zip(idx._graph_transposed(), fresh._graph_transposed()):
        same(a, b, "transposed mentions")
    cand = rng.integers(base, base + n, (nq, 40)).astype(np.int64)
    cand[:, :8] = base + n - 1 - np.arange(8)                            # appended candidates
    same(idx.maxsim(dev(qtok), dev(cand)), fresh.maxsim(dev(qtok), dev(cand)), "maxsim")
    r1 = idx.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok))
    r2 = fresh.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok))
    same_results((r1.ids, r1.scores, r1.counts), (r2.ids, r2.scores, r2.counts), "retrieve_batch")
    for ch in ("semantic", "lexical", "graph"):
        same_results(r1.channels[ch], r2.channels[ch], ch)
    assert int(r1.rescued) == int(r2.rescued)
    # the derived arrays a save would carry are the fresh build's
    e1, e2 = idx.export_derived(), fresh.export_derived()
    assert sorted(e1) == sorted(e2)
    for key, val in e2.items():
        assert np.array_equal(np.asarray(e1[key]).view(np.uint8) if isinstance(val, np.ndarray) else e1[key],
                              val.view(np.uint8) if isinstance(val, np.ndarray) else val), key


def test_stale_state_guards(T):
    x, rng = _dense_rows(20000, 768, 51)
    idx = T.GpuIndex().set_dense(x[:15000], shortlist="f16")
    q = x[rng.integers(0, 20000, 8)]
    idx.dense_shortlist(dev(q), 10, 1)
    idx.append_rows(x[15000:])
    with pytest.raises(T.NativeError, match="dense_shortlist"):
        idx.dense_finish(dev(q), 10, lb_all=None, gfloor=torch.full((8,), -1.0, device="cuda"))
    # a larger batch after the append: the workspace is regrown for the new row count
    big = x[rng.integers(0, 20000, 300)]
    S, I, cnt, _ = idx.dense_search(dev(big), 10)
    Se, Ie, _ = CO.dense_topk_exact(x, big, 10)
    assert np.array_equal(I.cpu().numpy(), Ie) and np.array_equal(S.cpu().numpy(), Se)
    # each part is required exactly when the index has the channel
    with pytest.raises(T.NativeError, match="no lexical channel"):
        idx.append_rows(x[:1], lex=(np.zeros(1, np.int32), np.zeros(1, np.int32), None, 4))
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    with pytest.raises(T.NativeError, match="not supported"):
        ShardedIndex.append_rows(object(), x[:1])


# --------------------------------------------------------------------------- drop-in surface
def _child_rows(n, d, seed, with_hash=True):
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(400)]
    rows = []
    for i in range(n):
        text = " ".join(rng.choice(words, 10)) + f" doc{i}"
        rows.append({"id": f"c{i}", "parent_id": f"p{i // 4}", "document_id": f"d{i // 50}", "text": text,
                     "page": None if i % 7 == 0 else i % 9 + 1, "modality": "text",
                     "embedding_1024": None if i == 13 else rng.standard_normal(d).astype(np.float32).tolist(),
                     "content_hash": f"h{i}" if with_hash else None, "org_id": "org"})
    parents = [{"id": f"p{j}", "text": f"parent text {j}", "section_heading": f"S{j}"} for j in range((n + 3) // 4)]
    return rows, parents


def test_dropin_insert_then_retrieve_and_save_load(T, tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.rag2.embedder import PrecomputedEmbedder
    from triple_hybrid_rag_amd.rag2.query_planner import QueryPlanner
    from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
    from triple_hybrid_rag_amd.config import SETTINGS

    n, d, n0 = 1200, 1024, 1000
    rows, parents = _child_rows(n, d, 61)
    hi = IB.from_rows(rows[:n0], parents[: n0 // 4])
    client = GpuIndexClient(hi.to_gpu(), hi.store, org_id="org")
    tbl = lambda: client.table("rag_child_chunks")
    # the ingest's dedup lookup
    got = tbl().select("content_hash").eq("org_id", "org").in_("content_hash", ["h3", "h1100", "nope"]).execute().data
    assert got == [{"content_hash": "h3"}]
    assert tbl().select("content_hash").eq("org_id", "other").in_("content_hash", ["h3"]).execute().data == []
    # parents first, then the children: one by one and as a list (one append of m rows)
    assert client.table("rag_parent_chunks").insert(parents[n0 // 4:]).execute().data == \
        [{"id": p["id"]} for p in parents[n0 // 4:]]
    assert tbl().insert(rows[n0]).execute().data == [{"id": f"c{n0}"}]
    assert tbl().insert(rows[n0 + 1:]).execute().data == [{"id": r["id"]} for r in rows[n0 + 1:]]
    assert client.index.n_docs == n == len(client.store.child_ids)
    with pytest.raises(Exception, match="duplicate"):
        tbl().insert(dict(rows[n0 + 5], id="another-id")).execute()       # same content_hash
    with pytest.raises(Exception, match="org_id"):
        tbl().insert(dict(rows[5], id="x", content_hash="hx", org_id="other")).execute()
    assert client.index.n_docs == n == len(client.store.child_ids)         # nothing changed
    # the same floats and search results as a bulk build from all rows
    full = IB.from_rows(rows, parents)
    ref = GpuIndexClient(full.to_gpu(), full.store, org_id="org")
    same(client.index.docs, ref.index.docs, "docs")
    same(client.index.lex["doclen"], ref.index.lex["doclen"], "doclen")
    target = rows[n - 2]
    emb = np.asarray(target["embedding_1024"], dtype=np.float32)
    for c in (client, ref):
        sem = c.rpc("rag2_semantic_search", {"p_org_id": "org", "p_embedding": emb.tolist(), "p_limit": 20}).data
        lex = c.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": target["text"], "p_limit": 20}).data
        if c is client:
            first = (sem, list(lex))
    assert first == (sem, list(lex))
    assert first[0][0]["child_id"] == target["id"] and first[1][0]["child_id"] == target["id"]
    assert first[1][0]["page"] == target["page"]
    # the retriever finds the inserted chunk with its parent context
    saved = dict(SETTINGS.__dict__)
    SETTINGS.rag2_safety_threshold = 0.0
    SETTINGS.rag2_denoise_alpha = 0.0
    try:
        e = PrecomputedEmbedder(store_dim=d)
        e.register(target["text"], emb.tolist())
        r = RAG2Retriever(org_id="org", embedder=e, query_planner=QueryPlanner())
        r._supabase = client
        res = asyncio.run(r.retrieve(target["text"], top_k=5, skip_rerank=True))
        assert res.success and res.contexts[0].child_id == target["id"]
        assert res.contexts[0].parent_text == f"parent text {(n - 2) // 4}"
    finally:
        SETTINGS.__dict__.update(saved)
    # save after the append writes the appended state; load equals it
    path = str(tmp_path / "idx")
    IB.save(hi, path, client.index)
    assert len(hi.docs) == n
    back = IB.load(path)
    assert back.store.pages == client.store.pages and None in back.store.pages[n0:]   # (nullable page)
    assert list(back.store.content_hashes) == client.store.content_hashes
    c2 = GpuIndexClient(back.to_gpu(), back.store, org_id="org")
    same(c2.index.docs, client.index.docs, "loaded docs")
    for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"):
        same(c2.index.lex[k], client.index.lex[k], "loaded " + k)
    sem2 = c2.rpc("rag2_semantic_search", {"p_org_id": "org", "p_embedding": emb.tolist(), "p_limit": 20}).data
    lex2 = c2.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": target["text"], "p_limit": 20}).data
    assert (sem2, list(lex2)) == first
    with pytest.raises(Exception, match="duplicate"):
        c2.table("rag_child_chunks").insert(rows[3]).execute()
