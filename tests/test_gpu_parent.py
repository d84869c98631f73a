"""Child -> parent expansion on the GPU (include/thr_hip_parent.h): the groups of a fused row array for array
against the numpy restatement, the parent scorers over the float16 packed store and the FP8 store against float64
(tests/parent_cases.py: the oracle's MaxSim of the query against the concatenated family block), and the route
through GpuIndex.maxsim(expand=), retrieve_batch(parents=), append / delete and the drop-in client.

Exact-family inputs are compared with np.array_equal; real-valued inputs are held to error_bound_parent, computed
from the inputs.  Each real-valued case prints its largest error / bound (run with -s)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxsim_cases as MC  # noqa: E402
import maxsim_fp8_cases as F8  # noqa: E402
import parent_cases as PC  # noqa: E402

STORES = ("f16", "fp8")


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def assert_exact(got, ref, what):
    assert got.shape == ref.shape and np.array_equal(got, ref), \
        f"{what}: {int((got != ref).sum())} of {ref.size} scores differ, first at " \
        f"{tuple(np.argwhere(got != ref)[0])}: got {got[got != ref][0]!r}, reference {ref[got != ref][0]!r}"


# ------------------------------------------------------------------------------------------ groups
def run_groups(T, ids, counts, P, base):
    out = T._native.parent_groups(dev(ids), None if counts is None else dev(counts), dev(P), base)
    assert [t.dtype for t in out] == [torch.int32, torch.int32, torch.int64, torch.int32]
    return [t.cpu().numpy() for t in out]


def assert_groups(got, want, what):
    for name, g, w in zip(("leader", "slot", "uniq_ids", "n_uniq"), got, want):
        assert g.shape == w.shape and np.array_equal(g, w), \
            f"{what}: {name} differs at {np.argwhere(g != w)[:4].tolist()}: got {g[g != w][:4].tolist()}, want {w[g != w][:4].tolist()}"


@pytest.mark.parametrize("case", PC.group_cases(), ids=lambda c: c[0])
def test_groups_equal_the_restatement(T, case):
    name, ids, counts, P, base = case
    got = run_groups(T, ids, counts, P, base)
    assert_groups(got, PC.groups_reference(ids, counts, P, base), name)
    again = run_groups(T, ids, counts, P, base)         # the same bits every run
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again)), name


def test_groups_of_many_queries_in_one_call(T):
    ids, counts, P = PC.many_queries_case(65600, 4)
    assert_groups(run_groups(T, ids, counts, P, 0), PC.groups_reference(ids, counts, P, 0), "65 600 queries, counts")
    assert_groups(run_groups(T, ids, None, P, 0), PC.groups_reference(ids, None, P, 0), "65 600 queries, no counts")


# ------------------------------------------------------------------------------------------ the raw scorers
def score_parent(T, store, q, d, P, cand, base, csr=None):
    """thr_maxsim_parent_ids / thr_maxsim_parent_fp8_ids over the device's own image of ``d`` -> float64."""
    N = T._native
    rowptr, child = PC.parent_csr(P) if csr is None else csr
    tail = (dev(np.asarray(cand, dtype=np.int64)), base, dev(P), dev(rowptr), dev(child))
    if store == "fp8":
        image, scales = N.maxsim_quantize_fp8(dev(d))
        out = N.maxsim_parent_fp8_ids(dev(q), image, scales, *tail)
    else:
        out = N.maxsim_parent_ids(dev(q), N.maxsim_pack(dev(d)), *tail)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(np.shape(cand))
    return f64(out)


def _matrix_ids(fp8):
    return [f"td{r[0]}-q{r[1]}-d{r[2]}-fan{r[3]}-{r[4]}-c{r[5]}-{r[6]}" for r in PC.exact_matrix(fp8)]


@pytest.mark.parametrize("row", PC.exact_matrix(False), ids=_matrix_ids(False))
def test_exact_family_f16(T, row):
    _exact(T, "f16", row)


@pytest.mark.parametrize("row", PC.exact_matrix(True), ids=_matrix_ids(True))
def test_exact_family_fp8(T, row):
    _exact(T, "fp8", row)


def _exact(T, store, row):
    td, qt, dt, fan, kind, n_cand, which = row
    base = 0 if fan % 2 else 7000
    q, d, P, cand, base, planted = PC.exact_case(td + fan, td, qt, dt, fan, kind, n_cand=n_cand, id_base=base, which=which)
    ref = PC.parent_reference(q, d, P, cand, base)
    got = score_parent(T, store, q, d, P, cand, base)
    assert_exact(got, ref, f"{store} {row}")
    assert got[0, 0] > PC.parent_reference(q[:1], PC.without_plant(d, planted), P, cand[:1, :1], base)[0, 0]
    if n_cand >= 4:
        assert got[0, 1] == -np.inf and got[-1, 2] == -np.inf and (not base or got[0, 3] == -np.inf)


@pytest.mark.parametrize("store", STORES)
def test_an_out_of_range_child_is_skipped(T, store):
    """A CSR the index layer would never build: one child at n_docs + 5, one negative, row pointers past nnz.  The
    bad children are skipped (never dereferenced), the pointers clamped: the family is what is left."""
    q, d, P, cand, base, _ = PC.exact_case(11, 32, 32, 64, 3, "interleaved", n_cand=5, n_queries=1)
    n_docs = len(P)
    rowptr, child = PC.parent_csr(P)
    assert PC.family(P, 0) == [0, 3, 6] and child[:3].tolist() == [0, 3, 6]
    cand = np.array([[0, 3, 6, 1, 2]], np.int64)
    for bad in (n_docs + 5, -3, 2 ** 31 - 1):
        broken = child.copy()
        broken[1] = bad
        left = P.copy()
        left[3] = -1                                   # the reference: row 3 is not in the family any more
        ref = PC.parent_reference(q, d, left, cand, 0)
        got = score_parent(T, store, q, d, P, cand, 0, csr=(rowptr, broken))
        assert_exact(got[:, [0, 2, 3, 4]], ref[:, [0, 2, 3, 4]], f"{store}, child {bad}")
        assert got[0, 1] == got[0, 0]                  # row 3 still names parent 0: it walks the same (cut) list
    wide = rowptr.copy()
    wide[-1] = len(child) + 1000                       # clamped to nnz
    assert_exact(score_parent(T, store, q, d, P, cand, 0, csr=(wide, child)), PC.parent_reference(q, d, P, cand, 0), "clamp")
    # a parent number at or above n_parents is a row on its own
    cut = (rowptr[:2].copy(), child[:rowptr[1]].copy())
    alone = np.where(P == 0, 0, -1).astype(np.int32)
    assert_exact(score_parent(T, store, q, d, P, cand, 0, csr=cut), PC.parent_reference(q, d, alone, cand, 0), "n_parents")


@pytest.mark.parametrize("store", STORES)
def test_many_queries_in_one_call(T, store):
    """65 600 queries x 1 candidate at 32 x 32 x 32 (queries sit on gridDim.y; the launch goes out in slices)."""
    rng = np.random.default_rng(65600)
    nq, pool_n, td = 65600, 257, 32
    P = PC.layout("loner", 2)
    n_docs = len(P)
    pool = MC.exact_tokens(rng, (pool_n, 32, td))
    d = MC.exact_tokens(rng, (n_docs, 32, td))
    table = PC.parent_reference(pool, d, P, np.tile(np.arange(n_docs), (pool_n, 1)), 0)      # [pool, row]
    which = np.arange(nq) % pool_n
    cand = rng.integers(0, n_docs, (nq, 1)).astype(np.int64)
    cand[rng.integers(0, nq, 500), 0] = -1
    cand[-1, 0], cand[65535, 0], cand[65536, 0] = -1, n_docs, 4
    ok = (cand >= 0) & (cand < n_docs)
    ref = np.where(ok, table[which[:, None], np.where(ok, cand, 0)], -np.inf)
    assert_exact(score_parent(T, store, pool[which], d, P, cand, 0), ref, f"{store}, 65 600 queries")


REAL = [(fam, fan, td) for fam in ("unit", "normal") for fan in (1, 4, 7) for td in (64, 128)]


@pytest.mark.parametrize("store", STORES)
@pytest.mark.parametrize("family,fan,td", REAL, ids=[f"{a}-fan{b}-td{c}" for a, b, c in REAL])
def test_real_family_within_the_bound(T, store, family, fan, td):
    rng = np.random.default_rng(fan * 1000 + td)
    P = PC.layout("loner", fan, n_families=4)
    n_docs = len(P)
    q = MC.real_tokens(family, rng, 3, 64, td, queries=True)
    d = MC.real_tokens(family, rng, n_docs, 32, td, queries=False)
    cand = np.stack([rng.permutation(n_docs)[:9] for _ in range(3)]).astype(np.int64)
    cand[1, 4] = -1
    idx = T.GpuIndex().set_dense(np.ones((n_docs, 8), np.float32), shortlist="exact").set_tokens(d, store=store)
    idx.set_parents(P)
    got = f64(idx.maxsim(dev(q), dev(cand), expand="parent"))
    if store == "fp8":
        codes, scales = F8.unpack(idx.tokens.cpu().numpy()), idx.token_scales.cpu().numpy()
        ref = PC.parent_reference_fp8(q, codes, scales, P, cand)
        bound = PC.error_bound_parent_fp8(q, codes, scales, P, cand)
    else:
        ref, bound = PC.parent_reference(q, d, P, cand), PC.error_bound_parent(q, d, P, cand)
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin) and got[1, 4] == -np.inf
    err = np.abs(got[fin] - ref[fin])
    print(f"\n{store} {family} fan-out {fan} tok_dim {td}: max error {err.max():.3e}, bound there {bound[fin][err.argmax()]:.3e}, "
          f"largest error / bound {np.max(err / bound[fin]):.3f}")
    assert np.all(err <= bound[fin]), (store, family, fan, td, float(np.max(err / bound[fin])))
    if fan == 1:        # every row its own parent: the plain scorer's bits
        assert torch.equal(idx.maxsim(dev(q), dev(cand), expand="parent"), idx.maxsim(dev(q), dev(cand)))


# ------------------------------------------------------------------------------------------ the index
def _lex_rows(rng, n, v, per=12):
    term = np.minimum((v * rng.random((n, per)) ** 3).astype(np.int32), v - 1).reshape(-1)
    doc = np.repeat(np.arange(n, dtype=np.int32), per)
    tf = rng.geometric(0.5, n * per).astype(np.int32)
    return doc, term, tf


@functools.lru_cache(maxsize=None)
def corpus():
    rng = np.random.default_rng(41)
    n, d, v, nq = 1500, 768, 500, 8
    x = rng.standard_normal((n, d)).astype(np.float32)
    # siblings are close in the dense space, so a fused list sees a parent through several children
    x = (x[(np.arange(n) // 4) * 4] + 0.4 * x).astype(np.float32)
    doc, term, tf = _lex_rows(rng, n, v)
    dtok = MC.exact_tokens(rng, (n, 32, 64))
    P = (np.arange(n) // 4).astype(np.int32)
    P[rng.choice(n, 100, replace=False)] = -1
    P[5::97] = P[3]                                   # a family spread over the whole shard
    qtok = MC.exact_tokens(rng, (nq, 32, 64))
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qt = rng.integers(0, v, (nq, 4)).astype(np.int32)
    return dict(n=n, v=v, x=x, doc=doc, term=term, tf=tf, dtok=dtok, qtok=qtok, q=q, qt=qt, P=P)


def _build(T, C, rows, store, parents=True):
    rows = np.asarray(rows)
    remap = np.full(C["n"], -1, dtype=np.int64)
    remap[rows] = np.arange(len(rows))
    sel = remap[C["doc"]] >= 0
    idx = T.GpuIndex().set_dense(C["x"][rows])
    idx.set_lexical_rows(remap[C["doc"][sel]].astype(np.int32), C["term"][sel], C["tf"][sel], C["v"], n_docs=len(rows))
    idx.set_tokens(C["dtok"][rows], store=store)
    return idx.set_parents(C["P"][rows]) if parents else idx


def _fused(idx, C, rows, n_fused=100):
    """The oracle's fused lists over the rows the index holds -> per query (ids, rrf scores)."""
    L = idx.lex
    rowptr, pd, ptf, dl, idf = (L[k].cpu().numpy() for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"))
    _, Id, _ = CO.dense_topk_exact(C["x"][rows], C["q"], 100)
    _, Il = O.bm25_topk(rowptr, pd, ptf, dl, idf, L["avgdl"], C["qt"], len(rows), 50)
    return [O.fused_topk_ids(list(Il[i]), list(Id[i]), None, n_fused) for i in range(len(C["q"]))]


def _check_pipeline(T, idx, C, rows, what):
    """maxsim(expand=), retrieve_batch(parents="rerank" / "collapse") against the references, over the rows
    ``rows`` of the corpus; the CSR against the restatement."""
    rows = np.asarray(rows)
    P, dtok, nq = C["P"][rows], C["dtok"][rows], len(C["q"])
    assert np.array_equal(idx.attribute("parent").cpu().numpy(), P), what
    want_csr = PC.parent_csr(P)
    rowptr, child = idx.parent_csr()
    assert np.array_equal(rowptr.cpu().numpy(), want_csr[0]) and np.array_equal(child.cpu().numpy(), want_csr[1]), what
    fused = _fused(idx, C, rows)
    qd, qtd, tokd = dev(C["q"]), dev(C["qt"]), dev(C["qtok"])
    # rerank: every candidate stays, scored on its parent; the exact family makes the device's scores the reference's
    for top_k in (10, 100):
        res = idx.retrieve_batch(qd, qtd, top_k=top_k, qtok=tokd, rerank_top_k=100, parents="rerank")
        ids, sc, cnt, par = (t.cpu().numpy() for t in (res.ids, res.scores, res.counts, res.parents))
        assert res.parents.dtype == torch.int32 and par.shape == ids.shape
        for i in range(nq):
            f100 = fused[i][0]
            ms = PC.parent_reference(C["qtok"][i:i + 1], dtok, P, np.array([f100], dtype=np.int64))[0]
            order = O.rerank_order(list(ms))[:top_k]
            assert int(cnt[i]) == len(order) and list(ids[i, :cnt[i]]) == [f100[j] for j in order], f"{what} rerank {top_k} q{i}"
            assert list(sc[i, :cnt[i]]) == [float(ms[j]) for j in order], f"{what} rerank {top_k} q{i}: scores"
            MC.assert_order_within(ids[i, :cnt[i]], f100, ms, 0.0, f"{what} rerank {top_k} q{i}")
            assert list(par[i, :cnt[i]]) == [int(P[g]) for g in ids[i, :cnt[i]]] and np.all(par[i, cnt[i]:] == -1)
    # collapse, with and without the rerank
    short = 0
    for top_k, with_q in ((10, True), (100, True), (10, False), (100, False)):
        res = idx.retrieve_batch(qd, qtd, top_k=top_k, qtok=tokd if with_q else None, rerank_top_k=100, parents="collapse")
        ids, sc, cnt, par = (t.cpu().numpy() for t in (res.ids, res.scores, res.counts, res.parents))
        for i in range(nq):
            f100, s100 = fused[i]
            pos, lead = PC.collapse_reference(f100, len(f100), P)
            if with_q:
                ms = PC.parent_reference(C["qtok"][i:i + 1], dtok, P, np.array([lead], dtype=np.int64))[0]
                order = O.rerank_order(list(ms))[:top_k]
                want_ids, want_sc = [lead[j] for j in order], [float(ms[j]) for j in order]
            else:
                want_ids, want_sc = lead[:top_k], [s100[p] for p in pos[:top_k]]
            tag = f"{what} collapse top_k {top_k} qtok {with_q} q{i}"
            assert int(cnt[i]) == len(want_ids) and list(ids[i, :cnt[i]]) == want_ids, tag
            assert list(sc[i, :cnt[i]]) == want_sc, tag + ": scores"
            assert np.all(ids[i, cnt[i]:] == -1) and np.all(par[i, cnt[i]:] == -1), tag
            got_par = [int(p) for p in par[i, :cnt[i]]]
            assert got_par == [int(P[g]) for g in want_ids], tag
            with_parent = [p for p in got_par if p >= 0]
            assert len(set(with_parent)) == len(with_parent), tag + ": two returned ids share a parent"
            for g in want_ids:          # each is its family's best-fused child
                fam = set(PC.family(P, g))
                assert g == next(c for c in f100 if c in fam), tag
            if top_k == 100:        # fewer distinct parents than top_k -> the short count
                assert int(cnt[i]) == len(lead) <= len(f100), tag
                short += len(lead) < 100
    assert short > 0, f"{what}: no query of the corpus has fewer than 100 distinct parents in its fused list"
    return fused


@pytest.mark.parametrize("store", STORES)
def test_maxsim_expand_parent_on_raw_rows(T, store):
    C = corpus()
    rows = np.arange(600)
    idx = _build(T, C, rows, store)
    P = C["P"][rows]
    rng = np.random.default_rng(3)
    cand = rng.integers(0, 600, (len(C["qtok"]), 40)).astype(np.int64)
    cand[:, :8] = np.array([0, 1, 2, 3, 3, 0, 5, 102])          # siblings, a repeat, the spread family
    cand[2, 9], cand[3, 10] = -1, 600
    got = idx.maxsim(dev(C["qtok"]), dev(cand), expand="parent")
    assert_exact(f64(got), PC.parent_reference(C["qtok"], C["dtok"][rows], P, cand), f"{store} expand")
    g = got.cpu().numpy().view(np.uint32)
    for i in range(cand.shape[0]):
        for a in range(cand.shape[1]):
            for b in range(a):
                ra, rb = int(cand[i, a]), int(cand[i, b])
                if 0 <= ra < 600 and 0 <= rb < 600 and P[ra] >= 0 and P[ra] == P[rb]:
                    assert g[i, a] == g[i, b]               # siblings: identical bits
    # a candidate row wider than a fused list goes through in pieces
    wide = rng.integers(0, 600, (2, 700)).astype(np.int64)
    assert_exact(f64(idx.maxsim(dev(C["qtok"][:2]), dev(wide), expand="parent")),
                 PC.parent_reference(C["qtok"][:2], C["dtok"][rows], P, wide), f"{store} expand, 700 candidates")
    # no row has a parent: the plain scores
    idx.set_parents(np.full(600, -1))
    assert idx.parent_csr() is None
    assert torch.equal(idx.maxsim(dev(C["qtok"]), dev(cand), expand="parent"), idx.maxsim(dev(C["qtok"]), dev(cand)))
    with pytest.raises(ValueError, match="PACKED float16 store"):
        T.GpuIndex().set_dense(C["x"][:40]).set_tokens(C["dtok"][:40], pack=False).set_parents(P[:40]) \
            .maxsim(dev(C["qtok"]), dev(cand), expand="parent")
    with pytest.raises(ValueError, match="no parent column"):
        _build(T, C, np.arange(40), store, parents=False).maxsim(dev(C["qtok"]), dev(cand), expand="parent")
    # the column is a scope like any other
    S, I, cnt, _ = _build(T, C, rows, store).dense_search(dev(C["q"][:2]), 10, scopes=[{"parent": 3}, {"parent": 10}])
    for i, p in enumerate((3, 10)):
        assert int(cnt[i]) == min(10, int((P == p).sum())) and all(P[g] == p for g in I[i, :cnt[i]].tolist())


def _answers(idx, C):
    qd, qtd, tokd = dev(C["q"]), dev(C["qt"]), dev(C["qtok"])
    out = []
    for mode, tk in (("rerank", tokd), ("collapse", tokd), ("collapse", None), (None, tokd)):
        r = idx.retrieve_batch(qd, qtd, top_k=10, qtok=tk, rerank_top_k=100, parents=mode)
        out += [r.ids, r.scores, r.counts] + ([r.parents] if mode else [])
    torch.cuda.synchronize()
    return out


def _assert_same_answers(a, b, what):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype and \
            torch.equal(x.contiguous().view(torch.uint8).cpu(), y.contiguous().view(torch.uint8).cpu()), f"{what}: output {j}"


@pytest.mark.parametrize("store", STORES)
def test_pipeline_append_delete(T, store):
    """retrieve_batch(parents=) on a fresh index, after an append (children of old and of new parents), after a
    delete (a middle child, a whole family, the last row) and after delete -> append -> delete: the column, the CSR
    and every answer equal a fresh index over the surviving rows, whatever the scratch buffers held."""
    C = corpus()
    n, n0 = C["n"], 1200
    idx = _build(T, C, np.arange(n0), store)
    _check_pipeline(T, idx, C, np.arange(n0), "fresh")
    # parents=None: what an index that never heard of parents returns
    twin = _build(T, C, np.arange(n0), store, parents=False)
    qd, qtd, tokd = dev(C["q"]), dev(C["qt"]), dev(C["qtok"])
    for tk in (tokd, None):
        a, b = idx.retrieve_batch(qd, qtd, top_k=10, qtok=tk), twin.retrieve_batch(qd, qtd, top_k=10, qtok=tk)
        _assert_same_answers([a.ids, a.scores, a.counts], [b.ids, b.scores, b.counts], "parents=None")
        assert a.parents is None and b.parents is None

    def append(rows_new):
        pos = np.full(n, -1, dtype=np.int64)
        pos[rows_new] = np.arange(len(rows_new))
        sel = pos[C["doc"]] >= 0
        idx.append_rows(C["x"][rows_new], lex=(pos[C["doc"][sel]].astype(np.int32), C["term"][sel], C["tf"][sel], C["v"]),
                        tokens=C["dtok"][rows_new], attributes={"parent": C["P"][rows_new]})

    def check(rows, what):
        _check_pipeline(T, idx, C, rows, what)
        for w in (idx._ws, idx._ws_rescue, idx._ws_lex, idx._ws_graph):      # the workspace contract
            if w is not None:
                w.fill_(0xFF)
        _assert_same_answers(_answers(idx, C), _answers(_build(T, C, rows, store), C), what + ": against a fresh index")

    append(np.arange(n0, n))            # rows 1200 .. : new parents, and (P[5::97] = P[3]) children of an old one
    assert set(C["P"][n0:].tolist()) & set(C["P"][:n0].tolist()) and set(C["P"][n0:].tolist()) - set(C["P"][:n0].tolist())
    check(np.arange(n), "append")
    fam = np.nonzero(C["P"] == C["P"][5])[0]          # the family spread over the shard, old and appended rows
    assert len(fam) >= 8 and fam.min() < n0 <= fam.max()
    gone = np.unique(np.concatenate([[401], fam, [n - 1], np.arange(700, 716)]))      # a middle child, a family, the last row
    idx.delete_rows(gone)
    keep = np.setdiff1d(np.arange(n), gone)
    check(keep, "delete")
    back = gone[:12]
    append(back)
    rows = np.concatenate([keep, back])
    gone2 = np.array([3, len(rows) - 1, len(rows) - 5])
    idx.delete_rows(gone2)
    rows = np.delete(rows, gone2)
    check(rows, "delete -> append -> delete")


# ------------------------------------------------------------------------------------------ the drop-in client
def test_drop_in_client_reranks_on_the_parent(T, tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    from triple_hybrid_rag_amd.retrieval.hybrid_search import SearchResult
    from triple_hybrid_rag_amd.retrieval.reranker import Reranker
    from triple_hybrid_rag_amd.store import CorpusStore
    rng = np.random.default_rng(9)
    n, dim = 64, 32
    x = rng.standard_normal((n + 8, dim)).astype(np.float32)
    dtok = MC.exact_tokens(rng, (n + 8, 32, 64))
    qtok = MC.exact_tokens(rng, (1, 32, 64))

    class Emb:
        def embed_query_tokens(self, query):
            return qtok[0]

    store = CorpusStore.synthetic(n, children_per_parent=4)
    hi = IB.HostIndex(docs=x[:n], store=store)
    idx = hi.to_gpu(shortlist="exact").set_tokens(dtok[:n], store="fp8")
    client = GpuIndexClient(idx, store, org_id="org", token_embedder=Emb(), parent_rerank=True)
    assert idx.attribute("parent").cpu().tolist() == [i // 4 for i in range(n)] and client._parent_code["p3"] == 3
    # insert: two more children of p2, four of a new parent
    new = [{"id": f"c{n + j}", "parent_id": "p2" if j < 2 else "p900", "document_id": "d0", "text": f"new {j}", "page": 1,
            "modality": "text", "embedding_1024": x[n + j].tolist(), "tokens": dtok[n + j]} for j in range(6)]
    client.insert_children(new)
    P = np.array([i // 4 for i in range(n)] + [2, 2, 16, 16, 16, 16], np.int32)
    assert idx.attribute("parent").cpu().tolist() == P.tolist() and client._parent_code["p900"] == 16

    def check(client, idx, P, tok, ids):
        rows = [client.store.row_index(c) for c in ids]
        ref = PC.parent_reference(qtok, tok, P, np.array([rows], np.int64))[0] / 32.0
        assert client.maxsim_scores("q", ids) == [float(v) for v in ref]
        hits = [SearchResult(chunk_id=c, content="", modality="text", source_document="d", page=1, chunk_index=0) for c in ids]
        out = Reranker(client=client, enabled=True).rerank_sync("q", hits, top_k=len(ids))
        by = {h.chunk_id: h.rerank_score for h in out}
        assert [h.chunk_id for h in out] == [ids[j] for j in O.rerank_order([float(v) for v in ref])]
        for a in ids:
            for b in ids:
                if P[client.store.row_index(a)] == P[client.store.row_index(b)]:
                    assert by[a] == by[b]           # siblings tie
        return by

    ids = ["c8", "c9", "c64", "c0", "c66", "c11", "c69", "c30"]
    by = check(client, idx, P, dtok[:n + 6], ids)
    assert by["c8"] == by["c64"] == by["c11"] and by["c66"] == by["c69"]
    # the family of p2 grew with the insert: its score is not the one of the four old rows alone
    assert by["c8"] >= PC.parent_reference(qtok, dtok[:n], P[:n], np.array([[8]], np.int64))[0, 0] / 32.0
    # delete a parent: its children leave the index and the column follows
    client.table("rag_parent_chunks").delete().eq("id", "p2").execute()
    keep = np.array([i for i in range(n + 6) if P[i] != 2])
    assert idx.n_docs == len(keep) and idx.attribute("parent").cpu().tolist() == P[keep].tolist()
    ids = ["c0", "c66", "c69", "c30", "c31", "c3"]
    check(client, idx, P[keep], dtok[keep], ids)
    # save -> load: the column comes back, a new client reads the numbering off it
    IB.save(hi, str(tmp_path / "ix"), idx)
    back = IB.load(str(tmp_path / "ix"))
    idx2 = back.to_gpu(shortlist="exact", token_store="fp8")
    assert idx2.attribute("parent").cpu().tolist() == P[keep].tolist()
    client2 = GpuIndexClient(idx2, back.store, org_id="org", token_embedder=Emb(), parent_rerank=True)
    assert client2._parent_code["p900"] == 16 and "p2" not in client2._parent_code
    assert check(client2, idx2, P[keep], dtok[keep], ids) == check(client, idx, P[keep], dtok[keep], ids)
