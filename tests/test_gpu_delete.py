"""Delete on the GPU: an index built from N rows and deleted from must equal, array for array and
result for result, a fresh index built from the surviving rows in their old order -- and the oracle
over those rows."""
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


def remap_of(keep):
    """old id -> new id (-1 = deleted): the exclusive scan of the keep mask."""
    return np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)


# --------------------------------------------------------------------------- thr_csr_compact alone
def _compact(rowptr, ids, pay, remap, id_base):
    """The numpy restatement: a boolean keep mask, its cumulative sum sampled at rowptr."""
    i = ids.astype(np.int64) - id_base
    ok = (i >= 0) & (i < len(remap))
    keep = np.zeros(len(ids), dtype=bool)
    keep[ok] = remap[i[ok]] >= 0
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    new_ids = (remap[i[keep]] + id_base).astype(np.int32)
    return before[rowptr], new_ids, pay[keep]


CASES = ["random", "nothing_deleted", "rows_emptied", "all_deleted", "long_row", "empty_rows", "id_base",
         "ids_outside"]


@pytest.mark.parametrize("case", CASES)
def test_csr_compact_equals_numpy_restatement(T, case):
    rng = np.random.default_rng(7)
    rows, n_ids, id_base = 3000, 5000, 0
    lens = rng.integers(0, 9, rows) * (rng.random(rows) < 0.6)          # many empty rows
    keep = rng.random(n_ids) < 0.7
    if case == "nothing_deleted":
        keep[:] = True
    elif case == "all_deleted":
        keep[:] = False
    elif case == "long_row":          # one row of ~1e6 entries among singletons: many workgroup slices
        lens = np.ones(rows, dtype=np.int64)
        lens[1717] = 1_000_003
        n_ids = 1_200_000
        keep = rng.random(n_ids) < 0.9
        keep[100_000:140_000] = False                                   # whole slices without a survivor
    elif case == "empty_rows":        # thousands of empty rows inside one slice, at both ends too
        rows = 40_000
        lens = np.zeros(rows, dtype=np.int64)
        lens[rng.integers(5000, 35_000, 300)] = rng.integers(1, 40, 300)
    elif case == "id_base":
        id_base = 1_000_000
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rowptr[-1])
    # id-ascending inside a row, as posting lists and mention lists are
    ids = np.concatenate([np.sort(rng.choice(n_ids, int(l), replace=False)) for l in lens if l] or
                         [np.zeros(0, dtype=np.int64)]).astype(np.int64) + id_base
    if case == "rows_emptied":        # everything in some rows goes
        for t in (0, 5, 1500, rows - 1):
            keep[ids[rowptr[t]:rowptr[t + 1]]] = False
    if case == "ids_outside":         # ids outside [id_base, id_base + n_ids) are dropped
        id_base = 700
        ids[::7] = rng.integers(0, 700, len(ids[::7]))
        ids[3::11] = 700 + n_ids + rng.integers(0, 50, len(ids[3::11]))
    ids = ids.astype(np.int32)
    pay = rng.random(nnz).astype(np.float32)
    remap = remap_of(keep)
    exp_rp, exp_ids, exp_pay = _compact(rowptr, ids, pay, remap, id_base)
    kept = len(exp_ids)
    N = T._native
    for two in (True, False):
        for extra in (0, 37):                      # into a capacity-reserved destination
            o_ids = torch.full((nnz + extra,), -7, dtype=torch.int32, device="cuda")
            o_pay = torch.full((nnz + extra,), -7.0, dtype=torch.float32, device="cuda") if two else None
            rp, oi, op, got = N.csr_compact(dev(rowptr), dev(ids), dev(pay) if two else None, dev(remap),
                                            id_base, o_ids, o_pay)
            assert got == kept and (op is None) == (not two)
            assert np.array_equal(rp.cpu().numpy(), exp_rp)
            assert np.array_equal(oi[:kept].cpu().numpy(), exp_ids)
            assert np.all(oi[kept:].cpu().numpy() == -7)                 # nothing written behind nnz_out
            if two:
                assert np.array_equal(op[:kept].cpu().numpy(), exp_pay)
                assert np.all(op[kept:].cpu().numpy() == -7.0)
    # destinations allocated by the wrapper; an int32 second payload (post_tf)
    rp, oi, op, got = N.csr_compact(dev(rowptr), dev(ids), dev(pay).view(torch.int32), dev(remap), id_base)
    assert got == kept and op.dtype == torch.int32
    assert np.array_equal(op[:kept].view(torch.float32).cpu().numpy(), exp_pay)
    # unaligned views (one element in): the element path
    if case in ("long_row", "random"):
        pad = lambda a: torch.cat([a[:1], a])[1:]
        rp, oi, op, got = N.csr_compact(dev(rowptr), pad(dev(ids)), pad(dev(pay)), dev(remap), id_base,
                                        torch.empty(nnz + 1, dtype=torch.int32, device="cuda")[1:],
                                        torch.empty(nnz + 3, dtype=torch.float32, device="cuda")[3:])
        assert got == kept and np.array_equal(rp.cpu().numpy(), exp_rp)
        assert np.array_equal(oi[:kept].cpu().numpy(), exp_ids) and np.array_equal(op[:kept].cpu().numpy(), exp_pay)


def test_csr_compact_without_entries_and_wrapper_refusals(T):
    N = T._native
    rowptr = torch.zeros(11, dtype=torch.int64, device="cuda")
    e32 = torch.zeros(0, dtype=torch.int32, device="cuda")
    rp, oi, op, got = N.csr_compact(rowptr, e32, e32.view(torch.float32), dev(remap_of(np.ones(4, bool))))
    assert got == 0 and rp.shape == (11,) and not rp.any() and oi.shape == (0,)
    ids = dev(np.arange(8, dtype=np.int32))
    rp8 = dev(np.array([0, 3, 8], dtype=np.int64))
    remap = dev(remap_of(np.ones(8, bool)))
    with pytest.raises(T.NativeError, match="4-byte"):
        N.csr_compact(rp8, ids, torch.zeros(8, dtype=torch.float64, device="cuda"), remap)
    with pytest.raises(T.NativeError, match="one per id"):
        N.csr_compact(rp8, ids, torch.zeros(7, dtype=torch.float32, device="cuda"), remap)
    with pytest.raises(T.NativeError, match="too small"):
        N.csr_compact(rp8, ids, None, remap, 0, torch.zeros(7, dtype=torch.int32, device="cuda"))
    with pytest.raises(T.NativeError, match="dtype"):
        N.csr_compact(rp8, ids.to(torch.int64), None, remap)


# --------------------------------------------------------------------------- deleted vs fresh
def _dense_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    x[11] = 0                                   # a row without an embedding
    x[n - 3] = 0
    return x, rng


def _delete_sets(n, coll, rng):
    """The shapes of delete the issue names -> {name: ids}."""
    return {"first": [0], "last": [n - 1], "tile": np.arange(64, 96), "run": np.arange(1000, 1077),
            "scattered": rng.choice(n, n // 100, replace=False), "collection": np.nonzero(coll == 1)[0],
            "repeats": np.array([5, 5, n - 1, 5, 4000]),
            # trailing rows only (the chunks just inserted are withdrawn): no row moves -- from a tile
            # edge on (nothing of the float16 image is rewritten either) and from inside a tile
            "tail_from_tile_edge": np.arange(n // 32 * 32 - 64, n), "tail_inside_tile": np.arange(n - 50, n)}


@pytest.mark.parametrize("shortlist", ["f16", "f16-inline", "f32", "exact"])
def test_dense_delete_equals_fresh_build(T, shortlist):
    n, d, nq, k = 9000 + 13, 768, 24, 50
    x, rng = _dense_rows(n, d, 21)
    x[17] *= 1e-3                               # the row with the largest float16 error: deleting it lowers doc_rel_err
    coll = rng.integers(0, 3, n).astype(np.int32)
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qc = np.array([-1, 0, 1, 2] * (nq // 4), dtype=np.int32)
    sets = _delete_sets(n, coll, rng)
    sets["row17"] = [17]
    for name, ids in sets.items():
        ids = np.asarray(ids, dtype=np.int64)
        keep = np.ones(n, dtype=bool)
        keep[ids] = False
        idx = T.GpuIndex().set_dense(x, shortlist=shortlist).set_collections(coll)
        if name == "scattered":                 # a smaller staging buffer: several chunks, a ragged last one
            idx.STAGING_BYTES = 1000 * d * 4
        remap = idx.delete_rows(torch.from_numpy(ids).cuda() if name == "run" else ids)
        assert remap.dtype == torch.int32 and np.array_equal(remap.cpu().numpy(), remap_of(keep)), name
        fresh = T.GpuIndex().set_dense(x[keep], shortlist=shortlist).set_collections(coll[keep])
        assert idx.n_docs == fresh.n_docs == int(keep.sum()) and idx.shortlist == fresh.shortlist == shortlist
        for a in ("docs", "dnorm", "inv_norm", "doc_coll"):
            same(getattr(idx, a), getattr(fresh, a), f"{name} {a}")
        assert idx.doc_rel_err == fresh.doc_rel_err, name
        assert (idx.docs16 is None) == (fresh.docs16 is None)
        if fresh.docs16 is not None:
            same(idx.docs16, fresh.docs16, f"{name} docs16")
        for c in (None, qc):
            same_results(idx.dense_search(dev(q), k, collections=c), fresh.dense_search(dev(q), k, collections=c),
                         f"dense_search {shortlist} {name}")
        if name in ("scattered", "first"):
            Se, Ie, _ = CO.dense_topk_exact(x[keep], q, k)
            S, I, _, _ = idx.dense_search(dev(q), k)
            assert np.array_equal(I.cpu().numpy(), Ie) and np.array_equal(S.cpu().numpy(), Se)
    # nothing to delete: the identity, nothing touched
    ptr = idx.docs.data_ptr()
    for nothing in (np.zeros(0, dtype=np.int64), [], torch.zeros(0, dtype=torch.int64, device="cuda")):
        ident = idx.delete_rows(nothing)
        assert ident.dtype == torch.int32 and np.array_equal(ident.cpu().numpy(), np.arange(idx.n_docs))
    assert idx.docs.data_ptr() == ptr and idx._mutations == 1


def test_delete_refusals_leave_the_index_as_it_was(T):
    x, _ = _dense_rows(3000, 768, 4)
    idx = T.GpuIndex().set_dense(x, shortlist="f16")
    for bad, msg in (([3000], "local doc ids"), ([-1], "local doc ids"), (np.array([0.5]), "integer"),
                     (np.arange(3000), "build a new index"), (torch.arange(3000).cuda().repeat(2), "build a new index")):
        with pytest.raises(T.NativeError, match=msg):
            idx.delete_rows(bad)
    assert idx.n_docs == 3000 and idx.docs.shape[0] == 3000
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    with pytest.raises(T.NativeError, match="not supported"):
        ShardedIndex.delete_rows(object(), [0])
    # an index that failed in its in-place phase refuses everything afterwards
    idx._unusable = "this index is unusable: test"
    for call in (lambda: idx.dense_search(dev(x[:2]), 5), lambda: idx.delete_rows([1]), lambda: idx.append_rows(x[:1])):
        with pytest.raises(T.NativeError, match="unusable"):
            call()


def _lex_rows(n, v, seed, everywhere=None):
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


def test_lexical_delete_equals_fresh_build(T):
    n, v = 20011, 3000
    doc, term, tf = _lex_rows(n, v, 31, everywhere=7)             # skewed: term 7 is in every doc
    rng = np.random.default_rng(33)
    # term 2999: dense before the delete (6 % of the docs), sparse after; term 2998 only in deleted docs
    hot = rng.choice(n, n * 6 // 100, replace=False).astype(np.int32)
    doc = np.concatenate([doc, hot, hot[:40]])
    term = np.concatenate([term, np.full(len(hot), 2999, np.int32), np.full(40, 2998, np.int32)])
    tf = np.concatenate([tf, np.ones(len(hot) + 40, np.int32)])
    gone = np.unique(np.concatenate([hot[: len(hot) * 3 // 4], doc[term == 2998], rng.choice(n, 200), [0, n - 1]]))
    keep = np.ones(n, dtype=bool)
    keep[gone] = False
    rm = remap_of(keep)
    sel = keep[doc]
    fresh = T.GpuIndex()
    fresh.set_lexical_rows(rm[doc[sel]], term[sel], tf[sel], v, n_docs=int(keep.sum()), dense_share=0.05)
    idx = T.GpuIndex()
    idx.set_lexical_rows(doc, term, tf, v, n_docs=n, dense_share=0.05)
    assert idx.lex["dense"][0].cpu().numpy()[2999] >= 0
    got = idx.delete_rows(gone[::-1].copy())                       # any order
    assert np.array_equal(got.cpu().numpy(), rm)
    assert fresh.lex["dense"][0].cpu().numpy()[2999] < 0 and int(fresh.df_local[2998]) == 0
    _assert_lex_equal(idx, fresh)
    rowptr, pd, ptf, dl = (fresh.lex[k].cpu().numpy() for k in ("rowptr", "post_doc", "post_tf", "doclen"))
    idf = fresh.lex["idf"].cpu().numpy()
    qt = np.full((12, 4), -1, dtype=np.int32)
    qt[:, :3] = rng.integers(0, v, (12, 3))
    qt[0] = [7, 2999, 3, -1]
    qt[1, :2] = [2998, 2999]
    for conj in (False, True):
        same_results(idx.bm25_search(dev(qt), 50, conjunctive=conj), fresh.bm25_search(dev(qt), 50, conjunctive=conj),
                     f"bm25 conjunctive={conj}")
    Se, Ie = O.bm25_topk(rowptr, pd, ptf, dl, idf, fresh.lex["avgdl"], qt, int(keep.sum()), 50)
    S, I, cnt = idx.bm25_search(dev(qt), 50)
    for i in range(len(qt)):
        c = int(cnt[i])
        assert c == len(Ie[i]) and np.array_equal(I[i, :c].cpu().numpy(), Ie[i]) \
            and np.array_equal(S[i, :c].cpu().numpy(), Se[i])
    coll = rng.integers(0, 3, int(keep.sum())).astype(np.int32)
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
    me[: n // 2] = 3                                              # a hub entity
    mc = rng.integers(0, n, n * per).astype(np.int64)
    mw = rng.uniform(0.5, 1.0, n * per).astype(np.float32)
    return ent_rowptr, ent_col, me, mc, mw


def _men_csr(me, mc, mw, n_ent):
    order = np.lexsort((mc, me))
    rp = np.concatenate([[0], np.cumsum(np.bincount(me, minlength=n_ent))]).astype(np.int64)
    return rp, mc[order].astype(np.int32), mw[order]


def test_triple_hybrid_delete_append_delete_equals_fresh_build(T):
    from triple_hybrid_rag_amd import synth
    n, d, v, n_ent, base = 12000 + 5, 768, 2000, 6000, 1000
    n0 = n - 1500                                                  # rows [n0, n) arrive by append, between two deletes
    x, rng = _dense_rows(n, d, 41)
    doc, term, tf = _lex_rows(n, v, 42)
    ent_rowptr, ent_col, me, mc, mw = _graph(rng, n_ent, n)
    dtok = synth.doc_tokens(0, n, 32, 64)

    def build(keep):
        """An index over the rows of the mask, in their order."""
        rm = remap_of(keep)
        sel, msel = keep[doc], keep[mc]
        rp, c, w = _men_csr(me[msel], rm[mc[msel]].astype(np.int64) + base, mw[msel], n_ent)
        idx = T.GpuIndex(doc_base=base).set_dense(x[keep], shortlist="f16")
        idx.set_lexical_rows(rm[doc[sel]], term[sel], tf[sel], v, n_docs=int(keep.sum()))
        return idx.set_graph(ent_rowptr, ent_col, rp, c, w).set_tokens(dtok[keep])

    first = np.arange(n) < n0
    idx = build(first)
    idx.reserve_rows(n + 100)
    cap, ptr = idx.capacity_rows(), idx.docs.data_ptr()
    nq = 16
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qt = rng.integers(0, v, (nq, 4)).astype(np.int32)
    seeds = rng.integers(0, n_ent, (nq, 3)).astype(np.int32)
    seeds[0] = [3, -1, -1]
    qtok = synth.query_tokens(nq, 32, 64)
    idx.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok))     # (caches sized for n0 exist)
    # delete 1: a "document" of 64 consecutive chunks + scattered rows
    gone1 = np.unique(np.concatenate([np.arange(2048, 2112), rng.choice(n0, 150, replace=False)]))
    alive = first.copy()
    alive[gone1] = False
    # phase 2 of a delete (the in-place moves, then the swap) allocates no device memory: not one
    # request reaches the caching allocator while either runs
    allocated = []

    def counted(fn):
        def call(*args):
            before = torch.cuda.memory_stats()["allocation.all.allocated"]
            out = fn(*args)
            allocated.append(torch.cuda.memory_stats()["allocation.all.allocated"] - before)
            return out
        return call
    idx._move_rows, idx._commit = counted(idx._move_rows), counted(idx._commit)
    r1 = idx.delete_rows(gone1)
    del idx._move_rows, idx._commit
    assert allocated == [0, 0]
    assert idx.capacity_rows() == cap and idx.docs.data_ptr() == ptr    # the reservation survives, nothing reallocated
    # append the rest (local ids continue behind the survivors)
    sel, msel = doc >= n0, mc >= n0
    idx.append_rows(x[n0:], lex=(doc[sel] - n0, term[sel], tf[sel], v), tokens=dtok[n0:],
                    mentions=(me[msel], mc[msel] - n0, mw[msel]))
    alive[n0:] = True
    assert idx.docs.data_ptr() == ptr
    # delete 2: old and appended rows, addressed by their CURRENT local ids
    cur = remap_of(alive)
    gone2 = np.concatenate([rng.choice(n0, 60, replace=False), np.arange(n - 40, n - 8), [n - 1]])
    gone2 = gone2[alive[gone2]]
    r2 = idx.delete_rows(torch.from_numpy(cur[gone2].astype(np.int64)).cuda())
    before2 = alive.copy()
    alive[gone2] = False
    assert np.array_equal(r1.cpu().numpy(), remap_of(np.where(first, ~np.isin(np.arange(n), gone1), False)[:n0]))
    assert np.array_equal(r2.cpu().numpy(), remap_of(alive[before2]))
    fresh = build(alive)
    assert idx.n_docs == fresh.n_docs == int(alive.sum())
    for k in ("men_rowptr", "men_chunk", "men_conf", "ent_rowptr", "ent_col"):
        same(idx.graph[k], fresh.graph[k], k)
    same(idx.docs, fresh.docs, "docs")
    same(idx.tokens, fresh.tokens, "tokens")
    same(idx.docs16, fresh.docs16, "docs16")
    same(idx.dnorm, fresh.dnorm, "dnorm")
    same(idx.inv_norm, fresh.inv_norm, "inv_norm")
    assert idx.doc_rel_err == fresh.doc_rel_err
    _assert_lex_equal(idx, fresh)
    for hops in (0, 1, 2):
        same_results(idx.graph_search(dev(seeds), 50, hops), fresh.graph_search(dev(seeds), 50, hops), "graph")
    for a, b in zip(idx._graph_transposed(), fresh._graph_transposed()):
        same(a, b, "transposed mentions")
    m = int(alive.sum())
    cand = rng.integers(base, base + m, (nq, 40)).astype(np.int64)
    same(idx.maxsim(dev(qtok), dev(cand)), fresh.maxsim(dev(qtok), dev(cand)), "maxsim")
    g1 = idx.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok))
    g2 = fresh.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok))
    same_results((g1.ids, g1.scores, g1.counts), (g2.ids, g2.scores, g2.counts), "retrieve_batch")
    for ch in ("semantic", "lexical", "graph"):
        same_results(g1.channels[ch], g2.channels[ch], ch)
    assert int(g1.rescued) == int(g2.rescued)
    ids = g1.ids.cpu().numpy()
    assert ids[ids >= 0].max() < base + m                                # no id behind the survivors
    # the oracle over the surviving rows
    Se, Ie, _ = CO.dense_topk_exact(x[alive], q, 20)
    S, I, _, _ = idx.dense_search(dev(q), 20)
    assert np.array_equal(I.cpu().numpy(), Ie + base) and np.array_equal(S.cpu().numpy(), Se)
    e1, e2 = idx.export_derived(), fresh.export_derived()
    assert sorted(e1) == sorted(e2)
    for key, val in e2.items():
        assert np.array_equal(np.asarray(e1[key]).view(np.uint8) if isinstance(val, np.ndarray) else e1[key],
                              val.view(np.uint8) if isinstance(val, np.ndarray) else val), key


@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("first", [4096, 4100, 40])
def test_trailing_and_leading_deletes_with_a_token_store_equal_fresh_build(T, first, pack, tmp_path):
    """Deleting exactly the last rows moves nothing, from a tile edge on not even float16 tiles: every
    per-row array must still come out at the new length.  first = 40: nearly everything goes."""
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd import synth
    n, d, v, n_ent, base = 5000 + 7, 512, 800, 500, 300
    x, rng = _dense_rows(n, d, 71)
    doc, term, tf = _lex_rows(n, v, 72)
    ent_rowptr, ent_col, me, mc, mw = _graph(rng, n_ent, n)
    dtok = synth.doc_tokens(0, n, 32, 64)
    coll = rng.integers(0, 3, n).astype(np.int32)

    def build(rows):
        sel, msel = doc < rows, mc < rows
        rp, c, w = _men_csr(me[msel], mc[msel] + base, mw[msel], n_ent)
        idx = T.GpuIndex(doc_base=base).set_dense(x[:rows], shortlist="f16").set_collections(coll[:rows])
        idx.set_lexical_rows(doc[sel], term[sel], tf[sel], v, n_docs=rows)
        return idx.set_graph(ent_rowptr, ent_col, rp, c, w).set_tokens(dtok[:rows], pack=pack)

    idx, fresh = build(n), build(first)
    remap = idx.delete_rows(np.arange(first, n)[::-1].copy())
    assert np.array_equal(remap.cpu().numpy(), np.where(np.arange(n) < first, np.arange(n), -1))
    assert idx.n_docs == first == fresh.n_docs
    for a in ("docs", "docs16", "dnorm", "inv_norm", "doc_coll", "tokens"):
        same(getattr(idx, a), getattr(fresh, a), a)
    assert idx.doc_rel_err == fresh.doc_rel_err and idx.capacity_rows() == n
    _assert_lex_equal(idx, fresh)
    for k in ("men_rowptr", "men_chunk", "men_conf"):
        same(idx.graph[k], fresh.graph[k], k)
    nq = 8
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qt = rng.integers(0, v, (nq, 4)).astype(np.int32)
    seeds = rng.integers(0, n_ent, (nq, 3)).astype(np.int32)
    qtok = synth.query_tokens(nq, 32, 64)
    tops = dict(semantic_top_k=20, lexical_top_k=20, graph_top_k=20, rerank_top_k=10)
    g1 = idx.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok), **tops)
    g2 = fresh.retrieve_batch(dev(q), dev(qt), dev(seeds), qtok=dev(qtok), **tops)
    same_results((g1.ids, g1.scores, g1.counts), (g2.ids, g2.scores, g2.counts), "retrieve_batch")
    # candidates among the deleted rows' old ids score -inf, as ids outside the shard do
    cand = np.tile(np.array([base, base + first - 1, base + first, base + n - 1], dtype=np.int64), (nq, 1))
    same(idx.maxsim(dev(qtok), dev(cand)), fresh.maxsim(dev(qtok), dev(cand)), "maxsim")
    assert torch.isinf(idx.maxsim(dev(qtok), dev(cand))[:, 2:]).all()
    # the float64 scorer takes n from the rows: it must agree with the norms' length
    Se, Ie, _ = CO.dense_topk_exact(x[:first], q, 10)
    idx.shortlist = "exact"
    S, I, _, _ = idx.dense_search(dev(q), 10)
    assert np.array_equal(I.cpu().numpy(), Ie + base) and np.array_equal(S.cpu().numpy(), Se)
    idx.shortlist = "f16"
    # a save pulls the rows of the index as it stands
    hi = IB.HostIndex(docs=x.copy(), tokens=None if pack else dtok.copy())
    IB.refresh_from_gpu(hi, idx)
    assert hi.docs.shape == (first, d) and np.array_equal(hi.docs, x[:first])
    if not pack:
        assert np.array_equal(hi.tokens, dtok[:first])
    # and the rows can come back behind the survivors: equal to the index that never lost them
    if first != 40:
        sel, msel = doc >= first, mc >= first
        idx.append_rows(x[first:], lex=(doc[sel] - first, term[sel], tf[sel], v), collections=coll[first:],
                        tokens=dtok[first:], mentions=(me[msel], mc[msel] - first, mw[msel]))
        full = build(n)
        for a in ("docs", "docs16", "dnorm", "inv_norm", "doc_coll", "tokens"):
            same(getattr(idx, a), getattr(full, a), "re-appended " + a)
        _assert_lex_equal(idx, full)
        assert idx.doc_rel_err == full.doc_rel_err


# --------------------------------------------------------------------------- drop-in surface
def _child_rows(n, d, seed):
    rng = np.random.default_rng(seed)
    words = [f"w{i}" for i in range(400)]
    rows = []
    for i in range(n):
        text = " ".join(rng.choice(words, 10)) + f" doc{i}"
        rows.append({"id": f"c{i}", "parent_id": f"p{i // 4}", "document_id": f"d{i // 48}", "text": text,
                     "page": None if i % 7 == 0 else i % 9 + 1, "modality": "text",
                     "embedding_1024": None if i == 13 else rng.standard_normal(d).astype(np.float32).tolist(),
                     "content_hash": f"h{i}", "org_id": "org"})
    parents = [{"id": f"p{j}", "text": f"parent text {j}", "section_heading": f"S{j}"} for j in range((n + 3) // 4)]
    return rows, parents


def test_dropin_delete_document_reinsert_save_load(T, tmp_path):
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
    client.table("rag_parent_chunks").insert(parents[n0 // 4:]).execute()
    tbl().insert(rows[n0:]).execute()
    target = rows[7 * 48 + 21]                                      # a chunk of document d7
    emb = np.asarray(target["embedding_1024"], dtype=np.float32)

    def search(c):
        sem = c.rpc("rag2_semantic_search", {"p_org_id": "org", "p_embedding": emb.tolist(), "p_limit": 20}).data
        lex = c.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": target["text"], "p_limit": 20}).data
        return sem, list(lex)
    sem, lex = search(client)
    assert sem[0]["child_id"] == target["id"] and lex[0]["child_id"] == target["id"]
    # a deferred lexical reply issued before the delete resolves against the rows as they were
    pending = client.rpc("rag2_lexical_search", {"p_org_id": "org", "p_query": target["text"], "p_limit": 20,
                                                 "_defer": True}).data
    # the document is withdrawn: its 48 chunks and their 12 parents go
    assert client.table("rag_documents").delete().eq("org_id", "other").eq("id", "d7").execute().data == []
    assert client.table("rag_documents").delete().eq("org_id", "org").eq("id", "d7").execute().data == [{"id": "d7"}]
    assert list(pending) == lex
    assert client.index.n_docs == n - 48 == len(client.store.child_ids)
    assert tbl().select("*").in_("id", [target["id"]]).execute().data == []
    assert client.table("rag_parent_chunks").select("*").in_("id", [target["parent_id"]]).execute().data == []
    sem, lex = search(client)
    assert sem and lex and all(r["document_id"] != "d7" for r in sem + lex)
    # the same state as a bulk build from the surviving rows
    left = [r for r in rows if r["document_id"] != "d7"]
    ref = IB.from_rows(left, [p for p in parents if not 84 <= int(p["id"][1:]) <= 95])
    refc = GpuIndexClient(ref.to_gpu(), ref.store, org_id="org")
    same(client.index.docs, refc.index.docs, "docs")
    same(client.index.lex["doclen"], refc.index.lex["doclen"], "doclen")
    assert search(refc) == (sem, lex)
    # an update: the same content hashes come back (ingest.py:388-391 would have skipped them before)
    assert tbl().select("content_hash").in_("content_hash", [target["content_hash"]]).execute().data == []
    client.table("rag_parent_chunks").insert([p for p in parents if 84 <= int(p["id"][1:]) <= 95]).execute()
    again = [r for r in rows if r["document_id"] == "d7"]
    assert tbl().insert(again).execute().data == [{"id": r["id"]} for r in again]
    assert client.index.n_docs == n
    sem, lex = search(client)
    assert sem[0]["child_id"] == target["id"] and lex[0]["child_id"] == target["id"]
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
        assert res.contexts[0].parent_text == f"parent text {(7 * 48 + 21) // 4}"
    finally:
        SETTINGS.__dict__.update(saved)
    # one more delete, so that the row count equals an earlier one: save must still write the current state
    tbl().delete().in_("id", [r["id"] for r in rows[n0:]]).execute()
    assert client.index.n_docs == n0 == len(hi.docs)
    first = search(client)
    path = str(tmp_path / "idx")
    IB.save(hi, path, client.index)
    back = IB.load(path)
    assert list(back.store.child_ids) == client.store.child_ids and back.store.pages == client.store.pages
    assert list(back.store.content_hashes) == client.store.content_hashes
    c2 = GpuIndexClient(back.to_gpu(), back.store, org_id="org")
    same(c2.index.docs, client.index.docs, "loaded docs")
    assert client.index.shortlist == c2.index.shortlist == "f16"
    same(c2.index.docs16, client.index.docs16, "loaded docs16")
    for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"):
        same(c2.index.lex[k], client.index.lex[k], "loaded " + k)
    for j in range(3):
        same(c2.index.lex["bounds"][j], client.index.lex["bounds"][j], f"loaded bounds[{j}]")
    assert search(c2) == first
    assert c2.store.has_hash(target["content_hash"]) and not c2.store.has_hash(rows[n - 1]["content_hash"])
