"""The runtime-dim f16 scan (shortlist="f16-anydim", csrc/dense_scan_anydim.hpp) against the float64
oracle: ids, scores (bits) and counts of CO.dense_topk_exact at every row length at which something can
break -- one K step, fewer chunks than the rescoring keeps in flight, a chunk count that is no multiple of
8, an odd one, the smallest query tile -- on the unsampled and the sampled path.

An uncertified query is redone exhaustively and would pass whatever the scan emitted, so every case also
asserts, on the flags BEFORE the rescue, that only the built-in degenerate queries are uncertified."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import c_oracle as CO  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_cases import (DOC_BASE, TIE_QUERY, ZERO_QUERY, assert_topk_equal, dev, floor_search,  # noqa: E402
                         planted, planted_oracle, rand_docs)

MODE = "f16-anydim"
DIMS = (32, 96, 384, 1536, 2048, 4000, 4096)


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def sampled_rows(d):
    return 20011 if d <= 1536 else 9001     # (keeps the CPU oracle to a few seconds)


def check_flags(flags, what):
    """Only the zero query and (if it is) the tie query may lack the certificate: at most 2 of 70."""
    bad = set(np.nonzero((flags & 1) == 0)[0].tolist())
    assert ZERO_QUERY in bad, f"{what}: the zero query is never certified"
    assert bad <= {ZERO_QUERY, TIE_QUERY}, f"{what}: uncertified plain queries {sorted(bad)}"
    return len(bad)


@pytest.mark.parametrize("path", ["unsampled", "sampled"])
@pytest.mark.parametrize("d", DIMS)
def test_anydim_shortlist_is_exact(T, d, path):
    """n = 3001: no sample pass (n <= 8192), every row a candidate, a ragged last tile of 25 rows;
    n = 20011 / 9001: the sampled threshold.  70 queries = two to five query tiles with a partial last
    one; k = 100 at k' = 192; doc_base != 0."""
    n = 3001 if path == "unsampled" else sampled_rows(d)
    x, q = planted(n, d)
    idx = T.GpuIndex(doc_base=DOC_BASE).set_dense(x, shortlist=MODE)
    assert idx.shortlist == MODE and idx.docs16 is None          # no second copy of the corpus
    assert 0 < idx.doc_rel_err < 6e-4
    nz = x.any(axis=1)
    rel = (np.linalg.norm(x.astype(np.float16).astype(np.float64) - x, axis=1)[nz]
           / np.linalg.norm(x.astype(np.float64), axis=1)[nz])
    assert rel.max() <= idx.doc_rel_err
    assert idx.max_batch() == 1 << 30
    tile = T._native.dense_f16_query_tile(d, False, 70)
    assert tile == (64 if d <= 768 else 32 if d <= 1536 else 16)
    Se, Ie, cnte = planted_oracle(n, d, 100)
    qd = dev(q)
    # the entry point itself: flags before any rescue, and certified queries are already the oracle's
    S, I, cnt, flg = T._native.dense_topk_f16(idx.docs, None, idx.doc_rel_err, idx.dnorm, idx.inv_norm, qd,
                                              100, 192, DOC_BASE)
    flags = flg.cpu().numpy()
    n_bad = check_flags(flags, f"d={d} n={n}")
    assert not np.any(flags & T._native.THR_FLAG_OVERFLOW)
    ok = np.nonzero(flags & 1)[0]
    assert_topk_equal(S[ok], I[ok], cnt[ok], [Se[i] for i in ok], [Ie[i] for i in ok], [cnte[i] for i in ok],
                      f"anydim-native d={d}")
    S, I, cnt, nres = idx.dense_search(qd, 100)
    assert nres <= n_bad
    assert_topk_equal(S, I, cnt, Se, Ie, cnte, f"anydim d={d} n={n}")
    # a batch of one (a single, mostly padded query tile; the rows stream non-temporally)
    S1, I1, c1, n1 = idx.dense_search(qd[2:3], 100)
    assert n1 == 0
    assert_topk_equal(S1, I1, c1, Se[2:3], Ie[2:3], cnte[2:3], f"anydim d={d} single query")


@pytest.mark.parametrize("d", [96, 4000])
def test_anydim_top10(T, d):
    n = sampled_rows(d)
    x, q = planted(n, d)
    idx = T.GpuIndex(doc_base=DOC_BASE).set_dense(x, shortlist=MODE)
    S, I, cnt, nres = idx.dense_search(dev(q), 10)
    assert nres <= 2
    Se, Ie, cnte = planted_oracle(n, d, 10)
    assert_topk_equal(S, I, cnt, Se, Ie, cnte, f"anydim top-10 d={d}")


@pytest.mark.parametrize("d", [768, 1024])
def test_anydim_beside_the_tuned_kernel(T, d):
    """Where both kernels exist the flavour runs the runtime-dim one: identical (S, I, cnt) and the same
    certificates as "f16-inline" on the planted inputs, and both the oracle's."""
    n = 20011
    x, q = planted(n, d)
    qd = dev(q)
    a = T.GpuIndex(doc_base=DOC_BASE).set_dense(x, shortlist=MODE)
    b = T.GpuIndex(doc_base=DOC_BASE).set_dense(x, shortlist="f16-inline")
    assert a.doc_rel_err == b.doc_rel_err and a.docs16 is None
    N = T._native
    with N.dense_f16_flavour(True):
        # (the library ignores a selection it cannot honour: make sure the other kernel is what runs)
        assert N.load().thr_dense_f16_select(-1) == N.THR_DENSE_F16_ANYDIM
        fa = N.dense_topk_f16(a.docs, None, a.doc_rel_err, a.dnorm, a.inv_norm, qd, 100, 192, DOC_BASE)[3]
    fb = N.dense_topk_f16(b.docs, None, b.doc_rel_err, b.dnorm, b.inv_norm, qd, 100, 192, DOC_BASE)[3]
    assert N.load().thr_dense_f16_select(-1) == N.THR_DENSE_F16_BY_DIM
    check_flags(fa.cpu().numpy(), f"anydim at {d}")
    assert torch.equal(fa & 1, fb & 1)
    ra, rb = a.dense_search(qd, 100), b.dense_search(qd, 100)
    assert torch.equal(ra[0], rb[0]) and torch.equal(ra[1], rb[1]) and torch.equal(ra[2], rb[2])
    assert ra[3] == rb[3] <= 2
    assert_topk_equal(*ra[:3], *planted_oracle(n, d, 100), f"anydim at {d}")


def test_anydim_collection_filter_before_topk(T):
    """The collection filter is applied as rows pass tau, a 2 % collection thinner than k included."""
    n, d, k = 20011, 384, 20
    x, rng = rand_docs(n, d, 23)
    x[77] = 0
    coll = (np.arange(n) * 7919 % 50).astype(np.int32)
    coll[n // 2:] = np.where(np.arange(n - n // 2) % 2 == 0, 60, coll[n // 2:])
    coll[coll == 33] = 34
    coll[[5, 6000, 12000]] = 33                       # a collection of 3 rows: thinner than k
    q = rng.standard_normal((9, d)).astype(np.float32)
    q[:4] = x[[5, 6000, 11000, n - 1]] + 0.5 * q[:4]
    qc = np.array([7, 60, -1, 7, 60, 12345, -1, 33, 60], dtype=np.int32)
    idx = T.GpuIndex(doc_base=500).set_dense(x, shortlist=MODE).set_collections(coll)
    S, I, cnt, nres = idx.dense_search(dev(q), k, collections=dev(qc))
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    dn = O.doc_norms_f64(x)
    for i in range(9):
        s = O.cosine_scores_f64(x, q[i], dn)
        if qc[i] != -1:
            s[coll != qc[i]] = -np.inf
        ts, ti = O.topk_desc(s, k)
        assert cnt[i] == len(ti) and np.array_equal(I[i, :len(ti)], ti + 500), (i, qc[i])
        assert np.array_equal(S[i, :len(ti)], ts)
    assert cnt[5] == 0 and cnt[7] == 3
    _, _, _, flg = T._native.dense_topk_f16(idx.docs, None, idx.doc_rel_err, idx.dnorm, idx.inv_norm, dev(q), k,
                                            192, 500, doc_coll=idx.doc_coll, query_coll=dev(qc))
    flg = flg.cpu().numpy()
    # (a collection too thin for the sampled threshold ends on the exhaustive path: thr_hip.h)
    assert all(flg[i] & 1 for i in range(9) if i not in (5, 7)), flg
    assert nres <= 2


def test_anydim_scopes_narrow_and_wide(T):
    """One scopes=[...] batch: a wide scope runs the scan with the scope's labels, a narrow one the row
    list (thr_dense_topk_rows), None the plain scan."""
    n, d, k = 20011, 384, 10
    x, rng = rand_docs(n, d, 3)
    org = rng.integers(1, 9, n).astype(np.int32)
    org[: n // 2] = 0                                 # a wide tenant, eight thin ones
    idx = T.GpuIndex().set_dense(x, shortlist=MODE).set_attributes({"org": org})
    q = rng.standard_normal((6, d)).astype(np.float32)
    q[:3] = x[[7, 15000, 19000]] + 0.5 * q[:3]
    scopes = [{"org": 0}, None, {"org": 3}, {"org": 0}, {"org": 77}, {"org": 5}]
    S, I, cnt, _ = idx.dense_search(dev(q), k, scopes=scopes, scope_rows_max=6000)
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    dn = O.doc_norms_f64(x)
    for i, sc in enumerate(scopes):
        s = O.cosine_scores_f64(x, q[i], dn)
        if sc is not None:
            s[org != sc["org"]] = -np.inf
        ts, ti = O.topk_desc(s, k)
        assert cnt[i] == len(ti) and np.array_equal(I[i, :len(ti)], ti) and np.array_equal(S[i, :len(ti)], ts), (i, sc)
    assert cnt[4] == 0


def test_anydim_shard_floor(T):
    """3 shards in one process: shortlist -> stacked bounds -> thr_dense_floor -> finish -> thr_merge_topk
    equals the unsharded oracle, every shard's list certified by the shortlist path."""
    n, d, nq, k = 30011, 384, 20, 100
    x, rng = rand_docs(n, d, 41)
    x[n // 3] = 0
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[:3] = x[[11, n // 2, n - 5]] + 0.3 * q[:3]
    (S, I, cnt), flags, nres = floor_search(T, x, q, k, 3, MODE)
    Se, Ie, cnte = CO.dense_topk_exact(x, q, k)
    assert_topk_equal(S, I, cnt, Se, Ie, cnte, "anydim shard floor")
    assert sum(nres) == 0 and np.all(flags & 1)


def test_anydim_candidate_list_overflow_goes_to_rescue(T):
    """60 queries sit on a 20 000-row cluster of near-duplicates: 1.2M rows pass tau in a query tile whose
    shared list holds 64 x 8192.  The queries are flagged, rescued and exact."""
    n, d, nq, ndup = 60000, 96, 96, 20000
    x, rng = rand_docs(n, d, 17)
    x[30000:30000 + ndup] = x[29999]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[:60] = x[29999] + 1e-3 * q[:60]
    q[60:80] = x[rng.integers(0, 29999, 20)] + 0.5 * q[60:80]
    idx = T.GpuIndex().set_dense(x, shortlist=MODE)
    idx.reserve(nq, 100)
    idx._ws.fill_(0xFF)
    qd = dev(q)
    S, I, cnt, flg = T._native.dense_topk_f16(idx.docs, None, idx.doc_rel_err, idx.dnorm, idx.inv_norm, qd,
                                              100, 192, 0, idx._ws)
    flags = flg.cpu().numpy()
    over = T._native.THR_FLAG_OVERFLOW
    assert np.all(flags[:60] & over) and np.all((flags[:60] & 1) == 0)
    assert np.any(flags[60:64] & over), "the rest of the cluster's tile shares the overflowed list"
    assert np.all((flags[(flags & over) != 0] & 1) == 0)
    idx._ws.fill_(0xFF)
    S, I, cnt, nres = idx.dense_search(qd, 100)
    assert nres >= 60
    Se, Ie, cnte = CO.dense_topk_exact(x, q, 100)
    assert_topk_equal(S, I, cnt, Se, Ie, cnte, "anydim overflow")
    assert list(I[0, :100].cpu().numpy()) == list(range(29999, 30099))


def test_anydim_refuses_what_it_cannot_hold(T):
    x, _ = rand_docs(3000, 384, 5)
    bad = x.copy()
    bad[17, 3] = 1e6                                  # rounds to +inf in float16
    with pytest.raises(T._native.NativeError, match="float16"):
        T.GpuIndex().set_dense(bad, shortlist=MODE)
    for d in (48, 4128):
        with pytest.raises(T._native.NativeError, match="32.*4096"):
            T.GpuIndex().set_dense(np.ones((40, d), np.float32), shortlist=MODE)


def test_anydim_append_then_delete_equals_a_fresh_build(T):
    n, d, k = 9013, 1536, 50
    rng = np.random.default_rng(21)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    x[11] = 0
    x[n - 3] = 0
    q = x[rng.integers(0, n, 24)] + 0.3 * rng.standard_normal((24, d)).astype(np.float32)
    q[0] = x[n - 1] * 2.0                             # its true top-1 is an appended row
    n0 = 8500
    idx = T.GpuIndex().set_dense(x[:n0], shortlist=MODE)
    assert idx.append_rows(x[n0:n0 + 33]) == range(n0, n0 + 33)
    idx.append_rows(x[n0 + 33:])
    gone = np.concatenate([np.arange(100, 164), [5, 4000, n - 2], np.arange(8600, 8700)])
    idx.delete_rows(gone)
    keep = np.setdiff1d(np.arange(n), gone)
    fresh = T.GpuIndex().set_dense(x[keep], shortlist=MODE)
    assert idx.shortlist == fresh.shortlist == MODE and idx.docs16 is None and idx.n_docs == len(keep)
    for name in ("docs", "dnorm", "inv_norm"):
        assert torch.equal(getattr(idx, name), getattr(fresh, name)), name
    assert idx.doc_rel_err == fresh.doc_rel_err
    got, exp = idx.dense_search(dev(q), k), fresh.dense_search(dev(q), k)
    assert all(torch.equal(a, b) for a, b in zip(got[:3], exp[:3])) and got[3] == exp[3]
    Se, Ie, cnte = CO.dense_topk_exact(x[keep], q, k)
    assert_topk_equal(*got[:3], Se, Ie, cnte, "anydim append + delete")
    assert int(got[1][0, 0]) == len(keep) - 1


@pytest.fixture(scope="module")
def legacy_store(T):
    """The legacy RAG 1.0 store's row length (config.py:216, 20260113_halfvec_4000.sql:70-105)."""
    n, d = 3000, 4000
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[7] = 0.0                                        # a chunk without an embedding
    q = rng.standard_normal((6, d)).astype(np.float32)
    idx = T.GpuIndex().set_dense(x, shortlist=MODE)
    return idx, q, CO.dense_topk_exact(x, q, 100)


def test_anydim_retrieve_batch_at_4000_dims(T, legacy_store):
    idx, q, (Se, Ie, _) = legacy_store
    res = idx.retrieve_batch(dev(q), top_k=10)        # dense -> RRF
    for i in range(6):
        assert list(res.ids[i].cpu().numpy()) == O.fused_topk_ids(None, list(Ie[i]), None, 10)[0]


def test_anydim_legacy_vector_search_rpc_at_4000_dims(T, legacy_store):
    from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
    idx, q, (Se, Ie, _) = legacy_store
    client = GpuIndexClient(idx, CorpusStore.synthetic(idx.n_docs), org_id="org")
    rows = client.rpc("kb_chunks_vector_search", {"p_org_id": "org", "p_embedding": q[2].tolist(),
                                                  "p_limit": 5}).execute().data
    assert [r["id"] for r in rows] == [f"c{i}" for i in Ie[2][:5]]
    assert [r["similarity"] for r in rows] == [float(v) for v in Se[2][:5]]


def test_anydim_through_a_built_index(T):
    """index_build: BuiltIndex.to_gpu(shortlist=...) hands the flavour to set_dense."""
    from triple_hybrid_rag_amd import index_build
    x, q = planted(3001, 384)
    hi = index_build.HostIndex(docs=np.array(x))
    idx = hi.to_gpu(doc_base=DOC_BASE, shortlist=MODE)
    assert idx.shortlist == MODE
    S, I, cnt, _ = idx.dense_search(dev(q), 100)
    assert_topk_equal(S, I, cnt, *planted_oracle(3001, 384, 100), "to_gpu")
