"""The operand contracts of the binding (_native) on the device: what dense_rescue and dense_finish_f16
now refuse is refused before anything is launched, what dense_rescue took before it still takes with
the same result, and the one workspace rule (_workspace) gives every call the same outputs whether the
caller brings no workspace or one that is too small."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

N_DOCS, DIM, NQ, K, KPRIME = 64, 256, 3, 10, 38
SENTINEL = -7


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


@pytest.fixture(scope="module")
def dense(T):
    """docs f32 [64, 256], their norms, queries f32 [3, 256]: made once, never written."""
    rng = np.random.default_rng(7)
    docs = dev(rng.standard_normal((N_DOCS, DIM)).astype(np.float32))
    queries = dev(rng.standard_normal((NQ, DIM)).astype(np.float32))
    dnorm, inv_norm = T._native.doc_norms(docs)
    return docs, dnorm, inv_norm, queries


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()       # (a copy: some cases' arrays are read-only)
    return t if dtype is None else t.to(dtype)


def same(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {a.shape} {a.dtype} != {b.shape} {b.dtype}"
    assert torch.equal(a.reshape(-1).contiguous().view(torch.uint8), b.reshape(-1).contiguous().view(torch.uint8)), \
        f"{what} differs"


def small_workspace():
    return torch.empty(16, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------ refused before any launch
def sentinel_outputs():
    return dict(S=torch.full((NQ, K), float(SENTINEL), dtype=torch.float64, device="cuda"),
                I=torch.full((NQ, K), SENTINEL, dtype=torch.int64, device="cuda"),
                cnt=torch.full((NQ,), SENTINEL, dtype=torch.int32, device="cuda"),
                flg=torch.full((NQ,), SENTINEL, dtype=torch.int32, device="cuda"))


RESCUE_REFUSALS = ("queries_dim", "dnorm_short", "I_int32", "S_strided", "cnt_short", "flg_host", "k_zero")


@pytest.mark.parametrize("what", RESCUE_REFUSALS)
def test_dense_rescue_refuses_before_any_launch(T, dense, what):
    """Each argument dense_rescue used to hand to the library unchecked raises NativeError, and after a
    device synchronise the four in-place outputs -- prefilled with a sentinel -- are bit for bit what
    they were: nothing was launched."""
    N = T._native
    docs, dnorm, _, queries = dense
    out = sentinel_outputs()
    held = dict(out)                     # the buffers to look at afterwards (the base of a view, not the view)
    if what == "queries_dim":
        queries = queries[:, :128].contiguous()
    elif what == "dnorm_short":
        dnorm = dnorm[:N_DOCS - 1].contiguous()
    elif what == "I_int32":
        out["I"] = held["I"] = torch.full((NQ, K), SENTINEL, dtype=torch.int32, device="cuda")
    elif what == "S_strided":
        held["S"] = torch.full((NQ, 2 * K), float(SENTINEL), dtype=torch.float64, device="cuda")
        out["S"] = held["S"][:, :K]
        assert not out["S"].is_contiguous()
    elif what == "cnt_short":
        out["cnt"] = held["cnt"] = torch.full((NQ - 1,), SENTINEL, dtype=torch.int32, device="cuda")
    elif what == "flg_host":
        out["flg"] = held["flg"] = torch.full((NQ,), SENTINEL, dtype=torch.int32)
    elif what == "k_zero":
        out["I"] = held["I"] = torch.full((NQ, 0), SENTINEL, dtype=torch.int64, device="cuda")
    before = {name: t.clone() for name, t in held.items()}
    with pytest.raises(N.NativeError):
        N.dense_rescue(docs, dnorm, queries, out["S"], out["I"], out["cnt"], out["flg"])
    torch.cuda.synchronize()
    for name, t in held.items():
        same(t, before[name], f"{what}: {name}")


def test_dense_finish_refuses_a_workspace_that_is_too_small(T, dense):
    """dense_finish_f16 reads the candidate lists its shortlist call left in the workspace: one of 16
    bytes holds none, and is refused here like dense_shortlist_f16 refuses it (not replaced, not read)."""
    N = T._native
    docs, dnorm, inv_norm, queries = dense
    need = N.dense_f16_workspace_bytes(N_DOCS, DIM, NQ, KPRIME)
    assert need > 16
    with pytest.raises(N.NativeError, match="workspace smaller"):
        N.dense_finish_f16(docs, None, 0.0, dnorm, inv_norm, queries, K, KPRIME, None, 0, small_workspace())
    with pytest.raises(N.NativeError, match="workspace smaller"):
        N.dense_shortlist_f16(docs, None, 0.0, inv_norm, queries, KPRIME, K, small_workspace())
    torch.cuda.synchronize()


# ------------------------------------------------------------------ accepted as before
def test_dense_rescue_redoes_the_query_whose_flag_is_cleared(T, dense):
    N = T._native
    docs, dnorm, inv_norm, queries = dense
    S, I, cnt, flg = N.dense_topk(docs, dnorm, inv_norm, queries, K, KPRIME)     # (_alloc_out's views: contiguous)
    Se, Ie, cnte, flge = N.dense_topk_exact(docs, dnorm, queries, K)
    torch.cuda.synchronize()
    flg |= N.THR_FLAG_CERTIFIED                              # (whatever the scan said: one query is to be redone)
    kept = [t.clone() for t in (S, I, cnt, flg)]
    flg[1] = 0
    S[1], I[1] = float(SENTINEL), SENTINEL                   # (what comes back in row 1 is the rescue's)
    n_rescued = N.dense_rescue(docs, dnorm, queries, S, I, cnt, flg, workspace=small_workspace())
    torch.cuda.synchronize()
    assert n_rescued.tolist() == [1]
    same(S[1], Se[1], "rescued scores")
    same(I[1], Ie[1], "rescued ids")
    assert int(cnt[1]) == int(cnte[1]) == K and int(flg[1]) == int(flge[1]) and int(flg[1]) & N.THR_FLAG_EXACT
    for q in (0, 2):                                          # the certified rows are left alone
        for t, t0, name in zip((S, I, cnt, flg), kept, "S I cnt flg".split()):
            same(t[q], t0[q], f"{name}[{q}]")


# ------------------------------------------------------------------ the workspace rule
def twice(call, compare):
    """``call(workspace)`` without a workspace and with one of 16 bytes (too small: replaced, not used)."""
    a = call(None)
    b = call(small_workspace())
    torch.cuda.synchronize()
    compare(a, b)


def same_tuple(a, b):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        if isinstance(x, torch.Tensor):
            same(x, y, f"output {j}")
        else:
            assert x == y, f"output {j}: {x} != {y}"


def test_workspace_rule_dense_topk(T, dense):
    docs, dnorm, inv_norm, queries = dense
    twice(lambda ws: T._native.dense_topk(docs, dnorm, inv_norm, queries, K, KPRIME, workspace=ws), same_tuple)


def test_workspace_rule_bm25_topk(T):
    import bm25_cases as BC
    case = BC.CASES["saturate"]
    c = case.corpus
    k1, b = case.params
    idx = T.GpuIndex().set_lexical(c.rowptr, c.post_doc, c.post_tf, c.doclen, c.idf, c.avgdl, k1=k1, b=b,
                                   dense_share=c.share)
    L, qt = idx.lex, dev(c.queries[case.rows])
    twice(lambda ws: T._native.bm25_topk(L["rowptr"], L["post_doc"], L["post_tf"], L["doclen"], L["idf"], L["avgdl"], qt,
                                         10, 0, L["k1"], L["b"], bounds=L["bounds"], dense=L["dense"], workspace=ws),
          same_tuple)


def test_workspace_rule_graph_topk(T):
    import graph_cases as GC
    case = GC.build("distances-h2", "whole", "asbuilt")
    base, n = case.window
    idx = T.GpuIndex(doc_base=base)
    idx.n_docs = n
    idx.set_graph(*case.g)
    G = idx.graph
    args = (G["ent_rowptr"], G["ent_col"], G["men_rowptr"], G["men_chunk"], G["men_conf"], dev(case.seeds))
    tr = idx._graph_transposed()
    twice(lambda ws: T._native.graph_topk(*args, case.hops, case.k, base, n, transposed=tr, workspace=ws), same_tuple)


def test_workspace_rule_entity_match(T):
    import entity_cases as EC
    from triple_hybrid_rag_amd.index_entities import pack_entity_names, plan_needles
    case = EC.case("three_queries")
    blob, ptr = pack_entity_names(case.names)
    plan = plan_needles(case.queries, case.limit)
    args = [dev(a) for a in (blob, ptr, plan.needles, plan.needle_len, plan.query_needles, plan.query_per)]
    twice(lambda ws: T._native.entity_match(*args, workspace=ws), same_tuple)


def test_workspace_rule_text_tokens(T):
    idx = T.GpuIndex().set_vocabulary(["ab", "cd", "ef"])
    blobs = [b"ab cd", b"ef xy ab"]
    ptr = np.concatenate([[0], np.cumsum([len(b) for b in blobs])]).astype(np.int64)
    blob = np.frombuffer(b"".join(blobs) + bytes(16), dtype=np.uint8)
    X, bytes_dev, ptr_dev = idx.text, dev(blob), dev(ptr)

    def compare(a, b):
        assert a["capacity"] == b["capacity"]
        for name in ("n_tokens", "flags", "n_total", "n_unknown"):
            same(a[name], b[name], name)
        nt, nu = int(a["n_total"].item()), int(a["n_unknown"].item())
        assert (nt, nu) == (5, 1)
        for name, n in (("doc", nt), ("term", nt), ("unknown_off", nu), ("unknown_len", nu)):   # (the valid rows)
            same(a[name][:n], b[name][:n], name)
    twice(lambda ws: T._native.text_tokens(bytes_dev, ptr_dev, int(ptr[-1]), X["table_dev"], X["slots"], X["term_bytes"],
                                           X["term_ptr"], workspace=ws), compare)


def test_workspace_rule_csr_merge(T):
    import graph_ingest_cases as GC
    case = GC.cases()["shapes"]
    args = (dev(case.rowptr_a), dev(case.ids_a), dev(case.pay_a).view(torch.float32), dev(case.rowptr_b),
            dev(case.ids_b), dev(case.pay_b).view(torch.float32), False)

    def compare(a, b):
        (rp1, ids1, pay1, nnz1, st1), (rp2, ids2, pay2, nnz2, st2) = a, b
        assert (nnz1, st1) == (nnz2, st2) and st1 == 0 and nnz1 == len(case.ids_a) + len(case.ids_b)
        same(rp1, rp2, "rowptr_out")
        same(ids1[:nnz1], ids2[:nnz1], "ids_out")
        same(pay1[:nnz1], pay2[:nnz1], "pay_out")
    twice(lambda ws: T._native.csr_merge(*args, workspace=ws), compare)
