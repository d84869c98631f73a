"""Scoped queries without a GPU: the new entry points are declared, exported and bound with matching
argument counts, refuse bad arguments on the host before any launch, and the attribute columns
survive save -> load (a directory written without them loads as before)."""
import os
import re

import numpy as np
import pytest

import triple_hybrid_rag_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("thr_scope_resolve", "thr_scope_resolve_workspace_bytes", "thr_dense_topk_rows",
       "thr_dense_topk_rows_workspace_bytes")


def declared_args(name):
    text = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in thr_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_new_entry_points_are_declared_exported_and_bound():
    N = T._native
    lib = N.load()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in N.EXPORTED_SYMBOLS
        assert len(N._SIGNATURES[name][1]) == declared_args(name), f"{name}: argument count differs from the header"
    assert lib.thr_abi_version() == N.ABI_VERSION == 9
    assert N.THR_SCOPE_MAX_COLS == 8 and N.THR_SCOPE_MAX_PREDS == 4096


def test_host_side_argument_checks_of_the_scope_calls():
    import ctypes as C
    lib = T._native.load()
    one = (C.c_void_p * 1)(8)    # (never dereferenced: every call below is refused before a launch)
    P8 = C.c_void_p(8)

    def resolve(cols=one, C_=1, n=100, preds=P8, P=2, rowptr=P8, rows=P8, cap=100, labels=P8, overlap=P8, ws=P8,
                wsb=1 << 30):
        return lib.thr_scope_resolve(cols, C_, n, preds, P, rowptr, rows, cap, labels, overlap, ws, wsb, None)
    assert resolve(C_=0) == -1 and resolve(C_=9) == -1
    assert resolve(P=0) == -1 and resolve(P=4097) == -1
    assert resolve(n=0) == -1 and resolve(cap=-1) == -1
    assert resolve(rows=None) == -1 and resolve(rows=P8, cap=0) == -1          # rows and cap: both or neither
    assert resolve(labels=None) == -1 and resolve(overlap=None) == -1           # labels and overlap: both or neither
    assert resolve(cols=None) == -1 and resolve(preds=None) == -1 and resolve(rowptr=None) == -1
    assert resolve(cols=(C.c_void_p * 1)(None)) == -1
    assert resolve(wsb=0) == -3
    assert lib.thr_scope_resolve_workspace_bytes(1_000_000, 64) >= 64 * (1_000_000 // 512) * 12
    assert lib.thr_scope_resolve_workspace_bytes(0, 4) == 0 == lib.thr_scope_resolve_workspace_bytes(10, 0)

    def rows(docs=P8, n=100, dim=768, nq=4, k=10, cap=50, rows_=P8, P=2, wsb=1 << 30, ws=P8):
        return lib.thr_dense_topk_rows(docs, P8, n, dim, 0, P8, nq, k, P8, rows_, cap, P, P8, P8, P8, P8, P8, ws, wsb, None)
    assert rows(docs=None) == -1 and rows(ws=None) == -1
    assert rows(k=0) == -1 and rows(k=257) == -1
    assert rows(P=0) == -1 and rows(P=4097) == -1 and rows(cap=-1) == -1 and rows(nq=0) == -1
    assert rows(rows_=None) == -1 and rows(cap=0) == -1
    assert rows(dim=770) == -2 and rows(nq=(1 << 20) + 1) == -2
    assert rows(wsb=0) == -3
    w = lib.thr_dense_topk_rows_workspace_bytes
    assert w(2048, 64, 100) >= 2048 * 100 * 16 and w(2048, 64, 256) > w(2048, 64, 100)
    assert w(0, 1, 10) == 0 == w(4, 0, 10) == w(4, 1, 257)


def test_wrappers_refuse_shapes_before_a_pointer_is_taken():
    torch = pytest.importorskip("torch")
    N = T._native
    col = torch.zeros(10, dtype=torch.int32)
    with pytest.raises(N.NativeError, match="attribute columns"):
        N.scope_resolve([], torch.zeros((1, 0), dtype=torch.int32))
    with pytest.raises(N.NativeError, match="same length"):
        N.scope_resolve([col, col[:5]], torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(N.NativeError, match=r"preds must be \[P, 1\]"):
        N.scope_resolve([col], torch.zeros((1, 2), dtype=torch.int32))
    with pytest.raises(N.NativeError, match="predicates per call"):
        N.scope_resolve([col], torch.zeros((5000, 1), dtype=torch.int32))


def test_scope_tables_and_refusals_of_the_index_layer():
    torch = pytest.importorskip("torch")
    idx = T.GpuIndex.__new__(T.GpuIndex)      # (no device: only the host half of the scope layer)
    idx.device, idx.n_docs, idx.doc_coll, idx._attrs = torch.device("cpu"), 6, None, {}
    idx.set_collections(np.arange(6, dtype=np.int32) % 2)
    idx.set_attributes({"org": np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)})
    assert idx.attribute_names() == ["collection", "org"]
    with pytest.raises(ValueError, match="one int32 per row"):
        idx.set_attributes({"category": np.zeros(5, dtype=np.int32)})
    with pytest.raises(ValueError, match="unknown attribute"):
        idx.attribute("tenant")
    names, tab = idx._scope_table([None, {"org": 2}, {"collection": 1, "org": 0}, {"org": None}], 4)
    assert names == ["collection", "org"]
    assert tab.tolist() == [[-1, -1], [-1, 2], [1, 0], [-1, -2]]
    with pytest.raises(ValueError, match="unknown attribute"):
        idx._scope_table([{"tenant": 1}], 1)
    with pytest.raises(ValueError, match="one per query"):
        idx._scope_table([None], 2)
    with pytest.raises(ValueError, match="table"):
        idx._scope_table(np.zeros((4, 3), dtype=np.int32), 4)
    for call in (lambda: idx.dense_search(None, 10, collections=[0], scopes=[None]),
                 lambda: idx.bm25_search(None, 10, collections=[0], scopes=[None])):
        with pytest.raises(ValueError, match="not both"):
            call()
    from triple_hybrid_rag_amd import index_scope as IS
    assert IS._may_overlap(np.array([0, -1]), np.array([-1, 3])) and not IS._may_overlap(np.array([0, 1]), np.array([1, 1]))
    with pytest.raises(ValueError, match=">= 0"):
        idx.set_attributes({"category": np.array([0, 1, -2, 0, 0, 0], dtype=np.int32)})
    empty = T.GpuIndex.__new__(T.GpuIndex)
    empty.device, empty.n_docs, empty.doc_coll, empty._attrs = torch.device("cpu"), 0, None, {}
    with pytest.raises(ValueError, match="no rows yet"):
        empty.set_attributes({"org": np.zeros(3, dtype=np.int32)})
    assert empty.n_docs == 0


def test_a_scope_plan_is_refused_once_a_column_was_replaced_or_on_another_index():
    torch = pytest.importorskip("torch")
    from triple_hybrid_rag_amd import index_scope as IS

    def index():
        idx = T.GpuIndex.__new__(T.GpuIndex)
        idx.device, idx.n_docs, idx.doc_coll, idx._attrs = torch.device("cpu"), 6, None, {}
        return idx.set_attributes({"org": np.array([0, 0, 1, 1, 2, 2], dtype=np.int32)})
    idx, other = index(), index()
    plan = IS.ScopePlan(["org"], np.zeros((0, 1), np.int32), np.full(3, -1, np.int32), np.zeros(0, np.int64), None,
                        None, [], n_docs=6, mutations=0, columns=idx._column_key())
    assert idx.scope_plan(plan, 3) is plan
    with pytest.raises(ValueError, match="another index"):
        other.scope_plan(plan, 3)
    with pytest.raises(ValueError, match="another batch size"):
        idx.scope_plan(plan, 4)
    idx.set_attributes({"org": np.array([2, 2, 1, 1, 0, 0], dtype=np.int32)})      # the column is replaced
    with pytest.raises(ValueError, match="columns changed"):
        idx.scope_plan(plan, 3)
    idx2 = index()
    plan2 = IS.ScopePlan(["org"], np.zeros((0, 1), np.int32), np.full(3, -1, np.int32), np.zeros(0, np.int64), None,
                         None, [], n_docs=6, mutations=0, columns=idx2._column_key())
    idx2.set_collections(np.zeros(6, dtype=np.int32))                               # a column is added
    with pytest.raises(ValueError, match="columns changed"):
        idx2.scope_plan(plan2, 3)


def test_a_sharded_index_refuses_scopes_with_a_clear_message():
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    sh = ShardedIndex.__new__(ShardedIndex)     # (the refusal comes before anything of the shard is touched)
    with pytest.raises(T._native.NativeError, match="not supported on a document-sharded index"):
        sh.retrieve_batch(None, scopes=[{"org": 1}])


def test_grouping_is_right_and_planning_2048_tenants_is_host_work_of_milliseconds():
    import time
    from triple_hybrid_rag_amd import index_scope as IS
    rng = np.random.default_rng(0)
    for _ in range(300):      # against the pair-by-pair definition
        preds = np.unique(rng.integers(-1, 3, (int(rng.integers(1, 30)), int(rng.integers(1, 4)))).astype(np.int32), axis=0)
        groups = IS.disjoint_groups(preds)
        assert sorted(np.concatenate(groups).tolist()) == list(range(len(preds)))
        for g in groups:
            assert not any(IS._may_overlap(preds[i], preds[j]) for i in g for j in g if i < j), (preds, g)
    assert IS.disjoint_groups(np.zeros((0, 2), np.int32)) == []
    # the normal batch: every query its own tenant -> ONE group; tenants and (tenant, collection) pairs
    # of other tenants -> still one; a tenant and a collection of its own -> two
    torch = pytest.importorskip("torch")
    idx = T.GpuIndex.__new__(T.GpuIndex)
    idx.device, idx.n_docs, idx.doc_coll, idx._attrs = torch.device("cpu"), 4, None, {}
    idx.set_collections(np.zeros(4, dtype=np.int32)).set_attributes({"org": np.zeros(4, dtype=np.int32),
                                                                     "document": np.zeros(4, dtype=np.int32)})
    for P in (2048, 4096):
        scopes = [{"org": i} for i in range(P)]
        t0 = time.perf_counter()
        _, tab = idx._scope_table(scopes, P)
        preds, inv = np.unique(tab, axis=0, return_inverse=True)
        groups = IS.disjoint_groups(preds)
        spent = time.perf_counter() - t0
        assert len(groups) == 1 and len(groups[0]) == P
        assert spent < 1.0, f"planning {P} distinct tenants took {spent:.2f} s on the host"    # (measured: ~10 ms)
    mixed = np.array([[-1, t, -1] for t in range(1000)] + [[1, 5000 + t, -1] for t in range(1000)], dtype=np.int32)
    assert len(IS.disjoint_groups(mixed)) == 1
    assert len(IS.disjoint_groups(np.array([[-1, 7, -1], [1, 7, -1]], dtype=np.int32))) == 2
    assert len(IS.disjoint_groups(np.array([[-1, 7, -1], [1, -1, -1]], dtype=np.int32))) == 2


def test_save_and_load_keep_the_attribute_columns(tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    docs = np.random.default_rng(0).standard_normal((12, 8)).astype(np.float32)
    org = (np.arange(12) % 3).astype(np.int32)
    IB.save(IB.HostIndex(docs=docs, attributes={"org": org, "category": org * 2}), str(tmp_path / "a"))
    back = IB.load(str(tmp_path / "a"))
    assert sorted(back.attributes) == ["category", "org"]
    assert np.array_equal(back.attributes["org"], org) and np.array_equal(back.attributes["category"], org * 2)
    IB.save(IB.HostIndex(docs=docs), str(tmp_path / "old"))          # a directory without the columns
    assert IB.load(str(tmp_path / "old")).attributes is None
    with pytest.raises(ValueError, match="one int32 per row"):
        IB.save(IB.HostIndex(docs=docs, attributes={"org": org[:5]}), str(tmp_path / "bad"))
