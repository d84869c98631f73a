"""The scoped graph channel and the multi-tenant client without a GPU: thr_graph_topk_scoped is declared,
exported and bound with matching argument counts and refuses bad arguments before any launch; the
store's org_ids column survives append, delete, save and load; the refusals of the multi-tenant mode."""
import inspect
import os
import re

import numpy as np
import pytest

import triple_hybrid_rag_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_args(name):
    text = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    m = re.search(r"\b" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S)
    assert m, f"{name} is not declared in thr_hip.h"
    return len([a for a in m.group(1).split(",") if a.strip()])


def test_the_scoped_graph_entry_is_declared_exported_and_bound():
    N = T._native
    lib = N.load()
    name = "thr_graph_topk_scoped"
    assert hasattr(lib, name), f"{name} is not exported"
    assert name in N.EXPORTED_SYMBOLS
    assert len(N._SIGNATURES[name][1]) == declared_args(name) == declared_args("thr_graph_topk") + 2
    assert lib.thr_abi_version() == N.ABI_VERSION == 9
    header = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    comment = header[:header.index("int thr_graph_topk_scoped(")].rsplit("/*", 1)[1]
    assert "graph_search.py:154-230" in comment
    # the same workspace as the unfiltered call
    assert lib.thr_graph_workspace_bytes(2, 1000) == 2 * 8192 * 8 + 64 * 1024


def test_host_side_argument_checks_of_the_scoped_graph_call():
    import ctypes as C
    lib = T._native.load()
    P8 = C.c_void_p(8)    # (never dereferenced: every call below is refused before a launch)

    def call(fn=lib.thr_graph_topk_scoped, er=P8, n_ent=100, n_chunks=50, labels=(P8, P8), seeds=P8, nq=2, ms=3,
             hops=2, k=10, ws=P8, wsb=1 << 30):
        return fn(er, P8, n_ent, P8, P8, P8, None, None, None, 0, n_chunks, *labels, seeds, nq, ms, hops, k,
                  P8, P8, P8, P8, ws, wsb, None)
    assert call(labels=(None, P8)) == -1 and call(labels=(P8, None)) == -1     # both labels are required
    # ... plus thr_graph_topk's own checks, with the same answers
    for fn, labels in ((lib.thr_graph_topk_scoped, (P8, P8)), (lib.thr_graph_topk, ())):
        assert call(fn, labels=labels, er=None) == -1 and call(fn, labels=labels, seeds=None) == -1
        assert call(fn, labels=labels, ws=None) == -1
        assert call(fn, labels=labels, n_ent=0) == -1 and call(fn, labels=labels, n_chunks=0) == -1
        assert call(fn, labels=labels, nq=0) == -1 and call(fn, labels=labels, ms=0) == -1
        assert call(fn, labels=labels, ms=17) == -1 and call(fn, labels=labels, hops=-1) == -1
        assert call(fn, labels=labels, hops=9) == -1 and call(fn, labels=labels, k=0) == -1
        assert call(fn, labels=labels, k=129) == -1
        assert call(fn, labels=labels, wsb=2 * 8192 * 8 - 1) == -3


def test_the_wrapper_refuses_before_a_pointer_is_taken():
    torch = pytest.importorskip("torch")
    N = T._native
    z = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(N.NativeError, match="doc_label and query_label are required"):
        N.graph_topk_scoped(z, z, z, z, z, z, 2, 10, 0, 4, None, z)
    with pytest.raises(N.NativeError, match="doc_label and query_label are required"):
        N.graph_topk_scoped(z, z, z, z, z, z, 2, 10, 0, 4, z, None)
    with pytest.raises(N.NativeError, match="expected a CUDA"):      # host tensors: refused like graph_topk's
        N.graph_topk_scoped(z, z, z, z, z, z, 2, 10, 0, 4, z, z)


def test_the_index_layer_takes_scopes_for_the_graph_channel():
    idx = T.GpuIndex
    assert inspect.signature(idx.graph_search).parameters["scopes"].default is None
    assert inspect.signature(idx.retrieve_batch).parameters["scope_graph"].default is False
    assert inspect.signature(idx.side_channels).parameters["scope_graph"].default is False
    assert list(inspect.signature(idx.graph_search).parameters)[:4] == ["self", "query_seeds", "k", "hops"]
    assert "org_id" in inspect.signature(T.backend.GpuIndexClient.graph_chunks).parameters


def rows_of(n, orgs=("acme", "bolt", "core")):
    return [{"id": f"c{i}", "parent_id": f"p{i // 2}", "document_id": f"d{i // 4}", "text": f"word{i % 5} text {i}",
             "page": 1, "modality": "text", "org_id": orgs[i % len(orgs)], "content_hash": f"h{i}",
             "embedding_1024": [float(i + 1), 1.0, 0.0, 0.0]} for i in range(n)]


def test_org_ids_survive_append_delete_save_and_load(tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import CorpusStore
    hi = IB.from_rows(rows_of(9))
    st = hi.store
    assert st.org_ids == ["acme", "bolt", "core"] * 3
    assert "org_id" not in st.child_row(4)           # (the rows a fetch returns are what they were)
    st.append([{"id": "x1", "text": "new", "org_id": "dune"}, {"id": "x2", "text": "new too", "org_id": "acme"}])
    assert st.org_ids[-2:] == ["dune", "acme"] and len(st.org_ids) == len(st.child_ids) == 11
    assert [r["id"] for r in st.delete([1, 9])] == ["c1", "x1"]
    assert st.org_ids == ["acme", "core", "acme", "bolt", "core", "acme", "bolt", "core", "acme"]
    hi.docs = np.zeros((len(st.child_ids), 4), dtype=np.float32)
    for name in ("rowptr", "post_doc", "post_tf", "doclen", "idf"):
        setattr(hi, name, None)
    IB.save(hi, str(tmp_path / "ix"))
    back = IB.load(str(tmp_path / "ix")).store
    assert list(back.org_ids) == st.org_ids
    back.append([{"id": "y", "text": "after load", "org_id": "bolt"}])      # (the loaded blob column becomes a list)
    assert back.org_ids[-1] == "bolt"
    assert [r["id"] for r in back.delete([0])] == ["c0"] and back.org_ids[0] == "core" and len(back.org_ids) == 9
    # a store without the column: rows may still name their org (the single-tenant ingest does), nothing is kept
    plain = IB.from_rows([{k: v for k, v in r.items() if k != "org_id"} for r in rows_of(4)])
    assert plain.store.org_ids is None
    plain.store.append([{"id": "z", "text": "t", "org_id": "acme"}])
    assert plain.store.org_ids is None
    plain.docs = np.zeros((5, 4), dtype=np.float32)
    for name in ("rowptr", "post_doc", "post_tf", "doclen", "idf"):
        setattr(plain, name, None)
    IB.save(plain, str(tmp_path / "old"))                                    # a directory saved without the column
    assert IB.load(str(tmp_path / "old")).store.org_ids is None
    assert CorpusStore.synthetic(4).org_ids is None


def host_index(n):
    torch = pytest.importorskip("torch")
    idx = T.GpuIndex.__new__(T.GpuIndex)      # (no device: only the host half of the client)
    idx.device, idx.n_docs, idx.doc_coll, idx._attrs = torch.device("cpu"), n, None, {}
    idx.docs = idx.lex = idx.graph = idx.tokens = None
    return idx


def test_multi_tenant_mode_and_its_refusals():
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    st = IB.from_rows(rows_of(9)).store
    idx = host_index(9)
    client = GpuIndexClient(idx, st)
    assert client.multi_tenant and idx.attribute_names() == ["org"]
    assert idx.attribute("org").tolist() == [0, 1, 2] * 3          # the sorted distinct names
    # a missing or unknown org: no rows, before anything is uploaded
    for params in ({"p_embedding": [0.0] * 4}, {"p_org_id": None, "p_embedding": [0.0] * 4},
                   {"p_org_id": "nobody", "p_embedding": [0.0] * 4}):
        idx.dim = 4
        assert client.rpc("rag2_semantic_search", params).execute().data == []
    assert client.graph_chunks([1, 2], 10, 2, org_id="nobody") == [] == client.graph_chunks([1, 2], 10)
    # reads by id inside an org; content hashes inside an org
    t = lambda: client.table("rag_child_chunks")          # noqa: E731
    assert [r["id"] for r in t().select("*").in_("id", ["c0", "c1", "c3"]).execute().data] == ["c0", "c1", "c3"]
    assert [r["id"] for r in t().select("*").eq("org_id", "acme").in_("id", ["c0", "c1", "c3"]).execute().data] == ["c0", "c3"]
    assert t().select("content_hash").eq("org_id", "bolt").in_("content_hash", ["h0", "h1"]).execute().data == \
        [{"content_hash": "h1"}]
    assert client.table("organizations").select("id").execute().data == [{"id": o} for o in ("acme", "bolt", "core")]
    # parents inside an org: the ones that org's chunks name (p0 = c0 acme, c1 bolt; p1 = c2 core, c3 acme)
    st.parents.update({f"p{j}": {"id": f"p{j}", "text": f"P{j}", "section_heading": None} for j in range(5)})
    ptab = lambda: client.table("rag_parent_chunks")          # noqa: E731
    assert [r["id"] for r in ptab().select("*").in_("id", ["p0", "p1"]).execute().data] == ["p0", "p1"]
    assert [r["id"] for r in ptab().select("*").eq("org_id", "bolt").in_("id", ["p0", "p1"]).execute().data] == ["p0"]
    assert client.table("rag_documents").select("org_id").eq("org_id", "bolt").execute().data == [{"org_id": "bolt"}]
    # an insert names its org on every row
    with pytest.raises(ValueError, match="every row needs its org_id"):
        t().insert([{"id": "n1", "text": "a", "org_id": "acme"}, {"id": "n2", "text": "b"}]).execute()
    with pytest.raises(ValueError, match="every row needs its org_id"):
        client.table("rag_parent_chunks").insert({"id": "pp", "text": "a"}).execute()
    assert len(st.child_ids) == 9 and "pp" not in st.parents
    # content-hash uniqueness is store-wide: another org's hash is still a duplicate
    with pytest.raises(ValueError, match="duplicate key"):
        t().insert({"id": "n3", "text": "a", "org_id": "bolt", "content_hash": "h0"}).execute()
    # every other construction is what it was
    single = GpuIndexClient(host_index(9), st, org_id="acme")
    assert not single.multi_tenant and single.index.attribute_names() == []
    assert single.rpc("rag2_semantic_search", {"p_org_id": "bolt", "p_embedding": [0.0]}).execute().data == []
    bare = GpuIndexClient(host_index(4), T.backend.CorpusStore.synthetic(4))
    assert not bare.multi_tenant and bare.index.attribute_names() == []


def test_an_org_column_that_came_with_the_index_is_checked_against_the_store():
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    st = IB.from_rows(rows_of(6)).store

    def with_column(codes):
        return host_index(6).set_attributes({"org": np.array(codes, dtype=np.int32)})
    assert GpuIndexClient(with_column([5, 0, 2] * 2), st)._org_code == {"acme": 5, "bolt": 0, "core": 2}
    with pytest.raises(ValueError, match="does not follow"):
        GpuIndexClient(with_column([0, 1, 2, 0, 1, 1]), st)       # one org, two ids
    with pytest.raises(ValueError, match="the same id"):
        GpuIndexClient(with_column([0, 1, 1] * 2), st)            # two orgs, one id
    with pytest.raises(ValueError, match="the same id"):
        GpuIndexClient(with_column([0, 1, -1] * 2), st)           # an org whose rows carry none


def test_a_sharded_client_refuses_a_store_with_org_ids():
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    st = IB.from_rows(rows_of(6)).store
    with pytest.raises(T._native.NativeError, match="org_ids"):
        ShardedIndexClient(host_index(6), st, org_id="acme")


def test_the_graph_searcher_passes_the_org_only_to_a_multi_tenant_client():
    import asyncio
    from triple_hybrid_rag_amd.rag2.graph_search import GraphSearcher

    class Client:
        multi_tenant = True

        def __init__(self):
            self.calls = []

        def find_entities(self, keywords, limit=20):
            return [4, 7]

        def entity_name(self, e):
            return f"entity{e}"

        def graph_chunks(self, seeds, top_k, hops=2, **kw):
            self.calls.append((list(seeds), top_k, hops, kw))
            return ["c1"]

    many, one = Client(), Client()
    one.multi_tenant = False
    for c in (many, one):
        res = asyncio.run(GraphSearcher(c).search(["a"], "MATCH", org_id="bolt", top_k=5))
        assert res.chunk_ids == ["c1"]
    assert many.calls == [([4, 7], 5, 2, {"org_id": "bolt"})]
    assert one.calls == [([4, 7], 5, 2, {})]
