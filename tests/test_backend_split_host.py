"""No GPU: the seams of the drop-in client.  What backend.py re-exports is what its new modules define, the
modules import no more than they say, every piece of the client's derived state exists from construction, and
each kind of change (rows, parents, graph) leaves every cache that depends on it fresh."""
import gc
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import triple_hybrid_rag_amd as T  # noqa: E402
from triple_hybrid_rag_amd import backend, backend_ingest, backend_tables, index_entities, index_text, store  # noqa: E402
from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient, LazyRows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DERIVED = ("_pending_lex", "_lazy", "_by_text", "_tri", "_plans", "_pin")


# --------------------------------------------------------------------------- the surface
def test_backend_re_exports_the_objects_of_their_new_homes():
    assert backend.tokenize is index_text.tokenize and backend.CorpusStore is store.CorpusStore is T.CorpusStore
    for name in ("_Reply", "LazyRows", "_TableQuery"):
        assert getattr(backend, name) is getattr(backend_tables, name), name
    assert issubclass(GpuIndexClient, backend_ingest.ClientIngest) and T.GpuIndexClient is GpuIndexClient
    assert callable(backend.set_default_client) and callable(backend.get_supabase_client)
    assert index_text.tokenizer_table(backend.tokenize, "x") is index_text.TextTable.default()
    moved = ("insert_children", "insert_parents", "insert_entities", "insert_relations", "insert_mentions",
             "delete_children", "_delete_rows", "_delete_children_where", "_delete_parents_where",
             "_delete_documents_where", "_child_rows_where", "_check_org", "_number_texts", "_settle_deferred", "_track")
    for name in moved:
        assert name in vars(backend_ingest.ClientIngest), name
    kept = ("rpc", "table", "_semantic", "_lexical", "_image", "_hybrid_rrf", "_legacy_row", "_scope", "_scoped",
            "_scoped_union", "_qcoll", "_upload", "_download", "_rows", "_query_terms", "graph_chunks", "maxsim_scores",
            "text_to_child_id", "find_entities", "find_entities_batch", "_entity_index", "query_terms_batch")
    for name in kept:
        assert name in vars(GpuIndexClient), name
    assert callable(index_entities.name_trigrams) and callable(index_entities.match_names)
    assert index_text.number_tokens is store.number_tokens            # (the store numbers without a device module)
    assert "from ." not in open(store.__file__).read()


def test_the_modules_import_no_more_than_they_say():
    """In a fresh interpreter, with the package's directory mounted WITHOUT running its __init__ (which
    imports everything): store alone brings neither torch nor _native, index_text alone no backend."""
    code = (
        "import importlib, sys, types\n"
        "pkg = types.ModuleType('thr_pkg'); pkg.__path__ = [sys.argv[1]]; sys.modules['thr_pkg'] = pkg\n"
        "importlib.import_module('thr_pkg.store')\n"
        "loaded = [m for m in sys.modules if m == 'torch' or m.startswith('thr_pkg.')]\n"
        "assert loaded == ['thr_pkg.store'], loaded\n"
        "importlib.import_module('thr_pkg.index_text')\n"
        "assert 'thr_pkg.backend' not in sys.modules and 'torch' in sys.modules\n")
    done = subprocess.run([sys.executable, "-c", code, os.path.join(ROOT, "triple-hybrid-rag_amd")],
                          capture_output=True, text=True)
    assert done.returncode == 0, done.stderr


# --------------------------------------------------------------------------- no ad hoc state
class _StubIndex:
    """What the client's writers need of an index, recorded; a scope plan is current while no row changed."""

    def __init__(self, n, collections=True):
        self.docs, self.dim, self.n_docs = None, 0, n
        self.lex = self.tokens = self.entities = None
        self.doc_coll = object() if collections else None
        self.graph = {"men_rowptr": None}
        self.device, self.rows_version, self.calls, self.before = "cpu", 0, [], None
        self._attrs = {}

    def attribute_names(self):
        return sorted(self._attrs)

    def set_attributes(self, columns):
        self._attrs.update(columns)

    def scope_plan(self, scopes, nq):
        return SimpleNamespace(scopes=scopes, rows_version=self.rows_version)

    def scope_plan_current(self, plan, nq):
        return plan.rows_version == self.rows_version

    def append_rows(self, **parts):
        self.rows_version += 1
        self.n_docs += parts["n_rows"]
        self.calls.append(("rows", sorted(parts)))

    def delete_rows(self, ids):
        if self.before is not None:
            self.before()
        self.rows_version += 1
        self.n_docs -= len(ids)
        self.calls.append(("delete", np.asarray(ids).tolist()))

    def append_graph(self, entity_names=None, n_new_entities=None, relations=None):
        self.calls.append(("graph", entity_names, n_new_entities, relations))

    def append_mentions(self, entity, chunk, conf=None):
        self.calls.append(("mentions", entity.tolist(), chunk.tolist()))


ORGS = ("acme", "bolt")


def _client(tenants, n=8):
    st = CorpusStore(child_ids=[f"c{i}" for i in range(n)], parent_ids=[f"p{i // 2}" for i in range(n)],
                     document_ids=[f"d{i // 4}" for i in range(n)], texts=[f"alpha t{i}" for i in range(n)],
                     pages=[1] * n, modalities=["text"] * n,
                     parents={f"p{j}": {"id": f"p{j}", "text": f"P{j}", "section_heading": None} for j in range(n // 2)},
                     collections=[("a", "b")[i % 2] for i in range(n)], entity_names=["Acme Corp", "Zeta"],
                     org_ids=[ORGS[i // 4 % 2] for i in range(n)] if tenants else None)
    idx = _StubIndex(n)
    return GpuIndexClient(idx, st, org_id=None if tenants else "acme"), idx, st


def test_a_new_client_has_every_piece_of_derived_state():
    for tenants in (False, True):
        client, _, _ = _client(tenants)
        assert client.multi_tenant == tenants
        assert all(name in vars(client) for name in DERIVED), sorted(vars(client))
        assert client._pending_lex is None and client._lazy == [] and client._by_text is None and client._tri is None
        assert client._plans == {} and client._pin == {}
    # a subclass with an __init__ of its own (the CLI's oracle client) still reads what it never set
    bare = object.__new__(GpuIndexClient)
    assert bare._pending_lex is None and bare._by_text is None and bare._tri is None and tuple(bare._lazy) == ()


def test_a_shard_endpoint_has_every_piece_of_derived_state(tmp_path):
    import torch
    import torch.distributed as dist
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    shard = SimpleNamespace(dim=8, device=torch.device("cpu"), doc_coll=None, lex=True)
    dist.init_process_group("gloo", init_method=f"file://{tmp_path / 'rendezvous'}", rank=0, world_size=1)
    try:
        with ShardedIndexClient(shard, CorpusStore.synthetic(16, vocab_size=8), collection_names=["faq"],
                                merge_fn=lambda S, I, k: (S[0], I[0])) as front:
            assert all(name in vars(front) for name in DERIVED), sorted(vars(front))
            assert front._plans == {} and front._lazy == [] and front._tri is None and front._by_text is None
    finally:
        dist.destroy_process_group()


# --------------------------------------------------------------------------- invalidation
def _prime(client, idx, st, seen):
    """Fill every cache and track one unresolved deferred reply -> (the reply, the keys of the plans)."""
    assert client.text_to_child_id("alpha t0") == "c0" and client._by_text is not None
    org = ORGS[0] if client.multi_tenant else None
    assert client._scoped(org, ["a", "b"]) is not None
    if client.multi_tenant:
        assert client._scoped(org, "a") is not None and client._scope(ORGS[1]) is not None
    assert client._plans and all(idx.scope_plan_current(p, 1) for p in client._plans.values())
    assert client.find_entities(["zeta"]) == [1] and client._tri is not None
    lazy = LazyRows(lambda: seen.append(list(st.child_ids)) or [st.result_row(0)])
    client._track(lazy)
    return lazy, set(client._plans)


def _fresh_after_a_row_change(client, idx):
    assert all(idx.scope_plan_current(p, 1) for p in client._plans.values())
    org = ORGS[0] if client.multi_tenant else None
    plan = client._scoped(org, ["a", "b"])["scopes"]
    assert idx.scope_plan_current(plan, 1) and plan in client._plans.values()


@pytest.mark.parametrize("tenants", [False, True])
def test_every_kind_of_change_leaves_its_caches_fresh(tenants):
    client, idx, st = _client(tenants)
    seen = []
    # rows in
    lazy, _ = _prime(client, idx, st, seen)
    new = {"id": "n0", "parent_id": "p0", "document_id": "d0", "text": "brand new", "org_id": ORGS[0], "collection": "b"}
    assert client.insert_children([new]) == [{"id": "n0"}]
    assert client.text_to_child_id("brand new") == "n0" and client.text_to_child_id("alpha t1") == "c1"
    assert len(seen) == 1 and lazy._fetch is None           # settled before the plans went
    _fresh_after_a_row_change(client, idx)
    assert client._tri is not None                          # (rows are not what the name index is derived from)
    # a parent in
    client.text_to_child_id("alpha t1")
    assert "fresh parent" not in client._by_text
    assert client.insert_parents([{"id": "pn", "text": "fresh parent", "org_id": ORGS[0]}]) == [{"id": "pn"}]
    assert client.text_to_child_id("fresh parent") is None and "fresh parent" in client._by_text
    # the graph tables
    assert client.insert_entities([{"id": 2, "name": "Beta GmbH", "org_id": ORGS[0]}]) == [{"id": 2}]
    assert client._tri is None and client.find_entities(["beta"]) == [2] and client._tri is not None
    client.insert_relations([{"id": "r0", "subject_entity_id": 0, "object_entity_id": 2, "org_id": ORGS[0]}])
    assert client._tri is None and idx.calls[-1][0] == "graph"
    client._entity_index()
    client.insert_mentions([{"id": "m0", "entity_id": 2, "child_chunk_id": "n0"}])
    assert client._tri is None and idx.calls[-1] == ("mentions", [2], [8])
    # rows out: the deferred reply is read back before the index and the store change
    del seen[:]
    lazy, _ = _prime(client, idx, st, seen)
    idx.before = lambda: seen.append("index")
    before = list(st.child_ids)
    assert [r["id"] for r in client.delete_children(["c1", "nope"])] == ["c1"]
    assert seen == [before, "index"] and lazy._fetch is None and lazy[0]["child_id"] == "c0"
    assert client.text_to_child_id("alpha t1") is None and client.text_to_child_id("alpha t2") == "c2"
    _fresh_after_a_row_change(client, idx)
    # a document out, through the table
    del seen[:]
    lazy, _ = _prime(client, idx, st, seen)
    before = list(st.child_ids)
    q = client.table("rag_documents").delete().eq("id", "d1")
    assert (q.eq("org_id", ORGS[1]) if tenants else q).execute().data == [{"id": "d1"}]
    assert seen == [before, "index"] and lazy._fetch is None
    assert client.text_to_child_id("alpha t5") is None and client.text_to_child_id("alpha t0") == "c0"
    assert st.child_ids == ["c0", "c2", "c3", "n0"] and "p2" not in st.parents
    _fresh_after_a_row_change(client, idx)
    # a reply nobody holds is not kept alive by the bookkeeping
    client._track(LazyRows(lambda: []))
    gc.collect()
    client._track(LazyRows(lambda: []))
    gc.collect()
    assert sum(r() is not None for r in client._lazy) == 0
