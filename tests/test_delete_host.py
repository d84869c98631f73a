"""Delete, the parts that need no GPU: the new C entries' host-side argument checks,
``GpuIndex.delete_rows`` validation (which runs before any device work), ``CorpusStore.delete``
and the delete surface of the tables over a stub index."""
import gc
import os
import re

import numpy as np
import pytest
import torch

import triple_hybrid_rag_amd as T
from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient, LazyRows
from triple_hybrid_rag_amd.index import GpuIndex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_csr_compact_is_declared_exported_and_bound():
    lib = T._native.load()
    header = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    for sym in ("thr_csr_compact", "thr_csr_compact_workspace_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in T._native._SIGNATURES and sym in T._native.EXPORTED_SYMBOLS and hasattr(lib, sym)
    assert lib.thr_abi_version() == T._native.ABI_VERSION == 9          # additive: no version bump
    assert "#define THR_ABI_VERSION 9" in header
    assert callable(T._native.csr_compact)


def test_csr_compact_checks_its_arguments_on_the_host():
    lib = T._native.load()
    INVALID, WORKSPACE = -1, -3
    need = lib.thr_csr_compact_workspace_bytes(6, 20_000)
    assert need > 0 and lib.thr_csr_compact_workspace_bytes(6, 0) == 0
    sizes = [lib.thr_csr_compact_workspace_bytes(6, nnz) for nnz in (1, 8192, 8193, 10**6, 10**7, 10**9)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] > sizes[0]          # monotonic in nnz
    p = 4096          # (a non-null, aligned pointer value: every call below is refused before any launch)
    ok = dict(rowptr=p, rows=6, nnz=20_000, ids=p + 64, pay=p + 128, remap=p + 192, n_ids=100, id_base=0,
              rowptr_out=p + 256, ids_out=p + 320, pay_out=p + 384, cap=20_000, nnz_out=p + 448, ws=p + 512,
              ws_bytes=need, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.thr_csr_compact(*[a[k] for k in ok])
    for name in ("rowptr", "rowptr_out", "nnz_out", "ids", "ids_out", "remap", "ws"):   # null pointers with nnz > 0
        assert call(**{name: None}) == INVALID, name
    assert call(pay_out=None) == INVALID and call(pay=None) == INVALID                # one payload in, none out
    assert call(cap=-1) == INVALID and call(nnz=-1) == INVALID and call(n_ids=-1) == INVALID
    assert call(rows=0) == INVALID and call(rows=-3) == INVALID and call(id_base=-1) == INVALID
    assert call(ids_out=ok["ids"]) == INVALID and call(pay_out=ok["pay"]) == INVALID   # out of place only
    assert call(rowptr_out=ok["rowptr"]) == INVALID and call(pay_out=ok["ids_out"]) == INVALID
    assert call(ws_bytes=need - 1) == WORKSPACE and call(ws_bytes=0) == WORKSPACE
    assert b"workspace" in lib.thr_error_string(WORKSPACE).lower()


def test_csr_compact_wrapper_refuses_shapes_and_dtypes_before_any_pointer_is_taken():
    N, E = T._native, T.NativeError
    rowptr = torch.tensor([0, 3, 8], dtype=torch.int64)
    ids = torch.arange(8, dtype=torch.int32)
    remap = torch.arange(8, dtype=torch.int32)
    with pytest.raises(E, match="4-byte"):
        N.csr_compact(rowptr, ids, torch.zeros(8, dtype=torch.float64), remap)
    with pytest.raises(E, match="4-byte"):
        N.csr_compact(rowptr, ids, torch.zeros(8, dtype=torch.float16), remap)
    with pytest.raises(E, match="one per id"):
        N.csr_compact(rowptr, ids, torch.zeros(7, dtype=torch.float32), remap)
    with pytest.raises(E, match="ids_out is too small"):
        N.csr_compact(rowptr, ids, None, remap, 0, torch.zeros(7, dtype=torch.int32))
    with pytest.raises(E, match="pay_out is too small .* or of another dtype"):
        N.csr_compact(rowptr, ids, torch.zeros(8, dtype=torch.float32), remap, 0, None, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(E, match="pay_out without a payload"):
        N.csr_compact(rowptr, ids, None, remap, 0, None, torch.zeros(8, dtype=torch.int32))
    with pytest.raises(E, match="no rows"):
        N.csr_compact(rowptr[:1], ids, None, remap)
    with pytest.raises(E, match="id_base"):
        N.csr_compact(rowptr, ids, None, remap, -5)
    with pytest.raises(E, match="HIP"):                  # well-formed host tensors: refused for where they live
        N.csr_compact(rowptr, ids, None, remap)


def _bare_index(**attrs):
    """A GpuIndex without a device: only what delete_rows' validation reads."""
    idx = object.__new__(GpuIndex)
    base = dict(docs=None, dim=0, n_docs=100, lex=None, doc_coll=None, tokens=None, graph=None, _lex_global=False)
    base.update(attrs)
    idx.__dict__.update(base)
    return idx


def test_delete_rows_validation_runs_before_any_device_work():
    E = T.NativeError
    idx = _bare_index()
    with pytest.raises(E, match="integer"):
        idx.delete_rows(np.array([1.0, 2.0]))
    with pytest.raises(E, match="integer"):
        idx.delete_rows(torch.tensor([True, False]))
    for bad in ([100], [-1], np.array([[3, 4], [5, 200]])):
        with pytest.raises(E, match="local doc ids, 0 .. 99"):
            idx.delete_rows(bad)
    with pytest.raises(E, match="build a new index"):
        idx.delete_rows(np.arange(100))
    with pytest.raises(E, match="build a new index"):
        idx.delete_rows(torch.arange(100).repeat(3))                                  # repeats, a host tensor
    with pytest.raises(E, match="not supported on a document shard"):
        _bare_index(_lex_global=True).delete_rows([1])
    with pytest.raises(E, match="unusable"):
        _bare_index(_unusable="this index is unusable: a delete failed").delete_rows([1])
    assert idx.n_docs == 100


def test_sharded_classes_refuse_deletes_whichever_way_they_arrive():
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    with pytest.raises(T.NativeError, match="not supported"):
        ShardedIndex.delete_rows(object(), [0])
    # the front of a sharded index: its store is the WHOLE corpus, its index one shard -- the table
    # route must stop before the index, the store or the parents are touched
    front = object.__new__(ShardedIndexClient)
    st, idx = _store(), _StubIndex(8)
    front.__dict__.update(index=idx, store=st, org_id="org", image_index=None, image_rows=None)
    seen = []
    front._track(LazyRows(lambda: seen.append("fetched") or []))
    for table, col, val in (("rag_child_chunks", "id", "c1"), ("rag_child_chunks", "document_id", "d0"),
                            ("rag_parent_chunks", "id", "p1"), ("rag_parent_chunks", "id", "p4"),   # (p4: no children)
                            ("rag_parent_chunks", "document_id", "d1"), ("rag_documents", "id", "d0")):
        with pytest.raises(T.NativeError, match="delete is not supported through a sharded index client"):
            front.table(table).delete().eq("org_id", "org").eq(col, val).execute()
        with pytest.raises(T.NativeError, match="not supported"):
            front.table(table).delete().in_(col, [val]).execute()
    with pytest.raises(T.NativeError, match="not supported"):
        front.delete_children(["c1"])
    assert idx.calls == [] and st.child_ids == [f"c{i}" for i in range(8)] and len(st.parents) == 5 and seen == []
    assert not hasattr(ShardedIndexClient, "delete_parents")
    # what the table surface refuses by itself is refused the same way
    with pytest.raises(ValueError, match="WHERE"):
        front.table("rag_child_chunks").delete().execute()
    assert front.table("rag_documents").delete().eq("org_id", "other").eq("id", "d0").execute().data == []


def _store(n=8):
    """n chunks, two per parent, four per document."""
    return CorpusStore(child_ids=[f"c{i}" for i in range(n)], parent_ids=[f"p{i // 2}" for i in range(n)],
                       document_ids=[f"d{i // 4}" for i in range(n)], texts=[f"alpha beta t{i}" for i in range(n)],
                       pages=[None if i == 3 else i for i in range(n)], modalities=["text"] * n,
                       parents={f"p{j}": {"id": f"p{j}", "text": f"P{j}", "section_heading": None}
                                for j in range((n + 1) // 2 + 1)},          # (the last parent has no children)
                       collections=[("a", "b", None)[i % 3] for i in range(n)],
                       vocab={"alpha": 0, "beta": 1, **{f"t{i}": 2 + i for i in range(n)}},
                       content_hashes=[f"h{i}" for i in range(n)])


def test_corpus_store_delete():
    st = _store()
    gone = st.delete([5, 1, 5, 2])
    assert [r["id"] for r in gone] == ["c1", "c2", "c5"] and gone[0] == {
        "id": "c1", "parent_id": "p0", "document_id": "d0", "text": "alpha beta t1", "page": 1, "modality": "text"}
    assert st.child_ids == ["c0", "c3", "c4", "c6", "c7"] and st.parent_ids == ["p0", "p1", "p2", "p3", "p3"]
    assert st.document_ids == ["d0", "d0", "d1", "d1", "d1"] and st.pages == [0, None, 4, 6, 7]
    assert st.texts[1] == "alpha beta t3" and st.modalities == ["text"] * 5
    assert st.collections == ["a", "a", "b", "a", "b"] and st.content_hashes == ["h0", "h3", "h4", "h6", "h7"]
    assert [st.row_index(c) for c in ("c0", "c3", "c7", "c1", "c5")] == [0, 1, 4, None, None]
    assert st.has_hash("h3") and not st.has_hash("h1") and not st.has_hash("h5")
    assert len(st.vocab) == 10 and len(st.parents) == 5                  # term ids never move; parents are the client's
    assert st.delete([]) == [] and len(st.child_ids) == 5
    with pytest.raises(ValueError, match="out of range"):
        st.delete([5])
    with pytest.raises(ValueError, match="out of range"):
        st.delete([-1])
    assert len(st.child_ids) == 5
    # a deleted id and a deleted content hash can be ingested again; a surviving one still cannot
    assert st.append([{"id": "c1", "text": "alpha new", "content_hash": "h1", "collection": "b"}]) == range(5, 6)
    assert st.row_index("c1") == 5 and st.has_hash("h1")
    with pytest.raises(ValueError, match="duplicate"):
        st.append([{"id": "z", "content_hash": "h3"}])


def test_a_loaded_blob_backed_store_takes_deletes(tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    rows = [{"id": f"c{i}", "text": f"a b c{i}", "page": None if i == 1 else i, "content_hash": f"h{i}",
             "document_id": f"d{i // 2}", "embedding_1024": [float(i), 1.0, 0.0, 0.0]} for i in range(5)]
    path = str(tmp_path / "idx")
    IB.save(IB.from_rows(rows), path)
    st = IB.load(path).store
    assert not isinstance(st.child_ids, list)                            # blob + offsets until the first change
    assert [r["id"] for r in st.delete([1, 4])] == ["c1", "c4"]
    assert st.child_ids == ["c0", "c2", "c3"] and st.pages == [0, 2, 3] and st.content_hashes == ["h0", "h2", "h3"]
    assert st.row_index("c3") == 2 and not st.has_hash("h4") and st.has_hash("h2")
    st.append([{"id": "c4", "text": "again", "content_hash": "h4"}])
    assert st.row_index("c4") == 3


class _Shape:
    def __init__(self, *shape):
        self.shape = shape


class _StubIndex:
    """What GpuIndexClient's delete path needs of an index: delete_rows (recorded)."""

    def __init__(self, n, refuse=False):
        self.docs, self.dim, self.n_docs = object(), 4, n
        self.lex = {"rowptr": _Shape(11)}
        self.doc_coll = self.tokens = self.graph = None
        self.calls, self.refuse, self.store_rows_at_call = [], refuse, []
        self.before = None

    def delete_rows(self, ids):
        if self.before is not None:
            self.before()
        if self.refuse:
            raise T.NativeError("delete_rows: every row would be deleted: build a new index")
        self.calls.append(np.asarray(ids).tolist())
        self.n_docs -= len(set(self.calls[-1]))


def _client(n=8, **kw):
    st = _store(n)
    idx = _StubIndex(n, **kw)
    idx.doc_coll = object()       # (the store has collections: the stub pretends they are set)
    return GpuIndexClient(idx, st, org_id="org"), idx, st


def test_child_table_delete_by_each_filter_form():
    client, idx, st = _client()
    tbl = lambda: client.table("rag_child_chunks")
    got = tbl().delete().eq("id", "c6").execute().data
    assert got == [{"id": "c6", "parent_id": "p3", "document_id": "d1", "text": "alpha beta t6", "page": 6,
                    "modality": "text"}]
    assert idx.calls == [[6]] and st.row_index("c6") is None and st.row_index("c7") == 6
    assert [r["id"] for r in tbl().delete().eq("org_id", "org").eq("parent_id", "p1").execute().data] == ["c2", "c3"]
    assert idx.calls[-1] == [2, 3] and st.child_ids == ["c0", "c1", "c4", "c5", "c7"]
    assert [r["id"] for r in tbl().delete().in_("id", ["c7", "nope", "c0", "c7"]).execute().data] == ["c0", "c7"]
    assert idx.calls[-1] == [0, 4]                                       # rows of the store as it is NOW
    assert [r["id"] for r in tbl().delete().in_("document_id", ["d1", "dx"]).execute().data] == ["c4", "c5"]
    assert st.child_ids == ["c1"] and idx.n_docs == 1
    # several filters combine with AND
    client, idx, st = _client()
    assert [r["id"] for r in tbl().delete().eq("document_id", "d0").eq("parent_id", "p1").execute().data] == ["c2", "c3"]
    assert tbl().delete().eq("document_id", "d0").eq("parent_id", "p3").execute().data == [] and len(idx.calls) == 1
    assert [r["id"] for r in tbl().delete().in_("id", ["c0", "c4", "c5"]).eq("document_id", "d1").execute().data] == ["c4", "c5"]
    # unknown ids delete nothing and are not an error; the index is not called
    n_calls = len(idx.calls)
    assert tbl().delete().eq("id", "nope").execute().data == [] and tbl().delete().in_("id", []).execute().data == []
    assert len(idx.calls) == n_calls and len(st.child_ids) == 4
    # the direct call
    assert [r["id"] for r in client.delete_children(["c1", "zz"])] == ["c1"]
    # selects are as before
    assert [r["id"] for r in tbl().select("*").in_("id", ["c0", "c1", "c6"]).execute().data] == ["c0", "c6"]
    with pytest.raises(ValueError, match="only id"):
        tbl().select("*").in_("document_id", ["d0"])


def test_deletes_that_are_refused():
    client, idx, st = _client()
    tbl = lambda: client.table("rag_child_chunks")
    for q in (tbl().delete(), tbl().delete().eq("org_id", "org"), tbl().delete().eq("org_id", "other"),
              client.table("rag_parent_chunks").delete(), client.table("rag_documents").delete().eq("org_id", "org")):
        with pytest.raises(ValueError, match="WHERE"):                    # no filter other than org_id
            q.execute()
    # another tenant's rows: nothing of this index matches
    assert tbl().delete().eq("org_id", "other").eq("document_id", "d0").execute().data == []
    assert client.table("rag_documents").delete().eq("id", "d0").eq("org_id", "other").execute().data == []
    with pytest.raises(ValueError, match="addressed by"):
        tbl().delete().eq("text", "alpha").execute()
    with pytest.raises(ValueError, match="addressed by"):
        client.table("rag_parent_chunks").delete().eq("parent_id", "p0").execute()
    with pytest.raises(ValueError, match="addressed by"):
        client.table("rag_documents").delete().eq("document_id", "d0").execute()
    with pytest.raises(ValueError, match="read-only"):
        client.table("organizations").delete()
    assert idx.calls == [] and len(st.child_ids) == 8 and len(st.parents) == 5
    # the index refuses (every row): the store is untouched -- index first, store second
    client, idx, st = _client(refuse=True)
    with pytest.raises(T.NativeError, match="build a new index"):
        client.table("rag_child_chunks").delete().in_("document_id", ["d0", "d1"]).execute()
    assert len(st.child_ids) == 8 and st.has_hash("h0") and st.row_index("c7") == 7


def test_parent_and_document_deletes_cascade():
    client, idx, st = _client()
    got = client.table("rag_parent_chunks").delete().eq("id", "p1").execute().data
    assert got == [{"id": "p1", "text": "P1", "section_heading": None}]
    assert idx.calls == [[2, 3]] and "p1" not in st.parents and st.child_ids == ["c0", "c1", "c4", "c5", "c6", "c7"]
    # a parent without children: only the parent row goes
    assert [p["id"] for p in client.table("rag_parent_chunks").delete().in_("id", ["p4", "zz"]).execute().data] == ["p4"]
    assert len(idx.calls) == 1 and "p4" not in st.parents
    # parents of a document
    got = client.table("rag_parent_chunks").delete().eq("document_id", "d1").execute().data
    assert [p["id"] for p in got] == ["p2", "p3"] and idx.calls[-1] == [2, 3, 4, 5]
    assert st.child_ids == ["c0", "c1"] and sorted(st.parents) == ["p0"]
    # a document: its children and the parents they reference
    client, idx, st = _client()
    assert client.table("rag_documents").delete().eq("id", "d0").execute().data == [{"id": "d0"}]
    assert idx.calls == [[0, 1, 2, 3]] and st.child_ids == ["c4", "c5", "c6", "c7"]
    assert sorted(st.parents) == ["p2", "p3", "p4"] and not st.has_hash("h2")
    assert client.table("rag_documents").delete().eq("id", "d0").execute().data == []      # already gone
    assert client.table("rag_documents").delete().in_("id", ["dx"]).execute().data == [] and len(idx.calls) == 1
    # the same content can come back (re-ingest after a withdrawn document)
    row = {"id": "c1", "parent_id": "p0", "document_id": "d0", "org_id": "org", "text": "alpha", "content_hash": "h1",
           "embedding_1024": [1, 2, 3, 4], "collection": "a"}
    idx.append_rows = lambda docs, lex=None, collections=None: range(4, 5)
    assert client.table("rag_child_chunks").insert(row).execute().data == [{"id": "c1"}]
    assert st.row_index("c1") == 4
    # the tenant discovery select of the documents table is as before
    assert client.table("rag_documents").select("org_id").limit(1).execute().data == [{"org_id": "org"}]


def test_pending_lazy_rows_are_materialised_before_anything_moves():
    client, idx, st = _client()
    seen = []

    def fetch():                      # a deferred reply: resolves LOCAL ids against the store when looked at
        seen.append(list(st.child_ids))
        return [st.result_row(6)]
    lazy, dropped = LazyRows(fetch), LazyRows(lambda: seen.append("dropped") or [])
    client._track(lazy)
    client._track(dropped)
    del dropped                       # nobody holds it any more: it is not kept alive, and not fetched
    gc.collect()
    idx.before = lambda: seen.append("index")
    client.table("rag_child_chunks").delete().eq("document_id", "d0").execute()
    # fetched once, before the index and the store changed, against the OLD numbering
    assert seen == [[f"c{i}" for i in range(8)], "index"]
    assert lazy.materialize()[0]["child_id"] == "c6" and len(seen) == 2
    assert st.child_ids[2] == "c6"                                       # (row 6 is row 2 now)
    # a reply whose fetch fails does not stop the delete; its caller sees the failure when it looks
    def boom():
        raise RuntimeError("HIP error")
    bad = LazyRows(boom)
    client._track(bad)
    client.delete_children(["c4"])
    assert st.child_ids == ["c5", "c6", "c7"]
    with pytest.raises(RuntimeError, match="HIP error"):
        len(bad)
    # a delete that matches nothing leaves a pending reply pending
    later = LazyRows(lambda: seen.append("later") or [])
    client._track(later)
    client.delete_children(["nope"])
    assert "later" not in seen


class _HostSideIndex:
    """What index_build.save / refresh_from_gpu read of a GpuIndex, on host tensors."""

    def __init__(self, docs, tokens, packed, mutations):
        self.docs, self.tokens, self.tokens_packed = torch.from_numpy(docs), torch.from_numpy(tokens), packed
        self.n_docs, self.lex, self.graph, self._mutations = len(docs), None, None, mutations

    def export_derived(self):
        return {}


def test_save_after_mutations_with_a_token_store(tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    rng = np.random.default_rng(3)
    docs = rng.standard_normal((5, 4)).astype(np.float32)
    tok = rng.standard_normal((5, 2, 8)).astype(np.float16)
    path = str(tmp_path / "idx")
    # packed layout (the default of to_gpu): the rows cannot be pulled back, so the caller keeps
    # HostIndex.tokens in step -- append, extend hi.tokens, save: as before deletes existed
    hi = IB.HostIndex(docs=docs[:3].copy(), tokens=tok[:3].copy())
    g = _HostSideIndex(docs, np.zeros((5, 99), np.float16), packed=True, mutations=1)
    with pytest.raises(ValueError, match="packed layout"):
        IB.save(hi, path, g)                                 # hi.tokens is 3 rows, the index 5
    hi.tokens = tok.copy()
    IB.save(hi, path, g)
    IB.save(hi, path, g)                                     # and again
    back = IB.load(path)
    assert np.array_equal(back.docs, docs) and np.array_equal(back.tokens, tok)
    # same row count after a delete + append: the rows are pulled back all the same, the packed tokens trusted
    g2 = _HostSideIndex(docs[::-1].copy(), np.zeros((5, 99), np.float16), packed=True, mutations=2)
    IB.save(hi, path, g2)
    assert np.array_equal(IB.load(path).docs, docs[::-1]) and np.array_equal(hi.tokens, tok)
    # a row-major token store is pulled back with the rows
    g3 = _HostSideIndex(docs, tok[::-1].copy(), packed=False, mutations=4)
    IB.save(hi, path, g3)
    assert np.array_equal(IB.load(path).tokens, tok[::-1])
    # an index without mutations built from the same HostIndex (a second to_gpu) pulls nothing
    hi.docs = docs + 1
    IB.save(hi, path, _HostSideIndex(docs, tok, packed=False, mutations=0))
    assert np.array_equal(IB.load(path).docs, docs + 1)
    # ... and the same index at the same mutation count is not pulled twice
    IB.save(hi, path, g3)
    hi.docs = docs + 2
    IB.save(hi, path, g3)
    assert np.array_equal(IB.load(path).docs, docs + 2)
