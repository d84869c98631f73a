"""Incremental ingest, the parts that need no GPU: the new C entry's host-side argument checks,
``GpuIndex.append_rows`` validation (which runs before any device work), ``CorpusStore.append``
and the ingest seam of the table surface over a stub index."""
import numpy as np
import pytest

import triple_hybrid_rag_amd as T
from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
from triple_hybrid_rag_amd.index import GpuIndex


def test_csr_append_is_exported_and_checks_its_arguments_on_the_host():
    lib = T._native.load()
    assert "thr_csr_append" in T._native.EXPORTED_SYMBOLS and hasattr(lib, "thr_csr_append")
    assert lib.thr_abi_version() == T._native.ABI_VERSION == 9          # additive: no version bump
    INVALID = -1
    p = 4096          # (a non-null, aligned pointer value: every call below is refused before any launch)
    ok = dict(rowptr_a=p, rows_a=4, nnz_a=8, a0=p + 64, a1=p + 128, rowptr_b=p + 192, rows_b=6, nnz_b=3,
              b0=p + 256, b1=p + 320, rowptr_out=p + 384, out0=p + 448, out1=p + 512, cap=11, stream=None)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.thr_csr_append(*[a[k] for k in ok])
    assert call(rowptr_b=None) == INVALID and call(rowptr_out=None) == INVALID      # null pointers
    assert call(rowptr_a=None) == INVALID and call(a0=None) == INVALID and call(b0=None) == INVALID
    assert call(out0=None) == INVALID and call(a1=None) == INVALID and call(b1=None) == INVALID
    assert call(rows_b=3) == INVALID                                                  # R_b < R
    assert call(rows_a=-1) == INVALID and call(nnz_a=-1) == INVALID and call(nnz_b=-2) == INVALID
    assert call(rows_b=0, rows_a=0) == INVALID
    assert call(cap=10) == INVALID                                                    # destination too small
    assert call(out1=None) == INVALID                                                 # one payload out, two in
    assert call(out0=ok["a0"]) == INVALID and call(rowptr_out=ok["rowptr_b"]) == INVALID   # out of place only
    assert call(rows_a=0, rowptr_a=None, nnz_a=5) == INVALID                          # postings without rows


def _bare_index(**attrs):
    """A GpuIndex without a device: only what append_rows' validation reads."""
    idx = object.__new__(GpuIndex)
    base = dict(docs=None, dim=0, n_docs=100, lex=None, doc_coll=None, tokens=None, graph=None,
                _lex_global=False)
    base.update(attrs)
    idx.__dict__.update(base)
    return idx


class _Shape:
    def __init__(self, *shape):
        self.shape = shape


def test_append_rows_validation_runs_before_any_device_work():
    E = T.NativeError
    lexical = _bare_index(docs=_Shape(100, 8), dim=8, lex={"rowptr": _Shape(51)})
    rows = np.zeros((3, 8), dtype=np.float32)
    d, t = np.array([0, 1, 2], dtype=np.int32), np.array([4, 50, 7], dtype=np.int32)
    with pytest.raises(E, match="lexical channel: lex=.* is required"):
        lexical.append_rows(rows)
    with pytest.raises(E, match="one length"):
        lexical.append_rows(rows, lex=(d, t[:2], None, 60))                           # ragged
    with pytest.raises(E, match="term id 50 >= n_vocab 50"):
        lexical.append_rows(rows, lex=(d, t, None, 50))
    with pytest.raises(E, match="smaller than the index's vocabulary"):
        lexical.append_rows(rows, lex=(d, np.array([1, 2, 3], dtype=np.int32), None, 40))
    with pytest.raises(E, match="local to the batch"):
        lexical.append_rows(rows, lex=(d + 1, t, None, 60))
    with pytest.raises(E, match="integer"):
        lexical.append_rows(rows, lex=(d.astype(np.float32), t, None, 60))
    with pytest.raises(E, match=r"docs must be \[m, 8\]"):
        lexical.append_rows(np.zeros((3, 16), dtype=np.float32), lex=(d, t, None, 60))
    with pytest.raises(E, match="no collection ids"):
        lexical.append_rows(rows, lex=(d, t, None, 60), collections=np.zeros(3, dtype=np.int32))
    sharded = _bare_index(docs=_Shape(100, 8), dim=8, lex={"rowptr": _Shape(51)}, _lex_global=True)
    with pytest.raises(E, match="not supported on a document shard"):
        sharded.append_rows(rows, lex=(d, t, None, 60))
    graph = _bare_index(docs=_Shape(100, 8), dim=8, graph={"men_rowptr": _Shape(11)}, doc_coll=_Shape(100))
    with pytest.raises(E, match="collections .* is required"):
        graph.append_rows(rows)
    c = np.zeros(3, dtype=np.int32)
    with pytest.raises(E, match="mentions=.* is required"):
        graph.append_rows(rows, collections=c)
    with pytest.raises(E, match="existing entities"):
        graph.append_rows(rows, collections=c, mentions=(np.array([10]), np.array([0]), None))
    with pytest.raises(E, match="local to the batch"):
        graph.append_rows(rows, collections=c, mentions=(np.array([9]), np.array([3]), None))
    with pytest.raises(E, match="needs n_rows"):
        _bare_index(lex={"rowptr": _Shape(51)}).append_rows(None, lex=(d, t, None, 60))
    # an empty batch is a no-op (no device is touched)
    assert lexical.append_rows(rows[:0], lex=(d[:0], t[:0], None, 50)) == range(100, 100)


def test_storage_knows_the_buffer_behind_an_array_until_the_array_is_replaced():
    import torch
    from triple_hybrid_rag_amd.index_mutate import _Storage
    S = _Storage()
    docs, docs16 = torch.arange(40.0).reshape(20, 2), torch.ones(32, 2, dtype=torch.float16)
    assert S.behind("docs", docs) is docs and S.with_room("docs", docs, 20) is docs
    assert S.padded("docs16", 33) == 64 and S.padded("docs", 33) == 33
    # reserve: exactly the rows asked for (the float16 image: whole tiles), the old rows copied
    buf, buf16 = S.with_room("docs", docs, 50, exact=True), S.with_room("docs16", docs16, 50, exact=True)
    assert buf.shape == (50, 2) and buf16.shape == (64, 2) and torch.equal(buf[:20], docs)
    view = buf[:20]
    S.held["docs"] = (buf, view)
    assert S.behind("docs", view) is buf and S.with_room("docs", view, 50) is buf
    grown = S.with_room("docs", view, 51)                  # too small: GROWTH x the rows so far, at least the need
    assert grown.shape[0] == 51 and torch.equal(grown[:20], docs)
    S.held["docs"] = (buf, buf[:])
    assert S.with_room("docs", S.held["docs"][1], 51).shape[0] == 75
    # a builder replaced the array (set_dense again): the record is about a tensor the index no longer holds
    again = docs.clone()
    assert S.behind("docs", again) is again and S.with_room("docs", again, 25).shape[0] == 30
    # CSR payloads: the buffer a mutation read from is the next one's destination
    old = torch.arange(8, dtype=torch.int32)
    dest = S.destination("post_doc", old, 10, grow=True)
    assert dest.shape[0] == 12 and S.destination("post_doc", old, 8, grow=False).shape[0] == 8
    S.rotate({"post_doc": (dest, dest[:10])}, {"post_doc": old, "doclen": docs})
    assert S.spare == {"post_doc": old} and S.held["post_doc"][0] is dest
    assert S.destination("post_doc", S.held["post_doc"][1], 8, grow=False) is old
    assert S.destination("post_doc", S.held["post_doc"][1], 9, grow=False).shape[0] == 9      # no room
    assert S.destination("post_doc", old[:4], 4, grow=False) is not old                        # never its own source


def test_sharded_classes_refuse_appends():
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    with pytest.raises(T.NativeError, match="not supported"):
        ShardedIndex.append_rows(object())
    with pytest.raises(T.NativeError, match="not supported"):
        ShardedIndexClient.insert_children(object(), [])


def _store(n=6):
    return CorpusStore(child_ids=[f"c{i}" for i in range(n)], parent_ids=[f"p{i // 2}" for i in range(n)],
                       document_ids=["d0"] * n, texts=[f"alpha beta t{i}" for i in range(n)],
                       pages=[1] * n, modalities=["text"] * n,
                       parents={f"p{j}": {"id": f"p{j}", "text": f"P{j}", "section_heading": None} for j in range(3)},
                       vocab={"alpha": 0, "beta": 1, **{f"t{i}": 2 + i for i in range(n)}},
                       content_hashes=[f"h{i}" for i in range(n)])


def test_corpus_store_append():
    from triple_hybrid_rag_amd.backend import tokenize
    st = _store()
    r = st.append([{"id": "n0", "parent_id": "p9", "text": "alpha gamma delta", "page": None, "content_hash": "hn0"},
                   {"id": "n1", "text": "gamma t0"}], tokenizer=tokenize)
    assert r == range(6, 8) and st.row_index("n1") == 7
    assert st.child_row(6) == {"id": "n0", "parent_id": "p9", "document_id": None, "text": "alpha gamma delta",
                               "page": None, "modality": "text"}                     # nullable page
    assert st.pages[7] == 1 and st.content_hashes[6:] == ["hn0", None]
    # new terms at the END: existing ids never move
    assert st.vocab["alpha"] == 0 and st.vocab["t5"] == 7 and st.vocab["gamma"] == 8 and st.vocab["delta"] == 9
    assert st.has_hash("hn0") and st.has_hash("h2") and not st.has_hash(None) and not st.has_hash("zz")
    for bad in ({"id": "c1", "text": ""}, {"id": "n2", "content_hash": "hn0"}):
        with pytest.raises(ValueError, match="duplicate"):
            st.append([bad])
    with pytest.raises(ValueError, match="duplicate"):                                 # inside one batch
        st.append([{"id": "a", "content_hash": "q"}, {"id": "b", "content_hash": "q"}])
    assert len(st.child_ids) == 8                                                      # refused whole


class _StubIndex:
    """What GpuIndexClient.insert_children needs of an index: the channels and append_rows."""

    def __init__(self, n, dim, v):
        self.docs, self.dim, self.n_docs = object(), dim, n
        self.lex = {"rowptr": _Shape(v + 1)}
        self.doc_coll = self.tokens = self.graph = None
        self.calls = []

    def append_rows(self, docs, lex=None, **kw):
        assert not kw
        self.calls.append((docs, lex))
        self.n_docs += len(docs)
        return range(self.n_docs - len(docs), self.n_docs)


def test_table_surface_of_the_ingest_seam():
    st = _store()
    idx = _StubIndex(6, 4, len(st.vocab))
    client = GpuIndexClient(idx, st, org_id="org")
    tbl = lambda: client.table("rag_child_chunks")
    # the dedup lookup (ingest.py:384-392)
    q = tbl().select("content_hash").eq("org_id", "org").in_("content_hash", ["h1", "nope", "h4", "h1"])
    assert q.execute().data == [{"content_hash": "h1"}, {"content_hash": "h4"}]
    assert tbl().select("content_hash").eq("org_id", "other").in_("content_hash", ["h1"]).execute().data == []
    # one row = one append; the row carries its embedding; no embedding = a zero vector
    row = {"id": "u1", "parent_id": "p0", "document_id": "d1", "org_id": "org", "text": "Beta epsilon beta",
           "page": None, "modality": "text", "content_hash": "hu1", "embedding_1024": [1, 2, 3, 4],
           "token_count": 3, "metadata": {}}
    assert tbl().insert(row).execute().data == [{"id": "u1"}]
    docs, (d, t, tf, n_vocab) = idx.calls[0]
    assert docs.dtype == np.float32 and docs.tolist() == [[1.0, 2.0, 3.0, 4.0]]
    assert d.tolist() == [0, 0, 0] and t.tolist() == [1, 8, 1] and tf is None and n_vocab == 9
    assert st.vocab["epsilon"] == 8 and st.child_row(6)["page"] is None and st.has_hash("hu1")
    # a list = one append of m rows
    more = [dict(row, id="u2", content_hash="hu2", embedding_1024=None), dict(row, id="u3", content_hash=None)]
    assert tbl().insert(more).execute().data == [{"id": "u2"}, {"id": "u3"}]
    assert len(idx.calls) == 2 and idx.calls[1][0].tolist() == [[0.0] * 4, [1.0, 2.0, 3.0, 4.0]]
    assert tbl().select("*").in_("id", ["u3", "c0"]).execute().data[0]["text"] == "Beta epsilon beta"
    # duplicates (what the reference's ingest catches, ingest.py:457-460), another tenant
    for bad in (dict(row, id="u9"), dict(row, content_hash="fresh")):
        with pytest.raises(Exception, match="duplicate"):
            tbl().insert(bad).execute()
    with pytest.raises(ValueError, match="org_id"):
        tbl().insert(dict(row, id="u9", content_hash="h9", org_id="other")).execute()
    with pytest.raises(ValueError, match="dims"):
        tbl().insert(dict(row, id="u9", content_hash="h9", embedding_1024=[1, 2])).execute()
    assert len(idx.calls) == 2 and len(st.child_ids) == 9                             # nothing changed
    # parents
    ptab = client.table("rag_parent_chunks")
    assert ptab.insert({"id": "p7", "text": "P7", "section_heading": "S", "org_id": "org"}).execute().data == [{"id": "p7"}]
    assert client.table("rag_parent_chunks").select("*").in_("id", ["p7"]).execute().data == \
        [{"id": "p7", "text": "P7", "section_heading": "S"}]
    with pytest.raises(ValueError, match="read-only"):
        client.table("rag_documents").insert({"id": 1})


def test_save_keeps_nullable_pages_hashes_and_drops_stale_derived_files(tmp_path):
    from triple_hybrid_rag_amd import index_build as IB
    rows = [{"id": f"c{i}", "text": f"a b c{i}", "page": None if i == 1 else i, "content_hash": f"h{i}",
             "embedding_1024": [float(i), 1.0, 0.0, 0.0]} for i in range(4)]
    hi = IB.from_rows(rows)
    hi.derived = {"docs16": np.zeros((32, 4), dtype=np.float16), "doc_rel_err": 1e-4, "f16_layout": "x"}
    path = str(tmp_path / "idx")
    IB.save(hi, path)
    assert (tmp_path / "idx" / "derived_docs16.npy").exists()
    hi.derived = None
    IB.save(hi, path)                       # a re-save without derived arrays leaves none behind
    assert not (tmp_path / "idx" / "derived_docs16.npy").exists()
    back = IB.load(path)
    assert back.store.pages == [0, None, 2, 3] and list(back.store.content_hashes) == ["h0", "h1", "h2", "h3"]
    assert back.store.has_hash("h2") and back.derived is None
    back.store.append([{"id": "z", "text": "q", "content_hash": "hz"}])      # a loaded store takes appends
    assert back.store.row_index("z") == 4 and back.store.child_ids[4] == "z"
    with pytest.raises(ValueError, match="not appended to together"):
        IB.save(back, path)
