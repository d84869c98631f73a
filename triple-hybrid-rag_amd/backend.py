"""Backend seam: a Supabase-shaped client answered by the GPU index.

The reference's retriever talks to PostgREST through four calls (SURVEY.md
section 8b; src/voice_agent/rag2/retrieval.py:282-290, 304-312, 339-341, 390-392):

    client.rpc("rag2_lexical_search",  {p_org_id, p_query, p_limit, p_collection}).execute().data
    client.rpc("rag2_semantic_search", {p_org_id, p_embedding, p_limit, p_collection}).execute().data
    client.table("rag_child_chunks").select(...).in_("id", ids).execute().data
    client.table("rag_parent_chunks").select(...).in_("id", ids).execute().data

``GpuIndexClient`` offers exactly that duck type.  The two RPCs run the HIP
scorers (thr_bm25_topk / thr_dense_topk + exhaustive rescue) on a ``GpuIndex``;
the table fetches are answered from ``CorpusStore``, the host-side row payloads
(ids, text, page, modality, parents) that the SQL rows would carry.
Rows come back in REQUEST order from ``in_()`` (PostgreSQL's order there is
unspecified; the reference ranks graph hits by that order, Appendix A.7).

The ingest seam (src/voice_agent/rag2/ingest.py:361-470) is served too:

    client.table("rag_child_chunks").select("content_hash").eq("org_id", o).in_("content_hash", hs).execute().data
    client.table("rag_child_chunks").insert(row | [rows]).execute().data      -> [{"id": ...}, ...]
    client.table("rag_parent_chunks").insert(row | [rows]).execute().data

An insert appends to the store AND to the live index (``GpuIndex.append_rows``): the next
``retrieve()`` sees the chunk.

Deletes are served as the SQL store serves them (ON DELETE CASCADE from documents to parents to
children, database/migrations/20260114_rag2_schema.sql:65-66, 106-108; the reference's own tests
clear a tenant this way, tests/test_rag2_e2e.py:276-293):

    client.table("rag_child_chunks").delete().eq("id" | "document_id" | "parent_id", v).execute().data
    client.table("rag_child_chunks").delete().in_("id" | "document_id", vs).execute().data
    client.table("rag_parent_chunks").delete().eq("id" | "document_id", v).execute().data   (+ their children)
    client.table("rag_documents").delete().eq("id", d).execute().data      (+ its children and their parents)

A delete removes the chunks from the live index (``GpuIndex.delete_rows``: the next ``retrieve()``
no longer sees them) and from the store; an update is a delete followed by an insert.

One client serves one tenant (``org_id=``) or, over a store with a per-row ``org_ids`` column and no
``org_id`` of its own, all of them: ``p_org_id`` then selects the rows a call ranks (scoped queries,
the graph channel included -- the reference's WHERE org_id = $1 and .eq("org_id", org_id)).
"""
from __future__ import annotations

from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .backend_ingest import ClientIngest
from .backend_tables import TABLES, LazyRows, _Reply, _TableQuery
from .index import GpuIndex
from .index_diversify import check_lam
from .index_entities import match_names, name_trigrams
from .index_scope import In
from .index_text import _TOKEN, TextTable, check_fuzzy, host_query_row, tokenize, tokenizer_table  # noqa: F401
from .store import CorpusStore


class GpuIndexClient(ClientIngest):
    """Supabase-shaped facade over (GpuIndex, CorpusStore); the writing half is ``ClientIngest``."""

    defers_readback = True   # rag2_lexical_search honours ``_defer`` (see _lexical)
    sets_collections = True  # derives the index's per-doc collection ids from the store's rows
    multi_tenant = False     # set by __init__: no org_id of its own over a store with an org_ids column
    graph_cascade = False    # set by __init__: a document delete also removes the entities first extracted from it
    tokenizer = staticmethod(tokenize)   # set by __init__: what turns a query's and a chunk's text into tokens
    parent_rerank = False    # set by __init__: maxsim_scores scores a chunk's parent passage (index "parent" column)
    diversify = None         # set by __init__: MMR's lambda of the final cut (mmr_order), None = the plain truncation

    # Derived state, made by __init__ (the class values serve a subclass with an __init__ of its own):
    #   attribute     derived from                                   filled by           dropped by (backend_ingest)
    #   _pending_lex  the index's lexical workspace in flight        _lexical(defer)     next _lexical, _settle_deferred
    #   _lazy         the local doc ids of unresolved replies        _track              _settle_deferred (_rows_changed, a delete)
    #   _plans        the index's rows, attributes and collections   _plan               _rows_changed
    #   _by_text      store.texts / child_ids, store.parents         text_to_child_id    _rows_changed, _parents_changed
    #   _tri          store.entity_names                             _entity_index       _graph_changed
    #   _pin          nothing (staging buffers by dtype and width)   _upload             never
    _pending_lex = _by_text = _tri = None
    _lazy: Sequence = ()

    def __init__(self, index: GpuIndex, store: CorpusStore, org_id: Optional[str] = None,
                 token_embedder: Any = None, lexical_and: bool = False,
                 image_index: Optional[GpuIndex] = None, image_rows: Any = None,
                 collection_names: Optional[Sequence[str]] = None, device_text: bool = False,
                 tokenizer: Any = None, number_on_device: bool = False, graph_cascade: bool = False,
                 parent_rerank: bool = False, diversify: Optional[float] = None, fuzzy: Any = None):
        """lexical_and: rank only chunks holding EVERY query term, as the reference's ``plainto_tsquery`` does
        (rag2_schema.sql:365); default is BM25's OR form, the north star's and the oracle's.
        image_index / image_rows: the legacy image channel (``kb_chunks_image_search``,
        20260113_add_kb_chunks.sql:236-268): a second dense index over the ``vector_image`` of the chunks that have one
        (``vector_image IS NOT NULL``), row j of it being store row ``image_rows[j]``.
        collection_names: fixes the collection name -> id mapping (sorted names of the WHOLE corpus): the shards of a
        document-sharded index must agree on it (sharded_client.py); default: the names this store's rows carry.
        org_id: the one tenant this client serves -- any other ``p_org_id`` is answered with no rows.  None over a store
        that has an ``org_ids`` column makes the client MULTI-TENANT: one index, one store, every tenant.  The index
        gets an ``"org"`` attribute column (the ids of the sorted distinct names; one it already has is checked against
        the store's column), each RPC and ``graph_chunks`` rank inside {"org": p_org_id} (+ "collection") through the
        index's scopes, a missing or unknown org gets no rows, ``table().eq("org_id", x)`` filters rows, and an insert
        needs ``org_id`` on every row.
        tokenizer: what the index's vocabulary was built with (default ``tokenize``, from_rows' default); queries and
        inserted chunks go through it.  An ``Analyzer``'s ``.tokenize`` (stop list + stemming) counts as a table's below.
        device_text: query and chunk text become term ids on the device (GpuIndex.set_vocabulary from ``store.vocab``
        -- derived state, rebuilt here, never saved): ``_lexical`` and ``insert_children`` take that route and
        ``query_terms_batch`` serves batches.  Needs ``tokenize`` or a TextTable's ``.tokenize`` as the tokenizer; any
        other is refused by name.
        number_on_device: (with device_text) ``insert_children`` also numbers the batch's new terms on the device
        (GpuIndex.number_text_rows / commit_vocabulary): the unknown tokens are not decoded one occurrence at a time,
        the new keys stay on the device, and the store's vocabulary gets one string per distinct new term.  The ids are
        the host loop's.  Without device_text it is refused by name.
        graph_cascade: ``table("rag_documents").delete()`` also removes the entities whose ``document_id`` is a deleted
        document, with their relations and mentions, as the schema's ON DELETE CASCADE does (rag2_schema.sql:187,
        217-220, 254, 258-259).  Needs the store's ``entity_documents`` column; default False: entities outlive their
        document, the behaviour before the flag.
        parent_rerank: ``maxsim_scores`` -- what ``Reranker._rerank_batch_native`` and ``RAG2Retriever._rerank`` rank on
        -- scores a chunk's PARENT passage (the token blocks of every chunk of the same parent), as the reference
        reranks ``c.parent_text or c.text`` (retrieval.py:419).  ``store.parent_ids`` are numbered by first appearance
        (None -> -1) into the index's "parent" column (GpuIndex.set_parents; one the index already has is checked
        against the store's column), ``insert_children`` passes the column with each append.  Needs a token store in
        the packed float16 or the FP8 layout.  Default False: the chunk's own tokens, the behaviour before the flag.
        diversify: MMR's lambda in [0, 1], or None.  With a value the final cut of ``RAG2Retriever._apply_safety``
        -- ``kept[:top_k]`` in the reference -- becomes ``mmr_order``: the top_k chosen greedily for relevance
        (``_effective_score``, min-max normalised) and dissimilarity to what is already chosen, the similarities taken
        from the index's dense rows on the device (GpuIndex.diversify).  Needs an index with dense rows.  Default
        None: the truncation, the behaviour before the argument.
        fuzzy: (with device_text) an ``index_text.Fuzzy``, or None.  With one, a query token the vocabulary does not
        hold is replaced by the vocabulary terms nearest to it (GpuIndex.query_terms(fuzzy=): within 1 .. 2 edits,
        ranked by distance, then document frequency): ``_lexical``, the lexical and hybrid RPCs' lexical leg and
        ``query_terms_batch`` take that route; under ``lexical_and`` the best correction alone stands in for the
        token, else up to ``fuzzy.n_best``.  Without device_text it is refused by name.  Default None: a misspelt
        word is unknown, the behaviour before the argument."""
        check_fuzzy("GpuIndexClient", fuzzy)
        if fuzzy is not None and not device_text:
            raise ValueError("fuzzy= needs device_text=True: the corrections are sought behind the device tokenizer")
        self.fuzzy = fuzzy
        if diversify is not None:
            diversify = check_lam("GpuIndexClient", diversify)
            if getattr(index, "docs", None) is None:
                raise ValueError("GpuIndexClient(diversify=): the index has no dense rows (MMR takes its similarities "
                                 "from them)")
        self.diversify = diversify
        if graph_cascade and getattr(store, "entity_documents", None) is None:
            raise ValueError("graph_cascade=True needs the store's entity_documents column (rag_entities.document_id): "
                             "no entity row of this store carries a document_id")
        self.graph_cascade = bool(graph_cascade)
        if number_on_device and not device_text:
            raise ValueError("number_on_device=True needs device_text=True: the terms are numbered behind "
                             "the device tokenizer")
        self.number_on_device = bool(number_on_device)
        self.lexical_and = bool(lexical_and)
        self.image_index = image_index
        self.image_rows = None if image_rows is None else [int(r) for r in image_rows]
        if (image_index is None) != (image_rows is None):
            raise ValueError("image_index and image_rows come together")
        self.index = index
        self.store = store
        self.org_id = org_id
        self.token_embedder = token_embedder
        self.tokenizer = tokenizer or tokenize
        self.device_text = False
        self._pin: Dict[Any, list] = {}   # reusable pinned staging buffers (one query per call)
        self._plans: Dict[Any, Any] = {}  # (index, org, collection | sorted names) -> the one-query ScopePlan
        self._lazy = []                   # weak references to the deferred replies still unresolved
        self._pending_lex = self._by_text = self._tri = None
        # collection names -> ids; the filter itself runs on the device, before the ranking
        self._coll_id: Dict[str, int] = {}
        if collection_names is not None:
            self._coll_id = {c: i for i, c in enumerate(sorted(set(collection_names)))}
        if store.collections is not None:
            if collection_names is None:
                names = sorted({c for c in store.collections if c is not None})
                self._coll_id = {c: i for i, c in enumerate(names)}
            if index.doc_coll is None and self.sets_collections:
                index.set_collections(np.array([self._coll_id.get(c, -2) if c is not None else -2
                                                for c in store.collections], dtype=np.int32))
        # one client, many tenants: no org_id of its own over a store whose rows name theirs.  Every RPC
        # then ranks inside {"org": p_org_id} (GpuIndex scopes), the graph channel included.
        self.multi_tenant = org_id is None and getattr(store, "org_ids", None) is not None
        self._org_code: Dict[Any, int] = {}
        if self.multi_tenant:
            if "org" in index.attribute_names():
                # a column that came with the index (a saved one: ids given at inserts never move, so they
                # need not be the sorted order any more): the numbering is read off the rows, once
                for o, c in zip(store.org_ids, index.attribute("org").cpu().tolist()):
                    if c != (-1 if o is None else self._org_code.setdefault(o, c)):
                        raise ValueError("the index's \"org\" attribute does not follow the store's org_ids column")
                if len(set(self._org_code.values())) != len(self._org_code) or min(self._org_code.values(), default=0) < 0:
                    raise ValueError("the index's \"org\" attribute gives two orgs of the store the same id, or one none")
            else:
                self._org_code = {o: i for i, o in enumerate(sorted({o for o in store.org_ids if o is not None}))}
            for ix, rows in ((index, None), (image_index, self.image_rows)):
                if ix is not None and "org" not in ix.attribute_names():
                    orgs = store.org_ids if rows is None else [store.org_ids[r] for r in rows]
                    ix.set_attributes({"org": np.array([self._org_code.get(o, -1) for o in orgs], dtype=np.int32)})
        self.parent_rerank = bool(parent_rerank)
        self._parent_code: Dict[Any, int] = {}
        if self.parent_rerank:
            self._number_parents()
        if device_text:
            self._text_table()          # (refuses a custom tokenizer before anything is uploaded)
            self.device_text = True
            self._sync_vocabulary()

    # -------------------------------------------------------------- parents
    def _number_parents(self) -> None:
        """``_parent_code``: parent id -> parent number, kept the way ``_org_code`` is.  A column that came with the
        index (a saved one: numbers given at inserts never move) is read off the rows, once; else the store's
        parent_ids are numbered by first appearance and the column is set."""
        index, pids = self.index, list(self.store.parent_ids)
        if "parent" in index.attribute_names():
            for p, c in zip(pids, index.attribute("parent").cpu().tolist()):
                if c != (-1 if p is None else self._parent_code.setdefault(p, c)):
                    raise ValueError("the index's \"parent\" attribute does not follow the store's parent_ids column")
            if len(set(self._parent_code.values())) != len(self._parent_code) or \
                    min(self._parent_code.values(), default=0) < 0:
                raise ValueError("the index's \"parent\" attribute gives two parents of the store the same number, or one none")
        else:
            for p in pids:
                if p is not None:
                    self._parent_code.setdefault(p, len(self._parent_code))
            index.set_parents(self._parent_column(pids, self._parent_code))

    @staticmethod
    def _parent_column(parent_ids, code: Dict[Any, int]) -> np.ndarray:
        return np.array([-1 if p is None else code[p] for p in parent_ids], dtype=np.int32)

    # -------------------------------------------------------------- text on the device
    def _text_table(self) -> TextTable:
        """The analysis table of this client's tokenizer; a tokenizer that is no table is refused."""
        return tokenizer_table(self.tokenizer, "device_text=True")

    def _sync_vocabulary(self) -> None:
        """The index's device vocabulary is store.vocab's (built on first use, rebuilt when another writer
        grew the store's)."""
        idx, vocab = self.index, self.store.vocab
        table = self._text_table()
        X = idx.text
        if X is None or X["table"] is not table or len(X["ids"]) != len(vocab):
            terms = [None] * len(vocab)
            for tok, t in vocab.items():
                terms[t] = tok
            if any(t is None for t in terms):
                raise ValueError("device_text: store.vocab's ids are not 0 .. len - 1")
            idx.set_vocabulary(terms, table)

    def query_terms_batch(self, queries: Sequence[str]):
        """``_query_terms`` for a batch of query texts, on the device (GpuIndex.query_terms) -> the int32
        [nq, THR_BM25_MAX_TERMS] device table ``index.retrieve_batch(query_terms=)`` / ``bm25_search`` take;
        under ``lexical_and`` a query nothing can match is an all -1 row."""
        if not self.device_text:
            raise ValueError("query_terms_batch: the client was made without device_text=True")
        self._sync_vocabulary()
        if self.fuzzy is None:
            return self.index.query_terms(list(queries), conjunctive=self.lexical_and)[0]
        return self.index.query_terms(list(queries), conjunctive=self.lexical_and, fuzzy=self.fuzzy)[0]

    def _scope(self, org, collection=None, index=None):
        """Multi-tenant: the ScopePlan of a one-query call inside ``org`` (and ``collection``), made
        once per (org, collection) and kept until the index changes -- a request then resolves no
        scope and reads no row pointers back.  None: no row can match (a missing org, or one the
        store has never seen: what ``WHERE org_id = $1`` gives)."""
        code = self._org_code.get(org) if org is not None else None
        if code is None:
            return None
        index = self.index if index is None else index
        key = (id(index), org, collection)
        plan = self._plan(index, key)
        if plan is None:
            scope = {"org": code}
            if collection is not None and index.doc_coll is not None:
                scope["collection"] = self._coll_id.get(collection)     # (None: a name no row carries)
            plan = self._plans[key] = index.scope_plan([scope], 1)
        return plan

    def _plan(self, index, key):
        """The one-query ScopePlan kept under ``key``, or None: there is none, or the index changed since."""
        plan = self._plans.get(key)
        return plan if plan is not None and index.scope_plan_current(plan, 1) else None

    def _qcoll(self, collection):
        """int32 [1] collection id of a one-query call, None when unfiltered; a name no row
        carries gets an id no row carries (empty result, as the SQL WHERE would give)."""
        if collection is None or self.index.doc_coll is None:
            return None
        return torch.tensor([self._coll_id.get(collection, -3)], dtype=torch.int32, device=self.index.device)

    # ---------------------------------------------------------------- RPCs
    def rpc(self, name: str, params: Dict[str, Any]):
        if self.org_id is not None and params.get("p_org_id") not in (None, self.org_id):
            return _Reply([])  # data isolation: another tenant's index
        # multi-tenant: p_org_id is the scope of the call (otherwise it was checked above, and the
        # channel methods are called as they always were: subclasses override them)
        org = {"org": params.get("p_org_id")} if self.multi_tenant else {}
        if name == "rag2_semantic_search":
            return _Reply(self._semantic(params["p_embedding"], int(params.get("p_limit", 100)),
                                         params.get("p_collection"), **org))
        if name == "rag2_lexical_search":
            return _Reply(self._lexical(params["p_query"], int(params.get("p_limit", 50)),
                                        params.get("p_collection"), defer=bool(params.get("_defer")), **org))
        if name == "rag2_hybrid_rrf_search":
            return _Reply(self._hybrid_rrf(params, **org))
        if name == "kb_chunks_vector_search":   # legacy RAG 1.0 (20260113_halfvec_4000.sql:70-105)
            rows = self._semantic(params["p_embedding"], int(params.get("p_limit", 50)), None, **org)
            return _Reply([self._legacy_row(r, "similarity") for r in rows])
        if name == "kb_chunks_fts_pt":          # legacy RAG 1.0 (20260113_add_kb_chunks.sql:152-190)
            rows = self._lexical(params["p_query"], int(params.get("p_limit", 50)), None, **org)
            return _Reply([self._legacy_row(r, "rank") for r in rows])
        if name == "kb_chunks_image_search":    # legacy RAG 1.0 (20260113_add_kb_chunks.sql:236-268)
            return _Reply(self._image(params["p_image_embedding"], int(params.get("p_limit", 10)), **org))
        raise ValueError(f"unknown RPC {name!r}")

    def table(self, name: str) -> _TableQuery:
        if name not in TABLES:
            raise ValueError(f"table {name!r} is not served by the GPU index")
        return _TableQuery(self, TABLES[name])

    def _scoped(self, org, collection=None, index=None) -> Optional[dict]:
        """The filter arguments of a one-query search: ``collections=`` as always, or, multi-tenant,
        ``scopes=`` the cached plan of (org, collection); None = answer no rows."""
        if isinstance(collection, (list, tuple)):
            return self._scoped_union(org, collection, index)
        if not self.multi_tenant:
            return {} if index is not None else {"collections": self._qcoll(collection)}
        plan = self._scope(org, collection, index)
        return None if plan is None else {"scopes": plan}

    def _scoped_union(self, org, wanted, index=None) -> Optional[dict]:
        """``p_collection`` as a list of names: rank inside their UNION -- an ``In`` clause on
        "collection" (AND the org, multi-tenant) through the index's scopes, single-tenant clients
        included.  Names no row carries are dropped; none left = answer no rows (None).  The plan
        is kept per (org, sorted names) until the index changes, as _scope keeps its own."""
        index = self.index if index is None else index
        scope = {}
        if self.multi_tenant:
            code = self._org_code.get(org) if org is not None else None
            if code is None:
                return None
            scope["org"] = code
        if index.doc_coll is None:          # no collection column: the filter does nothing, as with one name
            return self._scoped(org, None, None if index is self.index else index)
        names = tuple(sorted({c for c in wanted if c in self._coll_id}))
        if not names:
            return None
        key = (id(index), org if self.multi_tenant else None, names)
        plan = self._plan(index, key)
        if plan is None:
            scope["collection"] = In([self._coll_id[c] for c in names])
            plan = self._plans[key] = index.scope_plan([scope], 1)
        return {"scopes": plan}

    def _image(self, embedding, limit: int, org=None) -> List[Dict[str, Any]]:
        """Cosine top-``limit`` over the image vectors (exact; the SQL orders by ``<=>``)."""
        if self.image_index is None:
            return []
        within = self._scoped(org, None, self.image_index)
        if within is None:
            return []
        q = torch.tensor([list(map(float, embedding))], dtype=torch.float32,
                         device=self.image_index.device)
        if q.shape[1] != self.image_index.dim:
            raise ValueError(f"image embedding has {q.shape[1]} dims, index has {self.image_index.dim}")
        k = min(N.THR_DENSE_MAX_K, limit)
        S, I, cnt, _ = self.image_index.dense_search(q, k, **within)
        out = []
        for j, sc in zip(I[0].tolist()[:int(cnt[0])], S[0].tolist()):
            row = self.store.result_row(self.image_rows[int(j) - self.image_index.doc_base])
            out.append({"id": row["child_id"], "content": row["text"], "modality": row["modality"],
                        "source_document": row["document_id"], "page": row["page"], "alt_text": None,
                        "image_path": None, "similarity": float(np.float32(sc))})   # ::REAL
        return out

    def _legacy_row(self, row: Dict[str, Any], score_key: str) -> Dict[str, Any]:
        i = self.store.row_index(row["child_id"])
        return {"id": row["child_id"], "content": row["text"], "modality": row["modality"],
                "source_document": row["document_id"], "page": row["page"], "chunk_index": i,
                "ocr_confidence": None, "is_table": row["modality"] == "table",
                "table_context": None, "alt_text": None, "category": None, "title": None,
                score_key: row[score_key]}

    def _hybrid_rrf(self, params: Dict[str, Any], **org) -> List[Dict[str, Any]]:
        """Server-side hybrid variant ``rag2_hybrid_rrf_search`` (rag2_schema.sql:413-496): lexical and semantic top
        ``p_limit*2`` each, FULL OUTER JOIN on the chunk id, ``w_l/(k+rank_l) + w_s/(k+rank_s)``, ORDER BY rrf_score
        DESC LIMIT p_limit -- one call, fused on the device by thr_rrf_fuse (ties, unspecified in SQL, follow the RRF
        kernel's sighting order).  ``org``: rpc()'s scope of the call, handed on to the two channels."""
        limit = int(params.get("p_limit", 50))
        coll = params.get("p_collection")
        wide = min(N.THR_RRF_MAX_PER_CHANNEL, 2 * limit)
        lex = self._lexical(params["p_query"], wide, coll, **org)
        sem = self._semantic(params["p_embedding"], wide, coll, **org)

        def ids(rows):
            t = torch.full((1, max(len(rows), 1)), -1, dtype=torch.int64, device=self.index.device)
            for j, r in enumerate(rows):
                t[0, j] = self.store.doc_base + self.store.row_index(r["child_id"])
            return t

        if not lex and not sem:
            return []
        out_ids, out_sc, out_rk, cnt = N.rrf_fuse(
            ids(lex), ids(sem), None, min(limit, 512), float(params.get("p_lexical_weight", 0.7)),
            float(params.get("p_semantic_weight", 0.8)), 1.0, int(params.get("p_rrf_k", 60)),
            want_ranks=True)
        rows = []
        for gid, sc, rk in zip(out_ids[0, : int(cnt[0])].tolist(), out_sc[0].tolist(), out_rk[0].tolist()):
            row = self.store.result_row(int(gid) - self.store.doc_base)
            row.update(rrf_score=float(np.float32(sc)), lexical_rank=rk[0] or None,
                       semantic_rank=rk[1] or None)
            rows.append(row)
        return rows

    # ---- one query per call: the host side is most of the latency, so every RPC does ONE pinned
    # upload and ONE read-back (scores and ids are the two halves of one [2, 1, k] tile) ----
    def _upload(self, values, dtype, device) -> torch.Tensor:
        """[1, n] device tensor of ``values`` through a reusable pinned buffer."""
        a = np.asarray(values, dtype=np.float32 if dtype == torch.float32 else np.int32).reshape(1, -1)
        key = (dtype, a.shape[1])
        slot = self._pin.get(key)
        if slot is None:
            slot = self._pin[key] = [torch.empty((1, a.shape[1]), dtype=dtype).pin_memory(), None]
        buf, ev = slot
        if ev is not None:
            ev.synchronize()            # the previous copy out of this buffer has left the host
        buf.numpy()[...] = a
        out = buf.to(device, non_blocking=True)
        if device.type == "cuda":
            slot[1] = torch.cuda.Event()
            slot[1].record()
        return out

    @staticmethod
    def _download(S: torch.Tensor, I: torch.Tensor):
        """(scores list, ids list without the -1 padding) in one device-to-host copy."""
        k = I.shape[1]
        if (S.dtype == torch.float64 and S.untyped_storage().data_ptr() == I.untyped_storage().data_ptr()
                and I.data_ptr() - S.data_ptr() == k * 8 and S.shape[0] == 1):
            both = torch.as_strided(S.view(torch.int64), (2, k), (k, 1)).cpu()
            scores, ids = both[0].view(torch.float64).tolist(), both[1].tolist()
        else:
            scores, ids = S[0].tolist(), I[0].tolist()
        n = 0
        while n < k and ids[n] >= 0:
            n += 1
        return scores[:n], ids[:n]

    def _rows(self, ids, scores, count, score_key, limit):
        """RPC result rows (the columns of rag2_schema.sql:350-358 / :386-394), best first."""
        st = self.store
        base, cid, pid, did = st.doc_base, st.child_ids, st.parent_ids, st.document_ids
        txt, pg, md = st.texts, st.pages, st.modalities
        out = []
        for gid, sc in zip(ids[:min(count, limit)], scores[:count]):
            i = gid - base
            out.append({"child_id": cid[i], "parent_id": pid[i], "document_id": did[i], "text": txt[i],
                        "page": pg[i], "modality": md[i], score_key: sc})
        return out

    def _semantic(self, embedding, limit: int, collection, org=None):
        if len(embedding) != self.index.dim:
            raise ValueError(f"embedding has {len(embedding)} dims, index has {self.index.dim}")
        within = self._scoped(org, collection)
        if within is None:
            return []
        q = self._upload(embedding, torch.float32, self.index.device)
        k = min(N.THR_DENSE_MAX_K, limit)
        S, I, _, _ = self.index.dense_search(q, k, sync=False, **within)
        scores, ids = self._download(S, I)
        return self._rows(ids, scores, len(ids), "similarity", limit)

    def _query_terms(self, query: str) -> Optional[List[int]]:
        """The distinct term ids of the query in order of first appearance (at most
        THR_BM25_MAX_TERMS), or None when nothing can match."""
        terms, _, flags = host_query_row(self.tokenizer(query), self.store.vocab)
        if not terms or getattr(self.index, "lex", True) is None:
            return None
        # AND semantics (plainto_tsquery, rag2_schema.sql:365): a token no chunk holds, or a term
        # the kernel's term list would have to drop, makes the conjunction unsatisfiable -- the
        # SQL returns no rows, so does this (the OR form just ignores what it does not know)
        if self.lexical_and and flags & (N.THR_TEXT_UNKNOWN | N.THR_TEXT_TOO_MANY):
            return None
        return terms

    def _lexical(self, query: str, limit: int, collection, defer: bool = False, org=None):
        """defer=True (``_defer`` in the RPC's params; RAG2Retriever sets it): the kernels are
        enqueued on the index's side stream and the rows are read back when first looked at --
        the retriever issues its semantic RPC in between, and the two channels overlap."""
        pending = self._pending_lex
        if pending is not None:     # a deferred call still owns the index's lexical workspace:
            self._pending_lex = None
            try:
                pending.materialize()   # read it back before the kernels of this one are enqueued
            except Exception:           # (its own caller sees that failure when it looks at the rows)
                pass
        if self.device_text and getattr(self.index, "lex", None) is not None:
            terms = None
        else:
            terms = self._query_terms(query)
            if terms is None:
                return []
        within = self._scoped(org, collection)
        if within is None:
            return []
        if terms is None:
            qt = self.query_terms_batch([query])    # (a query nothing can match: an all -1 row, no rows)
        else:
            # (fixed width: one pinned buffer, one workspace size, whatever the number of terms)
            qt = self._upload(terms + [-1] * (N.THR_BM25_MAX_TERMS - len(terms)), torch.int32, self.index.device)
        k = min(N.THR_TOPK_MAX, limit)
        if not defer or self.index.device.type != "cuda":
            S, I, _ = self.index.bm25_search(qt, k, conjunctive=self.lexical_and, **within)
            scores, ids = self._download(S, I)
            return self._rows(ids, scores, len(ids), "rank", limit)
        side = self.index.side_stream()
        main = torch.cuda.current_stream(self.index.device)
        side.wait_stream(main)              # the upload was enqueued on the main stream
        qc = within.get("collections")
        with torch.cuda.stream(side):
            S, I, _ = self.index.bm25_search(qt, k, conjunctive=self.lexical_and, **within)
        for t in (qt, qc):
            if t is not None:
                t.record_stream(side)

        def fetch():
            with torch.cuda.stream(side):   # the copy is ordered after the kernels on their stream
                scores, ids = self._download(S, I)
            return self._rows(ids, scores, len(ids), "rank", limit)
        self._pending_lex = LazyRows(fetch)
        self._track(self._pending_lex)
        return self._pending_lex

    # --------------------------------------------------------------- graph
    def _entity_index(self):
        if self._tri is None:
            self._tri = name_trigrams(self.store.entity_names)
        return self._tri

    def find_entities(self, keywords: List[str], limit: int = 20) -> List[int]:
        """Entity ids whose name contains a keyword (ILIKE '%kw%'): 5 keywords, limit // len(keywords) each, ascending."""
        if not keywords or not self.store.entity_names:
            return []
        return match_names(self._entity_index(), keywords, limit)

    def find_entities_batch(self, keyword_lists: Sequence[List[str]], limit: int = 20, device: bool = False):
        """``find_entities`` for a batch of queries, on the device (GpuIndex.find_entities: one thr_entity_match call
        for all of them) -> one list of entity ids per query, equal to ``[self.find_entities(k, limit) for k in
        keyword_lists]``.  device=True: the (seeds int32 [nq, 16], counts int32 [nq]) device tensors instead, for a
        caller that goes on to index.retrieve_batch(query_seeds=seeds).  The names are uploaded on first use from
        store.entity_names, as _entity_index() builds its index on first use; a query with a keyword too long for the
        kernel is resolved by ``find_entities``."""
        keyword_lists = [list(k) for k in keyword_lists]
        idx = self.index
        if not self.store.entity_names:
            if device:
                return (torch.full((len(keyword_lists), N.THR_GRAPH_MAX_SEEDS), -1, dtype=torch.int32, device=idx.device),
                        torch.zeros(len(keyword_lists), dtype=torch.int32, device=idx.device))
            return [[] for _ in keyword_lists]
        if idx.entities is None or idx.entities["n"] != len(self.store.entity_names):
            idx.set_entity_names(self.store.entity_names)
        seeds, counts = idx.find_entities(keyword_lists, limit, long_keywords=self.find_entities)
        if device:
            return seeds, counts
        rows, cnt = seeds.cpu().numpy(), counts.cpu().numpy()
        return [rows[q, :cnt[q]].tolist() for q in range(len(keyword_lists))]

    def entity_name(self, e: int) -> str:
        return self.store.entity_names[e]

    def graph_chunks(self, seeds: List[int], top_k: int, hops: int = 2, org_id=None) -> List[str]:
        """The chunk ids of the graph channel, best first.  A multi-tenant client scores ``org_id``'s chunks only
        (graph_search(scopes=): the reference filters by .eq("org_id", org_id), graph_search.py:154-230); the seeds
        come from ``find_entities``, which is global -- entity names carry no org, isolation is at the chunk."""
        within = {}
        if self.multi_tenant:
            plan = self._scope(org_id)
            if plan is None:
                return []
            within = {"scopes": plan}
        qs = self._upload(seeds + [-1] * (N.THR_GRAPH_MAX_SEEDS - len(seeds)), torch.int32, self.index.device)
        S, I, _ = self.index.graph_search(qs, min(N.THR_TOPK_MAX, top_k), hops, **within)
        _, ids = self._download(S, I)
        return [self.store.child_ids[int(g) - self.store.doc_base] for g in ids]

    # -------------------------------------------------------------- rerank
    def maxsim_scores(self, query: str, child_ids: List[str]) -> List[float]:
        """MaxSim of the query's token matrix against the given chunks, divided by the number of
        query tokens so unit-norm tokens give a [-1, 1] relevance like a cross-encoder's.  Under
        ``parent_rerank`` the chunk's parent passage is scored: the chunks of one parent get one score."""
        if self.token_embedder is None or self.index.tokens is None:
            raise RuntimeError("no token embedder / token store: late-interaction rerank unavailable")
        qtok = np.asarray(self.token_embedder.embed_query_tokens(query), dtype=np.float16)[None]
        ids = [self.store.row_index(c) for c in child_ids]
        cand = torch.tensor([[self.store.doc_base + i if i is not None else -1 for i in ids]],
                            dtype=torch.int64, device=self.index.device)
        sc = self.index.maxsim(torch.from_numpy(qtok).to(self.index.device), cand,
                               **({"expand": "parent"} if self.parent_rerank else {}))[0]
        return [float(v) / qtok.shape[1] if np.isfinite(v) else 0.5 for v in sc.tolist()]

    def mmr_order(self, child_ids: List[str], scores: List[float], top_k: int) -> List[int]:
        """The diversified cut of a ranked list: positions into ``child_ids`` / ``scores`` (relevance, best first), at
        most ``top_k`` of them, in the order MMR selects them under this client's ``diversify`` value.  An unknown
        child id goes in as -1: it stays selectable and is similar to nothing.  A score that is not finite is never
        selected."""
        if self.diversify is None:
            raise RuntimeError("this client was made without diversify=: no MMR order")
        n = len(child_ids)
        if n == 0 or top_k < 1:
            return []
        if len(scores) != n:
            raise ValueError("mmr_order: one score per child id")
        rows = [self.store.row_index(c) for c in child_ids]
        dev = self.index.device
        ids = torch.tensor([[self.store.doc_base + i if i is not None else -1 for i in rows]], dtype=torch.int64, device=dev)
        sc = torch.tensor([[float(s) for s in scores]], dtype=torch.float64, device=dev)
        _, _, cnt, pos, _ = self.index.diversify(ids, sc, None, top_k=min(int(top_k), n), lam=self.diversify)
        return pos[0, :int(cnt[0])].tolist()

    def text_to_child_id(self, text: str) -> Optional[str]:
        if self._by_text is None:
            self._by_text = {t: c for t, c in zip(self.store.texts, self.store.child_ids)}
            for row in self.store.parents.values():
                self._by_text.setdefault(row["text"], None)
        return self._by_text.get(text)


_default_client: Optional[GpuIndexClient] = None


def set_default_client(client: Optional[GpuIndexClient]) -> None:
    global _default_client
    _default_client = client


def get_supabase_client() -> GpuIndexClient:
    """What ``RAG2Retriever.supabase`` resolves to (reference: utils/db.py:372-400)."""
    if _default_client is None:
        raise RuntimeError("no GPU index registered: call backend.set_default_client(...)")
    return _default_client
