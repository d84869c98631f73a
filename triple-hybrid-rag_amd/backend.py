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

import collections.abc
import re
import weakref
from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native as N
from .index import GpuIndex
from .index_scope import In
from .index_text import NumberedRows, PendingVocabulary, TextTable, host_query_row, number_tokens, tokenizer_table

_TOKEN = re.compile(r"[\w]+", re.UNICODE)


def tokenize(text: str) -> List[str]:
    """Lower-cased word tokens (the reference leaves tokenisation to PostgreSQL's
    'portuguese' text-search configuration, which is not reproduced: no stemming)."""
    return _TOKEN.findall(text.lower())


@dataclass
class CorpusStore:
    child_ids: List[str]
    parent_ids: List[str]
    document_ids: List[str]
    texts: List[str]
    pages: List[int]
    modalities: List[str]
    parents: Dict[str, Dict[str, Any]] = field(default_factory=dict)  # id -> row
    collections: Optional[List[Optional[str]]] = None
    vocab: Dict[str, int] = field(default_factory=dict)               # term -> id
    entity_names: List[str] = field(default_factory=list)
    doc_base: int = 0
    content_hashes: Optional[List[Optional[str]]] = None            # the dedup key of the ingest (nullable)
    org_ids: Optional[List[Optional[str]]] = None                   # per-row tenant (rows' ``org_id``): one store, many orgs
    # rag_entities.id / .canonical_name, parallel to entity_names.  None (older saved indexes, synth):
    # the integer index is the id and the name the canonical name
    entity_ids: Optional[List[Any]] = None
    entity_canonical: Optional[List[Optional[str]]] = None

    def __post_init__(self):
        self._row_of = {cid: i for i, cid in enumerate(self.child_ids)}
        self._hashes = {h for h in (self.content_hashes or ()) if h is not None}
        self._ent_of: Optional[Dict[Any, int]] = None       # entity id -> index, built on first use
        self._canon_of: Optional[Dict[str, int]] = None     # canonical name -> first index

    # ---- entities (rag_entities): index e of the graph is row e of these columns
    def entity_index(self, entity_id: Any) -> Optional[int]:
        """Index of the entity with this id, or None.  Without an id column the integer index is the id."""
        if self.entity_ids is None:
            ok = isinstance(entity_id, (int, np.integer)) and not isinstance(entity_id, bool)
            return int(entity_id) if ok and 0 <= int(entity_id) < len(self.entity_names) else None
        if self._ent_of is None:
            self._ent_of = {}
            for i, e in enumerate(self.entity_ids):
                self._ent_of.setdefault(e, i)
                self._ent_of.setdefault(str(e), i)     # (a saved column comes back as strings)
        i = self._ent_of.get(entity_id)
        return self._ent_of.get(str(entity_id)) if i is None else i

    def entity_row(self, i: int) -> Dict[str, Any]:
        canon = None if self.entity_canonical is None else self.entity_canonical[i]
        return {"id": i if self.entity_ids is None else self.entity_ids[i], "name": self.entity_names[i],
                "canonical_name": self.entity_names[i] if canon is None else canon}

    def entity_by_canonical(self, canonical: str) -> Optional[int]:
        """Index of the first entity with this canonical name, or None."""
        if self._canon_of is None:
            self._canon_of = {}
            for i in range(len(self.entity_names)):
                self._canon_of.setdefault(self.entity_row(i)["canonical_name"], i)
        return self._canon_of.get(canonical)

    def check_new_entities(self, rows: Sequence[Dict[str, Any]]) -> None:
        """The unique constraint on rag_entities.id, before anything is changed."""
        seen = set()
        for r in rows:
            if self.entity_index(r["id"]) is not None or r["id"] in seen:
                raise ValueError(f"duplicate key value violates unique constraint on rag_entities (id {r['id']!r})")
            seen.add(r["id"])

    def append_entities(self, rows: Sequence[Dict[str, Any]]) -> range:
        """Append rag_entities rows (id, name, canonical_name) -> the range of their indices.  The id
        and canonical-name columns come into being here, the old entities keeping their defaults."""
        rows = list(rows)
        self.check_new_entities(rows)
        n0 = len(self.entity_names)
        if not rows:
            return range(n0, n0)
        for name in ("entity_names", "entity_ids", "entity_canonical"):
            if getattr(self, name) is not None and not isinstance(getattr(self, name), list):
                setattr(self, name, list(getattr(self, name)))
        if self.entity_ids is None:
            self.entity_ids = list(range(n0))
        if self.entity_canonical is None:
            self.entity_canonical = [None] * n0
        for r in rows:
            self.entity_ids.append(r["id"])
            self.entity_names.append(r.get("name") or "")
            self.entity_canonical.append(r.get("canonical_name"))
        self._ent_of = self._canon_of = None
        return range(n0, n0 + len(rows))

    def has_hash(self, content_hash: Optional[str]) -> bool:
        return content_hash is not None and content_hash in self._hashes

    def append(self, rows: Sequence[Dict[str, Any]], tokenizer=None) -> range:
        """Append child-chunk rows (the columns ``index_build.from_rows`` reads, plus the
        optional ``content_hash``) -> the range of their row indices.  ``page`` is nullable, as
        the SQL column is.  A row whose id or content hash the store already holds -- or that
        repeats one inside the batch -- raises before anything is changed (the message names
        the ``duplicate``: what the reference's ingest catches, ingest.py:457-460).
        ``tokenizer``: unseen terms of the rows' texts get the next vocabulary ids, at the END,
        so existing term ids never move."""
        rows = list(rows)
        ids, hashes = set(), set()
        for r in rows:
            if r["id"] in self._row_of or r["id"] in ids:
                raise ValueError(f"duplicate key value violates unique constraint: id {r['id']!r}")
            h = r.get("content_hash")
            if h is not None and (h in self._hashes or h in hashes):
                raise ValueError(f"duplicate key value violates unique constraint: content_hash {h!r}")
            ids.add(r["id"])
            hashes.add(h)
        n0 = len(self.child_ids)
        # (a loaded store keeps its columns as read-only blobs: they become lists on the first append)
        for name in ("child_ids", "parent_ids", "document_ids", "texts", "pages", "modalities"):
            if not isinstance(getattr(self, name), list):
                setattr(self, name, list(getattr(self, name)))
        if self.collections is None and any(r.get("collection") is not None for r in rows):
            raise ValueError("the store has no collection column: rows cannot carry a collection")
        if self.collections is not None and not isinstance(self.collections, list):
            self.collections = list(self.collections)
        # (a store without the column ignores the rows' org_id: the single-tenant ingest sends it too)
        if self.org_ids is not None and not isinstance(self.org_ids, list):
            self.org_ids = list(self.org_ids)
        if self.content_hashes is None:
            self.content_hashes = [None] * n0
        elif not isinstance(self.content_hashes, list):
            self.content_hashes = list(self.content_hashes)
        for i, r in enumerate(rows):
            self.child_ids.append(r["id"])
            self.parent_ids.append(r.get("parent_id"))
            self.document_ids.append(r.get("document_id"))
            self.texts.append(r.get("text", ""))
            self.pages.append(r.get("page", 1))
            self.modalities.append(r.get("modality", "text"))
            if self.collections is not None:
                self.collections.append(r.get("collection"))
            if self.org_ids is not None:
                self.org_ids.append(r.get("org_id"))
            self.content_hashes.append(r.get("content_hash"))
            self._row_of[r["id"]] = n0 + i
        if tokenizer is not None:
            v0 = len(self.vocab)
            new_terms = number_tokens((tokenizer(r.get("text", "")) for r in rows), self.vocab)[2]
            self.vocab.update((tok, v0 + i) for i, tok in enumerate(new_terms))
        self._hashes.update(h for h in hashes if h is not None)
        return range(n0, n0 + len(rows))

    def delete(self, rows: Sequence[int]) -> List[Dict[str, Any]]:
        """Remove the child-chunk rows with these row indices (any order, repeats allowed) -> the
        deleted rows as ``child_row`` gives them, in row order.  Every column is compacted (the
        survivors keep their order: row i becomes row i - #deleted below i, as
        ``GpuIndex.delete_rows`` renumbers the index), the id lookup is rebuilt and the rows'
        content hashes are forgotten, so the same content can be ingested again.  Parents, the
        vocabulary and the entity names are not touched (term and entity ids never move)."""
        n = len(self.child_ids)
        gone = sorted({int(r) for r in rows})
        if gone and (gone[0] < 0 or gone[-1] >= n):
            raise ValueError(f"row index out of range 0 .. {n - 1}")
        if not gone:
            return []
        out = [self.child_row(i) for i in gone]
        dead = set(gone)
        # (a loaded store keeps its columns as read-only blobs: they become lists here, as in append)
        names = ["child_ids", "parent_ids", "document_ids", "texts", "pages", "modalities"]
        names += [c for c in ("collections", "content_hashes", "org_ids") if getattr(self, c) is not None]
        lost = {self.content_hashes[i] for i in gone} if self.content_hashes is not None else set()
        for name in names:
            col = getattr(self, name)
            setattr(self, name, [col[i] for i in range(n) if i not in dead])
        self._row_of = {cid: i for i, cid in enumerate(self.child_ids)}
        self._hashes -= {h for h in lost if h is not None}
        return out

    def row_index(self, child_id: str) -> Optional[int]:
        return self._row_of.get(child_id)

    def child_row(self, i: int) -> Dict[str, Any]:
        return {"id": self.child_ids[i], "parent_id": self.parent_ids[i],
                "document_id": self.document_ids[i], "text": self.texts[i],
                "page": self.pages[i], "modality": self.modalities[i]}

    def result_row(self, i: int) -> Dict[str, Any]:
        row = self.child_row(i)
        row["child_id"] = row.pop("id")
        return row

    @classmethod
    def synthetic(cls, n: int, doc_base: int = 0, children_per_parent: int = 4,
                  vocab_size: int = 0, n_entities: int = 0) -> "CorpusStore":
        """Row payloads for a synthetic corpus: ids derive from the global doc index."""
        g = [doc_base + i for i in range(n)]
        parents = {f"p{j}": {"id": f"p{j}", "text": f"parent text {j}",
                             "section_heading": f"Section {j}"}
                   for j in sorted({x // children_per_parent for x in g})}
        return cls(child_ids=[f"c{x}" for x in g],
                   parent_ids=[f"p{x // children_per_parent}" for x in g],
                   document_ids=[f"d{x // 64}" for x in g], texts=[f"chunk {x}" for x in g],
                   pages=[x % 9 + 1 for x in g], modalities=["text"] * n, parents=parents,
                   vocab={f"t{t}": t for t in range(vocab_size)},
                   entity_names=[f"entity{e}" for e in range(n_entities)], doc_base=doc_base)


class _Reply:
    def __init__(self, data):
        self.data = data

    def execute(self):
        return self


class LazyRows(collections.abc.Sequence):
    """Rows of an RPC whose kernels are in flight: the read-back happens when the rows are first
    looked at, so the caller can issue its next RPC in the meantime.  A failure of the deferred
    part (the read-back is where an asynchronous HIP error of the lexical kernels surfaces) RAISES
    at that first look and again on every later one -- the reference's ``_lexical_search`` has no
    try/except either (retrieval.py:273-292: only the graph channel swallows errors), so a failing
    lexical RPC propagates out of ``retrieve()``; a GPU fault never becomes an empty channel.
    Not a ``list`` subclass: every consumer goes through the Sequence protocol, so nothing can
    read an unfilled list storage behind the fetch (``json.dumps(rows.materialize())`` for C-level
    consumers that insist on a real list)."""

    __slots__ = ("_fetch", "_rows", "_error", "__weakref__")

    def __init__(self, fetch):
        self._fetch = fetch
        self._rows = None
        self._error = None

    def materialize(self) -> list:
        """The rows as a plain list (fetched once; a failed fetch re-raises its exception)."""
        if self._error is not None:
            raise self._error
        if self._rows is None:
            fetch, self._fetch = self._fetch, None
            try:
                self._rows = list(fetch())
            except BaseException as exc:
                self._error = exc
                raise
        return self._rows

    _ready = materialize

    def __iter__(self):
        return iter(self.materialize())

    def __len__(self):
        return len(self.materialize())

    def __getitem__(self, i):
        return self.materialize()[i]

    def __eq__(self, other):
        if isinstance(other, LazyRows):
            other = other.materialize()
        return self.materialize() == other

    def __add__(self, other):
        return self.materialize() + list(other)

    def __radd__(self, other):
        return list(other) + self.materialize()

    def __repr__(self):
        return f"LazyRows({'pending' if self._rows is None and self._error is None else self._rows!r})"

    __hash__ = None


class _TableQuery:
    def __init__(self, fetch, by_hash=None, insert=None, org_id=None, delete=None, tenants=False, by_eq=None):
        self._fetch = fetch
        self._by_hash = by_hash       # content_hash lookup (rag_child_chunks only)
        self._by_eq = by_eq           # equality lookup {column: value} -> rows (rag_entities.canonical_name)
        self._eqs: Dict[str, Any] = {}
        self._insert = insert         # row writer (the two chunk tables)
        self._delete = delete         # row remover: [(column, values), ...] -> the deleted rows
        self._filters: Optional[List[Any]] = None   # delete(): the filters so far (AND)
        self._org_id = org_id
        self._ids: Optional[List[Any]] = None
        self._hashes: Optional[List[Any]] = None
        self._rows: Optional[List[Dict[str, Any]]] = None
        self._limit: Optional[int] = None
        self._foreign = False         # eq("org_id", another tenant): nothing of this index matches
        self._tenants = tenants       # a multi-tenant client: eq("org_id", x) is a row filter like any other
        self._org_eq: Optional[List[Any]] = None

    def select(self, *_cols, **_kw):
        return self

    def eq(self, *a, **_kw):
        if len(a) == 2 and a[0] == "org_id" and self._org_id is not None and a[1] not in (None, self._org_id):
            self._foreign = True
        if self._by_eq is not None and len(a) == 2 and a[0] != "org_id":
            self._eqs[a[0]] = a[1]
        if self._tenants and len(a) == 2 and a[0] == "org_id":
            self._org_eq = [a[1]]
            if self._filters is not None:
                self._filters.append(("org_id", [a[1]]))
            return self
        if self._filters is not None and len(a) == 2 and a[0] != "org_id":
            self._filters.append((a[0], [a[1]]))
        return self

    def delete(self):
        """``table(t).delete().eq(col, v)`` / ``.in_(col, vs)`` ... ``.execute().data`` = the deleted
        rows of the table addressed; several filters combine with AND.  A delete without a filter
        other than ``org_id`` is refused at execute() (PostgREST refuses it too, and it would
        empty the index)."""
        if self._delete is None:
            raise ValueError("this table is read-only in the GPU index")
        self._filters = [] if self._org_eq is None else [("org_id", list(self._org_eq))]
        return self

    def insert(self, rows):
        if self._insert is None:
            raise ValueError("this table is read-only in the GPU index")
        self._rows = [rows] if isinstance(rows, dict) else list(rows)
        return self

    def limit(self, n: int):
        self._limit = n
        return self

    def in_(self, column: str, values: Sequence[Any]):
        if self._filters is not None:
            self._filters.append((column, list(values)))
            return self
        if column == "content_hash" and self._by_hash is not None:
            self._hashes = list(values)
            return self
        if column != "id":
            raise ValueError("only id (and rag_child_chunks.content_hash) lookups are served from the GPU index store")
        self._ids = list(values)
        return self

    def execute(self):
        if self._filters is not None:
            if not self._filters:
                raise ValueError("DELETE requires a WHERE clause: a delete without a filter other than org_id is refused")
            return _Reply([] if self._foreign else self._delete(self._filters))
        if self._rows is not None:
            return _Reply(self._insert(self._rows))
        org = {} if self._org_eq is None else {"org": self._org_eq[0]}
        if self._hashes is not None:
            rows = [] if self._foreign else self._by_hash(self._hashes, **org)
        elif self._by_eq is not None and self._ids is None:
            rows = [] if self._foreign else self._by_eq(dict(self._eqs), **org)
        else:
            rows = self._fetch(self._ids or [], **org)
        return _Reply(rows[: self._limit] if self._limit is not None else rows)


class GpuIndexClient:
    """Supabase-shaped facade over (GpuIndex, CorpusStore)."""

    defers_readback = True   # rag2_lexical_search honours ``_defer`` (see _lexical)
    sets_collections = True  # derives the index's per-doc collection ids from the store's rows
    multi_tenant = False     # set by __init__: no org_id of its own over a store with an org_ids column

    def __init__(self, index: GpuIndex, store: CorpusStore, org_id: Optional[str] = None,
                 token_embedder: Any = None, lexical_and: bool = False,
                 image_index: Optional[GpuIndex] = None, image_rows: Any = None,
                 collection_names: Optional[Sequence[str]] = None, device_text: bool = False,
                 tokenizer: Any = None, number_on_device: bool = False):
        """lexical_and: rank only chunks holding EVERY query term, as the reference's
        ``plainto_tsquery`` does (rag2_schema.sql:365); default is BM25's OR form, the
        north star's and the oracle's.
        image_index / image_rows: the legacy image channel (``kb_chunks_image_search``,
        20260113_add_kb_chunks.sql:236-268): a second dense index over the ``vector_image`` of the
        chunks that have one (``vector_image IS NOT NULL``), row j of it being store row
        ``image_rows[j]``.
        collection_names: fixes the collection name -> id mapping (sorted names of the WHOLE
        corpus): the shards of a document-sharded index must agree on it (sharded_client.py);
        default: the names this store's rows carry.
        org_id: the one tenant this client serves -- any other ``p_org_id`` is answered with no rows.
        None over a store that has an ``org_ids`` column makes the client MULTI-TENANT: one index,
        one store, every tenant.  The index gets an ``"org"`` attribute column (the ids of the sorted
        distinct names; one it already has is checked against the store's column), each RPC and
        ``graph_chunks`` rank inside {"org": p_org_id} (+ "collection") through the index's scopes,
        a missing or unknown org gets no rows, ``table().eq("org_id", x)`` filters rows, and an
        insert needs ``org_id`` on every row.
        tokenizer: what the index's vocabulary was built with (default ``tokenize``, from_rows' default).
        device_text: query and chunk text become term ids on the device (GpuIndex.set_vocabulary from
        ``store.vocab`` -- derived state, rebuilt here, never saved): ``_lexical`` and ``insert_children``
        take that route and ``query_terms_batch`` serves batches.  Needs ``tokenize`` or a TextTable's
        ``.tokenize`` as the tokenizer; any other is refused by name.
        number_on_device: (with device_text) ``insert_children`` also numbers the batch's new terms on the
        device (GpuIndex.number_text_rows / commit_vocabulary): the unknown tokens are not decoded one
        occurrence at a time, the new keys stay on the device, and the store's vocabulary gets one string per
        distinct new term.  The ids are the host loop's.  Without device_text it is refused by name."""
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
        self._plans: Dict[Any, Any] = {}    # (index, org, collection) -> the one-query ScopePlan
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
        if device_text:
            self._text_table()          # (refuses a custom tokenizer before anything is uploaded)
            self.device_text = True
            self._sync_vocabulary()

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
        return self.index.query_terms(list(queries), conjunctive=self.lexical_and)[0]

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
        plan = self._plans.get(key)
        if plan is None or not index.scope_plan_current(plan, 1):
            scope = {"org": code}
            if collection is not None and index.doc_coll is not None:
                scope["collection"] = self._coll_id.get(collection)     # (None: a name no row carries)
            plan = self._plans[key] = index.scope_plan([scope], 1)
        return plan

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
            return _Reply(self._hybrid_rrf(params))
        if name == "kb_chunks_vector_search":   # legacy RAG 1.0 (20260113_halfvec_4000.sql:70-105)
            rows = self._semantic(params["p_embedding"], int(params.get("p_limit", 50)), None, **org)
            return _Reply([self._legacy_row(r, "similarity") for r in rows])
        if name == "kb_chunks_fts_pt":          # legacy RAG 1.0 (20260113_add_kb_chunks.sql:152-190)
            rows = self._lexical(params["p_query"], int(params.get("p_limit", 50)), None, **org)
            return _Reply([self._legacy_row(r, "rank") for r in rows])
        if name == "kb_chunks_image_search":    # legacy RAG 1.0 (20260113_add_kb_chunks.sql:236-268)
            return _Reply(self._image(params["p_image_embedding"], int(params.get("p_limit", 10)), **org))
        raise ValueError(f"unknown RPC {name!r}")

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
        plan = self._plans.get(key)
        if plan is None or not index.scope_plan_current(plan, 1):
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

    def _hybrid_rrf(self, params: Dict[str, Any]) -> List[Dict[str, Any]]:
        """Server-side hybrid variant ``rag2_hybrid_rrf_search`` (rag2_schema.sql:413-496):
        lexical and semantic top ``p_limit*2`` each, FULL OUTER JOIN on the chunk id,
        ``w_l/(k+rank_l) + w_s/(k+rank_s)``, ORDER BY rrf_score DESC LIMIT p_limit -- one call,
        fused on the device by thr_rrf_fuse (ties, unspecified in SQL, follow the RRF kernel's
        sighting order)."""
        limit = int(params.get("p_limit", 50))
        coll = params.get("p_collection")
        wide = min(N.THR_RRF_MAX_PER_CHANNEL, 2 * limit)
        org = {"org": params.get("p_org_id")} if self.multi_tenant else {}
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
        terms, _, flags = host_query_row(tokenize(query), self.store.vocab)
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
        pending = getattr(self, "_pending_lex", None)
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

    def _track(self, lazy: LazyRows) -> None:
        """Deferred replies hold LOCAL doc ids: a delete materialises the unresolved ones before
        the ids shift (weak references: a reply nobody holds any more is not kept alive)."""
        alive = [r for r in getattr(self, "_lazy", ()) if r() is not None and r()._fetch is not None]
        self._lazy = alive + [weakref.ref(lazy)]      # (LazyRows compares by value: no hash, no WeakSet)

    # -------------------------------------------------------------- ingest
    def _check_org(self, rows: Sequence[Dict[str, Any]]) -> None:
        if self.multi_tenant and any(r.get("org_id") is None for r in rows):
            raise ValueError("insert refused: this client serves several tenants, every row needs its org_id")
        if self.org_id is not None and any(r.get("org_id") not in (None, self.org_id) for r in rows):
            raise ValueError("insert refused: the rows belong to another org_id than this index "
                             "(data isolation, as rpc() answers another tenant with no rows)")

    def _number_texts(self, texts: Sequence[str]) -> NumberedRows:
        """The token rows of a batch of chunk texts, new terms numbered, on the route the client was made
        with: ``self.tokenizer`` and ``number_tokens`` (host arrays, the new terms as strings), or under
        device_text the index's ``number_text_rows`` (device tensors; with number_on_device the new keys
        stay there).  Nothing is committed: neither vocabulary has changed when this returns."""
        if self.device_text:
            self._sync_vocabulary()
            if self.number_on_device:
                return self.index.number_text_rows(texts)
            return self.index.number_text_rows(texts, on_device=False)
        n_before = len(self.store.vocab)
        doc, term, new_terms = number_tokens(map(self.tokenizer, texts), self.store.vocab)
        return NumberedRows(doc, term, n_before, PendingVocabulary(n_before, len(new_terms), terms=new_terms))

    def insert_children(self, rows: Sequence[Dict[str, Any]], embedding_key: str = "embedding_1024"):
        """``table("rag_child_chunks").insert(rows)``: one append of len(rows) chunks to the store
        and to the live index -> [{"id": ...}, ...].  A row is stored as ``index_build.from_rows``
        stores it (float32 embedding; no embedding = a zero vector, outside the dense channel; the
        text tokenised with ``self.tokenizer``), so a bulk build and an insert hold the same
        floats.  Everything is checked first (org, duplicate ids / content hashes, what the
        index's channels need); the index is appended to before the store, so a refused append
        leaves both as they were."""
        rows = list(rows)
        self._check_org(rows)
        if not rows:
            return []
        st, idx = self.store, self.index
        seen_id, seen_h = set(), set()
        for r in rows:
            h = r.get("content_hash")
            if st.row_index(r["id"]) is not None or r["id"] in seen_id or st.has_hash(h) or (h is not None and h in seen_h):
                raise ValueError("duplicate key value violates unique constraint on rag_child_chunks "
                                 f"(id {r['id']!r}, content_hash {h!r})")
            seen_id.add(r["id"])
            seen_h.add(h)
        m = len(rows)
        parts: Dict[str, Any] = {}
        if idx.docs is not None:
            docs = np.zeros((m, idx.dim), dtype=np.float32)
            for i, r in enumerate(rows):
                if r.get(embedding_key) is not None:
                    if len(r[embedding_key]) != idx.dim:
                        raise ValueError(f"embedding has {len(r[embedding_key])} dims, index has {idx.dim}")
                    docs[i] = np.asarray(r[embedding_key], dtype=np.float32)
            parts["docs"] = docs
        else:
            parts.update(docs=None, n_rows=m)
        numbered = None
        if getattr(idx, "lex", None) is not None:
            # term ids of the vocabulary; unseen terms get the next ids (committed to the device vocabulary
            # and to the store only after the index took the rows)
            numbered = self._number_texts([r.get("text", "") for r in rows])
            parts["lex"] = (numbered.doc, numbered.term, None, max(numbered.n_before + numbered.pending.n_new, 1))
        if idx.doc_coll is not None:
            for r in rows:   # a collection no earlier row carries gets the next id (ids never move)
                c = r.get("collection")
                if c is not None and c not in self._coll_id:
                    self._coll_id[c] = max(self._coll_id.values(), default=-1) + 1
            parts["collections"] = np.array([self._coll_id[r["collection"]] if r.get("collection") is not None
                                             else -2 for r in rows], dtype=np.int32)
        if self.multi_tenant:
            org_code = dict(self._org_code)
            for r in rows:   # an org no earlier row carries gets the next id (ids never move)
                org_code.setdefault(r["org_id"], max(org_code.values(), default=-1) + 1)
            parts["attributes"] = {"org": np.array([org_code[r["org_id"]] for r in rows], dtype=np.int32)}
        if idx.tokens is not None:
            if any(r.get("tokens") is None for r in rows):
                raise ValueError("the index has a late-interaction token store: every inserted row needs its "
                                 "'tokens' matrix [d_tokens, tok_dim]")
            parts["tokens"] = np.stack([np.asarray(r["tokens"], dtype=np.float16) for r in rows])
        if idx.graph is not None:
            me, mc, mw = [], [], []
            for i, r in enumerate(rows):   # optional per-row mentions: [(entity index, confidence), ...]
                for e, w in r.get("mentions", ()):
                    me.append(int(e))
                    mc.append(i)
                    mw.append(float(w))
            parts["mentions"] = (np.asarray(me, dtype=np.int64), np.asarray(mc, dtype=np.int64),
                                 np.asarray(mw, dtype=np.float32))
        idx.append_rows(**parts)
        # index, device vocabulary, store rows, store vocabulary: in that order
        if numbered is not None and self.device_text:
            idx.commit_vocabulary(numbered.pending)
        st.append(rows)
        if numbered is not None:
            st.vocab.update((tok, numbered.n_before + i) for i, tok in enumerate(numbered.pending.terms))
        if self.multi_tenant:
            self._org_code = org_code
            self._settle_deferred()   # (a deferred search may still read the plans' labels)
            self._plans.clear()       # (resolved over the old rows)
        if hasattr(self, "_by_text"):
            del self._by_text
        return [{"id": r["id"]} for r in rows]

    def insert_parents(self, rows: Sequence[Dict[str, Any]]):
        rows = list(rows)
        self._check_org(rows)
        for p in rows:
            if p["id"] in self.store.parents:
                raise ValueError(f"duplicate key value violates unique constraint on rag_parent_chunks (id {p['id']!r})")
        for p in rows:
            self.store.parents[p["id"]] = {"id": p["id"], "text": p.get("text", ""),
                                           "section_heading": p.get("section_heading")}
        if hasattr(self, "_by_text"):
            del self._by_text
        return [{"id": p["id"]} for p in rows]

    # -------------------------------------------------------------- graph ingest
    # What the reference's entity extraction writes behind a document's chunk inserts
    # (rag2/entity_extraction.py:449-554): rag_entities upserts, rag_relations and rag_entity_mentions
    # inserts.  Index first, store second, as insert_children: a refused call leaves both as they were.
    def _check_foreign_org(self, rows: Sequence[Dict[str, Any]]) -> None:
        """rag_entity_mentions rows carry no org_id in the reference (a mention's tenant is its
        chunk's): only rows that name ANOTHER org than this client's are refused."""
        if self.org_id is not None and any(r.get("org_id") not in (None, self.org_id) for r in rows):
            raise ValueError("insert refused: the rows belong to another org_id than this index "
                             "(data isolation, as rpc() answers another tenant with no rows)")

    def insert_entities(self, rows: Sequence[Dict[str, Any]]):
        """``table("rag_entities").insert(rows)``: the entities get the next entity ids of the live
        index (``GpuIndex.append_graph``), their lower-cased names join the device name store, and
        the rows (id, name, canonical_name) the store -> [{"id": ...}, ...].  A duplicate id is the
        unique-constraint ValueError, raised before anything is changed."""
        rows = list(rows)
        self._check_org(rows)
        if not rows:
            return []
        st, idx = self.store, self.index
        st.check_new_entities(rows)
        names = [r.get("name") or "" for r in rows]
        if idx.entities is None and len(st.entity_names) > 0:
            # the names of this store were not uploaded yet (find_entities_batch does it on first use,
            # from all of store.entity_names): only the rows grow now
            idx.append_graph(n_new_entities=len(rows))
        else:
            idx.append_graph(entity_names=names)
        st.append_entities(rows)
        self._tri = None       # (the trigram index of find_entities is over the old names)
        return [{"id": r["id"]} for r in rows]

    def insert_relations(self, rows: Sequence[Dict[str, Any]]):
        """``table("rag_relations").insert(rows)``: subject_entity_id / object_entity_id become entity
        indices; a row naming an unknown entity is skipped, as ``index_build.build_graph`` skips it;
        the rest go through ``GpuIndex.append_graph(relations=)`` (both directions, self-loops and
        edges the index already holds dropped).  Relation types and confidences are not stored: the
        walk does not read them."""
        rows = list(rows)
        self._check_org(rows)
        st = self.store
        pairs = [(st.entity_index(r.get("subject_entity_id")), st.entity_index(r.get("object_entity_id"))) for r in rows]
        pairs = [(a, b) for a, b in pairs if a is not None and b is not None]
        if pairs:
            self.index.append_graph(relations=(np.asarray([a for a, _ in pairs], dtype=np.int64),
                                               np.asarray([b for _, b in pairs], dtype=np.int64)))
            self._tri = None
        return [{"id": r.get("id")} for r in rows]

    def insert_mentions(self, rows: Sequence[Dict[str, Any]]):
        """``table("rag_entity_mentions").insert(rows)``: entity_id / child_chunk_id become an entity
        index and a chunk of the live index; a row naming an unknown entity or chunk is skipped, as
        ``build_graph`` skips it; ``confidence`` defaults to 1.0; the rest go through
        ``GpuIndex.append_mentions``."""
        rows = list(rows)
        self._check_foreign_org(rows)
        st = self.store
        me, mc, mw = [], [], []
        for r in rows:
            e, c = st.entity_index(r.get("entity_id")), st.row_index(r.get("child_chunk_id"))
            if e is None or c is None:
                continue
            me.append(e)
            mc.append(c)
            mw.append(1.0 if r.get("confidence") is None else float(r["confidence"]))
        if me:
            self.index.append_mentions(np.asarray(me, dtype=np.int64), np.asarray(mc, dtype=np.int64),
                                       np.asarray(mw, dtype=np.float32))
            self._tri = None
        return [{"id": r.get("id")} for r in rows]

    # -------------------------------------------------------------- delete
    def _child_rows_where(self, filters, columns=("id", "document_id", "parent_id")) -> List[int]:
        """Row indices of the child chunks that match every (column, values) filter; a multi-tenant
        client also takes ``org_id`` (the store's per-row column)."""
        st = self.store
        rows: Optional[set] = None
        for column, values in filters:
            if column == "org_id" and self.multi_tenant:
                want = set(values)
                hit = {i for i, v in enumerate(st.org_ids) if v in want}
                rows = hit if rows is None else rows & hit
                continue
            if column not in columns:
                raise ValueError(f"delete: rag_child_chunks rows are addressed by {' / '.join(columns)}, not {column!r}")
            if column == "id":
                hit = {i for i in (st.row_index(v) for v in values) if i is not None}
            else:
                want = set(values)
                col = st.document_ids if column == "document_id" else st.parent_ids
                hit = {i for i, v in enumerate(col) if v in want}
            rows = hit if rows is None else rows & hit
        return sorted(rows or ())

    def _settle_deferred(self) -> None:
        """Read back every deferred reply that is still unresolved: before a delete shifts the local
        ids they hold, and before the cached scope plans are dropped (a deferred lexical search may
        still be reading a plan's labels on the side stream)."""
        self._pending_lex = None
        for ref in getattr(self, "_lazy", ()):
            lazy = ref()
            if lazy is not None:
                try:
                    lazy.materialize()
                except Exception:   # (its own caller sees that failure when it looks at the rows)
                    pass
        self._lazy = []

    def _delete_rows(self, rows: List[int]) -> List[Dict[str, Any]]:
        """Remove store rows ``rows`` (sorted, distinct) from the index, then from the store."""
        if not rows:
            return []
        # a deferred reply issued before the delete holds local ids that are about to shift
        self._settle_deferred()
        images = None
        if self.image_index is not None:
            dead = set(rows)
            images = [j for j, r in enumerate(self.image_rows) if r in dead]
            if images and len(images) >= len(self.image_rows):
                raise N.NativeError("delete refused: every row of the image index would be deleted: build a new index")
        self.index.delete_rows(np.asarray(rows, dtype=np.int64))       # index first: a refusal leaves both untouched
        deleted = self.store.delete(rows)
        if self.multi_tenant:
            self._plans.clear()       # (resolved over the old rows)
        if self.image_index is not None:
            if images:
                self.image_index.delete_rows(np.asarray(images, dtype=np.int64))
            gone = np.asarray(rows, dtype=np.int64)
            self.image_rows = [int(r - np.searchsorted(gone, r)) for r in self.image_rows if r not in dead]
        if hasattr(self, "_by_text"):
            del self._by_text
        return deleted

    def delete_children(self, ids: Sequence[Any]) -> List[Dict[str, Any]]:
        """``table("rag_child_chunks").delete().in_("id", ids)``: the chunks leave the live index
        (``GpuIndex.delete_rows``) and then the store -> the deleted rows.  Unknown ids delete
        nothing and are not an error.  Unresolved deferred replies (``LazyRows``) are read back
        first; the index is changed before the store, so a refused delete (every row of the
        index) leaves both as they were."""
        return self._delete_rows(self._child_rows_where([("id", list(ids))]))

    def _delete_children_where(self, filters) -> List[Dict[str, Any]]:
        return self._delete_rows(self._child_rows_where(filters))

    def _delete_parents_where(self, filters) -> List[Dict[str, Any]]:
        """Parent rows by ``id`` / ``document_id`` (a parent belongs to one document: the one its
        children name) -> the deleted parent rows; their children go with them (schema :106).
        Multi-tenant, ``org_id`` restricts the delete to that org's chunks: a parent that other
        orgs' chunks still name loses the org's children and stays."""
        st = self.store
        pids: Optional[set] = None
        orgs: Optional[set] = None
        for column, values in filters:
            if column == "org_id" and self.multi_tenant:
                orgs = set(values) if orgs is None else orgs & set(values)
                hit = {p for p, o in zip(st.parent_ids, st.org_ids) if o in orgs and p in st.parents}
            elif column == "id":
                hit = {v for v in values if v in st.parents}
            elif column == "document_id":
                want = set(values)
                hit = {p for p, d in zip(st.parent_ids, st.document_ids) if d in want and p in st.parents}
            else:
                raise ValueError(f"delete: rag_parent_chunks rows are addressed by id / document_id, not {column!r}")
            pids = hit if pids is None else pids & hit
        pids = pids or set()
        if not pids:
            return []
        self._delete_rows([i for i, p in enumerate(st.parent_ids)
                           if p in pids and (orgs is None or st.org_ids[i] in orgs)])
        if orgs is not None:
            pids -= set(st.parent_ids)      # (still named by another org's chunks)
        return [st.parents.pop(p) for p in sorted(pids, key=list(st.parents).index)]

    def _delete_documents_where(self, filters) -> List[Dict[str, Any]]:
        """Documents by ``id`` -> [{"id": d}, ...] of those that had chunks; their children and
        the parents those reference go with them (schema :65, :107).  Multi-tenant, ``org_id``
        restricts the delete to that org's chunks (alone: every document of the org): a document
        or parent that other orgs' chunks still name loses the org's chunks and stays."""
        st = self.store
        docs: Optional[set] = None
        orgs: Optional[set] = None
        for column, values in filters:
            if column == "org_id" and self.multi_tenant:
                orgs = set(values) if orgs is None else orgs & set(values)
                values = {d for d, o in zip(st.document_ids, st.org_ids) if o in orgs}
            elif column != "id":
                raise ValueError(f"delete: rag_documents rows are addressed by id, not {column!r}")
            docs = set(values) if docs is None else docs & set(values)
        rows = [i for i, d in enumerate(st.document_ids)
                if d in (docs or ()) and (orgs is None or st.org_ids[i] in orgs)]
        found = list(dict.fromkeys(st.document_ids[i] for i in rows))
        pids = {st.parent_ids[i] for i in rows}
        self._delete_rows(rows)
        if orgs is not None:
            pids -= set(st.parent_ids)
            found = [d for d in found if d not in set(st.document_ids)]
        for p in pids:
            st.parents.pop(p, None)
        return [{"id": d} for d in found]

    # -------------------------------------------------------------- tables
    def table(self, name: str) -> _TableQuery:
        if name == "rag_child_chunks":
            def fetch(ids, **within):       # (within: {"org": x} of a multi-tenant eq("org_id", x))
                rows = []
                for cid in ids:
                    i = self.store.row_index(cid)
                    if i is not None and ("org" not in within or self.store.org_ids[i] == within["org"]):
                        rows.append(self.store.child_row(i))
                return rows

            def by_hash(hashes, **within):
                if "org" not in within:
                    return [{"content_hash": h} for h in dict.fromkeys(hashes) if self.store.has_hash(h)]
                own = {h for h, o in zip(self.store.content_hashes or (), self.store.org_ids) if o == within["org"]}
                return [{"content_hash": h} for h in dict.fromkeys(hashes) if h is not None and h in own]
            return _TableQuery(fetch, by_hash=by_hash, insert=self.insert_children, org_id=self.org_id,
                               delete=self._delete_children_where, tenants=self.multi_tenant)
        if name == "rag_parent_chunks":
            def parents(ids, **within):     # (within an org: the parents that org's chunks name)
                st = self.store
                own = None if "org" not in within else \
                    {p for p, o in zip(st.parent_ids, st.org_ids) if o == within["org"]}
                return [dict(st.parents[p]) for p in ids if p in st.parents and (own is None or p in own)]
            return _TableQuery(parents, insert=self.insert_parents, org_id=self.org_id,
                               delete=self._delete_parents_where, tenants=self.multi_tenant)
        # the graph tables of the entity extraction (rag2/entity_extraction.py:449-554).  Entities carry
        # no org in the store: eq("org_id", x) does not narrow a multi-tenant lookup
        if name == "rag_entities":
            def entities(ids, **_within):
                st = self.store
                return [st.entity_row(i) for i in (st.entity_index(e) for e in ids) if i is not None]

            def by_eq(eqs, **_within):
                unknown = set(eqs) - {"canonical_name"}
                if unknown or not eqs:
                    raise ValueError("rag_entities rows are looked up by id or canonical_name, not "
                                     f"{sorted(unknown) or 'without a filter'}")
                i = self.store.entity_by_canonical(eqs["canonical_name"])
                return [] if i is None else [self.store.entity_row(i)]
            return _TableQuery(entities, by_eq=by_eq, insert=self.insert_entities, org_id=self.org_id,
                               tenants=self.multi_tenant)
        if name == "rag_relations":
            return _TableQuery(lambda _ids, **_w: [], insert=self.insert_relations, org_id=self.org_id,
                               tenants=self.multi_tenant)
        if name == "rag_entity_mentions":
            return _TableQuery(lambda _ids, **_w: [], insert=self.insert_mentions, org_id=self.org_id,
                               tenants=self.multi_tenant)
        # tenant discovery of the tool layer (tools/crm_knowledge.py:89-101 in the reference)
        if name in ("rag_documents", "organizations") and self.multi_tenant:
            key = "org_id" if name == "rag_documents" else "id"

            def tenants(_ids, **within):    # (the orgs that hold rows now, in order of first appearance)
                return [{key: o} for o in dict.fromkeys(self.store.org_ids)
                        if o is not None and ("org" not in within or o == within["org"])]
            return _TableQuery(tenants, tenants=True,
                               delete=self._delete_documents_where if name == "rag_documents" else None)
        if name == "rag_documents":
            return _TableQuery(lambda _ids: [{"org_id": self.org_id}] if self.org_id else [], org_id=self.org_id,
                               delete=self._delete_documents_where)
        if name == "organizations":
            return _TableQuery(lambda _ids: [{"id": self.org_id}] if self.org_id else [])
        raise ValueError(f"table {name!r} is not served by the GPU index")

    # --------------------------------------------------------------- graph
    def _entity_index(self):
        """Trigram index of the lower-cased entity names, built on first use: (sorted trigram
        codes, entity of each) -- a keyword of >= 3 characters is looked up by intersecting the
        entity lists of its trigrams instead of scanning every name (2.5M names at 10M docs)."""
        if getattr(self, "_tri", None) is None:
            names = [nm.lower() for nm in self.store.entity_names]
            cp = np.frombuffer("\x00".join(names).encode("utf-32-le"), dtype=np.uint32).astype(np.int64)
            ent = np.repeat(np.arange(len(names), dtype=np.int64),
                            np.fromiter((len(nm) + 1 for nm in names), dtype=np.int64, count=len(names)))[:len(cp)]
            ok = np.ones(max(len(cp) - 2, 0), dtype=bool)
            for off in range(3):   # a trigram must not straddle the separator between two names
                ok &= cp[off:len(cp) - 2 + off] != 0
            code = (cp[:-2] * 1114112 + cp[1:-1]) * 1114112 + cp[2:] if len(cp) > 2 else cp[:0]
            code, e3 = code[ok], ent[:len(ok)][ok]
            order = np.argsort(code, kind="stable")      # (entities stay ascending inside a trigram)
            self._tri = (code[order], e3[order], names)
        return self._tri

    def find_entities(self, keywords: List[str], limit: int = 20) -> List[int]:
        """Entity ids whose name contains a keyword (ILIKE '%kw%'), at most 5 keywords and
        limit // len(keywords) entities each, in ascending entity order (graph_search.py:161-170)."""
        if not keywords or not self.store.entity_names:
            return []
        codes, ents, names = self._entity_index()
        per = max(1, limit // len(keywords))
        found: List[int] = []
        for kw in keywords[:5]:
            needle, hits = kw.lower(), 0
            if len(needle) >= 3:
                cp = np.frombuffer(needle.encode("utf-32-le"), dtype=np.uint32).astype(np.int64)
                tri = np.unique((cp[:-2] * 1114112 + cp[1:-1]) * 1114112 + cp[2:])
                lo, hi = np.searchsorted(codes, tri, "left"), np.searchsorted(codes, tri, "right")
                cand = None
                for j in np.argsort(hi - lo):            # rarest trigram first
                    part = np.unique(ents[lo[j]:hi[j]])
                    cand = part if cand is None else cand[np.isin(cand, part, assume_unique=True)]
                    if len(cand) == 0:
                        break
                pool = cand.tolist() if cand is not None else []
            else:
                pool = range(len(names))                 # too short for a trigram: the plain scan
            for e in pool:
                if needle in names[e]:
                    if e not in found:
                        found.append(e)
                    hits += 1
                    if hits == per:
                        break
        return found[: N.THR_GRAPH_MAX_SEEDS]

    def find_entities_batch(self, keyword_lists: Sequence[List[str]], limit: int = 20, device: bool = False):
        """``find_entities`` for a batch of queries, on the device (GpuIndex.find_entities: one
        thr_entity_match call for all of them) -> one list of entity ids per query, equal to
        ``[self.find_entities(k, limit) for k in keyword_lists]``.  device=True: the (seeds int32
        [nq, 16], counts int32 [nq]) device tensors instead, for a caller that goes on to
        index.retrieve_batch(query_seeds=seeds).  The names are uploaded on first use from
        store.entity_names, as _entity_index() builds its index on first use; a query with a keyword
        too long for the kernel is resolved by ``find_entities``."""
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
        """The chunk ids of the graph channel, best first.  A multi-tenant client scores ``org_id``'s
        chunks only (graph_search(scopes=): the reference filters by .eq("org_id", org_id),
        graph_search.py:154-230); the seeds come from ``find_entities``, which is global -- entity
        names carry no org, isolation is at the chunk."""
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
        query tokens so unit-norm tokens give a [-1, 1] relevance like a cross-encoder's."""
        if self.token_embedder is None or self.index.tokens is None:
            raise RuntimeError("no token embedder / token store: late-interaction rerank unavailable")
        qtok = np.asarray(self.token_embedder.embed_query_tokens(query), dtype=np.float16)[None]
        ids = [self.store.row_index(c) for c in child_ids]
        cand = torch.tensor([[self.store.doc_base + i if i is not None else -1 for i in ids]],
                            dtype=torch.int64, device=self.index.device)
        sc = self.index.maxsim(torch.from_numpy(qtok).to(self.index.device), cand)[0]
        return [float(v) / qtok.shape[1] if np.isfinite(v) else 0.5 for v in sc.tolist()]

    def text_to_child_id(self, text: str) -> Optional[str]:
        if not hasattr(self, "_by_text"):
            self._by_text = {t: c for t, c in zip(self.store.texts, self.store.child_ids)}
            for pid, row in self.store.parents.items():
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
