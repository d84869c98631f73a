"""``CorpusStore``: the host-side row payloads of the SQL rows and the vocabulary; numpy alone, no device."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

# column -> (key of a rag_child_chunks row, what a row without it gets); the last three may be None: no such column
ROW_COLUMNS = {"child_ids": ("id", None), "parent_ids": ("parent_id", None), "document_ids": ("document_id", None),
               "texts": ("text", ""), "pages": ("page", 1), "modalities": ("modality", "text"),
               "collections": ("collection", None), "content_hashes": ("content_hash", None), "org_ids": ("org_id", None)}
ENTITY_COLUMNS = ("entity_names", "entity_ids", "entity_canonical", "entity_documents")


def number_tokens(per_text_tokens, vocab: Dict[str, int]) -> tuple:
    """THE host numbering: the token lists of a batch, one per text -> (doc int32 [T], term int32 [T], the new
    terms in id order).  A token outside ``vocab`` gets the next id at its first sighting, in text order
    (build_lexical's numbering; thr_vocab_grow's on the device); ``vocab`` itself is not changed."""
    grown: Dict[str, int] = {}
    doc, term = [], []
    for d, tokens in enumerate(per_text_tokens):
        for tok in tokens:
            t = vocab.get(tok)
            if t is None:
                t = grown.setdefault(tok, len(vocab) + len(grown))
            doc.append(d)
            term.append(t)
    return np.asarray(doc, dtype=np.int32), np.asarray(term, dtype=np.int32), list(grown)


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
    # rag_entities.document_id (the document an entity was first extracted from: ON DELETE CASCADE), parallel to
    # entity_names.  None until a row carries one
    entity_documents: Optional[List[Optional[Any]]] = None

    def __post_init__(self):
        self._row_of = {cid: i for i, cid in enumerate(self.child_ids)}
        self._hashes = {h for h in (self.content_hashes or ()) if h is not None}
        self._ent_of: Optional[Dict[Any, int]] = None       # entity id -> index, built on first use
        self._canon_of: Optional[Dict[str, int]] = None     # canonical name -> first index

    def _writable(self, names: Sequence[str]) -> List[str]:
        """A loaded column is a read-only blob: make these lists before a write -> those the store has (not None)."""
        have = [name for name in names if getattr(self, name) is not None]
        for name in have:
            if not isinstance(getattr(self, name), list):
                setattr(self, name, list(getattr(self, name)))
        return have

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
        self._writable(ENTITY_COLUMNS)
        if self.entity_ids is None:
            self.entity_ids = list(range(n0))
        if self.entity_canonical is None:
            self.entity_canonical = [None] * n0
        if self.entity_documents is None and any(r.get("document_id") is not None for r in rows):
            self.entity_documents = [None] * n0
        for r in rows:
            self.entity_ids.append(r["id"])
            self.entity_names.append(r.get("name") or "")
            self.entity_canonical.append(r.get("canonical_name"))
            if self.entity_documents is not None:
                self.entity_documents.append(r.get("document_id"))
        self._ent_of = self._canon_of = None
        return range(n0, n0 + len(rows))

    def delete_entities(self, indices: Sequence[int]) -> List[Dict[str, Any]]:
        """Remove the entities with these indices (any order, repeats allowed) -> the removed rows as ``entity_row``
        gives them, in index order.  entity_names and the id / canonical-name / document columns are compacted (entity i
        becomes entity i - #deleted below i, as ``GpuIndex.delete_graph`` renumbers the index) and the lookup caches
        are dropped.  A store without an id column gets one first: the integer ids it answered to stay those entities'."""
        n = len(self.entity_names)
        gone = sorted({int(i) for i in indices})
        if gone and (gone[0] < 0 or gone[-1] >= n):
            raise ValueError(f"entity index out of range 0 .. {n - 1}")
        if not gone:
            return []
        out = [self.entity_row(i) for i in gone]
        if self.entity_ids is None:
            self.entity_ids = list(range(n))
        dead = set(gone)
        for name in self._writable(ENTITY_COLUMNS):
            col = getattr(self, name)
            setattr(self, name, [col[i] for i in range(n) if i not in dead])
        self._ent_of = self._canon_of = None
        return out

    # ---- child chunks (rag_child_chunks)
    def has_hash(self, content_hash: Optional[str]) -> bool:
        return content_hash is not None and content_hash in self._hashes

    def check_new_children(self, rows: Sequence[Dict[str, Any]], table: Optional[str] = None) -> None:
        """The unique constraints on id and content_hash (nullable), against the store and inside the batch.  The message
        names the ``duplicate`` (ingest.py:457-460 catches it): the key that collided or, given ``table``, it and both keys."""
        ids, hashes = set(), set()
        for r in rows:
            i, h = r["id"], r.get("content_hash")
            dup_id = i in self._row_of or i in ids
            if dup_id or (h is not None and (h in self._hashes or h in hashes)):
                what = f" on {table} (id {i!r}, content_hash {h!r})" if table else \
                    f": id {i!r}" if dup_id else f": content_hash {h!r}"
                raise ValueError("duplicate key value violates unique constraint" + what)
            ids.add(i)
            hashes.add(h)

    def append(self, rows: Sequence[Dict[str, Any]], tokenizer=None) -> range:
        """Append child-chunk rows (the columns ``index_build.from_rows`` reads, plus the optional ``content_hash``) ->
        the range of their row indices.  ``page`` is nullable, as the SQL column is.  A row whose id or content hash
        the store already holds -- or that repeats one inside the batch -- raises before anything is changed
        (``check_new_children``). ``tokenizer``: unseen terms of the rows' texts get the next vocabulary ids, at the
        END, so existing term ids never move."""
        rows = list(rows)
        self.check_new_children(rows)
        if self.collections is None and any(r.get("collection") is not None for r in rows):
            raise ValueError("the store has no collection column: rows cannot carry a collection")
        n0 = len(self.child_ids)
        if self.content_hashes is None:
            self.content_hashes = [None] * n0
        # (a store without the column ignores the rows' org_id: the single-tenant ingest sends it too)
        for name in self._writable(ROW_COLUMNS):
            key, default = ROW_COLUMNS[name]
            getattr(self, name).extend(r.get(key, default) for r in rows)
        self._row_of.update((r["id"], n0 + i) for i, r in enumerate(rows))
        if tokenizer is not None:
            v0 = len(self.vocab)
            new_terms = number_tokens((tokenizer(r.get("text", "")) for r in rows), self.vocab)[2]
            self.vocab.update((tok, v0 + i) for i, tok in enumerate(new_terms))
        self._hashes.update(r["content_hash"] for r in rows if r.get("content_hash") is not None)
        return range(n0, n0 + len(rows))

    def delete(self, rows: Sequence[int]) -> List[Dict[str, Any]]:
        """Remove the child-chunk rows with these row indices (any order, repeats allowed) -> the deleted rows as
        ``child_row`` gives them, in row order.  Every column is compacted (the survivors keep their order: row i
        becomes row i - #deleted below i, as ``GpuIndex.delete_rows`` renumbers the index), the id lookup is rebuilt
        and the rows' content hashes are forgotten, so the same content can be ingested again.  Parents, the vocabulary
        and the entity names are not touched (term and entity ids never move)."""
        n = len(self.child_ids)
        gone = sorted({int(r) for r in rows})
        if gone and (gone[0] < 0 or gone[-1] >= n):
            raise ValueError(f"row index out of range 0 .. {n - 1}")
        if not gone:
            return []
        out = [self.child_row(i) for i in gone]
        dead = set(gone)
        lost = {self.content_hashes[i] for i in gone} if self.content_hashes is not None else set()
        for name in self._writable(ROW_COLUMNS):
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
