"""The writing half of ``GpuIndexClient``: inserts, deletes with their cascades, and one invalidation point per
kind of change for the client's derived state.  Index first, store second: a refused call leaves both as they were."""
from __future__ import annotations

import weakref
from typing import Any, Dict, List, Optional, Sequence

import numpy as np

from . import _native as N
from .backend_tables import LazyRows
from .index_text import NumberedRows, PendingVocabulary, number_tokens


class ClientIngest:
    # ---------------------------------------------------------- derived state: who invalidates what
    def _track(self, lazy: LazyRows) -> None:
        """Deferred replies hold LOCAL doc ids: a delete materialises the unresolved ones before
        the ids shift (weak references: a reply nobody holds any more is not kept alive)."""
        alive = [r for r in self._lazy if r() is not None and r()._fetch is not None]
        self._lazy = alive + [weakref.ref(lazy)]      # (LazyRows compares by value: no hash, no WeakSet)

    def _settle_deferred(self) -> None:
        """Read back every deferred reply that is still unresolved: before a delete shifts the local
        ids they hold, and before the cached scope plans are dropped (a deferred lexical search may
        still be reading a plan's labels on the side stream)."""
        self._pending_lex = None
        for ref in self._lazy:
            lazy = ref()
            if lazy is not None:
                try:
                    lazy.materialize()
                except Exception:   # (its own caller sees that failure when it looks at the rows)
                    pass
        self._lazy = []

    def _rows_changed(self) -> None:
        """Child rows were appended or deleted.  Deferred replies are settled BEFORE the plans go (a delete did so
        already, before the ids shifted); ``scope_plan_current`` would reject every old plan: dropping them changes no answer."""
        self._settle_deferred()
        self._plans.clear()
        self._by_text = None

    def _parents_changed(self) -> None:
        self._by_text = None        # (parent texts are in it, as "no chunk of this text")

    def _graph_changed(self) -> None:
        self._tri = None            # (entities, relations or mentions were added or removed: the index is over the old names)

    # -------------------------------------------------------------- ingest
    def _check_foreign_org(self, rows: Sequence[Dict[str, Any]]) -> None:
        """Rows of ANOTHER org are refused (alone: rag_entity_mentions rows, whose tenant is their chunk's)."""
        if self.org_id is not None and any(r.get("org_id") not in (None, self.org_id) for r in rows):
            raise ValueError("insert refused: the rows belong to another org_id than this index "
                             "(data isolation, as rpc() answers another tenant with no rows)")

    def _check_org(self, rows: Sequence[Dict[str, Any]]) -> None:
        if self.multi_tenant and any(r.get("org_id") is None for r in rows):
            raise ValueError("insert refused: this client serves several tenants, every row needs its org_id")
        self._check_foreign_org(rows)

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
        """``table("rag_child_chunks").insert(rows)``: one append of len(rows) chunks to the store and to the live
        index -> [{"id": ...}, ...].  A row is stored as ``index_build.from_rows`` stores it (float32 embedding; no
        embedding = a zero vector, outside the dense channel; the text tokenised with ``self.tokenizer``), so a bulk
        build and an insert hold the same floats.  Everything is checked first (org, duplicate ids / content hashes,
        what the index's channels need); the index is appended to before the store, so a refused append leaves both as
        they were."""
        rows = list(rows)
        self._check_org(rows)
        if not rows:
            return []
        st, idx = self.store, self.index
        st.check_new_children(rows, table="rag_child_chunks")
        parts: Dict[str, Any] = {}
        if idx.docs is not None:
            docs = np.zeros((len(rows), idx.dim), dtype=np.float32)
            for i, r in enumerate(rows):
                if r.get(embedding_key) is not None:
                    if len(r[embedding_key]) != idx.dim:
                        raise ValueError(f"embedding has {len(r[embedding_key])} dims, index has {idx.dim}")
                    docs[i] = np.asarray(r[embedding_key], dtype=np.float32)
            parts["docs"] = docs
        else:
            parts.update(docs=None, n_rows=len(rows))
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
        if self.parent_rerank:
            parent_code = dict(self._parent_code)
            for r in rows:   # a parent no earlier row names gets the next number (numbers never move)
                if r.get("parent_id") is not None:
                    parent_code.setdefault(r["parent_id"], max(parent_code.values(), default=-1) + 1)
            parts.setdefault("attributes", {})["parent"] = self._parent_column([r.get("parent_id") for r in rows], parent_code)
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
        if self.parent_rerank:
            self._parent_code = parent_code
        self._rows_changed()
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
        self._parents_changed()
        return [{"id": p["id"]} for p in rows]

    # -------------------------------------------------------------- graph ingest
    # What the reference's entity extraction writes behind a document's chunk inserts (rag2/entity_extraction.py:
    # 449-554): rag_entities upserts, rag_relations and rag_entity_mentions inserts.
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
        self._graph_changed()
        return [{"id": r["id"]} for r in rows]

    def insert_relations(self, rows: Sequence[Dict[str, Any]]):
        """``table("rag_relations").insert(rows)``: subject_entity_id / object_entity_id become entity indices; a row
        naming an unknown entity is skipped, as ``index_build.build_graph`` skips it; the rest go through
        ``GpuIndex.append_graph(relations=)`` (both directions, self-loops and edges the index already holds dropped).
        Relation types and confidences are not stored: the walk does not read them."""
        rows = list(rows)
        self._check_org(rows)
        st = self.store
        pairs = [(st.entity_index(r.get("subject_entity_id")), st.entity_index(r.get("object_entity_id"))) for r in rows]
        pairs = [(a, b) for a, b in pairs if a is not None and b is not None]
        if pairs:
            self.index.append_graph(relations=(np.asarray([a for a, _ in pairs], dtype=np.int64),
                                               np.asarray([b for _, b in pairs], dtype=np.int64)))
            self._graph_changed()
        return [{"id": r.get("id")} for r in rows]

    def insert_mentions(self, rows: Sequence[Dict[str, Any]]):
        """``table("rag_entity_mentions").insert(rows)``: entity_id / child_chunk_id become an entity index and a chunk
        of the live index; a row naming an unknown entity or chunk is skipped, as ``build_graph`` skips it;
        ``confidence`` defaults to 1.0; the rest go through ``GpuIndex.append_mentions``."""
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
            self._graph_changed()
        return [{"id": r.get("id")} for r in rows]

    # -------------------------------------------------------------- delete
    def _keys_where(self, filters, table: str, key: Sequence[Any], columns: Dict[str, Any]):
        """The AND of a delete's (column, values) filters -> (the keys they admit, the rows of the orgs named or None).
        ``key``: per store row, what ``table``'s rows are known by; ``columns``: per column the table is addressed by,
        the store column compared, None for the key itself.  Multi-tenant, ``org_id`` admits the keys of those orgs' rows."""
        keys = own = None
        for column, values in filters:
            want = set(values)
            if column == "org_id" and self.multi_tenant:
                rows = {i for i, o in enumerate(self.store.org_ids) if o in want}
                own = rows if own is None else own & rows
                hit = {key[i] for i in own}
            elif column not in columns:
                raise ValueError(f"delete: {table} rows are addressed by {' / '.join(columns)}, not {column!r}")
            elif columns[column] is None:
                hit = want
            else:
                hit = {k for k, v in zip(key, columns[column]) if v in want}
            keys = hit if keys is None else keys & hit
        return keys or set(), own

    def _child_rows_where(self, filters) -> List[int]:
        """Row indices of the child chunks that match every (column, values) filter."""
        st = self.store
        filters = [(c, [st.row_index(v) for v in vs] if c == "id" else vs) for c, vs in filters]
        rows, _ = self._keys_where(filters, "rag_child_chunks", range(len(st.child_ids)),
                                   {"id": None, "document_id": st.document_ids, "parent_id": st.parent_ids})
        return sorted(rows - {None})            # (None: an id the store does not hold)

    def _delete_rows(self, rows: List[int]) -> List[Dict[str, Any]]:
        """Remove store rows ``rows`` (sorted, distinct) from the index, then from the store."""
        if not rows:
            return []
        self._settle_deferred()     # (a deferred reply issued before the delete holds local ids that are about to shift)
        images = None
        if self.image_index is not None:
            dead = set(rows)
            images = [j for j, r in enumerate(self.image_rows) if r in dead]
            if images and len(images) >= len(self.image_rows):
                raise N.NativeError("delete refused: every row of the image index would be deleted: build a new index")
        self.index.delete_rows(np.asarray(rows, dtype=np.int64))       # index first: a refusal leaves both untouched
        deleted = self.store.delete(rows)
        if self.image_index is not None:
            if images:
                self.image_index.delete_rows(np.asarray(images, dtype=np.int64))
            gone = np.asarray(rows, dtype=np.int64)
            self.image_rows = [int(r - np.searchsorted(gone, r)) for r in self.image_rows if r not in dead]
        self._rows_changed()
        return deleted

    def delete_children(self, ids: Sequence[Any]) -> List[Dict[str, Any]]:
        """``table("rag_child_chunks").delete().in_("id", ids)``: the chunks leave the live index
        (``GpuIndex.delete_rows``) and then the store -> the deleted rows.  Unknown ids delete nothing and are not an
        error.  Unresolved deferred replies (``LazyRows``) are read back first; the index is changed before the store,
        so a refused delete (every row of the index) leaves both as they were."""
        return self._delete_rows(self._child_rows_where([("id", list(ids))]))

    def _delete_children_where(self, filters) -> List[Dict[str, Any]]:
        return self._delete_rows(self._child_rows_where(filters))

    def _delete_parents_where(self, filters) -> List[Dict[str, Any]]:
        """Parent rows by ``id`` / ``document_id`` (a parent belongs to one document: the one its children name) -> the
        deleted parent rows; their children go with them (schema :106). Multi-tenant, ``org_id`` restricts the delete
        to that org's chunks: a parent that other orgs' chunks still name loses the org's children and stays."""
        st = self.store
        pids, own = self._keys_where(filters, "rag_parent_chunks", st.parent_ids,
                                     {"id": None, "document_id": st.document_ids})
        pids = {p for p in pids if p in st.parents}
        if not pids:
            return []
        self._delete_rows([i for i, p in enumerate(st.parent_ids) if p in pids and (own is None or i in own)])
        if own is not None:
            pids -= set(st.parent_ids)      # (still named by another org's chunks)
        return [st.parents.pop(p) for p in sorted(pids, key=list(st.parents).index)]

    def _delete_documents_where(self, filters) -> List[Dict[str, Any]]:
        """Documents by ``id`` -> [{"id": d}, ...] of those that had chunks; their children and
        the parents those reference go with them (schema :65, :107).  Multi-tenant, ``org_id``
        restricts the delete to that org's chunks (alone: every document of the org): a document
        or parent that other orgs' chunks still name loses the org's chunks and stays.
        With ``graph_cascade`` the entities whose ``document_id`` is a document that is gone afterwards
        leave too, with their relations and mentions (schema :187, :217-220, :254, :258-259): after the
        chunk cascade, in one ``GpuIndex.delete_graph`` call, refused before anything is touched when it
        would leave no entity."""
        st = self.store
        docs, own = self._keys_where(filters, "rag_documents", st.document_ids, {"id": None})
        rows = [i for i, d in enumerate(st.document_ids) if d in docs and (own is None or i in own)]
        found = list(dict.fromkeys(st.document_ids[i] for i in rows))
        pids = {st.parent_ids[i] for i in rows}
        ents: List[int] = []
        if self.graph_cascade:
            dead = set(rows)
            left = {str(d) for i, d in enumerate(st.document_ids) if i not in dead}
            gone = {str(d) for d in docs} - left
            ents = [e for e, d in enumerate(st.entity_documents or ()) if d is not None and str(d) in gone]
            if ents and len(ents) >= len(st.entity_names):
                raise N.NativeError("delete refused: every entity of the index would be deleted with these documents "
                                    "(graph_cascade): build a new index")
        self._delete_rows(rows)
        self._delete_entities(ents)
        if own is not None:
            pids -= set(st.parent_ids)
            found = [d for d in found if d not in set(st.document_ids)]
        for p in pids:
            st.parents.pop(p, None)
        return [{"id": d} for d in found]

    # -------------------------------------------------------------- graph delete
    # What the reference's schema does by cascade (20260114_rag2_schema.sql:187, 217-220, 254, 258-259) and its
    # entity extraction needs before it re-runs over an updated document: rag_entities / rag_relations /
    # rag_entity_mentions rows out of the live index (``GpuIndex.delete_graph``), then out of the store.
    def _delete_entities(self, indices: Sequence[int]) -> List[Dict[str, Any]]:
        """Remove the entities ``indices`` (sorted, distinct) from the index, then from the store -> their rows."""
        if not indices:
            return []
        self.index.delete_graph(entities=np.asarray(indices, dtype=np.int64))   # index first: a refusal leaves both untouched
        deleted = self.store.delete_entities(indices)
        self._graph_changed()
        return deleted

    def _entity_filter(self, values) -> set:
        return {i for i in (self.store.entity_index(v) for v in values) if i is not None}

    def _delete_entities_where(self, filters) -> List[Dict[str, Any]]:
        """``table("rag_entities").delete()`` by ``id`` / ``canonical_name`` / ``document_id`` (the last only when the
        store holds the column) -> the deleted entity rows in index order; each leaves with its relations and its
        mentions.  Unknown ids delete nothing.  Entities carry no org in the store: ``org_id`` narrows nothing, and
        alone it is no filter."""
        st = self.store
        served = ["id", "canonical_name"] + (["document_id"] if st.entity_documents is not None else [])
        found = None
        for column, values in filters:
            if column == "org_id":
                continue
            if column not in served:
                raise ValueError(f"delete: rag_entities rows are addressed by {' / '.join(served)}, not {column!r}")
            if column == "id":
                hit = self._entity_filter(values)
            elif column == "canonical_name":
                want = set(values)
                hit = {i for i in range(len(st.entity_names)) if st.entity_row(i)["canonical_name"] in want}
            else:
                want = {str(v) for v in values}
                hit = {i for i, d in enumerate(st.entity_documents) if d is not None and str(d) in want}
            found = hit if found is None else found & hit
        if found is None:
            raise ValueError("DELETE requires a WHERE clause: a delete without a filter other than org_id is refused")
        return self._delete_entities(sorted(found))

    def _delete_relations_where(self, filters) -> List[Dict[str, Any]]:
        """``table("rag_relations").delete()`` by ``subject_entity_id`` AND ``object_entity_id`` (``in_``: the cross
        product of the known entities) -> one {"subject_entity_id", "object_entity_id"} per named pair whose edge
        the index held.  The edge goes in both directions; relation rows as rows (types, ids) are not stored."""
        ends: Dict[str, Optional[set]] = {"subject_entity_id": None, "object_entity_id": None}
        for column, values in filters:
            if column == "org_id":
                continue
            if column not in ends:
                raise ValueError(f"delete: rag_relations rows are addressed by {' / '.join(ends)}, not {column!r}")
            hit = self._entity_filter(values)
            ends[column] = hit if ends[column] is None else ends[column] & hit
        if ends["subject_entity_id"] is None or ends["object_entity_id"] is None:
            raise ValueError("delete: rag_relations rows are addressed by subject_entity_id AND object_entity_id: the "
                             "index keeps undirected edges (the set union of the relation rows) and cannot tell subject "
                             "from object -- delete the entity to remove every relation it has")
        subjects = sorted(ends["subject_entity_id"])
        if not subjects or not ends["object_entity_id"]:
            return []
        rp, ids, _ = self.index.graph_rows_host("relations", subjects)
        held = [(a, b) for j, a in enumerate(subjects) for b in sorted(ends["object_entity_id"])
                if a != b and b in set(ids[rp[j]:rp[j + 1]].tolist())]
        if not held:
            return []
        self.index.delete_graph(relations=(np.asarray([a for a, _ in held], dtype=np.int64),
                                           np.asarray([b for _, b in held], dtype=np.int64)))
        self._graph_changed()
        eid = lambda i: self.store.entity_row(i)["id"]
        return [{"subject_entity_id": eid(a), "object_entity_id": eid(b)} for a, b in held]

    def _delete_mentions_where(self, filters) -> List[Dict[str, Any]]:
        """``table("rag_entity_mentions").delete()`` by ``entity_id`` and / or ``child_chunk_id`` -> one {"entity_id",
        "child_chunk_id", "confidence"} per removed mention, in (entity, chunk) order.  Multi-tenant, ``org_id``
        restricts the delete to mentions of that org's chunks (a mention's tenant is its chunk's)."""
        st = self.store
        ents = chunks = own = None
        for column, values in filters:
            if column == "org_id":
                if self.multi_tenant:
                    rows = {i for i, o in enumerate(st.org_ids) if o in set(values)}
                    own = rows if own is None else own & rows
                continue
            if column == "entity_id":
                hit = self._entity_filter(values)
                ents = hit if ents is None else ents & hit
            elif column == "child_chunk_id":
                hit = {i for i in (st.row_index(v) for v in values) if i is not None}
                chunks = hit if chunks is None else chunks & hit
            else:
                raise ValueError(f"delete: rag_entity_mentions rows are addressed by entity_id / child_chunk_id, not {column!r}")
        if ents is None and chunks is None:
            raise ValueError("DELETE requires a WHERE clause: a delete without a filter other than org_id is refused")
        if (ents is not None and not ents) or (chunks is not None and not chunks):
            return []
        which = None if ents is None else sorted(ents)
        rp, ids, conf = self.index.graph_rows_host("mentions", which)
        gone = []
        for j in range(len(rp) - 1):
            e = j if which is None else which[j]
            for c, w in zip(ids[rp[j]:rp[j + 1]].tolist(), conf[rp[j]:rp[j + 1]].tolist()):
                if (chunks is None or c in chunks) and (own is None or c in own):
                    gone.append((e, c, w))
        if not gone:
            return []
        if own is None and chunks is None:
            named = (np.asarray(which, dtype=np.int64), np.full(len(which), -1, dtype=np.int64))
        elif own is None and ents is None:
            named = (np.full(len(chunks), -1, dtype=np.int64), np.asarray(sorted(chunks), dtype=np.int64))
        else:
            pairs = sorted({(e, c) for e, c, _ in gone})
            named = (np.asarray([e for e, _ in pairs], dtype=np.int64), np.asarray([c for _, c in pairs], dtype=np.int64))
        self.index.delete_graph(mentions=named)
        self._graph_changed()
        return [{"entity_id": st.entity_row(e)["id"], "child_chunk_id": st.child_ids[c], "confidence": float(w)}
                for e, c, w in gone]
