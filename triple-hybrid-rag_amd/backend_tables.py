"""The table half of the backend seam: replies, deferred rows, what each table serves (``TABLES``) and ``_TableQuery``,
which collects a chain's calls and decides once, in ``execute()``, among delete, insert, hash, equality and id lookup."""
from __future__ import annotations

import collections.abc
from functools import partial
from typing import Any, Callable, Dict, NamedTuple, Optional, Sequence


class _Reply:
    def __init__(self, data):
        self.data = data

    def execute(self):
        return self


class LazyRows(collections.abc.Sequence):
    """Rows of an RPC whose kernels are in flight: the read-back happens when the rows are first looked at, so the
    caller can issue its next RPC in the meantime.  A failure of the deferred part (the read-back is where an
    asynchronous HIP error of the lexical kernels surfaces) RAISES at that first look and again on every later one --
    the reference's ``_lexical_search`` has no try/except either (retrieval.py:273-292: only the graph channel swallows
    errors), so a failing lexical RPC propagates out of ``retrieve()``; a GPU fault never becomes an empty channel. Not
    a ``list`` subclass: every consumer goes through the Sequence protocol, so nothing can read an unfilled list
    storage behind the fetch (``json.dumps(rows.materialize())`` for C-level consumers that insist on a real list)."""

    __slots__ = ("_fetch", "_rows", "_error", "__weakref__")

    def __init__(self, fetch):
        self._fetch, self._rows, self._error = fetch, None, None

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


# ---- lookups: (client, keys, **within) -> rows; ``within`` is {"org": x} of a multi-tenant eq("org_id", x), else empty
def _children_by_id(c, ids, **within):
    st, rows = c.store, []
    for cid in ids:
        i = st.row_index(cid)
        if i is not None and ("org" not in within or st.org_ids[i] == within["org"]):
            rows.append(st.child_row(i))
    return rows


def _children_by_hash(c, hashes, **within):
    st = c.store
    if "org" not in within:
        return [{"content_hash": h} for h in dict.fromkeys(hashes) if st.has_hash(h)]
    own = {h for h, o in zip(st.content_hashes or (), st.org_ids) if o == within["org"]}
    return [{"content_hash": h} for h in dict.fromkeys(hashes) if h is not None and h in own]


def _parents_by_id(c, ids, **within):     # (within an org: the parents that org's chunks name)
    st = c.store
    own = None if "org" not in within else {p for p, o in zip(st.parent_ids, st.org_ids) if o == within["org"]}
    return [dict(st.parents[p]) for p in ids if p in st.parents and (own is None or p in own)]


# (rag2/entity_extraction.py:449-554; entities carry no org in the store, DESIGN 4.7: eq("org_id", x) narrows nothing)
def _entities_by_id(c, ids, **_within):
    st = c.store
    return [st.entity_row(i) for i in (st.entity_index(e) for e in ids) if i is not None]


def _entities_by_eq(c, eqs, **_within):
    unknown = set(eqs) - {"canonical_name"}
    if unknown or not eqs:
        raise ValueError("rag_entities rows are looked up by id or canonical_name, not "
                         f"{sorted(unknown) or 'without a filter'}")
    i = c.store.entity_by_canonical(eqs["canonical_name"])
    return [] if i is None else [c.store.entity_row(i)]


def _tenants(key, c, _ids, **within):
    """Tenant discovery (tools/crm_knowledge.py:89-101): the client's org, or the orgs that hold rows, in first-seen order."""
    if not c.multi_tenant:
        return [{key: c.org_id}] if c.org_id else []
    return [{key: o} for o in dict.fromkeys(c.store.org_ids) if o is not None and within.get("org", o) == o]


class _Table(NamedTuple):
    fetch: Callable                         # in_("id", ids), or no filter at all
    by_hash: Optional[Callable] = None      # in_("content_hash", hashes)
    by_eq: Optional[Callable] = None        # eq(column, value) ... -> {column: value}
    insert: Optional[str] = None            # NAME of the client's writer (a subclass may refuse it); None: read-only
    delete: Optional[str] = None            # [(column, values), ...] (AND) -> the deleted rows


TABLES: Dict[str, _Table] = {
    "rag_child_chunks": _Table(_children_by_id, by_hash=_children_by_hash, insert="insert_children",
                               delete="_delete_children_where"),
    "rag_parent_chunks": _Table(_parents_by_id, insert="insert_parents", delete="_delete_parents_where"),
    "rag_entities": _Table(_entities_by_id, by_eq=_entities_by_eq, insert="insert_entities", delete="_delete_entities_where"),
    "rag_relations": _Table(lambda _c, _ids, **_within: [], insert="insert_relations", delete="_delete_relations_where"),
    "rag_entity_mentions": _Table(lambda _c, _ids, **_within: [], insert="insert_mentions", delete="_delete_mentions_where"),
    "rag_documents": _Table(partial(_tenants, "org_id"), delete="_delete_documents_where"),
    "organizations": _Table(partial(_tenants, "id")),
}


class _TableQuery:
    def __init__(self, client, table: _Table):
        self._client, self._table = client, table
        self._ids = self._hashes = self._new_rows = self._limit = None
        self._eqs: Dict[str, Any] = {}
        self._filters: Optional[list] = None    # delete(): the (column, values) filters so far (AND)
        self._within: Dict[str, Any] = {}       # a multi-tenant client: eq("org_id", x) is a row filter, {"org": x}
        self._foreign = False                   # eq("org_id", another tenant): nothing of this index matches

    def select(self, *_cols, **_kw):
        return self

    def eq(self, *a, **_kw):
        if len(a) != 2:
            return self
        column, value = a
        if column == "org_id":
            if self._client.org_id is not None and value not in (None, self._client.org_id):
                self._foreign = True
            if not self._client.multi_tenant:
                return self
            self._within = {"org": value}
        elif self._table.by_eq is not None:
            self._eqs[column] = value
        if self._filters is not None:
            self._filters.append((column, [value]))
        return self

    def delete(self):
        """``table(t).delete().eq(col, v)`` / ``.in_(col, vs)`` ... ``.execute().data`` = the deleted rows of the table
        addressed; several filters combine with AND.  A delete without a filter other than ``org_id`` is refused at
        execute() (PostgREST refuses it too, and it would empty the index)."""
        if self._table.delete is None:
            raise ValueError("this table is read-only in the GPU index")
        self._filters = [("org_id", [self._within["org"]])] if self._within else []
        return self

    def insert(self, rows):
        if self._table.insert is None:
            raise ValueError("this table is read-only in the GPU index")
        self._new_rows = [rows] if isinstance(rows, dict) else list(rows)
        return self

    def limit(self, n: int):
        self._limit = n
        return self

    def in_(self, column: str, values: Sequence[Any]):
        if self._filters is not None:
            self._filters.append((column, list(values)))
        elif column == "content_hash" and self._table.by_hash is not None:
            self._hashes = list(values)
        elif column != "id":
            raise ValueError("only id (and rag_child_chunks.content_hash) lookups are served from the GPU index store")
        else:
            self._ids = list(values)
        return self

    def execute(self):
        c, t = self._client, self._table
        if self._filters is not None:
            if not self._filters:
                raise ValueError("DELETE requires a WHERE clause: a delete without a filter other than org_id is refused")
            return _Reply([] if self._foreign else getattr(c, t.delete)(self._filters))
        if self._new_rows is not None:
            return _Reply(getattr(c, t.insert)(self._new_rows))
        if self._hashes is not None:
            rows = [] if self._foreign else t.by_hash(c, self._hashes, **self._within)
        elif t.by_eq is not None and self._ids is None:
            rows = [] if self._foreign else t.by_eq(c, dict(self._eqs), **self._within)
        else:
            rows = t.fetch(c, self._ids or [], **self._within)
        return _Reply(rows[: self._limit] if self._limit is not None else rows)
