"""Scoped queries: every query of a batch names the rows it may see.

A SCOPE is a conjunction of clauses over per-row int32 attribute columns (org, collection,
document, category, ...) -- an equality, a set (``In``, or any list of values), a range
(``Between``, ``range``) or the negation of one (``Not``) per column: what the reference's RPCs
filter by in SQL before their LIMIT (p_org_id
and p_collection, database/migrations/20260114_rag2_schema.sql:341-410; p_category and
p_source_document, src/voice_agent/retrieval/hybrid_search.py:227-231).  ``ScopedSearch`` is the part
of ``GpuIndex`` that holds the columns (``set_attributes``), resolves the distinct scopes of a batch
on the device (``scope_plan``: thr_scope_resolve; thr_scope_resolve_clauses once a clause of the batch
is more than an equality) and routes every query:

    unscoped                     the search as it always was;
    at most scope_rows_max rows  thr_dense_topk_rows over the scope's row list: the cost of its rows;
    wider                        the unchanged shortlist scan / exhaustive path with doc_coll = the
                                 labels thr_scope_resolve wrote and query_coll = the scope's index;
                                 scopes that may share a row are split into groups of disjoint ones,
                                 one pass per group.

Both routes return the same bits (the float64 rescoring of the float32 rows, (score desc, id asc)),
so ``scope_rows_max`` only moves time.  BM25 always filters through the labels (idf / avgdl stay
corpus-wide, as across collections and shards), and so does the graph channel where it is asked to
(graph_search(scopes=), retrieve_batch(scope_graph=True): thr_graph_topk_scoped -- the walk over the
entities is unfiltered, a chunk outside the scope is not scored).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _native as N

NO_ROW = -2      # a predicate value that matches no row: a name the store has never seen


INT32_MAX = 2 ** 31 - 1
GENERAL = -3     # in ScopePlan.preds: the column carries a clause that is no equality (see ScopePlan.clauses)
SCOPE_MAX_GENERAL = 256   # distinct scopes of a batch that holds a set, a range or a negation


class In:
    """Clause: the row's value is one of ``values`` (what a plain list, tuple, set, frozenset, 1-d integer
    array or tensor means too).  Negative members are dropped; an empty set matches no row."""
    __slots__ = ("values",)

    def __init__(self, values):
        self.values = values

    def __repr__(self):
        return f"In({self.values!r})"


class Between:
    """Clause: ``lo <= value <= hi``, both ends inclusive; None = open.  The ends are clipped to
    [0, 2^31 - 1]; ``lo > hi`` matches no row.  ``range(a, b)`` (step 1) means Between(a, b - 1)."""
    __slots__ = ("lo", "hi")

    def __init__(self, lo=None, hi=None):
        self.lo, self.hi = lo, hi

    def __repr__(self):
        return f"Between({self.lo!r}, {self.hi!r})"


class Not:
    """Clause: the negation of an equality, an ``In`` or a ``Between``.  A row whose value is -1 (it has
    none) still matches nothing: SQL's NULL under <> and NOT IN."""
    __slots__ = ("clause",)

    def __init__(self, clause):
        self.clause = clause

    def __repr__(self):
        return f"Not({self.clause!r})"


# Canonical clauses (hashable; what the distinct scopes of a batch are found by):
#   None                      any value (the attribute is not named)
#   ("none",)                 no row
#   ("eq", v)                 value == v
#   ("range", lo, hi, neg)    lo <= value <= hi, lo < hi or negated; neg: every OTHER value >= 0
#   ("set", (v, ...), neg)    two or more members, ascending and distinct
_NONE = ("none",)


def _as_int(x, what: str) -> int:
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
        raise ValueError(f"scopes: {what} must be an integer, got {x!r}")
    return int(x)


def _members(values) -> np.ndarray:
    if isinstance(values, torch.Tensor):
        values = values.detach().cpu().numpy()
    if isinstance(values, np.ndarray):
        if values.ndim != 1 or values.dtype == np.bool_ or not np.issubdtype(values.dtype, np.integer):
            raise ValueError(f"scopes: a set of values is a 1-d integer array, got {values.dtype} {values.shape}")
        v = values.astype(np.int64)
    elif isinstance(values, (list, tuple, set, frozenset)):
        v = np.array([_as_int(x, "a member of a set") for x in values], dtype=np.int64)
    else:
        raise ValueError(f"scopes: In() takes a list, tuple, set or 1-d integer array, got {values!r}")
    return np.unique(v[(v >= 0) & (v <= INT32_MAX)])


def canonical_clause(value):
    """One clause as the caller writes it -> its canonical form (see above).  Equal predicates get
    equal forms: {"org": [3]}, {"org": In([3, 3])}, {"org": Between(3, 3)} and {"org": 3} are one."""
    if value is None:
        return _NONE
    if isinstance(value, Not):
        inner = value.clause
        if inner is None or isinstance(inner, Not):
            raise ValueError(f"scopes: Not() takes an equality, In or Between, got {inner!r}")
        c = canonical_clause(inner)
        if c == _NONE:                       # Not(In([])): every row that has a value
            return ("range", 0, INT32_MAX, False)
        if c[0] == "eq":
            return ("range", c[1], c[1], True)
        return (c[0], *c[1:-1], True)
    if isinstance(value, range):
        if value.step != 1:
            raise ValueError(f"scopes: a range clause has step 1, got step {value.step}")
        value = Between(value.start, value.stop - 1)
    if isinstance(value, Between):
        lo = 0 if value.lo is None else _as_int(value.lo, "an end of Between")
        hi = INT32_MAX if value.hi is None else _as_int(value.hi, "an end of Between")
        if lo > hi or hi < 0 or lo > INT32_MAX:
            return _NONE
        lo, hi = max(lo, 0), min(hi, INT32_MAX)
        return ("eq", lo) if lo == hi else ("range", lo, hi, False)
    if isinstance(value, In) or isinstance(value, (list, tuple, set, frozenset, np.ndarray, torch.Tensor)):
        v = _members(value.values if isinstance(value, In) else value)
        if v.size == 0:
            return _NONE
        return ("eq", int(v[0])) if v.size == 1 else ("set", tuple(v.tolist()), False)
    v = _as_int(value, "a scope value")
    return ("eq", v) if 0 <= v <= INT32_MAX else _NONE


def _general(c) -> bool:
    return c is not None and c[0] in ("range", "set")


def _clause_disjoint(a, b) -> bool:
    """Provably no value satisfies both canonical clauses (neither is None)?  False = may overlap."""
    if a == _NONE or b == _NONE:
        return True
    a = ("range", a[1], a[1], False) if a[0] == "eq" else a
    b = ("range", b[1], b[1], False) if b[0] == "eq" else b
    if a[-1] and b[-1]:
        return False                                    # two negations: may overlap
    if a[-1] or b[-1]:                                  # Not(X) against Y: disjoint iff Y lies inside X
        x, y = (a, b) if a[-1] else (b, a)
        if x[0] == "range":
            lo, hi = (y[1], y[2]) if y[0] == "range" else (y[1][0], y[1][-1])
            return x[1] <= lo and hi <= x[2]
        xs = np.asarray(x[1], dtype=np.int64)
        if y[0] == "set":
            return bool(np.isin(np.asarray(y[1], dtype=np.int64), xs).all())
        inside = np.searchsorted(xs, y[2], side="right") - np.searchsorted(xs, y[1], side="left")
        return int(inside) == y[2] - y[1] + 1
    if a[0] == "range" and b[0] == "range":
        return a[2] < b[1] or b[2] < a[1]
    if a[0] == "set" and b[0] == "set":
        if a[1][-1] < b[1][0] or b[1][-1] < a[1][0]:
            return True
        return np.intersect1d(np.asarray(a[1], dtype=np.int64), np.asarray(b[1], dtype=np.int64)).size == 0
    r, st = (a, b) if a[0] == "range" else (b, a)
    xs = np.asarray(st[1], dtype=np.int64)
    return int(np.searchsorted(xs, r[2], side="right") - np.searchsorted(xs, r[1], side="left")) == 0


def scopes_disjoint(a, b) -> bool:
    """Provably no row satisfies both canonical scopes (tuples of canonical clauses, one per column)?
    True when one of them holds a clause that matches nothing, or when on some column both constrain
    the clauses are disjoint: equalities of different values, ranges that do not intersect, sets
    without a common member, a range and a set with no member inside it, Not(X) against a clause
    contained in X.  Everything else counts as "may overlap": conservative -- a pass more, never a
    wrong filter."""
    if _NONE in a or _NONE in b:
        return True
    return any(x is not None and y is not None and _clause_disjoint(x, y) for x, y in zip(a, b))


def clause_groups(keys) -> List[np.ndarray]:
    """Greedy placement, pair by pair, of the distinct canonical scopes into groups whose members are
    pairwise disjoint (scopes_disjoint) -> scope indices per group.  O(P^2) clause comparisons: what
    SCOPE_MAX_GENERAL bounds."""
    # (the members of a set as an array, once: the comparisons below are numpy's)
    keys = [tuple(("set", np.asarray(c[1], dtype=np.int64), c[2]) if c is not None and c[0] == "set" else c for c in key)
            for key in keys]
    groups: List[List[int]] = []
    for i, key in enumerate(keys):
        for g in groups:
            if all(scopes_disjoint(key, keys[j]) for j in g):
                g.append(i)
                break
        else:
            groups.append([i])
    return [np.asarray(g, dtype=np.int64) for g in groups]


def encode_clauses(keys, n_cols: int):
    """Canonical scopes -> (int32 [P, C, 4] clause table, int32 set values) of thr_scope_resolve_clauses."""
    tab = np.zeros((len(keys), n_cols, 4), dtype=np.int32)
    sets, used = [], 0
    for p, key in enumerate(keys):
        for c, cl in enumerate(key):
            if cl is None:
                continue
            if cl == _NONE:
                tab[p, c] = (N.SCOPE_NONE, 0, 0, 0)
            elif cl[0] == "eq":
                tab[p, c] = (N.SCOPE_RANGE, cl[1], cl[1], 0)
            elif cl[0] == "range":
                tab[p, c] = (N.SCOPE_RANGE | (N.SCOPE_NEGATED if cl[3] else 0), cl[1], cl[2], 0)
            else:
                tab[p, c] = (N.SCOPE_SET | (N.SCOPE_NEGATED if cl[2] else 0), used, len(cl[1]), 0)
                sets.append(np.asarray(cl[1], dtype=np.int32))
                used += len(cl[1])
    if used > N.THR_SCOPE_MAX_SET_VALUES:
        raise ValueError(f"scopes: the sets of one batch hold at most {N.THR_SCOPE_MAX_SET_VALUES} values together, got {used}")
    return tab, (np.concatenate(sets) if sets else np.zeros(0, np.int32))


def decode_clauses(tab: np.ndarray, set_values: np.ndarray):
    """encode_clauses' inverse: the canonical scopes a clause table holds."""
    keys = []
    for pred in np.asarray(tab):
        key = []
        for kind, a, b, _ in pred.tolist():
            neg = bool(kind & N.SCOPE_NEGATED)
            if kind == N.SCOPE_ANY:
                key.append(None)
            elif kind == N.SCOPE_NONE:
                key.append(_NONE)
            elif kind & ~N.SCOPE_NEGATED == N.SCOPE_RANGE:
                key.append(("eq", a) if a == b and not neg else ("range", a, b, neg))
            else:
                key.append(("set", tuple(np.asarray(set_values[a:a + b]).tolist()), neg))
        keys.append(tuple(key))
    return keys


@dataclass
class ScopePlan:
    """The distinct scopes of a batch, resolved: what dense_search / bm25_search / retrieve_batch
    take as ``scopes=`` instead of the scopes themselves (no read-back in the search then)."""
    names: List[str]                 # the attribute columns, in predicate column order
    preds: np.ndarray                # int32 [P, C] distinct predicates (-1 = any), host
    qscope: np.ndarray               # int32 [nq]: predicate of each query, -1 = unscoped
    counts: np.ndarray               # int64 [P]: rows per predicate (the one read-back)
    rowptr: Optional[torch.Tensor]   # int64 [P + 1] device
    rows: Optional[torch.Tensor]     # int32 device: the row lists, ascending per predicate
    groups: List[np.ndarray]         # predicate indices, each group pairwise disjoint
    labels: List[torch.Tensor] = field(default_factory=list)   # per group: int32 [n_docs], LOCAL index in the group
    local: Optional[np.ndarray] = None   # predicate -> (group, index in the group)
    n_docs: int = 0
    mutations: int = 0
    columns: tuple = ()              # data_ptr of every attribute column the plan was resolved over
    # a batch with a set, a range or a negation (else None: the plan is an equality plan, as it always was):
    # the table thr_scope_resolve_clauses took, and ``preds`` then holds GENERAL where a clause is no equality
    clauses: Optional[np.ndarray] = None      # int32 [P, C, 4] (kind, a, b, 0), host
    set_values: Optional[np.ndarray] = None   # int32: the members of every set clause, host


def _may_overlap(a: np.ndarray, b: np.ndarray) -> bool:
    """Can a row satisfy both predicates?  (They agree wherever both name a value.)"""
    return bool(np.all((a == -1) | (b == -1) | (a == b)))


def _row_keys(a: np.ndarray) -> np.ndarray:
    """The rows of an int32 [m, c] array as one sortable value each."""
    a = np.ascontiguousarray(a, dtype=np.int32)
    return a.view([("", np.int32)] * a.shape[1]).reshape(-1)


def disjoint_groups(preds: np.ndarray) -> List[np.ndarray]:
    """Split the DISTINCT predicates int32 [P, C] (-1 = any) into groups whose members cannot share a
    row -> predicate indices per group.  Predicates that name the same columns differ in a value, so
    they are disjoint by construction: the unit is the class of one wildcard mask (at most 2^C of
    them, one for a batch of tenants), and two classes go into different groups when some predicate of
    one agrees with some predicate of the other on every column both name (one sorted intersection
    of the projections).  O(P log P) per pair of classes; coarser than pair by pair -- a class is
    never split -- which can cost a scan pass more, never a wrong filter."""
    preds = np.asarray(preds, dtype=np.int32)
    if preds.shape[0] == 0:
        return []
    named = preds != -1
    masks, cls = np.unique(named, axis=0, return_inverse=True)
    cls = cls.reshape(-1)
    members = [np.nonzero(cls == c)[0] for c in range(masks.shape[0])]

    def conflict(a: int, b: int) -> bool:
        both = np.nonzero(masks[a] & masks[b])[0]
        if both.size == 0:
            return True     # nothing in common to differ in
        ka = _row_keys(preds[members[a]][:, both])
        kb = _row_keys(preds[members[b]][:, both])
        return np.intersect1d(ka, kb).size > 0

    groups: List[List[int]] = []     # classes per group
    for c in range(masks.shape[0]):
        for g in groups:
            if not any(conflict(c, o) for o in g):
                g.append(c)
                break
        else:
            groups.append([c])
    return [np.sort(np.concatenate([members[c] for c in g])).astype(np.int64) for g in groups]


class ScopedSearch:
    # rows up to which a scope is ranked over its row list instead of through the scan: the crossover of
    # scripts/bench_scope.py's one timing (between 4 K and 16 K rows at 1M x 768, one scope
    # per batch); batches of many thin scopes and other shapes are unmeasured
    SCOPE_ROWS_MAX = 8192
    _attrs: Optional[Dict[str, torch.Tensor]] = None   # attribute columns besides "collection" (= doc_coll)

    # ------------------------------------------------------------ columns
    def _column_key(self) -> tuple:
        return tuple(self.attribute(n).data_ptr() for n in self.attribute_names())

    def attribute_names(self) -> List[str]:
        names = ["collection"] if self.doc_coll is not None else []
        return names + list(self._attrs or {})

    def attribute(self, name: str) -> torch.Tensor:
        if name == "collection" and self.doc_coll is not None:
            return self.doc_coll
        if name not in (self._attrs or {}):
            raise ValueError(f"unknown attribute {name!r}: this index has {self.attribute_names()}")
        return self._attrs[name]

    def set_attributes(self, columns: Dict[str, object]) -> "ScopedSearch":
        """Per-row attribute columns {name: int32 [n_docs]} a scope may test (values >= 0; -1 = the row
        has none; anything below is refused).  "collection" is set_collections' column.  Replaces
        the columns of the same names.  The rows come first (set_dense / set_lexical): the row count
        is theirs.  Index set-up, not the query path: reads each column's minimum back."""
        if not self.n_docs:
            raise ValueError("set_attributes: the index has no rows yet (set_dense / set_lexical first)")
        cols = {}
        for name, col in dict(columns).items():
            t = self._t(col, torch.int32)
            if t.dim() != 1 or t.shape[0] != self.n_docs:
                raise ValueError(f"attribute {name!r}: one int32 per row ({self.n_docs}), got shape {tuple(t.shape)}")
            if int(t.min()) < -1:
                raise ValueError(f"attribute {name!r}: values are >= 0, or -1 for a row without one")
            cols[str(name)] = t
        total = set(self.attribute_names()) | set(cols)
        if len(total) > N.THR_SCOPE_MAX_COLS:
            raise ValueError(f"at most {N.THR_SCOPE_MAX_COLS} attribute columns")
        for name, t in cols.items():
            if name == "collection":
                self.set_collections(t)
            else:
                self._attrs = dict(self._attrs or {}, **{name: t})
        return self

    # ------------------------------------------------------------ plan
    def _scope_table(self, scopes, nq: int):
        """``scopes`` -> (names, int32 [nq, C] host table, -1 = any)."""
        names = self.attribute_names()
        if isinstance(scopes, (torch.Tensor, np.ndarray)):
            tab = scopes.detach().cpu().numpy() if isinstance(scopes, torch.Tensor) else np.asarray(scopes)
            if not np.issubdtype(tab.dtype, np.integer) or tab.ndim != 2 or tab.shape != (nq, len(names)):
                raise ValueError(f"scopes: an integer [{nq}, {len(names)}] table (columns {names}, -1 = any)")
            return names, np.ascontiguousarray(tab, dtype=np.int32)
        scopes = list(scopes)
        if len(scopes) != nq:
            raise ValueError(f"scopes: one per query ({nq}), got {len(scopes)}")
        tab = np.full((nq, max(len(names), 1)), -1, dtype=np.int32)
        for i, sc in enumerate(scopes):
            for name, value in (sc or {}).items():
                if name not in names:
                    raise ValueError(f"unknown attribute {name!r}: this index has {names}")
                tab[i, names.index(name)] = NO_ROW if value is None or int(value) < 0 else int(value)
        return names, tab

    def scope_plan_current(self, plan: ScopePlan, n_queries: int) -> bool:
        """Does ``plan`` still hold for a batch of n_queries on this index?  (Made for that batch size,
        no mutation and no column replaced since.)  What a caller that keeps plans asks before reuse."""
        return plan.qscope.shape[0] == n_queries and plan.n_docs == self.n_docs and \
            plan.mutations == getattr(self, "_mutations", 0) and plan.columns == self._column_key()

    def scope_plan(self, scopes, n_queries: int) -> ScopePlan:
        """Resolve the distinct scopes of a batch on the device (thr_scope_resolve) -> ScopePlan.
        ``scopes``: per query a dict {attribute: clause} (None / {} = unscoped), or an int32 [nq, C]
        table over attribute_names() (-1 = any value; equalities only).  A clause is an int >= 0
        (equality), None or an int < 0 (no row), a list / tuple / set / 1-d integer array or ``In``
        (one of the values), ``Between(lo, hi)`` or ``range(a, b)`` (inclusive range, None = open), or
        ``Not`` of one of these; the clauses of a scope are AND-ed, and a row whose value is -1 (it has
        none) matches no clause, negated or not -- only an attribute the scope does not name accepts it.
        A batch of equalities alone takes the path it always took; one with a set, a range or a
        negation resolves through thr_scope_resolve_clauses, may name at most SCOPE_MAX_GENERAL
        distinct scopes, and its scopes are grouped pair by pair (scopes_disjoint).  Scopes that may
        share a row land in different groups, and BM25 and the graph channel run ONE PASS PER GROUP
        (labels carry one scope per row): overlapping per-user document lists, for instance, cost a
        pass each -- as {"org": 3} beside {"org": 3, "collection": 1} always did.
        Host side: the distinct scopes are found
        with numpy (a table given as a DEVICE tensor is copied to the host for that: pass host data)
        and split into groups of disjoint ones (disjoint_groups: near-linear in P).  ONE small
        read-back from the device: the P + 1 row pointers (how many rows each distinct scope holds
        decide its route).  A plan stays valid until the index is mutated or a column is replaced
        (set_attributes / set_collections), on the index that made it; pass it as ``scopes=`` to
        search without the host work and the read-back."""
        if isinstance(scopes, ScopePlan):
            if not self.scope_plan_current(scopes, n_queries):
                raise ValueError("scopes: this ScopePlan was made for another batch size, another index, or before "
                                 "the index or its attribute columns changed")
            return scopes
        if not isinstance(scopes, (torch.Tensor, np.ndarray)):
            scopes = list(scopes)
        keys = self._scope_keys(scopes, n_queries)
        if keys is not None:
            if any(_general(c) for key in keys for c in key):
                return self._clause_plan(keys, n_queries)
            # equalities after all ({"org": [3]}): the same predicates as values, the path they always took
            names = self.attribute_names()
            scopes = [{n: (None if c == _NONE else c[1]) for n, c in zip(names, key) if c is not None} for key in keys]
        names, tab = self._scope_table(scopes, n_queries)
        scoped = np.any(tab != -1, axis=1)
        qscope = np.full(n_queries, -1, dtype=np.int32)
        plan = ScopePlan(names, np.zeros((0, len(names)), np.int32), qscope, np.zeros(0, np.int64), None, None, [],
                         n_docs=self.n_docs, mutations=getattr(self, "_mutations", 0), columns=self._column_key())
        if not scoped.any():
            return plan
        if not names:
            raise ValueError("scopes: this index has no attribute columns (set_attributes / set_collections)")
        preds, inv = np.unique(tab[scoped], axis=0, return_inverse=True)
        qscope[scoped] = inv.reshape(-1).astype(np.int32)
        if preds.shape[0] > N.THR_SCOPE_MAX_PREDS:
            raise ValueError(f"scopes: at most {N.THR_SCOPE_MAX_PREDS} distinct scopes per batch")
        plan.preds = np.ascontiguousarray(preds, dtype=np.int32)
        # groups of pairwise disjoint predicates (different tenants or documents: one group)
        groups = plan.groups = disjoint_groups(plan.preds)
        plan.local = np.zeros((preds.shape[0], 2), dtype=np.int32)
        for gi, g in enumerate(plan.groups):
            plan.local[g, 0] = gi
            plan.local[g, 1] = np.arange(len(g), dtype=np.int32)
        cols = [self.attribute(n) for n in names]
        dpreds = torch.from_numpy(plan.preds).to(self.device)
        rowptr, rows, labels, _ = N.scope_resolve(cols, dpreds, cap=self.n_docs, want_labels=len(groups) == 1)
        h = rowptr.cpu().numpy()                    # the one read-back
        if h[-1] > rows.shape[0]:                   # overlapping scopes: more list entries than rows
            rowptr, rows, _, _ = N.scope_resolve(cols, dpreds, cap=int(h[-1]), want_labels=False)
        plan.rowptr, plan.rows, plan.counts = rowptr, rows, np.diff(h)
        if len(groups) == 1:
            plan.labels = [labels]
        else:
            for g in plan.groups:
                _, _, lab, _ = N.scope_resolve(cols, dpreds[torch.from_numpy(g).to(self.device)].contiguous(), cap=0)
                plan.labels.append(lab)
        return plan

    def _scope_keys(self, scopes, nq: int):
        """The canonical scope of every query (a tuple of canonical clauses over attribute_names()), or
        None when ``scopes`` is a table or names nothing but plain ints and None: the batch the
        equality path has always taken, which it then takes as it is."""
        if isinstance(scopes, (torch.Tensor, np.ndarray)):
            return None
        plain = (int, np.integer)
        if all(v is None or (isinstance(v, plain) and not isinstance(v, (bool, np.bool_)))
               for sc in scopes for v in (sc or {}).values()):
            return None
        if len(scopes) != nq:
            raise ValueError(f"scopes: one per query ({nq}), got {len(scopes)}")
        names = self.attribute_names()
        keys = []
        for sc in scopes:
            key = [None] * max(len(names), 1)
            for name, value in (sc or {}).items():
                if name not in names:
                    raise ValueError(f"unknown attribute {name!r}: this index has {names}")
                key[names.index(name)] = canonical_clause(value)
            keys.append(tuple(key))
        return keys

    def _clause_plan(self, keys, n_queries: int) -> ScopePlan:
        """scope_plan for a batch that holds a set, a range or a negation: the distinct canonical scopes
        in order of first appearance, grouped pair by pair, resolved by thr_scope_resolve_clauses."""
        names = self.attribute_names()
        qscope = np.full(n_queries, -1, dtype=np.int32)
        index: Dict[tuple, int] = {}
        for i, key in enumerate(keys):
            if any(c is not None for c in key):
                qscope[i] = index.setdefault(key, len(index))
        distinct = list(index)
        if len(distinct) > SCOPE_MAX_GENERAL:
            raise ValueError(f"scopes: a batch with a set, a range or a negation names at most {SCOPE_MAX_GENERAL} "
                             f"distinct scopes, got {len(distinct)}")
        tab, sv = encode_clauses(distinct, len(names))
        preds = np.full((len(distinct), len(names)), -1, dtype=np.int32)
        for p, key in enumerate(distinct):
            for c, cl in enumerate(key):
                if cl is not None:
                    preds[p, c] = NO_ROW if cl == _NONE else cl[1] if cl[0] == "eq" else GENERAL
        groups = clause_groups(distinct)
        plan = ScopePlan(names, preds, qscope, np.zeros(0, np.int64), None, None, groups, n_docs=self.n_docs,
                         mutations=getattr(self, "_mutations", 0), columns=self._column_key(), clauses=tab, set_values=sv)
        plan.local = np.zeros((len(distinct), 2), dtype=np.int32)
        for gi, g in enumerate(groups):
            plan.local[g, 0] = gi
            plan.local[g, 1] = np.arange(len(g), dtype=np.int32)
        cols = [self.attribute(n) for n in names]
        rowptr, rows, labels, _ = N.scope_resolve_clauses(cols, tab, sv, cap=self.n_docs, want_labels=len(groups) == 1)
        h = rowptr.cpu().numpy()                    # the one read-back
        if h[-1] > rows.shape[0]:                   # overlapping scopes: more list entries than rows
            rowptr, rows, _, _ = N.scope_resolve_clauses(cols, tab, sv, cap=int(h[-1]), want_labels=False)
        plan.rowptr, plan.rows, plan.counts = rowptr, rows, np.diff(h)
        if len(groups) == 1:
            plan.labels = [labels]
        else:
            for g in groups:
                sub, sub_sv = encode_clauses([distinct[j] for j in g], len(names))
                plan.labels.append(N.scope_resolve_clauses(cols, sub, sub_sv, cap=0)[2])
        return plan

    # ------------------------------------------------------------ routes
    def _scope_rows_max(self, scope_rows_max: Optional[int]) -> int:
        return self.SCOPE_ROWS_MAX if scope_rows_max is None else int(scope_rows_max)

    def _dense_scoped(self, queries, k: int, kprime, rescue: bool, sync: bool, scopes,
                      scope_rows_max: Optional[int]):
        queries = self._t(queries, torch.float32)
        nq = queries.shape[0]
        plan = self.scope_plan(scopes, nq)
        if not plan.groups:
            return self.dense_search(queries, k, kprime, rescue, sync)
        rmax = self._scope_rows_max(scope_rows_max)
        S, I, cnt, _ = N._alloc_out(nq, k, self.device)
        n_rescued = 0 if sync else torch.zeros(1, dtype=torch.int32, device=self.device)
        qs = plan.qscope
        thin_pred = (plan.counts <= rmax) & (rmax > 0)
        thin_q = (qs >= 0) & thin_pred[np.maximum(qs, 0)]

        def put(idx: np.ndarray, res):
            nonlocal n_rescued
            at = torch.from_numpy(idx).to(self.device)
            S[at], I[at], cnt[at] = res[0], res[1], res[2]
            if len(res) > 3:
                n_rescued = n_rescued + res[3]

        idx = np.nonzero(qs < 0)[0]
        if idx.size:
            put(idx, self.dense_search(queries[torch.from_numpy(idx).to(self.device)], k, kprime, rescue, sync))
        idx = np.nonzero(thin_q)[0]
        if idx.size:
            sub = queries[torch.from_numpy(idx).to(self.device)].contiguous()
            put(idx, N.dense_topk_rows(self.docs, self.dnorm, sub, k, plan.rowptr, plan.rows,
                                       torch.from_numpy(qs[idx]).to(self.device), self.doc_base)[:3])
        for gi in range(len(plan.groups)):
            idx = np.nonzero((qs >= 0) & ~thin_q & (plan.local[np.maximum(qs, 0), 0] == gi))[0]
            if idx.size:
                sub = queries[torch.from_numpy(idx).to(self.device)].contiguous()
                qc = torch.from_numpy(plan.local[qs[idx], 1].astype(np.int32)).to(self.device)
                put(idx, self.dense_search(sub, k, kprime, rescue, sync, collections=qc, _labels=plan.labels[gi]))
        return S, I, cnt, n_rescued

    def _per_group(self, plan: ScopePlan, nq: int, call):
        """``call(at, labels, query_label)`` once per group of disjoint scopes -- ``at``: the device indices
        of the group's queries (None: the whole batch), ``labels``: the group's row labels, ``query_label``
        int32: each query's index in the group -- and the results put back in batch order.  The unscoped
        queries ride with the first group (query label -1: no filter)."""
        qs = plan.qscope
        out = None
        for gi in range(len(plan.groups)):
            mask = ((qs >= 0) & (plan.local[np.maximum(qs, 0), 0] == gi)) | ((qs < 0) & (gi == 0))
            idx = np.nonzero(mask)[0]
            if not idx.size:
                continue
            ql = np.where(qs[idx] >= 0, plan.local[np.maximum(qs[idx], 0), 1], -1).astype(np.int32)
            whole = len(plan.groups) == 1 and idx.size == nq
            at = None if whole else torch.from_numpy(idx).to(self.device)
            res = call(at, plan.labels[gi], torch.from_numpy(ql).to(self.device))
            if whole:
                return res
            if out is None:
                out = tuple(torch.empty((nq,) + tuple(r.shape[1:]), dtype=r.dtype, device=r.device) for r in res)
            for o, r in zip(out, res):
                o[at] = r
        return out

    def _bm25_scoped(self, query_terms, k: int, scopes, conjunctive: bool, prune: bool, dense_rows: bool):
        qt = self._t(query_terms, torch.int32)
        plan = self.scope_plan(scopes, qt.shape[0])
        if not plan.groups:
            return self.bm25_search(qt, k, None, conjunctive, prune, dense_rows)
        return self._per_group(plan, qt.shape[0], lambda at, labels, ql: self.bm25_search(
            qt if at is None else qt[at].contiguous(), k, ql, conjunctive, prune, dense_rows, _labels=labels))

    def _graph_scoped(self, query_seeds, k: int, hops: int, scopes):
        seeds = self._t(query_seeds, torch.int32)
        plan = self.scope_plan(scopes, seeds.shape[0])
        if not plan.groups:
            return self.graph_search(seeds, k, hops)
        return self._per_group(plan, seeds.shape[0], lambda at, labels, ql: self.graph_search(
            seeds if at is None else seeds[at].contiguous(), k, hops, _labels=(labels, ql)))
