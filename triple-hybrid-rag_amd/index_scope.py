"""Scoped queries: every query of a batch names the rows it may see.

A SCOPE is a conjunction of equalities over per-row int32 attribute columns (org, collection,
document, category, ...): what the reference's RPCs filter by in SQL before their LIMIT (p_org_id
and p_collection, database/migrations/20260114_rag2_schema.sql:341-410; p_category and
p_source_document, src/voice_agent/retrieval/hybrid_search.py:227-231).  ``ScopedSearch`` is the part
of ``GpuIndex`` that holds the columns (``set_attributes``), resolves the distinct scopes of a batch
on the device (``scope_plan``: thr_scope_resolve) and routes every query:

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
        ``scopes``: per query a dict {attribute: value} (None / {} = unscoped), or an int32 [nq, C]
        table over attribute_names() (-1 = any value).  Host side: the distinct scopes are found
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
