"""Built cases for graph delete: thr_csr_prune's row shapes and ``csr_prune_ref``, its plain numpy
restatement (tests/test_graph_delete_host.py pins the restatement to index_build.build_graph, so the GPU
tests may use it as their reference); reference-shaped table rows with deletions of every kind for the
index-level tests.

A case is a CSR A built from named rows, the rows that leave, an id remap (or none) and the (row, id)
pairs B names, so that a test can find the row a property is about.  Payloads are int32 bit patterns
(viewed as float32 on the device), all distinct: which copy of an id survived is visible in the result."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

S = 1024                      # THR_CSR_PRUNE_SLICE (test_graph_delete_host pins it to the header and the library)
UNSORTED_B, OVERFLOW, BAD_ROW = 1, 2, 4


def row_of_positions(rowptr):
    return np.repeat(np.arange(len(rowptr) - 1, dtype=np.int64), np.diff(rowptr))


def csr_prune_ref(rowptr_a, ids_a, pay_a, row_remap, rows_out, id_remap, id_base, rowptr_b, ids_b):
    """thr_csr_prune in numpy -> dict(rowptr, ids, pay or None, keep uint8, nnz, status).  An entry of
    row t survives when the row does (row_remap[t] >= 0), its id does (id_remap given: inside
    [id_base, id_base + len) and remapped >= 0) and B's row t does not hold its id; survivors keep
    their order, rows and ids are renumbered.  B's rows under removed rows are not looked at.  A B
    row that is not strictly ascending sets UNSORTED_B and leaves the arrays undefined (None)."""
    rows_a, nnz_a = len(rowptr_a) - 1, len(ids_a)
    row = row_of_positions(rowptr_a)
    alive = np.ones(rows_a, dtype=bool) if row_remap is None else (np.asarray(row_remap) >= 0)
    assert int(alive.sum()) == rows_out
    if row_remap is not None:
        assert np.array_equal(np.asarray(row_remap)[alive], np.arange(rows_out))
    status = 0
    keep = alive[row] if nnz_a else np.zeros(0, dtype=bool)
    new_ids = ids_a.astype(np.int64)
    if id_remap is not None:
        i = new_ids - id_base
        ok = (i >= 0) & (i < len(id_remap))
        m = np.full(nnz_a, -1, dtype=np.int64)
        m[ok] = np.asarray(id_remap, dtype=np.int64)[i[ok]]
        keep = keep & (m >= 0)
        new_ids = m + id_base
    if rowptr_b is not None and len(ids_b):
        row_b = row_of_positions(rowptr_b)
        d = np.diff(ids_b.astype(np.int64))
        same_row = row_b[1:] == row_b[:-1]
        if np.any(same_row & alive[row_b[1:]] & (d <= 0)):
            return dict(rowptr=None, ids=None, pay=None, keep=None, nnz=None, status=UNSORTED_B)
        live_b = alive[row_b]
        named = (row_b[live_b] << 32) | (ids_b[live_b].astype(np.int64) & 0xFFFFFFFF)
        mine = (row << 32) | (ids_a.astype(np.int64) & 0xFFFFFFFF)
        keep = keep & ~np.isin(mine, named)
    before = np.concatenate([[0], np.cumsum(keep)]).astype(np.int64)
    rowptr = np.concatenate([before[rowptr_a[:-1]][alive], before[-1:]]).astype(np.int64)
    return dict(rowptr=rowptr, ids=new_ids[keep].astype(np.int32), pay=None if pay_a is None else pay_a[keep],
                keep=keep.astype(np.uint8), nnz=int(before[-1]), status=status)


@dataclass
class Case:
    name: str
    rowptr_a: np.ndarray
    ids_a: np.ndarray
    pay_a: np.ndarray
    row_remap: Optional[np.ndarray]
    rows_out: int
    id_remap: Optional[np.ndarray]
    id_base: int
    rowptr_b: Optional[np.ndarray]
    ids_b: Optional[np.ndarray]
    short: int = 0                                           # out_capacity = the kept count - short
    status: int = 0                                          # the expected status word
    rows: Dict[str, int] = field(default_factory=dict)       # named row -> its OLD index

    def row(self, t: int) -> np.ndarray:
        return self.ids_a[self.rowptr_a[t]:self.rowptr_a[t + 1]]

    def span(self, name: str):
        t = self.rows[name]
        return int(self.rowptr_a[t]), int(self.rowptr_a[t + 1])


def expected(c: Case) -> dict:
    """The restatement's answer for a case; with ``short`` the status gains OVERFLOW and only the first
    out_capacity elements of ids / pay are defined (the test cuts there)."""
    out = csr_prune_ref(c.rowptr_a, c.ids_a, c.pay_a, c.row_remap, c.rows_out, c.id_remap, c.id_base, c.rowptr_b, c.ids_b)
    if c.short and out["nnz"] is not None:
        out["status"] |= OVERFLOW
    return out


def capacity(c: Case) -> int:
    e = expected(c)
    return len(c.ids_a) if e["nnz"] is None else e["nnz"] - c.short


def _csr(rows: List[np.ndarray]):
    lens = [len(r) for r in rows]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] or [np.zeros(0, np.int64)]).astype(np.int32)
    return rowptr, ids


def make_case(name, rows, id_remap=None, id_base=0, with_b=True, remap_rows=True, **kw) -> Case:
    """``rows``: [(row name or None, A's ids, B's ids, the row stays?), ...]."""
    rp_a, ids_a = _csr([np.asarray(a) for _, a, _, _ in rows])
    rp_b, ids_b = _csr([np.asarray(b) for _, _, b, _ in rows])
    stays = np.array([bool(s) for _, _, _, s in rows], dtype=bool)
    remap = np.where(stays, np.cumsum(stays) - 1, -1).astype(np.int32)
    if not remap_rows:
        assert stays.all()
    pay_a = np.arange(1, len(ids_a) + 1, dtype=np.int32)
    names = {nm: t for t, (nm, _, _, _) in enumerate(rows) if nm}
    return Case(name, rp_a, ids_a, pay_a, remap if remap_rows else None, int(stays.sum()),
                None if id_remap is None else np.asarray(id_remap, dtype=np.int32), id_base,
                rp_b if with_b else None, ids_b if with_b else None, rows=names, **kw)


def _asc(rng, n, hi=200_000):
    return np.sort(rng.choice(hi, n, replace=False))


def _empty(n):
    return [(None, [], [], True)] * n


def _slice_edges() -> Case:
    """Rows of exactly S - 1, S and S + 1 entries, in front of them a row of 5 so that each straddles a
    slice edge or ends on one; a few entries of each leave."""
    rng = np.random.default_rng(11)
    rows = [("lead", _asc(rng, 5), [], True)]
    for nm, n in (("s_minus_1", S - 1), ("s", S), ("s_plus_1", S + 1)):
        a = _asc(rng, n)
        rows.append((nm, a, a[::97], True))
    rows.append(("removed", _asc(rng, 40), [], False))
    a = _asc(rng, 1100)
    rows.append(("straddles", a, a[300:320], True))
    return make_case("slice_edges", rows)


def _star() -> Case:
    rng = np.random.default_rng(12)
    a = _asc(rng, 3 * S + 5)
    rows = [("small", [3, 9], [9], True), ("star", a, a[::3], True), ("after", [1, 2, 3], [], True)]
    return make_case("star", rows)


def _empty_runs() -> Case:
    """1 000 consecutive empty rows at the start, in the middle and at the end; some of them leave."""
    rng = np.random.default_rng(13)
    head, mid, tail = _empty(1000), _empty(1000), _empty(1000)
    head[7] = mid[500] = tail[998] = (None, [], [], False)
    rows = head + [("first", _asc(rng, 30), [], True), ("gone", _asc(rng, 9), [], False)] + mid + \
        [("second", _asc(rng, 50), [], True)] + tail
    return make_case("empty_runs", rows)


def _first_last_removed() -> Case:
    rng = np.random.default_rng(14)
    rows = [("first", _asc(rng, 20), [], False)] + [(None, _asc(rng, int(n)), [], True) for n in rng.integers(0, 9, 40)] + \
        [("last", _asc(rng, 33), [], False)]
    return make_case("first_last_removed", rows)


def _slice_emptied() -> Case:
    """Three slices of A; every entry of the second is named by B (rows cut so that they end on its edges)."""
    rng = np.random.default_rng(15)
    rows = [("front", _asc(rng, S), [], True)]
    for n in (400, 24, 600):
        a = _asc(rng, n)
        rows.append((None, a, a, True))
    rows.append(("back", _asc(rng, S - 17), [], True))
    return make_case("slice_emptied", rows)


def _nothing_dropped() -> Case:
    """Identity remaps and a B that names nothing A holds: the output equals the input."""
    rng = np.random.default_rng(16)
    rows = []
    for n in rng.integers(0, 60, 80):
        a = 2 * _asc(rng, int(n), 5000)
        rows.append((None, a, (a + 1)[::5], True))
    return make_case("nothing_dropped", rows, id_remap=np.arange(10_000))


def _b_absent() -> Case:
    rows = [("below", [10, 20, 30], [1, 2, 3], True), ("above", [1, 2, 3], [50, 60], True),
            ("between", [10, 30, 50], [20, 30, 40], True), ("empty_a", [], [4, 5], True), ("empty_b", [7, 8], [], True)]
    return make_case("b_absent", rows)


def _b_under_removed() -> Case:
    """B rows under removed rows are ignored -- the unsorted one too."""
    rows = [("kept", [1, 2, 3, 4], [2], True), ("removed_sorted_b", [5, 6, 7], [5, 7], False),
            ("removed_unsorted_b", [8, 9], [9, 8, 8], False), ("kept_2", [4, 5, 6], [6], True)]
    return make_case("b_under_removed", rows)


def _multiset() -> Case:
    """An unsorted multiset row: five copies of the dropped id beside kept ones, each with its own payload."""
    rows = [("multi", [7, 3, 7, 9, 7, 3, 7, 1, 7, 9], [7], True), ("plain", [7, 8], [8], True)]
    return make_case("multiset", rows)


def _ids_outside(with_remap: bool, id_base: int) -> Case:
    """Ids outside [id_base, id_base + n_ids): dropped under an id_remap, passed through without one."""
    n_ids = 50
    remap = np.where(np.arange(n_ids) % 4 == 1, -1, 0)
    remap[remap == 0] = np.arange((remap == 0).sum())
    inside = id_base + np.arange(n_ids)
    rows = [("mixed", np.concatenate([[max(id_base - 1, 0)], inside[:20], [id_base + n_ids, 2 ** 31 - 1]]), [], True),
            ("inside", inside[20:], inside[25:27], True), ("outside", [id_base + n_ids + 5, id_base + 9000], [], True)]
    name = f"ids_outside_{'with' if with_remap else 'without'}_remap_base_{id_base}"
    return make_case(name, rows, id_remap=remap if with_remap else None, id_base=id_base)


def _overflow() -> Case:
    rng = np.random.default_rng(17)
    rows = []
    for n in rng.integers(0, 40, 60):
        a = _asc(rng, int(n), 3000)
        rows.append((None, a, a[::4], True))
    return make_case("overflow", rows, short=1)


def _unsorted_b() -> Case:
    rows = [("fine", [1, 2, 3], [1, 3], True), ("unsorted", [4, 5, 6], [6, 4], True)]
    return make_case("unsorted_b", rows, status=UNSORTED_B)


def _repeated_b() -> Case:
    rows = [("repeat", [4, 5, 6], [4, 4], True)]
    return make_case("repeated_b", rows, status=UNSORTED_B)


def _nnz_zero() -> Case:
    rows = [(None, [], [], True), ("gone", [], [], False), (None, [], [], True)]
    return make_case("nnz_zero", rows, with_b=False)


def _rows_zero() -> Case:
    return make_case("rows_zero", [], with_b=False)


def _no_remaps() -> Case:
    """Neither remap: only B's pairs leave."""
    rng = np.random.default_rng(18)
    rows = []
    for n in rng.integers(0, 30, 50):
        a = _asc(rng, int(n), 2000)
        rows.append((None, a, a[1::3], True))
    return make_case("no_remaps", rows, remap_rows=False)


def _random_70000() -> Case:
    """About 70 000 entries, a square CSR (ids are rows: the entity CSR's shape) with removals of all three kinds."""
    rng = np.random.default_rng(19)
    n = 4000
    lens = rng.integers(0, 36, n)
    lens[n // 3] = 2 * S + 77
    stays = rng.random(n) >= 0.1
    stays[[0, n - 1]] = True
    remap = np.where(stays, np.cumsum(stays) - 1, -1)
    rows = []
    for t in range(n):
        a = _asc(rng, int(lens[t]), n)
        b = np.sort(np.concatenate([a[rng.random(len(a)) < 0.1], rng.choice(n, 2, replace=False)]))
        rows.append((None, a, np.unique(b), bool(stays[t])))
    return make_case("random_70000", rows, id_remap=remap)


_CASES: Dict[str, Case] = {}


def cases() -> Dict[str, Case]:
    if not _CASES:
        for c in (_slice_edges(), _star(), _empty_runs(), _first_last_removed(), _slice_emptied(), _nothing_dropped(),
                  _b_absent(), _b_under_removed(), _multiset(), _ids_outside(True, 0), _ids_outside(False, 0),
                  _ids_outside(True, 700), _ids_outside(False, 700), _overflow(), _unsorted_b(), _repeated_b(),
                  _nnz_zero(), _rows_zero(), _no_remaps(), _random_70000()):
            for a in (c.rowptr_a, c.ids_a, c.pay_a, c.row_remap, c.id_remap, c.rowptr_b, c.ids_b):
                if a is not None:
                    a.setflags(write=False)
            _CASES[c.name] = c
    return _CASES


# ------------------------------------------------------------------ table rows and deletions of every kind
def graph_deletions(seed: int, n_entities: int, relations, mentions, n_chunks: int):
    """Random deletions over reference-shaped rows -> (entity positions, (subject, object) positions,
    (entity, chunk) positions with -1 wildcards).  ``relations`` / ``mentions``: rows with e<i> / c<j> ids."""
    rng = np.random.default_rng(seed)
    ents = rng.choice(n_entities, max(1, n_entities // 8), replace=False)
    ents = np.concatenate([ents, ents[:2]])                                     # repeats are allowed
    e = lambda s: int(s[1:])
    rel = [(e(r["subject_entity_id"]), e(r["object_entity_id"])) for r in relations]
    pick = rng.choice(len(rel), max(1, len(rel) // 6), replace=False)
    pairs = [rel[i] if k % 2 else rel[i][::-1] for k, i in enumerate(pick)]     # either orientation
    pairs += [(3, 3), (0, n_entities - 1)]                                      # a self pair; (most likely) no edge
    men = [(e(m["entity_id"]), int(m["child_chunk_id"][1:])) for m in mentions]
    pick = rng.choice(len(men), max(1, len(men) // 6), replace=False)
    mp = [men[i] for i in pick] + [(int(rng.integers(n_entities)), -1), (-1, int(rng.integers(n_chunks)))]
    return (ents.astype(np.int64), (np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])),
            (np.array([p[0] for p in mp]), np.array([p[1] for p in mp])))


def surviving_rows(entities, relations, mentions, del_entities=(), del_relations=None, del_mentions=None, chunk_ids=None):
    """The table rows a fresh build sees after the deletions.  The deletions name entities by their position in
    ``entities`` and chunks by their position in ``chunk_ids`` (default: chunk j is "c<j>")."""
    eid = [r["id"] for r in entities]
    cid = (lambda j: f"c{int(j)}") if chunk_ids is None else (lambda j: chunk_ids[int(j)])
    gone = {eid[int(i)] for i in del_entities}
    edges = set()
    if del_relations is not None:
        for s, o in zip(*del_relations):
            edges |= {(eid[int(s)], eid[int(o)]), (eid[int(o)], eid[int(s)])}
    named = set()
    if del_mentions is not None:
        named = {(None if en < 0 else eid[int(en)], None if ch < 0 else cid(ch)) for en, ch in zip(*del_mentions)}
    ents = [r for r in entities if r["id"] not in gone]
    rels = [r for r in relations if r["subject_entity_id"] not in gone and r["object_entity_id"] not in gone
            and (r["subject_entity_id"], r["object_entity_id"]) not in edges]
    mens = [m for m in mentions if m["entity_id"] not in gone
            and (m["entity_id"], m["child_chunk_id"]) not in named and (m["entity_id"], None) not in named
            and (None, m["child_chunk_id"]) not in named]
    return ents, rels, mens


def delete_graph_ref(graph, n_docs, doc_base, entities=None, relations=None, mentions=None):
    """GpuIndex.delete_graph restated with csr_prune_ref over host arrays -> (the five graph arrays, remap):
    the entity CSR pruned with the entity remap as row and id remap and B = the named pairs in both
    directions; the mention CSR with the entity remap as row remap, a chunk mask for (-1, chunk) and
    B = the named (entity, chunk) pairs, (entity, -1) spelled out from the entity's own row."""
    er, ec, mr, mc, mw = graph
    n_ent = len(er) - 1
    keep = np.ones(n_ent, dtype=bool)
    if entities is not None and len(entities):
        keep[np.asarray(entities, dtype=np.int64)] = False
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    n_new = int(keep.sum())

    def pairs_csr(rows, ids):
        key = np.unique((np.asarray(rows, dtype=np.int64) << 32) | np.asarray(ids, dtype=np.int64))
        rp = np.concatenate([[0], np.cumsum(np.bincount(key >> 32, minlength=n_ent))]).astype(np.int64)
        return rp, (key & 0xFFFFFFFF).astype(np.int32)

    rp_b = ids_b = None
    if relations is not None and len(relations[0]):
        s, o = (np.asarray(a, dtype=np.int64) for a in relations)
        rp_b, ids_b = pairs_csr(np.concatenate([s, o]), np.concatenate([o, s]))
    ent = csr_prune_ref(er, ec, None, remap, n_new, remap, 0, rp_b, ids_b)
    rp_b = ids_b = mask = None
    if mentions is not None and len(mentions[0]):
        e, c = (np.asarray(a, dtype=np.int64) for a in mentions)
        if (e < 0).any():
            mask = np.arange(n_docs, dtype=np.int32)
            mask[c[e < 0]] = -1
        pe, pc = list(e[(e >= 0) & (c >= 0)]), list(c[(e >= 0) & (c >= 0)] + doc_base)
        for x in np.unique(e[(c < 0) & (e >= 0)]):
            row = mc[mr[x]:mr[x + 1]]
            pe += [x] * len(row)
            pc += row.tolist()
        if pe:
            rp_b, ids_b = pairs_csr(pe, pc)
    men = csr_prune_ref(mr, mc, mw.view(np.int32), remap, n_new, mask, doc_base, rp_b, ids_b)
    return (ent["rowptr"], ent["ids"], men["rowptr"], men["ids"], men["pay"].view(np.float32)), remap
