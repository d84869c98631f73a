"""Scope clauses: the numpy restatement of the clause table (what a scope written with In / Between /
Not / lists / ranges accepts) and the builders the host and the GPU tests share.  Nothing here goes
through the package's canonical forms: ``accepts`` reads the clause as the caller wrote it."""
import numpy as np

INT32_MAX = 2 ** 31 - 1


def accepts(clause, v, T):
    """Rows (values ``v``, int array; -1 = the row has none) the clause accepts -> bool array."""
    v = np.asarray(v, dtype=np.int64)
    has = v >= 0                                # a row without a value matches no clause, negated or not
    if clause is None:
        return np.zeros(v.shape, dtype=bool)
    if isinstance(clause, T.Not):
        return has & ~accepts(clause.clause, v, T)
    if isinstance(clause, T.In):
        clause = clause.values
    if isinstance(clause, range):
        clause = T.Between(clause.start, clause.stop - 1)
    if isinstance(clause, T.Between):
        lo = 0 if clause.lo is None else clause.lo
        hi = INT32_MAX if clause.hi is None else clause.hi
        return has & (v >= lo) & (v <= hi)
    if isinstance(clause, (int, np.integer)):
        return has & (v == int(clause)) if clause >= 0 else np.zeros(v.shape, dtype=bool)
    members = np.asarray(clause.cpu() if hasattr(clause, "cpu") else list(clause), dtype=np.int64).reshape(-1)
    return has & np.isin(v, members[members >= 0])


def scope_mask(scope, cols, T):
    """Rows a scope {attribute: clause} accepts over ``cols`` {attribute: int array} (None / {} = all)."""
    n = len(next(iter(cols.values())))
    m = np.ones(n, dtype=bool)
    for name, clause in (scope or {}).items():
        m &= accepts(clause, cols[name], T)
    return m


def np_resolve_masks(masks):
    """thr_scope_resolve's outputs from the match matrix bool [P, n] -> (rowptr, rows, labels, overlap)."""
    lists = [np.nonzero(m)[0].astype(np.int32) for m in masks]
    rowptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    hit = masks.any(axis=0)
    labels = np.where(hit, masks.argmax(axis=0), -2).astype(np.int32)
    rows = np.concatenate(lists).astype(np.int32) if lists else np.zeros(0, np.int32)
    return rowptr, rows, labels, int((masks.sum(axis=0) > 1).any())


def table_masks(tab, set_values, n_set, cols):
    """The kernel's contract restated for a RAW clause table int32 [P, C, 4], valid or not: an unknown
    kind matches no row, a set's window is clamped into [0, n_set] -> bool [P, n]."""
    n = len(cols[0])
    out = np.ones((tab.shape[0], n), dtype=bool)
    for p in range(tab.shape[0]):
        for c in range(tab.shape[1]):
            kind, a, b, _ = (int(x) for x in tab[p, c])
            v = cols[c].astype(np.int64)
            if kind == 0:
                continue
            if kind in (2, 6):
                inside = (v >= a) & (v <= b)
            elif kind in (3, 7):
                lo = min(max(a, 0), n_set)
                ln = min(max(b, 0), n_set - lo)
                inside = np.isin(v, np.asarray(set_values[lo:lo + ln], dtype=np.int64))
            else:
                out[p] = False
                continue
            out[p] &= (v >= 0) & (inside != (kind >= 4))
    return out


def resolve_columns(n, n_cols, seed):
    """``n_cols`` int32 columns of n rows: column 0 small values with -1 rows, column 1 a wide range
    that holds 0 and 2^31 - 1, column 2 document-like runs; the others small."""
    rng = np.random.default_rng(seed)
    cols = [rng.integers(-1, 40, n).astype(np.int32)]
    if n_cols > 1:
        c = rng.integers(0, 3000, n).astype(np.int64)
        c[rng.random(n) < 0.1] = INT32_MAX
        c[rng.random(n) < 0.1] = 0
        c[rng.random(n) < 0.1] = -1
        cols.append(c.astype(np.int32))
    if n_cols > 2:
        cols.append((np.arange(n) // 7).astype(np.int32))
    while len(cols) < n_cols:
        cols.append(rng.integers(-1, 4, n).astype(np.int32))
    return cols


def resolve_scopes(T, n_cols, names):
    """Predicates mixing every clause kind (as scopes over ``names``): sets of 0, 2, 63, 64, 65 and 1000
    members whose first and last member are the column's smallest and largest value and that hold
    members no row carries; ranges with a == b, a == 0 and b == 2^31 - 1; negations over columns
    with -1 rows."""
    In, Between, Not = T.In, T.Between, T.Not
    a = names[0]
    rng = np.random.default_rng(7)

    def members(m, lo, hi, top):
        """m distinct members: ``lo`` and ``hi`` (the column's extremes) and others below ``top``, most of
        which no row carries (50 000 .. 60 000 when there is room for it)."""
        pool = np.concatenate([np.arange(lo + 1, top), np.arange(50_000, 60_000)])
        return [lo] + sorted(rng.choice(pool, m - 2, replace=False).tolist()) + [hi]

    scopes = [{a: In([])}, {a: [0, 39]}, {a: Between(5, 5)}, {a: Between(0, 9)}, {a: Not([0, 39, 12])},
              {a: Not(Between(3, 30))}, {a: Not(7)}, {a: Between(20, None)}, {a: range(10, 12)}]
    if n_cols > 1:
        b = names[1]
        scopes += [{b: members(m, 0, INT32_MAX, 3000)} for m in (63, 64, 65, 1000)]
        scopes += [{b: Between(2999, None)}, {b: Between(INT32_MAX, INT32_MAX)}, {b: Not(members(64, 0, INT32_MAX, 3000))},
                   {a: [1, 2, 3], b: Not(Between(0, 10))}, {a: Not(In([])), b: Between(None, 100)}]
    if n_cols > 2:
        c = names[2]
        scopes += [{c: [0, 2, 4, 100000]}, {a: Between(0, 20), c: Not([1, 3]), names[1]: Between(1, None)}]
    if n_cols > 3:
        scopes += [{names[-1]: [0, 3], names[3]: Not(1)}]
    return scopes


# the scopes of the index-level tests, over make_index's columns (org 0 .. 3 with a wide tenant 0,
# collection 0 .. 2, document = row // 50)
def index_scopes(T):
    In, Between, Not = T.In, T.Between, T.Not
    return [None, {"org": 1}, {"org": 0}, {"collection": [0, 2]}, {"document": In(list(range(3, 40)))},
            {"document": Between(100, 180)}, {"org": Not(In([0, 1]))}, {"org": Not(0)},
            {"document": In([5, 17, 44, 90000]), "org": 0}, {"org": [77, 78]}, {"document": [9, 399], "collection": 1, "org": 2},
            {"document": Between(0, 10)}, {"document": Between(5, 15)}, {"collection": Not(1), "org": [1, 2, 3]}]
