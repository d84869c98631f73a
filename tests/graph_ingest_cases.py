"""Built cases for graph ingest: thr_csr_merge's row shapes and ``csr_merge_ref``, its plain numpy
restatement in both modes; reference-shaped table rows in ingest steps for the index-level tests.

A case is two CSRs over one row space (A: the index so far, B: the canonicalised batch) built from
named row pairs, so that a test can find the row a property is about.  Payloads are int32 bit
patterns (viewed as float32 on the device): A's are positive and B's negative, all distinct, so the
order of equal ids is visible in the result."""
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import numpy as np

S = 1024                      # THR_CSR_MERGE_SLICE (test_graph_ingest_host pins it to the header and the library)
ID_MAX = 2 ** 31 - 2
UNSORTED_A, UNSORTED_B, OVERFLOW = 1, 2, 4
NEG_ZERO, NAN_A, NAN_B = -2 ** 31, 0x7FC00001, -0x400000     # float bit patterns: -0.0, two NaNs


def _in_order(rowptr, ids, strict):
    """Every entry against its predecessor inside its row."""
    if len(ids) < 2:
        return True
    d = np.diff(ids.astype(np.int64))
    inside = np.ones(len(ids) - 1, dtype=bool)
    starts = rowptr[(rowptr > 0) & (rowptr < len(ids))]
    inside[starts - 1] = False
    return bool(np.all((d > 0) | ~inside)) if strict else bool(np.all((d >= 0) | ~inside))


def csr_merge_ref(rowptr_a, ids_a, pay_a, rowptr_b, ids_b, pay_b, drop_present, variant=None):
    """thr_csr_merge in numpy -> (rowptr_out, ids_out, pay_out or None, nnz_out, status).  Row t of
    the result is the stable sort by id of A's row t followed by B's (A first on equal ids, each side
    in its own order); drop_present removes from B what A's row holds.  A non-zero status (an input
    out of order for the mode) leaves the arrays undefined: None.
    ``variant``: a deliberately wrong rule, for the tests that show the cases tell them apart --
    "b_first" (B before A on ties), "drop_in_multiset", "keep_in_union"."""
    rows_a, rows_b = len(rowptr_a) - 1, len(rowptr_b) - 1
    assert rows_b >= rows_a
    status = (0 if _in_order(rowptr_a, ids_a, drop_present) else UNSORTED_A) | \
        (0 if _in_order(rowptr_b, ids_b, drop_present) else UNSORTED_B)
    if status:
        return None, None, None, None, status
    drop = (drop_present and variant != "keep_in_union") or (not drop_present and variant == "drop_in_multiset")
    two = pay_a is not None or pay_b is not None
    out_ids, out_pay, lens = [], [], np.zeros(rows_b, dtype=np.int64)
    for t in range(rows_b):
        a0, a1 = (int(rowptr_a[t]), int(rowptr_a[t + 1])) if t < rows_a else (0, 0)
        b0, b1 = int(rowptr_b[t]), int(rowptr_b[t + 1])
        if a0 == a1 and b0 == b1:
            continue
        a, b = ids_a[a0:a1], ids_b[b0:b1]
        keep = ~np.isin(b, a) if drop else np.ones(len(b), dtype=bool)
        first, second = (b[keep], a) if variant == "b_first" else (a, b[keep])
        both = np.concatenate([first, second])
        order = np.argsort(both, kind="stable")
        out_ids.append(both[order])
        lens[t] = len(both)
        if two:
            pa, pb = pay_a[a0:a1], pay_b[b0:b1][keep]
            out_pay.append(np.concatenate([pb, pa] if variant == "b_first" else [pa, pb])[order])
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate(out_ids).astype(np.int32) if out_ids else np.zeros(0, dtype=np.int32)
    pay = (np.concatenate(out_pay).astype(np.int32) if out_pay else np.zeros(0, dtype=np.int32)) if two else None
    return rowptr, ids, pay, int(rowptr[-1]), 0


@dataclass
class Case:
    name: str
    rowptr_a: np.ndarray
    ids_a: np.ndarray
    pay_a: np.ndarray
    rowptr_b: np.ndarray
    ids_b: np.ndarray
    pay_b: np.ndarray
    modes: Tuple[int, ...] = (1, 0)            # drop_present values the inputs are in order for
    rows: Dict[str, int] = field(default_factory=dict)     # named row -> its index
    status: Dict[int, int] = field(default_factory=dict)   # mode -> expected status (precondition cases)

    def row(self, side: str, t: int) -> np.ndarray:
        rp, ids = (self.rowptr_a, self.ids_a) if side == "a" else (self.rowptr_b, self.ids_b)
        return ids[rp[t]:rp[t + 1]] if t < len(rp) - 1 else ids[:0]


def _csr(rows: List[np.ndarray]):
    lens = [len(r) for r in rows]
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] or [np.zeros(0, np.int64)]).astype(np.int32)
    return rowptr, ids


def make_case(name, pairs, rows_a=None, **kw) -> Case:
    """``pairs``: [(row name or None, A's ids, B's ids), ...]; rows >= rows_a exist in B only."""
    rows_a = len(pairs) if rows_a is None else rows_a
    assert all(len(a) == 0 for _, a, _ in pairs[rows_a:])
    rp_a, ids_a = _csr([np.asarray(a) for _, a, _ in pairs[:rows_a]])
    rp_b, ids_b = _csr([np.asarray(b) for _, _, b in pairs])
    pay_a = np.arange(1, len(ids_a) + 1, dtype=np.int32)
    pay_b = -np.arange(1, len(ids_b) + 1, dtype=np.int32) - 1
    names = {nm: t for t, (nm, _, _) in enumerate(pairs) if nm}
    return Case(name, rp_a, ids_a, pay_a, rp_b, ids_b, pay_b, rows=names, **kw)


def _split(rng, n_a, n_b, n_both, lo=0, hi=200_000):
    """Sorted distinct ids: A's row of n_a, B's row of n_b, n_both of them shared."""
    pool = np.sort(rng.choice(np.arange(lo, hi), n_a + n_b - n_both, replace=False))
    pick = rng.permutation(len(pool))
    both, only_a, only_b = pick[:n_both], pick[n_both:n_a], pick[n_a:]
    return np.sort(pool[np.concatenate([both, only_a])]), np.sort(pool[np.concatenate([both, only_b])])


def _shapes() -> Case:
    a = np.array([10, 20, 30, 40])
    return make_case("shapes", [
        ("both_empty", [], []),
        ("only_a", [1, 5, 9], []),
        ("only_b", [], [2, 4]),
        ("b_below", [100, 200, 300], [1, 2, 3]),
        ("b_above", [1, 2, 3], [100, 101]),
        ("interleaved", [0, 2, 4, 6, 8], [1, 3, 5, 7, 9]),
        ("b_present", a, [20, 40]),
        ("ends_equal", [3, 7, 11, 20], [3, 9, 20]),
        ("id_extremes", [0, 5, ID_MAX], [0, 1, ID_MAX]),
        ("id_max_alone", [ID_MAX], [0]),
        (None, [], []),
        ("b_only_row", [], [7, 8, ID_MAX]),          # t >= rows_a
        ("b_only_row_empty", [], []),
        ("b_only_last", [], [0]),
    ], rows_a=11)


def _all_present() -> Case:
    rng = np.random.default_rng(11)
    pairs = []
    for t in range(40):
        a, _ = _split(rng, int(rng.integers(0, 30)), 0, 0)
        pairs.append((None, a, a[rng.random(len(a)) < 0.5]))
    pairs[7] = ("whole_row", pairs[7][1], pairs[7][1])
    return make_case("all_present", pairs)


def _slice_edges() -> Case:
    """Rows of S-1, S, S+1 and 2S+1 entries in A, in B and in the output, one after another, so
    that rows start, end and span slice edges of A's, B's and the row pointers' slicing."""
    rng = np.random.default_rng(12)
    pairs = []
    for L in (S - 1, S, S + 1, 2 * S + 1):
        a, b = _split(rng, L, 5, 2)
        pairs.append((f"a_{L}", a, b))
        a, b = _split(rng, 3, L, 1)
        pairs.append((f"b_{L}", a, b))
        a, b = _split(rng, L // 2 + 3, L - L // 2, 3)        # |A u B| = L: the union's output row
        pairs.append((f"out_union_{L}", a, b))
        a, b = _split(rng, L // 3, L - L // 3, L // 5)       # |A| + |B| = L: the multiset's output row
        pairs.append((f"out_multiset_{L}", a, b))
        pairs.append((None, [], []))
    return make_case("slice_edges", pairs)


def _star() -> Case:
    rng = np.random.default_rng(13)
    a, b = _split(rng, 4097, 1025, 512, hi=50_000)
    pairs = [(None, [t], [t + 1]) for t in range(5)] + [("star", a, b)] + [(None, [t], []) for t in range(5)]
    return make_case("star", pairs)


def _random(seed=14, rows=3000, rows_a=2500) -> Case:
    rng = np.random.default_rng(seed)
    pairs = []
    for t in range(rows):
        n_a = int(rng.integers(0, 12)) * int(rng.random() < 0.6) if t < rows_a else 0
        n_b = int(rng.integers(0, 6)) * int(rng.random() < 0.5)
        n_both = int(rng.integers(0, min(n_a, n_b) + 1))
        a, b = _split(rng, n_a, n_b, n_both, hi=5000)
        pairs.append((None, a, b))
    return make_case("random", pairs, rows_a=rows_a)


def _empties() -> List[Case]:
    some = [(None, [1, 2], []), (None, [], []), (None, [0, 9], [])]
    return [make_case("nnz_b_zero", some),
            make_case("nnz_a_zero", [(None, [], b) for _, b, _ in some] + [(None, [], [4])], rows_a=2),
            make_case("rows_a_zero", [(None, [], [3, 4]), (None, [], []), (None, [], [1])], rows_a=0),
            make_case("nothing", [(None, [], [])] * 3, rows_a=1)]


def _runs() -> Case:
    """Multiset only: runs of equal ids inside A, inside B and across both."""
    c = make_case("runs", [
        ("run_in_a", [5, 5, 5, 7], [6]),
        ("run_in_b", [6], [5, 5, 7, 7, 7]),
        ("run_across", [5, 5, 7, 9, 9], [5, 5, 7, 7, 9]),
        ("all_equal", [4] * 9, [4] * 7),
        ("long_run", [8] * (S + 3), [8] * (S - 1)),
        (None, [], []),
        ("run_new_row", [], [2, 2, 2]),
    ], rows_a=6, modes=(0,))
    c.status = {1: UNSORTED_A | UNSORTED_B}        # (as a set union both sides break the strict order)
    return c


def _float_bits() -> Case:
    c = make_case("float_bits", [("bits", [1, 2, 3, 4], [2, 2, 3, 9])], modes=(0,), status={1: UNSORTED_B})
    c.pay_a[:] = [NEG_ZERO, 0, NAN_A, 0x3F800000]
    c.pay_b[:] = [NAN_B, NEG_ZERO, 0x7F800000, 1]          # (NaN, -0.0, +inf, a denormal)
    return c


def _unordered() -> List[Case]:
    good = [5, 6, 9]
    out = []
    for side in "ab":
        dup = make_case(f"duplicate_in_{side}", [(None, [1], [2]), ("bad", [5, 5, 9] if side == "a" else good,
                                                                   [5, 5, 9] if side == "b" else good)])
        dup.modes, dup.status = (0,), {1: UNSORTED_A if side == "a" else UNSORTED_B}     # fine as a multiset
        desc = make_case(f"descending_in_{side}", [("bad", [9, 5] if side == "a" else good,
                                                    [9, 5] if side == "b" else good), (None, [1], [0])])
        desc.modes = ()
        desc.status = {m: UNSORTED_A if side == "a" else UNSORTED_B for m in (0, 1)}
        out += [dup, desc]
    both = make_case("descending_in_both", [(None, [3, 4], [1]), ("bad", [2, 1], [7, 7, 6])])
    both.modes, both.status = (), {0: UNSORTED_A | UNSORTED_B, 1: UNSORTED_A | UNSORTED_B}
    # the last id of a row above the first of the next is no violation
    edge = make_case("descending_across_rows", [(None, [8, 9], [7, 9]), (None, [1, 2], [0, 2])])
    return out + [both, edge]


def all_cases() -> List[Case]:
    return [_shapes(), _all_present(), _slice_edges(), _star(), _random()] + _empties() + \
        [_runs(), _float_bits()] + _unordered()


_CACHE: Dict[str, Case] = {}


def cases() -> Dict[str, Case]:
    """Built once and shared (read-only)."""
    if not _CACHE:
        _CACHE.update({c.name: c for c in all_cases()})
    return _CACHE


def expected(case: Case, mode: int):
    """csr_merge_ref of a case, computed once per (case, mode)."""
    key = f"{case.name}/{mode}"
    if key not in _EXPECTED:
        _EXPECTED[key] = csr_merge_ref(case.rowptr_a, case.ids_a, case.pay_a if mode == 0 else None, case.rowptr_b,
                                       case.ids_b, case.pay_b if mode == 0 else None, mode)
    return _EXPECTED[key]


_EXPECTED: Dict[str, tuple] = {}

CASE_NAMES = ["shapes", "all_present", "slice_edges", "star", "random", "nnz_b_zero", "nnz_a_zero", "rows_a_zero",
              "nothing", "runs", "float_bits", "duplicate_in_a", "descending_in_a", "duplicate_in_b",
              "descending_in_b", "descending_in_both", "descending_across_rows"]


# --------------------------------------------------------------------------- the batch, canonicalised
def canonical_relations(subject, obj, n_entities):
    """What append_graph makes of a relation batch, in numpy: both directions, no self-loops, unique,
    sorted by (src, dst) -> (rowptr [n_entities + 1], dst int32)."""
    s, o = np.asarray(subject, dtype=np.int64), np.asarray(obj, dtype=np.int64)
    real = s != o
    s, o = s[real], o[real]
    key = np.unique(np.concatenate([s * n_entities + o, o * n_entities + s]))
    src, dst = key // n_entities, key % n_entities
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n_entities))]).astype(np.int64)
    return rowptr, dst.astype(np.int32)


def canonical_mentions(entity, chunk, conf, n_entities):
    """What append_mentions makes of a batch: sorted by (entity, chunk), stably -> (rowptr, chunk int32, conf f32)."""
    e, c = np.asarray(entity, dtype=np.int64), np.asarray(chunk, dtype=np.int64)
    order = np.lexsort((c, e))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(e, minlength=n_entities))]).astype(np.int64)
    return rowptr, c[order].astype(np.int32), np.asarray(conf, dtype=np.float32)[order]


# --------------------------------------------------------------------------- table rows, in ingest steps
NAMES_OLD = ["Acme Corp", "São Paulo", "İstanbul Büyükşehir", "acme robotics", "Zeta"]


def entity_name(e: int) -> str:
    return NAMES_OLD[e] if e < len(NAMES_OLD) else f"Entity {e} ünit"


def graph_rows(seed: int, n_chunks: int, n_ent: int, n_rel: int, n_men: int, ent_base: int = 0, chunk_lo: int = 0,
               ent_lo: int = 0):
    """Random reference-shaped rows: entities ent_base .. ent_base + n_ent - 1; relations and
    mentions over entities ent_lo .. ent_base + n_ent - 1 and chunks chunk_lo .. n_chunks - 1, with
    self-loops, repeated relations (both orientations) and repeated (entity, chunk) mentions."""
    rng = np.random.default_rng(seed)
    hi = ent_base + n_ent
    ents = [{"id": f"e{e}", "name": entity_name(e), "canonical_name": entity_name(e).lower()}
            for e in range(ent_base, hi)]
    s, o = rng.integers(ent_lo, hi, n_rel), rng.integers(ent_lo, hi, n_rel)
    if n_rel >= 8:
        s[1], o[1] = o[0], s[0]          # the reverse of relation 0
        s[2], o[2] = s[0], o[0]          # a repeat
        o[3] = s[3]                      # a self-loop
    rels = [{"id": f"r{seed}_{i}", "subject_entity_id": f"e{a}", "object_entity_id": f"e{b}", "confidence": 0.5}
            for i, (a, b) in enumerate(zip(s.tolist(), o.tolist()))]
    me, mc = rng.integers(ent_lo, hi, n_men), rng.integers(chunk_lo, n_chunks, n_men)
    if n_men >= 4:
        me[1], mc[1] = me[0], mc[0]      # the same (entity, chunk) twice: both kept, in row order
    mens = [{"id": f"m{seed}_{i}", "entity_id": f"e{e}", "child_chunk_id": f"c{c}",
             **({} if i % 5 == 0 else {"confidence": float(np.float32(rng.random()))})}
            for i, (e, c) in enumerate(zip(me.tolist(), mc.tolist()))]
    return ents, rels, mens


def child_rows(lo: int, hi: int, dim: int = 0, seed: int = 5):
    rng = np.random.default_rng(seed + lo)
    rows = []
    for i in range(lo, hi):
        r = {"id": f"c{i}", "parent_id": f"p{i // 4}", "document_id": f"d{i // 16}", "text": f"chunk {i} w{i % 7} w{i % 3}",
             "page": 1, "modality": "text"}
        if dim:
            r["embedding_1024"] = rng.standard_normal(dim).astype(np.float32).tolist()
        rows.append(r)
    return rows
