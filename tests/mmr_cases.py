"""Inputs and the numpy restatement of the diversified top-k tests (tests/test_mmr_host.py, tests/test_gpu_mmr.py).
Pure numpy: nothing here needs a GPU.

The contract (include/thr_hip_diversify.h), for one query over ids[0 .. n), scores[0 .. n) (float64), cnt:
  candidates   positions p < cnt with a finite score, |score| <= 1e300; m of them
  has_row(p)   id_base <= ids[p] < id_base + n_docs and dnorm[ids[p] - id_base] > 0; a candidate without a row stays
               selectable and has similarity 0.0 to everything
  rel(p)       1.0 when hi == lo (the candidates' extreme scores), else (scores[p] - lo) / (hi - lo)
  sim(a, b)    seq_dot_f64(row_a, row_b) / (dnorm_a * dnorm_b): the sequential float64 sum in dimension order
  selection    greedy, min(m, top_k) steps; value = lam * rel at step 0, lam * rel - (1.0 - lam) * pen afterwards,
               pen the plain maximum of sim to the selected (``if sim > pen: pen = sim`` from -inf); the greatest
               value wins, ties go to the lowest position
  outputs      ids, original scores, positions, values in selection order; padding -1 / -inf / -1 / -inf

``mmr_reference`` restates it for a whole batch at once (every numpy operation below is one IEEE float64 rounding
per element); its keyword flags are the WRONG variants the host test shows each to change a named case.
"""
import functools
from typing import NamedTuple, Optional

import numpy as np

from oracle import thr_oracle as O

SCORE_MAX = 1e300
BIG_BASE = (1 << 40) + 12345
NS = (1, 2, 63, 64, 65, 100, 512)
DIMS = (4, 36, 768, 1024, 4000, 4096)


class Case(NamedTuple):
    name: str
    ids: np.ndarray                 # int64 [nq, n]
    scores: np.ndarray              # float64 [nq, n]
    counts: Optional[np.ndarray]    # int32 [nq] or None
    docs: np.ndarray                # float32 [n_docs, dim]
    dnorm: np.ndarray               # float64 [n_docs]
    id_base: int
    lam: float
    top_k: int


class Selection(NamedTuple):
    ids: np.ndarray                 # int64 [nq, top_k]
    scores: np.ndarray              # float64 [nq, top_k]
    pos: np.ndarray                 # int32 [nq, top_k]
    mmr: np.ndarray                 # float64 [nq, top_k]
    counts: np.ndarray              # int32 [nq]


# ------------------------------------------------------------------------------------------ the restatement
def seq_dot_batch(R: np.ndarray, S: np.ndarray) -> np.ndarray:
    """R float32 [nq, n, dim], S float32 [nq, dim] -> float64 [nq, n]: oracle.thr_oracle.seq_dot_f64 of each query's
    rows against its vector (the same loop, one query axis more)."""
    acc = np.zeros(R.shape[:2], dtype=np.float64)
    S64 = S.astype(np.float64)
    for i in range(R.shape[2]):
        acc += R[:, :, i].astype(np.float64) * S64[:, i][:, None]
    return acc


def mmr_reference(ids, scores, counts, docs, dnorm, id_base, lam, top_k, *, clip_pen=False, ties_high=False,
                  pairwise=False, reverse_sum=False, raw_rel=False, skip_rowless=False) -> Selection:
    ids = np.asarray(ids, dtype=np.int64)
    scores = np.asarray(scores, dtype=np.float64)
    docs = np.asarray(docs, dtype=np.float32)
    dnorm = np.asarray(dnorm, dtype=np.float64)
    nq, n = ids.shape
    n_docs = docs.shape[0]
    cnt = np.full(nq, n) if counts is None else np.clip(np.asarray(counts, dtype=np.int64), 0, n)
    with np.errstate(all="ignore"):
        cand = (np.arange(n)[None, :] < cnt[:, None]) & np.isfinite(scores) & (np.abs(scores) <= SCORE_MAX)
        local = ids >= id_base
        row = np.where(local, ids - np.where(local, id_base, 0), 0)
        has = local & (row < n_docs)
        row = np.where(has, row, 0)
        has &= dnorm[row] > 0
        if skip_rowless:
            cand &= has
        lo = np.where(cand, scores, np.inf).min(axis=1)
        hi = np.where(cand, scores, -np.inf).max(axis=1)
        rel = np.where((hi == lo)[:, None], 1.0, (scores - lo[:, None]) / (hi - lo)[:, None])
        if raw_rel:
            rel = scores.copy()
        rel = np.where(cand, rel, 0.0)
        steps = np.minimum(cand.sum(axis=1), top_k)
        R = docs[row]                                   # [nq, n, dim]; rows of positions without one are masked below
        nrm = dnorm[row]
        one_minus_lam = 1.0 - lam
        out = Selection(np.full((nq, top_k), -1, np.int64), np.full((nq, top_k), -np.inf), np.full((nq, top_k), -1, np.int32),
                        np.full((nq, top_k), -np.inf), steps.astype(np.int32))
        open_ = cand.copy()
        pen = np.full((nq, n), -np.inf)
        qs = np.arange(nq)
        for t in range(int(steps.max()) if nq else 0):
            shown = np.maximum(pen, 0.0) if clip_pen else pen
            value = lam * rel if t == 0 else lam * rel - one_minus_lam * shown
            v = np.where(open_, value, -np.inf)
            best = n - 1 - np.argmax(v[:, ::-1], axis=1) if ties_high else np.argmax(v, axis=1)
            live = t < steps
            out.ids[live, t] = ids[qs, best][live]
            out.scores[live, t] = scores[qs, best][live]
            out.pos[live, t] = best[live]
            out.mmr[live, t] = value[qs, best][live]
            open_[qs[live], best[live]] = False
            if t + 1 >= top_k:
                break
            S = R[qs, best]
            if pairwise:
                dot = (R.astype(np.float64) * S.astype(np.float64)[:, None, :]).sum(axis=-1)
            elif reverse_sum:
                dot = seq_dot_batch(R[:, :, ::-1], S[:, ::-1])
            else:
                dot = seq_dot_batch(R, S)
            sim = dot / (nrm * nrm[qs, best][:, None])
            sim = np.where(has & has[qs, best][:, None], sim, 0.0)
            pen = np.where(sim > pen, sim, pen)
    return out


def reference(case: Case, **variant) -> Selection:
    return mmr_reference(case.ids, case.scores, case.counts, case.docs, case.dnorm, case.id_base, case.lam, case.top_k,
                         **variant)


@functools.lru_cache(maxsize=None)
def expected(name: str) -> Selection:
    """The restatement of a built case, computed once and shared (treat as read-only)."""
    return reference(case(name))


# ------------------------------------------------------------------------------------------ builders
def _rng(*seed):
    return np.random.Generator(np.random.PCG64([20260, *seed]))


def _table(rng, n_docs, dim):
    docs = rng.standard_normal((n_docs, dim)).astype(np.float32)
    return docs, O.doc_norms_f64(docs)


def _descending(rng, nq, n):
    return -np.sort(-rng.random((nq, n)), axis=1)


def _mk(name, ids, scores, counts, docs, dnorm, id_base, lam, top_k) -> Case:
    return Case(name, np.ascontiguousarray(ids, dtype=np.int64), np.ascontiguousarray(scores, dtype=np.float64),
                None if counts is None else np.ascontiguousarray(counts, dtype=np.int32),
                np.ascontiguousarray(docs, dtype=np.float32), np.ascontiguousarray(dnorm, dtype=np.float64),
                int(id_base), float(lam), int(top_k))


CLUSTERS, MEMBERS = 5, 4


def duplicates_case() -> Case:
    """CLUSTERS clusters of MEMBERS rows under distinct ids: member 0 the base, member 1 the same bytes, members 2, 3
    the base plus noise of 1e-3.  The bases are nearly orthogonal; member j of cluster c sits at position
    j * CLUSTERS + c, so every cluster has a member among the first CLUSTERS positions."""
    rng, dim = _rng(1), 36
    base = np.zeros((CLUSTERS, dim), np.float32)
    for c in range(CLUSTERS):
        base[c, 7 * c:7 * c + 3] = (1.0, 0.5, -0.25)
    base += rng.standard_normal(base.shape).astype(np.float32) * np.float32(0.01)
    docs = np.empty((CLUSTERS * MEMBERS, dim), np.float32)
    for c in range(CLUSTERS):
        for j in range(MEMBERS):
            noise = rng.standard_normal(dim).astype(np.float32) * np.float32(1e-3) if j >= 2 else 0
            docs[c * MEMBERS + j] = base[c] + noise
    pos_row = [c * MEMBERS + j for j in range(MEMBERS) for c in range(CLUSTERS)]
    ids = 100 + np.array([pos_row])
    scores = np.linspace(1.0, 0.5, CLUSTERS * MEMBERS)[None, :]
    return _mk("duplicates", ids, scores, None, docs, O.doc_norms_f64(docs), 100, 0.5, 10)


def cluster_of(case: Case, pos):
    return (case.ids[0, pos] - case.id_base) // MEMBERS


def lam_case(lam: float) -> Case:
    rng = _rng(2)
    docs, dn = _table(rng, 300, 36)
    ids = np.stack([rng.choice(300, 100, replace=False) for _ in range(3)])
    return _mk(f"lam-{lam}", ids, _descending(rng, 3, 100), None, docs, dn, 0, lam, 10)


TIE_BLOCKS = ((0, 3, 1.0), (3, 71, 0.9), (71, 500, 0.85), (500, 512, 0.5))
TIE_SPLIT = 71          # base rows 0 .. 5 sit before this position, base rows 6 .. 11 from it on


def ties_case() -> Case:
    """512 positions in four blocks of equal scores; 512 rows that are copies of 12 small-integer base rows, under
    distinct ids: byte-identical rows with identical scores at distant positions, so exact ties in value.  Six of
    the base rows appear only from position TIE_SPLIT on: fresh rows there are worth selecting, and their copies
    lie on both sides of 256 as the copies of the first six lie on both sides of 64."""
    rng = _rng(3)
    base = np.array([[3, 0, 0, 1], [0, 3, 1, 0], [0, -1, 3, 0], [1, 0, 0, -3], [2, 2, -2, 2], [-2, 2, 2, 2],
                     [-3, 1, 0, 0], [0, -3, 0, 1], [1, 0, -3, 0], [0, 1, 0, 3], [2, -2, 2, 2], [2, 2, 2, -2]], np.float32)
    which = np.concatenate([rng.integers(0, 6, size=TIE_SPLIT), rng.integers(6, 12, size=512 - TIE_SPLIT)])
    docs = np.empty((512, 4), np.float32)
    ids = rng.permutation(512)[None, :]
    docs[ids[0]] = base[which]
    scores = np.empty((1, 512))
    for lo, hi, s in TIE_BLOCKS:
        scores[0, lo:hi] = s
    return _mk("exact-ties", ids, scores, None, docs, O.doc_norms_f64(docs), 0, 0.5, 24)


def negative_case() -> Case:
    """Rows in opposite pairs (row 2i + 1 = -row 2i): the opposite of a selected row has sim -1, pen goes negative."""
    rng = _rng(4)
    half = rng.integers(-4, 5, size=(6, 4)).astype(np.float32)
    half[np.all(half == 0, axis=1)] = 2
    docs = np.empty((12, 4), np.float32)
    docs[0::2], docs[1::2] = half, -half
    ids = np.array([[0, 2, 4, 1, 6, 3, 8, 5, 10, 7, 9, 11]])
    return _mk("negative-sims", ids, np.linspace(1.0, 0.2, 12)[None, :], None, docs, O.doc_norms_f64(docs), 0, 0.5, 6)


ORDER_DIM, ORDER_N = 768, 12


def order_case() -> Case:
    """Position 0 holds S, a constant row, with the best score; the last two positions hold B and A = B reversed with
    the lowest score (rel 0) and one shared norm: their dot products with S have the same real value and differ only
    by the order of the float64 sum.  A's entries are all negative, so A and B have the least similarity to S by far
    and step 1 chooses between them on those last bits alone: value = 0 - 0.5 * sim.  The seed is the first for which
    the sequential sum prefers A (the HIGHER position: no tie can favour it) and the pairwise sum does not."""
    for seed in range(400):
        rng = _rng(5, seed)
        a = -np.abs(rng.standard_normal(ORDER_DIM)).astype(np.float32) * np.exp(rng.standard_normal(ORDER_DIM)).astype(np.float32)
        s = np.full(ORDER_DIM, 0.7, np.float32)
        fill = rng.standard_normal((ORDER_N - 3, ORDER_DIM)).astype(np.float32)
        docs = np.concatenate([s[None], fill, a[::-1][None], a[None]])       # B = row n - 2, A = row n - 1
        dn = O.doc_norms_f64(docs)
        dn[ORDER_N - 2] = dn[ORDER_N - 1]
        seq = O.seq_dot_f64(docs[-2:], s)
        pw = (docs[-2:].astype(np.float64) * s.astype(np.float64)).sum(axis=-1)
        if seq[1] < seq[0] and pw[1] >= pw[0]:
            ids = 50 + np.arange(ORDER_N)[None, :]
            scores = np.concatenate([[1.0], np.linspace(0.2, 0.11, ORDER_N - 3), [0.1, 0.1]])[None, :]
            return _mk("order-sensitive", ids, scores, None, docs, dn, 50, 0.5, 2)
    raise AssertionError("no seed separates the sequential from the pairwise sum")


def rowless_case() -> Case:
    """id_base 1000 over 50 rows; rows 3, 17 are all zeros (dnorm 0).  Negative ids, ids below the base, at and past
    base + n_docs and the two empty rows stand between ordinary candidates, all inside cnt."""
    rng = _rng(6)
    docs, _ = _table(rng, 50, 8)
    docs[[3, 17]] = 0
    ids = np.array([[1005, -1, 1010, 999, 1003, 1020, 1050, 5, 1017, 1030, -7, 1051, 1001, 1049, 0, 1000,
                     1044, -(1 << 40), 1002, 1 << 50, 1011, 1012, 1013, 1014]])
    return _mk("rowless", ids, _descending(rng, 1, 24), np.array([24]), docs, O.doc_norms_f64(docs), 1000, 0.5, 24)


def duplicate_ids_case() -> Case:
    rng = _rng(7)
    docs, dn = _table(rng, 20, 36)
    ids = np.array([[4, 9, 4, 2, 9, 9, 1, 4, 0, 2, 13, 13, 7, 1, 4, 19]])
    return _mk("duplicate-ids", ids, _descending(rng, 1, 16), None, docs, dn, 0, 0.5, 16)


UNUSABLE = {2: np.nan, 5: np.inf, 6: -np.inf, 9: 1e301, 12: -1e301}


def unusable_case() -> Case:
    rng = _rng(8)
    docs, dn = _table(rng, 40, 36)
    ids = rng.choice(40, 16, replace=False)[None, :]
    scores = _descending(rng, 1, 16)
    for p, v in UNUSABLE.items():
        scores[0, p] = v
    scores[0, 0], scores[0, 15] = 1e300, -1e300        # the extremes that still count
    return _mk("unusable-scores", ids, scores, None, docs, dn, 0, 0.5, 16)


def all_equal_case() -> Case:
    rng = _rng(9)
    docs, dn = _table(rng, 80, 36)
    ids = np.stack([rng.choice(80, 65, replace=False) for _ in range(2)])
    return _mk("all-equal", ids, np.full((2, 65), 0.25), None, docs, dn, 0, 0.5, 10)


def offset_case() -> Case:
    """Scores in a narrow band far from zero (100.0 .. 100.5): min-max normalisation spreads them over [0, 1]; taken
    raw they would all weigh 100 and the order among them would hardly count."""
    rng = _rng(14)
    docs, dn = _table(rng, 60, 36)
    ids = rng.choice(60, 30, replace=False)[None, :]
    return _mk("offset-scores", ids, np.linspace(100.5, 100.0, 30)[None, :], None, docs, dn, 0, 0.5, 10)


COUNTS = (0, 1, 4, 5, 12, 15, -3, 7)        # top_k 5, n 12: 0, 1, top_k - 1, top_k, n, above n, negative, between


def counts_case(null: bool) -> Case:
    rng = _rng(10)
    docs, dn = _table(rng, 40, 36)
    nq = len(COUNTS)
    ids = np.stack([rng.choice(40, 12, replace=False) for _ in range(nq)])
    return _mk("counts-null" if null else "counts", ids, _descending(rng, nq, 12), None if null else np.array(COUNTS),
               docs, dn, 0, 0.5, 5)


# (n, top_k, dim, n_queries, id_base): every n with top_k 1, 10 (where it fits) and n; every dim; both bases
SHAPES = (
    (1, 1, 4, 3, 0), (2, 1, 36, 3, BIG_BASE), (2, 2, 4, 2, 0),
    (63, 1, 1024, 1, 0), (63, 10, 36, 2, 0), (63, 63, 4, 2, BIG_BASE),
    (64, 1, 768, 2, 0), (64, 10, 1024, 1, BIG_BASE), (64, 64, 36, 2, 0),
    (65, 1, 4, 2, 0), (65, 10, 4000, 1, 0), (65, 65, 36, 2, BIG_BASE),
    (100, 1, 1024, 1, 0), (100, 10, 768, 2, BIG_BASE), (100, 100, 36, 1, 0),
    (512, 1, 4, 1, 0), (512, 10, 36, 2, BIG_BASE), (512, 512, 64, 1, 0),
    (40, 10, 4096, 1, BIG_BASE),
    (512, 3, 4096, 1, 0),           # the largest LDS image: eight staging tiles beside a 4096-dim row
)


def shape_name(shape) -> str:
    n, top_k, dim, nq, base = shape
    return f"shape-n{n}-k{top_k}-d{dim}-{'big' if base else 'zero'}"


def shape_case(shape) -> Case:
    """Random rows and descending scores; one position in ten is rowless (-1, below the base, past the table)."""
    n, top_k, dim, nq, base = shape
    rng = _rng(11, n, top_k, dim)
    n_docs = 2 * n + 5
    docs, dn = _table(rng, n_docs, dim)
    ids = base + np.stack([rng.choice(n_docs, n, replace=False) for _ in range(nq)]).astype(np.int64)
    odd = rng.random((nq, n)) < 0.1
    ids[odd] = rng.choice(np.array([-1, base - 1, base + n_docs]), int(odd.sum()))
    return _mk(shape_name(shape), ids, _descending(rng, nq, n), None, docs, dn, base, 0.5, top_k)


MANY_QUERIES = 65600


def many_queries_case() -> Case:
    rng = _rng(12)
    docs = rng.integers(-3, 4, size=(16, 4)).astype(np.float32)
    ids = rng.integers(-1, 17, size=(MANY_QUERIES, 4))
    counts = rng.integers(0, 5, size=MANY_QUERIES)
    return _mk("many-queries", ids, _descending(rng, MANY_QUERIES, 4), counts, docs, O.doc_norms_f64(docs), 0, 0.5, 2)


def real_case() -> Case:
    """64 queries x 100 candidates x 768 dims, top_k 10, drawn from 3 000 rows of the synthetic corpus."""
    from triple_hybrid_rag_amd import synth
    rng = _rng(13)
    docs = synth.dense_rows(0, 3000, 768)
    ids = np.stack([rng.choice(3000, 100, replace=False) for _ in range(64)])
    return _mk("real", ids, _descending(rng, 64, 100), None, docs, O.doc_norms_f64(docs), 0, 0.5, 10)


_BUILDERS = {"duplicates": duplicates_case, "exact-ties": ties_case, "negative-sims": negative_case,
             "order-sensitive": order_case, "rowless": rowless_case, "duplicate-ids": duplicate_ids_case,
             "unusable-scores": unusable_case, "all-equal": all_equal_case, "offset-scores": offset_case,
             "counts": lambda: counts_case(False), "counts-null": lambda: counts_case(True),
             "many-queries": many_queries_case, "real": real_case}
LAMS = (1.0, 0.0, 0.5, 0.999)
_BUILDERS.update({f"lam-{lam}": functools.partial(lam_case, lam) for lam in LAMS})
_BUILDERS.update({shape_name(s): functools.partial(shape_case, s) for s in SHAPES})
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def case(name: str) -> Case:
    c = _BUILDERS[name]()
    assert c.name == name
    return c
