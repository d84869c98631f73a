"""Inputs, restatements and bounds of the child -> parent expansion tests (tests/test_parent_host.py,
tests/test_gpu_parent.py).  Pure numpy: nothing here needs a GPU.

The contract (include/thr_hip_parent.h).  P int32 [n_docs]: P[r] the parent number of local row r, or -1.
family(r) = {r} when P[r] < 0, else every row r' with P[r'] == P[r], ascending.  The parent score of (q, r) is
oracle.thr_oracle.maxsim_scores of the query against the CONCATENATION of the family's token blocks in row order
(``parent_reference``: float64, the oracle unchanged); over the FP8 store, against the dequantised blocks.  The
bound of a score is maxsim_cases.error_bound (maxsim_fp8_cases.error_bound_fp8) applied to that concatenated
block.  The groups of a fused row are restated in ``groups_reference``.
"""
import numpy as np

import maxsim_cases as MC
import maxsim_fp8_cases as F8
from oracle import thr_oracle as O


# ------------------------------------------------------------------------------------------ the definitions
def family(P, r: int) -> list:
    P = np.asarray(P)
    if P[r] < 0:
        return [int(r)]
    return [int(x) for x in np.nonzero(P == P[r])[0]]


def parent_csr(P):
    """-> (rowptr int64 [n_parents + 1], child int32 [nnz]) or None when no row has a parent."""
    P = np.asarray(P)
    if not np.any(P >= 0):
        return None
    n_parents = int(P.max()) + 1
    child = [r for p in range(n_parents) for r in np.nonzero(P == p)[0]]
    rowptr = np.concatenate([[0], np.cumsum([int((P == p).sum()) for p in range(n_parents)])])
    return rowptr.astype(np.int64), np.asarray(child, dtype=np.int32)


def groups_reference(ids, counts, P, id_base: int = 0):
    """ids int64 [nq, n], counts [nq] or None -> (leader, slot int32 [nq, n]; uniq_ids int64 [nq, n]; n_uniq int32 [nq]),
    word for word the definition: position p's key is P[ids[p] - id_base] when the id is local and that value is
    >= 0, else its own; leader = lowest position with the key; the unique list = the leaders in position order."""
    ids, P = np.asarray(ids, dtype=np.int64), np.asarray(P)
    nq, n = ids.shape
    leader = np.full((nq, n), -1, np.int32)
    slot = np.full((nq, n), -1, np.int32)
    uniq = np.full((nq, n), -1, np.int64)
    n_uniq = np.zeros(nq, np.int32)
    for q in range(nq):
        cnt = n if counts is None else min(max(int(counts[q]), 0), n)
        first, order = {}, []
        for p in range(cnt):
            g = int(ids[q, p])
            row = g - id_base if g >= 0 else -1
            key = ("own", p)
            if 0 <= row < len(P) and P[row] >= 0:
                key = ("parent", int(P[row]))
            if key not in first:
                first[key] = p
                order.append(p)
            leader[q, p] = first[key]
            slot[q, p] = order.index(first[key])
        uniq[q, :len(order)] = ids[q, order]
        n_uniq[q] = len(order)
    return leader, slot, uniq, n_uniq


def _local(cand, n_docs: int, id_base: int) -> np.ndarray:
    return MC.local_candidates(cand, n_docs, id_base)


def _per_family(qtok, P, cand, id_base, n_docs, score_one):
    """score_one(q, rows of the family) for every valid (q, candidate), computed once per (q, family)."""
    loc = _local(cand, n_docs, id_base)
    out = np.full(loc.shape, -np.inf, dtype=np.float64)
    seen = {}
    for q in range(loc.shape[0]):
        for c in range(loc.shape[1]):
            r = int(loc[q, c])
            if r < 0:
                continue
            fam = tuple(family(P, r))
            if (q, fam) not in seen:
                seen[(q, fam)] = score_one(q, list(fam))
            out[q, c] = seen[(q, fam)]
    return out


def parent_reference(qtok, dtok, P, cand, id_base: int = 0) -> np.ndarray:
    """float64 parent scores: the oracle's MaxSim of the query against the concatenated family block; -inf where
    the device owes -inf (negative, out of range, another shard).  ``dtok`` float16 (or the float64 dequantised
    tokens of an FP8 store)."""
    one = np.zeros((1, 1), dtype=np.int64)

    def score(q, fam):
        block = np.concatenate([dtok[r] for r in fam], axis=0)
        return O.maxsim_scores(qtok[q:q + 1], block[None], one)[0, 0]
    return _per_family(qtok, P, cand, id_base, len(dtok), score)


def parent_reference_fp8(qtok, codes, scales, P, cand, id_base: int = 0) -> np.ndarray:
    return parent_reference(qtok, F8.dequantise(codes, scales), P, cand, id_base)


def error_bound_parent(qtok, dtok, P, cand, id_base: int = 0) -> np.ndarray:
    """maxsim_cases.error_bound of the concatenated family block, per score; -inf scores get 0."""
    one = np.zeros((1, 1), dtype=np.int64)

    def bound(q, fam):
        block = np.concatenate([dtok[r] for r in fam], axis=0)
        return MC.error_bound(qtok[q:q + 1], block[None], one)[0, 0]
    out = _per_family(qtok, P, cand, id_base, len(dtok), bound)
    return np.where(np.isfinite(out), out, 0.0)


def error_bound_parent_fp8(qtok, codes, scales, P, cand, id_base: int = 0) -> np.ndarray:
    """maxsim_fp8_cases.error_bound_fp8 of the concatenated family block (codes row-major)."""
    one = np.zeros((1, 1), dtype=np.int64)

    def bound(q, fam):
        c = np.concatenate([codes[r] for r in fam], axis=0)
        s = np.concatenate([scales[r] for r in fam], axis=0)
        return F8.error_bound_fp8(qtok[q:q + 1], c[None], s[None], one)[0, 0]
    out = _per_family(qtok, P, cand, id_base, len(codes), bound)
    return np.where(np.isfinite(out), out, 0.0)


def collapse_reference(ids_row, cnt: int, P, id_base: int = 0):
    """The leaders of one fused row -> (their positions, their ids): what retrieve_batch(parents="collapse") keeps."""
    leader, _, uniq, n = groups_reference(np.asarray(ids_row)[None], [cnt], P, id_base)
    pos = [p for p in range(cnt) if leader[0, p] == p]
    return pos, [int(g) for g in uniq[0, :n[0]]]


# ------------------------------------------------------------------------------------------ group cases
GROUP_WIDTHS = (1, 63, 64, 65, 255, 256, 257, 512)


def group_cases():
    """[(name, ids int64 [nq, n], counts int32 [nq] or None, P int32 [n_docs], id_base)]"""
    rng = np.random.default_rng(2024)
    out = []
    for n in GROUP_WIDTHS:
        n_docs = 700
        P = rng.integers(-1, max(2, n // 3), size=n_docs).astype(np.int32)
        ids = np.stack([rng.permutation(n_docs)[:n] for _ in range(3)]).astype(np.int64)
        out.append((f"random-n{n}", ids, None, P, 0))
        counts = np.array([0, 1, max(n - 1, 0), n, n + 5, -3], dtype=np.int32)       # (beyond n / negative: clamped)
        ids6 = np.stack([rng.permutation(n_docs)[:n] for _ in range(6)]).astype(np.int64)
        out.append((f"counts-n{n}", ids6, counts, P, 0))
    n, n_docs = 512, 600
    ids = np.arange(n, dtype=np.int64)[None]
    out.append(("one-parent", ids, None, np.full(n_docs, 4, np.int32), 0))
    out.append(("all-distinct", ids, None, np.arange(n_docs, dtype=np.int32), 0))
    out.append(("all-none", ids, None, np.full(n_docs, -1, np.int32), 0))
    P = np.arange(n_docs, dtype=np.int32)
    P[511] = P[0]          # a group at positions 0 and 511
    P[64] = P[63]          # across the wave edge 63 / 64
    P[256] = P[255]        # across 255 / 256
    P[300] = P[100] = P[7]
    out.append(("far-pairs", ids, None, P, 0))
    # negative ids and ids of other shards between valid ones, id_base != 0
    id_base, n_docs = 1000, 300
    P = rng.integers(-1, 20, size=n_docs).astype(np.int32)
    row = rng.permutation(n_docs)[:257].astype(np.int64) + id_base
    row[::5] = -1
    row[1::7] = rng.integers(0, id_base, size=len(row[1::7]))                 # below the shard
    row[2::11] = id_base + n_docs + rng.integers(0, 50, size=len(row[2::11]))  # above it
    row[3::13] = -7
    out.append(("foreign-ids", np.stack([row, row[::-1]]), np.array([257, 200], np.int32), P, id_base))
    # the same valid id twice in a row: one group
    out.append(("repeated-ids", np.array([[5, 9, 5, 9, 2, 5]], np.int64), None, np.array([-1] * 10, np.int32), 0))
    return out


def many_queries_case(nq: int = 65600, n: int = 4):
    rng = np.random.default_rng(5)
    P = rng.integers(-1, 6, size=40).astype(np.int32)
    return rng.integers(-2, 44, size=(nq, n)).astype(np.int64), rng.integers(0, n + 1, size=nq).astype(np.int32), P


# ------------------------------------------------------------------------------------------ scorer cases
def layout(kind: str, fanout: int, n_families: int = 3):
    """A parent column with ``n_families`` families of ``fanout`` rows -> P int32.
    'blocks': a family's rows contiguous; 'interleaved': row r belongs to family r % n_families (row 0 and the
    last row are in families); 'loner': as interleaved with a row without a parent between the families."""
    if kind == "blocks":
        return np.repeat(np.arange(n_families), fanout).astype(np.int32)
    P = np.tile(np.arange(n_families), fanout).astype(np.int32)
    if kind == "loner":
        P = np.insert(P, [1, len(P) // 2, len(P)], -1).astype(np.int32)
    else:
        assert kind == "interleaved"
    return P


PLANTS = ("last", "first", "middle")


def plant(dtok, qtok, P, which: str, fam_of_row: int = 0):
    """Plant the decisive token of family(fam_of_row): an all-ones document token (every other document element is
    at most 7/8 in magnitude) at the last token of the last child / the first token of the first child / token 5
    of a middle child, and make query token 0 of every query all ones -> (row, token) of the plant.  The query
    token's maximum is then tok_dim, reached at the plant alone."""
    fam = family(P, fam_of_row)
    row, tok = {"last": (fam[-1], dtok.shape[1] - 1), "first": (fam[0], 0), "middle": (fam[len(fam) // 2], 5)}[which]
    dtok[row, tok, :] = 1
    qtok[:, 0, :] = 1
    return row, tok


def exact_case(seed: int, tok_dim: int, q_tokens: int, d_tokens: int, fanout: int, kind: str = "interleaved",
               n_cand: int = 5, n_queries: int = 2, id_base: int = 0, which: str = "last", n_families: int = 3):
    """The exact family of maxsim_cases (multiples of 1/8; document elements in [-7/8, 7/8] so that a plant of
    ones decides) -> (qtok, dtok, P, cand int64 global ids [n_queries, n_cand], id_base, (plant row, token)).
    The candidates walk the rows (so siblings appear), with a -1, an id above the shard and one below it where
    n_cand has room."""
    rng = np.random.default_rng(seed)
    P = layout(kind, fanout, n_families)
    n_docs = len(P)
    q = MC.exact_tokens(rng, (n_queries, q_tokens, tok_dim))
    d = MC.exact_tokens(rng, (n_docs, d_tokens, tok_dim), lo=-7, hi=7)
    planted = plant(d, q, P, which)
    cand = np.stack([(np.arange(n_cand) * (1 + qi) + qi) % n_docs for qi in range(n_queries)]).astype(np.int64) + id_base
    cand[:, 0] = id_base                        # the planted family's row 0 is always asked for
    if n_cand >= 4:
        cand[0, 1] = -1
        cand[-1, 2] = id_base + n_docs          # one past the shard
        if id_base:
            cand[0, 3] = id_base - 1            # another shard's id
    return q, d, P, cand, id_base, planted


def without_plant(dtok, planted):
    d = dtok.copy()
    d[planted[0], planted[1], :] = 0
    return d


# (tok_dim, q_tokens, d_tokens, fanout, kind, n_cand, which): the matrix of the issue at tok_dim 32 and 128, one case
# for every other tok_dim of each list
def exact_matrix(fp8: bool):
    rows = []
    for td in (32, 128):
        for fan in (1, 2, 3, 4, 5, 33):
            rows.append((td, 32, 32, fan, "interleaved", 5, PLANTS[fan % 3]))
        for dt, fan in ((32, 1), (32, 3), (32, 2), (64, 1), (64, 3), (64, 2)):     # odd and even tile totals
            for qt in (32, 64, 128):
                rows.append((td, qt, dt, fan, "loner", 4, PLANTS[(fan + qt // 32) % 3]))
        rows.append((td, 32, 32, 4, "blocks", 100, "middle"))
        rows.append((td, 64, 32, 3, "loner", 1, "first"))
    rows.append((32, 32, 32, 257, "interleaved", 4, "last"))
    rows.append((32, 32, 32, 3, "interleaved", 512, "middle"))
    others = [t for t in (F8.TOK_DIMS if fp8 else MC.TOK_DIMS) if t not in (32, 128)]
    for td in others:
        rows.append((td, 64, 64, 3, "loner", 5, "last"))
    return rows
