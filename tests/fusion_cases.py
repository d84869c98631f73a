"""Built cases for the fusion tail: thr_rrf_fuse, thr_rrf_fuse_standalone (both flavours),
thr_fuse_post, thr_rerank_order and thr_merge_topk.  Pure numpy / Python: test_fusion_cases_host.py
asserts on the CPU that every builder really reaches the branch it names, test_gpu_fusion.py runs the
same rows on the device and compares bits with the oracle (oracle/thr_oracle.py).

Limits of the kernels, restated here as data about them (csrc/rrf.hip, csrc/dense_exact.hip):
128 ids per channel, 512 table slots, blocks of 128 threads = two waves of 64, 1024 candidates in the
ranked merge.  NaN is the one input class left out everywhere except as an INVALID merge entry: the
reference's ``sorted`` on NaN keys is not an order, so there is nothing to compare with.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import thr_oracle as O

MAXC = 128          # THR_RRF_MAX_PER_CHANNEL
SLOTS = 512         # RRF_SLOTS
WAVE = 64
MERGE_CAP = 1024    # EX_CAP
NAMES = ("lexical", "semantic", "graph")

# weight sets (lexical, semantic, graph); the two-channel flavour takes the first two as (a, b)
W_DEFAULT = (0.7, 0.8, 1.0)
W_EQUAL = (1.0, 1.0, 1.0)        # w_lex == w_sem (== w_graph): the exact ties of tie_cycles
W_ZERO_SEM = (0.7, 0.0, 1.0)     # ids seen only in the semantic channel score 0.0
W_NEGATIVE = (0.7, -0.5, 1.0)
W_ALL_ZERO = (0.0, 0.0, 0.0)
WEIGHT_SETS = {"default": W_DEFAULT, "equal": W_EQUAL, "zero_sem": W_ZERO_SEM,
               "negative": W_NEGATIVE, "all_zero": W_ALL_ZERO}
RRF_KS = (0, 1, 60)
RRF_K_MAX = 2 ** 31 - 1 - MAXC   # the largest rrf_k thr_rrf_fuse takes: k + rank stays an int


def cut(ids):
    """A channel ends at its first negative id (None stays None)."""
    if ids is None:
        return None
    out = []
    for i in ids:
        if i < 0:
            break
        out.append(int(i))
    return out


# ------------------------------------------------------------------------------------------ RRF
def hash_slot(i: int) -> int:
    """Start slot of an id in the one-channel shortcut's open-addressing table."""
    return (((i * 0x9E3779B97F4A7C15) % 2 ** 64) >> 40) & (SLOTS - 1)


def colliding_ids(n: int = MAXC, min_slot: int = 500):
    """n distinct ids that all start at ONE slot >= min_slot: a probe chain of length n that wraps
    past slot 511."""
    by = {}
    i = 1
    while True:
        s = hash_slot(i)
        if s >= min_slot:
            by.setdefault(s, []).append(i)
            if len(by[s]) == n:
                return by[s], s
        i += 1


def rrf_rows():
    """name -> (lexical, semantic, graph) raw id lists (an entry < 0 ends the list; at most 128
    wide).  One batched call takes all of them, -1 padded to width 128."""
    R = {}
    A = list(range(1000, 1000 + MAXC))
    B = list(range(2000, 2000 + MAXC))
    C = list(range(3000, 3000 + MAXC))
    # capacity: 384 sightings
    R["cap_disjoint"] = (A, B, C)
    # overlap
    R["overlap_same"] = (A, A, A)
    R["overlap_sem_reversed"] = (A, A[::-1], A)
    R["overlap_gra_rot1"] = (A, A, A[1:] + A[:1])
    # wave boundary: where the first sightings of the 2nd / 3rd channel fall
    R["wave_low"] = (A, B[:64] + A[:64], C[:64] + B[:64])          # new ids at 0..63 only
    R["wave_high"] = (A, A[:64] + B[:64], B[:64] + C[:64])         # new ids at 64..127 only
    R["wave_63_64"] = (A, A[:63] + B[:2] + A[65:], A[:63] + C[:2] + A[65:])   # new at {63, 64}
    R["wave_no_new"] = (A, A[::-1], A[5:] + C[:5])                 # nothing new in sem; base carries on
    R["wave_no_new_gra"] = (A[:100], B[:70] + A[:30], A[:50] + B[:50])   # nothing new in graph
    # duplicates inside a channel
    R["dup_ends"] = ([7] + A[:126] + [7], [8] + B[:125] + [7, 8], [7, 9, 9])
    R["dup_128"] = ([5] * MAXC, [5] * MAXC, [5, 6])
    R["b_only_twice"] = ([1, 2, 3], [9, 1, 9], [])
    # list ends
    R["interior_minus1"] = ([5, 6, -1, 7, 8], [7, 5, 9], [8, -1, 6])
    R["minus1_first"] = ([-1, 5, 6], [3, 4], [4, 5])
    R["negative_other"] = ([1, 2], [3, 4, -7, 9], [9, 1])
    R["ids_extreme"] = ([0, 2 ** 62], [2 ** 62, 0, 5], [5, 2 ** 62 - 1])
    R["width_1"] = ([4], [4], [6])
    R["width_37"] = (A[:37], B[:30] + A[:7], C[:37])
    R["all_empty"] = ([], [], [])
    # exact ties by commutativity (weights equal): triple j lives at ranks a = 2j+1, b = 2j+2 --
    # T1 at (lex a, sem b), T2 at (sem a, graph b), T3 at (graph a, lex b): the three sums are
    # x_a + x_b in one order or the other.  T1 and T3 are sighted in the lexical channel (positions
    # 2j, 2j+1), T2 in the semantic one at position 128 + j: every group straddles position 128.
    lex, sem, gra = [0] * MAXC, [0] * MAXC, [0] * MAXC
    for j in range(MAXC // 2):
        a, b = 2 * j, 2 * j + 1
        t1, t2, t3 = 10000 + j, 20000 + j, 30000 + j
        lex[a], lex[b] = t1, t3
        sem[a], sem[b] = t2, t1
        gra[a], gra[b] = t3, t2
    R["tie_cycles"] = (lex, sem, gra)
    # pairs: A at (lex a, sem b), B at (lex b, sem a); with w_lex == w_sem the sums are equal
    R["tie_pairs"] = (A, [A[i ^ 1] for i in range(MAXC)], C)
    # ids only in the semantic channel (in descending id order): with its weight 0.0 a tie group of
    # 128 at 0.0 that starts at sighting position 100 and straddles 128
    R["zero_group"] = (A[:100], B[::-1], C[:10] + A[:10])
    return R


def rrf_batch(rows, names=None, width=MAXC):
    """-> three int64 [nq, width] arrays, -1 padded."""
    names = list(rows) if names is None else names
    out = [np.full((len(names), width), -1, dtype=np.int64) for _ in range(3)]
    for q, nm in enumerate(names):
        for c in range(3):
            ids = rows[nm][c]
            out[c][q, :len(ids)] = ids
    return out


def shortcut_rows():
    """One-channel rows [3, 128] for the duplicate-free shortcut: a probe chain of 128 that wraps (no
    duplicate: shortcut taken), the same chain ending in a copy of its first id and the chain with
    an adjacent duplicate pair in the middle (both: general path, occurrences merged)."""
    chain, slot = colliding_ids()
    dup_last = chain[:-1] + [chain[0]]
    dup_mid = chain[:64] + [chain[63]] + chain[64:-1]
    return np.array([chain, dup_last, dup_mid], dtype=np.int64), slot


def rrf_expect(flavour, lex, sem, gra, weights, top_k, rrf_k=60):
    """Oracle for one row.  flavour: "rag2" (thr_rrf_fuse), "standalone", "two" (lex = a, sem = b; the
    graph channel is not given).  -> (ids, scores, ranks, count) cut to top_k."""
    lex, sem, gra = cut(lex), cut(sem), cut(gra)
    if flavour == "rag2":
        w = dict(zip(NAMES, weights))
        i, s, r = O.fused_topk_ranks(lex, sem or [], gra, SLOTS, w, rrf_k)
    elif flavour == "standalone":
        i, s, r = O.standalone_fuse_ids(lex, sem, gra, dict(zip(NAMES, weights)))
    else:
        i, s, r = O.standalone_fuse_two_ids(lex or [], sem or [], weights[0], weights[1])
    return i[:top_k], s[:top_k], r[:top_k], min(len(i), top_k)


def rrf_calls():
    """The batched calls over rrf_rows(): (flavour, weight-set name, rrf_k, top_k).  Every flavour
    under every weight set at top_k = 512; thr_rrf_fuse also at rrf_k 0, 1 and the largest value it
    takes; top_k 1 and 384 for the capacity edge."""
    calls = [(f, w, 60, SLOTS) for f in ("rag2", "standalone", "two") for w in WEIGHT_SETS]
    calls += [("rag2", "default", k, SLOTS) for k in (0, 1, RRF_K_MAX)]
    calls += [(f, "default", 60, t) for f in ("rag2", "standalone", "two") for t in (1, 3 * MAXC)]
    return calls


def sighting_order(lex, sem, gra):
    seen = []
    for ch in (cut(lex), cut(sem), cut(gra)):
        for i in ch or []:
            if i not in seen:
                seen.append(i)
    return seen


def first_sighting_positions(lex, sem, gra):
    """Per channel, the list positions that hold a first sighting."""
    seen, out = set(), []
    for ch in (cut(lex), cut(sem), cut(gra)):
        here = []
        for p, i in enumerate(ch or []):
            if i not in seen:
                seen.add(i)
                here.append(p)
        out.append(here)
    return out


# ------------------------------------------------------------------------------------- fuse_post
ALPHAS = sorted({i / 20 for i in range(21)} | {0.3, 0.6, 0.9, 1 / 3, 2 / 3, 1e-9, 1 - 1e-9})
SWEEP_M = list(range(3, 41)) + [127, 128, 129, 384, 512]
POST_SIZES = (1, 2, 3, 4, 127, 128, 129, 256, 257, 384, 512)


def quantile_of(alpha: float) -> float:
    """The quantile RRFFusion.fuse_batch hands to thr_fuse_post."""
    return float(np.true_divide((1 - alpha) * 100, 100))


@functools.lru_cache(maxsize=None)
def score_pool(n: int = SLOTS):
    """n strictly decreasing float64 scores taken from real fused outputs."""
    rows = rrf_rows()
    vals = set()
    for nm, w in (("cap_disjoint", W_DEFAULT), ("wave_low", W_DEFAULT), ("cap_disjoint", (0.9, 1.3, 0.6)),
                  ("overlap_gra_rot1", W_DEFAULT)):
        vals.update(O.standalone_fuse_ids(*[cut(c) for c in rows[nm]], dict(zip(NAMES, w)))[1])
    pool = sorted(vals, reverse=True)
    assert len(pool) >= n
    return pool[:n]


def plateau_pool(n: int = SLOTS, run: int = 4):
    """Runs of ``run`` equal scores: the percentile's two neighbours fall inside one run for most
    (m, alpha), the cut then equals the run's value and every row of the run must stay."""
    p = score_pool(n)
    return [p[i // run] for i in range(n)]


def wide_pool(n: int = SLOTS):
    """Strictly decreasing scores that halve (and a little more) from row to row: the gap between
    the percentile's two neighbours is as large as the neighbours, so the two forms of numpy's lerp
    (a + (b - a) t below t = 0.5, b - (b - a)(1 - t) from there on) round to different doubles."""
    p = score_pool(n)
    return [p[i] * 0.5 ** i for i in range(n)]


class PostCall:
    """One thr_fuse_post call: arrays for the batch plus the call's parameters."""

    def __init__(self, name, ids, scores, counts=None, ranks=None, channel_scores=(None, None, None),
                 safety=0.0, alpha=None, normalize=False, top_k=0, row_names=None):
        self.name = name
        self.ids = np.ascontiguousarray(ids, dtype=np.int64)
        self.scores = np.ascontiguousarray(scores, dtype=np.float64)
        self.counts = None if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        self.ranks = None if ranks is None else np.ascontiguousarray(ranks, dtype=np.int32)
        self.channel_scores = tuple(None if c is None else np.ascontiguousarray(c, dtype=np.float64)
                                    for c in channel_scores)
        self.safety, self.alpha, self.normalize, self.top_k = safety, alpha, normalize, top_k
        self.row_names = row_names or [str(q) for q in range(self.ids.shape[0])]

    @property
    def quantile(self):
        return None if self.alpha is None else quantile_of(self.alpha)

    def row_count(self, q):
        n = self.ids.shape[1]
        return n if self.counts is None else max(0, min(n, int(self.counts[q])))

    def expect(self, q, fn=None):
        """Oracle for row q -> (ids, scores)."""
        m = self.row_count(q)
        fn = fn or O.fuse_post_rows
        return fn([int(x) for x in self.ids[q, :m]], [float(x) for x in self.scores[q, :m]],
                  None if self.ranks is None else [tuple(int(v) for v in r) for r in self.ranks[q, :m]],
                  tuple(None if c is None else [float(v) for v in c[q]] for c in self.channel_scores),
                  self.safety, self.alpha, self.top_k or None, self.normalize)


def _rows_from_pool(pool, n, nq):
    ids = np.tile(np.arange(n, dtype=np.int64) + 100, (nq, 1))
    sc = np.tile(np.array(pool[:n], dtype=np.float64), (nq, 1))
    return ids, sc


def post_size_calls():
    """Every n of POST_SIZES, counts as None and as 0, 1, 2, 3, n - 1, n, n + 5; denoise at
    alpha 0.6, normalise on."""
    pool = score_pool()
    calls = []
    for n in POST_SIZES:
        counts = [0, 1, 2, 3, n - 1, n, n + 5]
        ids, sc = _rows_from_pool(pool, n, len(counts))
        calls.append(PostCall(f"size_{n}_counts", ids, sc, counts, alpha=0.6, normalize=True,
                              row_names=[f"count={c}" for c in counts]))
        calls.append(PostCall(f"size_{n}_none", ids[:1], sc[:1], None, alpha=0.6, normalize=True))
    return calls


def post_sweep_call(alpha):
    """One launch per alpha: every m of SWEEP_M through ``counts``; strictly decreasing scores,
    plateaus and widely spaced scores."""
    nm = len(SWEEP_M)
    ids, strict = _rows_from_pool(score_pool(), SLOTS, nm)
    _, plat = _rows_from_pool(plateau_pool(), SLOTS, nm)
    _, wide = _rows_from_pool(wide_pool(), SLOTS, nm)
    return PostCall(f"sweep_alpha_{alpha!r}", np.concatenate([ids, ids, ids]),
                    np.concatenate([strict, plat, wide]), SWEEP_M * 3, alpha=alpha,
                    row_names=[f"{fam} m={m}" for fam in ("strict", "plateau", "wide") for m in SWEEP_M])


def lerp_weight(m, alpha):
    v = (m - 1) * quantile_of(alpha)
    return v - np.floor(v)


SAFETY = 0.5


def post_safety_calls():
    """Safety-threshold rows built on the fused output of cap_disjoint (384 rows, each seen in
    exactly one channel, so a row's keep flag is one channel score) and of dup_ends."""
    rows = rrf_rows()
    ids, sc, rk = O.standalone_fuse_ids(*rows["cap_disjoint"])
    n = len(ids)
    keeps = {
        "all_kept": set(range(n)),
        "none_kept": set(),
        "straddle_127_128": {127, 128},
        "straddle_255_256": {3, 255, 256, 300},
        "trips": {0, 127, 128, 255, 256, 383},
        "two_survivors": {5, 200},
        "three_survivors": {5, 200, 383},
        "every_third": set(range(0, n, 3)),
    }
    names = list(keeps) + ["at_threshold", "dup_last_rank_low", "dup_last_rank_high"]
    nq = len(names)
    I = np.full((nq, n), -1, dtype=np.int64)
    S = np.full((nq, n), -np.inf)
    RK = np.zeros((nq, n, 3), dtype=np.int32)
    CS = [np.full((nq, MAXC), 0.25) for _ in range(3)]
    counts = np.zeros(nq, dtype=np.int32)
    for q, nm in enumerate(names[:len(keeps)]):
        I[q], S[q], RK[q], counts[q] = ids, sc, rk, n
        for j in keeps[nm]:
            c = [x > 0 for x in rk[j]].index(True)
            CS[c][q, rk[j][c] - 1] = 0.75
    q = names.index("at_threshold")                 # best score == threshold exactly: kept
    I[q], S[q], RK[q], counts[q] = ids, sc, rk, n
    for c in range(3):
        CS[c][q, :] = np.nextafter(SAFETY, 0.0)
    for j in (1, 130, 383):
        c = [x > 0 for x in rk[j]].index(True)
        CS[c][q, rk[j][c] - 1] = SAFETY
    # id 7 of dup_ends sits at lexical positions 1 and 128: its score is the one at the LAST rank
    di, ds, dr = O.standalone_fuse_ids(*[cut(c) for c in rows["dup_ends"]])
    for nm, first, last in (("dup_last_rank_low", 0.75, 0.25), ("dup_last_rank_high", 0.25, 0.75)):
        q = names.index(nm)
        m = len(di)
        I[q, :m], S[q, :m], RK[q, :m], counts[q] = di, ds, dr, m
        for c in range(3):
            CS[c][q, :] = 0.25
        CS[0][q, 0], CS[0][q, MAXC - 1] = first, last
        CS[1][q, 126] = 0.25                       # (7 is also at semantic rank 127, graph rank 1)
    mk = lambda name, cs, **kw: PostCall(name, I, S, counts, RK, cs, safety=SAFETY, row_names=names, **kw)
    return [mk("safety", CS, alpha=0.6),
            mk("safety_no_denoise", CS),
            # the graph score tensor absent while graph ranks are > 0: those rows read 0.0
            mk("safety_graph_scores_absent", (CS[0], CS[1], None), alpha=0.6),
            mk("safety_only_sem_scores", (None, CS[1], None))]


def post_topk_norm_calls():
    pool = score_pool()
    m = 10
    ids, sc = _rows_from_pool(pool, 16, 1)
    calls = []
    for top_k in (0, 1, m, m + 1):
        for normalize in (False, True):
            calls.append(PostCall(f"topk_{top_k}_norm_{int(normalize)}", ids, sc, [m], top_k=top_k,
                                  normalize=normalize))
    # normalise value families, one row each (counts give the length)
    fam = {
        "all_equal": [0.25] * 6,
        "two_values": [0.5, 0.5, 0.125, 0.125, 0.125],
        "one_row": [0.3],
        "zero_rows": [],
        "negatives_and_zero": [2.5, 0.0, -0.0, -1.5, -3.0],
        "decreasing": pool[:8],
    }
    n = 8
    I = np.tile(np.arange(n, dtype=np.int64), (len(fam), 1))
    S = np.full((len(fam), n), -np.inf)
    cnt = []
    for q, v in enumerate(fam.values()):
        S[q, :len(v)] = v
        cnt.append(len(v))
    calls.append(PostCall("normalize_families", I, S, cnt, normalize=True, row_names=list(fam)))
    # min and max come from the rows top_k kept
    calls.append(PostCall("normalize_after_topk", I, S, cnt, normalize=True, top_k=3, row_names=list(fam)))
    calls.append(PostCall("normalize_after_denoise_topk", I, S, cnt, normalize=True, top_k=2, alpha=0.3,
                          row_names=list(fam)))
    return calls


def channel_scores_for(ids3, seed=5):
    """Synthetic channel scores in {0.25, 0.5, 0.75, ...} for id arrays [nq, w] (end to end)."""
    rng = np.random.default_rng(seed)
    return [None if a is None else rng.integers(1, 8, a.shape).astype(np.float64) / 8.0 for a in ids3]


# ---------------------------------------------------------------------------------- rerank_order
RERANK_SIZES = (1, 2, 128, 129, 512)
RERANK_LISTS = (1, 3, 8)
F32_DENORM = float(np.float32(1e-41))


def rerank_rows(n):
    """name -> list of n values (None = nobody scored the row) for one query.  Float32-exact."""
    f = lambda x: float(np.float32(x))
    rng = np.random.default_rng(n)
    R = {}
    R["all_unscored"] = [None] * n
    R["zeros_next_to_unscored"] = [(None, -0.0, 0.0)[p % 3] for p in range(n)]
    R["negatives_below_unscored"] = [(f(-0.5), None, f(-2.0), f(0.25))[p % 4] for p in range(n)]
    R["plus_inf"] = [(float("inf"), f(1.5), None, float("inf"))[p % 4] for p in range(n)]
    R["denormals"] = [(F32_DENORM, -F32_DENORM, None, 2 * F32_DENORM, 0.0)[p % 5] for p in range(n)]
    R["random_ties"] = [f(x) for x in rng.standard_normal(n).round(1)]
    # one tie group of 300 of 512 (scaled down for smaller n), spread over the row
    big = (n * 300) // 512
    v = [f(0.75)] * big + [f(x) for x in rng.standard_normal(n - big)]
    R["tie_group"] = [v[i] for i in rng.permutation(n)]
    return R


def rerank_lists(vals, n_lists, second_best=False):
    """Spread one row's values over n_lists float32 score lists: the owner (p mod n_lists) holds the
    value, the others -inf.  ``second_best``: the next list holds a smaller finite value too -- the
    maximum wins."""
    n = len(vals)
    out = np.full((n_lists, n), -np.inf, dtype=np.float32)
    for p, v in enumerate(vals):
        if v is None:
            continue
        out[p % n_lists, p] = v
        if second_best and n_lists > 1 and np.isfinite(v):
            out[(p + 1) % n_lists, p] = np.float32(v) - np.float32(1.0)
    return out


def rerank_case(n, n_lists):
    """-> (scores f32 [n_lists, nq, n], ids [nq, n], vals per row, names)."""
    R = rerank_rows(n)
    names = list(R) + ["two_lists_finite"]
    vals = [R[k] for k in R] + [R["random_ties"]]
    sc = np.stack([rerank_lists(v, n_lists, second_best=(nm == "two_lists_finite"))
                   for nm, v in zip(names, vals)], axis=1)
    ids = np.stack([np.random.default_rng(7 + q).permutation(10 * n)[:n] for q in range(len(names))]).astype(np.int64)
    return sc, ids, vals, names


def rerank_counts(n, nq):
    return np.array([(0, n, n + 3, n // 2, n - 1)[q % 5] for q in range(nq)], dtype=np.int32)


def rerank_expect(vals, ids_row, count, top_k):
    c = max(0, min(len(vals), count))
    order = O.rerank_order(vals[:c])[:top_k]
    return [int(ids_row[p]) for p in order], [float(vals[p] or 0.0) for p in order]


# ------------------------------------------------------------------------------------ merge_topk
MERGE_SHAPES = ((8, 128), (5, 205), (1, 1))     # n_lists x k_in: 1024 (ranked kernel), 1025 (general)
MERGE_K_OUT = (1, 10, 512)


def _ranked(s, i):
    """Rank each list (last axis) under (score desc, id asc)."""
    s, i = s.copy(), i.copy()
    for l in range(s.shape[0]):
        o = np.lexsort((i[l], -s[l]))
        s[l], i[l] = s[l][o], i[l][o]
    return s, i


def merge_rows(G, k):
    """name -> (scores [G, k], ids [G, k]) for one query."""
    rng = np.random.default_rng(G * 1000 + k)
    ids = (rng.permutation(G * k * 4)[:G * k].reshape(G, k) + 10).astype(np.int64)
    R = {}
    R["random"] = _ranked(rng.standard_normal((G, k)), ids)
    # cross-list ties on the score, distinct ids: (score desc, id asc) must decide
    R["cross_ties"] = _ranked(rng.integers(0, 6, (G, k)).astype(np.float64) / 4.0, ids)
    R["all_tied"] = _ranked(np.full((G, k), 0.5), ids)
    # a list ranked by score whose tied ids DESCEND: not ranked under the total order
    s, i = _ranked(rng.integers(0, 4, (G, k)).astype(np.float64), ids)
    for l in range(G):
        for v in np.unique(s[l]):
            m = s[l] == v
            i[l][m] = i[l][m][::-1]
    R["tied_ids_descend"] = (s, i)
    # invalid entries: finite score with id -1, NaN score, -inf with a live id, an empty list; a
    # valid entry after an invalid one
    s, i = _ranked(rng.standard_normal((G, k)), ids)
    s0, i0 = s.copy(), i.copy()
    if k > 1:
        i[0, k // 3] = -1
        s[G // 2, k // 2] = np.nan
        s[G - 1, k // 4] = -np.inf
        if G > 2:
            s[1, :], i[1, :] = -np.inf, -1
    R["invalid_entries"] = (s, i)
    # the tail of every list invalid: fewer valid entries than k_out = 512
    s, i = s0.copy(), i0.copy()
    keep = max(1, min(k, 300 // G))
    s[:, keep:], i[:, keep:] = -np.inf, -1
    R["few_valid"] = (s, i)
    s = rng.standard_normal((G, k))
    s[:, : max(1, k // 16)] = np.inf
    R["plus_inf"] = _ranked(s, ids)
    # -0.0 and +0.0 in different lists: equal, the id decides.  A third of the entries are positive
    # (the zeros fill places past the first third), every entry is valid.
    s = np.where(rng.random((G, k)) < 0.3, rng.random((G, k)) + 0.5, 0.0)
    s[::2] = np.where(s[::2] == 0.0, -0.0, s[::2])
    R["signed_zeros"] = _ranked(s, ids)
    # the same (score, id) pair in two lists (and in three): both copies count, and come out
    s, i = _ranked(rng.integers(0, 50, (G, k)).astype(np.float64), ids)
    if G > 1:
        h = max(1, k // 2)
        s[1, :h], i[1, :h] = s[0, :h], i[0, :h]
        if G > 2:
            s[G - 1, :1], i[G - 1, :1] = s[0, :1], i[0, :1]
        s, i = _ranked(s, i)
    R["duplicate_pairs"] = (s, i)
    return R


def merge_case(G, k):
    R = merge_rows(G, k)
    names = list(R)
    S = np.stack([R[nm][0] for nm in names], axis=1)    # [G, nq, k]
    I = np.stack([R[nm][1] for nm in names], axis=1)
    return np.ascontiguousarray(S), np.ascontiguousarray(I), names


def merge_expect(S_q, I_q, k_out, fn=None):
    """Oracle for one query: entries with id < 0 are invalid, as are -inf and NaN scores."""
    s, i = S_q.ravel().copy(), I_q.ravel()
    s[i < 0] = -np.inf
    return (fn or O.topk_desc)(s, k_out, i)
