"""Inputs and reference of the graph-channel tests (tests/test_graph_cases_host.py checks what the
builders promise, on the CPU; tests/test_gpu_graph.py runs them through thr_graph_topk and
thr_graph_topk_scoped).  Pure numpy: nothing here needs a GPU.

The reference of every case is oracle.thr_oracle.graph_scores with topk_desc (float64, entity
ascending, mention order); inside a scope, the same scores with the chunks outside the scope at
-inf.  Every comparison is bit for bit, so the builders choose inputs on which a wrong distance, a
wrong summation order or a wrong tie-break changes bits.

Every builder takes a window (chunk_base, n_chunks) of a corpus of N_CORPUS chunks and a tier
variant.  The variants of one case have the same expected output:

* "asbuilt": the case alone (the small on-chip tier, unless the case says otherwise);
* "full":    pushed past the small capacities (1024 entities / 2048 contributions);
* "global":  pushed past the full ones (4096 / 8192): the global-memory tier, or, without the
             transposed mention CSR, THR_FLAG_OVERFLOW.

The push is tier_ballast: one extra seed entity that at hops >= 1 has R out-edges to entities with
neither mentions nor edges (they count as reached and contribute nothing), and at hops 0 has M
mentions of chunks outside the window (thr_graph_topk gives each a contribution slot,
thr_graph_topk_scoped gives them none).  A row that already has 16 seeds gets the same ballast hung
on its first seed entity instead.
"""
import functools

import numpy as np

from oracle import thr_oracle as O

N_CORPUS = 3000
WHOLE = (0, N_CORPUS)
SHARD = (700, 1500)                 # an interior shard: mentions lie below 700 and at or beyond 2200
WINDOWS = {"whole": WHOLE, "shard": SHARD}
TIERS = ("asbuilt", "full", "global")

SMALL_ENT, SMALL_CON = 1024, 2048   # GrSmall::MAX_ENT / MAX_CON  (csrc/graph_common.hpp)
FULL_ENT, FULL_CON = 4096, 8192     # GrFull
FB_BLOCKS = 64                      # workgroups of the global-memory tier: query q goes to q % 64
MAX_SEEDS, TOPK_MAX, MAX_HOPS = 16, 128, 8

N_ENT = -1000                       # placeholder in edges and seeds: "n_entities", resolved by finish()


class Case:
    """One call of the graph channel.  g: the five CSR arrays as the device gets them; clean_g /
    clean_seeds: the same with edge targets and seeds outside [0, n_entities) removed -- what the
    oracle is given (it does not guard them).  ballasted[q]: the tier push applies to query q."""

    def __init__(self, name, window, tier, g, clean_g, seeds, clean_seeds, hops, k, asbuilt_tier, ballasted,
                 hits):
        self.name, self.window, self.tier = name, window, tier
        self.g, self.clean_g, self.seeds, self.clean_seeds = g, clean_g, seeds, clean_seeds
        self.hops, self.k, self.asbuilt_tier, self.ballasted, self.hits = hops, k, asbuilt_tier, ballasted, hits
        self.n_entities = len(g[0]) - 1
        self.nq = seeds.shape[0]
        self._dist = {}
        self.doc_label = None          # a labelling of the window's chunks that belongs to the case
        self.query_label = None

    @property
    def intended_tier(self):
        return self.asbuilt_tier if self.tier == "asbuilt" else self.tier


class Draft:
    """A graph under construction: out-edges and mentions per entity, in the order they were added."""

    def __init__(self, n_entities):
        self.edges = [[] for _ in range(n_entities)]
        self.mentions = [[] for _ in range(n_entities)]     # (global chunk, float32 confidence)

    @property
    def n(self):
        return len(self.edges)

    def add_entities(self, m):
        first = self.n
        self.edges.extend([] for _ in range(m))
        self.mentions.extend([] for _ in range(m))
        return first

    def edge(self, a, b, both=True):
        self.edges[a].append(b)
        if both:
            self.edges[b].append(a)

    def mention(self, e, chunk, conf):
        self.mentions[e].append((int(chunk), np.float32(conf)))


def outside_chunks(window, m):
    """m global chunk ids outside the window: below its base where there is room, and at or beyond
    its end (the first beyond is the end itself)."""
    base, n = window
    below = np.arange(base - 1, -1, -1)[: m // 2]
    beyond = base + n + np.arange(m - len(below))
    out = np.empty(m, dtype=np.int64)
    out[: 2 * len(below): 2] = below
    rest = np.ones(m, dtype=bool)
    rest[: 2 * len(below): 2] = False
    out[rest] = beyond
    return out


def tier_ballast(d, seeds, hops, tier, window):
    """Push every query of ``seeds`` (rows of <= 16 seeds) into ``tier`` without changing its answer.
    -> (seeds with the ballast seed, ballasted rows).  A row of nothing but padding stays as it is:
    a query without seeds has nothing to hang the ballast on when the row is full, and an empty row
    with a ballast seed is no longer the empty row."""
    nq, ms = seeds.shape
    ballasted = np.array([np.any(seeds[q] != -1) for q in range(nq)])
    if tier == "asbuilt":
        return seeds, ballasted
    edges = {"full": SMALL_ENT, "global": FULL_ENT}[tier]         # R: reached >= R + 1
    slots = {"full": SMALL_CON + 1, "global": FULL_CON + 1}[tier]  # M: contributions >= M
    if ms < MAX_SEEDS:
        host = [d.add_entities(1)]
        col = np.where(ballasted, host[0], -1).astype(np.int32)
        seeds = np.concatenate([seeds, col[:, None]], axis=1)
    else:
        host = sorted({int(seeds[q, 0]) for q in range(nq) if ballasted[q]})
        assert all(0 <= h < d.n for h in host), "a full row's first seed carries the ballast: it must be valid"
    if hops >= 1:
        first = d.add_entities(edges)
        for h in host:
            for t in range(first, first + edges):
                d.edge(h, t, both=False)
    else:
        for h in host:
            for c in outside_chunks(window, slots):
                d.mention(h, c, 0.75)
    return seeds, ballasted


def finish(name, d, seeds, hops, k, window, tier, asbuilt_tier="small", hits=None):
    """Ballast, then the CSR arrays; N_ENT placeholders become n_entities."""
    seeds = np.asarray(seeds, dtype=np.int32)
    seeds, ballasted = tier_ballast(d, seeds, hops, tier, window)
    n = d.n
    seeds = np.where(seeds == N_ENT, n, seeds).astype(np.int32)

    def csr(clean):
        cols = []
        for e in range(n):
            row = [n if t == N_ENT else t for t in d.edges[e]]
            cols.append([t for t in row if 0 <= t < n] if clean else row)
        ent_rowptr = np.concatenate([[0], np.cumsum([len(r) for r in cols])]).astype(np.int64)
        ent_col = np.array([t for r in cols for t in r], dtype=np.int32)
        men_rowptr = np.concatenate([[0], np.cumsum([len(r) for r in d.mentions])]).astype(np.int64)
        men_chunk = np.array([c for r in d.mentions for c, _ in r], dtype=np.int32)
        men_conf = np.array([w for r in d.mentions for _, w in r], dtype=np.float32)
        return ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf

    g, clean_g = csr(False), csr(True)
    clean_seeds = np.where((seeds >= 0) & (seeds < n), seeds, -1).astype(np.int32)
    return Case(name, window, tier, g, clean_g, seeds, clean_seeds, hops, k, asbuilt_tier, ballasted, hits or {})


# ------------------------------------------------------------------------------------ the reference
def oracle_scores(case):
    """float64 scores of every chunk of the window, one vector per query."""
    base, n = case.window
    return [O.graph_scores(*case.clean_g, [int(s) for s in case.clean_seeds[q]], case.hops, n, base)
            for q in range(case.nq)]


@functools.lru_cache(maxsize=None)
def scores(name, window_name):
    """The expected scores of a case in a window: the oracle's over the case AS BUILT.  The host test
    proves that the ballasted variants have the same ones, so they are computed once and shared."""
    out = oracle_scores(build(name, window_name, "asbuilt"))
    for s in out:
        s.setflags(write=False)
    return out


def expected(case, window_name, query_label=None, doc_label=None):
    """[(scores, global ids)] per query; with labels, the chunks outside the query's scope at -inf."""
    base = case.window[0]
    out = []
    for q, s in enumerate(scores(case.name, window_name)):
        if query_label is not None and query_label[q] >= 0:
            s = np.where(doc_label == query_label[q], s, -np.inf)
        ts, ti = O.topk_desc(s, case.k)
        out.append((ts, ti + base))
    return out


def oracle_dist(case, q):
    """The oracle's own BFS: graph_scores over a mention CSR in which entity e mentions 'chunk' e with
    confidence 1 gives 1 / (1 + dist(e)) for a reached entity and -inf elsewhere.  -> dist, -1 = not reached"""
    if q not in case._dist:
        n = case.n_entities
        ident = (np.arange(n + 1, dtype=np.int64), np.arange(n, dtype=np.int32), np.ones(n, dtype=np.float32))
        s = O.graph_scores(case.clean_g[0], case.clean_g[1], *ident, [int(x) for x in case.clean_seeds[q]],
                           case.hops, n, 0)
        ok = np.isfinite(s)
        case._dist[q] = np.where(ok, np.rint(1.0 / np.where(ok, s, 1.0)) - 1, -1).astype(np.int64)
    return case._dist[q]


def reach_counts(case, q, query_label=-1, doc_label=None):
    """-> (reached entities, contribution slots of thr_graph_topk, of thr_graph_topk_scoped): every
    mention of a reached entity takes a slot in the first, the kept in-window mentions in the second."""
    reached = oracle_dist(case, q) >= 0
    rp, mc = case.g[2], case.g[3].astype(np.int64)
    base, n = case.window
    of_reached = np.repeat(reached, np.diff(rp))          # per mention: is its entity reached?
    c = mc[of_reached] - base
    c = c[(c >= 0) & (c < n)]
    kept = int((doc_label[c] == query_label).sum()) if query_label >= 0 else len(c)
    return int(reached.sum()), int(of_reached.sum()), kept


def beyond_full(case):
    """Per query: does thr_graph_topk need more than the full on-chip capacities?  (Without the
    transposed CSR these queries, and no others, come back with THR_FLAG_OVERFLOW.)"""
    if "hub" in case.hits:           # fallback_reuse: the host test proves this is the same set
        return case.hits["hub"] >= 0
    return np.array([tier_of(*reach_counts(case, q)[:2]) == "global" for q in range(case.nq)])


def tier_of(n_reached, n_slots):
    if n_reached <= SMALL_ENT and n_slots <= SMALL_CON:
        return "small"
    if n_reached <= FULL_ENT and n_slots <= FULL_CON:
        return "full"
    return "global"


def contributions(case, q, chunk):
    """The float64 terms of one chunk's score in the oracle's order (entity asc, mention order)."""
    dist = oracle_dist(case, q)
    rp, mc, mw = case.clean_g[2], case.clean_g[3], case.clean_g[4]
    out = []
    for e in np.flatnonzero(dist >= 0):
        for j in range(rp[e], rp[e + 1]):
            if mc[j] == chunk:
                out.append(np.float64(mw[j]) / np.float64(1.0 + float(dist[e])))
    return out


def sum_in_order(terms):
    s = np.float64(0.0)
    for t in terms:
        s = s + t
    return s


def sorted_positions(case, q):
    """Where thr_graph_topk's sorted key array holds each in-window chunk's segment: contributions in
    (local chunk, position) order.  -> {global chunk: (first index, one past the last)}"""
    dist = oracle_dist(case, q)
    rp, mc = case.g[2], case.g[3].astype(np.int64)
    base, n = case.window
    c = np.concatenate([mc[rp[e]:rp[e + 1]] for e in np.flatnonzero(dist >= 0)] or [np.zeros(0, np.int64)]) - base
    c = np.sort(c[(c >= 0) & (c < n)], kind="stable")
    out = {}
    for chunk in np.unique(c):
        lo, hi = np.searchsorted(c, chunk, "left"), np.searchsorted(c, chunk, "right")
        out[int(chunk) + base] = (int(lo), int(hi))
    return out


def dkey_prefix(x):
    """Top 32 bits of the order-preserving key of a float64 (thr_common.hpp dkey): larger score,
    larger key.  BlockTopK::compact selects on these bits."""
    u = np.asarray(x, dtype=np.float64).view(np.uint64)
    key = np.where(u >> np.uint64(63), ~u, u | np.uint64(1 << 63))
    return (key >> np.uint64(32)).astype(np.uint32)


def chunk_labels(window, n_labels=3):
    """A labelling of the window's chunks by their global id: neighbours get different labels."""
    base, n = window
    return ((base + np.arange(n)) % n_labels).astype(np.int32)


# ------------------------------------------------------------------------------------------ 4. distances
DIST_UNIT = 2520.0       # lcm(1..9): confidence / (1 + d) is an exact integer for every d <= 8


def distances(window, tier, hops):
    """Hand-made: a path 0..9 (hops 0..8 reach one entity more each); a shortcut 20 - 3 that puts
    entity 3 at distance 1 from seed 20 and 3 from seed 0; a 4-cycle 30..33 with a self loop on 30
    and the edge 31 -> 32 stored twice; 40 -> 41 stored in one direction only; entity 42 with edge
    targets -1 and n_entities beside a good one.  Entity e mentions its own chunk with confidence
    2520 (e + 1) and two chunks that several entities share: every term conf / (1 + d) is an exact
    integer and differs for every d, so a wrong distance is a wrong score."""
    base, n = window
    d = Draft(50)
    for e in range(9):
        d.edge(e, e + 1)
    d.edge(20, 3)
    for a, b in ((30, 31), (32, 33), (33, 30)):
        d.edge(a, b)
    d.edge(30, 30, both=False)
    d.edge(31, 32), d.edge(31, 32)
    d.edge(40, 41, both=False)
    d.edges[42] += [-1, 43, N_ENT, -1]
    d.edges[43] += [N_ENT, 42]
    own = base + (np.arange(50) * 29 + 7) % n                       # in the window
    own[[5, 32]] = outside_chunks(window, 2)                        # ... but for two of them
    shared = (base + 3, base + n - 1)
    for e in range(50):
        d.mention(e, own[e], DIST_UNIT * (e + 1))
        d.mention(e, shared[e % 2], DIST_UNIT * (100 + e))
    seeds = [[0, -1], [20, -1], [0, 20], [9, 0], [30, -1], [31, 33], [40, -1], [41, -1], [42, -1], [43, 5]]
    return finish(f"distances-h{hops}", d, seeds, hops, 50, window, tier)


# ------------------------------------------------------------------------------------------ 5. sum_order
SEGMENTS = (255, 2, 17, 256, 257, 600)         # laid out in this order: the 2 sits on positions 255, 256
SEGMENTS_LONG = SEGMENTS + (600, 257)          # 1387 + 600 = 1987: the last one straddles 2048


def sum_order(window, tier, long=False):
    """Chunks whose scores are long sums of conf / (1 + d), d in {0, 1, 2}: a seed, its 40 neighbours,
    their 200 neighbours.  A segment of L terms takes L // 3 (at most 100) repeated mentions by one
    entity and the rest from entities drawn over all three distances.  The chunks are the lowest of
    the window, so the sorted key array holds the segments back to back from position 0."""
    base, n = window
    segs = SEGMENTS_LONG if long else SEGMENTS
    rng = np.random.default_rng(77 + base + (1 if long else 0))
    d = Draft(241)
    for a in range(1, 41):
        d.edge(0, a)
        for b in range(5):
            d.edge(a, 41 + (a - 1) * 5 + b)
    chunks = [base + i for i in range(len(segs))]

    def draw(L, chunk):
        heavy = int(rng.integers(0, 241))
        ents = [heavy] * min(L // 3, 100)
        ents += [int(e) for e in rng.integers(0, 241, L - len(ents))]
        return [(e, chunk, np.float32(rng.uniform(0.5, 1.0))) for e in ents]

    def order_sensitive(ms):
        dist = lambda e: 0 if e == 0 else (1 if e <= 40 else 2)
        terms = [np.float64(w) / np.float64(1.0 + dist(e)) for e, _, w in sorted(ms, key=lambda m: m[0])]
        s = sum_in_order(terms)
        return s != sum_in_order(terms[::-1]) and s != sum_in_order(sorted(terms))

    for L, chunk in zip(segs, chunks):
        ms = draw(L, chunk)
        while L > 2 and not order_sensitive(ms):     # an input that cannot tell the orders apart is redrawn
            ms = draw(L, chunk)
        for e, c, w in ms:
            d.mention(e, c, w)
    # a few mentions outside the window, from entities that also feed the segments
    noise = 60 if window[0] else 0
    for c in outside_chunks(window, noise):
        d.mention(int(rng.integers(0, 241)), c, rng.uniform(0.5, 1.0))
    name = "sum_order_long" if long else "sum_order"
    return finish(name, d, [[0, -1]], 2, 50, window, tier, asbuilt_tier="full" if long else "small",
                  hits=dict(chunks=chunks, segments=segs))


# ----------------------------------------------------------------------------------------------- 6. ties
TIE_LO, TIE_N = 500, 2000        # the tied chunks: global ids 500 .. 2499 (in the shard: 700 .. 2199)
TIE_QUERIES = ("plain", "ids_descending", "flood", "magnitudes", "zeros", "short")


def ties(window, tier, k):
    """hops 0, one seed entity per query, each with its own pattern of confidences over chunks
    500 .. 2499 (2000 contributions: the small tier, whose top-k buffer holds 512)."""
    d = Draft(len(TIE_QUERIES))
    span = np.arange(TIE_LO, TIE_LO + TIE_N)
    for c in span:
        j = int(c - TIE_LO)
        d.mention(0, c, 1.0)                                        # plain: everything ties
        d.mention(1, c, 1.0 + j // 250)                             # best scores on the highest ids, 250 tied each
        d.mention(2, c, np.float32(1.0) + np.float32((j * 5) % 8) * np.float32(2.0 ** -23))   # flood
        d.mention(3, c, np.ldexp(1.0 + (j % 5) / 8.0, (j * 7) % 97 - 48))                     # many binades
    for j, c in enumerate(span[::9]):                               # zeros: 223 chunks, 12 of them positive
        d.mention(4, c, 0.5 + j / 64.0 if j % 19 == 0 else 0.0)
    for j, c in enumerate(span[300:1700:70]):                       # short: 20 chunks, fewer than k = 50
        d.mention(5, c, 0.25 + j / 32.0)
    d.edge(4, 5)                                                    # (hops 0: never walked; ent_col is not empty)
    seeds = [[q] for q in range(len(TIE_QUERIES))]
    return finish(f"ties-k{k}", d, seeds, 0, k, window, tier)


# ---------------------------------------------------------------------------------------------- 7. seeds
def _random_graph(rng, n_ent, window, lonely=()):
    base, n = window
    d = Draft(n_ent)
    for e in range(n_ent):
        if e in lonely:
            continue
        for t in rng.integers(0, n_ent, 2):
            if int(t) not in lonely:
                d.edge(e, int(t))
        for c in rng.integers(max(0, base - 200), min(N_CORPUS, base + n + 200), 3):
            d.mention(e, c, rng.uniform(0.5, 1.0))
    return d


def seeds_one(window, tier):
    """max_seeds = 1: a plain seed, a seed entity without edges or mentions, a seed equal to
    n_entities, one far beyond it, and padding."""
    d = _random_graph(np.random.default_rng(5), 300, window, lonely=(17,))
    seeds = [[4], [17], [N_ENT], [2 ** 31 - 1], [-1], [250]]
    return finish("seeds_one", d, seeds, 2, 50, window, tier)


def seeds_sixteen(window, tier):
    """max_seeds = 16: sixteen distinct seeds, sixteen with duplicates, a row of all -1, seeds at and
    beyond n_entities and below -1 mixed with valid ones."""
    rng = np.random.default_rng(6)
    d = _random_graph(rng, 300, window)
    distinct = rng.choice(300, 16, replace=False)
    dup = np.array([8, 8, 120, 8, 33, 120, 8, 33, 33, 8, 120, 8, 8, 33, 120, 8])
    mixed = np.array([77, N_ENT, 2 ** 31 - 1, 140, -7, N_ENT, 77, 299, -1, 0, 2 ** 30, -1, 12, N_ENT, 5, -2 ** 31])
    seeds = np.stack([distinct, dup, np.full(16, -1), mixed])
    return finish("seeds_sixteen", d, seeds, 2, 50, window, tier)


# ------------------------------------------------------------------------------------ 2. capacity_edges
STAR_SIZES = (1023, 1024, 1025, 4095, 4096, 4097)
MENTION_SIZES = (2047, 2048, 2049, 8191, 8192, 8193)


def star(window, tier, reached):
    """A hub whose hops-1 neighbourhood is exactly ``reached`` entities, hub included; every entity
    mentions one chunk of the window.  A second query has two ordinary seeds."""
    assert tier == "asbuilt"
    base, n = window
    rng = np.random.default_rng(reached)
    d = Draft(reached + 6)
    for t in range(1, reached):
        d.edge(0, t)
    d.edge(reached, reached + 1), d.edge(reached + 2, reached + 3)
    for e in range(d.n):
        d.mention(e, base + int(rng.integers(0, n)), rng.uniform(0.5, 1.0))
    case = finish(f"star-{reached}", d, [[0, -1], [reached, reached + 2]], 1, 50, window, tier,
                  asbuilt_tier=tier_of(reached, reached), hits=dict(reached=reached))
    case.ballasted = np.array([True, False])            # (the tier is the hub query's)
    return case


def mentions(window, tier, m):
    """One entity with exactly ``m`` mentions, all inside the window, at hops 0."""
    assert tier == "asbuilt"
    base, n = window
    rng = np.random.default_rng(m)
    d = Draft(4)
    for c in rng.integers(0, n, m):
        d.mention(0, base + int(c), rng.uniform(0.5, 1.0))
    for e in (1, 2, 3):
        d.mention(e, base + e, 0.5 + e / 8.0)
    d.edge(0, 1)
    case = finish(f"mentions-{m}", d, [[0, -1], [1, 2]], 0, 50, window, tier, asbuilt_tier=tier_of(1, m),
                  hits=dict(mentions=m))
    case.ballasted = np.array([True, False])
    return case


SCOPED_TOTAL = 16384


def scoped_mentions(window, tier, kept):
    """One entity with 16 384 mentions inside the window, of which the label 0 keeps exactly ``kept``
    (8192 or 8193): mentions j < 16 383 go to local chunk j % 1024, sixteen each, chunks 0 .. 511
    carry the label 0; the last mention goes to local chunk 1024, whose label decides."""
    assert tier == "asbuilt" and kept in (FULL_CON, FULL_CON + 1)
    base, n = window
    rng = np.random.default_rng(kept)
    d = Draft(2)
    for j in range(SCOPED_TOTAL - 1):
        d.mention(0, base + j % 1024, rng.uniform(0.5, 1.0))
    d.mention(0, base + 1024, 0.875)
    d.mention(1, base + 5, 0.5)
    d.edge(0, 1)                                        # (hops 0: never walked)
    case = finish(f"scoped_mentions-{kept}", d, [[0, -1], [1, -1], [0, 1]], 0, 50, window, tier,
                  asbuilt_tier="global", hits=dict(kept=kept))
    case.ballasted = np.array([True, False, True])      # (the tier is the one of the queries seeded at the hub)
    label = np.ones(n, dtype=np.int32)
    label[:512] = 0                 # 15 full rounds of 512 kept + 512 of the last 1023 mentions = 8192
    label[1024] = 0 if kept == FULL_CON + 1 else 1
    case.doc_label = label
    case.query_label = np.array([0, 0, -1], dtype=np.int32)
    return case


# ------------------------------------------------------------------------------------ 3. fallback_reuse
REUSE_NQ, REUSE_HUB = 192, 4200


def reuse_plan():
    """Which of the 192 queries overflow and which hub each takes: every fifth query stays on chip;
    the others alternate between the hubs in the order ONE workgroup of the third tier meets them
    (it takes q, q + 64, q + 128, ...).  -> hub[q] in {0, 1}, -1 = an on-chip query"""
    hub = np.full(REUSE_NQ, -1, dtype=np.int64)
    for b in range(FB_BLOCKS):
        mine = [q for q in range(b, REUSE_NQ, FB_BLOCKS) if q % 5 != 4]
        for rank, q in enumerate(mine):
            hub[q] = (rank + b) % 2
    return hub


def fallback_reuse(window, tier):
    """154 queries beyond the full capacities in one call, 38 on-chip ones between them.  Hub 1's 4200
    neighbours are entities 62 .. 4261, hub 0's 4262 .. 8461 -- the last entity; n_entities = 8462 is
    no multiple of 4.  Every query has a second seed of its own among the 60 ordinary entities."""
    assert tier == "asbuilt"
    base, n = window
    rng = np.random.default_rng(31)
    d = Draft(2 + 60 + 2 * REUSE_HUB)
    for h, first in ((1, 62), (0, 62 + REUSE_HUB)):
        for t in range(first, first + REUSE_HUB):
            d.edge(h, t, both=False)
    lo, hi = max(0, base - 150), min(N_CORPUS, base + n + 150)
    for e in range(2, 62):
        d.edge(e, 2 + int(rng.integers(0, 60)))
        for c in rng.integers(lo, hi, 3):
            d.mention(e, c, rng.uniform(0.5, 1.0))
    for e in range(62, d.n):
        d.mention(e, rng.integers(lo, hi), rng.uniform(0.5, 1.0))
    d.mention(0, base + 1, 0.625), d.mention(1, base + 2, 0.875)
    hub = reuse_plan()
    seeds = np.full((REUSE_NQ, 3), -1, dtype=np.int32)
    for q in range(REUSE_NQ):
        other = 2 + (q * 7) % 60
        seeds[q] = [other, 2 + (q * 11 + 3) % 60, -1] if hub[q] < 0 else [other, hub[q], -1]
    case = finish("fallback_reuse", d, seeds, 1, 50, window, tier, asbuilt_tier="global", hits=dict(hub=hub))
    case.ballasted = hub >= 0
    return case


# ----------------------------------------------------------------------------------------- the registry
CONTENT = {}                     # cases that run in all three tiers
for _h in range(MAX_HOPS + 1):
    CONTENT[f"distances-h{_h}"] = functools.partial(distances, hops=_h)
CONTENT["sum_order"] = sum_order
CONTENT["sum_order_long"] = functools.partial(sum_order, long=True)
for _k in (1, 50, TOPK_MAX):
    CONTENT[f"ties-k{_k}"] = functools.partial(ties, k=_k)
CONTENT["seeds_one"] = seeds_one
CONTENT["seeds_sixteen"] = seeds_sixteen

EDGES = {}                       # cases that are about one tier boundary: as built only
for _r in STAR_SIZES:
    EDGES[f"star-{_r}"] = functools.partial(star, reached=_r)
for _m in MENTION_SIZES:
    EDGES[f"mentions-{_m}"] = functools.partial(mentions, m=_m)
for _m in (FULL_CON, FULL_CON + 1):
    EDGES[f"scoped_mentions-{_m}"] = functools.partial(scoped_mentions, kept=_m)
EDGES["fallback_reuse"] = fallback_reuse

BUILDERS = {**CONTENT, **EDGES}


def variants():
    """(name, tier, window name) of every run."""
    out = []
    for name in BUILDERS:
        for tier in (TIERS if name in CONTENT else TIERS[:1]):
            for w in WINDOWS:
                out.append((name, tier, w))
    return out


@functools.lru_cache(maxsize=8)
def build(name, window_name, tier="asbuilt"):
    return BUILDERS[name](WINDOWS[window_name], tier)
