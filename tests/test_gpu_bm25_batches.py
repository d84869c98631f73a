"""BM25 top-k along the batch-size axis: what bm25_plan_kernel does changes with n_queries (plan
workgroups and their 64-workgroup cap, the two item budgets and the fit loop that doubles the slice
sizes, the item order, the sweep filter's queries per thread), and a query's result must not.

Every assertion is bit equality of ids, scores and counts with oracle.thr_oracle.bm25_topk.  The
oracle runs ONCE per corpus and mode on a pool of a few hundred distinct queries -- every kind the
planner tells apart -- and a batch of N queries draws pool rows with a seeded permutation, with
replacement: row i of the batch must equal the oracle's list of its pool row, wherever it stands
in the batch and whatever stands next to it, although its slicing depends on both.  The control
words at the start of the lexical workspace (items, queries with probed terms, sweep items, plan
workgroups, stage-A slice size, queries of the workgroup walk) say which branch a case took, and
are asserted: a case that stops reaching its branch after a retune fails.

Batches above 16384 queries: before the waves' budget grew with the batch (one slot per query on
top of the tuned 16384) the fit loop could not end for more than 16384 wave-walked queries -- a
kernel that never returns.  That was established from the code, never run; the evidence for the
fix is the termination argument in bm25_plan_kernel and these cases passing.

Two corpora: 4000 docs (one pass, one slice per query: the large batches) and 80000 docs (sliced
queries, up to 3000 of them).  Largest workspaces, from thr_bm25_workspace_bytes at 32 term
columns: 65600 queries at k = 10: 192 MB; 20000 queries at k = 128: 251 MB; 40000 at k = 10: 127 MB."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import thr_oracle as O  # noqa: E402

MT = 32                      # term columns of the pool (THR_BM25_MAX_TERMS)
K_MAX = 128                  # the oracle's lists are cut once, at THR_TOPK_MAX: a top-k is a prefix of it
WAVE_ITEMS = 16384           # bm25.hip: BM_WAVE_ITEMS, BM_EXTRA_ITEMS
WW_TARGET_MIN, WW_TARGET_MAX, BM_TARGET0, BM_MAX_SLICES = 640, 1536, 24576, 128
BLOCK_WALK = os.environ.get("THR_BM25_WALK", "")[:1] == "b"   # (inside the knob run of this file)


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


# --------------------------------------------------------------------------- the pool
def _row(rng, terms, width):
    """``terms`` at random columns of the first ``width`` (padding anywhere in the row)."""
    row = np.full(MT, -1, dtype=np.int32)
    row[rng.permutation(width)[:len(terms)]] = terms
    return row


def build_pool(df, has_row, n, v, seed, reps, sliced):
    """-> (pool int32 [P, MT], kind [P]).  Kinds: wave (1 / 2 / 5 / 8 terms without rows), longwave
    (8 of the longest lists without rows), pw (probed + walked terms), probed (probed terms only: no
    stage A), rowwalk (terms with rows rare enough to be walked), block (9 / 12 / 32 terms: the
    workgroup walk), bigblock (12 - 32 of the longest lists), empty (nothing to score)."""
    rng = np.random.default_rng(seed)
    order = np.argsort(-df, kind="stable").astype(np.int32)
    heavy = order[has_row[order] & (df[order] * 64 >= n)]        # always probed
    light = order[has_row[order] & (df[order] * 64 < n)]         # rows, but rare enough to be walked
    nr = order[~has_row[order] & (df[order] > 0)]                # no rows, longest first
    rare = np.nonzero((df >= 1) & (df <= 3))[0].astype(np.int32)
    none = np.nonzero(df == 0)[0].astype(np.int32)
    p_nr = df[nr] / df[nr].sum()
    assert len(heavy) >= 8 and len(nr) >= 64 and len(rare) >= 8
    pool, kind = [], []

    def add(k, terms, width=MT):
        pool.append(_row(rng, np.asarray(terms, dtype=np.int32), max(width, len(terms))))
        kind.append(k)

    for rep in range(reps):
        for nt in (1, 2, 5, 8):
            w = 8 if rep % 2 == 0 else MT
            add("wave", nr[rep * nt:(rep + 1) * nt], w)                       # the longest lists without rows
            add("wave", rng.choice(nr, nt, replace=False, p=p_nr), w)          # by df
            add("wave", rng.choice(nr, nt, replace=False), w)                  # mostly short lists
            add("wave", rng.choice(rare, nt, replace=False), w)
            a, b = rng.choice(nr[:200], 2, replace=False)
            add("wave", [a, b, a, a, b, a, b, b][:nt], w)                      # repeated terms
        add("wave", [nr[rep], v + 5, 2 ** 30 + rep], 8)                        # ids outside the vocabulary
        for a in (1, 2, 3):
            for b in (1, 2, 5):
                add("pw", np.concatenate([rng.choice(heavy, a, replace=False),
                                          rng.choice(nr, b, replace=False, p=p_nr)]), 8 if rep % 2 else MT)
        for nt in (1, 2, 3, 4):
            add("probed", rng.choice(heavy, nt, replace=False), 8)
        h = rng.choice(heavy, 2, replace=False)
        add("probed", [h[0], h[0]], 8)                                          # a probed term repeated
        add("probed", [h[0], h[1], h[0], v + 1], MT)
        if len(light) >= 4:
            add("rowwalk", rng.choice(light, 1), 8)
            add("rowwalk", rng.choice(light, 3, replace=False), 8)
            add("rowwalk", np.concatenate([rng.choice(light, 2, replace=False), rng.choice(heavy, 2, replace=False)]), 8)
            add("rowwalk", np.concatenate([rng.choice(light, 1), rng.choice(nr, 2, replace=False, p=p_nr)]), MT)
        for nt in (9, 12, 32):
            add("block", np.concatenate([rng.choice(order[:40], nt // 3, replace=False),
                                         rng.choice(nr, nt - nt // 3, replace=False, p=p_nr)]))
            add("block", rng.choice(nr, nt, replace=False))
        if sliced:
            add("longwave", rng.choice(nr[:24], 8, replace=False), 8)
            add("longwave", nr[rep % 8:rep % 8 + 8], 8)
            add("bigblock", order[:32] if rep % 3 == 0 else rng.choice(order[:40], 12 + 4 * (rep % 6), replace=False))
    add("empty", [])                                                           # all padding
    add("empty", [v, v + 7, 2 ** 30])                                          # nothing inside the vocabulary
    if len(none):
        add("wave", [none[0]], 8)                                              # a term no doc holds
        add("wave", [none[0], rare[0]], 8)
    return np.stack(pool), np.array(kind)


class Corpus:
    def __init__(self, T, n, share, base, seed, reps, sliced):
        from triple_hybrid_rag_amd import synth
        self.T, self.n, self.base = T, n, base
        self.v = v = synth.vocab_size(n)
        doc, term, tf = synth.lexical_rows(0, n, n)
        self.csr = csr = synth.build_lexical_csr(doc, term, tf, n, v)
        self.df = csr.df_local.astype(np.int64)
        self.idf = O.bm25_idf(n, csr.df_local)
        self.avgdl = csr.sum_dl_local / n
        self.share = share
        self.has_row = self.df >= share * n
        self.coll = (np.arange(n) * 7919 % 50).astype(np.int32)            # 50 collections of 2 % each
        self.coll[n // 2:] = np.where(np.arange(n - n // 2) % 2 == 0, 60, self.coll[n // 2:])   # + a fat one
        self.pool, self.kind = build_pool(self.df, self.has_row, n, v, seed, reps, sliced)
        P = len(self.pool)
        self.qc = np.array([-1, 7, 60, -1, 3][:5] * (P // 5 + 1), dtype=np.int32)[:P]   # unfiltered, thin, fat
        self.qc[::37] = 12345                                                # a collection no doc is in
        valid = (self.pool >= 0) & (self.pool < v)
        self.nt = valid.sum(axis=1)
        # probed for certain: a term with rows that is never walked (held by >= 1/64 of the docs)
        heavy_t = self.has_row & (self.df * 64 >= n)
        self.sure_probed = (self.nt <= 8) & (np.where(valid, heavy_t[np.clip(self.pool, 0, v - 1)], False).any(axis=1))
        self.any_row = (self.nt <= 8) & (np.where(valid, self.has_row[np.clip(self.pool, 0, v - 1)], False).any(axis=1))
        self.idx = self.index()
        slot = self.idx.lex["dense"][0].cpu().numpy()
        assert np.array_equal(slot >= 0, self.has_row), "the terms with rows are the ones held by >= share of the docs"
        self._exp = {}

    def index(self):
        c = self.csr
        idx = self.T.GpuIndex(doc_base=self.base).set_lexical(c.rowptr, c.post_doc, c.post_tf, c.doclen, self.idf,
                                                              self.avgdl, dense_share=self.share)
        return idx.set_collections(self.coll)

    def rows_of(self, *kinds):
        return np.nonzero(np.isin(self.kind, kinds))[0]

    def postings(self, rows):
        """Postings of all the lists of each of the pool rows ``rows``."""
        t = self.pool[rows]
        return np.where((t >= 0) & (t < self.v), self.df[np.clip(t, 0, self.v - 1)], 0).sum(axis=1)

    def expected(self, conjunctive, collections):
        """The oracle's lists of the pool at k = 128, as device arrays (ids padded with -1)."""
        key = (bool(conjunctive), bool(collections))
        if key not in self._exp:
            c = self.csr
            Se, Ie = O.bm25_topk(c.rowptr, c.post_doc, c.post_tf, c.doclen, self.idf, self.avgdl, self.pool, self.n,
                                 K_MAX, doc_id_base=self.base, conjunctive=key[0],
                                 doc_coll=self.coll if key[1] else None, query_coll=self.qc if key[1] else None)
            P = len(self.pool)
            S, I = np.zeros((P, K_MAX)), np.full((P, K_MAX), -1, dtype=np.int64)
            cnt = np.array([len(s) for s in Se], dtype=np.int32)
            for p in range(P):
                S[p, :cnt[p]], I[p, :cnt[p]] = Se[p], Ie[p]
            self._exp[key] = (dev(S), dev(I), dev(cnt))
        return self._exp[key]


def draw(rng, rows, N):
    """N pool rows: every one of ``rows`` when N allows it, then repeats, in a seeded order."""
    return rng.permutation(np.resize(rng.permutation(rows), N))


def check(c, rows, k, S, I, cnt, conjunctive, collections, what):
    ES, EI, Ecnt = c.expected(conjunctive, collections)
    r = dev(rows).long()
    ecnt = Ecnt[r].clamp(max=k)
    live = torch.arange(k, device=r.device)[None, :] < ecnt[:, None]
    ei = torch.where(live, EI[r][:, :k], torch.full_like(I, -1))
    bad = (cnt != ecnt) | (I != ei).any(dim=1) | ((S != ES[r][:, :k]) & live).any(dim=1)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        p = int(rows[i])
        n = int(ecnt[i])
        raise AssertionError(
            f"{what}: row {i} of {len(rows)} (pool row {p}, {c.kind[p]}, terms {c.pool[p][c.pool[p] != -1].tolist()}, "
            f"collection {c.qc[p] if collections else None}; {int(bad.sum())} rows differ): count {int(cnt[i])} != {n}"
            f" or ids {I[i, :n].tolist()} != {ei[i, :n].tolist()} or scores {S[i, :n].tolist()} != {ES[p, :n].tolist()}")


def search(c, rows, k=10, conjunctive=False, collections=True, prune=True, dense_rows=True, mt=MT, idx=None,
           what=""):
    """One bm25_search of the batch ``rows`` against the oracle; -> the call's control words."""
    idx = idx or c.idx
    N = len(rows)
    assert not (c.pool[rows][:, mt:] != -1).any()
    qd = dev(c.pool[rows][:, :mt])
    qc = dev(c.qc[rows]) if collections else None
    S, I, cnt = idx.bm25_search(qd, k, collections=qc, conjunctive=conjunctive, prune=prune, dense_rows=dense_rows)
    torch.cuda.synchronize()
    ctl = idx._ws_lex[:64].view(torch.int32).cpu().numpy().copy()   # (bm_layout: the control words are at offset 0)
    what = f"{what} N={N} k={k} and={conjunctive} coll={collections} prune={prune} rows={dense_rows} mt={mt}"
    assert S.shape == (N, k) and I.shape == (N, k) and cnt.shape == (N,)
    check(c, rows, k, S, I, cnt, conjunctive, collections, what)
    # what the planner did with the batch
    wave = prune and not conjunctive and k <= 64 and not BLOCK_WALK
    probing = prune and dense_rows and not conjunctive
    assert ctl[6] == min(64, (N + 255) // 256), f"{what}: plan workgroups {ctl[6]}"
    assert N <= ctl[0] <= 3 * N + 2 * WAVE_ITEMS, f"{what}: {ctl[0]} items"
    if probing:
        assert int(c.sure_probed[rows].sum()) <= ctl[3] <= int(c.any_row[rows].sum()), f"{what}: {ctl[3]} probed queries"
    else:
        assert ctl[3] == 0, f"{what}: {ctl[3]} probed queries without rows"
    if wave:   # the workgroup walk is left the queries without a term, and those of more than eight
        assert ctl[8] == int(((c.nt[rows] == 0) | (c.nt[rows] > 8)).sum()), f"{what}: {ctl[8]} workgroup-walk queries"
    else:
        assert ctl[8] == N - ctl[3], f"{what}: {ctl[8]} workgroup-walk queries"
    return ctl


@pytest.fixture(scope="module")
def small(T):
    """4000 docs, rows for the terms held by >= 1 % (415 of 2000 terms; the ones below 1/64 may be walked)."""
    return Corpus(T, 4000, 0.01, 700, 11, reps=8, sliced=False)


@pytest.fixture(scope="module")
def large(T):
    """80000 docs, rows for the terms held by >= 20 % (19): lists of up to 16 K postings are walked."""
    return Corpus(T, 80000, 0.2, 1000, 12, reps=8, sliced=True)


# --------------------------------------------------------------------------- the small corpus: batch size
@pytest.mark.parametrize("N", [1, 255, 256, 257, 511, 512, 513, 1023, 1025, 4097,      # PLAN_THREADS / FILTER_THREADS edges
                               16383, 16384, 16385, 20000, 40000])                    # 64 plan workgroups; BM_WAVE_ITEMS
def test_batch_sizes(small, N):
    """The mixed pool at every edge of the planner: ceil(N / 256) plan workgroups and the hand-over to
    the last one, queries per thread 1 -> 2 of the plan's part 2 and of the sweep filter, the
    grid-stride part 1 above 64 * 256 queries, and batches beyond the waves' 16384 tuned slots."""
    c = small
    rows = draw(np.random.default_rng(N), np.arange(len(c.pool)), N)
    ctl = search(c, rows, what="batch size")
    if N >= 4097:
        assert ctl[5] > 0, "no sweep ran: the probed-only queries of the pool have no stage A to rule theirs out"


def test_sweep_filter_beyond_its_mask(small):
    """65600 queries: 65 per thread of bm25_sweep_filter_kernel, one more than its 64-bit ``live``
    mask holds, so the 65th is decided again in the second loop.  Most queries are probed, and the
    probed-only ones always sweep (no stage A, no threshold)."""
    c = small
    N = 65600
    rng = np.random.default_rng(5)
    rows = draw(rng, np.concatenate([c.rows_of("probed", "pw", "rowwalk")] * 3 + [np.arange(len(c.pool))]), N)
    per = (N + 1023) // 1024
    assert per == 65 and ((np.arange(N) % per == 64) & (c.kind[rows] == "probed")).sum() > 100   # sweeping 65th queries
    ctl = search(c, rows, what="sweep filter")
    only = int((c.kind[rows] == "probed").sum())
    assert ctl[5] >= only and ctl[3] > N // 2, f"{ctl[5]} sweep items for {only} probed-only queries"


@pytest.mark.parametrize("conjunctive,prune,dense_rows,k,collections", [
    (False, True, True, 1, True), (False, True, True, 64, True), (False, True, True, 65, True),
    (False, True, True, 128, True), (False, True, True, 64, False), (False, True, True, 65, False),
    (False, True, False, 10, True), (False, False, True, 10, True), (True, True, True, 10, True),
    (True, False, True, 65, False), (True, True, True, 128, False)])
def test_modes_over_a_big_batch(small, conjunctive, prune, dense_rows, k, collections):
    """20000 queries of the mixed pool in every mode: k 64 -> 65 (and AND, and no bounds) moves every
    query from the waves to the workgroup walk; without rows every query of <= 8 terms is the waves'."""
    c = small
    rows = draw(np.random.default_rng(k), np.arange(len(c.pool)), 20000)
    search(c, rows, k=k, conjunctive=conjunctive, collections=collections, prune=prune, dense_rows=dense_rows,
           what="modes")


@pytest.mark.parametrize("N", [3000, 20000])
@pytest.mark.parametrize("kinds,mt", [(("wave",), 8), (("wave",), MT), (("probed",), 8), (("pw", "probed"), MT),
                                      (("block", "empty"), MT)])
def test_homogeneous_batches(small, kinds, mt, N):
    """Batches of one kind: nothing for the workgroup walk (its launches return at once), nothing
    for the waves, every query probed (the fused-launch choice of the workgroup walk)."""
    c = small
    rows = c.rows_of(*kinds)
    if mt < MT:
        rows = rows[(c.pool[rows][:, mt:] == -1).all(axis=1)]
    assert len(rows) >= 10
    ctl = search(c, draw(np.random.default_rng(N + mt), rows, N), mt=mt, what=f"all {'+'.join(kinds)}")
    if not BLOCK_WALK:
        if kinds == ("wave",):
            assert ctl[8] == 0 and ctl[3] == 0 and ctl[5] == 0
        elif "probed" in kinds:
            assert ctl[8] == 0 and ctl[3] == N
        else:
            assert ctl[8] == N and ctl[3] == 0


@pytest.mark.parametrize("N", [1000, 16000, 17000, 30000])
def test_permutation_invariance(small, N):
    """The same multiset of queries in two orders: every query keeps its row, bit for bit."""
    c = small
    rng = np.random.default_rng(N)
    rows = draw(rng, np.arange(len(c.pool)), N)
    perm = rng.permutation(N)
    out = []
    for r in (rows, rows[perm]):
        S, I, cnt = c.idx.bm25_search(dev(c.pool[r]), 10, collections=dev(c.qc[r]))
        check(c, r, 10, S, I, cnt, False, True, f"order N={N}")
        out.append((S.clone(), I.clone(), cnt.clone()))
    p = dev(perm).long()
    live = torch.arange(10, device=p.device)[None, :] < out[0][2][p][:, None]
    assert torch.equal(out[0][2][p], out[1][2]) and torch.equal(out[0][1][p], out[1][1])
    assert torch.equal(torch.where(live, out[0][0][p], 0.0), torch.where(live, out[1][0], 0.0))


def test_workspace_reuse(small):
    """One index searched with 40000, then 3, then 20000 queries: the kept workspace is larger than
    the later calls need and holds the earlier calls' item lists behind the live ones."""
    c = small
    idx = c.index()
    size = None
    for N in (40000, 3, 20000, 16385, 1):
        search(c, draw(np.random.default_rng(N), np.arange(len(c.pool)), N), idx=idx, what="reuse")
        size = size or idx._ws_lex.numel()
        assert idx._ws_lex.numel() == size == c.T._native.bm25_workspace_bytes(40000, MT, 10)


# --------------------------------------------------------------------------- the large corpus: sliced queries
def test_one_query_of_more_than_the_most_slices(large):
    """Eight lists without rows, > 128 * 640 postings together: alone in its batch the query is cut
    at the smallest wave slice size and capped at BM_MAX_SLICES."""
    c = large
    rows = c.rows_of("longwave")
    tot = c.postings(rows)
    p = rows[int(np.argmax(tot))]
    assert tot.max() > BM_MAX_SLICES * WW_TARGET_MIN
    ctl = search(c, np.array([p]), what="one long query")
    if not BLOCK_WALK:
        assert ctl[0] == BM_MAX_SLICES and ctl[7] == WW_TARGET_MIN
    ctl = search(c, np.array([p]), k=65, what="one long query, workgroup walk")
    assert ctl[0] > 1


@pytest.mark.parametrize("N", [3, 64, 257, 1025, 3000])
def test_sliced_batches(large, N):
    """The mixed pool over lists of up to 16 K postings (walked) and 80 K (probed, swept): a query is
    many slices in a small batch and few in a large one; the items behind the first N are the
    slices s >= 1, query by query."""
    c = large
    rows = draw(np.random.default_rng(N), np.arange(len(c.pool)), N)
    lw = c.rows_of("longwave")
    rows[N // 2] = lw[int(np.argmax(c.postings(lw)))]       # (a query of > 128 * 640 walked postings in every batch)
    ctl = search(c, rows, what="sliced")
    assert ctl[0] > N, f"{ctl[0]} items: no query was sliced"
    if N <= 64 and not BLOCK_WALK:
        assert ctl[7] == WW_TARGET_MIN and ctl[0] >= N + BM_MAX_SLICES - 1


@pytest.mark.parametrize("k,collections", [(10, True), (64, False)])
def test_fit_loop_doubles_the_wave_slice_size(large, k, collections):
    """1500 wave-walked queries of ~100 K postings: at the largest tuned slice size (1536) they are
    ~100 K slices, the waves have 16384 + 1500 slots: the fit loop doubles the waves' slice size (and
    only theirs) until they fit."""
    c = large
    N = 1500
    rows = draw(np.random.default_rng(k), c.rows_of("longwave"), N)
    assert np.minimum(BM_MAX_SLICES, -(-c.postings(rows) // WW_TARGET_MAX)).sum() > N + WAVE_ITEMS
    ctl = search(c, rows, k=k, collections=collections, what="wave slice size doubled")
    if not BLOCK_WALK:
        assert ctl[7] > WW_TARGET_MAX and ctl[7] % WW_TARGET_MAX == 0, f"stage-A slice size {ctl[7]}"
        assert N < ctl[0] <= N + WAVE_ITEMS


@pytest.mark.parametrize("conjunctive,prune", [(True, True), (False, False), (True, False)])
def test_fit_loop_doubles_the_shared_slice_size(large, conjunctive, prune):
    """1000 queries of 12 - 32 of the longest lists on the workgroup walk (AND, or no bounds): ~25
    slices each at 24576 postings, the list has 2 * 1000 + 16384 slots: the shared slice size doubles."""
    c = large
    N = 1000
    rows = draw(np.random.default_rng(3), c.rows_of("bigblock"), N)
    assert np.minimum(BM_MAX_SLICES, -(-c.postings(rows) // BM_TARGET0)).sum() > 2 * N + WAVE_ITEMS
    ctl = search(c, rows, conjunctive=conjunctive, prune=prune, what="shared slice size doubled")
    assert ctl[7] > BM_TARGET0 and ctl[7] % BM_TARGET0 == 0, f"slice size {ctl[7]}"
    assert N < ctl[0] <= 2 * N + WAVE_ITEMS


def test_modes_over_sliced_queries(large):
    """2000 sliced queries of the mixed pool in the other modes: AND, no bounds, no rows, k = 65 / 128."""
    c = large
    rows = draw(np.random.default_rng(8), np.arange(len(c.pool)), 2000)
    for conjunctive, prune, dense_rows, k in ((True, True, True, 10), (False, False, True, 10), (False, True, False, 64),
                                              (False, True, True, 65), (False, True, True, 128)):
        search(c, rows, k=k, conjunctive=conjunctive, prune=prune, dense_rows=dense_rows, what="sliced modes")


# --------------------------------------------------------------------------- the alternate walks
@pytest.mark.parametrize("knobs", ["THR_BM25_WALK=block", "THR_BM25_SHAPE=small"])
def test_alternate_walks_over_big_batches_in_a_subprocess(knobs):
    """THR_BM25_WALK=block (every query on the workgroup walk, stage A included) and
    THR_BM25_SHAPE=small (256-thread workgroups) are read once per process: the batch-size cases
    around and above 16384 queries, the sweep filter's and the fit loop's run again under each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    if env.get("THR_BM25_KNOB_RUN"):
        pytest.skip("already inside a knob run")
    env["THR_BM25_KNOB_RUN"] = "1"
    name, value = knobs.split("=")
    env[name] = value
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "test_batch_sizes and (257 or 16385 or 20000) or test_sweep_filter_beyond_its_mask or "
                          "test_fit_loop or test_one_query"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and "10 passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-3000:] + out.stderr[-1000:]
