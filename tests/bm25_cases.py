"""Inputs and reference of the BM25 value-edge tests (tests/test_bm25_cases_host.py checks what the
builders promise, on the CPU; tests/test_gpu_bm25_values.py runs them through thr_bm25_bounds,
thr_bm25_dense_rows and thr_bm25_topk).  Pure numpy: nothing here needs a GPU.

The reference of every case is oracle.thr_oracle.bm25_topk with the case's own k1 and b; every
comparison is bit for bit.  The other BM25 tests score synth.lexical_rows (tf = 1 + Geometric(0.5),
dl / avgdl near 1, idf from bm25_idf, k1 = 1.2, b = 0.75): the pruning arithmetic in the middle of
its range.  The corpora here are written posting by posting to stand at its ends: impacts that
saturate the 8-bit quantiser beside impacts near zero, term frequencies on both sides of the
16-bit rows' sign and range edges, idf from 0.0 and the smallest allowed value to 30, k1 = 0 and
b in {0, 1}, top-k lists that exist only through the stage-B sweep, and ties laid across slice edges.

``idf``, ``avgdl`` and ``doclen`` are INPUTS of every corpus, set by its builder: they do not follow
from the rows (a doc's length is not the sum of its term frequencies, a term's idf says nothing
about its df).  That is what a document shard passes -- global statistics over local rows -- and
what thr_bm25_topk is specified for.

Three corpora, each with a table of named queries; a case is a set of rows of one table:

* values (3000 docs, avgdl 2000): saturate, tf_ladder, idf_spread, conj_values, and k1b -- the
  whole table under four (k1, b);
* stageb (3000 docs, avgdl 100): stage_b_wins, stage_b_skipped, stage_b_tie;
* sliced (40000 docs, avgdl 100): slice_ties and slice_saturate -- every term is held by every doc,
  more than one slice's 24576 postings, so each query is cut into doc-range slices that share a
  threshold.

In the small corpora a query is at most 8192 postings: one item of the workgroup walk, one sweep.
"""
import functools

import numpy as np

from oracle import thr_oracle as O

MT = 8                           # term columns of the query tables
K_MAX = 128                      # THR_TOPK_MAX: the oracle's lists are cut once, a top-k is a prefix
KS = (10, 65, 128)               # the wave walk; the workgroup walk (k > 64)
SLICE_KS = (1, 10, 64, 65, 128)  # slice_ties: 64 -> 65 is the switch from the waves to the workgroups
DEFAULT = (1.2, 0.75)
K1B = ((1.2, 0.75), (0.0, 0.75), (2.0, 0.0), (1.2, 1.0))
BM_TARGET0 = 24576               # bm25_plan.hip: postings per slice aimed at when the batch fills the chip
WW_TARGET_MIN, WW_TARGET_MAX = 640, 1536   # ... and per stage-A slice of the wave walk

# The smallest idf bm25_idf yields for a corpus of 2^31 docs -- the most thr_bm25_topk indexes (doc
# ids are int32): idf = ln(1 + (N - df + 0.5) / (df + 0.5)) is smallest at df = N, where it is
# ln(1 + 0.5 / (N + 0.5)) = 0.5 / (2^31 + 0.5) - ... = 2.328e-10.
IDF_TINY = float(O.bm25_idf(2 ** 31, np.array([2 ** 31]))[0])
IDF_HUGE = 30.0                  # (bm25_idf never exceeds ln(2 N + 2) = 22.2 for 2^31 docs)
IDF_MIN = 1e-300                 # the smallest positive idf bm25_check_params lets through (thr_hip.h, a3)


class Corpus:
    """rowptr / post_doc / post_tf: the CSR, terms in the order they were added, docs ascending.
    term[name] -> term id; queries int32 [P, MT] (-1 = padding), qname[P], qcase[P] (the case a row
    belongs to), qcoll[P] or None (-1 = unfiltered)."""

    def __init__(self, name, n, doclen, avgdl, share):
        self.name, self.n, self.avgdl, self.share = name, n, float(avgdl), float(share)
        self.doclen = np.asarray(doclen, dtype=np.float32)
        assert self.doclen.shape == (n,)
        self.term, self._lists, self._idf = {}, [], []
        self._q, self.qname, self.qcase, self._qc = [], [], [], []
        self.coll = None

    # ---- building
    def add_term(self, name, docs, tf, idf):
        docs = np.asarray(docs, dtype=np.int64)
        assert name not in self.term and np.all(np.diff(docs) > 0) and (len(docs) == 0 or (0 <= docs[0] and docs[-1] < self.n))
        tf = np.broadcast_to(np.asarray(tf, dtype=np.int64), docs.shape)
        assert np.all(tf >= 1) and np.all(tf <= 2 ** 31 - 1)
        self.term[name] = len(self._lists)
        self._lists.append((docs.astype(np.int32), tf.astype(np.int32)))
        self._idf.append(float(idf))

    def add_query(self, case, name, terms, coll=-1):
        row = np.full(MT, -1, dtype=np.int32)
        row[:len(terms)] = [self.term[t] for t in terms]
        self._q.append(row)
        self.qname.append(name)
        self.qcase.append(case)
        self._qc.append(coll)

    def finish(self):
        self.rowptr = np.concatenate([[0], np.cumsum([len(d) for d, _ in self._lists])]).astype(np.int64)
        self.post_doc = np.concatenate([d for d, _ in self._lists]).astype(np.int32)
        self.post_tf = np.concatenate([t for _, t in self._lists]).astype(np.int32)
        self.idf = np.array(self._idf, dtype=np.float64)
        self.v = len(self._lists)
        self.df = np.diff(self.rowptr)
        self.queries = np.stack(self._q)
        self.qcase = np.array(self.qcase)
        self.qcoll = np.array(self._qc, dtype=np.int32) if self.coll is not None else None
        self.post_term = np.repeat(np.arange(self.v), self.df)
        # the terms that get per-doc rows (_native.bm25_dense_terms): held by >= share of the docs, tf <= 65535
        self.max_tf = np.array([int(t.max()) if len(t) else 0 for _, t in self._lists], dtype=np.int64)
        self.has_row = (self.df >= self.share * self.n) & (self.max_tf <= 65535) & (self.df > 0)
        for a in (self.rowptr, self.post_doc, self.post_tf, self.idf, self.doclen, self.queries):
            a.setflags(write=False)
        return self

    # ---- reading
    def docs_of(self, name):
        return self._lists[self.term[name]][0].astype(np.int64)

    def tf_of(self, name):
        return self._lists[self.term[name]][1].astype(np.int64)

    def rows(self, case):
        return np.flatnonzero(self.qcase == case)

    def row(self, name):
        return self.qname.index(name)

    def terms_of(self, p):
        t = self.queries[p]
        return t[(t >= 0) & (t < self.v)]

    def probing(self, p):
        """Does the OR form of row p hold a term with rows?  (Every term with rows here is held by
        >= 1/64 of the docs, so bm25_plan_kernel always probes it: the host test checks that.)"""
        t = self.terms_of(p)
        return len(t) <= 8 and bool(self.has_row[t].any())


# ------------------------------------------------------------------------------------ the arithmetic
def impacts(c, k1, b):
    """Per posting, float64 with the oracle's operations: (impact, contribution, x = impact * 255 /
    (k1 + 1) -- what bm25_bounds_kernel takes the ceiling of)."""
    k1, b, avgdl = np.float64(k1), np.float64(b), np.float64(c.avgdl)
    tf = c.post_tf.astype(np.float64)
    dl = c.doclen[c.post_doc].astype(np.float64)
    nrm = k1 * ((1.0 - b) + b * (dl / avgdl))
    imp = (tf * (k1 + 1.0)) / (tf + nrm)
    con = c.idf[c.post_term] * imp
    x = imp * (255.0 / (k1 + 1.0))
    return imp, con, x


def quantised(x):
    """post_imp as thr_hip.h states it: ceil(x) + 1, clipped to 255."""
    return np.minimum(np.ceil(x) + 1.0, 255.0).astype(np.uint8)


def clipped(x):
    """The postings whose quantised impact the clip at 255 cuts: ceil(x) + 1 > 255."""
    return x > 254.0


def bounds(c, k1, b):
    """-> (term_ub [V], block_ub [ceil(nnz / 128)]): the maxima of the oracle's contribution, 0.0 for
    a term without postings."""
    _, con, _ = impacts(c, k1, b)
    term_ub = np.zeros(c.v)
    for t in range(c.v):
        if c.df[t]:
            term_ub[t] = con[c.rowptr[t]:c.rowptr[t + 1]].max()
    nb = (len(con) + 127) // 128
    block_ub = np.array([con[128 * j:128 * j + 128].max() for j in range(nb)])
    return term_ub, block_ub


@functools.lru_cache(maxsize=None)
def expected(cname, k1=DEFAULT[0], b=DEFAULT[1], conjunctive=False, base=0):
    """The oracle's lists of every row of a corpus' table at k = 128: (S [P, 128], I [P, 128] padded
    with -1, cnt [P]).  Shared by every test and left unchanged."""
    c = corpus(cname)
    Se, Ie = O.bm25_topk(c.rowptr, c.post_doc, c.post_tf, c.doclen, c.idf, c.avgdl, c.queries, c.n, K_MAX,
                         doc_id_base=base, k1=k1, b=b, conjunctive=conjunctive, doc_coll=c.coll, query_coll=c.qcoll)
    P = len(c.queries)
    S, I = np.zeros((P, K_MAX)), np.full((P, K_MAX), -1, dtype=np.int64)
    cnt = np.array([len(s) for s in Se], dtype=np.int32)
    for p in range(P):
        S[p, :cnt[p]], I[p, :cnt[p]] = Se[p], Ie[p]
    for a in (S, I, cnt):
        a.setflags(write=False)
    return S, I, cnt


def all_scores(c, p, k1=DEFAULT[0], b=DEFAULT[1], conjunctive=False):
    """The oracle's score of every doc for row p (-inf: not a result)."""
    mask = None
    if c.coll is not None and c.qcoll[p] != -1:
        mask = c.coll == c.qcoll[p]
    return O.bm25_scores(c.rowptr, c.post_doc, c.post_tf, c.doclen, c.idf, c.avgdl, [int(t) for t in c.queries[p]],
                         c.n, k1, b, conjunctive, mask)


# ------------------------------------------------------------------------------------------- values
N_SMALL = 3000
SHARE_SMALL = 0.05                                   # rows from df >= 150 (and every such term has df >= n / 64)
SAT_TF = (1000, 4096, 32767, 32768, 65535, 50000)    # saturated postings: x > 254 at the default k1, b
LADDER_TF = (1, 2, 255, 256, 32767, 32768, 65535)    # in docs LADDER0 ..: both sides of int16's and uint16's ends
LADDER0 = 1500


def _near_dl(x, tf=1000.0, avgdl=2000.0, k1=1.2, b=0.75):
    """The doc length at which a posting of ``tf`` has impact * 255 / (k1 + 1) = x (to within the
    rounding to an integer length)."""
    nrm = tf * (255.0 / x - 1.0)
    return float(round((nrm / k1 - (1.0 - b)) / b * avgdl))


def values():
    """Doc d is of one of three kinds by d % 3, and every term's postings follow the kind:
    0 "saturated" -- dl 1000 .. 3976, tf from SAT_TF: x > 254, the quantiser clips;
    1 "near"      -- tf 1000 and the dl that puts x at 253.5 or 252.5: the last unclipped steps;
    2 "zero"      -- dl = 2^24, tf 1: impact 0.0003, x = 0.03.
    Docs 1500 .. 1519 have dl 100 and belong to the ladder terms."""
    n = N_SMALL
    d = np.arange(n)
    dl = np.where(d % 3 == 0, 1000.0 + (d % 97) * 31.0,
                  np.where(d % 3 == 1, np.where((d // 3) % 2 == 0, _near_dl(253.5), _near_dl(252.5)), 2.0 ** 24))
    dl[LADDER0:LADDER0 + 20] = 100.0
    c = Corpus("values", n, dl, avgdl=2000.0, share=SHARE_SMALL)

    def kind_tf(docs, j):
        return np.where(docs % 3 == 0, np.array(SAT_TF)[(docs // 3 + j) % len(SAT_TF)], np.where(docs % 3 == 1, 1000, 1))

    def pick(*conds):
        m = np.zeros(n, dtype=bool)
        for cond in conds:
            m |= cond
        return d[m]

    for j in range(8):       # walked (df 144): the 120 docs of d % 25 == 0 hold all eight
        docs = pick(d % 25 == 0, d % 125 == j + 1)
        c.add_term(f"S{j}", docs, kind_tf(docs, j), 2.0 + 0.125 * j)
    for j in range(8):       # with rows (df 236): the 215 docs of d % 14 == 0 hold all eight
        docs = pick(d % 14 == 0, d % 140 == j + 1)
        c.add_term(f"P{j}", docs, kind_tf(docs, j + 3), 0.5 + 0.0625 * j)
    docs = pick(d % 5 != 0)  # the majority term of k1b (df 2400, rows)
    c.add_term("W", docs, 1 + docs % 3, 0.25)
    # tf_ladder: L (rows), its twin L2 with one posting of 65536 (no rows: walked), L3 with 2^24 and 2^31 - 1
    ladder = np.arange(LADDER0, LADDER0 + len(LADDER_TF))
    docs = pick(d % 15 == 7, np.isin(d, ladder))
    tf = np.where(np.isin(docs, ladder), np.array(LADDER_TF)[np.clip(docs - LADDER0, 0, len(LADDER_TF) - 1)], 1 + docs % 5)
    c.add_term("L", docs, tf, 1.0)
    c.add_term("L2", docs, np.where(tf == 65535, 65536, tf), 1.0)
    docs = pick(d % 15 == 8, np.isin(d, (LADDER0 + 10, LADDER0 + 11)))
    c.add_term("L3", docs, np.where(docs == LADDER0 + 10, 2 ** 24, np.where(docs == LADDER0 + 11, 2 ** 31 - 1, 1 + docs % 5)), 1.0)
    c.add_term("RARE", np.array([33, LADDER0 + 3, LADDER0 + 5, LADDER0 + 6, LADDER0 + 10, LADDER0 + 11, 2801]), 1, 6.0)
    for j in range(8):       # eight equal idfs (walked, df 144; 24 docs hold all eight)
        docs = pick(d % 25 == j + 10, d % 125 == 60)
        c.add_term(f"E{j}", docs, 1 + docs % 4, 1.5)
    for j, (name, idf) in enumerate((("T_TINY", IDF_TINY), ("T_ZERO", 0.0), ("T_HUGE", IDF_HUGE), ("T_MIN", IDF_MIN))):
        docs = pick(d % 25 == 20 + j)                                    # walked (df 120)
        c.add_term(name, docs, 1 + docs % 6, idf)
    for j, (name, idf) in enumerate((("PT_TINY", IDF_TINY), ("PT_ZERO", 0.0), ("PT_HUGE", IDF_HUGE), ("PT_MIN", IDF_MIN))):
        docs = pick(d % 15 == 10 + j)                                    # with rows (df 200)
        c.add_term(name, docs, 1 + docs % 6, idf)
    c.add_term("EMPTY", np.zeros(0, dtype=np.int64), 1, 4.0)             # a term no doc holds: its bound is 0.0

    S, P, E = [f"S{j}" for j in range(8)], [f"P{j}" for j in range(8)], [f"E{j}" for j in range(8)]
    for name, terms in (("S1", S[:1]), ("S2", S[:2]), ("S8", S), ("P1", P[:1]), ("P2", P[:2]), ("P8", P),
                        ("S1P1", [S[0], P[0]]), ("S4P4", S[:4] + P[:4])):
        c.add_query("saturate", name, terms)
    for name, terms in (("L", ["L"]), ("L2", ["L2"]), ("L3", ["L3"]), ("RARE+L", ["RARE", "L"]), ("RARE+L2", ["RARE", "L2"]),
                        ("RARE+L3", ["RARE", "L3"]), ("L+RARE", ["L", "RARE"]), ("L+L2+L3", ["L", "L2", "L3"])):
        c.add_query("tf_ladder", name, terms)
    for name, terms in (("tiny+huge", ["T_TINY", "T_HUGE"]), ("all_zero", ["T_ZERO", "PT_ZERO"]), ("zero", ["T_ZERO"]),
                        ("zero_row", ["PT_ZERO"]), ("one_zero", ["T_ZERO", "T_HUGE", "S0"]), ("equal8", E),
                        ("same8", ["S0"] * 8), ("row_tiny+huge", ["PT_TINY", "T_HUGE"]), ("row_huge+tiny", ["PT_HUGE", "T_TINY"]),
                        ("rows_tiny+zero+huge", ["PT_TINY", "PT_ZERO", "PT_HUGE"]), ("row_huge+rare", ["PT_HUGE", "RARE"]),
                        ("min", ["T_MIN"]), ("min+huge", ["T_MIN", "T_HUGE"]), ("row_min", ["PT_MIN"]),
                        ("row_min+tiny", ["PT_MIN", "T_TINY"]), ("empty", ["EMPTY"]), ("empty+tiny", ["EMPTY", "T_TINY"])):
        c.add_query("idf_spread", name, terms)
    for name, terms in (("W", ["W"]), ("W+RARE", ["W", "RARE"]), ("RARE+W", ["RARE", "W"])):
        c.add_query("k1b", name, terms)
    return c.finish()


# ------------------------------------------------------------------------------------------- stageb
TIE_LOW, TIE_HIGH = (0, 400), (2500, 2900)      # stage_b_tie: the D2-only docs, the docs with R0 too


def stageb():
    """dl = 100 = avgdl but for the docs of R.  D, D2, PZ have rows and are probed; R, R2, R0 are walked.
    stage_b_wins    [R, D]:   R's 100 docs have dl = 2^22, impact ~ 0: stage A's k-th score is far below
                              D's bound, the sweep runs, and the best docs hold D and not R;
    stage_b_skipped [R2, D]:  idf[R2] = 5: D's bound 1.76 lies below the k-th of R2's 100 docs;
    stage_b_tie     [R0, D2]: idf[R0] = 0.0; the docs with R0 and D2 (ids 2500 ..) score (0 + 0) + c, c the
                              largest contribution of D2, which 100 docs with D2 alone (ids below 400) also
                              score: the probed bound EQUALS stage A's threshold, and the lower ids win;
                    [R0, PZ]: the same with idf[PZ] = 0.0: bound and threshold are both 0.0."""
    n = N_SMALL
    d = np.arange(n)
    dl = np.full(n, 100.0)
    dl[2000:2100] = 2.0 ** 22
    c = Corpus("stageb", n, dl, avgdl=100.0, share=SHARE_SMALL)
    docs = d[d % 4 == 0]
    c.add_term("D", docs, 1 + docs % 3, 0.8)
    c.add_term("R", d[2000:2100], 1, 3.0)
    docs = d[1000:1100]
    c.add_term("R2", docs, 1 + docs % 4, 5.0)
    docs = d[d % 4 == 1]
    tied = (docs < TIE_LOW[1]) | ((docs >= TIE_HIGH[0]) & (docs < TIE_HIGH[1]))
    c.add_term("D2", docs, np.where(tied, 3, 1), 0.8)
    c.add_term("R0", d[(d >= TIE_HIGH[0]) & (d < TIE_HIGH[1]) & ((d % 4 == 1) | (d % 16 == 3))], 2, 0.0)   # (df 125: no rows)
    c.add_term("PZ", d[d % 4 == 2], 1, 0.0)
    c.add_query("stage_b_wins", "R+D", ["R", "D"])
    c.add_query("stage_b_wins", "D+R", ["D", "R"])
    c.add_query("stage_b_skipped", "R2+D", ["R2", "D"])
    c.add_query("stage_b_skipped", "D+R2", ["D", "R2"])
    c.add_query("stage_b_tie", "R0+D2", ["R0", "D2"])
    c.add_query("stage_b_tie", "D2+R0", ["D2", "R0"])
    c.add_query("stage_b_tie", "R0+PZ", ["R0", "PZ"])
    return c.finish()


# ------------------------------------------------------------------------------------------- sliced
N_SLICED = 40000
LAST_FROM = 39800                # slice_ties "last": the docs that score higher (inside the last slice of every cut)
SPREAD_EVERY = 250               # slice_ties "spread": one better doc per 250 (160 of them: more than k)
KEEP_EVERY = 50                  # the collection filter keeps every 50th doc


def sliced():
    """Every term is held by every doc with dl = 100 = avgdl (rows: the sweep is cut into doc ranges; without
    the rows the walks are).  ALL: tf 2 everywhere -- 40000 docs tie.  LAST: tf 3 from doc 39800 on.
    SPREAD: tf 3 in every 250th doc.  SAT0 .. SAT7 (slice_saturate): tf 1000 .. 61000, impact * 255 / (k1 + 1)
    above 254 in every posting -- a doc's eight clipped impacts are the largest sum a 16-bit accumulator takes,
    here in items that start with the other slices' threshold.  Each query runs unfiltered and inside
    collection 1 = every 50th doc."""
    n = N_SLICED
    d = np.arange(n)
    c = Corpus("sliced", n, np.full(n, 100.0), avgdl=100.0, share=0.5)
    c.add_term("ALL", d, 2, 1.0)
    c.add_term("LAST", d, np.where(d >= LAST_FROM, 3, 2), 1.0)
    c.add_term("SPREAD", d, np.where(d % SPREAD_EVERY == 0, 3, 2), 1.0)
    for j in range(8):       # slice_saturate: every posting clips the quantiser, every doc holds all eight
        c.add_term(f"SAT{j}", d, 1000 + (d * (7919 + 104729 * j)) % 60001, 2.0 + 0.125 * j)
    c.coll = (d % KEEP_EVERY == 0).astype(np.int32)
    for coll in (-1, 1):
        tag = "" if coll < 0 else "/filtered"
        c.add_query("slice_saturate", "sat1" + tag, ["SAT0"], coll)
        c.add_query("slice_saturate", "sat8" + tag, [f"SAT{j}" for j in range(8)], coll)
        for name, terms in (("all", ["ALL"]), ("last", ["LAST"]), ("spread", ["SPREAD"]), ("all+last", ["ALL", "LAST"]),
                            ("spread+last", ["SPREAD", "LAST"])):
            c.add_query("slice_ties", name + tag, terms, coll)
    return c.finish()


BUILDERS = {"values": values, "stageb": stageb, "sliced": sliced}


@functools.lru_cache(maxsize=None)
def corpus(name):
    return BUILDERS[name]()


class Case:
    """Rows of one corpus' table under one (k1, b).  ``conj``: the AND form is run instead of the OR form."""

    def __init__(self, name, cname, rows_of, params=DEFAULT, conj=False, ks=KS):
        self.name, self.cname, self.rows_of, self.params, self.conj, self.ks = name, cname, rows_of, params, conj, ks

    @property
    def corpus(self):
        return corpus(self.cname)

    @property
    def rows(self):
        c = self.corpus
        if self.rows_of is None:
            return np.arange(len(c.queries))
        return np.concatenate([c.rows(r) for r in self.rows_of])

    def expected(self, conjunctive=None, base=0):
        return expected(self.cname, self.params[0], self.params[1], self.conj if conjunctive is None else conjunctive, base)


CASES = {}
for _name in ("saturate", "tf_ladder", "idf_spread"):
    CASES[_name] = Case(_name, "values", (_name,))
for _k1, _b in K1B:
    CASES[f"k1b-{_k1}-{_b}"] = Case(f"k1b-{_k1}-{_b}", "values", None, (_k1, _b))
CASES["conj_values"] = Case("conj_values", "values", ("saturate", "tf_ladder"), conj=True)
for _name in ("stage_b_wins", "stage_b_skipped", "stage_b_tie"):
    CASES[_name] = Case(_name, "stageb", (_name,))
CASES["slice_ties"] = Case("slice_ties", "sliced", ("slice_ties",), ks=SLICE_KS)
CASES["slice_saturate"] = Case("slice_saturate", "sliced", ("slice_saturate",), ks=(10, 65))
