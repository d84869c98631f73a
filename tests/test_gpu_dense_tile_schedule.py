"""The whole-tile schedule of dense_scan_f16qs (one barrier per 32-row tile, a ring of whole-tile LDS buffers,
group B emitting the previous tile before it multiplies) against the CPU oracle, bit for bit, at the
corpus sizes at which a block's own tile count takes every value the ring's bookkeeping distinguishes.

With one query tile (<= 256 queries) the filter scan runs 8 * min(32, max(1, tiles / 8)) blocks (scan_grid),
block b owning tiles b, b + blocks, ...; with two query tiles (257 and 300 queries) half as many row
slices, so twice the tiles per block.  The last tile of every corpus is partly padding.

    rows      tiles   blocks   own tiles per block (one query tile)   (two query tiles: 128 slices)
    40        2       8        0 or 1                                 0 or 1  (8 slices)
    8 200     257     256      1 or 2                                 2 or 3
    19 600    613     256      2 or 3                                 4 or 5
    28 010    876     256      3 or 4  (the first wrap of 3 buffers)  6 or 7
    57 400    1794    256      7 or 8                                 14 or 15

Batches: 1 query (seven padding waves, in both groups), 33, 255, 257 (a second query tile of one live wave), 300.
Every corpus has a row without an embedding.  Required of every case: zero rescues, every query certified.

One corpus, one index and one oracle run (300 queries) per (rows, dim), shared and left unchanged; the
smaller batches are prefixes of the 300 queries.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_cases import assert_topk_equal, dev, rand_docs  # noqa: E402
from dense_emit_cases import (CAND_BYTES, CAND_CAP, SAMPLE_TOP, carve, plan, scan_slack,  # noqa: E402
                              segment_of_row, unpack_copy16)

K, NQ_MAX = 10, 300
ROWS = (40, 8200, 19600, 28010, 57400)
MID = 19600
DIMS = (512, 768)
BATCHES = (1, 33, 255, 257, 300)
SHAPE = 32 if os.environ.get("THR_DENSE_MFMA") == "32" else 16     # the knob, as dense_knobs() reads it
SEGS = 2 if SHAPE == 32 else 4                                     # segments per row slice (QAcc::SEGS)
COLL_SMALL, COLL_BIG = 7, 60


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def collections(n):
    """50 collections of 2 % of the rows each; in the second half every other row belongs to collection
    60 instead (25 % of the corpus)."""
    coll = (np.arange(n) * 7919 % 50).astype(np.int32)
    coll[n // 2:] = np.where(np.arange(n - n // 2) % 2 == 0, COLL_BIG, coll[n // 2:])
    return coll


@functools.lru_cache(maxsize=None)
def corpus(n, d):
    """Unit rows, row 5 without an embedding; every other query a neighbour of a random row >= 6."""
    x, rng = rand_docs(n, d, 5200 + d + n)
    x[5] = 0
    q = rng.standard_normal((NQ_MAX, d)).astype(np.float32)
    q[::2] = x[rng.integers(6, n, len(q[::2]))] + 0.5 * q[::2]
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


@functools.lru_cache(maxsize=None)
def oracle(n, d):
    x, q = corpus(n, d)
    out = CO.dense_topk_exact(x, q, K)
    for a in out:
        a.setflags(write=False)
    return out


_index = {}


def index(T, n, d):
    if (n, d) not in _index:
        _index[(n, d)] = T.GpuIndex().set_dense(corpus(n, d)[0], shortlist="f16").set_collections(collections(n))
    return _index[(n, d)]


def certified(T, idx, q, **kw):
    """The flags before any rescue, through the entry point itself: every query certified, none overflowed."""
    kp = idx._kprime(K, None)
    _, _, _, flg = T._native.dense_topk_f16(idx.docs, idx.docs16, idx.doc_rel_err, idx.dnorm, idx.inv_norm,
                                            dev(q), K, kp, **kw)
    return bool(np.all((flg.cpu().numpy() & 3) == 1))


@pytest.mark.parametrize("nq", BATCHES, ids=lambda v: f"q{v}")
@pytest.mark.parametrize("d", DIMS, ids=lambda v: f"d{v}")
@pytest.mark.parametrize("n", ROWS, ids=lambda v: f"r{v}")
def test_unfiltered(T, n, d, nq):
    """COLL = false: scores (bits), ids and counts are the oracle's, nothing is rescued, every query certified."""
    x, q = corpus(n, d)
    idx = index(T, n, d)
    S, I, cnt, nres = idx.dense_search(dev(q[:nq]), K)
    assert nres == 0
    assert_topk_equal(S, I, cnt, *(a[:nq] for a in oracle(n, d)), f"r{n} d{d} nq{nq}")
    assert certified(T, idx, q[:nq]), "every query certified, none overflowed"


@functools.lru_cache(maxsize=None)
def filtered_oracle(d):
    """Query i is filtered by qc[i] in (-1, 2 % collection, 25 % collection, ...): the oracle of a filtered
    query is the oracle over the rows of its collection (ties by ascending id either way)."""
    x, q = corpus(MID, d)
    Se, Ie, cnte = (a.copy() for a in oracle(MID, d))
    coll = collections(MID)
    qc = np.array([-1, COLL_SMALL, COLL_BIG] * (NQ_MAX // 3), dtype=np.int32)
    for c in (COLL_SMALL, COLL_BIG):
        rows = np.nonzero(coll == c)[0]
        sel = np.nonzero(qc == c)[0]
        s, i, m = CO.dense_topk_exact(x[rows], q[sel], K)
        Se[sel], cnte[sel] = s, m
        Ie[sel] = np.where(i >= 0, rows[np.maximum(i, 0)], -1)
    return qc, (Se, Ie, cnte)


@pytest.mark.parametrize("nq", (33, 300), ids=lambda v: f"q{v}")
@pytest.mark.parametrize("d", DIMS, ids=lambda v: f"d{v}")
def test_collection_filter(T, d, nq):
    """COLL = true on the mid-size corpus: a per-query filter mixing -1 with the 2 % and the 25 % collection;
    and an all -1 filter array gives the unfiltered result byte for byte."""
    x, q = corpus(MID, d)
    idx = index(T, MID, d)
    qc, expected = filtered_oracle(d)
    S, I, cnt, nres = idx.dense_search(dev(q[:nq]), K, collections=dev(qc[:nq]))
    assert nres == 0
    assert_topk_equal(S, I, cnt, *(a[:nq] for a in expected), f"filtered d{d} nq{nq}")
    S1, I1, c1, n1 = idx.dense_search(dev(q[:nq]), K, collections=dev(np.full(nq, -1, dtype=np.int32)))
    S0, I0, c0, n0 = idx.dense_search(dev(q[:nq]), K)
    assert n1 == 0 and n0 == 0
    for a, b in ((S1, S0), (I1, I0), (c1, c0)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_sample_values(T):
    """The sample area after a search of the mid-size corpus at dim 768: a lane's SAMPLE_TOP kept values per
    (query, segment) are the SAMPLE_TOP largest finite scan scores of the sample rows that lane scored,
    -inf padded -- as sorted multisets, against the float64 sum of the float16 products (the kernel sums them
    in float32: within scan_slack).  Queries of the first query tile."""
    n, d, nq = MID, 768, NQ_MAX
    x, q = corpus(n, d)
    idx = index(T, n, d)
    kp = idx._kprime(K, None)
    qtile = T._native.dense_f16_query_tile(d, True, nq)
    where, total, qpad = carve(qtile, nq, d)
    ws = idx._scan_workspace(nq, kp)
    assert ws.numel() >= total
    ws.fill_(0xFF)                                   # NaN: a value the sample pass never writes
    _, _, _, nres = idx.dense_search(dev(q), K)
    assert nres == 0
    off, nbytes = where["sample"]
    area = ws[off:off + nbytes].view(torch.float32).cpu().numpy()
    written = ~np.isnan(area)
    n_written = int(written.sum())
    assert n_written % (qpad * SAMPLE_TOP * SEGS) == 0 and written[:n_written].all(), "a prefix [qpad][nseg][4]"
    nseg = n_written // (qpad * SAMPLE_TOP)
    nslices = nseg // SEGS
    kept = area[:n_written].reshape(qpad, nseg, SAMPLE_TOP)
    assert np.all((kept[nq:] == -np.inf) | (kept[nq:] == 0))
    assert np.all(kept[:, :, :-1] >= kept[:, :, 1:]), "sorted descending"

    stride, sg = plan(n, kp)
    rows16 = unpack_copy16(idx.docs16.cpu().numpy(), d, SHAPE).astype(np.float64)   # NaN: no embedding, padding
    seg_rows = {}
    for t in range(sg):
        for r in range(32):
            seg_rows.setdefault(SEGS * (t % nslices) + segment_of_row(r, SHAPE), []).append(32 * t * stride + r)
    assert sorted(seg_rows) == list(range(min(nseg, SEGS * sg)))
    for i in range(0, min(nq, qtile), 7):
        q16 = q[i].astype(np.float16).astype(np.float64)
        slack = scan_slack(q[i])
        for s in range(nseg):
            sc = rows16[seg_rows.get(s, [])] @ q16
            sc = np.sort(sc[np.isfinite(sc)])[::-1][:SAMPLE_TOP]
            exp = np.concatenate([sc, np.full(SAMPLE_TOP - len(sc), -np.inf)])
            got = kept[i, s]
            assert np.array_equal(np.isinf(got), np.isinf(exp)), (i, s, got, exp)
            fin = np.isfinite(exp)
            assert np.all(np.abs(got[fin] - exp[fin]) <= slack), (i, s, got, exp, slack)


def test_overflowed_segments(T):
    """40 001 identical rows at dim 768, 33 queries: every score is equal, tau is that score, every row passes
    -- far more than a segment holds.  Every query is flagged overflowed, rescued, and the oracle's; the
    cursors run on past the segments' capacity and no store leaves the candidate area.  (The one case in
    which queries ARE rescued: the overflow path is what it is about.)"""
    n, d, nq = 40001, 768, 33
    rng = np.random.default_rng(d + nq + 1)
    x = np.tile(rng.standard_normal(d).astype(np.float32), (n, 1))
    q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = T.GpuIndex().set_dense(x, shortlist="f16")
    Se, Ie, cnte = CO.dense_topk_exact(x[:K + 1], q, K)      # the oracle of n identical rows is that of K + 1
    assert np.all(Ie == np.arange(K)) and np.all(cnte == K)

    kp = idx._kprime(K, None)
    N = T._native
    qtile = N.dense_f16_query_tile(d, True, nq)
    where, total, qpad = carve(qtile, nq, d)
    ws = torch.full((max(total, N.dense_f16_workspace_bytes(n, d, nq, kp)),), 0xA5, dtype=torch.uint8, device="cuda")
    S, I, cnt, flg = N.dense_topk_f16(idx.docs, idx.docs16, idx.doc_rel_err, idx.dnorm, idx.inv_norm, dev(q), K,
                                      kp, 0, ws)
    torch.cuda.synchronize()
    flg = flg.cpu().numpy()
    assert np.all(flg & 2) and not np.any(flg & 1), "every query overflowed, none certified"
    off, nbytes = where["cnt"]
    counts = ws[off:off + nbytes].view(torch.int32).cpu().numpy()
    written = counts != np.int32(-1515870811)          # 0xA5A5A5A5
    nseg = int(written.sum()) // qpad
    assert nseg > 0 and written[:qpad * nseg].all() and int(written.sum()) == qpad * nseg
    counts = counts[:qpad * nseg].reshape(qpad, nseg)
    assert np.all(counts[:nq] > CAND_CAP // nseg) and int(counts[0].sum()) == n
    assert np.all(counts[nq:] == 0)
    off, nbytes = where["cand"]
    seg_cap = CAND_CAP // nseg
    c0 = ws[off:off + CAND_BYTES * CAND_CAP].view(torch.int32).cpu().numpy().reshape(nseg, seg_cap, 2)
    assert np.all(c0[:, :, 0] == c0[0, 0, 0]) and np.all((c0[:, :, 1] >= 0) & (c0[:, :, 1] < n))
    assert np.all(c0[:, :-2, 1] < c0[:, 1:-1, 1]), "a lane emits its rows in ascending order"
    assert off + CAND_BYTES * qpad * CAND_CAP == where["tlist"][0]
    t_off, s_off = where["tlist"][0], where["sample"][0]
    assert bool((ws[t_off:s_off] == 0xA5).all()), "words behind the candidate area were overwritten"
    if qpad > nq:   # the padding queries' candidate segments are untouched (tau = +inf: nothing passes)
        assert bool((ws[off + CAND_BYTES * nq * CAND_CAP:off + nbytes] == 0xA5).all())

    S, I, cnt, nres = idx.dense_search(dev(q), K)
    assert nres == nq
    assert_topk_equal(S, I, cnt, Se, Ie, cnte, f"overflow d{d} nq{nq}")


MFMA32_SELECT = "(unfiltered and (q1 or q257)) or collection_filter or sample_values or overflowed"
MFMA32_CASES = len(ROWS) * len(DIMS) * 2 + len(DIMS) * 2 + 1 + 1


def test_mfma_shape_32():
    """The 32x32x16 shape (QAcc<32>: one query per lane, sixteen registers, two segments per row slice) through
    every corpus and dim with 1 and 257 queries, the filtered cases, the sample values and the overflow case.
    The knob is read once per process: a fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          MFMA32_SELECT],
                         env=dict(os.environ, THR_DENSE_MFMA="32"), cwd=root, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and f"{MFMA32_CASES} passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-2000:] + out.stderr[-1000:]
