"""The emit of the register-resident filter scans and their sample pass (dense_scan_f16qs /
dense_scan_f16q: QEmit, QTop) against the CPU oracle, at the smallest shapes at which they can go wrong:

* 12 001 rows: the sample pass runs (more than CAND_CAP / 2 rows) and the last tile is padded with NaN rows;
* dims 512 and 768 (dense_scan_f16qs), dim 1024 (dense_scan_f16q with 48 queries per wave);
* 33 queries (a full wave plus one query) and 300 (two query tiles, padding waves).

An unfiltered batch runs the collection-free instantiation (COLL = false), a batch with a filter array the
other one.  A rescued query would pass whatever the scan emitted, so the cases assert n_rescued == 0
-- except the overflow case, where every query must be rescued.

One corpus and one index per dim, one oracle run per (dim, batch), shared and left unchanged; the queries
of the smaller batch are a prefix of the 300.
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

N_ROWS, NQ_MAX, K = 12001, 300, 10
DIMS = (512, 768, 1024)
BATCHES = (33, 300)
SHAPE = 32 if os.environ.get("THR_DENSE_MFMA") == "32" else 16     # the knob, as dense_knobs() reads it
SEGS = 2 if SHAPE == 32 else 4                                     # segments per row slice (QAcc::SEGS)


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def queries_near(x, rng, nq, lo):
    """Every other query a neighbour of a random row >= lo, the rest random."""
    q = rng.standard_normal((nq, x.shape[1])).astype(np.float32)
    q[::2] = x[rng.integers(lo, len(x), len(q[::2]))] + 0.5 * q[::2]
    return q


COLL_SMALL, COLL_BIG = 7, 60


def collections(n):
    """50 collections of 2 % of the rows each; in the second half every other row belongs to collection
    60 instead (25 % of the corpus)."""
    coll = (np.arange(n) * 7919 % 50).astype(np.int32)
    coll[n // 2:] = np.where(np.arange(n - n // 2) % 2 == 0, COLL_BIG, coll[n // 2:])
    return coll


@functools.lru_cache(maxsize=None)
def corpus(d):
    x, rng = rand_docs(N_ROWS, d, 4100 + d)
    x[5] = 0                                   # a row without an embedding
    q = queries_near(x, rng, NQ_MAX, 6)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


@functools.lru_cache(maxsize=None)
def oracle(d, nq):
    x, q = corpus(d)
    return CO.dense_topk_exact(x, q[:nq], K)


_index = {}


def index(T, d):
    if d not in _index:
        _index[d] = T.GpuIndex().set_dense(corpus(d)[0], shortlist="f16").set_collections(collections(N_ROWS))
    return _index[d]


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("d", DIMS)
def test_unfiltered_batch(T, d, nq):
    """COLL = false: scores (bits), ids, counts and flags are the oracle's, nothing is rescued."""
    x, q = corpus(d)
    idx = index(T, d)
    S, I, cnt, nres = idx.dense_search(dev(q[:nq]), K)
    assert nres == 0
    assert_topk_equal(S, I, cnt, *oracle(d, nq), f"d{d} nq{nq}")
    # the flags before any rescue, through the entry point itself
    kp = idx._kprime(K, None)
    _, _, _, flg = T._native.dense_topk_f16(idx.docs, idx.docs16, idx.doc_rel_err, idx.dnorm, idx.inv_norm,
                                            dev(q[:nq]), K, kp)
    assert np.all((flg.cpu().numpy() & 3) == 1), "every query certified, none overflowed"


@functools.lru_cache(maxsize=None)
def filtered_oracle(d, nq):
    """Query i is filtered by qc[i] in (-1, 2 % collection, 25 % collection, ...): the oracle of a filtered
    query is the oracle over the rows of its collection (ties by ascending id either way)."""
    x, q = corpus(d)
    Se, Ie, cnte = (a.copy() for a in oracle(d, nq))
    coll = collections(N_ROWS)
    qc = np.array([-1, COLL_SMALL, COLL_BIG] * (NQ_MAX // 3), dtype=np.int32)[:nq]
    for c in (COLL_SMALL, COLL_BIG):
        rows = np.nonzero(coll == c)[0]
        sel = np.nonzero(qc == c)[0]
        s, i, n = CO.dense_topk_exact(x[rows], q[sel], K)
        Se[sel], cnte[sel] = s, n
        Ie[sel] = np.where(i >= 0, rows[np.maximum(i, 0)], -1)
    return qc, (Se, Ie, cnte)


@pytest.mark.parametrize("nq", BATCHES)
@pytest.mark.parametrize("d", DIMS)
def test_collection_filter(T, d, nq):
    """COLL = true: a per-query filter mixing -1 with a 2 % and a 25 % collection; and an all -1 filter
    array gives the unfiltered result byte for byte -- one instantiation against the other."""
    x, q = corpus(d)
    idx = index(T, d)
    qc, expected = filtered_oracle(d, nq)
    S, I, cnt, nres = idx.dense_search(dev(q[:nq]), K, collections=dev(qc))
    assert nres == 0
    assert_topk_equal(S, I, cnt, *expected, f"filtered d{d} nq{nq}")
    S1, I1, c1, n1 = idx.dense_search(dev(q[:nq]), K, collections=dev(np.full(nq, -1, dtype=np.int32)))
    S0, I0, c0, n0 = idx.dense_search(dev(q[:nq]), K)
    assert n1 == 0 and n0 == 0
    for a, b in ((S1, S0), (I1, I0), (c1, c0)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@pytest.mark.parametrize("d", DIMS)
def test_rows_without_an_embedding(T, d):
    """One row in four zero (NaN in the copy): one of the four registers of every accumulator tile of a
    lane -- register 0, 2, 3, 1 of the tile in turn from one group of four rows to the next, so that a NaN
    sits in every register position beside registers that pass.  No such row appears in a list, and the
    lists are the oracle's."""
    x, rng = rand_docs(N_ROWS, d, 4200 + d)
    r = np.arange(N_ROWS)
    dead = (r % 4) == np.array([0, 2, 3, 1])[(r // 4) % 4]
    x[dead] = 0
    live = np.nonzero(~dead)[0]
    q = rng.standard_normal((33, d)).astype(np.float32)
    q[::2] = x[live[rng.integers(0, len(live), len(q[::2]))]] + 0.5 * q[::2]     # neighbours of live rows
    idx = T.GpuIndex().set_dense(x, shortlist="f16")
    S, I, cnt, nres = idx.dense_search(dev(q), K)
    assert nres == 0
    Se, Ie, cnte = CO.dense_topk_exact(x, q, K)
    assert_topk_equal(S, I, cnt, Se, Ie, cnte, f"one row in four zero, d{d}")
    ids = I.cpu().numpy()
    assert np.all(cnt.cpu().numpy() == K) and not dead[ids].any()


@pytest.mark.parametrize("d", DIMS)
def test_sample_values(T, d):
    """The sample area after a search: a lane's SAMPLE_TOP kept values per (query, segment) are the
    SAMPLE_TOP largest finite scan scores of the sample rows that lane scored, -inf padded -- as sorted
    multisets, against the float64 sum of the float16 products (the kernel sums them in float32: within
    scan_slack).  Queries of the first query tile."""
    x, q = corpus(d)
    idx = index(T, d)
    nq = NQ_MAX
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
    # padding queries: a zero query image in a live wave (every finite score is 0), nothing in an idle one
    assert np.all((kept[nq:] == -np.inf) | (kept[nq:] == 0))
    assert np.all(kept[:, :, :-1] >= kept[:, :, 1:]), "sorted descending"

    stride, sg = plan(N_ROWS, kp)
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


@pytest.mark.parametrize("d,nq", [(768, 33), (768, 300), (1024, 300)])
def test_overflowed_segments(T, d, nq):
    """40 001 identical rows: every score is equal, tau is that score, every row passes -- far more than a
    segment holds.  Every query is flagged overflowed, rescued, and the oracle's (ids ascending); and no
    store leaves the candidate area while the cursors run on: the carve behind it keeps its sentinel."""
    n = 40001
    rng = np.random.default_rng(d + nq)
    row = rng.standard_normal(d).astype(np.float32)
    x = np.tile(row, (n, 1))
    q = rng.standard_normal((nq, d)).astype(np.float32)
    idx = T.GpuIndex().set_dense(x, shortlist="f16")
    # the oracle of n identical rows is the oracle of K + 1 of them
    Se, Ie, cnte = CO.dense_topk_exact(x[:K + 1], q, K)
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
    # segment counts of the live queries: all above the segment's capacity (the cursor runs on)
    off, nbytes = where["cnt"]
    counts = ws[off:off + nbytes].view(torch.int32).cpu().numpy()
    written = counts != np.int32(-1515870811)          # 0xA5A5A5A5
    nseg = int(written.sum()) // qpad
    assert nseg > 0 and written[:qpad * nseg].all() and int(written.sum()) == qpad * nseg
    counts = counts[:qpad * nseg].reshape(qpad, nseg)
    assert np.all(counts[:nq] > CAND_CAP // nseg) and int(counts[0].sum()) == n
    assert np.all(counts[nq:] == 0)
    # what a full segment holds: seg_cap true candidates of its query -- the common score, rows of the corpus
    off, nbytes = where["cand"]
    seg_cap = CAND_CAP // nseg
    c0 = ws[off:off + CAND_BYTES * CAND_CAP].view(torch.int32).cpu().numpy().reshape(nseg, seg_cap, 2)
    assert np.all(c0[:, :, 0] == c0[0, 0, 0]) and np.all((c0[:, :, 1] >= 0) & (c0[:, :, 1] < n))
    assert np.all(c0[:, :-2, 1] < c0[:, 1:-1, 1]), "a lane emits its rows in ascending order"
    # behind the candidate area: the tile-list carve (unused by this scan) is untouched, and so is the
    # sample area past what the sample pass wrote
    assert off + CAND_BYTES * qpad * CAND_CAP == where["tlist"][0]
    t_off = where["tlist"][0]
    s_off, s_bytes = where["sample"]
    assert bool((ws[t_off:s_off] == 0xA5).all()), "words behind the candidate area were overwritten"
    sample = ws[s_off:s_off + s_bytes].cpu().numpy()
    untouched = (sample.reshape(-1, 4) == 0xA5).all(axis=1)
    first = int(np.argmax(untouched))
    assert untouched[first:].all() and first % (qpad * SAMPLE_TOP) == 0 and first <= qpad * 1024 * SAMPLE_TOP
    # the padding queries' candidate segments are untouched as well (tau = +inf: nothing passes)
    if qpad > nq:
        assert bool((ws[off + CAND_BYTES * nq * CAND_CAP:off + nbytes] == 0xA5).all())

    S, I, cnt, nres = idx.dense_search(dev(q), K)
    assert nres == nq
    assert_topk_equal(S, I, cnt, Se, Ie, cnte, f"overflow d{d} nq{nq}")


def test_mfma_shape_32():
    """The 32x32x16 shape (QAcc<32>: one query per lane, sixteen registers, two segments per row slice) through the 33-query unfiltered and filtered cases, the no-embedding cases, the sample
    values (300 queries) and the overflow cases (33 and 300 queries).  The knob is read once per process:
    a fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "((unfiltered or collection_filter) and 33) or without or overflowed or sample_values"],
                         env=dict(os.environ, THR_DENSE_MFMA="32"), cwd=root, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and "15 passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-2000:] + out.stderr[-1000:]


def test_pipelined_emit_at_32_queries_per_wave():
    """THR_DENSE_QW=32: dim 1024 with 32 queries per wave, where the emit of a row tile runs between the
    MFMAs of the next one (qsx_steps_pe) -- with the 16x16x32 shape here, with 32x32x16 in the test
    above.  Read once per process: a fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "(unfiltered or collection_filter or overflowed) and 1024"],
                         env=dict(os.environ, THR_DENSE_QW="32"), cwd=root, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and "5 passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-2000:] + out.stderr[-1000:]
