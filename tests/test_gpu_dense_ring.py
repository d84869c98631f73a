"""The k-loop of dense_scan_f16qs (qs_steps_il: a ring of A fragments whose depth belongs to the instantiation,
the slot read a step ago refilled between the two MFMAs of a step, the next fragment waited for there) against
the float64 oracle, bit for bit, at the smallest shapes at which the ring's bookkeeping can go wrong.

A block's own tile count decides how often the ring is filled and drained and how the tile buffers wrap
(3 buffers at dim 768, 4 at dim 512).  One query tile (<= 256 queries) runs 8 * min(32, max(1, tiles / 8))
blocks, block b owning tiles b, b + blocks, ...; two query tiles (257 queries) half as many row slices.

    rows      tiles   own tiles per block, <= 256 queries      257 queries (a second query tile of one live wave)
    33        2       0 or 1  (8 blocks)                        0 or 1
    97        4       0 or 1                                    0 or 1
    2 049     65      1 or 2  (64 blocks)                       2 or 3  (32 slices)
    12 001    376     1 or 2  (256 blocks)                      2 or 3  (128 slices)
    18 433    577     2 or 3                                    4 or 5  (nbuf and nbuf + 1 at either dim)

1 query leaves seven padding waves, in both groups; 33 a live wave in group A only next to one full one.
Dim 768 is 48 k-steps (ring of 5), dim 512 is 32 (ring of 6: neither divides the steps, the tail of the waits
counts down).  A batch with a collection filter runs other instantiations than one without.  12 001 and 18 433
rows are more than CAND_CAP / 2: the sample pass (MODE_ALL) runs and sets tau.  The 32x32x16 shape
(THR_DENSE_MFMA=32, one MFMA per step) runs in a child process: the knob is read once per process.

Required of every case: ids and scores (bits) the oracle's, zero rescues, every query certified.
One corpus, one index and one oracle run per (rows, dim), shared and left unchanged."""
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
from dense_emit_cases import CAND_CAP  # noqa: E402

K, NQ_MAX = 10, 257
ROWS = (33, 97, 2049, 12001, 18433)
FILTER_ROWS = (2049, 18433)
DIMS = (512, 768)
BATCHES = (1, 33, 257)
COLL_SMALL, COLL_BIG = 7, 60
assert ROWS[-2] > CAND_CAP // 2, "the two largest corpora are sampled"


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def collections(n):
    """50 collections of 2 % of the rows each; in the second half every other row is of collection 60."""
    coll = (np.arange(n) * 7919 % 50).astype(np.int32)
    coll[n // 2:] = np.where(np.arange(n - n // 2) % 2 == 0, COLL_BIG, coll[n // 2:])
    return coll


@functools.lru_cache(maxsize=None)
def corpus(n, d):
    """Unit rows, row 5 without an embedding; every other query a neighbour of a random row >= 6."""
    x, rng = rand_docs(n, d, 7300 + d + n)
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


@functools.lru_cache(maxsize=None)
def filtered_oracle(n, d):
    """Query i is filtered by qc[i] in (-1, the 2 % collection, the 25 % collection, ...): the oracle of a
    filtered query is the oracle over the rows of its collection."""
    x, q = corpus(n, d)
    Se, Ie, cnte = (a.copy() for a in oracle(n, d))
    coll = collections(n)
    qc = np.array(([-1, COLL_SMALL, COLL_BIG] * (NQ_MAX // 3 + 1))[:NQ_MAX], dtype=np.int32)
    for c in (COLL_SMALL, COLL_BIG):
        rows = np.nonzero(coll == c)[0]
        sel = np.nonzero(qc == c)[0]
        s, i, m = CO.dense_topk_exact(x[rows], q[sel], K)
        Se[sel], cnte[sel] = s, m
        Ie[sel] = np.where(i >= 0, rows[np.maximum(i, 0)], -1)
    return qc, (Se, Ie, cnte)


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
    """COLL = false: scores (bits), ids and counts are the oracle's, nothing rescued, every query certified."""
    x, q = corpus(n, d)
    idx = index(T, n, d)
    S, I, cnt, nres = idx.dense_search(dev(q[:nq]), K)
    assert nres == 0
    assert_topk_equal(S, I, cnt, *(a[:nq] for a in oracle(n, d)), f"r{n} d{d} nq{nq}")
    assert certified(T, idx, q[:nq]), "every query certified, none overflowed"


@pytest.mark.parametrize("nq", (33, 257), ids=lambda v: f"q{v}")
@pytest.mark.parametrize("d", DIMS, ids=lambda v: f"d{v}")
@pytest.mark.parametrize("n", FILTER_ROWS, ids=lambda v: f"r{v}")
def test_collection_filter(T, n, d, nq):
    """COLL = true: a per-query filter mixing -1 with the 2 % and the 25 % collection."""
    x, q = corpus(n, d)
    idx = index(T, n, d)
    qc, expected = filtered_oracle(n, d)
    S, I, cnt, nres = idx.dense_search(dev(q[:nq]), K, collections=dev(qc[:nq]))
    assert nres == 0
    assert_topk_equal(S, I, cnt, *(a[:nq] for a in expected), f"filtered r{n} d{d} nq{nq}")
    assert certified(T, idx, q[:nq], doc_coll=idx.doc_coll, query_coll=dev(qc[:nq])), "every query certified, none overflowed"


MFMA32_SELECT = "(unfiltered and (q1 or q257)) or (collection_filter and q33)"
MFMA32_CASES = len(ROWS) * len(DIMS) * 2 + len(FILTER_ROWS) * len(DIMS)


def test_mfma_shape_32():
    """The 32x32x16 shape (one MFMA per k-step: refill and wait follow it) through every corpus and dim with 1
    and 257 queries and the filtered cases of 33.  The knob is read once per process: a fresh child."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          MFMA32_SELECT],
                         env=dict(os.environ, THR_DENSE_MFMA="32"), cwd=root, capture_output=True, text=True,
                         timeout=900)
    assert out.returncode == 0 and f"{MFMA32_CASES} passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-2000:] + out.stderr[-1000:]
