"""The four tile-list scans -- dense_scan_mfma2 (float32 rows, dim <= 768), dense_scan_mfma (dim 1024),
dense_scan_f16 ("f16-inline") and dense_scan_anydim ("f16-anydim") -- through the pieces they share
(csrc/dense_scan_tilelist.hpp: the flush of a wave's candidate buffer, the ballot that fills it, the
per-lane tau / collection filter, the loader tables), each at its smallest row length and at the smallest
shapes that reach every path of those pieces:

* 8229 rows: above CAND_CAP / 2 = 8192, so the sample pass (MODE_ALL) runs and the filter scan has a tau;
  1000 rows: no sample, every row passes, so a wave's 256-slot buffer is flushed inside the row loop
  (32 rows x 32 queries per tile), not only at the end;
* both have a ragged last row tile (8229 = 257 * 32 + 5, 1000 = 31 * 32 + 8);
* 33 queries: one full query tile of 32 and a second one with a single query;
* without and with a collection filter (three collections, one query without one, one query whose
  collection does not exist).

Asserted as the other dense tests do: ids and float64 scores are the oracle's (an uncertified query is
redone exhaustively by dense_search, so every query is certified or rescued)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import thr_oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_cases import dev, rand_docs  # noqa: E402

K, NQ, BASE = 10, 33, 500
FLAVOURS = [("f32", 256), ("f32", 1024), ("f16-inline", 512), ("f16-anydim", 32), ("f16-anydim", 96)]


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


@functools.lru_cache(maxsize=None)
def case(n, d):
    """Unit rows, row 77 all zero; even queries are noisy copies of rows, the last one of the last row.
    Collections 0 / 1 / 2 by row; query collections cycle through them, with one query unfiltered and
    one asking for a collection no row has.  -> x, q, coll, qc and the float64 scores [NQ, n].  Read-only."""
    x, rng = rand_docs(n, d, 1000 + d)
    x[77] = 0
    q = rng.standard_normal((NQ, d)).astype(np.float32)
    q[::2] = x[rng.integers(0, n, len(q[::2]))] + 0.5 * q[::2]
    q[NQ - 1] = x[n - 1] + 0.25 * q[NQ - 1]
    coll = (np.arange(n) * 7919 % 3).astype(np.int32)
    qc = (np.arange(NQ) % 3).astype(np.int32)
    qc[4], qc[9] = -1, 12345
    dn = O.doc_norms_f64(x)
    scores = np.stack([O.cosine_scores_f64(x, q[i], dn) for i in range(NQ)])
    return x, q, coll, qc, scores


@pytest.mark.parametrize("filtered", [False, True], ids=["all", "collections"])
@pytest.mark.parametrize("n", [1000, 8229], ids=["unsampled", "sampled"])
@pytest.mark.parametrize("shortlist,d", FLAVOURS)
def test_tilelist_scan_is_the_oracle(T, shortlist, d, n, filtered):
    x, q, coll, qc, scores = case(n, d)
    idx = T.GpuIndex(doc_base=BASE).set_dense(x, shortlist=shortlist)
    assert idx.shortlist == shortlist and idx.docs16 is None
    if filtered:
        idx.set_collections(coll)
        S, I, cnt, nres = idx.dense_search(dev(q), K, collections=dev(qc))
    else:
        S, I, cnt, nres = idx.dense_search(dev(q), K)
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    print(f"{shortlist} d={d} n={n} filtered={filtered}: rescued {int(nres)} of {NQ}")
    for i in range(NQ):
        s = scores[i].copy()
        if filtered and qc[i] != -1:
            s[coll != qc[i]] = -np.inf
        ts, ti = O.topk_desc(s, K)
        what = (shortlist, d, n, filtered, i)
        assert cnt[i] == len(ti), what
        assert np.array_equal(I[i, :len(ti)], ti + BASE), what
        assert np.array_equal(S[i, :len(ti)], ts), what
        assert np.all(I[i, len(ti):] == -1), what
    if filtered:
        assert cnt[9] == 0 and cnt[4] == K
