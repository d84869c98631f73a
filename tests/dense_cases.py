"""Inputs and checks the dense-channel tests of the runtime-dim f16 scan share (tests/test_gpu_dense_anydim.py):
the planted corpus of test_dense_f16_shortlist_is_still_exact at any row length, its float64 oracle
(computed once per shape), and the single-process recipe of the shards' floor exchange."""
import functools

import numpy as np
import torch

from oracle import c_oracle as CO

DOC_BASE = 123
ZERO_QUERY, TIE_QUERY = 5, 0


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def rand_docs(n, d, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x, rng


def assert_topk_equal(S, I, cnt, Se, Ie, cnte, what=""):
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    for q in range(len(cnte)):
        n = int(cnte[q])
        assert int(cnt[q]) == n, f"{what} q{q}: count {cnt[q]} != {n}"
        assert np.array_equal(I[q, :n], Ie[q][:n]), f"{what} q{q}: ids differ"
        assert np.array_equal(S[q, :n], Se[q][:n]), f"{what} q{q}: scores differ (bits)"
        assert np.all(I[q, n:] == -1)


@functools.lru_cache(maxsize=None)
def planted(n, d, nq=70):
    """Standard-normal unit rows; row 13 all zero, rows 200..229 copies of row 199.  Query 0 sits next to
    row 199 (a 31-way tie inside its top-100), the other even queries are planted neighbours of random
    rows, query 5 is all zero.  Read-only: shared by every test of the shape."""
    x, rng = rand_docs(n, d, 77)
    x[13] = 0
    x[200:230] = x[199]
    q = rng.standard_normal((nq, d)).astype(np.float32)
    q[::2] = x[rng.integers(0, n, len(q[::2]))] + 0.5 * q[::2]
    q[TIE_QUERY] = x[199] + 0.05 * rng.standard_normal(d).astype(np.float32)
    q[ZERO_QUERY] = 0
    return x, q


@functools.lru_cache(maxsize=None)
def planted_oracle(n, d, k, nq=70):
    x, q = planted(n, d, nq)
    return CO.dense_topk_exact(x, q, k, doc_id_base=DOC_BASE)


def floor_search(T, x, q, k, n_shards, shortlist, seen=None):
    """The dense channel of a document-sharded index with every shard in this process: shortlist on every
    shard -> the lower bounds stacked (what the all-gather delivers) -> thr_dense_floor -> finish on every
    shard -> thr_merge_topk.  -> merged (S, I, cnt), the flags the finishes wrote [G, nq], rescued per shard.
    seen: a dict that receives what was exchanged, "lbs" [G, nq, m] and "gfloor" [nq]."""
    n = x.shape[0]
    shards = [T.GpuIndex(doc_base=s * n // n_shards).set_dense(x[s * n // n_shards:(s + 1) * n // n_shards],
                                                              shortlist=shortlist) for s in range(n_shards)]
    qd = dev(q)
    lbs = torch.stack([ix.dense_shortlist(qd, k, n_shards) for ix in shards])
    assert lbs.shape == (n_shards, q.shape[0], T.index.floor_width(k, n_shards))
    gfloor = T._native.dense_floor(lbs, k)
    if seen is not None:
        seen.update(lbs=lbs, gfloor=gfloor)
    # the floor as thr_dense_floor's output on the even shards, as the gathered bounds on the odd ones
    outs = [ix.dense_finish(qd, k, lb_all=lbs) if si % 2 else ix.dense_finish(qd, k, gfloor)
            for si, ix in enumerate(shards)]
    Sm, Im, cm = T._native.merge_topk(torch.stack([o[0] for o in outs]), torch.stack([o[1] for o in outs]), k)
    flags = torch.stack([o[3] for o in outs]).cpu().numpy()
    return (Sm, Im, cm), flags, [int(o[4]) for o in outs]
