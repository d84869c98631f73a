"""Inputs, reference and bounds of the MaxSim tests (tests/test_gpu_maxsim.py, the rerank legs
of tests/test_gpu_parity.py).  Pure numpy: nothing here needs a GPU.

The reference of every case is oracle.thr_oracle.maxsim_scores (float64).  Two input families:

* EXACT: float16 tokens that are multiples of 1/8 in [-1, 1].  Every product is a multiple of
  1/64, so every partial sum of up to 256 products (|sum| <= 256 = 2^14 / 64) and of up to 128
  per-token maxima (|sum| <= 2^21 / 64) is an integer multiple of 1/64 below 2^24 / 64: exactly
  representable in float32.  Whatever the accumulation order, the device must return the bits
  of the float64 reference -- these cases are compared with np.array_equal, no tolerance.
* REAL: unit-norm synth tokens and non-normalised standard_normal tokens, held to the float32
  forward-error bound computed from the inputs (error_bound), not to a chosen number.
"""
import numpy as np

from oracle import thr_oracle as O

TOK_DIMS = (16, 32, 64, 96, 128, 192, 256)       # one kernel instantiation each (tok_dim / 16)
U = 2.0 ** -24                                   # unit roundoff of float32


def gamma(n: int) -> float:
    return n * U / (1.0 - n * U)


def exact_tokens(rng, shape, lo=-8, hi=8) -> np.ndarray:
    """float16 multiples of 1/8 in [lo/8, hi/8]."""
    return (rng.integers(lo, hi + 1, size=shape) / 8.0).astype(np.float16)


def real_tokens(family: str, rng, n: int, n_tokens: int, tok_dim: int, queries: bool) -> np.ndarray:
    """'unit': unit-norm tokens -- the project's synth tokens (synth draws document tokens in blocks
    of 4096 documents: above 128 x 128 per document the same recipe is applied to ``rng`` here);
    'normal': standard_normal, not normalised."""
    if family == "unit":
        from triple_hybrid_rag_amd import synth
        if queries:
            return synth.query_tokens(n, n_tokens, tok_dim)
        if n_tokens * tok_dim <= 128 * 128:
            return synth.doc_tokens(0, n, n_tokens, tok_dim)
        x = rng.standard_normal((n, n_tokens, tok_dim)).astype(np.float32)
        x /= np.linalg.norm(x, axis=2, keepdims=True)
        return x.astype(np.float16)
    assert family == "normal"
    return rng.standard_normal((n, n_tokens, tok_dim)).astype(np.float16)


def local_candidates(cand, n_docs: int, id_base=None) -> np.ndarray:
    """Candidates as the oracle takes them: local doc index, -1 for everything the device
    scores -inf (negative, outside [0, n_docs); with id_base: global ids of another shard)."""
    c = np.asarray(cand).astype(np.int64)
    if id_base is not None:
        c = np.where(c >= 0, c - id_base, -1)
    return np.where((c >= 0) & (c < n_docs), c, -1)


def reference(qtok, dtok, cand, id_base=None) -> np.ndarray:
    """float64 MaxSim of the oracle, -inf where the device owes -inf."""
    return O.maxsim_scores(qtok, dtok, local_candidates(cand, dtok.shape[0], id_base))


def error_bound(qtok, dtok, cand) -> np.ndarray:
    """Forward-error bound of a float32 evaluation of MaxSim, per score, in float64:
        gamma(tok_dim) * sum_i max_j sum_k |q_ik| |d_jk|  +  gamma(q_tokens) * sum_i |max_j s_ij|
    (the fp16 products are exact; a dot product of tok_dim terms accumulated in float32 in any
    order is within gamma(tok_dim) * sum |terms|, the max is exact and monotone, and the sum of
    q_tokens maxima adds gamma(q_tokens) of their magnitudes).  0 where the score is -inf."""
    cand = local_candidates(cand, dtok.shape[0])
    nq, qt, td = qtok.shape
    out = np.zeros(cand.shape, dtype=np.float64)
    for q in range(nq):
        a = qtok[q].astype(np.float64)
        for c in range(cand.shape[1]):
            d = int(cand[q, c])
            if d < 0:
                continue
            b = dtok[d].astype(np.float64)
            mag = (np.abs(a) @ np.abs(b).T).max(axis=1).sum()
            mx = np.abs((a @ b.T).max(axis=1)).sum()
            out[q, c] = gamma(td) * mag + gamma(qt) * mx
    return out


def pack_reference(dtok: np.ndarray) -> np.ndarray:
    """numpy restatement of thr_maxsim_pack: [doc][tile of 32 tokens][k-step][lane][8 halves],
    lane = 32 * h + r holding token 32 * tile + r, dims 16 * ks + 8 * h .. + 8."""
    n, dt, td = dtok.shape
    x = dtok.reshape(n, dt // 32, 32, td // 16, 2, 8)        # [doc][tile][r][ks][h][8]
    return np.ascontiguousarray(x.transpose(0, 1, 3, 4, 2, 5)).reshape(n, dt, td)


def assert_order_within(got_ids, cand_ids, ref_scores, tol: float, what: str = "") -> None:
    """The reranked ids of ONE query against the float64 scores of its candidates, where the
    device's scores are within ``tol`` of the reference:
      * got_ids has no duplicates and is drawn from cand_ids;
      * consecutive results: ref[a] >= ref[a + 1] - 2 tol;
      * every candidate not returned: ref <= ref[last] + 2 tol.
    Where the reference's gaps exceed 2 tol this admits the exact order only.  Nothing is skipped."""
    got = [int(g) for g in got_ids]
    cands = [int(c) for c in cand_ids]
    assert len(set(cands)) == len(cands), f"{what}: candidate ids repeat"
    ref = {c: float(s) for c, s in zip(cands, ref_scores)}
    assert len(set(got)) == len(got), f"{what}: an id is returned twice: {got}"
    assert all(g in ref for g in got), f"{what}: an id outside the candidates: {got}"
    assert len(got) > 0 or len(cands) == 0, f"{what}: nothing returned"
    for a, b in zip(got, got[1:]):
        assert ref[a] >= ref[b] - 2 * tol, f"{what}: {a} ({ref[a]!r}) is ranked before {b} ({ref[b]!r})"
    if got:
        last = ref[got[-1]]
        left = [c for c in cands if c not in set(got)]
        for c in left:
            assert ref[c] <= last + 2 * tol, f"{what}: {c} ({ref[c]!r}) is left out, {got[-1]} ({last!r}) is in"
