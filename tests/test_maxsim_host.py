"""MaxSim shapes without a GPU: which token shapes thr_maxsim_pack / thr_maxsim / thr_maxsim_ids
take is host arithmetic, answered before a pointer is looked at, so the refusal paths of the C ABI
can be asked here (as tests/test_native_abi.py does) -- and the list in C (csrc/maxsim.hip
THR_MS_KSTEPS) must be the Python constant _native.MAXSIM_TOK_DIMS, dim by dim."""
import os
import sys

import numpy as np
import pytest

import triple_hybrid_rag_amd as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxsim_cases as MC  # noqa: E402

N = T._native
UNSUPPORTED, INVALID = -2, -1


def c_pack(d_tokens, tok_dim):
    return N.load().thr_maxsim_pack(None, 1, d_tokens, tok_dim, None, None)


def c_maxsim(q_tokens, d_tokens, tok_dim, packed=0):
    return N.load().thr_maxsim(None, 1, q_tokens, None, 1, d_tokens, tok_dim, None, 1, None, packed, None)


def c_maxsim_ids(q_tokens, d_tokens, tok_dim, packed=0):
    return N.load().thr_maxsim_ids(None, 1, q_tokens, None, 1, d_tokens, tok_dim, None, 0, 1, None, packed, None)


def test_c_list_and_python_constant_agree_dim_by_dim():
    """Null pointers: a supported shape gets as far as the pointer check (THR_ERR_INVALID), an
    unsupported one is refused first (THR_ERR_UNSUPPORTED) -- by the pack and by both scorers,
    packed or not, for every multiple of 16 from 16 to 272 and for what lies between."""
    assert N.MAXSIM_TOK_DIMS == (16, 32, 64, 96, 128, 192, 256)
    assert N.load().thr_error_string(UNSUPPORTED) == b"unsupported shape"
    seen = []
    for td in range(16, 272 + 1, 16):
        want = INVALID if td in N.MAXSIM_TOK_DIMS else UNSUPPORTED
        got = [c_pack(32, td), c_maxsim(32, 32, td), c_maxsim(32, 32, td, 1), c_maxsim_ids(32, 32, td),
               c_maxsim_ids(32, 32, td, 1)]
        assert got == [want] * 5, (td, got)
        if want == INVALID:
            seen.append(td)
    assert tuple(seen) == N.MAXSIM_TOK_DIMS
    for td in (0, -16, 8, 24, 100, 257, 1 << 20, -(1 << 31)):
        assert [c_pack(32, td), c_maxsim(32, 32, td), c_maxsim_ids(32, 32, td)] == [UNSUPPORTED] * 3, td


def test_token_counts_are_multiples_of_32():
    for n_tok in (0, -32, 1, 31, 33, 48):
        assert c_pack(n_tok, 128) == UNSUPPORTED
        assert c_maxsim(n_tok, 32, 128) == UNSUPPORTED and c_maxsim(32, n_tok, 128) == UNSUPPORTED
        assert c_maxsim_ids(n_tok, 32, 128) == UNSUPPORTED and c_maxsim_ids(32, n_tok, 128) == UNSUPPORTED
    for n_tok in (32, 64, 96, 160, 512):
        assert c_pack(n_tok, 128) == INVALID and c_maxsim(n_tok, n_tok, 128) == INVALID
    # supported shapes, bad counts: still the pointer / count check's answer
    lib = N.load()
    assert lib.thr_maxsim(None, 0, 32, None, 1, 32, 128, None, 1, None, 0, None) == INVALID
    assert lib.thr_maxsim_ids(None, 1, 32, None, 1, 32, 128, None, 0, 0, None, 0, None) == INVALID


def test_python_check_names_the_supported_dims():
    for td in range(16, 272 + 1, 16):
        if td in N.MAXSIM_TOK_DIMS:
            N.maxsim_check_tokens("x", td, 32, 512)
        else:
            with pytest.raises(N.NativeError, match=r"tok_dim %d .*\[16, 32, 64, 96, 128, 192, 256\]" % td):
                N.maxsim_check_tokens("x", td, 32)
    for bad in (0, 31, 33, -32):
        with pytest.raises(N.NativeError, match="multiples of 32"):
            N.maxsim_check_tokens("x", 128, 32, bad)


def test_cases_helper_is_sound_on_the_cpu():
    """The helper module's own claims, checked where they can be without a GPU: the exact
    family is exact in float32 under any accumulation order, the bound covers a float32
    evaluation, the pack restatement is a permutation with the documented index map, and
    assert_order_within admits and refuses what its docstring says."""
    rng = np.random.default_rng(5)
    for td in (16, 96, 256):
        q = MC.exact_tokens(rng, (2, 32, td))
        d = MC.exact_tokens(rng, (3, 32, td))
        cand = np.array([[0, 1, 2], [2, 2, -1]])
        ref = MC.reference(q, d, cand)
        got = np.full(cand.shape, -np.inf, dtype=np.float32)
        for qi in range(2):
            for c in range(3):
                if cand[qi, c] < 0:
                    continue
                total = np.float32(0)
                for i in rng.permutation(32):
                    best = np.float32(-np.inf)
                    for j in range(32):
                        acc = np.float32(0)
                        prods = q[qi, i].astype(np.float32) * d[cand[qi, c], j].astype(np.float32)
                        for k in rng.permutation(td):
                            acc = np.float32(acc + prods[k])
                        best = max(best, acc)
                    total = np.float32(total + best)
                got[qi, c] = total
        assert np.array_equal(got.astype(np.float64), ref), td
    # the bound covers a float32 matmul of real-valued tokens
    q = rng.standard_normal((2, 32, 64)).astype(np.float16)
    d = rng.standard_normal((4, 64, 64)).astype(np.float16)
    cand = np.array([[0, 1, 2, 3], [3, 4, -1, 0]])
    ref, bound = MC.reference(q, d, cand), MC.error_bound(q, d, cand)
    assert ref[1, 1] == -np.inf and ref[1, 2] == -np.inf and bound[1, 1] == 0.0
    for qi in range(2):
        for c in range(4):
            if np.isfinite(ref[qi, c]):
                s = (q[qi].astype(np.float32) @ d[cand[qi, c]].astype(np.float32).T).max(axis=1).sum(dtype=np.float32)
                assert 0 < bound[qi, c] < 1e-2 and abs(float(s) - ref[qi, c]) <= bound[qi, c]
    # the pack restatement against its index map, element by element
    d = np.arange(2 * 64 * 32, dtype=np.uint16).view(np.float16).reshape(2, 64, 32)
    p = MC.pack_reference(d).reshape(2, 2, 2, 64, 8)
    for doc, tile, ks, lane in ((0, 0, 0, 0), (1, 1, 1, 63), (0, 1, 0, 31), (1, 0, 1, 32), (0, 0, 1, 45)):
        r, h = lane & 31, lane >> 5
        assert np.array_equal(p[doc, tile, ks, lane].view(np.uint16),
                              d[doc, 32 * tile + r, 16 * ks + 8 * h:16 * ks + 8 * h + 8].view(np.uint16))
    # the order rule
    ids, ref = [10, 11, 12, 13], [4.0, 3.0, 3.0 - 1e-5, 1.0]
    MC.assert_order_within([10, 11, 12], ids, ref, 1e-4)
    MC.assert_order_within([10, 12, 11], ids, ref, 1e-4)          # inside 2 tol: either order
    MC.assert_order_within([10, 12], ids, ref, 1e-4)              # ... and either one may be the last
    for bad in ([11, 10, 12], [10, 11, 13], [10, 10, 11], [10, 11, 99], [10, 13]):
        with pytest.raises(AssertionError):
            MC.assert_order_within(bad, ids, ref, 1e-4)
    with pytest.raises(AssertionError):
        MC.assert_order_within([10, 12, 11], ids, ref, 1e-6)      # gaps above 2 tol: the exact order only
    with pytest.raises(AssertionError):
        MC.assert_order_within([], ids, ref, 1e-4)
