"""No GPU: the FP8 token store.  The new header against its binding table, the shape and argument
refusals of the three entry points (through the library and in a stand-alone sanitized program), the
numpy restatement of the quantiser against torch's float8_e4m3fn cast at every edge of the rounding, the
packed-layout restatement, the error bound, the built cases' properties, and the refusals of
set_tokens(store=) / append_rows / to_gpu(token_store=) that need no device."""
import os
import re
import shutil
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxsim_cases as MC  # noqa: E402
import maxsim_fp8_cases as F8  # noqa: E402
import triple_hybrid_rag_amd as T  # noqa: E402
from test_native_abi import ctype_class, declared_symbols, header_class  # noqa: E402
from triple_hybrid_rag_amd import _native as N  # noqa: E402
from triple_hybrid_rag_amd import index_build as IB  # noqa: E402
from triple_hybrid_rag_amd.index import GpuIndex  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thr_hip_rerank.h")
UNSUPPORTED, INVALID = -2, -1
NAMES = ["thr_maxsim_fp8", "thr_maxsim_fp8_ids", "thr_maxsim_quantize_fp8"]


# --------------------------------------------------------------------------- header, binding, constants
def _header_prototypes():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))
    protos = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(thr_[a-z0-9_]+)\s*\(([^;{}()]*)\)\s*;", text):
        res, name, params = m.group(1), m.group(2), m.group(3).strip()
        res = " ".join(w for w in res.split() if w != "extern")
        args = []
        for p in params.split(","):
            p = p.strip()
            args.append(header_class(re.sub(r"[A-Za-z_]\w*$", "", p) if re.search(r"[\s\*][A-Za-z_]\w*$", p) else p))
        protos[name] = (header_class(res), args)
    return protos


def test_the_new_header_and_the_third_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(N._SIGNATURES_RERANK) == NAMES
    for name, (res, args) in N._SIGNATURES_RERANK.items():
        want_res, want_args = protos[name]
        assert ctype_class(res) == want_res, name
        got = [ctype_class(a) for a in args]
        assert len(got) == len(want_args), f"{name}: {len(got)} argtypes, the header declares {len(want_args)} parameters"
        for i, (g, w) in enumerate(zip(got, want_args)):
            assert g == w, f"{name}: argument {i}"
    lib = N.load()
    for name in protos:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == N._SIGNATURES_RERANK[name][1]
    assert '#include "thr_hip.h"' in open(HEADER).read()
    assert "thr_hip_rerank.h" in [os.path.basename(h) for h in T._build._headers()]


def test_thr_hip_h_and_the_exported_symbols_are_unchanged_in_count():
    assert len(declared_symbols()) == len(N.EXPORTED_SYMBOLS) == 65 and N.ABI_VERSION == 9
    assert not set(N._SIGNATURES_RERANK) & (set(N.EXPORTED_SYMBOLS) | set(N._SIGNATURES_GRAPH) | set(N._SIGNATURES_TEXT))
    assert "fp8" not in open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    assert N.MAXSIM_TOK_DIMS == (16, 32, 64, 96, 128, 192, 256)      # the float16 list stays


# --------------------------------------------------------------------------- shapes, through null pointers
def c_quant(d_tokens, tok_dim):
    return N.load().thr_maxsim_quantize_fp8(None, 1, d_tokens, tok_dim, None, None, None)


def c_score(q_tokens, d_tokens, tok_dim):
    return N.load().thr_maxsim_fp8(None, 1, q_tokens, None, None, 1, d_tokens, tok_dim, None, 1, None, None)


def c_score_ids(q_tokens, d_tokens, tok_dim):
    return N.load().thr_maxsim_fp8_ids(None, 1, q_tokens, None, None, 1, d_tokens, tok_dim, None, 0, 1, None, None)


def test_c_list_and_python_constant_agree_dim_by_dim():
    assert N.MAXSIM_FP8_TOK_DIMS == F8.TOK_DIMS == (32, 64, 96, 128, 192, 256)
    seen = []
    for td in range(16, 272 + 1):        # every multiple of 16 and what lies between
        want = INVALID if td in N.MAXSIM_FP8_TOK_DIMS else UNSUPPORTED
        got = [c_quant(32, td), c_score(32, 32, td), c_score_ids(32, 32, td)]
        assert got == [want] * 3, (td, got)
        if want == INVALID:
            seen.append(td)
    assert tuple(seen) == N.MAXSIM_FP8_TOK_DIMS
    for td in (0, -32, 8, 16, 1 << 20, -(1 << 31)):
        assert [c_quant(32, td), c_score(32, 32, td), c_score_ids(32, 32, td)] == [UNSUPPORTED] * 3, td


def test_token_counts_are_multiples_of_32():
    for n_tok in (0, -32, 1, 31, 33, 48):
        assert c_quant(n_tok, 128) == UNSUPPORTED
        assert c_score(n_tok, 32, 128) == UNSUPPORTED and c_score(32, n_tok, 128) == UNSUPPORTED
        assert c_score_ids(n_tok, 32, 128) == UNSUPPORTED and c_score_ids(32, n_tok, 128) == UNSUPPORTED
    for n_tok in (32, 64, 96, 160, 512):
        assert c_quant(n_tok, 128) == INVALID and c_score(n_tok, n_tok, 128) == INVALID
    lib, p = N.load(), 4096
    # supported shapes, every pointer given, bad counts: the count check's answer
    assert lib.thr_maxsim_fp8(p, 0, 32, p, p, 1, 32, 128, p, 1, p, None) == INVALID
    assert lib.thr_maxsim_fp8(p, 1, 32, p, p, 0, 32, 128, p, 1, p, None) == INVALID
    assert lib.thr_maxsim_fp8_ids(p, 1, 32, p, p, 1, 32, 128, p, 0, 0, p, None) == INVALID
    assert lib.thr_maxsim_quantize_fp8(p, 0, 32, 128, 2 * p, p, None) == INVALID
    assert lib.thr_maxsim_quantize_fp8(p, 1, 32, 128, p, p, None) == INVALID          # in place
    for i in (0, 3, 4, 8, 10):
        a = [p, 1, 32, p, p, 1, 32, 128, p, 1, p, None]
        a[i] = None
        assert lib.thr_maxsim_fp8(*a) == INVALID, i


def test_python_checks_name_the_supported_dims():
    for td in range(16, 272 + 1, 16):
        if td in N.MAXSIM_FP8_TOK_DIMS:
            N.maxsim_fp8_check_tokens("x", td, 32, 512)
        else:
            with pytest.raises(N.NativeError, match=r"tok_dim %d .*\[32, 64, 96, 128, 192, 256\]" % td):
                N.maxsim_fp8_check_tokens("x", td, 32)
    for bad in (0, 31, 33, -32):
        with pytest.raises(N.NativeError, match="multiples of 32"):
            N.maxsim_fp8_check_tokens("x", 128, 32, bad)
    # the operand checks of the family: host tensors, wrong dtypes are refused before the library is asked
    q, c, s = torch.zeros((1, 32, 32), dtype=torch.float16), torch.zeros((2, 32, 32), dtype=torch.uint8), torch.ones((2, 32))
    for call in (lambda: N.maxsim_quantize_fp8(q), lambda: N.maxsim_fp8(q, c, s, torch.zeros((1, 2), dtype=torch.int32)),
                 lambda: N.maxsim_fp8_ids(q, c, s, torch.zeros((1, 2), dtype=torch.int64), 0)):
        with pytest.raises(N.NativeError, match="expected a CUDA"):
            call()


def test_host_checks_are_clean_under_address_and_ub_sanitizer(tmp_path):
    """The three entries' argument checks, compiled together with a stand-alone program (its own main) with
    the host side under ASan + UBSan, run on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "maxsim_fp8_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "maxsim_fp8.hip"),
                    os.path.join(ROOT, "tests", "native", "maxsim_fp8_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "maxsim_fp8 host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# --------------------------------------------------------------------------- the quantiser's restatement
def torch_codes(y: np.ndarray) -> np.ndarray:
    """torch's CPU cast of float32 values (it does not saturate: |y| <= 448 is the caller's business)."""
    assert np.all(np.abs(y) <= 448)
    return torch.from_numpy(np.ascontiguousarray(y, dtype=np.float32)).to(torch.float8_e4m3fn).view(torch.uint8).numpy()


def test_value_table_is_torchs():
    codes = torch.arange(256, dtype=torch.int32).to(torch.uint8)
    tv = codes.view(torch.float8_e4m3fn).to(torch.float64).numpy()
    assert np.array_equal(np.isnan(tv), np.isnan(F8.VALUES)) and int(np.isnan(tv).sum()) == 2
    ok = ~np.isnan(tv)
    assert np.array_equal(tv[ok], F8.VALUES[ok]) and np.array_equal(np.signbit(tv[ok]), np.signbit(F8.VALUES[ok]))
    assert F8.VALUES[0x7e] == 448 and F8.VALUES[0x01] == 2.0 ** -9 and F8.VALUES[0x08] == 2.0 ** -6
    assert len(F8.FINITE_CODES) == 254
    # every E4M3 value is a float16
    assert np.array_equal(F8.VALUES[F8.FINITE_CODES].astype(np.float16).astype(np.float64), F8.VALUES[F8.FINITE_CODES])


def test_rounding_equals_torchs_cast_for_every_finite_half_at_several_exponents():
    x = F8.finite_halves()
    assert len(x) == 63488
    x64 = x.astype(np.float64)
    for e in (-8, -7, -1, 0, 1, 5, 9, 14, 22, 32):
        y = np.ldexp(x64, e)
        y = y[np.abs(y) <= 448]
        assert len(y) >= (4 if e == 32 else 2000)      # (at e = 32 only 0 and the smallest subnormal fit)
        assert np.array_equal(y.astype(np.float32).astype(np.float64), y)       # exact in float32
        assert np.array_equal(F8.rne_e4m3(y), torch_codes(y)), e


def test_rounding_at_every_midpoint_and_below_half_the_smallest_subnormal():
    mid = F8.midpoints()
    assert len(mid) == 126
    lo, hi = F8.rne_e4m3(mid) & 0x7f, np.arange(126)
    # a tie goes to the even code of its two neighbours
    assert np.array_equal(lo, np.where(hi % 2 == 0, hi, hi + 1))
    for pts in (mid, -mid, np.nextafter(mid.astype(np.float32), np.float32(np.inf)).astype(np.float64),
                np.nextafter(mid.astype(np.float32), np.float32(0)).astype(np.float64)):
        assert np.array_equal(F8.rne_e4m3(pts), torch_codes(pts))
    tiny = np.array([2.0 ** -10, np.nextafter(np.float32(2.0 ** -10), np.float32(0)), np.nextafter(np.float32(2.0 ** -10), np.float32(1)),
                     2.0 ** -11, 2.0 ** -30, 3 * 2.0 ** -10, 0.0], dtype=np.float64)
    assert F8.rne_e4m3(tiny).tolist() == [0, 0, 1, 0, 0, 2, 0]         # 2^-10 is a tie: to zero; 3 * 2^-10: to the even 2
    assert F8.rne_e4m3(-tiny).tolist() == [0x80, 0x80, 0x81, 0x80, 0x80, 0x82, 0x80]      # the sign of a zero is kept
    assert np.array_equal(F8.rne_e4m3(tiny), torch_codes(tiny)) and np.array_equal(F8.rne_e4m3(-tiny), torch_codes(-tiny))


@pytest.mark.parametrize("tok_dim", F8.TOK_DIMS)
def test_quantiser_restatement_on_the_token_set(tok_dim):
    """The inputs the device quantiser is held to (tests/test_gpu_maxsim_fp8.py): the exponent rule in exact
    arithmetic, the codes against torch's cast of x * 2^e, no NaN code, nothing above 448."""
    tok = F8.quantiser_tokens(tok_dim)
    codes, scales = F8.quantise(tok)
    e = F8.exponents(tok)
    assert e.min() == -8 and e.max() == 32 and len(set(e.tolist())) >= 30
    amax = np.abs(tok.astype(np.float64)).max(axis=1)
    for a, ee in zip(amax.tolist(), e.tolist()):
        if a == 0:
            assert ee == 0
        else:           # the largest e with amax * 2^e <= 448, in rationals
            assert Fraction(a) * Fraction(2) ** ee <= 448 < Fraction(a) * Fraction(2) ** (ee + 1)
    assert np.array_equal(scales.astype(np.float64), np.ldexp(1.0, -e)) and np.all(F8.is_pow2(scales))
    y = np.ldexp(tok.astype(np.float64), e[:, None])
    assert np.array_equal(y.astype(np.float32).astype(np.float64), y) and np.abs(y).max() == 448
    assert np.array_equal(codes, torch_codes(y))
    assert not np.any(codes & 0x7f == 0x7f)
    # the named tokens
    z = len(tok) - 6
    assert codes[z].tolist() == [0] * tok_dim and scales[z] == 1 and codes[z + 1].tolist() == [0x80] * tok_dim
    assert scales[z + 2] == scales[z + 3] == 256 and set(codes[z + 2].tolist()) == {F8.rne_e4m3(65504 / 256).item()}
    assert set(codes[z + 3].tolist()) == {int(F8.rne_e4m3(-65504 / 256))}
    assert scales[z + 4] == 2.0 ** -32 and codes[z + 4, -1] == 0x78 and F8.VALUES[0x78] == 256
    assert codes[z + 5, 0] == 0x80 and codes[z + 5, 1] == 0x78 and scales[z + 5] == 2.0 ** -8    # 1.0 -> 256 * 2^-8
    # amax exactly 448 * 2^-e, one ulp above, one below
    for ee in F8.EDGE_EXPONENTS:
        top = np.float16(np.ldexp(448.0, -ee))
        t3 = np.stack([np.full(tok_dim, v, np.float16) for v in (top, np.nextafter(top, np.float16(np.inf)), np.nextafter(top, np.float16(0)))])
        assert F8.exponents(t3).tolist() == [ee, ee - 1, ee]
        assert (F8.quantise(t3)[0][:, 0] & 0x7f).tolist() == [0x7e, 0x76, 0x7e]       # 448; one ulp above: 224 and a bit; one below: rounds to 448
    # tokens of float16 subnormals only exist in the set
    sub = amax < 2.0 ** -14
    assert sub.sum() >= 2 and np.all(e[sub & (amax > 0)] >= 22)
    # a dequantised token is within half a grid step of the token: |x - d| <= scale * 2^-4 * |x| or scale * 2^-10
    d = F8.dequantise(codes, scales)
    x = tok.astype(np.float64)
    assert np.all(np.abs(x - d) <= np.maximum(np.abs(x) * 2.0 ** -4, scales.astype(np.float64)[:, None] * 2.0 ** -10))


def test_the_exact_family_quantises_without_loss():
    rng = np.random.default_rng(11)
    for td in F8.TOK_DIMS:
        d = MC.exact_tokens(rng, (3, 64, td))
        d[0, 0] = 0
        d[0, 1] = np.float16(0.125)
        codes, scales = F8.quantise(d)
        assert np.array_equal(F8.dequantise(codes, scales), d.astype(np.float64)), td


def test_pack_restatement_against_its_index_map():
    rng = np.random.default_rng(3)
    for td in (32, 96, 256):
        c = rng.integers(0, 256, size=(2, 64, td), dtype=np.uint8)
        p = F8.pack(c)
        assert p.shape == c.shape and np.array_equal(F8.unpack(p), c)
        img = p.reshape(2, 2, td // 32, 64, 16)
        for doc, tile, kp, lane in ((0, 0, 0, 0), (1, 1, td // 32 - 1, 63), (0, 1, 0, 31), (1, 0, td // 32 - 1, 32), (0, 0, 0, 45)):
            r, h = lane & 31, lane >> 5
            row = c[doc, 32 * tile + r]
            assert np.array_equal(img[doc, tile, kp, lane, :8], row[32 * kp + 8 * h:32 * kp + 8 * h + 8])
            assert np.array_equal(img[doc, tile, kp, lane, 8:], row[32 * kp + 16 + 8 * h:32 * kp + 16 + 8 * h + 8])


def test_the_bound_covers_a_float32_evaluation():
    rng = np.random.default_rng(9)
    q = rng.standard_normal((2, 32, 64)).astype(np.float16)
    d = rng.standard_normal((4, 64, 64)).astype(np.float16)
    cand = np.array([[0, 1, 2, 3], [3, 4, -1, 0]])
    codes, scales = F8.quantise(d)
    for n_sc, sc in enumerate((scales, F8.odd_scales(rng, scales.shape))):
        ref, bound = F8.reference(q, codes, sc, cand), F8.error_bound_fp8(q, codes, sc, cand)
        assert ref[1, 1] == -np.inf and ref[1, 2] == -np.inf and bound[1, 1] == 0.0
        v = F8.VALUES[codes].astype(np.float32)
        for qi in range(2):
            for c in range(4):
                if np.isfinite(ref[qi, c]):
                    j = cand[qi, c]
                    s = (q[qi].astype(np.float32) @ v[j].T) * sc[j][None, :]           # float32 throughout
                    assert s.dtype == np.float32
                    got = float(s.max(axis=1).sum(dtype=np.float32))
                    assert 0 < bound[qi, c] < (np.inf if n_sc else 1e-2) and abs(got - ref[qi, c]) <= bound[qi, c]
    # a non-power-of-two scale costs one more rounding, nothing else
    b2, b3 = F8.error_bound_fp8(q, codes, scales, cand), F8.error_bound_fp8(q, codes, scales * np.float32(1.5), cand)
    ok = b2 > 0
    assert np.all(b3[ok] > 1.5 * b2[ok]) and np.all(b3[ok] < 1.5 * b2[ok] * 1.05)
    # and the quantisation error itself is of another order: the FP8 scores are not the float16 scores
    fin = np.isfinite(ref)
    assert np.abs(F8.reference(q, codes, scales, cand)[fin] - MC.reference(q, d, cand)[fin]).max() > 100 * b2.max()


def test_each_built_case_has_the_property_it_is_named_for():
    for dim in (0, 9, 31):
        q, codes, scales, cand, want = F8.code_table_case(dim)
        assert codes.shape == (254, 32, 32) and np.all(scales == 1) and cand.shape == (1, 254)
        assert np.array_equal(F8.reference(q, codes, scales, cand), want)
        assert np.count_nonzero(codes[:, :, [k for k in range(32) if k != dim]]) == 0
        assert len(set(want[0].tolist())) == 253          # +0 and -0 score alike: every other value is its own
        # FNUZ would read 0x80 as NaN and every exponent one lower: the expected scores tell the two apart
        assert want[0, list(F8.FINITE_CODES).index(0x80)] == 0 and want[0, list(F8.FINITE_CODES).index(0x38)] == 32.0
    q, codes, scales, cand, want = F8.scale_row_case(96)
    assert codes.shape == (96, 96, 32) and np.array_equal(F8.reference(q, codes, scales, cand), want) and np.all(want == 64)
    for j in range(96):
        assert scales[j].sum() == 95 + 4 and scales[j, j] == 4
        wrong = scales[j].copy()
        wrong[j], wrong[(j + 1) % 96] = 1, 4            # the scale on a neighbour's row: 32 * 4
        assert F8.reference(q, codes[j:j + 1], wrong[None], np.zeros((1, 1), np.int32))[0, 0] == 128
    rng = np.random.default_rng(2)
    q, d, cand = F8.exact_case(rng, 96, 64, 160)
    codes, scales = F8.quantise(d)
    assert np.array_equal(F8.dequantise(codes, scales), d.astype(np.float64)) and (cand == -1).sum() == 2
    assert np.array_equal(F8.reference(q, codes, scales, cand), MC.reference(q, d, cand))
    s = F8.odd_scales(rng, (5, 96))
    assert s.dtype == np.float32 and np.all(s > 0) and np.all(np.isfinite(s)) and not np.any(F8.is_pow2(s))


# --------------------------------------------------------------------------- refusals that need no device
def _bare_index(**attrs):
    idx = object.__new__(GpuIndex)
    base = dict(docs=None, dim=0, n_docs=100, lex=None, doc_coll=None, tokens=None, graph=None, _lex_global=False)
    base.update(attrs)
    idx.__dict__.update(base)
    return idx


def test_set_tokens_refuses_before_any_device_work():
    E = T.NativeError
    idx = _bare_index()
    assert idx.token_store == "f16" and idx.token_scales is None
    with pytest.raises(E, match=r"store must be one of \['f16', 'fp8'\], got 'bf8'"):
        idx.set_tokens(np.zeros((4, 32, 32), np.float16), store="bf8")
    with pytest.raises(E, match=r"tok_dim 16 is not supported.*\[32, 64, 96, 128, 192, 256\]"):
        idx.set_tokens(np.zeros((4, 32, 16), np.float16), store="fp8")
    with pytest.raises(E, match=r"tok_dim 48 .*\[32, 64, 96, 128, 192, 256\]"):
        idx.set_tokens(np.zeros((4, 32, 48), np.float16), store="fp8")
    with pytest.raises(E, match="multiples of 32"):
        idx.set_tokens(np.zeros((4, 48, 32), np.float16), store="fp8")
    with pytest.raises(E, match=r"\[n, d_tokens, tok_dim\]"):
        idx.set_tokens(np.zeros((4, 32), np.float16), store="fp8")
    with pytest.raises(E, match=r"tok_dim 16"):
        idx.set_tokens_fp8(np.zeros((4, 32, 16), np.uint8), np.ones((4, 32), np.float32))
    with pytest.raises(E, match=r"scales must be \[4, 32\]"):
        idx.set_tokens_fp8(np.zeros((4, 32, 32), np.uint8), np.ones((4, 31), np.float32))
    assert idx.tokens is None and idx.token_store == "f16"


def test_append_rows_refuses_a_store_the_fp8_scorer_cannot_read():
    E = T.NativeError
    # an FP8 index whose store came past set_tokens: tok_dim 16 is refused with the FP8 list
    idx = _bare_index(tokens=torch.zeros((100, 32, 16), dtype=torch.uint8), token_store="fp8",
                      token_scales=torch.ones((100, 32)))
    with pytest.raises(E, match=r"append_rows: tokens: tok_dim 16 .*\[32, 64, 96, 128, 192, 256\]"):
        idx.append_rows(None, tokens=np.zeros((2, 32, 16), np.float16), n_rows=2)
    # ... the same shape is fine for a float16 store as far as the shape check goes
    idx16 = _bare_index(tokens=torch.zeros((100, 32, 16), dtype=torch.float16))
    assert idx16._check_tokens_part(np.zeros((2, 32, 16), np.float16), 2).shape == (2, 32, 16)
    good = _bare_index(tokens=torch.zeros((100, 32, 64), dtype=torch.uint8), token_store="fp8",
                       token_scales=torch.ones((100, 32)))
    with pytest.raises(E, match=r"tokens must be \[2, 32, 64\]"):
        good.append_rows(None, tokens=np.zeros((2, 32, 32), np.float16), n_rows=2)
    with pytest.raises(E, match="token store: tokens"):
        good.append_rows(None, n_rows=2)
    from triple_hybrid_rag_amd.index_mutate import _Storage
    assert "token_scales" in _Storage.ROWS and "tokens" in _Storage.ROWS


def test_to_gpu_refuses_before_a_device_is_asked_for(tmp_path):
    docs = np.zeros((4, 8), np.float32)
    with pytest.raises(ValueError, match="token_store must be one of"):
        IB.HostIndex(docs=docs).to_gpu(token_store="int4")
    with pytest.raises(ValueError, match="neither token matrices nor a saved FP8 image"):
        IB.HostIndex(docs=docs).to_gpu(token_store="fp8")
    with pytest.raises(T.NativeError, match=r"tok_dim 16 .*\[32, 64, 96, 128, 192, 256\]"):
        IB.HostIndex(docs=docs, tokens=np.zeros((4, 32, 16), np.float16)).to_gpu(token_store="fp8")
    # an image of another row count is not this index' image
    hi = IB.HostIndex(docs=docs, derived=dict(tokens_fp8=np.zeros((3, 32, 32), np.uint8), token_scales=np.ones((3, 32), np.float32)))
    assert hi.fp8_image() is None
    with pytest.raises(ValueError, match="neither"):
        hi.to_gpu(token_store="fp8")
    # save / load carry the image and the scales with the other derived arrays; the float16 tokens may be absent
    codes, scales = F8.quantise(MC.exact_tokens(np.random.default_rng(0), (4, 32, 32)))
    hi = IB.HostIndex(docs=docs, derived=dict(tokens_fp8=F8.pack(codes), token_scales=scales))
    IB.save(hi, str(tmp_path / "ix"))
    back = IB.load(str(tmp_path / "ix"))
    assert back.tokens is None and not os.path.exists(tmp_path / "ix" / "tokens.npy")
    c2, s2 = back.fp8_image()
    assert np.array_equal(c2, F8.pack(codes)) and c2.dtype == np.uint8 and np.array_equal(s2, scales) and s2.dtype == np.float32
    if not torch.cuda.is_available():              # (only the device is missing now)
        with pytest.raises(T.NativeError, match="HIP device"):
            back.to_gpu(token_store="fp8")


class _StubGpu:
    """What refresh_from_gpu reads of an index with an FP8 store."""
    docs = lex = graph = None
    tokens_packed, token_store, _mutations = True, "fp8", 1

    def __init__(self, n):
        self.n_docs = n


def test_refresh_from_gpu_cannot_pull_an_fp8_store_back():
    hi = IB.HostIndex(docs=np.zeros((4, 8), np.float32), tokens=np.zeros((4, 32, 32), np.float16))
    with pytest.raises(ValueError, match="cannot be pulled back"):
        IB.refresh_from_gpu(hi, _StubGpu(6))
    IB.refresh_from_gpu(hi, _StubGpu(4))          # in step: trusted, as the packed float16 store is
    assert hi.tokens.shape == (4, 32, 32)
    hi.tokens = None                               # a deployment without the float16 tokens: nothing to pull
    IB.refresh_from_gpu(hi, _StubGpu(6))
