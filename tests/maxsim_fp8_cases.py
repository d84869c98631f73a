"""Inputs, restatements and bounds of the FP8 token-store tests (tests/test_maxsim_fp8_host.py,
tests/test_gpu_maxsim_fp8.py).  Pure numpy: nothing here needs a GPU.

The store (include/thr_hip_rerank.h): a document token x (float16 [tok_dim]) is kept as tok_dim OCP
E4M3FN codes and one float32 scale, x_k ~ scale * value(code_k).  The reference of every score is
oracle.thr_oracle.maxsim_scores over the DEQUANTISED tokens (float64: scale * value is exact there).

THE QUANTISER, restated (``quantise``):
    amax = max_k |x_k|;  e = floor(log2(448 / amax)) -- the largest e with amax * 2^e <= 448 --, 0 for
    amax == 0;  code_k = RNE_e4m3(x_k * 2^e);  scale = 2^-e.
Here e comes from frexp (amax = m * 2^p, 0.5 <= m < 1; 448 = 0.875 * 2^9: e = 9 - p when m <= 0.875,
else 8 - p) and RNE_e4m3 from float64 arithmetic on exact values (``rne_e4m3``: the grid's quantum is
2^-9 below 2^-6 and 2^(floor(log2 |y|) - 3) above; numpy's rint rounds ties to even); the device uses the
bits of the float32 instead.  The two meet in the tests, and both meet torch's float8_e4m3fn cast.

THE IMAGE, restated (``pack``): [doc][tile of 32 tokens][k-pair = tok_dim / 32][lane][16 bytes], lane
32 h + r holding token 32 tile + r, its bytes 0..7 dims 32 kp + 8 h .. + 8, its bytes 8..15 dims
32 kp + 16 + 8 h .. + 8.

THE BOUND (``error_bound_fp8``).  The device computes, in float32, s^_ij = fl(scale_j * D^_ij) with D^_ij
the accumulated dot product of tok_dim exact products (float16 x float16) -- any order --, then max_j,
then the sum over the q_tokens maxima.  With u = 2^-24 and gamma(n) = n u / (1 - n u):
    |D^_ij - D_ij| <= gamma(tok_dim) * A_ij,  A_ij = sum_k |q_ik| |v_jk|          (v: the code's value)
    s^_ij = scale_j * D^_ij * (1 + d), |d| <= u -- d = 0 when scale_j is a power of two (no rounding;
    no score of the tests is near 2^-126) --, so every term carries at most tok_dim + 1 factors (1 + d):
    |s^_ij - s_ij| <= gamma(tok_dim + x) * scale_j * A_ij,  x = 1 if a scale is not a power of two else 0
    the max is exact and monotone:  |m^_i - m_i| <= eps_i = max_j gamma(tok_dim + x) scale_j A_ij
    the sum of q_tokens values:  |S^ - S| <= E + gamma(q_tokens) * (sum_i |m_i| + E),  E = sum_i eps_i
scale_j * A_ij is sum_k |q_ik| |d_jk| over the dequantised tokens d, so the bound is
maxsim_cases.error_bound's over the dequantised tokens with one more rounding in the first gamma (and the
second-order term kept).  0 where the score is -inf.
"""
import numpy as np

import maxsim_cases as MC

TOK_DIMS = (32, 64, 96, 128, 192, 256)           # one kernel instantiation each (tok_dim / 32)
E4M3_MAX = 448.0


def _value_table() -> np.ndarray:
    v = np.empty(256, dtype=np.float64)
    for c in range(256):
        exp, man = (c >> 3) & 15, c & 7
        if exp == 15 and man == 7:
            mag = np.nan                          # E4M3FN: no infinities, one NaN per sign
        elif exp == 0:
            mag = man * 2.0 ** -9
        else:
            mag = (1 + man / 8.0) * 2.0 ** (exp - 7)
        v[c] = -mag if c & 0x80 else mag
    return v


VALUES = _value_table()                           # OCP E4M3FN: code -> value
FINITE_CODES = np.array([c for c in range(256) if c & 0x7f != 0x7f], dtype=np.uint8)    # 254 of them
_POS = VALUES[:0x7f]                              # 0 .. 448, ascending, code = index


def rne_e4m3(y) -> np.ndarray:
    """Exact values |y| <= 448 (float64) -> their E4M3FN codes, round to nearest, ties to the even code."""
    y = np.asarray(y, dtype=np.float64)
    a = np.abs(y)
    assert np.all(a <= E4M3_MAX)
    with np.errstate(divide="ignore"):
        q = np.where(a < 2.0 ** -6, 2.0 ** -9, 2.0 ** (np.floor(np.log2(np.maximum(a, 2.0 ** -6))) - 3))
    v = np.rint(a / q) * q                        # (a / q is exact: q is a power of two)
    code = np.searchsorted(_POS, v).astype(np.uint8)
    assert np.array_equal(_POS[code], v)
    return code | (np.signbit(y).astype(np.uint8) << 7)


def exponents(dtok: np.ndarray) -> np.ndarray:
    """e per token (int, [...]) of float16 tokens [..., tok_dim]."""
    amax = np.abs(dtok.astype(np.float64)).max(axis=-1)
    m, p = np.frexp(amax)
    e = np.where(m <= 0.875, 9 - p, 8 - p)
    return np.where(amax == 0, 0, e).astype(np.int64)


def quantise(dtok: np.ndarray):
    """float16 [..., tok_dim] -> (codes uint8 [..., tok_dim] ROW-MAJOR, scales float32 [...])."""
    assert dtok.dtype == np.float16 and np.all(np.isfinite(dtok))
    e = exponents(dtok)
    codes = rne_e4m3(np.ldexp(dtok.astype(np.float64), e[..., None]))
    return codes, np.ldexp(1.0, -e).astype(np.float32)


def dequantise(codes: np.ndarray, scales: np.ndarray) -> np.ndarray:
    """Row-major codes [..., tok_dim], scales [...] -> the tokens the scorer sees, float64 (exact)."""
    return scales.astype(np.float64)[..., None] * VALUES[codes]


def pack(codes: np.ndarray) -> np.ndarray:
    """Row-major codes [n, d_tokens, tok_dim] -> the packed image, same shape (see the module docstring)."""
    n, dt, td = codes.shape
    x = codes.reshape(n, dt // 32, 32, td // 32, 2, 2, 8)    # [doc][tile][r][kp][half of the 16 bytes][h][8]
    return np.ascontiguousarray(x.transpose(0, 1, 3, 5, 2, 4, 6)).reshape(n, dt, td)   # [doc][tile][kp][h][r][half][8]


def unpack(image: np.ndarray) -> np.ndarray:
    n, dt, td = image.shape
    x = image.reshape(n, dt // 32, td // 32, 2, 32, 2, 8)
    return np.ascontiguousarray(x.transpose(0, 1, 4, 2, 5, 3, 6)).reshape(n, dt, td)


def is_pow2(scales: np.ndarray) -> np.ndarray:
    m, _ = np.frexp(scales.astype(np.float64))
    return m == 0.5


def error_bound_fp8(qtok, codes, scales, cand) -> np.ndarray:
    """The bound of the module docstring, per score, float64; codes row-major."""
    d = dequantise(codes, scales)
    extra = 0 if np.all(is_pow2(scales)) else 1
    cand = MC.local_candidates(cand, d.shape[0])
    nq, qt, td = qtok.shape
    out = np.zeros(cand.shape, dtype=np.float64)
    for q in range(nq):
        a = qtok[q].astype(np.float64)
        for c in range(cand.shape[1]):
            j = int(cand[q, c])
            if j < 0:
                continue
            E = MC.gamma(td + extra) * (np.abs(a) @ np.abs(d[j]).T).max(axis=1).sum()
            mx = np.abs((a @ d[j].T).max(axis=1)).sum()
            out[q, c] = E + MC.gamma(qt) * (mx + E)
    return out


def reference(qtok, codes, scales, cand, id_base=None) -> np.ndarray:
    """float64 MaxSim of the oracle over the dequantised tokens, -inf where the device owes -inf."""
    return MC.reference(qtok, dequantise(codes, scales), cand, id_base)


# ----------------------------------------------------------------------------------- quantiser inputs
def finite_halves() -> np.ndarray:
    """All 63 488 finite float16 values, in the order of their bits (neighbours are close in magnitude)."""
    x = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    return x[np.isfinite(x)]


def midpoints() -> np.ndarray:
    """The 126 round-to-even midpoints between neighbouring non-negative E4M3 values (float64, exact)."""
    return (_POS[:-1] + _POS[1:]) / 2


def edge_values(e: int) -> np.ndarray:
    """float16 values x whose x * 2^e sits on the edges of the E4M3 rounding, both signs: every midpoint and
    its float16 neighbours, around half the smallest subnormal (2^-10: a tie that goes to zero), the grid
    itself.  Only those that float16 holds exactly are kept (all of them for the e of the tests)."""
    pts = np.concatenate([midpoints(), _POS, [2.0 ** -10, 2.0 ** -11, 2.0 ** -12, 3 * 2.0 ** -11]])
    x = np.ldexp(pts, -e)
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    h = h[np.isfinite(h) & (h.astype(np.float64) == x)]
    near = np.concatenate([h, np.nextafter(h, np.float16(np.inf)), np.nextafter(h, np.float16(0))])
    near = near[np.isfinite(near) & (np.abs(near.astype(np.float64)) <= np.ldexp(E4M3_MAX, -e))]
    return np.concatenate([near, -near])


EDGE_EXPONENTS = (-7, -3, 0, 1, 8, 15, 22)        # 448 * 2^-e is a float16 for each


def quantiser_tokens(tok_dim: int) -> np.ndarray:
    """float16 [n_tokens, tok_dim]: what the quantiser is held to, laid out as tokens.
      * every finite float16 value, consecutive bit patterns sharing a token (tokens of float16
        subnormals only, of +-65504, of one binade: exponents from -8 up to the high twenties);
      * for each e of EDGE_EXPONENTS tokens whose amax is exactly 448 * 2^-e (at a moving position, either
        sign) and whose other elements are edge_values(e): every midpoint at that exponent;
      * tokens whose amax is one float16 ulp above / below 448 * 2^-e (the exponent flips between them);
      * an all-zero token, an all -0.0 token, tokens of 65504 and of -65504, single-element tokens."""
    rows = []
    fin = finite_halves()
    pad = (-len(fin)) % tok_dim
    rows.append(np.concatenate([fin, np.zeros(pad, np.float16)]).reshape(-1, tok_dim))
    for n_e, e in enumerate(EDGE_EXPONENTS):
        top = np.float16(np.ldexp(E4M3_MAX, -e))
        assert float(top) == np.ldexp(E4M3_MAX, -e)
        vals = edge_values(e)
        per = tok_dim - 1
        vals = np.concatenate([vals, np.zeros((-len(vals)) % per, np.float16)]).reshape(-1, per)
        for t, v in enumerate(vals):
            at = (t + n_e) % tok_dim
            rows.append(np.insert(v, at, top if t % 2 == 0 else -top)[None])
        for amax in (np.nextafter(top, np.float16(np.inf)), np.nextafter(top, np.float16(0))):
            tok = np.resize(vals[0] / np.float16(2), tok_dim).astype(np.float16)
            tok[n_e % tok_dim] = -amax if n_e % 2 else amax
            rows.append(tok[None])
    special = np.zeros((6, tok_dim), dtype=np.float16)
    special[1] = np.float16(-0.0)
    special[2], special[3] = np.float16(65504), np.float16(-65504)
    special[4, tok_dim - 1] = np.float16(2.0 ** -24)         # the smallest subnormal alone: e = 32
    special[5, 0], special[5, 1] = np.float16(-0.0), np.float16(1.0)
    rows.append(special)
    return np.concatenate(rows).astype(np.float16)


def as_store(tokens: np.ndarray, d_tokens: int) -> np.ndarray:
    """Tokens [m, tok_dim] -> a store [n, d_tokens, tok_dim], zero tokens behind the last one."""
    m, td = tokens.shape
    pad = (-m) % d_tokens
    return np.concatenate([tokens, np.zeros((pad, td), np.float16)]).reshape(-1, d_tokens, td)


# ----------------------------------------------------------------------------------- scorer cases
def code_table_case(dim: int):
    """254 documents of 32 x 32 tokens, document c holding finite code FINITE_CODES[c] in dim ``dim`` of every
    token and scale 1; one query of 32 tokens e_dim -> (qtok, codes row-major, scales, cand, expected
    float64 = 32 * value(code))."""
    n = len(FINITE_CODES)
    codes = np.zeros((n, 32, 32), dtype=np.uint8)
    codes[:, :, dim] = FINITE_CODES[:, None]
    scales = np.ones((n, 32), dtype=np.float32)
    q = np.zeros((1, 32, 32), dtype=np.float16)
    q[0, :, dim] = 1
    cand = np.arange(n, dtype=np.int32)[None]
    return q, codes, scales, cand, 32 * VALUES[FINITE_CODES][None]


def scale_row_case(d_tokens: int = 96):
    """One document per token position j*: token j* is 0.5 e_0 with scale 4, every other token 1.0 e_0 with
    scale 1; one query of 32 tokens e_0.  Every score is 32 * 2; a scale applied to another accumulator
    register's row gives 32 * 4 or 32 * 1."""
    half, one = int(rne_e4m3(0.5)), int(rne_e4m3(1.0))
    codes = np.zeros((d_tokens, d_tokens, 32), dtype=np.uint8)
    codes[:, :, 0] = one
    scales = np.ones((d_tokens, d_tokens), dtype=np.float32)
    for j in range(d_tokens):
        codes[j, j, 0], scales[j, j] = half, 4.0
    q = np.zeros((1, 32, 32), dtype=np.float16)
    q[0, :, 0] = 1
    return q, codes, scales, np.arange(d_tokens, dtype=np.int32)[None], np.full((1, d_tokens), 64.0)


def exact_case(rng, tok_dim: int, q_tokens: int, d_tokens: int, n_docs: int = 5, n_queries: int = 2):
    """The exact family of maxsim_cases (multiples of 1/8 in [-1, 1]): it quantises without loss, and every
    float32 partial sum of the scorer is exact whatever the order (maxsim_cases' argument; a power-of-two
    scale changes no mantissa) -> (qtok, dtok float16, cand int32 with every document and a -1)."""
    q = MC.exact_tokens(rng, (n_queries, q_tokens, tok_dim))
    d = MC.exact_tokens(rng, (n_docs, d_tokens, tok_dim))
    cand = np.stack([np.concatenate([rng.permutation(n_docs), [-1]]) for _ in range(n_queries)]).astype(np.int32)
    return q, d, cand


def odd_scales(rng, shape) -> np.ndarray:
    """Finite positive float32 scales that are NOT powers of two (three to nine significant bits)."""
    s = (rng.integers(129, 256, size=shape) / 128.0 * 2.0 ** rng.integers(-6, 3, size=shape)).astype(np.float32)
    assert not np.any(is_pow2(s))
    return s
