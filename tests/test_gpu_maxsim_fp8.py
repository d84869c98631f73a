"""The FP8 token store on the GPU (include/thr_hip_rerank.h): the code table of the in-register
conversion, the scale's accumulator row, the device quantiser against its numpy restatement, every
instantiation of the scorer against float64, the edges of the grid and of the number format, and
GpuIndex.set_tokens(store="fp8") through rerank, append, delete and save / load.

The reference of every score is oracle.thr_oracle.maxsim_scores over the DEQUANTISED tokens
(tests/maxsim_fp8_cases.py).  Exact-family inputs are compared with np.array_equal; real-valued inputs
are held to error_bound_fp8, computed from the inputs.  Each real-valued case prints its largest
error / bound (run with -s)."""
import functools
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import maxsim_cases as MC  # noqa: E402
import maxsim_fp8_cases as F8  # noqa: E402

ID_BASE = 7000


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def f64(t):
    return t.cpu().numpy().astype(np.float64)


def score(T, q, codes, scales, cand):
    """thr_maxsim_fp8 over ROW-MAJOR codes (packed here by the restatement) -> float64."""
    out = T._native.maxsim_fp8(dev(q), dev(F8.pack(codes)), dev(scales), dev(np.asarray(cand, dtype=np.int32)))
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(np.shape(cand))
    return f64(out)


def both_entry_points(T, q, image, scales, cand):
    """(thr_maxsim_fp8 on local indices, thr_maxsim_fp8_ids on the same candidates as global ids) over a
    device image."""
    N = T._native
    cand = np.asarray(cand)
    gids = np.where(cand >= 0, cand.astype(np.int64) + ID_BASE, -1)
    return (f64(N.maxsim_fp8(dev(q), image, scales, dev(cand.astype(np.int32)))),
            f64(N.maxsim_fp8_ids(dev(q), image, scales, dev(gids), ID_BASE)))


def assert_exact(got, ref, what):
    assert got.shape == ref.shape and np.array_equal(got, ref), \
        f"{what}: {int((got != ref).sum())} of {ref.size} scores differ, first at " \
        f"{tuple(np.argwhere(got != ref)[0])}: got {got[got != ref][0]!r}, reference {ref[got != ref][0]!r}"


# ------------------------------------------------------------------ the conversion, code by code
@pytest.mark.parametrize("dim", (0, 9, 31))
def test_code_table(T, dim):
    """Document c holds finite code c in dim ``dim`` of every token, scale 1; the query is 32 tokens e_dim:
    score c is 32 * value_OCP(c), to the bit, for all 254 finite codes.  FNUZ would halve every normal and
    make 0x80 a NaN; a swapped byte order would read a zero.  Dims 0, 9 and 31: bytes 0..7 of the lane with
    h = 0, bytes 0..7 with h = 1 (k-step 0), bytes 8..15 with h = 1 (k-step 1)."""
    q, codes, scales, cand, want = F8.code_table_case(dim)
    got = score(T, q, codes, scales, cand)
    assert_exact(got, want, f"code table, dim {dim}")
    neg0 = list(F8.FINITE_CODES).index(0x80)
    assert got[0, neg0] == 0 and not np.isnan(got).any()


# ------------------------------------------------------------------ the scale and its accumulator row
def test_scale_reaches_its_own_row(T):
    """For every token position j* in 0..95 (three tiles: a pair and the tail): token j* is 0.5 e_0 with
    scale 4, the others 1.0 e_0 with scale 1 -> 32 * 2.  A scale on a neighbouring register: 32 * 4 or 32."""
    q, codes, scales, cand, want = F8.scale_row_case(96)
    got = score(T, q, codes, scales, cand)
    wrong = np.flatnonzero(got[0] != 64.0)
    assert_exact(got, want, f"scale row (token positions {wrong.tolist()} score {got[0][wrong].tolist()})")
    # ... and with two and four tiles (pairs only), one and five (a lone tail, two pairs and a tail)
    for dt in (32, 64, 128, 160):
        q, codes, scales, cand, want = F8.scale_row_case(dt)
        assert_exact(score(T, q, codes, scales, cand), want, f"scale row, d_tokens {dt}")


# ------------------------------------------------------------------ the quantiser
@pytest.mark.parametrize("tok_dim", F8.TOK_DIMS, ids=lambda td: f"td{td}")
def test_quantiser_equals_the_restatement(T, tok_dim):
    """Codes (the documented packed image) and scales of the device, byte for byte, on the inputs the host
    test holds the restatement to: every finite float16, every midpoint, the exponent flips, zeros, -0.0,
    +-65504, subnormal-only tokens."""
    tok = F8.quantiser_tokens(tok_dim)
    for dt in (32, 96):
        store = F8.as_store(tok, dt)
        codes, scales = T._native.maxsim_quantize_fp8(dev(store))
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == store.shape
        assert scales.dtype == torch.float32 and tuple(scales.shape) == store.shape[:2]
        want_c, want_s = F8.quantise(store)
        got_c, got_s = codes.cpu().numpy(), scales.cpu().numpy()
        assert np.array_equal(got_s.view(np.uint32), want_s.view(np.uint32)), \
            (tok_dim, dt, "scales", np.argwhere(got_s != want_s)[:4].tolist())
        bad = np.argwhere(F8.unpack(got_c) != want_c)
        assert len(bad) == 0, (tok_dim, dt, "codes", len(bad), bad[:4].tolist(),
                               [(hex(F8.unpack(got_c)[tuple(b)]), hex(want_c[tuple(b)]), float(store[tuple(b)])) for b in bad[:4]])
        assert np.array_equal(got_c, F8.pack(want_c))
        # the same bits every run
        again = T._native.maxsim_quantize_fp8(dev(store))
        assert torch.equal(again[0], codes) and torch.equal(again[1], scales)


# ------------------------------------------------------------------ every instantiation
Q_TOKENS, D_TOKENS = (32, 64), (32, 64, 96, 160)


@functools.lru_cache(maxsize=None)
def exact_inputs(tok_dim, qt, dt):
    rng = np.random.default_rng(1000 * tok_dim + qt + dt)
    q, d, cand = F8.exact_case(rng, tok_dim, qt, dt)
    return q, d, cand, MC.reference(q, d, cand)


@pytest.mark.parametrize("tok_dim", F8.TOK_DIMS, ids=lambda td: f"td{td}")
def test_every_instantiation_exact(T, tok_dim):
    """Exact family (it quantises without loss): both entry points return the bits of the float64
    reference -- which is also the float16 store's -- and of the float16 kernel."""
    N = T._native
    for qt in Q_TOKENS:
        for dt in D_TOKENS:
            q, d, cand, ref = exact_inputs(tok_dim, qt, dt)
            image, scales = N.maxsim_quantize_fp8(dev(d))
            rows = F8.unpack(image.cpu().numpy())
            assert np.array_equal(F8.dequantise(rows, scales.cpu().numpy()), d.astype(np.float64))
            assert np.isinf(ref).sum() == 2 and np.array_equal(ref, F8.reference(q, rows, scales.cpu().numpy(), cand))
            f16 = f64(N.maxsim(dev(q), N.maxsim_pack(dev(d)), dev(cand), packed=True))
            for got, name in zip(both_entry_points(T, q, image, scales, cand), ("thr_maxsim_fp8", "thr_maxsim_fp8_ids")):
                assert_exact(got, ref, f"{name} td{tok_dim} q{qt} d{dt}")
                assert_exact(got, f16, f"{name} against thr_maxsim, td{tok_dim} q{qt} d{dt}")


@pytest.mark.parametrize("family", ("unit", "normal"))
@pytest.mark.parametrize("tok_dim", F8.TOK_DIMS, ids=lambda td: f"td{td}")
def test_every_instantiation_real_valued(T, tok_dim, family):
    """Real-valued tokens quantised by the device: within error_bound_fp8 of MaxSim over the dequantised
    tokens.  (The distance to the float16 store's scores is the quantisation error: printed, not bounded.)"""
    N = T._native
    rng = np.random.default_rng(7 * tok_dim + len(family))
    worst = 0.0
    for qt, dt in ((32, 96), (64, 160), (64, 32)):
        q = MC.real_tokens(family, rng, 3, qt, tok_dim, queries=True)
        d = MC.real_tokens(family, rng, 6, dt, tok_dim, queries=False)
        cand = np.stack([rng.permutation(6) for _ in range(3)]).astype(np.int32)
        cand[1, 2] = -1
        image, scales = N.maxsim_quantize_fp8(dev(d))
        rows, sc = F8.unpack(image.cpu().numpy()), scales.cpu().numpy()
        assert np.array_equal(rows, F8.quantise(d)[0]) and np.array_equal(sc, F8.quantise(d)[1])
        ref, bound = F8.reference(q, rows, sc, cand), F8.error_bound_fp8(q, rows, sc, cand)
        for got, name in zip(both_entry_points(T, q, image, scales, cand), ("thr_maxsim_fp8", "thr_maxsim_fp8_ids")):
            assert np.array_equal(np.isinf(got), np.isinf(ref)) and got[1, 2] == -np.inf
            fin = np.isfinite(ref)
            err = np.abs(got[fin] - ref[fin])
            worst = max(worst, float((err / bound[fin]).max()))
            print(f"{name} {family} td{tok_dim} q{qt} d{dt}: max err {err.max():.3e}, bound {bound[fin].min():.3e}.."
                  f"{bound[fin].max():.3e}, |fp8 - f16 store| {np.abs(ref[fin] - MC.reference(q, d, cand)[fin]).max():.3e}")
            assert np.all(err <= bound[fin]), (name, family, tok_dim, qt, dt, float(err.max()), float(bound[fin].min()))
    assert worst <= 1.0


def test_hand_set_scales_through_the_raw_abi(T):
    """Scales that are NOT powers of two (the kernel takes any finite positive scale), codes drawn from the
    whole finite table, handed to thr_maxsim_fp8 / _ids as pointers: within the bound with its extra rounding."""
    rng = np.random.default_rng(77)
    td, qt, dt, nd, nq = 96, 64, 96, 7, 3
    codes = F8.FINITE_CODES[rng.integers(0, 254, size=(nd, dt, td))]
    codes = np.where(rng.random(codes.shape) < 0.7, codes & 0xbf, codes).astype(np.uint8)     # mostly |v| < 2
    scales = F8.odd_scales(rng, (nd, dt))
    q = rng.standard_normal((nq, qt, td)).astype(np.float16)
    cand = np.stack([rng.permutation(nd) for _ in range(nq)]).astype(np.int32)
    ref, bound = F8.reference(q, codes, scales, cand), F8.error_bound_fp8(q, codes, scales, cand)
    lib = T._native.load()
    qd, cd, sd, c32 = dev(q), dev(F8.pack(codes)), dev(scales), dev(cand)
    c64 = dev(cand.astype(np.int64) + ID_BASE)
    out = torch.empty((2, nq, nd), dtype=torch.float32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.thr_maxsim_fp8(qd.data_ptr(), nq, qt, cd.data_ptr(), sd.data_ptr(), nd, dt, td, c32.data_ptr(), nd,
                              out[0].data_ptr(), stream) == 0
    assert lib.thr_maxsim_fp8_ids(qd.data_ptr(), nq, qt, cd.data_ptr(), sd.data_ptr(), nd, dt, td, c64.data_ptr(), ID_BASE,
                                  nd, out[1].data_ptr(), stream) == 0
    got = f64(out)
    err = np.abs(got - ref[None])
    print(f"hand-set scales: max err {err.max():.3e}, bound {bound.min():.3e}..{bound.max():.3e}")
    assert np.all(err <= bound[None]) and err.max() > 0      # (a real rounding happened: the bound is not idle)
    assert np.array_equal(got[0], got[1])


# ------------------------------------------------------------------ edges of the grid
@pytest.mark.parametrize("nq", (1, 3))
@pytest.mark.parametrize("n_cand", (1, 4, 5, 257))
def test_candidate_edges(T, n_cand, nq):
    """n_cand around the 4 waves of a block; negative, too-large and other-shard candidates -> -inf; an
    id_base that is not 0."""
    rng = np.random.default_rng(n_cand * 10 + nq)
    td, n_docs = 64, 9
    q, d = MC.exact_tokens(rng, (nq, 32, td)), MC.exact_tokens(rng, (n_docs, 64, td))
    cand = rng.integers(0, n_docs, (nq, n_cand)).astype(np.int64)
    bad = [-1, -5, n_docs, n_docs + 1, 2 ** 31 - 1, -(2 ** 31)]
    for k in range(min(n_cand, len(bad)) if n_cand > 1 else 0):
        cand[rng.integers(0, nq), rng.integers(0, n_cand)] = bad[k]
    image, scales = T._native.maxsim_quantize_fp8(dev(d))
    ref = MC.reference(q, d, cand)
    got = f64(T._native.maxsim_fp8(dev(q), image, scales, dev(cand.astype(np.int32))))
    assert_exact(got, ref, f"thr_maxsim_fp8 n_cand {n_cand} nq {nq}")
    if n_cand == 1:
        lone = np.full((nq, 1), -1, dtype=np.int32)
        assert np.all(f64(T._native.maxsim_fp8(dev(q), image, scales, dev(lone))) == -np.inf)
    for base in (0, ID_BASE, 2 ** 40):
        gid = np.where((cand >= 0) & (cand < n_docs), cand + base, cand)
        # ids of another shard: below the base, at and above base + n_docs, negative
        other = gid.copy()
        if n_cand > 1:
            other[0, 0], other[-1, -1] = base + n_docs, (base - 1 if base else -1)
        want = MC.reference(q, d, other, id_base=base)
        got = f64(T._native.maxsim_fp8_ids(dev(q), image, scales, dev(other), base))
        assert_exact(got, want, f"thr_maxsim_fp8_ids n_cand {n_cand} nq {nq} id_base {base}")
        if n_cand > 1:
            assert got[0, 0] == -np.inf and got[-1, -1] == -np.inf


def test_float16_extremes_and_subnormals(T):
    """Document tokens at the ends of float16, scored exactly against the reference over the dequantised
    tokens.  +-65504: e = -8 (scale 2^8), the code is 256 (255.875 rounds up), the dequantised token
    +-65536; one-hot queries of +-65504 keep every product (2047 * 2^21) and sum of four exact.
    Subnormals 16 k * 2^-24, |k| <= 7, amax 112 * 2^-24: e = 26 (scale 2^-26), scaled values 64 k are E4M3
    values, so the store is lossless; a token whose only element is 2^-24: e = 32 (scale 2^-32)."""
    rng = np.random.default_rng(9)
    big = np.float16(65504.0)
    td, qt, dt, nq, n_docs = 64, 32, 64, 5, 7
    d = (rng.choice([-1.0, 1.0], (n_docs, dt, td)) * 65504.0).astype(np.float16)
    d[6] = -big
    q = np.zeros((nq, qt, td), dtype=np.float16)
    for qi in range(nq):
        for t in rng.choice(qt, 4, replace=False):
            q[qi, t, rng.integers(0, td)] = big if (qi + t) % 3 else -big
    q[4] = 0
    q[4, 31, 0], q[4, 0, 2] = big, big
    cand = np.tile(np.arange(n_docs, dtype=np.int32), (nq, 1))
    image, scales = T._native.maxsim_quantize_fp8(dev(d))
    rows, sc = F8.unpack(image.cpu().numpy()), scales.cpu().numpy()
    assert np.all(sc == 256.0) and set(np.unique(rows).tolist()) == {0x78, 0xf8}
    ref = F8.reference(q, rows, sc, cand)
    assert ref[4, 6] == -2 * 65504.0 * 65536.0 and np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    for got, name in zip(both_entry_points(T, q, image, scales, cand), ("thr_maxsim_fp8", "thr_maxsim_fp8_ids")):
        assert_exact(got, ref, f"+-65504, {name}")
    # subnormal document tokens against multiples of 1/8
    td, qt, dt = 96, 64, 64
    sub = (16 * rng.integers(-7, 8, (5, dt, td)) * 2.0 ** -24).astype(np.float16)
    sub[:, :, 0] = np.float16(112 * 2.0 ** -24)
    sub[4] = -np.abs(sub[4])
    sub[3] = 0
    sub[3, 17, 5] = 2.0 ** -24
    assert np.all(np.abs(sub.astype(np.float64)) < 2.0 ** -14)
    other = MC.exact_tokens(rng, (3, qt, td))
    other[2] = 0
    other[2, :, 5] = 1.0
    cand = np.tile(np.arange(5, dtype=np.int32), (3, 1))
    image, scales = T._native.maxsim_quantize_fp8(dev(sub))
    rows, sc = F8.unpack(image.cpu().numpy()), scales.cpu().numpy()
    assert np.all(sc[[0, 1, 2, 4]] == 2.0 ** -26) and sc[3, 17] == 2.0 ** -32 and sc[3, 0] == 1.0
    assert np.array_equal(F8.dequantise(rows, sc), sub.astype(np.float64))          # lossless
    ref = MC.reference(other, sub, cand)
    assert ref[2, 3] == qt * 2.0 ** -24 and np.count_nonzero(ref) >= ref.size - 2
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    for got, name in zip(both_entry_points(T, other, image, scales, cand), ("thr_maxsim_fp8", "thr_maxsim_fp8_ids")):
        assert_exact(got, ref, f"subnormal documents, {name}")


def test_many_queries_in_one_call(T):
    """65 600 queries of 32 x 32 x 32 in one call (queries sit on gridDim.y; the launch goes out in slices).
    Query q is pool[q % 257] -- 257 is prime, so a slice that started at the wrong row of qtok, cand or out
    would not line up."""
    rng = np.random.default_rng(65600)
    nq, pool_n, n_docs, td, n_cand = 65600, 257, 13, 32, 3
    pool = MC.exact_tokens(rng, (pool_n, 32, td))
    d = MC.exact_tokens(rng, (n_docs, 32, td))
    table = MC.reference(pool, d, np.tile(np.arange(n_docs), (pool_n, 1)))      # [pool, doc]
    which = np.arange(nq) % pool_n
    q = pool[which]
    cand = rng.integers(0, n_docs, (nq, n_cand)).astype(np.int32)
    cand[rng.integers(0, nq, 500), rng.integers(0, n_cand, 500)] = -1
    cand[-1, -1], cand[65535, 0], cand[65536, 1] = -1, -1, -1
    ref = np.where(cand >= 0, table[which[:, None], np.maximum(cand, 0)], -np.inf)
    N = T._native
    image, scales = N.maxsim_quantize_fp8(dev(d))
    qd = dev(q)
    assert_exact(f64(N.maxsim_fp8(qd, image, scales, dev(cand))), ref, "thr_maxsim_fp8, 65 600 queries")
    gids = np.where(cand >= 0, cand.astype(np.int64) + ID_BASE, -1)
    assert_exact(f64(N.maxsim_fp8_ids(qd, image, scales, dev(gids), ID_BASE)), ref, "thr_maxsim_fp8_ids, 65 600 queries")


# ------------------------------------------------------------------ the index
def _lex_rows(rng, n, v, per=12):
    term = np.minimum((v * rng.random((n, per)) ** 3).astype(np.int32), v - 1).reshape(-1)
    doc = np.repeat(np.arange(n, dtype=np.int32), per)
    tf = rng.geometric(0.5, n * per).astype(np.int32)
    return doc, term, tf


@pytest.fixture(scope="module")
def corpus():
    rng = np.random.default_rng(31)
    n, d, v, nq = 3000, 768, 900, 12
    x = rng.standard_normal((n, d)).astype(np.float32)
    x *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    doc, term, tf = _lex_rows(rng, n, v)
    pool = MC.exact_tokens(rng, (211, 32, 64))
    dtok = pool[rng.integers(0, 211, n)]                      # docs share token matrices: exact ties
    qtok = MC.exact_tokens(rng, (nq, 32, 64))
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qt = rng.integers(0, v, (nq, 4)).astype(np.int32)
    return dict(n=n, v=v, x=x, doc=doc, term=term, tf=tf, dtok=dtok, qtok=qtok, q=q, qt=qt)


def _build(T, C, rows):
    """A fresh index over the (sorted) row numbers ``rows`` of the corpus, FP8 token store."""
    rows = np.asarray(rows)
    remap = np.full(C["n"], -1, dtype=np.int64)
    remap[rows] = np.arange(len(rows))
    sel = remap[C["doc"]] >= 0
    idx = T.GpuIndex().set_dense(C["x"][rows])
    idx.set_lexical_rows(remap[C["doc"][sel]].astype(np.int32), C["term"][sel], C["tf"][sel], C["v"], n_docs=len(rows))
    return idx.set_tokens(C["dtok"][rows], store="fp8")


def _check_rerank(T, idx, C, rows, what):
    """The rerank leg of retrieve_batch against the oracle: fused top-100 -> float64 MaxSim over the
    DEQUANTISED tokens -> O.rerank_order.  Ids, float64 scores and counts, every query."""
    rows = np.asarray(rows)
    x, n = C["x"][rows], len(rows)
    assert idx.n_docs == n and idx.token_store == "fp8" and idx.tokens.dtype == torch.uint8
    assert tuple(idx.tokens.shape) == (n, 32, 64) and tuple(idx.token_scales.shape) == (n, 32)
    deq = F8.dequantise(F8.unpack(idx.tokens.cpu().numpy()), idx.token_scales.cpu().numpy())
    assert np.array_equal(deq, C["dtok"][rows].astype(np.float64))          # (exact family: lossless)
    L = idx.lex
    rowptr, pd, ptf, dl, idf = (L[k].cpu().numpy() for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"))
    _, Id, _ = CO.dense_topk_exact(x, C["q"], 100)
    _, Il = O.bm25_topk(rowptr, pd, ptf, dl, idf, L["avgdl"], C["qt"], n, 50)
    out = []
    for top_k in (10, 100):
        res = idx.retrieve_batch(dev(C["q"]), dev(C["qt"]), top_k=top_k, qtok=dev(C["qtok"]), rerank_top_k=100)
        ids, sc, cnt = res.ids.cpu().numpy(), res.scores.cpu().numpy(), res.counts.cpu().numpy()
        for i in range(len(C["q"])):
            f100, _ = O.fused_topk_ids(list(Il[i]), list(Id[i]), None, 100)
            ms = O.maxsim_scores(C["qtok"][i:i + 1], deq, np.array([f100], dtype=np.int64))[0]
            order = O.rerank_order(list(ms))[:top_k]
            assert int(cnt[i]) == len(order), f"{what} top_k {top_k} query {i}: count"
            assert list(ids[i]) == [f100[j] for j in order], f"{what} top_k {top_k} query {i}: ids"
            assert list(sc[i]) == [float(ms[j]) for j in order], f"{what} top_k {top_k} query {i}: scores"
        out.append((ids, sc, cnt))
    return out


def _same_store(a, b, what):
    assert a.token_store == b.token_store == "fp8" and a.n_docs == b.n_docs
    assert torch.equal(a.tokens, b.tokens), f"{what}: tokens differ from a fresh build"
    assert torch.equal(a.token_scales, b.token_scales), f"{what}: token_scales differ from a fresh build"


def test_index_rerank_append_delete(T, corpus):
    """set_tokens(store="fp8"), then append, delete and delete -> append: ``tokens`` and ``token_scales`` stay
    byte-equal to a fresh build over the same rows, and the rerank leg answers as the oracle does."""
    C = corpus
    n, n0 = C["n"], 2400
    idx = _build(T, C, np.arange(n0))
    assert idx.tokens_packed and idx.token_store == "fp8"
    _check_rerank(T, idx, C, np.arange(n0), "fresh")
    # the float16 store over the same (exact) tokens gives the same scores
    ids = dev(np.tile(np.arange(50, dtype=np.int64), (len(C["q"]), 1)))
    f16 = T.GpuIndex().set_tokens(C["dtok"][:n0])
    assert torch.equal(idx.maxsim(dev(C["qtok"]), ids), f16.maxsim(dev(C["qtok"]), ids))
    # append
    sel = C["doc"] >= n0
    idx.append_rows(C["x"][n0:], lex=(C["doc"][sel] - n0, C["term"][sel], C["tf"][sel], C["v"]), tokens=C["dtok"][n0:])
    _same_store(idx, _build(T, C, np.arange(n)), "append")
    _check_rerank(T, idx, C, np.arange(n), "append")
    # delete: a run, scattered rows, the last row
    rng = np.random.default_rng(5)
    gone = np.unique(np.concatenate([np.arange(1024, 1100), rng.choice(n, 200, replace=False), [n - 1, n0, n0 - 1]]))
    idx.delete_rows(gone)
    keep = np.setdiff1d(np.arange(n), gone)
    _same_store(idx, _build(T, C, keep), "delete")
    _check_rerank(T, idx, C, keep, "delete")
    # delete -> append: the deleted rows come back at the end
    back = gone[:100]
    rows = np.concatenate([keep, back])
    # (lexical rows of the batch, local ids)
    pos = np.full(n, -1, dtype=np.int64)
    pos[back] = np.arange(len(back))
    sel = pos[C["doc"]] >= 0
    idx.append_rows(C["x"][back], lex=(pos[C["doc"][sel]].astype(np.int32), C["term"][sel], C["tf"][sel], C["v"]),
                    tokens=C["dtok"][back])
    fresh = T.GpuIndex().set_tokens(C["dtok"][rows], store="fp8")
    assert torch.equal(idx.tokens, fresh.tokens) and torch.equal(idx.token_scales, fresh.token_scales)
    assert idx.n_docs == len(rows)
    _check_rerank(T, idx, C, rows, "delete -> append")
    # real-valued tokens too: quantisation is per token, so a mutated store is a fresh build's, byte for byte
    real = MC.real_tokens("normal", rng, 300, 32, 64, queries=False)
    a = T.GpuIndex().set_dense(C["x"][:200]).set_tokens(real[:200], store="fp8")
    a.append_rows(C["x"][200:300], tokens=real[200:])
    a.delete_rows(np.arange(50, 120))
    keep = np.setdiff1d(np.arange(300), np.arange(50, 120))
    b = T.GpuIndex().set_tokens(real[keep], store="fp8")
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.token_scales, b.token_scales)
    # reserve_rows keeps both arrays' logical size and gives both room
    a.reserve_rows(1000)
    assert a.capacity_rows() >= 1000 and tuple(a.token_scales.shape) == (len(keep), 32)
    assert torch.equal(a.tokens, b.tokens) and torch.equal(a.token_scales, b.token_scales)


def test_index_save_load(T, corpus, tmp_path, monkeypatch):
    """save(hi, path, gpu_index=) writes the image and the scales; load().to_gpu(token_store="fp8") takes them
    as they are -- with the float16 source and without it -- same bytes, same answers."""
    from triple_hybrid_rag_amd import index_build as IB
    C, N = corpus, T._native
    n = 500
    hi = IB.HostIndex(docs=C["x"][:n], tokens=C["dtok"][:n].copy())
    g = hi.to_gpu(token_store="fp8")                        # quantised from hi.tokens: there is no image yet
    assert g.token_store == "fp8" and hi.fp8_image() is None
    assert torch.equal(g.tokens, N.maxsim_quantize_fp8(dev(C["dtok"][:n]))[0])
    ids = dev(np.tile(np.arange(60, dtype=np.int64), (len(C["q"]), 1)))
    want = g.maxsim(dev(C["qtok"]), ids)
    assert hi.to_gpu().token_store == "f16"                 # the default stays float16
    IB.save(hi, str(tmp_path / "with"), g)
    hi.tokens = None
    IB.save(hi, str(tmp_path / "without"), g)
    assert not os.path.exists(tmp_path / "without" / "tokens.npy")

    def refuse(*a, **k):
        raise AssertionError("to_gpu requantised although the saved image was there")
    monkeypatch.setattr(N, "maxsim_quantize_fp8", refuse)
    for name in ("with", "without"):
        back = IB.load(str(tmp_path / name))
        assert (back.tokens is None) == (name == "without") and back.fp8_image() is not None
        g2 = back.to_gpu(token_store="fp8")
        assert g2.token_store == "fp8" and g2.tokens_packed
        assert torch.equal(g2.tokens, g.tokens) and torch.equal(g2.token_scales, g.token_scales), name
        assert torch.equal(g2.maxsim(dev(C["qtok"]), ids), want), name
    back = IB.load(str(tmp_path / "with"))
    assert back.to_gpu().token_store == "f16" and back.to_gpu().tokens.dtype == torch.float16
    monkeypatch.undo()
    # after a mutation the FP8 store cannot be pulled back, as the packed float16 store cannot
    hi = IB.HostIndex(docs=C["x"][:n], tokens=C["dtok"][:n].copy())
    g = hi.to_gpu(token_store="fp8")
    g.append_rows(C["x"][n:n + 10], tokens=C["dtok"][n:n + 10])
    with pytest.raises(ValueError, match="cannot be pulled back"):
        IB.refresh_from_gpu(hi, g)


def test_tok_dim_16_is_refused_where_the_tokens_enter(T, corpus):
    """16 is a float16 store's dim only: refused at set_tokens, at append_rows and at to_gpu, with the list in
    the message and the index as it was."""
    from triple_hybrid_rag_amd import index_build as IB
    N, C = T._native, corpus
    tok16 = np.zeros((40, 32, 16), dtype=np.float16)
    msg = r"tok_dim 16 .*\[32, 64, 96, 128, 192, 256\]"
    idx = T.GpuIndex()
    with pytest.raises(N.NativeError, match=msg):
        idx.set_tokens(tok16, store="fp8")
    with pytest.raises(N.NativeError, match=msg):
        idx.set_tokens(dev(tok16), store="fp8")
    assert idx.tokens is None and idx.token_scales is None and idx.token_store == "f16"
    with pytest.raises(N.NativeError, match=msg):
        N.maxsim_quantize_fp8(dev(tok16))
    assert idx.set_tokens(tok16).token_store == "f16"        # the float16 store takes it
    with pytest.raises(N.NativeError, match=msg):
        IB.HostIndex(docs=C["x"][:40], tokens=tok16).to_gpu(token_store="fp8")
    # append_rows: an FP8 index whose store came past set_tokens refuses the append before anything is stored
    idx = T.GpuIndex().set_dense(C["x"][:40]).set_tokens(C["dtok"][:40], store="fp8")
    good = idx.tokens
    idx.tokens = torch.zeros((40, 32, 16), dtype=torch.uint8, device="cuda")
    with pytest.raises(N.NativeError, match="append_rows: tokens: " + msg):
        idx.append_rows(C["x"][40:50], tokens=np.zeros((10, 32, 16), dtype=np.float16))
    idx.tokens = good
    assert idx.n_docs == 40 and tuple(idx.token_scales.shape) == (40, 32)
    # the library itself, should a caller come past the wrappers: nothing launched
    out = torch.full((40, 32), 7.0, dtype=torch.float32, device="cuda")
    t = dev(tok16)
    assert N.load().thr_maxsim_quantize_fp8(t.data_ptr(), 40, 32, 16, torch.empty((40, 32, 16), dtype=torch.uint8, device="cuda").data_ptr(),
                                            out.data_ptr(), None) == -2
    torch.cuda.synchronize()
    assert torch.all(out == 7.0)
