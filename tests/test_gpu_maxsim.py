"""MaxSim rerank on the GPU against float64: every kernel instantiation (tok_dim / 16 in
{1, 2, 4, 6, 8, 12, 16}, packed and row-major, local indices and global ids), the edges of the
grid, the float16 range, more queries than gridDim.y holds, thr_maxsim_pack on its own, and the
rerank step of retrieve_batch end to end.

The reference of every case is oracle.thr_oracle.maxsim_scores (float64 numpy).  Exact-family
inputs (tests/maxsim_cases.py) are compared with np.array_equal -- no tolerance; real-valued inputs
are held to the float32 forward-error bound computed from the inputs, and to BASELINE's 1e-4
absolute at the 128 x 128 unit-norm shape.  The packed-versus-row-major bit equality is an extra
assertion, never the ground truth.  Each real-valued case prints its largest error / bound (run
with -s); DESIGN.md "MaxSim rerank" records them."""
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

LAYOUTS = ("rowmajor", "packed")
Q_TOKENS = (32, 64, 96, 128)
D_TOKENS = (32, 64, 96, 160, 512)
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


def shapes_for(tok_dim):
    """The thinned cross of q_tokens x d_tokens for one tok_dim: the single-tile corner, every
    q_tokens and every d_tokens at least once, a multi-tile q_tokens against a multi-tile d_tokens
    (several), rotated by tok_dim so that over the seven dims every pair of the cross is met."""
    r = MC.TOK_DIMS.index(tok_dim)
    out = [(32, 32), (128, 512)]
    for a, qt in enumerate(Q_TOKENS):
        for b, dt in enumerate(D_TOKENS):
            if (a + 2 * b + r) % 3 == 0 and (qt, dt) not in out:
                out.append((qt, dt))
    assert {q for q, _ in out} == set(Q_TOKENS) and {d for _, d in out} == set(D_TOKENS)
    assert any(q > 32 and d > 32 for q, d in out)
    return out


def test_the_thinned_cross_meets_every_pair():
    met = {s for td in MC.TOK_DIMS for s in shapes_for(td)}
    assert met == {(q, d) for q in Q_TOKENS for d in D_TOKENS}


def scores(T, qtok, dtok, cand, layout, ids=False, id_base=ID_BASE, store=None):
    """One device call -> float64 numpy.  ids=True: thr_maxsim_ids with cand as global ids."""
    N = T._native
    packed = layout == "packed"
    if store is None:
        store = N.maxsim_pack(dev(dtok)) if packed else dev(dtok)
    if ids:
        out = N.maxsim_ids(dev(qtok), store, dev(np.asarray(cand, dtype=np.int64)), id_base, packed=packed)
    else:
        out = N.maxsim(dev(qtok), store, dev(np.asarray(cand, dtype=np.int32)), packed=packed)
    assert out.dtype == torch.float32 and tuple(out.shape) == tuple(np.shape(cand))
    return out.cpu().numpy().astype(np.float64)


def both_entry_points(T, qtok, dtok, cand, layout):
    """(thr_maxsim on local indices, thr_maxsim_ids on the same candidates as global ids)."""
    cand = np.asarray(cand)
    N = T._native
    store = N.maxsim_pack(dev(dtok)) if layout == "packed" else dev(dtok)
    gids = np.where(cand >= 0, cand.astype(np.int64) + ID_BASE, -1)
    return (scores(T, qtok, dtok, cand, layout, store=store),
            scores(T, qtok, dtok, gids, layout, ids=True, store=store))


def assert_exact(got, ref, what):
    assert np.array_equal(got, ref), \
        f"{what}: {int((got != ref).sum())} of {ref.size} scores differ, first at " \
        f"{tuple(np.argwhere(got != ref)[0])}: got {got[got != ref][0]!r}, reference {ref[got != ref][0]!r}"


@functools.lru_cache(maxsize=None)
def exact_case(tok_dim, qt, dt):
    rng = np.random.default_rng(1000 * tok_dim + qt + dt)
    n_docs, nq, n_cand = 11, 3, 9
    q = MC.exact_tokens(rng, (nq, qt, tok_dim))
    d = MC.exact_tokens(rng, (n_docs, dt, tok_dim))
    d[1] = -np.abs(d[1]) - np.float16(0.125)             # one doc whose products with q[0] are all negative
    q[0] = np.abs(q[0]) + np.float16(0.125)
    d[1] = np.maximum(d[1], np.float16(-1))
    q[0] = np.minimum(q[0], np.float16(1))
    cand = rng.integers(0, n_docs, (nq, n_cand)).astype(np.int32)
    cand[0, 0], cand[2, 4] = 1, -1
    return q, d, cand, MC.reference(q, d, cand)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tok_dim", MC.TOK_DIMS, ids=lambda td: f"td{td}")
def test_every_instantiation_exact(T, tok_dim, layout):
    """Exact family: the device returns the bits of the float64 reference."""
    for qt, dt in shapes_for(tok_dim):
        q, d, cand, ref = exact_case(tok_dim, qt, dt)
        assert ref[0, 0] < 0 and ref[2, 4] == -np.inf
        for got, name in zip(both_entry_points(T, q, d, cand, layout), ("thr_maxsim", "thr_maxsim_ids")):
            assert_exact(got, ref, f"{name} td{tok_dim} {qt}x{dt} {layout}")


@functools.lru_cache(maxsize=None)
def real_case(family, tok_dim, qt, dt):
    rng = np.random.default_rng(77 * tok_dim + qt + dt)
    n_docs, nq, n_cand = 11, 3, 9
    q = MC.real_tokens(family, rng, nq, qt, tok_dim, True)
    d = MC.real_tokens(family, rng, n_docs, dt, tok_dim, False)
    cand = rng.integers(0, n_docs, (nq, n_cand)).astype(np.int32)
    cand[1, 7] = -1
    return q, d, cand, MC.reference(q, d, cand), MC.error_bound(q, d, cand)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("family", ["unit", "normal"])
@pytest.mark.parametrize("tok_dim", MC.TOK_DIMS, ids=lambda td: f"td{td}")
def test_every_instantiation_real_valued(T, tok_dim, family, layout):
    """Real-valued tokens: |got - reference| <= the float32 forward-error bound of each score."""
    for qt, dt in shapes_for(tok_dim):
        q, d, cand, ref, bound = real_case(family, tok_dim, qt, dt)
        ok = np.isfinite(ref)
        assert ok.sum() == ref.size - 1 and np.all(bound[ok] > 0)
        got_l, got_g = both_entry_points(T, q, d, cand, layout)
        assert np.array_equal(got_l, got_g)                      # the same kernel, the same arithmetic
        assert np.array_equal(got_l[~ok], ref[~ok])
        err = np.abs(got_l[ok] - ref[ok])
        print(f"maxsim error/bound {family} td{tok_dim} {qt}x{dt} {layout}: max |err| {err.max():.3e} "
              f"bound {bound[ok].min():.3e} max err/bound {np.max(err / bound[ok]):.4f}")
        assert np.all(err <= bound[ok]), (family, tok_dim, qt, dt, layout, float(np.max(err / bound[ok])))
        if layout == "packed":    # extra: the packed image changes where bytes lie, not what is computed
            assert np.array_equal(got_l, scores(T, q, d, cand, "rowmajor"))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_north_star_shape_within_1e_4(T, layout):
    """BASELINE's bar: 128 doc tokens x 128 dims, unit-norm tokens, 1e-4 absolute (scores <= 32)."""
    from triple_hybrid_rag_amd import synth
    dt = synth.doc_tokens(0, 300, 128, 128)
    rng = np.random.default_rng(3)
    for q_tokens, n_cand in ((32, 100), (128, 17)):
        qt = synth.query_tokens(6, q_tokens, 128)
        cand = rng.integers(0, 300, size=(6, n_cand)).astype(np.int32)
        cand[0, 5] = -1
        ref = MC.reference(qt, dt, cand)
        ok = np.isfinite(ref)
        got_l, got_g = both_entry_points(T, qt, dt, cand, layout)
        assert np.array_equal(got_l, got_g) and np.array_equal(got_l[~ok], ref[~ok])
        err = np.abs(got_l[ok] - ref[ok])
        print(f"maxsim north star q{q_tokens} {layout}: max |err| {err.max():.3e}, "
              f"max err/bound {np.max(err / MC.error_bound(qt, dt, cand)[ok]):.4f}")
        assert err.max() < 1e-4
        assert np.all(err <= MC.error_bound(qt, dt, cand)[ok])


# ------------------------------------------------------------------ planted positions (exact family)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tok_dim", (16, 128), ids=lambda td: f"td{td}")
def test_planted_doc_token(T, tok_dim, layout):
    """Doc j of 128: token j alone is the maximum for every query token, every other product is
    strictly negative -- and in the odd docs the planted product is negative too, so a running
    maximum started at 0, or a tile of zero padding, changes the answer."""
    rng = np.random.default_rng(tok_dim)
    n = 128
    q = MC.exact_tokens(rng, (2, 64, tok_dim), 1, 8)                       # all positive
    d = -MC.exact_tokens(rng, (n, n, tok_dim), 4, 8)                      # all <= -1/2: dots <= -tok_dim / 16
    for j in range(n):
        d[j, j] = 0
        if j % 2:
            d[j, j, (5 * j) % tok_dim] = -0.125                            # dot in [-1/8, -1/64]: still the maximum
        else:
            d[j, j] = MC.exact_tokens(rng, (tok_dim,), 0, 8)
            d[j, j, j % tok_dim] = 1.0
    cand = np.stack([np.arange(n), rng.permutation(n)]).astype(np.int32)
    ref = MC.reference(q, d, cand)
    s = np.einsum("qik,djk->qdij", q.astype(np.float64), d.astype(np.float64))
    assert np.all(s.argmax(axis=3) == np.arange(n)[None, :, None])         # the planted token wins everywhere
    others = np.where(np.eye(n, dtype=bool)[None, :, None, :], -np.inf, s)
    assert others.max() < -0.5 and np.all(ref[0, 1::2] < 0) and np.all(ref[0, ::2] > 0)
    for got, name in zip(both_entry_points(T, q, d, cand, layout), ("thr_maxsim", "thr_maxsim_ids")):
        assert_exact(got, ref, f"planted doc token, {name} td{tok_dim} {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tok_dim", (32, 192), ids=lambda td: f"td{td}")
def test_planted_query_token(T, tok_dim, layout):
    """Query i of 128 is zero except at token i: a query token that is dropped, read twice or
    read from another query's rows shows in exactly that query."""
    rng = np.random.default_rng(tok_dim + 1)
    n = 128
    q = np.zeros((n, n, tok_dim), dtype=np.float16)
    q[np.arange(n), np.arange(n)] = MC.exact_tokens(rng, (n, tok_dim))
    d = MC.exact_tokens(rng, (6, 96, tok_dim))
    d[5] = -np.abs(d[5])
    cand = rng.integers(0, 6, (n, 5)).astype(np.int32)
    ref = MC.reference(q, d, cand)
    assert len(np.unique(ref)) > 20
    for got, name in zip(both_entry_points(T, q, d, cand, layout), ("thr_maxsim", "thr_maxsim_ids")):
        assert_exact(got, ref, f"planted query token, {name} td{tok_dim} {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("tok_dim", MC.TOK_DIMS, ids=lambda td: f"td{td}")
def test_planted_dimension(T, tok_dim, layout):
    """Doc k has every token one-hot at dimension k; the query's weights are distinct per
    dimension ((k + 1) / 256, signs alternating: one product per dot, so still exact) and every
    doc's score is different.  A lane map or a packed image that puts dimension k anywhere else
    gives doc k another doc's score."""
    qt, dt = 64, 64
    i, k = np.arange(qt)[:, None], np.arange(tok_dim)[None, :]
    w = (k + 1) / 256.0 * np.where((i + k) % 2, -1.0, 1.0)
    q = np.stack([w, -w[::-1]]).astype(np.float16)
    assert np.array_equal(q.astype(np.float64), np.stack([w, -w[::-1]]))
    d = np.zeros((tok_dim, dt, tok_dim), dtype=np.float16)
    v = (1 + np.arange(dt) % 8) / 8.0 * np.where(np.arange(dt) % 8 < 3, -1.0, 1.0)      # max 1, min -3/8
    for kk in range(tok_dim):
        d[kk, :, kk] = np.roll(v, kk)
    cand = np.stack([np.arange(tok_dim), np.arange(tok_dim)[::-1]]).astype(np.int32)
    ref = MC.reference(q, d, cand)
    assert np.array_equal(ref[0], (np.arange(tok_dim) + 1) / 256.0 * (32 + 32 * 0.375)) and np.array_equal(ref[1], ref[0][::-1])
    for got, name in zip(both_entry_points(T, q, d, cand, layout), ("thr_maxsim", "thr_maxsim_ids")):
        assert_exact(got, ref, f"planted dimension, {name} td{tok_dim} {layout}")


# ------------------------------------------------------------------ grid edges
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("n_queries", (1, 3))
@pytest.mark.parametrize("n_cand", (1, 2, 3, 4, 5, 257))
def test_grid_edges(T, n_cand, n_queries, layout):
    """The tail of the four-waves-per-block split, candidates repeated within a row, and the
    candidates that owe -inf (-1, n_docs, id_base - 1, id_base + n_docs) with their neighbours
    untouched."""
    rng = np.random.default_rng(10 * n_cand + n_queries)
    n_docs, qt, dt, td = 9, 64, 96, 64
    q = MC.exact_tokens(rng, (n_queries, qt, td))
    d = MC.exact_tokens(rng, (n_docs, dt, td))
    d[3] = -np.abs(d[3]) - np.float16(0.125)
    q[0] = np.abs(q[0])
    cand = rng.integers(0, n_docs, (n_queries, n_cand)).astype(np.int32)
    cand[:, n_cand // 2:] = cand[:, : n_cand - n_cand // 2]                # repeats within the row
    for bad_local, bad_global in ((None, None), (-1, -1), (n_docs, ID_BASE + n_docs), (-1, ID_BASE - 1),
                                  (2 ** 31 - 1, 2 ** 62), (-(2 ** 31), -(2 ** 62))):
        loc, gid = cand.copy(), cand.astype(np.int64) + ID_BASE
        if bad_local is not None:
            for p in sorted({0, n_cand - 1, n_cand // 2, min(3, n_cand - 1)}):
                if n_cand == 1 or p != 1:                                   # slot 1 stays a live neighbour
                    loc[n_queries - 1, p], gid[n_queries - 1, p] = bad_local, bad_global
        ref = MC.reference(q, d, loc)
        assert np.array_equal(ref, MC.reference(q, d, gid, id_base=ID_BASE))
        assert bad_local is None or np.isneginf(ref[n_queries - 1, 0])
        assert_exact(scores(T, q, d, loc, layout), ref, f"thr_maxsim n_cand {n_cand} nq {n_queries} bad {bad_local}")
        assert_exact(scores(T, q, d, gid, layout, ids=True), ref,
                     f"thr_maxsim_ids n_cand {n_cand} nq {n_queries} bad {bad_global}")
    # a row that belongs to another shard entirely, between two that do not
    gid = cand.astype(np.int64) + ID_BASE
    gid[n_queries // 2] = rng.integers(ID_BASE + n_docs, ID_BASE + 10 * n_docs, n_cand)
    ref = MC.reference(q, d, gid, id_base=ID_BASE)
    assert np.all(np.isneginf(ref[n_queries // 2]))
    assert_exact(scores(T, q, d, gid, layout, ids=True), ref, "a row of another shard")
    # id_base 0 and a large one
    for base in (0, 2 ** 40):
        gid = cand.astype(np.int64) + base
        assert_exact(scores(T, q, d, gid, layout, ids=True, id_base=base), MC.reference(q, d, cand),
                     f"id_base {base}")


# ------------------------------------------------------------------ float16 range (exact family)
@pytest.mark.parametrize("layout", LAYOUTS)
def test_float16_extremes(T, layout):
    """Tokens at +-65504: each query token is one-hot, so a dot is one product, +-65504^2 =
    +-2047^2 * 2^10 (23 bits: exact in float32), and four such query tokens keep the sum below
    2^24 * 2^10.  The expected result is the exact one."""
    rng = np.random.default_rng(9)
    big = np.float16(65504.0)
    td, qt, dt, nq, n_docs = 64, 32, 64, 5, 7
    d = (rng.integers(-1, 2, (n_docs, dt, td)) * 65504.0).astype(np.float16)
    d[6] = -np.abs(d[6])
    d[6, :, ::2] = -big
    q = np.zeros((nq, qt, td), dtype=np.float16)
    for qi in range(nq):
        for t in rng.choice(qt, 4, replace=False):
            q[qi, t, rng.integers(0, td)] = big if (qi + t) % 3 else -big
    q[4] = 0
    q[4, 31, 0], q[4, 0, 2] = big, big                                     # against doc 6: -65504^2 twice
    cand = np.tile(np.arange(n_docs, dtype=np.int32), (nq, 1))
    ref = MC.reference(q, d, cand)
    assert np.all(np.isfinite(ref)) and np.abs(ref).max() >= 2 * 65504.0 ** 2 and ref[4, 6] == -2 * 65504.0 ** 2
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    for got, name in zip(both_entry_points(T, q, d, cand, layout), ("thr_maxsim", "thr_maxsim_ids")):
        assert_exact(got, ref, f"+-65504, {name} {layout}")


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("side", ("docs", "queries"))
def test_float16_subnormals_are_not_flushed(T, side, layout):
    """Subnormal float16 tokens (m * 2^-24, |m| < 128) on one side against multiples of 1/8 on the
    other: products are multiples of 2^-27 and every sum stays an integer number of them below
    8 * 127 * 96 * 64 < 2^24, so the exact result is owed -- a matrix core that flushed subnormal inputs would return 0 (or, for
    the all-negative doc, a different maximum)."""
    rng = np.random.default_rng(12)
    td, qt, dt = 96, 64, 64
    sub = (rng.integers(-127, 128, (5, dt, td)) * 2.0 ** -24).astype(np.float16)
    assert np.all(np.abs(sub.astype(np.float64)) < 2.0 ** -14) and np.count_nonzero(sub) > sub.size * 0.99
    sub[4] = -np.abs(sub[4])
    sub[3] = 0
    sub[3, 17, 5] = 2.0 ** -20                                             # 2^-20 against 1.0
    other = MC.exact_tokens(rng, (3, qt, td))
    other[2] = 0
    other[2, :, 5] = 1.0
    q, d = (other, sub) if side == "docs" else (sub[:, :qt], other)
    cand = np.tile(np.arange(d.shape[0], dtype=np.int32), (q.shape[0], 1))
    ref = MC.reference(q, d, cand)
    assert np.count_nonzero(ref) >= ref.size - 2 and np.abs(ref).max() < 2.0 ** -3
    if side == "docs":
        assert ref[2, 3] == qt * 2.0 ** -20
    assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref)
    for got, name in zip(both_entry_points(T, q, d, cand, layout), ("thr_maxsim", "thr_maxsim_ids")):
        assert_exact(got, ref, f"subnormal {side}, {name} {layout}")


# ------------------------------------------------------------------ more queries than gridDim.y holds
@pytest.mark.parametrize("layout", LAYOUTS)
def test_many_queries_in_one_call(T, layout):
    """65 600 queries in one call (queries sit on gridDim.y; the launch goes out in slices of at
    most the device's limit), smallest shape, exact family.  Query q is pool[q % 257] -- 257 is
    prime, so a slice that started at the wrong row of qtok, cand or out would not line up --
    and the reference is float64 over the distinct (query, doc) pairs."""
    rng = np.random.default_rng(65600)
    nq, pool_n, n_docs, td, n_cand = 65600, 257, 13, 16, 3
    pool = MC.exact_tokens(rng, (pool_n, 32, td))
    d = MC.exact_tokens(rng, (n_docs, 32, td))
    table = MC.reference(pool, d, np.tile(np.arange(n_docs), (pool_n, 1)))      # [pool, doc]
    assert len(np.unique(table)) > 100
    which = np.arange(nq) % pool_n
    q = pool[which]
    assert q.nbytes == nq * 32 * td * 2
    cand = rng.integers(0, n_docs, (nq, n_cand)).astype(np.int32)
    cand[rng.integers(0, nq, 500), rng.integers(0, n_cand, 500)] = -1
    cand[-1, -1], cand[65535, 0], cand[65536, 1] = -1, -1, -1
    ref = np.where(cand >= 0, table[which[:, None], np.maximum(cand, 0)], -np.inf)
    N = T._native
    qd, store = dev(q), (N.maxsim_pack(dev(d)) if layout == "packed" else dev(d))
    got = N.maxsim(qd, store, dev(cand), packed=layout == "packed").cpu().numpy().astype(np.float64)
    assert_exact(got, ref, f"thr_maxsim, 65 600 queries {layout}")
    gids = np.where(cand >= 0, cand.astype(np.int64) + ID_BASE, -1)
    got = N.maxsim_ids(qd, store, dev(gids), ID_BASE, packed=layout == "packed").cpu().numpy().astype(np.float64)
    assert_exact(got, ref, f"thr_maxsim_ids, 65 600 queries {layout}")


# ------------------------------------------------------------------ thr_maxsim_pack on its own
@pytest.mark.parametrize("tok_dim", MC.TOK_DIMS, ids=lambda td: f"td{td}")
def test_pack_is_the_fragment_major_image(T, tok_dim):
    """thr_maxsim_pack against the numpy restatement of [doc][tile][k-step][lane][8 halves],
    bit for bit, on tokens that are all different bit patterns where the shape allows."""
    rng = np.random.default_rng(tok_dim)
    for n, dt in ((1, 32), (5, 96), (3, 512)):
        bits = rng.permutation(n * dt * tok_dim).astype(np.uint64) * 7 + 3
        tok = (bits % 65536).astype(np.uint16).reshape(n, dt, tok_dim)
        got = T._native.maxsim_pack(torch.from_numpy(tok.view(np.float16)).cuda())
        assert got.dtype == torch.float16 and tuple(got.shape) == (n, dt, tok_dim)
        got = got.cpu().numpy().view(np.uint16)
        exp = MC.pack_reference(tok)
        assert np.array_equal(got, exp), (tok_dim, n, dt, int((got != exp).sum()))


# ------------------------------------------------------------------ unsupported shapes
def test_unsupported_tok_dim_is_refused_where_the_tokens_enter(T):
    """48, 80, ... have no kernel: refused by the pack, by both scorers, by set_tokens (packed or
    not) and by the token leg of append_rows -- with the supported dims in the message and the
    index as it was -- not at the first query."""
    N = T._native
    for td in (48, 80, 112, 144, 160, 176, 208, 224, 240, 272):
        tok = torch.zeros((4, 32, td), dtype=torch.float16, device="cuda")
        q = torch.zeros((1, 32, td), dtype=torch.float16, device="cuda")
        c32 = torch.zeros((1, 2), dtype=torch.int32, device="cuda")
        for call in (lambda: N.maxsim_pack(tok), lambda: N.maxsim(q, tok, c32), lambda: N.maxsim(q, tok, c32, packed=True),
                     lambda: N.maxsim_ids(q, tok, c32.long(), 0), lambda: T.GpuIndex().set_tokens(tok),
                     lambda: T.GpuIndex().set_tokens(tok, pack=False)):
            with pytest.raises(N.NativeError, match=r"tok_dim %d.*\[16, 32, 64, 96, 128, 192, 256\]" % td):
                call()
        # the library itself, should a caller come past the wrappers: the same answer, nothing launched
        out = torch.full((1, 2), 7.0, dtype=torch.float32, device="cuda")
        lib = N.load()
        assert lib.thr_maxsim_pack(tok.data_ptr(), 4, 32, td, torch.empty_like(tok).data_ptr(), None) == -2
        assert lib.thr_maxsim(q.data_ptr(), 1, 32, tok.data_ptr(), 4, 32, td, c32.data_ptr(), 2, out.data_ptr(), 0, None) == -2
        torch.cuda.synchronize()
        assert out.tolist() == [[7.0, 7.0]]
    idx = T.GpuIndex()
    with pytest.raises(N.NativeError):
        idx.set_tokens(torch.zeros((4, 32, 48), dtype=torch.float16, device="cuda"), pack=False)
    assert idx.tokens is None
    # append_rows: an index whose store came past set_tokens refuses the append before anything is stored
    rng = np.random.default_rng(1)
    x = rng.standard_normal((600, 768)).astype(np.float32)
    idx = T.GpuIndex().set_dense(x[:500]).set_tokens(MC.exact_tokens(rng, (500, 32, 64)), pack=False)
    good = idx.tokens
    idx.tokens = torch.zeros((500, 32, 48), dtype=torch.float16, device="cuda")
    with pytest.raises(N.NativeError, match=r"tok_dim 48.*\[16, 32, 64, 96, 128, 192, 256\]"):
        idx.append_rows(x[500:], tokens=np.zeros((100, 32, 48), dtype=np.float16))
    assert idx.n_docs == 500 and idx.docs.shape[0] == 500 and tuple(idx.tokens.shape) == (500, 32, 48)
    idx.tokens = good
    with pytest.raises(N.NativeError, match="tokens must be"):
        idx.append_rows(x[500:], tokens=np.zeros((100, 32, 48), dtype=np.float16))
    assert idx.n_docs == 500
    assert list(idx.append_rows(x[500:], tokens=MC.exact_tokens(rng, (100, 32, 64)))) == list(range(500, 600))
    assert idx.n_docs == 600 and tuple(idx.tokens.shape) == (600, 32, 64)


# ------------------------------------------------------------------ the rerank step end to end
def _lex_rows(rng, n, v, per=12):
    term = np.minimum((v * rng.random((n, per)) ** 3).astype(np.int32), v - 1).reshape(-1)
    doc = np.repeat(np.arange(n, dtype=np.int32), per)
    tf = rng.geometric(0.5, n * per).astype(np.int32)
    return doc, term, tf


def _men_csr(me, mc, mw, n_ent):
    order = np.lexsort((mc, me))
    rp = np.concatenate([[0], np.cumsum(np.bincount(me, minlength=n_ent))]).astype(np.int64)
    return rp, mc[order].astype(np.int32), mw[order]


def _check_rerank_against_oracle(T, idx, x, dtok, q, qt, seeds, qtok, what):
    """retrieve_batch(qtok=, rerank_top_k=100) at top_k 10 and 100 against the oracle pipeline over
    the rows the index now holds: fused top-100 -> float64 MaxSim -> O.rerank_order (stable:
    ties keep the fused order).  Ids, float64 scores and counts, every query."""
    n = idx.n_docs
    assert n == len(x) == len(dtok)
    L, G = idx.lex, idx.graph
    rowptr, pd, ptf, dl, idf = (L[k].cpu().numpy() for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"))
    graph = [G[k].cpu().numpy() for k in ("ent_rowptr", "ent_col", "men_rowptr", "men_chunk", "men_conf")]
    _, Id, _ = CO.dense_topk_exact(x, q, 100)
    _, Il = O.bm25_topk(rowptr, pd, ptf, dl, idf, L["avgdl"], qt, n, 50)
    _, Ig = O.graph_topk(*graph, seeds, 2, n, 50)
    tied = 0
    for top_k in (10, 100):
        res = idx.retrieve_batch(dev(q), dev(qt), dev(seeds), top_k=top_k, qtok=dev(qtok), rerank_top_k=100)
        ids, sc, cnt = res.ids.cpu().numpy(), res.scores.cpu().numpy(), res.counts.cpu().numpy()
        assert sc.dtype == np.float64 and ids.shape == (len(q), top_k)
        for i in range(len(q)):
            f100, _ = O.fused_topk_ids(list(Il[i]), list(Id[i]), list(Ig[i]), 100)
            assert len(f100) == 100
            ms = MC.reference(qtok[i:i + 1], dtok, np.array([f100], dtype=np.int64))[0]
            order = O.rerank_order(list(ms))[:top_k]
            tied += len(set(ms[order])) < len(order)
            assert int(cnt[i]) == len(order), f"{what} top_k {top_k} query {i}: count"
            assert list(ids[i]) == [f100[j] for j in order], f"{what} top_k {top_k} query {i}: ids"
            assert list(sc[i]) == [float(ms[j]) for j in order], f"{what} top_k {top_k} query {i}: scores"
    assert tied >= len(q) // 2, "the case is meant to hold real ties"


@pytest.mark.parametrize("pack", (True, False), ids=("packed", "rowmajor"))
def test_rerank_pipeline_exact(T, pack):
    """A small triple-hybrid index with exact-family tokens: MaxSim scores are exact, ties between
    them are real (docs share token matrices), and retrieve_batch must return O.rerank_order of
    the float64 scores over the oracle's fused top-100 -- ids, scores, ties in fused order.
    Then again after an append_rows and a delete_rows that carry tokens."""
    rng = np.random.default_rng(31)
    n, n0, d, v, n_ent, nq = 7000, 5600, 768, 1500, 3000, 24
    x = rng.standard_normal((n, d)).astype(np.float32)
    x *= rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)
    doc, term, tf = _lex_rows(rng, n, v)
    deg = rng.integers(1, 6, n_ent)
    ent_rowptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.int64)
    ent_col = rng.integers(0, n_ent, ent_rowptr[-1]).astype(np.int32)
    me = rng.integers(0, n_ent, n * 2).astype(np.int64)
    mc = rng.integers(0, n, n * 2).astype(np.int64)
    mw = rng.uniform(0.5, 1.0, n * 2).astype(np.float32)
    pool = MC.exact_tokens(rng, (211, 32, 64))
    dtok = pool[rng.integers(0, 211, n)]                      # docs share token matrices: exact ties
    qtok = MC.exact_tokens(rng, (nq, 32, 64))
    q = x[rng.integers(0, n, nq)] + 0.3 * rng.standard_normal((nq, d)).astype(np.float32)
    qt = rng.integers(0, v, (nq, 4)).astype(np.int32)
    seeds = rng.integers(0, n_ent, (nq, 3)).astype(np.int32)

    sel, msel = doc < n0, mc < n0
    rp, c, w = _men_csr(me[msel], mc[msel], mw[msel], n_ent)
    idx = T.GpuIndex().set_dense(x[:n0])
    idx.set_lexical_rows(doc[sel], term[sel], tf[sel], v, n_docs=n0)
    idx.set_graph(ent_rowptr, ent_col, rp, c, w).set_tokens(dtok[:n0], pack=pack)
    assert idx.tokens_packed == pack
    _check_rerank_against_oracle(T, idx, x[:n0], dtok[:n0], q, qt, seeds, qtok, "fresh")
    # append rows [n0, n), delete a run and scattered rows (old and appended): tokens travel with both
    sel, msel = doc >= n0, mc >= n0
    idx.append_rows(x[n0:], lex=(doc[sel] - n0, term[sel], tf[sel], v), tokens=dtok[n0:],
                    mentions=(me[msel], mc[msel] - n0, mw[msel]))
    gone = np.unique(np.concatenate([np.arange(1024, 1100), rng.choice(n, 300, replace=False), [n - 1, n0, n0 - 1]]))
    idx.delete_rows(gone)
    keep = np.ones(n, dtype=bool)
    keep[gone] = False
    assert idx.n_docs == int(keep.sum()) and idx.tokens_packed == pack
    _check_rerank_against_oracle(T, idx, x[keep], dtok[keep], q, qt, seeds, qtok, "after append + delete")
