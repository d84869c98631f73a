"""The query-side value edges of the dense channel (tests/test_gpu_dense_query_edges.py and its host
companion): the 70 planted queries of dense_cases.planted with edge queries substituted at fixed odd
positions, each derived from the planted-neighbour query next to it, so that it has a meaningful top-k.

The f16 scans certify a score with  eps32 + ea (1 + eq) + eq,  eq = ||fp16(q) - q|| / ||q||  (qerr in
the workspace).  The edges are the queries at which that term, or the float16 image itself, leaves the
range every other test draws from: an image that is all zero, one that holds an infinity, one in
float16's subnormals, and float32 values at the ends of float32's own range.

Also the workspace carve of an f16 batch over float32 rows (shortlist "f16-inline" / "f16-anydim"), a
Python replica of make_plan (csrc/dense.hip) held to the library by the host test."""
import functools

import numpy as np

from dense_cases import TIE_QUERY, ZERO_QUERY, planted
from dense_emit_cases import CAND_BYTES, CAND_CAP, SEL_BIG_BAND

CLASSES = ("plain", "subnormal", "inf_image", "zero_image")
F16_MAX = 65504.0
SUBNORMAL_EQ = 2.0 ** -10     # a finite image whose eq reaches this is in float16's subnormals
F32_TINY = float(np.finfo(np.float32).tiny)

# power-of-two scales of the base query; the three named ones depend on its largest component
POW2 = (-140, -120, -40, -28, -24, -20, -17, -14, 10, "f16max", "f16over", 40, 100, "f32max")
COMPONENT = (65504.0, 65519.0, 65520.0, -65520.0, 3e38)      # 65519 rounds down to 65504, 65520 to inf


def image(q):
    """fp16(q) in float64 (round to nearest even, as the kernels' conversion)."""
    with np.errstate(over="ignore"):
        return np.asarray(q, np.float32).astype(np.float16).astype(np.float64)


def eq_f64(q):
    """||fp16(q) - q|| / ||q|| in float64: inf for an image that holds a non-finite value, 0 for a query
    without a non-zero component."""
    q64 = np.asarray(q, np.float32).astype(np.float64)
    img = image(q)
    if not np.all(np.isfinite(img)):
        return np.inf
    nn = float(np.sum(q64 * q64))
    return float(np.sqrt(np.sum((img - q64) ** 2) / nn)) if nn > 0.0 else 0.0


def classify(q):
    img = image(q)
    if not np.all(np.isfinite(img)):
        return "inf_image"
    if not img.any():
        return "zero_image"
    return "subnormal" if eq_f64(q) >= SUBNORMAL_EQ else "plain"


def _scaled(base, e):
    """base x 2^e, computed in float64 and rounded to float32."""
    return (base.astype(np.float64) * 2.0 ** e).astype(np.float32)


def pow2_exponent(base, what):
    """The exponents that depend on the query: the largest power of two whose image is still finite, the
    next one (the image holds infinities), the one that puts the largest component at 2^127."""
    if isinstance(what, int):
        return what
    big = float(np.max(np.abs(base)))
    if what == "f32max":
        return 127 - int(np.floor(np.log2(big)))
    e = 0
    while np.all(np.isfinite(image(_scaled(base, e + 1)))):
        e += 1
    return e if what == "f16max" else e + 1


def edge_positions(nq=70):
    """Odd positions except ZERO_QUERY's, six in every full tile of 16 and every odd one of the last:
    every tile of 16, 32 and 64 consecutive queries holds edge queries beside its even (planted
    neighbour) and remaining odd (random) ordinary ones.  Dealt across the tiles in turn, so that the
    classes spread over them."""
    per_tile = [[p for p in range(t, min(t + 16, nq)) if p % 2 == 1 and p != ZERO_QUERY][:6]
                for t in range(0, nq, 16)]
    out = []
    for j in range(6):
        out += [tile[j] for tile in per_tile if j < len(tile)]
    return out


def base_of(p):
    """The planted-neighbour query an edge query at odd position p is derived from."""
    return p - 1 if p - 1 != TIE_QUERY else p + 1


@functools.lru_cache(maxsize=None)
def catalogue(n, d):
    """-> (queries float32 [70, d], names, classes, bases): position p is ordinary (name "ordinary", base
    -1) or the edge query `names[p]` derived from query bases[p].  Read-only, shared."""
    _, q0 = planted(n, d)
    q = q0.copy()
    nq = len(q)
    names, bases = ["ordinary"] * nq, [-1] * nq
    builders = []
    for what in POW2:
        builders.append((f"scale 2^{what}", lambda b, w=what: _scaled(b, pow2_exponent(b, w))))
    for v in COMPONENT:
        for dim_at, tag in ((0, "first"), (d - 1, "last")):
            def put(b, v=v, at=dim_at):
                out = b.copy()
                out[at] = np.float32(v)
                return out
            builders.append((f"component {v:g} in the {tag} dim", put))

    def one_hot_over_dust(b):
        out = _scaled(b, -30)
        out[d // 3] = 1.0
        return out

    def denormal_one_hot(b):
        out = np.zeros_like(b)
        out[int(np.argmax(np.abs(b)))] = np.float32(1.4e-45)
        return out

    builders += [("one hot over dust", one_hot_over_dust), ("float32 one-hot 1.4e-45", denormal_one_hot),
                 ("all -0.0", lambda b: np.full_like(b, -0.0))]
    positions = edge_positions(nq)
    assert len(builders) == len(positions) == 27
    for p, (name, make) in zip(positions, builders):
        b = base_of(p)
        assert b % 2 == 0 and b not in (TIE_QUERY, ZERO_QUERY) and names[b] == "ordinary"
        q[p] = make(q0[b])
        assert np.all(np.isfinite(q[p])), name       # every catalogue query is a finite float32 vector
        names[p], bases[p] = name, b
    classes = [classify(v) for v in q]

    # what the builder promises of its own queries
    at = {names[p]: p for p in positions}
    expect = dict({"scale 2^-28": "zero_image", "scale 2^-40": "zero_image", "scale 2^-120": "zero_image",
                   "scale 2^-140": "zero_image", "float32 one-hot 1.4e-45": "zero_image", "all -0.0": "zero_image",
                   "scale 2^-20": "subnormal", "scale 2^-17": "subnormal",
                   "scale 2^10": "plain", "scale 2^f16max": "plain", "scale 2^f16over": "inf_image",
                   "scale 2^40": "inf_image", "scale 2^100": "inf_image", "scale 2^f32max": "inf_image",
                   "one hot over dust": "plain"})
    for v in COMPONENT:
        for tag in ("first", "last"):
            expect[f"component {v:g} in the {tag} dim"] = "plain" if abs(v) < 65520 else "inf_image"
    for name, cls in expect.items():
        assert classes[at[name]] == cls, (name, classes[at[name]], cls)
    # (the two ends of the subnormal range: eq is about 1e-3 at 2^-14 and 0.9 at 2^-24)
    assert classes[at["scale 2^-24"]] in ("subnormal", "zero_image")
    assert classes[at["scale 2^-14"]] in ("subnormal", "plain")
    assert q[at["float32 one-hot 1.4e-45"]].any() and not image(q[at["float32 one-hot 1.4e-45"]]).any()
    assert q[at["scale 2^-140"]].any() and np.max(np.abs(q[at["scale 2^-140"]])) < F32_TINY
    assert 2.0 ** 127 <= np.max(np.abs(q[at["scale 2^f32max"]].astype(np.float64))) < 2.0 ** 128
    assert np.count_nonzero(image(q[at["one hot over dust"]])) == 1 and eq_f64(q[at["one hot over dust"]]) < 1e-7
    with np.errstate(over="ignore"):                 # the float32 norm overflows
        assert not np.isfinite(np.sum(q[at["scale 2^100"]] ** 2, dtype=np.float32))
    assert classes[ZERO_QUERY] == "zero_image" and names[ZERO_QUERY] == names[TIE_QUERY] == "ordinary"
    assert np.array_equal(q[ZERO_QUERY], q0[ZERO_QUERY]) and np.array_equal(q[TIE_QUERY], q0[TIE_QUERY])
    q.setflags(write=False)
    return q, tuple(names), tuple(classes), tuple(bases)


def is_edge(names):
    return np.array([nm != "ordinary" for nm in names])


def tiles_mix(names, tile):
    """Every tile of `tile` consecutive queries holds ordinary and edge queries."""
    edge = is_edge(names)
    return all(edge[t:t + tile].any() and (~edge[t:t + tile]).any() for t in range(0, len(names), tile))


def representatives(names, classes):
    """One edge position per class (the first), for the batches of one."""
    edge = is_edge(names)
    return {c: next(p for p in range(len(names)) if edge[p] and classes[p] == c) for c in CLASSES}


def carve_rows32(qtile, nq, n_docs, kprime):
    """{name: (byte offset, bytes)} of make_plan's workspace for an f16 batch over float32 rows (the
    in-flight-rounding scan and the runtime-dim scan: one count per query, a shared list per query
    tile, every sample score), the total and qpad.  Arena: every piece rounded up to 256 bytes."""
    ntiles = (nq + qtile - 1) // qtile
    qpad = ntiles * qtile
    groups = (n_docs + 31) // 32
    ks = min(kprime, 64)
    aim = 4096.0 * np.sqrt(n_docs / 1.0e6)
    aim = min(max(aim, min(8.0 * kprime, 4096.0)), 4096.0)
    target = max(min(int(n_docs * ks / aim), 1 << 20), 4 * ks)
    sg = min((target + 31) // 32, groups)
    sample_docs = 32 * sg if n_docs > CAND_CAP // 2 else 0
    tile_cap = qtile * (CAND_CAP // 2)
    pieces = [("tau", 4 * qpad), ("qerr", 4 * qpad), ("cnt", 4 * qpad), ("tcnt", 4 * ntiles),
              ("cand", CAND_BYTES * qpad * CAND_CAP), ("tlist", CAND_BYTES * ntiles * tile_cap),
              ("sample", 4 * qpad * sample_docs), ("qfrag", 0), ("sel_rows", 4 * qpad * SEL_BIG_BAND),
              ("sel_meta", 4 * 4 * qpad)]
    out, total = {}, 0
    for name, nbytes in pieces:
        out[name] = (total, nbytes)
        total += (nbytes + 255) & ~255
    return out, total, qpad
