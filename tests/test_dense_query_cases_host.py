"""Host side of tests/test_gpu_dense_query_edges.py: the catalogue of edge queries is what it says it is,
the float64 oracle answers every one of them, a power-of-two scaling leaves its answer unchanged, and
the restated workspace carve of an f16 batch over float32 rows is the library's.  No GPU."""
import os
import sys

import numpy as np
import pytest

import triple_hybrid_rag_amd as T
from oracle import c_oracle as CO

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_cases import DOC_BASE, TIE_QUERY, ZERO_QUERY, planted  # noqa: E402
from dense_emit_cases import carve  # noqa: E402
from dense_query_cases import (CLASSES, F32_TINY, POW2, carve_rows32, catalogue, classify, eq_f64,  # noqa: E402
                               image, is_edge, representatives, tiles_mix)

N = T._native
SHAPE = (3001, 512)


@pytest.fixture(scope="module")
def oracle():
    x, _ = planted(*SHAPE)
    q, names, classes, bases = catalogue(*SHAPE)
    return x, q, names, classes, bases, CO.dense_topk_exact(x, q, 100, doc_id_base=DOC_BASE)


@pytest.mark.parametrize("d", [96, 512, 768, 1024])
def test_the_catalogue_is_what_it_says(d):
    """catalogue() asserts the class of every query it builds; here what the GPU tests rely on beside that."""
    q, names, classes, bases = catalogue(3001, d)
    _, q0 = planted(3001, d)
    assert q.shape == (70, d) and q.dtype == np.float32 and np.all(np.isfinite(q))
    edge = is_edge(names)
    assert edge.sum() == 27 and len(set(np.array(names)[edge])) == 27
    assert np.array_equal(q[~edge], q0[~edge]), "the ordinary queries are planted()'s"
    assert not edge[ZERO_QUERY] and not edge[TIE_QUERY] and not edge[::2].any()
    for p in np.nonzero(edge)[0]:
        assert bases[p] % 2 == 0 and not edge[bases[p]] and abs(bases[p] - p) == 1
        assert classes[p] == classify(q[p]) and classes[p] in CLASSES
    assert set(representatives(names, classes)) == set(CLASSES), "every class has an edge query"
    for p in range(70):
        e = eq_f64(q[p])
        img = image(q[p])
        assert (classes[p] == "inf_image") == (e == np.inf) == (not np.all(np.isfinite(img)))
        assert (classes[p] == "zero_image") == (not img.any())
        if classes[p] == "subnormal":
            assert 2.0 ** -10 <= e <= 1.0
        if classes[p] == "plain":
            assert e < 2.0 ** -10
    # a non-zero query whose image is zero has eq = 1 exactly; the zero queries 0 by definition
    at = {nm: p for p, nm in enumerate(names)}
    assert eq_f64(q[at["scale 2^-28"]]) == 1.0 and eq_f64(q[at["all -0.0"]]) == 0.0 == eq_f64(q[ZERO_QUERY])
    assert np.all(np.signbit(q[at["all -0.0"]])) and not q[at["all -0.0"]].any()


@pytest.mark.parametrize("tile", [16, 32, 64])
def test_every_query_tile_mixes_ordinary_and_edge_queries(tile):
    _, names, _, _ = catalogue(*SHAPE)
    assert tiles_mix(names, tile)


def test_the_oracle_answers_every_query(oracle):
    x, q, names, classes, bases, (Se, Ie, cnte) = oracle
    assert np.all(cnte == 100), "a full count for every position"
    assert np.all(np.isfinite(Se)) and np.all((Ie >= DOC_BASE) & (Ie < DOC_BASE + len(x)))
    assert np.all(Se[:, :-1] >= Se[:, 1:])


def test_a_power_of_two_scale_in_the_normal_range_keeps_the_oracles_bits(oracle):
    """Scaling by 2^e is exact while every non-zero value stays normal in float32, and the cosine does
    not see it: the base query's ids and score bits."""
    x, q, names, classes, bases, (Se, Ie, cnte) = oracle
    checked = []
    for p, nm in enumerate(names):
        if not nm.startswith("scale 2^"):
            continue
        v = np.abs(q[p].astype(np.float64))
        if not np.all(v[v > 0] >= F32_TINY) or np.count_nonzero(v) != np.count_nonzero(q[bases[p]]):
            continue
        checked.append(nm)
        assert np.array_equal(Ie[p], Ie[bases[p]]) and np.array_equal(Se[p], Se[bases[p]]), nm
    assert len(checked) >= len(POW2) - 3, checked       # all but the scales that reach float32's subnormals
    assert {"scale 2^-40", "scale 2^-28", "scale 2^f16over", "scale 2^100", "scale 2^f32max"} <= set(checked)


@pytest.mark.parametrize("kp", [192, 128])
@pytest.mark.parametrize("nq", [1, 70, 300])
@pytest.mark.parametrize("n,d", [(3001, 96), (20011, 96), (3001, 512), (20011, 768), (9001, 1024), (9001, 2048)])
def test_the_rows32_carve_is_the_librarys(n, d, nq, kp):
    """carve_rows32 against thr_dense_f16_workspace_bytes: equal where the runtime-dim scan is the only
    one; at 512 / 768 / 1024 the library sizes one workspace for either f16 scan, the larger of this
    carve and the packed one (dense_emit_cases.carve)."""
    qtile = N.dense_f16_query_tile(d, False, nq)
    assert qtile == (64 if d <= 768 else 32 if d <= 1536 else 16)
    where, total, qpad = carve_rows32(qtile, nq, n, kp)
    assert qpad % qtile == 0 and nq <= qpad < nq + qtile
    need = N.dense_f16_workspace_bytes(n, d, nq, kp)
    if d in (512, 768, 1024):
        packed_total = carve(N.dense_f16_query_tile(d, True, nq), nq, d)[1]
        assert need == max(total, packed_total)
    else:
        assert need == total
    assert where["qerr"] == ((4 * qpad + 255) & ~255, 4 * qpad)
    end = 0
    for name, (off, nbytes) in where.items():
        assert off % 256 == 0 and off >= end and off - end < 256, name
        end = off + nbytes
    assert (where["sample"][1] == 0) == (n <= 8192)
