"""Host side of tests/test_gpu_dense_emit.py: the Python replica of the workspace carve it reads the
candidate, count and sample areas through, and the two instantiations (with and without a collection
filter) of the register-resident scans in the built library.  No GPU."""
import os
import sys

import pytest

import triple_hybrid_rag_amd as T

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_emit_cases import (CAND_BYTES, CAND_CAP, QREG_MAX_SEG, SAMPLE_TOP, carve, plan,  # noqa: E402
                              segment_of_row, unpack_copy16)

N = T._native


@pytest.fixture(scope="module")
def library():
    """The built library's path (a build only when a source is newer than it)."""
    return T._build.build_native()


@pytest.mark.parametrize("n", [12001, 40001])
@pytest.mark.parametrize("nq", [33, 300])
@pytest.mark.parametrize("d", [512, 768, 1024])
def test_the_carve_fits_the_workspace_the_library_asks_for(d, nq, n):
    qtile = N.dense_f16_query_tile(d, True, nq)
    assert qtile in (128, 192, 256)
    where, total, qpad = carve(qtile, nq, d)
    assert qpad % qtile == 0 and nq <= qpad < nq + qtile
    # the library sizes one workspace for either f16 scan: at least the packed plan's
    assert total <= N.dense_f16_workspace_bytes(n, d, nq, 102)
    # the pieces follow one another in make_plan's order, each on a 256-byte boundary
    names = ["tau", "qerr", "cnt", "tcnt", "cand", "tlist", "sample", "qfrag", "sel_rows", "sel_meta"]
    assert list(where) == names
    end = 0
    for name in names:
        off, nbytes = where[name]
        assert off % 256 == 0 and off >= end and off - end < 256
        end = off + nbytes
    assert where["cand"][1] == CAND_BYTES * qpad * CAND_CAP
    assert where["sample"][1] == 4 * qpad * QREG_MAX_SEG * SAMPLE_TOP


def test_the_constants_are_the_sources():
    src = open(os.path.join(T._build.CSRC, "dense_common.hpp")).read()
    for name, value in (("CAND_CAP", CAND_CAP), ("QREG_MAX_SEG", QREG_MAX_SEG), ("SAMPLE_TOP", SAMPLE_TOP)):
        assert f"constexpr int {name} = {value};" in src, name


def test_the_sample_of_the_test_shapes():
    # 12 001 rows at k' = 102: 15 sample tiles, every 25th row group; 40 001 rows: 49 of them
    assert plan(12001, 102) == (25, 15)
    assert plan(40001, 102) == (25, 49)


@pytest.mark.parametrize("shape", [16, 32])
def test_unpack_is_the_inverse_of_the_copys_row_order(shape):
    import numpy as np
    dim, tiles = 64, 3
    ks = dim // 16
    packed = np.full(tiles * 32 * dim, -1, dtype=np.int64)
    for row in range(tiles * 32):
        tile, r = row >> 5, row & 31
        for i in range(dim):
            if shape == 32:        # quantize_f16_norm, shape 32
                s, hh, e = i >> 4, (i >> 3) & 1, i & 7
                at = (((tile * ks + s) * 64) + r + 32 * hh) * 8 + e
            else:                  # shape 16
                k32, g, e, ra = i >> 5, (i >> 3) & 3, i & 7, r >> 4
                at = (((tile * ks + 2 * k32 + ra) * 64) + (r & 15) + 16 * g) * 8 + e
            packed[at] = row * dim + i
    assert np.array_equal(unpack_copy16(packed, dim, shape).ravel(), np.arange(tiles * 32 * dim))
    # the rows of a tile fall into SEGS lane groups of equal size
    segs = [segment_of_row(r, shape) for r in range(32)]
    assert sorted(set(segs)) == list(range(2 if shape == 32 else 4))
    assert all(segs.count(s) == 32 // len(set(segs)) for s in set(segs))


def test_both_instantiations_are_in_the_library(library):
    """dense_scan_f16qs<DIM, MODE, SHAPE, COLL> and dense_scan_f16q<DIM, MODE, PROF, SHAPE, COLL>: the
    launcher picks COLL = false for a batch without a collection filter, so every (dim, mode, shape) it
    reaches exists in both (Itanium mangling: ...ELb0EEE / ...ELb1EEE close the argument list)."""
    blob = open(library, "rb").read()
    for dim in (512, 768):
        for mode in (0, 1):
            for shape in (16, 32):
                for coll in (0, 1):
                    name = f"dense_scan_f16qsILi{dim}ELi{mode}ELi{shape}ELb{coll}EEE"
                    assert name.encode() in blob, name
    for shape in (16, 32, 48):
        for mode in (0, 1):
            for coll in (0, 1):
                name = f"dense_scan_f16qILi1024ELi{mode}ELb0ELi{shape}ELb{coll}EEE"
                assert name.encode() in blob, name
