"""Host side of the runtime-dim f16 scan (shortlist="f16-anydim"): which row lengths the f16 entry
points take, the query tile they report, the sizes -- pure host arithmetic, no GPU."""
import os
import re

import pytest

import triple_hybrid_rag_amd as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = T._native
T._build.build_native()     # (a no-op unless a source is newer than the library)


def test_the_headers_limits_are_the_bindings():
    header = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    step = re.search(r"#define\s+THR_DENSE_ANYDIM_STEP\s+(\d+)", header)
    top = re.search(r"#define\s+THR_DENSE_ANYDIM_MAX\s+(\d+)", header)
    assert step and top
    assert int(step.group(1)) == N.THR_DENSE_ANYDIM_STEP == 32
    assert int(top.group(1)) == N.THR_DENSE_ANYDIM_MAX == 4096
    assert N.load().thr_abi_version() == N.ABI_VERSION == 9
    assert "f16-anydim" in T.GpuIndex.SHORTLISTS
    assert [d for d in (32, 48, 96, 384, 4000, 4096, 4128, 8192, 0, -32) if N.dense_anydim_ok(d)] == \
        [32, 96, 384, 4000, 4096]


@pytest.mark.parametrize("dim", [32, 96, 384, 1536, 4000, 4096])
def test_row_lengths_the_f16_entry_points_take_without_a_copy(dim):
    tile = N.dense_f16_query_tile(dim, False, 1)
    assert tile > 0 and tile % 16 == 0
    # the float16 tile and the 8 waves' candidate buffers (2 KiB each) fit the CU's 160 KiB of LDS
    assert tile * dim * 2 + 8 * 2048 <= 160 * 1024
    assert N.dense_f16_max_queries(dim, False) > 0
    # ... and none of them with a float16 copy
    assert N.dense_f16_query_tile(dim, True, 1) == 0 and N.dense_f16_max_queries(dim, True) == 0


def test_row_lengths_they_refuse():
    for dim in (48, 4128, 8192):
        assert N.dense_f16_query_tile(dim, False, 1) == 0
        assert N.dense_f16_max_queries(dim, False) == 0
    assert N.dense_f16_query_tile(384, True, 1) == 0
    lib = N.load()
    # thr_dense_topk_f16 itself: a good length gets as far as the null pointers (THR_ERR_INVALID), a bad one
    # or a copy at such a length is THR_ERR_UNSUPPORTED before anything is launched
    def topk(dim, docs16):
        # non-null pointer values that are never followed: workspace_bytes = 0 is refused (-3) by the last
        # host check, after the shape checks under test and before the first launch
        one = 1
        return lib.thr_dense_topk_f16(one, docs16, 0.0, one, one, 100, dim, 0, one, 1, 10, 100, None, None,
                                      one, one, one, one, one, 0, None)
    assert topk(384, None) == -3 and topk(4000, None) == -3          # (workspace too small: the shape passed)
    assert topk(48, None) == -2 and topk(4128, None) == -2 and topk(384, 1) == -2


def test_the_tuned_lengths_report_what_they_did():
    """512 / 768 / 1024: the values of the build before this flavour existed."""
    for dim, tile, packed_tile, packed_max in ((512, 64, 256, 32512), (768, 64, 256, 32512), (1024, 32, 192, 32640)):
        assert N.dense_f16_query_tile(dim, False, 2048) == tile
        assert N.dense_f16_query_tile(dim, True, 2048) == packed_tile
        assert N.dense_f16_max_queries(dim, False) == 2 ** 31 - 1
        assert N.dense_f16_max_queries(dim, True) == packed_max
        # the runtime-dim scan has the same tile at these lengths: selecting it changes no size
        with N.dense_f16_flavour(True):
            assert N.load().thr_dense_f16_select(-1) == N.THR_DENSE_F16_ANYDIM     # the selection took
            assert N.dense_f16_query_tile(dim, False, 2048) == tile
            assert N.dense_f16_query_tile(dim, True, 2048) == packed_tile
    assert N.load().thr_dense_f16_select(-1) == N.THR_DENSE_F16_BY_DIM      # restored; -1 only queries


def test_workspace_grows_with_the_batch():
    sizes = [N.dense_f16_workspace_bytes(100_000, 384, nq, 192) for nq in (1, 64, 65, 2048)]
    assert sizes[0] > 0 and sizes[0] == sizes[1] and sizes[1] < sizes[2] < sizes[3]
    # 16 queries per tile at 4096: 17 queries are two tiles
    assert N.dense_f16_workspace_bytes(100_000, 4096, 17, 192) > N.dense_f16_workspace_bytes(100_000, 4096, 16, 192)
