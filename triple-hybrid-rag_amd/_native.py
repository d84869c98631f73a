"""ctypes binding of libthr_hip.so (include/thr_hip.h) over PyTorch-ROCm tensors.

PyTorch is used for device memory, streams and torch.distributed only; every
scorer is a hand-written HIP kernel behind the C ABI.  There is NO CPU or
eager-PyTorch fallback: if the library is missing or a call fails, this module
raises.  Operand shapes/dtypes/devices are validated here, on the host, before
any kernel is launched.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import math
import os
from typing import Optional, Tuple

import torch

from . import _build

THR_FLAG_CERTIFIED = 1
THR_FLAG_OVERFLOW = 2
THR_FLAG_EXACT = 4
THR_DENSE_MAX_K = 256
THR_DENSE_ANYDIM_STEP = 32      # the runtime-dim f16 scan: row lengths that are a multiple of this ...
THR_DENSE_ANYDIM_MAX = 4096     # ... up to this
THR_DENSE_F16_BY_DIM, THR_DENSE_F16_ANYDIM = 0, 1   # thr_dense_f16_select
THR_BM25_MAX_TERMS = 32
THR_BM25_MAX_QUERIES = 1 << 20
THR_GRAPH_MAX_SEEDS = 16
THR_RRF_MAX_PER_CHANNEL = 128
THR_RRF_MAX_TOP_K = 512          # rows of one fused list (thr_rrf_fuse*, thr_fuse_post, thr_rerank_order)
THR_TOPK_MAX = 128
THR_SCOPE_MAX_COLS = 8
THR_SCOPE_MAX_PREDS = 4096
THR_SCOPE_MAX_QUERIES = 1 << 20
THR_SCOPE_MAX_SET_VALUES = 1 << 22   # set members of one thr_scope_resolve_clauses call
# clause kinds of thr_scope_resolve_clauses: (kind, a, b, 0); + SCOPE_NEGATED on a range or a set
SCOPE_ANY, SCOPE_NONE, SCOPE_RANGE, SCOPE_SET, SCOPE_NEGATED = 0, 1, 2, 3, 4
THR_ENTITY_MAX_NEEDLE = 128     # bytes of a keyword's lowered UTF-8 thr_entity_match takes
THR_ENTITY_MAX_KEYWORDS = 5
THR_ENTITY_MAX_QUERIES = 1 << 20
THR_ENTITY_SLICE_BYTES = 8192   # name bytes a workgroup of thr_entity_match stages at a time
THR_TEXT_SLICE_BYTES = 8192     # text bytes a workgroup of thr_text_tokens stages at a time
THR_TEXT_MAX_TEXTS = 1 << 20    # texts of one thr_text_tokens / thr_query_terms call
THR_TEXT_MAX_BYTES = 0x7FFFFFFF   # bytes of one thr_text_tokens call
THR_TEXT_WORD, THR_TEXT_EXC = 1 << 16, 1 << 17   # bits of a TextTable entry above the lowered code point
# bits of the text flags: redo on the host; (thr_query_terms) an unknown token occurred; more than 32 distinct terms
THR_TEXT_EXCEPTIONAL, THR_TEXT_UNKNOWN, THR_TEXT_TOO_MANY = 1, 2, 4
# thr_hip_fuzzy.h THR_TEXT_CORRECTED: (thr_query_terms_fuzzy) an unknown token was replaced by its nearest terms
TEXT_CORRECTED = 8
THR_VOCAB_MIN_SLOTS, THR_VOCAB_MAX_SLOTS = 16, 1 << 30
# bits of thr_vocab_grow's status word: two tokens under one masked hash; new_bytes_capacity below n_new_bytes
THR_VOCAB_GROW_COLLISION, THR_VOCAB_GROW_OVERFLOW = 1, 2
THR_CSR_MERGE_SLICE = 1024      # positions a workgroup of thr_csr_merge owns
# bits of thr_csr_merge's status word: an input breaks its mode's ordering; the result exceeds out_capacity
THR_CSR_MERGE_UNSORTED_A, THR_CSR_MERGE_UNSORTED_B, THR_CSR_MERGE_OVERFLOW = 1, 2, 4
# token dims thr_maxsim has a kernel for (csrc/maxsim.hip THR_MS_KSTEPS, times 16)
MAXSIM_TOK_DIMS = (16, 32, 64, 96, 128, 192, 256)
ABI_VERSION = 9

_lib = None


class NativeError(RuntimeError):
    pass


_i64, _i32, _dbl, _sz, _vp = C.c_int64, C.c_int, C.c_double, C.c_size_t, C.c_void_p
_SIGNATURES = {
    "thr_abi_version": (C.c_int, []),
    "thr_error_string": (C.c_char_p, [_i32]),
    "thr_device_info": (_i32, [C.POINTER(_i32), C.POINTER(_i64), C.c_char_p, _i32]),
    "thr_embed_postproc": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp]),
    "thr_doc_norms": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp]),
    "thr_dense_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "thr_dense_topk": (_i32, [_vp, _vp, _vp, _i64, _i32, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp,
                              _vp, _vp, _vp, _sz, _vp]),
    "thr_dense_exact_workspace_bytes": (_sz, [_i64, _i32]),
    "thr_dense_topk_exact": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _sz, _vp]),
    "thr_dense_scan_probe": (_i32, [_vp, _vp, _i64, _i32, _vp, _i32, _vp, _sz, _vp]),
    "thr_dense_rescue_workspace_bytes": (_sz, [_i32, _i32]),
    "thr_dense_rescue": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                _vp, _sz, _vp]),
    "thr_dense_quantize_f16": (_i32, [_vp, _i64, _i32, _vp, _vp, _vp]),
    "thr_dense_f16_workspace_bytes": (_sz, [_i64, _i32, _i32, _i32]),
    "thr_dense_f16_copy_bytes": (_sz, [_i64, _i32]),
    "thr_dense_f16_query_tile": (_i32, [_i32, _i32, _i32]),
    "thr_dense_f16_max_queries": (_i32, [_i32, _i32]),
    "thr_dense_f16_select": (_i32, [_i32]),
    "thr_dense_topk_f16": (_i32, [_vp, _vp, _dbl, _vp, _vp, _i64, _i32, _i64, _vp, _i32, _i32,
                                  _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_dense_shortlist_f16": (_i32, [_vp, _vp, _dbl, _vp, _i64, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _vp,
                                       _vp, _sz, _vp]),
    "thr_dense_floor": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "thr_dense_finish_f16": (_i32, [_vp, _vp, _dbl, _vp, _vp, _i64, _i32, _i64, _vp, _i32, _i32,
                                    _i32, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_dense_scan_probe_f16": (_i32, [_vp, _vp, _vp, _i64, _i32, _vp, _i32, _vp, _sz, _vp]),
    "thr_dense_scan_stamps_f16": (_i32, [_vp, _i64, _i32, _i32, _vp, _sz, _vp, C.POINTER(_i32), _vp]),
    "thr_lexical_build_workspace_bytes": (_sz, [_i64, _i64]),
    "thr_lexical_build": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_csr_append": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _vp]),
    "thr_csr_compact_workspace_bytes": (_sz, [_i64, _i64]),
    "thr_csr_compact": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp, _sz, _vp]),
    "thr_csr_merge_slice": (_i32, []),
    "thr_csr_merge_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "thr_csr_merge": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _i32, _vp, _vp, _vp, _i64, _vp, _vp,
                             _vp, _sz, _vp]),
    "thr_scope_resolve_workspace_bytes": (_sz, [_i64, _i32]),
    "thr_scope_resolve": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "thr_scope_resolve_clauses_workspace_bytes": (_sz, [_i64, _i32]),
    "thr_scope_resolve_clauses": (_i32, [_vp, _i32, _i64, _vp, _i32, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _vp, _sz, _vp]),
    "thr_dense_topk_rows_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "thr_dense_topk_rows": (_i32, [_vp, _vp, _i64, _i32, _i64, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _vp,
                                   _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_bm25_block_count": (_sz, [_i64]),
    "thr_bm25_bounds": (_i32, [_vp, _vp, _vp, _vp, _vp, _dbl, _dbl, _dbl, _i64, _i64, _vp, _vp, _vp, _vp]),
    "thr_bm25_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "thr_bm25_dense_stride": (_i64, [_i64]),
    "thr_bm25_dense_rows": (_i32, [_vp, _vp, _vp, _vp, _vp, _i32, _i64, _i64, _vp, _vp, _vp]),
    "thr_bm25_topk": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _dbl, _dbl, _dbl, _i64, _i64, _i64,
                             _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_graph_workspace_bytes": (_sz, [_i32, _i64]),
    "thr_graph_topk": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _i32,
                              _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_graph_topk_scoped": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp,
                                     _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_entity_match_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "thr_entity_match": (_i32, [_vp, _vp, _i64, _vp, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _sz, _vp]),
    "thr_vocab_table_bytes": (_sz, [_i64]),
    "thr_vocab_insert": (_i32, [_vp, _i64, _vp, _vp, _i64, _i64, _vp]),
    "thr_text_tokens_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "thr_text_tokens": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                               _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_query_terms_workspace_bytes": (_sz, [_i32]),
    "thr_query_terms": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_vocab_grow_workspace_bytes": (_sz, [_i64]),
    "thr_vocab_grow": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _i64, _i64, C.c_uint64, _vp, _vp, _i64,
                              _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "thr_rrf_fuse": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _dbl, _dbl, _dbl, _i32, _i32,
                            _vp, _vp, _vp, _vp, _vp]),
    "thr_rrf_fuse_standalone": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _dbl, _dbl, _dbl, _i32, _i32,
                                       _vp, _vp, _vp, _vp, _vp]),
    "thr_fuse_post": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _vp, _i32, _dbl, _i32,
                             _dbl, _i32, _i32, _vp, _vp, _vp, _vp]),
    "thr_rerank_order": (_i32, [_vp, _i32, _i64, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "thr_maxsim": (_i32, [_vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _vp]),
    "thr_maxsim_ids": (_i32, [_vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _i32, _vp]),
    "thr_maxsim_pack": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "thr_merge_topk": (_i32, [_vp, _vp, _i32, _i32, _i32, _i64, _i32, _vp, _vp, _vp, _vp]),
}
EXPORTED_SYMBOLS = tuple(_SIGNATURES)
# include/thr_hip_graph.h: the entry points that came after ABI version 9 (additive: the version stays)
_SIGNATURES_GRAPH = {
    "thr_csr_prune_slice": (_i32, []),
    "thr_csr_prune_workspace_bytes": (_sz, [_i64, _i64]),
    "thr_csr_prune": (_i32, [_vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i64,
                             _vp, _vp, _vp, _vp, _sz, _vp]),
}
# thr_hip_graph.h's #defines (THR_CSR_PRUNE_*): positions a workgroup of thr_csr_prune owns; the bits of its
# status word -- a row of B not strictly ascending, the result exceeds out_capacity, a row destination >= rows_out
CSR_PRUNE_SLICE = 1024
CSR_PRUNE_UNSORTED_B, CSR_PRUNE_OVERFLOW, CSR_PRUNE_BAD_ROW = 1, 2, 4
# include/thr_hip_text.h: the token-level analysis behind the character table (additive as well)
_SIGNATURES_TEXT = {
    "thr_text_tokens_analyzed_workspace_bytes": (_sz, [_i64, _i64, _i64]),
    "thr_text_tokens_analyzed": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _i64,
                                        _vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
}
# thr_hip_text.h's #defines (THR_STEM_*): code points of a suffix, steps and rules of a table, bytes of a rule record
STEM_MAX_SUFFIX, STEM_MAX_STEPS, STEM_MAX_RULES, STEM_RULE_BYTES = 8, 4, 1024, 24
# include/thr_hip_rerank.h: the FP8 token store of the late-interaction rerank (additive as well)
_SIGNATURES_RERANK = {
    "thr_maxsim_quantize_fp8": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp, _vp]),
    "thr_maxsim_fp8": (_i32, [_vp, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp]),
    "thr_maxsim_fp8_ids": (_i32, [_vp, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _vp]),
}
# token dims thr_maxsim_fp8 has a kernel for (csrc/maxsim_fp8.hip THR_M8_KPAIRS, times 32): a lane's 16 bytes
# of the packed image are two k-steps, so 16 -- which thr_maxsim takes -- is not among them
MAXSIM_FP8_TOK_DIMS = (32, 64, 96, 128, 192, 256)
# include/thr_hip_parent.h: child -> parent expansion (the groups of a fused row, MaxSim over a parent's children;
# additive as well).  The scorers take MAXSIM_TOK_DIMS (float16, packed image) / MAXSIM_FP8_TOK_DIMS.
_SIGNATURES_PARENT = {
    "thr_parent_groups": (_i32, [_vp, _vp, _i32, _i32, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp]),
    "thr_maxsim_parent_ids": (_i32, [_vp, _i32, _i32, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _i32, _i64,
                                     _vp, _vp]),
    "thr_maxsim_parent_fp8_ids": (_i32, [_vp, _i32, _i32, _vp, _vp, _i64, _i32, _i32, _vp, _i64, _i32, _vp, _vp, _vp, _i32,
                                         _i64, _vp, _vp]),
}
# include/thr_hip_diversify.h: diversified top-k (MMR over the candidates' dense rows; additive as well)
_SIGNATURES_DIVERSIFY = {
    "thr_mmr_select": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i64, _i32, _i64, _dbl, _i32, _vp, _vp, _vp, _vp, _vp,
                              _vp]),
}
# include/thr_hip_fuzzy.h: the nearest vocabulary terms of unknown tokens, and the query table with them (additive as well)
_SIGNATURES_FUZZY = {
    "thr_vocab_nearest_workspace_bytes": (_sz, [_i64, _i64, _i64, _i64, _i32]),
    "thr_vocab_nearest": (_i32, [_vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _i64, _i64, _vp, _i32, _i32, _vp, _vp, _vp,
                                 _sz, _vp]),
    "thr_query_terms_fuzzy_workspace_bytes": (_sz, [_i32]),
    "thr_query_terms_fuzzy": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _sz, _vp]),
}
# thr_hip_fuzzy.h's #defines: code points of a needle, corrections kept per token, key bytes a workgroup stages
FUZZY_MAX_LEN, FUZZY_MAX_BEST, FUZZY_SLICE_BYTES, FUZZY_MAX_EDITS = 32, 4, 8192, 2


def lib_path() -> str:
    return _build.LIB_PATH


def load(build_if_missing: bool = True):
    """Load libthr_hip.so; raises NativeError when it cannot (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    path = _build.LIB_PATH
    if not os.path.exists(path):
        if not build_if_missing:
            raise NativeError(f"{path} is missing: build it with __graft_entry__.build()")
        _build.build_native()
    try:
        lib = C.CDLL(path)
    except OSError as e:  # pragma: no cover
        raise NativeError(f"cannot load {path}: {e}") from e
    for name, (res, args) in (list(_SIGNATURES.items()) + list(_SIGNATURES_GRAPH.items()) + list(_SIGNATURES_TEXT.items())
                              + list(_SIGNATURES_RERANK.items()) + list(_SIGNATURES_PARENT.items())
                              + list(_SIGNATURES_DIVERSIFY.items()) + list(_SIGNATURES_FUZZY.items())):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise NativeError(f"{path} does not export {name}") from e
        fn.restype, fn.argtypes = res, args
    if lib.thr_abi_version() != ABI_VERSION:
        raise NativeError("libthr_hip.so ABI version mismatch; rebuild")
    _lib = lib
    return lib


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().thr_error_string(rc).decode()
        raise NativeError(f"{what} failed: {msg} (code {rc})")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _dev(t: Optional[torch.Tensor], dtype, name: str, ndim: Optional[int] = None) -> int:
    if t is None:
        return 0
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise NativeError(f"{name}: expected a CUDA(HIP) tensor")
    if t.dtype != dtype:
        raise NativeError(f"{name}: expected dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise NativeError(f"{name}: must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise NativeError(f"{name}: expected {ndim} dims, got {t.dim()}")
    return t.data_ptr()


def _workspace(workspace: Optional[torch.Tensor], need: int, device) -> Tuple[torch.Tensor, int]:
    """THE workspace rule -> (the tensor to hand to the library, its size in bytes): the caller's
    ``workspace`` when it holds at least ``need`` bytes (any dtype: bytes are numel x element size;
    a contiguous device tensor), else a fresh uint8 one of max(need, 16) bytes (no call hands the
    library a null workspace)."""
    if workspace is not None:
        nbytes = workspace.numel() * workspace.element_size()
        if nbytes >= need:
            _dev(workspace, workspace.dtype, "workspace")
            return workspace, nbytes
    nbytes = max(int(need), 16)
    return torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def device_info() -> Tuple[int, int, str]:
    cus, hbm = C.c_int(0), C.c_int64(0)
    arch = C.create_string_buffer(128)
    torch.cuda.current_device()  # make sure the HIP context exists on the right device
    _check(load().thr_device_info(C.byref(cus), C.byref(hbm), arch, 128), "thr_device_info")
    return cus.value, hbm.value, arch.value.decode()


# --------------------------------------------------------------------- a1
def embed_postproc(full: torch.Tensor, store_dim: int) -> torch.Tensor:
    p = _dev(full, torch.float32, "full", 2)
    n, fd = full.shape
    out = torch.empty((n, min(fd, store_dim)), dtype=torch.float32, device=full.device)
    if n:
        _check(load().thr_embed_postproc(p, n, fd, store_dim, out.data_ptr(), _stream()),
               "thr_embed_postproc")
    return out


def doc_norms(docs: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    p = _dev(docs, torch.float32, "docs", 2)
    n, d = docs.shape
    dn = torch.empty(n, dtype=torch.float64, device=docs.device)
    inv = torch.empty(n, dtype=torch.float32, device=docs.device)
    if n:
        _check(load().thr_doc_norms(p, n, d, dn.data_ptr(), inv.data_ptr(), _stream()),
               "thr_doc_norms")
    return dn, inv


# --------------------------------------------------------------------- a2
def dense_workspace_bytes(n_docs: int, dim: int, n_queries: int, kprime: int) -> int:
    return int(load().thr_dense_workspace_bytes(n_docs, dim, n_queries, kprime))


def _alloc_out(nq: int, k: int, device):
    # scores and ids are the two halves of ONE [2, nq, k] 8-byte tile: the multi-GPU exchange
    # all-gathers that tile as it is (distributed.gather_topk), no packing copy
    tile = torch.empty((2, nq, k), dtype=torch.int64, device=device)
    return (tile[0].view(torch.float64), tile[1],
            torch.empty(nq, dtype=torch.int32, device=device),
            torch.empty(nq, dtype=torch.int32, device=device))


def _coll(doc_coll, query_coll, n: int, nq: int):
    """(doc_coll ptr, query_coll ptr) of the collection filter, or (None, None)."""
    if query_coll is None:
        return None, None
    if doc_coll is None:
        raise NativeError("query_coll without doc_coll")
    if doc_coll.shape != (n,) or query_coll.shape != (nq,):
        raise NativeError("doc_coll / query_coll have the wrong length")
    return _dev(doc_coll, torch.int32, "doc_coll", 1), _dev(query_coll, torch.int32, "query_coll", 1)


def _dense_operands(docs, queries, dnorm=None, inv_norm=None, docs16=None):
    """THE operand check of the dense calls -> (docs, queries, dnorm, inv_norm, docs16 pointers, n, d, nq).
    docs f32 [n, d]; queries f32 [nq, d]; of the rest what the entry takes (None: a null pointer, which
    the library refuses where the operand is not optional): dnorm f64 [n], inv_norm f32 [n], docs16 the
    fragment-major f16 [ceil32(n), d] image of docs."""
    pd = _dev(docs, torch.float32, "docs", 2)
    n, d = docs.shape
    pq = _dev(queries, torch.float32, "queries", 2)
    nq = queries.shape[0]
    if queries.shape[1] != d:
        raise NativeError(f"queries dim {queries.shape[1]} != docs dim {d}")
    pn = _dev(dnorm, torch.float64, "dnorm", 1)
    pi = _dev(inv_norm, torch.float32, "inv_norm", 1)
    if (dnorm is not None and dnorm.shape[0] != n) or (inv_norm is not None and inv_norm.shape[0] != n):
        raise NativeError("dnorm / inv_norm length != n_docs")
    ph = _dev(docs16, torch.float16, "docs16", 2)
    if docs16 is not None and tuple(docs16.shape) != ((n + 31) // 32 * 32, d):
        raise NativeError("docs16 is not the fragment-major copy of docs (thr_dense_quantize_f16)")
    return pd, pq, pn, pi, ph, n, d, nq


def dense_topk(docs, dnorm, inv_norm, queries, k: int, kprime: int, id_base: int = 0,
               workspace: Optional[torch.Tensor] = None, doc_coll=None, query_coll=None):
    """-> (scores f64 [nq,k], ids i64 [nq,k], counts i32 [nq], flags i32 [nq])."""
    pd, pq, pn, pi, _, n, d, nq = _dense_operands(docs, queries, dnorm, inv_norm)
    ws, nbytes = _workspace(workspace, dense_workspace_bytes(n, d, nq, kprime), docs.device)
    S, I, cnt, flg = _alloc_out(nq, k, docs.device)
    pdc, pqc = _coll(doc_coll, query_coll, n, nq)
    _check(load().thr_dense_topk(pd, pn, pi, n, d, id_base, pq, nq, k, kprime, pdc, pqc, S.data_ptr(),
                                 I.data_ptr(), cnt.data_ptr(), flg.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_dense_topk")
    return S, I, cnt, flg


def dense_topk_exact(docs, dnorm, queries, k: int, id_base: int = 0, doc_coll=None, query_coll=None,
                     workspace: Optional[torch.Tensor] = None):
    """thr_dense_topk_exact -> (scores, ids, counts, flags); ``workspace``: reused when it holds
    thr_dense_exact_workspace_bytes(n_docs, nq) bytes (_workspace), whatever it holds."""
    pd, pq, pn, _, _, n, d, nq = _dense_operands(docs, queries, dnorm)
    ws, nbytes = _workspace(workspace, int(load().thr_dense_exact_workspace_bytes(n, nq)), docs.device)
    S, I, cnt, flg = _alloc_out(nq, k, docs.device)
    pdc, pqc = _coll(doc_coll, query_coll, n, nq)
    _check(load().thr_dense_topk_exact(pd, pn, n, d, id_base, pq, nq, k, pdc, pqc, S.data_ptr(),
                                       I.data_ptr(), cnt.data_ptr(), flg.data_ptr(),
                                       ws.data_ptr(), nbytes, _stream()), "thr_dense_topk_exact")
    return S, I, cnt, flg


def dense_scan_probe(docs, inv_norm, queries, workspace: torch.Tensor) -> None:
    pd, pq, _, pi, _, n, d, nq = _dense_operands(docs, queries, inv_norm=inv_norm)
    ws, nbytes = _workspace(workspace, 0, docs.device)      # (the caller's as it is: the library judges its size)
    _check(load().thr_dense_scan_probe(pd, pi, n, d, pq, nq, ws.data_ptr(), nbytes, _stream()),
           "thr_dense_scan_probe")


def dense_f16_query_tile(dim: int, packed: bool, n_queries: int) -> int:
    return int(load().thr_dense_f16_query_tile(dim, 1 if packed else 0, n_queries))


def dense_f16_max_queries(dim: int, packed: bool) -> int:
    """Largest batch of one thr_dense_topk_f16 call (32-bit candidate-segment offsets)."""
    return int(load().thr_dense_f16_max_queries(dim, 1 if packed else 0))


def dense_anydim_ok(dim: int) -> bool:
    """Row lengths the runtime-dim f16 scan (shortlist="f16-anydim") takes."""
    return THR_DENSE_ANYDIM_STEP <= dim <= THR_DENSE_ANYDIM_MAX and dim % THR_DENSE_ANYDIM_STEP == 0


@contextlib.contextmanager
def dense_f16_flavour(anydim: bool):
    """The f16 calls (docs16 None) made inside run the runtime-dim scan at dim 512 / 768 / 1024 too,
    where the tuned kernel is the default (thr_dense_f16_select: per calling thread, restored on exit);
    at every other length it is the only one and nothing is switched."""
    if not anydim:
        yield
        return
    before = load().thr_dense_f16_select(THR_DENSE_F16_ANYDIM)
    try:
        yield
    finally:
        load().thr_dense_f16_select(before)


def dense_rescue_workspace_bytes(n_queries: int, k: int) -> int:
    return int(load().thr_dense_rescue_workspace_bytes(n_queries, k))


def dense_rescue(docs, dnorm, queries, S, I, cnt, flg, id_base: int = 0,
                 workspace: Optional[torch.Tensor] = None, doc_coll=None, query_coll=None) -> torch.Tensor:
    """Redo, in place and without a host read-back, the queries of a dense_topk[_f16] result
    whose flags lack THR_FLAG_CERTIFIED.  -> device int32[1]: how many were redone."""
    pd, pq, pn, _, _, n, d, nq = _dense_operands(docs, queries, dnorm)
    # the one dense call that writes into tensors the caller made (one test for the four of them,
    # written out: this runs in front of every search step)
    k = I.shape[1] if I.dim() == 2 else 0
    dev, SI, CF = docs.device, (nq, k), (nq,)
    if S.dtype != torch.float64 or I.dtype != torch.int64 or cnt.dtype != torch.int32 or flg.dtype != torch.int32 or \
            S.shape != SI or I.shape != SI or cnt.shape != CF or flg.shape != CF or \
            S.device != dev or I.device != dev or cnt.device != dev or flg.device != dev or \
            not (S.is_contiguous() and I.is_contiguous() and cnt.is_contiguous() and flg.is_contiguous()) or \
            not 1 <= k <= THR_DENSE_MAX_K:
        raise NativeError(f"dense_rescue: S float64 and I int64 [{nq}, k], 1 <= k <= {THR_DENSE_MAX_K}, cnt and flg "
                          f"int32 [{nq}], all contiguous and on docs' device; got " +
                          ", ".join(f"{tuple(t.shape)} {t.dtype} {t.device}" for t in (S, I, cnt, flg)))
    lib = load()
    ws, nbytes = _workspace(workspace, lib.thr_dense_rescue_workspace_bytes(nq, k), dev)
    n_rescued = torch.empty(1, dtype=torch.int32, device=dev)   # (thr_dense_rescue writes the zero)
    pdc, pqc = _coll(doc_coll, query_coll, n, nq)
    _check(lib.thr_dense_rescue(pd, pn, n, d, id_base, pq, nq, k, pdc, pqc, S.data_ptr(), I.data_ptr(),
                                cnt.data_ptr(), flg.data_ptr(), n_rescued.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_dense_rescue")
    return n_rescued


def dense_quantize_f16(docs: torch.Tensor, keep_copy: bool = True):
    """-> (docs16 or None, max relative row error of the rounding as a float).  docs16 is the
    fragment-major float16 image of the rows (opaque; f16 [ceil32(n), D] elements)."""
    p = _dev(docs, torch.float32, "docs", 2)
    n, d = docs.shape
    d16 = None
    if keep_copy:
        nbytes = int(load().thr_dense_f16_copy_bytes(n, d))
        d16 = torch.empty((nbytes // (2 * d), d), dtype=torch.float16, device=docs.device)
    err = torch.zeros(1, dtype=torch.float32, device=docs.device)
    _check(load().thr_dense_quantize_f16(p, n, d, d16.data_ptr() if keep_copy else None,
                                         err.data_ptr(), _stream()), "thr_dense_quantize_f16")
    return d16, float(err.item())


def dense_quantize_f16_into(docs: torch.Tensor, d16: Optional[torch.Tensor], err: torch.Tensor) -> None:
    """thr_dense_quantize_f16 into buffers the caller holds: ``d16`` float16 with room for the
    image of the rows (None: measure only), ``err`` a float32 [1] device slot for the max relative
    row error.  Allocates nothing and reads nothing back (GpuIndex.delete_rows, phase 2)."""
    p = _dev(docs, torch.float32, "docs", 2)
    n, d = docs.shape
    pe = _dev(err, torch.float32, "err", 1)
    ph = None
    if d16 is not None:
        ph = _dev(d16, torch.float16, "d16", 2)
        if d16.shape[1] != d or d16.numel() * 2 < int(load().thr_dense_f16_copy_bytes(n, d)):
            raise NativeError("dense_quantize_f16_into: the float16 destination is too small")
    if err.numel() != 1:
        raise NativeError("dense_quantize_f16_into: err is one float32")
    _check(load().thr_dense_quantize_f16(p, n, d, ph, pe, _stream()), "thr_dense_quantize_f16")


def dense_f16_layout(dim: int) -> str:
    """Tag of the fragment-major layout thr_dense_quantize_f16 writes in this process: the
    register image of the MFMA shape the copy scan runs with (16x16x32, or 32x32x16 under the
    A/B knob THR_DENSE_MFMA=32, which the library reads the same way).  A saved float16 image is
    reused only under the tag it was written with."""
    return f"fragment-major/mfma{32 if os.environ.get('THR_DENSE_MFMA') == '32' else 16}/dim{dim}"


def dense_f16_workspace_bytes(n_docs: int, dim: int, n_queries: int, kprime: int) -> int:
    return int(load().thr_dense_f16_workspace_bytes(n_docs, dim, n_queries, kprime))


def dense_topk_f16(docs, docs16, doc_rel_err: float, dnorm, inv_norm, queries, k: int,
                   kprime: int, id_base: int = 0, workspace: Optional[torch.Tensor] = None,
                   doc_coll=None, query_coll=None):
    pd, pq, pn, pi, ph, n, d, nq = _dense_operands(docs, queries, dnorm, inv_norm, docs16)
    ws, nbytes = _workspace(workspace, dense_f16_workspace_bytes(n, d, nq, kprime), docs.device)
    S, I, cnt, flg = _alloc_out(nq, k, docs.device)
    pdc, pqc = _coll(doc_coll, query_coll, n, nq)
    _check(load().thr_dense_topk_f16(pd, ph, float(doc_rel_err), pn, pi, n, d, id_base, pq, nq, k,
                                     kprime, pdc, pqc, S.data_ptr(), I.data_ptr(), cnt.data_ptr(),
                                     flg.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_dense_topk_f16")
    return S, I, cnt, flg


def _held_workspace(what: str, workspace: torch.Tensor, need: int) -> Tuple[torch.Tensor, int]:
    """The workspace rule for the one that carries the candidate lists from dense_shortlist_f16 to the
    matching dense_finish_f16: the caller's or none -- a too-small one is refused, not replaced."""
    nbytes = 0 if workspace is None else workspace.numel() * workspace.element_size()
    if nbytes < need:
        raise NativeError(f"{what}: workspace smaller than thr_dense_f16_workspace_bytes")
    _dev(workspace, workspace.dtype, "workspace")
    return workspace, nbytes


def dense_shortlist_f16(docs, docs16, doc_rel_err: float, inv_norm, queries, kprime: int, m: int,
                        workspace: torch.Tensor, doc_coll=None, query_coll=None) -> torch.Tensor:
    """First half of the search split around the shards' exchange (thr_hip.h e1): the filter scan
    (candidate lists left in ``workspace``) and per query the ``m`` largest scan scores as lower
    bounds of ||q|| x cosine -> float32 [nq, m], -inf padded."""
    pd, pq, _, pi, ph, n, d, nq = _dense_operands(docs, queries, inv_norm=inv_norm, docs16=docs16)
    ws, nbytes = _held_workspace("shortlist", workspace, dense_f16_workspace_bytes(n, d, nq, kprime))
    pdc, pqc = _coll(doc_coll, query_coll, n, nq)
    lb = torch.empty((nq, m), dtype=torch.float32, device=docs.device)
    _check(load().thr_dense_shortlist_f16(pd, ph, float(doc_rel_err), pi, n, d, pq, nq, kprime, pdc, pqc,
                                          m, lb.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_dense_shortlist_f16")
    return lb


def dense_floor(top_lb: torch.Tensor, k: int) -> torch.Tensor:
    """[n_shards, nq, m] gathered lower bounds -> float32 [nq]: the k-th largest per query, a lower
    bound of ||q|| x the k-th best cosine over all the shards (-inf: no floor)."""
    p = _dev(top_lb, torch.float32, "top_lb", 3)
    g, nq, m = top_lb.shape
    out = torch.empty(nq, dtype=torch.float32, device=top_lb.device)
    _check(load().thr_dense_floor(p, g, nq, m, k, out.data_ptr(), _stream()), "thr_dense_floor")
    return out


def dense_finish_f16(docs, docs16, doc_rel_err: float, dnorm, inv_norm, queries, k: int, kprime: int,
                     gfloor: Optional[torch.Tensor], id_base: int, workspace: torch.Tensor,
                     doc_coll=None, query_coll=None, lb_all: Optional[torch.Tensor] = None):
    """Second half: band, float64 rescoring, order and certificate on the candidate lists the
    matching dense_shortlist_f16 call left in ``workspace`` (same arguments), with the shards'
    common floor: ``gfloor`` [nq] (dense_floor's output), or ``lb_all`` [n_shards, nq, m] -- the
    gathered bounds themselves, the k-th largest found inside the band kernel."""
    pd, pq, pn, pi, ph, n, d, nq = _dense_operands(docs, queries, dnorm, inv_norm, docs16)
    pg = None
    if gfloor is not None:
        pg = _dev(gfloor, torch.float32, "gfloor", 1)
        if gfloor.shape[0] != nq:
            raise NativeError("gfloor: one value per query")
    pl, g, m = None, 0, 0
    if lb_all is not None:
        if gfloor is not None:
            raise NativeError("finish: gfloor or lb_all, not both")
        pl = _dev(lb_all, torch.float32, "lb_all", 3)
        g, nq_l, m = lb_all.shape
        if nq_l != nq:
            raise NativeError("lb_all: [n_shards, nq, m]")
    ws, nbytes = _held_workspace("finish", workspace, dense_f16_workspace_bytes(n, d, nq, kprime))
    S, I, cnt, flg = _alloc_out(nq, k, docs.device)
    pdc, pqc = _coll(doc_coll, query_coll, n, nq)
    _check(load().thr_dense_finish_f16(pd, ph, float(doc_rel_err), pn, pi, n, d, id_base, pq, nq, k,
                                       kprime, pdc, pqc, pg, pl, g, m, S.data_ptr(), I.data_ptr(),
                                       cnt.data_ptr(), flg.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_dense_finish_f16")
    return S, I, cnt, flg


def dense_scan_probe_f16(docs, docs16, inv_norm, queries, workspace: torch.Tensor) -> None:
    pd, pq, _, pi, ph, n, d, nq = _dense_operands(docs, queries, inv_norm=inv_norm, docs16=docs16)
    ws, nbytes = _workspace(workspace, 0, docs.device)      # (the caller's as it is: the library judges its size)
    _check(load().thr_dense_scan_probe_f16(pd, ph, pi, n, d, pq, nq, ws.data_ptr(), nbytes, _stream()),
           "thr_dense_scan_probe_f16")


def dense_scan_stamps_f16(docs16, n_docs: int, queries_n: int, workspace: torch.Tensor):
    """Phase stamps of the float16-copy scan -> int64 [n_waves, 8] (see thr_hip.h)."""
    ph = _dev(docs16, torch.float16, "docs16", 2)
    d = docs16.shape[1]
    ws, nbytes = _workspace(workspace, 0, docs16.device)    # (as the probes: the library judges its size)
    pw = ws.data_ptr()
    nw = C.c_int(0)
    _check(load().thr_dense_scan_stamps_f16(ph, n_docs, d, queries_n, pw, nbytes, None, C.byref(nw),
                                            _stream()), "thr_dense_scan_stamps_f16")
    out = torch.zeros((nw.value, 8), dtype=torch.int64, device=docs16.device)
    _check(load().thr_dense_scan_stamps_f16(ph, n_docs, d, queries_n, pw, nbytes, out.data_ptr(),
                                            C.byref(nw), _stream()), "thr_dense_scan_stamps_f16")
    return out


# --------------------------------------------------------------------- f1
def lexical_build(doc: torch.Tensor, term: torch.Tensor, tf: Optional[torch.Tensor], n_docs: int,
                  n_vocab: int, workspace: Optional[torch.Tensor] = None):
    """Tokenised rows on the device -> (rowptr i64 [V+1], post_doc i32 [nnz], post_tf i32 [nnz],
    doclen f32 [n_docs], df i64 [V]): the CSR inverted index of this shard.  ``tf`` None: one
    entry per token occurrence.  One host read-back at the end (the number of postings, to cut
    the posting arrays to size).  ``workspace``: reused when large enough (_workspace)."""
    pdoc = _dev(doc, torch.int32, "doc", 1)
    pterm = _dev(term, torch.int32, "term", 1)
    ptf = _dev(tf, torch.int32, "tf", 1) if tf is not None else None
    n = doc.shape[0]
    if term.shape[0] != n or (tf is not None and tf.shape[0] != n):
        raise NativeError("lexical_build: doc / term / tf lengths differ")
    dev = doc.device
    rowptr = torch.empty(n_vocab + 1, dtype=torch.int64, device=dev)
    post_doc = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    post_tf = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
    doclen = torch.empty(n_docs, dtype=torch.float32, device=dev)
    df = torch.empty(n_vocab, dtype=torch.int64, device=dev)
    nnz = torch.zeros(1, dtype=torch.int64, device=dev)
    if n == 0:
        return rowptr.zero_(), post_doc[:0], post_tf[:0], doclen.zero_(), df.zero_()
    ws, nbytes = _workspace(workspace, int(load().thr_lexical_build_workspace_bytes(n, n_vocab)), dev)
    _check(load().thr_lexical_build(pdoc, pterm, ptf, n, n_docs, n_vocab, rowptr.data_ptr(),
                                    post_doc.data_ptr(), post_tf.data_ptr(), doclen.data_ptr(),
                                    df.data_ptr(), nnz.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_lexical_build")
    k = int(nnz.item())
    return rowptr, post_doc[:k].clone(), post_tf[:k].clone(), doclen, df


# --------------------------------------------------------------------- f2
def csr_append(rowptr_a, a0, a1, rowptr_b, b0, b1, out0=None, out1=None):
    """Segmented concatenation of two CSRs over one row space (thr_csr_append): row t of the
    result is A's row t followed by B's.  ``rowptr_a`` int64 [rows_a + 1] or None (an empty A),
    ``rowptr_b`` int64 [rows_b + 1], rows_b >= rows_a; payloads are 4-byte tensors [nnz] (int32 /
    float32), the second of each pair optional.  ``out0`` / ``out1``: capacity-reserved 1-d
    destinations of the payloads' dtypes (allocated to size when None) -- the first
    nnz_a + nnz_b elements are written.  -> (rowptr_out, out0, out1 or None, nnz)."""
    rows_a = 0 if rowptr_a is None else rowptr_a.shape[0] - 1
    rows_b = rowptr_b.shape[0] - 1
    pra = _dev(rowptr_a, torch.int64, "rowptr_a", 1)
    prb = _dev(rowptr_b, torch.int64, "rowptr_b", 1)
    if rows_b < max(rows_a, 1):
        raise NativeError(f"csr_append: B has {rows_b} rows, A has {rows_a} (rows only grow)")
    if b0.dtype.itemsize != 4 or (a0 is not None and a0.dtype != b0.dtype):
        raise NativeError("csr_append: payloads are 4-byte elements of one dtype per array")
    if a0 is not None and (a1 is None) != (b1 is None):
        raise NativeError("csr_append: A and B carry the same number of payload arrays")
    if b1 is not None and (b1.dtype.itemsize != 4 or (a1 is not None and a1.dtype != b1.dtype)):
        raise NativeError("csr_append: payloads are 4-byte elements of one dtype per array")
    nnz_a = 0 if a0 is None else a0.shape[0]
    nnz_b = b0.shape[0]
    if (a1 is not None and a1.shape[0] != nnz_a) or (b1 is not None and b1.shape[0] != nnz_b):
        raise NativeError("csr_append: the payloads of one CSR have one length")
    dev = rowptr_b.device
    nnz = nnz_a + nnz_b
    if out0 is None:
        out0 = torch.empty(nnz, dtype=b0.dtype, device=dev)
    if out1 is None and b1 is not None:
        out1 = torch.empty(nnz, dtype=b1.dtype, device=dev)
    if out0.dtype != b0.dtype or out0.shape[0] < nnz or \
            (b1 is not None and (out1.dtype != b1.dtype or out1.shape[0] < nnz)):
        raise NativeError("csr_append: destination too small or of another dtype")
    rowptr_out = torch.empty(rows_b + 1, dtype=torch.int64, device=dev)
    cap = out0.shape[0] if b1 is None else min(out0.shape[0], out1.shape[0])
    _check(load().thr_csr_append(pra, rows_a, nnz_a, _dev(a0, b0.dtype, "a0", 1) if nnz_a else None,
                                 _dev(a1, b1.dtype, "a1", 1) if nnz_a and b1 is not None else None,
                                 prb, rows_b, nnz_b, _dev(b0, b0.dtype, "b0", 1) if nnz_b else None,
                                 _dev(b1, b1.dtype, "b1", 1) if nnz_b and b1 is not None else None,
                                 rowptr_out.data_ptr(), _dev(out0, b0.dtype, "out0", 1) if nnz else None,
                                 _dev(out1, b1.dtype, "out1", 1) if nnz and b1 is not None else None,
                                 cap, _stream()), "thr_csr_append")
    return rowptr_out, out0, (out1 if b1 is not None else None), nnz


def csr_compact(rowptr, ids, pay, remap, id_base: int = 0, ids_out=None, pay_out=None, workspace=None):
    """Order-preserving removal of entries from a CSR, with renumbering (thr_csr_compact): entry p
    is kept iff ``remap[ids[p] - id_base] >= 0`` (ids outside [id_base, id_base + len(remap)) are
    dropped) and is written as ``remap[...] + id_base``.  ``rowptr`` int64 [rows + 1], ``ids`` int32
    [nnz], ``pay`` a 4-byte tensor [nnz] or None, ``remap`` int32 [n_ids] (-1 = deleted, ascending over
    the survivors).  ``ids_out`` / ``pay_out``: capacity-reserved 1-d destinations of the payloads'
    dtypes with room for all nnz entries (the kept count is not known before the call; allocated
    when None) -- only the kept entries are written.  One host read-back at the end (the kept
    count).  ``workspace``: reused when large enough (_workspace).
    -> (rowptr_out, ids_out, pay_out or None, nnz_kept)."""
    # (shapes and dtypes first: they are refused on any device, before a pointer is taken)
    rows, nnz = rowptr.shape[0] - 1, ids.shape[0]
    if rows < 1:
        raise NativeError("csr_compact: rowptr has no rows")
    if id_base < 0:
        raise NativeError("csr_compact: id_base is negative")
    if pay is not None and (pay.dtype.itemsize != 4 or pay.dim() != 1 or pay.shape[0] != nnz):
        raise NativeError("csr_compact: the payload is a 1-d array of 4-byte elements, one per id")
    if pay is None and pay_out is not None:
        raise NativeError("csr_compact: pay_out without a payload")
    for out, like, name in ((ids_out, ids, "ids_out"), (pay_out, pay, "pay_out")):
        if out is not None and (out.dtype != like.dtype or out.dim() != 1 or out.shape[0] < nnz):
            raise NativeError(f"csr_compact: {name} is too small (room for every entry is needed) or of another dtype")
    prp = _dev(rowptr, torch.int64, "rowptr", 1)
    pid = _dev(ids, torch.int32, "ids", 1)
    prm = _dev(remap, torch.int32, "remap", 1)
    dev = ids.device
    if ids_out is None:
        ids_out = torch.empty(nnz, dtype=torch.int32, device=dev)
    if pay_out is None and pay is not None:
        pay_out = torch.empty(nnz, dtype=pay.dtype, device=dev)
    rowptr_out = torch.empty(rows + 1, dtype=torch.int64, device=dev)
    kept = torch.zeros(1, dtype=torch.int64, device=dev)
    ws, nbytes = _workspace(workspace, int(load().thr_csr_compact_workspace_bytes(rows, nnz)), dev)
    cap = ids_out.shape[0] if pay is None else min(ids_out.shape[0], pay_out.shape[0])
    _check(load().thr_csr_compact(prp, rows, nnz, pid if nnz else None,
                                  _dev(pay, pay.dtype, "pay", 1) if nnz and pay is not None else None,
                                  prm if remap.shape[0] else None, remap.shape[0], int(id_base),
                                  rowptr_out.data_ptr(), _dev(ids_out, torch.int32, "ids_out", 1) if nnz else None,
                                  _dev(pay_out, pay.dtype, "pay_out", 1) if nnz and pay is not None else None,
                                  cap, kept.data_ptr(), ws.data_ptr(), nbytes, _stream()), "thr_csr_compact")
    return rowptr_out, ids_out, (pay_out if pay is not None else None), int(kept.item())


def csr_merge_status_message(status: int) -> Optional[str]:
    """What a non-zero status word of thr_csr_merge says, or None."""
    if not status:
        return None
    said = []
    if status & (THR_CSR_MERGE_UNSORTED_A | THR_CSR_MERGE_UNSORTED_B):
        who = " and ".join(n for n, b in (("A (the index's rows)", THR_CSR_MERGE_UNSORTED_A),
                                          ("B (the batch)", THR_CSR_MERGE_UNSORTED_B)) if status & b)
        said.append(f"{who} not in build_graph's canonical form (ids ascending within a row; "
                    "for relations strictly: no duplicate edge)")
    if status & THR_CSR_MERGE_OVERFLOW:
        said.append("the result does not fit the destination (out_capacity)")
    return "; ".join(said)


def csr_merge(rowptr_a, ids_a, pay_a, rowptr_b, ids_b, pay_b, drop_present: bool, ids_out=None, pay_out=None,
              workspace=None, check: bool = True):
    """Row-wise stable merge of two CSRs over one row space (thr_csr_merge): row t of the result is
    the merge of A's and B's row t by id, A first on equal ids.  ``rowptr_a`` int64 [rows_a + 1] or
    None (an empty A), ``rowptr_b`` int64 [rows_b + 1], rows_b >= rows_a; ``ids_*`` int32 [nnz],
    ``pay_*`` 4-byte tensors [nnz] of one dtype, on both sides or on neither.  ``drop_present``: the
    set union (a B entry whose id is in A's row is dropped; both sides strictly ascending within a
    row), else the multiset merge.  ``ids_out`` / ``pay_out``: capacity-reserved 1-d destinations
    (allocated for nnz_a + nnz_b when None); ``workspace``: reused when large enough (_workspace).  One
    host read-back at the end (the count and the status word).  ``check``: raise NativeError on a
    non-zero status (inputs not in canonical form, destination too small) instead of returning it.
    -> (rowptr_out, ids_out, pay_out or None, nnz_out, status)."""
    rows_a = 0 if rowptr_a is None else rowptr_a.shape[0] - 1
    rows_b = rowptr_b.shape[0] - 1
    if rows_b < rows_a or rows_b < 0:
        raise NativeError(f"csr_merge: B has {rows_b} rows, A has {rows_a} (rows only grow)")
    nnz_a = 0 if ids_a is None else ids_a.shape[0]
    nnz_b = 0 if ids_b is None else ids_b.shape[0]
    if (pay_a is not None and ids_a is None) or (pay_b is not None and ids_b is None):
        raise NativeError("csr_merge: a payload without ids")
    if (ids_a is not None and ids_b is not None and (pay_a is None) != (pay_b is None)) or \
            (pay_out is not None and pay_a is None and pay_b is None):
        raise NativeError("csr_merge: a payload travels on both sides or on neither")
    pay_like = pay_a if pay_a is not None else pay_b
    for pay, n, name in ((pay_a, nnz_a, "pay_a"), (pay_b, nnz_b, "pay_b")):
        if pay is not None and (pay.dtype.itemsize != 4 or pay.dim() != 1 or pay.shape[0] != n or
                                pay.dtype != pay_like.dtype):
            raise NativeError(f"csr_merge: {name} is a 1-d array of 4-byte elements of one dtype, one per id")
    for out, like, name in ((ids_out, torch.int32, "ids_out"),
                            (pay_out, None if pay_like is None else pay_like.dtype, "pay_out")):
        if out is not None and (out.dtype != like or out.dim() != 1):
            raise NativeError(f"csr_merge: {name} is a 1-d array of the source's dtype")
    pra = _dev(rowptr_a, torch.int64, "rowptr_a", 1)
    prb = _dev(rowptr_b, torch.int64, "rowptr_b", 1)
    pia = _dev(ids_a, torch.int32, "ids_a", 1)
    pib = _dev(ids_b, torch.int32, "ids_b", 1)
    dev = rowptr_b.device
    if ids_out is None:
        ids_out = torch.empty(nnz_a + nnz_b, dtype=torch.int32, device=dev)
    if pay_out is None and pay_like is not None:
        pay_out = torch.empty(nnz_a + nnz_b, dtype=pay_like.dtype, device=dev)
    rowptr_out = torch.empty(rows_b + 1, dtype=torch.int64, device=dev)
    tail = torch.zeros(2, dtype=torch.int64, device=dev)      # *nnz_out, *status_out
    ws, nbytes = _workspace(workspace, int(load().thr_csr_merge_workspace_bytes(rows_b, nnz_a, nnz_b)), dev)
    cap = ids_out.shape[0] if pay_like is None else min(ids_out.shape[0], pay_out.shape[0])
    has = pay_like is not None
    _check(load().thr_csr_merge(pra if rows_a else None, rows_a, nnz_a, pia if nnz_a else None,
                                _dev(pay_a, pay_like.dtype, "pay_a", 1) if nnz_a and has else None,
                                prb, rows_b, nnz_b, pib if nnz_b else None,
                                _dev(pay_b, pay_like.dtype, "pay_b", 1) if nnz_b and has else None,
                                1 if drop_present else 0, rowptr_out.data_ptr(),
                                _dev(ids_out, torch.int32, "ids_out", 1) if cap else None,
                                _dev(pay_out, pay_like.dtype, "pay_out", 1) if has and cap else None,
                                cap, tail.data_ptr(), tail.data_ptr() + 8, ws.data_ptr(), nbytes, _stream()),
           "thr_csr_merge")
    nnz_out, status = (int(v) for v in tail.tolist())
    status &= 0xFFFFFFFF
    if check and status:
        raise NativeError("csr_merge: " + csr_merge_status_message(status))
    return rowptr_out, ids_out, (pay_out if has else None), nnz_out, status


def csr_prune_workspace_bytes(rows_a: int, nnz_a: int) -> int:
    return int(load().thr_csr_prune_workspace_bytes(int(rows_a), int(nnz_a)))


def csr_prune_status_message(status: int) -> Optional[str]:
    """What a non-zero status word of thr_csr_prune says, or None."""
    if not status:
        return None
    said = []
    if status & CSR_PRUNE_UNSORTED_B:
        said.append("B (the pairs to drop) is not strictly ascending within a row")
    if status & CSR_PRUNE_OVERFLOW:
        said.append("the result does not fit the destination (out_capacity)")
    if status & CSR_PRUNE_BAD_ROW:
        said.append("row_remap names a row outside the result (rows_out)")
    return "; ".join(said)


def csr_prune(rowptr_a, ids_a, pay_a=None, row_remap=None, rows_out: Optional[int] = None, id_remap=None,
              id_base: int = 0, rowptr_b=None, ids_b=None, ids_out=None, pay_out=None, want_keep: bool = False,
              workspace=None, check: bool = True):
    """One order-preserving pass over a CSR that drops rows, entries by id and (row, id) pairs
    (thr_csr_prune).  ``rowptr_a`` int64 [rows_a + 1], ``ids_a`` int32 [nnz_a], ``pay_a`` a 4-byte tensor
    [nnz_a] or None.  ``row_remap`` int32 [rows_a] or None: the new row of old row t, -1 = removed with
    everything in it, ascending over the survivors 0 .. rows_out - 1 (``rows_out`` is required with it;
    without it every row stays).  ``id_remap`` int32 [n_ids] or None with ``id_base``: as csr_compact;
    None: ids pass through untouched and unchecked.  ``rowptr_b`` / ``ids_b``: a CSR over A's rows,
    strictly ascending within a row, in A's old numbering -- an entry of A's row t whose id is in B's
    row t is dropped -- or None.  ``ids_out`` / ``pay_out``: capacity-reserved 1-d destinations (allocated
    for nnz_a when None); ``want_keep``: also return the uint8 [nnz_a] keep mask; ``workspace``: reused when
    large enough (_workspace).  One host read-back at the end (the count and the status word).  ``check``:
    raise NativeError on a non-zero status instead of returning it.
    -> (rowptr_out, ids_out, pay_out or None, nnz_out, status, keep or None)."""
    rows_a, nnz_a = rowptr_a.shape[0] - 1, ids_a.shape[0]
    if rows_a < 0:
        raise NativeError("csr_prune: rowptr_a has no entry")
    if row_remap is None:
        if rows_out is not None and int(rows_out) != rows_a:
            raise NativeError("csr_prune: rows_out differs from A's row count, and no row_remap says which rows leave")
        rows_out = rows_a
    else:
        if rows_out is None:
            raise NativeError("csr_prune: row_remap needs rows_out")
        if row_remap.dim() != 1 or row_remap.shape[0] != rows_a:
            raise NativeError("csr_prune: row_remap holds one entry per row of A")
    rows_out = int(rows_out)
    if rows_out < 0 or rows_out > rows_a:
        raise NativeError(f"csr_prune: rows_out is {rows_out}, A has {rows_a} rows")
    if id_base < 0:
        raise NativeError("csr_prune: id_base is negative")
    if pay_a is not None and (pay_a.dtype.itemsize != 4 or pay_a.dim() != 1 or pay_a.shape[0] != nnz_a):
        raise NativeError("csr_prune: the payload is a 1-d array of 4-byte elements, one per id")
    if pay_a is None and pay_out is not None:
        raise NativeError("csr_prune: pay_out without a payload")
    if (rowptr_b is None) != (ids_b is None):
        raise NativeError("csr_prune: B is row pointers and ids, or neither")
    if rowptr_b is not None and (rowptr_b.dim() != 1 or rowptr_b.shape[0] != rows_a + 1):
        raise NativeError("csr_prune: rowptr_b holds one entry per row of A and one more")
    for out, like, name in ((ids_out, torch.int32, "ids_out"), (pay_out, None if pay_a is None else pay_a.dtype, "pay_out")):
        if out is not None and (out.dtype != like or out.dim() != 1):
            raise NativeError(f"csr_prune: {name} is a 1-d array of the source's dtype")
    pra = _dev(rowptr_a, torch.int64, "rowptr_a", 1)
    pia = _dev(ids_a, torch.int32, "ids_a", 1)
    prr = _dev(row_remap, torch.int32, "row_remap", 1)
    pir = _dev(id_remap, torch.int32, "id_remap", 1)
    prb = _dev(rowptr_b, torch.int64, "rowptr_b", 1)
    pib = _dev(ids_b, torch.int32, "ids_b", 1)
    dev = rowptr_a.device
    has = pay_a is not None
    if ids_out is None:
        ids_out = torch.empty(nnz_a, dtype=torch.int32, device=dev)
    if pay_out is None and has:
        pay_out = torch.empty(nnz_a, dtype=pay_a.dtype, device=dev)
    rowptr_out = torch.empty(rows_out + 1, dtype=torch.int64, device=dev)
    keep = torch.empty(nnz_a, dtype=torch.uint8, device=dev) if want_keep else None
    tail = torch.zeros(2, dtype=torch.int64, device=dev)      # *nnz_out, *status_out
    ws, nbytes = _workspace(workspace, csr_prune_workspace_bytes(rows_a, nnz_a), dev)
    cap = ids_out.shape[0] if not has else min(ids_out.shape[0], pay_out.shape[0])
    n_ids = 0 if id_remap is None else id_remap.shape[0]
    nnz_b = 0 if ids_b is None else ids_b.shape[0]
    if id_remap is not None and n_ids == 0:
        raise NativeError("csr_prune: an empty id_remap (pass None to let every id through)")
    _check(load().thr_csr_prune(pra if rows_a else None, rows_a, nnz_a, pia if nnz_a else None,
                                _dev(pay_a, pay_a.dtype, "pay_a", 1) if has and nnz_a else None,
                                prr if row_remap is not None and rows_a else None, rows_out,
                                pir if n_ids else None, n_ids, int(id_base),
                                prb if rowptr_b is not None else None, nnz_b, pib if nnz_b else None,
                                rowptr_out.data_ptr(), _dev(ids_out, torch.int32, "ids_out", 1) if nnz_a else None,
                                _dev(pay_out, pay_a.dtype, "pay_out", 1) if has and nnz_a else None, cap,
                                keep.data_ptr() if want_keep and nnz_a else None,
                                tail.data_ptr(), tail.data_ptr() + 8, ws.data_ptr(), nbytes, _stream()),
           "thr_csr_prune")
    nnz_out, status = (int(v) for v in tail.tolist())
    status &= 0xFFFFFFFF
    if check and status:
        raise NativeError("csr_prune: " + csr_prune_status_message(status))
    return rowptr_out, ids_out, (pay_out if has else None), nnz_out, status, keep


# --------------------------------------------------------------------- f4
def scope_resolve(cols, preds, cap: Optional[int] = None, want_labels: bool = True, rows_out=None, workspace=None):
    """thr_scope_resolve: ``cols`` a sequence of C int32 [n_docs] device columns, ``preds`` int32
    [P, C] (-1 = any value, below -1 = no row).  -> (rowptr i64 [P + 1], rows i32 [cap], labels i32
    [n_docs] or None, overlap i32 [1] or None).  ``cap`` (default n_docs; 0 = counts and labels only)
    is the room for the lists: rowptr is complete either way and the caller compares rowptr[P] with
    cap before it reads ``rows``.  ``rows_out``: an int32 buffer of at least cap entries to write the
    lists into (returned as ``rows``; nothing behind cap is written).  ``workspace``: reused when large
    enough (_workspace).  No host read-back."""
    cols, n = _scope_columns("scope_resolve", cols)
    if preds.dim() != 2 or preds.shape[1] != len(cols):
        raise NativeError(f"scope_resolve: preds must be [P, {len(cols)}]")
    P = preds.shape[0]
    if not 1 <= P <= THR_SCOPE_MAX_PREDS:
        raise NativeError(f"scope_resolve: 1 .. {THR_SCOPE_MAX_PREDS} predicates per call, got {P}")
    cap = _scope_cap("scope_resolve", cap, n)
    lib = load()
    return _scope_call("scope_resolve", lib.thr_scope_resolve, lib.thr_scope_resolve_workspace_bytes, cols, n,
                       lambda: (_dev(preds, torch.int32, "preds", 2), P), P, cap, want_labels, preds.device, rows_out,
                       workspace)


def _scope_columns(what: str, cols):
    """The column checks the two scope calls share, made before any device pointer is taken (they are
    refused on any device) -> (cols as a list, n_docs)."""
    cols = list(cols)
    if not 1 <= len(cols) <= THR_SCOPE_MAX_COLS:
        raise NativeError(f"{what}: 1 .. {THR_SCOPE_MAX_COLS} attribute columns, got {len(cols)}")
    n = cols[0].shape[0]
    if any(c.dim() != 1 or c.shape[0] != n for c in cols):
        raise NativeError(f"{what}: every column is 1-d of the same length")
    return cols, n


def _scope_cap(what: str, cap: Optional[int], n: int) -> int:
    cap = n if cap is None else int(cap)
    if cap < 0:
        raise NativeError(f"{what}: cap is negative")
    return cap


def _scope_call(what: str, entry, workspace_bytes, cols, n: int, table, P: int, cap: int, want_labels: bool, dev,
                rows_out=None, workspace=None):
    """The device half the two scope calls share: column pointers, outputs, workspace and the call of
    ``entry`` (thr_<what>; ``workspace_bytes`` its size function).  ``table()`` -> the entry's
    predicate-table arguments (pointers of device tensors and counts), taken behind the columns'."""
    ptrs = (C.c_void_p * len(cols))(*[_dev(c, torch.int32, "column", 1) for c in cols])
    table = table()
    rowptr = torch.empty(P + 1, dtype=torch.int64, device=dev)
    if rows_out is not None:
        if rows_out.dim() != 1 or rows_out.shape[0] < cap:
            raise NativeError(f"{what}: rows_out holds fewer than cap entries")
        _dev(rows_out, torch.int32, "rows_out", 1)
    rows = torch.empty(cap, dtype=torch.int32, device=dev) if rows_out is None else rows_out
    labels = torch.empty(n, dtype=torch.int32, device=dev) if want_labels else None
    overlap = torch.empty(1, dtype=torch.int32, device=dev) if want_labels else None
    ws, nbytes = _workspace(workspace, workspace_bytes(n, P), dev)
    _check(entry(ptrs, len(cols), n, *table, rowptr.data_ptr(), rows.data_ptr() if cap else None, cap,
                 labels.data_ptr() if want_labels else None, overlap.data_ptr() if want_labels else None,
                 ws.data_ptr(), nbytes, _stream()), f"thr_{what}")
    return rowptr, rows, labels, overlap


def scope_check_clauses(clauses, set_values, n_cols: int):
    """The host validation of a clause table before its upload -> (int32 [P, C, 4], int32 [n_set]) numpy,
    contiguous.  Refused: a kind outside any / none / range / set (+ negated), a range with a > b or
    a < 0, a set whose window leaves set_values or is empty, or whose members are not ascending,
    distinct and >= 0."""
    import numpy as np
    tab = np.ascontiguousarray(clauses, dtype=np.int32)
    sv = np.ascontiguousarray(np.zeros(0, np.int32) if set_values is None else set_values, dtype=np.int32).reshape(-1)
    if tab.ndim != 3 or tab.shape[1] != n_cols or tab.shape[2] != 4:
        raise NativeError(f"scope_resolve_clauses: clauses must be [P, {n_cols}, 4]")
    P = tab.shape[0]
    if not 1 <= P <= THR_SCOPE_MAX_PREDS:
        raise NativeError(f"scope_resolve_clauses: 1 .. {THR_SCOPE_MAX_PREDS} predicates per call, got {P}")
    if sv.shape[0] > THR_SCOPE_MAX_SET_VALUES:
        raise NativeError(f"scope_resolve_clauses: at most {THR_SCOPE_MAX_SET_VALUES} set values per call, got {sv.shape[0]}")
    kind, a, b = tab[..., 0], tab[..., 1].astype(np.int64), tab[..., 2].astype(np.int64)
    base = kind & ~SCOPE_NEGATED
    known = (kind == SCOPE_ANY) | (kind == SCOPE_NONE) | (((base == SCOPE_RANGE) | (base == SCOPE_SET)) & (kind >= 0) & (kind < 8))
    if not known.all():
        raise NativeError(f"scope_resolve_clauses: unknown clause kind {int(kind[~known][0])}")
    rng = base == SCOPE_RANGE
    if (rng & ((a > b) | (a < 0))).any():
        raise NativeError("scope_resolve_clauses: a range clause needs 0 <= a <= b")
    sets = base == SCOPE_SET
    if (sets & ((a < 0) | (b < 1) | (a + b > sv.shape[0]))).any():
        raise NativeError(f"scope_resolve_clauses: a set clause's offset / length leaves the {sv.shape[0]} set values")
    if sv.shape[0] and int(sv.min()) < 0:
        raise NativeError("scope_resolve_clauses: set values are >= 0")
    if sets.any() and sv.shape[0] > 1:
        rising = np.concatenate([[0], np.cumsum(np.diff(sv) <= 0)])     # breaks of the ascent before each position
        lo, hi = a[sets], a[sets] + b[sets] - 1
        if (rising[hi] != rising[lo]).any():
            raise NativeError("scope_resolve_clauses: the values of a set are ascending and distinct")
    return tab, sv


def scope_resolve_clauses(cols, clauses, set_values=None, cap: Optional[int] = None, want_labels: bool = True,
                          workspace=None):
    """thr_scope_resolve_clauses: scope_resolve over predicates of CLAUSES.  ``clauses`` int32 [P, C, 4]
    and ``set_values`` int32 [n] are HOST numpy arrays: they are validated here (scope_check_clauses:
    the device cannot be asked) and uploaded.  ``workspace``: as scope_resolve's.
    -> scope_resolve's (rowptr, rows, labels, overlap)."""
    cols, n = _scope_columns("scope_resolve_clauses", cols)
    if isinstance(clauses, torch.Tensor) or isinstance(set_values, torch.Tensor):
        raise NativeError("scope_resolve_clauses: the clause table and the set values are host numpy arrays")
    tab, sv = scope_check_clauses(clauses, set_values, len(cols))
    P = tab.shape[0]
    cap = _scope_cap("scope_resolve_clauses", cap, n)
    dev = cols[0].device
    dtab = torch.from_numpy(tab).to(dev)
    dsv = torch.from_numpy(sv).to(dev) if sv.shape[0] else None
    lib = load()
    return _scope_call("scope_resolve_clauses", lib.thr_scope_resolve_clauses,
                       lib.thr_scope_resolve_clauses_workspace_bytes, cols, n,
                       lambda: (dtab.data_ptr(), P, dsv.data_ptr() if dsv is not None else None, sv.shape[0]), P, cap,
                       want_labels, dev, None, workspace)


def dense_topk_rows(docs, dnorm, queries, k: int, rowptr, rows, query_scope, id_base: int = 0,
                    workspace: Optional[torch.Tensor] = None):
    """thr_dense_topk_rows: exact cosine top-k of every query over the row list of its scope
    (rowptr i64 [P + 1] / rows i32 of scope_resolve, query_scope i32 [nq] in [0, P), anything else =
    no rows).  ``workspace``: reused when large enough (_workspace).
    -> (scores f64 [nq,k], ids i64 [nq,k], counts i32 [nq], flags i32 [nq])."""
    pd, pq, pn, _, _, n, d, nq = _dense_operands(docs, queries, dnorm)
    P = rowptr.shape[0] - 1
    if not 1 <= P <= THR_SCOPE_MAX_PREDS:
        raise NativeError(f"dense_topk_rows: 1 .. {THR_SCOPE_MAX_PREDS} scopes")
    if query_scope.shape != (nq,):
        raise NativeError("dense_topk_rows: query_scope has the wrong length")
    if not 1 <= k <= THR_DENSE_MAX_K:
        raise NativeError(f"dense_topk_rows: k must be 1 .. {THR_DENSE_MAX_K}")
    prp = _dev(rowptr, torch.int64, "rowptr", 1)
    prw = _dev(rows, torch.int32, "rows", 1)
    pqs = _dev(query_scope, torch.int32, "query_scope", 1)
    ws, nbytes = _workspace(workspace, int(load().thr_dense_topk_rows_workspace_bytes(nq, P, k)), docs.device)
    S, I, cnt, flg = _alloc_out(nq, k, docs.device)
    _check(load().thr_dense_topk_rows(pd, pn, n, d, int(id_base), pq, nq, k, prp, prw if rows.shape[0] else None,
                                      rows.shape[0], P, pqs, S.data_ptr(), I.data_ptr(), cnt.data_ptr(),
                                      flg.data_ptr(), ws.data_ptr(), nbytes, _stream()), "thr_dense_topk_rows")
    return S, I, cnt, flg


# --------------------------------------------------------------------- a3
def bm25_bounds(rowptr, post_doc, post_tf, doclen, idf, avgdl: float, k1: float = 1.2,
                b: float = 0.75):
    """Index set-up -> (term_ub f64 [V], block_ub f64 [ceil(nnz/128)], post_imp u8 [nnz]): the
    upper bounds thr_bm25_topk prunes with (per term, per 128 postings, per posting)."""
    pr = _dev(rowptr, torch.int64, "rowptr", 1)
    pdoc = _dev(post_doc, torch.int32, "post_doc", 1)
    ptf = _dev(post_tf, torch.int32, "post_tf", 1)
    pdl = _dev(doclen, torch.float32, "doclen", 1)
    pidf = _dev(idf, torch.float64, "idf", 1)
    v, nnz = idf.shape[0], post_doc.shape[0]
    tub = torch.zeros(v, dtype=torch.float64, device=rowptr.device)
    bub = torch.zeros(max(int(load().thr_bm25_block_count(nnz)), 1), dtype=torch.float64,
                      device=rowptr.device)
    imp = torch.zeros(nnz + 4, dtype=torch.uint8, device=rowptr.device)   # (+4: read as aligned 32-bit words)
    if nnz:
        _check(load().thr_bm25_bounds(pr, pdoc, ptf, pdl, pidf, avgdl, k1, b, v, nnz, tub.data_ptr(),
                                      bub.data_ptr(), imp.data_ptr(), _stream()), "thr_bm25_bounds")
    return tub, bub, imp


def bm25_dense_terms(rowptr, post_doc, post_tf, post_imp, n_docs: int, min_share: float = 0.125,
                     max_terms: int = 512, max_bytes: int = 12 << 30):
    """Index set-up -> (dense_slot i32 [V], dense_imp u8 [T, stride], dense_tf u16 [T, stride],
    stride) for the terms held by at least ``min_share`` of the docs (the ``max_terms`` longest
    of them, term frequencies <= 65535), or None when there is none: per-doc rows of impacts and
    term frequencies, so that thr_bm25_topk never walks a stop word's postings.  At most
    ``max_bytes`` of rows (12 GiB: 400 terms of a 10M-doc shard)."""
    _dev(rowptr, torch.int64, "rowptr", 1)
    df = rowptr[1:] - rowptr[:-1]
    cand = torch.nonzero(df.to(torch.float64) >= min_share * n_docs).flatten()
    if cand.numel() == 0 or n_docs <= 0:
        return None
    # 3 bytes per doc and term: the longest lists first, as many as ``max_bytes`` holds
    max_terms = min(max_terms, max_bytes // (3 * int(load().thr_bm25_dense_stride(n_docs))))
    if max_terms <= 0:
        return None
    keep = []
    for t in cand[torch.argsort(df[cand], descending=True, stable=True)][:max_terms].tolist():
        lo, hi = int(rowptr[t]), int(rowptr[t + 1])
        if int(post_tf[lo:hi].max()) <= 65535:
            keep.append(t)
    if not keep:
        return None
    terms = torch.tensor(sorted(keep), dtype=torch.int32, device=rowptr.device)
    stride = int(load().thr_bm25_dense_stride(n_docs))
    dimp = torch.empty((len(keep), stride), dtype=torch.uint8, device=rowptr.device)
    dtf = torch.empty((len(keep), stride), dtype=torch.int16, device=rowptr.device)   # (read as uint16)
    _check(load().thr_bm25_dense_rows(_dev(rowptr, torch.int64, "rowptr", 1), _dev(post_doc, torch.int32, "post_doc", 1),
                                      _dev(post_tf, torch.int32, "post_tf", 1), _dev(post_imp, torch.uint8, "post_imp", 1),
                                      terms.data_ptr(), len(keep), n_docs, int(df[terms.long()].max()),
                                      dimp.data_ptr(), dtf.data_ptr(), _stream()), "thr_bm25_dense_rows")
    slot = torch.full((rowptr.shape[0] - 1,), -1, dtype=torch.int32, device=rowptr.device)
    slot[terms.long()] = torch.arange(len(keep), dtype=torch.int32, device=rowptr.device)
    return slot, dimp, dtf, stride


def bm25_workspace_bytes(n_queries: int, max_terms: int, k: int) -> int:
    return int(load().thr_bm25_workspace_bytes(n_queries, max_terms, k))


def bm25_check_batch(n_queries: int) -> None:
    """One thr_bm25_topk call takes at most THR_BM25_MAX_QUERIES queries (its item counts are 32 bits)."""
    if n_queries > THR_BM25_MAX_QUERIES:
        raise NativeError(f"bm25: {n_queries} queries in one call, the limit is {THR_BM25_MAX_QUERIES} "
                          "(THR_BM25_MAX_QUERIES): split the batch")


BM25_IDF_MIN = 1e-300   # the smallest positive idf (thr_hip.h, a3: the input contract of the pruning bounds)


def bm25_check_params(idf, avgdl: float, k1: float = 1.2, b: float = 0.75) -> None:
    """What the BM25 pruning bounds assume of their inputs (thr_hip.h, a3): avgdl > 0, k1 >= 0,
    0 <= b <= 1, every idf finite and 0 or >= BM25_IDF_MIN.  Outside it a quantised impact is no
    upper bound (a negative idf times an impact rounded up) or the accumulator weights are not
    finite, and a wrong top-k comes back without a flag.  ``idf``: a tensor on any device (read
    back once: call it at index set-up, not per query); raises NativeError naming the value."""
    for name, v, ok in (("avgdl", avgdl, lambda x: x > 0.0), ("k1", k1, lambda x: x >= 0.0),
                        ("b", b, lambda x: 0.0 <= x <= 1.0)):
        v = float(v)
        if not (math.isfinite(v) and ok(v)):
            raise NativeError(f"bm25: {name} = {v!r}; the scoring bounds need avgdl > 0, k1 >= 0, 0 <= b <= 1, all finite")
    t = idf.detach() if isinstance(idf, torch.Tensor) else torch.tensor(idf, dtype=torch.float64)   # (a copy: numpy arrays may be read-only)
    t = t.reshape(-1).to(torch.float64)
    bad = ~torch.isfinite(t) | (t < 0) | ((t > 0) & (t < BM25_IDF_MIN))
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        raise NativeError(f"bm25: idf[{i}] = {float(t[i])!r}; every idf must be finite and either 0 or >= {BM25_IDF_MIN!r}"
                          f" ({int(bad.sum())} of {t.numel()} are not)")


def bm25_topk(rowptr, post_doc, post_tf, doclen, idf, avgdl: float, query_terms, k: int,
              id_base: int = 0, k1: float = 1.2, b: float = 0.75, bounds=None,
              conjunctive: bool = False, doc_coll=None, query_coll=None,
              workspace: Optional[torch.Tensor] = None, dense=None):
    """``dense``: bm25_dense_terms' tuple (needs ``bounds`` with the impacts).
    ``workspace``: a device tensor of >= bm25_workspace_bytes(nq, max_terms, k) bytes
    (item list, slice edges and per-slice lists of the work decomposition); allocated when
    missing or too small."""
    pr = _dev(rowptr, torch.int64, "rowptr", 1)
    pdoc = _dev(post_doc, torch.int32, "post_doc", 1)
    ptf = _dev(post_tf, torch.int32, "post_tf", 1)
    pdl = _dev(doclen, torch.float32, "doclen", 1)
    pidf = _dev(idf, torch.float64, "idf", 1)
    pqt = _dev(query_terms, torch.int32, "query_terms", 2)
    if post_doc.shape != post_tf.shape or idf.shape[0] + 1 != rowptr.shape[0]:
        raise NativeError("bm25: CSR arrays are inconsistent")
    nq, mt = query_terms.shape
    bm25_check_batch(nq)
    if mt > THR_BM25_MAX_TERMS or k > THR_TOPK_MAX:
        raise NativeError("bm25: too many terms per query or k too large")
    ptu = pbu = pim = None
    if bounds is not None:
        ptu, pbu = _dev(bounds[0], torch.float64, "term_ub", 1), _dev(bounds[1], torch.float64, "block_ub", 1)
        if bounds[0].shape[0] != idf.shape[0]:
            raise NativeError("bm25: term_ub length != vocabulary size")
        if len(bounds) > 2 and bounds[2] is not None:
            pim = _dev(bounds[2], torch.uint8, "post_imp", 1)
            if bounds[2].shape[0] < post_doc.shape[0]:
                raise NativeError("bm25: post_imp shorter than the posting array")
    pds = pdi = pdt = None
    dstride = 0
    if dense is not None:
        if pim is None:
            raise NativeError("bm25: dense rows need the bounds with the impacts")
        pds, pdi = _dev(dense[0], torch.int32, "dense_slot", 1), _dev(dense[1], torch.uint8, "dense_imp", 2)
        pdt, dstride = _dev(dense[2], torch.int16, "dense_tf", 2), int(dense[3])
        if dense[0].shape[0] != idf.shape[0] or dense[1].shape != dense[2].shape or dense[1].shape[1] != dstride:
            raise NativeError("bm25: dense rows are inconsistent")
    pdc, pqc = _coll(doc_coll, query_coll, doclen.shape[0], nq)
    S, I, cnt, _ = _alloc_out(nq, k, rowptr.device)
    ws, nbytes = _workspace(workspace, bm25_workspace_bytes(nq, mt, k), rowptr.device)
    _check(load().thr_bm25_topk(pr, pdoc, ptf, pdl, pidf, ptu, pbu, pim, pds, pdi, pdt, dstride,
                                avgdl, k1, b, doclen.shape[0],
                                idf.shape[0], id_base, pqt, nq, mt, k, 1 if conjunctive else 0, pdc,
                                pqc, S.data_ptr(), I.data_ptr(), cnt.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_bm25_topk")
    return S, I, cnt


# --------------------------------------------------------------------- a4
def graph_workspace_bytes(n_queries: int, n_entities: int) -> int:
    return int(load().thr_graph_workspace_bytes(n_queries, n_entities))


def graph_topk(ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf, query_seeds, hops: int,
               k: int, chunk_base: int, n_chunks: int, transposed=None,
               workspace: Optional[torch.Tensor] = None):
    """-> (scores, ids, counts, flags).  ``transposed`` = (tmen_rowptr i64 [n_chunks+1], tmen_ent
    i32, tmen_conf f32) from ``graph_transpose_mentions`` enables the capacity-free third tier."""
    return _graph_call("thr_graph_topk", ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf, query_seeds,
                       hops, k, chunk_base, n_chunks, transposed, workspace, None)


def graph_topk_scoped(ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf, query_seeds, hops: int,
                      k: int, chunk_base: int, n_chunks: int, doc_label, query_label, transposed=None,
                      workspace: Optional[torch.Tensor] = None):
    """thr_graph_topk_scoped: graph_topk over the chunks of each query's scope -> (scores, ids,
    counts, flags).  doc_label i32 [n_chunks] (scope_resolve's labels, or any per-chunk labelling),
    query_label i32 [nq] (negative = no filter): chunk c counts for query q only if its label is
    the query's.  Both are required: an unfiltered search is graph_topk."""
    if doc_label is None or query_label is None:
        raise NativeError("graph_topk_scoped: doc_label and query_label are required (graph_topk is the unfiltered call)")
    return _graph_call("thr_graph_topk_scoped", ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf,
                       query_seeds, hops, k, chunk_base, n_chunks, transposed, workspace, (doc_label, query_label))


def _graph_call(entry, ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf, query_seeds, hops, k, chunk_base,
                n_chunks, transposed, workspace, labels):
    per = _dev(ent_rowptr, torch.int64, "ent_rowptr", 1)
    pec = _dev(ent_col, torch.int32, "ent_col", 1)
    pmr = _dev(men_rowptr, torch.int64, "men_rowptr", 1)
    pmc = _dev(men_chunk, torch.int32, "men_chunk", 1)
    pmw = _dev(men_conf, torch.float32, "men_conf", 1)
    pqs = _dev(query_seeds, torch.int32, "query_seeds", 2)
    if ent_rowptr.shape != men_rowptr.shape or men_chunk.shape != men_conf.shape:
        raise NativeError("graph: CSR arrays are inconsistent")
    ptr = pte = ptw = None
    n_ent = ent_rowptr.shape[0] - 1
    if transposed is not None:
        tr, te, tw = transposed
        ptr, pte, ptw = (_dev(tr, torch.int64, "tmen_rowptr", 1), _dev(te, torch.int32, "tmen_ent", 1),
                         _dev(tw, torch.float32, "tmen_conf", 1))
        if tr.shape[0] != n_chunks + 1 or te.shape != tw.shape:
            raise NativeError("graph: transposed mention CSR is inconsistent")
    nq, ms = query_seeds.shape
    if ms > THR_GRAPH_MAX_SEEDS or k > THR_TOPK_MAX:
        raise NativeError("graph: too many seeds per query or k too large")
    scoped = ()
    if labels is not None:
        doc_label, query_label = labels
        scoped = (_dev(doc_label, torch.int32, "doc_label", 1), _dev(query_label, torch.int32, "query_label", 1))
        if doc_label.shape[0] != n_chunks or query_label.shape[0] != nq:
            raise NativeError("graph: doc_label holds one label per chunk of the shard, query_label one per query")
    ws, nbytes = _workspace(workspace, load().thr_graph_workspace_bytes(nq, n_ent if transposed is not None else 0),
                            ent_rowptr.device)
    S, I, cnt, flg = _alloc_out(nq, k, ent_rowptr.device)
    _check(getattr(load(), entry)(per, pec, n_ent, pmr, pmc, pmw, ptr, pte, ptw, chunk_base, n_chunks, *scoped,
                                  pqs, nq, ms, hops, k, S.data_ptr(), I.data_ptr(), cnt.data_ptr(),
                                  flg.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           entry)
    return S, I, cnt, flg


def entity_match_workspace_bytes(n_entities: int, n_needles: int, n_queries: int) -> int:
    return int(load().thr_entity_match_workspace_bytes(n_entities, n_needles, n_queries))


def entity_match(name_bytes, name_ptr, needles, needle_len, query_needles, query_per, workspace=None):
    """thr_entity_match: the seed entities of a batch from its keywords -> (seeds i32 [nq, 16] padded
    with -1, counts i32 [nq]).  name_bytes u8 / name_ptr i64 [E + 1]: the packed lowered names
    (index_entities.pack_entity_names: 0xFF behind every name and THR_ENTITY_MAX_NEEDLE more behind
    the last); needles u8 [M, 128] / needle_len i32 [M]: the batch's distinct lowered keywords;
    query_needles i32 [nq, 5] (-1 = none), query_per i32 [nq].  No host read-back."""
    pb = _dev(name_bytes, torch.uint8, "name_bytes", 1)
    pp = _dev(name_ptr, torch.int64, "name_ptr", 1)
    n_ent = name_ptr.shape[0] - 1
    pn = _dev(needles, torch.uint8, "needles", 2)
    pl = _dev(needle_len, torch.int32, "needle_len", 1)
    M = needles.shape[0]
    if needles.shape[1] != THR_ENTITY_MAX_NEEDLE or needle_len.shape[0] != M:
        raise NativeError(f"entity_match: needles must be [M, {THR_ENTITY_MAX_NEEDLE}] with M lengths")
    pq = _dev(query_needles, torch.int32, "query_needles", 2)
    pr = _dev(query_per, torch.int32, "query_per", 1)
    nq = query_needles.shape[0]
    if query_needles.shape[1] != THR_ENTITY_MAX_KEYWORDS or query_per.shape[0] != nq:
        raise NativeError(f"entity_match: query_needles must be [nq, {THR_ENTITY_MAX_KEYWORDS}] with nq per-values")
    if not 1 <= nq <= THR_ENTITY_MAX_QUERIES:
        raise NativeError(f"entity_match: 1 .. {THR_ENTITY_MAX_QUERIES} queries per call, got {nq}")
    if n_ent < 1 or not 1 <= M <= THR_ENTITY_MAX_KEYWORDS * nq:
        raise NativeError(f"entity_match: {n_ent} entities, {M} needles for {nq} queries")
    ws, nbytes = _workspace(workspace, entity_match_workspace_bytes(n_ent, M, nq), name_bytes.device)
    seeds = torch.empty((nq, THR_GRAPH_MAX_SEEDS), dtype=torch.int32, device=name_bytes.device)
    counts = torch.empty(nq, dtype=torch.int32, device=name_bytes.device)
    _check(load().thr_entity_match(pb, pp, n_ent, pn, pl, M, pq, pr, nq, seeds.data_ptr(), counts.data_ptr(),
                                   ws.data_ptr(), nbytes, _stream()), "thr_entity_match")
    return seeds, counts


def vocab_insert(slots, term_bytes, term_ptr, first_id: int, count: int) -> None:
    """thr_vocab_insert: keys first_id .. first_id + count - 1 of the key store (term_bytes u8, term_ptr i64
    [V + 1]) into the open-addressing table ``slots`` (int64 [capacity, 2]: a slot's hash word and its
    (term_id, pad) pair; zero = empty)."""
    ps = _dev(slots, torch.int64, "slots", 2)
    if slots.shape[1] != 2:
        raise NativeError("vocab_insert: slots is int64 [capacity, 2]")
    pb = _dev(term_bytes, torch.uint8, "term_bytes", 1)
    pp = _dev(term_ptr, torch.int64, "term_ptr", 1)
    if first_id < 0 or count < 1 or first_id + count > term_ptr.shape[0] - 1:
        raise NativeError(f"vocab_insert: keys {first_id} .. {first_id + count - 1} of {term_ptr.shape[0] - 1}")
    _check(load().thr_vocab_insert(ps, slots.shape[0], pb, pp, first_id, count, _stream()), "thr_vocab_insert")


def text_token_capacity(n_texts: int, n_bytes: int) -> int:
    """Token rows that always suffice: a token takes a byte and two tokens of a text a byte between them."""
    return max((n_bytes + n_texts + 1) // 2, 1)


def text_tokens_workspace_bytes(n_texts: int, n_bytes: int, token_capacity: int) -> int:
    return int(load().thr_text_tokens_workspace_bytes(n_texts, n_bytes, token_capacity))


def query_terms_workspace_bytes(n_queries: int) -> int:
    return int(load().thr_query_terms_workspace_bytes(n_queries))


def vocab_grow_workspace_bytes(unknown_capacity: int) -> int:
    return int(load().thr_vocab_grow_workspace_bytes(unknown_capacity))


def text_tokens(text_bytes, text_ptr, n_bytes: int, table, slots, term_bytes, term_ptr, workspace=None,
                token_capacity: Optional[int] = None, _analysis=None):
    """thr_text_tokens -> dict(doc i32 [cap], term i32 [cap], n_tokens i32 [n], flags i32 [n], n_total i32 [1],
    unknown_off i64 [cap], unknown_len i32 [cap], n_unknown i32 [1], capacity), all on the device: the first
    n_total rows (n_unknown entries) are valid.  text_bytes u8 holds n_bytes bytes of texts and at least 4
    more; text_ptr i64 [n + 1]; table u32-as-int32 [65536]; the vocabulary as vocab_insert takes it.  No host
    read-back."""
    pb = _dev(text_bytes, torch.uint8, "text_bytes", 1)
    pp = _dev(text_ptr, torch.int64, "text_ptr", 1)
    n = text_ptr.shape[0] - 1
    pt = _dev(table, torch.int32, "table", 1)
    ps = _dev(slots, torch.int64, "slots", 2)
    pk = _dev(term_bytes, torch.uint8, "term_bytes", 1)
    pkp = _dev(term_ptr, torch.int64, "term_ptr", 1)
    if table.shape[0] != 65536 or slots.shape[1] != 2:
        raise NativeError("text_tokens: table is [65536], slots int64 [capacity, 2]")
    if not 1 <= n <= THR_TEXT_MAX_TEXTS:
        raise NativeError(f"text_tokens: 1 .. {THR_TEXT_MAX_TEXTS} texts per call, got {n}")
    if not 0 <= n_bytes <= THR_TEXT_MAX_BYTES or text_bytes.shape[0] < n_bytes + 4:
        raise NativeError(f"text_tokens: {n_bytes} bytes (at most {THR_TEXT_MAX_BYTES}) and 4 of padding behind them, "
                          f"the array holds {text_bytes.shape[0]}")
    cap = text_token_capacity(n, n_bytes) if token_capacity is None else int(token_capacity)
    dev = text_bytes.device
    size = text_tokens_workspace_bytes if _analysis is None else text_tokens_analyzed_workspace_bytes
    ws, nbytes = _workspace(workspace, size(n, n_bytes, cap), dev)
    out = dict(doc=torch.empty(cap, dtype=torch.int32, device=dev), term=torch.empty(cap, dtype=torch.int32, device=dev),
               n_tokens=torch.empty(n, dtype=torch.int32, device=dev), flags=torch.empty(n, dtype=torch.int32, device=dev),
               n_total=torch.empty(1, dtype=torch.int32, device=dev),
               unknown_off=torch.empty(cap, dtype=torch.int64, device=dev),
               unknown_len=torch.empty(cap, dtype=torch.int32, device=dev),
               n_unknown=torch.empty(1, dtype=torch.int32, device=dev), capacity=cap)
    head = (pb, pp, n, n_bytes, pt, ps, slots.shape[0], pk, pkp, term_ptr.shape[0] - 1)
    tail = (cap, out["doc"].data_ptr(), out["term"].data_ptr(), out["n_tokens"].data_ptr(), out["flags"].data_ptr(),
            out["n_total"].data_ptr(), out["unknown_off"].data_ptr(), out["unknown_len"].data_ptr(),
            out["n_unknown"].data_ptr(), ws.data_ptr(), nbytes, _stream())
    if _analysis is None:
        _check(load().thr_text_tokens(*head, *tail), "thr_text_tokens")
    else:
        _check(load().thr_text_tokens_analyzed(*head, *_analysis, *tail), "thr_text_tokens_analyzed")
    return out


def text_tokens_analyzed_workspace_bytes(n_texts: int, n_bytes: int, token_capacity: int) -> int:
    return int(load().thr_text_tokens_analyzed_workspace_bytes(n_texts, n_bytes, token_capacity))


def text_tokens_analyzed(text_bytes, text_ptr, n_bytes: int, table, slots, term_bytes, term_ptr, stop_slots=None,
                         stop_bytes=None, stop_ptr=None, step_ptr=(0,), rules=None, workspace=None,
                         token_capacity: Optional[int] = None):
    """thr_text_tokens_analyzed (thr_hip_text.h) -> text_tokens' dict, with the stop tokens dropped and the stems
    looked up.  The stop set as vocab_insert built it (stop_slots int64 [capacity, 2], stop_bytes u8, stop_ptr i64
    [n_stop + 1]) or three Nones; ``step_ptr``: a HOST sequence of n_steps + 1 ascending ints from 0; ``rules``:
    a device uint8 tensor of step_ptr[-1] records of STEM_RULE_BYTES bytes (None when there is none)."""
    if (stop_slots is None) != (stop_bytes is None) or (stop_slots is None) != (stop_ptr is None):
        raise NativeError("text_tokens_analyzed: the stop set is slots, bytes and pointers, or none of them")
    pss = _dev(stop_slots, torch.int64, "stop_slots", 2)
    if stop_slots is not None and stop_slots.shape[1] != 2:
        raise NativeError("text_tokens_analyzed: stop_slots is int64 [capacity, 2]")
    psb = _dev(stop_bytes, torch.uint8, "stop_bytes", 1)
    psp = _dev(stop_ptr, torch.int64, "stop_ptr", 1)
    steps = [int(v) for v in step_ptr]
    if not 1 <= len(steps) <= STEM_MAX_STEPS + 1:
        raise NativeError(f"text_tokens_analyzed: 0 .. {STEM_MAX_STEPS} steps, step_ptr holds {len(steps)} entries")
    if steps[0] != 0 or any(a > b for a, b in zip(steps, steps[1:])) or steps[-1] > STEM_MAX_RULES:
        raise NativeError(f"text_tokens_analyzed: step_ptr ascends from 0 to at most {STEM_MAX_RULES}, got {steps}")
    pr = _dev(rules, torch.uint8, "rules", 1)
    if (rules.shape[0] if rules is not None else 0) < steps[-1] * STEM_RULE_BYTES:
        raise NativeError(f"text_tokens_analyzed: {steps[-1]} rules of {STEM_RULE_BYTES} bytes, the array holds "
                          f"{0 if rules is None else rules.shape[0]} bytes")
    h_steps = (C.c_int32 * len(steps))(*steps)
    analysis = (pss, 0 if stop_slots is None else stop_slots.shape[0], psb, psp,
                0 if stop_ptr is None else stop_ptr.shape[0] - 1, C.cast(h_steps, C.c_void_p), len(steps) - 1,
                pr if steps[-1] else None)
    return text_tokens(text_bytes, text_ptr, n_bytes, table, slots, term_bytes, term_ptr, workspace=workspace,
                       token_capacity=token_capacity, _analysis=analysis)


def query_terms(rows: dict, workspace=None):
    """thr_query_terms over the rows text_tokens returned for a batch of queries -> (terms i32
    [nq, THR_BM25_MAX_TERMS] padded with -1, n_distinct i32 [nq], flags i32 [nq]).  No host read-back."""
    nq = rows["n_tokens"].shape[0]
    dev = rows["term"].device
    ws, nbytes = _workspace(workspace, query_terms_workspace_bytes(nq), dev)
    terms = torch.empty((nq, THR_BM25_MAX_TERMS), dtype=torch.int32, device=dev)
    nd = torch.empty(nq, dtype=torch.int32, device=dev)
    fl = torch.empty(nq, dtype=torch.int32, device=dev)
    _check(load().thr_query_terms(_dev(rows["term"], torch.int32, "term", 1), _dev(rows["n_tokens"], torch.int32, "n_tokens", 1),
                                  _dev(rows["flags"], torch.int32, "flags", 1), _dev(rows["n_total"], torch.int32, "n_total", 1),
                                  rows["capacity"], nq, terms.data_ptr(), nd.data_ptr(), fl.data_ptr(), ws.data_ptr(),
                                  nbytes, _stream()), "thr_query_terms")
    return terms, nd, fl


def vocab_grow(text_bytes, text_ptr, n_bytes: int, table, rows: dict, n_unknown: int, n_vocab: int,
               new_bytes_capacity: Optional[int] = None, hash_mask: int = (1 << 64) - 1, term=None,
               workspace=None):
    """thr_vocab_grow over what ``text_tokens`` returned for the batch (``rows``: flags, unknown_off,
    unknown_len, n_unknown) -> dict(unknown_term i32 [n_unknown], new_bytes u8 [new_bytes_capacity + 16],
    new_ptr i64 [n_unknown + 1], n_new i32 [1], n_new_bytes i64 [1], status i32 [1]), all on the device.
    ``n_unknown`` (>= 1) is the host's copy of rows["n_unknown"]: it sizes the list and the workspace.
    ``term``: the first n_total rows of rows["term"] (a contiguous int32 tensor), patched in place.
    new_bytes_capacity: room for the lowered keys (default 16 bytes per occurrence); THR_VOCAB_GROW_OVERFLOW
    in status asks for n_new_bytes.  new_bytes carries 16 bytes of padding behind the capacity (the key store's).
    No host read-back."""
    pb = _dev(text_bytes, torch.uint8, "text_bytes", 1)
    pp = _dev(text_ptr, torch.int64, "text_ptr", 1)
    pt = _dev(table, torch.int32, "table", 1)
    n = text_ptr.shape[0] - 1
    pf = _dev(rows["flags"], torch.int32, "flags", 1)
    po = _dev(rows["unknown_off"], torch.int64, "unknown_off", 1)
    pl = _dev(rows["unknown_len"], torch.int32, "unknown_len", 1)
    pn = _dev(rows["n_unknown"], torch.int32, "n_unknown", 1)
    if table.shape[0] != 65536 or rows["flags"].shape[0] != n:
        raise NativeError("vocab_grow: table is [65536], flags one per text")
    if not 1 <= n_unknown <= min(rows["unknown_off"].shape[0], rows["unknown_len"].shape[0]):
        raise NativeError(f"vocab_grow: n_unknown {n_unknown} outside 1 .. the unknown list's {rows['unknown_off'].shape[0]}")
    if not 0 <= n_bytes <= THR_TEXT_MAX_BYTES or text_bytes.shape[0] < n_bytes + 4:
        raise NativeError(f"vocab_grow: {n_bytes} bytes and 4 of padding behind them, the array holds {text_bytes.shape[0]}")
    if not 0 < hash_mask < 1 << 64:
        raise NativeError("vocab_grow: hash_mask is a non-zero 64-bit mask")
    dev = text_bytes.device
    cap_b = max(int(new_bytes_capacity if new_bytes_capacity is not None else 16 * n_unknown), 0)
    ws, nbytes = _workspace(workspace, vocab_grow_workspace_bytes(n_unknown), dev)
    ptk = pnt = None
    tcap = 0
    if term is not None:
        ptk = _dev(term, torch.int32, "term", 1)
        pnt = _dev(rows["n_total"], torch.int32, "n_total", 1)
        tcap = term.shape[0]
        if tcap < 1:
            raise NativeError("vocab_grow: an empty term array cannot hold unknown tokens")
    out = dict(unknown_term=torch.empty(n_unknown, dtype=torch.int32, device=dev),
               new_bytes=torch.zeros(cap_b + 16, dtype=torch.uint8, device=dev),
               new_ptr=torch.empty(n_unknown + 1, dtype=torch.int64, device=dev),
               n_new=torch.empty(1, dtype=torch.int32, device=dev), n_new_bytes=torch.empty(1, dtype=torch.int64, device=dev),
               status=torch.empty(1, dtype=torch.int32, device=dev), capacity=cap_b)
    _check(load().thr_vocab_grow(pb, pp, n, n_bytes, pt, pf, po, pl, pn, n_unknown, n_vocab, hash_mask, ptk, pnt, tcap,
                                 out["unknown_term"].data_ptr(), out["new_bytes"].data_ptr(), cap_b,
                                 out["new_ptr"].data_ptr(), out["n_new"].data_ptr(), out["n_new_bytes"].data_ptr(),
                                 out["status"].data_ptr(), ws.data_ptr(), nbytes, _stream()), "thr_vocab_grow")
    return out


# ------------------------------------------------- typo-tolerant lexical queries (thr_hip_fuzzy.h)
def fuzzy_check(what: str, max_edits, n_best) -> None:
    """THE refusal of an edit budget or a correction count outside the header's ranges, by name."""
    if isinstance(max_edits, bool) or not isinstance(max_edits, int) or not 1 <= max_edits <= FUZZY_MAX_EDITS:
        raise NativeError(f"{what}: max_edits {max_edits!r} outside 1 .. {FUZZY_MAX_EDITS}")
    if isinstance(n_best, bool) or not isinstance(n_best, int) or not 1 <= n_best <= FUZZY_MAX_BEST:
        raise NativeError(f"{what}: n_best {n_best!r} outside 1 .. THR_FUZZY_MAX_BEST ({FUZZY_MAX_BEST})")


def vocab_nearest_workspace_bytes(n_bytes: int, unknown_capacity: int, n_vocab: int, n_term_bytes: int, n_best: int) -> int:
    return int(load().thr_vocab_nearest_workspace_bytes(n_bytes, unknown_capacity, n_vocab, n_term_bytes, n_best))


def query_terms_fuzzy_workspace_bytes(n_queries: int) -> int:
    return int(load().thr_query_terms_fuzzy_workspace_bytes(n_queries))


def vocab_nearest(text_bytes, n_bytes: int, table, unknown_off, unknown_len, n_unknown, term_bytes, term_ptr,
                  n_term_bytes: int, term_rowptr=None, max_edits: int = 2, n_best: int = 2, workspace=None,
                  near_term=None, near_dist=None):
    """thr_vocab_nearest over the unknown list of a text_tokens call (unknown_off i64 / unknown_len i32 [cap],
    n_unknown i32 [1], on the device) -> (near_term, near_dist) int32 [cap, n_best] on the device: rows at or behind
    n_unknown are NOT written (``near_term`` / ``near_dist``: the arrays to write into, else fresh ones filled with
    -1).  term_rowptr i64 [n_vocab + 1] (the postings' row pointer) or None: no document frequencies.  No host
    read-back."""
    fuzzy_check("vocab_nearest", max_edits, n_best)
    pb = _dev(text_bytes, torch.uint8, "text_bytes", 1)
    pt = _dev(table, torch.int32, "table", 1)
    po = _dev(unknown_off, torch.int64, "unknown_off", 1)
    pl = _dev(unknown_len, torch.int32, "unknown_len", 1)
    pn = _dev(n_unknown, torch.int32, "n_unknown", 1)
    pk = _dev(term_bytes, torch.uint8, "term_bytes", 1)
    pkp = _dev(term_ptr, torch.int64, "term_ptr", 1)
    pr = _dev(term_rowptr, torch.int64, "term_rowptr", 1)
    cap = min(unknown_off.shape[0], unknown_len.shape[0])
    n_vocab = term_ptr.shape[0] - 1
    if table.shape[0] != 65536 or n_unknown.shape[0] != 1:
        raise NativeError("vocab_nearest: table is [65536], n_unknown [1]")
    if not 0 <= n_bytes <= min(THR_TEXT_MAX_BYTES, text_bytes.shape[0]):
        raise NativeError(f"vocab_nearest: {n_bytes} text bytes, the array holds {text_bytes.shape[0]}")
    if not 1 <= cap <= THR_TEXT_MAX_BYTES:
        raise NativeError(f"vocab_nearest: an unknown list of 1 .. {THR_TEXT_MAX_BYTES} entries, got {cap}")
    if n_vocab < 0 or not 0 <= n_term_bytes <= term_bytes.shape[0]:
        raise NativeError(f"vocab_nearest: {n_term_bytes} key bytes, the array holds {term_bytes.shape[0]}; term_ptr is [n_vocab + 1]")
    if term_rowptr is not None and term_rowptr.shape[0] < n_vocab + 1:
        raise NativeError(f"vocab_nearest: term_rowptr holds {term_rowptr.shape[0]} entries for {n_vocab} terms")
    dev = text_bytes.device
    for name, arr in (("near_term", near_term), ("near_dist", near_dist)):
        if arr is not None and (_dev(arr, torch.int32, name, 2) == 0 or tuple(arr.shape) != (cap, n_best)):
            raise NativeError(f"vocab_nearest: {name} is int32 [{cap}, {n_best}]")
    if near_term is None:
        near_term = torch.full((cap, n_best), -1, dtype=torch.int32, device=dev)
    if near_dist is None:
        near_dist = torch.full((cap, n_best), -1, dtype=torch.int32, device=dev)
    ws, nbytes = _workspace(workspace, vocab_nearest_workspace_bytes(n_bytes, cap, n_vocab, n_term_bytes, n_best), dev)
    _check(load().thr_vocab_nearest(pb, n_bytes, pt, po, pl, pn, cap, pk, pkp, n_vocab, n_term_bytes, pr or None, max_edits,
                                    n_best, near_term.data_ptr(), near_dist.data_ptr(), ws.data_ptr(), nbytes, _stream()),
           "thr_vocab_nearest")
    return near_term, near_dist


def query_terms_fuzzy(rows: dict, near_term, n_use: int, workspace=None):
    """thr_query_terms_fuzzy: ``query_terms`` with the corrections ``near_term`` (int32 [cap, n_best], vocab_nearest's)
    folded in, the first ``n_use`` of each unknown token -> (terms, n_distinct, flags).  No host read-back."""
    nq = rows["n_tokens"].shape[0]
    dev = rows["term"].device
    pnear = _dev(near_term, torch.int32, "near_term", 2)
    n_best = near_term.shape[1]
    fuzzy_check("query_terms_fuzzy", 1, n_best)
    if isinstance(n_use, bool) or not isinstance(n_use, int) or not 1 <= n_use <= n_best:
        raise NativeError(f"query_terms_fuzzy: n_use {n_use!r} outside 1 .. n_best ({n_best})")
    if near_term.shape[0] < 1:
        raise NativeError("query_terms_fuzzy: near_term holds no row")
    ws, nbytes = _workspace(workspace, query_terms_fuzzy_workspace_bytes(nq), dev)
    terms = torch.empty((nq, THR_BM25_MAX_TERMS), dtype=torch.int32, device=dev)
    nd = torch.empty(nq, dtype=torch.int32, device=dev)
    fl = torch.empty(nq, dtype=torch.int32, device=dev)
    _check(load().thr_query_terms_fuzzy(_dev(rows["term"], torch.int32, "term", 1), _dev(rows["n_tokens"], torch.int32, "n_tokens", 1),
                                        _dev(rows["flags"], torch.int32, "flags", 1), _dev(rows["n_total"], torch.int32, "n_total", 1),
                                        rows["capacity"], nq, pnear, near_term.shape[0], n_best, n_use, terms.data_ptr(),
                                        nd.data_ptr(), fl.data_ptr(), ws.data_ptr(), nbytes, _stream()), "thr_query_terms_fuzzy")
    return terms, nd, fl


def graph_transpose_mentions(men_rowptr, men_chunk, men_conf, chunk_base: int, n_chunks: int):
    """Index set-up (device tensors, torch ops): the entity-major mention CSR restricted to this
    shard's chunks, re-sorted chunk-major with a STABLE sort, so a chunk's entries stay in
    (entity asc, mention) order -- the oracle's summation order."""
    ne = men_rowptr.shape[0] - 1
    ent = torch.repeat_interleave(torch.arange(ne, dtype=torch.int32, device=men_rowptr.device),
                                  (men_rowptr[1:] - men_rowptr[:-1]))
    local = men_chunk.to(torch.int64) - chunk_base
    keep = (local >= 0) & (local < n_chunks)
    ent, conf, local = ent[keep], men_conf[keep], local[keep]
    order = torch.sort(local, stable=True).indices
    counts = torch.bincount(local, minlength=n_chunks)
    rowptr = torch.zeros(n_chunks + 1, dtype=torch.int64, device=men_rowptr.device)
    rowptr[1:] = torch.cumsum(counts, 0)
    return rowptr, ent[order].contiguous(), conf[order].contiguous()


# ----------------------------------------------------------------- a5 + a6
def rrf_check_top_k(what: str, top_k: int) -> None:
    """The top_k thr_rrf_fuse / thr_rrf_fuse_standalone take, refused here with the limit in the
    message (the library answers anything else with THR_ERR_INVALID)."""
    if not 1 <= int(top_k) <= THR_RRF_MAX_TOP_K:
        raise NativeError(f"{what}: top_k must be in 1 .. {THR_RRF_MAX_TOP_K} (the rows of one fused list), "
                          f"got {top_k}")


def rrf_fuse(lex_ids, sem_ids, graph_ids, top_k: int, w_lex: float = 0.7, w_sem: float = 0.8,
             w_graph: float = 1.0, rrf_k: int = 60, want_ranks: bool = False):
    return _rrf_call("thr_rrf_fuse", lex_ids, sem_ids, graph_ids, top_k, w_lex, w_sem, w_graph, rrf_k, want_ranks)


def rrf_fuse_standalone(lex_ids, sem_ids, graph_ids, top_k: int, w_lex: float = 0.7, w_sem: float = 0.8,
                        w_graph: float = 1.0, two_channels: bool = False, want_ranks: bool = True):
    """The standalone package's RRFFusion.fuse / fuse_two_channels on id lists [nq, n_c] (-1
    padded) -> (ids i64 [nq, top_k], scores f64, ranks i32 [nq, top_k, 3] or None, counts)."""
    return _rrf_call("thr_rrf_fuse_standalone", lex_ids, sem_ids, graph_ids, top_k, w_lex, w_sem, w_graph,
                     1 if two_channels else 0, want_ranks)


def _rrf_call(entry: str, lex_ids, sem_ids, graph_ids, top_k: int, w_lex, w_sem, w_graph, scalar: int, want_ranks: bool):
    """``entry`` (thr_rrf_fuse / thr_rrf_fuse_standalone) over the three id lists; ``scalar`` is the one
    argument in which the two differ (rrf_k / the two_channels flag), in the same position."""
    rrf_check_top_k(entry[4:], top_k)
    chans = [lex_ids, sem_ids, graph_ids]
    ref = next(c for c in chans if c is not None)
    nq = ref.shape[0]
    ptrs, widths = [], []
    for name, c in zip(("lex_ids", "sem_ids", "graph_ids"), chans):
        if c is None:
            ptrs.append(0)
            widths.append(0)
            continue
        ptrs.append(_dev(c, torch.int64, name, 2))
        if c.shape[0] != nq or c.shape[1] > THR_RRF_MAX_PER_CHANNEL:
            raise NativeError(f"rrf: bad shape for {name}")
        widths.append(c.shape[1])
    dev = ref.device
    out_ids = torch.empty((nq, top_k), dtype=torch.int64, device=dev)
    out_sc = torch.empty((nq, top_k), dtype=torch.float64, device=dev)
    out_rk = torch.empty((nq, top_k, 3), dtype=torch.int32, device=dev) if want_ranks else None
    cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    _check(getattr(load(), entry)(ptrs[0], widths[0], ptrs[1], widths[1], ptrs[2], widths[2], nq,
                                          w_lex, w_sem, w_graph, scalar, top_k,
                                          out_ids.data_ptr(), out_sc.data_ptr(),
                                          out_rk.data_ptr() if want_ranks else 0, cnt.data_ptr(),
                                          _stream()), entry)
    return out_ids, out_sc, out_rk, cnt


def fuse_post(ids, scores, ranks=None, counts=None, channel_scores=(None, None, None),
              safety_threshold: float = 0.0, denoise_quantile: Optional[float] = None,
              normalize: bool = False, top_k: int = 0):
    """Safety threshold / percentile denoise / truncation / min-max normalisation of a batch of
    fused lists (thr_fuse_post).  denoise_quantile = ((1 - alpha) * 100) / 100 or None."""
    pi = _dev(ids, torch.int64, "ids", 2)
    ps = _dev(scores, torch.float64, "scores", 2)
    nq, n = ids.shape
    if tuple(scores.shape) != (nq, n):
        raise NativeError("fuse_post: ids / scores shape mismatch")
    pr = _dev(ranks, torch.int32, "ranks", 3) if ranks is not None else None
    if ranks is not None and tuple(ranks.shape) != (nq, n, 3):
        raise NativeError("fuse_post: ranks must be [nq, n, 3]")
    pc = _dev(counts, torch.int32, "counts", 1) if counts is not None else None
    cp, cw = [], []
    for name, c in zip(("lex_scores", "sem_scores", "graph_scores"), channel_scores):
        cp.append(_dev(c, torch.float64, name, 2) if c is not None else None)
        cw.append(c.shape[1] if c is not None else 0)
        if c is not None and c.shape[0] != nq:
            raise NativeError(f"fuse_post: bad shape for {name}")
    out_ids = torch.empty_like(ids)
    out_sc = torch.empty_like(scores)
    out_c = torch.empty(nq, dtype=torch.int32, device=ids.device)
    _check(load().thr_fuse_post(pi, ps, pr, pc, nq, n, cp[0], cw[0], cp[1], cw[1], cp[2], cw[2],
                                float(safety_threshold), 0 if denoise_quantile is None else 1,
                                float(denoise_quantile or 0.0), 1 if normalize else 0, int(top_k),
                                out_ids.data_ptr(), out_sc.data_ptr(), out_c.data_ptr(), _stream()),
           "thr_fuse_post")
    return out_ids, out_sc, out_c


# --------------------------------------------------------------------- a8
def maxsim_check_tokens(what: str, tok_dim: int, *n_tokens: int) -> None:
    """The shapes thr_maxsim_pack / thr_maxsim / thr_maxsim_ids take, refused here with the
    list in the message (the library answers the same shapes with THR_ERR_UNSUPPORTED)."""
    if any(n <= 0 or n % 32 for n in n_tokens):
        raise NativeError(f"{what}: q_tokens / d_tokens must be positive multiples of 32, got {n_tokens}")
    if tok_dim not in MAXSIM_TOK_DIMS:
        raise NativeError(f"{what}: tok_dim {tok_dim} is not supported: the MaxSim kernels take tok_dim in "
                          f"{list(MAXSIM_TOK_DIMS)}")


def maxsim_pack(dtok: torch.Tensor) -> torch.Tensor:
    """Row-major token store -> fragment-major image for maxsim(..., packed=True)."""
    pdt = _dev(dtok, torch.float16, "dtok", 3)
    nd, dt, td = dtok.shape
    maxsim_check_tokens("maxsim_pack", td, dt)
    out = torch.empty_like(dtok)
    _check(load().thr_maxsim_pack(pdt, nd, dt, td, out.data_ptr(), _stream()), "thr_maxsim_pack")
    return out


def maxsim(qtok: torch.Tensor, dtok: torch.Tensor, cand: torch.Tensor,
           packed: bool = False) -> torch.Tensor:
    """cand holds LOCAL doc indices; negative or out-of-range entries score -inf."""
    return _maxsim_call("thr_maxsim", qtok, dtok, cand, torch.int32, "cand", (), packed)


def maxsim_ids(qtok: torch.Tensor, dtok: torch.Tensor, cand_ids: torch.Tensor, id_base: int,
               packed: bool = False) -> torch.Tensor:
    """cand_ids holds GLOBAL doc ids (int64) of a shard starting at ``id_base``; negative ids and
    ids outside the shard score -inf."""
    return _maxsim_call("thr_maxsim_ids", qtok, dtok, cand_ids, torch.int64, "cand_ids", (int(id_base),), packed)


def _maxsim_call(entry: str, qtok, dtok, cand, cand_dtype, cand_name: str, id_base: tuple, packed: bool):
    """``entry`` (thr_maxsim / thr_maxsim_ids) over candidates of ``cand_dtype``; ``id_base``: the
    argument thr_maxsim_ids takes behind the candidates, () for thr_maxsim."""
    pq = _dev(qtok, torch.float16, "qtok", 3)
    pdt = _dev(dtok, torch.float16, "dtok", 3)
    pc = _dev(cand, cand_dtype, cand_name, 2)
    nq, qt, td = qtok.shape
    nd, dt, td2 = dtok.shape
    if td != td2 or cand.shape[0] != nq:
        raise NativeError("maxsim: shape mismatch")
    maxsim_check_tokens(entry[4:], td, qt, dt)
    out = torch.empty(cand.shape, dtype=torch.float32, device=qtok.device)
    _check(getattr(load(), entry)(pq, nq, qt, pdt, nd, dt, td, pc, *id_base, cand.shape[1], out.data_ptr(),
                                  1 if packed else 0, _stream()), entry)
    return out


# ------------------------------------------------- a8, FP8 token store (thr_hip_rerank.h)
def maxsim_fp8_check_tokens(what: str, tok_dim: int, *n_tokens: int) -> None:
    """The shapes thr_maxsim_quantize_fp8 / thr_maxsim_fp8 / thr_maxsim_fp8_ids take, refused here with
    the list in the message (the library answers the same shapes with THR_ERR_UNSUPPORTED)."""
    if any(n <= 0 or n % 32 for n in n_tokens):
        raise NativeError(f"{what}: q_tokens / d_tokens must be positive multiples of 32, got {n_tokens}")
    if tok_dim not in MAXSIM_FP8_TOK_DIMS:
        raise NativeError(f"{what}: tok_dim {tok_dim} is not supported: the FP8 MaxSim kernels take tok_dim in "
                          f"{list(MAXSIM_FP8_TOK_DIMS)}")


def maxsim_quantize_fp8(dtok: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """Row-major float16 token store [n, d_tokens, tok_dim] -> (codes uint8 [n, d_tokens, tok_dim]: the
    packed E4M3 image of thr_hip_rerank.h, d_tokens * tok_dim bytes per document -- the shape names the
    store, not the place of a byte; scales float32 [n, d_tokens])."""
    pdt = _dev(dtok, torch.float16, "dtok", 3)
    nd, dt, td = dtok.shape
    maxsim_fp8_check_tokens("maxsim_quantize_fp8", td, dt)
    codes = torch.empty(dtok.shape, dtype=torch.uint8, device=dtok.device)
    scales = torch.empty((nd, dt), dtype=torch.float32, device=dtok.device)
    if nd:
        _check(load().thr_maxsim_quantize_fp8(pdt, nd, dt, td, codes.data_ptr(), scales.data_ptr(), _stream()),
               "thr_maxsim_quantize_fp8")
    return codes, scales


def maxsim_fp8(qtok: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, cand: torch.Tensor) -> torch.Tensor:
    """cand holds LOCAL doc indices; negative or out-of-range entries score -inf."""
    return _maxsim_fp8_call("thr_maxsim_fp8", qtok, codes, scales, cand, torch.int32, "cand", ())


def maxsim_fp8_ids(qtok: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, cand_ids: torch.Tensor,
                   id_base: int) -> torch.Tensor:
    """cand_ids holds GLOBAL doc ids (int64) of a shard starting at ``id_base``; negative ids and
    ids outside the shard score -inf."""
    return _maxsim_fp8_call("thr_maxsim_fp8_ids", qtok, codes, scales, cand_ids, torch.int64, "cand_ids",
                            (int(id_base),))


def _maxsim_fp8_call(entry: str, qtok, codes, scales, cand, cand_dtype, cand_name: str, id_base: tuple):
    """``entry`` (thr_maxsim_fp8 / thr_maxsim_fp8_ids) over candidates of ``cand_dtype``; ``id_base``: the
    argument thr_maxsim_fp8_ids takes behind the candidates, () for thr_maxsim_fp8."""
    pq = _dev(qtok, torch.float16, "qtok", 3)
    pcd = _dev(codes, torch.uint8, "codes", 3)
    psc = _dev(scales, torch.float32, "scales", 2)
    pc = _dev(cand, cand_dtype, cand_name, 2)
    nq, qt, td = qtok.shape
    nd, dt, td2 = codes.shape
    if td != td2 or cand.shape[0] != nq or tuple(scales.shape) != (nd, dt):
        raise NativeError("maxsim_fp8: shape mismatch")
    maxsim_fp8_check_tokens(entry[4:], td, qt, dt)
    out = torch.empty(cand.shape, dtype=torch.float32, device=qtok.device)
    _check(getattr(load(), entry)(pq, nq, qt, pcd, psc, nd, dt, td, pc, *id_base, cand.shape[1], out.data_ptr(),
                                  _stream()), entry)
    return out


# ------------------------------------------------- child -> parent expansion (thr_hip_parent.h)
def parent_groups(ids: torch.Tensor, counts: Optional[torch.Tensor], parent_of: torch.Tensor, id_base: int = 0):
    """The groups of each fused row ids[q][0 .. counts[q]) under the column ``parent_of`` (int32 [n_docs], -1 = no
    parent) -> (leader i32 [nq, n], slot i32 [nq, n], uniq_ids i64 [nq, n], n_uniq i32 [nq]): thr_hip_parent.h."""
    pi = _dev(ids, torch.int64, "ids", 2)
    pc = _dev(counts, torch.int32, "counts", 1) if counts is not None else None
    pp = _dev(parent_of, torch.int32, "parent_of", 1)
    nq, n = ids.shape
    if counts is not None and counts.shape[0] != nq:
        raise NativeError("parent_groups: one count per query")
    rrf_check_top_k("parent_groups", n)
    leader = torch.empty((nq, n), dtype=torch.int32, device=ids.device)
    slot = torch.empty((nq, n), dtype=torch.int32, device=ids.device)
    uniq = torch.empty((nq, n), dtype=torch.int64, device=ids.device)
    n_uniq = torch.empty(nq, dtype=torch.int32, device=ids.device)
    if nq:
        _check(load().thr_parent_groups(pi, pc, nq, n, pp, parent_of.shape[0], int(id_base), leader.data_ptr(),
                                        slot.data_ptr(), uniq.data_ptr(), n_uniq.data_ptr(), _stream()),
               "thr_parent_groups")
    return leader, slot, uniq, n_uniq


def maxsim_parent_ids(qtok: torch.Tensor, dtok: torch.Tensor, cand_ids: torch.Tensor, id_base: int,
                      parent_of: torch.Tensor, par_rowptr: torch.Tensor, par_child: torch.Tensor) -> torch.Tensor:
    """MaxSim of each query against the PARENT of each candidate -- the token blocks of every row of the candidate's
    family -- over the float16 store in its PACKED image (maxsim_pack); candidates as maxsim_ids."""
    return _maxsim_parent_call("thr_maxsim_parent_ids", maxsim_check_tokens, qtok, (dtok, torch.float16, "dtok", 3), None,
                               cand_ids, id_base, parent_of, par_rowptr, par_child)


def maxsim_parent_fp8_ids(qtok: torch.Tensor, codes: torch.Tensor, scales: torch.Tensor, cand_ids: torch.Tensor,
                          id_base: int, parent_of: torch.Tensor, par_rowptr: torch.Tensor,
                          par_child: torch.Tensor) -> torch.Tensor:
    """maxsim_parent_ids over the FP8 store (maxsim_quantize_fp8's image and scales)."""
    return _maxsim_parent_call("thr_maxsim_parent_fp8_ids", maxsim_fp8_check_tokens, qtok, (codes, torch.uint8, "codes", 3),
                               scales, cand_ids, id_base, parent_of, par_rowptr, par_child)


def _maxsim_parent_call(entry: str, check_tokens, qtok, store, scales, cand_ids, id_base, parent_of, par_rowptr, par_child):
    pq = _dev(qtok, torch.float16, "qtok", 3)
    pst = _dev(*store)
    pc = _dev(cand_ids, torch.int64, "cand_ids", 2)
    pp = _dev(parent_of, torch.int32, "parent_of", 1)
    pr = _dev(par_rowptr, torch.int64, "par_rowptr", 1)
    pch = _dev(par_child, torch.int32, "par_child", 1)
    nq, qt, td = qtok.shape
    nd, dt, td2 = store[0].shape
    if td != td2 or cand_ids.shape[0] != nq or parent_of.shape[0] != nd or par_rowptr.shape[0] < 2:
        raise NativeError(f"{entry[4:]}: shape mismatch")
    sc = ()
    if scales is not None:
        if tuple(scales.shape) != (nd, dt):
            raise NativeError(f"{entry[4:]}: shape mismatch")
        sc = (_dev(scales, torch.float32, "scales", 2),)
    check_tokens(entry[4:], td, qt, dt)
    out = torch.empty(cand_ids.shape, dtype=torch.float32, device=qtok.device)
    _check(getattr(load(), entry)(pq, nq, qt, pst, *sc, nd, dt, td, pc, int(id_base), cand_ids.shape[1], pp, pr, pch,
                                  par_rowptr.shape[0] - 1, par_child.shape[0], out.data_ptr(), _stream()), entry)
    return out


# ------------------------------------------------- diversified top-k (thr_hip_diversify.h)
def mmr_check_dim(what: str, dim: int) -> None:
    """The row length thr_mmr_select takes, refused here with the limits in the message."""
    if not (4 <= int(dim) <= THR_DENSE_ANYDIM_MAX and int(dim) % 4 == 0):
        raise NativeError(f"{what}: dim must be a multiple of 4 in 4 .. {THR_DENSE_ANYDIM_MAX}, got {dim}")


def mmr_check_lam(what: str, lam) -> float:
    """MMR's lambda as thr_mmr_select takes it: a float in [0, 1] (-0.0 and 1.0 are inside, NaN is not)."""
    lam = float(lam)
    if not 0.0 <= lam <= 1.0:       # (NaN fails both)
        raise NativeError(f"{what}: lam must be in [0, 1], got {lam}")
    return lam


def mmr_select(ids: torch.Tensor, scores: torch.Tensor, counts: Optional[torch.Tensor], docs: torch.Tensor,
               dnorm: torch.Tensor, id_base: int, top_k: int, lam: float, want_mmr: bool = True):
    """Maximal Marginal Relevance over each list ids[q][0 .. counts[q]) / scores (float64, best first), the
    similarities from the float32 rows ``docs`` and their float64 norms ``dnorm`` (thr_hip_diversify.h) ->
    (ids i64 [nq, top_k], scores f64 [nq, top_k] -- the original ones, in selection order --, counts i32 [nq],
    pos i32 [nq, top_k], mmr f64 [nq, top_k] or None)."""
    pi = _dev(ids, torch.int64, "ids", 2)
    ps = _dev(scores, torch.float64, "scores", 2)
    pc = _dev(counts, torch.int32, "counts", 1) if counts is not None else None
    pd = _dev(docs, torch.float32, "docs", 2)
    pn = _dev(dnorm, torch.float64, "dnorm", 1)
    nq, n = ids.shape
    nd, dim = docs.shape
    if tuple(scores.shape) != (nq, n) or (counts is not None and counts.shape[0] != nq):
        raise NativeError("mmr_select: one score per id and one count per query")
    if dnorm.shape[0] != nd:
        raise NativeError("mmr_select: dnorm length != n_docs")
    if nd < 1:
        raise NativeError("mmr_select: no rows")
    if pd % 16:
        raise NativeError("mmr_select: docs must be 16-byte aligned")
    if any(t.device != ids.device for t in (scores, docs, dnorm) + (() if counts is None else (counts,))):
        raise NativeError("mmr_select: every operand lives on one device")
    mmr_check_dim("mmr_select", dim)
    rrf_check_top_k("mmr_select (the width of the list)", n)
    if not 1 <= int(top_k) <= n:
        raise NativeError(f"mmr_select: top_k must be in 1 .. {n} (the width of the list), got {top_k}")
    lam = mmr_check_lam("mmr_select", lam)
    dev = ids.device
    out_ids = torch.empty((nq, top_k), dtype=torch.int64, device=dev)
    out_sc = torch.empty((nq, top_k), dtype=torch.float64, device=dev)
    out_pos = torch.empty((nq, top_k), dtype=torch.int32, device=dev)
    out_mmr = torch.empty((nq, top_k), dtype=torch.float64, device=dev) if want_mmr else None
    cnt = torch.empty(nq, dtype=torch.int32, device=dev)
    if nq:
        _check(load().thr_mmr_select(pi, ps, pc, nq, n, pd, pn, nd, dim, int(id_base), lam, int(top_k),
                                     out_ids.data_ptr(), out_sc.data_ptr(), out_pos.data_ptr(),
                                     out_mmr.data_ptr() if want_mmr else None, cnt.data_ptr(), _stream()),
               "thr_mmr_select")
    return out_ids, out_sc, cnt, out_pos, out_mmr


def rerank_order(scores: torch.Tensor, ids: torch.Tensor, counts: Optional[torch.Tensor], top_k: int):
    """scores f32 [nq, n] or [n_lists, nq, n] (per-shard MaxSim lists: -inf where the shard does
    not own the candidate) -> (ids i64 [nq, top_k], scores f64 [nq, top_k], counts i32 [nq]):
    the reference's stable descending sort on ``rerank_score or 0`` (retrieval.py:455)."""
    if scores.dim() == 2:
        scores = scores.unsqueeze(0)
    ps = _dev(scores, torch.float32, "scores", 3)
    pi = _dev(ids, torch.int64, "ids", 2)
    pc = _dev(counts, torch.int32, "counts", 1) if counts is not None else None
    nl, nq, n = scores.shape
    if tuple(ids.shape) != (nq, n):
        raise NativeError("rerank_order: ids shape != scores shape")
    out_ids = torch.empty((nq, top_k), dtype=torch.int64, device=ids.device)
    out_s = torch.empty((nq, top_k), dtype=torch.float64, device=ids.device)
    out_c = torch.empty(nq, dtype=torch.int32, device=ids.device)
    _check(load().thr_rerank_order(ps, nl, nq * n, pi, pc, nq, n, top_k, out_ids.data_ptr(),
                                   out_s.data_ptr(), out_c.data_ptr(), _stream()), "thr_rerank_order")
    return out_ids, out_s, out_c


# ------------------------------------------------------------- multi-GPU
def merge_topk(in_scores: torch.Tensor, in_ids: torch.Tensor, k_out: int):
    """in_* are [n_lists, n_queries, k_in] (the layout an all-gather of each rank's
    [n_queries, k_in] block produces); they may be strided views of one gathered
    [n_lists, 2, n_queries, k_in] tile (same list stride, contiguous [n_queries, k_in] blocks).
    Top k_out of the multiset of entries under (score desc, id asc): the same (score, id) pair in
    two lists comes out twice (disjoint shards never produce one).  -inf / NaN scores and negative
    ids are padding."""
    if in_scores.shape != in_ids.shape or in_scores.dim() != 3:
        raise NativeError("merge: shape mismatch")
    if in_scores.dtype != torch.float64 or in_ids.dtype != torch.int64 or not in_scores.is_cuda:
        raise NativeError("merge: in_scores must be float64, in_ids int64, on the GPU")
    nl, nq, kin = in_scores.shape
    for t in (in_scores, in_ids):
        if t.stride(2) != 1 or t.stride(1) != kin or (nl > 1 and t.stride(0) < nq * kin):
            raise NativeError("merge: lists must be contiguous [n_queries, k_in] blocks")
    if nl > 1 and in_scores.stride(0) != in_ids.stride(0):
        raise NativeError("merge: scores and ids must share the list stride")
    stride = in_scores.stride(0) if nl > 1 else nq * kin
    S, I, cnt, _ = _alloc_out(nq, k_out, in_scores.device)
    _check(load().thr_merge_topk(in_scores.data_ptr(), in_ids.data_ptr(), nq, nl, kin, stride,
                                 k_out, S.data_ptr(), I.data_ptr(), cnt.data_ptr(), _stream()),
           "thr_merge_topk")
    return S, I, cnt
