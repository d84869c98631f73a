"""No GPU: child -> parent expansion.  The new header against its binding table, the shape and argument refusals of
the three entry points (through the library and in a stand-alone sanitized program), the numpy restatement of the
groups on hand-written rows, the built cases' properties (each plant decides its score), the refusals of
set_parents / maxsim(expand=) / retrieve_batch(parents=) over a bare index, the sharded refusals, and the drop-in
client's parent numbering and insert path over a stub."""
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import maxsim_cases as MC  # noqa: E402
import maxsim_fp8_cases as F8  # noqa: E402
import parent_cases as PC  # noqa: E402
import triple_hybrid_rag_amd as T  # noqa: E402
from test_native_abi import ctype_class, declared_symbols, header_class  # noqa: E402
from triple_hybrid_rag_amd import _native as N  # noqa: E402
from triple_hybrid_rag_amd import index_parent as IP  # noqa: E402
from triple_hybrid_rag_amd.backend import GpuIndexClient  # noqa: E402
from triple_hybrid_rag_amd.index import BatchResult, GpuIndex  # noqa: E402
from triple_hybrid_rag_amd.store import CorpusStore  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thr_hip_parent.h")
UNSUPPORTED, INVALID = -2, -1
NAMES = ["thr_maxsim_parent_fp8_ids", "thr_maxsim_parent_ids", "thr_parent_groups"]


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


def test_the_header_and_the_parent_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(N._SIGNATURES_PARENT) == NAMES
    for name, (res, args) in N._SIGNATURES_PARENT.items():
        want_res, want_args = protos[name]
        assert ctype_class(res) == want_res, name
        got = [ctype_class(a) for a in args]
        assert len(got) == len(want_args), f"{name}: {len(got)} argtypes, the header declares {len(want_args)} parameters"
        for i, (g, w) in enumerate(zip(got, want_args)):
            assert g == w, f"{name}: argument {i}"
    lib = N.load()
    for name in protos:
        assert hasattr(lib, name) and getattr(lib, name).argtypes == N._SIGNATURES_PARENT[name][1]
    assert '#include "thr_hip.h"' in open(HEADER).read()
    assert "thr_hip_parent.h" in [os.path.basename(h) for h in T._build._headers()]


def test_thr_hip_h_and_the_other_tables_are_untouched():
    assert len(declared_symbols()) == len(N.EXPORTED_SYMBOLS) == 65 and N.ABI_VERSION == 9
    others = set(N.EXPORTED_SYMBOLS) | set(N._SIGNATURES_GRAPH) | set(N._SIGNATURES_TEXT) | set(N._SIGNATURES_RERANK)
    assert not set(N._SIGNATURES_PARENT) & others
    assert "thr_parent" not in open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    assert "maxsim_parent" not in open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    assert sorted(N._SIGNATURES_RERANK) == ["thr_maxsim_fp8", "thr_maxsim_fp8_ids", "thr_maxsim_quantize_fp8"]
    # every call into the library stays in _native.py
    pkg = os.path.join(ROOT, "triple-hybrid-rag_amd")
    assert not re.search(r"\.thr_[a-z0-9_]+\(", open(os.path.join(pkg, "index_parent.py")).read())


# --------------------------------------------------------------------------- shapes, through null pointers
def c_f16(q_tokens, d_tokens, tok_dim):
    return N.load().thr_maxsim_parent_ids(None, 1, q_tokens, None, 1, d_tokens, tok_dim, None, 0, 1, None, None, None, 1, 1,
                                          None, None)


def c_fp8(q_tokens, d_tokens, tok_dim):
    return N.load().thr_maxsim_parent_fp8_ids(None, 1, q_tokens, None, None, 1, d_tokens, tok_dim, None, 0, 1, None, None,
                                              None, 1, 1, None, None)


def test_each_scorer_takes_its_store_s_tok_dims_dim_by_dim():
    seen16, seen8 = [], []
    for td in range(16, 272 + 1):
        want16 = INVALID if td in N.MAXSIM_TOK_DIMS else UNSUPPORTED
        want8 = INVALID if td in N.MAXSIM_FP8_TOK_DIMS else UNSUPPORTED
        assert (c_f16(32, 32, td), c_fp8(32, 32, td)) == (want16, want8), td
        seen16 += [td] if want16 == INVALID else []
        seen8 += [td] if want8 == INVALID else []
    assert tuple(seen16) == N.MAXSIM_TOK_DIMS == MC.TOK_DIMS and tuple(seen8) == N.MAXSIM_FP8_TOK_DIMS == F8.TOK_DIMS
    for td in (0, -32, 8, 1 << 20, -(1 << 31)):
        assert c_f16(32, 32, td) == c_fp8(32, 32, td) == UNSUPPORTED, td
    assert c_fp8(32, 32, 16) == UNSUPPORTED and c_f16(32, 32, 16) == INVALID


def test_token_counts_sizes_and_null_pointers():
    for n_tok in (0, -32, 1, 31, 33, 48):
        assert c_f16(n_tok, 32, 128) == c_f16(32, n_tok, 128) == UNSUPPORTED
        assert c_fp8(n_tok, 32, 128) == c_fp8(32, n_tok, 128) == UNSUPPORTED
    for n_tok in (32, 64, 96, 160, 512):
        assert c_f16(n_tok, n_tok, 128) == c_fp8(n_tok, n_tok, 128) == INVALID
    lib, p = N.load(), 4096
    good = [p, 1, 32, p, 4, 32, 128, p, 0, 1, p, p, p, 2, 4, p, None]
    for i in (0, 3, 7, 10, 11, 12, 15):         # each pointer
        a = list(good)
        a[i] = None
        assert lib.thr_maxsim_parent_ids(*a) == INVALID, i
    for i in (1, 4, 9, 13, 14):                 # each count
        for v in (0, -1):
            a = list(good)
            a[i] = v
            assert lib.thr_maxsim_parent_ids(*a) == INVALID, i
    a = list(good)
    a[4] = 1 << 31
    assert lib.thr_maxsim_parent_ids(*a) == UNSUPPORTED
    good8 = [p, 1, 32, p, p, 4, 32, 128, p, 0, 1, p, p, p, 2, 4, p, None]
    for i in (0, 3, 4, 8, 11, 12, 13, 16):
        a = list(good8)
        a[i] = None
        assert lib.thr_maxsim_parent_fp8_ids(*a) == INVALID, i
    for i in (1, 5, 10, 14, 15):
        a = list(good8)
        a[i] = 0
        assert lib.thr_maxsim_parent_fp8_ids(*a) == INVALID, i
    # the groups: the width first, then pointers and counts
    g = [p, None, 1, 8, p, 4, 0, p, p, p, p, None]
    for n in (0, -1, N.THR_RRF_MAX_TOP_K + 1):
        a = [None, None, 1, n, None, 4, 0, None, None, None, None, None]
        assert lib.thr_parent_groups(*a) == UNSUPPORTED, n
    for i in (0, 4, 7, 8, 9, 10):
        a = list(g)
        a[i] = None
        assert lib.thr_parent_groups(*a) == INVALID, i
    for i in (2, 5):
        a = list(g)
        a[i] = 0
        assert lib.thr_parent_groups(*a) == INVALID, i


def test_python_wrappers_refuse_host_tensors_and_bad_widths():
    q = torch.zeros((1, 32, 32), dtype=torch.float16)
    d = torch.zeros((2, 32, 32), dtype=torch.float16)
    P, rp, ch = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32)
    ids = torch.zeros((1, 2), dtype=torch.int64)
    for call in (lambda: N.parent_groups(ids, None, P), lambda: N.maxsim_parent_ids(q, d, ids, 0, P, rp, ch),
                 lambda: N.maxsim_parent_fp8_ids(q, d.to(torch.uint8), torch.ones((2, 32)), ids, 0, P, rp, ch)):
        with pytest.raises(N.NativeError, match="expected a CUDA"):
            call()


def test_host_checks_are_clean_under_address_and_ub_sanitizer(tmp_path):
    """The three entries' argument checks, compiled together with a stand-alone program (its own main) with
    the host side under ASan + UBSan, run on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "parent_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "maxsim_parent.hip"),
                    os.path.join(ROOT, "tests", "native", "parent_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "parent host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# --------------------------------------------------------------------------- the restatements
def test_groups_restatement_on_hand_written_rows():
    #            row: 0  1  2   3  4  5
    P = np.array([3, 3, -1, 0, 3, 0], np.int32)
    ids = np.array([[1, 2, 0, 5, 2, 4, 3, -1, 9]], np.int64)      # 2 twice: no parent, never merges; 9: out of range
    leader, slot, uniq, n_uniq = PC.groups_reference(ids, None, P)
    assert leader.tolist() == [[0, 1, 0, 3, 4, 0, 3, 7, 8]]
    assert slot.tolist() == [[0, 1, 0, 2, 3, 0, 2, 4, 5]]
    assert uniq.tolist() == [[1, 2, 5, 2, -1, 9, -1, -1, -1]] and n_uniq.tolist() == [6]
    # a count cuts the row; beyond it leader = slot = -1 and the list is padded
    leader, slot, uniq, n_uniq = PC.groups_reference(ids, [3], P)
    assert leader.tolist() == [[0, 1, 0] + [-1] * 6] and slot.tolist() == [[0, 1, 0] + [-1] * 6]
    assert uniq.tolist() == [[1, 2] + [-1] * 7] and n_uniq.tolist() == [2]
    assert PC.groups_reference(ids, [0], P)[3].tolist() == [0]
    # global ids of a shard at 100: 99 and 106 are another shard's
    ids = np.array([[100, 99, 101, 106, 104]], np.int64)
    leader, slot, uniq, n_uniq = PC.groups_reference(ids, None, P, id_base=100)
    assert leader.tolist() == [[0, 1, 0, 3, 0]] and uniq.tolist() == [[100, 99, 106, -1, -1]] and n_uniq.tolist() == [3]
    assert PC.family(P, 0) == [0, 1, 4] and PC.family(P, 2) == [2] and PC.family(P, 5) == [3, 5]
    rowptr, child = PC.parent_csr(P)
    assert rowptr.tolist() == [0, 2, 2, 2, 5] and child.tolist() == [3, 5, 0, 1, 4]
    assert PC.parent_csr(np.array([-1, -1])) is None
    assert PC.collapse_reference([1, 2, 0, 5, 3], 5, P) == ([0, 1, 3], [1, 2, 5])


def test_group_cases_cover_what_they_are_named_for():
    cases = {name: c for name, *c in PC.group_cases()}
    assert {f"random-n{n}" for n in PC.GROUP_WIDTHS} <= set(cases) and PC.GROUP_WIDTHS == (1, 63, 64, 65, 255, 256, 257, 512)
    for name, (ids, counts, P, base) in cases.items():
        assert ids.dtype == np.int64 and P.dtype == np.int32 and 1 <= ids.shape[1] <= N.THR_RRF_MAX_TOP_K, name
        leader, slot, uniq, n_uniq = PC.groups_reference(ids, counts, P, base)
        n = ids.shape[1]
        for q in range(ids.shape[0]):
            cnt = n if counts is None else min(max(int(counts[q]), 0), n)
            assert np.all(leader[q, cnt:] == -1) and np.all(slot[q, cnt:] == -1) and np.all(uniq[q, n_uniq[q]:] == -1)
            assert np.all(leader[q, :cnt] <= np.arange(cnt)) and n_uniq[q] == len(set(leader[q, :cnt].tolist()))
    assert PC.groups_reference(*cases["one-parent"][:3])[3].tolist() == [1]
    assert PC.groups_reference(*cases["all-distinct"][:3])[3].tolist() == [512]
    assert PC.groups_reference(*cases["all-none"][:3])[3].tolist() == [512]
    leader = PC.groups_reference(*cases["far-pairs"][:3])[0][0]
    assert leader[511] == 0 and leader[64] == 63 and leader[256] == 255 and leader[300] == leader[100] == 7
    ids, counts, P, base = cases["foreign-ids"]
    assert base == 1000 and (ids < 0).sum() > 20 and ((ids >= 0) & (ids < base)).sum() > 5 and (ids >= base + len(P)).sum() > 5
    c = cases["counts-n64"][1]
    assert c.tolist() == [0, 1, 63, 64, 69, -3]
    assert PC.groups_reference(*cases["repeated-ids"][:3])[0].tolist() == [[0, 1, 2, 3, 4, 5]]
    ids, counts, P = PC.many_queries_case(65600)
    assert ids.shape == (65600, 4) and ids.min() < 0 and ids.max() >= len(P) and set(counts.tolist()) == {0, 1, 2, 3, 4}


def test_each_plant_decides_its_score_and_the_layouts_are_what_they_say():
    assert PC.layout("blocks", 3).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2]
    assert PC.layout("interleaved", 2).tolist() == [0, 1, 2, 0, 1, 2]
    P = PC.layout("loner", 2)
    assert P.tolist() == [0, -1, 1, 2, -1, 0, 1, 2, -1] and PC.family(P, 0) == [0, 5]
    for fp8 in (False, True):
        rows = PC.exact_matrix(fp8)
        dims = F8.TOK_DIMS if fp8 else MC.TOK_DIMS
        assert {r[0] for r in rows} == set(dims)
        assert {r[3] for r in rows} >= {1, 2, 3, 4, 5, 33, 257} and {r[5] for r in rows} >= {1, 4, 5, 100, 512}
        assert {(r[2], r[3]) for r in rows} >= {(32, 1), (32, 3), (32, 2), (64, 1), (64, 3), (64, 2)}
        assert {r[1] for r in rows} >= {32, 64, 128} and {r[6] for r in rows} == set(PC.PLANTS)
    for which in PC.PLANTS:
        for kind, fan in (("interleaved", 3), ("loner", 2), ("blocks", 4), ("interleaved", 1)):
            q, d, P, cand, base, planted = PC.exact_case(3, 32, 64, 64, fan, kind, n_cand=5, id_base=40, which=which)
            fam = PC.family(P, 0)
            want_row = {"last": fam[-1], "first": fam[0], "middle": fam[len(fam) // 2]}[which]
            assert planted[0] == want_row and planted[0] in fam
            assert planted[1] == {"last": 63, "first": 0, "middle": 5}[which]
            ref = PC.parent_reference(q, d, P, cand, base)
            less = PC.parent_reference(q, PC.without_plant(d, planted), P, cand, base)
            # query token 0 reaches tok_dim at the plant alone: without it the family's score is lower by an exact,
            # known amount -- tok_dim minus the next best dot product of that query token
            sib = [c for c in range(cand.shape[1]) if 0 <= cand[0, c] - base < len(P) and cand[0, c] - base in fam]
            assert 0 in sib and np.all(ref[0, sib] == ref[0, 0]) and np.all(less[0, sib] < ref[0, sib])
            block = np.concatenate([PC.without_plant(d, planted)[r] for r in fam]).astype(np.float64)
            drop = 32 - (q[0, 0].astype(np.float64) @ block.T).max()
            others = (q[0, 1:].astype(np.float64) @ np.concatenate([d[r] for r in fam]).astype(np.float64).T).max(axis=1).sum()
            assert drop >= 4 and ref[0, 0] == 32 + others
            # every other family is untouched; invalid candidates are -inf in both
            rest = [c for c in range(cand.shape[1]) if c not in sib]
            assert np.array_equal(ref[0, rest], less[0, rest])
            assert ref[0, 1] == -np.inf and ref[-1, 2] == -np.inf and ref[0, 3] == -np.inf
            # the exact family: float16 inputs, multiples of 1/8, and the FP8 store holds them without loss
            assert np.array_equal(d.astype(np.float64) * 8, np.round(d.astype(np.float64) * 8))
            codes, scales = F8.quantise(d)
            assert np.array_equal(F8.dequantise(codes, scales), d.astype(np.float64))
            assert np.array_equal(PC.parent_reference_fp8(q, codes, scales, P, cand, base), ref)


def test_reference_of_a_family_of_one_is_the_plain_reference_and_the_bound_covers_float32():
    rng = np.random.default_rng(8)
    q = rng.standard_normal((2, 32, 64)).astype(np.float16)
    d = rng.standard_normal((6, 32, 64)).astype(np.float16)
    cand = np.array([[0, 1, 5, -1], [3, 2, 9, 4]], np.int64)
    none = np.full(6, -1, np.int32)
    assert np.array_equal(PC.parent_reference(q, d, none, cand), MC.reference(q, d, cand))
    assert np.array_equal(PC.error_bound_parent(q, d, none, cand), MC.error_bound(q, d, cand))
    P = np.array([0, 1, 0, -1, 1, 0], np.int32)
    ref, bound = PC.parent_reference(q, d, P, cand), PC.error_bound_parent(q, d, P, cand)
    assert ref[0, 0] == ref[0, 2] and ref[0, 3] == -np.inf and ref[1, 2] == -np.inf and bound[0, 3] == 0
    assert ref[0, 0] >= MC.reference(q, d, cand)[0, 0]         # a maximum over more tokens
    for qi in range(2):
        for c in range(4):
            if np.isfinite(ref[qi, c]):
                block = np.concatenate([d[r] for r in PC.family(P, int(cand[qi, c]))]).astype(np.float32)
                got = float((q[qi].astype(np.float32) @ block.T).max(axis=1).sum(dtype=np.float32))
                assert 0 < bound[qi, c] < 1e-2 and abs(got - ref[qi, c]) <= bound[qi, c]
    codes, scales = F8.quantise(d)
    b8 = PC.error_bound_parent_fp8(q, codes, scales, P, cand)
    assert np.array_equal(PC.error_bound_parent_fp8(q, codes, scales, none, cand), F8.error_bound_fp8(q, codes, scales, cand))
    assert np.all((b8 > 0) == np.isfinite(ref))


# --------------------------------------------------------------------------- refusals that need no device
def _bare_index(**attrs):
    idx = object.__new__(GpuIndex)
    base = dict(docs=None, dim=0, n_docs=6, lex=None, doc_coll=None, tokens=None, graph=None, _lex_global=False,
                device=torch.device("cpu"), doc_base=0, _attrs={}, _mutations=0)
    base.update(attrs)
    idx.__dict__.update(base)
    return idx


def test_set_parents_is_the_parent_attribute_column():
    idx = _bare_index()
    assert not idx.has_parents()
    with pytest.raises(ValueError, match=r"attribute 'parent': values are >= 0, or -1"):
        idx.set_parents(np.array([0, 1, -2, 0, 1, 0]))
    with pytest.raises(ValueError, match=r"one int32 per row \(6\)"):
        idx.set_parents(np.array([0, 1]))
    assert not idx.has_parents()
    assert idx.set_parents(np.array([2, 0, -1, 0, 2, 2])) is idx
    assert idx.has_parents() and idx.attribute_names() == ["parent"] and idx.attribute("parent").dtype == torch.int32
    # the derived CSR: one owner, keyed on the column's buffer and the mutation count
    rowptr, child = idx.parent_csr()
    want = PC.parent_csr(np.array([2, 0, -1, 0, 2, 2]))
    assert rowptr.tolist() == want[0].tolist() and child.tolist() == want[1].tolist() and child.dtype == torch.int32
    assert idx.parent_csr()[0] is rowptr                       # kept
    idx._mutations += 1
    assert idx.parent_csr()[0] is not rowptr                   # any commit drops it
    idx.set_parents(np.full(6, -1))
    assert idx.parent_csr() is None                            # a new column, no parent anywhere
    ids = torch.tensor([[0, 4, -1, 9, 2]])
    idx.set_parents(np.array([2, 0, -1, 0, 2, 2]))
    assert idx.parents_of(ids).tolist() == [[2, 2, -1, -1, -1]] and idx.parents_of(ids).dtype == torch.int32


def test_maxsim_expand_refusals():
    idx = _bare_index(tokens=torch.zeros((6, 32, 32), dtype=torch.float16), tokens_packed=True)
    q, c = torch.zeros((1, 32, 32), dtype=torch.float16), torch.zeros((1, 2), dtype=torch.int64)
    with pytest.raises(ValueError, match=r"maxsim\(expand='parent'\): this index has no parent column \(set_parents\)"):
        idx.maxsim(q, c, expand="parent")
    with pytest.raises(ValueError, match="expand must be None or 'parent', got 'document'"):
        idx.maxsim(q, c, expand="document")
    idx.set_parents(np.zeros(6, np.int32))
    idx.tokens_packed = False
    with pytest.raises(ValueError, match=r"PACKED float16 store \(set_tokens\(pack=True\)\)"):
        idx.maxsim(q, c, expand="parent")
    idx.tokens = None
    with pytest.raises(ValueError, match="no token store"):
        idx.maxsim(q, c, expand="parent")


def test_retrieve_batch_parents_refusals():
    q = torch.zeros((1, 8))
    idx = _bare_index()
    with pytest.raises(ValueError, match=r"parents must be one of \[None, 'rerank', 'collapse'\], got 'merge'"):
        idx.retrieve_batch(q, parents="merge")
    for mode in ("rerank", "collapse"):
        with pytest.raises(ValueError, match="no parent column"):
            idx.retrieve_batch(q, parents=mode)
    idx.set_parents(np.zeros(6, np.int32))
    with pytest.raises(ValueError, match=r"parents='rerank'\) reranks on the parent score: it needs qtok and a token store"):
        idx.retrieve_batch(q, parents="rerank")
    with pytest.raises(ValueError, match="needs qtok and a token store"):
        idx.retrieve_batch(q, parents="rerank", qtok=torch.zeros((1, 32, 32), dtype=torch.float16))
    idx.tokens, idx.tokens_packed = torch.zeros((6, 32, 32), dtype=torch.float16), False
    for mode in ("rerank", "collapse"):
        with pytest.raises(ValueError, match="PACKED float16 store"):
            idx.retrieve_batch(q, parents=mode, qtok=torch.zeros((1, 32, 32), dtype=torch.float16))
    assert BatchResult(None, None, None).parents is None
    assert list(BatchResult.__dataclass_fields__)[-1] == "parents"


def test_sharded_surfaces_refuse_by_name():
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    sh = object.__new__(ShardedIndex)
    with pytest.raises(NotImplementedError, match=r"ShardedIndex.retrieve_batch: parents='collapse' is not built"):
        sh.retrieve_batch(None, parents="collapse")
    with pytest.raises(NotImplementedError, match="parent_rerank=True is not built for a document-sharded index"):
        ShardedIndexClient(None, None, parent_rerank=True)
    IP.refuse_on_shards("x", parents=None, expand=None)       # nothing asked: nothing refused


# --------------------------------------------------------------------------- the drop-in client over a stub
class _StubIndex:
    """What the client's parent path needs of an index, recorded."""

    def __init__(self, n, tokens=None):
        self.docs, self.dim, self.n_docs = None, 0, n
        self.lex = self.entities = self.graph = self.doc_coll = None
        self.tokens, self.device, self.calls = tokens, torch.device("cpu"), []
        self._attrs = {}

    def attribute_names(self):
        return sorted(self._attrs)

    def attribute(self, name):
        return torch.as_tensor(self._attrs[name])

    def set_parents(self, col):
        self.calls.append(("set_parents", np.asarray(col).tolist()))
        self._attrs["parent"] = np.asarray(col)

    def append_rows(self, **parts):
        self.n_docs += parts["n_rows"]
        self.calls.append(("rows", {k: np.asarray(v).tolist() for k, v in parts.get("attributes", {}).items()}))
        for k, v in parts.get("attributes", {}).items():
            self._attrs[k] = np.concatenate([self._attrs[k], v])

    def maxsim(self, qtok, cand, **kw):
        self.calls.append(("maxsim", cand.tolist(), kw))
        return torch.tensor([[64.0, float("-inf")][:cand.shape[1]]])


class _Embedder:
    def embed_query_tokens(self, query):
        return np.ones((32, 16), np.float16)


def _store(parent_ids):
    n = len(parent_ids)
    return CorpusStore(child_ids=[f"c{i}" for i in range(n)], parent_ids=list(parent_ids),
                       document_ids=["d0"] * n, texts=[f"t{i}" for i in range(n)], pages=[1] * n, modalities=["text"] * n,
                       parents={p: {"id": p, "text": p.upper(), "section_heading": None} for p in parent_ids if p})


def test_client_numbers_parents_by_first_appearance_and_passes_the_column_with_inserts():
    idx, st = _StubIndex(6), _store(["pb", "pa", None, "pb", "pc", "pa"])
    client = GpuIndexClient(idx, st, org_id="acme", parent_rerank=True)
    assert client.parent_rerank and client._parent_code == {"pb": 0, "pa": 1, "pc": 2}
    assert idx.calls == [("set_parents", [0, 1, -1, 0, 2, 1])]
    new = [{"id": "c6", "parent_id": "pa", "document_id": "d0", "text": "x", "page": 1, "modality": "text"},
           {"id": "c7", "parent_id": "pz", "document_id": "d0", "text": "y", "page": 1, "modality": "text"},
           {"id": "c8", "parent_id": None, "document_id": "d0", "text": "z", "page": 1, "modality": "text"},
           {"id": "c9", "parent_id": "pz", "document_id": "d0", "text": "w", "page": 1, "modality": "text"}]
    client.insert_children(new)
    assert idx.calls[-1] == ("rows", {"parent": [1, 3, -1, 3]}) and client._parent_code["pz"] == 3
    assert st.parent_ids[-4:] == ["pa", "pz", None, "pz"]
    # a second client over the same index reads the numbering off the rows (numbers given at inserts never move)
    again = GpuIndexClient(idx, st, org_id="acme", parent_rerank=True)
    assert again._parent_code == client._parent_code and [c[0] for c in idx.calls].count("set_parents") == 1
    st.parent_ids[0] = "pa"
    with pytest.raises(ValueError, match="does not follow the store's parent_ids column"):
        GpuIndexClient(idx, st, org_id="acme", parent_rerank=True)
    st.parent_ids[0] = "pb"
    # maxsim_scores: the parent mode is asked of the index, the / q_tokens normalisation is kept
    idx.tokens = object()
    client.token_embedder = _Embedder()
    assert client.maxsim_scores("q", ["c1", "gone"]) == [2.0, 0.5]
    assert idx.calls[-1] == ("maxsim", [[1, -1]], {"expand": "parent"})
    # the default changes nothing: no column, no argument
    idx2 = _StubIndex(6, tokens=object())
    plain = GpuIndexClient(idx2, _store(["pb", "pa", None, "pb", "pc", "pa"]), org_id="acme", token_embedder=_Embedder())
    assert not plain.parent_rerank and idx2.calls == [] and plain._parent_code == {}
    plain.maxsim_scores("q", ["c1"])
    assert idx2.calls[-1] == ("maxsim", [[1]], {})
    idx2.tokens = None
    plain.insert_children([dict(new[0])])
    assert idx2.calls[-1] == ("rows", {})
