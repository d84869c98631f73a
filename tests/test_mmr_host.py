"""No GPU: diversified top-k (MMR).  The new header against its binding table, every refusal of thr_mmr_select
(through the library with null pointers and in a stand-alone sanitized program), the properties the built cases
are named for, proved from the numpy restatement, the wrong variants of the restatement that each change a named
case, the refusals of GpuIndex.diversify / retrieve_batch(diversify=) over a bare index, the sharded refusals, and
the drop-in client's hook and its fallback over a stub index."""
import logging
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import mmr_cases as MM  # noqa: E402
import triple_hybrid_rag_amd as T  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402
from test_native_abi import ctype_class, declared_symbols, header_class  # noqa: E402
from triple_hybrid_rag_amd import _native as N  # noqa: E402
from triple_hybrid_rag_amd import index_diversify as ID  # noqa: E402
from triple_hybrid_rag_amd.backend import GpuIndexClient  # noqa: E402
from triple_hybrid_rag_amd.index import GpuIndex  # noqa: E402
from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever, RetrievalCandidate  # noqa: E402
from triple_hybrid_rag_amd.store import CorpusStore  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "thr_hip_diversify.h")
UNSUPPORTED, INVALID = -2, -1


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


def test_the_header_and_the_diversify_signature_table_agree():
    protos = _header_prototypes()
    assert sorted(protos) == sorted(N._SIGNATURES_DIVERSIFY) == ["thr_mmr_select"]
    for name, (res, args) in N._SIGNATURES_DIVERSIFY.items():
        want_res, want_args = protos[name]
        assert ctype_class(res) == want_res, name
        got = [ctype_class(a) for a in args]
        assert len(got) == len(want_args) == 18
        for i, (g, w) in enumerate(zip(got, want_args)):
            assert g == w, f"{name}: argument {i}"
    lib = N.load()
    assert lib.thr_mmr_select.argtypes == N._SIGNATURES_DIVERSIFY["thr_mmr_select"][1]
    assert '#include "thr_hip.h"' in open(HEADER).read()
    assert "thr_hip_diversify.h" in [os.path.basename(h) for h in T._build._headers()]
    assert os.path.join(T._build.CSRC, "mmr.hip") in T._build.sources()


def test_thr_hip_h_the_abi_and_the_other_tables_are_untouched():
    assert len(declared_symbols()) == len(N.EXPORTED_SYMBOLS) == 65 and N.ABI_VERSION == 9
    others = (set(N.EXPORTED_SYMBOLS) | set(N._SIGNATURES_GRAPH) | set(N._SIGNATURES_TEXT) | set(N._SIGNATURES_RERANK)
              | set(N._SIGNATURES_PARENT))
    assert not set(N._SIGNATURES_DIVERSIFY) & others
    main = open(os.path.join(ROOT, "include", "thr_hip.h")).read()
    assert "mmr" not in main.lower() and "diversif" not in main.lower()
    # every call into the library stays in _native.py; the entry takes no workspace
    pkg = os.path.join(ROOT, "triple-hybrid-rag_amd")
    for f in ("index_diversify.py", "backend.py", "index.py"):
        assert not re.search(r"\.thr_mmr[a-z0-9_]*\(", open(os.path.join(pkg, f)).read()), f
    src = open(os.path.join(pkg, "csrc", "mmr.hip")).read()
    assert "Arena" not in src and "workspace" not in src and "atomic" not in src.replace("No atomics", "")
    assert MM.SCORE_MAX == 1e300 and "MMR_SCORE_MAX = 1e300" in src


# --------------------------------------------------------------------------- refusals, through null pointers
def _c(n_queries=1, n=8, n_docs=4, dim=64, lam=0.5, top_k=4, ptr=None, **over):
    a = dict(ids=ptr, scores=ptr, counts=None, docs=ptr, dnorm=ptr, out_ids=ptr, out_scores=ptr, out_pos=ptr, out_mmr=None,
             out_counts=ptr)
    a.update(over)
    return N.load().thr_mmr_select(a["ids"], a["scores"], a["counts"], n_queries, n, a["docs"], a["dnorm"], n_docs, dim, 7,
                                   lam, top_k, a["out_ids"], a["out_scores"], a["out_pos"], a["out_mmr"], a["out_counts"],
                                   None)


def test_shapes_are_refused_before_any_pointer_value_by_value():
    for dim in range(-8, N.THR_DENSE_ANYDIM_MAX + 9):
        ok = 4 <= dim <= N.THR_DENSE_ANYDIM_MAX and dim % 4 == 0
        assert _c(dim=dim) == (INVALID if ok else UNSUPPORTED), dim
    for dim in (-(1 << 31), (1 << 31) - 1, 1 << 20):
        assert _c(dim=dim, ptr=4096) == UNSUPPORTED
    for n in range(-2, N.THR_RRF_MAX_TOP_K + 3):
        ok = 1 <= n <= N.THR_RRF_MAX_TOP_K
        assert _c(n=n, top_k=1) == (INVALID if ok else UNSUPPORTED), n
        if ok:
            for k, good in ((0, False), (-1, False), (1, True), (n, True), (n + 1, False)):
                assert _c(n=n, top_k=k) == (INVALID if good else UNSUPPORTED), (n, k)
    assert _c(n_docs=(1 << 31) - 1) == INVALID
    for nd in (1 << 31, (1 << 63) - 1):
        assert _c(n_docs=nd) == _c(n_docs=nd, ptr=4096) == UNSUPPORTED
    assert N.THR_RRF_MAX_TOP_K == 512 and N.THR_DENSE_ANYDIM_MAX == 4096


def test_null_pointers_counts_and_lam_are_invalid():
    p = 4096
    for name in ("ids", "scores", "docs", "dnorm", "out_ids", "out_scores", "out_pos", "out_counts"):
        assert _c(ptr=p, counts=p, out_mmr=p, **{name: None}) == INVALID, name
    for v in (0, -1, -(1 << 31)):
        assert _c(ptr=p, n_queries=v) == INVALID and _c(ptr=p, n_docs=v) == INVALID
    one_up = math.nextafter(1.0, 2.0)
    for lam in (math.nextafter(0.0, -1.0), -1.0, one_up, 2.0, math.inf, -math.inf, math.nan):
        assert _c(ptr=p, lam=lam) == INVALID, lam
        assert _c(ptr=p, lam=lam, dim=6) == UNSUPPORTED       # the shape is looked at first
        with pytest.raises(N.NativeError, match=r"lam must be in \[0, 1\]"):
            N.mmr_check_lam("x", lam)
        with pytest.raises(ValueError, match=r"diversify is None or a float in \[0, 1\]"):
            ID.check_lam("x", lam)
    # -0.0 and 1.0 are inside: nothing but the missing pointers is wrong with these calls
    for lam in (-0.0, 0.0, 1.0, math.nextafter(1.0, 0.0)):
        assert _c(lam=lam) == INVALID
        assert N.mmr_check_lam("x", lam) == lam and ID.check_lam("x", lam) == lam
    with pytest.raises(ValueError, match="got 'half'"):
        ID.check_lam("x", "half")
    with pytest.raises(ValueError, match="got True"):
        ID.check_lam("x", True)


def test_python_wrapper_refuses_host_tensors():
    ids, sc = torch.zeros((1, 4), dtype=torch.int64), torch.zeros((1, 4), dtype=torch.float64)
    with pytest.raises(N.NativeError, match="expected a CUDA"):
        N.mmr_select(ids, sc, None, torch.zeros((3, 8)), torch.ones(3, dtype=torch.float64), 0, 2, 0.5)
    with pytest.raises(N.NativeError, match=r"dim must be a multiple of 4 in 4 \.\. 4096, got 6"):
        N.mmr_check_dim("x", 6)


def test_host_checks_are_clean_under_address_and_ub_sanitizer(tmp_path):
    """The entry's argument checks, compiled together with a stand-alone program (its own main) with the host
    side under ASan + UBSan, run on the CPU."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = str(tmp_path / "mmr_host_check")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host",
                    "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined",
                    os.path.join(ROOT, "triple-hybrid-rag_amd", "csrc", "mmr.hip"),
                    os.path.join(ROOT, "tests", "native", "mmr_host_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and "mmr host check: ok" in run.stdout, run.stdout + run.stderr
    assert "runtime error" not in run.stderr and "AddressSanitizer" not in run.stderr


# --------------------------------------------------------------------------- the restatement
def _one_query_by_the_letter(c: MM.Case, q: int):
    """The contract once more, one query, scalar Python over oracle.seq_dot_f64: what the batch restatement must equal."""
    n = c.ids.shape[1]
    cnt = n if c.counts is None else min(max(int(c.counts[q]), 0), n)
    cand = [p for p in range(cnt) if math.isfinite(c.scores[q, p]) and abs(c.scores[q, p]) <= 1e300]
    row = {}
    for p in cand:
        g = int(c.ids[q, p])
        if c.id_base <= g < c.id_base + len(c.docs) and c.dnorm[g - c.id_base] > 0:
            row[p] = g - c.id_base
    if not cand:
        return [], []
    lo, hi = min(c.scores[q, p] for p in cand), max(c.scores[q, p] for p in cand)
    rel = {p: 1.0 if hi == lo else float((c.scores[q, p] - lo) / (hi - lo)) for p in cand}
    lam, oml = np.float64(c.lam), np.float64(1.0) - np.float64(c.lam)
    pen = {p: -math.inf for p in cand}
    picked, values = [], []
    for t in range(min(len(cand), c.top_k)):
        best = None
        for p in cand:
            if p in picked:
                continue
            v = lam * np.float64(rel[p]) if t == 0 else lam * np.float64(rel[p]) - oml * np.float64(pen[p])
            if best is None or v > best[0]:
                best = (v, p)
        picked.append(best[1])
        values.append(float(best[0]))
        s = best[1]
        for p in cand:
            sim = 0.0
            if p in row and s in row:
                sim = float(O.seq_dot_f64(c.docs[row[p]][None], c.docs[row[s]])[0] / (c.dnorm[row[p]] * c.dnorm[row[s]]))
            if sim > pen[p]:
                pen[p] = sim
    return picked, values


@pytest.mark.parametrize("name", ["duplicates", "negative-sims", "rowless", "duplicate-ids", "unusable-scores", "counts",
                                  "order-sensitive", "lam-0.0", "lam-0.999", "shape-n65-k65-d36-big"])
def test_the_batch_restatement_is_the_contract_by_the_letter(name):
    c, ref = MM.case(name), MM.expected(name)
    for q in range(c.ids.shape[0]):
        picked, values = _one_query_by_the_letter(c, q)
        k = len(picked)
        assert ref.counts[q] == k and ref.pos[q, :k].tolist() == picked
        assert ref.mmr[q, :k].view(np.int64).tolist() == np.array(values).view(np.int64).tolist()
        assert ref.ids[q, :k].tolist() == c.ids[q, picked].tolist()
        assert ref.scores[q, :k].view(np.int64).tolist() == c.scores[q, picked].view(np.int64).tolist()
        assert np.all(ref.ids[q, k:] == -1) and np.all(ref.pos[q, k:] == -1)
        assert np.all(ref.scores[q, k:] == -np.inf) and np.all(ref.mmr[q, k:] == -np.inf)


def test_every_case_is_small_well_typed_and_selects_distinct_candidates():
    assert set(MM.NAMES) >= {"duplicates", "exact-ties", "negative-sims", "order-sensitive", "rowless", "duplicate-ids",
                             "unusable-scores", "all-equal", "offset-scores", "counts", "counts-null", "many-queries", "real"}
    assert {f"lam-{v}" for v in (1.0, 0.0, 0.5, 0.999)} <= set(MM.NAMES)
    shapes = [MM.case(MM.shape_name(s)) for s in MM.SHAPES]
    assert {c.ids.shape[1] for c in shapes} >= set(MM.NS) == {1, 2, 63, 64, 65, 100, 512}
    assert {c.docs.shape[1] for c in shapes} == set(MM.DIMS) | {64} == {4, 36, 64, 768, 1024, 4000, 4096}
    for n in MM.NS:
        assert {c.top_k for c in shapes if c.ids.shape[1] == n} >= {1, min(10, n), n} - ({10} if n < 10 else set()), n
    assert {c.id_base for c in shapes} == {0, MM.BIG_BASE}
    assert any(c.ids.shape[1] == c.top_k == 512 and c.docs.shape[1] == 64 for c in shapes)
    assert any(c.ids.shape[1] == 40 and c.docs.shape[1] == 4096 for c in shapes)
    big = MM.case("many-queries")
    assert big.ids.shape == (65600, 4) and big.docs.shape[1] == 4 and set(big.counts.tolist()) == {0, 1, 2, 3, 4}
    real = MM.case("real")
    assert real.ids.shape == (64, 100) and real.docs.shape == (3000, 768) and real.top_k == 10
    for name in MM.NAMES:
        c, ref = MM.case(name), MM.expected(name)
        nq, n = c.ids.shape
        assert c.scores.shape == (nq, n) and c.dnorm.shape == (len(c.docs),) and 1 <= c.top_k <= n <= 512, name
        assert c.docs.shape[1] % 4 == 0 and np.all(np.isfinite(c.docs))
        for q in range(min(nq, 50)):
            k = int(ref.counts[q])
            assert len(set(ref.pos[q, :k].tolist())) == k and np.all(ref.pos[q, :k] >= 0), name


def test_duplicates_one_member_per_cluster_before_any_second():
    c, ref = MM.case("duplicates"), MM.expected("duplicates")
    assert sorted(MM.cluster_of(c, ref.pos[0, :MM.CLUSTERS]).tolist()) == list(range(MM.CLUSTERS))
    # the rows are what they say: byte-identical pairs and near-identical ones under distinct ids
    assert np.array_equal(c.docs[0], c.docs[1]) and not np.array_equal(c.docs[0], c.docs[2])
    assert len(set(c.ids[0].tolist())) == MM.CLUSTERS * MM.MEMBERS
    # the plain truncation would have handed out two members of each cluster
    assert sorted(MM.cluster_of(c, np.arange(10)).tolist()) == sorted(list(range(MM.CLUSTERS)) * 2)


def test_lam_one_is_the_input_prefix_and_lam_zero_is_pure_diversity():
    one = MM.expected("lam-1.0")
    assert np.array_equal(one.pos, np.tile(np.arange(10, dtype=np.int32), (3, 1)))
    c, zero = MM.case("lam-0.0"), MM.expected("lam-0.0")
    assert np.all(zero.pos[:, 0] == 0) and np.all(zero.mmr[:, 0] == 0.0)          # step 0: every value is 0.0
    for q in range(3):
        # step 1: the candidate least similar to the first pick, whatever its score
        sims = O.seq_dot_f64(c.docs[c.ids[q]], c.docs[c.ids[q, 0]]) / (c.dnorm[c.ids[q]] * c.dnorm[c.ids[q, 0]])
        sims[0] = np.inf
        assert zero.pos[q, 1] == np.argmin(sims) and zero.mmr[q, 1] == -sims.min()
    assert not np.array_equal(MM.expected("lam-0.5").pos, one.pos)
    assert not np.array_equal(MM.expected("lam-0.999").pos, MM.expected("lam-0.5").pos)


def test_exact_ties_go_to_the_lowest_position_on_both_sides_of_64_and_256():
    c, ref = MM.case("exact-ties"), MM.expected("exact-ties")
    k = int(ref.counts[0])
    straddled = set()
    for t in range(k):
        p = int(ref.pos[0, t])
        still_open = [x for x in range(512) if x not in ref.pos[0, :t].tolist() and x != p]
        twins = [x for x in still_open if c.scores[0, x] == c.scores[0, p]
                 and np.array_equal(c.docs[c.ids[0, x]], c.docs[c.ids[0, p]])]
        # a twin has the same rel and the same pen, bit for bit: an exact tie, and the lowest position was taken
        assert all(x > p for x in twins), (t, p)
        straddled |= {edge for edge in (64, 256) if any(p < edge <= x for x in twins)}
    assert straddled == {64, 256}


def test_negative_similarities_are_not_clipped():
    c, ref = MM.case("negative-sims"), MM.expected("negative-sims")
    # position 0 (row 0) first; its opposite (row 1, position 3) has sim -1: value = lam * rel + 0.5 beats the rest
    assert ref.pos[0, 0] == 0 and ref.pos[0, 1] == 3 and np.array_equal(c.docs[1], -c.docs[0])
    rel = (c.scores[0, 3] - c.scores[0, -1]) / (c.scores[0, 0] - c.scores[0, -1])
    sim = O.seq_dot_f64(c.docs[1][None], c.docs[0])[0] / (c.dnorm[1] * c.dnorm[0])
    assert abs(sim + 1.0) < 1e-15 and ref.mmr[0, 1] == 0.5 * rel - 0.5 * sim and ref.mmr[0, 1] > 0.5 * rel + 0.49


def test_the_order_of_the_sum_decides_the_planted_near_tie():
    c, ref = MM.case("order-sensitive"), MM.expected("order-sensitive")
    n = MM.ORDER_N
    a, b, s = c.docs[n - 1], c.docs[n - 2], c.docs[0]
    assert np.array_equal(a[::-1], b) and len(set(s.tolist())) == 1 and c.dnorm[n - 1] == c.dnorm[n - 2]
    seq = O.seq_dot_f64(np.stack([b, a]), s)
    rev = O.seq_dot_f64(np.stack([b[::-1], a[::-1]]), s[::-1])
    pw = (np.stack([b, a]).astype(np.float64) * s.astype(np.float64)).sum(axis=-1)
    assert seq[0] != seq[1] and rev[0] == seq[1] and rev[1] == seq[0]      # the same real sum, other bits
    assert abs(seq[0] - seq[1]) < 1e-9 * abs(seq[0]) and (seq[1] < seq[0]) and not (pw[1] < pw[0])
    assert ref.pos[0].tolist() == [0, n - 1] and ref.ids[0, 1] == c.id_base + n - 1


WRONG = {"clip_pen": "negative-sims", "ties_high": "exact-ties", "pairwise": "order-sensitive",
         "reverse_sum": "order-sensitive", "raw_rel": "offset-scores", "skip_rowless": "rowless"}


@pytest.mark.parametrize("variant", sorted(WRONG))
def test_each_wrong_variant_changes_its_named_case(variant):
    name = WRONG[variant]
    right, wrong = MM.expected(name), MM.reference(MM.case(name), **{variant: True})
    assert not np.array_equal(right.ids, wrong.ids), (variant, name)
    if variant in ("pairwise", "reverse_sum"):
        n = MM.ORDER_N
        assert wrong.pos[0].tolist() == [0, n - 2]             # B instead of A: the selected id changes with the bits
    if variant == "skip_rowless":
        assert wrong.counts[0] < right.counts[0]


def test_rowless_candidates_stay_selectable_and_are_similar_to_nothing():
    c, ref = MM.case("rowless"), MM.expected("rowless")
    rowless = [p for p in range(24) if not (c.id_base <= c.ids[0, p] < c.id_base + 50) or c.dnorm[c.ids[0, p] - c.id_base] == 0]
    assert len(rowless) == 11 and {int(c.ids[0, p]) for p in rowless} >= {-1, -7, 999, 5, 0, 1050, 1051, 1003, 1017}
    assert ref.counts[0] == 24 and sorted(ref.pos[0].tolist()) == list(range(24))
    # behind the first pick a rowless candidate's penalty is exactly 0.0
    t = next(t for t in range(1, 24) if int(ref.pos[0, t]) in rowless)
    p = int(ref.pos[0, t])
    rel = (c.scores[0, p] - c.scores[0].min()) / (c.scores[0].max() - c.scores[0].min())
    assert ref.mmr[0, t] == 0.5 * rel - 0.5 * 0.0


def test_duplicate_ids_unusable_scores_equal_scores_and_counts():
    c, ref = MM.case("duplicate-ids"), MM.expected("duplicate-ids")
    assert ref.counts[0] == 16 and sorted(ref.pos[0].tolist()) == list(range(16))
    first4 = ref.pos[0].tolist().index(0)
    later4 = [ref.pos[0].tolist().index(p) for p in (2, 7, 14)]         # the same id again: sim 1, picked late
    assert all(t > first4 for t in later4) and len(set(c.ids[0].tolist())) < 16
    c, ref = MM.case("unusable-scores"), MM.expected("unusable-scores")
    assert ref.counts[0] == 16 - len(MM.UNUSABLE) and not set(ref.pos[0, :11].tolist()) & set(MM.UNUSABLE)
    assert {0, 15} <= set(ref.pos[0, :11].tolist()) and np.all(ref.pos[0, 11:] == -1) and np.all(ref.ids[0, 11:] == -1)
    assert np.all(np.isfinite(ref.mmr[0, :11]))
    c, ref = MM.case("all-equal"), MM.expected("all-equal")
    assert np.all(ref.pos[:, 0] == 0) and np.all(ref.mmr[:, 0] == 0.5) and np.all(ref.counts == 10)    # rel = 1.0
    c, ref = MM.case("counts"), MM.expected("counts")
    assert ref.counts.tolist() == [0, 1, 4, 5, 5, 5, 0, 5] and MM.COUNTS == (0, 1, 4, 5, 12, 15, -3, 7)
    for q, cnt in enumerate(MM.COUNTS):
        assert np.all(ref.pos[q, :ref.counts[q]] < max(cnt, 0))
    assert MM.expected("counts-null").counts.tolist() == [5] * 8 and MM.case("counts-null").counts is None


# --------------------------------------------------------------------------- refusals that need no device
def _bare_index(**attrs):
    idx = object.__new__(GpuIndex)
    base = dict(docs=None, dnorm=None, dim=0, n_docs=6, lex=None, doc_coll=None, tokens=None, graph=None,
                _lex_global=False, device=torch.device("cpu"), doc_base=0, _attrs={}, _mutations=0)
    base.update(attrs)
    idx.__dict__.update(base)
    return idx


def test_an_index_without_dense_rows_refuses_in_plain_words():
    idx = _bare_index()
    ids, sc = torch.zeros((1, 4), dtype=torch.int64), torch.zeros((1, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"diversify: this index has no dense rows"):
        idx.diversify(ids, sc, top_k=2)
    with pytest.raises(ValueError, match=r"retrieve_batch\(diversify=\): this index has no dense rows"):
        idx.retrieve_batch(torch.zeros((1, 8)), diversify=0.5)
    for bad in (1.5, -0.1, math.nan, "x"):
        with pytest.raises(ValueError, match=r"retrieve_batch: diversify is None or a float in \[0, 1\]"):
            idx.retrieve_batch(torch.zeros((1, 8)), diversify=bad)
    idx = _bare_index(docs=torch.zeros((6, 8)), dnorm=torch.ones(6, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"diversify: diversify is None or a float in \[0, 1\]"):
        idx.diversify(ids, sc, top_k=2, lam=1.01)
    with pytest.raises(N.NativeError, match="expected a CUDA"):          # past the refusals: the binding's own check
        idx.diversify(ids, sc, top_k=2)
    import inspect
    assert list(inspect.signature(GpuIndex.retrieve_batch).parameters)[-1] == "diversify"
    assert inspect.signature(GpuIndex.retrieve_batch).parameters["diversify"].default is None


def test_sharded_surfaces_refuse_by_name_with_a_message_of_their_own():
    from triple_hybrid_rag_amd.distributed import ShardedIndex
    from triple_hybrid_rag_amd.sharded_client import ShardedIndexClient
    sh = object.__new__(ShardedIndex)
    with pytest.raises(NotImplementedError, match=r"ShardedIndex.retrieve_batch: diversify=0.5 is not built .* dense rows"):
        sh.retrieve_batch(None, diversify=0.5)
    with pytest.raises(NotImplementedError, match=r"a sharded index client: diversify=0.3 is not built"):
        ShardedIndexClient(None, None, diversify=0.3)
    try:
        sh.retrieve_batch(None, diversify=0.5)
    except NotImplementedError as e:
        assert "parent" not in str(e) and "family" not in str(e)
    ID.refuse_diversify_on_shards("x", None)


# --------------------------------------------------------------------------- the drop-in client over a stub
class _StubIndex:
    def __init__(self, n, docs=True, fail=False):
        self.docs, self.dim, self.n_docs = (object() if docs else None), 0, n
        self.lex = self.entities = self.graph = self.doc_coll = self.tokens = None
        self.device, self.calls, self.fail = torch.device("cpu"), [], fail

    def attribute_names(self):
        return []

    def diversify(self, ids, scores, counts=None, top_k=10, lam=0.5):
        self.calls.append((ids.tolist(), scores.tolist(), counts, top_k, lam))
        if self.fail:
            raise RuntimeError("device lost")
        assert ids.dtype == torch.int64 and scores.dtype == torch.float64
        pos = torch.tensor([list(range(ids.shape[1]))[::-1][:top_k]], dtype=torch.int32)      # the list backwards
        return None, None, torch.tensor([top_k], dtype=torch.int32), pos, None


def _store(n):
    return CorpusStore(child_ids=[f"c{i}" for i in range(n)], parent_ids=[None] * n, document_ids=["d0"] * n,
                       texts=[f"t{i}" for i in range(n)], pages=[1] * n, modalities=["text"] * n, parents={})


def _cand(i, rrf, rerank=None):
    return RetrievalCandidate(child_id=f"c{i}", parent_id="", document_id="d0", text=f"t{i}", page=1, modality="text",
                              rrf_score=rrf, rerank_score=rerank)


def _retriever(client):
    r = RAG2Retriever(org_id="acme", embedder=object(), query_planner=object())
    r._supabase = client
    return r


def test_client_hook_orders_the_final_cut_and_falls_back(caplog):
    idx = _StubIndex(6)
    client = GpuIndexClient(idx, _store(6), org_id="acme", diversify=0.25)
    assert client.diversify == 0.25
    assert client.mmr_order(["c4", "gone", "c0"], [0.9, 0.8, 0.7], 2) == [2, 1]
    assert idx.calls[-1] == ([[4, -1, 0]], [[0.9, 0.8, 0.7]], None, 2, 0.25)
    assert client.mmr_order(["c1", "c2"], [0.9, 0.8], 7) == [1, 0] and idx.calls[-1][3] == 2      # top_k <= the list
    assert client.mmr_order([], [], 3) == [] and client.mmr_order(["c1"], [1.0], 0) == []
    with pytest.raises(ValueError, match="one score per child id"):
        client.mmr_order(["c1", "c2"], [1.0], 1)
    # the retriever: threshold, floor and max score as before, then the hook's order instead of the prefix;
    # the relevance handed over is _effective_score (a rerank score of 0.0 falls through to the RRF score)
    cands = [_cand(0, 0.1, 0.9), _cand(1, 0.85, 0.0), _cand(2, 0.1, 0.8), _cand(3, 0.1, 0.7), _cand(4, 0.1, 0.2)]
    final, refused, reason, best = _retriever(client)._apply_safety(list(cands), 3)
    assert (refused, reason, best) == (False, None, 0.9)
    assert idx.calls[-1] == ([[0, 1, 2, 3]], [[0.9, 0.85, 0.8, 0.7]], None, 3, 0.25)      # c4 fell under 0.6 * 0.9
    assert [c.child_id for c in final] == ["c3", "c2", "c1"]
    # refusals and single survivors never reach the hook
    calls = len(idx.calls)
    assert _retriever(client)._apply_safety([_cand(0, 0.1, 0.5)], 3)[1:3] == (True, "Max score 0.50 below threshold 0.6")
    assert _retriever(client)._apply_safety([], 3)[1] is True
    assert [c.child_id for c in _retriever(client)._apply_safety([_cand(0, 0.1, 0.9), _cand(1, 0.1, 0.1)], 3)[0]] == ["c0"]
    assert len(idx.calls) == calls
    # a failing hook: a warning, and the reference's truncation
    bad = GpuIndexClient(_StubIndex(6, fail=True), _store(6), org_id="acme", diversify=0.25)
    with caplog.at_level(logging.WARNING):
        final = _retriever(bad)._apply_safety(list(cands), 3)[0]
    assert [c.child_id for c in final] == ["c0", "c1", "c2"] and "Diversified cut failed: device lost" in caplog.text
    # without the argument: no hook, the truncation
    plain_idx = _StubIndex(6)
    plain = GpuIndexClient(plain_idx, _store(6), org_id="acme")
    assert plain.diversify is None
    assert [c.child_id for c in _retriever(plain)._apply_safety(list(cands), 3)[0]] == ["c0", "c1", "c2"]
    assert plain_idx.calls == []
    with pytest.raises(RuntimeError, match="made without diversify="):
        plain.mmr_order(["c1"], [1.0], 1)
    # refused at construction: a lambda outside [0, 1], an index without dense rows
    with pytest.raises(ValueError, match=r"GpuIndexClient: diversify is None or a float in \[0, 1\]"):
        GpuIndexClient(_StubIndex(6), _store(6), org_id="acme", diversify=1.5)
    with pytest.raises(ValueError, match="the index has no dense rows"):
        GpuIndexClient(_StubIndex(6, docs=False), _store(6), org_id="acme", diversify=0.5)
