"""Every dense scan against the float64 oracle at the QUERY's value edges (tests/dense_query_cases.py):
float16 images that are all zero, hold an infinity or sit in float16's subnormals, float32 values at the
ends of float32's range -- mixed into every query tile of the 70 planted queries.

The dense channel promises the oracle's bits for every finite query.  The scans keep it through the
certificate  |scan score - cosine| <= eps32 + ea (1 + eq) + eq,  eq = ||fp16(q) - q|| / ||q||  (qerr),  and
a query the certificate cannot cover is redone exhaustively.  A rescued query passes whatever the scan
did, so every (mode, shape) is checked in steps, on one raw call kept per case:

  a  a query the raw entry point certifies already IS the oracle's (soundness);
  b  which queries may lack the certificate, so that (a) is not vacuous;
  c  an edge query costs the ordinary queries of its tile nothing (the same flags with the edge
     queries zeroed);
  d  dense_search, rescue included, is the oracle's for the whole batch;
  e  qerr, read from the workspace, against eq recomputed in float64 (f16 modes);
  f  an edge query alone in its batch (sampled shapes).

Shapes: the smallest that reach each path -- 3001 rows (no sample pass), 20011 / 9001 (sampled); dims
512 / 768 (dense_scan_f16qs, pack_queries_f16 <= 768), 1024 (dense_scan_f16q), 96 (dense_scan_anydim).
k = 100, k' = 192, doc_base != 0.  One oracle run per shape, shared and left unchanged.
"""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from dense_cases import DOC_BASE, TIE_QUERY, ZERO_QUERY, assert_topk_equal, dev, floor_search, planted  # noqa: E402
from dense_emit_cases import carve  # noqa: E402
from dense_query_cases import CLASSES, carve_rows32, catalogue, eq_f64, is_edge, representatives  # noqa: E402

K, KP = 100, 192
F16_MODES = ("f16", "f16-inline", "f16-anydim")
# (mode, n, d); the copy scan is "copy" in the test ids, so that -k can pick it alone
CASES = [("f16", 3001, 512), ("f16", 20011, 768), ("f16", 9001, 1024),
         ("f16-inline", 3001, 512), ("f16-inline", 20011, 768), ("f16-inline", 9001, 1024),
         ("f16-anydim", 3001, 96), ("f16-anydim", 20011, 96),
         ("f32", 3001, 768), ("f32", 20011, 768),
         ("exact", 3001, 512)]


def case_id(case):
    mode, n, d = case
    return f"{'copy' if mode == 'f16' else mode}-{n}x{d}"


every_case = pytest.mark.parametrize("case", CASES, ids=case_id)
f16_cases = pytest.mark.parametrize("case", [c for c in CASES if c[0] in F16_MODES], ids=case_id)
sampled_cases = pytest.mark.parametrize("case", [c for c in CASES if c[1] > 8192], ids=case_id)


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


@functools.lru_cache(maxsize=None)
def oracle(n, d):
    x, _ = planted(n, d)
    q = catalogue(n, d)[0]
    return CO.dense_topk_exact(x, q, K, doc_id_base=DOC_BASE)


_index = {}


def index(T, mode, n, d):
    if (mode, n, d) not in _index:
        _index[(mode, n, d)] = T.GpuIndex(doc_base=DOC_BASE).set_dense(planted(n, d)[0], shortlist=mode)
    return _index[(mode, n, d)]


def raw_call(T, idx, mode, qd, ws=None, k=K):
    """The scan's entry point itself: (S, I, cnt, flags) before any rescue."""
    N = T._native
    if mode == "exact":
        return N.dense_topk_exact(idx.docs, idx.dnorm, qd, k, DOC_BASE)
    if mode == "f32":
        return N.dense_topk(idx.docs, idx.dnorm, idx.inv_norm, qd, k, KP, DOC_BASE, ws)
    with N.dense_f16_flavour(mode == "f16-anydim"):
        return N.dense_topk_f16(idx.docs, idx.docs16, idx.doc_rel_err, idx.dnorm, idx.inv_norm, qd, k, KP,
                                DOC_BASE, ws)


def qerr_of(T, mode, ws, n, d, nq):
    """qerr[0, qpad) of the raw call that ran on `ws`: the packed batch's carve, or the one of a batch
    over float32 rows (dense_query_cases.carve_rows32, held to the library by the host test)."""
    N = T._native
    if mode == "f16":
        where, total, qpad = carve(N.dense_f16_query_tile(d, True, nq), nq, d)
    else:
        where, total, qpad = carve_rows32(N.dense_f16_query_tile(d, False, nq), nq, n, KP)
    assert total <= ws.numel()
    off, nbytes = where["qerr"]
    return ws[off:off + nbytes].view(torch.float32).cpu().numpy().astype(np.float64)


class Run:
    pass


_runs = {}


def run(T, case):
    """The raw call on the catalogue, the same call with every edge query zeroed, and dense_search --
    once per case, shared by the steps."""
    if case in _runs:
        return _runs[case]
    mode, n, d = case
    N = T._native
    idx = index(T, mode, n, d)
    q, names, classes, bases = catalogue(n, d)
    edge = is_edge(names)
    r = Run()
    r.names, r.classes, r.bases, r.edge, r.q = names, np.array(classes), np.array(bases), edge, q
    ws = None
    if mode != "exact":
        size = N.dense_workspace_bytes if mode == "f32" else N.dense_f16_workspace_bytes
        ws = torch.empty(size(n, d, len(q), KP), dtype=torch.uint8, device="cuda")
        ws.fill_(0xFF)
    S, I, cnt, flg = raw_call(T, idx, mode, dev(q), ws)
    torch.cuda.synchronize()
    r.raw = (S, I, cnt)
    r.flags = flg.cpu().numpy()
    r.qerr = qerr_of(T, mode, ws, n, d, len(q)) if mode in F16_MODES else None
    q0 = q.copy()
    q0[edge] = 0
    if ws is not None:
        ws.fill_(0xFF)
    r.flags_zeroed = raw_call(T, idx, mode, dev(q0), ws)[3].cpu().numpy()
    r.search = idx.dense_search(dev(q), K, kprime=KP)
    _runs[case] = r
    cert = (r.flags & 1) != 0
    ratio = ""
    if r.qerr is not None:
        e = np.array([eq_f64(v) for v in q])
        fin = np.isfinite(e) & (e > 0)
        ratio = f" max qerr/eq {np.max(r.qerr[:len(q)][fin] / e[fin]):.9f}"
    print(f"\nRECORD {case_id(case)}: certified before the rescue: {int(cert.sum())} of {len(q)}; edge positions "
          f"certified {np.nonzero(cert & edge)[0].tolist()}; ordinary uncertified {np.nonzero(~cert & ~edge)[0].tolist()}; "
          f"overflow flags {np.nonzero(r.flags & N.THR_FLAG_OVERFLOW)[0].tolist()}; n_rescued {r.search[3]};{ratio}")
    return r


@every_case
def test_a_certified_before_the_rescue_is_already_the_oracle(T, case):
    """Soundness: whatever the raw entry point certifies equals the oracle in ids, score bits, count and
    -1 padding -- no rescue has run yet."""
    r = run(T, case)
    Se, Ie, cnte = oracle(*case[1:])
    ok = np.nonzero(r.flags & 1)[0]
    S, I, cnt = r.raw
    assert len(ok) > 0
    assert_topk_equal(S[ok], I[ok], cnt[ok], [Se[i] for i in ok], [Ie[i] for i in ok], [cnte[i] for i in ok],
                      f"raw {case_id(case)} (positions {ok.tolist()})")


@every_case
def test_b_who_may_lack_the_certificate(T, case):
    """The conditions that keep (a) from being vacuous."""
    r = run(T, case)
    mode = case[0]
    cert = (r.flags & 1) != 0
    what = case_id(case)
    if mode in F16_MODES:
        for p in np.nonzero(np.isin(r.classes, ("zero_image", "inf_image")))[0]:
            assert not cert[p], f"{what}: {r.names[p]} ({r.classes[p]}, position {p}) is certified by an f16 scan"
    for p in np.nonzero(r.edge & (r.classes == "plain"))[0]:
        assert cert[p] == cert[r.bases[p]], \
            f"{what}: {r.names[p]} (position {p}) certified {cert[p]}, its base query {cert[r.bases[p]]}"
    bad = set(np.nonzero(~cert & ~r.edge)[0].tolist())
    assert bad <= {ZERO_QUERY, TIE_QUERY}, f"{what}: uncertified ordinary queries {sorted(bad)}"
    over = (r.flags & T._native.THR_FLAG_OVERFLOW) != 0
    assert not np.any(over & ~r.edge), f"{what}: ordinary queries overflowed {np.nonzero(over & ~r.edge)[0].tolist()}"


@every_case
def test_c_an_edge_query_costs_its_tile_mates_nothing(T, case):
    """The same batch with every edge query replaced by an all-zero query: the ordinary queries' flags
    are identical."""
    r = run(T, case)
    diff = np.nonzero((r.flags != r.flags_zeroed) & ~r.edge)[0]
    assert len(diff) == 0, f"{case_id(case)}: ordinary queries {diff.tolist()} have flags " \
                           f"{r.flags[diff].tolist()} beside the edge queries, {r.flags_zeroed[diff].tolist()} without"


@every_case
def test_d_the_search_is_the_oracle(T, case):
    r = run(T, case)
    S, I, cnt, nres = r.search
    assert_topk_equal(S, I, cnt, *oracle(*case[1:]), f"search {case_id(case)}")
    assert nres <= int(np.sum((r.flags & 1) == 0))


@f16_cases
def test_e_qerr_is_eq_rounded_up(T, case):
    """qerr[q] >= eq (the certificate may never under-estimate it) and qerr[q] <= eq (1 + 2^-20) + 2^-149:
    eq is formed in float64, rounded to float32 once and stepped up one ulp (pack_queries_f16 at
    d <= 768 and at 1024, the prologue of kth_select for the scans of float32 rows).  An image with an
    infinity: not finite.  A query without a non-zero component, and the padding of the last tile:
    0 stepped up once, 2^-149."""
    r = run(T, case)
    nq = len(r.q)
    for p in range(nq):
        e, got, what = eq_f64(r.q[p]), r.qerr[p], f"{case_id(case)}: {r.names[p]} at position {p}"
        if r.classes[p] == "inf_image":
            assert not np.isfinite(got), f"{what}: qerr {got}"
        elif not r.q[p].any():
            assert got == 2.0 ** -149, f"{what}: qerr {got}"
        else:
            assert got >= e, f"{what}: qerr {got!r} < eq {e!r}"
            assert got <= e * (1 + 2.0 ** -20) + 2.0 ** -149, f"{what}: qerr {got!r} far above eq {e!r}"
    assert np.all(r.qerr[nq:] == 2.0 ** -149), "the padding queries of the last tile"


@sampled_cases
def test_f_an_edge_query_alone_in_its_batch(T, case):
    """nq = 1: a query tile with nothing else in it, one representative of each class."""
    mode, n, d = case
    idx = index(T, mode, n, d)
    q, names, classes, _ = catalogue(n, d)
    Se, Ie, cnte = oracle(n, d)
    reps = representatives(names, classes)
    assert set(reps) == set(CLASSES)
    for cls, p in reps.items():
        S, I, cnt, _ = idx.dense_search(dev(q[p:p + 1]), K, kprime=KP)
        assert_topk_equal(S, I, cnt, Se[p:p + 1], Ie[p:p + 1], cnte[p:p + 1], f"{case_id(case)} alone: {names[p]} ({cls})")


# ---- further consumers of the same queries ----
@functools.lru_cache(maxsize=None)
def filtered_oracle(n, d, n_labels=3):
    """Row r carries label r % 3, query p asks for label p % 4 - 1 (-1: unfiltered): the oracle of a
    filtered query is the oracle over its label's rows."""
    x, _ = planted(n, d)
    q = catalogue(n, d)[0]
    Se, Ie, cnte = (a.copy() for a in oracle(n, d))
    labels = (np.arange(n) % n_labels).astype(np.int32)
    want = (np.arange(len(q)) % (n_labels + 1) - 1).astype(np.int32)
    for c in range(n_labels):
        rows = np.nonzero(labels == c)[0]
        sel = np.nonzero(want == c)[0]
        s, i, cn = CO.dense_topk_exact(x[rows], q[sel], K)
        Se[sel], cnte[sel] = s, cn
        Ie[sel] = np.where(i >= 0, rows[np.maximum(i, 0)] + DOC_BASE, -1)
    return labels, want, (Se, Ie, cnte)


@pytest.mark.parametrize("mode", ["f16", "f32"], ids=["copy", "f32"])
def test_collection_filter_on_the_edge_queries(T, mode):
    n, d = 20011, 768
    labels, want, expected = filtered_oracle(n, d)
    idx = T.GpuIndex(doc_base=DOC_BASE).set_dense(planted(n, d)[0], shortlist=mode).set_collections(labels)
    S, I, cnt, _ = idx.dense_search(dev(catalogue(n, d)[0]), K, kprime=KP, collections=dev(want))
    assert_topk_equal(S, I, cnt, *expected, f"collections {mode}")


def test_scoped_row_lists_on_the_edge_queries(T):
    """Scopes narrow enough for the row-list route (thr_dense_topk_rows): every query scoped, none left
    to the scan."""
    n, d = 3001, 512
    labels, want, _ = filtered_oracle(n, d)
    x, _ = planted(n, d)
    q = catalogue(n, d)[0]
    idx = T.GpuIndex(doc_base=DOC_BASE).set_dense(x, shortlist="f16").set_attributes({"org": labels})
    org = np.arange(len(q)) % 3
    S, I, cnt, _ = idx.dense_search(dev(q), K, scopes=[{"org": int(o)} for o in org], scope_rows_max=n)
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    for c in range(3):
        rows = np.nonzero(labels == c)[0]
        sel = np.nonzero(org == c)[0]
        s, i, cn = CO.dense_topk_exact(x[rows], q[sel], K)
        assert np.array_equal(cnt[sel], cn) and np.all(cn == K)
        assert np.array_equal(I[sel], rows[i] + DOC_BASE) and np.array_equal(S[sel], s), f"scope org={c}"


@pytest.mark.parametrize("mode", ["f16", "f16-anydim"], ids=["copy", "f16-anydim"])
def test_shard_floor_on_the_edge_queries(T, mode):
    """4 shards in one process.  An image with an infinity gives the exchange no bound at all (its scan
    emits nothing: every slot -inf), so its floor is -inf, and no shard certifies it before the rescue."""
    n, d = 20011, 768
    x, _ = planted(n, d)
    q, names, classes, _ = catalogue(n, d)
    seen = {}
    (S, I, cnt), flags, _ = floor_search(T, x, q, K, 4, mode, seen=seen)
    Se, Ie, cnte = oracle(n, d)
    assert_topk_equal(S, I, cnt, Se, Ie - DOC_BASE, cnte, f"shard floor {mode}")
    inf = np.nonzero(np.array(classes) == "inf_image")[0]
    assert len(inf) >= 8
    assert np.all(seen["gfloor"].cpu().numpy()[inf] == -np.inf)
    assert np.all(seen["lbs"].cpu().numpy()[:, inf, :] == -np.inf)
    assert not np.any(flags[:, inf] & 1), "a shard certified a query whose image holds an infinity"
    zero = np.nonzero(np.array(classes) == "zero_image")[0]
    assert not np.any(flags[:, zero] & 1)
    ordinary = np.nonzero(~is_edge(names))[0]
    assert not np.any(flags[:, ordinary] & T._native.THR_FLAG_OVERFLOW)


ALTERNATE = {"THR_DENSE_MFMA=32": "x512 or x768", "THR_DENSE_F16=q": "x768", "THR_DENSE_QW=32": "x1024"}


@pytest.mark.parametrize("knob", sorted(ALTERNATE))
def test_alternate_scan_builds_in_a_subprocess(knob):
    """The copy scan's cases again under the A/B knobs -- the 32x32x16 MFMA shape (the other
    pack_queries_f16 instantiations) at dims 512 and 768, the 4-wave kernel at 768, 32 queries per wave
    at 1024.  The knobs are read once per process: a fresh child."""
    name, value = knob.split("=")
    if os.environ.get(name) == value:
        pytest.skip("already inside that run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          f"copy and ({ALTERNATE[knob]}) and not subprocess"],
                         env=dict(os.environ, **{name: value}), cwd=root, capture_output=True, text=True,
                         timeout=600)
    passed = re.search(r"(\d+) passed", out.stdout)
    assert out.returncode == 0 and passed and int(passed.group(1)) >= 5 and "failed" not in out.stdout, \
        out.stdout[-2000:] + out.stderr[-1000:]


# ---- queries that are not finite ----
NONFINITE = [("f16", 3001, 512), ("f16-inline", 3001, 512), ("f16-anydim", 3001, 512), ("f32", 3001, 768),
             ("exact", 3001, 512)]


@pytest.mark.parametrize("case", NONFINITE, ids=case_id)
def test_nonfinite_queries_stay_in_bounds(T, case):
    """A NaN component, a +inf component.  The oracle has no answer for such a query, so its own row is
    held only to the shape of a result: the call returns, count <= k, ids -1 or real rows; and the
    ordinary queries beside it are the oracle's, none overflowed.

    Why the batch is safe to run -- the kernels between the query and the result, read for where a SCORE
    could become an index, a loop bound or an address:
      * kth_select / kth_select_top look at the query first (query_kind): a float16 image (f16 scans) or a
        float32 value (fp32 scan) that is not finite gives tau = NaN and the kernel returns before it
        reads a sample score.  For every other query the sample scores are finite or NaN (|score| <= ||q||
        ||d||, in range by query_kind's bounds); they index histograms only as key digits masked to the
        histogram's size, or as (v - lo) * scale of a finite v in [lo, hi], clamped to the last bin.
      * the scans' emit compares `score >= tau`: false for a NaN tau, so such a query emits nothing, and
        a NaN score never passes any tau.  Slots come from counters compared with the capacity.
      * bucket_candidates, select_band: indices are list positions, counters checked against CAND_CAP /
        SEL_BIG_BAND / kprime, and the histogram bin of a candidate score -- candidates are scores that
        passed a non-NaN tau, finite by the above, so the bin lies in [0, 4095].  With no candidates
        (ns = 0) no row is read.
      * rescore_rank reads rows sel_rows[0, ns) only, ranks by counting (rank < ns), and a NaN bound or
        norm makes every certificate comparison false: the query is left uncertified.
      * thr_dense_rescue / thr_dense_topk_exact / thr_dense_topk_rows score every row in float64 and push
        `sim > -inf` (false for NaN) into BlockTopK, whose slots come from a counter kept below its
        capacity and whose select uses masked key digits.
    So no index, loop bound or address is derived from a score value other than through a mask or a
    clamp, and a non-finite query reaches the exhaustive path with an empty shortlist."""
    mode, n, d = case
    x, q0 = planted(n, d)
    q = q0.copy()
    nan_at, inf_at = 1, 3
    q[nan_at, d // 2] = np.nan
    q[inf_at, 7] = np.inf
    idx = index(T, mode, n, d)
    Se, Ie, cnte = CO.dense_topk_exact(x, q0, K, doc_id_base=DOC_BASE)
    fine = np.array([p for p in range(len(q)) if p not in (nan_at, inf_at)])
    flags = raw_call(T, idx, mode, dev(q))[3].cpu().numpy()
    assert not np.any(flags[fine] & T._native.THR_FLAG_OVERFLOW)
    assert set(np.nonzero((flags[fine] & 1) == 0)[0].tolist()) <= {int(np.nonzero(fine == p)[0][0]) for p in (ZERO_QUERY, TIE_QUERY)}
    if mode != "exact":
        assert not flags[nan_at] & 1 and not flags[inf_at] & 1, "a scan certified a query that is not finite"
    S, I, cnt, _ = idx.dense_search(dev(q), K, kprime=KP)
    torch.cuda.synchronize()
    assert_topk_equal(S[fine], I[fine], cnt[fine], Se[fine], Ie[fine], cnte[fine], f"beside non-finite queries, {case_id(case)}")
    cnt, I = cnt.cpu().numpy(), I.cpu().numpy()
    for p in (nan_at, inf_at):
        assert 0 <= cnt[p] <= K
        assert np.all((I[p] == -1) | ((I[p] >= DOC_BASE) & (I[p] < DOC_BASE + n)))
        assert np.all(I[p, cnt[p]:] == -1)
