"""BM25 at the ends of its value range: the cases of tests/bm25_cases.py (what each one stands for is
proved on the CPU by tests/test_bm25_cases_host.py) through thr_bm25_bounds, thr_bm25_dense_rows and
every path of thr_bm25_topk.

Every result is held to oracle.thr_oracle.bm25_topk bit for bit -- ids, scores as uint64, counts,
padding -- on the default path (the wave walk at k <= 64), at k = 65 and 128 (the workgroup walk),
without bounds, without the dense rows, with term and block bounds but no impacts, with a doc id
base, and in the AND form where the case has one.  The control words at the start of the lexical
workspace say which branch a call took and are asserted: a case that stops reaching its branch after
a retune fails.  The bounds and the rows are also checked alone, against float64 numpy.

The oracle runs once per corpus, (k1, b) and mode (bm25_cases.expected); each index is built once
per module."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bm25_cases as BC  # noqa: E402

CTL_ITEMS, CTL_DENSE_Q, CTL_SWEEPS, CTL_TARGET_A = 0, 3, 5, 7      # bm25_common.hpp: BmCtl
BLOCK_WALK = os.environ.get("THR_BM25_WALK", "")[:1] == "b"        # (inside the knob run of this file)
ID_BASE = 1_000_003


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()       # (a copy: the cases' arrays are read-only)
    return t if dtype is None else t.to(dtype)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


_INDEX, _EXPECTED = {}, {}


def index(T, cname, k1, b):
    """One GpuIndex per corpus and (k1, b), kept for the module."""
    key = (cname, k1, b)
    if key not in _INDEX:
        c = BC.corpus(cname)
        idx = T.GpuIndex().set_lexical(c.rowptr, c.post_doc, c.post_tf, c.doclen, c.idf, c.avgdl, k1=k1, b=b,
                                       dense_share=c.share)
        if c.coll is not None:
            idx.set_collections(c.coll)
        slot = idx.lex["dense"][0].cpu().numpy()
        assert np.array_equal(slot >= 0, c.has_row), "the terms with rows are the ones the builder says"
        _INDEX[key] = idx
    return _INDEX[key]


def expected_dev(case, conjunctive):
    key = (case.cname, case.params, conjunctive)
    if key not in _EXPECTED:
        S, I, cnt = case.expected(conjunctive)
        _EXPECTED[key] = (dev(S), dev(I), dev(cnt))
    return _EXPECTED[key]


def check(case, rows, k, S, I, cnt, conjunctive, base, what):
    c = case.corpus
    ES, EI, Ecnt = expected_dev(case, conjunctive)
    r = dev(rows).long()
    assert S.shape == (len(rows), k) and I.shape == (len(rows), k) and cnt.shape == (len(rows),), what
    assert S.dtype == torch.float64 and I.dtype == torch.int64
    ecnt = Ecnt[r].clamp(max=k)
    live = torch.arange(k, device=r.device)[None, :] < ecnt[:, None]
    ei = torch.where(live, EI[r][:, :k] + base, torch.full_like(I, -1))
    es = torch.where(live, ES[r][:, :k], torch.full_like(S, float("-inf")))     # padding: -inf, id -1
    bad = (cnt != ecnt) | (I != ei).any(dim=1) | (S.view(torch.int64) != es.view(torch.int64)).any(dim=1)
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        p, n = int(rows[i]), int(ecnt[i])
        raise AssertionError(
            f"{what}: query {c.qname[p]!r} ({int(bad.sum())} of {len(rows)} rows differ): count {int(cnt[i])} != {n} or ids "
            f"{I[i, :n + 1].tolist()} != {ei[i, :n + 1].tolist()} or scores {S[i, :n + 1].tolist()} != {es[i, :n + 1].tolist()}")


def native_call(T, idx, qt, k, qc, conjunctive, bounds, dense, id_base):
    """thr_bm25_topk with the index's arrays and the given bounds / rows / doc id base."""
    L = idx.lex
    return T._native.bm25_topk(L["rowptr"], L["post_doc"], L["post_tf"], L["doclen"], L["idf"], L["avgdl"], qt, k, id_base,
                               L["k1"], L["b"], bounds=bounds, conjunctive=conjunctive,
                               doc_coll=idx.doc_coll if qc is not None else None, query_coll=qc, dense=dense)


def paths_of(case):
    out = [("plain", k) for k in case.ks]
    sliced = case.cname == "sliced"
    out += [("noprune", k) for k in ((10, 65) if sliced else (10,))]
    out += [("norows", k) for k in (case.ks if sliced else (10, 65))]
    out += [("termblock", 10), ("termblock", 65), ("base", 10), ("base", 65)]
    return out


PARAMS = [(name, path, k) for name, case in BC.CASES.items() for path, k in paths_of(case)]


@pytest.mark.parametrize("name,path,k", PARAMS, ids=[f"{n}-{p}-{k}" for n, p, k in PARAMS])
def test_case(T, name, path, k):
    case = BC.CASES[name]
    c = case.corpus
    idx = index(T, case.cname, *case.params)
    rows = case.rows
    nq = len(rows)
    qt = dev(c.queries[rows])
    qc = dev(c.qcoll[rows]) if c.coll is not None else None
    conj = case.conj
    what = f"{name} {path} k={k} k1={case.params[0]} b={case.params[1]} and={conj}"
    L = idx.lex
    if path == "termblock":      # term and block bounds, no impacts: the workgroup walk, no accumulators, no rows
        S, I, cnt = native_call(T, idx, qt, k, qc, conj, L["bounds"][:2], None, 0)
        return check(case, rows, k, S, I, cnt, conj, 0, what)
    if path == "base":
        S, I, cnt = native_call(T, idx, qt, k, qc, conj, L["bounds"], L["dense"], ID_BASE)
        return check(case, rows, k, S, I, cnt, conj, ID_BASE, what)
    S, I, cnt = idx.bm25_search(qt, k, collections=qc, conjunctive=conj, prune=path != "noprune",
                                dense_rows=path != "norows")
    torch.cuda.synchronize()
    ctl = idx._ws_lex[:64].view(torch.int32).cpu().numpy().copy()   # (bm_layout: the control words are at offset 0)
    check(case, rows, k, S, I, cnt, conj, 0, what)
    # ---- the branch the call took
    probing = path == "plain" and not conj
    n_probed = sum(c.probing(p) for p in rows) if probing else 0
    assert ctl[CTL_DENSE_Q] == n_probed, f"{what}: {ctl[CTL_DENSE_Q]} queries with probed terms, not {n_probed}"
    if not probing:
        assert ctl[CTL_SWEEPS] == 0, f"{what}: sweeps without rows"
    elif name in ("stage_b_wins", "stage_b_tie"):
        # (3000 docs are one sweep slice: a sweep item per query that sweeps)
        assert ctl[CTL_SWEEPS] == nq, f"{what}: {ctl[CTL_SWEEPS]} sweep items, every one of the {nq} queries needs its sweep"
    elif name == "stage_b_skipped" and k <= 100:      # (at k = 128 stage A's 100 docs give no threshold)
        assert ctl[CTL_SWEEPS] == 0, f"{what}: {ctl[CTL_SWEEPS]} sweep items, the probed bound rules every sweep out"
    elif name == "idf_spread":
        assert ctl[CTL_SWEEPS] >= 1, f"{what}: the all-zero query sweeps (bound 0.0 == threshold 0.0)"
    if case.cname == "sliced":
        assert ctl[CTL_ITEMS] > nq, f"{what}: {ctl[CTL_ITEMS]} items for {nq} queries: nothing was sliced"
        if path == "norows" and k <= 64 and not BLOCK_WALK:
            assert BC.WW_TARGET_MIN <= ctl[CTL_TARGET_A] <= BC.WW_TARGET_MAX, f"{what}: wave slices of {ctl[CTL_TARGET_A]}"
            assert ctl[CTL_ITEMS] >= nq * (c.n // BC.WW_TARGET_MAX), f"{what}: {ctl[CTL_ITEMS]} items"
    else:
        assert nq <= ctl[CTL_ITEMS] <= 4 * nq, f"{what}: {ctl[CTL_ITEMS]} items for {nq} one-slice queries"


# --------------------------------------------------------------------------------- thr_bm25_bounds alone
@pytest.mark.parametrize("cname,k1,b", [("values", *p) for p in BC.K1B] + [("stageb", *BC.DEFAULT)])
def test_bounds_against_float64(T, cname, k1, b):
    """term_ub / block_ub: the maximum of the oracle's contribution over the term's postings / over
    postings [128 j, 128 j + 128) -- blocks that straddle two lists and the short last block included
    --, bit for bit; 0.0 for a term without postings.  post_imp: ceil(x) + 1 clipped to 255, x =
    impact * 255 / (k1 + 1); an unclipped one times the unit lies in [impact, impact + 2 units]
    (ceil(x) + 1 - x < 2); a clipped one has x > 254 and bounds the impact within the 1e-12 slack
    of the kernels' thresholds (255 * fl((k1 + 1) / 255) may be an ulp below k1 + 1)."""
    c = BC.corpus(cname)
    N = T._native
    tub, bub, imp = N.bm25_bounds(dev(c.rowptr), dev(c.post_doc), dev(c.post_tf), dev(c.doclen), dev(c.idf), c.avgdl, k1, b)
    torch.cuda.synchronize()
    nnz = len(c.post_doc)
    etub, ebub = BC.bounds(c, k1, b)
    tub, bub, imp = tub.cpu().numpy(), bub.cpu().numpy(), imp.cpu().numpy()
    assert nnz % 128 != 0 and len(bub) == len(ebub) == (nnz + 127) // 128
    straddle = np.setdiff1d(c.rowptr[1:-1] // 128, c.rowptr[1:-1][c.rowptr[1:-1] % 128 == 0] // 128)
    assert len(straddle) >= 3, "blocks that straddle two lists"
    assert np.array_equal(bits(tub), bits(etub)), f"term_ub differs at terms {np.flatnonzero(bits(tub) != bits(etub))[:5]}"
    assert np.array_equal(bits(bub), bits(ebub)), f"block_ub differs at blocks {np.flatnonzero(bits(bub) != bits(ebub))[:5]}"
    if cname == "values":
        assert c.df[c.term["EMPTY"]] == 0 and bits(tub[c.term["EMPTY"]]) == 0
    true, _, x = BC.impacts(c, k1, b)
    unit = (k1 + 1.0) / 255.0
    q = imp[:nnz].astype(np.float64)
    assert np.all(imp[nnz:] == 0)
    clip = BC.clipped(x)
    assert np.array_equal(imp[:nnz], BC.quantised(x)), \
        f"post_imp is not ceil(x) + 1 clipped at postings {np.flatnonzero(imp[:nnz] != BC.quantised(x))[:5]}"
    un = ~clip
    assert np.all(q[un] * unit >= true[un]) and np.all(q[un] * unit <= true[un] + 2.0 * unit)
    assert np.all(imp[:nnz][clip] == 255) and np.all(255.0 * unit * (1.0 + 1e-12) >= true[clip])
    if k1 == 0.0:
        assert clip.all()
    elif cname == "values":
        assert clip.sum() > 500 and un.sum() > 500


# ----------------------------------------------------------------------------- thr_bm25_dense_rows alone
def test_dense_rows_against_the_postings(T):
    """Every row equals its postings scattered -- the term frequencies as uint16, 32768 .. 65535
    included --, zeros elsewhere and in the padding up to thr_bm25_dense_stride; the twin term with
    one posting of 65536 gets no row."""
    c = BC.corpus("values")
    N = T._native
    rp, pd, ptf = dev(c.rowptr), dev(c.post_doc), dev(c.post_tf)
    _, _, imp = N.bm25_bounds(rp, pd, ptf, dev(c.doclen), dev(c.idf), c.avgdl, *BC.DEFAULT)
    slot, dimp, dtf, stride = N.bm25_dense_terms(rp, pd, ptf, imp, c.n, c.share)
    torch.cuda.synchronize()
    assert stride == int(N.load().thr_bm25_dense_stride(c.n)) == ((c.n + 15) & ~15) + 65536
    slot = slot.cpu().numpy()
    assert np.array_equal(slot >= 0, c.has_row) and slot[c.term["L2"]] == -1 and slot[c.term["L3"]] == -1
    assert slot[c.term["L"]] >= 0 and sorted(slot[slot >= 0]) == list(range(c.has_row.sum()))
    assert dimp.shape == dtf.shape == (c.has_row.sum(), stride)
    dimp, dtf, imp = dimp.cpu().numpy(), dtf.cpu().numpy().view(np.uint16), imp.cpu().numpy()
    for t in np.flatnonzero(c.has_row):
        lo, hi = c.rowptr[t], c.rowptr[t + 1]
        etf, eimp = np.zeros(stride, dtype=np.uint16), np.zeros(stride, dtype=np.uint8)
        etf[c.post_doc[lo:hi]] = c.post_tf[lo:hi].astype(np.uint16)
        eimp[c.post_doc[lo:hi]] = imp[lo:hi]
        assert np.array_equal(dtf[slot[t]], etf) and np.array_equal(dimp[slot[t]], eimp), f"row of term {t}"
    row = dtf[slot[c.term["L"]]]
    assert tuple(row[BC.LADDER0:BC.LADDER0 + len(BC.LADDER_TF)]) == BC.LADDER_TF


# ------------------------------------------------------------------------------------ the alternate walks
@pytest.mark.parametrize("knobs", ["THR_BM25_WALK=block", "THR_BM25_SHAPE=small THR_BM25_FUSE_DIV=1000000"])
def test_cases_under_the_alternate_walks_in_a_subprocess(knobs):
    """THR_BM25_WALK=block (stage A on the workgroup walk: its accumulators and probes at every value
    edge) and the small block shape with stage A always fused into the ordinary items' launch are
    read once per process: every case runs again under each."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    if env.get("THR_BM25_KNOB_RUN"):
        pytest.skip("already inside a knob run")
    env["THR_BM25_KNOB_RUN"] = "1"
    for kv in knobs.split():
        name, value = kv.split("=")
        env[name] = value
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "test_case and not subprocess"],
                         env=env, cwd=root, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0 and f"{len(PARAMS)} passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-3000:] + out.stderr[-1000:]
