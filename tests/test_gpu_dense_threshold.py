"""The threshold pass of the register-resident dense scans (dense_scan_f16qs / dense_scan_f16q): the
sample pass keeps each lane's SAMPLE_TOP best scores per query and segment, kth_select_top takes the
ks-th largest of them.  tau may therefore sit BELOW the ks-th best sample score, never above it, and
the search stays exact and certified: every case compares with the CPU oracle bit for bit.

The shapes are the smallest that still sample (n_docs > CAND_CAP / 2 = 8192).  One index and one
oracle run per (n, dim), shared by the cases of that shape: the queries of a smaller batch are a
prefix of the 257, the top 10 a prefix of the top 100.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle import c_oracle as CO  # noqa: E402
from oracle import thr_oracle as O  # noqa: E402

NQ_MAX, K_MAX = 257, 100
# make_plan (dense.hip): ks of the register-resident scans and their aim at 1M rows -- or what the A/B
# knobs THR_DENSE_KS / THR_DENSE_AIM set them to, read the way dense_knobs() reads them
KS = int(os.environ.get("THR_DENSE_KS") or 32)
KS = KS if 4 <= KS <= 64 else 32
AIM_1M = float(os.environ.get("THR_DENSE_AIM") or 1448.0)
AIM_1M = AIM_1M if AIM_1M >= 64.0 else 1448.0
F32_U = 2.0 ** -24


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def plan(n, kprime):
    """make_plan's sample of a packed batch (dense.hip): -> (aim, stride in 32-row groups, groups sampled).
    Sample group i is row group i * stride: rows 32 * i * stride .. + 32."""
    groups = (n + 31) // 32
    ks = min(kprime, KS)
    aim = AIM_1M * math.sqrt(n / 1.0e6)
    aim = min(max(aim, min(8.0 * kprime, 4096.0)), 4096.0)
    target = max(min(int(n * ks / aim), 1 << 20), 4 * ks)
    sg = min((target + 31) // 32, groups)
    return aim, groups // sg, sg


def sample_rows(n, kprime):
    _, stride, sg = plan(n, kprime)
    rows = (np.arange(sg)[:, None] * stride * 32 + np.arange(32)[None, :]).ravel()
    return rows[rows < n]


def scan_scores(x, q, rows):
    """What the f16 scan computes for `rows`: fp16(d / ||d||) . fp16(q), here in float64 (NaN for a
    row without an embedding).  The scan accumulates in float32: within scan_slack of this."""
    xr = x[rows].astype(np.float64)
    nn = np.linalg.norm(xr, axis=1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        d16 = (xr / nn).astype(np.float16).astype(np.float64)
    return d16 @ q.astype(np.float16).astype(np.float64)


def scan_slack(q):
    """fp32 accumulation bound of the scan (scan_eps, dense_common.hpp): (dim + 16) 2^-24 ||q|| ||d||, ||d|| = 1.

    Every tau bound below is "tau <= the ks-th largest f16-rounded sample score + scan_slack".  The
    slack LOOSENS the plain "tau <= the ks-th largest f16-rounded score": the kernel adds the same
    f16 products in float32, this file adds them in float64, and the two sums of one row differ by
    up to this much (about 5e-5 ||q|| at dim 768, where a score's spread over rows is about
    ||q|| / sqrt(dim) = 3.6e-2 ||q||).  It comes from the number format alone, not from what the
    kernel returns."""
    return (len(q) + 16) * F32_U * float(np.linalg.norm(q.astype(np.float64))) * (1 + 2.0 ** -10)


def kth_largest(v, kk):
    v = v[np.isfinite(v)]
    return -np.inf if len(v) < kk else np.sort(v)[len(v) - kk]


class Case:
    """An index, a batch, and the search through the scan's entry point with a workspace of the
    test's own, so that tau (the workspace's first qpad floats) can be read back."""

    def __init__(self, T, x, q):
        self.T, self.x, self.q = T, x, q
        self.idx = T.GpuIndex().set_dense(x, shortlist="f16")

    def search(self, nq, k, coll=None):
        T, idx, N = self.T, self.idx, self.T._native
        n, d = self.x.shape
        kp = idx._kprime(k, None)
        ws = torch.empty(N.dense_f16_workspace_bytes(n, d, nq, kp), dtype=torch.uint8, device="cuda")
        S, I, cnt, flg = N.dense_topk_f16(idx.docs, idx.docs16, idx.doc_rel_err, idx.dnorm, idx.inv_norm,
                                          dev(self.q[:nq]), k, kp, 0, ws,
                                          doc_coll=None if coll is None else idx.doc_coll,
                                          query_coll=None if coll is None else dev(coll))
        torch.cuda.synchronize()
        qt = N.dense_f16_query_tile(d, True, nq)
        qpad = (nq + qt - 1) // qt * qt
        tau = ws[:4 * qpad].view(torch.float32).cpu().numpy()
        return S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy(), flg.cpu().numpy(), tau, kp


def assert_exact_and_certified(S, I, cnt, flg, Se, Ie, cnte, k, what):
    assert np.all(flg & 1), f"{what}: uncertified queries (they would be rescued): {np.nonzero(~(flg & 1).astype(bool))[0]}"
    for i in range(len(cnt)):
        m = min(int(cnte[i]), k)
        assert int(cnt[i]) == m, f"{what} q{i}: count {cnt[i]} != {m}"
        assert np.array_equal(I[i, :m], Ie[i][:m]), f"{what} q{i}: ids differ"
        assert np.array_equal(S[i, :m], Se[i][:m]), f"{what} q{i}: scores differ (bits)"
        assert np.all(I[i, m:] == -1)


_shape_cache = {}


def shape_case(T, n, d):
    if (n, d) not in _shape_cache:
        rng = np.random.default_rng(1000 * n + d)
        x = rng.standard_normal((n, d)).astype(np.float32)
        x[5] = 0                                   # a row without an embedding
        q = rng.standard_normal((NQ_MAX, d)).astype(np.float32)
        q[::2] = x[rng.integers(6, n, (NQ_MAX + 1) // 2)] + 0.5 * q[::2]
        c = Case(T, x, q)
        c.oracle = CO.dense_topk_exact(x, q, K_MAX)
        _shape_cache[(n, d)] = c
    return _shape_cache[(n, d)]


@pytest.mark.parametrize("k", [10, 100])
@pytest.mark.parametrize("nq", [1, 33, 257])
@pytest.mark.parametrize("d", [512, 768, 1024])
@pytest.mark.parametrize("n", [12001, 40000])
def test_threshold_shapes(T, n, d, nq, k):
    """n = 12001: a last tile with NaN padding rows; dim 1024: dense_scan_f16q; 1 / 33 / 257 queries:
    padding waves, a partly filled wave, two query tiles."""
    c = shape_case(T, n, d)
    S, I, cnt, flg, tau, kp = c.search(nq, k)
    Se, Ie, cnte = c.oracle
    assert_exact_and_certified(S, I, cnt, flg, Se[:nq], Ie[:nq], cnte[:nq], k, f"n{n} d{d} nq{nq} k{k}")
    # tau is at most the ks-th best score of the sample, and padding queries never emit
    rows = sample_rows(n, kp)
    for i in range(min(nq, 8)):
        bound = kth_largest(scan_scores(c.x, c.q[i], rows), min(kp, KS)) + scan_slack(c.q[i])
        assert tau[i] <= bound, (i, tau[i], bound)
    assert np.all(tau[nq:] == np.inf)


@pytest.mark.parametrize("knob", ["THR_DENSE_MFMA=32", "THR_DENSE_F16=q"])
def test_threshold_shapes_under_the_scan_knobs(knob):
    """The dim-768 shapes again with the 32x32x16 MFMA shape (two segments per row slice, 16 rows per
    lane and tile) and with the 4-wave kernel: the knobs are read once per process."""
    name, value = knob.split("=")
    if os.environ.get(name) == value:
        pytest.skip("already inside that run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          "test_threshold_shapes and 768 and not knobs"],
                         env=dict(os.environ, **{name: value}), cwd=root, capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0 and "12 passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-2000:] + out.stderr[-1000:]


@pytest.mark.parametrize("n,d,k", [(12001, 768, 10), (40000, 768, 100), (40000, 1024, 10)])
def test_threshold_concentrated_top(T, n, d, k):
    """64 copies of the query's best row in consecutive rows from the start of a sample group: the 32
    of them that are sampled sit in ONE tile, where a lane holds 8 (16 with the 32x32x16 shape) of one
    query's rows and keeps SAMPLE_TOP -- far fewer than the ks = 32 copies that head the sample.  tau
    drops below the ks-th best sample score (the copies' score), never above, and the search stays
    exact and certified."""
    rng = np.random.default_rng(n + d + k)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    kp = k + 92
    _, stride, sg = plan(n, kp)
    assert stride > 1 and sg > 3
    g = 3 * stride                                    # sample group 3
    x[32 * g:32 * g + 64] = x[32 * g]
    q[0] = x[32 * g] + 0.3 * q[0]
    c = Case(T, x, q)
    S, I, cnt, flg, tau, kp2 = c.search(3, k)
    assert kp2 == kp
    assert_exact_and_certified(S, I, cnt, flg, *CO.dense_topk_exact(x, q, k), k, "concentrated")
    assert set(range(32 * g, 32 * g + min(k, 64))) <= set(I[0].tolist())
    sc = scan_scores(x, q[0], sample_rows(n, kp))
    kth = kth_largest(sc, KS)
    assert abs(kth - scan_scores(x, q[0], np.array([32 * g]))[0]) < 1e-12      # the copies head the sample
    print(f"concentrated n{n} d{d}: tau {tau[0]:.6f}  ks-th sample score {kth:.6f}")
    assert tau[0] <= kth + scan_slack(q[0])
    # ... and the case is what it claims to be: one lane held more than SAMPLE_TOP of the top ks, so
    # tau fell clearly below the score the full-score pass would have taken
    assert tau[0] < kth - scan_slack(q[0])
    for i in (1, 2):
        assert tau[i] <= kth_largest(scan_scores(x, q[i], sample_rows(n, kp)), KS) + scan_slack(q[i])


def test_threshold_thin_sample_and_void_queries(T):
    """Fewer than ks finite sample scores (all but a handful of rows have no embedding): tau = -inf
    and the result is still exact.  A zero query and the padding queries get tau = +inf."""
    n, d, k = 12001, 768, 10
    rng = np.random.default_rng(77)
    x = np.zeros((n, d), dtype=np.float32)
    live = np.concatenate([np.arange(0, 640, 32), rng.integers(640, n, 9)])   # some of them sample rows
    x[live] = rng.standard_normal((len(live), d)).astype(np.float32)
    q = rng.standard_normal((3, d)).astype(np.float32)
    q[1] = 0
    c = Case(T, x, q)
    S, I, cnt, flg, tau, kp = c.search(3, k)
    assert np.isfinite(scan_scores(x, q[0], sample_rows(n, kp))).sum() < KS
    assert tau[0] == -np.inf and tau[2] == -np.inf
    assert tau[1] == np.inf and np.all(tau[3:] == np.inf)
    Se, Ie, cnte = CO.dense_topk_exact(x, q, k)
    live_q = np.array([0, 2])
    assert_exact_and_certified(S[live_q], I[live_q], cnt[live_q], flg[live_q], Se[live_q], Ie[live_q],
                               cnte[live_q], k, "thin sample")


def test_threshold_collection_filter(T):
    """Collections of 2 % and of 25 % of the rows: the sample pass counts only the query's own
    collection, so about as many rows of it pass as unfiltered rows would -- nothing is rescued."""
    n, d, k = 40000, 768, 20
    rng = np.random.default_rng(23)
    x = rng.standard_normal((n, d)).astype(np.float32)
    x[77] = 0
    coll = (np.arange(n) * 7919 % 50).astype(np.int32)                       # 2 % each
    coll[n // 2:] = np.where(np.arange(n - n // 2) % 2 == 0, 60, coll[n // 2:])   # 60: 25 %
    q = rng.standard_normal((9, d)).astype(np.float32)
    q[:4] = x[[5, 6000, 31000, 39999]] + 0.5 * q[:4]
    qc = np.array([7, 60, -1, 7, 60, 12345, -1, 3, 60], dtype=np.int32)
    c = Case(T, x, q)
    c.idx.set_collections(coll)
    S, I, cnt, nres = c.idx.dense_search(dev(q), k, collections=dev(qc))
    assert nres == 0
    S, I, cnt = S.cpu().numpy(), I.cpu().numpy(), cnt.cpu().numpy()
    _, _, _, flg, tau, _ = c.search(9, k, coll=qc)
    assert all(flg[i] & 1 for i in range(9)), flg
    dn = O.doc_norms_f64(x)
    for i in range(9):
        s = O.cosine_scores_f64(x, q[i], dn)
        if qc[i] != -1:
            s[coll != qc[i]] = -np.inf
        ts, ti = O.topk_desc(s, k)
        assert cnt[i] == len(ti) and np.array_equal(I[i, :len(ti)], ti), (i, qc[i])
        assert np.array_equal(S[i, :len(ti)], ts)
    assert cnt[5] == 0 and tau[5] == -np.inf


def test_threshold_pass_count(T):
    """64 random queries at n = 40 000: the rows whose float64 score x ||q|| reaches tau are at least k'
    for every query, and their median count lies within [aim / 2, 2 aim] of the plan's aim.  The same
    band is first checked, on the CPU, for the threshold the full-score pass took -- the exact ks-th
    best sample score -- so that the inputs are known to be fair."""
    n, d, k, nq = 40000, 768, 100, 64
    rng = np.random.default_rng(4242)
    x = rng.standard_normal((n, d)).astype(np.float32)
    q = rng.standard_normal((nq, d)).astype(np.float32)
    c = Case(T, x, q)
    S, I, cnt, flg, tau, kp = c.search(nq, k)
    aim = plan(n, kp)[0]
    xn = x.astype(np.float64)
    xn /= np.linalg.norm(xn, axis=1, keepdims=True)
    sc = xn @ q.astype(np.float64).T                  # [n, nq]: cosine x ||q||
    rows = sample_rows(n, kp)
    before = np.array([np.sum(sc[:, i] >= kth_largest(sc[rows, i], KS)) for i in range(nq)])
    assert aim / 2 <= np.median(before) <= 2 * aim, (np.median(before), aim)
    counts = np.array([np.sum(sc[:, i] >= tau[i]) for i in range(nq)])
    print(f"pass count: aim {aim:.0f}, median {np.median(counts):.0f} (full-score threshold {np.median(before):.0f}), "
          f"min {counts.min()}, max {counts.max()}")
    assert counts.min() >= kp, counts.min()
    assert aim / 2 <= np.median(counts) <= 2 * aim, (np.median(counts), aim)
    assert_exact_and_certified(S, I, cnt, flg, *CO.dense_topk_exact(x, q, k), k, "pass count")
