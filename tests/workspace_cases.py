"""The workspace contract of thr_hip.h, as a harness and a registry (tests/test_workspace_cases_host.py
proves on the CPU that the harness bites; tests/test_gpu_workspace.py runs the registry on the device).

The contract: what a workspace holds on entry is never read, and nothing outside
[workspace, workspace + thr_*_workspace_bytes(...)) is written.  ``exercise`` holds one entry point to it:
two shapes A and B of the same entry, B's workspace a prefix of a slab sized for A, and three prior states
of that slab, all deterministic --

* ZERO   every byte 0x00;
* ONES   every byte 0xFF (NaN / -1 / a count of four billion);
* LIVED  what a call of the same entry at the OTHER shape left behind: valid-looking small integers
         and finite scores at another carve, what a serving process hands to every call but its first.

Every run of a shape must give the same bytes in every defined output, those bytes must be the
reference's, and every byte of the slab outside the exact view the call was handed must be as it was.

An ``Adapter`` is one entry point with its two shapes: need(shape) bytes, run(shape, workspace) ->
{name: tensor}, expected(shape) -> {name: array} (the oracle of the cases module the inputs come from;
a subset of the names), undefined(shape, outputs) -> the outputs without the regions thr_hip.h calls
undefined (UNDEFINED lists them with the header's words; nothing else is cut), and rows(shape, outputs)
-> which leading-axis rows of the expected arrays the reference answers (all, but for the two flags by
which an entry says "not this row": a dense query that is not THR_FLAG_CERTIFIED is thr_dense_rescue's,
a text that is THR_TEXT_EXCEPTIONAL is the host's).

Inputs are the built cases of the neighbouring modules (dense_cases, bm25_cases, graph_cases,
entity_cases, text_cases, vocab_grow_cases, graph_ingest_cases, scope_clause_cases); where an entry has
no cases module (csr_compact, lexical_build, scope_resolve, dense_topk_rows) the generator of its own
GPU test is restated here at the smallest size that still has more than one slice."""
import contextlib
import functools
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

GUARD, ALIGN = 4096, 256            # bytes on either side of the room; Arena's alignment
ZERO, ONES, LIVED = "zero", "ones", "lived"
FILL = {ZERO: 0x00, ONES: 0xFF}

# The only output regions exempt from comparison, each with the words of include/thr_hip.h that make it so.
UNDEFINED = {
    "csr": "ids_out / pay_out behind *nnz_out",
    "scope_rows": "``rows`` behind min(rowptr[n_preds], cap)",
    "token_rows": "tok_doc / tok_term behind *n_total",
    "unknown": "unknown_off / unknown_len / unknown_term behind *n_unknown",
    "new_keys": "new_ptr behind entry *n_new, new_bytes behind min(*n_new_bytes, new_bytes_capacity)",
    # two more, which no byte-for-byte rule can include: the header gives these outputs no defined value at all
    "graph_overflow": "such a query keeps THR_FLAG_OVERFLOW and its list is incomplete",
    "grow_collision": "the numbering is not to be used",
}


class Slab:
    """One uint8 buffer [GUARD | room of ``need`` bytes | GUARD]; the room starts on an ALIGN boundary.
    ``view(nbytes)`` is the exact workspace a call is handed: the first nbytes of the room."""

    def __init__(self, need: int, device):
        assert need > 0
        self.need = int(need)
        self.buf = torch.empty(GUARD + self.need + ALIGN + GUARD, dtype=torch.uint8, device=device)
        self.start = GUARD + (-(self.buf.data_ptr() + GUARD)) % ALIGN
        assert (self.buf.data_ptr() + self.start) % ALIGN == 0 and self.start + self.need + GUARD <= self.buf.numel()

    def fill(self, byte: int) -> None:
        self.buf.fill_(byte)

    def view(self, nbytes: int) -> torch.Tensor:
        assert 0 < nbytes <= self.need, f"a view of {nbytes} bytes in a room of {self.need}"
        return self.buf[self.start:self.start + nbytes]

    @contextlib.contextmanager
    def unchanged_outside(self, view: torch.Tensor, what: str = ""):
        """Every byte of the slab outside ``view`` -- the guards and, for a small shape in a slab sized for
        a large one, the leftovers behind it -- is the same after the block as before it."""
        lo = view.data_ptr() - self.buf.data_ptr()
        hi = lo + view.numel()
        assert self.start == lo and hi <= self.start + self.need
        before = (self.buf[:lo].clone(), self.buf[hi:].clone())
        yield
        if self.buf.is_cuda:
            torch.cuda.synchronize()
        for name, was, now, base in (("in front of", before[0], self.buf[:lo], 0), ("behind", before[1], self.buf[hi:], hi)):
            if not torch.equal(was, now):
                at = int(torch.nonzero(was != now)[0]) + base
                raise AssertionError(f"{what}: byte {at - lo} relative to the workspace ({name} it, {hi - lo} bytes long) was written")


class Adapter(NamedTuple):
    name: str
    sizes: Tuple[str, ...]                   # the thr_*_workspace_bytes exports that size its workspace
    shapes: Dict[str, object]                # {"A": the larger shape, "B": the smaller}
    need: Callable[[object], int]
    run: Callable[[object, torch.Tensor], Dict[str, torch.Tensor]]
    expected: Callable[[object], Dict[str, np.ndarray]]
    undefined: Optional[Callable[[object, Dict[str, np.ndarray]], Dict[str, np.ndarray]]] = None
    rows: Optional[Callable[[object, Dict[str, np.ndarray]], np.ndarray]] = None
    min_rows: float = 1.0                    # the share of rows ``rows`` must at least keep
    family: str = ""                         # "dense" / "bm25": run again under the knobs of that family


def host_outputs(adapter: Adapter, shape, out: Dict[str, torch.Tensor]) -> Dict[str, np.ndarray]:
    """The defined outputs of one run, on the host."""
    got = {k: (v.detach().contiguous().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)) for k, v in out.items()}
    return adapter.undefined(shape, got) if adapter.undefined else got


def run_once(adapter: Adapter, slab: Slab, key: str, state: str) -> Dict[str, np.ndarray]:
    shape = adapter.shapes[key]
    view = slab.view(adapter.need(shape))
    if state != LIVED:
        slab.fill(FILL[state])
    with slab.unchanged_outside(view, f"{adapter.name} shape {key} on {state}"):
        out = adapter.run(shape, view)
    return host_outputs(adapter, shape, out)


def assert_same(a: Dict[str, np.ndarray], b: Dict[str, np.ndarray], what: str) -> None:
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, f"{what}: {k}: {a[k].shape} {a[k].dtype} != {b[k].shape} {b[k].dtype}"
        if a[k].tobytes() != b[k].tobytes():
            x, y = a[k].reshape(-1).view(np.uint8), b[k].reshape(-1).view(np.uint8)
            at = int(np.flatnonzero(x != y)[0]) // max(a[k].dtype.itemsize, 1)
            raise AssertionError(f"{what}: output {k!r} differs from element {at} on ({int((x != y).sum())} bytes differ): "
                                 f"{a[k].reshape(-1)[at:at + 4]} != {b[k].reshape(-1)[at:at + 4]}")


def assert_expected(adapter: Adapter, key: str, got: Dict[str, np.ndarray]) -> None:
    shape = adapter.shapes[key]
    exp = adapter.expected(shape)
    assert exp, f"{adapter.name}: no reference"
    rows = adapter.rows(shape, got) if adapter.rows else None
    if rows is not None:
        assert rows.mean() >= adapter.min_rows - 1e-12, \
            f"{adapter.name} shape {key}: only {int(rows.sum())} of {len(rows)} rows are the reference's to answer"
    for k, e in exp.items():
        g = got[k]
        if rows is not None and g.ndim and g.shape[0] == len(rows):
            g, e = g[rows], e[rows]
        assert g.shape == e.shape and g.dtype == e.dtype, f"{adapter.name} shape {key}: {k}: {g.shape} {g.dtype}, the reference has {e.shape} {e.dtype}"
        if g.tobytes() != e.tobytes():
            bad = np.flatnonzero(g.reshape(-1).view(np.uint8) != e.reshape(-1).view(np.uint8))
            at = int(bad[0]) // max(g.dtype.itemsize, 1)
            raise AssertionError(f"{adapter.name} shape {key}: output {k!r} is not the reference's from element {at} on: "
                                 f"{g.reshape(-1)[at:at + 4]} != {e.reshape(-1)[at:at + 4]}")


def exercise(adapter: Adapter, device) -> None:
    """B on ZERO, B on ONES, A then B, B then A on one slab sized for A: the same bytes from every run of a
    shape, the reference's, and not a byte written outside the view of any call."""
    need_a, need_b = adapter.need(adapter.shapes["A"]), adapter.need(adapter.shapes["B"])
    assert need_a >= need_b > 0, f"{adapter.name}: shape A needs {need_a} bytes, shape B {need_b}: A is the larger one"
    slab = Slab(need_a, device)
    b_zero = run_once(adapter, slab, "B", ZERO)
    b_ones = run_once(adapter, slab, "B", ONES)
    a_first = run_once(adapter, slab, "A", LIVED)        # (on 0xFF and what B left)
    b_lived = run_once(adapter, slab, "B", LIVED)        # A then B
    a_lived = run_once(adapter, slab, "A", LIVED)        # B then A
    assert_same(b_zero, b_ones, f"{adapter.name}: shape B on a zeroed workspace and on one of 0xFF")
    assert_same(b_zero, b_lived, f"{adapter.name}: shape B on a zeroed workspace and behind a call of shape A")
    assert_same(a_first, a_lived, f"{adapter.name}: shape A on 0xFF and behind a call of shape B")
    assert_expected(adapter, "B", b_zero)
    assert_expected(adapter, "A", a_first)


# =============================================================================================== the registry
# Everything below builds device inputs lazily (the first run of an adapter) and keeps them for the process.
from triple_hybrid_rag_amd import _native as N  # noqa: E402

CERTIFIED, OVERFLOW, EXACT = N.THR_FLAG_CERTIFIED, N.THR_FLAG_OVERFLOW, N.THR_FLAG_EXACT


def _pkg():
    import triple_hybrid_rag_amd as T
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a)).cuda()         # (a copy: the cases' arrays are read-only)
    return t if dtype is None else t.to(dtype)


def _lib():
    return N.load()


# ------------------------------------------------------------------------------------------------ dense
N_DENSE = 12001                                      # sampled (> CAND_CAP / 2 rows), a ragged last row tile
DENSE_SHAPES = {"A": (70, 100), "B": (5, 10)}        # (queries, k)


@functools.lru_cache(maxsize=None)
def _dense_index(dim: int, shortlist: str):
    import dense_cases as DC
    x, _ = DC.planted(N_DENSE, dim)
    return _pkg().GpuIndex(doc_base=DC.DOC_BASE).set_dense(x, shortlist=shortlist)


@functools.lru_cache(maxsize=None)
def _dense_queries(dim: int) -> torch.Tensor:
    import dense_cases as DC
    return dev(DC.planted(N_DENSE, dim)[1])


def _dense_expected(dim: int, shape) -> Dict[str, np.ndarray]:
    """The oracle's lists at k = 100, cut: a top-k under (score desc, id asc) is a prefix of the top-100."""
    import dense_cases as DC
    nq, k = shape
    S, I, cnt = DC.planted_oracle(N_DENSE, dim, 100)
    return dict(S=np.ascontiguousarray(S[:nq, :k]), I=np.ascontiguousarray(I[:nq, :k]),
                cnt=np.minimum(cnt[:nq], k).astype(np.int32))


def _certified(shape, got) -> np.ndarray:
    return (got["flags"].astype(np.int64) & CERTIFIED) != 0


def _kprime(k: int, f16: bool) -> int:
    return min(N.THR_DENSE_MAX_K, k + (92 if f16 else 28))     # GpuIndex._kprime


def _dense_scan_adapter(name: str, dim: int, shortlist: str) -> Adapter:
    import dense_cases as DC
    f16 = shortlist != "f32"

    def need(shape):
        size = N.dense_f16_workspace_bytes if f16 else N.dense_workspace_bytes
        return size(N_DENSE, dim, shape[0], _kprime(shape[1], f16))

    def run(shape, ws):
        nq, k = shape
        ix, q = _dense_index(dim, shortlist), _dense_queries(dim)[:nq].contiguous()
        if f16:
            with N.dense_f16_flavour(shortlist == "f16-anydim"):
                S, I, cnt, flg = N.dense_topk_f16(ix.docs, ix.docs16, ix.doc_rel_err, ix.dnorm, ix.inv_norm, q, k,
                                                  _kprime(k, True), DC.DOC_BASE, ws)
        else:
            S, I, cnt, flg = N.dense_topk(ix.docs, ix.dnorm, ix.inv_norm, q, k, _kprime(k, False), DC.DOC_BASE, ws)
        return dict(S=S, I=I, cnt=cnt, flags=flg)
    return Adapter(name, ("thr_dense_f16_workspace_bytes" if f16 else "thr_dense_workspace_bytes",), DENSE_SHAPES, need, run,
                   functools.partial(_dense_expected, dim), rows=_certified, min_rows=0.6, family="dense")


def _dense_trio_adapter(dim: int = 768) -> Adapter:
    """thr_dense_shortlist_f16 -> thr_dense_floor -> thr_dense_finish_f16 as one unit: the workspace is in its
    prior state before the shortlist only (the finish reads what the shortlist left: the header's exception)."""
    import dense_cases as DC

    def need(shape):
        return N.dense_f16_workspace_bytes(N_DENSE, dim, shape[0], _kprime(shape[1], True))

    def run(shape, ws):
        nq, k = shape
        ix, q, kp = _dense_index(dim, "f16"), _dense_queries(dim)[:nq].contiguous(), _kprime(k, True)
        m = _pkg().index.floor_width(k, 1)
        lb = N.dense_shortlist_f16(ix.docs, ix.docs16, ix.doc_rel_err, ix.inv_norm, q, kp, m, ws)
        gfloor = N.dense_floor(lb[None].contiguous(), k)
        S, I, cnt, flg = N.dense_finish_f16(ix.docs, ix.docs16, ix.doc_rel_err, ix.dnorm, ix.inv_norm, q, k, kp, gfloor,
                                            DC.DOC_BASE, ws)
        return dict(top_lb=lb, gfloor=gfloor, S=S, I=I, cnt=cnt, flags=flg)
    return Adapter(f"dense_shortlist_floor_finish/copy/{dim}", ("thr_dense_f16_workspace_bytes",), DENSE_SHAPES, need, run,
                   functools.partial(_dense_expected, dim), rows=_certified, min_rows=0.6, family="dense")


def _dense_exact_adapter(dim: int = 768) -> Adapter:
    import dense_cases as DC

    def need(shape):
        return int(_lib().thr_dense_exact_workspace_bytes(N_DENSE, shape[0]))

    def run(shape, ws):
        nq, k = shape
        ix = _dense_index(dim, "f32")
        S, I, cnt, flg = N.dense_topk_exact(ix.docs, ix.dnorm, _dense_queries(dim)[:nq].contiguous(), k, DC.DOC_BASE, workspace=ws)
        return dict(S=S, I=I, cnt=cnt, flags=flg)

    def expected(shape):
        return dict(_dense_expected(dim, shape), flags=np.full(shape[0], CERTIFIED | EXACT, dtype=np.int32))
    return Adapter(f"dense_topk_exact/{dim}", ("thr_dense_exact_workspace_bytes",), DENSE_SHAPES, need, run, expected, family="dense")


def _dense_rescue_adapter(dim: int = 768) -> Adapter:
    """A result whose flags are a mix: two queries of three certified and holding the oracle's rows, the third
    cleared (flags 0, or THR_FLAG_OVERFLOW alone) and holding junk: the call redoes exactly those, in place."""
    import dense_cases as DC

    def cleared(nq):
        return np.arange(nq) % 3 == 1

    def need(shape):
        return N.dense_rescue_workspace_bytes(*shape)

    def run(shape, ws):
        nq, k = shape
        e, redo = _dense_expected(dim, shape), cleared(nq)
        S, I, cnt = e["S"].copy(), e["I"].copy(), e["cnt"].copy()
        S[redo], I[redo], cnt[redo] = 0.25, 5, 3
        flg = np.where(redo, np.where(np.arange(nq) % 2 == 0, OVERFLOW, 0), CERTIFIED).astype(np.int32)
        ix = _dense_index(dim, "f32")
        tile = torch.empty((2, nq, k), dtype=torch.int64, device="cuda")
        dS, dI, dcnt, dflg = tile[0].view(torch.float64), tile[1], dev(cnt), dev(flg)
        dS.copy_(dev(S))
        dI.copy_(dev(I))
        n = N.dense_rescue(ix.docs, ix.dnorm, _dense_queries(dim)[:nq].contiguous(), dS, dI, dcnt, dflg, DC.DOC_BASE, ws)
        return dict(S=dS, I=dI, cnt=dcnt, flags=dflg, n_rescued=n)

    def expected(shape):
        redo = cleared(shape[0])
        return dict(_dense_expected(dim, shape), flags=np.where(redo, CERTIFIED | EXACT, CERTIFIED).astype(np.int32),
                    n_rescued=np.array([redo.sum()], dtype=np.int32))
    return Adapter(f"dense_rescue/{dim}", ("thr_dense_rescue_workspace_bytes",), DENSE_SHAPES, need, run, expected, family="dense")


ROWS_ID_BASE = 1000
ROWS_SCOPES = 7


@functools.lru_cache(maxsize=None)
def _rows_inputs(dim: int, nq: int, k: int):
    """The scope mix of test_dense_topk_rows_equals_oracle over the planted corpus: row lists of 0, 1, k - 1, k,
    k + 1, 3000 and 50 rows (the duplicates and the zero row inside), many queries on the long list, the others
    spread, one query without a scope and one with a scope no list has."""
    import dense_cases as DC
    from oracle import thr_oracle as O
    x, q = DC.planted(N_DENSE, dim)
    rng = np.random.default_rng(dim + k)
    sizes = [0, 1, max(k - 1, 1), k, k + 1, 3000, 50]
    lists = [np.sort(rng.choice(N_DENSE, s, replace=False)).astype(np.int32) for s in sizes]
    lists[5] = np.union1d(lists[5], np.arange(195, 235)).astype(np.int32)
    lists[6] = np.union1d(lists[6], [13, 199]).astype(np.int32)
    P = len(lists)
    assert P == ROWS_SCOPES
    mix = [5] * 19 + list(range(P)) + [6, 4, -1, P + 3]
    qscope = np.array((mix * 3)[:nq] if nq > 5 else [5, 0, 6, -1, 3], dtype=np.int32)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in lists])]).astype(np.int64)
    rows = np.concatenate(lists).astype(np.int32)
    dn = O.doc_norms_f64(x)
    S = np.full((nq, k), -np.inf)
    I = np.full((nq, k), -1, dtype=np.int64)
    cnt = np.zeros(nq, dtype=np.int32)
    for i, p in enumerate(qscope.tolist()):
        if 0 <= p < P and len(lists[p]):
            s = O.cosine_scores_f64(x[lists[p]], q[i], dn[lists[p]])
            ts, ti = O.topk_desc(s, k, lists[p].astype(np.int64) + ROWS_ID_BASE)
            S[i, :len(ts)], I[i, :len(ti)], cnt[i] = ts, ti, len(ti)
    exp = dict(S=S, I=I, cnt=cnt, flags=np.full(nq, CERTIFIED | EXACT, dtype=np.int32))
    return dev(rowptr), dev(rows), dev(qscope), exp


def _dense_rows_adapter(dim: int = 768) -> Adapter:
    def need(shape):
        return int(_lib().thr_dense_topk_rows_workspace_bytes(shape[0], ROWS_SCOPES, shape[1]))

    def run(shape, ws):
        nq, k = shape
        rowptr, rows, qscope, _ = _rows_inputs(dim, nq, k)
        ix = _dense_index(dim, "f32")
        S, I, cnt, flg = N.dense_topk_rows(ix.docs, ix.dnorm, _dense_queries(dim)[:nq].contiguous(), k, rowptr, rows, qscope,
                                           ROWS_ID_BASE, workspace=ws)
        return dict(S=S, I=I, cnt=cnt, flags=flg)
    return Adapter(f"dense_topk_rows/{dim}", ("thr_dense_topk_rows_workspace_bytes",), DENSE_SHAPES, need, run,
                   lambda shape: _rows_inputs(dim, *shape)[3], family="dense")


def dense_adapters() -> List[Adapter]:
    return [_dense_scan_adapter("dense_topk/768", 768, "f32"),
            _dense_scan_adapter("dense_topk_f16/copy/768", 768, "f16"),
            _dense_scan_adapter("dense_topk_f16/copy/1024", 1024, "f16"),
            _dense_scan_adapter("dense_topk_f16/inline/768", 768, "f16-inline"),
            _dense_scan_adapter("dense_topk_f16/anydim/96", 96, "f16-anydim"),
            _dense_trio_adapter(), _dense_exact_adapter(), _dense_rescue_adapter(), _dense_rows_adapter()]


# ------------------------------------------------------------------------------------------------- BM25
@functools.lru_cache(maxsize=None)
def _bm25_index(cname: str):
    import bm25_cases as BC
    c = BC.corpus(cname)
    idx = _pkg().GpuIndex().set_lexical(c.rowptr, c.post_doc, c.post_tf, c.doclen, c.idf, c.avgdl, k1=BC.DEFAULT[0],
                                        b=BC.DEFAULT[1], dense_share=c.share)
    if c.coll is not None:
        idx.set_collections(c.coll)
    return idx


def _bm25_rows(cname: str, cases: Tuple[str, ...], max_terms: int) -> np.ndarray:
    """The rows of the corpus' table that belong to ``cases`` and hold at most ``max_terms`` terms."""
    import bm25_cases as BC
    c = BC.corpus(cname)
    rows = np.concatenate([c.rows(name) for name in cases])
    return rows[[(c.queries[p] >= 0).sum() <= max_terms for p in rows]]


def _bm25_adapter(name: str, cname: str, cases: Tuple[str, ...], ks: Tuple[int, int], conj: bool = False,
                  dense_rows: bool = True) -> Adapter:
    """Shape A: every row of the cases, the table at its full width, k = ks[0]; shape B: the rows of at most two
    terms, a table two columns wide, k = ks[1] -- other queries, another max_terms, another k."""
    import bm25_cases as BC
    shapes = {"A": (BC.MT, ks[0]), "B": (2, ks[1])}

    def need(shape):
        mt, k = shape
        return N.bm25_workspace_bytes(len(_bm25_rows(cname, cases, mt)), mt, k)

    def run(shape, ws):
        mt, k = shape
        c, idx = BC.corpus(cname), _bm25_index(cname)
        rows = _bm25_rows(cname, cases, mt)
        L = idx.lex
        qc = dev(c.qcoll[rows]) if c.coll is not None else None
        S, I, cnt = N.bm25_topk(L["rowptr"], L["post_doc"], L["post_tf"], L["doclen"], L["idf"], L["avgdl"],
                                dev(np.ascontiguousarray(c.queries[rows][:, :mt])), k, 0, L["k1"], L["b"], bounds=L["bounds"],
                                conjunctive=conj, doc_coll=idx.doc_coll if qc is not None else None, query_coll=qc,
                                workspace=ws, dense=L["dense"] if dense_rows else None)
        return dict(S=S, I=I, cnt=cnt)

    def expected(shape):
        mt, k = shape
        rows = _bm25_rows(cname, cases, mt)
        assert len(rows) >= 2
        ES, EI, Ecnt = BC.expected(cname, BC.DEFAULT[0], BC.DEFAULT[1], conj)
        cnt = np.minimum(Ecnt[rows], k).astype(np.int32)
        live = np.arange(k)[None, :] < cnt[:, None]
        return dict(S=np.where(live, ES[rows][:, :k], -np.inf), I=np.where(live, EI[rows][:, :k], -1).astype(np.int64), cnt=cnt)
    return Adapter(name, ("thr_bm25_workspace_bytes",), shapes, need, run, expected, family="bm25")


def bm25_adapters() -> List[Adapter]:
    values = ("saturate", "tf_ladder", "idf_spread", "k1b")
    stageb = ("stage_b_wins", "stage_b_skipped", "stage_b_tie")
    sliced = ("slice_ties", "slice_saturate")
    return [_bm25_adapter("bm25/values/or", "values", values, (64, 10)),                       # the wave walk, probed rows
            _bm25_adapter("bm25/values/or/k>64", "values", values, (128, 65)),                 # the workgroup walk
            _bm25_adapter("bm25/values/or/no_rows", "values", values, (64, 10), dense_rows=False),
            _bm25_adapter("bm25/values/and", "values", ("saturate", "tf_ladder"), (65, 10), conj=True),
            _bm25_adapter("bm25/stageb/or", "stageb", stageb, (64, 10)),                       # sweeps run, are skipped, tie
            _bm25_adapter("bm25/stageb/or/k>64", "stageb", stageb, (128, 65)),
            _bm25_adapter("bm25/stageb/or/no_rows", "stageb", stageb, (65, 10), dense_rows=False),
            _bm25_adapter("bm25/sliced/or+filter", "sliced", sliced, (64, 10)),                # sliced sweeps, a collection filter
            _bm25_adapter("bm25/sliced/or+filter/k>64", "sliced", sliced, (128, 65)),
            _bm25_adapter("bm25/sliced/or+filter/no_rows", "sliced", sliced, (64, 10), dense_rows=False),   # sliced walks
            _bm25_adapter("bm25/sliced/and+filter", "sliced", sliced, (65, 10), conj=True)]


# ------------------------------------------------------------------------------------------------ graph
GRAPH_WINDOW = "whole"
GRAPH_B = {"small": ("distances-h2", "asbuilt"), "full": ("sum_order", "full"), "global": ("seeds_sixteen", "global")}


@functools.lru_cache(maxsize=None)
def _graph_inputs(name: str, tier: str):
    import graph_cases as GC
    case = GC.build(name, GRAPH_WINDOW, tier)
    base, n = case.window
    g = tuple(dev(a) for a in case.g)
    tr = N.graph_transpose_mentions(g[2], g[3], g[4], base, n)
    doc = case.doc_label if case.doc_label is not None else GC.chunk_labels(case.window)
    ql = (np.arange(case.nq) % 3).astype(np.int32) if case.query_label is None else case.query_label.copy()
    ql[::4] = -1                                        # (labels and "no filter" in one batch)
    return case, g, dev(case.seeds), tr, doc, ql


def _graph_adapter(tier: str, scoped: bool, transposed: bool) -> Adapter:
    import graph_cases as GC
    shapes = {"A": ("fallback_reuse", "asbuilt"), "B": GRAPH_B[tier]}

    def need(shape):
        case = _graph_inputs(*shape)[0]
        return N.graph_workspace_bytes(case.nq, case.n_entities if transposed else 0)

    def run(shape, ws):
        case, g, seeds, tr, doc, ql = _graph_inputs(*shape)
        base, n = case.window
        if scoped:
            S, I, cnt, flg = N.graph_topk_scoped(*g, seeds, case.hops, case.k, base, n, dev(doc), dev(ql),
                                                 transposed=tr if transposed else None, workspace=ws)
        else:
            S, I, cnt, flg = N.graph_topk(*g, seeds, case.hops, case.k, base, n, transposed=tr if transposed else None,
                                          workspace=ws)
        return dict(S=S, I=I, cnt=cnt, flags=flg)

    def expected(shape):
        case, _, _, _, doc, ql = _graph_inputs(*shape)
        exp = GC.expected(case, GRAPH_WINDOW, ql, doc) if scoped else GC.expected(case, GRAPH_WINDOW)
        S = np.full((case.nq, case.k), -np.inf)
        I = np.full((case.nq, case.k), -1, dtype=np.int64)
        cnt = np.zeros(case.nq, dtype=np.int32)
        for q, (es, ei) in enumerate(exp):
            S[q, :len(es)], I[q, :len(ei)], cnt[q] = es, ei, len(ei)
        out = dict(S=S, I=I, cnt=cnt)
        if not scoped:      # (which queries a scope keeps on chip is the scope's matter; unscoped, the cases say)
            beyond = GC.beyond_full(case)
            out["flags"] = np.where(beyond, (CERTIFIED | EXACT) if transposed else OVERFLOW, CERTIFIED).astype(np.int32)
        return out

    def complete(shape, got):
        return (got["flags"].astype(np.int64) & OVERFLOW) == 0

    def undefined(shape, got):
        """UNDEFINED["graph_overflow"]: the rows of a query that comes back with THR_FLAG_OVERFLOW (no transposed
        mentions: which entities the full on-chip walk holds when it overflows depends on the order of its atomics)."""
        keep = complete(shape, got)
        out = dict(got)
        for k in ("S", "I", "cnt"):
            out[k] = np.where(keep.reshape((-1,) + (1,) * (got[k].ndim - 1)), got[k], 0).astype(got[k].dtype)
        return out
    name = f"graph_topk{'_scoped' if scoped else ''}/{tier}/{'transposed' if transposed else 'on_chip'}"
    return Adapter(name, ("thr_graph_workspace_bytes",), shapes, need, run, expected,
                   undefined=None if transposed else undefined, rows=None if transposed else complete, min_rows=0.15)


def graph_adapters() -> List[Adapter]:
    return [_graph_adapter(t, s, tr) for t in GRAPH_B for s in (False, True) for tr in (True, False)]


# ----------------------------------------------------------------------------------------------- entity
@functools.lru_cache(maxsize=None)
def _entity_inputs(name: str):
    import entity_cases as EC
    from triple_hybrid_rag_amd.index_entities import pack_entity_names, plan_needles
    case = EC.case(name)
    blob, ptr = pack_entity_names(case.names)
    plan = plan_needles(case.queries, case.limit)
    assert not plan.long_rows
    return tuple(dev(a) for a in (blob, ptr, plan.needles, plan.needle_len, plan.query_needles, plan.query_per))


def _entity_adapter(b: str) -> Adapter:
    import entity_cases as EC
    shapes = {"A": "six_thousand_needles", "B": b}

    def need(shape):
        a = _entity_inputs(shape)
        return N.entity_match_workspace_bytes(a[1].shape[0] - 1, a[2].shape[0], a[4].shape[0])

    def run(shape, ws):
        seeds, counts = N.entity_match(*_entity_inputs(shape), workspace=ws)
        return dict(seeds=seeds, counts=counts)

    def expected(shape):
        _, seeds, counts = EC.expected(shape)
        return dict(seeds=seeds, counts=counts)
    return Adapter(f"entity_match/{b}", ("thr_entity_match_workspace_bytes",), shapes, need, run, expected)


def entity_adapters() -> List[Adapter]:
    return [_entity_adapter("many_hits"), _entity_adapter("launch_geometry")]


# ------------------------------------------------------------------------------------------------- text
TEXT_A = "70000_texts_of_0_to_3_bytes"


def _text_case(name: str):
    return next(c for c in _all_text_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def _all_text_cases():
    import text_cases as TC
    return tuple(TC.all_cases())


@functools.lru_cache(maxsize=None)
def _text_inputs(name: str):
    from triple_hybrid_rag_amd.index_text import pack_texts
    case = _text_case(name)
    idx = _pkg().GpuIndex().set_vocabulary(case.vocab)
    blob, ptr = pack_texts(case.texts)
    return case, idx, dev(blob), dev(ptr), int(ptr[-1])


def _text_tokens(name: str, ws=None) -> dict:
    case, idx, blob, ptr, n_bytes = _text_inputs(name)
    X = idx.text
    return N.text_tokens(blob, ptr, n_bytes, X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"], workspace=ws)


@functools.lru_cache(maxsize=None)
def _text_expected(name: str):
    import text_cases as TC
    case = _text_case(name)
    return TC.expect_rows(case.texts, {t: i for i, t in enumerate(case.vocab)})


def _text_tokens_adapter(b: str) -> Adapter:
    shapes = {"A": TEXT_A, "B": b}

    def need(shape):
        case, _, _, _, n_bytes = _text_inputs(shape)
        return N.text_tokens_workspace_bytes(len(case.texts), n_bytes, N.text_token_capacity(len(case.texts), n_bytes))

    def run(shape, ws):
        rows = _text_tokens(shape, ws)
        return {k: rows[k] for k in ("doc", "term", "n_tokens", "flags", "n_total", "unknown_off", "unknown_len", "n_unknown")}

    def undefined(shape, got):
        """UNDEFINED["token_rows"] and ["unknown"]; the rows of the plain texts are named apart (term_plain,
        n_tokens_plain): the reference answers those, "the rows of a flagged text may hold anything"."""
        n_total, n_unknown = int(got["n_total"][0]), int(got["n_unknown"][0])
        out = dict(got, doc=got["doc"][:n_total], term=got["term"][:n_total], unknown_off=got["unknown_off"][:n_unknown],
                   unknown_len=got["unknown_len"][:n_unknown])
        plain = got["flags"] == 0
        out["n_tokens_plain"] = got["n_tokens"][plain]
        ok = (out["doc"] >= 0) & (out["doc"] < len(plain))
        out["term_plain"] = out["term"][ok][plain[out["doc"][ok]]]
        return out

    def expected(shape):
        doc, term, n_tokens, flags = _text_expected(shape)
        plain = flags == 0
        out = dict(flags=flags, n_tokens_plain=n_tokens[plain], term_plain=term[plain[doc]])
        if plain.all():
            out.update(doc=doc, term=term, n_tokens=n_tokens, n_total=np.array([len(doc)], dtype=np.int32),
                       n_unknown=np.array([(term < 0).sum()], dtype=np.int32))
        return out
    return Adapter(f"text_tokens/{b}", ("thr_text_tokens_workspace_bytes",), shapes, need, run, expected, undefined=undefined)


@functools.lru_cache(maxsize=None)
def _query_rows(name: str) -> dict:
    return _text_tokens(name)            # (a workspace of its own: this call is an input here)


def _query_terms_adapter(b: str) -> Adapter:
    import text_cases as TC
    shapes = {"A": TEXT_A, "B": b}

    def need(shape):
        return N.query_terms_workspace_bytes(len(_text_case(shape).texts))

    def run(shape, ws):
        terms, nd, fl = N.query_terms(_query_rows(shape), workspace=ws)
        return dict(terms=terms, n_distinct=nd, flags=fl)

    def expected(shape):
        case = _text_case(shape)
        terms, nd, flags = TC.expect_query_table(case.texts, {t: i for i, t in enumerate(case.vocab)})
        return dict(terms=terms, n_distinct=nd, flags=flags)

    def plain(shape, got):             # (an exceptional text's row is the host's: the surface patches it in)
        return (got["flags"] & N.THR_TEXT_EXCEPTIONAL) == 0
    return Adapter(f"query_terms/{b}", ("thr_query_terms_workspace_bytes",), shapes, need, run, expected, rows=plain, min_rows=0.5)


GROW_A = "one_new_token_100000_times_among_50_others"      # (100 050 occurrences: the longest list)


@functools.lru_cache(maxsize=None)
def _all_grow_cases():
    import vocab_grow_cases as VG
    return tuple(VG.all_cases())


@functools.lru_cache(maxsize=None)
def _grow_inputs(name: str):
    """thr_text_tokens over the case (an input here), and the restatement over the list it left."""
    import vocab_grow_cases as VG
    from triple_hybrid_rag_amd.index_text import pack_texts
    case = next(c for c in _all_grow_cases() if c.name == name)
    idx = _pkg().GpuIndex().set_vocabulary(case.vocab)
    X = idx.text
    blob, ptr = pack_texts(case.texts)
    n_bytes = int(ptr[-1])
    dblob, dptr = dev(blob), dev(ptr)
    rows = N.text_tokens(dblob, dptr, n_bytes, X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"])
    n_total, n_unknown = int(rows["n_total"].item()), int(rows["n_unknown"].item())
    n_vocab = X["term_ptr"].shape[0] - 1
    E = VG.expect_grow(blob.tobytes()[:n_bytes], ptr, rows["flags"].cpu().numpy(), rows["unknown_off"][:n_unknown].cpu().numpy(),
                       rows["unknown_len"][:n_unknown].cpu().numpy(), n_vocab, X["table"], case.hash_mask,
                       tok_term=rows["term"][:n_total].cpu().numpy())
    return case, X, dblob, dptr, n_bytes, rows, n_total, n_unknown, n_vocab, E


def _vocab_grow_adapter(b: str) -> Adapter:
    import vocab_grow_cases as VG
    shapes = {"A": GROW_A, "B": b}

    def need(shape):
        return N.vocab_grow_workspace_bytes(max(_grow_inputs(shape)[7], 1))

    def run(shape, ws):
        case, X, dblob, dptr, n_bytes, rows, n_total, n_unknown, n_vocab, E = _grow_inputs(shape)
        term = rows["term"][:n_total].clone() if n_total else None          # (patched in place)
        out = N.vocab_grow(dblob, dptr, n_bytes, X["table_dev"], rows, max(n_unknown, 1), n_vocab,
                           new_bytes_capacity=E["n_new_bytes"], hash_mask=case.hash_mask, term=term, workspace=ws)
        out = {k: out[k] for k in ("unknown_term", "new_bytes", "new_ptr", "n_new", "n_new_bytes", "status")}
        out["tok_term"] = term if term is not None else torch.zeros(0, dtype=torch.int32, device="cuda")
        return out

    def undefined(shape, got):
        """UNDEFINED["unknown"] and ["new_keys"]; under ["grow_collision"] the status word alone."""
        n_unknown = _grow_inputs(shape)[7]
        if int(got["status"][0]) & VG.COLLISION:
            return dict(status=got["status"])
        n_new, n_new_bytes = int(got["n_new"][0]), int(got["n_new_bytes"][0])
        room = len(got["new_bytes"]) - 16
        return dict(got, unknown_term=got["unknown_term"][:n_unknown], new_ptr=got["new_ptr"][:n_new + 1],
                    new_bytes=got["new_bytes"][:min(n_new_bytes, room)])

    def expected(shape):
        E = _grow_inputs(shape)[9]
        if E["collision"]:
            return dict(status=np.array([VG.COLLISION], dtype=np.int32))
        return dict(status=np.zeros(1, dtype=np.int32), n_new=np.array([E["n_new"]], dtype=np.int32),
                    n_new_bytes=np.array([E["n_new_bytes"]], dtype=np.int64), unknown_term=E["unknown_term"],
                    new_ptr=E["new_ptr"], new_bytes=E["new_bytes"], tok_term=E["tok_term"])
    return Adapter(f"vocab_grow/{b}", ("thr_vocab_grow_workspace_bytes",), shapes, need, run, expected, undefined=undefined)


def text_adapters() -> List[Adapter]:
    out = [_text_tokens_adapter(c.name) for c in _all_text_cases() if c.name != TEXT_A]
    out += [_query_terms_adapter("query_table_edges"), _query_terms_adapter("exceptional_texts_between_plain_neighbours")]
    return out + [_vocab_grow_adapter(c.name) for c in _all_grow_cases() if c.name != GROW_A]


# -------------------------------------------------------------------------------------------------- CSR
MERGE_A = "slice_edges"


@functools.lru_cache(maxsize=None)
def _merge_inputs(name: str):
    import graph_ingest_cases as GI
    c = GI.cases()[name]
    rows_a = len(c.rowptr_a) - 1
    return c, (dev(c.rowptr_a) if rows_a else None, dev(c.ids_a), dev(c.pay_a), dev(c.rowptr_b), dev(c.ids_b), dev(c.pay_b))


def _csr_merge_adapter(b: str, mode: int) -> Adapter:
    """mode 1: the set union (no payload, as the relations travel); mode 0: the multiset merge with its payload."""
    import graph_ingest_cases as GI
    shapes = {"A": MERGE_A, "B": b}

    def need(shape):
        c = GI.cases()[shape]
        return int(_lib().thr_csr_merge_workspace_bytes(len(c.rowptr_b) - 1, len(c.ids_a), len(c.ids_b)))

    def run(shape, ws):
        _, (rpa, ida, paya, rpb, idb, payb) = _merge_inputs(shape)
        two = mode == 0
        rp, ids, pay, nnz, status = N.csr_merge(rpa, ida, paya if two else None, rpb, idb, payb if two else None, bool(mode),
                                                workspace=ws)
        out = dict(rowptr=rp, ids=ids[:nnz], nnz=np.array([nnz], dtype=np.int64), status=np.array([status], dtype=np.int64))
        if two:
            out["pay"] = pay[:nnz]       # UNDEFINED["csr"]: cut at nnz_out
        return out

    def expected(shape):
        rp, ids, pay, nnz, status = GI.expected(GI.cases()[shape], mode)
        out = dict(rowptr=rp, ids=ids, nnz=np.array([nnz], dtype=np.int64), status=np.array([status], dtype=np.int64))
        if mode == 0:
            out["pay"] = pay
        return out
    return Adapter(f"csr_merge/{'union' if mode else 'multiset'}/{b}", ("thr_csr_merge_workspace_bytes",), shapes, need, run, expected)


@functools.lru_cache(maxsize=None)
def _compact_inputs(shape):
    """test_csr_compact_equals_numpy_restatement's generator: random rows (many empty), one long row that spans
    workgroup slices in shape A, ids outside the remap's range, a payload."""
    rows, long_row, n_ids, id_base = shape
    rng = np.random.default_rng(rows)
    lens = rng.integers(0, 9, rows) * (rng.random(rows) < 0.6)
    if long_row:
        lens[rows // 2] = long_row
    keep = rng.random(n_ids) < 0.7
    rowptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = np.concatenate([np.sort(rng.choice(n_ids, int(l), replace=False)) for l in lens if l]).astype(np.int64) + id_base
    ids[::7] = id_base + n_ids + rng.integers(0, 50, len(ids[::7]))           # outside: dropped
    if id_base:
        ids[3::11] = rng.integers(0, id_base, len(ids[3::11]))
    ids = ids.astype(np.int32)
    pay = rng.random(len(ids)).astype(np.float32)
    remap = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    i = ids.astype(np.int64) - id_base
    ok = (i >= 0) & (i < n_ids)
    kept = np.zeros(len(ids), dtype=bool)
    kept[ok] = remap[i[ok]] >= 0
    before = np.concatenate([[0], np.cumsum(kept)]).astype(np.int64)
    exp = dict(rowptr=before[rowptr], ids=(remap[i[kept]] + id_base).astype(np.int32), pay=pay[kept],
               nnz=np.array([kept.sum()], dtype=np.int64))
    return (dev(rowptr), dev(ids), dev(pay), dev(remap)), exp


def _csr_compact_adapter() -> Adapter:
    shapes = {"A": (3000, 600_011, 700_000, 700), "B": (300, 0, 500, 0)}    # (rows, a long row, ids, id base): 75 slices, 1

    def need(shape):
        (rowptr, ids, _, _), _ = _compact_inputs(shape)
        return int(_lib().thr_csr_compact_workspace_bytes(rowptr.shape[0] - 1, ids.shape[0]))

    def run(shape, ws):
        (rowptr, ids, pay, remap), _ = _compact_inputs(shape)
        rp, oi, op, kept = N.csr_compact(rowptr, ids, pay, remap, shape[3], workspace=ws)
        return dict(rowptr=rp, ids=oi[:kept], pay=op[:kept], nnz=np.array([kept], dtype=np.int64))   # UNDEFINED["csr"]
    return Adapter("csr_compact", ("thr_csr_compact_workspace_bytes",), shapes, need, run, lambda shape: _compact_inputs(shape)[1])


@functools.lru_cache(maxsize=None)
def _build_inputs(shape):
    """Shuffled (doc, term, tf) entries in which many pairs repeat (they add up: a pair split in two or more),
    with what the build must drop behind them: doc / term out of range, tf <= 0."""
    n_docs, n_vocab, n_pairs = shape
    rng = np.random.default_rng(n_pairs)
    doc, term, tf = rng.integers(0, n_docs, n_pairs), rng.integers(0, n_vocab, n_pairs), rng.integers(1, 6, n_pairs)
    assert len(np.unique(term.astype(np.int64) << 32 | doc)) < n_pairs, "some pair repeats"
    junk_d, junk_t, junk_f = [n_docs, -1, 5, 7, 9], [3, 3, n_vocab, 11, 2], [1, 1, 1, 0, -4]
    d2, t2, f2 = (np.concatenate(p).astype(np.int32) for p in ((doc, junk_d), (term, junk_t), (tf, junk_f)))
    perm = rng.permutation(len(d2))
    uk, inv = np.unique(term.astype(np.int64) << 32 | doc, return_inverse=True)
    df = np.bincount((uk >> 32).astype(np.int64), minlength=n_vocab).astype(np.int64)
    dl = np.bincount(doc, weights=tf, minlength=n_docs).astype(np.float32)
    dl[5] += 1                                   # (term out of range: still a token of chunk 5)
    exp = dict(rowptr=np.concatenate([[0], np.cumsum(df)]).astype(np.int64), post_doc=(uk & 0xFFFFFFFF).astype(np.int32),
               post_tf=np.bincount(inv, weights=tf).astype(np.int32), doclen=dl, df=df)
    return (dev(d2[perm]), dev(t2[perm]), dev(f2[perm])), exp


def _lexical_build_adapter() -> Adapter:
    shapes = {"A": (3000, 500, 40_000), "B": (50, 20, 300)}      # (docs, vocabulary, entries)

    def need(shape):
        return int(_lib().thr_lexical_build_workspace_bytes(shape[2] + 5, shape[1]))

    def run(shape, ws):
        (doc, term, tf), _ = _build_inputs(shape)
        rowptr, post_doc, post_tf, doclen, df = N.lexical_build(doc, term, tf, shape[0], shape[1], workspace=ws)
        return dict(rowptr=rowptr, post_doc=post_doc, post_tf=post_tf, doclen=doclen, df=df)   # (cut at nnz_out by the binding)
    return Adapter("lexical_build", ("thr_lexical_build_workspace_bytes",), shapes, need, run, lambda shape: _build_inputs(shape)[1])


def csr_adapters() -> List[Adapter]:
    import graph_ingest_cases as GI
    out = [_csr_merge_adapter(name, mode) for name, c in GI.cases().items() if name != MERGE_A for mode in c.modes]
    return out + [_csr_compact_adapter(), _lexical_build_adapter()]


# ------------------------------------------------------------------------------------------------ scope
SCOPE_PREDS = np.array([[0, -1, -1], [1, 7, -1], [-1, -1, -1], [2, -1, 1], [4, 39, 2], [3, -2, -1], [9, -1, -1], [-1, 7, -1]],
                       dtype=np.int32)


def _resolve_expected(masks: np.ndarray, cap: int) -> Dict[str, np.ndarray]:
    import scope_clause_cases as SC
    rowptr, rows, labels, ov = SC.np_resolve_masks(masks)
    return dict(rowptr=rowptr, rows=rows[:cap], labels=labels, overlap=np.array([ov], dtype=np.int32))


@functools.lru_cache(maxsize=None)
def _scope_inputs(shape):
    """test_scope_resolve_equals_numpy's columns and predicates (-1 = any value, below -1 = no row)."""
    import scope_clause_cases as SC
    n, P = shape
    rng = np.random.default_rng(n)
    cols = [rng.integers(0, 5, n).astype(np.int32), rng.integers(-1, 40, n).astype(np.int32), rng.integers(0, 3, n).astype(np.int32)]
    preds = SCOPE_PREDS[:P]
    tab = np.zeros((P, 3, 4), dtype=np.int32)           # the same predicates as a clause table: what SC restates
    tab[..., 0] = np.where(preds == -1, 0, np.where(preds < -1, 1, 2))
    tab[..., 1] = tab[..., 2] = np.maximum(preds, 0)
    masks = SC.table_masks(tab, [], 0, cols)         # (no predicate value is -1: a row without a value equals none)
    return [dev(c) for c in cols], dev(preds), _resolve_expected(masks, n)


def _cut_rows(shape, got):
    """UNDEFINED["scope_rows"]: behind min(rowptr[P], cap)."""
    return dict(got, rows=got["rows"][:min(int(got["rowptr"][-1]), len(got["rows"]))])


def _scope_resolve_adapter() -> Adapter:
    shapes = {"A": (10007, 8), "B": (777, 5)}            # (rows, predicates)

    def need(shape):
        return int(_lib().thr_scope_resolve_workspace_bytes(*shape))

    def run(shape, ws):
        cols, preds, _ = _scope_inputs(shape)
        rowptr, rows, labels, overlap = N.scope_resolve(cols, preds, workspace=ws)
        return dict(rowptr=rowptr, rows=rows, labels=labels, overlap=overlap)
    return Adapter("scope_resolve", ("thr_scope_resolve_workspace_bytes",), shapes, need, run,
                   lambda shape: _scope_inputs(shape)[2], undefined=_cut_rows)


@functools.lru_cache(maxsize=None)
def _clause_inputs(shape):
    """test_resolve_clauses_equals_numpy's columns and scopes: every clause kind in one call."""
    import scope_clause_cases as SC
    from triple_hybrid_rag_amd import index_scope as IS
    T = _pkg()
    n, n_cols = shape
    names = [f"a{c}" for c in range(n_cols)]
    cols = SC.resolve_columns(n, n_cols, seed=n * 10 + n_cols)
    cols[0][0] = -1
    cols[1][0], cols[1][n - 1] = SC.INT32_MAX, 0
    by_name = dict(zip(names, cols))
    scopes = SC.resolve_scopes(T, n_cols, names)
    masks = np.stack([SC.scope_mask(sc, by_name, T) for sc in scopes])
    keys = [tuple(IS.canonical_clause(sc[nm]) if nm in sc else None for nm in names) for sc in scopes]
    tab, sv = IS.encode_clauses(keys, n_cols)
    return [dev(c) for c in cols], tab, sv, _resolve_expected(masks, n)


def _scope_clauses_adapter() -> Adapter:
    shapes = {"A": (10007, 8), "B": (513, 3)}            # (rows, columns): 21 and 20 predicates

    def need(shape):
        return int(_lib().thr_scope_resolve_clauses_workspace_bytes(shape[0], _clause_inputs(shape)[1].shape[0]))

    def run(shape, ws):
        cols, tab, sv, _ = _clause_inputs(shape)
        rowptr, rows, labels, overlap = N.scope_resolve_clauses(cols, tab, sv, workspace=ws)
        return dict(rowptr=rowptr, rows=rows, labels=labels, overlap=overlap)
    return Adapter("scope_resolve_clauses", ("thr_scope_resolve_clauses_workspace_bytes",), shapes, need, run,
                   lambda shape: _clause_inputs(shape)[3], undefined=_cut_rows)


def scope_adapters() -> List[Adapter]:
    return [_scope_resolve_adapter(), _scope_clauses_adapter()]


@functools.lru_cache(maxsize=None)
def registry() -> Tuple[Adapter, ...]:
    out = dense_adapters() + bm25_adapters() + graph_adapters() + entity_adapters() + text_adapters() + csr_adapters() + \
        scope_adapters()
    assert len({a.name for a in out}) == len(out)
    return tuple(out)


# The entry points that read a workspace as a call before them left it: the header's two exceptions.  They
# have no size function of their own and are named here so that the host test can say why no adapter runs them alone.
EXCEPTIONS = {
    "thr_dense_finish_f16": "reads what thr_dense_shortlist_f16 left (run as one unit with it: dense_shortlist_floor_finish)",
    "thr_dense_scan_probe": "reads the previous call's tau",
    "thr_dense_scan_probe_f16": "reads the previous call's tau",
    "thr_dense_scan_stamps_f16": "reads the previous call's tau",
}
# thr_*_workspace_bytes exports without an adapter, each with its reason (none today)
SIZES_WITHOUT_ADAPTER: Dict[str, str] = {}
