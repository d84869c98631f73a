"""The workspace contract on the device (include/thr_hip.h, WORKSPACES; the audit table is DESIGN.md's
"Workspace contract"): every entry point that takes a workspace, at two shapes on one slab, gives the same
bits whatever the workspace held before -- zeros, 0xFF, or what a call of the other shape left -- the bits of
its oracle, and writes nothing outside the bytes it was handed (tests/workspace_cases.py holds the harness
and the adapters; tests/test_workspace_cases_host.py proves on the CPU that the harness catches a read
before a write and a write past the size).

A serving process never hands a clean workspace to a call: GpuIndex keeps one grow-only buffer per channel.
The last tests are that: one index, workspaces full of 0xFF, batches of 300, 7 and 64 queries one after
another, each byte-equal to the same call on a freshly built index.  The dense and the BM25 adapters run
again under the kernels' A/B knobs, each in a child process (the knobs are read once per process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import workspace_cases as W  # noqa: E402

ADAPTERS = {a.name: a for a in W.registry()}


@pytest.fixture(scope="module")
def T():
    import triple_hybrid_rag_amd as T
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    T._native.load()
    return T


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


@pytest.mark.parametrize("name", list(ADAPTERS))
def test_workspace_contract(T, name):
    """B on 0x00, B on 0xFF, A then B, B then A: byte-identical defined outputs, the oracle's, and every
    byte of the slab outside each call's view unchanged."""
    W.exercise(ADAPTERS[name], "cuda")


# ------------------------------------------------------------------------------------------ the index
N_DOCS, DIM = 12001, 768
BATCHES = ((300, 100), (7, 10), (64, 50))        # (queries, k), in this order on ONE index


_HOST = {}


def host_arrays():
    if not _HOST:
        from oracle import thr_oracle as O
        from triple_hybrid_rag_amd import synth
        doc, term, tf = synth.lexical_rows(0, N_DOCS, N_DOCS)
        csr = synth.build_lexical_csr(doc, term, tf, N_DOCS, synth.vocab_size(N_DOCS))
        nq = max(b[0] for b in BATCHES)
        _HOST.update(x=synth.dense_rows(0, N_DOCS, DIM), csr=csr, idf=O.bm25_idf(N_DOCS, csr.df_local),
                     avgdl=csr.sum_dl_local / N_DOCS, g=synth.build_graph(N_DOCS), q=synth.dense_queries(nq, DIM, N_DOCS),
                     qt=synth.lexical_queries(nq, csr.df_local, 4), seeds=synth.graph_queries(nq, N_DOCS, 3))
    return _HOST


def build_index(T):
    H = host_arrays()
    csr, g = H["csr"], H["g"]
    return (T.GpuIndex().set_dense(H["x"], shortlist="f16")
            .set_lexical(csr.rowptr, csr.post_doc, csr.post_tf, csr.doclen, H["idf"], H["avgdl"])
            .set_graph(g.ent_rowptr, g.ent_col, g.men_rowptr, g.men_chunk, g.men_conf))


def calls(nq, k):
    """(name, call on an index -> tuple of tensors) of the four searches at one batch shape."""
    H = host_arrays()
    q, qt, seeds = dev(H["q"][:nq]), dev(H["qt"][:nq]), dev(H["seeds"][:nq])

    def retrieve(ix):
        r = ix.retrieve_batch(q, qt, seeds, top_k=10, semantic_top_k=k, lexical_top_k=k, graph_top_k=k)
        out = [r.ids, r.scores, r.counts]
        for ch in ("semantic", "lexical", "graph"):
            out += list(r.channels[ch])
        return tuple(out) + (torch.as_tensor([int(r.rescued)]),)

    def dense(ix):
        S, I, cnt, n_rescued = ix.dense_search(q, k)
        return S, I, cnt, torch.as_tensor([n_rescued])
    return [("retrieve_batch", retrieve), ("dense_search", dense), ("bm25_search", lambda ix: tuple(ix.bm25_search(qt, k))),
            ("graph_search", lambda ix: tuple(ix.graph_search(seeds, k)))]


def test_an_index_whose_workspaces_are_never_clean_answers_like_a_fresh_one(T):
    N = T._native
    idx = build_index(T)
    nq0, k0 = BATCHES[0]
    idx.reserve(nq0, k0)
    idx._scratch("_ws_lex", N.bm25_workspace_bytes(nq0, 4, k0))
    idx._scratch("_ws_graph", N.graph_workspace_bytes(nq0, idx.graph["ent_rowptr"].shape[0] - 1))
    held = [idx._ws, idx._ws_rescue, idx._ws_lex, idx._ws_graph]
    assert all(w is not None and w.numel() > 0 for w in held)
    for w in held:
        w.fill_(0xFF)
    for nq, k in BATCHES:
        for name, call in calls(nq, k):
            got = call(idx)
            want = call(build_index(T))
            torch.cuda.synchronize()
            assert len(got) == len(want)
            for j, (a, b) in enumerate(zip(got, want)):
                assert a.shape == b.shape and a.dtype == b.dtype, f"{name} at {nq} x {k}, output {j}"
                assert torch.equal(a.contiguous().view(torch.uint8).cpu(), b.contiguous().view(torch.uint8).cpu()), \
                    f"{name} at {nq} queries, k = {k}: output {j} differs from the same call on a freshly built index"
    # the buffers were the ones filled: nothing was re-allocated behind the test's back
    assert [w.data_ptr() for w in held] == [idx._ws.data_ptr(), idx._ws_rescue.data_ptr(), idx._ws_lex.data_ptr(),
                                            idx._ws_graph.data_ptr()]


# -------------------------------------------------------------------------------------------- the knobs
KNOBS = ["THR_DENSE_MFMA=32", "THR_DENSE_F16=q", "THR_DENSE_QW=32", "THR_BM25_WALK=block", "THR_BM25_SHAPE=small"]


@pytest.mark.parametrize("knob", KNOBS)
def test_dense_and_bm25_adapters_under_a_knob_in_a_child_process(knob):
    """The alternate scans (32x32x16 MFMA shape, the 4-wave copy scan at every dim, 32 queries per wave at dim
    1024) and the alternate walks (stage A on the workgroup walk, the small block shape) carve the same
    workspaces: every adapter of the family again, in a process that reads the knob."""
    if os.environ.get("THR_WORKSPACE_KNOB_RUN"):
        pytest.skip("already inside a knob run")
    name, value = knob.split("=")
    family = "dense" if name.startswith("THR_DENSE") else "bm25"
    n = sum(a.family == family for a in ADAPTERS.values())
    assert n >= 9
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", os.path.abspath(__file__), "-k",
                          f"test_workspace_contract and {family}"],
                         env=dict(os.environ, THR_WORKSPACE_KNOB_RUN="1", **{name: value}), cwd=root, capture_output=True,
                         text=True, timeout=900)
    assert out.returncode == 0 and f"{n} passed" in out.stdout and "failed" not in out.stdout, \
        out.stdout[-3000:] + out.stderr[-1000:]
