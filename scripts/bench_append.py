#!/usr/bin/env python3
"""Cost of GpuIndex.append_rows on a dense + lexical index (default 1M x 768): wall and device time
of appending 1 / 256 / 16 384 chunks, the split by native call (CSR append, BM25 bounds, dense-term
rows, float16 quantisation of the tail, delta CSR build), and one retrieve_batch step before and
after.  Needs the GPU; prints one JSON line per measurement.

    python3 scripts/bench_append.py [--n 1000000] [--dim 768] [--queries 256] [--batches 1,256,16384]

--delete: the same for GpuIndex.delete_rows instead -- 1 / 256 / 16 384 rows spread over the corpus and
one whole "document" of 64 consecutive chunks (the deletes follow one another on one index); wall and
device time, thr_csr_compact alone with GB/s by device
events, first deleted row (what decides how many rows move), one retrieve_batch step before and after.

Kernel times proper come from a profiler run of its own:
    rocprofv3 --kernel-trace --stats -d <out> -- python3 scripts/bench_append.py --batches 16384
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import triple_hybrid_rag_amd as T   # noqa: E402
from triple_hybrid_rag_amd import _native as N, synth   # noqa: E402


def timed(fn, reps=1):
    """(result, wall ms, device ms) of fn() -- the wall clock ends in a device synchronise."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3 / reps, e0.elapsed_time(e1) / reps


def step_ms(idx, q, qt, steps=20):
    for _ in range(3):
        idx.retrieve_batch(q, qt, top_k=10)
    _, wall, _ = timed(lambda: idx.retrieve_batch(q, qt, top_k=10), steps)
    return wall


def delete_leg(a, batches):
    n = a.n
    v = synth.vocab_size(n)
    x = synth.dense_rows(0, n, a.dim)
    doc, term, tf = synth.lexical_rows(0, n, n)
    idx = T.GpuIndex().set_dense(x)
    idx.set_lexical_rows(doc, term, tf, v, n_docs=n)
    del x
    q = torch.from_numpy(synth.dense_queries(a.queries, a.dim, n)).cuda()
    qt = torch.from_numpy(synth.lexical_queries(a.queries, idx.df_local.cpu().numpy(), 4)).cuda()
    print(json.dumps({"n": n, "dim": a.dim, "shortlist": idx.shortlist, "postings": int(idx.lex["post_doc"].shape[0]),
                      "vocab": v, "step_ms_before": round(step_ms(idx, q, qt), 3)}), flush=True)
    rng = np.random.default_rng(1)
    cases = [(f"spread_{m}", np.sort(rng.choice(idx.n_docs - 70_000, m, replace=False))) for m in batches]
    cases.append(("document_64", np.arange(n // 2, n // 2 + 64)))
    for name, ids in cases:
        ids = ids[ids < idx.n_docs]
        # thr_csr_compact alone, on the index as it stands, into buffers of its own
        L = idx.lex
        nnz = int(L["post_doc"].shape[0])
        keep = torch.ones(idx.n_docs, dtype=torch.bool, device="cuda")
        keep[torch.from_numpy(ids).cuda()] = False
        rank = torch.cumsum(keep, 0, dtype=torch.int32) - 1
        remap = torch.where(keep, rank, torch.full_like(rank, -1))
        out0, out1 = (torch.empty(nnz, dtype=torch.int32, device="cuda") for _ in range(2))
        kept = N.csr_compact(L["rowptr"], L["post_doc"], L["post_tf"], remap, 0, out0, out1)[3]
        # (the C entry itself, without the wrapper's read-back of the kept count: launches only)
        lib, rows = N.load(), int(L["rowptr"].shape[0]) - 1
        need = int(lib.thr_csr_compact_workspace_bytes(rows, nnz))
        ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        rp_out, k_out = torch.empty(rows + 1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def compact():
            rc = lib.thr_csr_compact(L["rowptr"].data_ptr(), rows, nnz, L["post_doc"].data_ptr(), L["post_tf"].data_ptr(),
                                     remap.data_ptr(), idx.n_docs, 0, rp_out.data_ptr(), out0.data_ptr(), out1.data_ptr(),
                                     nnz, k_out.data_ptr(), ws.data_ptr(), need, st)
            assert rc == 0, rc
        compact()
        _, _, t_csr = timed(compact, 20)
        assert int(k_out.item()) == kept
        # bytes the three launches move: ids read twice, the payload once, the kept entries written, the
        # remap gathered twice (4 bytes per entry each time, mostly from cache), the row pointers in and out
        moved = nnz * 4 * (2 + 1 + 2) + kept * 8 + 16 * int(L["rowptr"].shape[0])
        del out0, out1
        _, wall, devt = timed(lambda: idx.delete_rows(ids))
        print(json.dumps({"delete": name, "rows": int(len(ids)), "first_deleted": int(ids[0]), "wall_ms": round(wall, 3),
                          "device_ms": round(devt, 3), "csr_compact_ms": round(t_csr, 4),
                          "csr_compact_GBps": round(moved / t_csr / 1e6, 1), "postings_before": nnz,
                          "postings_after": int(idx.lex["post_doc"].shape[0]), "n_docs": idx.n_docs,
                          "rows_moved": int(idx.n_docs - ids[0] // 32 * 32)}), flush=True)
    print(json.dumps({"step_ms_after": round(step_ms(idx, q, qt), 3), "n_docs": idx.n_docs}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--batches", default="1,256,16384")
    ap.add_argument("--delete", action="store_true", help="measure delete_rows instead of append_rows")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    if a.delete:
        return delete_leg(a, batches)
    n_all = a.n + sum(batches)
    v = synth.vocab_size(n_all)
    x = synth.dense_rows(0, n_all, a.dim)
    doc, term, tf = synth.lexical_rows(0, n_all, n_all)
    base = doc < a.n
    idx = T.GpuIndex().set_dense(x[:a.n])
    idx.set_lexical_rows(doc[base], term[base], tf[base], v, n_docs=a.n)
    q = torch.from_numpy(synth.dense_queries(a.queries, a.dim, a.n)).cuda()
    df = idx.df_local.cpu().numpy()
    qt = torch.from_numpy(synth.lexical_queries(a.queries, df, 4)).cuda()
    print(json.dumps({"n": a.n, "dim": a.dim, "shortlist": idx.shortlist, "postings": int(idx.lex["post_doc"].shape[0]),
                      "vocab": v, "step_ms_before": round(step_ms(idx, q, qt), 3)}), flush=True)
    lo = a.n
    for m in batches:
        sel = (doc >= lo) & (doc < lo + m)
        lex = (doc[sel] - lo, term[sel], tf[sel], v)
        _, wall, devt = timed(lambda: idx.append_rows(x[lo:lo + m], lex=lex))
        lo += m
        # the native calls of that append again, one by one, on the index as it now stands
        L = idx.lex
        nnz = int(L["post_doc"].shape[0])
        d_b = torch.from_numpy(doc[sel]).cuda()
        t_b, f_b = torch.from_numpy(term[sel]).cuda(), torch.from_numpy(tf[sel]).cuda()
        (rp_b, pd_b, ptf_b, _, _), _, t_build = timed(lambda: N.lexical_build(d_b, t_b, f_b, lo, v))
        out0, out1 = (torch.empty(nnz + int(pd_b.shape[0]), dtype=torch.int32, device="cuda") for _ in range(2))
        _, _, t_csr = timed(lambda: N.csr_append(L["rowptr"], L["post_doc"], L["post_tf"], rp_b, pd_b, ptf_b, out0, out1), 5)
        bounds, _, t_bounds = timed(lambda: N.bm25_bounds(L["rowptr"], L["post_doc"], L["post_tf"], L["doclen"], L["idf"],
                                                          L["avgdl"], L["k1"], L["b"]))
        _, _, t_rows = timed(lambda: N.bm25_dense_terms(L["rowptr"], L["post_doc"], L["post_tf"], bounds[2], lo,
                                                        L["dense_share"]))
        t0 = (lo - m) // 32 * 32
        _, _, t_quant = timed(lambda: N.dense_quantize_f16(idx.docs[t0:lo], keep_copy=idx.shortlist == "f16"))
        moved = (nnz + int(pd_b.shape[0])) * 8 * 2     # read + write of both payloads, A + B
        print(json.dumps({"append_rows": m, "wall_ms": round(wall, 3), "device_ms": round(devt, 3),
                          "delta_csr_build_ms": round(t_build, 3), "csr_append_ms": round(t_csr, 4),
                          "csr_append_GBps": round(moved / t_csr / 1e6, 1), "bm25_bounds_ms": round(t_bounds, 3),
                          "bm25_dense_rows_ms": round(t_rows, 3), "quantize_tail_ms": round(t_quant, 3),
                          "n_docs": idx.n_docs, "postings": nnz}), flush=True)
    print(json.dumps({"step_ms_after": round(step_ms(idx, q, qt), 3), "n_docs": idx.n_docs}), flush=True)


if __name__ == "__main__":
    main()
