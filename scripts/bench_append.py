#!/usr/bin/env python3
"""Cost of GpuIndex.append_rows on a dense + lexical index (default 1M x 768): wall and device time
of appending 1 / 256 / 16 384 chunks, the split by native call (CSR append, BM25 bounds, dense-term
rows, float16 quantisation of the tail, delta CSR build), and one retrieve_batch step before and
after.  Needs the GPU; prints one JSON line per measurement.

    python3 scripts/bench_append.py [--n 1000000] [--dim 768] [--queries 256] [--batches 1,256,16384]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=256)
    ap.add_argument("--batches", default="1,256,16384")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
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
