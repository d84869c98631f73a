#!/usr/bin/env python3
"""Where the two routes of a scoped dense search cross (default 1M x 768, f16 shortlist): per scope
size, the time of one batch of queries that all name one scope of that many rows, ranked (a) over
the scope's row list (thr_dense_topk_rows), (b) through the shortlist scan with the scope labels as
doc_coll, (c) on the exhaustive float64 path with the labels (what a scope too thin for the sampled
threshold fell back to before the row lists existed).  The three return the same bits (checked).
Needs the GPU; prints one JSON line per measurement.  GpuIndex.SCOPE_ROWS_MAX is read off this table.

    python3 scripts/bench_scope.py [--n 1000000] [--dim 768] [--queries 16,256] [--sizes 1024,...,262144]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import triple_hybrid_rag_amd as T   # noqa: E402
from triple_hybrid_rag_amd import _native as N, synth   # noqa: E402


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", default="16,256")
    ap.add_argument("--sizes", default="1024,4096,16384,65536,262144")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    n = a.n
    idx = T.GpuIndex().set_dense(synth.dense_rows(0, n, a.dim))
    rng = np.random.default_rng(0)
    for size in [int(s) for s in a.sizes.split(",") if int(s) <= n]:
        tenant = np.zeros(n, dtype=np.int32)
        tenant[rng.choice(n, size, replace=False)] = 1
        idx.set_attributes({"tenant": tenant})
        for nq in [int(s) for s in a.queries.split(",")]:
            q = torch.from_numpy(synth.dense_queries(nq, a.dim, n)).cuda()
            plan = idx.scope_plan([{"tenant": 1}] * nq, nq)     # (resolved once: the routes alone are timed)
            qc = torch.zeros(nq, dtype=torch.int32, device="cuda")
            rows, t_rows = device_ms(lambda: idx.dense_search(q, a.k, scopes=plan, scope_rows_max=n, sync=False), a.reps)
            scan, t_scan = device_ms(lambda: idx.dense_search(q, a.k, scopes=plan, scope_rows_max=0, sync=False), a.reps)
            full, t_full = device_ms(lambda: N.dense_topk_exact(idx.docs, idx.dnorm, q, a.k, 0, plan.labels[0], qc), 1)
            _, t_plan = device_ms(lambda: idx.scope_plan([{"tenant": 1}] * nq, nq), a.reps)
            same = all(torch.equal(rows[j], scan[j]) and torch.equal(rows[j], full[j]) for j in range(3))
            print(json.dumps(dict(scope_rows=size, queries=nq, k=a.k, rows_ms=round(t_rows, 3), scan_ms=round(t_scan, 3),
                                  exhaustive_ms=round(t_full, 3), resolve_ms=round(t_plan, 3),
                                  rescued_by_scan=int(scan[3]), same_bits=same)), flush=True)


if __name__ == "__main__":
    main()
