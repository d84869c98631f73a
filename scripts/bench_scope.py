#!/usr/bin/env python3
"""Where the two routes of a scoped dense search cross (default 1M x 768, f16 shortlist): per scope
size, the time of one batch of queries that all name one scope of that many rows, ranked (a) over
the scope's row list (thr_dense_topk_rows), (b) through the shortlist scan with the scope labels as
doc_coll, (c) on the exhaustive float64 path with the labels (what a scope too thin for the sampled
threshold fell back to before the row lists existed).  The three return the same bits (checked).
Needs the GPU; prints one JSON line per measurement.  GpuIndex.SCOPE_ROWS_MAX is read off this table.

    python3 scripts/bench_scope.py [--n 1000000] [--dim 768] [--queries 16,256] [--sizes 1024,...,262144]

--graph times the graph channel instead: graph_search of one batch (default 2048 queries, 1M chunks,
k 50, 2 hops) unscoped, with every query in a tenant that holds 1/4 of the rows, and with every query in
one that holds 1/256 -- device milliseconds per call, wrappers included, scopes resolved beforehand
(a ScopePlan).  The three are timed in alternation, ``--rounds`` times after a warm-up of every shape;
the line gives the median and the range of the rounds, and what the thin tenant's lists hold.

    python3 scripts/bench_scope.py --graph [--n 1000000] [--graph-queries 2048] [--rounds 7] [--reps 200]

--graph --unscoped-only times the unscoped call alone and uses nothing this change added: copied into a
checkout of an earlier commit, it gives that commit's figure with the same timing code.
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


def graph_bench(a, scoped=True):
    """One JSON line: graph_search per call, unscoped and (``scoped``) inside a wide and a thin tenant."""
    n, nq, k, hops = a.n, a.graph_queries, 50, 2
    g = synth.build_graph(n)
    idx = T.GpuIndex()
    idx.n_docs = n
    idx.set_graph(g.ent_rowptr, g.ent_col, g.men_rowptr, g.men_chunk, g.men_conf)
    seeds = torch.from_numpy(synth.graph_queries(nq, n, 3)).cuda()
    runs = {"unscoped": lambda: idx.graph_search(seeds, k, hops)}
    if scoped:
        org = np.zeros(n, dtype=np.int32)
        org[np.arange(n) % 4 == 1] = 1           # a quarter of the rows
        org[np.arange(n) % 256 == 2] = 2         # 1/256 of them
        idx.set_attributes({"org": org})
        quarter, thin = (idx.scope_plan([{"org": o}] * nq, nq) for o in (1, 2))
        runs["quarter"] = lambda: idx.graph_search(seeds, k, hops, scopes=quarter)
        runs["thin"] = lambda: idx.graph_search(seeds, k, hops, scopes=thin)
    for fn in runs.values():                     # warm-up: every shape, the transposed CSR, the workspace
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, fn in runs.items():
            ms[name].append(device_ms(fn, a.reps)[1])
    out = dict(bench="graph_scope", chunks=n, entities=int(len(g.ent_rowptr) - 1), mentions=int(len(g.men_chunk)),
               queries=nq, k=k, hops=hops, rounds=a.rounds, reps=a.reps)
    for name, v in ms.items():
        out[name + "_ms"] = dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))
    if scoped:
        S, I, cnt = runs["thin"]()
        ids = I[I >= 0]
        out["thin_in_scope"] = bool((torch.from_numpy(org).cuda()[ids] == 2).all())
        out["thin_mean_count"] = round(float(cnt.float().mean()), 2)
        out["unscoped_mean_count"] = round(float(runs["unscoped"]()[2].float().mean()), 2)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graph", action="store_true", help="time the graph channel, unscoped and scoped")
    ap.add_argument("--unscoped-only", action="store_true", help="with --graph: the unscoped call alone")
    ap.add_argument("--graph-queries", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--queries", default="16,256")
    ap.add_argument("--sizes", default="1024,4096,16384,65536,262144")
    ap.add_argument("--reps", type=int, default=None, help="calls per timing (default 5; --graph: 200)")
    a = ap.parse_args()
    if a.graph:
        a.reps = a.reps or 200      # (0.2 ms a call: 40 ms per timing window)
        return graph_bench(a, scoped=not a.unscoped_only)
    a.reps = a.reps or 5
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
