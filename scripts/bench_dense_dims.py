#!/usr/bin/env python3
"""Dense search by row length: shortlist="f16-anydim" (the runtime-dim f16 scan) against what the index
ran at those lengths before it -- shortlist="exact", every row scored in float64 -- and, at 768 and
1024, against the tuned "f16-inline" kernel.

    python scripts/bench_dense_dims.py [--rows 1000000] [--queries 2048] [--k 100] [--dims 384,1536,...]
                                       [--out profiles/dense_anydim.json]

Per (dim, flavour): warm-up calls of the very shape (never timed), then dense_search calls between two
device events -- as many as fill about --window seconds, at least one.  "exact" gets the full batch when one call fits
--exact-budget seconds, else the largest power-of-two part of it that does -- stated in the output,
with the rate per query so the two can be compared.  The scan's own time is the filter-scan launch
alone (GpuIndex.scan_probe, same thresholds), timed the same way; its share, its f16 FLOP/s
(2 n dim nq) against the 2.5 PF dense peak and the bytes it must read at least once (4 n dim) against
8 TB/s are derived from it.  The rows shrink until the float32 corpus is under a quarter of the
device's memory.  Results are checked: both flavours must return the same ids for the first queries."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F16_PEAK = 2.5e15     # dense f16 matrix peak, FLOP/s (spec)
HBM_PEAK = 8.0e12     # bytes/s (spec)


def event_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def timed(fn, window_s, warm=1):
    """-> (ms per call, calls timed).  The first call (allocations, code objects) is never timed; when it
    alone takes longer than the window, one more call is the measurement (it is long enough to be one),
    else `warm` calls in all warm up and the window is filled."""
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    first = time.perf_counter() - t0
    if first > window_s:
        return event_ms(fn, 1), 1
    for _ in range(warm - 1):
        fn()
    one = event_ms(fn, 1)
    reps = max(1, min(20, int(window_s * 1e3 / max(one, 1e-3))))
    return (event_ms(fn, reps), reps) if reps > 1 else (one, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--k", type=int, default=100)
    ap.add_argument("--dims", default="384,1536,2048,4000,4096,768,1024")
    ap.add_argument("--window", type=float, default=2.0, help="seconds of timed work per measurement")
    ap.add_argument("--exact-budget", type=float, default=20.0, help="seconds one 'exact' call may take")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_dense_dims needs the GPU: nothing is measured without one")
    import triple_hybrid_rag_amd as T
    N = T._native
    N.load()
    total_mem = torch.cuda.get_device_properties(0).total_memory
    results = []
    for dim in [int(d) for d in args.dims.split(",")]:
        n = min(args.rows, int(0.25 * total_mem / (4 * dim)))
        g = torch.Generator(device="cuda").manual_seed(dim)
        x = torch.randn((n, dim), generator=g, device="cuda", dtype=torch.float32)
        x /= x.norm(dim=1, keepdim=True)
        q = torch.randn((args.queries, dim), generator=g, device="cuda", dtype=torch.float32)
        q[::2] = x[torch.randint(0, n, (len(q[::2]),), generator=g, device="cuda")] + 0.5 * q[::2]
        row = {"dim": dim, "rows": n, "queries": args.queries, "k": args.k}
        idx = T.GpuIndex().set_dense(x, shortlist="f16-anydim")
        idx.reserve(args.queries, args.k)
        ms, reps = timed(lambda: idx.dense_search(q, args.k, sync=False), args.window, warm=2)
        S, I, cnt, nres = idx.dense_search(q, args.k)
        scan_ms = event_ms(lambda: idx.scan_probe(q), max(1, reps))
        tile = N.dense_f16_query_tile(dim, False, args.queries)
        row["f16-anydim"] = {
            "ms": ms, "calls_timed": reps, "queries_per_s": args.queries / ms * 1e3, "rescued": int(nres),
            "query_tile": tile, "tile_passes": -(-args.queries // tile), "scan_ms": scan_ms,
            "scan_share": scan_ms / ms, "scan_f16_flops": 2.0 * n * dim * args.queries / (scan_ms * 1e-3),
            "scan_share_of_f16_peak": 2.0 * n * dim * args.queries / (scan_ms * 1e-3) / F16_PEAK,
            "scan_min_bytes_per_s": 4.0 * n * dim / (scan_ms * 1e-3),
            "scan_share_of_hbm_peak": 4.0 * n * dim / (scan_ms * 1e-3) / HBM_PEAK}
        other = "f16-inline" if dim in T.GpuIndex.F16_DIMS else "exact"
        ref = T.GpuIndex().set_dense(x, shortlist=other)
        nq_ref = args.queries
        if other == "exact":
            # one call of a small batch sizes the full one (the exhaustive path is linear in the batch)
            probe = min(64, args.queries)
            ref.dense_search(q[:probe], args.k)
            t = event_ms(lambda: ref.dense_search(q[:probe], args.k, sync=False), 1) * 1e-3 / probe
            while nq_ref > probe and t * nq_ref > args.exact_budget:
                nq_ref //= 2
        else:
            ref.reserve(args.queries, args.k)
        ms_r, reps_r = timed(lambda: ref.dense_search(q[:nq_ref], args.k, sync=False), args.window,
                             warm=1 if other == "exact" else 2)
        Sr, Ir, cr, _ = ref.dense_search(q[:min(nq_ref, 256)], args.k)
        same = bool(torch.equal(Ir, I[:Ir.shape[0]]) and torch.equal(Sr, S[:Sr.shape[0]]))
        row[other] = {"ms": ms_r, "calls_timed": reps_r, "queries": nq_ref, "full_batch": nq_ref == args.queries,
                      "queries_per_s": nq_ref / ms_r * 1e3}
        row["same_results"] = same
        row["speedup_per_query"] = row["f16-anydim"]["queries_per_s"] / row[other]["queries_per_s"]
        print(json.dumps(row), flush=True)
        results.append(row)
        if not same:
            sys.exit(f"dim {dim}: f16-anydim and {other} disagree")
        del idx, ref, x, q
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "when": time.strftime("%Y-%m-%d"),
                       "results": results}, f, indent=1)


if __name__ == "__main__":
    main()
