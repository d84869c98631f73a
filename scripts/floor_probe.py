#!/usr/bin/env python3
"""A document-sharded dense step with every shard in this process, for a kernel trace:
    rocprofv3 --kernel-trace --stats -d D -o floor -- python3 scripts/floor_probe.py floor 8
    rocprofv3 --kernel-trace --stats -d D -o classic -- python3 scripts/floor_probe.py classic 8
(bench.py --full --shard-proxy times the same two loops; here only one of them runs, so the per-kernel
averages of the stats file belong to it.)"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import triple_hybrid_rag_amd as T  # noqa: E402
from triple_hybrid_rag_amd import synth  # noqa: E402
from triple_hybrid_rag_amd.distributed import shard_range  # noqa: E402


def main():
    mode, G = sys.argv[1], int(sys.argv[2])
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 1_000_000
    d, nq, k, reps = 768, 2048, 100, 10
    N = T._native
    shards = []
    for s in range(G):
        lo, hi = shard_range(n, s, G)
        ix = T.GpuIndex(doc_base=lo).set_dense(synth.dense_rows(lo, hi - lo, d))
        ix.reserve(nq, k)
        shards.append(ix)
    q = torch.from_numpy(synth.dense_queries(nq, d, n)).cuda()

    def classic():
        return [ix.dense_search(q, k, sync=False) for ix in shards]

    state = {}

    def floor():
        # a rank runs shortlist -> exchange -> finish back to back, its candidate lists still in
        # cache: here shard by shard, the finish taking the gathered bounds of the PREVIOUS
        # repetition (the same values: the inputs do not change)
        if "lbs" not in state:
            state["lbs"] = torch.stack([ix.dense_shortlist(q, k, G) for ix in shards])
        outs, lbs = [], []
        for ix in shards:
            lbs.append(ix.dense_shortlist(q, k, G))
            outs.append(ix.dense_finish(q, k, lb_all=state["lbs"]))
        state["lbs"] = torch.stack(lbs)
        return outs

    fn = floor if mode == "floor" else classic
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    print(f"{mode}: {e0.elapsed_time(e1) / reps / G:.3f} ms per shard, "
          f"{float(torch.stack([o[2] for o in out]).float().mean()):.1f} rows rescored per query and shard")


if __name__ == "__main__":
    main()
