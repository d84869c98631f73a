#!/usr/bin/env python3
"""Diversified top-k (thr_mmr_select, include/thr_hip_diversify.h) on one MI355X, in ONE process, seeded inputs,
the variants alternating inside every round.

    python3 scripts/bench_diversify.py [--docs 1000000] [--dims 768,1024] [--queries 2048] [--cand 100] [--top-k 10]
                                       [--md profiles/diversify_table.md]

Per row length: an index of ``docs`` synthetic rows (triple_hybrid_rag_amd.synth, the benchmark's corpus) and
``queries`` queries; the candidates of a query are its exact dense top ``cand`` (what the fusion of a dense-only
step hands on: near neighbours, best first).  Timed:

  mmr        thr_mmr_select alone over those lists (top_k, lam 0.5);
  step       GpuIndex.retrieve_batch(top_k) as the benchmark's flagship step runs it (dense only);
  step100    the same step asked for ``cand`` results: what the diversified step fuses before it selects;
  step+mmr   GpuIndex.retrieve_batch(top_k, diversify=0.5);
  torch      THE YARDSTICK FOR TIME ONLY, what a user would write today on the device: gather the candidates' rows,
             float64, divide by the norms, a bmm Gram matrix, then a top_k-step loop of torch calls (value, argmax,
             fold the picked column into the penalty).  It does not give the contract's bits (a GEMM's sum order);
             how many of its selections equal the kernel's is reported.

Rounds of ``reps`` calls each, device events around each group; the median round with the fastest and slowest.
"requested bytes" of mmr are what the kernel asks of the memory system -- (steps - 1) x m x dim x 4 for the
candidates' rows re-read every step plus steps x dim x 4 for the selected rows, per query -- most of which a query's
workgroup finds in cache after its first step; they are not HBM traffic.  No GPU, no numbers: it fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def rounds_ms(fns, rounds, reps):
    """{name: [ms per call, one per round]}: each round times ``reps`` calls of each fn in turn."""
    import torch
    for fn in fns.values():     # warm-up: code objects, allocator
        fn()
        fn()
    torch.cuda.synchronize()
    out = {name: [] for name in fns}
    for _ in range(rounds):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps)
    return out


def summary(ms):
    return {"ms": round(statistics.median(ms), 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4)}


def torch_mmr(docs, dnorm, ids, scores, counts, id_base, top_k, lam):
    """The yardstick: MMR with stock torch calls, everything on the device, no read-back.  -> ids [nq, top_k]."""
    import torch
    nq, n = ids.shape
    live = torch.arange(n, device=ids.device)[None, :] < counts[:, None]
    row = torch.where(live, ids - id_base, torch.zeros_like(ids))
    R = docs[row].to(torch.float64) / dnorm[row][:, :, None]
    G = torch.bmm(R, R.transpose(1, 2))
    s = torch.where(live, scores, torch.full_like(scores, float("inf")))
    lo = s.min(dim=1, keepdim=True).values
    hi = torch.where(live, scores, torch.full_like(scores, float("-inf"))).max(dim=1, keepdim=True).values
    rel = torch.where(hi == lo, torch.ones_like(scores), (scores - lo) / (hi - lo))
    open_ = live.clone()
    pen = torch.full_like(scores, float("-inf"))
    out = torch.full((nq, top_k), -1, dtype=torch.int64, device=ids.device)
    qs = torch.arange(nq, device=ids.device)
    neg = torch.full_like(scores, float("-inf"))
    for t in range(top_k):
        value = lam * rel if t == 0 else lam * rel - (1.0 - lam) * pen
        best = torch.where(open_, value, neg).argmax(dim=1)
        out[:, t] = ids[qs, best]
        open_[qs, best] = False
        pen = torch.maximum(pen, G[qs, :, best])
    return out


def run_dim(T, dim, args):
    import torch
    from triple_hybrid_rag_amd import synth
    N = T._native
    idx = T.GpuIndex().set_dense(synth.dense_rows(0, args.docs, dim))
    q = torch.from_numpy(synth.dense_queries(args.queries, dim, args.docs)).cuda()
    sc, ids, cnt, _ = idx.dense_search(q, args.cand)
    ids, sc, cnt = ids.contiguous(), sc.contiguous(), cnt.contiguous()
    lam, top_k = 0.5, args.top_k
    got = N.mmr_select(ids, sc, cnt, idx.docs, idx.dnorm, idx.doc_base, top_k, lam)
    ref = torch_mmr(idx.docs, idx.dnorm, ids, sc, cnt, idx.doc_base, top_k, lam)
    same_lists = float((got[0] == ref).all(dim=1).double().mean())
    same_picks = float((got[0] == ref).double().mean())
    plain = idx.retrieve_batch(q, top_k=top_k).ids
    div = idx.retrieve_batch(q, top_k=top_k, diversify=lam).ids
    fns = {"mmr": lambda: N.mmr_select(ids, sc, cnt, idx.docs, idx.dnorm, idx.doc_base, top_k, lam),
           "step": lambda: idx.retrieve_batch(q, top_k=top_k),
           "step100": lambda: idx.retrieve_batch(q, top_k=args.cand),
           "step+mmr": lambda: idx.retrieve_batch(q, top_k=top_k, diversify=lam),
           "torch": lambda: torch_mmr(idx.docs, idx.dnorm, ids, sc, cnt, idx.doc_base, top_k, lam)}
    ms = rounds_ms(fns, args.rounds, args.reps)
    res = {name: summary(v) for name, v in ms.items()}
    m = int(cnt.min())
    steps = min(m, top_k)
    requested = args.queries * ((steps - 1) * args.cand * dim * 4 + steps * dim * 4)
    res.update(dim=dim, shortlist=idx.shortlist if hasattr(idx, "shortlist") else None, candidates_min=m,
               mmr_requested_bytes=requested, mmr_requested_GBps=round(requested / res["mmr"]["ms"] / 1e6, 1),
               mmr_fma=args.queries * (steps - 1) * args.cand * dim,
               torch_over_mmr_time=round(res["torch"]["ms"] / res["mmr"]["ms"], 2),
               step_mmr_minus_step_ms=round(res["step+mmr"]["ms"] - res["step"]["ms"], 4),
               step_mmr_minus_step100_ms=round(res["step+mmr"]["ms"] - res["step100"]["ms"], 4),
               torch_lists_equal_to_kernel=round(same_lists, 4), torch_picks_equal_to_kernel=round(same_picks, 4),
               queries_whose_top_k_changed=round(float((plain != div).any(dim=1).double().mean()), 4))
    del idx, q
    torch.cuda.empty_cache()
    return res


def markdown(out):
    lines = [f"{out['docs']:,} rows, {out['queries']} queries x {out['candidates']} candidates, top_k {out['top_k']}, lam 0.5; "
             f"{out['device']}; {out['rounds']} rounds of {out['reps']} calls, variants alternating.", "",
             "| dim | variant | ms (median; min .. max) |", "|---|---|---|"]
    for r in out["dims"]:
        for v in ("mmr", "torch", "step", "step100", "step+mmr"):
            m = r[v]
            lines.append(f"| {r['dim']} | {v} | {m['ms']} ({m['ms_min']} .. {m['ms_max']}) |")
    lines += ["", "| dim | torch / mmr time | step+mmr - step (ms) | step+mmr - step100 (ms) | mmr requested bytes | requested GB/s | "
              "torch lists = kernel's | torch picks = kernel's | queries whose top_k changed |", "|---|---|---|---|---|---|---|---|---|"]
    for r in out["dims"]:
        lines.append(f"| {r['dim']} | {r['torch_over_mmr_time']} | {r['step_mmr_minus_step_ms']} | {r['step_mmr_minus_step100_ms']} | "
                     f"{r['mmr_requested_bytes']:,} | {r['mmr_requested_GBps']} | {r['torch_lists_equal_to_kernel']} | "
                     f"{r['torch_picks_equal_to_kernel']} | {r['queries_whose_top_k_changed']} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--dims", default="768,1024")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--cand", type=int, default=100)
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_diversify: no GPU: nothing can be measured here")
    import triple_hybrid_rag_amd as T
    out = {"device": T._native.device_info()[2], "docs": args.docs, "queries": args.queries, "candidates": args.cand,
           "top_k": args.top_k, "rounds": args.rounds, "reps": args.reps, "dims": []}
    for dim in (int(d) for d in args.dims.split(",")):
        out["dims"].append(run_dim(T, dim, args))
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
