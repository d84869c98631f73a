#!/usr/bin/env python3
"""Parent rerank (thr_maxsim_parent_ids / thr_maxsim_parent_fp8_ids, include/thr_hip_parent.h) on one MI355X
against its same-bytes baseline, in ONE process, interleaved.

    python3 scripts/bench_parent_rerank.py [--docs 200000] [--queries 2048] [--cand 100] [--md profiles/parent_rerank.md]

A store of ``docs`` chunks of 128 x 128 tokens, far larger than the caches; per fan-out f in 1, 2, 4, 8 the chunks
are families of f consecutive rows (parent p = rows f p .. f p + f), and each query has ``cand`` candidates of
``cand`` DISTINCT random parents (one child each), so every candidate costs a whole family.  Timed, for the float16
packed store and the FP8 store:

  parent    the parent scorer over those candidates (parent column + CSR);
  concat    THE BASELINE: thr_maxsim_ids / thr_maxsim_fp8_ids over a store whose documents are the concatenated
            families -- the same image, viewed as docs / f documents of f x 128 tokens (a family's rows are
            adjacent, and the packed images are tile lists: the concatenation is the same bytes in place) -- with
            the parent numbers as candidates.  Same bytes, same flops, no column, no CSR;
  child     the parent-unaware rerank of the same candidates (one chunk each: 1 / f of the bytes), for context;
  expand    GpuIndex.maxsim(expand="parent") on a fused-list-like row: cand slots = cand / 2 parents seen through
            two children each (at f = 1: the same child twice), i.e. thr_parent_groups + the scorer over the unique
            list + the gather: half the candidates' families are read.

Rounds of ``reps`` calls each, the variants alternating inside a round, device events around each; the median round
and the fastest and slowest.  Bytes are the algorithm's (f x d_tokens x tok_dim x 2 per candidate, x (tok_dim + 4)
for FP8; 32 query tokens, so a family is read once); the share of the 8 TB/s HBM peak follows.  The scores of
parent and concat are compared bit for bit before anything is timed.  No GPU, no numbers: it fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBPS = 8000.0
Q_TOKENS, D_TOKENS, TOK_DIM = 32, 128, 128
FANOUTS = (1, 2, 4, 8)


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


def summary(ms, nbytes):
    med = statistics.median(ms)
    return {"ms": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "bytes": int(nbytes),
            "GBps": round(nbytes / med / 1e6, 1), "frac_hbm_peak": round(nbytes / med / 1e6 / HBM_PEAK_GBPS, 3)}


def run_fanout(T, idx, stores, qtok, f, nq, n_cand, rounds, reps):
    import torch
    N = T._native
    n = idx.n_docs - idx.n_docs % f
    n_par = n // f
    col = (torch.arange(idx.n_docs, device="cuda", dtype=torch.int32) // f)
    col[n:] = -1                                        # (a tail that fills no family: rows on their own)
    g = torch.Generator(device="cuda")
    g.manual_seed(100 + f)
    # cand distinct parents per query (the first cand of a random permutation's worth: sort of random keys)
    par = torch.argsort(torch.rand((nq, min(n_par, 4 * n_cand)), generator=g, device="cuda"), dim=1)[:, :n_cand] \
        + torch.randint(0, max(1, n_par - 4 * n_cand), (nq, 1), generator=g, device="cuda")
    child = par * f + torch.randint(0, f, (nq, n_cand), generator=g, device="cuda")
    two = torch.cat([par[:, :n_cand // 2] * f, par[:, :n_cand // 2] * f + (1 if f > 1 else 0)], dim=1)      # fused-list-like
    res = {"fanout": f, "parents": n_par}
    for name in ("f16", "fp8"):
        image, scales = stores[name]
        idx._install_tokens(image, scales, store=name)
        idx.set_parents(col)
        rowptr, kids = idx.parent_csr()
        per_tok = TOK_DIM * 2 if name == "f16" else TOK_DIM + 4
        if name == "f16":
            cat = image[:n].view(n_par, f * D_TOKENS, TOK_DIM)
            fns = {"parent": lambda: N.maxsim_parent_ids(qtok, image, child, 0, col, rowptr, kids),
                   "concat": lambda: N.maxsim_ids(qtok, cat, par, 0, packed=True),
                   "child": lambda: N.maxsim_ids(qtok, image, child, 0, packed=True)}
        else:
            cat, cat_s = image[:n].view(n_par, f * D_TOKENS, TOK_DIM), scales[:n].view(n_par, f * D_TOKENS)
            fns = {"parent": lambda: N.maxsim_parent_fp8_ids(qtok, image, scales, child, 0, col, rowptr, kids),
                   "concat": lambda: N.maxsim_fp8_ids(qtok, cat, cat_s, par, 0),
                   "child": lambda: N.maxsim_fp8_ids(qtok, image, scales, child, 0)}
        fns["expand"] = lambda: idx.maxsim(qtok, two, expand="parent")
        same = bool(torch.equal(fns["parent"](), fns["concat"]()))
        ms = rounds_ms(fns, rounds, reps)
        fam_bytes = nq * n_cand * f * D_TOKENS * per_tok
        r = {"parent": summary(ms["parent"], fam_bytes), "concat": summary(ms["concat"], fam_bytes),
             "child": summary(ms["child"], fam_bytes // f),
             "expand": summary(ms["expand"], fam_bytes // 2),      # cand / 2 distinct parents (at f = 1: each twice)
             "parent_equals_concat_bits": same}
        r["parent_over_concat_time"] = round(r["parent"]["ms"] / r["concat"]["ms"], 3)
        r["parent_over_child_time"] = round(r["parent"]["ms"] / r["child"]["ms"], 3)
        res[name] = r
    return res


def markdown(out):
    lines = [f"{out['docs']:,} chunks of {D_TOKENS} x {TOK_DIM} tokens, {out['queries']} queries x {out['candidates']} candidates, "
             f"{Q_TOKENS} query tokens; {out['device']}; {out['rounds']} rounds of {out['reps']} calls, variants alternating.",
             "",
             "| fan-out | store | variant | ms (median; min .. max) | bytes / call | GB/s | of 8 TB/s | parent / concat | parent / child | same bits as concat |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for r in out["fanouts"]:
        for name in ("f16", "fp8"):
            s = r[name]
            for v in ("parent", "concat", "child", "expand"):
                m = s[v]
                extra = f"{s['parent_over_concat_time']} | {s['parent_over_child_time']} | {s['parent_equals_concat_bits']}" \
                    if v == "parent" else " | | "
                lines.append(f"| {r['fanout']} | {name} | {v} | {m['ms']} ({m['ms_min']} .. {m['ms_max']}) | {m['bytes']:,} | "
                             f"{m['GBps']} | {m['frac_hbm_peak']} | {extra} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--cand", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_parent_rerank: no GPU: nothing can be measured here")
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd import synth
    N = T._native
    dtok = synth.device_tokens(0, args.docs, D_TOKENS, TOK_DIM)
    stores = {"f16": (N.maxsim_pack(dtok), None), "fp8": N.maxsim_quantize_fp8(dtok)}
    del dtok
    torch.cuda.empty_cache()
    idx = T.GpuIndex().set_dense(torch.ones((args.docs, 4), device="cuda"), shortlist="exact")
    qtok = torch.from_numpy(synth.query_tokens(args.queries, Q_TOKENS, TOK_DIM)).cuda()
    out = {"device": N.device_info()[2], "docs": args.docs, "queries": args.queries, "candidates": args.cand,
           "rounds": args.rounds, "reps": args.reps, "fanouts": []}
    for f in FANOUTS:
        out["fanouts"].append(run_fanout(T, idx, stores, qtok, f, args.queries, args.cand, args.rounds, args.reps))
    if args.md:
        with open(args.md, "w") as fh:
            fh.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
