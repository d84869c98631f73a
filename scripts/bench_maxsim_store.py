#!/usr/bin/env python3
"""MaxSim rerank over the two token stores on one MI355X: the packed float16 store (thr_maxsim) against
the FP8 store (thr_maxsim_fp8, include/thr_hip_rerank.h), in ONE process, interleaved.

    python3 scripts/bench_maxsim_store.py [--docs 200000] [--queries 2048] [--cand 100] [--md report.md]

For each shape (128 x 128 and 128 x 256 document tokens; 32 query tokens) over a store far larger than
the caches (random candidates: a document is met again only after gigabytes of others):
  * ms per call of both kernels -- rounds of ``reps`` calls each, alternating f16 / fp8, timed with device
    events; the median round, and the fastest and slowest, so the spread is on the page;
  * algorithmic bytes per call (d_tokens * tok_dim * 2 per candidate for float16, d_tokens * (tok_dim + 4)
    for FP8) and the resulting share of the 8 TB/s HBM peak -- the bound of both kernels (their flops would
    take a tenth of the time on the f16 matrix cores);
  * device memory of both stores;
  * quantiser throughput (thr_maxsim_quantize_fp8 over the whole store);
  * ranking agreement on the synth tokens: max |score difference| of the FP8 kernel against the float64
    MaxSim over the FLOAT16 store (so it includes the quantisation error), and the share of queries whose
    top-10 after the rerank -- ids and order -- is the float16 store's.  Two query sets: the synth queries
    (unrelated to the documents: scores crowd together) and PLANTED queries, whose tokens are noisy copies of
    tokens of ten of their candidates at ten noise levels (scores spread, as relevant chunks' do); with them
    the share of queries with the same top-1 and the widest float64 gap between two candidates that the FP8
    scores rank the other way round.
Prints one JSON object; --md also writes the table as markdown.  No GPU, no numbers: it fails."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_PEAK_GBPS = 8000.0
Q_TOKENS = 32


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


def reference_f64(qtok, dtok, cand):
    """float64 MaxSim over the float16 tokens, on the device (a check, not a hot path) -> [nq, n_cand]."""
    import torch
    out = torch.empty(cand.shape, dtype=torch.float64, device=qtok.device)
    for i in range(qtok.shape[0]):
        d = dtok[cand[i].long()].double()                     # [n_cand, d_tokens, tok_dim]
        s = torch.einsum("ik,cjk->cij", qtok[i].double(), d)  # [n_cand, q_tokens, d_tokens]
        out[i] = s.max(dim=2).values.sum(dim=1)
    return out


def top10(scores):
    import torch
    return torch.argsort(scores, dim=1, descending=True, stable=True)[:, :10]


def swapped_gap(ref, got):
    """The largest float64 score gap between two of a query's candidates that ``got`` ranks the other way
    round: how far apart two chunks can be and still change places."""
    d_ref = ref[:, :, None] - ref[:, None, :]
    d_got = got[:, :, None] - got[:, None, :]
    bad = (d_ref > 0) & (d_got < 0)
    return float(torch_max(d_ref[bad]))


def torch_max(t):
    return t.max() if t.numel() else 0.0


def planted_queries(dtok, cand):
    """Query tokens that are noisy copies of tokens of the query's first ten candidates: token i copies token i
    of candidate i % 10 with noise that grows with the candidate (cosine ~0.96 for candidate 0 down to ~0.37
    for candidate 9), so ten candidates stand out of the crowd by different margins."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(4242)
    nq, td = cand.shape[0], dtok.shape[2]
    q = torch.empty((nq, Q_TOKENS, td), dtype=torch.float32, device="cuda")
    for i in range(Q_TOKENS):
        j = i % 10
        src = dtok[cand[:, j].long(), i].float()
        q[:, i] = src + (0.3 + 0.25 * j) * torch.randn(src.shape, generator=g, device="cuda") / td ** 0.5
    return torch.nn.functional.normalize(q, dim=2).to(torch.float16)


def run_shape(T, synth, n_docs, d_tokens, tok_dim, nq, n_cand, rounds, reps, n_check):
    import torch
    N = T._native
    dtok = synth.device_tokens(0, n_docs, d_tokens, tok_dim)
    f16 = N.maxsim_pack(dtok)
    # quantiser: the whole store, out of place
    torch.cuda.synchronize()
    quant = rounds_ms({"q": lambda: N.maxsim_quantize_fp8(dtok)}, 3, 1)["q"]
    codes, scales = N.maxsim_quantize_fp8(dtok)
    g = torch.Generator(device="cuda")
    g.manual_seed(99)
    cand = torch.randint(0, n_docs, (nq, n_cand), device="cuda", dtype=torch.int32, generator=g)
    qtok = torch.from_numpy(synth.query_tokens(nq, Q_TOKENS, tok_dim)).cuda()
    ms = rounds_ms({"f16": lambda: N.maxsim(qtok, f16, cand, packed=True),
                    "fp8": lambda: N.maxsim_fp8(qtok, codes, scales, cand)}, rounds, reps)
    by = {"f16": nq * n_cand * d_tokens * tok_dim * 2, "fp8": nq * n_cand * d_tokens * (tok_dim + 4)}
    res = {"d_tokens": d_tokens, "tok_dim": tok_dim, "docs": n_docs, "queries": nq, "candidates": n_cand,
           "gflop": round(2.0 * nq * n_cand * Q_TOKENS * d_tokens * tok_dim / 1e9, 1)}
    for k in ("f16", "fp8"):
        med = statistics.median(ms[k])
        res[k] = {"ms": round(med, 4), "ms_min": round(min(ms[k]), 4), "ms_max": round(max(ms[k]), 4),
                  "bytes": by[k], "GBps": round(by[k] / med / 1e6, 1),
                  "frac_hbm_peak": round(by[k] / med / 1e6 / HBM_PEAK_GBPS, 3)}
    res["fp8_over_f16_time"] = round(res["fp8"]["ms"] / res["f16"]["ms"], 3)
    res["store_bytes"] = {"f16": f16.numel() * 2, "fp8": codes.numel() + scales.numel() * 4}
    qms = statistics.median(quant)
    res["quantiser"] = {"ms": round(qms, 3), "tokens_per_s": round(n_docs * d_tokens / qms * 1e3),
                        "GBps_read_plus_written": round((dtok.numel() * 3 + scales.numel() * 4) / qms / 1e6, 1)}
    # ranking agreement on the first n_check queries, both query sets
    agree = {}
    for name, qs in (("synth", qtok[:n_check]), ("planted", planted_queries(dtok, cand[:n_check]))):
        c = cand[:n_check]
        ref = reference_f64(qs, dtok, c)
        s16 = N.maxsim(qs, f16, c, packed=True).double()
        s8 = N.maxsim_fp8(qs, codes, scales, c).double()
        r10 = top10(ref)
        agree[name] = {"queries": int(n_check), "score_min": round(float(ref.min()), 3), "score_max": round(float(ref.max()), 3),
                       "max_abs_diff_fp8": float((s8 - ref).abs().max()), "max_abs_diff_f16": float((s16 - ref).abs().max()),
                       "top10_same_fp8": round(float((top10(s8) == r10).all(dim=1).double().mean()), 4),
                       "top10_same_f16": round(float((top10(s16) == r10).all(dim=1).double().mean()), 4),
                       "top1_same_fp8": round(float((top10(s8)[:, 0] == r10[:, 0]).double().mean()), 4),
                       "swapped_pairs_max_gap_fp8": swapped_gap(ref, s8),
                       "top10_same_set_fp8": round(float(torch.tensor(
                           [set(a.tolist()) == set(b.tolist()) for a, b in zip(top10(s8), r10)]).double().mean()), 4),
                       "top1_gap_median": round(float((torch.sort(ref, dim=1, descending=True).values[:, 0]
                                                       - torch.sort(ref, dim=1, descending=True).values[:, 1]).median()), 4)}
    res["agreement"] = agree
    return res


def markdown(out):
    lines = ["| shape (d_tokens x tok_dim) | store | ms (median; min .. max) | bytes / call | GB/s | of 8 TB/s | store bytes |",
             "|---|---|---|---|---|---|---|"]
    for r in out["shapes"]:
        for k in ("f16", "fp8"):
            m = r[k]
            lines.append(f"| {r['d_tokens']} x {r['tok_dim']} | {k} | {m['ms']} ({m['ms_min']} .. {m['ms_max']}) | {m['bytes']:,} | "
                         f"{m['GBps']} | {m['frac_hbm_peak']} | {r['store_bytes'][k]:,} |")
    lines += ["", "| shape | fp8 / f16 time | quantiser ms (whole store) | tokens / s | GB/s read + written |", "|---|---|---|---|---|"]
    for r in out["shapes"]:
        q = r["quantiser"]
        lines.append(f"| {r['d_tokens']} x {r['tok_dim']} | {r['fp8_over_f16_time']} | {q['ms']} | {q['tokens_per_s']:,} | {q['GBps_read_plus_written']} |")
    lines += ["", "| shape | queries | scores | max abs diff fp8 (f16) vs float64 of the f16 store | top-10 same ids and order fp8 (f16) | top-10 same set fp8 | top-1 same fp8 | widest gap that changed places | median top-1 gap |",
              "|---|---|---|---|---|---|---|---|---|"]
    for r in out["shapes"]:
        for name, a in r["agreement"].items():
            lines.append(f"| {r['d_tokens']} x {r['tok_dim']} | {name} ({a['queries']}) | {a['score_min']} .. {a['score_max']} | "
                         f"{a['max_abs_diff_fp8']:.3e} ({a['max_abs_diff_f16']:.3e}) | {a['top10_same_fp8']} ({a['top10_same_f16']}) | "
                         f"{a['top10_same_set_fp8']} | {a['top1_same_fp8']} | {a['swapped_pairs_max_gap_fp8']:.3e} | {a['top1_gap_median']} |")
    return "\n".join(lines) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=200_000)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--cand", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--check-queries", type=int, default=256)
    ap.add_argument("--shapes", default="128x128,128x256")
    ap.add_argument("--md", default=None)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_maxsim_store: no GPU: nothing can be measured here")
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd import synth
    out = {"device": T._native.device_info()[2], "rounds": args.rounds, "reps": args.reps, "shapes": []}
    for shape in args.shapes.split(","):
        dt, td = (int(v) for v in shape.split("x"))
        out["shapes"].append(run_shape(T, synth, args.docs, dt, td, args.queries, args.cand, args.rounds, args.reps,
                                       min(args.check_queries, args.queries)))
        torch.cuda.empty_cache()
    if args.md:
        with open(args.md, "w") as f:
            f.write(markdown(out))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
