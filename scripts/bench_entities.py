#!/usr/bin/env python3
"""Seed entities of a batch from its keywords: the device batch (GpuIndex.find_entities, one
thr_entity_match call) against the only way to seed that batch before it, the loop of host
GpuIndexClient.find_entities calls, on the same inputs.

    python scripts/bench_entities.py [--sizes 250000,2500000] [--queries 2048] [--out profiles/entity_match.md]

Inputs are seeded: names of two or three pseudo-words drawn (Zipf) from a vocabulary of syllable words --
not ``entity{e}``, whose names all share one trigram; three keywords per query: mostly whole words and
word fragments (the frequent ones match thousands of names), a few of one or two bytes, a few nobody
matches.  Per size:

  device ms   thr_entity_match alone, the needle tables already uploaded: warm-up calls, then --rounds
              rounds of --reps calls between two device events, the MEDIAN round (min and max are given);
              once for the whole batch and once for its first eighth -- an eighth of the needles over the
              same store: the pass is meant to cost the store, not the needle count;
  call ms     GpuIndex.find_entities as a caller sees it (lowering, de-duplication, upload, kernel), a host
              clock around calls that end in a synchronise, median;
  host s      wall time of [client.find_entities(k) for k in lists], the trigram index built beforehand (it
              is set-up on that side as the upload is on this).  When the loop would take longer than
              --host-budget seconds it is stopped after the queries done so far and scaled to the batch;
              the output says so.

The device answer is compared with the host's on every query the host loop got through."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SYLLABLES = ("ba be bi bo bu ca ce ci co cu da de di do du fa fe fi fo ga go la le li lo lu ma me mi mo mu na ne ni no "
             "pa pe pi po ra re ri ro ru sa se si so su ta te ti to tu va ve vi vo xa ze zi ção nha lha rra").split()


def make_inputs(n_names, n_queries, seed):
    rng = np.random.default_rng(seed)
    vocab = sorted({"".join(rng.choice(SYLLABLES, size=int(rng.integers(2, 5)))) for _ in range(30_000)})
    p = 1.0 / np.arange(1, len(vocab) + 1) ** 0.9
    p /= p.sum()
    words = rng.choice(len(vocab), size=(n_names, 3), p=p)
    three = rng.random(n_names) < 0.4
    names = [f"{vocab[a]} {vocab[b]} {vocab[c]}".title() if t else f"{vocab[a]} {vocab[b]}".title()
             for (a, b, c), t in zip(words.tolist(), three.tolist())]
    lists = []
    for _ in range(n_queries):
        kws = []
        for _ in range(3):
            u = rng.random()
            w = vocab[int(rng.choice(len(vocab), p=p))]
            if u < 0.03:
                kws.append(w[:int(rng.integers(1, 3))])                 # one or two bytes
            elif u < 0.08:
                kws.append(w + "qq")                                    # nobody matches
            elif u < 0.5:
                kws.append(w[int(rng.integers(0, 2)):][:int(rng.integers(3, 7))].upper())   # a fragment
            else:
                kws.append(w)
        lists.append(kws)
    return names, lists


def event_rounds(fn, rounds, reps):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="250000,2500000")
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-budget", type=float, default=60.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_entities needs the GPU: nothing is measured without one")
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
    from triple_hybrid_rag_amd.index_entities import plan_needles
    N = T._native
    N.load()
    lines = []
    for n_names in [int(s) for s in args.sizes.split(",")]:
        names, lists = make_inputs(n_names, args.queries, seed=n_names)
        store = CorpusStore.synthetic(4)
        store.entity_names = names
        idx = T.GpuIndex()
        t0 = time.perf_counter()
        idx.set_entity_names(names)
        torch.cuda.synchronize()
        setup_dev = time.perf_counter() - t0

        class Client(GpuIndexClient):       # (the host function needs the store alone)
            def __init__(self):
                self.store, self.index = store, idx
        client = Client()
        Ent = idx.entities
        store_bytes = int(Ent["name_bytes"].numel())

        def device_ms(sub):
            plan = plan_needles(sub, 20)
            tabs = [idx._t(a, dt) for a, dt in ((plan.needles, torch.uint8), (plan.needle_len, torch.int32),
                                                (plan.query_needles, torch.int32), (plan.query_per, torch.int32))]
            need = N.entity_match_workspace_bytes(Ent["n"], plan.needles.shape[0], len(sub))
            ws = torch.empty(need, dtype=torch.uint8, device=idx.device)
            call = lambda: N.entity_match(Ent["name_bytes"], Ent["name_ptr"], *tabs, workspace=ws)
            for _ in range(3):
                call()
            torch.cuda.synchronize()
            r = event_rounds(call, args.rounds, args.reps)
            return statistics.median(r), min(r), max(r), plan.needles.shape[0]
        full = device_ms(lists)
        eighth = device_ms(lists[:max(1, args.queries // 8)])
        walls = []
        for _ in range(5):
            t0 = time.perf_counter()
            seeds, counts = idx.find_entities(lists)
            torch.cuda.synchronize()
            walls.append((time.perf_counter() - t0) * 1e3)
        got = [row[:c].tolist() for row, c in zip(seeds.cpu().numpy(), counts.cpu().numpy())]

        t0 = time.perf_counter()
        client._entity_index()
        setup_host = time.perf_counter() - t0
        host, t0 = [], time.perf_counter()
        for kws in lists:
            host.append(client.find_entities(kws))
            if time.perf_counter() - t0 > args.host_budget:
                break
        host_s = time.perf_counter() - t0
        if got[:len(host)] != host:
            bad = next(q for q in range(len(host)) if got[q] != host[q])
            sys.exit(f"{n_names} names: query {bad} {lists[bad]}: device {got[bad]} != host {host[bad]}")
        scaled = host_s * len(lists) / len(host)
        how = "whole batch" if len(host) == len(lists) else f"first {len(host)} queries, scaled to {len(lists)}"
        lines += [
            f"### {n_names:,} names ({store_bytes / 1e6:.1f} MB of name bytes), {len(lists)} queries of 3 keywords, "
            f"{full[3]} distinct needles",
            "",
            f"- device, thr_entity_match alone: **{full[0]:.3f} ms** per batch (median of {args.rounds} rounds of "
            f"{args.reps} calls; min {full[1]:.3f}, max {full[2]:.3f}) = {store_bytes / full[0] / 1e6:.1f} GB/s of name bytes",
            f"- device, the first {max(1, args.queries // 8)} queries ({eighth[3]} needles) over the same store: "
            f"{eighth[0]:.3f} ms (min {eighth[1]:.3f}, max {eighth[2]:.3f})",
            f"- GpuIndex.find_entities as called (host planning + upload + kernel + synchronise): "
            f"{statistics.median(walls):.2f} ms (median of 5)",
            f"- host loop of GpuIndexClient.find_entities: **{scaled:.2f} s** per batch ({how}; measured {host_s:.2f} s)",
            f"- ratio host loop / device kernel: {scaled * 1e3 / full[0]:,.0f}x; host loop / find_entities call: "
            f"{scaled * 1e3 / statistics.median(walls):,.0f}x",
            f"- set-up, not in the above: upload of the packed names {setup_dev:.2f} s, host trigram index {setup_host:.2f} s",
            f"- the device answer equals the host's on the {len(host)} queries the host loop got through",
            ""]
        print("\n".join(lines[-10:]), flush=True)
        del idx, client, store, names
        torch.cuda.empty_cache()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Entity lookup for a batch: device pass against the host loop\n\n"
                    f"`python scripts/bench_entities.py --sizes {args.sizes} --queries {args.queries}` on "
                    f"{torch.cuda.get_device_name(0)}, {time.strftime('%Y-%m-%d')}.\n\n" + "\n".join(lines))


if __name__ == "__main__":
    main()
