#!/usr/bin/env python3
"""Headline benchmark: queries/sec for the fused top-10 of the RAG 2.0 retrieval hot path.

    python bench.py --gpus N --steps K --warmup W [--full] [--dump-outputs DIR]
                    [--config dense|dense_bm25|triple|triple_rerank|all]

A step = one pass of the hot path over one batch of ``--queries`` (default 2048) synthetic
queries, inputs resident in HBM.  The headline line is always BASELINE.json configs[1]
(1M-doc / 768-d dense-only cosine top-100 -> RRF -> fused top-10).  A plain run does what that
line needs and no more: it generates the inputs, warms up, times the K steps and prints the line.
For N > 1 the SAME corpus is sharded by document across the ranks (strong scaling, one process
per GPU, RCCL all-gather of the per-shard top-k per channel, second all-gather for the rerank
scores) and ``--config`` (default dense) is timed.

``--full`` adds everything else the benchmark measures and checks, each in runs of its own after
the headline's: at N = 1 configs[2]-[4]'s pipelines on the same corpus (``configs`` in the JSON:
dense + BM25, triple-hybrid, triple-hybrid + MaxSim rerank of the fused top-100) with a parity
sample against the oracle, each channel kernel alone (``stages_alone``), the other shortlist
flavours (``other_shortlists``) and ``--shard-proxy``; at N > 1 a rank's share of the step
(``config.per_rank_ms``) and the pure document-sharded layout (``config.strong_doc_sharded``); and
  roofline      the dominant kernel -- the dense scan -- launched alone through
                thr_dense_scan_probe_f16 and timed with HIP events on its stream: 2*N*D*Q flops
                per launch / average launch time against the dense f16 MFMA peak; ``traffic`` =
                HBM bytes per launch from the committed PMC pass (profiles/, same shape; null
                when the shape differs) and the HBM GB/s that traffic means at the measured time
  cpu_baseline  the CPU oracle's fast path (float32 BLAS shortlist + float64 rescoring,
                oracle/thr_oracle.py) timed on this host's cores on a bounded sample (rank 0, N = 1)
                and the fused top-10 of the timed path compared with it (``parity_check``)
  latency       the drop-in ``RAG2Retriever.retrieve()`` one query at a time (p50 / p95), and the
                scan alone for batches of 1 / 32 / 256 queries as HBM GB/s (one pass over the
                float16 copy: the regime where the HBM roofline applies)
``--no-extras`` and ``--no-cpu-baseline`` leave parts of a ``--full`` run out.

``--dump-outputs DIR`` writes what the LAST timed step of every timed pipeline returned (the
BatchResult of retrieve_batch: fused ids / scores / counts and every channel's list) as
``DIR/<pipeline>_<field>.npy``.  The inputs are seeded, so two builds of the library run with the
same arguments can be compared array by array.  At N = 1 without ``--config`` the arrays are those
of all four pipelines, with or without ``--full``: a plain run that dumps generates the lexical,
graph and token inputs too and gives configs[2]-[4]'s pipelines their W + K steps after the
headline's (their rates: ``configs``).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# MI355X peaks (MI355X_MICROARCH.md): HBM3E spec; dense f16 MFMA; f32-input MFMA (= f32 vector)
HBM_PEAK_GBPS = 8000.0
MFMA_F16_PEAK_TFLOPS = 2500.0
MFMA_F32_PEAK_TFLOPS = 157.3
CONFIGS = ("dense", "dense_bm25", "triple", "triple_rerank")
BASELINE_CONFIG = {"dense": "configs[1]", "dense_bm25": "configs[2]", "triple": "configs[3]",
                   "triple_rerank": "configs[4]"}
PMC_PROFILE = os.path.join(ROOT, "profiles", "r4_scan_f16qs_counters.json")
DUMP_MAX_BYTES = 64_000_000


def parse(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="after the headline's steps, also measure and check everything else: the other "
                         "pipelines, shortlist flavours and layouts, each kernel alone, the roofline, the "
                         "latency section, the CPU baseline and the parity with the oracle")
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--queries", type=int, default=2048,
                    help="queries per step (batch): 2048 = 8 workgroup tiles of 256 queries x 4 "
                         "row slices per XCD, one full round of the 256 CUs for the default scan")
    ap.add_argument("--top-k", type=int, default=10)
    ap.add_argument("--config", choices=CONFIGS + ("all",), default=None,
                    help="pipeline to time; default: dense (the headline), followed at N = 1 by the other "
                         "three when --full or --dump-outputs is given; all = the four of them")
    ap.add_argument("--preset", choices=("configs1", "configs2", "configs3", "configs4"), default=None,
                    help="a BASELINE.json config at its stated size and layout: configs1 = 1M dense-only; "
                         "configs2 = 1M dense + BM25 + RRF(0.8/0.7); configs3 = 10M triple-hybrid cut into "
                         "--gpus document shards; configs4 = the same + MaxSim rerank (sets --docs, --config "
                         "and, for the 10M-doc ones, --doc-shards N)")
    ap.add_argument("--token-docs", type=int, default=0,
                    help="docs that get a late-interaction token matrix (default: all; 32 KiB each)")
    ap.add_argument("--doc-shards", type=int, default=0,
                    help="N > 1: split the corpus into this many document shards; the N / doc-shards "
                         "groups are replicas that serve different query batches "
                         "(distributed.layout_2d).  Default 0 = auto: as many shards as keep "
                         ">= --min-shard-docs rows on a shard (the scan must dominate the per-batch "
                         "fixed work of a shard: threshold, shortlist, rescoring, exchange), so the 1M-doc "
                         "headline corpus is 2 shards x N/2 replicas and the 10M-doc configs are N shards; "
                         "--doc-shards N forces the pure document-sharded layout")
    ap.add_argument("--min-shard-docs", type=int, default=500_000)
    ap.add_argument("--shard-proxy", type=int, default=0, metavar="G",
                    help="--full at N = 1 only: also hold the --docs corpus as G document shards in THIS process and "
                         "time one shard's share of a dense step (everything but the collectives) with and "
                         "without the shard floor exchange -> config.shard_floor_proxy")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="--full without the CPU oracle's leg (cpu_baseline, parity_check, parity_sample)")
    ap.add_argument("--cpu-queries", type=int, default=2048)
    ap.add_argument("--probe-reps", type=int, default=5)
    ap.add_argument("--no-extras", "--no-f16-extra", dest="no_extras", action="store_true",
                    help="--full without the other shortlist flavours, the other configs and the latency "
                         "section; --dump-outputs without the other configs")
    ap.add_argument("--lexical-mix", choices=("survey", "no-stopwords"), default="survey",
                    help="query terms of the lexical channel: survey = 4 term ids sampled in proportion to "
                         "df (SURVEY 8d: stop words included, ~0.5M postings per query at 1M docs); "
                         "no-stopwords = the same draw without the terms held by more than 1 %% of the docs")
    ap.add_argument("--shortlist", choices=("auto", "f16-inline", "f16", "f32"), default="auto",
                    help="shortlist scan of the timed path (GpuIndex.set_dense): auto = f16 copy; "
                         "results are the same float64-exact bits in every flavour (DESIGN.md 4.1)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step of every timed pipeline "
                         "returned as DIR/<pipeline>_<field>.npy (float32 / float64; more than 64 MB in all: "
                         "the same seeded sample of the query rows of every array)")
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.shard_proxy and not args.full:
        ap.error("--shard-proxy is one of the measurements of --full")
    if args.preset:
        args.config = {"configs1": "dense", "configs2": "dense_bm25", "configs3": "triple",
                       "configs4": "triple_rerank"}[args.preset]
        if args.preset in ("configs3", "configs4"):
            if args.docs == 1_000_000:      # (an explicit --docs wins: rehearsals run the layout on a small corpus)
                args.docs = 10_000_000
            args.doc_shards = args.doc_shards or args.gpus
    return args


def which_config(args, world):
    """The pipeline a run times, or "all": the four of CONFIGS, the headline (dense) first.  Without
    ``--config`` that is dense alone, except at N = 1 in a ``--full`` run and in one that dumps its
    outputs (whose arrays are those of all four pipelines, ``--full`` or not)."""
    if args.config:
        return args.config
    return "all" if world == 1 and not args.no_extras and (args.full or args.dump_outputs) else "dense"


def result_arrays(cfg, res):
    """What a caller of the timed path holds after a step -- the BatchResult of retrieve_batch:
    the fused (or reranked) ids / scores / counts and every channel's merged list -- copied to
    the host as ``<pipeline>_<field>`` arrays, one row per query."""
    fields = {"ids": res.ids, "scores": res.scores, "counts": res.counts}
    for name, (S, I, cnt) in res.channels.items():
        fields[name + "_scores"], fields[name + "_ids"] = S, I
        if cnt is not None:
            fields[name + "_counts"] = cnt
    return {f"{cfg}_{k}": v.cpu().numpy() for k, v in fields.items()}


def dump_outputs(dirname, arrays, max_bytes=DUMP_MAX_BYTES):
    """Write ``arrays`` (name -> host array, one row per query) as dirname/<name>.npy.  float32
    and float64 stay as they are; ids and counts become float64 (exact below 2**53).  When the
    files would exceed max_bytes in all, every array keeps the same seeded sample of the query
    rows, and sample_rows.npy holds their numbers."""
    arrays = {k: a if a.dtype in (np.float32, np.float64) else a.astype(np.float64)
              for k, a in arrays.items()}
    n_rows = len(next(iter(arrays.values())))
    assert all(len(a) == n_rows for a in arrays.values())
    header = 256 * (len(arrays) + 1)   # (an .npy header is 128 bytes for these shapes)
    rows = None
    if sum(a.nbytes for a in arrays.values()) + header > max_bytes:
        row_bytes = sum(a.nbytes for a in arrays.values()) // n_rows + 8
        keep = max(0, max_bytes - header) // row_bytes
        rows = np.sort(np.random.Generator(np.random.PCG64([4321, 64])).choice(n_rows, size=keep, replace=False))
        arrays = {k: a[rows] for k, a in arrays.items()}
        arrays["sample_rows"] = rows.astype(np.float64)
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(dirname, name + ".npy"), a)
    return {"dir": dirname, "arrays": sorted(arrays), "query_rows": n_rows if rows is None else len(rows),
            "of": n_rows, "bytes": int(sum(a.nbytes for a in arrays.values()))}


def event_ms(fn, reps, torch):
    fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    args = parse()
    import torch
    import torch.distributed as dist
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd import synth
    from triple_hybrid_rag_amd.distributed import (ShardedIndex, auto_doc_shards, layout_2d, replica_groups,
                                                  shard_range)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch N>1 with torch.distributed.run (one process per GPU)")
    # THR_BENCH_REHEARSAL=1: all ranks on cuda:0 over gloo -- exercises the N > 1 control flow
    # (sharding, groups, exchange through the host, merge) on a one-GPU box; not a measurement
    rehearsal = os.environ.get("THR_BENCH_REHEARSAL") == "1"
    torch.cuda.set_device(0 if rehearsal else local_rank)
    backend = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = "gloo" if rehearsal else "nccl"
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world,
                                    device_id=torch.device("cuda", local_rank))
    which = which_config(args, world)
    # the sections of a --full run that --no-extras / --no-cpu-baseline leave out
    extras_on = args.full and not args.no_extras
    cpu_on = args.full and not args.no_cpu_baseline
    run_cfgs = list(CONFIGS) if which == "all" else [which]
    need_lex = any(c != "dense" for c in run_cfgs)
    need_graph = any(c.startswith("triple") for c in run_cfgs)
    need_tok = "triple_rerank" in run_cfgs

    # ---- inputs (deterministic, identical for every world size) ----
    import types
    doc_shards = args.doc_shards
    if not doc_shards:   # auto: shard only as far as the scan still dominates a shard's step
        doc_shards = auto_doc_shards(world, args.docs, args.min_shard_docs)
    nq = args.queries

    def build(doc_shards):
        """This rank's resident state for a layout of ``doc_shards`` document shards x
        world / doc_shards query replicas: its shard's index, its replica's query batch."""
        B = types.SimpleNamespace(doc_shards=doc_shards, n_replicas=world // doc_shards)
        B.shard, B.replica, _ = layout_2d(rank, world, doc_shards)
        n_replicas, replica = B.n_replicas, B.replica
        B.group = None
        if world > 1 and n_replicas > 1:
            B.group = replica_groups(world, doc_shards)[replica]
        lo, hi = shard_range(args.docs, B.shard, doc_shards)
        B.lo, B.hi, B.n_local = lo, hi, hi - lo
        t0 = time.time()
        B.docs = synth.dense_rows(lo, B.n_local, args.dim)
        queries = synth.dense_queries(nq * n_replicas, args.dim, args.docs)
        B.queries = np.ascontiguousarray(queries[replica::n_replicas])   # this replica's batch
        B.index = T.GpuIndex(doc_base=lo).set_dense(B.docs, shortlist=args.shortlist)
        B.qt = B.seeds = B.qtok = B.csr = B.graph = B.qt_alt = B.idf = B.avgdl = None
        if need_lex:
            v = synth.vocab_size(args.docs)
            d_, t_, f_ = synth.lexical_rows(lo, B.n_local, args.docs)
            B.csr = synth.build_lexical_csr(d_, t_, f_, B.n_local, v)
            df = torch.from_numpy(B.csr.df_local.copy())
            sdl = torch.tensor([B.csr.sum_dl_local], dtype=torch.float64)
            if doc_shards > 1:   # global statistics: every shard scores as the whole corpus would
                dev_ = "cpu" if rehearsal else "cuda"   # (summed over the shards of ONE replica: its group)
                df, sdl = df.to(dev_), sdl.to(dev_)
                dist.all_reduce(df, group=B.group)
                dist.all_reduce(sdl, group=B.group)
                df, sdl = df.cpu(), sdl.cpu()
            df = df.numpy()
            B.idf = np.log(1.0 + (args.docs - df.astype(np.float64) + 0.5) / (df.astype(np.float64) + 0.5))
            B.avgdl = float(sdl.item()) / args.docs
            B.index.set_lexical(B.csr.rowptr, B.csr.post_doc, B.csr.post_tf, B.csr.doclen, B.idf, B.avgdl)
            dfq = df.copy()
            dfq[dfq > 0.01 * args.docs] = 0          # the "no-stopwords" mix: no term held by > 1 % of the docs
            B.qt_alt = {"survey": synth.lexical_queries(nq * n_replicas, df, 4)[replica::n_replicas],
                        "no-stopwords": synth.lexical_queries(nq * n_replicas, dfq, 4)[replica::n_replicas]}
            B.qt = B.qt_alt[args.lexical_mix]
        if need_graph:
            B.graph = synth.build_graph(args.docs, lo, hi)
            B.index.set_graph(B.graph.ent_rowptr, B.graph.ent_col, B.graph.men_rowptr, B.graph.men_chunk,
                              B.graph.men_conf)
            B.seeds = synth.graph_queries(nq * n_replicas, args.docs, 3)[replica::n_replicas]
        if need_tok:
            n_tok = min(B.n_local, args.token_docs) if args.token_docs else B.n_local
            B.index.set_tokens(synth.device_tokens(lo, n_tok))
            g = torch.Generator(device="cuda")
            g.manual_seed(4321 + 3)
            B.qtok = torch.nn.functional.normalize(torch.randn((nq * n_replicas, 32, 128), generator=g, device="cuda"),
                                                   dim=2).to(torch.float16)[replica::n_replicas].contiguous()
        B.gen_s = time.time() - t0
        B.index.reserve(nq, 100)   # workspaces are part of the resident index, not of a step
        B.sharded = ShardedIndex(B.index, group=B.group)
        # The step starts where the reference's embed_query() starts its post-processing
        # (rag2/embedder.py:226-241): the embedding model's 4096-d vectors, resident in HBM.  Their
        # first ``dim`` components are the synthetic query directions at an arbitrary scale, the rest
        # is noise that the Matryoshka truncation drops; thr_embed_postproc (truncate + float32
        # L2-normalise) is the first kernel of every timed step.
        B.raw = np.empty((nq, 4096), dtype=np.float32)
        B.raw[:, :args.dim] = B.queries * np.float32(3.7)
        B.raw[:, args.dim:] = np.random.Generator(np.random.PCG64([4321, 9, replica])).standard_normal(
            (nq, 4096 - args.dim), dtype=np.float32)
        B.raw_pinned = torch.from_numpy(B.raw).pin_memory()
        B.raw_dev = B.raw_pinned.cuda()
        B.qd = T._native.embed_postproc(B.raw_dev, args.dim)   # (the query vectors the extras below use)
        B.qtd = torch.from_numpy(np.ascontiguousarray(B.qt)).cuda() if B.qt is not None else None
        B.sd = torch.from_numpy(np.ascontiguousarray(B.seeds)).cuda() if B.seeds is not None else None
        torch.cuda.synchronize()
        return B

    B = build(doc_shards)
    # (the names the rest of this file uses)
    n_replicas, group, n_local = B.n_replicas, B.group, B.n_local
    docs, queries, index, csr, graph = B.docs, B.queries, B.index, B.csr, B.graph
    qt, seeds, qtok, qt_alt, idf = B.qt, B.seeds, B.qtok, B.qt_alt, B.idf
    raw, raw_pinned, raw_dev, qd, qtd, sd, gen_s = B.raw, B.raw_pinned, B.raw_dev, B.qd, B.qtd, B.sd, B.gen_s

    def step_fn(cfg, B=B):
        kw = {}
        if cfg != "dense":
            kw["query_terms"] = B.qtd
        if cfg.startswith("triple"):
            kw["query_seeds"] = B.sd
        if cfg == "triple_rerank":
            kw.update(qtok=B.qtok, rerank_top_k=100)
        w = {"lexical": 0.7, "semantic": 0.8} if cfg == "dense_bm25" else None   # configs[2]: RRF(0.8/0.7)
        return lambda: B.sharded.retrieve_batch(T._native.embed_postproc(B.raw_dev, args.dim), top_k=args.top_k,
                                                weights=w, **kw)

    def barrier():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def measure(step):
        """W warm-up steps, then K timed steps between barriers; max over ranks."""
        res, counters = None, []
        for _ in range(args.warmup):
            res = step()
        barrier()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            res = step()
            counters.append(res.rescued)   # device counters: a step has no host read-back
        barrier()
        elapsed = time.perf_counter() - t0
        rescued = sum(int(c) for c in counters)
        if world > 1:
            t = torch.tensor([elapsed], dtype=torch.float64, device="cpu" if rehearsal else "cuda")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return res, rescued, elapsed

    FLAVOURS = ("f16-inline", "f16", "f32")
    KERNEL = {"f32": f"dense_scan_mfma2<dim={args.dim},MODE_FILTER>",
              "f16": (f"dense_scan_f16qs<dim={args.dim},MODE_FILTER,{os.environ.get('THR_DENSE_MFMA', '16')}> "
                      "(v_mfma_f32_16x16x32_f16 unless THR_DENSE_MFMA=32; " if args.dim <= 768 and
                      os.environ.get("THR_DENSE_F16") != "q" else
                      f"dense_scan_f16q<dim={args.dim},MODE_FILTER> (v_mfma_f32_32x32x16_f16; ") +
                     "queries in registers, fragment-major f16 rows through LDS-DMA)",
              "f16-inline": f"dense_scan_f16<dim={args.dim},MODE_FILTER> (float32 rows rounded in flight)"}

    def set_flavour(name):
        """Switch the shortlist scan of the (already resident) index in place."""
        index.shortlist = name
        if name == "f32":
            index.docs16, index.doc_rel_err = None, 0.0
        else:
            index.docs16, index.doc_rel_err = T._native.dense_quantize_f16(
                index.docs, keep_copy=name == "f16")

    def committed_pmc(n_local=n_local):
        """HBM bytes per launch of the default scan from the committed --pmc pass (profiles/,
        FETCH_SIZE x2 on gfx950): NOT measured in this run, and only quoted for the shape it
        was collected on."""
        try:
            with open(PMC_PROFILE) as f:
                pm = json.load(f)
            if (pm["n_docs"], pm["dim"], pm["queries"]) == (n_local, args.dim, nq):
                return pm
        except (OSError, KeyError, ValueError):
            pass
        return None

    def probe_scan(name, queries_dev=None, reps=None, B=B):
        """The streaming scan kernel alone: average launch time from HIP events on its stream."""
        index, n_local = B.index, B.n_local
        qx = B.qd if queries_dev is None else queries_dev
        if queries_dev is not None:
            index.dense_search(qx, 100, rescue=False)   # thresholds / query image for this batch
        ms = event_ms(lambda: index.scan_probe(qx), reps or args.probe_reps, torch)
        f16 = name != "f32"
        n_q = qx.shape[0]
        qtile = 32 if name == "f32" else T._native.dense_f16_query_tile(args.dim, name == "f16", n_q)
        flops = 2.0 * n_local * args.dim * n_q
        peak = MFMA_F16_PEAK_TFLOPS if f16 else MFMA_F32_PEAK_TFLOPS
        ach = flops / (ms * 1e-3) / 1e12
        out = {"bound": "mfma", "kernel": f"{KERNEL[name]} ({qtile} queries per workgroup)",
               "achieved": round(ach, 1), "peak": peak, "unit": "TFLOP/s",
               "frac": round(ach / peak, 4), "traffic": None,
               "launch_ms": round(ms, 4), "flops_per_launch": flops}
        # what one launch has to read: the float16 copy (or the float32 rows), once
        out["traffic_algorithmic"] = n_local * args.dim * (2 if name == "f16" else 4)
        pm = committed_pmc(n_local) if (name == "f16" and queries_dev is None) else None
        if pm:
            out["traffic"] = pm["hbm_read_bytes_per_launch"]
            out["traffic_source"] = (os.path.relpath(PMC_PROFILE, ROOT) + " (separate rocprofv3 --pmc run, same "
                                     "kernel and shape; not re-measured in this run)")
            out["traffic_over_algorithmic"] = round(pm["hbm_read_bytes_per_launch"] / out["traffic_algorithmic"], 3)
            out["hbm_gbps_at_this_launch_time"] = round(pm["hbm_read_bytes_per_launch"] / (ms * 1e-3) / 1e9, 1)
            out["mfma_pipe_busy_under_pmc"] = pm.get("mfma_pipe_busy")
            out["clock_ghz_under_pmc"] = pm.get("clock_ghz")
        return out

    primary = index.shortlist
    res, rescued, elapsed = measure(step_fn(run_cfgs[0] if which != "all" else "dense"))
    head_cfg = run_cfgs[0] if which != "all" else "dense"
    # --dump-outputs: the last timed step's result of every pipeline timed below, copied to the
    # host as soon as its timed window has closed (rank 0: the merged lists are the same on
    # every rank of a replica)
    dumped = {}
    if args.dump_outputs and rank == 0:
        dumped.update(result_arrays(head_cfg, res))
    qps = args.steps * nq * n_replicas / elapsed   # every replica serves its own batch
    roofline = probe_scan(primary) if args.full else None
    head_ids = res.ids.clone()
    def rank_breakdown(B, elapsed, roof):
        """Where this rank's share of a step goes: the scan alone, the exchange alone (the same
        all-gather on this step's own lists), and everything else of the step."""
        from triple_hybrid_rag_amd.distributed import gather_topk_many
        Ss_, Is_, _, _ = B.index.dense_search(B.qd, 100, sync=False)
        pairs = [(Ss_, Is_)]
        if head_cfg != "dense":
            Sl_, Il_, _ = B.index.bm25_search(B.qtd, 50)
            pairs.append((Sl_, Il_))
        if head_cfg.startswith("triple"):
            Sg_, Ig_, _ = B.index.graph_search(B.sd, 50, 2)
            pairs.append((Sg_, Ig_))
        ex_ms = event_ms(lambda: gather_topk_many(pairs, B.group), 5, torch)
        fx, fx_ms = B.sharded._floor_exchange(), 0.0
        if fx is not None:   # the dense channel's floor exchange: nq x m float32 per rank
            from triple_hybrid_rag_amd.index import floor_width
            lb_ = torch.zeros((B.qd.shape[0], floor_width(100, fx[1])), dtype=torch.float32, device=B.qd.device)
            fx_ms = event_ms(lambda: fx[0](lb_), 5, torch)
        step_ms = 1e3 * elapsed / args.steps
        return {"step_ms": round(step_ms, 3), "scan_ms": roof["launch_ms"], "exchange_ms": round(ex_ms, 3),
                "floor_exchange_ms": round(fx_ms, 3) if fx is not None else None,
                "fixed_ms": round(step_ms - roof["launch_ms"] - ex_ms - fx_ms, 3),
                "exchange_bytes_per_rank": int(sum(2 * 8 * s_.numel() for s_, _ in pairs)),
                "shard_docs": B.n_local,
                "note": "rank 0; fixed = embed post-processing, threshold sample + select, shortlist, "
                        "float64 rescoring, merge, fusion"}

    def shard_proxy(G):
        """One rank's GPU work of a DOCUMENT-SHARDED dense step, measured on one GPU: the --docs
        corpus as G shards resident in this process, every shard's kernels launched back to back
        (each fills the chip, so the total / G is a shard's share), the all-gathers replaced by the
        stacking copies that produce the same tensors.  Classic: every shard ranks a top-100 of its
        own.  Floor: thr_dense_shortlist_f16 -> (exchange) -> thr_dense_floor -> thr_dense_finish_f16."""
        from triple_hybrid_rag_amd.index import floor_width
        N_ = T._native
        shards = []
        for s_ in range(G):
            lo_, hi_ = shard_range(args.docs, s_, G)
            ix = T.GpuIndex(doc_base=lo_).set_dense(synth.dense_rows(lo_, hi_ - lo_, args.dim),
                                                    shortlist=args.shortlist)
            ix.reserve(nq, 100)
            shards.append(ix)
        if shards[0].shortlist not in ("f16", "f16-inline"):
            return None
        last = {}

        def tail(outs):
            S_ = torch.stack([o[0] for o in outs])
            I_ = torch.stack([o[1] for o in outs])
            for _ in shards:   # every rank merges the gathered lists and fuses
                _, Im, _ = N_.merge_topk(S_, I_, 100)
                ids_, _, _, _ = N_.rrf_fuse(None, Im, None, args.top_k, 0.7, 0.8, 1.0)
            last["ids"], last["counts"] = ids_, torch.stack([o[2] for o in outs])

        def classic():
            tail([ix.dense_search(N_.embed_postproc(B.raw_dev, args.dim), 100, sync=False) for ix in shards])

        def floor():
            # a rank runs shortlist -> exchange -> finish back to back (its candidate lists still in
            # cache): shard by shard here, the finish taking the gathered bounds of the PREVIOUS
            # repetition -- the same values, the inputs do not change
            if "lbs" not in last:
                last["lbs"] = torch.stack([ix.dense_shortlist(B.qd, 100, G) for ix in shards])
            outs, lbs = [], []
            for ix in shards:
                q_ = N_.embed_postproc(B.raw_dev, args.dim)
                lbs.append(ix.dense_shortlist(q_, 100, G))
                outs.append(ix.dense_finish(q_, 100, lb_all=last["lbs"]))
            last["lbs"] = torch.stack(lbs)
            tail(outs)

        reps = max(3, args.steps // 4)
        classic()
        ms_c = event_ms(classic, reps, torch) / G
        ids_c, rows_c = last["ids"].clone(), float(last["counts"].float().mean())
        floor()
        ms_f = event_ms(floor, reps, torch) / G
        same = bool(torch.equal(ids_c, last["ids"]))
        rows_f = float(last["counts"].float().mean())
        m = floor_width(100, G)
        return {"shards": G, "rows_per_shard": args.docs // G, "queries_per_step": nq,
                "ms_per_shard_step_classic": round(ms_c, 3), "ms_per_shard_step_floor": round(ms_f, 3),
                "rows_rescored_per_query_and_shard": {"classic": round(rows_c, 1), "floor": round(rows_f, 1)},
                "fused_ids_identical": same, "floor_exchange_bytes_per_rank": 4 * nq * m,
                "note": "one GPU runs the G shards' kernels back to back; total / G; the collectives (one "
                        "all-gather of the result lists; for the floor one more of nq x m float32) are NOT "
                        "in these figures -- they have never run on more than one GPU"}

    per_rank = strong = None
    if world > 1 and args.full:
        per_rank = rank_breakdown(B, elapsed, roofline)
        # The north star's layout -- the corpus cut into N document shards, ONE batch served by all
        # N GPUs, per-shard top-k merged through the all-gather -- is reported in every
        # N > 1 line, whatever layout the headline ran: the same run, the same corpus and batch.
        if B.n_replicas == 1:
            strong = {"layout": f"doc-shard x{world}", "same_run_as_the_headline": True, "scaling": "strong",
                      "ms_per_step": round(1e3 * elapsed / args.steps, 3), "value": round(qps, 1),
                      "unit": "queries/s", "per_rank_ms": per_rank}
        else:
            B2 = build(world)
            _, resc2, el2 = measure(step_fn(head_cfg, B2))
            roof2 = probe_scan(primary, B=B2)
            strong = {"layout": f"doc-shard x{world}", "same_run_as_the_headline": False, "scaling": "strong",
                      "ms_per_step": round(1e3 * el2 / args.steps, 3), "value": round(args.steps * nq / el2, 1),
                      "unit": "queries/s", "rescued_queries": resc2,
                      "scan": {k_: roof2[k_] for k_ in ("achieved", "peak", "unit", "frac", "launch_ms")},
                      "per_rank_ms": rank_breakdown(B2, el2, roof2)}
            del B2
            torch.cuda.empty_cache()

    # ---- the other configs (N = 1 default run): same corpus, same batch ----
    cfg_out = {}
    chan = {}
    if which == "all":
        for cfg in CONFIGS[1:]:
            r2, resc2, el2 = measure(step_fn(cfg))
            if args.dump_outputs:
                dumped.update(result_arrays(cfg, r2))
            cfg_out[cfg] = {"baseline_config": BASELINE_CONFIG[cfg] + " pipeline", "docs": args.docs,
                            "gpus": 1, "lexical_mix": args.lexical_mix,
                            "value": round(args.steps * nq / el2, 1), "unit": "queries/s",
                            "ms_per_step": round(1e3 * el2 / args.steps, 3), "rescued_queries": resc2,
                            "_ids": r2.ids}
    if which == "all" and args.full:
        # per-stage launch times, each stage alone (HIP events)
        Ss, Is, _, _ = index.dense_search(qd, 100, sync=False)
        Sl, Il, _ = index.bm25_search(qtd, 50)
        Sg, Ig, _ = index.graph_search(sd, 50, 2)
        fused = T._native.rrf_fuse(Il, Is, Ig, 100, 0.7, 0.8, 1.0)
        bm = {}
        for mix, q_ in qt_alt.items():     # the lexical kernel alone on BOTH query mixes
            qd_ = torch.from_numpy(np.ascontiguousarray(q_)).cuda()
            post = int(sum(int(csr.df_local[t]) for row in q_ for t in row if t >= 0))
            ms_b = event_ms(lambda: index.bm25_search(qd_, 50), 5, torch)
            ms_all = event_ms(lambda: index.bm25_search(qd_, 50, prune=False), 2, torch)
            by_b = post * 12 + nq * 64        # ids + term frequencies + doc lengths of every posting
            # The default call prunes (exact MaxScore / WAND bounds: same bits): most postings of a
            # stop-word query are never read, so bytes-of-every-posting / time is NOT its HBM rate --
            # it is quoted as an equivalent only; the HBM-rate figure is the unpruned call's.
            bm[mix] = {"ms": round(ms_b, 3), "queries": nq, "postings_per_query": round(post / nq, 1),
                       "ms_every_posting_scored": round(ms_all, 3),
                       "every_posting_scored_GBps": round(by_b / ms_all / 1e6, 1),
                       "every_posting_scored_frac_of_hbm_8TBps": round(by_b / ms_all / 1e6 / HBM_PEAK_GBPS, 4),
                       "pruned_equivalent_GBps_not_a_traffic_figure": round(by_b / ms_b / 1e6, 1)}
        bm["mix_of_the_timed_configs"] = args.lexical_mix
        bm["mixes"] = {"survey": "4 term ids sampled in proportion to df (SURVEY 8d; stop words included)",
                       "no-stopwords": "the same draw without the terms held by more than 1 % of the docs"}
        ms_g = event_ms(lambda: index.graph_search(sd, 50, 2), 5, torch)
        ms_r = event_ms(lambda: T._native.rrf_fuse(Il, Is, Ig, 10, 0.7, 0.8, 1.0), 5, torch)
        ms_m = event_ms(lambda: index.maxsim(qtok, fused[0]), 5, torch)
        ms_d = event_ms(lambda: index.dense_search(qd, 100, sync=False), 5, torch)
        by_m = nq * 100 * 128 * 128 * 2
        # north star's "per-query embedding encode" as far as this path owns it: the model's
        # 4096-d vectors -> truncate to dim -> L2-normalise (thr_embed_postproc), and the PCIe
        # transfer of the raw batch from pinned host memory
        ms_e = event_ms(lambda: T._native.embed_postproc(raw_dev, args.dim), 5, torch)
        ms_h = event_ms(lambda: raw_pinned.cuda(non_blocking=True), 5, torch)
        chan = {"embed_postproc": {"ms": round(ms_e, 4), "h2d_ms_4096d_fp32_batch": round(ms_h, 3),
                                   "note": "thr_embed_postproc IS the first kernel of every timed step "
                                           "(the step starts from the model's 4096-d vectors in HBM); the "
                                           "H2D copy of that raw batch from pinned memory is quoted "
                                           "beside it and is not in `value`"},
                "dense_search_ms": round(ms_d, 3),
                "bm25": bm,
                "graph": {"ms": round(ms_g, 3), "algorithmic_GBps": round(8800 * nq / ms_g / 1e6, 1)},
                "rrf_ms": round(ms_r, 3),
                "maxsim": {"ms": round(ms_m, 3), "algorithmic_GBps": round(by_m / ms_m / 1e6, 1),
                           "frac_of_hbm_8TBps": round(by_m / ms_m / 1e6 / HBM_PEAK_GBPS, 4),
                           "TFLOPs": round(2.0 * nq * 100 * 32 * 128 * 128 / ms_m / 1e9, 1)}}

    # ---- the other shortlist flavours, measured in the same run for comparison ----
    extras = {}
    if world == 1 and extras_on and args.dim in (512, 768, 1024):
        for name in FLAVOURS:
            if name == primary:
                continue
            set_flavour(name)
            r2, resc2, el2 = measure(step_fn("dense"))
            pr = probe_scan(name)
            extras[name] = {"value": round(args.steps * nq / el2, 1), "unit": "queries/s",
                            "ms_per_step": round(1e3 * el2 / args.steps, 3), "rescued_queries": resc2,
                            "scan": {k: pr[k] for k in ("kernel", "achieved", "peak", "unit", "frac", "launch_ms")},
                            "fused_top10_identical_to_primary": bool(torch.equal(r2.ids, head_ids))}
        set_flavour(primary)

    # ---- single-query regime (N = 1): drop-in retrieve() latency; the scan at small batches ----
    latency = None
    if world == 1 and extras_on:
        latency = {"scan_small_batches": []}
        copy_bytes = n_local * args.dim * 2
        for b in (1, 32, 256):
            pr = probe_scan(primary, qd[:b].contiguous(), reps=10)
            latency["scan_small_batches"].append({
                "queries": b, "launch_ms": pr["launch_ms"],
                "hbm_GBps_one_pass_over_the_f16_copy": round(copy_bytes / (pr["launch_ms"] * 1e-3) / 1e9, 1),
                "frac_of_hbm_8TBps": round(copy_bytes / (pr["launch_ms"] * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)})
        index.dense_search(qd, 100, rescue=False)
        # batch path for ONE query end to end, host vector included: embed post-processing
        # (thr_embed_postproc: truncate 4096 -> dim, L2-normalise) + H2D + dense + RRF
        full = np.random.default_rng(7).standard_normal((1, 4096)).astype(np.float32)
        pinned = torch.from_numpy(full).pin_memory()

        def one_query():
            v = T._native.embed_postproc(pinned.cuda(non_blocking=True), args.dim)
            return index.retrieve_batch(v, top_k=args.top_k)
        for _ in range(3):
            one_query()
        torch.cuda.synchronize()
        ts = []
        for _ in range(30):
            t1 = time.perf_counter()
            r = one_query()
            r.ids.cpu()
            ts.append((time.perf_counter() - t1) * 1e3)
        latency["batch_api_one_query_ms"] = {"p50": round(float(np.percentile(ts, 50)), 3),
                                             "p95": round(float(np.percentile(ts, 95)), 3),
                                             "includes": "H2D of a 4096-float vector, thr_embed_postproc, "
                                                         "dense top-100, RRF, D2H of the 10 ids"}
        # the reference's API: RAG2Retriever.retrieve(), one query per call, Python rows in / out
        import asyncio
        from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
        from triple_hybrid_rag_amd.config import SETTINGS
        from triple_hybrid_rag_amd.rag2.retrieval import RAG2Retriever
        SETTINGS.rag2_safety_threshold, SETTINGS.rag2_denoise_alpha = 0.0, 0.0
        store = CorpusStore.synthetic(n_local, vocab_size=synth.vocab_size(args.docs) if need_lex else 0)
        client = GpuIndexClient(index, store, org_id="org")

        class Emb:
            def __init__(self):
                self.i = 0

            def embed_query(self, text):
                self.i += 1
                return queries[self.i % nq].tolist()

        retr = RAG2Retriever(org_id="org", embedder=Emb(), query_planner=object())
        retr._supabase = client
        text = "t100 t2000 t77" if need_lex else ""
        ts = []
        loop = asyncio.new_event_loop()   # one loop for all the calls, as the reference's tool layer
        for i in range(33):               # keeps one (tools/crm_knowledge.py:111-124)
            t1 = time.perf_counter()
            out = loop.run_until_complete(retr.retrieve(text, top_k=args.top_k, skip_planning=True,
                                                        skip_rerank=True))
            if i >= 3:
                ts.append((time.perf_counter() - t1) * 1e3)
        loop.close()
        latency["dropin_retrieve_ms"] = {"p50": round(float(np.percentile(ts, 50)), 3),
                                         "p95": round(float(np.percentile(ts, 95)), 3),
                                         "contexts": len(out.contexts),
                                         "channels": "lexical + semantic" if need_lex else "semantic"}

    # ---- exactness of what was timed + CPU baseline (rank 0, N = 1) ----
    cpu = None
    check = None
    if rank == 0 and world == 1 and cpu_on:
        from oracle import c_oracle as CO
        from oracle import thr_oracle as O
        torch.set_num_threads(os.cpu_count() or 1)
        nq_cpu = min(args.cpu_queries, nq)
        # everything the CPU leg uses is computed on the CPU: the row norms (index set-up, not
        # timed on either side) and the post-processed query vectors (timed, as on the GPU)
        dn = CO.doc_norms(docs)
        norms_equal = bool(np.array_equal(index.dnorm.cpu().numpy(), dn))
        t0 = time.perf_counter()
        q_cpu = O.embed_postproc_batch(raw[:nq_cpu], args.dim)
        Sc, Ic = O.dense_topk_fast(docs, q_cpu, 100, dnorm=dn)
        fused_ids = [O.fused_topk_ids(None, list(i), None, args.top_k)[0] for i in Ic]
        cpu_s = time.perf_counter() - t0
        cpu = {"value": round(nq_cpu / cpu_s, 2), "unit": "queries/s", "cores": os.cpu_count(),
               "kind": "port",
               "sample": f"{nq_cpu} of the {nq} queries over the full "
                         f"{args.docs}x{args.dim} corpus (embedding post-processing + fp32 BLAS shortlist + "
                         f"fp64 rescoring + RRF), {cpu_s:.1f} s; row norms computed on the CPU beforehand",
               "gpu_inputs_equal_the_cpu_ones": {
                   "thr_doc_norms_bits": norms_equal,
                   "thr_embed_postproc_bits": bool(np.array_equal(qd[:nq_cpu].cpu().numpy(), q_cpu))}}
        ids = head_ids.cpu().numpy()
        if head_cfg == "dense":
            same = sum(list(ids[i]) == fused_ids[i] for i in range(nq_cpu))
            check = {"fused_top10_identical": f"{same}/{nq_cpu}", "recall_at_10": round(float(np.mean(
                [len(set(ids[i]) & set(fused_ids[i])) / args.top_k for i in range(nq_cpu)])), 4)}
        if which == "all":
            # the hybrid pipelines against the oracle's channels + fusion, on a bounded sample
            sub = list(range(0, nq, max(1, nq // 32)))[:32]
            _, Il_o = O.bm25_topk(csr.rowptr, csr.post_doc, csr.post_tf, csr.doclen, idf,
                                  B.avgdl, qt[sub], n_local, 50)
            _, Ig_o = O.graph_topk(graph.ent_rowptr, graph.ent_col, graph.men_rowptr, graph.men_chunk,
                                   graph.men_conf, seeds[sub], 2, n_local, 50)
            block = 8192
            for cfg in CONFIGS[1:]:
                got = cfg_out[cfg].pop("_ids").cpu().numpy()
                okc, checked = 0, 0
                for j, qi in enumerate(sub):
                    w = {"lexical": 0.7, "semantic": 0.8} if cfg == "dense_bm25" else None
                    n_f = 100 if cfg == "triple_rerank" else args.top_k
                    fi, _ = O.fused_topk_ids(list(Il_o[j]), list(Ic[qi]),
                                             list(Ig_o[j]) if cfg.startswith("triple") else None, n_f, w)
                    if cfg != "triple_rerank":
                        okc += int(list(got[qi]) == fi)
                        checked += 1
                        continue
                    if j >= 8:      # oracle MaxSim on 8 queries: their candidates' token rows are
                        continue    # regenerated block by block on the device and copied back
                    rows_ = {}
                    for b in sorted({d // block for d in fi}):
                        blk = synth.device_tokens(b * block, min(block, n_local - b * block))
                        for d in fi:
                            if d // block == b:
                                rows_[d] = blk[d - b * block].cpu().numpy()
                        del blk
                    dt = np.stack([rows_[d] for d in fi])
                    ms_o = CO.maxsim(qtok[qi:qi + 1].cpu().numpy(), dt, np.arange(len(fi), dtype=np.int64)[None])[0]
                    order = O.rerank_order([float(np.float32(x)) for x in ms_o])[:args.top_k]
                    es_ = np.array([ms_o[p_] for p_ in order])
                    good = True
                    for a in range(len(order)):   # identical wherever the oracle's scores are > 2e-4 apart
                        if (a == 0 or es_[a - 1] - es_[a] > 2e-4) and (a == len(order) - 1 or es_[a] - es_[a + 1] > 2e-4):
                            good &= int(got[qi][a]) == fi[order[a]]
                    okc += int(good)
                    checked += 1
                cfg_out[cfg]["parity_sample"] = (f"{okc}/{checked} " +
                                                 ("reranked top-10 = the oracle's MaxSim order of the oracle's fused top-100"
                                                  if cfg == "triple_rerank" else "fused top-10 identical to the oracle"))
    for cfg in cfg_out:
        cfg_out[cfg].pop("_ids", None)

    if rank == 0:
        names = {"dense": f"{args.docs}-doc / {args.dim}-d dense-only brute-force cosine top-{args.top_k}",
                 "dense_bm25": f"{args.docs}-doc dense + BM25 + RRF(0.8/0.7)",
                 "triple": f"{args.docs}-doc triple-hybrid (dense + BM25 + graph avg-deg 8)",
                 "triple_rerank": f"{args.docs}-doc triple-hybrid + late-interaction rerank (32x128x128, top-100)"}
        out = {
            "metric": "queries/sec (fused top-10)", "value": round(qps, 1), "unit": "queries/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "full": args.full,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
            # same corpus at every N; with replicas the per-GPU work is fixed from doc_shards GPUs on
            "scaling": "weak" if n_replicas > 1 else "strong", "vs_baseline": None,
            "dtype": ("f32" if primary == "f32" else "f16") + " MFMA shortlist scan (f32 accumulate) + "
                     "f64 rescoring of the f32 rows",
            "data": "synthetic",
            "config": {"workload": f"{names[head_cfg]} (BASELINE.json {BASELINE_CONFIG[head_cfg]})",
                       "pipeline": head_cfg, "docs": args.docs, "dim": args.dim, "queries_per_step": nq,
                       "semantic_top_k": 100, "fused_top_k": args.top_k, "shortlist": primary,
                       "parallelism": (f"doc-shard x{doc_shards}" + (f" x {n_replicas} replicas (each serves its own "
                                       f"{nq}-query batch per step)" if n_replicas > 1 else "") +
                                       ("" if args.doc_shards else f"; auto layout: >= {args.min_shard_docs} rows per shard"))
                       if world > 1 else "single GPU",
                       "collective_backend": backend, "world_size_seen": dist.get_world_size() if world > 1 else 1,
                       "rescued_queries": rescued, "input_gen_s": round(gen_s, 1),
                       "step": "thr_embed_postproc of the 4096-d query batch (resident in HBM) -> dense top-100"
                               + ("" if head_cfg == "dense" else " + BM25 top-50" + (" + graph top-50" if head_cfg.startswith("triple") else ""))
                               + " -> weighted RRF -> fused top-10" + (" of the MaxSim-reranked top-100" if head_cfg == "triple_rerank" else ""),
                       "lexical_mix": args.lexical_mix if head_cfg != "dense" else None,
                       "per_rank_ms": per_rank, "strong_doc_sharded": strong,
                       "shard_floor_proxy": shard_proxy(args.shard_proxy)
                       if world == 1 and args.shard_proxy > 1 else None},
            "roofline": roofline, "cpu_baseline": cpu,
        }
        if cfg_out:
            out["configs"] = cfg_out
        if chan:
            out["stages_alone"] = chan
        if extras:
            out["other_shortlists"] = extras
        if latency:
            out["latency"] = latency
        if check:
            out["parity_check"] = check
        if args.dump_outputs:
            out["dumped_outputs"] = dump_outputs(args.dump_outputs, dumped)
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
