#!/usr/bin/env python3
"""What a scope clause costs next to an equality (default 1M rows, five attribute columns): the time of
resolving P distinct scopes that select THE SAME ROWS written as an equality (thr_scope_resolve), as a
range and as sets of 2, 64 and 4096 members (thr_scope_resolve_clauses) -- scope p of every variant is
the rows with row % 1024 == p, each variant over a column of its own that spreads those rows over
the values the clause names.  Two figures per cell, device milliseconds between two events ending
in a synchronise: ``resolve`` -- the native call alone (count, scan, scatter; operands already on the
device) -- and ``plan`` -- one GpuIndex.scope_plan, host work, upload and read-back included.  The
variants are timed in alternation in one process after a warm-up of every shape; a cell is the median
(min .. max) of ``--rounds`` rounds.  Then dense_search end to end (scopes resolved inside the call) for
one thin ``In`` scope against the equality scope that selects the same rows: the bits must be equal.
Needs the GPU; prints one JSON line per measurement and, with --md, writes the table as markdown.

    python3 scripts/bench_scope_clauses.py [--n 1000000] [--preds 1,16,256] [--rounds 7] [--reps 20]
                                           [--dense-n 1000000] [--dim 768] [--md profiles/scope_clauses.md]
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import triple_hybrid_rag_amd as T   # noqa: E402
from triple_hybrid_rag_amd import _native as N, index_scope as IS, synth   # noqa: E402

KEYS = 1024                      # scope p = the rows with row % KEYS == p
VARIANTS = (("equality", 1), ("range", 8), ("set2", 2), ("set64", 64), ("set4096", 4096))


def column(n, width):
    """Values (row % KEYS) * width + (row // KEYS) % width: the rows of key p hold width values of their own."""
    r = np.arange(n, dtype=np.int64)
    return ((r % KEYS) * width + (r // KEYS) % width).astype(np.int32)


def scope_of(name, width, p):
    if name == "equality":
        return {name: p}
    if name == "range":
        return {name: T.Between(p * width, p * width + width - 1)}
    return {name: T.In(np.arange(p * width, p * width + width, dtype=np.int32))}


def events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, e0.elapsed_time(e1) / reps


def native_call(idx, name, scopes, n):
    """The native resolve of ``scopes`` as a closure over device operands -> (fn, rowptr tensor)."""
    names = idx.attribute_names()
    cols = [idx.attribute(c) for c in names]
    P = len(scopes)
    dev = cols[0].device
    rowptr = torch.empty(P + 1, dtype=torch.int64, device=dev)
    rows = torch.empty(n, dtype=torch.int32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    overlap = torch.empty(1, dtype=torch.int32, device=dev)
    ptrs = (C.c_void_p * len(cols))(*[c.data_ptr() for c in cols])
    lib = N.load()
    if name == "equality":
        _, tab = idx._scope_table(scopes, P)
        dtab = torch.from_numpy(tab).to(dev)
        need = int(lib.thr_scope_resolve_workspace_bytes(n, P))
        ws = torch.empty(need, dtype=torch.uint8, device=dev)

        def fn():
            N._check(lib.thr_scope_resolve(ptrs, len(cols), n, dtab.data_ptr(), P, rowptr.data_ptr(), rows.data_ptr(), n,
                                           labels.data_ptr(), overlap.data_ptr(), ws.data_ptr(), need, N._stream()),
                     "thr_scope_resolve")
            return rowptr
        return fn, (dtab, ws, rows, labels, overlap, cols)
    keys = idx._scope_keys(scopes, P)
    tab, sv = N.scope_check_clauses(*IS.encode_clauses(keys, len(names)), len(names))
    dtab, dsv = torch.from_numpy(tab).to(dev), torch.from_numpy(sv).to(dev) if sv.size else None
    need = int(lib.thr_scope_resolve_clauses_workspace_bytes(n, P))
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def fn():
        N._check(lib.thr_scope_resolve_clauses(ptrs, len(cols), n, dtab.data_ptr(), P,
                                               dsv.data_ptr() if dsv is not None else None, int(sv.size),
                                               rowptr.data_ptr(), rows.data_ptr(), n, labels.data_ptr(),
                                               overlap.data_ptr(), ws.data_ptr(), need, N._stream()),
                 "thr_scope_resolve_clauses")
        return rowptr
    return fn, (dtab, dsv, ws, rows, labels, overlap, cols)


def stat(v):
    return dict(median=round(float(np.median(v)), 4), min=round(min(v), 4), max=round(max(v), 4))


def cell(s):
    return f"{s['median']:.3f} ({s['min']:.3f} .. {s['max']:.3f})"


def resolve_bench(a, lines):
    n = a.n
    idx = T.GpuIndex()
    idx.n_docs = n
    idx.set_attributes({name: column(n, width) for name, width in VARIANTS})
    out = []
    for P in a.preds:
        runs, keep, counts = {}, [], {}
        for name, width in VARIANTS:
            scopes = [scope_of(name, width, p) for p in range(P)]
            fn, hold = native_call(idx, name, scopes, n)
            keep.append(hold)
            runs[name] = (fn, (lambda s=scopes: idx.scope_plan(s, len(s))))
            counts[name] = idx.scope_plan(scopes, P).counts.tolist()
        assert all(c == counts["equality"] for c in counts.values()), "the variants select different row counts"
        for fn, plan in runs.values():              # warm-up: every shape
            for _ in range(3):
                fn()
                plan()
        torch.cuda.synchronize()
        ms = {name: ([], []) for name in runs}
        for _ in range(a.rounds):
            for name, (fn, plan) in runs.items():
                ms[name][0].append(events_ms(fn, a.reps)[1])
                ms[name][1].append(events_ms(plan, max(1, a.reps // 4))[1])
        for name, (r, p) in ms.items():
            line = dict(bench="scope_clauses", rows=n, columns=len(VARIANTS), scopes=P, variant=name,
                        rows_per_scope=int(np.mean(counts[name])), resolve_ms=stat(r), plan_ms=stat(p),
                        rounds=a.rounds, reps=a.reps)
            print(json.dumps(line), flush=True)
            out.append(line)
    lines += ["| scopes | variant | rows per scope | resolve ms | scope_plan ms |", "|---|---|---|---|---|"]
    lines += [f"| {r['scopes']} | {r['variant']} | {r['rows_per_scope']} | {cell(r['resolve_ms'])} | {cell(r['plan_ms'])} |"
              for r in out]


def dense_bench(a, lines):
    n, dim, nq, k = a.dense_n, a.dim, 16, 10
    idx = T.GpuIndex().set_dense(synth.dense_rows(0, n, dim), shortlist="f16")
    idx.set_attributes({"equality": column(n, 1), "set64": column(n, 64)})
    q = torch.from_numpy(synth.dense_queries(nq, dim, n)).cuda()
    runs = {"equality": [scope_of("equality", 1, 5)] * nq, "set64": [scope_of("set64", 64, 5)] * nq}
    res = {name: idx.dense_search(q, k, scopes=s) for name, s in runs.items()}
    equal = all(torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8))
                for x, y in zip(res["equality"][:3], res["set64"][:3]))
    assert equal, "the In scope and the equality scope over the same rows returned different bits"
    for s in runs.values():
        for _ in range(3):
            idx.dense_search(q, k, scopes=s)
    torch.cuda.synchronize()
    ms = {name: [] for name in runs}
    for _ in range(a.rounds):
        for name, s in runs.items():
            ms[name].append(events_ms(lambda: idx.dense_search(q, k, scopes=s), a.reps)[1])
    line = dict(bench="scope_clauses_dense", rows=n, dim=dim, queries=nq, k=k, rows_in_scope=int(idx.scope_plan(runs["equality"], nq).counts[0]), bits_equal=equal, rounds=a.rounds, reps=a.reps,
                **{name + "_ms": stat(v) for name, v in ms.items()})
    print(json.dumps(line), flush=True)
    lines += ["", f"dense_search end to end, {n} x {dim}, f16 shortlist, {nq} queries in one scope of {line['rows_in_scope']} rows "
              f"(scopes resolved inside the call), bits equal: {equal}", "",
              "| scope written as | dense_search ms |", "|---|---|",
              f"| equality | {cell(line['equality_ms'])} |", f"| In of 64 members | {cell(line['set64_ms'])} |"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--preds", default="1,16,256")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--dense-n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--no-dense", action="store_true")
    ap.add_argument("--md", default=None, help="write the tables as markdown to this file")
    a = ap.parse_args()
    a.preds = [int(x) for x in a.preds.split(",")]
    assert max(a.preds) <= min(KEYS, IS.SCOPE_MAX_GENERAL) and a.rounds >= 1
    cus, _, arch = N.device_info()
    lines = [f"{arch}, {cus} CUs; {a.n} rows, {len(VARIANTS)} int32 attribute columns; device ms between two events ending in a "
             f"synchronise, median (min .. max) of {a.rounds} rounds of {a.reps} calls ({max(1, a.reps // 4)} scope_plan calls), "
             "variants alternated in one process after a warm-up", ""]
    resolve_bench(a, lines)
    if not a.no_dense:
        dense_bench(a, lines)
    if a.md:
        os.makedirs(os.path.dirname(os.path.abspath(a.md)), exist_ok=True)
        with open(a.md, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
