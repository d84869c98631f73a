#!/usr/bin/env python3
"""Cost of graph ingest on the synthetic graph of an n-chunk corpus (default 1M chunks: 250k
entities, ~2M stored edges, 1M mentions): thr_csr_merge alone by device events, GpuIndex.append_graph
of 1 / 256 / 16 384 entities + relations and GpuIndex.append_mentions of 1 / 256 / 16 384 mentions
(wall time of one call ending in a synchronise, after the same calls ran once at that batch size on
a throw-away index), the same change made by a rebuild (a vectorised host build of
the graph over all rows -- a lower bound of index_build.build_graph, which walks dict rows --
+ set_graph + set_entity_names), and graph_search of --queries queries before and after, with the
run-to-run spread of the "before" side.  Needs the GPU; prints one JSON line per measurement.

    python3 scripts/bench_graph_ingest.py [--n 1000000] [--queries 2048] [--batches 1,256,16384]
    python3 scripts/bench_graph_ingest.py --delete [--n 1000000] [--queries 2048] [--share 0.01]

--delete measures graph delete instead: --share of the entities removed with their cascade (relations in both
directions, mentions, names) by GpuIndex.delete_graph, thr_csr_prune alone on both CSRs by device events, the
same change by a rebuild over the surviving rows, and graph_search before and after.

synth.build_graph draws its edges at random and keeps the few repeated ones; the index is built
from the de-duplicated edge list (index_build.build_graph's canonical form), which the merge needs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import triple_hybrid_rag_amd as T   # noqa: E402
from triple_hybrid_rag_amd import _native as N, synth   # noqa: E402


def timed(fn, reps=1):
    """(result, wall ms, device ms) of fn() -- the wall clock ends in a device synchronise."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return out, (time.perf_counter() - t0) * 1e3 / reps, e0.elapsed_time(e1) / reps


def host_graph(n_ent, src, dst, me, mc, mw):
    """The fresh build over edge and mention lists, vectorised: (src, dst) unique and sorted, mentions
    by (entity, chunk), stably."""
    key = np.unique(src.astype(np.int64) * n_ent + dst)
    s, d = key // n_ent, (key % n_ent).astype(np.int32)
    er = np.concatenate([[0], np.cumsum(np.bincount(s, minlength=n_ent))]).astype(np.int64)
    order = np.lexsort((mc, me))
    mr = np.concatenate([[0], np.cumsum(np.bincount(me, minlength=n_ent))]).astype(np.int64)
    return er, d, mr, mc[order].astype(np.int32), mw[order].astype(np.float32)


def edge_list(g):
    src = np.repeat(np.arange(len(g[0]) - 1, dtype=np.int64), np.diff(g[0]))
    return src, g[1].astype(np.int64)


def mention_list(g):
    me = np.repeat(np.arange(len(g[2]) - 1, dtype=np.int64), np.diff(g[2]))
    return me, g[3].astype(np.int64), g[4]


def warm_up(m):
    """The two calls at batch size m on a throw-away index: the torch ops of the canonicalisation
    (unique, sort, bincount, cumsum pick their kernels by size) have run once before anything is timed."""
    e = 1024
    rp = np.zeros(e + 1, dtype=np.int64)
    idx = T.GpuIndex()
    idx.n_docs = 4096
    idx.set_graph(rp, np.zeros(0, np.int32), rp, np.zeros(0, np.int32), np.zeros(0, np.float32))
    idx.set_entity_names([f"w{i}" for i in range(e)])
    r = np.random.default_rng(m)
    idx.append_graph(entity_names=[f"x{j}" for j in range(m)], relations=(r.integers(0, e, m), r.integers(0, e + m, m)))
    idx.append_mentions(r.integers(0, e + m, m), r.integers(0, 4096, m), r.random(m).astype(np.float32))
    torch.cuda.synchronize()


def search_ms(idx, seeds, reps):
    for _ in range(3):
        idx.graph_search(seeds, 50, 2)
    return [timed(lambda: idx.graph_search(seeds, 50, 2), 5)[2] for _ in range(reps)]


HBM_PEAK_GBPS = 8000.0      # MI355X: 8 TB/s


def prune_alone(lib, st, rowptr, ids, pay, remap, n_new, with_ids: bool):
    """thr_csr_prune by device events on one CSR of the index -> (ms, bytes the three kernels move, kept)."""
    rows, nnz = int(rowptr.shape[0]) - 1, int(ids.shape[0])
    out = torch.empty(nnz, dtype=torch.int32, device="cuda")
    pout = None if pay is None else torch.empty(nnz, dtype=pay.dtype, device="cuda")
    rp_out = torch.empty(n_new + 1, dtype=torch.int64, device="cuda")
    tail = torch.zeros(2, dtype=torch.int64, device="cuda")
    ws = torch.empty(max(N.csr_prune_workspace_bytes(rows, nnz), 8), dtype=torch.uint8, device="cuda")

    def prune():
        rc = lib.thr_csr_prune(rowptr.data_ptr(), rows, nnz, ids.data_ptr(), None if pay is None else pay.data_ptr(),
                               remap.data_ptr(), n_new, remap.data_ptr() if with_ids else None, rows if with_ids else 0, 0,
                               None, 0, None, rp_out.data_ptr(), out.data_ptr(), None if pout is None else pout.data_ptr(),
                               nnz, None, tail.data_ptr(), tail.data_ptr() + 8, ws.data_ptr(), ws.numel(), st)
        assert rc == 0, rc
    prune()
    _, _, ms = timed(prune, 20)
    kept, status = (int(v) for v in tail.tolist())
    assert status == 0
    # count: ids in, keep words out; scatter: keep words and ids in, kept ids (and payload in and out) out;
    # row pointers in and out, the row remap (the id remap is gathered: at least once per entry)
    moved = nnz * 4 * 4 + kept * 4 * (1 + (2 if pay is not None else 0)) + rows * (8 + 4) + n_new * 8 + \
        (nnz * 4 * 2 if with_ids else 0)
    return ms, moved, kept


def delete_main(a):
    sg = synth.build_graph(a.n)
    n_ent = synth.n_entities(a.n)
    src, dst = edge_list((sg.ent_rowptr, sg.ent_col))
    me, mc, mw = mention_list((None, None, sg.men_rowptr, sg.men_chunk, sg.men_conf))
    g = host_graph(n_ent, src, dst, me, mc, mw)
    names = [f"entity{e}" for e in range(n_ent)]
    idx = T.GpuIndex()
    idx.n_docs = a.n
    idx.set_graph(*g).set_entity_names(names)
    seeds_h = synth.graph_queries(a.queries, a.n)
    before = search_ms(idx, torch.from_numpy(seeds_h).cuda(), a.repeats)
    print(json.dumps({"n": a.n, "entities": n_ent, "edges": int(len(g[1])), "mentions": int(len(g[3])),
                      "graph_search_ms_before": [round(t, 3) for t in before]}), flush=True)
    rng = np.random.default_rng(7)
    gone = rng.choice(n_ent, max(1, int(n_ent * a.share)), replace=False)
    keep = np.ones(n_ent, dtype=bool)
    keep[gone] = False
    remap_h = np.where(keep, np.cumsum(keep) - 1, -1).astype(np.int32)
    remap, n_new = torch.from_numpy(remap_h).cuda(), int(keep.sum())
    lib, st = N.load(), torch.cuda.current_stream().cuda_stream
    G = idx.graph
    t_ent, b_ent, k_ent = prune_alone(lib, st, G["ent_rowptr"], G["ent_col"], None, remap, n_new, True)
    t_men, b_men, k_men = prune_alone(lib, st, G["men_rowptr"], G["men_chunk"], G["men_conf"], remap, n_new, False)
    # the torch ops of the call have run once at this size before anything is timed (a throw-away index)
    warm = T.GpuIndex()
    warm.n_docs = a.n
    warm.set_graph(*g).set_entity_names(names)
    warm.delete_graph(entities=gone)
    del warm
    _, wall_d, dev_d = timed(lambda: idx.delete_graph(entities=gone))
    # the same change as the parent commit offers it: a host build over the surviving rows + set_graph + set_entity_names
    t0 = time.perf_counter()
    es, em = keep[src] & keep[dst], keep[me]
    g2 = host_graph(n_new, remap_h[src[es]].astype(np.int64), remap_h[dst[es]].astype(np.int64),
                    remap_h[me[em]].astype(np.int64), mc[em], mw[em])
    names2 = [nm for nm, k in zip(names, keep) if k]
    t_host = (time.perf_counter() - t0) * 1e3
    fresh = T.GpuIndex()
    fresh.n_docs = a.n
    _, wall_up, _ = timed(lambda: fresh.set_graph(*g2).set_entity_names(names2))
    same = all(torch.equal(idx.graph[k], fresh.graph[k]) for k in ("ent_rowptr", "ent_col", "men_rowptr", "men_chunk", "men_conf"))
    same = same and torch.equal(idx.entities["name_bytes"], fresh.entities["name_bytes"]) and \
        torch.equal(idx.entities["name_ptr"], fresh.entities["name_ptr"])
    print(json.dumps({"deleted_entities": int(len(gone)), "delete_graph_wall_ms": round(wall_d, 3),
                      "delete_graph_device_ms": round(dev_d, 3),
                      "csr_prune_entities_ms": round(t_ent, 4), "csr_prune_entities_GBps": round(b_ent / t_ent / 1e6, 1),
                      "csr_prune_entities_share_of_hbm_peak": round(b_ent / t_ent / 1e6 / HBM_PEAK_GBPS, 4),
                      "csr_prune_mentions_ms": round(t_men, 4), "csr_prune_mentions_GBps": round(b_men / t_men / 1e6, 1),
                      "csr_prune_mentions_share_of_hbm_peak": round(b_men / t_men / 1e6 / HBM_PEAK_GBPS, 4),
                      "edges_kept": k_ent, "mentions_kept": k_men, "rebuild_host_ms": round(t_host, 1),
                      "rebuild_upload_ms": round(wall_up, 1), "equal_to_rebuild": bool(same), "entities": n_new}), flush=True)
    # the same queries, their seeds renumbered with the remap (a removed seed leaves its slot)
    s2 = np.where(seeds_h >= 0, remap_h[np.maximum(seeds_h, 0)], -1).astype(np.int32)
    s2 = np.stack([np.concatenate([r[r >= 0], r[r < 0]]) for r in s2])
    seeds2 = torch.from_numpy(s2).cuda()
    after, after_fresh = search_ms(idx, seeds2, a.repeats), search_ms(fresh, seeds2, a.repeats)
    print(json.dumps({"graph_search_ms_after": [round(t, 3) for t in after],
                      "graph_search_ms_fresh_build": [round(t, 3) for t in after_fresh],
                      "before_spread_ms": round(max(before) - min(before), 3),
                      "after_minus_before_median_ms": round(float(np.median(after) - np.median(before)), 3),
                      "after_minus_fresh_median_ms": round(float(np.median(after) - np.median(after_fresh)), 3)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--delete", action="store_true", help="measure graph delete instead of graph ingest")
    ap.add_argument("--share", type=float, default=0.01, help="--delete: the share of the entities that is removed")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=2048)
    ap.add_argument("--batches", default="1,256,16384")
    ap.add_argument("--repeats", type=int, default=5, help="graph_search timings per side (the spread is the noise)")
    a = ap.parse_args()
    batches = [int(b) for b in a.batches.split(",")]
    if a.n < 64 or a.queries < 1 or not batches or min(batches) < 1:
        ap.error("--n >= 64, --queries >= 1, --batches positive")
    if a.delete:
        if not 0 < a.share < 1:
            ap.error("--share inside (0, 1)")
        return delete_main(a)
    sg = synth.build_graph(a.n)
    n_ent = synth.n_entities(a.n)
    src, dst = edge_list((sg.ent_rowptr, sg.ent_col))
    me, mc, mw = mention_list((None, None, sg.men_rowptr, sg.men_chunk, sg.men_conf))
    g = host_graph(n_ent, src, dst, me, mc, mw)
    names = [f"entity{e}" for e in range(n_ent)]
    idx = T.GpuIndex()
    idx.n_docs = a.n
    idx.set_graph(*g).set_entity_names(names)
    seeds = torch.from_numpy(synth.graph_queries(a.queries, a.n)).cuda()
    before = search_ms(idx, seeds, a.repeats)
    print(json.dumps({"n": a.n, "entities": n_ent, "edges": int(len(g[1])), "mentions": int(len(g[3])),
                      "graph_search_ms_before": [round(t, 3) for t in before]}), flush=True)
    rng = np.random.default_rng(7)
    lib, st = N.load(), torch.cuda.current_stream().cuda_stream
    for m in batches:
        G = idx.graph
        e_now = int(G["ent_rowptr"].shape[0]) - 1
        # ---- thr_csr_merge alone: m relations (both directions) into the entity CSR as it stands
        s, o = rng.integers(0, e_now, m), rng.integers(0, e_now, m)
        key = torch.unique(torch.from_numpy(np.concatenate([s * e_now + o, o * e_now + s])[np.tile(s != o, 2)]).cuda())
        bsrc, bdst = key // e_now, (key % e_now).to(torch.int32).contiguous()
        rp_b = torch.zeros(e_now + 1, dtype=torch.int64, device="cuda")
        rp_b[1:] = torch.cumsum(torch.bincount(bsrc, minlength=e_now), 0)
        nnz_a, nnz_b = int(G["ent_col"].shape[0]), int(bdst.shape[0])
        out = torch.empty(nnz_a + nnz_b, dtype=torch.int32, device="cuda")
        rp_out = torch.empty(e_now + 1, dtype=torch.int64, device="cuda")
        tail = torch.zeros(2, dtype=torch.int64, device="cuda")
        need = int(lib.thr_csr_merge_workspace_bytes(e_now, nnz_a, nnz_b))
        ws = torch.empty(max(need, 8), dtype=torch.uint8, device="cuda")

        def merge():
            rc = lib.thr_csr_merge(G["ent_rowptr"].data_ptr(), e_now, nnz_a, G["ent_col"].data_ptr(), None,
                                   rp_b.data_ptr(), e_now, nnz_b, bdst.data_ptr() if nnz_b else None, None, 1,
                                   rp_out.data_ptr(), out.data_ptr(), None, out.shape[0], tail.data_ptr(),
                                   tail.data_ptr() + 8, ws.data_ptr(), ws.numel(), st)
            assert rc == 0, rc
        merge()
        _, _, t_merge = timed(merge, 20)
        assert int(tail[1].item()) == 0
        moved = (nnz_a + nnz_b) * 4 * 2 + 16 * (e_now + 1) * 2 + nnz_b * 8    # ids in and out, row pointers, keep words
        del out, ws
        warm_up(m)
        # ---- append_graph: m entities + m relations (half of them to the new entities)
        o2 = np.where(np.arange(m) % 2 == 0, o, e_now + rng.integers(0, m, m))
        new_names = [f"entity{e_now + j}" for j in range(m)]
        _, wall_g, dev_g = timed(lambda: idx.append_graph(entity_names=new_names, relations=(s, o2)))
        names += new_names
        # ---- append_mentions: m mentions of stored chunks
        e_m, c_m = rng.integers(0, e_now + m, m), rng.integers(0, a.n, m)
        w_m = (0.5 + 0.5 * rng.random(m)).astype(np.float32)
        _, wall_m, dev_m = timed(lambda: idx.append_mentions(e_m, c_m, w_m))
        # ---- the same change by a rebuild: host build over all rows + set_graph + set_entity_names
        src = np.concatenate([src, s, o2])
        dst = np.concatenate([dst, o2, s])
        me, mc, mw = np.concatenate([me, e_m]), np.concatenate([mc, c_m]), np.concatenate([mw, w_m])
        real = src != dst
        src, dst = src[real], dst[real]
        t0 = time.perf_counter()
        g = host_graph(e_now + m, src, dst, me, mc, mw)
        t_host = (time.perf_counter() - t0) * 1e3
        fresh = T.GpuIndex()
        fresh.n_docs = a.n
        _, wall_up, _ = timed(lambda: fresh.set_graph(*g).set_entity_names(names))
        same = all(torch.equal(idx.graph[k], fresh.graph[k]) for k in ("ent_rowptr", "ent_col", "men_rowptr", "men_chunk", "men_conf"))
        same = same and torch.equal(idx.entities["name_bytes"], fresh.entities["name_bytes"])
        del fresh
        print(json.dumps({"batch": m, "csr_merge_ms": round(t_merge, 4), "csr_merge_GBps": round(moved / t_merge / 1e6, 1),
                          "append_graph_wall_ms": round(wall_g, 3), "append_graph_device_ms": round(dev_g, 3),
                          "append_mentions_wall_ms": round(wall_m, 3), "append_mentions_device_ms": round(dev_m, 3),
                          "rebuild_host_ms": round(t_host, 1), "rebuild_upload_ms": round(wall_up, 1),
                          "equal_to_rebuild": bool(same), "entities": e_now + m,
                          "edges": int(idx.graph["ent_col"].shape[0]), "mentions": int(idx.graph["men_chunk"].shape[0])}),
              flush=True)
    after = search_ms(idx, seeds, a.repeats)
    print(json.dumps({"graph_search_ms_after": [round(t, 3) for t in after],
                      "before_spread_ms": round(max(before) - min(before), 3),
                      "after_minus_before_median_ms": round(float(np.median(after) - np.median(before)), 3)}), flush=True)


if __name__ == "__main__":
    main()
