#!/usr/bin/env python3
"""Where the float16-copy scan spends its time: per-phase s_memtime sums of every wave
(thr_dense_scan_stamps_f16), at the bench shape.  At dim <= 768 the staggered kernel dense_scan_f16qs
is stamped (16 words per wave, dense_scan_f16q.hpp QS_PH_*: per group, cycles per interval and the
k-loop's pace per quarter); with THR_DENSE_F16=q, or at dim 1024, the 4-wave-block kernel dense_scan_f16q.
    [THR_DENSE_F16=q] python3 scripts/scan_stamps.py [queries] [docs] [dim]"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def staggered(st, d):
    """dense_scan_f16qs: [waves, 16] -> cycles per interval (= row tile) of every phase, per group."""
    names = ["wait_own_dma", "barrier", "fill", "k_q0", "k_q1", "k_q2", "k_q3", "emit"]
    steps = d // 16 / 4          # k-steps per quarter, 32 matrix-pipe cycles each
    wave = np.arange(st.shape[0]) % 8
    live = st[:, 2:7].sum(axis=1) > 0       # (a padding wave stamps nothing)
    out = {"waves": int(st.shape[0]), "live_waves": int(live.sum()), "intervals_per_wave": float(st[:, 8].mean())}
    for grp, sel in (("A", live & (wave < 4)), ("B", live & (wave >= 4))):
        if not sel.any():
            continue
        per = st[sel, :8] / st[sel, 8:9]
        g = {nm: round(float(per[:, j].mean()), 1) for j, nm in enumerate(names)}
        g["k_loop"] = round(float(per[:, 3:7].sum(axis=1).mean()), 1)
        g["interval"] = round(float((st[sel, 9] / st[sel, 8]).mean()), 1)
        g["cycles_per_step_by_quarter"] = [round(float(per[:, 3 + k].mean() / steps), 1) for k in range(4)]
        g["max_wave"] = {nm: round(float(per[:, j].max()), 1) for j, nm in enumerate(names)}
        out[grp] = g
    return out


def main():
    import torch
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd import synth
    nq = int(sys.argv[1]) if len(sys.argv) > 1 else 2048
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 1_000_000
    d = int(sys.argv[3]) if len(sys.argv) > 3 else 768
    x = torch.from_numpy(synth.dense_rows(0, n, d)).cuda()
    q = torch.from_numpy(synth.dense_queries(nq, d, n)).cuda()
    idx = T.GpuIndex().set_dense(x, shortlist="f16")
    idx.dense_search(q, 100, rescue=False)
    st = T._native.dense_scan_stamps_f16(idx.docs16, n, nq, idx._ws)
    torch.cuda.synchronize()
    st = st.cpu().numpy().astype(np.float64)
    if os.environ.get("THR_DENSE_F16") != "q" and d <= 768:
        print(json.dumps(staggered(st.reshape(-1, 16), d)))
        return
    tiles = st[:, 5]
    names = ["wait_own_dma", "barrier", "ring_fill", "k_loop", "emit"]
    # s_memtime ticks are shader cycles (MI355X_MICROARCH.md); sums are per HALF tile
    out = {"waves": int(st.shape[0]), "half_tiles_per_wave": float(tiles.mean()),
           "cycles_per_half_tile": {nm: round(float((st[:, j] / tiles).mean()), 2) for j, nm in enumerate(names)},
           "cycles_per_half_tile_max_wave": {nm: round(float((st[:, j] / tiles).max()), 2) for j, nm in enumerate(names)},
           "loop_cycles_per_half_tile": round(float((st[:, 6] / tiles).mean()), 2)}
    lo, hi = st[:st.shape[0] // 2], st[st.shape[0] // 2:]
    w = np.arange(st.shape[0]) % 4
    out["by_wave_in_block"] = {int(k): {nm: round(float((st[w == k, j] / tiles[w == k]).mean()), 2)
                                        for j, nm in enumerate(names)} for k in range(4)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
