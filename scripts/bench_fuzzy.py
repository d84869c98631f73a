#!/usr/bin/env python3
"""Typo-tolerant lexical queries (thr_vocab_nearest / thr_query_terms_fuzzy, include/thr_hip_fuzzy.h) on one
MI355X, in ONE process, seeded inputs.

    python scripts/bench_fuzzy.py [--out profiles/fuzzy_terms.md] [--keys 1000000]

1. thr_vocab_nearest alone over a synthetic vocabulary of --keys keys (random lower-case words of 4 - 14 code
   points, one in eight with an accented letter; Zipf document frequencies) for 100 / 1 000 / 10 000 needles (keys
   with one or two random edits): time between device events, key-store bytes per second against the HBM peak, and
   the (key, needle) pairs per second that are left after the length pruning -- counted on the host from the two
   length histograms, the kernel's own rule.
2. GpuIndex.query_terms(fuzzy=Fuzzy()) on a batch of 2 048 queries of 4 - 12 tokens of that vocabulary in which 0 %,
   5 % and 50 % of the queries hold one misspelt token, against query_terms(fuzzy=None) -- the route before this
   feature -- on the same batch, alternating, wall clock around a device synchronise (pack, upload, kernels).

Every figure is a median over the rounds with the smallest and the largest beside it.  The lexical leg of a
retrieve_batch step is not measured here."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUNDS = 7
HBM_PEAK = 8.0e12          # bytes per second, the data sheet's
LETTERS = "abcdefghijklmnopqrstuvwxyz"
ACCENTED = "áàâãéêíóôõúç"


def make_keys(rng, n):
    """n distinct words of 4 - 14 code points."""
    keys = {}
    while len(keys) < n:
        m = n - len(keys) + 1024
        lens = rng.integers(4, 15, m)
        mat = rng.integers(0, 26, (m, 14))
        acc = rng.random(m) < 0.125
        where = rng.integers(0, 4, m)
        which = rng.integers(0, len(ACCENTED), m)
        for i in range(m):
            w = "".join(LETTERS[c] for c in mat[i, :lens[i]])
            if acc[i]:
                w = w[:where[i]] + ACCENTED[which[i]] + w[where[i] + 1:]
            keys.setdefault(w, None)
            if len(keys) == n:
                break
    return list(keys)


def misspell(rng, w, edits):
    for _ in range(edits):
        p = int(rng.integers(0, len(w)))
        kind = int(rng.integers(0, 3))
        ch = LETTERS[int(rng.integers(0, 26))]
        w = w[:p] + ch + w[p:] if kind == 0 else (w[:p] + w[p + 1:] if len(w) > 4 else w[:p] + ch + w[p + 1:]) if kind == 1 \
            else w[:p] + ch + w[p + 1:]
    return w


def spread(xs):
    return f"**{statistics.median(xs):.3f} ms** ({min(xs):.3f} .. {max(xs):.3f})"


def events(fn, calls):
    """Per-call ms between device events, ROUNDS rounds of ``calls`` calls, after a warm-up."""
    for _ in range(2):
        fn()
    out = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / calls)
    return out


def wall_pair(a, b, calls=5):
    """Two routes alternating: per-call wall ms around a synchronise, ROUNDS rounds each."""
    for fn in (a, b, a, b):
        fn()
    ta, tb = [], []
    for _ in range(ROUNDS):
        for fn, out in ((a, ta), (b, tb)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) * 1e3 / calls)
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--keys", type=int, default=1_000_000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fuzzy needs the GPU: nothing is measured without one")
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd.index_text import Fuzzy, TextTable, fuzzy_edits, pack_texts
    N = T._native
    N.load()
    cus, hbm, arch = N.device_info()
    rng = np.random.default_rng(41)
    t0 = time.perf_counter()
    keys = make_keys(rng, args.keys)
    v = len(keys)
    df = np.maximum(1, (200_000 / (1 + rng.permutation(v))).astype(np.int64))       # Zipf over a random order
    rowptr = np.concatenate([[0], np.cumsum(df)]).astype(np.int64)
    key_len = np.fromiter(map(len, keys), dtype=np.int64, count=v)
    blob, ptr = pack_texts(keys)
    n_key_bytes = int(ptr[-1])
    d_keys, d_ptr, d_rowptr = (torch.from_numpy(a).cuda() for a in (blob, ptr, rowptr))
    table = torch.from_numpy(TextTable.default().entries.view(np.int32)).cuda()
    lines = [f"Vocabulary: {v:,} keys of 4 - 14 code points, {n_key_bytes / 1e6:.2f} MB of UTF-8, Zipf document frequencies "
             f"(made in {time.perf_counter() - t0:.1f} s on the host).", ""]

    # ---- 1: the scan alone
    lines += ["## thr_vocab_nearest alone (max_edits 2, n_best 2, with document frequencies)", "",
              "| needles | time per call | key-store bytes / s | of the 8 TB/s HBM peak | pairs after pruning | pairs / s | needles answered |",
              "|---|---|---|---|---|---|---|"]
    hist_k = np.bincount(key_len, minlength=64)
    for n_needles in (100, 1000, 10000):
        pick = rng.integers(0, v, n_needles)
        needles = [misspell(rng, keys[i], 1 + int(rng.integers(0, 2))) for i in pick]
        nb_blob, nb_ptr = pack_texts(needles)
        n_bytes = int(nb_ptr[-1])
        off = torch.from_numpy(nb_ptr[:-1].copy()).cuda()
        ln = torch.from_numpy(np.diff(nb_ptr).astype(np.int32)).cuda()
        cnt = torch.tensor([n_needles], dtype=torch.int32, device="cuda")
        text = torch.from_numpy(nb_blob).cuda()
        near = torch.empty((n_needles, 2), dtype=torch.int32, device="cuda")
        dist = torch.empty_like(near)
        ws = torch.empty(max(N.vocab_nearest_workspace_bytes(n_bytes, n_needles, v, n_key_bytes, 2), 16), dtype=torch.uint8, device="cuda")

        def fn():
            N.vocab_nearest(text, n_bytes, table, off, ln, cnt, d_keys, d_ptr, n_key_bytes, term_rowptr=d_rowptr, max_edits=2,
                            n_best=2, workspace=ws, near_term=near, near_dist=dist)
        ms = events(fn, 10 if n_needles < 10000 else 2)
        answered = int((near[:, 0] >= 0).sum().item())
        pairs = 0
        for w in needles:
            n = len(w)
            d = fuzzy_edits(n, 2)
            if d and n <= 32:
                pairs += int(hist_k[max(n - d, 0):n + d + 1].sum())
        med = statistics.median(ms) * 1e-3
        lines.append(f"| {n_needles:,} | {spread(ms)} | {n_key_bytes / med / 1e9:.1f} GB/s | {100 * n_key_bytes / med / HBM_PEAK:.2f} % | "
                     f"{pairs:,} | {pairs / med / 1e9:.2f} G/s | {answered:,} |")
        print(lines[-1], flush=True)
    lines.append("")

    # ---- 2: the route, against the route before the feature
    idx = T.GpuIndex().set_vocabulary(keys)
    idx.lex = dict(rowptr=d_rowptr)                 # (this route reads the lexical index's row pointer and nothing else of it)
    zipf = np.cumsum(1.0 / (1 + np.arange(v)))
    zipf /= zipf[-1]
    lines += ["## GpuIndex.query_terms on 2,048 queries of 4 - 12 tokens (pack, upload, kernels; wall clock around a synchronise)", "",
              "| queries with one misspelt token | fuzzy=None (the route before) | fuzzy=Fuzzy() | ratio of the medians | the same between device events: None, Fuzzy() |",
              "|---|---|---|---|---|"]
    for share in (0.0, 0.05, 0.5):
        queries = []
        for q in range(2048):
            toks = [keys[int(i)] for i in np.searchsorted(zipf, rng.random(int(rng.integers(4, 13))))]
            if rng.random() < share:
                p = int(rng.integers(0, len(toks)))
                toks[p] = misspell(rng, toks[p], 1)
            queries.append(" ".join(toks))
        plain = lambda: idx.query_terms(queries)                         # noqa: E731
        fuzzy = lambda: idx.query_terms(queries, fuzzy=Fuzzy())          # noqa: E731
        flags = fuzzy()[1]
        corrected = int(((flags & N.TEXT_CORRECTED) != 0).sum().item())
        ta, tb = wall_pair(plain, fuzzy)
        ea, eb = events(plain, 5), events(fuzzy, 5)
        lines.append(f"| {100 * share:.0f} % ({corrected} rows corrected) | {spread(ta)} | {spread(tb)} | "
                     f"{statistics.median(tb) / statistics.median(ta):.2f}x | {statistics.median(ea):.3f} ms, {statistics.median(eb):.3f} ms |")
        print(lines[-1], flush=True)
    lines += ["", "The lexical leg of a `retrieve_batch` step with the corrections: not measured.", ""]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Typo-tolerant lexical queries: nearest vocabulary terms on the device\n\n"
                    f"`python scripts/bench_fuzzy.py` on {arch} ({cus} CUs, {hbm / 2 ** 30:.0f} GiB), Python {sys.version.split()[0]}, "
                    f"{time.strftime('%Y-%m-%d')}.  Every timing: the median of {ROUNDS} warm rounds, the smallest and the largest "
                    "in brackets.  Everything ran in this one process.\n\n" + "\n".join(lines))


if __name__ == "__main__":
    main()
