#!/usr/bin/env python3
"""The token-level analysis (stop list + suffix stemming) on the device: what it costs and what it saves.

    python scripts/bench_text_analyzer.py [--parent-lib PATH] [--out profiles/text_analyzer.md]

1. Kernel time of thr_text_tokens_analyzed with Analyzer.portuguese() against thr_text_tokens on the two batches
   of profiles/text_terms.md (scripts/bench_text.py's generators and seed: 65 536 queries of 4 - 12 tokens, 10 000
   chunks of about 1 KB; their tokens are ``t{i}``, which no rule strips and no stop word equals, so every token
   pays the walk, the stop probe and the rule scan and none is dropped) and on 10 000 chunks of Portuguese-like
   text (below), where stop words drop and suffixes strip.  --parent-lib: another build of the library (the
   parent commit's), whose thr_text_tokens is timed on the same device buffers.  The stop list alone and the rules
   alone are timed too: what the extra walk and the drop cost.
2. The device route (GpuIndex.text_rows / query_terms with the analyzer set) against the host loop over
   Analyzer.tokenize with a dict lookup, wall clock.
3. One index over 100 000 Portuguese-like chunks built WITH stop words as terms; one batch of 2 048
   natural-language-like queries turned into term tables without and with the stop list (no stemming: the index's
   terms are whole words); postings per query (the sum of the terms' document frequencies) and bm25_search time.

Every timing is a median of 5 between device events (10 calls per round), the wall clock of the same rounds beside
it."""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_text import make_chunks, make_queries, zipf_words  # noqa: E402

ROUNDS, CALLS = 5, 10
ENDINGS = ("o", "os", "a", "as", "ar", "ou", "ando", "ado", "ação", "ações", "amente", "inho", "e", "es")
GLUE = "de a o que e do da em um para com não uma os no se na por mais as dos como mas foi ao ele das tem à seu sua ou ser".split()


def portuguese_like(rng, n, lo, hi, roots=20_000):
    """n texts of lo .. hi words: 45 % function words (Zipf over GLUE), else a Zipf-drawn root with an ending."""
    lens = rng.integers(lo, hi + 1, n)
    total = int(lens.sum())
    root = zipf_words(rng, roots, total)
    glue = zipf_words(rng, len(GLUE), total, s=0.9)
    end = rng.integers(0, len(ENDINGS), total)
    is_glue = rng.random(total) < 0.45
    cap = rng.random(total) < 0.06
    words = []
    for i in range(total):
        w = GLUE[glue[i]] if is_glue[i] else f"r{root[i]}x{ENDINGS[end[i]]}"
        words.append(w.capitalize() if cap[i] else w)
    out, at = [], 0
    for k in lens.tolist():
        out.append(" ".join(words[at:at + k]) + ".")
        at += k
    return out


def timed(fn):
    """-> (median ms between device events, median wall ms), per call."""
    for _ in range(3):
        fn()
    ev, wl = [], []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        for _ in range(CALLS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        wl.append((time.perf_counter() - t0) * 1e3 / CALLS)
        ev.append(e0.elapsed_time(e1) / CALLS)
    return statistics.median(ev), statistics.median(wl)


def wall(fn, rounds=3):
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_text_analyzer needs the GPU: nothing is measured without one")
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd import index_build as IB, synth
    from triple_hybrid_rag_amd.index_text import Analyzer, TextTable, host_query_row, pack_texts
    N = T._native
    lib = N.load()
    cus, hbm, arch = N.device_info()
    parent = None
    if args.parent_lib:
        parent = C.CDLL(args.parent_lib)
        parent.thr_text_tokens.restype, parent.thr_text_tokens.argtypes = N._SIGNATURES["thr_text_tokens"]
    pt = Analyzer.portuguese()
    stop_only, rules_only = Analyzer(stop=pt.stop), Analyzer(steps=pt.steps)
    lines = [f"Analyzer.portuguese(): {len(pt.stop)} stop words, {sum(map(len, pt.steps))} rules in {len(pt.steps)} steps.", ""]
    rng = np.random.default_rng(17)
    v = synth.vocab_size(1_000_000)
    vocab = [f"t{i}" for i in range(v)]
    rng_pt = np.random.default_rng(23)
    batches = [("65,536 queries of 4 - 12 tokens `t{i}`", make_queries(rng, v, 65536), vocab),
               ("10,000 chunks of about 1 KB, tokens `t{i}`", make_chunks(rng, 20_000, 10000, 0), vocab),
               ("10,000 Portuguese-like chunks of 120 - 200 words", portuguese_like(rng_pt, 10000, 120, 200), None)]

    # ---- 1 + 2: kernel time and the routes
    for title, texts, voc in batches:
        if voc is None:
            voc = list(dict.fromkeys(tok for t in texts[:3000] for tok in pt.tokenize(t)))
        indexes = {name: T.GpuIndex().set_vocabulary(voc, a) for name, a in
                   (("plain", None), ("portuguese", pt), ("stop list alone", stop_only), ("rules alone", rules_only))}
        blob, ptr = pack_texts(texts)
        nb = int(ptr[-1])
        dblob, dptr = indexes["plain"]._t(blob, torch.uint8), indexes["plain"]._t(ptr, torch.int64)
        cap = N.text_token_capacity(len(texts), nb)
        ws = torch.empty(max(N.text_tokens_workspace_bytes(len(texts), nb, cap), 16), dtype=torch.uint8, device="cuda")
        lines += [f"### {title} ({nb / 1e6:.2f} MB)", ""]
        base = None
        for name, idx in indexes.items():
            X = idx.text
            common = (dblob, dptr, nb, X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"])
            if X["analysis"] is None:
                fn = lambda: N.text_tokens(*common, workspace=ws)       # noqa: E731
            else:
                fn = lambda: N.text_tokens_analyzed(*common, workspace=ws, **X["analysis"])       # noqa: E731
            rows = fn()
            n_total, n_unknown = int(rows["n_total"].item()), int(rows["n_unknown"].item())
            ev, wl = timed(fn)
            base = base or ev
            entry = "thr_text_tokens" if X["analysis"] is None else "thr_text_tokens_analyzed"
            lines.append(f"- {entry}, {name}: **{ev:.3f} ms** between device events ({wl:.3f} ms wall), {ev / base:.2f}x; "
                         f"{n_total:,} rows, {n_unknown:,} unknown")
            if X["analysis"] is None and parent is not None:
                out = {k: rows[k].data_ptr() for k in ("doc", "term", "n_tokens", "flags", "n_total", "unknown_off", "unknown_len", "n_unknown")}

                def old():
                    rc = parent.thr_text_tokens(dblob.data_ptr(), dptr.data_ptr(), len(texts), nb, X["table_dev"].data_ptr(),
                                                X["slots"].data_ptr(), X["slots"].shape[0], X["term_bytes"].data_ptr(),
                                                X["term_ptr"].data_ptr(), X["term_ptr"].shape[0] - 1, cap, out["doc"], out["term"],
                                                out["n_tokens"], out["flags"], out["n_total"], out["unknown_off"],
                                                out["unknown_len"], out["n_unknown"], ws.data_ptr(), ws.numel(),
                                                torch.cuda.current_stream().cuda_stream)
                    assert rc == 0, rc
                ev0, wl0 = timed(old)
                lines.append(f"- thr_text_tokens of the parent commit's library, same buffers: **{ev0:.3f} ms** ({wl0:.3f} ms wall)")
        idx = indexes["portuguese"]
        ids = idx.text["ids"]
        if "queries" in title:
            host_ms, _ = wall(lambda: [host_query_row(pt.tokenize(t), ids) for t in texts])
            dev_ms, _ = wall(lambda: idx.query_terms(texts))
            what = "`GpuIndex.query_terms`"
        else:
            host_ms, _ = wall(lambda: [ids.get(tok, -1) for t in texts for tok in pt.tokenize(t)])
            dev_ms, _ = wall(lambda: idx.text_rows(texts))
            what = "`GpuIndex.text_rows`"
        lines += [f"- routes, wall clock, median of 3: host `Analyzer.tokenize` loop + dict lookup **{host_ms:.1f} ms**, {what} with the "
                  f"analyzer set (pack, upload, kernels, read-back of the unknown list) **{dev_ms:.1f} ms**, {host_ms / dev_ms:.1f}x", ""]
        print("\n".join(lines[-8:]), flush=True)
        del indexes

    # ---- 3: postings per query and bm25_search time, with and without the stop list, one index
    n = 100_000
    corpus = portuguese_like(rng_pt, n, 30, 60)
    t0 = time.perf_counter()
    vocab_d, d_dev, t_dev = IB.lexical_rows_device(corpus)
    rowptr, pd, ptf, dl, df = (a.cpu().numpy() for a in N.lexical_build(d_dev, t_dev, None, n, max(len(vocab_d), 1)))
    rowptr, df = rowptr[:len(vocab_d) + 1], df[:len(vocab_d)]
    dfh = df.astype(np.float64)
    idf = np.log(1.0 + (float(n) - dfh + 0.5) / (dfh + 0.5))
    avgdl = float(dl.astype(np.float64).sum()) / n
    build_ms = (time.perf_counter() - t0) * 1e3
    terms = list(vocab_d)
    queries = portuguese_like(np.random.default_rng(29), 2048, 5, 12)
    lines += [f"### One index, {n:,} Portuguese-like chunks of 30 - 60 words ({len(terms):,} terms, stop words among them; "
              f"built from text on the device in {build_ms:.0f} ms); 2,048 queries of 5 - 12 words", ""]
    for name, a in (("without the stop list (TextTable.default())", None), ("with the stop list (Analyzer(stop=...), no rules)", stop_only)):
        idx = T.GpuIndex().set_lexical(rowptr, pd, ptf, dl, idf, avgdl).set_vocabulary(terms, a)
        qt, _ = idx.query_terms(queries)
        q = qt.cpu().numpy()
        postings = float(np.where(q >= 0, df[np.maximum(q, 0)], 0).sum(axis=1).mean())
        nterms = float((q >= 0).sum(axis=1).mean())
        ev, wl = timed(lambda: idx.bm25_search(qt, 10))
        lines.append(f"- {name}: {nterms:.1f} terms and **{postings:,.0f} postings per query**; bm25_search(k=10) of the batch "
                     f"**{ev:.3f} ms** between device events ({wl:.3f} ms wall)")
    lines.append("")
    print("\n".join(lines[-4:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Text analyzer on the device: stop list and suffix stemming\n\n"
                    f"`python scripts/bench_text_analyzer.py{' --parent-lib <the parent commit build>' if parent else ''}` on "
                    f"{arch} ({cus} CUs, {hbm / 2 ** 30:.0f} GiB), Python {sys.version.split()[0]}, {time.strftime('%Y-%m-%d')}.  "
                    f"Kernel timings: median of {ROUNDS} rounds of {CALLS} calls between device events, the wall clock of the same "
                    "rounds beside it.  Everything ran in this one process.\n\n" + "\n".join(lines))


if __name__ == "__main__":
    main()
