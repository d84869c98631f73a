#!/usr/bin/env python3
"""Text to BM25 term ids: the device route (GpuIndex.query_terms / text_rows: thr_text_tokens, thr_query_terms)
against the host route it stands beside, the GpuIndexClient._query_terms loop and insert_children's token loop,
on the same inputs in the same run.

    python scripts/bench_text.py [--queries 2048,65536] [--chunks 10000] [--out profiles/text_terms.md]

Inputs are seeded: the synthetic vocabulary of synth.py (``t{i}``, Zipf-drawn), queries of 4 - 12 tokens (a
few capitalised, a few unknown), chunks of about 1 KB (~220 tokens Zipf-drawn from 20 000 words, 1 in 200 of
them a term no earlier chunk holds; the index is built from 2 000 such chunks first).

Query path, per batch size, text -> the int32 [nq, 32] table on the device:
  host    [client._query_terms(q) for q in queries], the rows padded into one array and uploaded; wall clock,
          median of --rounds;
  device  GpuIndex.query_terms(queries) as called (encode + pack on the host, two uploads, the kernels, a
          synchronise); wall clock, median; of which: the host packing alone, the two uploads alone (H2D, between
          synchronises) and the kernels alone (device events over pre-uploaded inputs).
Insert path: the same --chunks rows through GpuIndexClient.insert_children of twin clients, device_text off and
on, wall clock of one call each; and the text step alone (the token loop / GpuIndex.text_rows).
The two routes' answers are compared."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def zipf_words(rng, v, n, s=1.05):
    w = 1.0 / np.power(np.arange(1, v + 1, dtype=np.float64), s)
    cdf = np.cumsum(w) / w.sum()
    return np.minimum(np.searchsorted(cdf, rng.random(n)), v - 1)


def make_queries(rng, v, nq):
    lens = rng.integers(4, 13, nq)
    t = zipf_words(rng, v, int(lens.sum()))
    u = rng.random(len(t))
    toks = [f"T{x}" if a < 0.05 else f"u{x}" if a < 0.08 else f"t{x}" for x, a in zip(t.tolist(), u.tolist())]
    out, at = [], 0
    for n in lens.tolist():
        out.append(" ".join(toks[at:at + n]))
        at += n
    return out


def make_chunks(rng, v, n, first):
    out = []
    for i in range(n):
        t = zipf_words(rng, v, 220)
        u = rng.random(220)
        toks = [f"novo{x}" if a < 0.005 else f"T{x}," if a < 0.05 else f"t{x}" for x, a in zip(t.tolist(), u.tolist())]
        out.append(" ".join(toks) + f". doc{first + i}")
    return out


def wall(fn, rounds):
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
    ap.add_argument("--queries", default="2048,65536")
    ap.add_argument("--chunks", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_text needs the GPU: nothing is measured without one")
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd import index_build as IB, synth
    from triple_hybrid_rag_amd.backend import CorpusStore, GpuIndexClient
    from triple_hybrid_rag_amd.index_text import pack_texts
    N = T._native
    N.load()
    cus, hbm, arch = N.device_info()
    lines = []
    rng = np.random.default_rng(17)
    v = synth.vocab_size(1_000_000)
    vocab = [f"t{i}" for i in range(v)]
    store = CorpusStore.synthetic(4, vocab_size=v)
    idx = T.GpuIndex()
    t0 = time.perf_counter()
    idx.set_vocabulary(vocab)
    torch.cuda.synchronize()
    lines += [f"Vocabulary: {v:,} terms `t{{i}}`; device table built in {(time.perf_counter() - t0) * 1e3:.0f} ms "
              f"({idx.text['slots'].shape[0]:,} slots).", ""]

    class Client(GpuIndexClient):           # (the host function needs the store and an index with a lexical side)
        def __init__(self):
            self.store, self.index, self.lexical_and = store, type("Lexical", (), {"lex": {}})(), False
    client = Client()
    for nq in [int(s) for s in args.queries.split(",")]:
        queries = make_queries(rng, v, nq)

        def host():
            tab = np.full((nq, N.THR_BM25_MAX_TERMS), -1, dtype=np.int32)
            for q, text in enumerate(queries):
                row = client._query_terms(text)
                if row:
                    tab[q, :len(row)] = row
            return torch.from_numpy(tab).to(idx.device)
        host_ms, host_tab = wall(host, args.rounds)
        dev_ms, (dev_tab, _) = wall(lambda: idx.query_terms(queries), args.rounds)
        if not torch.equal(host_tab, dev_tab):
            sys.exit(f"{nq} queries: the device table differs from the host's")
        pack_ms, (blob, ptr) = wall(lambda: pack_texts(queries), args.rounds)
        h2d_ms, (dblob, dptr) = wall(lambda: (idx._t(blob, torch.uint8), idx._t(ptr, torch.int64)), args.rounds)
        X = idx.text

        def kernels():
            rows = N.text_tokens(dblob, dptr, int(ptr[-1]), X["table_dev"], X["slots"], X["term_bytes"], X["term_ptr"],
                                 workspace=idx._ws_text)
            return N.query_terms(rows, workspace=idx._ws_qterms)
        for _ in range(3):
            kernels()
        ker = []
        for _ in range(args.rounds):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(10):
                kernels()
            e1.record()
            torch.cuda.synchronize()
            ker.append(e0.elapsed_time(e1) / 10)
        ker_ms = statistics.median(ker)
        lines += [f"### Query path: {nq:,} queries of 4 - 12 tokens ({int(ptr[-1]) / 1e6:.2f} MB of text)", "",
                  f"- host `_query_terms` loop + one upload of the table: **{host_ms:.1f} ms** "
                  f"({nq / host_ms * 1e3 / 1e6:.3f} M queries/s)",
                  f"- device route, `GpuIndex.query_terms` as called: **{dev_ms:.1f} ms** "
                  f"({nq / dev_ms * 1e3 / 1e6:.3f} M queries/s), {host_ms / dev_ms:.1f}x",
                  f"- of the device route: host encode + pack {pack_ms:.2f} ms, the two uploads (H2D) {h2d_ms:.2f} ms "
                  f"= {100 * h2d_ms / dev_ms:.0f} % of the call, kernels alone {ker_ms:.3f} ms "
                  f"({nq / ker_ms * 1e3 / 1e6:.1f} M queries/s; median of {args.rounds} rounds of 10 between device events)",
                  "- the two tables are equal", ""]
        print("\n".join(lines[-7:]), flush=True)

    # ---- insert path
    d, n0, m = 1024, 2000, args.chunks
    vc = 20_000         # the chunks' words: few enough for the base rows to have seen most of them
    base_texts = make_chunks(rng, vc, n0, 0)
    emb = rng.standard_normal((n0 + m, d)).astype(np.float32)

    def rows_of(texts, first):
        return [{"id": f"c{first + i}", "parent_id": "p0", "document_id": "d0", "text": t, "page": 1, "modality": "text",
                 "embedding_1024": emb[first + i], "org_id": "org"} for i, t in enumerate(texts)]
    parents = [{"id": "p0", "text": "parent", "section_heading": "S"}]
    base = rows_of(base_texts, 0)
    batch = rows_of(make_chunks(rng, vc, m, n0), n0)
    kb = sum(len(r["text"].encode()) for r in batch) / m / 1e3
    took = {}
    clients = {}
    for name, kw in (("host", {}), ("device", {"device_text": True})):
        hi = IB.from_rows(base, parents)
        c = clients[name] = GpuIndexClient(hi.to_gpu(), hi.store, org_id="org", **kw)
        texts = [r["text"] for r in batch]
        if name == "host":
            def text_step():
                return [c.store.vocab.get(tok) for t in texts for tok in c.tokenizer(t)]
        else:
            def text_step():
                return c.index.text_rows(texts)
        step_ms, _ = wall(text_step, 3)
        v_before = len(c.store.vocab)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        c.insert_children(batch)
        torch.cuda.synchronize()
        took[name] = ((time.perf_counter() - t0) * 1e3, step_ms)
    a, b = clients["host"], clients["device"]
    if list(a.store.vocab.items()) != list(b.store.vocab.items()) or \
            not all(torch.equal(a.index.lex[k], b.index.lex[k]) for k in ("rowptr", "post_doc", "post_tf", "doclen")):
        sys.exit("insert path: the two routes left different indexes")
    lines += [f"### Insert path: {m:,} chunks of {kb:.2f} KB through `insert_children` (index of {n0:,} rows, dim {d})", "",
              f"- host route: **{took['host'][0]:.0f} ms** per call; its token loop alone {took['host'][1]:.0f} ms",
              f"- `device_text=True`: **{took['device'][0]:.0f} ms** per call; `GpuIndex.text_rows` alone "
              f"{took['device'][1]:.0f} ms ({took['host'][1] / took['device'][1]:.1f}x the loop)",
              f"- new terms in the batch: {len(b.store.vocab) - v_before:,} on top of {v_before:,}; "
              "vocabulary, CSR and document lengths equal after both", ""]
    print("\n".join(lines[-5:]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Text to BM25 term ids: the device route against the host loops\n\n"
                    f"`python scripts/bench_text.py --queries {args.queries} --chunks {args.chunks}` on "
                    f"{arch} ({cus} CUs, {hbm / 2 ** 30:.0f} GiB), {os.cpu_count()} host CPUs visible (one used), "
                    f"Python {sys.version.split()[0]}, {time.strftime('%Y-%m-%d')}; "
                    f"wall-clock medians of {args.rounds} unless noted.  Both sides ran in this one process.\n\n"
                    + "\n".join(lines))


if __name__ == "__main__":
    main()
