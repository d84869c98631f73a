#!/usr/bin/env python3
"""Numbering new BM25 terms on the device (GpuIndex.number_text_rows / commit_vocabulary: thr_text_tokens +
thr_vocab_grow) against the routes it stands beside, in ONE process on one GPU, wall-clock medians of --rounds.

    python scripts/bench_text_ingest.py [--chunks 10000] [--bulk 200000] [--out profiles/text_numbering.md]

Insert: --chunks chunks of about 1 KB (bench_text.py's: ~220 tokens Zipf-drawn from 20 000 words, 1 in 200 a
term no earlier chunk holds) through GpuIndexClient.insert_children into an index of 2 000 rows, twin clients
with device_text=True, number_on_device off and on; every round inserts into a freshly built pair.  Also the
text step alone (text_rows + the host numbering against number_text_rows + commit_vocabulary + the new terms'
strings), the kernels alone between device events over pre-uploaded inputs, and the host read-backs of one batch
(counted: every .cpu() / .item() / .tolist() of a device tensor).
Bulk: --bulk such chunks (rows without embeddings: the lexical part) through index_build.from_rows(),
device=True (host tokenizer + pandas factorize, CSR on the device) and device="text".
The routes' answers are compared; nothing is promised, the file records what was measured."""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from bench_text import make_chunks, zipf_words  # noqa: E402


def bulk_chunks(rng, v, n):
    """make_chunks' distribution, built with array operations (200 000 chunks in seconds)."""
    words = np.array([f"t{x}" for x in range(v)] + [f"T{x}," for x in range(v)] + [f"novo{x}" for x in range(v)], dtype=object)
    out = []
    for a in range(0, n, 20_000):
        m = min(20_000, n - a)
        t = zipf_words(rng, v, 220 * m)
        u = rng.random(220 * m)
        pick = (t + v * np.where(u < 0.005, 2, np.where(u < 0.05, 1, 0))).reshape(m, 220)
        out += [" ".join(words[row].tolist()) + f". doc{a + i}" for i, row in enumerate(pick)]
    return out


def median_ms(fn, rounds, setup=None):
    took, last = [], None
    for _ in range(rounds):
        arg = setup() if setup else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = fn(arg) if setup else fn()
        torch.cuda.synchronize()
        took.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(took), last


class ReadBacks:
    """Counts the host read-backs of device tensors inside a ``with`` block."""
    NAMES = ("cpu", "item", "tolist")

    def __enter__(self):
        self.count = 0
        self.saved = {n: getattr(torch.Tensor, n) for n in self.NAMES}
        for n, fn in self.saved.items():
            def counted(t, *a, _fn=fn, **kw):
                if t.is_cuda:
                    self.count += 1
                return _fn(t, *a, **kw)
            setattr(torch.Tensor, n, counted)
        return self

    def __exit__(self, *exc):
        for n, fn in self.saved.items():
            setattr(torch.Tensor, n, fn)


def events_ms(fn, rounds, reps=10):
    for _ in range(3):
        fn()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=10000)
    ap.add_argument("--bulk", type=int, default=200000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_text_ingest needs the GPU: nothing is measured without one")
    import triple_hybrid_rag_amd as T
    from triple_hybrid_rag_amd import index_build as IB
    from triple_hybrid_rag_amd.backend import GpuIndexClient
    N = T._native
    N.load()
    cus, hbm, arch = N.device_info()
    lines = []
    rng = np.random.default_rng(17)
    d, n0, m, vc = 1024, 2000, args.chunks, 20_000
    base_texts = make_chunks(rng, vc, n0, 0)
    emb = rng.standard_normal((n0 + m, d)).astype(np.float32)

    def rows_of(texts, first):
        return [{"id": f"c{first + i}", "parent_id": "p0", "document_id": "d0", "text": t, "page": 1, "modality": "text",
                 "embedding_1024": emb[first + i], "org_id": "org"} for i, t in enumerate(texts)]
    parents = [{"id": "p0", "text": "parent", "section_heading": "S"}]
    base = rows_of(base_texts, 0)
    batch = rows_of(make_chunks(rng, vc, m, n0), n0)
    texts = [r["text"] for r in batch]
    kb = sum(len(t.encode()) for t in texts) / m / 1e3

    def client(**kw):
        hi = IB.from_rows(base, parents)
        return GpuIndexClient(hi.to_gpu(), hi.store, org_id="org", device_text=True, **kw)

    # ---- insert_children, a fresh pair of clients per round
    took = {}
    for name, kw in (("text_rows", {}), ("numbered", {"number_on_device": True})):
        client(**kw).insert_children(batch)          # (warm-up: workspaces, the allocator)
        took[name], c = median_ms(lambda c: (c.insert_children(batch), c)[1], args.rounds, setup=lambda kw=kw: client(**kw))
        took[name + "_client"] = c
    a, b = took["text_rows_client"], took["numbered_client"]
    v_after = len(b.store.vocab)
    if list(a.store.vocab.items()) != list(b.store.vocab.items()) or \
            not all(torch.equal(a.index.lex[k], b.index.lex[k]) for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf")):
        sys.exit("insert path: the two routes left different indexes")

    # ---- the text step alone, on a client that is never inserted into
    c = client()
    idx = c.index
    v_before = len(c.store.vocab)

    def step_host():
        R = idx.number_text_rows(texts, on_device=False)
        return R.doc, R.term, R.pending.terms

    def step_device():
        R = idx.number_text_rows(texts)
        return R.doc, R.term, R.pending.terms        # (the strings: what store.vocab.update needs)
    host_ms, H = median_ms(step_host, args.rounds)
    dev_ms, D = median_ms(step_device, args.rounds)
    if not (torch.equal(H[0], D[0]) and torch.equal(H[1], D[1]) and H[2] == D[2]):
        sys.exit("text step: the two routes number differently")
    with ReadBacks() as rb_host:
        step_host()
    with ReadBacks() as rb_dev:
        step_device()
    # the kernels alone, over pre-uploaded inputs
    X = idx.text
    rows = idx._text_tokens(texts)
    n_total, n_unknown = int(rows["n_total"].item()), int(rows["n_unknown"].item())
    n_bytes = int(rows["ptr"][-1])
    tokens_ms = events_ms(lambda: N.text_tokens(rows["bytes_dev"], rows["ptr_dev"], n_bytes, X["table_dev"], X["slots"],
                                                X["term_bytes"], X["term_ptr"], workspace=idx._ws_text), args.rounds)
    term = rows["term"][:n_total].clone()
    ws = torch.empty(N.vocab_grow_workspace_bytes(n_unknown), dtype=torch.uint8, device=idx.device)
    fresh = rows["term"][:n_total].clone()

    def grow():
        term.copy_(fresh)           # (the -1 rows again: the patch has the same work every time)
        return N.vocab_grow(rows["bytes_dev"], rows["ptr_dev"], n_bytes, X["table_dev"], rows, n_unknown, v_before,
                            term=term, workspace=ws)
    grow_ms = events_ms(grow, args.rounds)
    lines += [f"### Insert: {m:,} chunks of {kb:.2f} KB through `insert_children` (index of {n0:,} rows, dim {d})", "",
              f"- `device_text=True` (the parent commit's route: `text_rows` + the host numbering): "
              f"**{took['text_rows']:.0f} ms** per call",
              f"- `device_text=True, number_on_device=True`: **{took['numbered']:.0f} ms** per call "
              f"({took['text_rows'] / took['numbered']:.2f}x)",
              f"- the text step alone: `text_rows` + numbering + patch upload {host_ms:.1f} ms; `number_text_rows` + the "
              f"new terms' strings {dev_ms:.1f} ms ({host_ms / dev_ms:.1f}x)",
              f"- kernels alone (device events, median of {args.rounds} rounds of 10): thr_text_tokens {tokens_ms:.3f} ms, "
              f"thr_vocab_grow with the tok_term patch {grow_ms:.3f} ms "
              f"({n_total:,} tokens, {n_unknown:,} unknown occurrences, {v_after - v_before:,} new terms)",
              f"- host read-backs of one batch (text step): {rb_host.count} on the `text_rows` route, {rb_dev.count} on the "
              "device route (the counts; n_new / n_new_bytes / status; the key blob and its pointers)",
              f"- new terms in the batch: {v_after - v_before:,} on top of {v_before:,}; vocabulary, CSR, document "
              "lengths and idf equal after both", ""]
    print("\n".join(lines), flush=True)
    del a, b, c, idx, took, rows, term, ws, emb, base, batch
    torch.cuda.empty_cache()

    # ---- bulk build, lexical part (rows without embeddings)
    if args.bulk:
        t0 = time.perf_counter()
        bulk = bulk_chunks(np.random.default_rng(23), vc, args.bulk)
        gen_s = time.perf_counter() - t0
        rows = [{"id": i, "text": t} for i, t in enumerate(bulk)]
        mb = sum(map(len, bulk)) / 1e6
        IB.from_rows(rows[:2000], device="text")
        res = {}
        for name, mode in (("text", "text"), ("true", True)):
            res[name] = median_ms(lambda mode=mode: IB.from_rows(rows, device=mode), args.rounds)
        (text_ms, A), (true_ms, B) = res["text"], res["true"]
        same = list(A.store.vocab.items()) == list(B.store.vocab.items()) and \
            all(getattr(A, k).tobytes() == getattr(B, k).tobytes() for k in ("rowptr", "post_doc", "post_tf", "doclen", "idf"))
        if not same:
            sys.exit("bulk build: the two routes built different indexes")
        lines += [f"### Bulk build: {args.bulk:,} chunks ({mb:.0f} MB of text, generated in {gen_s:.0f} s) through "
                  "`from_rows()`, rows without embeddings", "",
                  f"- `device=True` (host tokenizer per chunk, pandas factorize, thr_lexical_build): **{true_ms / 1e3:.2f} s**",
                  f"- `device=\"text\"` (batches of 64 MiB: thr_text_tokens, thr_vocab_grow, thr_vocab_insert, then "
                  f"thr_lexical_build): **{text_ms / 1e3:.2f} s** ({true_ms / text_ms:.1f}x)",
                  f"- {len(A.store.vocab):,} terms, {len(A.post_doc):,} postings; vocabulary and every lexical array equal", ""]
        print("\n".join(lines[-5:]), flush=True)
    lines += ["### Not measured", "",
              "Hardware counters of the new kernels; the cost of same-address atomics when one new token fills a batch "
              "(a per-wave pre-merge is not built); the scratch table's size and zeroing against a sort-based dedupe.", ""]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("# Numbering new BM25 terms on the device: inserts and bulk builds from text\n\n"
                    f"`python scripts/bench_text_ingest.py --chunks {args.chunks} --bulk {args.bulk}` on "
                    f"{arch} ({cus} CUs, {hbm / 2 ** 30:.0f} GiB), {os.cpu_count()} host CPUs visible (one used), "
                    f"Python {sys.version.split()[0]}, {time.strftime('%Y-%m-%d')}; "
                    f"wall-clock medians of {args.rounds}.  All routes ran in this one process on one GPU.\n\n"
                    + "\n".join(lines))


if __name__ == "__main__":
    main()
