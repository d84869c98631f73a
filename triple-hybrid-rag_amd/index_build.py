"""Index build / ingest boundary (the step BEFORE the path).

Turns the rows the reference's ingestion writes -- ``rag_child_chunks(id, parent_id,
document_id, text, page, modality, embedding_1024)``, ``rag_parent_chunks(id, text,
section_heading)``, ``rag_entities(id, name)``, ``rag_relations(subject_entity_id,
object_entity_id, confidence)``, ``rag_entity_mentions(entity_id, child_chunk_id[,
confidence])`` (database/migrations/20260114_rag2_schema.sql:104-283;
src/voice_agent/rag2/ingest.py:361-470) -- into the GPU-resident arrays / CSRs and the host
row store, and saves / loads them as a directory of ``.npy`` files + one JSON.

Two routes to the lexical index.  ``build_lexical`` is host numpy (what runs without a GPU:
small corpora, the CPU tests).  ``from_rows(..., device=True)`` / ``lexical_rows`` +
``GpuIndex.set_lexical_rows`` tokenise at C speed on the host (one regex pass per chunk, one
hash factorisation of all tokens) and build the CSR ON THE DEVICE (thr_lexical_build: radix sort
of the (term, doc) pairs, segmented reduce, row pointers by binary search) -- a 1M-chunk shard's
32M postings in well under a second; document shards all-reduce their df / length sums for the
global idf / avgdl.  ``save`` writes, next to the source arrays, what index set-up computed on
the device (``GpuIndex.export_derived``: the float16 image of the rows, the BM25 bounds /
impacts / dense-term rows) and ``load(...).to_gpu()`` reuses them; the row payloads live in
blob + offset files (``StringColumn``), not in ``meta.json``.
"""
from __future__ import annotations

import json
import os
import weakref
from dataclasses import dataclass
from typing import Any, Callable, Dict, Iterable, List, Optional, Sequence

import numpy as np

from .index_text import tokenize
from .store import CorpusStore

K1, B = 1.2, 0.75


@dataclass
class HostIndex:
    """Everything an index holds, on the host (numpy), ready for ``to_gpu``."""
    docs: np.ndarray                      # f32 [n, D]
    rowptr: Optional[np.ndarray] = None   # lexical CSR
    post_doc: Optional[np.ndarray] = None
    post_tf: Optional[np.ndarray] = None
    doclen: Optional[np.ndarray] = None
    idf: Optional[np.ndarray] = None
    avgdl: float = 0.0
    ent_rowptr: Optional[np.ndarray] = None
    ent_col: Optional[np.ndarray] = None
    men_rowptr: Optional[np.ndarray] = None
    men_chunk: Optional[np.ndarray] = None
    men_conf: Optional[np.ndarray] = None
    tokens: Optional[np.ndarray] = None   # f16 [n, T, 128]
    store: Optional[CorpusStore] = None
    derived: Optional[Dict[str, Any]] = None   # GpuIndex.export_derived(): saved with the index, reused by to_gpu()
    attributes: Optional[Dict[str, np.ndarray]] = None   # per-row int32 columns a scope tests (GpuIndex.set_attributes)

    def fp8_image(self):
        """(codes, scales) of a saved FP8 token store that belongs to these rows, or None."""
        d = self.derived or {}
        codes, scales = d.get("tokens_fp8"), d.get("token_scales")
        if codes is None or scales is None or len(codes) != len(self.docs) or tuple(scales.shape) != tuple(codes.shape[:2]):
            return None
        return codes, scales

    def to_gpu(self, doc_base: int = 0, shortlist: str = "auto", token_store: str = "f16"):
        """``shortlist``: GpuIndex.set_dense's -- "f16-anydim" puts a 1536-d or the 4000-d legacy store
        on the f16 matrix cores, where "auto" scores every row in float64.
        ``token_store``: GpuIndex.set_tokens' ``store``.  "fp8" takes the E4M3 image a save wrote
        (``save(hi, path, gpu_index=)`` of an index with an FP8 store) as it is -- ``tokens`` may then be
        None: a deployment need never hold the float16 tokens -- and quantises ``tokens`` on the device
        when there is no image."""
        from .index import GpuIndex
        if token_store not in GpuIndex.TOKEN_STORES:
            raise ValueError(f"to_gpu: token_store must be one of {list(GpuIndex.TOKEN_STORES)}, got {token_store!r}")
        image = self.fp8_image() if token_store == "fp8" else None
        if token_store == "fp8":     # refused before a device is asked for
            if image is None and self.tokens is None:
                raise ValueError("to_gpu(token_store='fp8'): this index has neither token matrices nor a saved FP8 image")
            GpuIndex._check_token_store("to_gpu", "fp8", image[0] if image is not None else self.tokens)
        idx = GpuIndex(doc_base=doc_base).set_dense(self.docs, shortlist=shortlist, derived=self.derived)
        if self.rowptr is not None:
            idx.set_lexical(self.rowptr, self.post_doc, self.post_tf, self.doclen, self.idf,
                            self.avgdl, K1, B, derived=self.derived)
        if self.ent_rowptr is not None:
            idx.set_graph(self.ent_rowptr, self.ent_col, self.men_rowptr, self.men_chunk,
                          self.men_conf)
        if image is not None:
            idx.set_tokens_fp8(*image)
        elif self.tokens is not None:
            idx.set_tokens(self.tokens, store=token_store)
        if self.attributes:
            idx.set_attributes(self.attributes)
        return idx


class StringColumn(Sequence):
    """A column of strings as ONE utf-8 blob + int64 offsets (memory-mapped when loaded): what a
    10M-row store keeps instead of ten million Python objects in a JSON file.  Decodes on access."""

    def __init__(self, blob, offsets):
        self.blob, self.offsets = blob, offsets

    @classmethod
    def from_strings(cls, values: Sequence[Optional[str]]) -> "StringColumn":
        enc = [b"\x00" if v is None else str(v).encode("utf-8") for v in values]   # (NUL alone = None)
        off = np.zeros(len(enc) + 1, dtype=np.int64)
        np.cumsum(np.fromiter(map(len, enc), dtype=np.int64, count=len(enc)), out=off[1:])
        return cls(np.frombuffer(b"".join(enc), dtype=np.uint8), off)

    def __len__(self):
        return len(self.offsets) - 1

    def __getitem__(self, i):
        if isinstance(i, slice):
            return [self[j] for j in range(*i.indices(len(self)))]
        if i < 0:
            i += len(self)
        raw = bytes(self.blob[int(self.offsets[i]):int(self.offsets[i + 1])])
        return None if raw == b"\x00" else raw.decode("utf-8")

    def __eq__(self, other):
        return len(self) == len(other) and all(a == b for a, b in zip(self, other))

    __hash__ = None


def lexical_rows(texts: Sequence[str], tokenizer: Callable[[str], List[str]] = tokenize,
                 vocab: Optional[Dict[str, int]] = None):
    """Texts -> (vocab, doc int32 [n_tokens], term int32 [n_tokens]): one entry per token
    occurrence, term -1 for a token outside a given ``vocab`` (it still counts toward its chunk's
    length).  One tokenizer call per chunk, then array work: a new vocabulary numbers the tokens in
    order of first appearance (pandas' hash factorisation), exactly as ``build_lexical`` does."""
    import itertools
    per_doc = [tokenizer(t) for t in texts]
    lens = np.fromiter(map(len, per_doc), dtype=np.int64, count=len(per_doc))
    flat = list(itertools.chain.from_iterable(per_doc))
    doc = np.repeat(np.arange(len(per_doc), dtype=np.int32), lens)
    if vocab is None:
        import pandas as pd
        codes, uniques = pd.factorize(np.asarray(flat, dtype=object)) if flat else (np.zeros(0, np.int64), [])
        return {tok: i for i, tok in enumerate(uniques)}, doc, codes.astype(np.int32)
    term = np.fromiter((vocab.get(t, -1) for t in flat), dtype=np.int32, count=len(flat))
    return vocab, doc, term


def lexical_rows_device(texts: Sequence[str], tokenizer: Callable[[str], List[str]] = tokenize,
                        batch_bytes: int = 64 << 20):
    """``lexical_rows`` for a fresh vocabulary with the text itself on the device -> (vocab, doc int32
    [n_tokens], term int32 [n_tokens]), the two arrays DEVICE tensors.  The texts go through
    ``GpuIndex.number_text_rows`` / ``commit_vocabulary`` in batches of at most ``batch_bytes`` of UTF-8 (a
    longer text is a batch of its own), from an empty vocabulary: every token is new at its first sighting
    and gets the next id there, the numbering of ``lexical_rows`` / ``build_lexical``.  A batch with an
    exceptional text is answered on the host (number_text_rows says when).  The vocabulary's strings are
    decoded once, from the final key store."""
    import torch
    from .index import GpuIndex
    from .index_text import decode_keys, pack_encoded, tokenizer_table
    table = tokenizer_table(tokenizer, "from_rows(device=\"text\")")
    if batch_bytes < 1:
        raise ValueError("from_rows(device=\"text\"): batch_bytes is at least 1")
    idx = GpuIndex().set_vocabulary([], table)
    enc = [t.encode("utf-8", "surrogatepass") for t in texts]
    docs, terms = [], []
    a = 0
    while a < len(enc):
        b, size = a + 1, len(enc[a])
        while b < len(enc) and size + len(enc[b]) <= batch_bytes:
            size += len(enc[b])
            b += 1
        rows = idx.number_text_rows(texts[a:b], packed=pack_encoded(enc[a:b]))
        idx.commit_vocabulary(rows.pending, mirror=False)
        docs.append(rows.doc + a if a else rows.doc)
        terms.append(rows.term)
        a = b
    X = idx.text
    n_vocab = X["term_ptr"].shape[0] - 1
    vocab = {t: i for i, t in enumerate(decode_keys(X["term_bytes"][:X["n_bytes"]], X["term_ptr"]))} if n_vocab else {}
    if len(vocab) != n_vocab:
        raise RuntimeError("lexical_rows_device: the key store holds a key twice")
    empty = torch.empty(0, dtype=torch.int32, device=idx.device)
    return vocab, (torch.cat(docs) if docs else empty), (torch.cat(terms) if terms else empty.clone())


def build_lexical(texts: Sequence[str], tokenizer: Callable[[str], List[str]] = tokenize,
                  vocab: Optional[Dict[str, int]] = None, n_docs_global: Optional[int] = None,
                  df_global: Optional[np.ndarray] = None, sum_dl_global: Optional[float] = None):
    """Texts -> (vocab, rowptr, post_doc, post_tf, doclen, idf, avgdl).  For a document shard
    pass the GLOBAL ``vocab`` / ``n_docs_global`` / ``df_global`` / ``sum_dl_global`` so that
    idf and avgdl are the whole corpus's."""
    grow = vocab is None
    vocab = {} if vocab is None else vocab
    d_idx, t_idx, tfs = [], [], []
    doclen = np.zeros(len(texts), dtype=np.float32)
    for i, text in enumerate(texts):
        counts: Dict[int, int] = {}
        toks = tokenizer(text)
        doclen[i] = len(toks)
        for tok in toks:
            t = vocab.get(tok)
            if t is None:
                if not grow:
                    continue
                t = vocab[tok] = len(vocab)
            counts[t] = counts.get(t, 0) + 1
        for t, c in counts.items():
            d_idx.append(i)
            t_idx.append(t)
            tfs.append(c)
    v = len(vocab)
    d_idx = np.asarray(d_idx, dtype=np.int32)
    t_idx = np.asarray(t_idx, dtype=np.int32)
    tfs = np.asarray(tfs, dtype=np.int32)
    order = np.lexsort((d_idx, t_idx))
    df_local = np.bincount(t_idx, minlength=v).astype(np.int64)
    rowptr = np.concatenate([[0], np.cumsum(df_local)]).astype(np.int64)
    n_glob = n_docs_global if n_docs_global is not None else len(texts)
    df = (df_global if df_global is not None else df_local).astype(np.float64)
    idf = np.log(1.0 + (float(n_glob) - df + 0.5) / (df + 0.5))
    total_dl = sum_dl_global if sum_dl_global is not None else float(doclen.astype(np.float64).sum())
    avgdl = total_dl / max(n_glob, 1)
    return vocab, rowptr, d_idx[order], tfs[order], doclen, idf, (avgdl if avgdl > 0 else 1.0)


def build_graph(entity_ids: Sequence[Any], relations: Iterable[Dict[str, Any]],
                mentions: Iterable[Dict[str, Any]], chunk_index: Dict[Any, int]):
    """Entity / relation / mention rows -> (ent_rowptr, ent_col, men_rowptr, men_chunk,
    men_conf).  Relations are stored in both directions (the reference walks them
    undirected, graph_search.py:196-226); mention confidence defaults to 1.0;
    ``chunk_index`` maps child-chunk id -> GLOBAL doc index."""
    eidx = {e: i for i, e in enumerate(entity_ids)}
    n = len(eidx)
    src, dst = [], []
    for r in relations:
        a, b = eidx.get(r["subject_entity_id"]), eidx.get(r["object_entity_id"])
        if a is None or b is None or a == b:
            continue
        src += [a, b]
        dst += [b, a]
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    if len(src):
        pairs = np.unique(np.stack([src, dst], axis=1), axis=0)  # sorted by (src, dst), deduplicated
        src, dst = pairs[:, 0], pairs[:, 1]
    ent_rowptr = np.concatenate([[0], np.cumsum(np.bincount(src, minlength=n))]).astype(np.int64)
    me, mc, mw = [], [], []
    for m in mentions:
        e, c = eidx.get(m["entity_id"]), chunk_index.get(m["child_chunk_id"])
        if e is None or c is None:
            continue
        me.append(e)
        mc.append(c)
        mw.append(float(m.get("confidence", 1.0)))
    me = np.asarray(me, dtype=np.int64)
    order = np.lexsort((np.asarray(mc, dtype=np.int64), me)) if len(me) else np.zeros(0, dtype=np.int64)
    men_rowptr = np.concatenate([[0], np.cumsum(np.bincount(me, minlength=n))]).astype(np.int64)
    return (ent_rowptr, dst.astype(np.int32), men_rowptr,
            np.asarray(mc, dtype=np.int32)[order], np.asarray(mw, dtype=np.float32)[order])


def from_rows(child_rows: Sequence[Dict[str, Any]], parent_rows: Sequence[Dict[str, Any]] = (),
              entity_rows: Sequence[Dict[str, Any]] = (), relation_rows: Sequence[Dict[str, Any]] = (),
              mention_rows: Sequence[Dict[str, Any]] = (), embedding_key: str = "embedding_1024",
              tokenizer: Callable[[str], List[str]] = tokenize, doc_base: int = 0,
              device: Any = False, batch_bytes: int = 64 << 20) -> HostIndex:
    """Reference table rows -> HostIndex (+ CorpusStore).  Rows without an embedding keep a
    zero vector, i.e. are excluded from the dense channel (``embedding_1024 IS NOT NULL``).
    device=True builds the inverted index on the GPU (``lexical_rows`` + thr_lexical_build) and
    brings the arrays back for ``save``; the result equals the host route's.
    device="text" takes the chunk TEXTS to the device as well (``lexical_rows_device``): tokens, case
    folding and the numbering of the vocabulary, in batches of at most ``batch_bytes`` of UTF-8; the
    tokenizer must be ``backend.tokenize`` or a TextTable's ``.tokenize``, any other is refused by name."""
    n = len(child_rows)
    dim = next((len(r[embedding_key]) for r in child_rows if r.get(embedding_key) is not None), 0)
    docs = np.zeros((n, dim), dtype=np.float32)
    for i, r in enumerate(child_rows):
        if r.get(embedding_key) is not None:
            docs[i] = np.asarray(r[embedding_key], dtype=np.float32)
    texts = [r.get("text", "") for r in child_rows]
    if isinstance(device, str) and device != "text":
        raise ValueError(f"from_rows: device is False, True or \"text\", not {device!r}")
    if device:
        from . import _native as N
        if device == "text":
            vocab, d_dev, t_dev = lexical_rows_device(texts, tokenizer, batch_bytes)
        else:
            import torch
            vocab, d_tok, t_tok = lexical_rows(texts, tokenizer)
            dev = torch.device("cuda", torch.cuda.current_device())
            d_dev, t_dev = torch.from_numpy(d_tok).to(dev), torch.from_numpy(t_tok).to(dev)
        rowptr, pd, ptf, dl, df = (a.cpu().numpy() for a in N.lexical_build(d_dev, t_dev, None, n, max(len(vocab), 1)))
        rowptr, df = rowptr[:len(vocab) + 1], df[:len(vocab)]      # (no token at all: build_lexical's empty CSR)
        dfh = df.astype(np.float64)
        idf = np.log(1.0 + (float(n) - dfh + 0.5) / (dfh + 0.5))
        avgdl = float(dl.astype(np.float64).sum()) / max(n, 1) or 1.0
    else:
        vocab, rowptr, pd, ptf, dl, idf, avgdl = build_lexical(texts, tokenizer)
    store = CorpusStore(
        child_ids=[r["id"] for r in child_rows], parent_ids=[r.get("parent_id") for r in child_rows],
        document_ids=[r.get("document_id") for r in child_rows], texts=texts,
        pages=[r.get("page", 1) for r in child_rows],
        modalities=[r.get("modality", "text") for r in child_rows],
        parents={p["id"]: {"id": p["id"], "text": p.get("text", ""),
                           "section_heading": p.get("section_heading")} for p in parent_rows},
        collections=[r.get("collection") for r in child_rows]
        if any("collection" in r for r in child_rows) else None,
        vocab=vocab, entity_names=[e.get("name", "") for e in entity_rows], doc_base=doc_base,
        content_hashes=[r.get("content_hash") for r in child_rows]
        if any(r.get("content_hash") is not None for r in child_rows) else None,
        org_ids=[r.get("org_id") for r in child_rows] if any("org_id" in r for r in child_rows) else None,
        entity_ids=[e["id"] for e in entity_rows] if entity_rows else None,
        entity_canonical=[e.get("canonical_name") for e in entity_rows]
        if any(e.get("canonical_name") is not None for e in entity_rows) else None,
        entity_documents=[e.get("document_id") for e in entity_rows]     # (rag_entities.document_id, nullable)
        if any(e.get("document_id") is not None for e in entity_rows) else None)
    hi = HostIndex(docs=docs, rowptr=rowptr, post_doc=pd, post_tf=ptf, doclen=dl, idf=idf,
                   avgdl=avgdl, store=store)
    if entity_rows:
        cidx = {cid: doc_base + i for i, cid in enumerate(store.child_ids)}
        (hi.ent_rowptr, hi.ent_col, hi.men_rowptr, hi.men_chunk, hi.men_conf) = build_graph(
            [e["id"] for e in entity_rows], relation_rows, mention_rows, cidx)
    return hi


_ARRAYS = ("docs", "rowptr", "post_doc", "post_tf", "doclen", "idf", "ent_rowptr", "ent_col",
           "men_rowptr", "men_chunk", "men_conf", "tokens")
_DERIVED_ARRAYS = ("docs16", "term_ub", "block_ub", "post_imp", "dense_slot", "dense_imp", "dense_tf",
                   "tokens_fp8", "token_scales")    # (the last two: GpuIndex.set_tokens(store="fp8")'s image)
_DERIVED_SCALARS = ("doc_rel_err", "f16_layout", "lexical_tag", "dense_stride")
_STRING_COLUMNS = ("child_ids", "parent_ids", "document_ids", "texts", "modalities", "collections",
                   "entity_names", "content_hashes", "org_ids", "entity_ids", "entity_canonical", "entity_documents")
_NO_PAGE = np.iinfo(np.int32).min   # store_pages.npy: the SQL column is nullable (page INT)


def _mutated_since_sync(hi: HostIndex, gpu_index) -> bool:
    """True when ``gpu_index`` was appended to or deleted from since ``hi`` last held its rows: it
    was built from ``hi`` (no mutation yet), or ``refresh_from_gpu`` pulled THIS index at THIS
    mutation count.  (The row count alone does not tell: a delete followed by an append can leave
    it as it was.)"""
    count = getattr(gpu_index, "_mutations", 0)
    if not count:
        return False
    ref, seen = getattr(hi, "_synced", (None, 0))
    return ref is None or ref() is not gpu_index or seen != count


def refresh_from_gpu(hi: HostIndex, gpu_index) -> HostIndex:
    """After ``GpuIndex.append_rows`` (the ingest seam, rag2/ingest.py:361-470) or
    ``GpuIndex.delete_rows`` -- or a graph ingest, ``append_graph`` / ``append_mentions`` -- the
    device holds other rows than the HostIndex: pull the source arrays back, in place, so that
    ``hi`` -- and a ``save`` of it -- equals a build from the rows the index holds now.  The store
    is appended to and deleted from by the client (``CorpusStore.append`` / ``.delete`` /
    ``.append_entities``) and is not touched here."""
    g = gpu_index
    if g.docs is not None:
        hi.docs = g.docs.cpu().numpy()
    if g.lex is not None:
        L = g.lex
        hi.rowptr, hi.post_doc, hi.post_tf = (L[k].cpu().numpy() for k in ("rowptr", "post_doc", "post_tf"))
        hi.doclen, hi.idf, hi.avgdl = L["doclen"].cpu().numpy(), L["idf"].cpu().numpy(), float(L["avgdl"])
    if g.graph is not None:
        G = g.graph
        hi.ent_rowptr, hi.ent_col = G["ent_rowptr"].cpu().numpy(), G["ent_col"].cpu().numpy()   # (append_graph)
        hi.men_rowptr, hi.men_chunk, hi.men_conf = (G[k].cpu().numpy() for k in ("men_rowptr", "men_chunk", "men_conf"))
    if hi.tokens is not None:
        stale = len(hi.tokens) != g.n_docs
        if g.tokens_packed:
            # the packed layout cannot be pulled back: the caller keeps HostIndex.tokens in step, and a
            # token store of the right length is trusted (as before deletes existed)
            if stale:
                raise ValueError("the index keeps its token store in the packed layout only: the appended rows' "
                                 "token matrices cannot be pulled back -- append them to HostIndex.tokens (and drop "
                                 "the deleted rows' with the remap delete_rows returned) before save()")
        elif stale or _mutated_since_sync(hi, g):
            hi.tokens = g.tokens.cpu().numpy()
    names = g.attribute_names() if hasattr(g, "attribute_names") else []
    if names:
        hi.attributes = {name: g.attribute(name).cpu().numpy() for name in names}
    hi._synced = (weakref.ref(g), getattr(g, "_mutations", 0))
    hi.derived = None   # (computed for the old rows; save(hi, path, gpu_index) exports the current ones)
    return hi



def save(hi: HostIndex, path: str, gpu_index=None) -> None:
    """``gpu_index``: the GpuIndex built from ``hi`` -- what its set-up computed on the device
    (export_derived) is saved too, so that a later ``load(path).to_gpu()`` does not recompute it."""
    os.makedirs(path, exist_ok=True)
    if gpu_index is not None and (gpu_index.n_docs != len(hi.docs) or _mutated_since_sync(hi, gpu_index)):
        # rows were appended or deleted on the device (a delete followed by an append can leave the
        # row count as it was): never save the stale arrays
        refresh_from_gpu(hi, gpu_index)
    if hi.store is not None and len(hi.store.child_ids) != len(hi.docs):
        raise ValueError(f"the row store holds {len(hi.store.child_ids)} chunks, the index {len(hi.docs)}: "
                         "they were not appended to together (GpuIndexClient.insert_children / delete_children change both)")
    for name in _ARRAYS:
        arr = getattr(hi, name)
        if arr is not None:
            np.save(os.path.join(path, name + ".npy"), arr, allow_pickle=False)
    meta: Dict[str, Any] = {"avgdl": hi.avgdl, "format": 2}
    if hi.attributes:    # (optional: a directory without the key loads as before)
        names = sorted(hi.attributes)
        for i, name in enumerate(names):
            col = np.ascontiguousarray(hi.attributes[name], dtype=np.int32)
            if col.shape != (len(hi.docs),):
                raise ValueError(f"attribute {name!r}: one int32 per row ({len(hi.docs)}), got shape {col.shape}")
            np.save(os.path.join(path, f"attr_{i}.npy"), col, allow_pickle=False)
        meta["attributes"] = names
    derived = gpu_index.export_derived() if gpu_index is not None else hi.derived
    for name in _DERIVED_ARRAYS:   # a directory saved before may hold derived arrays this index does not have
        fp = os.path.join(path, "derived_" + name + ".npy")
        if derived and derived.get(name) is not None:
            np.save(fp, np.asarray(derived[name]), allow_pickle=False)
        elif os.path.exists(fp):
            os.remove(fp)
    if derived:
        meta["derived"] = {k: derived[k] for k in _DERIVED_SCALARS if derived.get(k) is not None}
    if hi.store is not None:
        s = hi.store
        columns = []
        for name in _STRING_COLUMNS:   # the big columns: blob + offsets, not JSON
            values = getattr(s, name)
            if values is None:
                continue
            col = values if isinstance(values, StringColumn) else StringColumn.from_strings(values)
            np.save(os.path.join(path, f"store_{name}_blob.npy"), np.asarray(col.blob), allow_pickle=False)
            np.save(os.path.join(path, f"store_{name}_off.npy"), np.asarray(col.offsets), allow_pickle=False)
            columns.append(name)
        np.save(os.path.join(path, "store_pages.npy"),
                np.asarray([_NO_PAGE if pg is None else pg for pg in s.pages], dtype=np.int32), allow_pickle=False)
        voc = list(s.vocab.items())
        vcol = StringColumn.from_strings([k for k, _ in voc])
        np.save(os.path.join(path, "store_vocab_blob.npy"), np.asarray(vcol.blob), allow_pickle=False)
        np.save(os.path.join(path, "store_vocab_off.npy"), np.asarray(vcol.offsets), allow_pickle=False)
        np.save(os.path.join(path, "store_vocab_ids.npy"), np.asarray([v for _, v in voc], dtype=np.int64),
                allow_pickle=False)
        meta["store"] = {"columns": columns, "parents": s.parents, "doc_base": s.doc_base}
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump(meta, f)


def load(path: str, mmap: bool = True) -> HostIndex:
    with open(os.path.join(path, "meta.json")) as f:
        meta = json.load(f)
    mode = "r" if mmap else None

    def arr(name):
        fp = os.path.join(path, name + ".npy")
        return np.load(fp, mmap_mode=mode, allow_pickle=False) if os.path.exists(fp) else None
    arrays = {name: arr(name) for name in _ARRAYS}
    derived = None
    if "derived" in meta:
        derived = dict(meta["derived"])
        derived.update({name: arr("derived_" + name) for name in _DERIVED_ARRAYS})
    store = None
    if "store" in meta:
        ms = meta["store"]
        if "columns" not in ms:    # format 1: everything in the JSON
            store = CorpusStore(**ms)
        else:
            cols = {name: StringColumn(arr(f"store_{name}_blob"), arr(f"store_{name}_off")) for name in ms["columns"]}
            vcol = StringColumn(arr("store_vocab_blob"), arr("store_vocab_off"))
            vocab = dict(zip(vcol, (int(v) for v in arr("store_vocab_ids"))))
            store = CorpusStore(child_ids=cols["child_ids"], parent_ids=cols["parent_ids"],
                                document_ids=cols["document_ids"], texts=cols["texts"],
                                pages=[None if pg == _NO_PAGE else pg for pg in arr("store_pages").tolist()],
                                modalities=cols["modalities"], parents=ms["parents"],
                                collections=cols.get("collections"), vocab=vocab,
                                entity_names=cols.get("entity_names", []), doc_base=ms["doc_base"],
                                content_hashes=cols.get("content_hashes"),
                                org_ids=cols.get("org_ids"),    # (None: a directory saved without the column)
                                entity_ids=cols.get("entity_ids"), entity_canonical=cols.get("entity_canonical"),
                                entity_documents=cols.get("entity_documents"))   # (None: saved without the column)
    attributes = {name: arr(f"attr_{i}") for i, name in enumerate(meta.get("attributes", []))} or None
    return HostIndex(avgdl=meta["avgdl"], store=store, derived=derived, attributes=attributes, **arrays)
