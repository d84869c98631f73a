"""HBM-resident retrieval index and the batched device pipeline.

``GpuIndex`` owns the tensors the HIP scorers read (one document shard per
GPU) and exposes one method per channel plus ``retrieve_batch`` -- dense ->
lexical -> graph -> weighted RRF (-> MaxSim rerank) with every stage a kernel
behind the C ABI and no host round trip between stages.  The reference has no
batch entry point (its ``retrieve()`` is one query per call,
src/voice_agent/rag2/retrieval.py:118-201); the per-query drop-in sits on top
of this in ``rag2/retrieval.py`` + ``backend.py``.

Layout in HBM (per shard of n documents, D dims):
    docs      float32 [n, D]   row-major, the only large array of the dense path
    dnorm     float64 [n]      ||d||  (sequential float64, oracle contract)
    inv_norm  float32 [n]      1/||d|| for the fp32 scan, 0 = no embedding
    lexical   CSR by term: rowptr int64 [V+1], post_doc int32, post_tf int32,
              doclen float32 [n], idf float64 [V] (global), avgdl (global)
    graph     entity CSR (replicated) + entity->chunk mention CSR (this shard's chunks)
    tokens    float16 [n, T_d, 128] late-interaction token matrices
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import functools
import logging
import os
import warnings

import numpy as np
import torch

from . import _native as N

log = logging.getLogger(__name__)


def floor_width(k: int, n_shards: int) -> int:
    """Lower bounds a shard sends per query for the common floor (thr_dense_floor): twice its fair
    share of the k best, at least 16 -- the k-th largest of the n_shards * m values is then close
    to the true k-th score unless one shard holds most of the k best."""
    m = max(16, 2 * -(-k // max(1, n_shards)))
    return max(1, min(m, N.THR_DENSE_MAX_K, 4096 // max(1, n_shards)))   # (n_shards * m values fit the band kernel's LDS)


def _refuse_when_unusable(fn):
    """A delete that failed in its in-place phase leaves rows half moved (GpuIndex.delete_rows): the
    index marks itself unusable, and no search, append or delete may run on it afterwards."""
    @functools.wraps(fn)
    def call(self, *a, **kw):
        if getattr(self, "_unusable", None):
            raise N.NativeError(self._unusable)
        return fn(self, *a, **kw)
    return call


@dataclass
class BatchResult:
    ids: torch.Tensor            # int64 [nq, top_k] fused (or reranked) global doc ids, -1 pad
    scores: torch.Tensor         # float64 [nq, top_k] RRF scores (rerank: MaxSim scores)
    counts: torch.Tensor         # int32 [nq]
    channels: Dict[str, tuple] = field(default_factory=dict)  # name -> (scores, ids, counts)
    # queries that needed the exhaustive float64 path: an int, or (batch path, so that a batch
    # needs no host synchronisation) a device int32[1] -- int(result.rescued) reads it back
    rescued: object = 0


class GpuIndex:
    def __init__(self, device: Optional[torch.device] = None, doc_base: int = 0):
        if not torch.cuda.is_available():
            raise N.NativeError("GpuIndex needs a HIP device (no CPU fallback exists)")
        N.load()
        self.device = device or torch.device("cuda", torch.cuda.current_device())
        self.doc_base = int(doc_base)
        self.n_docs = 0
        self.dim = 0
        self.docs = self.dnorm = self.inv_norm = self.docs16 = None
        self.doc_rel_err = 0.0
        self.shortlist = "f32"
        self.lex = None
        self.graph = None
        self.tokens = None
        self.doc_coll = None
        self.tokens_packed = False
        self._ws: Optional[torch.Tensor] = None
        self._ws_rescue: Optional[torch.Tensor] = None
        self._ws_lex: Optional[torch.Tensor] = None
        self._ws_graph: Optional[torch.Tensor] = None
        self._lex_done = None   # event: the last bm25_search's kernels have left the lexical workspace
        self._shortlist_auto = False   # set_dense(shortlist="auto"): an append may re-decide the flavour
        self._backing: Dict[str, torch.Tensor] = {}   # name -> buffer with spare capacity (reserve_rows / append_rows)
        self._lex_global = False    # idf / avgdl are a sharded corpus' (set_lexical_rows with a group)
        self._spare: Dict[str, torch.Tensor] = {}     # CSR payload name -> destination of the next append
        self._csr_cap: Dict[str, torch.Tensor] = {}   # CSR payload name -> the capacity buffer behind its view
        self._mutations = 0     # appends + deletes so far (index_build.save: the host arrays are stale)
        self._unusable: Optional[str] = None   # set when a delete failed while rows were moving in place

    # ------------------------------------------------------------ builders
    def _t(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        a = np.ascontiguousarray(a)
        if not a.flags.writeable:   # a memory-mapped index (index_build.load): read-only is fine,
            with warnings.catch_warnings():   # the tensor is only the source of the device copy
                warnings.simplefilter("ignore", UserWarning)
                return torch.from_numpy(a).to(device=self.device, dtype=dtype)
        return torch.from_numpy(a).to(device=self.device, dtype=dtype)

    SHORTLISTS = ("auto", "f32", "f16", "f16-inline", "exact")
    F16_DIMS = (512, 768, 1024)
    SCAN_DIMS = (256, 512, 768, 1024)   # row lengths the streaming shortlist scans are built for
    AUTO_COPY_FRACTION = 0.25    # of the device's memory: every shard the f16 scans can index (2^25 rows)
    F16_MAX_ROWS = 1 << 25       # per shard: the f16 scans pack (query-in-tile, row) in 32 bits
    F16_MAX_REL_ERR = 2e-3       # ~8x the rounding error of rows in float16's normal range
    DENSE_SHARE = 0.01           # lexical terms held by this share of the docs get per-doc rows

    def set_dense(self, docs, shortlist: str = "auto", derived: Optional[dict] = None) -> "GpuIndex":
        """How the streaming pass picks its shortlist (the returned scores are ALWAYS the float64
        rescoring of the float32 rows, and the per-query certificate covers the scan's error):
          "f32"        float32 rows on the fp32 matrix cores (32 queries per pass);
          "f16-inline" float32 rows rounded to float16 in registers, f16 matrix cores
                       (64 queries per pass, no extra memory);
          "f16"        additionally keeps a float16 copy of the rows and streams that;
          "exact"      no shortlist pass: every row scored in float64 (thr_dense_topk_exact) -- any
                       row length that is a multiple of 4;
          ``derived``: the saved float16 image of a loaded index (export_derived), reused when
                       its layout is the one this build's scan reads.
          "auto"       an f16 flavour when the dimension has an f16 kernel and every row fits the
                       float16 range -- "f16" while the copy is small next to the device's memory
                       (<= AUTO_COPY_FRACTION of it: a quarter, which covers every shard size the f16 scans
                       index), "f16-inline" beyond -- else "f32"; a row length none of the scans is
                       built for (the reference's legacy RAG 1.0 store keeps 4000-d halfvec rows,
                       src/voice_agent/config.py:216, 20260113_halfvec_4000.sql:70-105) goes to
                       "exact" with a logged warning: same bits, O(n * dim) float64 work per query."""
        if shortlist not in self.SHORTLISTS:
            raise ValueError(f"shortlist must be one of {self.SHORTLISTS}")
        self.docs = self._t(docs, torch.float32)
        self.n_docs, self.dim = self.docs.shape
        if self.dim % 4:
            raise N.NativeError(f"row length {self.dim} is not a multiple of 4")
        self.dnorm, self.inv_norm = N.doc_norms(self.docs)
        self.docs16, self.doc_rel_err = (None, 0.0)
        auto = self._shortlist_auto = shortlist == "auto"
        if self.dim not in self.SCAN_DIMS and shortlist != "exact":
            if not auto:
                raise N.NativeError(f"shortlist={shortlist!r} needs a row length in {self.SCAN_DIMS}, got "
                                    f"{self.dim}: use shortlist='exact' (or 'auto')")
            log.warning("dense rows of %d dims: no streaming scan is built for that length, every search "
                        "scores all %d rows in float64 (thr_dense_topk_exact)", self.dim, self.n_docs)
            shortlist, auto = "exact", False
        if shortlist == "exact":
            self.shortlist = shortlist
            return self
        if auto:
            shortlist = "f32"
            if self.dim in self.F16_DIMS and self.n_docs < self.F16_MAX_ROWS:
                total = torch.cuda.get_device_properties(self.device).total_memory
                copy_bytes = 2 * self.n_docs * self.dim
                shortlist = "f16" if copy_bytes <= self.AUTO_COPY_FRACTION * total else "f16-inline"
        if shortlist != "f32":
            have = derived and derived.get("docs16") is not None and shortlist == "f16" \
                and derived.get("f16_layout") == N.dense_f16_layout(self.dim)
            if have:   # (a saved index: the float16 image and its measured error come with it)
                self.docs16 = self._t(derived["docs16"], torch.float16)
                self.doc_rel_err = float(derived["doc_rel_err"])
            else:
                self.docs16, self.doc_rel_err = N.dense_quantize_f16(self.docs,
                                                                     keep_copy=shortlist == "f16")
            # float16 holds the rows when no value overflows (|v| < 65504: else the measured error
            # is +inf) and few underflow (rows scaled to ~1e-6 are all subnormals: the error bound
            # would exceed F16_MAX_REL_ERR and no query could be certified)
            if not np.isfinite(self.doc_rel_err) or self.doc_rel_err > self.F16_MAX_REL_ERR:
                if not auto:
                    raise N.NativeError("rows do not fit float16 (values >= 65504 or mostly below "
                                        "6e-5 in magnitude): use shortlist='f32'")
                shortlist, self.docs16, self.doc_rel_err = "f32", None, 0.0
        self.shortlist = shortlist
        return self

    def set_lexical(self, rowptr, post_doc, post_tf, doclen, idf, avgdl: float,
                    k1: float = 1.2, b: float = 0.75, dense_share: Optional[float] = None,
                    derived: Optional[dict] = None) -> "GpuIndex":
        """``dense_share``: a term held by at least this share of the shard's docs also gets
        per-doc rows of impacts / term frequencies (3 bytes per doc and term; 0 = none;
        default DENSE_SHARE, or the A/B knob THR_BM25_DENSE_SHARE).
        ``derived``: the saved bounds / impacts / dense rows of a loaded index (export_derived):
        reused when they were computed for the same k1, b, avgdl and dense share."""
        if dense_share is None:
            dense_share = float(os.environ.get("THR_BM25_DENSE_SHARE", self.DENSE_SHARE))
        self.lex = dict(rowptr=self._t(rowptr, torch.int64), post_doc=self._t(post_doc, torch.int32),
                        post_tf=self._t(post_tf, torch.int32), doclen=self._t(doclen, torch.float32),
                        idf=self._t(idf, torch.float64), avgdl=float(avgdl), k1=float(k1), b=float(b),
                        dense_share=float(dense_share))
        L = self.lex
        tag = [L["avgdl"], L["k1"], L["b"], L["dense_share"]]
        if derived and derived.get("term_ub") is not None and list(derived.get("lexical_tag", [])) == tag:
            L["bounds"] = (self._t(derived["term_ub"], torch.float64), self._t(derived["block_ub"], torch.float64),
                           self._t(derived["post_imp"], torch.uint8))
            L["dense"] = None
            if derived.get("dense_slot") is not None:
                L["dense"] = (self._t(derived["dense_slot"], torch.int32), self._t(derived["dense_imp"], torch.uint8),
                              self._t(derived["dense_tf"], torch.int16), int(derived["dense_stride"]))
        else:
            # per-term / per-128-posting score bounds for the WAND-style pruning of thr_bm25_topk
            L["bounds"] = N.bm25_bounds(L["rowptr"], L["post_doc"], L["post_tf"], L["doclen"], L["idf"],
                                        L["avgdl"], L["k1"], L["b"])
            L["dense"] = N.bm25_dense_terms(L["rowptr"], L["post_doc"], L["post_tf"], L["bounds"][2],
                                            int(L["doclen"].shape[0]), dense_share) if dense_share > 0 else None
        if self.n_docs == 0:
            self.n_docs = int(self.lex["doclen"].shape[0])
        return self

    def set_lexical_rows(self, doc, term, tf, n_vocab: int, n_docs: Optional[int] = None,
                         n_docs_global: Optional[int] = None, group=None, k1: float = 1.2,
                         b: float = 0.75, dense_share: Optional[float] = None) -> "GpuIndex":
        """The lexical side from tokenised ROWS, built on the device (thr_lexical_build): ``doc`` /
        ``term`` / ``tf`` int32 [n_pairs] -- one entry per distinct (doc, term) of a chunk, or one
        per token occurrence with ``tf`` None; doc ids LOCAL to this shard.  A document shard
        passes the corpus' ``n_docs_global`` and its process ``group``: the per-term document
        frequencies and the length total are all-reduced over the shards, so idf and avgdl are the
        whole corpus'  -- idf itself is float64 numpy on the host, the oracle's formula
        to the bit.  The reference leaves this step to PostgreSQL's generated tsvector column +
        GIN index (rag2_schema.sql:146-148, 171-172; rows from rag2/ingest.py:361-470)."""
        import torch.distributed as dist
        n = int(n_docs if n_docs is not None else self.n_docs)
        if n <= 0:
            raise N.NativeError("set_lexical_rows: the shard's doc count is unknown (n_docs)")
        rowptr, post_doc, post_tf, doclen, df = N.lexical_build(
            self._t(doc, torch.int32), self._t(term, torch.int32),
            None if tf is None else self._t(tf, torch.int32), n, int(n_vocab))
        sum_dl = doclen.sum(dtype=torch.float64).reshape(1)
        df_glob = df.clone()
        if group is not None or (dist.is_initialized() and n_docs_global is not None and n_docs_global != n):
            if dist.get_backend(group) == "gloo":   # (CPU rendezvous: rehearsals and tests)
                df_c, sd_c = df_glob.cpu(), sum_dl.cpu()
                dist.all_reduce(df_c, group=group)
                dist.all_reduce(sd_c, group=group)
                df_glob, sum_dl = df_c.to(self.device), sd_c.to(self.device)
            else:
                dist.all_reduce(df_glob, group=group)
                dist.all_reduce(sum_dl, group=group)
        n_glob = int(n_docs_global if n_docs_global is not None else n)
        dfh = df_glob.cpu().numpy().astype(np.float64)
        idf = np.log(1.0 + (float(n_glob) - dfh + 0.5) / (dfh + 0.5))
        avgdl = float(sum_dl.item()) / max(n_glob, 1)
        self.df_local, self.df_global = df, df_glob
        self._lex_global = group is not None or n_glob != n
        return self.set_lexical(rowptr, post_doc, post_tf, doclen, idf, avgdl if avgdl > 0 else 1.0, k1, b,
                                dense_share)

    def export_derived(self) -> dict:
        """What index set-up computed on the device and a saved index can carry along, as host
        arrays: the float16 image of the rows (+ its layout tag and measured error), the BM25
        bounds / per-posting impacts and the dense-term rows (+ the parameters they hold for)."""
        out: dict = {}
        if self.docs16 is not None and self.shortlist == "f16":
            out.update(docs16=self.docs16.cpu().numpy(), doc_rel_err=float(self.doc_rel_err),
                       f16_layout=N.dense_f16_layout(self.dim))
        if self.lex is not None:
            L = self.lex
            out.update(term_ub=L["bounds"][0].cpu().numpy(), block_ub=L["bounds"][1].cpu().numpy(),
                       post_imp=L["bounds"][2].cpu().numpy(),
                       lexical_tag=[L["avgdl"], L["k1"], L["b"], L["dense_share"]])
            if L["dense"] is not None:
                out.update(dense_slot=L["dense"][0].cpu().numpy(), dense_imp=L["dense"][1].cpu().numpy(),
                           dense_tf=L["dense"][2].cpu().numpy(), dense_stride=int(L["dense"][3]))
        return out

    def set_collections(self, doc_coll) -> "GpuIndex":
        """Per-document collection id (int32 [n], any non-negative labelling): the
        ``p_collection`` filter of the two RPCs (rag2_schema.sql:368-373, 404-408) is applied
        on the device BEFORE the ranking -- per query, -1 = unfiltered."""
        self.doc_coll = self._t(doc_coll, torch.int32)
        return self

    def set_graph(self, ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf) -> "GpuIndex":
        self.graph = dict(ent_rowptr=self._t(ent_rowptr, torch.int64),
                          ent_col=self._t(ent_col, torch.int32),
                          men_rowptr=self._t(men_rowptr, torch.int64),
                          men_chunk=self._t(men_chunk, torch.int32),
                          men_conf=self._t(men_conf, torch.float32))
        return self

    def _graph_transposed(self):
        """Chunk-major copy of this shard's mentions (the capacity-free third tier of
        thr_graph_topk), built on first use: the shard's chunk count must be known."""
        G = self.graph
        if G.get("n_chunks") != self.n_docs:
            G["n_chunks"] = self.n_docs
            G["transposed"] = N.graph_transpose_mentions(G["men_rowptr"], G["men_chunk"],
                                                         G["men_conf"], self.doc_base, self.n_docs)
        return G["transposed"]

    def set_tokens(self, dtok, pack: bool = True) -> "GpuIndex":
        """Late-interaction token store f16 [n, d_tokens, tok_dim].  pack=True keeps it in the
        fragment-major layout of thr_maxsim_pack (the row-major copy is dropped)."""
        tok = self._t(dtok, torch.float16)
        self.tokens_packed = bool(pack)
        self.tokens = N.maxsim_pack(tok) if pack else tok
        return self

    # ------------------------------------------------------------ incremental ingest
    # Append in place (DESIGN.md "Incremental ingest"): after append_rows every device array is
    # what a fresh build over all the rows would hold, so the query kernels and their throughput
    # are the fresh build's.  The reference's ingest only ever inserts (rag2/ingest.py:361-470).
    GROWTH = 1.5    # a buffer that is too small is replaced by one of GROWTH x its size (at least the need)

    def _row_arrays(self) -> Dict[str, torch.Tensor]:
        """The per-document arrays (leading dimension = rows; docs16: rows padded to tiles of 32)."""
        arrs = dict(docs=self.docs, docs16=self.docs16, dnorm=self.dnorm, inv_norm=self.inv_norm,
                    doc_coll=self.doc_coll, tokens=self.tokens,
                    doclen=self.lex["doclen"] if self.lex is not None else None)
        return {k: v for k, v in arrs.items() if v is not None}

    def _set_row_array(self, name: str, view: torch.Tensor) -> None:
        if name == "doclen":
            self.lex["doclen"] = view
        else:
            setattr(self, name, view)

    def _buffer(self, name: str, view: torch.Tensor, rows: int, capacity: Optional[int] = None) -> torch.Tensor:
        """A buffer with room for ``rows`` leading rows of array ``name`` that already holds the rows
        of ``view``: the view's own backing buffer when that has the room (the rows behind the
        view are free to write: no kernel is given more than the logical size), else a new one of
        max(rows, capacity or GROWTH x the old size) rows, the old rows copied on the device."""
        back = self._backing.get(name)
        if back is not None and back.shape[0] >= rows and back.shape[1:] == view.shape[1:] and \
                back.data_ptr() == view.data_ptr():
            return back
        cap = max(rows, capacity or int(self.GROWTH * view.shape[0]))
        buf = torch.empty((cap,) + tuple(view.shape[1:]), dtype=view.dtype, device=self.device)
        buf[:view.shape[0]].copy_(view)
        return buf

    def _sync_streams(self) -> None:
        """An append is not on the query path: queued BM25 / graph work on the side stream and
        dense work on the main one may still read the arrays about to be swapped or extended."""
        torch.cuda.current_stream(self.device).synchronize()
        if getattr(self, "_side", None) is not None:
            self._side.synchronize()
        if self._lex_done is not None:
            self._lex_done.synchronize()

    def capacity_rows(self) -> int:
        """Rows the per-document buffers hold without a reallocation (= n_docs until
        reserve_rows / the first append)."""
        caps = [self._backing[k].shape[0] if k in self._backing and self._backing[k].data_ptr() == v.data_ptr()
                else v.shape[0] for k, v in self._row_arrays().items() if k != "docs16"]
        return min(caps) if caps else 0

    def reserve_rows(self, capacity: int, postings: Optional[int] = None) -> "GpuIndex":
        """Room for ``capacity`` documents in every per-document array (rows, float16 image, norms,
        collections, lengths, token store), so that appends up to there copy nothing old;
        ``postings``: room for that many postings in the destination of the next lexical append.
        The logical sizes, and what the kernels are given, do not change."""
        capacity = int(capacity)
        if capacity > self.n_docs:
            self._sync_streams()
            for name, view in self._row_arrays().items():
                rows = (capacity + 31) // 32 * 32 if name == "docs16" else capacity
                buf = self._buffer(name, view, rows, capacity=rows)
                self._backing[name] = buf
                self._set_row_array(name, buf[:view.shape[0]])
        if postings and self.lex is not None:
            sp = self._spare
            for name in ("post_doc", "post_tf"):
                if name not in sp or sp[name].shape[0] < postings:
                    sp[name] = torch.empty(int(postings), dtype=torch.int32, device=self.device)
        return self

    @staticmethod
    def _host_or_device(a, name: str, integer: bool = False, who: str = "append_rows"):
        """``a`` where it lives, as a tensor or a numpy array (host data: no device work)."""
        t = a if isinstance(a, torch.Tensor) else np.asarray(a)
        is_int = not t.dtype.is_floating_point and t.dtype != torch.bool if isinstance(t, torch.Tensor) \
            else np.issubdtype(t.dtype, np.integer)
        if integer and not is_int:
            raise N.NativeError(f"{who}: {name} must be an integer array, got {t.dtype}")
        return t

    def _validate_append(self, docs, lex, collections, tokens, mentions, n_rows) -> dict:
        """Everything about an append that can be refused before any device work: which parts are
        required (exactly the channels the index has), shapes, dtypes, id ranges.  -> the parts as
        tensors where the caller left them + the batch size."""
        E = N.NativeError
        has_dense = self.docs is not None
        if has_dense:
            if docs is None:
                raise E("append_rows: this index has a dense channel: docs [m, dim] is required")
            docs = self._host_or_device(docs, "docs")
            if docs.ndim != 2 or docs.shape[1] != self.dim:
                raise E(f"append_rows: docs must be [m, {self.dim}], got {tuple(docs.shape)}")
            m = int(docs.shape[0])
            if n_rows is not None and int(n_rows) != m:
                raise E("append_rows: n_rows differs from the number of dense rows")
        else:
            if docs is not None:
                raise E("append_rows: this index has no dense channel (set_dense): docs must be None")
            if n_rows is None:
                raise E("append_rows: an index without a dense channel needs n_rows")
            m = int(n_rows)
        if m < 0 or self.n_docs + m > (1 << 31) - 1:
            raise E("append_rows: row count out of range")
        out = dict(m=m, docs=docs, lex=None, collections=None, tokens=None, mentions=None)
        if (self.lex is not None) != (lex is not None):
            raise E("append_rows: this index has a lexical channel: lex=(doc, term, tf, n_vocab) is required"
                    if lex is None else "append_rows: this index has no lexical channel: lex must be None")
        if lex is not None:
            if self._lex_global:
                raise E("append_rows: not supported on a document shard (idf / avgdl are the whole corpus': "
                        "the append needs a collective df / length all-reduce)")
            if len(lex) != 4:
                raise E("append_rows: lex is (doc, term, tf or None, n_vocab)")
            d, t, f, n_vocab = lex
            d, t = self._host_or_device(d, "lex doc", True), self._host_or_device(t, "lex term", True)
            f = None if f is None else self._host_or_device(f, "lex tf", True)
            n_vocab = int(n_vocab)
            if d.ndim != 1 or t.shape != d.shape or (f is not None and f.shape != d.shape):
                raise E("append_rows: lex doc / term / tf are 1-d arrays of one length")
            v_old = int(self.lex["rowptr"].shape[0]) - 1
            if n_vocab < v_old or n_vocab > (1 << 31) - 2:
                raise E(f"append_rows: n_vocab {n_vocab} is smaller than the index's vocabulary {v_old} "
                        "(term ids never move: new terms get new ids at the end)")
            if d.shape[0]:
                if int(d.min()) < 0 or int(d.max()) >= m:
                    raise E(f"append_rows: lex doc ids are local to the batch, 0 .. {m - 1}")
                if int(t.max()) >= n_vocab:
                    raise E(f"append_rows: term id {int(t.max())} >= n_vocab {n_vocab}")
            out["lex"] = (d, t, f, n_vocab)
        if (self.doc_coll is not None) != (collections is not None):
            raise E("append_rows: this index has collection ids: collections [m] is required"
                    if collections is None else "append_rows: this index has no collection ids (set_collections)")
        if collections is not None:
            c = self._host_or_device(collections, "collections", True)
            if tuple(c.shape) != (m,):
                raise E("append_rows: collections: one id per appended row")
            out["collections"] = c
        if (self.tokens is not None) != (tokens is not None):
            raise E("append_rows: this index has a token store: tokens [m, d_tokens, tok_dim] is required"
                    if tokens is None else "append_rows: this index has no token store (set_tokens)")
        if tokens is not None:
            tk = self._host_or_device(tokens, "tokens")
            if tk.ndim != 3 or tk.shape[0] != m or tuple(tk.shape[1:]) != tuple(self.tokens.shape[1:]):
                raise E(f"append_rows: tokens must be [{m}, {self.tokens.shape[1]}, {self.tokens.shape[2]}]")
            out["tokens"] = tk
        if (self.graph is not None) != (mentions is not None):
            raise E("append_rows: this index has a graph channel: mentions=(entity, chunk, conf) is required "
                    "(empty arrays when the new chunks mention nothing)"
                    if mentions is None else "append_rows: this index has no graph channel (set_graph)")
        if mentions is not None:
            if len(mentions) != 3:
                raise E("append_rows: mentions is (entity, chunk, conf or None)")
            e, c, w = mentions
            e, c = self._host_or_device(e, "mention entity", True), self._host_or_device(c, "mention chunk", True)
            w = None if w is None else self._host_or_device(w, "mention conf")
            if e.ndim != 1 or c.shape != e.shape or (w is not None and w.shape != e.shape):
                raise E("append_rows: mention entity / chunk / conf are 1-d arrays of one length")
            n_ent = int(self.graph["men_rowptr"].shape[0]) - 1
            if e.shape[0]:
                if int(e.min()) < 0 or int(e.max()) >= n_ent:
                    raise E(f"append_rows: mention entity ids must be existing entities, 0 .. {n_ent - 1} "
                            "(new entities need set_graph)")
                if int(c.min()) < 0 or int(c.max()) >= m:
                    raise E(f"append_rows: mention chunk ids are local to the batch, 0 .. {m - 1}")
            out["mentions"] = (e, c, w)
        return out

    def _dense_flavour_after(self, new: torch.Tensor, n_new: int):
        """What set_dense would decide for the rows so far + ``new``, without touching the index:
        -> (shortlist, float16 image of the tail tiles or None, doc_rel_err, first row of the tail)."""
        n_old, cur = self.n_docs, self.shortlist
        t0 = n_old // 32 * 32     # the last partially filled tile of 32 rows is re-quantised
        if cur not in ("f16", "f16-inline"):
            return cur, None, self.doc_rel_err, t0
        want = cur
        if self._shortlist_auto:
            total = torch.cuda.get_device_properties(self.device).total_memory
            fits = cur == "f16" and 2 * n_new * self.dim <= self.AUTO_COPY_FRACTION * total
            want = "f32" if n_new >= self.F16_MAX_ROWS else ("f16" if fits else "f16-inline")
        tail16, err = None, 0.0
        if want == "f16":         # (cur is "f16": growth never shrinks the copy)
            tail16, e = N.dense_quantize_f16(torch.cat([self.docs[t0:n_old], new]), keep_copy=True)
            err = max(self.doc_rel_err, e)
        elif want == "f16-inline":
            _, err = N.dense_quantize_f16(new, keep_copy=False)
            # (the copy's error is measured on the normalised rows: the in-flight rounding's is not)
            old = self.doc_rel_err if cur == "f16-inline" else N.dense_quantize_f16(self.docs, keep_copy=False)[1]
            err = max(err, old)
        if want != "f32" and (not np.isfinite(err) or err > self.F16_MAX_REL_ERR):
            if not self._shortlist_auto:
                raise N.NativeError("append_rows: the new rows do not fit float16 (values >= 65504 or mostly "
                                    "below 6e-5 in magnitude): build the index with shortlist='f32'")
            want = "f32"
        if want == "f32":
            tail16, err = None, 0.0
        return want, tail16, err, t0

    @_refuse_when_unusable
    def append_rows(self, docs, lex=None, collections=None, tokens=None, mentions=None,
                    n_rows: Optional[int] = None) -> range:
        """Append m chunks to the live index -> the range of their LOCAL doc ids (add doc_base for
        the global ones).  Afterwards every device array is, to the bit, what a fresh build over
        all the rows would hold, and the next search sees the rows.
          docs        float32 [m, dim] (row without an embedding: zeros);
          lex         (doc, term, tf or None, n_vocab): the tokenised rows as set_lexical_rows
                      takes them, doc ids LOCAL TO THE BATCH (0 .. m-1); term ids of the index's
                      vocabulary, new terms numbered from the old vocabulary size on
                      (n_vocab >= the old one); a negative term is a token outside the
                      vocabulary (counts toward its chunk's length only);
          collections int32 [m];   tokens float16 [m, d_tokens, tok_dim];
          mentions    (entity, chunk, conf or None): entity ids of EXISTING entities, chunk ids
                      local to the batch, in any order (stored by entity, then chunk, stably: the
                      order index_build.build_graph gives the same rows).
        Each part is required exactly when the index has that channel.  Everything is validated
        before the first change and the new arrays are swapped in last: a failure leaves the index
        answering over the old rows.  Synchronises the main and the side stream (not a query-path
        call).  Not supported on a document shard of a sharded index."""
        P = self._validate_append(docs, lex, collections, tokens, mentions, n_rows)
        m, n_old = P["m"], self.n_docs
        if m == 0:
            return range(n_old, n_old)
        n_new = n_old + m
        new = {}          # name -> (buffer, logical rows): swapped in at the end
        state = {}
        # ---- dense rows: norms of the new rows, float16 image of the tail tiles
        if self.docs is not None:
            rows = self._t(P["docs"], torch.float32)
            want, tail16, err, t0 = self._dense_flavour_after(rows, n_new)
            dn, inv = N.doc_norms(rows)
            self._sync_streams()
            for name, view, tail in (("docs", self.docs, rows), ("dnorm", self.dnorm, dn), ("inv_norm", self.inv_norm, inv)):
                buf = self._buffer(name, view, n_new)
                buf[n_old:n_new].copy_(tail)
                new[name] = (buf, n_new)
            state.update(shortlist=want, doc_rel_err=err)
        else:
            self._sync_streams()
            want, tail16 = None, None
        if P["collections"] is not None:
            buf = self._buffer("doc_coll", self.doc_coll, n_new)
            buf[n_old:n_new].copy_(self._t(P["collections"], torch.int32))
            new["doc_coll"] = (buf, n_new)
        if P["tokens"] is not None:
            tok = self._t(P["tokens"], torch.float16)
            buf = self._buffer("tokens", self.tokens, n_new)
            buf[n_old:n_new].copy_(N.maxsim_pack(tok) if self.tokens_packed else tok)   # (the layout is doc-local)
            new["tokens"] = (buf, n_new)
        dest = {}         # CSR payload name -> the capacity buffer it was appended into
        lex_new = self._append_lexical(P["lex"], n_old, n_new, new, dest) if P["lex"] is not None else None
        graph_new = self._append_mentions(P["mentions"], n_old, dest) if P["mentions"] is not None else None
        if tail16 is not None:    # last: the one write that lands inside the old logical extent
            rows16 = (n_new + 31) // 32 * 32    # (the old last tile's NaN padding becomes rows)
            buf = self._buffer("docs16", self.docs16, rows16)
            buf[t0:rows16].copy_(tail16)
            new["docs16"] = (buf, rows16)
        # ---- swap
        # the buffers the CSRs were read from become the destinations of the next append
        old = dict(self.lex or {}, **(self.graph or {}))
        cap = self._csr_cap
        self._spare = {k: cap[k] if k in cap and cap[k].data_ptr() == old[k].data_ptr() else old[k] for k in dest}
        self._csr_cap = dest
        if lex_new is not None:
            self.lex = lex_new
            self.df_local = self.df_global = lex_new.pop("df")
        if graph_new is not None:
            self.graph = graph_new
        for name, (buf, n) in new.items():
            self._backing[name] = buf
            self._set_row_array(name, buf[:n])
        if self.docs is not None:
            self.shortlist, self.doc_rel_err = state["shortlist"], state["doc_rel_err"]
            if self.shortlist not in ("f16",):
                self.docs16 = None
                self._backing.pop("docs16", None)
        self.n_docs = n_new
        # sized or cached for the old row count: the dense workspace (the threshold sample grows
        # with n), the candidate lists of a pending dense_shortlist
        self._ws = None
        self._shortlist_of = None
        self._mutations += 1
        torch.cuda.current_stream(self.device).synchronize()
        return range(n_old, n_new)

    def _csr_dest(self, name: str, like: torch.Tensor, nnz_new: int) -> torch.Tensor:
        """Destination of a CSR append (out of place): the buffer the previous append read from
        when it has the room, else a new one of max(need, GROWTH x the old size) elements."""
        sp = self._spare.get(name)
        if sp is not None and sp.shape[0] >= nnz_new and sp.dtype == like.dtype and sp.data_ptr() != like.data_ptr():
            return sp
        return torch.empty(max(nnz_new, int(self.GROWTH * like.shape[0])), dtype=like.dtype, device=self.device)

    def _append_lexical(self, lex, n_old: int, n_new: int, new: dict, dest: dict) -> dict:
        """The lexical side after the append, as a new ``self.lex`` dict (the old one is untouched)."""
        d, t, f, n_vocab = lex
        L = self.lex
        # the delta CSR over the new rows, doc ids already in the index's numbering: no sort of old postings
        rp_b, pd_b, ptf_b, dl_full, df_b = N.lexical_build(
            self._t(d, torch.int32) + n_old, self._t(t, torch.int32),
            None if f is None else self._t(f, torch.int32), n_new, n_vocab)
        nnz = L["post_doc"].shape[0] + pd_b.shape[0]
        rowptr, post_doc, post_tf, _ = N.csr_append(
            L["rowptr"], L["post_doc"], L["post_tf"], rp_b, pd_b, ptf_b,
            self._csr_dest("post_doc", L["post_doc"], nnz), self._csr_dest("post_tf", L["post_tf"], nnz))
        dest.update(post_doc=post_doc, post_tf=post_tf)
        post_doc, post_tf = post_doc[:nnz], post_tf[:nnz]
        doclen_buf = self._buffer("doclen", L["doclen"], n_new)
        doclen_buf[n_old:n_new].copy_(dl_full[n_old:n_new])
        doclen = doclen_buf[:n_new]
        out = self._lexical_derived(rowptr, post_doc, post_tf, doclen, n_new)
        # (doclen is swapped in with the dict: only its backing buffer is noted among the row arrays)
        new["doclen"] = (doclen_buf, n_new)
        return out

    def _lexical_derived(self, rowptr, post_doc, post_tf, doclen, n_new: int) -> dict:
        """What follows a changed CSR (an append's or a delete's), as a new ``self.lex`` dict + "df":
        df from the row pointers, idf / avgdl as set_lexical_rows computes them, the pruning bounds
        and the dense-term rows for the new row count."""
        L = self.lex
        # idf / avgdl as set_lexical_rows computes them: float64 numpy on the host from the device's df
        df = rowptr[1:] - rowptr[:-1]
        dfh = df.cpu().numpy().astype(np.float64)
        idf = np.log(1.0 + (float(n_new) - dfh + 0.5) / (dfh + 0.5))
        avgdl = float(doclen.sum(dtype=torch.float64).item()) / max(n_new, 1)
        out = dict(rowptr=rowptr, post_doc=post_doc, post_tf=post_tf, doclen=doclen,
                   idf=self._t(idf, torch.float64), avgdl=avgdl if avgdl > 0 else 1.0, k1=L["k1"], b=L["b"],
                   dense_share=L["dense_share"])
        out["bounds"] = N.bm25_bounds(rowptr, post_doc, post_tf, doclen, out["idf"], out["avgdl"], out["k1"], out["b"])
        out["dense"] = N.bm25_dense_terms(rowptr, post_doc, post_tf, out["bounds"][2], n_new, out["dense_share"]) \
            if out["dense_share"] > 0 else None
        out["df"] = df
        return out

    def _append_mentions(self, mentions, n_old: int, dest: dict) -> dict:
        """The graph side after the append (entity CSR unchanged; the chunk-major copy of the
        mentions is rebuilt on next use, as after set_graph)."""
        e, c, w = mentions
        G = self.graph
        n_ent = G["men_rowptr"].shape[0] - 1
        e = self._t(e, torch.int64)
        c = self._t(c, torch.int64)
        w = torch.ones(e.shape[0], dtype=torch.float32, device=self.device) if w is None else self._t(w, torch.float32)
        # the batch's mentions in the build's order: by entity, then chunk, stably
        order = torch.sort(c, stable=True).indices
        order = order[torch.sort(e[order], stable=True).indices]
        rp_b = torch.zeros(n_ent + 1, dtype=torch.int64, device=self.device)
        rp_b[1:] = torch.cumsum(torch.bincount(e, minlength=n_ent), 0)
        mc_b = (c[order] + (self.doc_base + n_old)).to(torch.int32).contiguous()
        mw_b = w[order].contiguous()
        nnz = G["men_chunk"].shape[0] + mc_b.shape[0]
        rowptr, mc, mw, _ = N.csr_append(G["men_rowptr"], G["men_chunk"], G["men_conf"], rp_b, mc_b, mw_b,
                                         self._csr_dest("men_chunk", G["men_chunk"], nnz),
                                         self._csr_dest("men_conf", G["men_conf"], nnz))
        dest.update(men_chunk=mc, men_conf=mw)
        return dict(ent_rowptr=G["ent_rowptr"], ent_col=G["ent_col"], men_rowptr=rowptr,
                    men_chunk=mc[:nnz], men_conf=mw[:nnz])

    # ------------------------------------------------------------ delete
    # Delete in place (DESIGN.md "Delete in place"): after delete_rows every device array is what a
    # fresh build over the surviving rows, in their old order, would hold -- the delete pays, the query
    # path does not change.  The store this index stands in for deletes by cascade
    # (20260114_rag2_schema.sql:65-66, 106-108, 187, 217-218; tests/test_rag2_e2e.py:276-293).
    STAGING_BYTES = 256 << 20    # the large per-row arrays are compacted through a buffer of at most this size

    def _own_buffer(self, name: str, view: torch.Tensor) -> torch.Tensor:
        """The capacity buffer behind ``view`` (reserve_rows / append_rows), or the view itself."""
        back = self._backing.get(name)
        if back is not None and back.data_ptr() == view.data_ptr() and back.shape[1:] == view.shape[1:] and \
                back.shape[0] >= view.shape[0]:
            return back
        return view

    def _compact_dest(self, name: str, like: torch.Tensor) -> torch.Tensor:
        """Destination of a CSR compaction (out of place, room for every old entry: the kept count
        is the kernel's result): the spare buffer of the last append or delete when it has the room."""
        sp = self._spare.get(name)
        if sp is not None and sp.shape[0] >= like.shape[0] and sp.dtype == like.dtype and sp.data_ptr() != like.data_ptr():
            return sp
        return torch.empty(like.shape[0], dtype=like.dtype, device=self.device)

    @_refuse_when_unusable
    def delete_rows(self, ids) -> torch.Tensor:
        """Delete chunks from the live index -> the int32 [n_old] remap on the device: old LOCAL
        doc id -> new local id, -1 = deleted.  ``ids``: local doc ids, host or device, any order,
        repeats allowed.  The survivors keep their order and are renumbered 0 .. n' - 1; afterwards
        every device array is, to the bit, what a fresh build over the surviving rows would hold
        (same vocabulary size, entity set and shortlist flavour: a term or entity whose list empties
        keeps its id, and "auto" is not re-decided on the smaller row count), and the next search
        no longer sees the rows.  An update is a delete followed by an append.

        Two phases.  Phase 1 does everything that can fail -- validation (integer ids inside
        [0, n_docs), at least one survivor: deleting every row is refused, build a new index),
        every allocation (the CSR destinations, the staging buffer, the bounds and dense-term
        rows), thr_csr_compact over the postings and the mentions, the new idf / avgdl / bounds,
        the small per-row arrays (norms, collections, lengths) gathered out of place -- and touches
        nothing a query reads: a failure there leaves the index answering over the old rows.
        Phase 2 only copies inside buffers that already exist: the float32 rows and the token
        store are compacted IN PLACE from the first deleted row on, in ascending chunks through
        the staging buffer (every source row lies at or behind its destination, so nothing is read
        after it was overwritten), the float16 image is re-quantised from the tile of the first
        deleted row on; then the new views and the row count are swapped in.  It allocates
        no device memory (every buffer it writes, the error slots included, exists by then).  An exception out of phase 2 (a HIP error) leaves rows half moved: the index marks
        itself unusable and every later search, append or delete raises.

        Synchronises the main and the side stream first (not a query-path call): a query running
        concurrently on another stream is excluded by that, exactly as for the float16 tail write
        of append_rows.  The backing buffers keep their capacity for later appends.  Not supported
        on a document shard of a sharded index."""
        E = N.NativeError
        n_old = self.n_docs
        if getattr(self, "_lex_global", False):
            raise E("delete_rows: not supported on a document shard (idf / avgdl are the whole corpus': "
                    "the delete needs a collective df / length all-reduce)")
        if (ids.numel() if isinstance(ids, torch.Tensor) else np.asarray(ids).size) == 0:
            return torch.arange(n_old, dtype=torch.int32, device=self.device)   # (also a plain [])
        t = self._host_or_device(ids, "ids", integer=True, who="delete_rows").reshape(-1)
        first, hi = int(t.min()), int(t.max())
        if first < 0 or hi >= n_old:
            raise E(f"delete_rows: ids are local doc ids, 0 .. {n_old - 1}")
        uniq = int(torch.unique(t).numel()) if isinstance(t, torch.Tensor) else int(np.unique(t).size)
        if uniq >= n_old:
            raise E("delete_rows: every row would be deleted: build a new index")
        # ---- phase 1: nothing a query reads is written
        self._sync_streams()
        keep = torch.ones(n_old, dtype=torch.bool, device=self.device)
        keep[self._t(t, torch.int64)] = False
        src = keep.nonzero().reshape(-1)          # new id -> old id, ascending
        n_new = int(src.shape[0])
        rank = torch.cumsum(keep, 0, dtype=torch.int32) - 1
        remap = torch.where(keep, rank, torch.full_like(rank, -1))
        new = {}          # name -> (buffer, logical rows): swapped in at the end
        for name, view in self._row_arrays().items():
            if name in ("docs", "docs16", "tokens"):
                continue
            buf = torch.empty_like(self._own_buffer(name, view))     # (4 - 8 bytes a row; keeps the capacity)
            torch.index_select(view, 0, src, out=buf[:n_new])
            new[name] = (buf, n_new)
        dest = {}         # CSR payload name -> the capacity buffer it was compacted into
        lex_new = graph_new = None
        if self.lex is not None:
            L = self.lex
            rowptr, pd, ptf, k = N.csr_compact(L["rowptr"], L["post_doc"], L["post_tf"], remap, 0,
                                               self._compact_dest("post_doc", L["post_doc"]),
                                               self._compact_dest("post_tf", L["post_tf"]))
            dest.update(post_doc=pd, post_tf=ptf)
            lex_new = self._lexical_derived(rowptr, pd[:k], ptf[:k], new["doclen"][0][:n_new], n_new)
        if self.graph is not None:
            G = self.graph
            rowptr, mc, mw, k = N.csr_compact(G["men_rowptr"], G["men_chunk"], G["men_conf"], remap, self.doc_base,
                                              self._compact_dest("men_chunk", G["men_chunk"]),
                                              self._compact_dest("men_conf", G["men_conf"]))
            dest.update(men_chunk=mc, men_conf=mw)
            graph_new = dict(ent_rowptr=G["ent_rowptr"], ent_col=G["ent_col"], men_rowptr=rowptr,
                             men_chunk=mc[:k], men_conf=mw[:k])
        # the large arrays: rows below the first deleted one stay where they are
        t0 = first // 32 * 32                     # the float16 tile of the first deleted row is re-quantised
        f16 = self.docs is not None and self.shortlist in ("f16", "f16-inline")
        moves = []        # (name, buffer, first row that moves, rows per chunk)
        per_q = 32        # rows per chunk of the float16 re-measure / re-quantisation
        for name, start in (("docs", t0), ("tokens", first)):
            view = getattr(self, name)
            if view is None:
                continue
            buf = self._own_buffer(name, view)
            new[name] = (buf, n_new)              # the shorter view is swapped in whether or not a row moves
            row_bytes = max(1, view[0].numel() * view.element_size())
            per = max(32, self.STAGING_BYTES // row_bytes // 32 * 32)
            if name == "docs":
                per_q = min(per, (max(n_new - t0, t0) + 31) // 32 * 32)
            if start < n_new:                     # (a delete of trailing rows only moves nothing)
                moves.append((name, buf, start, min(per, (n_new - start + 31) // 32 * 32)))
        stage = torch.empty(max([per * (buf[0].numel() * buf.element_size()) for _, buf, _, per in moves] or [0]),
                            dtype=torch.uint8, device=self.device)
        q16 = buf16 = errs = err_max = None
        if f16:
            per_tail = max([p for name, _, _, p in moves if name == "docs"] or [32])
            below = range(0, t0, per_q) if self.shortlist == "f16" else range(0, min(t0, 1))
            n_tail = len(range(t0, n_new, per_tail))
            errs = torch.zeros(len(below) + n_tail, dtype=torch.float32, device=self.device)
            err_max = torch.zeros(1, dtype=torch.float32, device=self.device)
            if self.shortlist == "f16":
                q16 = torch.empty((per_q, self.dim), dtype=torch.float16, device=self.device)
                buf16 = self._own_buffer("docs16", self.docs16)
            # the error of the rows that do not move, measured as the fresh build measures it (the
            # float16 copy's on the normalised rows, into the temporary; the in-flight rounding's in one call)
            for j, a in enumerate(below):
                if self.shortlist == "f16":
                    b = min(a + per_q, t0)
                    N.dense_quantize_f16_into(self.docs[a:b], q16[:b - a], errs[n_tail + j:n_tail + j + 1])
                else:
                    N.dense_quantize_f16_into(self.docs[:t0], None, errs[n_tail:n_tail + 1])
        torch.cuda.current_stream(self.device).synchronize()    # (an asynchronous failure of phase 1 surfaces here)
        # ---- phase 2: in-place row moves inside existing buffers, then the swap; no device allocation
        try:
            for name, buf, start, per in moves:
                view = getattr(self, name)
                tmp_all = stage[:per * buf[0].numel() * buf.element_size()].view(buf.dtype).view((per,) + tuple(buf.shape[1:]))
                for j, a in enumerate(range(start, n_new, per)):
                    b = min(a + per, n_new)
                    tmp = tmp_all[:b - a]
                    torch.index_select(view, 0, src[a:b], out=tmp)
                    buf[a:b].copy_(tmp)
                    if name == "docs" and f16:
                        if q16 is not None:
                            r16 = (b - a + 31) // 32 * 32     # (the last tile's padding is what a full quantisation writes)
                            N.dense_quantize_f16_into(tmp, q16[:r16], errs[j:j + 1])
                            buf16[a:a + r16].copy_(q16[:r16])
                        else:
                            N.dense_quantize_f16_into(tmp, None, errs[j:j + 1])
            if self.docs16 is not None:
                new["docs16"] = (self._own_buffer("docs16", self.docs16), (n_new + 31) // 32 * 32)
            # ---- swap
            # the buffers the CSRs were read from become the destinations of the next append or delete
            old = dict(self.lex or {}, **(self.graph or {}))
            cap = self._csr_cap
            self._spare = {k: cap[k] if k in cap and cap[k].data_ptr() == old[k].data_ptr() else old[k] for k in dest}
            self._csr_cap = dest
            if lex_new is not None:
                self.df_local = self.df_global = lex_new.pop("df")
                self.lex = lex_new
            if graph_new is not None:
                self.graph = graph_new          # (the chunk-major copy of the mentions is rebuilt on next use)
            for name, (buf, n) in new.items():
                self._backing[name] = buf
                self._set_row_array(name, buf[:n])
            if f16:
                self.doc_rel_err = float(torch.amax(errs, 0, keepdim=True, out=err_max).item())
            self.n_docs = n_new
            self._ws = None
            self._shortlist_of = None
            self._mutations += 1
            torch.cuda.current_stream(self.device).synchronize()
        except BaseException as exc:
            self._unusable = ("this index is unusable: a delete failed while rows were being moved in place "
                              f"({type(exc).__name__}: {exc}); build a new index")
            raise
        return remap

    # ------------------------------------------------------------ channels
    def _workspace(self, nbytes: int) -> torch.Tensor:
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self._ws

    def reserve(self, n_queries: int, k: int, kprime: Optional[int] = None) -> "GpuIndex":
        """Allocate the dense workspaces for batches of ``n_queries`` up front (index set-up), so
        that no search pays a device allocation."""
        if self.shortlist == "exact":
            return self
        if self.shortlist != "f32":
            kp = min(N.THR_DENSE_MAX_K, max(k, kprime or (k + 92)))
            self._workspace(N.dense_f16_workspace_bytes(self.n_docs, self.dim, n_queries, kp))
        else:
            kp = min(N.THR_DENSE_MAX_K, max(k, kprime or (k + 28)))
            self._workspace(N.dense_workspace_bytes(self.n_docs, self.dim, n_queries, kp))
        need = N.dense_rescue_workspace_bytes(n_queries, k)
        if self._ws_rescue is None or self._ws_rescue.numel() < need:
            self._ws_rescue = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self

    def max_batch(self) -> int:
        """Queries one dense_search call hands to the scan at once (larger batches are split)."""
        if self.shortlist == "f16":
            return N.dense_f16_max_queries(self.dim, True)
        return 1 << 30

    @_refuse_when_unusable
    def dense_search(self, queries: torch.Tensor, k: int, kprime: Optional[int] = None,
                     rescue: bool = True, sync: bool = True, collections=None, floor_exchange=None):
        """Exact cosine top-k -> (scores f64, ids i64, counts i32, n_rescued).  Queries the
        error-bound certificate cannot prove exact (massive ties / duplicates) are redone on the
        exhaustive float64 path, on the device (thr_dense_rescue: no host read-back).
        n_rescued is an int, or with sync=False the device int32[1] it would be read from.
        collections: int32 [nq] collection id per query (-1 = unfiltered), applied before the
        ranking (set_collections).
        floor_exchange: (callable, n_shards) of a DOCUMENT-SHARDED index -- the callable maps this
        shard's float32 [nq, m] lower bounds to all the shards' [n_shards, nq, m] (an all-gather).
        The search is then split around that one exchange (thr_dense_shortlist_f16 / thr_dense_floor
        / thr_dense_finish_f16): rows that cannot be among the k best of ALL shards are not
        rescored, the returned list may hold fewer than k rows and is this shard's part of the
        global top-k (merge the shards' lists with thr_merge_topk).  Every shard must make the same
        sequence of calls.  Used by the f16 scans only."""
        queries = self._t(queries, torch.float32)
        nq = queries.shape[0]
        self._shortlist_of = None     # (the workspace's candidate lists are about to be overwritten)
        if self.shortlist == "f16":
            # one call of the copy scan takes at most dense_f16_max_queries queries (its
            # candidate-segment offsets are 32 bits): larger batches go through in pieces
            step = self.max_batch()
            if nq > step:
                S, I, cnt, _ = N._alloc_out(nq, k, self.device)
                n_rescued = 0 if sync else torch.zeros(1, dtype=torch.int32, device=self.device)
                coll = None if collections is None else self._t(collections, torch.int32)
                for lo in range(0, nq, step):
                    hi = min(nq, lo + step)
                    s_, i_, c_, r_ = self.dense_search(queries[lo:hi], k, kprime, rescue, sync,
                                                       None if coll is None else coll[lo:hi],
                                                       floor_exchange)
                    S[lo:hi], I[lo:hi], cnt[lo:hi] = s_, i_, c_
                    n_rescued = n_rescued + r_
                return S, I, cnt, n_rescued
        dc, qc = self._qcoll(collections, nq)
        if self.shortlist == "exact":
            S, I, cnt, _ = N.dense_topk_exact(self.docs, self.dnorm, queries, k, self.doc_base, dc, qc)
            return S, I, cnt, (0 if sync else torch.zeros(1, dtype=torch.int32, device=self.device))
        if self.shortlist != "f32":
            # tau must sit clearly below the k-th score for the quantisation-aware certificate:
            # k' = 192 puts it ~6e-3 below on a 1M-row corpus, ~6x the f16 error bound
            kp = min(N.THR_DENSE_MAX_K, max(k, kprime or (k + 92)))
            ws = self._workspace(N.dense_f16_workspace_bytes(self.n_docs, self.dim,
                                                             queries.shape[0], kp))
            if floor_exchange is not None:
                exchange, n_shards = floor_exchange
                lb = N.dense_shortlist_f16(self.docs, self.docs16, self.doc_rel_err, self.inv_norm,
                                           queries, kp, floor_width(k, n_shards), ws,
                                           doc_coll=dc, query_coll=qc)
                S, I, cnt, flg = N.dense_finish_f16(self.docs, self.docs16, self.doc_rel_err, self.dnorm,
                                                    self.inv_norm, queries, k, kp, None, self.doc_base,
                                                    ws, doc_coll=dc, query_coll=qc, lb_all=exchange(lb))
            else:
                S, I, cnt, flg = N.dense_topk_f16(self.docs, self.docs16, self.doc_rel_err, self.dnorm,
                                                  self.inv_norm, queries, k, kp, self.doc_base, ws,
                                                  doc_coll=dc, query_coll=qc)
        else:
            kp = min(N.THR_DENSE_MAX_K, max(k, kprime or (k + 28)))
            ws = self._workspace(N.dense_workspace_bytes(self.n_docs, self.dim, queries.shape[0], kp))
            S, I, cnt, flg = N.dense_topk(self.docs, self.dnorm, self.inv_norm, queries, k, kp,
                                          self.doc_base, ws, doc_coll=dc, query_coll=qc)
        n_rescued = 0
        if rescue:
            need = N.dense_rescue_workspace_bytes(queries.shape[0], k)
            if self._ws_rescue is None or self._ws_rescue.numel() < need:
                self._ws_rescue = torch.empty(need, dtype=torch.uint8, device=self.device)
            n_rescued = N.dense_rescue(self.docs, self.dnorm, queries, S, I, cnt, flg,
                                       self.doc_base, self._ws_rescue, doc_coll=dc, query_coll=qc)
            if sync:
                n_rescued = int(n_rescued)
        return S, I, cnt, n_rescued

    # The two halves of dense_search(floor_exchange=...) on their own, for a caller that holds
    # several shards in ONE process (tests, bench.py's shard proxy): shortlist on every shard,
    # stack the results, thr_dense_floor, finish on every shard.
    def _f16_call(self, queries, k, kprime, collections):
        if self.shortlist not in ("f16", "f16-inline"):
            raise N.NativeError("the shard floor is built for the f16 scans")
        queries = self._t(queries, torch.float32)
        if queries.shape[0] > self.max_batch():
            raise N.NativeError("dense_shortlist/finish: one scan batch at a time (max_batch())")
        kp = min(N.THR_DENSE_MAX_K, max(k, kprime or (k + 92)))
        ws = self._workspace(N.dense_f16_workspace_bytes(self.n_docs, self.dim, queries.shape[0], kp))
        dc, qc = self._qcoll(collections, queries.shape[0])
        return queries, kp, ws, dc, qc

    @_refuse_when_unusable
    def dense_shortlist(self, queries: torch.Tensor, k: int, n_shards: int, kprime: Optional[int] = None,
                        collections=None) -> torch.Tensor:
        queries, kp, ws, dc, qc = self._f16_call(queries, k, kprime, collections)
        self._shortlist_of = None
        lb = N.dense_shortlist_f16(self.docs, self.docs16, self.doc_rel_err, self.inv_norm, queries, kp,
                                   floor_width(k, n_shards), ws, doc_coll=dc, query_coll=qc)
        # what the candidate lists in the workspace belong to: dense_finish refuses anything else
        self._shortlist_of = (queries.shape[0], kp, collections is not None, ws.data_ptr())
        return lb

    @_refuse_when_unusable
    def dense_finish(self, queries: torch.Tensor, k: int, gfloor: Optional[torch.Tensor] = None,
                     kprime: Optional[int] = None, rescue: bool = True, collections=None,
                     lb_all: Optional[torch.Tensor] = None):
        """-> (scores, ids, counts, flags BEFORE the rescue, n_rescued device int32[1] or 0).
        The floor: gfloor [nq], or the gathered bounds lb_all [n_shards, nq, m] themselves."""
        queries, kp, ws, dc, qc = self._f16_call(queries, k, kprime, collections)
        if getattr(self, "_shortlist_of", None) != (queries.shape[0], kp, collections is not None, ws.data_ptr()):
            raise N.NativeError("dense_finish: the workspace does not hold the candidate lists of a matching "
                                "dense_shortlist call (same batch size, k, collections; no other dense "
                                "search on this index in between)")
        S, I, cnt, flg = N.dense_finish_f16(self.docs, self.docs16, self.doc_rel_err, self.dnorm,
                                            self.inv_norm, queries, k, kp, gfloor, self.doc_base, ws,
                                            doc_coll=dc, query_coll=qc, lb_all=lb_all)
        flags0 = flg.clone()
        n_rescued = 0
        if rescue:
            need = N.dense_rescue_workspace_bytes(queries.shape[0], k)
            if self._ws_rescue is None or self._ws_rescue.numel() < need:
                self._ws_rescue = torch.empty(need, dtype=torch.uint8, device=self.device)
            n_rescued = N.dense_rescue(self.docs, self.dnorm, queries, S, I, cnt, flg, self.doc_base,
                                       self._ws_rescue, doc_coll=dc, query_coll=qc)
        return S, I, cnt, flags0, n_rescued

    @_refuse_when_unusable
    def scan_probe(self, queries: torch.Tensor) -> None:
        """Launch ONLY the streaming scan kernel of the last dense_search (same workspace, so the
        thresholds tau are the ones that search computed): the timing/roofline probe."""
        if self._ws is None or self.shortlist == "exact":
            raise N.NativeError("scan_probe needs a preceding dense_search on this index (and a shortlist scan)")
        queries = self._t(queries, torch.float32)
        if self.shortlist != "f32":
            N.dense_scan_probe_f16(self.docs, self.docs16, self.inv_norm, queries, self._ws)
        else:
            N.dense_scan_probe(self.docs, self.inv_norm, queries, self._ws)

    def _qcoll(self, collections, nq: int):
        if collections is None:
            return None, None
        if self.doc_coll is None:
            raise N.NativeError("collection filter without set_collections()")
        qc = self._t(collections, torch.int32)
        if qc.shape != (nq,):
            raise N.NativeError("collections: one id per query")
        return self.doc_coll, qc

    @_refuse_when_unusable
    def bm25_search(self, query_terms: torch.Tensor, k: int, collections=None,
                    conjunctive: bool = False, prune: bool = True, dense_rows: bool = True):
        """collections: int32 [nq] collection id per query (-1 = unfiltered) or None.
        One call takes at most N.THR_BM25_MAX_QUERIES (2^20) queries; a larger batch is refused."""
        L = self.lex
        qt = self._t(query_terms, torch.int32)
        N.bm25_check_batch(qt.shape[0])
        dc, qc = self._qcoll(collections, qt.shape[0])
        need = N.bm25_workspace_bytes(qt.shape[0], qt.shape[1], k)
        # ONE lexical workspace per index, used from whichever stream the caller is on (the main
        # one, or the side stream of side_channels / GpuIndexClient's deferred RPC): the stream of
        # this call waits for the previous call's kernels before its memset touches the workspace
        cur = torch.cuda.current_stream(self.device)
        if self._lex_done is not None:
            cur.wait_event(self._lex_done)
        if self._ws_lex is None or self._ws_lex.numel() < need:   # kept: no allocation per search
            self._ws_lex = torch.empty(need, dtype=torch.uint8, device=self.device)
        try:
            return self._bm25_call(L, qt, k, dc, qc, conjunctive, prune, dense_rows)
        finally:
            if self._lex_done is None:
                self._lex_done = torch.cuda.Event()
            self._lex_done.record(cur)

    def _bm25_call(self, L, qt, k, dc, qc, conjunctive, prune, dense_rows):
        return N.bm25_topk(L["rowptr"], L["post_doc"], L["post_tf"], L["doclen"], L["idf"],
                           L["avgdl"], qt, k, self.doc_base, L["k1"], L["b"],
                           bounds=L["bounds"] if prune else None, conjunctive=conjunctive,
                           doc_coll=dc, query_coll=qc, workspace=self._ws_lex,
                           dense=L["dense"] if prune and dense_rows else None)

    @_refuse_when_unusable
    def graph_search(self, query_seeds: torch.Tensor, k: int, hops: int = 2):
        G = self.graph
        # three tiers on the device (small / full on-chip capacities, then a capacity-free walk
        # in global memory): no flag to read back, nothing to raise in the middle of a batch
        seeds = self._t(query_seeds, torch.int32)
        need = N.graph_workspace_bytes(seeds.shape[0], G["ent_rowptr"].shape[0] - 1)
        if self._ws_graph is None or self._ws_graph.numel() < need:   # kept: no allocation per search
            self._ws_graph = torch.empty(need, dtype=torch.uint8, device=self.device)
        S, I, cnt, _ = N.graph_topk(G["ent_rowptr"], G["ent_col"], G["men_rowptr"],
                                    G["men_chunk"], G["men_conf"], seeds, hops, k, self.doc_base,
                                    self.n_docs, transposed=self._graph_transposed(),
                                    workspace=self._ws_graph)
        return S, I, cnt

    @_refuse_when_unusable
    def maxsim(self, qtok: torch.Tensor, cand_global_ids: torch.Tensor) -> torch.Tensor:
        """MaxSim of each query against its candidate docs (global ids; ids outside this
        shard or negative score -inf)."""
        return N.maxsim_ids(self._t(qtok, torch.float16), self.tokens, self._t(cand_global_ids, torch.int64),
                            self.doc_base, packed=self.tokens_packed)

    # ------------------------------------------------------------ pipeline
    @_refuse_when_unusable
    def side_channels(self, query_terms, lexical_top_k: int, query_seeds, graph_top_k: int, hops: int):
        """The lexical and graph channels of a batch on a second HIP stream, so that they run
        beside the dense channel instead of after it: they do not depend on it before the fusion,
        they are latency-bound (one workgroup per query, a few per CU), and the dense pipeline has
        stretches that leave CUs idle (sample pass, shortlist, the gather-bound rescoring, the
        tail of the scan).  Returns (lexical result or None, graph result or None, join): call
        ``join()`` on the main stream before the results are read there.  THR_SIDE_STREAM=0 keeps
        everything on one stream."""
        want_lex = query_terms is not None and self.lex is not None
        want_gra = query_seeds is not None and self.graph is not None
        if not (want_lex or want_gra):
            return None, None, (lambda: None)
        if os.environ.get("THR_SIDE_STREAM") == "0" or self.device.type != "cuda":
            lex = self.bm25_search(query_terms, lexical_top_k) if want_lex else None
            gra = self.graph_search(query_seeds, graph_top_k, hops) if want_gra else None
            return lex, gra, (lambda: None)
        self.side_stream()
        main = torch.cuda.current_stream(self.device)
        self._side.wait_stream(main)            # the inputs were produced on the main stream
        for t in (query_terms, query_seeds):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(self._side)
        with torch.cuda.stream(self._side):
            lex = self.bm25_search(query_terms, lexical_top_k) if want_lex else None
            gra = self.graph_search(query_seeds, graph_top_k, hops) if want_gra else None
        for res in (lex, gra):
            if res is not None:
                for t in res:
                    t.record_stream(main)       # allocated on the side stream, read on the main one

        def join():
            torch.cuda.current_stream(self.device).wait_stream(self._side)
        return lex, gra, join

    def side_stream(self) -> "torch.cuda.Stream":
        if getattr(self, "_side", None) is None:
            # a high-priority queue: its short kernels get their CUs first and are gone before
            # the scan's one-workgroup-per-CU launch needs them (triple + rerank step 4.57 ms on
            # one stream, 4.42 with an equal-priority side stream -- THR_SIDE_STREAM=eq --, 4.32 so)
            eq = os.environ.get("THR_SIDE_STREAM") == "eq"
            self._side = torch.cuda.Stream(device=self.device, priority=0 if eq else -1)
        return self._side

    @_refuse_when_unusable
    def retrieve_batch(self, queries: torch.Tensor, query_terms: Optional[torch.Tensor] = None,
                       query_seeds: Optional[torch.Tensor] = None, top_k: int = 10,
                       semantic_top_k: int = 100, lexical_top_k: int = 50, graph_top_k: int = 50,
                       weights: Optional[Dict[str, float]] = None, hops: int = 2,
                       qtok: Optional[torch.Tensor] = None, rerank_top_k: int = 100,
                       rescue: bool = True) -> BatchResult:
        """plan.semantic/lexical/graph_top_k = 100/50/50 and weights 0.7/0.8/1.0 are the
        reference's QueryPlan defaults (src/voice_agent/rag2/query_planner.py:23-50)."""
        w = {"lexical": 0.7, "semantic": 0.8, "graph": 1.0}
        w.update(weights or {})
        ch = {}
        lex, gra, join = self.side_channels(query_terms, lexical_top_k, query_seeds, graph_top_k, hops)
        Ss, Is, Cs, nres = self.dense_search(queries, semantic_top_k, rescue=rescue, sync=False)
        ch["semantic"] = (Ss, Is, Cs)
        join()
        Il = Ig = None
        if lex is not None:
            ch["lexical"] = lex
            Il = lex[1]
        if gra is not None:
            ch["graph"] = gra
            Ig = gra[1]
        rerank = qtok is not None and self.tokens is not None
        n_fused = max(rerank_top_k, top_k) if rerank else top_k
        ids, sc, _, cnt = N.rrf_fuse(Il, Is, Ig, n_fused, w["lexical"], w["semantic"], w["graph"])
        if rerank:
            # MaxSim of the fused top rerank_top_k, then the reference's stable descending sort
            # on ``rerank_score or 0`` (retrieval.py:449-455), on the device
            ids, sc, cnt = N.rerank_order(self.maxsim(qtok, ids), ids, cnt, top_k)
        return BatchResult(ids, sc, cnt, ch, nres)

