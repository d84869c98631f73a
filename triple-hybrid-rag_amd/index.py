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
    entities  uint8 lower-cased entity names, 0xFF-separated + int64 [E+1] offsets (set_entity_names;
              index_entities.EntitySearch: find_entities, a batch's keywords -> its graph seeds)
    tokens    float16 [n, T_d, 128] late-interaction token matrices; with set_tokens(store="fp8") uint8
              [n, T_d, 128] E4M3 codes (packed image) + token_scales float32 [n, T_d]
    attributes int32 [n] per name (set_attributes; "collection" = doc_coll): what a scope tests
               (index_scope.ScopedSearch: scope_plan, the row-list and the label routes); "parent" = the parent
               number of a chunk (set_parents; index_parent.ParentSearch: maxsim(expand="parent"), its derived CSR)

Changing a live index (reserve_rows, append_rows, delete_rows) and the record of which buffer holds
which of these arrays is the base class, ``index_mutate.MutableIndex``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, Optional

import logging
import os

import numpy as np
import torch

from . import _native as N
from .index_mutate import MutableIndex, _refuse_when_unusable, _Storage
from .index_entities import EntitySearch
from .index_text import TextSearch
from .index_scope import ScopedSearch, ScopePlan
from .index_parent import PARENT_MODES, ParentSearch
from .index_diversify import DiversifiedSearch, check_lam

log = logging.getLogger(__name__)


def floor_width(k: int, n_shards: int) -> int:
    """Lower bounds a shard sends per query for the common floor (thr_dense_floor): twice its fair
    share of the k best, at least 16 -- the k-th largest of the n_shards * m values is then close
    to the true k-th score unless one shard holds most of the k best."""
    m = max(16, 2 * -(-k // max(1, n_shards)))
    return max(1, min(m, N.THR_DENSE_MAX_K, 4096 // max(1, n_shards)))   # (n_shards * m values fit the band kernel's LDS)


@dataclass
class BatchResult:
    ids: torch.Tensor            # int64 [nq, top_k] fused (or reranked) global doc ids, -1 pad
    scores: torch.Tensor         # float64 [nq, top_k] RRF scores (rerank: MaxSim scores)
    counts: torch.Tensor         # int32 [nq]
    channels: Dict[str, tuple] = field(default_factory=dict)  # name -> (scores, ids, counts)
    # queries that needed the exhaustive float64 path: an int, or (batch path, so that a batch
    # needs no host synchronisation) a device int32[1] -- int(result.rescued) reads it back
    rescued: object = 0
    # retrieve_batch(parents=): int32 [nq, top_k], the parent number of each returned id; -1 for padding and for a
    # row without a parent.  None when the parent modes were not asked for.
    parents: Optional[torch.Tensor] = None


class GpuIndex(ScopedSearch, ParentSearch, DiversifiedSearch, EntitySearch, TextSearch, MutableIndex):
    # what an index has before anything sets it (also: one made without __init__, as the host tests do)
    _side = None                # the second HIP stream of side_channels, made on first use
    _shortlist_of = None        # what the candidate lists in the dense workspace belong to (dense_shortlist)
    _lex_global = False         # idf / avgdl are a sharded corpus' (set_lexical_rows with a group)
    _unusable: Optional[str] = None    # set when a delete failed while rows were moving in place
    df_local = df_global = None        # per-term document frequencies (set_lexical_rows, append_rows, delete_rows)
    token_store = "f16"         # set_tokens(store=): "fp8" keeps ``tokens`` as the packed E4M3 image ...
    token_scales = None         # ... and one float32 scale per document token here

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
        self._shortlist_auto = False   # set_dense(shortlist="auto"): an append may re-decide the flavour
        self.lex = None
        self.graph = None
        self.tokens = None
        self.doc_coll = None
        self._attrs = {}
        self.tokens_packed = False
        # scratch memory of the searches, grown on demand and kept (_scratch)
        self._ws: Optional[torch.Tensor] = None
        self._ws_rescue: Optional[torch.Tensor] = None
        self._ws_lex: Optional[torch.Tensor] = None
        self._ws_graph: Optional[torch.Tensor] = None
        self._lex_done = None   # event: the last bm25_search's kernels have left the lexical workspace
        self._store = _Storage()    # which capacity buffer is behind which array (reserve_rows / mutations)
        self._mutations = 0     # appends + deletes so far (index_build.save: the host arrays are stale)

    # ------------------------------------------------------------ builders
    SHORTLISTS = ("auto", "f32", "f16", "f16-inline", "f16-anydim", "exact")
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
          "f16-anydim" as "f16-inline" (rows rounded in registers, no copy) by the scan that takes the row
                       length at run time: any multiple of 32 up to 4096 -- 1536-, 2048-, 3072-d models,
                       the 4000-d legacy store -- 64 queries per pass up to 768 dims, 32 up to 1536, 16
                       beyond.  Opt-in: "auto" never picks it; at 512 / 768 / 1024 it runs beside the
                       tuned kernels for comparison;
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
        if shortlist == "f16-anydim":
            if not N.dense_anydim_ok(self.dim) or self.n_docs >= self.F16_MAX_ROWS:
                raise N.NativeError(f"shortlist='f16-anydim' needs a row length that is a multiple of "
                                    f"{N.THR_DENSE_ANYDIM_STEP} up to {N.THR_DENSE_ANYDIM_MAX} (got {self.dim}) "
                                    f"and fewer than {self.F16_MAX_ROWS} rows")
        elif self.dim not in self.SCAN_DIMS and shortlist != "exact":
            if not auto:
                raise N.NativeError(f"shortlist={shortlist!r} needs a row length in {self.SCAN_DIMS}, got "
                                    f"{self.dim}: use shortlist='exact' (or 'auto')")
            log.warning("dense rows of %d dims: no streaming scan is built for that length, every search "
                        "scores all %d rows in float64 (thr_dense_topk_exact)%s", self.dim, self.n_docs,
                        "; shortlist='f16-anydim' scans it on the f16 matrix cores"
                        if N.dense_anydim_ok(self.dim) else "")
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
                                        "6e-5 in magnitude): use shortlist='f32'" +
                                        ("" if self.dim in self.SCAN_DIMS else " or 'exact'"))
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
        N.bm25_check_params(idf, avgdl, k1, b)   # (the pruning bounds' input contract: thr_hip.h, a3)
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
            self._score_bounds(L)
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
        idf, avgdl = self._idf_avgdl(df_glob, sum_dl, n_glob)
        self.df_local, self.df_global = df, df_glob
        self._lex_global = group is not None or n_glob != n
        return self.set_lexical(rowptr, post_doc, post_tf, doclen, idf, avgdl, k1, b, dense_share)

    def export_derived(self) -> dict:
        """What index set-up computed on the device and a saved index can carry along, as host
        arrays: the float16 image of the rows (+ its layout tag and measured error), the BM25
        bounds / per-posting impacts and the dense-term rows (+ the parameters they hold for), the
        FP8 token store (packed E4M3 image + scales: HostIndex.to_gpu(token_store="fp8") takes it as it is)."""
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
        if self.token_store == "fp8" and self.tokens is not None:
            out.update(tokens_fp8=self.tokens.cpu().numpy(), token_scales=self.token_scales.cpu().numpy())
        return out

    def set_collections(self, doc_coll) -> "GpuIndex":
        """Per-document collection id (int32 [n], any non-negative labelling): the
        ``p_collection`` filter of the two RPCs (rag2_schema.sql:368-373, 404-408) is applied
        on the device BEFORE the ranking -- per query, -1 = unfiltered."""
        self.doc_coll = self._t(doc_coll, torch.int32)
        return self

    def set_graph(self, ent_rowptr, ent_col, men_rowptr, men_chunk, men_conf) -> "GpuIndex":
        if self.entities is not None and self.entities["n"] != len(ent_rowptr) - 1:
            raise ValueError(f"set_graph: {len(ent_rowptr) - 1} entities, the index holds {self.entities['n']} "
                             "entity names (set_entity_names)")
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

    TOKEN_STORES = ("f16", "fp8")

    def set_tokens(self, dtok, pack: bool = True, store: str = "f16") -> "GpuIndex":
        """Late-interaction token store f16 [n, d_tokens, tok_dim].  pack=True keeps it in the
        fragment-major layout of thr_maxsim_pack (the row-major copy is dropped).  d_tokens is a
        multiple of 32 and tok_dim one of _native.MAXSIM_TOK_DIMS.

        store="fp8" (opt-in) keeps the tokens as OCP E4M3 codes with one float32 scale per token
        (thr_hip_rerank.h: half the bytes per chunk; scores differ from the float16 store's by the
        quantisation error): ``tokens`` is then the packed uint8 image, ``token_scales`` float32
        [n, d_tokens], the float16 copy is dropped (the image is always packed: ``pack`` is not asked),
        and tok_dim is one of _native.MAXSIM_FP8_TOK_DIMS."""
        shape = self._check_token_store("set_tokens", store, dtok)
        tok = self._t(dtok, torch.float16)
        if store == "fp8":
            self._install_tokens(*N.maxsim_quantize_fp8(tok), store="fp8")
            return self
        # a store the scorer has no kernel for is refused here, packed or not, not at the first query
        N.maxsim_check_tokens("set_tokens", shape[2], shape[1])
        self._install_tokens(N.maxsim_pack(tok) if pack else tok, None, store="f16", packed=bool(pack))
        return self

    @classmethod
    def _check_token_store(cls, what: str, store: str, dtok) -> tuple:
        """What can be refused about a token store before any device work -> its shape."""
        if store not in cls.TOKEN_STORES:
            raise N.NativeError(f"{what}: store must be one of {list(cls.TOKEN_STORES)}, got {store!r}")
        shape = tuple(int(s) for s in (dtok.shape if hasattr(dtok, "shape") else np.shape(dtok)))
        if len(shape) != 3:
            raise N.NativeError(f"{what}: tokens must be [n, d_tokens, tok_dim]")
        if store == "fp8":
            N.maxsim_fp8_check_tokens(f"{what}(store='fp8')", shape[2], shape[1])
        return shape

    def _install_tokens(self, tokens, scales, store: str, packed: bool = True) -> None:
        self.tokens, self.token_scales = tokens, scales
        self.token_store, self.tokens_packed = store, packed

    def set_tokens_fp8(self, codes, scales) -> "GpuIndex":
        """An FP8 token store that exists already (a saved index' image: index_build.load): codes uint8
        [n, d_tokens, tok_dim] in the packed layout of thr_hip_rerank.h, scales float32 [n, d_tokens].
        Nothing is requantised."""
        shape = self._check_token_store("set_tokens_fp8", "fp8", codes)
        if tuple(int(s) for s in scales.shape) != shape[:2]:
            raise N.NativeError(f"set_tokens_fp8: scales must be [{shape[0]}, {shape[1]}], got {tuple(scales.shape)}")
        self._install_tokens(self._t(codes, torch.uint8), self._t(scales, torch.float32), store="fp8")
        return self

    # ------------------------------------------------------------ channels
    def _scratch(self, slot: str, nbytes: int) -> torch.Tensor:
        """The workspace kept in attribute ``slot`` (_ws: dense scan, _ws_rescue, _ws_lex, _ws_graph),
        replaced by a larger one when it is too small: no allocation per search."""
        ws = getattr(self, slot)
        if ws is None or ws.numel() < nbytes:
            ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            setattr(self, slot, ws)
        return ws

    def _kprime(self, k: int, kprime: Optional[int]) -> int:
        """Candidates per query the shortlist scan keeps.  The f16 scans' threshold tau must sit
        clearly below the k-th score for the quantisation-aware certificate: k' = 192 puts it ~6e-3
        below on a 1M-row corpus, ~6x the f16 error bound."""
        return min(N.THR_DENSE_MAX_K, max(k, kprime or (k + (28 if self.shortlist == "f32" else 92))))

    def _scan_workspace(self, n_queries: int, kp: int) -> torch.Tensor:
        size = N.dense_workspace_bytes if self.shortlist == "f32" else N.dense_f16_workspace_bytes
        return self._scratch("_ws", size(self.n_docs, self.dim, n_queries, kp))

    def reserve(self, n_queries: int, k: int, kprime: Optional[int] = None) -> "GpuIndex":
        """Allocate the dense workspaces for batches of ``n_queries`` up front (index set-up), so
        that no search pays a device allocation."""
        if self.shortlist != "exact":
            self._scan_workspace(n_queries, self._kprime(k, kprime))
            self._scratch("_ws_rescue", N.dense_rescue_workspace_bytes(n_queries, k))
        return self

    def _rescue(self, queries, k: int, S, I, cnt, flg, dc, qc) -> torch.Tensor:
        """Redo the queries the certificate flagged on the exhaustive float64 path, in place
        -> how many, a device int32[1]."""
        ws = self._scratch("_ws_rescue", N.dense_rescue_workspace_bytes(queries.shape[0], k))
        return N.dense_rescue(self.docs, self.dnorm, queries, S, I, cnt, flg, self.doc_base, ws,
                              doc_coll=dc, query_coll=qc)

    def max_batch(self) -> int:
        """Queries one dense_search call hands to the scan at once (larger batches are split)."""
        if self.shortlist == "f16":
            return N.dense_f16_max_queries(self.dim, True)
        return 1 << 30

    @_refuse_when_unusable
    def dense_search(self, queries: torch.Tensor, k: int, kprime: Optional[int] = None,
                     rescue: bool = True, sync: bool = True, collections=None, floor_exchange=None,
                     scopes=None, scope_rows_max: Optional[int] = None, _labels=None):
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
        sequence of calls.  Used by the f16 scans only.
        scopes: per query a dict {attribute: value} / an int32 [nq, C] table over attribute_names()
        (-1 = any), or a ScopePlan (scope_plan): only rows that satisfy the query's scope are ranked.
        Resolving the scopes reads the P + 1 row pointers of the P distinct scopes back (the route
        depends on the row counts); a ScopePlan made beforehand avoids that, for sync=False callers.
        A scope of at most ``scope_rows_max`` rows (default SCOPE_ROWS_MAX; 0 = never) is ranked
        over its row list (thr_dense_topk_rows), a wider one through this search with the scope
        labels as doc_coll: the same bits either way.  Not together with ``collections``."""
        if scopes is not None:
            if collections is not None:
                raise ValueError("dense_search: pass scopes= or collections=, not both")
            if floor_exchange is not None:
                raise N.NativeError("dense_search: scopes= is not supported on a document shard (floor_exchange)")
            return self._dense_scoped(queries, k, kprime, rescue, sync, scopes, scope_rows_max)
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
                                                       floor_exchange, _labels=_labels)
                    S[lo:hi], I[lo:hi], cnt[lo:hi] = s_, i_, c_
                    n_rescued = n_rescued + r_
                return S, I, cnt, n_rescued
        dc, qc = self._qcoll(collections, nq, _labels)
        if self.shortlist == "exact":
            S, I, cnt, _ = N.dense_topk_exact(self.docs, self.dnorm, queries, k, self.doc_base, dc, qc)
            return S, I, cnt, (0 if sync else torch.zeros(1, dtype=torch.int32, device=self.device))
        kp = self._kprime(k, kprime)
        ws = self._scan_workspace(nq, kp)
        if self.shortlist != "f32":
            if floor_exchange is not None:
                exchange, n_shards = floor_exchange
                with self._f16_flavour():
                    lb = N.dense_shortlist_f16(self.docs, self.docs16, self.doc_rel_err, self.inv_norm,
                                               queries, kp, floor_width(k, n_shards), ws,
                                               doc_coll=dc, query_coll=qc)
                lb_all = exchange(lb)
                with self._f16_flavour():
                    S, I, cnt, flg = N.dense_finish_f16(self.docs, self.docs16, self.doc_rel_err, self.dnorm,
                                                        self.inv_norm, queries, k, kp, None, self.doc_base,
                                                        ws, doc_coll=dc, query_coll=qc, lb_all=lb_all)
            else:
                with self._f16_flavour():
                    S, I, cnt, flg = N.dense_topk_f16(self.docs, self.docs16, self.doc_rel_err, self.dnorm,
                                                      self.inv_norm, queries, k, kp, self.doc_base, ws,
                                                      doc_coll=dc, query_coll=qc)
        else:
            S, I, cnt, flg = N.dense_topk(self.docs, self.dnorm, self.inv_norm, queries, k, kp,
                                          self.doc_base, ws, doc_coll=dc, query_coll=qc)
        n_rescued = 0
        if rescue:
            n_rescued = self._rescue(queries, k, S, I, cnt, flg, dc, qc)
            if sync:
                n_rescued = int(n_rescued)
        return S, I, cnt, n_rescued

    # The two halves of dense_search(floor_exchange=...) on their own, for a caller that holds
    # several shards in ONE process (tests, bench.py's shard proxy): shortlist on every shard,
    # stack the results, thr_dense_floor, finish on every shard.
    def _f16_flavour(self):
        """The native f16 calls of this index run under it: "f16-anydim" selects the runtime-dim scan at
        the row lengths where the tuned kernel is the default."""
        return N.dense_f16_flavour(self.shortlist == "f16-anydim")

    def _f16_call(self, queries, k, kprime, collections):
        if self.shortlist not in ("f16", "f16-inline", "f16-anydim"):
            raise N.NativeError("the shard floor is built for the f16 scans")
        queries = self._t(queries, torch.float32)
        if queries.shape[0] > self.max_batch():
            raise N.NativeError("dense_shortlist/finish: one scan batch at a time (max_batch())")
        kp = self._kprime(k, kprime)
        ws = self._scan_workspace(queries.shape[0], kp)
        dc, qc = self._qcoll(collections, queries.shape[0])
        return queries, kp, ws, dc, qc

    @_refuse_when_unusable
    def dense_shortlist(self, queries: torch.Tensor, k: int, n_shards: int, kprime: Optional[int] = None,
                        collections=None) -> torch.Tensor:
        queries, kp, ws, dc, qc = self._f16_call(queries, k, kprime, collections)
        self._shortlist_of = None
        with self._f16_flavour():
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
        if self._shortlist_of != (queries.shape[0], kp, collections is not None, ws.data_ptr()):
            raise N.NativeError("dense_finish: the workspace does not hold the candidate lists of a matching "
                                "dense_shortlist call (same batch size, k, collections; no other dense "
                                "search on this index in between)")
        with self._f16_flavour():
            S, I, cnt, flg = N.dense_finish_f16(self.docs, self.docs16, self.doc_rel_err, self.dnorm,
                                                self.inv_norm, queries, k, kp, gfloor, self.doc_base, ws,
                                                doc_coll=dc, query_coll=qc, lb_all=lb_all)
        flags0 = flg.clone()
        n_rescued = self._rescue(queries, k, S, I, cnt, flg, dc, qc) if rescue else 0
        return S, I, cnt, flags0, n_rescued

    @_refuse_when_unusable
    def scan_probe(self, queries: torch.Tensor) -> None:
        """Launch ONLY the streaming scan kernel of the last dense_search (same workspace, so the
        thresholds tau are the ones that search computed): the timing/roofline probe."""
        if self._ws is None or self.shortlist == "exact":
            raise N.NativeError("scan_probe needs a preceding dense_search on this index (and a shortlist scan)")
        queries = self._t(queries, torch.float32)
        if self.shortlist != "f32":
            with self._f16_flavour():
                N.dense_scan_probe_f16(self.docs, self.docs16, self.inv_norm, queries, self._ws)
        else:
            N.dense_scan_probe(self.docs, self.inv_norm, queries, self._ws)

    def _qcoll(self, collections, nq: int, labels=None):
        """(doc_coll, query_coll) of a filtered search; ``labels``: a scope plan's row labels in
        the place of the collection ids."""
        if collections is None:
            return None, None
        if self.doc_coll is None and labels is None:
            raise N.NativeError("collection filter without set_collections()")
        qc = self._t(collections, torch.int32)
        if qc.shape != (nq,):
            raise N.NativeError("collections: one id per query")
        return (self.doc_coll if labels is None else labels), qc

    @_refuse_when_unusable
    def bm25_search(self, query_terms: torch.Tensor, k: int, collections=None,
                    conjunctive: bool = False, prune: bool = True, dense_rows: bool = True, scopes=None,
                    _labels=None):
        """collections: int32 [nq] collection id per query (-1 = unfiltered) or None.
        scopes: as dense_search -- every scope, thin or wide, filters through the scope labels
        (groups of disjoint scopes, one call per group); idf / avgdl stay the corpus'.
        One call takes at most N.THR_BM25_MAX_QUERIES (2^20) queries; a larger batch is refused."""
        if scopes is not None:
            if collections is not None:
                raise ValueError("bm25_search: pass scopes= or collections=, not both")
            return self._bm25_scoped(query_terms, k, scopes, conjunctive, prune, dense_rows)
        L = self.lex
        qt = self._t(query_terms, torch.int32)
        N.bm25_check_batch(qt.shape[0])
        dc, qc = self._qcoll(collections, qt.shape[0], _labels)
        need = N.bm25_workspace_bytes(qt.shape[0], qt.shape[1], k)
        # ONE lexical workspace per index, used from whichever stream the caller is on (the main
        # one, or the side stream of side_channels / GpuIndexClient's deferred RPC): the stream of
        # this call waits for the previous call's kernels before its memset touches the workspace
        cur = torch.cuda.current_stream(self.device)
        if self._lex_done is not None:
            cur.wait_event(self._lex_done)
        self._scratch("_ws_lex", need)
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
    def graph_search(self, query_seeds: torch.Tensor, k: int, hops: int = 2, scopes=None, _labels=None):
        """-> (scores f64, ids i64, counts i32).  scopes: as dense_search -- only chunks that satisfy
        the query's scope are scored and ranked (thr_graph_topk_scoped over the scope labels: groups of
        disjoint scopes, one call per group).  The walk over the entities is not filtered: entities
        carry no attributes, isolation is at the chunk.  ``_labels``: (doc labels, query labels) of
        one such call."""
        if scopes is not None:
            return self._graph_scoped(query_seeds, k, hops, scopes)
        G = self.graph
        # three tiers on the device (small / full on-chip capacities, then a capacity-free walk
        # in global memory): no flag to read back, nothing to raise in the middle of a batch
        seeds = self._t(query_seeds, torch.int32)
        ws = self._scratch("_ws_graph", N.graph_workspace_bytes(seeds.shape[0], G["ent_rowptr"].shape[0] - 1))
        if _labels is not None:
            S, I, cnt, _ = N.graph_topk_scoped(G["ent_rowptr"], G["ent_col"], G["men_rowptr"],
                                               G["men_chunk"], G["men_conf"], seeds, hops, k, self.doc_base,
                                               self.n_docs, _labels[0], _labels[1],
                                               transposed=self._graph_transposed(), workspace=ws)
            return S, I, cnt
        S, I, cnt, _ = N.graph_topk(G["ent_rowptr"], G["ent_col"], G["men_rowptr"],
                                    G["men_chunk"], G["men_conf"], seeds, hops, k, self.doc_base,
                                    self.n_docs, transposed=self._graph_transposed(),
                                    workspace=ws)
        return S, I, cnt

    @_refuse_when_unusable
    def maxsim(self, qtok: torch.Tensor, cand_global_ids: torch.Tensor, expand: Optional[str] = None) -> torch.Tensor:
        """MaxSim of each query against its candidate docs (global ids; ids outside this
        shard or negative score -inf).  Over an FP8 store (set_tokens(store="fp8")) the scores are
        MaxSim over the dequantised tokens.
        expand="parent" (set_parents; the packed float16 or the FP8 store): the score of a candidate is MaxSim
        against its PARENT -- the token blocks of every row with the candidate's parent number, the row alone when it
        has none -- as the reference reranks ``c.parent_text or c.text`` (retrieval.py:419).  The candidates of one
        parent are scored once and share the bits (index_parent.ParentSearch)."""
        if self._check_expand("maxsim", expand):
            return self._maxsim_parent(qtok, cand_global_ids)
        if self.token_store == "fp8":
            return N.maxsim_fp8_ids(self._t(qtok, torch.float16), self.tokens, self.token_scales,
                                    self._t(cand_global_ids, torch.int64), self.doc_base)
        return N.maxsim_ids(self._t(qtok, torch.float16), self.tokens, self._t(cand_global_ids, torch.int64),
                            self.doc_base, packed=self.tokens_packed)

    # ------------------------------------------------------------ pipeline
    @_refuse_when_unusable
    def side_channels(self, query_terms, lexical_top_k: int, query_seeds, graph_top_k: int, hops: int,
                      scopes=None, scope_graph: bool = False):
        """The lexical and graph channels of a batch on a second HIP stream, so that they run
        beside the dense channel instead of after it: they do not depend on it before the fusion,
        they are latency-bound (one workgroup per query, a few per CU), and the dense pipeline has
        stretches that leave CUs idle (sample pass, shortlist, the gather-bound rescoring, the
        tail of the scan).  Returns (lexical result or None, graph result or None, join): call
        ``join()`` on the main stream before the results are read there.  THR_SIDE_STREAM=0 keeps
        everything on one stream.  ``scopes`` filters the lexical channel, and with ``scope_graph``
        the graph channel too (graph_search(scopes=))."""
        gscopes = scopes if scope_graph else None
        want_lex = query_terms is not None and self.lex is not None
        want_gra = query_seeds is not None and self.graph is not None
        if not (want_lex or want_gra):
            return None, None, (lambda: None)
        if os.environ.get("THR_SIDE_STREAM") == "0" or self.device.type != "cuda":
            lex = self.bm25_search(query_terms, lexical_top_k, scopes=scopes) if want_lex else None
            gra = self.graph_search(query_seeds, graph_top_k, hops, scopes=gscopes) if want_gra else None
            return lex, gra, (lambda: None)
        self.side_stream()
        main = torch.cuda.current_stream(self.device)
        self._side.wait_stream(main)            # the inputs were produced on the main stream
        for t in (query_terms, query_seeds):
            if isinstance(t, torch.Tensor) and t.is_cuda:
                t.record_stream(self._side)
        with torch.cuda.stream(self._side):
            lex = self.bm25_search(query_terms, lexical_top_k, scopes=scopes) if want_lex else None
            gra = self.graph_search(query_seeds, graph_top_k, hops, scopes=gscopes) if want_gra else None
        for res in (lex, gra):
            if res is not None:
                for t in res:
                    t.record_stream(main)       # allocated on the side stream, read on the main one

        def join():
            torch.cuda.current_stream(self.device).wait_stream(self._side)
        return lex, gra, join

    def side_stream(self) -> "torch.cuda.Stream":
        if self._side is None:
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
                       rescue: bool = True, scopes=None, scope_rows_max: Optional[int] = None,
                       scope_graph: bool = False, parents: Optional[str] = None,
                       diversify: Optional[float] = None) -> BatchResult:
        """plan.semantic/lexical/graph_top_k = 100/50/50 and weights 0.7/0.8/1.0 are the
        reference's QueryPlan defaults (src/voice_agent/rag2/query_planner.py:23-50).
        scopes: as dense_search, resolved once for the batch; the dense and the lexical channel
        rank inside each query's scope.
        scope_graph: True passes the batch's ScopePlan to the graph channel too (on the side stream):
        a chunk outside the query's scope is neither scored nor ranked there, so no channel list and
        no fused id leaves the scope.  The reference's graph search filters by tenant -- every entity
        and relation query carries .eq("org_id", org_id), graph_search.py:154-230 -- and by nothing
        else (no p_collection there, retrieval.py:316-356).  False (the default) keeps the graph
        channel unfiltered under ``scopes=``: right only where an org's entities mention that org's
        chunks alone.
        parents: child -> parent expansion between the fusion and the rerank (the reference's funnel step 4; needs
        set_parents).  None: no expansion.  "rerank": every fused candidate stays, its rerank score is MaxSim against
        its PARENT (maxsim(expand="parent")); siblings tie and keep their fused order.  Needs ``qtok`` and a token
        store.  "collapse": max(rerank_top_k, top_k) candidates are fused, of each parent only the best-fused child
        stays (with its RRF score), then the parent-score rerank when ``qtok`` is given, then top_k: no two returned
        ids share a parent.  Either way ``BatchResult.parents`` holds the parent number of each returned id.
        diversify: None, or MMR's lambda in [0, 1] (index_diversify.DiversifiedSearch): max(rerank_top_k, top_k)
        candidates are fused, the collapse and the rerank run over all of them, and the ``top_k`` are then SELECTED
        for relevance and mutual dissimilarity over the index's dense rows rather than cut off the top
        (``diversify(ids, scores, counts, top_k, lam)``).  ``ids`` / ``scores`` / ``counts`` are the selection, in
        selection order, the scores the candidates' own (no longer descending).  None: today's path."""
        if diversify is not None:
            diversify = check_lam("retrieve_batch", diversify)
            self._dense_rows_for("retrieve_batch(diversify=)")
        if parents not in PARENT_MODES:
            raise ValueError(f"retrieve_batch: parents must be one of {list(PARENT_MODES)}, got {parents!r}")
        if parents is not None:
            self._parent_column(f"retrieve_batch(parents={parents!r})")
            if parents == "rerank" and (qtok is None or self.tokens is None):
                raise ValueError("retrieve_batch(parents='rerank') reranks on the parent score: it needs qtok and a "
                                 "token store (set_tokens)")
            if qtok is not None and self.tokens is not None:
                self._check_expand("retrieve_batch", "parent")
        if scopes is not None:
            scopes = self.scope_plan(scopes, queries.shape[0])
        w = {"lexical": 0.7, "semantic": 0.8, "graph": 1.0}
        w.update(weights or {})
        ch = {}
        lex, gra, join = self.side_channels(query_terms, lexical_top_k, query_seeds, graph_top_k, hops, scopes,
                                            scope_graph=scope_graph and scopes is not None)
        Ss, Is, Cs, nres = self.dense_search(queries, semantic_top_k, rescue=rescue, sync=False, scopes=scopes,
                                             scope_rows_max=scope_rows_max)
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
        n_fused = max(rerank_top_k, top_k) if rerank or parents == "collapse" or diversify is not None else top_k
        n_kept = top_k if diversify is None else n_fused     # what the collapse and the rerank leave for the cut
        ids, sc, _, cnt = N.rrf_fuse(Il, Is, Ig, n_fused, w["lexical"], w["semantic"], w["graph"])
        if parents == "collapse":
            # the leaders only: the best-fused child stands for its parent, with its RRF score
            leader, _, ids, cnt = self.parent_groups(ids, cnt)
            at = torch.sort((leader == torch.arange(n_fused, device=leader.device, dtype=leader.dtype)).to(torch.int8),
                            dim=1, descending=True, stable=True).indices      # the leaders' positions, in order
            live = torch.arange(n_fused, device=cnt.device)[None, :] < cnt[:, None]
            sc = torch.where(live, torch.gather(sc, 1, at), torch.full_like(sc, float("-inf")))
            if not rerank:
                ids, sc = ids[:, :n_kept].contiguous(), sc[:, :n_kept].contiguous()
                cnt = torch.clamp(cnt, max=n_kept)
        if rerank:
            # MaxSim of the fused top rerank_top_k, then the reference's stable descending sort
            # on ``rerank_score or 0`` (retrieval.py:449-455), on the device
            expand = None if parents is None else "parent"
            ids, sc, cnt = N.rerank_order(self.maxsim(qtok, ids, expand=expand), ids, cnt, n_kept)
        if diversify is not None:
            ids, sc, cnt, _, _ = self.diversify(ids, sc, cnt, top_k=top_k, lam=diversify)
        return BatchResult(ids, sc, cnt, ch, nres, None if parents is None else self.parents_of(ids))

