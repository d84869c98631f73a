"""The live index's storage and its mutations: ``reserve_rows``, ``append_rows``, ``delete_rows``.

``MutableIndex`` is the base class of ``index.GpuIndex``: it works on the arrays and the state that
``GpuIndex.__init__`` declares and that the ``set_*`` builders fill.  Both mutations keep one
invariant -- afterwards every device array is, to the bit, what a fresh build would hold -- and the
same shape: validate, build the new state in memory no query reads, hand it to ``_commit``.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple

import functools
import warnings

import numpy as np
import torch

from . import _native as N


def _refuse_when_unusable(fn):
    """A delete that failed in its in-place phase leaves rows half moved (MutableIndex.delete_rows): the
    index marks itself unusable, and no search, append or delete may run on it afterwards."""
    @functools.wraps(fn)
    def call(self, *a, **kw):
        if self._unusable:
            raise N.NativeError(self._unusable)
        return fn(self, *a, **kw)
    return call


def _tiles32(rows: int) -> int:
    """``rows`` rounded up to whole tiles of 32: the unit of the float16 image and of a chunk of moved rows."""
    return (rows + 31) // 32 * 32


class _Storage:
    """Which buffer holds which array of an index, and how much room it has.

    After a build every per-document array (``ROWS`` + the lexical ``doclen``) and every CSR payload
    (post_doc, post_tf, men_chunk, men_conf) is a tensor of exactly its logical size.  reserve_rows and the mutations move an array
    into a larger buffer, of which the index then holds the leading part; ``held`` records that
    buffer together with the view it was recorded for.  A builder that replaces the array (set_dense
    again, ...) leaves a record about a tensor the index no longer holds: it counts for nothing."""
    ROWS = ("docs", "docs16", "dnorm", "inv_norm", "doc_coll", "tokens", "token_scales")    # GpuIndex attributes
    GROWTH = 1.5    # a buffer that is too small is replaced by one of GROWTH x its size (at least the need)

    def __init__(self):
        self.held: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = {}   # name -> (buffer, the index's view of it)
        self.spare: Dict[str, torch.Tensor] = {}    # CSR payload name -> destination of the next mutation

    @staticmethod
    def padded(name: str, rows: int) -> int:
        """Buffer rows behind ``rows`` documents: the float16 image is kept in whole tiles of 32 rows."""
        return _tiles32(rows) if name == "docs16" else rows

    def behind(self, name: str, view: torch.Tensor) -> torch.Tensor:
        """The capacity buffer behind the index's array ``view``, or the array itself."""
        buf, of = self.held.get(name, (view, view))
        return buf if of is view else view

    def with_room(self, name: str, view: torch.Tensor, rows: int, exact: bool = False) -> torch.Tensor:
        """A buffer of array ``name`` with room for ``rows`` documents that holds the rows of ``view``:
        the buffer behind the view when that has the room (what lies behind the view is free to
        write: no kernel is given more than the logical size), else a new one -- of just that
        size (``exact``) or at least GROWTH x the old one -- with the old rows copied on the device."""
        need = self.padded(name, rows)
        buf = self.behind(name, view)
        if buf.shape[0] >= need:
            return buf
        cap = need if exact else max(need, int(self.GROWTH * view.shape[0]))
        buf = torch.empty((cap,) + tuple(view.shape[1:]), dtype=view.dtype, device=view.device)
        buf[:view.shape[0]].copy_(view)
        return buf

    def destination(self, name: str, like: torch.Tensor, need: int, grow: bool) -> torch.Tensor:
        """Where an out-of-place CSR mutation writes payload ``name`` (now ``like``), ``need`` entries:
        the spare buffer when it has the room, else a new one (``grow``: at least GROWTH x the old size)."""
        sp = self.spare.get(name)
        # (a destination is never the memory it is filled from: thr_csr_append / _compact are out of place)
        if sp is not None and sp.shape[0] >= need and sp.dtype == like.dtype and sp.data_ptr() != like.data_ptr():
            return sp
        size = max(need, int(self.GROWTH * like.shape[0])) if grow else need
        return torch.empty(size, dtype=like.dtype, device=like.device)

    def rotate(self, dest: Dict[str, Tuple[torch.Tensor, torch.Tensor]], old: Dict[str, torch.Tensor]) -> None:
        """The CSR payloads now live in ``dest`` (name -> (buffer, view)): the buffers they were read
        from (behind the ``old`` views) become the destinations of the next append or delete."""
        self.spare = {name: self.behind(name, old[name]) for name in dest}
        self.held.update(dest)


@dataclass
class _NewState:
    """What a mutation built and ``_commit`` installs."""
    n_docs: int
    rows: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = field(default_factory=dict)   # row array -> (buffer, view)
    csr: Dict[str, Tuple[torch.Tensor, torch.Tensor]] = field(default_factory=dict)    # CSR payload -> (buffer, view)
    lex: Optional[dict] = None       # the new ``lex`` dict + "df"
    graph: Optional[dict] = None
    entities: Optional[dict] = None  # the new name store (append_graph with names)
    shortlist: Optional[str] = None  # dense channel: the flavour and the float16 error bound afterwards
    doc_rel_err: float = 0.0


@dataclass
class _MovePlan:
    """Phase 2 of delete_rows, decided and allocated: ``_move_rows`` only copies inside these buffers."""
    src: torch.Tensor                # new row -> old row, ascending
    n_new: int
    moves: List[tuple]               # (name, rows as the index holds them, buffer, first row that moves, rows per chunk)
    stage: torch.Tensor              # uint8: the chunk in flight
    # float16 flavours: the error of every surviving row, one slot per measured chunk
    errs: Optional[torch.Tensor] = None        # the tail chunks' slots first, then those of the rows that stay
    err_tail: Optional[torch.Tensor] = None    # errs[:number of "docs" chunks]: written as the chunks pass
    err_max: Optional[torch.Tensor] = None
    q16: Optional[torch.Tensor] = None         # "f16": the float16 image of one chunk ...
    buf16: Optional[torch.Tensor] = None       # ... and the buffer of the index's image it is copied into


class MutableIndex:
    STAGING_BYTES = 256 << 20    # delete: the large per-row arrays are compacted through a buffer of at most this size
    LEX_CSR = ("rowptr", "post_doc", "post_tf")            # keys of a CSR in ``lex`` / ``graph``: row pointers,
    GRAPH_CSR = ("men_rowptr", "men_chunk", "men_conf")    # ids, payload

    def _t(self, a, dtype):
        if isinstance(a, torch.Tensor):
            return a.to(device=self.device, dtype=dtype).contiguous()
        a = np.ascontiguousarray(a)
        if not a.flags.writeable:   # a memory-mapped index (index_build.load): read-only is fine,
            with warnings.catch_warnings():   # the tensor is only the source of the device copy
                warnings.simplefilter("ignore", UserWarning)
                return torch.from_numpy(a).to(device=self.device, dtype=dtype)
        return torch.from_numpy(a).to(device=self.device, dtype=dtype)

    # ------------------------------------------------------------ derivations the builders share with the mutations
    # (one copy each: "equal to a fresh build" means these very formulas)
    @staticmethod
    def _idf_avgdl(df: torch.Tensor, sum_dl: torch.Tensor, n: int):
        """BM25's idf per term and the mean chunk length from the document frequencies, the length
        total and the corpus' row count: float64 numpy on the host, the oracle's formula to the bit."""
        dfh = df.cpu().numpy().astype(np.float64)
        idf = np.log(1.0 + (float(n) - dfh + 0.5) / (dfh + 0.5))
        avgdl = float(sum_dl.item()) / max(n, 1)
        return idf, avgdl if avgdl > 0 else 1.0

    @staticmethod
    def _score_bounds(L: dict) -> None:
        """Into the lexical dict ``L``: per-term / per-128-posting score bounds for the WAND-style
        pruning of thr_bm25_topk, and the per-doc rows of the terms ``dense_share`` of the docs hold."""
        L["bounds"] = N.bm25_bounds(L["rowptr"], L["post_doc"], L["post_tf"], L["doclen"], L["idf"],
                                    L["avgdl"], L["k1"], L["b"])
        L["dense"] = N.bm25_dense_terms(L["rowptr"], L["post_doc"], L["post_tf"], L["bounds"][2],
                                        int(L["doclen"].shape[0]), L["dense_share"]) if L["dense_share"] > 0 else None

    def _lexical_derived(self, rowptr, post_doc, post_tf, doclen) -> dict:
        """What follows a changed CSR (an append's or a delete's), as a new ``self.lex`` dict + "df":
        df from the row pointers, idf / avgdl, the pruning bounds and the dense-term rows for the
        new row count, all as set_lexical_rows -> set_lexical derive them."""
        L = self.lex
        df = rowptr[1:] - rowptr[:-1]
        idf, avgdl = self._idf_avgdl(df, doclen.sum(dtype=torch.float64), int(doclen.shape[0]))
        out = dict(rowptr=rowptr, post_doc=post_doc, post_tf=post_tf, doclen=doclen,
                   idf=self._t(idf, torch.float64), avgdl=avgdl, k1=L["k1"], b=L["b"], dense_share=L["dense_share"])
        self._score_bounds(out)
        out["df"] = df
        return out

    def _graph_with(self, men_rowptr, men_chunk, men_conf, ent_rowptr=None, ent_col=None) -> dict:
        """A new ``self.graph`` dict: the entity CSR as it is (or the one given), the mentions given
        (the chunk-major copy of the mentions is rebuilt on next use, as after set_graph)."""
        G = self.graph
        return dict(ent_rowptr=G["ent_rowptr"] if ent_rowptr is None else ent_rowptr,
                    ent_col=G["ent_col"] if ent_col is None else ent_col, men_rowptr=men_rowptr,
                    men_chunk=men_chunk, men_conf=men_conf)

    # ------------------------------------------------------------ storage
    def _row_arrays(self) -> Dict[str, torch.Tensor]:
        """The per-document arrays the index has (leading dimension = rows; docs16: whole tiles)."""
        arrs = {name: getattr(self, name) for name in _Storage.ROWS}
        arrs["doclen"] = self.lex["doclen"] if self.lex is not None else None
        for name, col in (getattr(self, "_attrs", None) or {}).items():    # attribute columns (set_attributes)
            arrs["attr:" + name] = col
        return {k: v for k, v in arrs.items() if v is not None}

    def _install_rows(self, rows: Dict[str, Tuple[torch.Tensor, torch.Tensor]]) -> None:
        for name, (_, view) in rows.items():
            if name == "doclen":
                self.lex["doclen"] = view
            elif name.startswith("attr:"):
                self._attrs = dict(self._attrs, **{name[5:]: view})
            else:
                setattr(self, name, view)
        self._store.held.update(rows)

    def _sync_streams(self) -> None:
        """A mutation is not on the query path: queued BM25 / graph work on the side stream and
        dense work on the main one may still read the arrays about to be swapped or extended."""
        torch.cuda.current_stream(self.device).synchronize()
        if self._side is not None:
            self._side.synchronize()
        if self._lex_done is not None:
            self._lex_done.synchronize()

    def capacity_rows(self) -> int:
        """Rows the per-document buffers hold without a reallocation (= n_docs until
        reserve_rows / the first append)."""
        caps = [self._store.behind(k, v).shape[0] for k, v in self._row_arrays().items() if k != "docs16"]
        return min(caps) if caps else 0

    def reserve_rows(self, capacity: int, postings: Optional[int] = None) -> "MutableIndex":
        """Room for ``capacity`` documents in every per-document array (rows, float16 image, norms,
        collections, lengths, token store), so that appends up to there copy nothing old;
        ``postings``: room for that many postings in the destination of the next lexical append.
        The logical sizes, and what the kernels are given, do not change."""
        capacity = int(capacity)
        if capacity > self.n_docs:
            self._sync_streams()
            rows = {}
            for name, view in self._row_arrays().items():
                buf = self._store.with_room(name, view, capacity, exact=True)
                rows[name] = (buf, buf[:view.shape[0]])
            self._install_rows(rows)
        if postings and self.lex is not None:
            sp = self._store.spare
            for name in ("post_doc", "post_tf"):
                if name not in sp or sp[name].shape[0] < postings:
                    sp[name] = torch.empty(int(postings), dtype=torch.int32, device=self.device)
        return self

    def _commit(self, new: _NewState) -> None:
        """Swap a mutation's result in: the one place where the index changes hands."""
        # the buffers the CSRs were read from become the destinations of the next append or delete
        self._store.rotate(new.csr, dict(self.lex or {}, **(self.graph or {})))
        if new.lex is not None:
            self.df_local = self.df_global = new.lex.pop("df")
            self.lex = new.lex
        if new.graph is not None:
            self.graph = new.graph
        if new.entities is not None:
            self.entities = new.entities
        self._install_rows(new.rows)
        if self.docs is not None:
            self.shortlist, self.doc_rel_err = new.shortlist, new.doc_rel_err
            if self.shortlist != "f16":
                self.docs16 = None
                self._store.held.pop("docs16", None)
        self.n_docs = new.n_docs
        # sized or cached for the old row count: the dense workspace (the threshold sample grows
        # with n), the candidate lists of a pending dense_shortlist
        self._ws = None
        self._shortlist_of = None
        self._mutations += 1
        torch.cuda.current_stream(self.device).synchronize()

    # ------------------------------------------------------------ incremental ingest
    # Append in place (DESIGN.md "Incremental ingest"): after append_rows every device array is
    # what a fresh build over all the rows would hold, so the query kernels and their throughput
    # are the fresh build's.  The reference's ingest only ever inserts (rag2/ingest.py:361-470).
    @staticmethod
    def _host_or_device(a, name: str, integer: bool = False, who: str = "append_rows"):
        """``a`` where it lives, as a tensor or a numpy array (host data: no device work)."""
        t = a if isinstance(a, torch.Tensor) else np.asarray(a)
        is_int = not t.dtype.is_floating_point and t.dtype != torch.bool if isinstance(t, torch.Tensor) \
            else np.issubdtype(t.dtype, np.integer)
        if integer and not is_int:
            raise N.NativeError(f"{who}: {name} must be an integer array, got {t.dtype}")
        return t

    def _check_attributes_part(self, attributes, m: int):
        have = set(getattr(self, "_attrs", None) or {})
        if set(attributes) != have:
            raise N.NativeError(f"append_rows: attributes must hold exactly the index's columns {sorted(have)}, "
                                f"got {sorted(attributes)}")
        out = {}
        for name, col in attributes.items():
            c = self._host_or_device(col, f"attributes[{name!r}]", True)
            if tuple(c.shape) != (m,):
                raise N.NativeError(f"append_rows: attributes[{name!r}]: one value per appended row")
            out[name] = c
        return out

    def _validate_append(self, docs, lex, collections, tokens, mentions, n_rows, attributes=None) -> dict:
        """Everything about an append that can be refused before any device work: which parts are
        required (exactly the channels the index has), shapes, dtypes, id ranges.  -> the parts as
        tensors where the caller left them + the batch size."""
        m, docs = self._check_dense_part(docs, n_rows)
        out = dict(m=m, docs=docs)
        attributes = dict(attributes or {})
        if "collection" in attributes and collections is None:
            collections = attributes.pop("collection")
        for name, have, part, check, required, absent in (
                ("lex", self.lex, lex, self._check_lex_part,
                 "this index has a lexical channel: lex=(doc, term, tf, n_vocab) is required",
                 "this index has no lexical channel: lex must be None"),
                ("collections", self.doc_coll, collections, self._check_collections_part,
                 "this index has collection ids: collections [m] is required",
                 "this index has no collection ids (set_collections)"),
                ("tokens", self.tokens, tokens, self._check_tokens_part,
                 "this index has a token store: tokens [m, d_tokens, tok_dim] is required",
                 "this index has no token store (set_tokens)"),
                ("mentions", self.graph, mentions, self._check_mentions_part,
                 "this index has a graph channel: mentions=(entity, chunk, conf) is required "
                 "(empty arrays when the new chunks mention nothing)",
                 "this index has no graph channel (set_graph)")):
            if (have is None) != (part is None):
                raise N.NativeError("append_rows: " + (required if part is None else absent))
            out[name] = None if part is None else check(part, m)
        if (getattr(self, "_attrs", None) or {}) and not attributes:
            raise N.NativeError("append_rows: this index has attribute columns: attributes={name: [m]} is required")
        out["attributes"] = self._check_attributes_part(attributes, m)
        return out

    def _check_collections_part(self, collections, m: int):
        c = self._host_or_device(collections, "collections", True)
        if tuple(c.shape) != (m,):
            raise N.NativeError("append_rows: collections: one id per appended row")
        return c

    def _check_tokens_part(self, tokens, m: int):
        tk = self._host_or_device(tokens, "tokens")
        if tk.ndim != 3 or tk.shape[0] != m or tuple(tk.shape[1:]) != tuple(self.tokens.shape[1:]):
            raise N.NativeError(f"append_rows: tokens must be [{m}, {self.tokens.shape[1]}, {self.tokens.shape[2]}]")
        # (set_tokens applies the same check: this one holds for a store that came another way)
        check = N.maxsim_fp8_check_tokens if self.token_store == "fp8" else N.maxsim_check_tokens
        check("append_rows: tokens", int(tk.shape[2]), int(tk.shape[1]))
        return tk

    def _check_dense_part(self, docs, n_rows):
        """-> (batch size, docs where the caller left them or None)."""
        E = N.NativeError
        if self.docs is not None:
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
        return m, docs

    def _check_lex_part(self, lex, m: int):
        E = N.NativeError
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
        return d, t, f, n_vocab

    def _check_mentions_part(self, mentions, m: int):
        E = N.NativeError
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
                        "(append_graph adds entities)")
            if int(c.min()) < 0 or int(c.max()) >= m:
                raise E(f"append_rows: mention chunk ids are local to the batch, 0 .. {m - 1}")
        return e, c, w

    def _dense_flavour_after(self, new: torch.Tensor, n_new: int):
        """What set_dense would decide for the rows so far + ``new``, without touching the index:
        -> (shortlist, float16 image of the tail tiles or None, doc_rel_err, first row of the tail)."""
        n_old, cur = self.n_docs, self.shortlist
        t0 = n_old // 32 * 32     # the last partially filled tile of 32 rows is re-quantised
        if cur not in ("f16", "f16-inline", "f16-anydim"):
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
        elif want in ("f16-inline", "f16-anydim"):    # ("f16-anydim" is never auto: want is cur)
            _, err = N.dense_quantize_f16(new, keep_copy=False)
            # (the copy's error is measured on the normalised rows: the in-flight rounding's is not)
            old = self.doc_rel_err if cur != "f16" else N.dense_quantize_f16(self.docs, keep_copy=False)[1]
            err = max(err, old)
        if want != "f32" and (not np.isfinite(err) or err > self.F16_MAX_REL_ERR):
            if not self._shortlist_auto:
                raise N.NativeError("append_rows: the new rows do not fit float16 (values >= 65504 or mostly "
                                    "below 6e-5 in magnitude): build the index with shortlist='f32'")
            want = "f32"
        if want == "f32":
            tail16, err = None, 0.0
        return want, tail16, err, t0

    def _extend(self, new: _NewState, name: str, view: torch.Tensor, tail: torch.Tensor, first: int) -> torch.Tensor:
        """Write ``tail`` from row ``first`` on behind (docs16: over the last tile of) the rows of
        ``view``, in a buffer with room for new.n_docs documents -> the extended view."""
        S = self._store
        buf = S.with_room(name, view, new.n_docs)
        rows = S.padded(name, new.n_docs)
        buf[first:rows].copy_(tail)
        new.rows[name] = (buf, buf[:rows])
        return new.rows[name][1]

    @_refuse_when_unusable
    def append_rows(self, docs, lex=None, collections=None, tokens=None, mentions=None,
                    n_rows: Optional[int] = None, attributes=None) -> range:
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
          attributes  {name: int32 [m]} for exactly the columns set_attributes gave the index
                      ("collection" may come here instead of ``collections``);
          mentions    (entity, chunk, conf or None): entity ids of EXISTING entities, chunk ids
                      local to the batch, in any order (stored by entity, then chunk, stably: the
                      order index_build.build_graph gives the same rows).
        Each part is required exactly when the index has that channel.  Everything is validated
        before the first change and the new arrays are swapped in last (_commit): a failure leaves
        the index answering over the old rows.  Synchronises the main and the side stream (not a
        query-path call).  Not supported on a document shard of a sharded index."""
        P = self._validate_append(docs, lex, collections, tokens, mentions, n_rows, attributes)
        m, n_old = P["m"], self.n_docs
        if m == 0:
            return range(n_old, n_old)
        new = _NewState(n_old + m)
        # ---- dense rows: norms of the new rows, float16 image of the tail tiles
        tail16 = None
        if self.docs is not None:
            rows = self._t(P["docs"], torch.float32)
            new.shortlist, tail16, new.doc_rel_err, t0 = self._dense_flavour_after(rows, new.n_docs)
            dn, inv = N.doc_norms(rows)
            self._sync_streams()
            for name, tail in (("docs", rows), ("dnorm", dn), ("inv_norm", inv)):
                self._extend(new, name, getattr(self, name), tail, n_old)
        else:
            self._sync_streams()
        if P["collections"] is not None:
            self._extend(new, "doc_coll", self.doc_coll, self._t(P["collections"], torch.int32), n_old)
        for name, col in P["attributes"].items():
            self._extend(new, "attr:" + name, self._attrs[name], self._t(col, torch.int32), n_old)
        if P["tokens"] is not None:
            tok = self._t(P["tokens"], torch.float16)
            if self.token_store == "fp8":   # (quantised per token: the batch's image is a fresh build's rows)
                tok, scales = N.maxsim_quantize_fp8(tok)
                self._extend(new, "token_scales", self.token_scales, scales, n_old)
            elif self.tokens_packed:
                tok = N.maxsim_pack(tok)
            self._extend(new, "tokens", self.tokens, tok, n_old)     # (the packed layouts are doc-local)
        if P["lex"] is not None:
            self._append_lexical(P["lex"], n_old, new)
        if P["mentions"] is not None:
            self._append_mentions(P["mentions"], n_old, new)
        if tail16 is not None:    # last: the one write that lands inside the old logical extent
            self._extend(new, "docs16", self.docs16, tail16, t0)    # (the old last tile's NaN padding becomes rows)
        self._commit(new)
        return range(n_old, new.n_docs)

    def _csr_append(self, new: _NewState, csr: dict, keys: Tuple[str, str, str], rowptr_b, ids_b, pay_b):
        """thr_csr_append of a batch's CSR behind the one ``csr`` holds under ``keys`` (row pointers,
        ids, payload), out of place -> (rowptr, ids, payload) of the result."""
        kr, k0, k1 = keys
        nnz = csr[k0].shape[0] + ids_b.shape[0]
        dest = [self._store.destination(k, csr[k], nnz, grow=True) for k in (k0, k1)]
        rowptr, out0, out1, _ = N.csr_append(csr[kr], csr[k0], csr[k1], rowptr_b, ids_b, pay_b, *dest)
        new.csr[k0], new.csr[k1] = (out0, out0[:nnz]), (out1, out1[:nnz])
        return rowptr, new.csr[k0][1], new.csr[k1][1]

    def _append_lexical(self, lex, n_old: int, new: _NewState) -> None:
        """The lexical side after the append, as a new ``lex`` dict (the old one is untouched)."""
        d, t, f, n_vocab = lex
        L = self.lex
        # the delta CSR over the new rows, doc ids already in the index's numbering: no sort of old postings
        rp_b, pd_b, ptf_b, dl_full, _ = N.lexical_build(
            self._t(d, torch.int32) + n_old, self._t(t, torch.int32),
            None if f is None else self._t(f, torch.int32), new.n_docs, n_vocab)
        rowptr, post_doc, post_tf = self._csr_append(new, L, self.LEX_CSR, rp_b, pd_b, ptf_b)
        doclen = self._extend(new, "doclen", L["doclen"], dl_full[n_old:], n_old)
        new.lex = self._lexical_derived(rowptr, post_doc, post_tf, doclen)

    def _append_mentions(self, mentions, n_old: int, new: _NewState) -> None:
        """The graph side after the append (entity CSR unchanged)."""
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
        new.graph = self._graph_with(*self._csr_append(new, G, self.GRAPH_CSR, rp_b, mc_b, mw_b))

    # ------------------------------------------------------------ graph ingest
    # New entities, relations and mentions of chunks that are already stored (DESIGN.md "Graph
    # ingest"): what the reference's entity extraction writes behind a document's chunk inserts
    # (rag2/entity_extraction.py:449-554).  Afterwards every graph array and the name store are what
    # index_build.build_graph over the old rows followed by the new ones, set_graph and
    # set_entity_names would hold: thr_csr_merge is that build's stable sort, row by row.
    CANONICAL = ("the index's graph is not in index_build.build_graph's canonical form (relations sorted by "
                 "(src, dst) without duplicates, mentions chunk-ascending within an entity): it came through "
                 "set_graph from other arrays and cannot be merged into -- rebuild it with build_graph")

    def _graph_or_refuse(self, who: str) -> dict:
        if self.graph is None:
            raise N.NativeError(f"{who}: this index has no graph channel (set_graph)")
        return self.graph

    def _merge_or_refuse(self, who: str, *a, **kw):
        """thr_csr_merge; a status word that names an input is an error, not a graph to commit."""
        rowptr, ids, pay, nnz, status = N.csr_merge(*a, check=False, **kw)
        if status & N.THR_CSR_MERGE_UNSORTED_A:
            raise N.NativeError(f"{who}: {self.CANONICAL}")
        if status:
            raise N.NativeError(f"{who}: thr_csr_merge: {N.csr_merge_status_message(status)}")
        return rowptr, ids, pay, nnz

    def _validate_append_graph(self, entity_names, n_new_entities, relations):
        """What append_graph refuses before any device work -> (m, names or None, subject, object)."""
        E, who = N.NativeError, "append_graph"
        G = self._graph_or_refuse(who)
        n_ent = int(G["men_rowptr"].shape[0]) - 1
        names = None if entity_names is None else [str(nm) for nm in entity_names]
        if names is not None and n_new_entities is not None and int(n_new_entities) != len(names):
            raise E(f"{who}: n_new_entities differs from the number of entity names")
        m = len(names) if names is not None else int(n_new_entities or 0)
        if m < 0 or n_ent + m > (1 << 31) - 2:
            raise E(f"{who}: entity count out of range")
        if self.entities is not None and names is None and m > 0:
            raise E(f"{who}: this index holds entity names (set_entity_names): entity_names for the "
                    f"{m} new entities are required")
        if self.entities is None and names and n_ent > 0:
            raise E(f"{who}: entity_names given, but the index holds no names for its {n_ent} entities "
                    "(set_entity_names first, or pass n_new_entities)")
        s = o = None
        if relations is not None and len(relations) != 2:
            raise E(f"{who}: relations is (subject, object)")
        if relations is not None and (self._size(relations[0]) or self._size(relations[1])):
            s = self._host_or_device(relations[0], "relation subject", True, who).reshape(-1)
            o = self._host_or_device(relations[1], "relation object", True, who).reshape(-1)
            if s.shape != o.shape:
                raise E(f"{who}: relation subject / object are 1-d arrays of one length")
            if s.shape[0] and (min(int(s.min()), int(o.min())) < 0 or max(int(s.max()), int(o.max())) >= n_ent + m):
                raise ValueError(f"{who}: relation endpoints are entity ids, 0 .. {n_ent + m - 1} "
                                 f"({n_ent} existing + {m} new)")
        return m, names, s, o

    @staticmethod
    def _size(a) -> int:
        return int(a.numel()) if isinstance(a, torch.Tensor) else int(np.asarray(a).size)

    def _names_with(self, names: List[str]) -> dict:
        """The name store after ``names`` were added: byte for byte pack_entity_names(all names) -- the
        old bytes up to name_ptr[E], the new names lower-cased with one 0xFF each, the padding at the
        new end -- without the old names coming back to the host."""
        from .index_entities import pack_entity_names
        blob, ptr = pack_entity_names(names)
        Ent = self.entities
        if Ent is None:
            return dict(name_bytes=self._t(blob, torch.uint8), name_ptr=self._t(ptr, torch.int64), n=len(names))
        used = int(Ent["name_bytes"].shape[0]) - N.THR_ENTITY_MAX_NEEDLE      # = name_ptr[E]
        return dict(name_bytes=torch.cat([Ent["name_bytes"][:used], self._t(blob, torch.uint8)]),
                    name_ptr=torch.cat([Ent["name_ptr"], self._t(ptr[1:] + used, torch.int64)]),
                    n=Ent["n"] + len(names))

    @staticmethod
    def _rows_grown(rowptr: torch.Tensor, m: int) -> torch.Tensor:
        """``rowptr`` with m empty rows behind the last."""
        return rowptr if m == 0 else torch.cat([rowptr, rowptr[-1:].expand(m)])

    @_refuse_when_unusable
    def append_graph(self, entity_names=None, n_new_entities: Optional[int] = None, relations=None) -> range:
        """New entities and relations into the live index -> the range of the new entity ids.
          entity_names    names of the m new entities: they get the ids E .. E+m-1.  Required when the
                          index holds entity names (set_entity_names): the device name store becomes,
                          byte for byte, pack_entity_names(all names).  An index with a graph but
                          without names takes ``n_new_entities`` = m instead;
          relations       (subject, object): int arrays of entity ids, old or new.  As build_graph
                          treats them: both directions, self-loops dropped, duplicates -- inside the
                          batch or of an edge the index holds -- dropped.
        Afterwards ent_rowptr / ent_col / men_rowptr (and the name store) are, to the bit, what
        build_graph over the old rows followed by the new ones, set_graph and set_entity_names would
        hold; the new entities' rows are empty until relations or mentions arrive (append_mentions,
        append_rows(mentions=)).  The mentions are carried over.  Everything is validated before the
        first change and swapped in last (_commit): a refused call -- an endpoint outside the entity
        ids (ValueError), a graph that is not in build_graph's canonical form -- leaves the index
        answering over the old graph.  One host read of the merged edge count.  Synchronises the
        main and the side stream (not a query-path call).  Nothing to add: a no-op."""
        who = "append_graph"
        m, names, s, o = self._validate_append_graph(entity_names, n_new_entities, relations)
        G = self.graph
        n_ent = int(G["men_rowptr"].shape[0]) - 1
        if m == 0 and s is None:
            return range(n_ent, n_ent)
        n_all = n_ent + m
        self._sync_streams()
        new = _NewState(self.n_docs, shortlist=self.shortlist, doc_rel_err=self.doc_rel_err)
        ent_rowptr, ent_col = self._rows_grown(G["ent_rowptr"], m), G["ent_col"]
        if s is not None:
            s, o = self._t(s, torch.int64), self._t(o, torch.int64)
            real = s != o
            s, o = s[real], o[real]
            # both directions, unique and sorted by (src, dst): build_graph's np.unique over the pairs
            key = torch.unique(torch.cat([s * n_all + o, o * n_all + s]))
            src, dst = key // n_all, (key % n_all).to(torch.int32).contiguous()
            rp_b = torch.zeros(n_all + 1, dtype=torch.int64, device=self.device)
            rp_b[1:] = torch.cumsum(torch.bincount(src, minlength=n_all), 0)
            dest = self._store.destination("ent_col", ent_col, int(ent_col.shape[0] + dst.shape[0]), grow=True)
            ent_rowptr, out, _, nnz = self._merge_or_refuse(who, G["ent_rowptr"], ent_col, None, rp_b, dst, None,
                                                            True, ids_out=dest)
            new.csr["ent_col"] = (out, out[:nnz])
            ent_col = new.csr["ent_col"][1]
        new.graph = dict(ent_rowptr=ent_rowptr, ent_col=ent_col, men_rowptr=self._rows_grown(G["men_rowptr"], m),
                         men_chunk=G["men_chunk"], men_conf=G["men_conf"])
        if names:
            new.entities = self._names_with(names)
        self._commit(new)
        return range(n_ent, n_all)

    @_refuse_when_unusable
    def append_mentions(self, entity, chunk, conf=None) -> None:
        """Mentions of chunks the index already holds.  ``entity``: ids of existing entities (those of
        an earlier append_graph included), ``chunk``: LOCAL doc ids 0 .. n_docs-1 (stored as
        + doc_base), ``conf``: float per mention, 1.0 when None; any order, repeats are kept.  The
        batch is sorted by (entity, chunk), stably, and merged into the entity-major mention CSR with
        thr_csr_merge: afterwards men_rowptr / men_chunk / men_conf are, to the bit, what build_graph
        over the old mention rows followed by these would hold.  Validated before the first change,
        swapped in last; a refused call leaves the index answering over the old graph.  Synchronises
        the main and the side stream (not a query-path call)."""
        E, who = N.NativeError, "append_mentions"
        G = self._graph_or_refuse(who)
        if not (self._size(entity) or self._size(chunk) or (conf is not None and self._size(conf))):
            return
        e = self._host_or_device(entity, "entity", True, who).reshape(-1)
        c = self._host_or_device(chunk, "chunk", True, who).reshape(-1)
        w = None if conf is None else self._host_or_device(conf, "conf", who=who).reshape(-1)
        if c.shape != e.shape or (w is not None and w.shape != e.shape):
            raise E(f"{who}: entity / chunk / conf are 1-d arrays of one length")
        if not e.shape[0]:
            return
        n_ent = int(G["men_rowptr"].shape[0]) - 1
        if int(e.min()) < 0 or int(e.max()) >= n_ent:
            raise ValueError(f"{who}: entity ids are existing entities, 0 .. {n_ent - 1} (append_graph adds entities)")
        if int(c.min()) < 0 or int(c.max()) >= self.n_docs:
            raise ValueError(f"{who}: chunk ids are local doc ids of stored chunks, 0 .. {self.n_docs - 1}")
        self._sync_streams()
        e, c = self._t(e, torch.int64), self._t(c, torch.int64)
        w = torch.ones(e.shape[0], dtype=torch.float32, device=self.device) if w is None else self._t(w, torch.float32)
        order = torch.sort(c, stable=True).indices
        order = order[torch.sort(e[order], stable=True).indices]
        rp_b = torch.zeros(n_ent + 1, dtype=torch.int64, device=self.device)
        rp_b[1:] = torch.cumsum(torch.bincount(e, minlength=n_ent), 0)
        mc_b = (c[order] + self.doc_base).to(torch.int32).contiguous()
        mw_b = w[order].contiguous()
        new = _NewState(self.n_docs, shortlist=self.shortlist, doc_rel_err=self.doc_rel_err)
        nnz = int(G["men_chunk"].shape[0] + mc_b.shape[0])
        d0, d1 = (self._store.destination(k, G[k], nnz, grow=True) for k in ("men_chunk", "men_conf"))
        rowptr, out0, out1, nnz = self._merge_or_refuse(who, G["men_rowptr"], G["men_chunk"], G["men_conf"], rp_b,
                                                        mc_b, mw_b, False, ids_out=d0, pay_out=d1)
        new.csr["men_chunk"], new.csr["men_conf"] = (out0, out0[:nnz]), (out1, out1[:nnz])
        # (a fresh dict: the chunk-major copy cached in the old one is keyed on n_docs, which stays)
        new.graph = self._graph_with(rowptr, new.csr["men_chunk"][1], new.csr["men_conf"][1])
        self._commit(new)

    # ------------------------------------------------------------ graph delete
    # Entities, relations and mentions out of the live index (DESIGN.md "Graph delete"): what the
    # reference's schema does by cascade when a document or an entity row is deleted
    # (20260114_rag2_schema.sql:187, 217-220, 254, 258-259).  Afterwards every graph array and the
    # name store are what index_build.build_graph over the surviving rows, set_graph and
    # set_entity_names would hold: thr_csr_prune drops and renumbers in one order-preserving pass.
    def _ids_part(self, a, name: str, who: str, lo: int, hi: int, what: str):
        """``a`` flat, where the caller left it, every value in [lo, hi) (ValueError) -> the array or None (empty)."""
        if a is None or not self._size(a):
            return None
        t = self._host_or_device(a, name, True, who).reshape(-1)
        if int(t.min()) < lo or int(t.max()) >= hi:
            raise ValueError(f"{who}: {name}: {what}")
        return t

    def _validate_delete_graph(self, entities, relations, mentions):
        """What delete_graph refuses before any device work -> (entities, (subject, object), (entity, chunk)),
        each flat where the caller left it, or None."""
        E, who = N.NativeError, "delete_graph"
        G = self._graph_or_refuse(who)
        n_ent = int(G["men_rowptr"].shape[0]) - 1
        ents = self._ids_part(entities, "entities", who, 0, n_ent, f"entity ids are 0 .. {n_ent - 1}")
        pairs = []
        for part, name, los, his, says in (
                (relations, "relations", (0, 0), (n_ent, n_ent),
                 (f"relation endpoints are entity ids, 0 .. {n_ent - 1}",) * 2),
                (mentions, "mentions", (-1, -1), (n_ent, self.n_docs),
                 (f"entity ids are 0 .. {n_ent - 1} (-1: every entity)",
                  f"chunk ids are local doc ids, 0 .. {self.n_docs - 1} (-1: every chunk)"))):
            if part is None:
                pairs.append(None)
                continue
            if len(part) != 2:
                raise E(f"{who}: {name} is a pair of id arrays")
            if self._size(part[0]) != self._size(part[1]):
                raise E(f"{who}: the two arrays of {name} are 1-d arrays of one length")
            a = self._ids_part(part[0], f"{name}[0]", who, los[0], his[0], says[0])
            b = self._ids_part(part[1], f"{name}[1]", who, los[1], his[1], says[1])
            if name == "mentions" and a is not None and bool(((a < 0) & (b < 0)).any()):
                raise ValueError(f"{who}: a mention names an entity, a chunk or both ((-1, -1) names nothing)")
            pairs.append(None if a is None else (a, b))
        if ents is not None:
            uniq = int(torch.unique(ents).numel()) if isinstance(ents, torch.Tensor) else int(np.unique(ents).size)
            if uniq >= n_ent:
                raise E(f"{who}: every entity would be deleted: build a new index")
        return ents, pairs[0], pairs[1]

    def _pairs_csr(self, rows: torch.Tensor, ids: torch.Tensor, n_rows: int):
        """(row, id) pairs, int64 on the device, ids in [0, 2^31) -> (rowptr, ids int32): sorted by
        (row, id) without duplicates, thr_csr_prune's B."""
        key = torch.unique((rows << 32) | ids)
        rp = torch.zeros(n_rows + 1, dtype=torch.int64, device=self.device)
        rp[1:] = torch.cumsum(torch.bincount(key >> 32, minlength=n_rows), 0)
        return rp, (key & 0xFFFFFFFF).to(torch.int32).contiguous()

    def _prune_or_refuse(self, who: str, *a, **kw):
        rowptr, ids, pay, nnz, status, _ = N.csr_prune(*a, check=False, **kw)
        if status:
            raise N.NativeError(f"{who}: thr_csr_prune: {N.csr_prune_status_message(status)}")
        return rowptr, ids, pay, nnz

    def _names_without(self, keep: torch.Tensor, n_new: int) -> dict:
        """The name store without the removed entities' names: byte for byte pack_entity_names(surviving
        names) -- each kept name's bytes with its 0xFF, in order, the padding moved to the new end -- by
        device tensor operations; no name comes back to the host."""
        Ent = self.entities
        used = int(Ent["name_bytes"].shape[0]) - N.THR_ENTITY_MAX_NEEDLE      # = name_ptr[E]
        lens = Ent["name_ptr"][1:] - Ent["name_ptr"][:-1]
        of_kept = keep[torch.repeat_interleave(lens, output_size=used)]      # per byte: does its name stay?
        ptr = torch.zeros(n_new + 1, dtype=torch.int64, device=self.device)
        ptr[1:] = torch.cumsum(lens[keep], 0)
        return dict(name_bytes=torch.cat([Ent["name_bytes"][:used][of_kept], Ent["name_bytes"][used:]]),
                    name_ptr=ptr, n=n_new)

    def graph_rows_host(self, which: str, entities=None):
        """Rows of the entity CSR (``which`` = "relations") or of the mention CSR ("mentions") on the host ->
        (rowptr int64 [len(entities) + 1], ids, conf float32 or None): the rows of ``entities`` in the order
        given (None: every row); ids are entity ids, or LOCAL chunk ids.  What the drop-in client builds a
        delete's reply from; one gather and one read-back, not a query-path call."""
        G = self._graph_or_refuse("graph_rows_host")
        kr, k0, k1 = ("ent_rowptr", "ent_col", None) if which == "relations" else self.GRAPH_CSR
        rp, ids, pay = G[kr], G[k0], None if k1 is None else G[k1]
        base = 0 if which == "relations" else self.doc_base
        if entities is not None:
            es = self._t(np.asarray(entities, dtype=np.int64).reshape(-1), torch.int64)
            lo, n = rp[es], rp[es + 1] - rp[es]
            ends = torch.cumsum(n, 0)
            total = int(ends[-1].item()) if es.shape[0] else 0
            at = torch.repeat_interleave(lo - (ends - n), n, output_size=total) + \
                torch.arange(total, dtype=torch.int64, device=self.device)
            rp = torch.cat([torch.zeros(1, dtype=torch.int64, device=self.device), ends])
            ids, pay = ids[at], None if pay is None else pay[at]
        return (rp.cpu().numpy(), ids.cpu().numpy().astype(np.int64) - base, None if pay is None else pay.cpu().numpy())

    @_refuse_when_unusable
    def delete_graph(self, entities=None, relations=None, mentions=None) -> torch.Tensor:
        """Entities, relations and mentions out of the live index -> the int32 [E_old] remap on the
        device: old entity id -> new id, -1 = deleted (a caller that holds seed tables renumbers
        them with it).
          entities   entity ids, any order, repeats allowed: each leaves with its relations, in both
                     directions, and its mentions; the survivors are renumbered ascending;
          relations  (subject, object) id arrays: the edge between each pair goes, in both
                     directions (the index keeps the undirected set union of the relation rows, so
                     the edge is what can be removed); a pair that names no edge, or a self pair,
                     is ignored;
          mentions   (entity, chunk) with LOCAL chunk ids: every mention of that pair goes;
                     chunk = -1: every mention of the entity; entity = -1: every mention of the
                     chunk (the chunk itself stays).
        One call may combine all three; the result does not depend on their order: a row is gone
        if any argument names it.  Afterwards ent_rowptr / ent_col / men_rowptr / men_chunk /
        men_conf and the name store are, to the bit, what build_graph over the surviving rows in
        their old order, set_graph and set_entity_names would hold.  Everything is validated before
        the first change (no graph, ids outside the entity / chunk range: ValueError, arrays of
        unequal length, every entity deleted: build a new index), written out of place and swapped
        in last (_commit): a refused or failed call leaves the index answering over the old graph.
        Two host reads of kept counts.  Synchronises the main and the side stream (not a query-path
        call)."""
        who = "delete_graph"
        ents, rel, men = self._validate_delete_graph(entities, relations, mentions)
        G = self.graph
        n_ent = int(G["men_rowptr"].shape[0]) - 1
        if ents is None and rel is None and men is None:
            return torch.arange(n_ent, dtype=torch.int32, device=self.device)
        self._sync_streams()
        keep = torch.ones(n_ent, dtype=torch.bool, device=self.device)
        if ents is not None:
            keep[self._t(ents, torch.int64)] = False
        rank = torch.cumsum(keep, 0, dtype=torch.int32) - 1
        remap = torch.where(keep, rank, torch.full_like(rank, -1))
        n_new = int(keep.sum().item())
        rows = dict(row_remap=remap, rows_out=n_new) if ents is not None else {}
        new = _NewState(self.n_docs, shortlist=self.shortlist, doc_rel_err=self.doc_rel_err)
        # ---- relations: the entity CSR, rows and ids renumbered alike, the named edges in both directions
        ent_rowptr, ent_col = G["ent_rowptr"], G["ent_col"]
        rp_b = ids_b = None
        if rel is not None:
            s, o = self._t(rel[0], torch.int64), self._t(rel[1], torch.int64)
            rp_b, ids_b = self._pairs_csr(torch.cat([s, o]), torch.cat([o, s]), n_ent)
        if ents is not None or rel is not None:
            dest = self._store.destination("ent_col", ent_col, int(ent_col.shape[0]), grow=False)
            ent_rowptr, out, _, nnz = self._prune_or_refuse(who, ent_rowptr, ent_col, None, id_remap=remap if ents is not None else None,
                                                            rowptr_b=rp_b, ids_b=ids_b, ids_out=dest, **rows)
            new.csr["ent_col"] = (out, out[:nnz])
            ent_col = new.csr["ent_col"][1]
        # ---- mentions: rows renumbered, chunks named alone masked by id, pairs through B
        men_rowptr, men_chunk, men_conf = (G[k] for k in self.GRAPH_CSR)
        rp_b = ids_b = chunk_mask = None
        if men is not None:
            e, c = self._t(men[0], torch.int64), self._t(men[1], torch.int64)
            every_chunk, every_entity = c < 0, e < 0
            if bool(every_entity.any()):
                chunk_mask = torch.arange(self.n_docs, dtype=torch.int32, device=self.device)
                chunk_mask[c[every_entity]] = -1
            pe, pc = e[~every_chunk & ~every_entity], c[~every_chunk & ~every_entity] + self.doc_base
            if bool(every_chunk.any()):        # every mention the entity has: its row's own chunk ids
                es = torch.unique(e[every_chunk])
                lo, n = men_rowptr[es], men_rowptr[es + 1] - men_rowptr[es]
                total = int(n.sum().item())
                at = torch.repeat_interleave(lo - (torch.cumsum(n, 0) - n), n, output_size=total) + \
                    torch.arange(total, dtype=torch.int64, device=self.device)
                pe = torch.cat([pe, torch.repeat_interleave(es, n, output_size=total)])
                pc = torch.cat([pc, men_chunk[at].to(torch.int64)])
            if pe.shape[0]:
                rp_b, ids_b = self._pairs_csr(pe, pc, n_ent)
        if ents is not None or rp_b is not None or chunk_mask is not None:
            d0, d1 = (self._store.destination(k, G[k], int(G[k].shape[0]), grow=False) for k in ("men_chunk", "men_conf"))
            men_rowptr, out0, out1, nnz = self._prune_or_refuse(who, men_rowptr, men_chunk, men_conf, id_remap=chunk_mask,
                                                                id_base=self.doc_base, rowptr_b=rp_b, ids_b=ids_b,
                                                                ids_out=d0, pay_out=d1, **rows)
            new.csr["men_chunk"], new.csr["men_conf"] = (out0, out0[:nnz]), (out1, out1[:nnz])
            men_chunk, men_conf = new.csr["men_chunk"][1], new.csr["men_conf"][1]
        # (a fresh dict: the chunk-major copy of the mentions cached in the old one is not reused)
        new.graph = self._graph_with(men_rowptr, men_chunk, men_conf, ent_rowptr, ent_col)
        if self.entities is not None and ents is not None:
            new.entities = self._names_without(keep, n_new)
        self._commit(new)
        return remap

    # ------------------------------------------------------------ delete
    # Delete in place (DESIGN.md "Delete in place"): after delete_rows every device array is what a
    # fresh build over the surviving rows, in their old order, would hold -- the delete pays, the query
    # path does not change.  The store this index stands in for deletes by cascade
    # (20260114_rag2_schema.sql:65-66, 106-108, 187, 217-218; tests/test_rag2_e2e.py:276-293).
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
        Phase 2 (_move_rows, _commit) only copies inside buffers that already exist: the float32
        rows and the token store are compacted IN PLACE from the first deleted row on, in ascending
        chunks through the staging buffer (every source row lies at or behind its destination, so
        nothing is read after it was overwritten), the float16 image is re-quantised from the tile
        of the first deleted row on; then the new views and the row count are swapped in.  It
        allocates no device memory (every buffer it writes, the error slots included, exists by
        then).  An exception out of phase 2 (a HIP error) leaves rows half moved: the index marks
        itself unusable and every later search, append or delete raises.

        Synchronises the main and the side stream first (not a query-path call): a query running
        concurrently on another stream is excluded by that, exactly as for the float16 tail write
        of append_rows.  The backing buffers keep their capacity for later appends.  Not supported
        on a document shard of a sharded index."""
        n_old = self.n_docs
        t = self._validate_delete(ids)
        if t is None:
            return torch.arange(n_old, dtype=torch.int32, device=self.device)
        # ---- phase 1: nothing a query reads is written
        self._sync_streams()
        keep = torch.ones(n_old, dtype=torch.bool, device=self.device)
        keep[self._t(t, torch.int64)] = False
        src = keep.nonzero().reshape(-1)          # new id -> old id, ascending
        rank = torch.cumsum(keep, 0, dtype=torch.int32) - 1
        remap = torch.where(keep, rank, torch.full_like(rank, -1))
        new = _NewState(int(src.shape[0]), shortlist=self.shortlist, doc_rel_err=self.doc_rel_err)
        self._gather_small_rows(src, new)
        self._compact_csrs(remap, new)
        plan = self._plan_moves(int(t.min()), src, new)
        torch.cuda.current_stream(self.device).synchronize()    # (an asynchronous failure of phase 1 surfaces here)
        # ---- phase 2: in-place row moves inside existing buffers, then the swap; no device allocation
        try:
            err = self._move_rows(plan)
            if err is not None:
                new.doc_rel_err = err
            self._commit(new)
        except BaseException as exc:
            self._unusable = ("this index is unusable: a delete failed while rows were being moved in place "
                              f"({type(exc).__name__}: {exc}); build a new index")
            raise
        return remap

    def _validate_delete(self, ids):
        """What can be refused before any device work -> the ids, flat, where the caller left them
        (None: nothing to delete, also a plain [])."""
        E = N.NativeError
        n_old = self.n_docs
        if self._lex_global:
            raise E("delete_rows: not supported on a document shard (idf / avgdl are the whole corpus': "
                    "the delete needs a collective df / length all-reduce)")
        if (ids.numel() if isinstance(ids, torch.Tensor) else np.asarray(ids).size) == 0:
            return None
        t = self._host_or_device(ids, "ids", integer=True, who="delete_rows").reshape(-1)
        if int(t.min()) < 0 or int(t.max()) >= n_old:
            raise E(f"delete_rows: ids are local doc ids, 0 .. {n_old - 1}")
        uniq = int(torch.unique(t).numel()) if isinstance(t, torch.Tensor) else int(np.unique(t).size)
        if uniq >= n_old:
            raise E("delete_rows: every row would be deleted: build a new index")
        return t

    def _gather_small_rows(self, src: torch.Tensor, new: _NewState) -> None:
        """The survivors of the small per-row arrays (norms, collections, lengths), out of place."""
        for name, view in self._row_arrays().items():
            if name in ("docs", "docs16", "tokens"):
                continue
            buf = torch.empty_like(self._store.behind(name, view))     # (4 - 8 bytes a row; keeps the capacity)
            torch.index_select(view, 0, src, out=buf[:new.n_docs])
            new.rows[name] = (buf, buf[:new.n_docs])

    def _csr_compact(self, new: _NewState, csr: dict, keys: Tuple[str, str, str], remap: torch.Tensor, id_base: int):
        """thr_csr_compact of the CSR ``csr`` holds under ``keys``, out of place (room for every old
        entry: the kept count is the kernel's result) -> (rowptr, ids, payload) of the result."""
        kr, k0, k1 = keys
        dest = [self._store.destination(k, csr[k], csr[k].shape[0], grow=False) for k in (k0, k1)]
        rowptr, out0, out1, kept = N.csr_compact(csr[kr], csr[k0], csr[k1], remap, id_base, *dest)
        new.csr[k0], new.csr[k1] = (out0, out0[:kept]), (out1, out1[:kept])
        return rowptr, new.csr[k0][1], new.csr[k1][1]

    def _compact_csrs(self, remap: torch.Tensor, new: _NewState) -> None:
        """The postings and the mentions without the deleted chunks, and what follows from the postings."""
        if self.lex is not None:
            rowptr, pd, ptf = self._csr_compact(new, self.lex, self.LEX_CSR, remap, 0)
            new.lex = self._lexical_derived(rowptr, pd, ptf, new.rows["doclen"][1])
        if self.graph is not None:
            new.graph = self._graph_with(*self._csr_compact(new, self.graph, self.GRAPH_CSR, remap, self.doc_base))

    def _plan_moves(self, first: int, src: torch.Tensor, new: _NewState) -> _MovePlan:
        """Which rows of the large arrays (float32 rows, token store) move where, chunk by chunk, and
        every buffer the moves need; with a float16 flavour also the error of the rows that stay,
        measured as the fresh build measures it.  The shorter views go into ``new`` whether or not a
        row moves: rows below the first deleted one stay where they are."""
        S, n_new = self._store, new.n_docs
        t0 = first // 32 * 32                     # the float16 tile of the first deleted row is re-quantised
        moves = []
        per_q = 32        # rows per chunk of the float16 re-measure of the rows that stay
        for name, start in (("docs", t0), ("tokens", first)):
            view = getattr(self, name)
            if view is None:
                continue
            buf = S.behind(name, view)
            new.rows[name] = (buf, buf[:n_new])
            row_bytes = max(1, view[0].numel() * view.element_size())
            per = max(32, self.STAGING_BYTES // row_bytes // 32 * 32)
            if name == "docs":
                per_q = min(per, _tiles32(max(n_new - t0, t0)))
            if start < n_new:                     # (a delete of trailing rows only moves nothing)
                moves.append((name, view, buf, start, min(per, _tiles32(n_new - start))))
        stage = torch.empty(max([per * (buf[0].numel() * buf.element_size()) for _, _, buf, _, per in moves] or [0]),
                            dtype=torch.uint8, device=self.device)
        plan = _MovePlan(src, n_new, moves, stage)
        if self.docs is None or self.shortlist not in ("f16", "f16-inline", "f16-anydim"):
            return plan
        copy = self.shortlist == "f16"            # (else: float32 rows rounded in flight, nothing stored)
        n_tail = sum(len(range(start, n_new, per)) for name, _, _, start, per in moves if name == "docs")
        below = range(0, t0, per_q) if copy else range(0, min(t0, 1))
        plan.errs = torch.zeros(n_tail + len(below), dtype=torch.float32, device=self.device)
        plan.err_tail, err_below = plan.errs[:n_tail], plan.errs[n_tail:]
        plan.err_max = torch.zeros(1, dtype=torch.float32, device=self.device)
        if copy:
            plan.q16 = torch.empty((per_q, self.dim), dtype=torch.float16, device=self.device)
            plan.buf16 = S.behind("docs16", self.docs16)
            new.rows["docs16"] = (plan.buf16, plan.buf16[:S.padded("docs16", n_new)])
        # the rows that do not move: the float16 copy's error on the normalised rows, chunk by chunk
        # into the temporary; the in-flight rounding's in one call
        for j, a in enumerate(below):
            if copy:
                b = min(a + per_q, t0)
                N.dense_quantize_f16_into(self.docs[a:b], plan.q16[:b - a], err_below[j:j + 1])
            else:
                N.dense_quantize_f16_into(self.docs[:t0], None, err_below[j:j + 1])
        return plan

    @staticmethod
    def _move_rows(plan: _MovePlan) -> Optional[float]:
        """Phase 2 of delete_rows: compact the large arrays in place, ascending, through the staging
        buffer; with a float16 flavour re-quantise / re-measure the float32 rows as they pass
        -> the error bound of all surviving rows (None: no float16 flavour, nothing measured).
        Allocates no device memory."""
        for name, view, buf, start, per in plan.moves:
            tmp_all = plan.stage[:per * buf[0].numel() * buf.element_size()].view(buf.dtype).view((per,) + tuple(buf.shape[1:]))
            for j, a in enumerate(range(start, plan.n_new, per)):
                b = min(a + per, plan.n_new)
                tmp = tmp_all[:b - a]
                torch.index_select(view, 0, plan.src[a:b], out=tmp)
                buf[a:b].copy_(tmp)
                if name != "docs" or plan.errs is None:
                    continue
                if plan.q16 is not None:
                    r16 = _tiles32(b - a)    # (the last tile's padding is what a full quantisation writes)
                    N.dense_quantize_f16_into(tmp, plan.q16[:r16], plan.err_tail[j:j + 1])
                    plan.buf16[a:a + r16].copy_(plan.q16[:r16])
                else:
                    N.dense_quantize_f16_into(tmp, None, plan.err_tail[j:j + 1])
        if plan.errs is None:
            return None
        return float(torch.amax(plan.errs, 0, keepdim=True, out=plan.err_max).item())
