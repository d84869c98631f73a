"""Child -> parent expansion on the device (include/thr_hip_parent.h): step 4 of the reference's funnel
(src/voice_agent/rag2/retrieval.py:118-201 -- plan, three channels, weighted RRF, child -> parent expansion,
rerank, safety / denoise).  The reference reranks ``c.parent_text or c.text`` (retrieval.py:419): what is scored
is the parent passage, two children of one parent receive the same score.

The parent of a row is one more int32 attribute column, ``"parent"`` (index_scope.set_attributes): appends,
deletes, save / load and scopes ({"parent": 7}) carry it with no code of their own.  The parent -> children CSR
the scorer walks is a DERIVED CACHE with one owner, ``ParentSearch.parent_csr``: built on first use from the
column, keyed on the column's buffer and the index's mutation count, so any commit drops it.

Not built: a family that straddles document shards (ShardedIndex refuses ``parents=`` / ``expand=``), the
row-major float16 store (set_tokens(pack=False)), and the parent TEXT, which stays a host fetch."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _native as N

PARENT = "parent"                       # the attribute column's name
PARENT_MODES = (None, "rerank", "collapse")


def refuse_on_shards(what: str, **given) -> None:
    """ShardedIndex / ShardedIndexClient: the parent modes are not built there (a family can straddle shards)."""
    for name, value in given.items():
        if value is not None:
            raise NotImplementedError(f"{what}: {name}={value!r} is not built for a document-sharded index: the "
                                      "children of one parent can lie on several shards, and no shard holds the "
                                      "whole family's tokens")


class ParentSearch:
    _parent_csr_of = None       # (the column, its data_ptr, rows, mutations) the cached CSR was built for
    _parent_csr = None          # (par_rowptr int64 [n_parents + 1], par_child int32 [nnz]) or None: no row has a parent

    def set_parents(self, parent_of) -> "ParentSearch":
        """``parent_of`` int32 [n_docs]: the parent number of each row, >= 0, or -1 for a row without a parent
        (values below -1 are refused).  Kept as the attribute column "parent": ``append_rows(attributes={"parent":
        ...})`` names the parents of new chunks, deletes and save / load carry it, ``{"parent": p}`` is a scope."""
        self.set_attributes({PARENT: parent_of})
        return self

    def has_parents(self) -> bool:
        return PARENT in (self._attrs or {})

    def _parent_column(self, what: str) -> torch.Tensor:
        if not self.has_parents():
            raise ValueError(f"{what}: this index has no parent column (set_parents)")
        return self._attrs[PARENT]

    def parent_csr(self) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """The parent -> children CSR of the column (row pointers int64 [n_parents + 1], children int32 ascending
        within a parent), n_parents = 1 + the largest parent number; None when no row has a parent.  Built on
        the device on first use (a stable sort of the rows by parent: index set-up, one read-back of the largest
        number) and kept until the column's buffer or the index's mutation count changes.  (The key holds the
        column tensor itself as well: while the cache lives, no other column can be given the freed address.)"""
        col = self._parent_column("parent_csr")
        key = (col, col.data_ptr(), int(col.shape[0]), getattr(self, "_mutations", 0))
        old = self._parent_csr_of
        if old is None or old[0] is not col or old[1:] != key[1:]:
            rows = torch.nonzero(col >= 0).reshape(-1)
            if rows.numel() == 0:
                csr = None
            else:
                par = col[rows].to(torch.int64)
                n_parents = int(par.max()) + 1
                order = torch.sort(par, stable=True).indices      # ascending rows inside a parent
                rowptr = torch.zeros(n_parents + 1, dtype=torch.int64, device=col.device)
                rowptr[1:] = torch.cumsum(torch.bincount(par, minlength=n_parents), 0)
                csr = (rowptr, rows[order].to(torch.int32).contiguous())
            self._parent_csr, self._parent_csr_of = csr, key
        return self._parent_csr

    def parent_groups(self, ids, counts=None):
        """The groups of each fused row ``ids[q][0 .. counts[q])`` (global ids) -> (leader, slot, uniq_ids,
        n_uniq): thr_hip_parent.h.  Positions of one parent share the leader, the lowest of them."""
        col = self._parent_column("parent_groups")
        return N.parent_groups(self._t(ids, torch.int64), None if counts is None else self._t(counts, torch.int32),
                               col, self.doc_base)

    def parents_of(self, ids: torch.Tensor) -> torch.Tensor:
        """int32, the shape of ``ids``: the parent number of each global id; -1 for padding, another shard's id
        and a row without a parent."""
        col = self._parent_column("parents_of")
        row = ids - self.doc_base
        ok = (ids >= 0) & (row >= 0) & (row < col.shape[0])
        got = col[torch.where(ok, row, torch.zeros_like(row))]
        return torch.where(ok, got, torch.full_like(got, -1))

    def _check_expand(self, what: str, expand) -> bool:
        """-> is the parent score asked for?  Everything about ``expand`` that can be refused before device work."""
        if expand is None:
            return False
        if expand != PARENT:
            raise ValueError(f"{what}: expand must be None or 'parent', got {expand!r}")
        self._parent_column(f"{what}(expand='parent')")
        if self.tokens is None:
            raise ValueError(f"{what}(expand='parent'): this index has no token store (set_tokens)")
        if self.token_store != "fp8" and not self.tokens_packed:
            raise ValueError(f"{what}(expand='parent') reads the PACKED float16 store (set_tokens(pack=True)) or the "
                             "FP8 store: the row-major store is not built")
        return True

    def _maxsim_parent(self, qtok: torch.Tensor, cand_global_ids: torch.Tensor) -> torch.Tensor:
        """The parent score of every candidate: group the row, score one candidate per group, hand the score to
        the group's members through ``slot`` -- siblings share one computed score."""
        cand = self._t(cand_global_ids, torch.int64)
        qtok = self._t(qtok, torch.float16)
        col = self._attrs[PARENT]
        csr = self.parent_csr()
        if csr is None:         # no row has a parent: every family is its row, the plain kernel's walk
            return self.maxsim(qtok, cand)
        nq, n = cand.shape
        out = torch.empty((nq, n), dtype=torch.float32, device=cand.device)
        for lo in range(0, n, N.THR_RRF_MAX_TOP_K):       # (a candidate row wider than a fused list: in pieces)
            part = cand[:, lo:lo + N.THR_RRF_MAX_TOP_K].contiguous()
            _, slot, uniq, _ = N.parent_groups(part, None, col, self.doc_base)
            if self.token_store == "fp8":
                s = N.maxsim_parent_fp8_ids(qtok, self.tokens, self.token_scales, uniq, self.doc_base, col, *csr)
            else:
                s = N.maxsim_parent_ids(qtok, self.tokens, uniq, self.doc_base, col, *csr)
            out[:, lo:lo + N.THR_RRF_MAX_TOP_K] = torch.gather(s, 1, slot.to(torch.int64))
        return out
