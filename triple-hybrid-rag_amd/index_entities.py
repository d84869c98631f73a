"""Seed entities of the graph channel from query keywords, for a whole batch on the device.

The reference looks a query's keywords up one at a time (``rag_entities ... ILIKE '%kw%' LIMIT limit //
len(keywords)``, first 5 keywords, src/voice_agent/rag2/graph_search.py:151-176); the per-query host
restatement is ``match_names`` (``GpuIndexClient.find_entities``).  ``EntitySearch`` is the part of
``GpuIndex`` that holds a device copy of the lower-cased entity names (``set_entity_names``) and resolves
the keyword lists of a batch with one thr_entity_match call (``find_entities``) into the int32
[nq, 16] seed table ``graph_search`` / ``retrieve_batch(query_seeds=)`` take.

What stays on the host is what needs Unicode tables or a dictionary: ``str.lower()`` of names (once) and
keywords (per call), the UTF-8 encoding, the de-duplication of the batch's keywords and the ``per``
arithmetic.  On the lowered strings a code-point substring match IS a byte substring match of the
UTF-8 encodings -- UTF-8 is self-synchronising, a valid needle can only match at a character boundary
-- so the device compares bytes.  Strings are encoded with ("utf-8", "surrogatepass"): a lone
surrogate (Python strings may hold one) becomes its three-byte generalised form, still
self-synchronising and still free of 0xFF, instead of an exception.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _native as N

SEPARATOR = 0xFF     # behind every name: a byte no UTF-8 string holds


def _encode(s: str) -> bytes:
    return s.lower().encode("utf-8", "surrogatepass")


def pack_entity_names(names: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
    """The name store of thr_entity_match -> (bytes uint8, ptr int64 [E + 1]): the lower-cased names'
    UTF-8, each followed by one 0xFF, and THR_ENTITY_MAX_NEEDLE more 0xFF behind the last (the
    kernel's window at the last position stays inside the array).  Name e is
    bytes[ptr[e] : ptr[e + 1] - 1]; ptr[E] is the length without the padding."""
    enc = [_encode(nm) for nm in names]
    ptr = np.zeros(len(enc) + 1, dtype=np.int64)
    if enc:
        np.cumsum(np.fromiter((len(b) + 1 for b in enc), dtype=np.int64, count=len(enc)), out=ptr[1:])
    sep = bytes([SEPARATOR])
    blob = sep.join(enc) + (sep if enc else b"") + sep * N.THR_ENTITY_MAX_NEEDLE
    return np.frombuffer(blob, dtype=np.uint8).copy(), ptr


@dataclass
class NeedlePlan:
    """The host half of a find_entities call: the batch's distinct lowered keywords and who names them."""
    needles: np.ndarray          # uint8 [M, THR_ENTITY_MAX_NEEDLE], zero behind each needle
    needle_len: np.ndarray       # int32 [M]
    query_needles: np.ndarray    # int32 [nq, THR_ENTITY_MAX_KEYWORDS], -1 = none
    query_per: np.ndarray        # int32 [nq]: max(1, limit // len(keywords)) -- the FULL keyword count
    long_rows: List[int] = field(default_factory=list)   # queries with a keyword the kernel cannot take


def plan_needles(keyword_lists: Sequence[Sequence[str]], limit: int = 20) -> NeedlePlan:
    """Lower, encode and de-duplicate the keywords of a batch (queries share keywords: a needle is
    matched once).  Of a query the first THR_ENTITY_MAX_KEYWORDS keywords are used, ``per`` divides by
    all of them (graph_search.py:161, 170).  A query with a used keyword longer than
    THR_ENTITY_MAX_NEEDLE bytes gets no needles and is listed in ``long_rows``."""
    nq = len(keyword_lists)
    qn = np.full((nq, N.THR_ENTITY_MAX_KEYWORDS), -1, dtype=np.int32)
    per = np.ones(nq, dtype=np.int32)
    ids: dict = {}
    long_rows: List[int] = []
    for q, kws in enumerate(keyword_lists):
        if not kws:
            continue
        per[q] = min(max(1, limit // len(kws)), np.iinfo(np.int32).max)
        enc = [_encode(kw) for kw in kws[:N.THR_ENTITY_MAX_KEYWORDS]]
        if any(len(b) > N.THR_ENTITY_MAX_NEEDLE for b in enc):
            long_rows.append(q)
            continue
        for j, b in enumerate(enc):
            qn[q, j] = ids.setdefault(b, len(ids))
    needles = np.zeros((len(ids), N.THR_ENTITY_MAX_NEEDLE), dtype=np.uint8)
    lens = np.zeros(len(ids), dtype=np.int32)
    for b, i in ids.items():
        needles[i, :len(b)] = np.frombuffer(b, dtype=np.uint8)
        lens[i] = len(b)
    return NeedlePlan(needles, lens, qn, per, long_rows)


def name_trigrams(entity_names: Sequence[str]):
    """-> (sorted trigram codes, entity of each, lowered names): a keyword intersects lists, no scan of 2.5M names."""
    names = [nm.lower() for nm in entity_names]
    cp = np.frombuffer("\x00".join(names).encode("utf-32-le"), dtype=np.uint32).astype(np.int64)
    ent = np.repeat(np.arange(len(names), dtype=np.int64),
                    np.fromiter((len(nm) + 1 for nm in names), dtype=np.int64, count=len(names)))[:len(cp)]
    ok = np.ones(max(len(cp) - 2, 0), dtype=bool)
    for off in range(3):   # a trigram must not straddle the separator between two names
        ok &= cp[off:len(cp) - 2 + off] != 0
    code = (cp[:-2] * 1114112 + cp[1:-1]) * 1114112 + cp[2:] if len(cp) > 2 else cp[:0]
    code, e3 = code[ok], ent[:len(ok)][ok]
    order = np.argsort(code, kind="stable")      # (entities stay ascending inside a trigram)
    return code[order], e3[order], names


def match_names(trigrams, keywords: Sequence[str], limit: int = 20) -> List[int]:
    """``GpuIndexClient.find_entities`` over ``name_trigrams``' index (a keyword under 3 characters: the plain scan)."""
    codes, ents, names = trigrams
    per = max(1, limit // len(keywords))
    found: List[int] = []
    for kw in keywords[:5]:
        needle, hits = kw.lower(), 0
        if len(needle) >= 3:
            cp = np.frombuffer(needle.encode("utf-32-le"), dtype=np.uint32).astype(np.int64)
            tri = np.unique((cp[:-2] * 1114112 + cp[1:-1]) * 1114112 + cp[2:])
            lo, hi = np.searchsorted(codes, tri, "left"), np.searchsorted(codes, tri, "right")
            cand = None
            for j in np.argsort(hi - lo):            # rarest trigram first
                part = np.unique(ents[lo[j]:hi[j]])
                cand = part if cand is None else cand[np.isin(cand, part, assume_unique=True)]
                if len(cand) == 0:
                    break
            pool = cand.tolist() if cand is not None else []
        else:
            pool = range(len(names))                 # too short for a trigram: the plain scan
        for e in pool:
            if needle in names[e]:
                if e not in found:
                    found.append(e)
                hits += 1
                if hits == per:
                    break
    return found[: N.THR_GRAPH_MAX_SEEDS]


class EntitySearch:
    entities: Optional[dict] = None             # name_bytes u8, name_ptr i64 [E + 1] on the device; n
    _ws_entity: Optional[torch.Tensor] = None   # thr_entity_match's workspace, grown on demand and kept

    def set_entity_names(self, names: Sequence[str]) -> "EntitySearch":
        """The device copy of the entity names ``find_entities`` matches against (index set-up, not
        the query path): entity e is names[e].  append_rows / delete_rows never change the entity set
        (their mentions name existing entities only) and leave it alone; append_graph(entity_names=)
        extends it on the device -- the old bytes, the new names, the padding moved to the new end --
        to what this call would build from all the names.  After set_graph the count must be the
        entity CSR's, and a later set_graph must bring as many entities."""
        names = list(names)
        G = getattr(self, "graph", None)
        if G is not None and len(names) != G["ent_rowptr"].shape[0] - 1:
            raise ValueError(f"set_entity_names: {len(names)} names for the {G['ent_rowptr'].shape[0] - 1} "
                             "entities of the graph (set_graph)")
        if not names:
            self.entities = None
            return self
        blob, ptr = pack_entity_names(names)
        self.entities = dict(name_bytes=self._t(blob, torch.uint8), name_ptr=self._t(ptr, torch.int64), n=len(names))
        return self

    def find_entities(self, keyword_lists: Sequence[Sequence[str]], limit: int = 20,
                      long_keywords: Optional[Callable[[Sequence[str], int], List[int]]] = None):
        """The seed entities of every query of a batch -> (seeds int32 [nq, 16] padded with -1, counts
        int32 [nq]), both on the device: per query GpuIndexClient.find_entities' answer -- of
        keywords[:5] each contributes its first max(1, limit // len(keywords)) entities, in ascending
        id, whose lower-cased name contains the lower-cased keyword; duplicates are skipped, the list
        is cut at 16.  ``seeds`` is what graph_search(query_seeds) / retrieve_batch(query_seeds=) take.
        The host lowers, encodes and de-duplicates the keywords and uploads the needle tables (one
        copy each); the matching is thr_entity_match.
        A keyword among a query's first five whose UTF-8 is longer than THR_ENTITY_MAX_NEEDLE bytes
        cannot go through the kernel: ValueError, unless ``long_keywords`` -- a callable (keywords,
        limit) -> entity ids -- is given; it resolves those queries and their rows are patched in."""
        if self.entities is None:
            raise N.NativeError("find_entities: the index has no entity names (set_entity_names)")
        plan = plan_needles(keyword_lists, limit)
        if plan.long_rows and long_keywords is None:
            raise ValueError(f"find_entities: a keyword of query {plan.long_rows[0]} is longer than "
                             f"THR_ENTITY_MAX_NEEDLE = {N.THR_ENTITY_MAX_NEEDLE} bytes of UTF-8 "
                             "(pass long_keywords= to resolve such queries on the host)")
        nq = len(keyword_lists)
        if nq == 0 or plan.needles.shape[0] == 0:       # no query names a needle: nothing to match
            seeds = torch.full((nq, N.THR_GRAPH_MAX_SEEDS), -1, dtype=torch.int32, device=self.device)
            counts = torch.zeros(nq, dtype=torch.int32, device=self.device)
        else:
            Ent = self.entities
            need = N.entity_match_workspace_bytes(Ent["n"], plan.needles.shape[0], nq)
            seeds, counts = N.entity_match(Ent["name_bytes"], Ent["name_ptr"], self._t(plan.needles, torch.uint8),
                                           self._t(plan.needle_len, torch.int32),
                                           self._t(plan.query_needles, torch.int32),
                                           self._t(plan.query_per, torch.int32),
                                           workspace=self._scratch("_ws_entity", need))
        if plan.long_rows:
            rows = np.full((len(plan.long_rows), N.THR_GRAPH_MAX_SEEDS), -1, dtype=np.int32)
            cnt = np.zeros(len(plan.long_rows), dtype=np.int32)
            for i, q in enumerate(plan.long_rows):
                found = list(long_keywords(keyword_lists[q], limit))[:N.THR_GRAPH_MAX_SEEDS]
                rows[i, :len(found)] = found
                cnt[i] = len(found)
            at = self._t(np.asarray(plan.long_rows, dtype=np.int64), torch.int64)
            seeds[at] = self._t(rows, torch.int32)
            counts[at] = self._t(cnt, torch.int32)
        return seeds, counts
