"""Diversified top-k on the device (include/thr_hip_diversify.h): Maximal Marginal Relevance between the fusion
(and the optional collapse / rerank) and the final cut of the funnel.  The reference ends in a truncation
(``kept[:top_k]``, src/voice_agent/rag2/retrieval.py) and its only defence against look-alike chunks is an exact
``content_hash`` check at ingest (rag2/ingest.py:385-427); here the cut may instead pick, greedily, the candidate
of greatest ``lam * rel - (1 - lam) * max sim to what is already picked``.

The similarities come from what the index already holds in HBM -- the float32 rows ``docs`` and their float64
norms ``dnorm`` -- under the dense channel's cosine contract, so nothing is read back between the stages and the
result is bit-equal to a CPU restatement (tests/mmr_cases.py).

Not built: an index sharded by documents (ShardedIndex refuses ``diversify=``: the candidates' rows lie on
several shards), and a hard "drop anything above similarity x" mode."""
from __future__ import annotations

from typing import Optional

import torch

from . import _native as N


def check_lam(what: str, lam) -> float:
    """``lam`` as a float in [0, 1] (1.0: relevance alone, 0.0: diversity alone behind the first pick)."""
    try:
        value = float(lam)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: diversify is None or a float in [0, 1] (MMR's lambda), got {lam!r}") from None
    if isinstance(lam, bool) or not 0.0 <= value <= 1.0:        # (NaN fails both comparisons)
        raise ValueError(f"{what}: diversify is None or a float in [0, 1] (MMR's lambda), got {lam!r}")
    return value


def refuse_diversify_on_shards(what: str, diversify) -> None:
    """ShardedIndex / ShardedIndexClient: MMR is not built there."""
    if diversify is not None:
        raise NotImplementedError(f"{what}: diversify={diversify!r} is not built for a document-sharded index: the "
                                  "dense rows of one query's candidates lie on several shards, and no shard can take "
                                  "the similarity of two candidates it does not both hold")


class DiversifiedSearch:
    def _dense_rows_for(self, what: str):
        if getattr(self, "docs", None) is None or getattr(self, "dnorm", None) is None:
            raise ValueError(f"{what}: this index has no dense rows (MMR takes its similarities from them)")
        return self.docs, self.dnorm

    def diversify(self, ids, scores, counts=None, top_k: int = 10, lam: float = 0.5):
        """MMR over each list ``ids[q][0 .. counts[q])`` (global ids) / ``scores`` (float64, best first) ->
        (ids, scores, counts, pos, mmr), [nq, top_k] in selection order: the selected ids, their ORIGINAL scores,
        how many were selected, each one's position in the input and its MMR value when it was selected
        (thr_hip_diversify.h).  An id without a dense row here (negative, another shard's, a row without an
        embedding) stays selectable and is similar to nothing."""
        docs, dnorm = self._dense_rows_for("diversify")
        lam = check_lam("diversify", lam)
        return N.mmr_select(self._t(ids, torch.int64), self._t(scores, torch.float64),
                            None if counts is None else self._t(counts, torch.int32), docs, dnorm, self.doc_base,
                            int(top_k), lam)
