/* thr_hip_diversify.h -- diversified top-k behind the fusion: Maximal Marginal Relevance (Carbonell &
 * Goldstein) over the candidates' dense rows.  An entry point of libthr_hip.so that came after ABI version 9.
 *
 * An additive companion of thr_hip.h (same library, same conventions, THR_ABI_VERSION unchanged): every
 * pointer is device memory, all work is enqueued on ``stream``, nothing synchronises, allocates or frees,
 * the entry point takes no workspace; 0 on success, a negative THR_ERR_* for an argument error, a positive
 * hipError_t if a launch failed.
 *
 * THE LIST of query q is ids[q][0 .. n), scores[q][0 .. n) (float64, best first), cnt = counts[q] clamped
 * to [0, n], n when counts is NULL.
 *
 * CANDIDATES.  A candidate is a position p < cnt whose score is finite with |score| <= 1e300; any other
 * position is never selected.  m is the number of candidates.
 *
 * ROWS.  has_row(p) holds when id_base <= ids[p] < id_base + n_docs and dnorm[ids[p] - id_base] > 0.  A
 * candidate without a row (a negative id, an id of another shard, a row with no embedding) stays
 * selectable and has similarity 0.0 to everything.
 *
 * RELEVANCE.  lo, hi: the minimum and maximum of the candidates' scores.  rel(p) = 1.0 when hi == lo,
 * else (scores[p] - lo) / (hi - lo): two subtractions and one division, each one IEEE float64 rounding
 * (normalize_scores of the standalone RRFFusion, as thr_fuse_post restates it).
 *
 * SIMILARITY.  sim(a, b) = dot64(row_a, row_b) / (dnorm_a * dnorm_b), dot64 the cosine contract of the
 * dense channel: the sequential left-to-right float64 sum, in dimension order, of the float32 products
 * (exact in float64, so a fused multiply-add gives the same bits).  Rows are finite.
 *
 * SELECTION.  Greedy, min(m, top_k) steps.  Step 0: value(c) = lam * rel(c).  Step t > 0: pen(c) is the
 * maximum of sim(c, s) over the selected s -- a plain maximum (``if sim > pen: pen = sim`` from -inf), not
 * clipped at 0 -- and value(c) = lam * rel(c) - (1.0 - lam) * pen(c): two products and one subtraction,
 * each rounded, no contraction, 1.0 - lam formed once.  Each step selects the unselected candidate of
 * greatest value; ties go to the lowest position.
 *
 * OUTPUTS, [n_queries, top_k] in selection order: out_ids the selected ids; out_scores their ORIGINAL
 * scores (no longer descending); out_pos each one's position in the input; out_mmr (may be NULL) the value
 * at selection; out_counts[q] = min(m, top_k).  Padding behind the count: -1 / -inf / -1 / -inf.
 * With lam = 1.0 and a descending input the output is the first top_k candidates in input order.
 *
 * One workgroup per query, one lane per candidate; similarities are computed lazily, against the newly
 * selected row alone ((top_k - 1) * m dot products); a dot product is never split across lanes.  No
 * atomics: the same bits every run.  Any n_queries (slices of at most the device's gridDim.x).  Every
 * index is checked: a row outside [0, n_docs) is never dereferenced.  docs rows are read 16 bytes at a
 * time: docs is 16-byte aligned.
 *
 * Refused before any pointer is looked at (THR_ERR_UNSUPPORTED): dim outside the multiples of 4 in
 * 4 .. THR_DENSE_ANYDIM_MAX, n outside 1 .. THR_RRF_MAX_TOP_K, top_k outside 1 .. n, n_docs above
 * 2^31 - 1.  THR_ERR_INVALID: a null pointer other than counts / out_mmr, a non-positive n_queries /
 * n_docs, lam outside [0, 1] (NaN included). */
#ifndef THR_HIP_DIVERSIFY_H
#define THR_HIP_DIVERSIFY_H

#include "thr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int thr_mmr_select(const int64_t *ids /* [n_queries, n] */, const double *scores /* [n_queries, n] */,
                   const int32_t *counts /* [n_queries] or NULL */, int n_queries, int n,
                   const float *docs /* [n_docs, dim] */, const double *dnorm /* [n_docs] */, int64_t n_docs,
                   int dim, int64_t id_base, double lam, int top_k, int64_t *out_ids /* [n_queries, top_k] */,
                   double *out_scores /* [n_queries, top_k] */, int32_t *out_pos /* [n_queries, top_k] */,
                   double *out_mmr /* [n_queries, top_k] or NULL */, int32_t *out_counts /* [n_queries] */,
                   thr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* THR_HIP_DIVERSIFY_H */
