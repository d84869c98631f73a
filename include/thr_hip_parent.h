/* thr_hip_parent.h -- child -> parent expansion of the retrieval funnel: entry points of libthr_hip.so that
 * came after ABI version 9.
 *
 * An additive companion of thr_hip.h (same library, same conventions, THR_ABI_VERSION unchanged): every
 * pointer is device memory, all work is enqueued on ``stream``, nothing synchronises, allocates or frees,
 * no entry point here takes a workspace; 0 on success, a negative THR_ERR_* for an argument error, a
 * positive hipError_t if a launch failed.
 *
 * THE COLUMN.  parent_of is int32 [n_docs]: parent_of[r] is the parent number of local row r, in
 * [0, n_parents), or -1 for "no parent".  family(r) = {r} when parent_of[r] < 0, else every local row r'
 * with parent_of[r'] == parent_of[r], in ascending row order.  The parent -> children CSR says the same the
 * other way round: par_rowptr int64 [n_parents + 1], par_child int32 [nnz], the children of a parent
 * ascending.
 *
 * THE PARENT SCORE.
 *
 *     score(q, r) = sum_i  max_{r' in family(r)}  max_j  <qtok[q][i][:], dtok[r'][j][:]>
 *
 * which is thr_maxsim of the query against the concatenation of the family's token blocks in row order
 * (the oracle of a score); over the FP8 store (thr_hip_rerank.h) each token's scale is applied before the
 * max, as thr_maxsim_fp8 does.  A family of one row scores as thr_maxsim_ids / thr_maxsim_fp8_ids score
 * that row, to the bit.
 *
 * THE SCORERS (thr_maxsim_parent_ids: the float16 store, PACKED image of thr_maxsim_pack only;
 * thr_maxsim_parent_fp8_ids: the FP8 store) take the arguments of thr_maxsim_ids / thr_maxsim_fp8_ids (no
 * dtok_packed: the row-major store is not built) and the column and its CSR behind n_cand.  One wave per
 * (query, candidate) walks the 32-token tiles of the candidate's family, v_mfma_f32_32x32x16_f16 on the
 * transposed product as the plain scorers; the query tile is the outer loop (a family is read q_tokens /
 * 32 times by its wave).  No barrier, no LDS.  Any n_queries, sent out in slices of at most the device's
 * gridDim.y.  tok_dim: 16, 32, 64, 96, 128, 192, 256 (float16); 32, 64, 96, 128, 192, 256 (FP8); q_tokens
 * and d_tokens positive multiples of 32.
 * Every index is checked.  A candidate that is negative or outside [id_base, id_base + n_docs) scores -inf.
 * A parent number at or above n_parents is read as "no parent".  Row pointers are clamped to [0, nnz].  A
 * child outside [0, n_docs) is skipped and never dereferenced (a family whose children are all skipped
 * scores -inf).  The kernels do not check that the CSR is the column's: that is the caller's (one owner
 * builds it from the column, GpuIndex.parent_csr).
 *
 * THE GROUPS OF A FUSED ROW (thr_parent_groups).  A fused row is ids[q][0 .. cnt), cnt = counts[q] clamped
 * to [0, n], n when counts is NULL.  Position p has key parent_of[ids[q][p] - id_base] when the id is local
 * and that value is >= 0; otherwise its key is its own: negative ids, ids of other shards and rows without
 * a parent never merge with anything.
 *     leader[q][p]   the lowest position with p's key
 *     uniq_ids[q]    the ids of the leaders in position order, then -1
 *     slot[q][p]     the index of p's leader in that list
 *     n_uniq[q]      its length
 * Positions >= cnt get leader = slot = -1.  One workgroup per query; n in 1 .. THR_RRF_MAX_TOP_K; any
 * n_queries (slices of at most the device's gridDim.x).  No atomics: the same bits every run.
 *
 * Refused before any pointer is looked at (THR_ERR_UNSUPPORTED): a tok_dim outside the store's list, a
 * q_tokens / d_tokens that is not a positive multiple of 32, n_docs above 2^31 - 1 (children are int32
 * rows), n outside 1 .. THR_RRF_MAX_TOP_K.  THR_ERR_INVALID: a null pointer (counts may be NULL), a
 * non-positive n_queries / n_docs / n_cand / n_parents / nnz. */
#ifndef THR_HIP_PARENT_H
#define THR_HIP_PARENT_H

#include "thr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int thr_parent_groups(const int64_t *ids /* [n_queries, n] */, const int32_t *counts /* [n_queries] or NULL */,
                      int n_queries, int n, const int32_t *parent_of /* [n_docs] */, int64_t n_docs,
                      int64_t id_base, int32_t *out_leader /* [n_queries, n] */,
                      int32_t *out_slot /* [n_queries, n] */, int64_t *out_uniq_ids /* [n_queries, n] */,
                      int32_t *out_n_uniq /* [n_queries] */, thr_stream_t stream);
int thr_maxsim_parent_ids(const uint16_t *qtok /* f16 [n_queries, q_tokens, tok_dim] */, int n_queries,
                          int q_tokens, const uint16_t *dtok /* the packed image */, int64_t n_docs, int d_tokens,
                          int tok_dim, const int64_t *cand_ids /* [n_queries, n_cand] */, int64_t id_base,
                          int n_cand, const int32_t *parent_of /* [n_docs] */,
                          const int64_t *par_rowptr /* [n_parents + 1] */, const int32_t *par_child /* [nnz] */,
                          int n_parents, int64_t nnz, float *out_scores /* [n_queries, n_cand] */,
                          thr_stream_t stream);
int thr_maxsim_parent_fp8_ids(const uint16_t *qtok, int n_queries, int q_tokens, const uint8_t *codes,
                              const float *scales, int64_t n_docs, int d_tokens, int tok_dim,
                              const int64_t *cand_ids, int64_t id_base, int n_cand, const int32_t *parent_of,
                              const int64_t *par_rowptr, const int32_t *par_child, int n_parents,
                              int64_t nnz, float *out_scores, thr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* THR_HIP_PARENT_H */
