/* thr_hip_fuzzy.h -- typo-tolerant lexical queries: the nearest vocabulary terms of a batch's unknown tokens.
 *
 * An additive companion of thr_hip.h (same library, same conventions, same workspace contract,
 * THR_ABI_VERSION unchanged): every pointer is device memory unless its name begins with h_, all
 * work is enqueued on ``stream``, nothing synchronises, allocates or frees; 0 on success, a negative
 * THR_ERR_* for an argument error, a positive hipError_t if a launch failed.
 */
#ifndef THR_HIP_FUZZY_H
#define THR_HIP_FUZZY_H

#include "thr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a9  "did you mean" behind the exact lookup.  thr_text_tokens[_analyzed] answers a token the vocabulary does
 * not hold with term -1 and its place in the unknown list; under AND semantics that empties the query.  The
 * definition of the correction is index_text.nearest_terms_host / host_query_row_fuzzy, in plain Python:
 *
 *   edits(n)      = min(max_edits, 0 for n < 3, 1 for n < 6, else 2)          n = the needle's code points
 *   candidates    = the keys with | len(key) - n | <= edits(n), a document frequency > 0 (when frequencies
 *                   are given) and levenshtein(needle, key) <= edits(n)  -- insert / delete / substitute at
 *                   unit cost over CODE POINTS; a needle of fewer than 3 or more than THR_FUZZY_MAX_LEN code
 *                   points has none
 *   the answer    = the first n_best candidates under the TOTAL order (distance ascending, min(df, 2^31 - 1)
 *                   descending, term id ascending).
 *
 * thr_vocab_nearest: for the unknown list of a thr_text_tokens / thr_text_tokens_analyzed call over the batch
 * text_bytes (n_bytes of them; no alignment and no padding is asked: no byte outside [0, n_bytes) is read) --
 * unknown_off int64 / unknown_len int32 [unknown_capacity], n_unknown int32 [1], all as that call left them in
 * device memory -- against the key store term_bytes / term_ptr int64 [n_vocab + 1] (n_term_bytes: the bytes of
 * the store, term_ptr[n_vocab]; term_ptr ascending) and, when term_rowptr int64 [n_vocab + 1] is not NULL, the
 * document frequencies df[t] = term_rowptr[t + 1] - term_rowptr[t] (the postings' row pointer):
 *   near_term, near_dist int32 [unknown_capacity, n_best]: row u belongs to unknown u; best first, padded
 *      with -1.  Rows at or behind *n_unknown (clamped to 0 .. unknown_capacity) are NOT written; with
 *      *n_unknown 0 nothing is written.
 * The needle is the bytes [off, off + len) lowered through ``table`` (thr_text_tokens' character table) on the
 * device; with an analyzer the list names the kept prefix, so the needle is the stem.  Nothing is read back and
 * nothing is written in lowered form outside the workspace.
 * What the host cannot check is DEFINED: an offset or length that leaves [0, n_bytes) is clamped into it; a
 * needle that holds malformed UTF-8, an exceptional code point (THR_TEXT_EXC), a code point above U+FFFF, or
 * more than THR_FUZZY_MAX_LEN code points gets a row of -1; a key that is not valid UTF-8 (one- to three-byte
 * forms; the three-byte form of a surrogate counts as its code point, as the project's encoder writes it) or
 * holds a code point above U+FFFF is never a candidate; a key is read only inside [term_ptr[t], term_ptr[t +
 * 1]) and inside [0, n_term_bytes); a key whose term_ptr[t] lies outside the slice that found it is passed
 * over.  Keys are compared as they stand (never lowered), as the exact lookup does.
 *
 * How: three small kernels lower the needles once into a compact table (uint16 code points and a length per
 * needle) ordered by length -- the order is a deterministic counting sort, no atomics.  ONE pass over the key
 * store follows: a workgroup stages a slice of THR_FUZZY_SLICE_BYTES key bytes in LDS (with a halo of the
 * longest key that can still match), a lane owns one key that begins in the slice, decodes it once, and meets
 * only the needles of L - d .. L + d code points, staged in LDS in batches.  Per (key, needle) pair a banded
 * edit distance (band 2 max_edits + 1 <= 5) that ends as soon as a whole row exceeds d.  A match is packed as
 * (distance << 62 | (2^31 - 1 - min(df, 2^31 - 1)) << 31 | term id) and inserted into the needle's n_best
 * 64-bit slots by a chain of atomic minima (old = atomicMin(slot[j], x); x = max(old, x); on to slot j + 1):
 * every step keeps the smaller value and forwards the larger, so slot j ends as the (j + 1)-th smallest key
 * whatever the interleaving -- the exact top n_best, no candidate list, no capacity, no overflow.  The slots
 * are initialised by the call; the same bits every run, whatever the workspace held; no workgroup waits for
 * another.
 *
 * Refused before any launch: n_bytes outside 0 .. THR_TEXT_MAX_BYTES, unknown_capacity outside 1 ..
 * THR_TEXT_MAX_BYTES, n_vocab above INT32_MAX, n_term_bytes above 2^43 (THR_ERR_UNSUPPORTED; the size query
 * returns 0); null pointers (term_rowptr alone may be null), n_vocab < 0, n_term_bytes < 0, max_edits outside
 * 1 .. 2, n_best outside 1 .. THR_FUZZY_MAX_BEST, unknown_off / term_ptr / term_rowptr not 8-byte, table /
 * unknown_len / n_unknown / near_term / near_dist not 4-byte, workspace not 16-byte aligned (THR_ERR_INVALID);
 * ``workspace`` < thr_vocab_nearest_workspace_bytes() (THR_ERR_WORKSPACE).
 *
 * thr_query_terms_fuzzy: thr_query_terms with the corrections folded in.  It takes everything thr_query_terms
 * takes and near_term int32 [near_capacity, n_best] (thr_vocab_nearest's), n_use 1 .. n_best: how many
 * corrections of a token enter a row (1 for an AND query: the BM25 AND has no "t or t'" clause; up to n_best
 * for OR).  The u-th row of tok_term that holds -1, in row order over the whole batch, is unknown u (the order
 * thr_text_tokens emits).  A known token enters the row as before; an unknown token's non-negative
 * near_term[u][0 .. n_use) enter AT THE TOKEN'S PLACE, best first, under the same "first appearance" rule (a
 * correction that is in the row already changes nothing) and set THR_TEXT_CORRECTED; an unknown token with no
 * correction (or with u >= near_capacity) sets THR_TEXT_UNKNOWN.  n_distinct, the clamp at THR_BM25_MAX_TERMS,
 * THR_TEXT_TOO_MANY and the padding exactly as thr_query_terms.  With every near_term entry -1 the outputs
 * equal thr_query_terms' bit for bit.
 * Refused: thr_query_terms' refusals; a null near_term, near_capacity < 1, n_best outside 1 ..
 * THR_FUZZY_MAX_BEST, n_use outside 1 .. n_best (THR_ERR_INVALID); ``workspace`` <
 * thr_query_terms_fuzzy_workspace_bytes() (THR_ERR_WORKSPACE). */
#define THR_FUZZY_MAX_LEN 32
#define THR_FUZZY_MAX_BEST 4
#define THR_FUZZY_SLICE_BYTES 8192
#define THR_TEXT_CORRECTED 8
size_t thr_vocab_nearest_workspace_bytes(int64_t n_bytes, int64_t unknown_capacity, int64_t n_vocab,
                                         int64_t n_term_bytes, int n_best);
int thr_vocab_nearest(const uint8_t *text_bytes, int64_t n_bytes, const uint32_t *table /* [65536] */,
                      const int64_t *unknown_off, const int32_t *unknown_len, const int32_t *n_unknown,
                      int64_t unknown_capacity, const uint8_t *term_bytes, const int64_t *term_ptr,
                      int64_t n_vocab, int64_t n_term_bytes, const int64_t *term_rowptr /* or NULL */,
                      int max_edits, int n_best, int32_t *near_term, int32_t *near_dist, void *workspace,
                      size_t workspace_bytes, thr_stream_t stream);
size_t thr_query_terms_fuzzy_workspace_bytes(int n_queries);
int thr_query_terms_fuzzy(const int32_t *tok_term, const int32_t *n_tokens, const int32_t *text_flags,
                          const int32_t *n_total, int64_t token_capacity, int n_queries,
                          const int32_t *near_term /* [near_capacity, n_best] */, int64_t near_capacity,
                          int n_best, int n_use, int32_t *out_terms /* [nq, THR_BM25_MAX_TERMS] */,
                          int32_t *n_distinct, int32_t *out_flags, void *workspace, size_t workspace_bytes,
                          thr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* THR_HIP_FUZZY_H */
