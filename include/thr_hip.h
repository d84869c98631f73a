/* thr_hip.h -- C ABI of the MI355X-native retrieval hot path (libthr_hip.so).
 *
 * The reference (matheusfalcaopinto/triple-hybrid-rag) has no FFI layer: its
 * scorers run inside PostgreSQL / PuppyGraph / remote model servers and are
 * reached from Python over HTTP.  Each entry point
 * below replaces one of those out-of-process scorers; the reference call site
 * it stands behind is cited (paths relative to the reference root).
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers + sizes; every pointer is DEVICE memory (hipMalloc'd or a
 *     PyTorch-ROCm tensor's data_ptr) unless the name starts with ``h_``;
 *   - all work is enqueued on ``stream`` (a hipStream_t passed as void*; 0 =
 *     the null stream); nothing synchronises, allocates or frees;
 *   - return 0 on success, a negative THR_ERR_* for argument/capacity errors,
 *     or a positive hipError_t if a launch failed;
 *   - doc / chunk / entity ids are indices into the caller's arrays; outputs
 *     add ``id_base`` so a document-sharded index reports global ids;
 *   - total order of every ranked output: (score descending, id ascending).
 *
 * WORKSPACES.  An entry point that takes ``workspace`` / ``workspace_bytes`` carves the first
 * thr_*_workspace_bytes(...) bytes of it (the size function declared with the entry, called with the
 * same shape) into areas whose offsets follow from the shape of the call.  The workspace's contents on
 * entry are never read: every area is either cleared by the entry point itself or written by one of
 * its kernels before another reads it, on every path (pruned slices, skipped sweeps, padding queries,
 * empty scopes, overflowed lists), so a caller may hand in memory that holds anything -- zeros, 0xFF,
 * what an earlier call of any shape left there -- and gets the same bits.  Nothing outside
 * [workspace, workspace + thr_*_workspace_bytes(...)) is written, however large workspace_bytes is.
 * Two deliberate exceptions, both of the dense channel: thr_dense_finish_f16 reads what
 * thr_dense_shortlist_f16 left in the same workspace (the candidate lists, the thresholds, the query
 * image: the pair is one search), and the scan probes / stamps (thr_dense_scan_probe,
 * thr_dense_scan_probe_f16, thr_dense_scan_stamps_f16) read the previous call's tau and query image.
 * DESIGN.md ("Workspace contract") lists every area with the memset or kernel that writes it.
 * OUTPUTS.  Every output element an entry point documents is written by it.  Where a call reports
 * how much of an output array it used, the elements behind that length are not written and stay as
 * the caller left them: ids_out / pay_out behind *nnz_out, ``rows`` behind min(rowptr[n_preds], cap),
 * tok_doc / tok_term behind *n_total, unknown_off / unknown_len / unknown_term behind *n_unknown,
 * new_ptr behind entry *n_new, new_bytes behind min(*n_new_bytes, new_bytes_capacity).
 */
#ifndef THR_HIP_H
#define THR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define THR_ABI_VERSION 9

typedef void *thr_stream_t;

enum {
    THR_OK = 0,
    THR_ERR_INVALID = -1,     /* null pointer / negative size / k out of range */
    THR_ERR_UNSUPPORTED = -2, /* shape the kernels are not built for */
    THR_ERR_WORKSPACE = -3,   /* workspace smaller than thr_*_workspace_bytes */
    THR_ERR_CAPACITY = -4     /* a fixed on-chip capacity would be exceeded */
};

/* per-query status bits written by thr_dense_topk */
#define THR_FLAG_CERTIFIED 1u /* top-k proven exact by the fp32-error certificate */
#define THR_FLAG_OVERFLOW 2u  /* candidate buffer overflowed (never certified)    */
#define THR_FLAG_EXACT 4u     /* produced by the exhaustive float64 path          */

#define THR_DENSE_MAX_K 256   /* k and k' (shortlist) upper bound; the certificate needs a margin
                               * k' - k of rows (28 for the fp32 scan, 92 for the f16 scans), so
                               * beyond k ~ 200 queries increasingly take the exhaustive path
                               * (still exact, much slower) */
#define THR_BM25_MAX_TERMS 32
#define THR_BM25_MAX_QUERIES (1 << 20) /* queries of one thr_bm25_topk call (the caller splits a larger batch) */
#define THR_GRAPH_MAX_SEEDS 16
#define THR_RRF_MAX_PER_CHANNEL 128
#define THR_RRF_MAX_TOP_K 512  /* rows of one fused list: top_k of thr_rrf_fuse*, n of thr_fuse_post / thr_rerank_order */
#define THR_TOPK_MAX 128      /* bm25 / graph k upper bound */

int thr_abi_version(void);
const char *thr_error_string(int code);
/* CUs, HBM bytes and gcnArchName of the current device (host-side query). */
int thr_device_info(int *h_compute_units, int64_t *h_hbm_bytes, char *h_arch, int h_arch_len);

/* a1  query-embedding post-processing: prefix-truncate to ``store_dim`` and
 * L2-normalise in float32, zero rows stay zero.
 * Replaces truncate_matryoshka/normalize_l2, src/voice_agent/rag2/embedder.py:31-68
 * (the model forward that produces ``full`` is an external server). */
int thr_embed_postproc(const float *full, int n, int full_dim, int store_dim,
                       float *out /* [n, min(full_dim,store_dim)] */, thr_stream_t stream);

/* Index build helper: ||d|| per row as sqrt of the sequential float64 sum of
 * squares, and float32 1/||d|| (0 for a zero row = "embedding IS NULL",
 * database/migrations/20260114_rag2_schema.sql:404). */
int thr_doc_norms(const float *docs, int64_t n_docs, int dim, double *dnorm, float *inv_norm,
                  thr_stream_t stream);

/* a2  dense channel: exact brute-force cosine top-k of ``n_queries`` queries
 * over an HBM-resident float32 corpus [n_docs, dim] (dim % 256 == 0).
 * Replaces SQL rag2_semantic_search (`1 - (embedding_1024 <=> q)` ORDER BY
 * distance LIMIT k), database/migrations/20260114_rag2_schema.sql:377-410,
 * called from src/voice_agent/rag2/retrieval.py:304-312, and the client-side
 * np.dot fallback src/voice_agent/retrieval/hybrid_search.py:285-316.
 *
 * Pass 1 (this entry point: the fp32 matrix cores, 32 queries per workgroup and pass over a
 * row slice; thr_dense_topk_f16 below: f16 matrix cores over a float16 copy or over rows
 * rounded in flight) finds per query a threshold tau from a row sample, streams the corpus and
 * emits the rows scoring >= tau; pass 2 takes from those the band that can still reach the top
 * k' = ``kprime``, rescores it in float64 (sequential accumulation, the oracle's contract)
 * from the float32 rows and orders it.
 * out_flags[q] has THR_FLAG_CERTIFIED when the float32 error bound proves the
 * top-k exact; otherwise call thr_dense_topk_exact for that query.
 * Outputs are padded with (-inf, -1) beyond out_counts[q].
 *
 * Query values.  For every FINITE float32 query, of any magnitude, a scan entry point followed by
 * thr_dense_rescue returns the bits of the float64 oracle (thr_dense_topk_exact), and whatever a scan
 * certifies on its own is already that.  A query outside the range a scan's arithmetic covers gets a
 * threshold no row passes, stays uncertified and is answered by the exhaustive path alone, without
 * costing the other queries of its tile a candidate slot: a query with no non-zero value, every scan;
 * the f16 scans (thr_dense_topk_f16 and the shards' calls), a query whose float16 image is all zero
 * (every |v| <= 2^-25) or holds an infinity (some |v| >= 65520) -- between the two the measured
 * rounding error of the image, which reaches 1 in float16's subnormals, widens the certificate until
 * it fails; this scan, a query with every |v| < 2^-96 or some |v| >= 2^96 (products with the rows
 * would leave float32's range).  Its lower bounds in the shards' exchange are all -inf: no floor.
 * A query that holds a NaN or an infinity has no defined answer: the call returns, the query is never
 * certified by a scan, its out_counts is at most k, its ids are real rows or -1, and the other queries
 * of the batch are unaffected. */
size_t thr_dense_workspace_bytes(int64_t n_docs, int dim, int n_queries, int kprime);
/* Collection filter of the RPC (``AND (p_collection IS NULL OR d.collection = p_collection)``,
 * rag2_schema.sql:404-408), applied BEFORE the ranking on the device: doc_coll int32 [n_docs]
 * (any labelling) and query_coll int32 [nq] (-1 = unfiltered) -- both or neither (NULL).  The
 * threshold sample, the shortlist and the exhaustive path all see only rows of the query's
 * collection; a collection too thin for the sampled threshold ends on the exhaustive path. */
int thr_dense_topk(const float *docs, const double *dnorm, const float *inv_norm, int64_t n_docs,
                   int dim, int64_t id_base, const float *queries, int n_queries, int k,
                   int kprime, const int32_t *doc_coll, const int32_t *query_coll,
                   double *out_scores /* [nq,k] */, int64_t *out_ids /* [nq,k] */,
                   int32_t *out_counts /* [nq] */, uint32_t *out_flags /* [nq] */,
                   void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* Exhaustive float64 path (every row scored with the oracle's arithmetic);
 * used for queries thr_dense_topk could not certify (massive ties). */
size_t thr_dense_exact_workspace_bytes(int64_t n_docs, int n_queries);
int thr_dense_topk_exact(const float *docs, const double *dnorm, int64_t n_docs, int dim,
                         int64_t id_base, const float *queries, int n_queries, int k,
                         const int32_t *doc_coll, const int32_t *query_coll,
                         double *out_scores, int64_t *out_ids, int32_t *out_counts,
                         uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                         thr_stream_t stream);

/* Device-side completion of thr_dense_topk / thr_dense_topk_f16: every query whose flags lack
 * THR_FLAG_CERTIFIED is redone on the exhaustive float64 path and overwritten in place (flags
 * become CERTIFIED | EXACT); *n_rescued (a DEVICE int32, may be NULL; it need not be initialised)
 * is set to the number of redone queries.  No host read-back: a batch runs end to end without a synchronisation. */
size_t thr_dense_rescue_workspace_bytes(int n_queries, int k);
int thr_dense_rescue(const float *docs, const double *dnorm, int64_t n_docs, int dim,
                     int64_t id_base, const float *queries, int n_queries, int k,
                     const int32_t *doc_coll, const int32_t *query_coll,
                     double *io_scores, int64_t *io_ids, int32_t *io_counts, uint32_t *io_flags,
                     int32_t *n_rescued, void *workspace, size_t workspace_bytes,
                     thr_stream_t stream);

/* Shortlist scan on the f16 matrix cores (< 2^25 rows per shard).  The float32 corpus stays the
 * source of truth: scores are the same float64 rescoring of float32 rows, and the certificate's
 * error bound additionally covers row quantisation (doc_rel_err, measured by
 * thr_dense_quantize_f16 into *max_rel_err, a DEVICE float) and query quantisation (measured per
 * query on the device).  Two flavours:
 *   docs16 != NULL: the scan streams a float16 COPY written by thr_dense_quantize_f16: an opaque
 *                   FRAGMENT-MAJOR image of thr_dense_f16_copy_bytes(n_docs, dim) bytes,
 *                   [row tile of 32][dims 32 k .. +32][rows 16 a .. +16][lane = r + 16 g][8 halves]
 *                   = the register image of the v_mfma_f32_16x16x32_f16 row operand
 *                   (THR_DENSE_MFMA=32 in the environment of BOTH the quantiser and the scan:
 *                   [row tile of 32][k-step of 16 dims][lane = r + 32 h]
 *                   [8 halves], v_mfma_f32_32x32x16_f16), holding the NORMALISED rows
 *                   d/||d|| (NaN for rows without an embedding and for the padding of the last
 *                   tile; doc_rel_err = max_d ||fp16(d/||d||) - d/||d|| ||, any value range).
 *                   Row tiles reach LDS by LDS-DMA, once per CU; each wave keeps 32 queries in
 *                   registers as the other operand (256 queries per CU, 128 at dim 1024);
 *   docs16 == NULL: the scan streams the float32 rows and rounds them to float16 in registers
 *                   (no second copy; thr_dense_quantize_f16 with docs16 == NULL only measures
 *                   doc_rel_err = max_d ||fp16(d) - d|| / ||d||, +inf when a value leaves the
 *                   float16 range, which thr_dense_topk_f16 rejects; 64 queries per pass, 32 at
 *                   dim 1024).
 * dim in {512, 768, 1024}: the tuned kernels.  With docs16 == NULL every other row length that is
 * a multiple of THR_DENSE_ANYDIM_STEP up to THR_DENSE_ANYDIM_MAX is taken too, by a third flavour:
 *   the runtime-dim scan: the same interface as the docs16 == NULL scan (float32 rows rounded in
 *                   registers, no copy, doc_rel_err as measured by thr_dense_quantize_f16 with
 *                   docs16 == NULL, which takes these lengths), one v_mfma_f32_16x16x32_f16 per 32
 *                   dims in a run-time loop; the query tile stays in LDS as float16, so its size
 *                   follows the row length: 64 queries per pass up to dim 768, 32 up to 1536, 16
 *                   beyond (thr_dense_f16_query_tile reports it).  The legacy 4000-d store
 *                   (20260113_halfvec_4000.sql:70-105) and RAG2_EMBED_DIM_STORE settings other than
 *                   the default (config.py:292) are what it is for.
 * With docs16 != NULL such a length returns THR_ERR_UNSUPPORTED (sizes: 0). */
#define THR_DENSE_ANYDIM_STEP 32
#define THR_DENSE_ANYDIM_MAX 4096
/* Which kernel serves docs16 == NULL calls of the CALLING THREAD at dim 512 / 768 / 1024, where both
 * exist: THR_DENSE_F16_BY_DIM (the default: the tuned one) or THR_DENSE_F16_ANYDIM (the runtime-dim
 * scan, for comparing the two at one shape).  Returns the previous selection; any other value only
 * queries.  Sizes and results are the same either way: the two scans have the same query tile at
 * these three lengths (64, 64, 32), so the plan, the workspace and the candidate lists that
 * thr_dense_shortlist_f16 leaves for thr_dense_finish_f16 do not depend on the selection -- a pair of
 * calls made under different selections is still a pair.  (The library checks that equality and
 * ignores the selection should it ever not hold.)  A C caller that never calls this never sees it. */
#define THR_DENSE_F16_BY_DIM 0
#define THR_DENSE_F16_ANYDIM 1
int thr_dense_f16_select(int flavour);
size_t thr_dense_f16_copy_bytes(int64_t n_docs, int dim);
/* queries per workgroup (= per pass over a row slice) of the f16 scan */
int thr_dense_f16_query_tile(int dim, int packed /* docs16 != NULL */, int n_queries);
/* largest n_queries of ONE thr_dense_topk_f16 call: the copy scan addresses a lane's candidate
 * segment with a 32-bit byte offset (131072 bytes of candidate area per query), so a larger
 * batch returns THR_ERR_UNSUPPORTED and the caller splits it (GpuIndex.dense_search does). */
int thr_dense_f16_max_queries(int dim, int packed /* docs16 != NULL */);
int thr_dense_quantize_f16(const float *docs, int64_t n_docs, int dim,
                           uint16_t *docs16 /* thr_dense_f16_copy_bytes(...) bytes, or NULL */,
                           float *max_rel_err, thr_stream_t stream);
size_t thr_dense_f16_workspace_bytes(int64_t n_docs, int dim, int n_queries, int kprime);
int thr_dense_topk_f16(const float *docs, const uint16_t *docs16 /* or NULL */, double doc_rel_err,
                       const double *dnorm, const float *inv_norm, int64_t n_docs, int dim,
                       int64_t id_base, const float *queries, int n_queries, int k, int kprime,
                       const int32_t *doc_coll, const int32_t *query_coll,
                       double *out_scores, int64_t *out_ids, int32_t *out_counts,
                       uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                       thr_stream_t stream);
/* e1  The same search split around ONE exchange between document shards (ABI 9): what a shard of G
 * does NOT have to rescore.  The reference has a single table and a single `ORDER BY ... LIMIT k`
 * (rag2_schema.sql:404-410); sharded, every shard would rescore its own k best although only
 * about k / G of them are among the k best of all.
 *   thr_dense_shortlist_f16  thr_dense_topk_f16 up to and including the filter scan (the candidate
 *                            lists stay in ``workspace``), then per query the ``m`` largest scan
 *                            scores, each lowered by the scan's error bound to a LOWER bound of
 *                            ||q|| x cosine of its row: top_lb float32 [n_queries, m], -inf padded;
 *   (exchange)               all-gather top_lb over the shards -> [G, n_queries, m];
 *   thr_dense_floor          gfloor[q] = the k-th largest of a query's G * m values (-inf when
 *                            fewer than k are finite): a lower bound of ||q|| x the k-th best
 *                            cosine of the whole corpus;
 *   thr_dense_finish_f16     the rest of thr_dense_topk_f16 on the SAME workspace and arguments:
 *                            rows whose scan score is below gfloor[q] - 1.5 eps ||q|| are left out
 *                            of the float64 rescoring.  A shard's list may then hold FEWER than k
 *                            rows (out_counts); THR_FLAG_CERTIFIED now says "no row outside this
 *                            list can be among the k best of all shards" (proved against the
 *                            shard's own k-th score or against gfloor), and thr_dense_rescue
 *                            redoes the others exhaustively as before.  thr_merge_topk over the
 *                            shards' lists is then the exact top-k: no second exchange.
 * The floor reaches thr_dense_finish_f16 either as gfloor (thr_dense_floor's output) or as the
 * gathered bounds themselves (top_lb_all, n_shards, m; G * m <= 4096): the kernel that cuts the
 * band then finds the k-th largest itself and thr_dense_floor is not launched at all.  Neither
 * (or -inf entries) gives thr_dense_topk_f16's behaviour.  m <= THR_DENSE_MAX_K, G * m <= 8192
 * for thr_dense_floor; choose m >= k / G, about 2 k / G for a floor close to the true k-th score. */
int thr_dense_shortlist_f16(const float *docs, const uint16_t *docs16 /* or NULL */, double doc_rel_err,
                            const float *inv_norm, int64_t n_docs, int dim, const float *queries,
                            int n_queries, int kprime, const int32_t *doc_coll,
                            const int32_t *query_coll, int m, float *top_lb /* [nq, m] */,
                            void *workspace, size_t workspace_bytes, thr_stream_t stream);
int thr_dense_floor(const float *top_lb /* [n_shards, nq, m] */, int n_shards, int n_queries, int m,
                    int k, float *gfloor /* [nq] */, thr_stream_t stream);
int thr_dense_finish_f16(const float *docs, const uint16_t *docs16 /* or NULL */, double doc_rel_err,
                         const double *dnorm, const float *inv_norm, int64_t n_docs, int dim,
                         int64_t id_base, const float *queries, int n_queries, int k, int kprime,
                         const int32_t *doc_coll, const int32_t *query_coll,
                         const float *gfloor /* [nq] or NULL */,
                         const float *top_lb_all /* [n_shards, nq, m] or NULL */, int n_shards, int m,
                         double *out_scores, int64_t *out_ids, int32_t *out_counts,
                         uint32_t *out_flags, void *workspace, size_t workspace_bytes,
                         thr_stream_t stream);
int thr_dense_scan_probe_f16(const float *docs, const uint16_t *docs16 /* or NULL */,
                             const float *inv_norm, int64_t n_docs, int dim, const float *queries,
                             int n_queries, void *workspace, size_t workspace_bytes,
                             thr_stream_t stream);

/* Diagnostic build of the float16-copy scan (same launch as thr_dense_scan_probe_f16, on the
 * workspace of the last thr_dense_topk_f16): every wave sums s_memtime deltas around the phases
 * of its tile loop into stamps[wave * 8 + {0 wait for own DMA pieces, 1 barrier, 2 DMA issue,
 * 3 k-loop, 4 emit, 5 tiles, 6 whole loop, 7 HW_ID}] (device, uint64).  stamps == NULL: only
 * *h_n_waves (host) is set, to size the buffer.  Not a timing: the stamps drain the wave's
 * queues; it says where the time goes (profiles/README.md).
 * That is the 4-wave-block kernel (dim 1024, or THR_DENSE_F16=q).  At dim <= 768 the staggered
 * 8-wave kernel is stamped instead and a wave takes SIXTEEN words: *h_n_waves is then twice the
 * number of waves (the buffer is still *h_n_waves * 8 words) and wave w of the launch owns
 * stamps[w * 16 + {0 counted vmcnt wait (group B), 1 barrier arrival to release, 2 fill: release
 * (group B: the end of its emit) to the first A fragment in a register, 3..6 the k-loop in quarters
 * of its steps, 7 emit, 8 intervals (= row tiles), 9 whole loop, 10 HW_ID, 11..15 zero}]; waves
 * 0-3 of a block are group A, 4-7 group B; a wave of padding queries stamps nothing.  These stamps
 * are consumed once per interval and drain nothing inside it (dense_scan_f16q.hpp, QsClock). */
int thr_dense_scan_stamps_f16(const uint16_t *docs16, int64_t n_docs, int dim, int n_queries,
                              void *workspace, size_t workspace_bytes,
                              unsigned long long *stamps, int *h_n_waves, thr_stream_t stream);

/* Timing/roofline probe: ONLY the streaming pass-1 kernel of thr_dense_topk
 * (threshold filter against ``tau``), for ``n_tiles`` query tiles. */
int thr_dense_scan_probe(const float *docs, const float *inv_norm, int64_t n_docs, int dim,
                         const float *queries, int n_queries, void *workspace,
                         size_t workspace_bytes, thr_stream_t stream);

/* f1  index build (the step before the path): the inverted index from tokenised rows, on the
 * device.  The reference leaves this to PostgreSQL -- rag_child_chunks rows go in
 * (src/voice_agent/rag2/ingest.py:361-470) and the `tsv` generated column + GIN index
 * (database/migrations/20260114_rag2_schema.sql:146-148, 171-172) become the posting lists.
 * ``doc`` / ``term`` / ``tf`` [n_pairs]: one entry per distinct (doc, term) of a chunk, or one per
 * token occurrence with tf == NULL (every entry counts 1) -- entries that repeat add up; entries
 * with doc outside [0, n_docs), term outside [0, n_vocab) or tf <= 0 are dropped.  Outputs:
 * rowptr [V + 1], post_doc / post_tf [n_pairs] of which the first *nnz_out are written (doc
 * ascending within a term), doclen [n_docs] = the docs' summed term frequencies (entries whose term
 * is outside the vocabulary still count: they are tokens of the chunk), df [V] = postings
 * per term of THIS shard (all-reduce it over the shards for the global idf), *nnz_out (device
 * memory).  No host round trip inside; ``workspace`` >= thr_lexical_build_workspace_bytes(). */
size_t thr_lexical_build_workspace_bytes(int64_t n_pairs, int64_t n_vocab);
int thr_lexical_build(const int32_t *doc, const int32_t *term, const int32_t *tf /* or NULL */,
                      int64_t n_pairs, int64_t n_docs, int64_t n_vocab, int64_t *rowptr,
                      int32_t *post_doc, int32_t *post_tf, float *doclen, int64_t *df,
                      int64_t *nnz_out, void *workspace, size_t workspace_bytes,
                      thr_stream_t stream);

/* f2  incremental ingest: append the CSR of a batch of new chunks to a live index.  The reference
 * inserts rag_child_chunks rows one document at a time (src/voice_agent/rag2/ingest.py:361-470)
 * and PostgreSQL maintains the `tsv` column + GIN index behind the insert
 * (database/migrations/20260114_rag2_schema.sql:146-148, 171-172).  Appended chunks get the
 * largest doc ids and lists are doc-ascending within a row, so the merged list of row t is A's
 * followed by B's: a segmented concatenation of two CSRs over one row space, no sort over A.
 *   A: rowptr_a [rows_a + 1] (rowptr_a[rows_a] == nnz_a), payloads a0 / a1 [nnz_a];
 *   B: rowptr_b [rows_b + 1] (rowptr_b[rows_b] == nnz_b), payloads b0 / b1 [nnz_b];
 *      rows_b >= rows_a -- the vocabulary may have grown, rows >= rows_a are empty in A;
 *   out: rowptr_out [rows_b + 1] = rowptr_a[min(t, rows_a)] + rowptr_b[t], out0 / out1 with room
 *      for out_capacity >= nnz_a + nnz_b elements, buffers of their own (out of place).
 * Payloads are opaque 4-byte elements (post_doc / post_tf int32; men_chunk int32 / men_conf
 * float32); the second one is optional (a1 == b1 == out1 == NULL).  rows_a == 0 (rowptr_a may be
 * NULL) appends to an empty index.  Stream-ordered, no host round trip, no workspace.  The kernel
 * checks every source index against nnz_a / nnz_b and every destination against nnz_a + nnz_b. */
int thr_csr_append(const int64_t *rowptr_a, int64_t rows_a, int64_t nnz_a, const void *a0,
                   const void *a1 /* or NULL */, const int64_t *rowptr_b, int64_t rows_b,
                   int64_t nnz_b, const void *b0, const void *b1 /* or NULL */,
                   int64_t *rowptr_out, void *out0, void *out1 /* or NULL */,
                   int64_t out_capacity, thr_stream_t stream);

/* f2  delete: order-preserving removal of entries from a CSR, with renumbering.  The reference's
 * store deletes rows: every RAG 2.0 table hangs on its parent with ON DELETE CASCADE
 * (database/migrations/20260114_rag2_schema.sql:65-66, 106-108, 187, 217-218), its end-to-end tests
 * clear a tenant with table("rag_child_chunks").delete().eq(...) (tests/test_rag2_e2e.py:276-293)
 * and the RAG 1.0 ingestor has delete_by_source (src/voice_agent/ingestion/kb_ingest.py:492-510).
 *   ``ids`` [nnz] is the payload that decides liveness (post_doc; men_chunk with id_base = the
 *   shard's doc_base), ``pay`` [nnz] an opaque 4-byte companion (post_tf int32, men_conf float32)
 *   or NULL (then pay_out is NULL too); ``remap`` [n_ids]: new id of old id i, -1 = deleted,
 *   ascending over the survivors.  Entry p is kept iff 0 <= ids[p] - id_base < n_ids and
 *   remap[ids[p] - id_base] >= 0, and is written as remap[...] + id_base.  Kept entries keep their
 *   relative order; rowptr_out [rows + 1]: rowptr_out[t] = kept entries before position rowptr[t]
 *   (rows do not change: a row that empties keeps its id).  *nnz_out (device memory) = the number
 *   of kept entries; of ids_out / pay_out (buffers of their own, room for out_capacity elements)
 *   the first min(*nnz_out, out_capacity) are written, nothing behind them.
 * Stream-ordered, three launches, no workgroup waits for another, no host round trip inside;
 * ``workspace`` >= thr_csr_compact_workspace_bytes().  The kernels check every source index
 * against nnz, every remap index against n_ids and every destination against out_capacity. */
size_t thr_csr_compact_workspace_bytes(int64_t rows, int64_t nnz);
int thr_csr_compact(const int64_t *rowptr, int64_t rows, int64_t nnz, const int32_t *ids,
                    const void *pay /* or NULL */, const int32_t *remap, int64_t n_ids,
                    int64_t id_base, int64_t *rowptr_out, int32_t *ids_out,
                    void *pay_out /* or NULL */, int64_t out_capacity, int64_t *nnz_out,
                    void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* f2  graph ingest: row-wise stable merge of two CSRs over one row space.  The reference's entity
 * extraction runs behind the chunk inserts of a document and upserts rag_entities, inserts
 * rag_relations and inserts rag_entity_mentions for chunks that are already stored
 * (src/voice_agent/rag2/entity_extraction.py:449-554): a new relation may join two old entities and
 * land anywhere inside a sorted row or be there already, a new mention of an old chunk lands in the
 * middle of its entity's chunk-ascending row -- a merge, not thr_csr_append's concatenation.
 *   A: rowptr_a [rows_a + 1], ids_a int32 [nnz_a], pay_a [nnz_a] an opaque 4-byte companion or NULL;
 *   B: the same with rows_b >= rows_a (the entity set may have grown: rows >= rows_a are empty in A);
 *      within a row ids are non-decreasing in both (drop_present: strictly ascending);
 *   out: rowptr_out [rows_b + 1], ids_out / pay_out with room for out_capacity elements, *nnz_out,
 *      *status_out (all device memory, buffers of their own).  Row t of the result is the merge of
 *      A's and B's row t by id; on equal ids A's entries come first and each side keeps its order
 *      (what a stable sort gives a fresh build that lists the old rows before the new ones).
 *   drop_present = 1 (relations: set union): a B entry whose id is already in A's row is dropped,
 *      *nnz_out <= nnz_a + nnz_b and rowptr_out counts kept entries only;
 *   drop_present = 0 (mentions: multiset merge): nothing is dropped, *nnz_out = nnz_a + nnz_b.
 * *status_out is 0 or a sum of THR_CSR_MERGE_UNSORTED_A / _B (the input breaks the ordering its mode
 * needs: the result is then undefined, though inside its buffers, and must not be used) and
 * THR_CSR_MERGE_OVERFLOW (*nnz_out > out_capacity: only positions below out_capacity were written).
 * Of ids_out / pay_out the first min(*nnz_out, out_capacity) elements are written, nothing behind.
 * Work is cut in slices of THR_CSR_MERGE_SLICE positions, not by row; three launches (count, scan,
 * scatter), no workgroup waits for another, stream-ordered, no host round trip inside; ``workspace``
 * (8-byte aligned) >= thr_csr_merge_workspace_bytes().  The kernels check every source index
 * against nnz_a / nnz_b and every destination against out_capacity.  THR_ERR_INVALID before any
 * launch: a null pointer with a non-zero size, rows_b < rows_a, a negative size, drop_present other
 * than 0 / 1, a payload on one side only, a destination that is one of the sources.  rows_a == 0
 * (rowptr_a may be NULL) merges into an empty graph. */
#define THR_CSR_MERGE_SLICE 1024
#define THR_CSR_MERGE_UNSORTED_A 1
#define THR_CSR_MERGE_UNSORTED_B 2
#define THR_CSR_MERGE_OVERFLOW 4
int thr_csr_merge_slice(void);    /* THR_CSR_MERGE_SLICE as the library was built */
size_t thr_csr_merge_workspace_bytes(int64_t rows_b, int64_t nnz_a, int64_t nnz_b);
int thr_csr_merge(const int64_t *rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t *ids_a,
                  const void *pay_a /* or NULL */, const int64_t *rowptr_b, int64_t rows_b,
                  int64_t nnz_b, const int32_t *ids_b, const void *pay_b /* or NULL */,
                  int drop_present, int64_t *rowptr_out, int32_t *ids_out,
                  void *pay_out /* or NULL */, int64_t out_capacity, int64_t *nnz_out,
                  int32_t *status_out, void *workspace, size_t workspace_bytes,
                  thr_stream_t stream);

/* f4  scoped queries: which rows a query may see.  Every reference RPC carries p_org_id
 * (database/migrations/20260114_rag2_schema.sql:341-410), the RAG 2.0 ones p_collection, the RAG 1.0
 * ones p_category / p_source_document (src/voice_agent/retrieval/hybrid_search.py:227-231), all applied
 * in SQL BEFORE the LIMIT.  A scope is a conjunction over per-row int32 attribute columns -- of
 * equalities here, of sets, ranges and negations too in thr_scope_resolve_clauses below -- and a
 * batch names n_preds distinct ones.  The dense, lexical and graph scorers all filter by
 * the labels written here (doc_coll / query_coll; the graph channel: thr_graph_topk_scoped, a4).
 *   h_cols [n_cols]: a HOST array of device pointers, each column int32 [n_docs];
 *   preds int32 [n_preds, n_cols]: the value a row must hold per column, -1 = any value, a value
 *      below -1 matches no row (a name the store has never seen);
 *   rowptr int64 [n_preds + 1], rows int32 [cap]: per predicate its matching rows, ASCENDING.
 *      rowptr is always complete (rowptr[n_preds] = all matches); of ``rows`` only the first
 *      min(rowptr[n_preds], cap) entries are written, nothing behind them -- the caller compares
 *      rowptr[n_preds] with cap before it uses the lists.  rows == NULL with cap == 0: counts only;
 *   labels int32 [n_docs] + overlap int32 [1] (both or neither): the LOWEST predicate a row
 *      matches, -2 for none; *overlap != 0 when some row matched two.  With disjoint predicates
 *      ``labels`` is the doc_coll of thr_dense_topk* / thr_bm25_topk and a query's predicate index
 *      its query_coll: the unchanged kernels then rank inside the scope.
 * Rows without an embedding stay in the lists (the scorers skip them).  Three launches -- count per
 * slice of consecutive rows, one scan, scatter -- no workgroup waits for another, no atomic, no
 * host read-back, the same output every run; every destination index is checked against cap.
 * ``workspace`` >= thr_scope_resolve_workspace_bytes(). */
#define THR_SCOPE_MAX_COLS 8
#define THR_SCOPE_MAX_PREDS 4096
#define THR_SCOPE_MAX_QUERIES (1 << 20)
size_t thr_scope_resolve_workspace_bytes(int64_t n_docs, int n_preds);
int thr_scope_resolve(const int32_t *const *h_cols, int n_cols, int64_t n_docs, const int32_t *preds,
                      int n_preds, int64_t *rowptr, int32_t *rows, int64_t cap, int32_t *labels,
                      int32_t *overlap, void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* The general scope: per column a CLAUSE instead of a value -- set membership ("inside these
 * documents"), ranges ("ingested since day d") and their negations, AND-ed over the columns as the
 * equalities above are.  thr_scope_resolve's outputs, contract and kernel shape (three launches,
 * no atomic, the same output every run, every destination checked against cap):
 *   clauses int32 [n_preds, n_cols, 4], DEVICE memory: (kind, a, b, 0) per predicate and column --
 *      kind 0  any value;                       kind 1  no row;
 *      kind 2  a <= value <= b (an equality is a == b);
 *      kind 3  value is one of set_values[a .. a + b): ascending, distinct, >= 0;
 *      kind 6 / 7  kind 2 / 3 negated.
 *      A row whose value is -1 (it has none) matches no clause of kind 2 .. 7, negated or not: SQL's
 *      rule for NULL under =, IN, BETWEEN, <> and NOT IN; only kind 0 accepts it.
 *   set_values int32 [n_set_values], DEVICE memory: the members of every set of the call, one after
 *      another; NULL iff n_set_values == 0; at most THR_SCOPE_MAX_SET_VALUES.
 * The host cannot read the table, so the kernels are safe for any: an unknown kind matches no row,
 * and a set's window [a, a + b) is clamped into [0, n_set_values] before anything is read (callers
 * validate the table while it is still on the host).  A set costs each row a binary search over its
 * window.  ``workspace`` >= thr_scope_resolve_clauses_workspace_bytes(). */
#define THR_SCOPE_MAX_SET_VALUES (1 << 22)   /* set members of one call, all clauses together */
size_t thr_scope_resolve_clauses_workspace_bytes(int64_t n_docs, int n_preds);
int thr_scope_resolve_clauses(const int32_t *const *h_cols, int n_cols, int64_t n_docs,
                              const int32_t *clauses /* device [P, C, 4] */, int n_preds,
                              const int32_t *set_values /* device; NULL iff n_set_values == 0 */,
                              int64_t n_set_values,
                              int64_t *rowptr, int32_t *rows, int64_t cap,
                              int32_t *labels, int32_t *overlap,
                              void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* Exact cosine top-k of every query over the ROW LIST of its scope (rowptr / rows of
 * thr_scope_resolve, or any lists of local row indices; query_scope int32 [nq] in [0, n_scopes), any
 * other value = no rows, n_scopes <= THR_SCOPE_MAX_PREDS): thr_dense_topk_exact's contract and bits --
 * sequential float64 accumulation of the float32 products in dimension order, ||q|| the same way,
 * dot / (qn * dn), rows with dnorm 0 absent, a zero query scores 0.0, (score desc, id asc), flags
 * THR_FLAG_CERTIFIED | THR_FLAG_EXACT, padding (-inf, -1) -- at the cost of the scope's rows, not of
 * n_docs.  Any dim that is a multiple of 4.  The queries of a scope share its rows: a work item is
 * (8 queries of one scope, a slice of its row list); the queries are grouped by scope by a small
 * kernel of this call (the caller passes them in any order).  Row indices outside [0, n_docs) and
 * list positions at or behind rows_cap (the capacity ``rows`` was resolved with) are never read. */
size_t thr_dense_topk_rows_workspace_bytes(int n_queries, int n_scopes, int k);
int thr_dense_topk_rows(const float *docs, const double *dnorm, int64_t n_docs, int dim, int64_t id_base,
                        const float *queries, int n_queries, int k, const int64_t *rowptr,
                        const int32_t *rows, int64_t rows_cap, int n_scopes, const int32_t *query_scope,
                        double *out_scores, int64_t *out_ids, int32_t *out_counts, uint32_t *out_flags,
                        void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* a3  lexical channel: Okapi BM25 (k1, b) top-k over a CSR inverted index,
 * OR semantics, float64 accumulation in query-term order.
 * Stands where SQL rag2_lexical_search (ts_rank_cd ... ORDER BY rank DESC
 * LIMIT k) is called, rag2_schema.sql:341-374 / retrieval.py:282-290; the
 * north-star mandates BM25 in its place.  ``query_terms`` is [nq, max_terms]
 * term ids, negative = padding.  idf[] and avgdl are corpus-GLOBAL.
 *
 * INPUT CONTRACT of thr_bm25_bounds / thr_bm25_dense_rows / thr_bm25_topk.  idf, avgdl, doclen, k1
 * and b are the caller's: a shard passes global statistics that do not follow from its own rows.
 * The pruning is exact -- the same bits as scoring every posting -- for
 *     avgdl > 0,   k1 >= 0,   0 <= b <= 1,   tf >= 1,   doclen >= 0,
 *     every idf finite and either 0 or >= 1e-300.
 * Then every impact lies in (0, k1 + 1] and every contribution idf * impact in [0, idf * (k1 + 1)]:
 *  - idf >= 0: a quantised impact is rounded UP, and idf times it bounds the contribution from above
 *    only for a non-negative idf.  The classic Robertson idf ln((N - df + 0.5) / (df + 0.5)) is
 *    negative above df = N / 2: use the oracle's ln(1 + ...) form (bm25_idf), or clamp at 0.
 *  - the quantiser: post_imp = ceil(impact * 255 / (k1 + 1)) + 1, clipped to 255.  A clipped impact
 *    stands for 255 * fl((k1 + 1) / 255), which may be an ulp below k1 + 1; the thresholds the
 *    kernels compare against are integers (floor(theta * scale * (1 - 1e-12)) in accumulator
 *    units), so a bound that is short by a few ulps never prunes a doc that ties or beats theta.
 *  - the accumulator weights of a query: w_t = ceil(idf_t * unit * 248 / sum), unit = (k1 + 1) /
 *    255, sum = the sum of idf_t * unit over the query's (probed) terms, clamped to >= 1; they add
 *    up to <= 256, so eight clipped impacts (255 * 256) fit a 16-bit slot.  A query whose idfs are
 *    all 0.0 scores 0.0 everywhere and is never pruned.  248 / sum must be finite: the smallest
 *    sum is one idf * unit, unit >= 1 / 255 for k1 >= 0, so idf >= 248 * 255 / DBL_MAX = 3.52e-304
 *    suffices; the contract rounds that up to 1e-300 (bm25_idf yields >= 2.3e-10 for 2^31 docs).
 *    Below it the weight would be (int)ceil(inf) and a 16-bit slot could spill into its neighbour.
 * Nothing in these entry points reads idf back to check it (that would be a device round trip
 * per call): the host layer does once, at index set-up (_native.bm25_check_params, called by
 * GpuIndex.set_lexical), and refuses values outside the contract by name. */
/* Index set-up: upper bounds for the WAND-style pruning of thr_bm25_topk, computed with the
 * scoring formula itself: term_ub[t] = max contribution of a posting of term t, block_ub[j] = max
 * contribution among postings [128 j, 128 j + 128) of the posting array
 * (thr_bm25_block_count(nnz) doubles).  They depend on idf / avgdl / k1 / b. */
size_t thr_bm25_block_count(int64_t nnz);
int thr_bm25_bounds(const int64_t *rowptr, const int32_t *post_doc, const int32_t *post_tf,
                    const float *doclen, const double *idf, double avgdl, double k1, double b,
                    int64_t n_vocab, int64_t nnz, double *term_ub /* [V] */,
                    double *block_ub /* [thr_bm25_block_count(nnz)] */,
                    uint8_t *post_imp /* [nnz] or NULL */, thr_stream_t stream);
/* post_imp (ABI 6): per posting, its IMPACT tf (k1+1) / (tf + k1 ((1-b) + b dl/avgdl)) -- the
 * contribution is idf * impact, the impact does not depend on the query -- rounded UP to 8 bits
 * of (k1+1)/255.  Given to thr_bm25_topk, OR queries of <= 8 terms hold each candidate doc
 * against the SUM of its own postings' quantised impacts (accumulated in 16 bits per doc slot on
 * chip) instead of the sum of the per-term maxima: ~2.5 % of the postings of a stop-word query lead
 * to a survivor of that bound, ~16 % with the coarse one.  Results are the same bits either way. */
/* term ids outside [0, n_vocab) have no postings: the OR form ignores them, with conjunctive != 0 a
 * non-negative one makes the query unsatisfiable (empty result, as the SQL AND would give).  term_ub / block_ub (or NULL: score
 * every posting): a doc whose bound cannot beat the running k-th best score is dropped before its
 * term frequencies are fetched -- same results, bit for bit.  conjunctive != 0: only docs that
 * hold EVERY query term (the reference's plainto_tsquery is an AND, rag2_schema.sql:365; the
 * oracle's and north star's BM25 is the OR form, the default).  doc_coll [n_docs] / query_coll
 * [nq] (both or neither; query_coll -1 = unfiltered): only docs of the query's collection are
 * ranked, BEFORE the top-k -- ``AND (p_collection IS NULL OR d.collection = p_collection)``,
 * rag2_schema.sql:368-373. */
/* Work decomposition (ABI 5): queries whose lists hold more than one slice's postings (24576 when
 * the batch fills the chip, down to 8192 when it does not -- a one-query call spreads over several
 * workgroups) are cut into doc-range slices (up to 128, equal shares of the query's longest list), every slice is a work item of a
 * persistent grid, the slices of a query share the pruning threshold through a device-side
 * atomic max and are merged at the end -- a stop-word query is the job of many workgroups, not
 * of one.  ``workspace`` >= thr_bm25_workspace_bytes(n_queries, max_terms, k): item list, slice
 * edges, per-slice lists.
 * Batch size: the item list has 3 * n_queries + 32768 slots -- two per query and 16384 for the sweeps
 * and the workgroup walk, one per query and 16384 for the waves' slices -- and the slice sizes of a batch
 * are doubled until its slices fit.  Every query can be a single item of its walk (plus one sweep), so
 * every batch is planned in a bounded number of passes.  The workspace is 48 + 4 * max_terms bytes per
 * query and 368 + 8 * max_terms + 16 * k bytes per slot (item, sweep entry, slice edges, the waves'
 * records, per-slice list and count), each array rounded up to 256 bytes.  More than
 * THR_BM25_MAX_QUERIES queries in one call return THR_ERR_UNSUPPORTED before anything is launched (item
 * counts are 32 bits), and thr_bm25_workspace_bytes returns 0 for them, as for any size it does not take.
 * Wave walk (round 4, same ABI): with the bounds and impacts given, k <= 64 and the OR form, every
 * query of <= 8 terms is cut into slices of ~640-1536 postings instead and ONE WAVE walks a slice
 * (bm25_walk_wave_kernel: no workgroup barrier, sixteen waves -- sixteen independent latency chains --
 * per CU); queries of more terms, AND queries, k > 64 and calls without bounds keep the workgroup walk.
 * Same arithmetic, same bounds: the same bits either way (THR_BM25_WALK=block forces the latter). */
/* Dense terms (ABI 7).  A stop word's posting list is most of the corpus; walking it posting by
 * posting is the slowest way to learn that nearly all of its docs cannot make the top-k.  The
 * caller picks the terms held by a large share of the docs (the host layer: df >= 1 % of the
 * shard's docs, tf <= 65535, at most 512 of them), lists them in ``terms`` and gets, per term, one
 * ROW of thr_bm25_dense_stride(n_docs) entries: dense_imp[row][d] = post_imp of doc d's posting (0:
 * the doc does not hold the term), dense_tf[row][d] = its term frequency.  3 bytes per doc and
 * term.  dense_slot [V] maps a term to its row (-1: none).
 * Given to thr_bm25_topk, an OR query of <= 8 terms that holds such terms is evaluated the
 * MaxScore way, in two stages.  Stage A walks the postings of the query's OTHER terms only; where
 * a doc is scored, the dense terms' frequencies are read from their rows (no search), and every
 * bound carries the dense terms' largest impacts.  Stage B covers the docs that hold none of the
 * other terms: their score is at most the sum of the dense terms' bounds, so when that sum stays
 * below stage A's k-th best score -- the usual case: a stop word's idf is small -- the stage is
 * skipped; otherwise the shard is swept in doc windows, the dense terms' impacts arriving as
 * coalesced loads of the rows (no posting is staged for them), and the few docs whose summed
 * bound reaches the threshold are scored from dense_tf.  Both stages use the oracle's arithmetic
 * in query-term order: the results are the same bits as without the rows. */
int64_t thr_bm25_dense_stride(int64_t n_docs);
int thr_bm25_dense_rows(const int64_t *rowptr, const int32_t *post_doc, const int32_t *post_tf,
                        const uint8_t *post_imp, const int32_t *terms /* [n_terms] */, int n_terms,
                        int64_t n_docs, int64_t max_df /* longest of those lists */,
                        uint8_t *dense_imp /* [n_terms, stride] */,
                        uint16_t *dense_tf /* [n_terms, stride] */, thr_stream_t stream);
size_t thr_bm25_workspace_bytes(int n_queries, int max_terms, int k);
int thr_bm25_topk(const int64_t *rowptr /* [V+1] */, const int32_t *post_doc,
                  const int32_t *post_tf, const float *doclen /* [n_docs] */,
                  const double *idf /* [V] */, const double *term_ub, const double *block_ub,
                  const uint8_t *post_imp /* [nnz] or NULL */,
                  const int32_t *dense_slot /* [V] or NULL */, const uint8_t *dense_imp,
                  const uint16_t *dense_tf, int64_t dense_stride,
                  double avgdl, double k1, double b, int64_t n_docs, int64_t n_vocab,
                  int64_t id_base, const int32_t *query_terms, int n_queries, int max_terms, int k,
                  int conjunctive, const int32_t *doc_coll, const int32_t *query_coll,
                  double *out_scores, int64_t *out_ids, int32_t *out_counts, void *workspace,
                  size_t workspace_bytes, thr_stream_t stream);

/* a4  graph channel: bounded BFS (<= hops) from seed entities over the
 * entity CSR, then score(chunk) = sum_e conf(e,chunk)/(1+dist(e)) over the
 * entity->chunk mention CSR (ascending entity id, float64).
 * Stands where GraphSearcher.search is called, retrieval.py:316-356
 * (src/voice_agent/rag2/graph_search.py:290-418; score form
 * triple-hybrid-rag/src/triple_hybrid_rag/graph/puppygraph.py:152-167).
 * men_chunk holds GLOBAL chunk ids; only [chunk_base, chunk_base+n_chunks)
 * are scored (document sharding).  ``workspace`` >= thr_graph_workspace_bytes.
 * hops is 0..8 (more is THR_ERR_INVALID), max_seeds 1..THR_GRAPH_MAX_SEEDS, k 1..THR_TOPK_MAX.
 * Edge targets (ent_col) and seeds outside [0, n_entities) are ignored: such an edge leads
 * nowhere, such a seed is padding like -1.  In thr_graph_topk a mention of a chunk outside the
 * shard still takes one of a tier's contribution slots (it counts towards the 2048 / 8192 below
 * and for nothing in the scores); in thr_graph_topk_scoped only the mentions a query keeps do. */
size_t thr_graph_workspace_bytes(int n_queries, int64_t n_entities /* 0: no fallback tier */);
/* Three tiers, no host round trip: small on-chip capacities, full on-chip capacities for the
 * queries that overflowed them, and -- when the TRANSPOSED mention CSR is given (chunk ->
 * (entity, conf) in (entity asc, mention) order; tmen_rowptr indexed by LOCAL chunk) -- a
 * capacity-free walk in global memory for the rest, so THR_FLAG_OVERFLOW never comes back.
 * Without it (tmen_* NULL) such a query keeps THR_FLAG_OVERFLOW and its list is incomplete. */
int thr_graph_topk(const int64_t *ent_rowptr, const int32_t *ent_col, int64_t n_entities,
                   const int64_t *men_rowptr, const int32_t *men_chunk, const float *men_conf,
                   const int64_t *tmen_rowptr /* [n_chunks+1] or NULL */,
                   const int32_t *tmen_ent, const float *tmen_conf,
                   int64_t chunk_base, int64_t n_chunks, const int32_t *query_seeds,
                   int n_queries, int max_seeds, int hops, int k, double *out_scores,
                   int64_t *out_ids, int32_t *out_counts, uint32_t *out_flags, void *workspace,
                   size_t workspace_bytes, thr_stream_t stream);
/* thr_graph_topk inside a scope.  The reference's graph search filters every entity and relation
 * query by tenant (.eq("org_id", org_id), src/voice_agent/rag2/graph_search.py:154-230): a tenant's
 * graph list holds that tenant's chunks only.  doc_label int32 [n_chunks] (one label per LOCAL
 * chunk) and query_label int32 [n_queries] (negative = no filter) are the doc_coll / query_coll
 * convention of thr_dense_topk* / thr_bm25_topk, the labels thr_scope_resolve writes: chunk c is in
 * the result of query q only if query_label[q] < 0 or doc_label[c] == query_label[q].  The walk is
 * not filtered (entities carry no attributes: BFS distances are thr_graph_topk's), and an in-scope
 * chunk's score has thr_graph_topk's bits (its mentions in (entity asc, mention) order, float64).
 * Same workspace (thr_graph_workspace_bytes), tiers, flags, padding and order.  In the two on-chip
 * tiers only mentions that are in the shard AND in the scope take a contribution slot (16 lanes of
 * a wave per reached entity count and compact them), so the contribution capacities bound the scope's
 * mentions, not the graph's; the entity capacities are unchanged.  The third tier skips the chunks
 * whose label does not match.  Null doc_label / query_label: THR_ERR_INVALID. */
int thr_graph_topk_scoped(const int64_t *ent_rowptr, const int32_t *ent_col, int64_t n_entities,
                          const int64_t *men_rowptr, const int32_t *men_chunk, const float *men_conf,
                          const int64_t *tmen_rowptr /* [n_chunks+1] or NULL */,
                          const int32_t *tmen_ent, const float *tmen_conf,
                          int64_t chunk_base, int64_t n_chunks,
                          const int32_t *doc_label /* [n_chunks] */,
                          const int32_t *query_label /* [n_queries] */, const int32_t *query_seeds,
                          int n_queries, int max_seeds, int hops, int k, double *out_scores,
                          int64_t *out_ids, int32_t *out_counts, uint32_t *out_flags, void *workspace,
                          size_t workspace_bytes, thr_stream_t stream);

/* a4  seed entities from query keywords, for a batch.  Stands where SQLGraphFallback.find_entities
 * is called (src/voice_agent/rag2/graph_search.py:151-176: per keyword of keywords[:5],
 * rag_entities ... ILIKE '%kw%' LIMIT limit // len(keywords)); the result is the query_seeds table
 * of thr_graph_topk.  Case folding is the caller's: names and keywords arrive lower-cased, as UTF-8
 * bytes, and are compared as bytes (a byte match of valid UTF-8 is a code-point match).
 *   name_bytes uint8: every name followed by ONE 0xFF separator byte (0xFF never occurs in UTF-8),
 *      16-byte aligned; name_ptr int64 [n_entities + 1], name_ptr[0] = 0: name e is the bytes
 *      [name_ptr[e], name_ptr[e + 1] - 1).  REQUIRED PADDING: the allocation holds at least
 *      THR_ENTITY_MAX_NEEDLE further 0xFF bytes behind name_ptr[n_entities] -- the kernel reads a
 *      window of that length at every position and nothing behind name_ptr[n_entities] + the padding;
 *   needles uint8 [n_needles, THR_ENTITY_MAX_NEEDLE], 4-byte aligned + needle_len int32 [n_needles] in
 *      0 .. THR_ENTITY_MAX_NEEDLE: the batch's keywords (the caller de-duplicates them; equal needles
 *      are allowed).  Length 0 matches every entity; a length outside the range or a needle that
 *      holds 0xFF matches none;
 *   query_needles int32 [n_queries, THR_ENTITY_MAX_KEYWORDS]: the query's needles in keyword order,
 *      -1 (or any index outside [0, n_needles)) = none; query_per int32 [n_queries]: the entities a
 *      keyword may contribute, max(1, limit // len(keywords)) -- clamped to THR_GRAPH_MAX_SEEDS here,
 *      which changes no result (only a keyword's first 16 matches can reach a list of 16);
 *   seeds int32 [n_queries, THR_GRAPH_MAX_SEEDS] padded with -1, counts int32 [n_queries]: per
 *      keyword in order its first query_per matching entities in ascending id, those already in the
 *      list skipped (they still count towards query_per), cut at THR_GRAPH_MAX_SEEDS.
 * One pass over the name bytes for all needles (a hash table keyed by a needle's first bytes, built by
 * this call in the workspace: any number of needles, any number sharing a key), per needle its 16
 * smallest matching ids by commuting atomic minima -- the same output every run, no workgroup waits
 * for another, no host read-back -- then one thread per query.  The text is staged in slices of
 * THR_ENTITY_SLICE_BYTES.  Refused before any launch: null pointers, n_entities outside 1 .. 2^31 - 1,
 * n_queries outside 1 .. THR_ENTITY_MAX_QUERIES, n_needles outside 1 .. THR_ENTITY_MAX_KEYWORDS *
 * n_queries, name_bytes not 16-byte, needles not 4-byte or workspace not 8-byte aligned (THR_ERR_INVALID; the size query returns 0), ``workspace``
 * < thr_entity_match_workspace_bytes() (THR_ERR_WORKSPACE). */
#define THR_ENTITY_MAX_NEEDLE 128
#define THR_ENTITY_MAX_KEYWORDS 5
#define THR_ENTITY_MAX_QUERIES (1 << 20)
#define THR_ENTITY_SLICE_BYTES 8192
size_t thr_entity_match_workspace_bytes(int64_t n_entities, int n_needles, int n_queries);
int thr_entity_match(const uint8_t *name_bytes, const int64_t *name_ptr, int64_t n_entities,
                     const uint8_t *needles, const int32_t *needle_len, int n_needles,
                     const int32_t *query_needles, const int32_t *query_per, int n_queries,
                     int32_t *seeds /* [nq, THR_GRAPH_MAX_SEEDS] */, int32_t *counts /* [nq] */,
                     void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* a9  text to BM25 term ids, for a batch.  Stands where rag2_lexical_search hands p_query to
 * plainto_tsquery (rag2_schema.sql:365) for queries and where ingest.py inserts a child chunk's text
 * column (the database tokenises it) for rows; the host restatement is backend.tokenize (\w+ over
 * text.lower()), a lookup in store.vocab and GpuIndexClient._query_terms.
 *
 * THE ANALYSIS IS A TABLE: uint32 [65536], one entry per BMP code point: bits 0..15 the lowered code
 * point, bit 16 (THR_TEXT_WORD) the lowered character is a word character, bit 17 (THR_TEXT_EXC) the
 * code point is exceptional (its lowering is not one BMP code point or depends on context).  Every
 * surrogate's entry carries bit 17.  A text that holds an exceptional code point, a code point above
 * U+FFFF, a surrogate (three-byte generalised UTF-8) or malformed UTF-8 (a stray continuation byte, a
 * character cut off by the end of its text, an overlong form, 0xC0, 0xC1, 0xF5 ..) gets
 * THR_TEXT_EXCEPTIONAL in its flags: the caller redoes it on the host.
 *
 * THE VOCABULARY is an open-addressing table of ``capacity`` (a power of two, THR_VOCAB_MIN_SLOTS ..
 * THR_VOCAB_MAX_SLOTS) 16-byte slots { uint64 hash; int32 term_id; int32 pad } on a 16-byte boundary,
 * all zero when empty, beside the key store: term_bytes uint8 = the keys' UTF-8 as they stand (tokens
 * are lowered before they are compared, keys never), term_ptr int64 [n_vocab + 1], key t =
 * [term_ptr[t], term_ptr[t + 1]).  hash(key) = 64-bit FNV-1a over the key's bytes (h =
 * 0xCBF29CE484222325; per byte h = (h ^ byte) * 0x100000001B3 mod 2^64), a result of 0 replaced by 1
 * (hash 0 = an empty slot).  Home slot = (uint32)(hash ^ (hash >> 32)) & (capacity - 1); linear
 * probing, wrapping at the end; a lookup ends at the first empty slot.  A slot whose hash equals a
 * token's is taken only when the key's bytes equal the lowered token's: otherwise it is passed over.
 *
 * thr_vocab_insert puts keys first_id .. first_id + count - 1 of the key store into the table (each
 * claims the first free slot from its home by a 64-bit compare-and-swap on the hash word): the initial
 * build (first_id 0 into a zeroed table) and growth.  Equal keys in the store are the caller's error.
 * Refused (THR_ERR_INVALID): null pointers, capacity not such a power of two, slots not 16-byte or
 * term_ptr not 8-byte aligned, first_id < 0, count < 1, first_id + count > capacity / 2 (the load
 * stays at or below 1/2: the caller reallocates and inserts everything again).
 * thr_vocab_table_bytes: 16 * capacity, 0 for a capacity thr_vocab_insert refuses.
 *
 * thr_text_tokens: text_bytes uint8, 16-byte aligned + text_ptr int64 [n_texts + 1], text_ptr[0] = 0,
 * ascending, text_ptr[n_texts] = n_bytes: text d is [text_ptr[d], text_ptr[d + 1]).  REQUIRED PADDING:
 * the allocation holds at least 4 readable bytes behind n_bytes; nothing outside [0, n_bytes + 4) is
 * read, whatever the bytes are.
 * A token starts at the lead byte of a word character that is the first byte of its text or whose
 * previous character is not a word character, and runs to the last word character in front of the next
 * other character or the end of its text: no token crosses a text_ptr boundary.  Its term: each
 * character lowered through the table, the lowered characters' UTF-8 hashed as above, the table
 * probed, a hit verified byte for byte against the key store (the lowering can change a character's
 * encoded length; nothing is written anywhere in lowered form).
 *   tok_doc, tok_term int32 [token_capacity]: per token in text order its text and its term id, -1
 *      for a token outside the vocabulary (it still counts); n_tokens int32 [n_texts];
 *   flags int32 [n_texts]: THR_TEXT_EXCEPTIONAL.  The rows of a flagged text may hold anything; they
 *      are n_tokens[d] in number and in their place;
 *   n_total int32 [1]: all tokens.  Rows at or behind token_capacity are not written: a caller that
 *      reads n_total > token_capacity calls again with more room ((n_bytes + n_texts + 1) / 2 always
 *      suffices);
 *   unknown_off int64 / unknown_len int32 [token_capacity], n_unknown int32 [1]: byte offset and byte
 *      length of the tokens with term -1, in text order.
 * Count, scan, scatter over slices of THR_TEXT_SLICE_BYTES bytes staged in LDS with a halo; no
 * workgroup waits for another, nothing is read back, the same bits every run.
 * Refused before any launch: n_texts outside 1 .. THR_TEXT_MAX_TEXTS, n_bytes outside 0 ..
 * THR_TEXT_MAX_BYTES, token_capacity outside 1 .. THR_TEXT_MAX_BYTES (THR_ERR_UNSUPPORTED; the size
 * query returns 0); null pointers, a capacity thr_vocab_insert refuses, n_vocab outside 0 ..
 * capacity / 2, text_bytes or slots not 16-byte, text_ptr / term_ptr / unknown_off / workspace not
 * 8-byte, table not 4-byte aligned (THR_ERR_INVALID); ``workspace`` <
 * thr_text_tokens_workspace_bytes() (THR_ERR_WORKSPACE).
 *
 * thr_query_terms: GpuIndexClient._query_terms for a batch, from the rows of a thr_text_tokens call
 * whose texts are the queries (tok_term, n_tokens, flags, n_total, token_capacity as there): one wave
 * per query over its tokens, 64 at a time.
 *   out_terms int32 [n_queries, THR_BM25_MAX_TERMS]: the distinct known term ids in order of first
 *      appearance, padded with -1 (the query_terms table of thr_bm25_topk);
 *   n_distinct int32 [n_queries]: their number, clamped at THR_BM25_MAX_TERMS + 1;
 *   out_flags int32 [n_queries]: THR_TEXT_EXCEPTIONAL (copied), THR_TEXT_UNKNOWN (a token outside the
 *      vocabulary occurred), THR_TEXT_TOO_MANY (more than THR_BM25_MAX_TERMS distinct terms).
 * Refused: n_queries outside 1 .. THR_TEXT_MAX_TEXTS, token_capacity outside 1 .. THR_TEXT_MAX_BYTES
 * (THR_ERR_UNSUPPORTED; the size query returns 0), null pointers, workspace not 4-byte aligned
 * (THR_ERR_INVALID), ``workspace`` < thr_query_terms_workspace_bytes() (THR_ERR_WORKSPACE). */
#define THR_TEXT_SLICE_BYTES 8192
#define THR_TEXT_MAX_TEXTS (1 << 20)
#define THR_TEXT_MAX_BYTES 0x7FFFFFFF
#define THR_TEXT_WORD (1 << 16)
#define THR_TEXT_EXC (1 << 17)
#define THR_TEXT_EXCEPTIONAL 1
#define THR_TEXT_UNKNOWN 2
#define THR_TEXT_TOO_MANY 4
#define THR_VOCAB_MIN_SLOTS 16
#define THR_VOCAB_MAX_SLOTS (1 << 30)
size_t thr_vocab_table_bytes(int64_t capacity);
int thr_vocab_insert(void *slots, int64_t capacity, const uint8_t *term_bytes, const int64_t *term_ptr,
                     int64_t first_id, int64_t count, thr_stream_t stream);
size_t thr_text_tokens_workspace_bytes(int64_t n_texts, int64_t n_bytes, int64_t token_capacity);
int thr_text_tokens(const uint8_t *text_bytes, const int64_t *text_ptr, int64_t n_texts, int64_t n_bytes,
                    const uint32_t *table /* [65536] */, const void *slots, int64_t capacity,
                    const uint8_t *term_bytes, const int64_t *term_ptr, int64_t n_vocab,
                    int64_t token_capacity, int32_t *tok_doc, int32_t *tok_term, int32_t *n_tokens,
                    int32_t *flags, int32_t *n_total, int64_t *unknown_off, int32_t *unknown_len,
                    int32_t *n_unknown, void *workspace, size_t workspace_bytes, thr_stream_t stream);
size_t thr_query_terms_workspace_bytes(int n_queries);
int thr_query_terms(const int32_t *tok_term, const int32_t *n_tokens, const int32_t *text_flags,
                    const int32_t *n_total, int64_t token_capacity, int n_queries,
                    int32_t *out_terms /* [nq, THR_BM25_MAX_TERMS] */, int32_t *n_distinct,
                    int32_t *out_flags, void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* a9  numbering the new terms of a batch: the ingest step behind thr_text_tokens.  The host restatement is
 * the loop of GpuIndexClient.insert_children / TextSearch.text_rows / index_build.lexical_rows: a token the
 * vocabulary does not hold gets the next id at its first sighting, in text order.
 *
 * thr_vocab_grow takes the batch (text_bytes, text_ptr, n_texts, n_bytes, table: as thr_text_tokens took
 * them, the padding included), the per-text flags and the unknown list (unknown_off, unknown_len,
 * n_unknown) exactly as that call left them, unknown_capacity (the entries the three list arrays hold),
 * n_vocab (the first free id) and hash_mask (below).  All of it is device memory; *n_unknown is read on
 * the device and clamped to 0 .. unknown_capacity, every offset and length is clamped against n_bytes and
 * the end of its text: nothing outside [0, n_bytes + 4) of text_bytes is read, whatever the lists hold.
 *   unknown_term int32 [unknown_capacity]: per occurrence in list order n_vocab + r, r the rank of its
 *      (lowered) token among the distinct new tokens of the batch in order of first appearance in the list.
 *      An occurrence whose text carries THR_TEXT_EXCEPTIONAL gets -1 and is not numbered (its bytes reach
 *      no key).  Entries at or behind *n_unknown are not written;
 *   new_bytes uint8 [new_bytes_capacity], new_ptr int64 [unknown_capacity + 1]: the new keys in id order,
 *      LOWERED (each character through the table, re-encoded: the lowering can change the encoded length);
 *      key r = [new_ptr[r], new_ptr[r + 1]), new_ptr[0] = 0; entries 0 .. n_new are written;
 *   n_new int32 [1], n_new_bytes int64 [1]: the distinct new tokens and their bytes;
 *   status int32 [1]: THR_VOCAB_GROW_COLLISION (two different tokens under one masked hash were merged:
 *      the numbering is not to be used; the caller answers the batch on the host), THR_VOCAB_GROW_OVERFLOW
 *      (new_bytes_capacity < n_new_bytes: n_new / n_new_bytes / new_ptr / unknown_term are right, no byte
 *      at or behind the capacity is written; call again with the room);
 *   tok_term (may be null; then n_total and token_capacity are not looked at): the tok_term of the
 *      thr_text_tokens call with its n_total and token_capacity.  Its entries < 0 are, in row order, the
 *      list: each is replaced by its unknown_term (an entry whose unknown_term is -1 stays -1).
 * The vocabulary table is not touched: committing is thr_vocab_insert over the key store extended by
 * new_bytes / new_ptr.
 * hash_mask: the 64-bit FNV-1a hash of a lowered token (as above) is ANDed with it before the dedupe (a
 * result of 0 replaced by 1).  Production passes all ones; a smaller mask makes collisions reachable for a
 * test.  It concerns the scratch table only, never the keys.
 * Claim (compare-and-swap on the hash word of a zeroed scratch table of 16-byte slots, the smallest power of
 * two >= 2 * unknown_capacity of them, at least 16; the lowest occurrence of a slot kept by an integer
 * max), verify against the slot's first occurrence, scan, emit, patch: commuting integer atomics and
 * kernel boundaries only, no workgroup waits for another, nothing is read back, the same bits every run.
 * Refused before any launch: n_texts / n_bytes outside thr_text_tokens' limits, unknown_capacity outside
 * 1 .. THR_TEXT_MAX_BYTES, with tok_term a token_capacity outside 1 .. THR_TEXT_MAX_BYTES
 * (THR_ERR_UNSUPPORTED; the size query returns 0); null pointers (tok_term alone may be null; with it
 * n_total may not), n_vocab < 0, n_vocab + unknown_capacity > INT32_MAX, hash_mask 0, new_bytes_capacity
 * < 0, text_bytes or workspace not 16-byte, text_ptr / unknown_off / new_ptr / n_new_bytes not 8-byte,
 * table not 4-byte aligned (THR_ERR_INVALID); ``workspace`` < thr_vocab_grow_workspace_bytes()
 * (THR_ERR_WORKSPACE). */
#define THR_VOCAB_GROW_COLLISION 1
#define THR_VOCAB_GROW_OVERFLOW 2
size_t thr_vocab_grow_workspace_bytes(int64_t unknown_capacity);
int thr_vocab_grow(const uint8_t *text_bytes, const int64_t *text_ptr, int64_t n_texts, int64_t n_bytes,
                   const uint32_t *table /* [65536] */, const int32_t *flags, const int64_t *unknown_off,
                   const int32_t *unknown_len, const int32_t *n_unknown, int64_t unknown_capacity,
                   int64_t n_vocab, uint64_t hash_mask, int32_t *tok_term, const int32_t *n_total,
                   int64_t token_capacity, int32_t *unknown_term, uint8_t *new_bytes,
                   int64_t new_bytes_capacity, int64_t *new_ptr, int32_t *n_new, int64_t *n_new_bytes,
                   int32_t *status, void *workspace, size_t workspace_bytes, thr_stream_t stream);

/* a5+a6 candidate merge + weighted Reciprocal Rank Fusion, bit-for-bit the
 * float64 arithmetic and stable ordering of RAG2Retriever._retrieve_candidates
 * / _fuse_rrf, src/voice_agent/rag2/retrieval.py:203-271, 358-376.
 * Channel inputs are ranked id lists [nq, n_*] (negative id = end of list);
 * a null pointer or n_* == 0 disables the channel.  out_ranks: the id's LAST 1-based position
 * in each channel, 0 = absent; rows past out_counts[q] are (-1, -inf, ranks 0).  Refused with
 * THR_ERR_INVALID: top_k outside 1 .. THR_RRF_MAX_TOP_K, n_* above THR_RRF_MAX_PER_CHANNEL, and
 * rrf_k outside 0 .. INT_MAX - THR_RRF_MAX_PER_CHANNEL (k + rank is formed in int). */
int thr_rrf_fuse(const int64_t *lex_ids, int n_lex, const int64_t *sem_ids, int n_sem,
                 const int64_t *graph_ids, int n_graph, int n_queries, double w_lex, double w_sem,
                 double w_graph, int rrf_k, int top_k, int64_t *out_ids /* [nq,top_k] */,
                 double *out_scores /* [nq,top_k] */, int32_t *out_ranks /* [nq,top_k,3] or NULL */,
                 int32_t *out_counts, thr_stream_t stream);

/* f3  the standalone package's RRFFusion on the device (second fusion variant of the reference,
 * triple-hybrid-rag/src/triple_hybrid_rag/core/fusion.py): a channel's table value is
 * ``weight * (1.0 / (60 + rank))`` of the id's LAST rank (:167-185).  two_channels == 0: ``fuse``
 * (:52-165) -- the value is added once per OCCURRENCE of the id in the channel, channels in the
 * order lexical, semantic, graph; two_channels != 0: ``fuse_two_channels(a, b, wa, wb)``
 * (:249-292) with a in the lexical slot and b in the semantic slot (a's value assigned once, b's
 * added per occurrence; graph_ids must be NULL).  Sighting order and stable descending sort as in
 * thr_rrf_fuse; out_ranks (optional) feeds thr_fuse_post. */
int thr_rrf_fuse_standalone(const int64_t *lex_ids, int n_lex, const int64_t *sem_ids, int n_sem,
                            const int64_t *graph_ids, int n_graph, int n_queries, double w_lex,
                            double w_sem, double w_graph, int two_channels, int top_k,
                            int64_t *out_ids, double *out_scores, int32_t *out_ranks /* or NULL */,
                            int32_t *out_counts, thr_stream_t stream);
/* What RRFFusion.fuse does after its sort, and normalize_scores, for a batch of fused lists
 * [n_queries, n] (best first; counts[q] rows valid, NULL = n):
 *   safety_threshold > 0  keep rows whose best channel score max(semantic or 0, lexical or 0,
 *                         graph or 0) is >= it (fusion.py:187-216); the channel scores are read
 *                         at the id's last rank: ranks [n_queries, n, 3] from thr_rrf_fuse*,
 *                         *_scores [n_queries, n_*] float64 (NULL = channel absent);
 *   denoise != 0          with >= 3 rows left: cut = numpy.percentile(scores, 100 * quantile) with
 *                         numpy's linear interpolation, keep scores >= cut (:218-247); the caller
 *                         passes quantile = ((1 - denoise_alpha) * 100) / 100;
 *   top_k > 0             the first top_k of what is left;
 *   normalize != 0        min-max to [0, 1] over what is left, 1.0 when all equal (:294-318).
 * out_* are [n_queries, n] (ids -1 / scores -inf past out_counts[q]). */
int thr_fuse_post(const int64_t *ids, const double *scores, const int32_t *ranks,
                  const int32_t *counts, int n_queries, int n, const double *lex_scores, int n_lex,
                  const double *sem_scores, int n_sem, const double *graph_scores, int n_graph,
                  double safety_threshold, int denoise, double quantile, int normalize, int top_k,
                  int64_t *out_ids, double *out_scores, int32_t *out_counts, thr_stream_t stream);

/* a8  late-interaction rerank: MaxSim(q, c) = sum_i max_j <q_i, d_cj> with
 * float16 token matrices on MFMA (float32 accumulate).
 * Stands where Qwen3VLReranker._rerank_batch_native is called,
 * retrieval.py:427 (src/voice_agent/retrieval/reranker.py:287-354).
 * cand [nq, n_cand] are LOCAL doc indices into dtok, negative = padding
 * (score -inf).  q_tokens, d_tokens multiples of 32; tok_dim one of 16, 32, 64, 96, 128, 192, 256
 * (one kernel each).  Any other shape is THR_ERR_UNSUPPORTED, from thr_maxsim_pack too and before a
 * pointer is looked at.  n_queries is not bounded by the grid: a batch above the device's
 * gridDim.y limit is launched in slices. */
int thr_maxsim(const uint16_t *qtok /* f16 [nq,q_tokens,tok_dim] */, int n_queries, int q_tokens,
               const uint16_t *dtok /* f16 [n_docs,d_tokens,tok_dim], or its packed image */,
               int64_t n_docs, int d_tokens, int tok_dim, const int32_t *cand, int n_cand,
               float *out_scores /* [nq,n_cand] */, int dtok_packed, thr_stream_t stream);
/* The same with the candidates as GLOBAL ids (what thr_rrf_fuse returns) of a shard whose local
 * doc 0 has id id_base: local = id - id_base; negative ids and ids of other shards score -inf.
 * (Saves the caller the id arithmetic: nine elementwise launches per batch in PyTorch.) */
int thr_maxsim_ids(const uint16_t *qtok, int n_queries, int q_tokens, const uint16_t *dtok,
                   int64_t n_docs, int d_tokens, int tok_dim, const int64_t *cand_ids /* [nq,n_cand] */,
                   int64_t id_base, int n_cand, float *out_scores, int dtok_packed,
                   thr_stream_t stream);
/* Ordering after the rerank (retrieval.py:449-455): candidate p of query q gets the maximum of
 * scores[l][q][p] over the n_lists lists (document-sharded index: the shard that owns the
 * candidate wrote its MaxSim score, the others -inf; list_stride in floats, 0 = n_queries * n),
 * ``rerank_score or 0`` for a candidate nobody scored, and the first counts[q] candidates
 * (NULL = n) are stably sorted by it, descending -> top_k ids / float64 scores / counts. */
int thr_rerank_order(const float *scores /* [n_lists][nq,n] */, int n_lists, int64_t list_stride,
                     const int64_t *ids /* [nq,n] */, const int32_t *counts /* [nq] or NULL */,
                     int n_queries, int n, int top_k, int64_t *out_ids /* [nq,top_k] */,
                     double *out_scores /* [nq,top_k] */, int32_t *out_counts, thr_stream_t stream);
/* Index build: re-lay the token store fragment-major ([doc][32-token tile][k-step][lane][8
 * halves], the register image of the MFMA operand) so thr_maxsim(dtok_packed = 1) reads 1 KiB
 * contiguous per load instruction.  Out of place; same size as dtok.  Takes exactly the shapes
 * thr_maxsim scores: a store no later rerank could read is refused here. */
int thr_maxsim_pack(const uint16_t *dtok, int64_t n_docs, int d_tokens, int tok_dim,
                    uint16_t *packed, thr_stream_t stream);

/* Merge step of the multi-GPU path: G per-shard ranked lists -> global top-k under
 * (score desc, id asc).  List l of query q starts at in_*[l * list_stride + q * k_in]
 * (elements); list_stride = 0 means n_queries * k_in, i.e. the [n_lists, n_queries, k_in]
 * layout an all-gather of each rank's [n_queries, k_in] block produces -- a larger stride lets
 * scores and ids be read in place from one gathered [n_lists, 2, n_queries, k_in] tile.
 * Entries with a score of -inf or NaN or a negative id are padding; +inf is a score, and
 * -0.0 == +0.0 (the id decides).  The result is the top k_out of the MULTISET of entries: the
 * same (score, id) pair in two lists comes out twice, the copy of the lower-numbered list
 * first (disjoint shards never produce one; no (-inf, -1) hole is left inside
 * out_counts[q] either way).  Lists that arrive ranked (the normal case) are merged without
 * a sort.  k_out is at most 512; rows past out_counts[q] are (-inf, -1). */
int thr_merge_topk(const double *in_scores, const int64_t *in_ids, int n_queries, int n_lists,
                   int k_in, int64_t list_stride, int k_out, double *out_scores, int64_t *out_ids,
                   int32_t *out_counts, thr_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* THR_HIP_H */
