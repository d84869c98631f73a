/* thr_hip_graph.h -- graph mutation entry points of libthr_hip.so that came after ABI version 9.
 *
 * An additive companion of thr_hip.h (same library, same conventions, same workspace contract,
 * THR_ABI_VERSION unchanged): every pointer is device memory, all work is enqueued on ``stream``,
 * nothing synchronises, allocates or frees; 0 on success, a negative THR_ERR_* for an argument
 * error, a positive hipError_t if a launch failed.
 */
#ifndef THR_HIP_GRAPH_H
#define THR_HIP_GRAPH_H

#include "thr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* f3  graph delete: one order-preserving pass over a CSR that drops rows, entries by id and
 * (row, id) pairs.  The reference's schema hangs rag_entities.document_id,
 * rag_entity_mentions.entity_id, rag_relations.subject_entity_id / object_entity_id and
 * rag_relations.document_id on ON DELETE CASCADE
 * (database/migrations/20260114_rag2_schema.sql:187, 217-220, 254, 258-259): deleting a document
 * removes the entities first extracted from it, every relation that touches them and every mention
 * of them.  Here the survivors keep their order and are renumbered, so what is left is what
 * index_build.build_graph over the surviving rows would hold.
 *   A: rowptr_a [rows_a + 1], ids_a int32 [nnz_a], pay_a [nnz_a] an opaque 4-byte companion or NULL;
 *      the rows need not be sorted;
 *   row_remap int32 [rows_a] or NULL: the new row of old row t, -1 = the row is removed with
 *      everything in it; ascending over the survivors, 0 .. rows_out - 1.  NULL: every row stays
 *      (rows_out == rows_a);
 *   id_remap int32 [n_ids] or NULL, with id_base: as thr_csr_compact -- an entry is kept only if
 *      0 <= id - id_base < n_ids and id_remap[id - id_base] >= 0, and is written as
 *      id_remap[id - id_base] + id_base.  NULL (n_ids == 0): ids pass through untouched and unchecked;
 *   B: rowptr_b [rows_a + 1], ids_b int32 [nnz_b], or both NULL (nnz_b == 0): strictly ascending
 *      within a row, in A's OLD numbering.  An entry of A's row t whose id is in B's row t is dropped
 *      (in a multiset row every copy); a B entry that names nothing in A is ignored; B's rows under
 *      removed rows are ignored altogether (not read, not checked);
 *   out: rowptr_out [rows_out + 1], ids_out / pay_out with room for out_capacity elements,
 *      keep_out uint8 [nnz_a] or NULL (1 = the entry survived), *nnz_out, *status_out (buffers of
 *      their own).  Kept entries keep their relative order.
 * *status_out is 0 or a sum of THR_CSR_PRUNE_UNSORTED_B (a row of B is not strictly ascending: the
 * result is undefined, though inside its buffers, and must not be used), THR_CSR_PRUNE_OVERFLOW
 * (*nnz_out > out_capacity: only positions below out_capacity were written) and
 * THR_CSR_PRUNE_BAD_ROW (row_remap names a destination >= rows_out: that row is treated as removed
 * and its pointer is not written).
 * Of ids_out / pay_out the first min(*nnz_out, out_capacity) elements are written, nothing behind.
 * Work is cut in slices of THR_CSR_PRUNE_SLICE positions of A, not by row; three launches (count,
 * scan, scatter), no workgroup waits for another, stream-ordered, no host round trip inside;
 * ``workspace`` (8-byte aligned) >= thr_csr_prune_workspace_bytes().  The kernels check every source
 * index against nnz_a / nnz_b, every remap index against its length and every destination against
 * out_capacity / rows_out.  THR_ERR_INVALID before any launch: a null pointer with a non-zero size,
 * a negative size, rows_out > rows_a (NULL row_remap: rows_out != rows_a), a payload on one side
 * only, a destination that is one of the sources, B's ids without rowptr_b.  rows_a == 0 and
 * nnz_a == 0 are valid and write an empty result. */
#define THR_CSR_PRUNE_SLICE 1024
#define THR_CSR_PRUNE_UNSORTED_B 1
#define THR_CSR_PRUNE_OVERFLOW 2
#define THR_CSR_PRUNE_BAD_ROW 4
int thr_csr_prune_slice(void);    /* THR_CSR_PRUNE_SLICE as the library was built */
size_t thr_csr_prune_workspace_bytes(int64_t rows_a, int64_t nnz_a);
int thr_csr_prune(const int64_t *rowptr_a, int64_t rows_a, int64_t nnz_a, const int32_t *ids_a,
                  const void *pay_a /* or NULL */, const int32_t *row_remap /* or NULL */,
                  int64_t rows_out, const int32_t *id_remap /* or NULL */, int64_t n_ids,
                  int64_t id_base, const int64_t *rowptr_b /* or NULL */, int64_t nnz_b,
                  const int32_t *ids_b /* or NULL */, int64_t *rowptr_out, int32_t *ids_out,
                  void *pay_out /* or NULL */, int64_t out_capacity, uint8_t *keep_out /* or NULL */,
                  int64_t *nnz_out, int32_t *status_out, void *workspace, size_t workspace_bytes,
                  thr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* THR_HIP_GRAPH_H */
