/* thr_hip_text.h -- lexical analysis entry points of libthr_hip.so that came after ABI version 9.
 *
 * An additive companion of thr_hip.h (same library, same conventions, same workspace contract,
 * THR_ABI_VERSION unchanged): every pointer is device memory unless its name begins with h_, all
 * work is enqueued on ``stream``, nothing synchronises, allocates or frees; 0 on success, a negative
 * THR_ERR_* for an argument error, a positive hipError_t if a launch failed.
 */
#ifndef THR_HIP_TEXT_H
#define THR_HIP_TEXT_H

#include "thr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* a9  token-level analysis behind the character table: a stop list and suffix stemming.  The reference
 * sends p_query and every chunk's text through PostgreSQL's 'portuguese' text-search configuration
 * (plainto_tsquery('portuguese', q) in rag2_lexical_search, the generated tsv column), which drops stop
 * words and stems the rest.  No Snowball and no Postgres stop file is restated here: the analysis is
 * DATA, as the character table is, and its definition is index_text.Analyzer, in plain Python:
 *
 *   stem(tok):    for each step in order: among the step's rules (suffix, min_stem) with
 *                 tok.endswith(suffix) and len(tok) - len(suffix) >= min_stem the one with the longest
 *                 suffix is taken (none: the step does nothing) and tok = tok[:-len(suffix)];
 *   tokens(text): [stem(t) for t in table_tokens(text) if t not in stop]
 *
 * with lengths in code points of the LOWERED token, the stop check on the whole lowered token before
 * any stemming, and rules that only ever strip.  A stem is therefore the lowered form of a prefix of
 * the token's bytes in the text: it is named by (byte offset, byte length of the kept prefix), and
 * everything behind this call -- the unknown list, thr_vocab_grow's lowering, dedupe and key emit,
 * thr_query_terms -- takes these outputs exactly as it takes thr_text_tokens'.
 *
 * thr_text_tokens_analyzed takes everything thr_text_tokens takes (same meaning, same padding rule:
 * nothing outside [0, n_bytes + 4) of text_bytes is read, whatever the bytes are) and
 *
 *   THE STOP SET, in the vocabulary's own layout: stop_slots (stop_capacity 16-byte slots { uint64
 *      hash; int32 id; int32 pad }, built by thr_vocab_insert over the stop words' key store),
 *      stop_bytes / stop_ptr int64 [n_stop + 1] (the stop words as the tokenizer produces them:
 *      lowered).  The lookup is the vocabulary's: probe from the home slot, a slot with the token's hash
 *      is taken only when its key equals the lowered token byte for byte, otherwise passed over; it ends
 *      at the first empty slot.  stop_capacity 0 with three null pointers and n_stop 0: no stop list.
 *
 *   THE RULE TABLE: h_step_ptr int32 [n_steps + 1] in HOST memory (read during the call, not kept),
 *      rules in device memory, 8-byte aligned: h_step_ptr[n_steps] records of 24 bytes
 *          { uint16 tail[8]; int32 len; int32 min_stem }
 *      tail[i] is the i-th code point from the END of the suffix (tail[0] its last), entries at or
 *      behind len are 0; len is the suffix's length in code points, 1 .. THR_STEM_MAX_SUFFIX; min_stem
 *      >= 1 the code points that must remain.  Rules h_step_ptr[s] .. h_step_ptr[s + 1] - 1 are step s.
 *      DEVICE SEMANTICS: within a step the FIRST rule in table order that matches wins.  A table
 *      compiled longest-suffix-first (index_text.Analyzer does) is the definition above; a table in
 *      another order is answered in that order.  The records are device memory, which the host cannot
 *      check: a len outside 1 .. 8 is CLAMPED into it and a min_stem below 1 to 1 on the device (a stem
 *      is never empty and never reaches in front of its token, whatever the table holds).
 *
 * Outputs: thr_text_tokens', except that a stop token produces NO ROW -- n_tokens[d] and n_total count
 * the kept tokens only (the BM25 document length built from these rows leaves stop words out); rows
 * stay in text order at scanned positions; tok_term is the id of the STEM, -1 for a stem outside the
 * vocabulary; for such a row unknown_off is the token's first byte and unknown_len the BYTE LENGTH OF
 * THE KEPT PREFIX IN THE SOURCE BYTES (the lowering can change a character's encoded length: the length
 * reported is the text's, not the lowered stem's).  Flags as thr_text_tokens: the rows of a flagged text
 * may hold anything, n_tokens[d] in number and in their place.
 * With no stop list and n_steps 0 every output equals thr_text_tokens'.
 *
 * Count, scan, scatter over slices of THR_TEXT_SLICE_BYTES bytes, one lane per token, as
 * thr_text_tokens.  The drop is decided PER TOKEN IN THE COUNT PASS (with a stop list the count pass
 * walks each token and probes the stop set; the emit pass decides again from the same bytes), so the
 * scanned positions are the kept rows' and no further compaction or row buffer exists.  The emit pass
 * holds a token's last THR_STEM_MAX_STEPS * THR_STEM_MAX_SUFFIX lowered code points in registers,
 * matches them against the rules staged in LDS, and walks the kept prefix again for its hash when a
 * rule stripped something.  No workgroup waits for another, only commuting integer atomics, nothing
 * read back, the same bits every run, whatever the workspace held.
 * What is clamped and what is by construction: every byte is read through a walk that stops at the end
 * of its text (itself clamped to n_bytes), every key read lies inside [stop_ptr[id], stop_ptr[id + 1])
 * of a slot whose id is inside 0 .. n_stop - 1 (others are passed over), every rule index is below
 * h_step_ptr[n_steps] <= THR_STEM_MAX_RULES, and rows at or behind token_capacity are not written.
 *
 * Refused before any launch: thr_text_tokens' refusals, and (THR_ERR_INVALID) n_steps outside 0 ..
 * THR_STEM_MAX_STEPS, a null h_step_ptr with n_steps > 0, h_step_ptr[0] != 0, a descending
 * h_step_ptr, an entry above THR_STEM_MAX_RULES, null or not 8-byte aligned rules with at least one
 * rule, a stop_capacity thr_vocab_insert refuses, n_stop outside 0 .. stop_capacity / 2, a null stop
 * pointer with a non-zero capacity (or a non-null one, or n_stop != 0, with capacity 0), stop_slots not
 * 16-byte or stop_ptr not 8-byte aligned; ``workspace`` < thr_text_tokens_analyzed_workspace_bytes()
 * (THR_ERR_WORKSPACE; the size is thr_text_tokens_workspace_bytes'). */
#define THR_STEM_MAX_SUFFIX 8
#define THR_STEM_MAX_STEPS 4
#define THR_STEM_MAX_RULES 1024
#define THR_STEM_RULE_BYTES 24
size_t thr_text_tokens_analyzed_workspace_bytes(int64_t n_texts, int64_t n_bytes, int64_t token_capacity);
int thr_text_tokens_analyzed(const uint8_t *text_bytes, const int64_t *text_ptr, int64_t n_texts,
                             int64_t n_bytes, const uint32_t *table /* [65536] */, const void *slots,
                             int64_t capacity, const uint8_t *term_bytes, const int64_t *term_ptr,
                             int64_t n_vocab, const void *stop_slots /* or NULL */, int64_t stop_capacity,
                             const uint8_t *stop_bytes /* or NULL */, const int64_t *stop_ptr /* or NULL */,
                             int64_t n_stop, const int32_t *h_step_ptr /* host, [n_steps + 1] */,
                             int n_steps, const void *rules /* or NULL */, int64_t token_capacity,
                             int32_t *tok_doc, int32_t *tok_term, int32_t *n_tokens, int32_t *flags,
                             int32_t *n_total, int64_t *unknown_off, int32_t *unknown_len,
                             int32_t *n_unknown, void *workspace, size_t workspace_bytes,
                             thr_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* THR_HIP_TEXT_H */
