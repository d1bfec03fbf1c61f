/*
 * literalkg_hip_pair_accept.h -- threshold retrieval under the MLP pair head of the MI355X (gfx950) LiteralKG library,
 * under the conventions of literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no allocation,
 * 0 on success and a negative lkg_status with lkg_last_error() otherwise).  literalkg_amd/_native.py binds it from its
 * eighth table, PAIR_ACCEPT_PROTOTYPES; literalkg_amd/pairmlp.py (predict_accepted_mlp, count_accepted_mlp) drives it.
 */
#ifndef LITERALKG_HIP_PAIR_ACCEPT_H
#define LITERALKG_HIP_PAIR_ACCEPT_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The three entry points below share their operands with lkg_pair_mlp_select_f32 (lkg_pairmlp.hip): uq[n_q x 128] the
 * projected query rows (fc1's bias included), v[n_cand x 128] the projected candidate rows, (w2, b2, w3, b3) the folded
 * head, cand_ids[n_cand] the entity id of every candidate row (NULL: the row number), and the known-triples filter
 * (filter_row[n_q], filter_rel[n_q], rowptr, col, eptr, rel) of lkg_csr_build_device over entity ids: query i drops the
 * candidates whose id is a col of row filter_row[i] under relation filter_rel[i] (-1: under any).  The filter is absent
 * (rowptr NULL) or complete.  thr[n_q] holds one float32 logit threshold per query.
 *
 * The decision.  z(i, c) is the logit lkg_pair_mlp_scores_f32 stores for the pair, bit for bit, whatever tile, wave,
 * split or launch computes it.  Candidate c of query i is ACCEPTED iff z(i, c) > thr[i] in one float32 compare, strictly
 * (a NaN logit or a NaN threshold accepts nothing; thr = +inf accepts nothing; thr = -inf accepts every logit that is
 * neither NaN nor -inf), and the filter does not drop it.  Only a candidate that passes the compare is looked up in the
 * filter.
 *
 *   lkg_pair_mlp_accept_count_f32    counts[i] += the number of accepted candidates of query i.  The caller zeroes
 *                                    counts.  Integer atomics only: the counts do not depend on the order of anything.
 *   lkg_pair_mlp_accept_append_f32   the same counts, and in the same pass every accepted entry takes a slot from the
 *                                    ONE 64-bit cursor (*cursor, zeroed by the caller).  A slot below `capacity` writes
 *                                    out_rows[slot] = i, out_ids[slot] = the id, out_logits[slot] = z; a slot at or past
 *                                    it writes nothing.  The counts are exact whether or not the buffer overflows, and
 *                                    overflow is sum(counts) > capacity (then *cursor == sum(counts) too).  The entries
 *                                    are in no particular order.  capacity == 0 needs no output buffers.
 *   lkg_pair_mlp_accept_emit_f32     the second pass of the two-pass route: counts[n_q] are those of a count over the
 *                                    same arguments, base[n_q] their exclusive scan (int64), cursor[n_q] zeroed by the
 *                                    caller.  Every accepted entry of query i takes slot = cursor[i]++ and writes
 *                                    out_ids / out_scores (s = -2 z, exact, the ascending key of lkg_accept_order) /
 *                                    out_logits at base[i] + slot when 0 <= slot < counts[i]; otherwise it writes
 *                                    nothing and sets *flag to 1.  With the counts of the same arguments the flag stays 0.
 *                                    A row's entries are in no particular order; (s, id) is unique within a row, so
 *                                    lkg_accept_order makes the result unique.
 *
 * splits: candidate splits per launch, 0 = automatic, else 1 .. LKG_TOPK_MAX_SPLITS; resolved by lkg_pair_mlp_splits.
 * No result depends on it.
 *
 * Conventions: uq and v hold DENSE rows of 128 floats -- row i starts at element 128 i; there is no row-stride argument
 * (the projections that feed these entry points are dense, and every row-strided operand of this library is an operand
 * that has to be exercised past 2^32 elements) -- and uq, v and w2 are 16-byte aligned; n_q, n_cand and capacity below
 * 2^31 - 1; n_q == 0 or n_cand == 0 launches nothing; a bad size, a null pointer, a misaligned operand or an incomplete
 * filter is LKG_ERR_INVALID_ARG before any launch.  No float atomics.                                                      */
int lkg_pair_mlp_accept_count_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                  const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                                  const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                  const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                  int32_t splits, int32_t *counts, void *stream);

int lkg_pair_mlp_accept_append_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                   const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                                   const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                   const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                   int32_t splits, int32_t *counts, int64_t capacity, int64_t *cursor, int32_t *out_rows,
                                   int32_t *out_ids, float *out_logits, void *stream);

int lkg_pair_mlp_accept_emit_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                 const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                                 const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                 const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                 int32_t splits, const int32_t *counts, const int64_t *base, int32_t *cursor,
                                 int64_t *out_ids, float *out_scores, float *out_logits, int32_t *flag, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_PAIR_ACCEPT_H */
