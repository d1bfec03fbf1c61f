/*
 * literalkg_hip_lists.h -- scoring and ranking against per-query candidate lists of the MI355X (gfx950) LiteralKG
 * library, under the conventions of literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no
 * allocation, 0 on success and a negative lkg_status with lkg_last_error() otherwise).  literalkg_amd/_native.py binds it
 * from its ninth table, LIST_PROTOTYPES; literalkg_amd/lists.py (score_lists, rank_in_lists, evaluate_list_ranking)
 * drives it.
 */
#ifndef LITERALKG_HIP_LISTS_H
#define LITERALKG_HIP_LISTS_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Operands of both entry points.  q[n_q x k] (row stride q_stride) the query rows lkg_rank_queries_f32 makes; p[n_rows x k]
 * (row stride p_stride) the candidate rows with their squared norms pn[n_rows] (lkg_rank_sqnorm_f32; NULL: dot scoring);
 * lists[n_q x m] (row stride lists_stride, m >= 1) the slots of every query: slot j of query i holds a row number of p, or a
 * negative value for an EMPTY slot.  A row number at or past n_rows is treated as an empty slot (nothing is read out of
 * bounds); callers check their ids beforehand.
 *
 * The kernel score of (query i, row c) is s = pn[c] - 2 q_i . p_c (dot scoring: -2 q_i . p_c), the bits
 * lkg_rank_count_f32 compares and lkg_triple_scores_f32 stores for that (query, candidate), whatever slot, slice, wave
 * or launch computes it.
 *
 *   lkg_list_scores_f32   out[i * out_stride + j] = the score of slot j of query i, NaN for an empty slot.  flags bit 0
 *                         (reported): qn[i] + s with pn given (qn[n_q]: lkg_rank_sqnorm_f32 over q, required then) or
 *                         -s / 2 for dot scoring; flags 0: s itself (qn is not read).
 *   lkg_list_count_f32    truth[n_q] holds the row of p that is query i's truth; its score comes from the same chain.
 *                         Slot j of query i is COUNTED unless it is empty, its row is truth[i], or the filter drops it:
 *                         (filter_row[n_q], filter_rel[n_q], rowptr, col, eptr, rel) of lkg_csr_build_device over entity
 *                         ids, query i dropping the slots whose entity id is a col of row filter_row[i] under relation
 *                         filter_rel[i] (negative: under any).  cand_ids[n_rows] is the entity id of every row of p
 *                         (NULL: the row number).  The filter is absent (rowptr NULL) or complete.
 *                         kept[i] += the counted slots, better[i] += those with s < s_truth, equal[i] += those with
 *                         s == s_truth, by float32 compares (a NaN on either side is neither).  The caller zeroes the
 *                         three int64 arrays; the additions are integer atomics, so no order enters.  No score is stored.
 *
 * The row strides are named *_stride, in elements: tests/test_lists_gpu.py places p itself past 2^31 and 2^32 elements
 * (the ledger of tests/wide_cases.py follows the arguments named ld* of the training and query entry points).
 *
 * Conventions: n_q * ceil(m / 256) below 2^31 - 1 (one workgroup per query and slice of 256 slots); n_rows below
 * 2^31 - 1; all row offsets are 64-bit; 16-byte loads are used only where q, p and their strides allow them; n_q == 0 launches
 * nothing; a bad size, a null pointer or an incomplete filter is LKG_ERR_INVALID_ARG before any launch.  No float
 * atomics.                                                                                                             */
int lkg_list_scores_f32(int64_t n_q, int64_t m, int64_t n_rows, int32_t k, const float *q, int64_t q_stride, const float *qn,
                        const float *p, int64_t p_stride, const float *pn, const int64_t *lists, int64_t lists_stride,
                        int32_t flags, float *out, int64_t out_stride, void *stream);

int lkg_list_count_f32(int64_t n_q, int64_t m, int64_t n_rows, int32_t k, const float *q, int64_t q_stride, const float *p,
                       int64_t p_stride, const float *pn, const int64_t *lists, int64_t lists_stride, const int64_t *truth,
                       const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                       const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                       int64_t *better, int64_t *equal, int64_t *kept, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_LISTS_H */
