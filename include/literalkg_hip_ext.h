/*
 * literalkg_hip_ext.h -- further entry points of the MI355X (gfx950) LiteralKG library, under the conventions of
 * literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no allocation, 0 on success and a negative
 * lkg_status with lkg_last_error() otherwise, "ld*" in elements).  literalkg_amd/_native.py binds them from its second
 * table, EXTRA_PROTOTYPES.
 */
#ifndef LITERALKG_HIP_EXT_H
#define LITERALKG_HIP_EXT_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* KvsAll training loss (lkg_kvsall.hip; literalkg_amd/kvs_all.py): binary cross-entropy with logits of EVERY candidate
 * against the multi-hot vector of a query's known answers.  Queries, candidates and the kernel score s(i, c) as for
 * lkg_rank_* / lkg_softmax_all_*, bit for bit.  The logit is
 *     z(i, c) = fl(fl(-scale * beta * s(i, c)) + bias[i])      (pn given: beta = 1; pn NULL: beta = 1/2, s = -2 q.p),
 * bias float[n_q] or NULL (= 0); scale > 0, finite.  The positives of query i are the candidate POSITIONS
 * ycol[yptr[i] .. yptr[i + 1]) (ascending, unique, n_pos = yptr[n_q] < 2^31 entries in all; lkg_softmax_excluded with
 * truth = -1 builds them); yptr NULL = every list empty, with the same bits.  With y = 1 on a positive and 0 elsewhere,
 *     loss_i = sum_c softplus(z) - y' z,      y' = (1 - eps) y + eps / n,      0 <= eps < 1  (label smoothing),
 * each term as softplus(y ? -z : z) + ce_y z with ce_1 = eps (1 - 1/n), ce_0 = -eps / n formed in double and rounded once;
 * with eps == 0 the product is not executed.  A NaN logit poisons its own row only.
 *
 * lkg_sigmoid_all_partial_f32: per split j and query i  ws[j * n_q + i] = the sum of the terms of the split's candidates
 *     (splits = lkg_softmax_all_splits(n_q, n_cand, splits); n = n_cand).  The n_q x n_cand logits are never stored.
 * lkg_sigmoid_all_finish_f32 : loss[i] = fl32(sum_j ws[j * n_q + i]), added in split order in float64 (any splits >= 1: it
 *     also adds the row sums of lkg_sigmoid_all_weights_f32 over that call's tiles).
 * lkg_sigmoid_all_weights_f32: the backward's recompute for a chunk of n_cand candidates that starts at candidate c_base
 *     of the n_total candidates the forward pass ran over (p and pn point AT the chunk; bias and g are per query; the lists
 *     hold positions of the whole table, and n of the smoothing is n_total, not the chunk's width):
 *         v[i * ldv + c] = scale * beta * g[i] * (sigma(z(i, c_base + c)) - y'(i, c_base + c)),
 *     evaluated as ce_1 - sigma(-z) for a positive and sigma(z) + ce_0 otherwise.  With it  dQ = 2 V P,
 *     dP = 2 V^T Q - 2 diag(colsum V) P  (the second term only with pn)  and  dbias = rowsum(V) / (scale * beta).
 *     rowsum (nullable) float[ceil(n_cand / 256) * n_q]: rowsum[t * n_q + i] = the sum of v[i, 256 t .. 256 t + 255] as
 *     stored, added in a fixed order in registers and LDS.
 * No float atomics: for a given number of splits every output repeats bit for bit.  n_q == 0 launches nothing;
 * addressing is 64-bit.                                                                                               */
int lkg_sigmoid_all_partial_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *pn, const float *bias, float scale, double eps, int32_t splits,
                                const int32_t *yptr, const int32_t *ycol, int64_t n_pos, float *ws, void *stream);
int lkg_sigmoid_all_finish_f32(int64_t n_q, int32_t splits, const float *ws, float *loss, void *stream);
int lkg_sigmoid_all_weights_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *pn, const float *bias, int64_t c_base, int64_t n_total,
                                const float *g, float scale, double eps, const int32_t *yptr, const int32_t *ycol,
                                int64_t n_pos, float *v, int64_t ldv, float *rowsum, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_EXT_H */
