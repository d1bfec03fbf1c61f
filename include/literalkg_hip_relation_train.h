/*
 * literalkg_hip_relation_train.h -- the relation-slot training objective of the MI355X (gfx950) LiteralKG library, under
 * the conventions of literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no allocation, 0 on
 * success and a negative lkg_status with lkg_last_error() otherwise, "ld*" in elements).  literalkg_amd/_native.py binds
 * them from its fifth table, RELATION_TRAIN_PROTOTYPES.
 */
#ifndef LITERALKG_HIP_RELATION_TRAIN_H
#define LITERALKG_HIP_RELATION_TRAIN_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Softmax cross-entropy of the true relation of a pair against every relation (lkg_relation_loss.hip;
 * literalkg_amd/relation_loss.py).  n pairs, n_rel >= 1 relations, k >= 1 float32 columns per block.
 *
 * Slab mode (rel_stride > 0): pair i, relation j owns the block u[i * ldu + j * rel_stride ..] of k columns
 * (rel_stride >= k, ldu >= (n_rel - 1) * rel_stride + k).  Shared mode (rel_stride == 0): pair i owns the ONE row
 * u[i * ldu ..] of k columns, read for every relation (ldu >= k).  With e[j * lde ..] the relation's row (lde >= k),
 *     s_ij = sum_c (u_ijc + e_jc)^2   summed directly (one fma chain per lane over its 4-column units lane, lane + 64, ...,
 *                                     then one butterfly over the wave),
 *     z_ij = -fl(scale * s_ij),       scale > 0 and finite.
 * A filter (rowptr != NULL: the four arrays of lkg_csr_build_device, filter_row[n] and filter_col[n] in its row and column
 * ids, all in range) makes every relation rr != truth[i] listed under the entry (filter_row[i], filter_col[i]) ineligible:
 * z[i, rr] = -inf.  truth[i] in [0, n_rel) is never dropped; duplicates in the filter change nothing.  Then
 *     m_i = max_j z_ij,   sum_i = sum_j exp(z_ij - m_i),   lse_i = m_i + log(sum_i),
 *     loss_i = (m_i - z_i,truth_i) + log(sum_i)
 * (a pair whose only eligible relation is the truth: exactly 0).
 *
 * lkg_relation_loss_fwd_f32 stores z[i * ldz + j] (ldz >= n_rel), lse[n] and loss[n], each element once (a dropped
 * relation's logit twice: the value, then -inf).
 * lkg_relation_loss_bwd_f32 reads the upstream g[n], z and truth, takes m_i and sum_i from the stored row again (the
 * forward's own passes: the same bits; exp(z_ij - lse_i) would carry half an ulp of lse into every softmax) and forms
 *     c_ij = fl(fl(-2 scale * g_i) * (exp(z_ij - m_i) / sum_i - [j == truth_i])),      exactly 0.0 where z_ij = -inf.
 *   Slab mode: every block of u is OVERWRITTEN in place by c_ij (u_ij + e_j), each element stored once (zeros, not
 *     products, where z_ij = -inf); gd and c must be NULL.
 *   Shared mode: u is only read; gd[i * ldgd ..] = sum_j c_ij (u_i + e_j), added in increasing j (ldgd >= k), and
 *     c[i * ldc + j] = c_ij (ldc >= n_rel).  Either of gd, c may be NULL: it is not computed, the other keeps its bits.
 *
 * One wave per pair.  A pair's outputs depend on its own blocks, e, its truth and its filter entry alone -- not on n, on
 * its position or on other pairs -- the sums run in a fixed order and there are no atomics: every output repeats bit for
 * bit, and the 16-byte and the scalar load path (taken when k, a stride or a pointer is not a multiple of 4 elements /
 * 16 bytes) give the same bits.  n == 0 launches nothing; addressing is 64-bit.                                          */
int lkg_relation_loss_fwd_f32(int64_t n, int32_t n_rel, int32_t k, const float *u, int64_t ldu, int64_t rel_stride,
                              const float *e, int64_t lde, const int64_t *truth, const int64_t *filter_row,
                              const int64_t *filter_col, const int32_t *rowptr, const int32_t *col, const int32_t *eptr,
                              const int32_t *rel, float scale, float *z, int64_t ldz, float *lse, float *loss,
                              void *stream);
int lkg_relation_loss_bwd_f32(int64_t n, int32_t n_rel, int32_t k, float *u, int64_t ldu, int64_t rel_stride,
                              const float *e, int64_t lde, const int64_t *truth, float scale, const float *g,
                              const float *z, int64_t ldz, float *gd, int64_t ldgd, float *c, int64_t ldc,
                              void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_RELATION_TRAIN_H */
