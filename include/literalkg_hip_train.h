/*
 * literalkg_hip_train.h -- training objectives on sampled rows of the MI355X (gfx950) LiteralKG library, under the
 * conventions of literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no allocation, 0 on success
 * and a negative lkg_status with lkg_last_error() otherwise, "ld*" in elements).  literalkg_amd/_native.py binds them from
 * its third table, TRAIN_PROTOTYPES.
 */
#ifndef LITERALKG_HIP_TRAIN_H
#define LITERALKG_HIP_TRAIN_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Self-adversarial negative-sampling loss on grouped rows (lkg_nssa.hip; literalkg_amd/self_adversarial.py).  n_groups
 * groups; group g has the anchor row q[g * ldq ..], the positive row p[g * ldp ..] and the n_neg >= 1 negative rows
 * n[(g * n_neg + j) * ldn ..], all of k float32 columns with free row strides.  With s(x) = sum_c (q_c - x_c)^2 summed
 * directly (distance != 0) or s(x) = sum_c q_c x_c (distance == 0), the logit of a row is
 *     z(x) = fl(scale * fl(margin - s(x)))   (distance)        z(x) = fl(scale * fl(margin + s(x)))   (dot),
 * scale > 0 and finite, margin finite.  The weights are  w_j = e_j / sum_j e_j,  e_j = exp(temperature z_j - max_j
 * temperature z_j),  temperature >= 0 and finite (0: every w_j = fl(1 / n_neg)); they are constants of the loss
 *     loss_g = softplus(-z+) + sum_j w_j softplus(z_j),
 * every softplus evaluated as max(x, 0) + log1p(exp(-|x|)).
 *
 * lkg_nssa_fwd_f32: z_pos[n_groups], z_neg[n_groups * n_neg], w[n_groups * n_neg] and loss[n_groups], each written once.
 * lkg_nssa_bwd_f32: from the upstream g[n_groups] and the kept z_pos, z_neg, w, with a_0 = -g sigma(-z+),
 *     a_j = g w_j sigma(z_j) (sigma on the side that does not cancel) and c_x = (distance ? 2 scale : scale) a_x:
 *         distance:  dp = c_0 (q - p),   dn_j = c_j (q - n_j),   dq = -sum_x c_x (q - x)
 *         dot:       dp = c_0 q,         dn_j = c_j q,           dq = sum_x c_x x
 *     into dq[g * lddq ..], dp[g * lddp ..], dn[(g * n_neg + j) * lddn ..], every element stored once.  dq, dp or dn may
 *     be NULL: that output is not computed, the others keep their bits.
 * A group's outputs depend on its own rows alone (not on n_groups, its position or other groups), the sums run in a fixed
 * order and there are no atomics: every output repeats bit for bit, and the 16-byte and the scalar load path give the
 * same bits.  n_groups == 0 launches nothing; addressing is 64-bit.                                                    */
int lkg_nssa_fwd_f32(int64_t n_groups, int64_t n_neg, int32_t k, const float *q, int64_t ldq, const float *p,
                     int64_t ldp, const float *n, int64_t ldn, int32_t distance, float margin, float scale,
                     float temperature, float *z_pos, float *z_neg, float *w, float *loss, void *stream);
int lkg_nssa_bwd_f32(int64_t n_groups, int64_t n_neg, int32_t k, const float *q, int64_t ldq, const float *p,
                     int64_t ldp, const float *n, int64_t ldn, int32_t distance, float scale, const float *g,
                     const float *z_pos, const float *z_neg, const float *w, float *dq, int64_t lddq, float *dp,
                     int64_t lddp, float *dn, int64_t lddn, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_TRAIN_H */
