/*
 * literalkg_hip_gemm_ordered.h -- the ordered split-K GEMM of the MI355X (gfx950) LiteralKG library, under the conventions
 * of literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no allocation, 0 on success and a
 * negative lkg_status with lkg_last_error() otherwise, "ld*" in elements).  literalkg_amd/_native.py binds them from its
 * sixth table, ORDERED_GEMM_PROTOTYPES.
 */
#ifndef LITERALKG_HIP_GEMM_ORDERED_H
#define LITERALKG_HIP_GEMM_ORDERED_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* C = alpha * op(A) op(B) + beta * C (+ bias[n]) in float32 for products with a SMALL output and a LONG reduction
 * (lkg_gemm_ordered.hip; literalkg_amd/gemm_ordered.py): the reduction is spread over the chip as lkg_gemm_f32's atomic
 * split does, but the pieces are added in a fixed order, so every output repeats bit for bit.  op(A) is m x k (A stored
 * k x m with trans_a), op(B) is k x n (B stored n x k with trans_b), row-major with free row strides; ldc >= n.
 *
 * The partition.  For `splits` = S in [1, 256]:
 *     per   = 16 * ceil(ceil(k / S) / 16)          (0 for k == 0)
 *     S_eff = ceil(k / per)                        (0 for k == 0; at most min(S, ceil(k / 16)))
 * and split z in [0, S_eff) covers k in [z * per, min(k, (z + 1) * per)): every boundary but the last is a multiple of
 * 16.  lkg_gemm_ordered_partition returns S_eff and stores per (per may be NULL); a negative lkg_status on bad arguments.
 *
 * The arithmetic.  A first launch of (output tiles) x S_eff workgroups computes, per element and split, the partial
 *     p_z = the k-ordered fmaf chain of the exact f32-input MFMA (v_mfma_f32_32x32x2_f32) over the split's k, from 0.0,
 *           one rounding per product -- the bits an UNSPLIT call over the k-slice alone produces with alpha = 1, beta = 0,
 * and stores it with plain vector stores into workspace[z][m][n] (float32, contiguous).  A second launch forms
 *     s   = ((p_0 + p_1) + p_2) + ...               float32 adds in ascending z
 *     t   = fmaf(alpha, s, bias[j])                 (bias NULL: 0.0f)
 *     out = beta == 0 ? t : fmaf(beta, C_old, t)    (C is not read when beta == 0)
 * With S_eff == 1 the first launch applies the last two lines to s = p_0 itself: no workspace, no second launch.  k == 0
 * gives s = 0.0, that is beta * C + bias.  There are no atomics, no counters and no in-launch combine.
 *
 * The property.  An output element is a function of its row of op(A), its column of op(B), k, per, alpha, beta, its old C
 * and its bias -- not of m, n, other rows or columns, alignment, strides, the stream, the workspace's previous contents
 * or the run.  The 16-byte load path and the clamped scalar one (edge tiles; an operand whose address is not a multiple of
 * 16 bytes or whose row stride is not a multiple of 4 elements) give the same bits.
 *
 * lkg_gemm_ordered_splits: the default S, a pure function of its five arguments (no device query, no environment):
 *     tiles = ceil(m / 128) * ceil(n / 128)
 *     S     = max(1, min(512 / tiles, k / 512, 2^26 / (m * n), 256))          (integer divisions)
 * about two workgroups per CU of a 256-CU device, no split shorter than 512 k, partials within 256 MB.
 * lkg_gemm_ordered_workspace: the bytes lkg_gemm_ordered_f32 needs for (m, n, k, splits): S_eff * m * n * 4, 0 for
 * S_eff <= 1; a negative lkg_status on bad arguments.
 * lkg_gemm_ordered_f32: splits outside [1, 256], a workspace shorter than that, a leading dimension smaller than the
 * stored row or a null operand is LKG_ERR_INVALID_ARG before any launch.  m == 0 or n == 0 launches nothing.               */
int32_t lkg_gemm_ordered_splits(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k);
int64_t lkg_gemm_ordered_partition(int64_t k, int32_t splits, int64_t *per);
int64_t lkg_gemm_ordered_workspace(int64_t m, int64_t n, int64_t k, int32_t splits);
int lkg_gemm_ordered_f32(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, int32_t splits, float alpha,
                         const float *a, int64_t lda, const float *b, int64_t ldb, float beta, float *c, int64_t ldc,
                         const float *bias, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_GEMM_ORDERED_H */
