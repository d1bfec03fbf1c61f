// The scoring arithmetic shared by filtered ranking (lkg_rank.hip) and filtered top-k selection (lkg_topk.hip).  Both
// must produce the same bits for a (query, candidate) pair: the exact f32 MFMA v_mfma_f32_16x16x4_f32, the same
// lane -> k map, zero padding past k and the same final fma.
//
// k order (load4 / mfma_chunk): k is taken in chunks of 16; lane l holds elements 4(l>>4) .. 4(l>>4)+3 of the chunk for
// row l & 15; MFMA j of the chunk feeds element j, so the chain runs 0,4,8,12, 1,5,9,13, ... of each chunk.
// Elements past k are zero (x + 0 * 0 = x).
#pragma once
#include "lkg_common.h"

#include <type_traits>

using f32x4 = __attribute__((ext_vector_type(4))) float;

// host side: may the kernels be launched with VEC (16-byte loads of both operands' rows)?
static inline bool vec_ok(const void *a, long lda, const void *b, long ldb) {
    return lkg_aligned16(a) && lkg_aligned16(b) && lda % 4 == 0 && ldb % 4 == 0;
}

// host side: the one way to launch a VEC-templated kernel.  `launch` holds the launch statement, written once with
// kernel<decltype(vec)::value, ...>; it is called with std::true_type (16-byte loads) or std::false_type.
template <class Launch>
static inline void vec_dispatch(bool vec, Launch &&launch) {
    if (vec) launch(std::true_type{});
    else launch(std::false_type{});
}

template <bool VEC>
__device__ __forceinline__ float4 load4(const float *__restrict__ row, int kk, int k) {
    if (VEC && kk + 4 <= k) return *reinterpret_cast<const float4 *>(row + kk);
    float4 v;
    v.x = kk < k ? row[kk] : 0.f;
    v.y = kk + 1 < k ? row[kk + 1] : 0.f;
    v.z = kk + 2 < k ? row[kk + 2] : 0.f;
    v.w = kk + 3 < k ? row[kk + 3] : 0.f;
    return v;
}

__device__ __forceinline__ void mfma_chunk(f32x4 &acc, const float4 &a, const float4 &b) {
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.x, b.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.y, b.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.z, b.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.w, b.w, acc, 0, 0, 0);
}

// the score derived from a dot product (one rounding); pn NULL = dot scoring (s = -2 q.p)
__device__ __forceinline__ float rank_score(float dot, const float *__restrict__ pn, long c) {
    return __builtin_fmaf(-2.f, dot, pn ? pn[c] : 0.f);
}

// "Score these pairs with the counting arithmetic": lanes 0..15 return s(q, p[cand of lane]) -- every row of the A
// operand is q, column r of B is the candidate of lane r (lanes >= 16 feed the same candidates: the B map is r = l & 15).
// (lkg_rank.hip's prepare kernel and lkg_softmax.hip's finish kernel score the truth with it.)
template <bool VEC>
__device__ __forceinline__ float rank_pair_scores(const float *__restrict__ qrow, const float *__restrict__ p, long ldp,
                                                  const float *__restrict__ pn, long cand, int k) {
    const int s = (threadIdx.x & 63) >> 4;
    const float *prow = p + cand * ldp;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < k; k0 += 16) {
        const float4 a = load4<VEC>(qrow, k0 + 4 * s, k);
        const float4 b = load4<VEC>(prow, k0 + 4 * s, k);
        mfma_chunk(acc, a, b);
    }
    return rank_score(acc[0], pn, cand);     // C[4 s + 0][r]: the same value on every s
}

// The four operand rows lane r feeds to rank_tile_dots: rows first + 16 i + r of x, clamped to the last of the n rows (a
// tile may hang over the end: what a clamped row produces is never stored or counted).  For the kernels of one tile per
// workgroup; the kernels that walk a range of tiles keep the statement inline: through this helper their register
// allocation, though not their arithmetic, would change (profiles/all_entity_tile_merge.txt).
__device__ __forceinline__ void tile_rows(const float *(&row)[4], const float *__restrict__ x, long ldx, long first, long n,
                                          int r) {
#pragma unroll
    for (int i = 0; i < 4; ++i) row[i] = x + min(first + 16 * i + r, n - 1) * ldx;
}

// One wave's 64 x 64 block of dot products: acc[i][j][v] = q_(16 i + 4 s + v) . p_(16 j + r) for lane (r, s) = (l & 15,
// l >> 4), qrow[i] / prow[i] the rows that lane feeds (16 i + r).  The next k-chunk is in flight while this one runs on
// the matrix pipe.  (rank_count_kernel keeps the same loop inline: through this helper its register allocation, though
// not its arithmetic, would change.)
template <bool VEC>
__device__ __forceinline__ void rank_tile_dots(f32x4 (&acc)[4][4], const float *const (&qrow)[4],
                                               const float *const (&prow)[4], int k, int s) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    float4 a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        a[i] = load4<VEC>(qrow[i], 4 * s, k);
        b[i] = load4<VEC>(prow[i], 4 * s, k);
    }
    for (int k0 = 0; k0 < k; k0 += 16) {
        float4 an[4], bn[4];
        const int kn = k0 + 16 + 4 * s;
        const bool more = k0 + 16 < k;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            an[i] = more ? load4<VEC>(qrow[i], kn, k) : f4_zero();
            bn[i] = more ? load4<VEC>(prow[i], kn, k) : f4_zero();
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) mfma_chunk(acc[i][j], a[i], b[j]);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            a[i] = an[i];
            b[i] = bn[i];
        }
    }
}
