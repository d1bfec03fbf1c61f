// Self-adversarial negative-sampling loss on grouped rows (literalkg_amd/self_adversarial.py): G groups, each an anchor
// query row q_g, a positive row p_g and K negative rows n_gj (row g K + j of n).  With the logits
//     z+ = scale (margin - ||q - p||^2),   z_j = scale (margin - ||q - n_j||^2)      (dot: scale (margin + q . x))
// the weights  w_j = softmax_j(temperature z_j)  over the group's K negatives (constants: nothing flows through them) and
//     L_g = softplus(-z+) + sum_j w_j softplus(z_j).
// DESIGN.md 3.6p.
//
// Tiling: one 256-thread workgroup per group.  A lane owns the 4-column units lane, lane + 64, ... of a row (one 16-byte
// load each where k, the strides and the pointers allow it; four guarded scalar loads otherwise, into the SAME lane and
// the SAME order: the two paths give the same bits, so the choice between them never shows in a result).  Each wave reads
// the group's q row once and keeps it in registers (the first 512 columns; a wider row's remaining units are re-read
// through the cache); the group's K + 1 rows -- row 0 the positive -- go to the four waves in turn, each row gathered once.
//
// Forward: a row's squared distance is summed directly, sum (q - x)^2 with one fma per column in the lane's unit order,
// then one butterfly over the wave; z = fl(scale * fl(margin -+ s)).  After a workgroup barrier wave 0 reads the group's
// logits back and finishes: m = max_j t z_j, e_j = expf(t z_j - m), w_j = e_j / sum_j e_j (any K: the lanes loop), and
// the loss, every softplus as max(x, 0) + log1pf(expf(-|x|)).  t == 0 gives e_j = 1 and w_j = fl(1 / K).
//
// Backward: dL/dz+ = -sigma(-z+), dL/dz_j = w_j sigma(z_j) from the kept z and w (sigma on the side that does not
// cancel); c_x = cs g (dL/dz_x) with cs = 2 scale (dot: scale).  Distance: dp = c_0 (q - p), dn_j = c_j (q - n_j),
// dq = -sum_x c_x (q - x); dot: dx = c_x q, dq = sum_x c_x x.  Per 512-column tile a lane keeps q and the running dq of
// its columns in registers; a wave adds its rows in increasing order, the four waves meet in LDS and wave 0 adds them
// in wave order.  Every element of dq, dp and dn is stored once by plain stores; an output whose pointer is NULL is not
// computed, and the others keep their bits.  No atomics; a group's outputs depend on its own rows alone.
// Floating-point contraction is off in this file: every rounding is one the references count.
#include "lkg_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int NS_THREADS = 256;
constexpr int NS_WAVES = 4;
constexpr int NS_RU = 2;              // 4-column units of a row a lane keeps in registers (2 x 64 x 4 = 512 columns)

// softplus(x) without cancellation
__device__ __forceinline__ float nssa_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// sigma(x) on the side that does not cancel: 1 / (1 + e^-x) for x >= 0, e^x / (1 + e^x) below
__device__ __forceinline__ float nssa_sigmoid(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

// columns 4 u .. 4 u + 3 of a row (zeros past k)
template <bool VEC>
__device__ __forceinline__ float4 load_unit(const float *__restrict__ row, int u, int k) {
    if constexpr (VEC) {
        return reinterpret_cast<const float4 *>(row)[u];
    } else {
        const int c = 4 * u;
        float4 v;
        v.x = c < k ? row[c] : 0.f;
        v.y = c + 1 < k ? row[c + 1] : 0.f;
        v.z = c + 2 < k ? row[c + 2] : 0.f;
        v.w = c + 3 < k ? row[c + 3] : 0.f;
        return v;
    }
}

template <bool VEC>
__device__ __forceinline__ void store_unit(float *__restrict__ row, int u, int k, const float4 &v) {
    if constexpr (VEC) {
        reinterpret_cast<float4 *>(row)[u] = v;
    } else {
        const int c = 4 * u;
        if (c < k) row[c] = v.x;
        if (c + 1 < k) row[c + 1] = v.y;
        if (c + 2 < k) row[c + 2] = v.z;
        if (c + 3 < k) row[c + 3] = v.w;
    }
}

template <bool DOT>
__device__ __forceinline__ void score_unit(float &s, const float4 &a, const float4 &v) {
    if constexpr (DOT) {
        s = fmaf(a.x, v.x, s);
        s = fmaf(a.y, v.y, s);
        s = fmaf(a.z, v.z, s);
        s = fmaf(a.w, v.w, s);
    } else {
        const float dx = a.x - v.x, dy = a.y - v.y, dz = a.z - v.z, dw = a.w - v.w;
        s = fmaf(dx, dx, s);
        s = fmaf(dy, dy, s);
        s = fmaf(dz, dz, s);
        s = fmaf(dw, dw, s);
    }
}

template <bool VEC, bool DOT>
__global__ __launch_bounds__(NS_THREADS) void nssa_fwd_kernel(long n_neg, int k, const float *__restrict__ q, long ldq,
                                                               const float *__restrict__ p, long ldp,
                                                               const float *__restrict__ n, long ldn, float margin,
                                                               float scale, float temp, float *z_pos, float *z_neg,
                                                               float *__restrict__ w, float *__restrict__ loss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long g = blockIdx.x;
    const int nu = (k + 3) >> 2;
    const float *qrow = q + g * ldq;
    float4 qv[NS_RU];
#pragma unroll
    for (int i = 0; i < NS_RU; ++i) {
        const int u = lane + 64 * i;
        qv[i] = u < nu ? load_unit<VEC>(qrow, u, k) : f4_zero();
    }
    float *zn = z_neg + g * n_neg;
    for (long i = wave; i <= n_neg; i += NS_WAVES) {         // row 0: the positive; row i: negative i - 1
        const float *x = i == 0 ? p + g * ldp : n + (g * n_neg + (i - 1)) * ldn;
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < NS_RU; ++j) {
            const int u = lane + 64 * j;
            if (u < nu) score_unit<DOT>(s, qv[j], load_unit<VEC>(x, u, k));
        }
        for (int u = lane + 64 * NS_RU; u < nu; u += 64)     // (a row wider than 512 columns)
            score_unit<DOT>(s, load_unit<VEC>(qrow, u, k), load_unit<VEC>(x, u, k));
        s = wave_sum(s);
        const float z = scale * (DOT ? margin + s : margin - s);
        if (lane == 0) {
            if (i == 0) z_pos[g] = z;
            else zn[i - 1] = z;
        }
    }
    __syncthreads();                                         // the group's logits are in memory, visible to the workgroup
    if (wave != 0) return;
    float m = -__builtin_inff();
    for (long j = lane; j < n_neg; j += 64) m = fmaxf(m, temp * zn[j]);
    m = wave_max(m);
    float sum = 0.f;
    for (long j = lane; j < n_neg; j += 64) sum += expf(temp * zn[j] - m);
    sum = wave_sum(sum);
    float acc = 0.f;
    float *wg = w + g * n_neg;
    for (long j = lane; j < n_neg; j += 64) {
        const float zj = zn[j];
        const float wj = expf(temp * zj - m) / sum;
        wg[j] = wj;
        acc += wj * nssa_softplus(zj);
    }
    acc = wave_sum(acc);
    if (lane == 0) loss[g] = nssa_softplus(-z_pos[g]) + acc;
}

template <bool VEC, bool DOT>
__global__ __launch_bounds__(NS_THREADS) void nssa_bwd_kernel(long n_neg, int k, const float *__restrict__ q, long ldq,
                                                               const float *__restrict__ p, long ldp,
                                                               const float *__restrict__ n, long ldn, float scale,
                                                               const float *__restrict__ g_up,
                                                               const float *__restrict__ z_pos,
                                                               const float *__restrict__ z_neg,
                                                               const float *__restrict__ w, float *__restrict__ dq,
                                                               long lddq, float *__restrict__ dp, long lddp,
                                                               float *__restrict__ dn, long lddn) {
    __shared__ float4 red[NS_WAVES - 1][NS_RU][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long g = blockIdx.x;
    const int nu = (k + 3) >> 2;
    const float gu = g_up[g];
    const float cs = DOT ? scale : 2.f * scale;
    const float *qrow = q + g * ldq;
    const long first = (dq || dp) ? 0 : 1;                   // the positive's row is read for dq and dp only
    const long last = (dq || dn) ? n_neg : 0;                // the negatives' rows for dq and dn only
    for (int u0 = 0; u0 < nu; u0 += 64 * NS_RU) {
        float4 qv[NS_RU], sum[NS_RU];
#pragma unroll
        for (int j = 0; j < NS_RU; ++j) {
            const int u = u0 + lane + 64 * j;
            qv[j] = u < nu ? load_unit<VEC>(qrow, u, k) : f4_zero();
            sum[j] = f4_zero();
        }
#pragma unroll 2
        for (long i = wave; i <= last; i += NS_WAVES) {
            if (i < first) continue;
            float c;
            const float *x;
            float *dx;
            if (i == 0) {
                c = cs * (gu * -nssa_sigmoid(-z_pos[g]));
                x = p + g * ldp;
                dx = dp ? dp + g * lddp : nullptr;
            } else {
                const long t = g * n_neg + (i - 1);
                c = cs * (gu * (w[t] * nssa_sigmoid(z_neg[t])));
                x = n + t * ldn;
                dx = dn ? dn + t * lddn : nullptr;
            }
#pragma unroll
            for (int j = 0; j < NS_RU; ++j) {
                const int u = u0 + lane + 64 * j;
                if (u < nu) {
                    const float4 v = load_unit<VEC>(x, u, k);
                    float4 o;                                // the row's own gradient
                    if constexpr (DOT) {
                        o = make_float4(c * qv[j].x, c * qv[j].y, c * qv[j].z, c * qv[j].w);
                        sum[j].x += c * v.x;
                        sum[j].y += c * v.y;
                        sum[j].z += c * v.z;
                        sum[j].w += c * v.w;
                    } else {
                        o = make_float4(c * (qv[j].x - v.x), c * (qv[j].y - v.y), c * (qv[j].z - v.z),
                                        c * (qv[j].w - v.w));
                        sum[j].x += o.x;
                        sum[j].y += o.y;
                        sum[j].z += o.z;
                        sum[j].w += o.w;
                    }
                    if (dx) store_unit<VEC>(dx, u, k, o);
                }
            }
        }
        if (dq) {                                            // (uniform) the waves meet in wave order
            if (wave)
#pragma unroll
                for (int j = 0; j < NS_RU; ++j) red[wave - 1][j][lane] = sum[j];
            __syncthreads();
            if (wave == 0) {
#pragma unroll
                for (int j = 0; j < NS_RU; ++j) {
                    const int u = u0 + lane + 64 * j;
                    if (u < nu) {
                        const float4 a = red[0][j][lane], b = red[1][j][lane], d = red[2][j][lane];
                        float4 t = make_float4(((sum[j].x + a.x) + b.x) + d.x, ((sum[j].y + a.y) + b.y) + d.y,
                                               ((sum[j].z + a.z) + b.z) + d.z, ((sum[j].w + a.w) + b.w) + d.w);
                        if constexpr (!DOT) t = make_float4(-t.x, -t.y, -t.z, -t.w);
                        store_unit<VEC>(dq + g * lddq, u, k, t);
                    }
                }
            }
            __syncthreads();
        }
    }
}

bool vec4_ok(int k, const void *ptr, int64_t ld) { return !ptr || (k % 4 == 0 && ld % 4 == 0 && lkg_aligned16(ptr)); }

}  // namespace

extern "C" int lkg_nssa_fwd_f32(int64_t n_groups, int64_t n_neg, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *n, int64_t ldn, int32_t distance, float margin, float scale,
                                float temperature, float *z_pos, float *z_neg, float *w, float *loss, void *stream) {
    LKG_REQUIRE(n_groups >= 0 && n_groups < INT32_MAX && n_neg >= 1 && n_neg < INT32_MAX && k > 0 && ldq >= k && ldp >= k &&
                    ldn >= k && margin == margin && margin - margin == 0.f,
                "lkg_nssa_fwd_f32: bad sizes");
    LKG_REQUIRE(scale > 0.f && scale < __builtin_inff(), "lkg_nssa_fwd_f32: scale must be positive and finite");
    LKG_REQUIRE(temperature >= 0.f && temperature < __builtin_inff(),
                "lkg_nssa_fwd_f32: temperature must not be negative (and finite)");
    if (n_groups == 0) return LKG_OK;
    LKG_REQUIRE(q && p && n && z_pos && z_neg && w && loss, "lkg_nssa_fwd_f32: null pointer");
    const dim3 grid((unsigned)n_groups), block(NS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec4_ok(k, q, ldq) && vec4_ok(k, p, ldp) && vec4_ok(k, n, ldn);
#define LKG_NSSA_FWD(V, D)                                                                                             \
    hipLaunchKernelGGL((nssa_fwd_kernel<V, D>), grid, block, 0, s, (long)n_neg, k, q, (long)ldq, p, (long)ldp, n,      \
                       (long)ldn, margin, scale, temperature, z_pos, z_neg, w, loss)
    if (vec) {
        if (distance) LKG_NSSA_FWD(true, false);
        else LKG_NSSA_FWD(true, true);
    } else {
        if (distance) LKG_NSSA_FWD(false, false);
        else LKG_NSSA_FWD(false, true);
    }
#undef LKG_NSSA_FWD
    LKG_CHECK_LAUNCH("lkg_nssa_fwd_f32");
    return LKG_OK;
}

extern "C" int lkg_nssa_bwd_f32(int64_t n_groups, int64_t n_neg, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *n, int64_t ldn, int32_t distance, float scale, const float *g,
                                const float *z_pos, const float *z_neg, const float *w, float *dq, int64_t lddq,
                                float *dp, int64_t lddp, float *dn, int64_t lddn, void *stream) {
    LKG_REQUIRE(n_groups >= 0 && n_groups < INT32_MAX && n_neg >= 1 && n_neg < INT32_MAX && k > 0 && ldq >= k && ldp >= k &&
                    ldn >= k && (!dq || lddq >= k) && (!dp || lddp >= k) && (!dn || lddn >= k),
                "lkg_nssa_bwd_f32: bad sizes");
    LKG_REQUIRE(scale > 0.f && scale < __builtin_inff(), "lkg_nssa_bwd_f32: scale must be positive and finite");
    if (n_groups == 0 || (!dq && !dp && !dn)) return LKG_OK;
    LKG_REQUIRE(q && p && n && g && z_pos && z_neg && w, "lkg_nssa_bwd_f32: null pointer");
    const dim3 grid((unsigned)n_groups), block(NS_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec4_ok(k, q, ldq) && vec4_ok(k, p, ldp) && vec4_ok(k, n, ldn) && vec4_ok(k, dq, lddq) &&
                     vec4_ok(k, dp, lddp) && vec4_ok(k, dn, lddn);
#define LKG_NSSA_BWD(V, D)                                                                                             \
    hipLaunchKernelGGL((nssa_bwd_kernel<V, D>), grid, block, 0, s, (long)n_neg, k, q, (long)ldq, p, (long)ldp, n,      \
                       (long)ldn, scale, g, z_pos, z_neg, w, dq, (long)lddq, dp, (long)lddp, dn, (long)lddn)
    if (vec) {
        if (distance) LKG_NSSA_BWD(true, false);
        else LKG_NSSA_BWD(true, true);
    } else {
        if (distance) LKG_NSSA_BWD(false, false);
        else LKG_NSSA_BWD(false, true);
    }
#undef LKG_NSSA_BWD
    LKG_CHECK_LAUNCH("lkg_nssa_bwd_f32");
    return LKG_OK;
}

int lkg_internal_preload_nssa() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&nssa_fwd_kernel<true, false>)) == hipSuccess ? 0 : 1;
}
