// K5 row-wise epilogue of an aggregation layer (LeakyReLU -> LayerNorm -> L2-normalised copy,
// model.py:111/161/305) and K6 literal-gate blend (gate.py:24-26), forward and backward.
// All HBM-bound: each row is read once into registers (one wave per row, 16 bytes per lane per chunk),
// every statistic is a wave xor-shuffle reduction, every output is written once.
#include <algorithm>
#include <cmath>
#include <cstdlib>

#include "lkg_common.h"

namespace {

// A row of d floats spread over one wave: lane l holds elements [(l + 64*i)*W, +W) for i < CPL.
template <int W, int CPL>
struct RowRegs {
    float v[CPL * W];
    __device__ __forceinline__ void load(const float *p, int d, int lane, float fill = 0.f) {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int e = (lane + 64 * i) * W;
            if constexpr (W == 4) {
                if (e < d) {
                    const float4 t = *reinterpret_cast<const float4 *>(p + e);
                    v[i * 4 + 0] = t.x;
                    v[i * 4 + 1] = t.y;
                    v[i * 4 + 2] = t.z;
                    v[i * 4 + 3] = t.w;
                } else {
                    v[i * 4 + 0] = v[i * 4 + 1] = v[i * 4 + 2] = v[i * 4 + 3] = fill;
                }
            } else {
                v[i] = e < d ? p[e] : fill;
            }
        }
    }
    __device__ __forceinline__ void store(float *p, int d, int lane) const {
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int e = (lane + 64 * i) * W;
            if (e < d) {
                if constexpr (W == 4)
                    *reinterpret_cast<float4 *>(p + e) = make_float4(v[i * 4], v[i * 4 + 1], v[i * 4 + 2], v[i * 4 + 3]);
                else
                    p[e] = v[i];
            }
        }
    }
    __device__ __forceinline__ bool live(int k, int d, int lane) const { return (lane + 64 * (k / W)) * W + (k % W) < d; }
};

// (the counter-based dropout mask -- fmix32 / drop_row_key / drop_scale -- lives in lkg_common.h: the fused layer epilogue of
// lkg_gemm_tall.hip draws the same mask)
template <int W, int CPL>
__global__ __launch_bounds__(256) void act_ln_fwd_kernel(long n, int d, const float *__restrict__ z, long ldz,
                                                          float slope, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float eps,
                                                          float *__restrict__ y, long ldy, float *__restrict__ yn,
                                                          long ldyn, float norm_eps, float *__restrict__ save_mean,
                                                          float *__restrict__ save_rstd, float drop_p,
                                                          unsigned long long seed) {
    constexpr int K = CPL * W;
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    RowRegs<W, CPL> a, g, b;
    a.load(z + row * ldz, d, lane);
    g.load(gamma, d, lane);
    b.load(beta, d, lane);
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float t = a.v[k];
        a.v[k] = t > 0.f ? t : t * slope;
        s += a.live(k, d, lane) ? a.v[k] : 0.f;
    }
    const float mean = wave_sum(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float c = a.live(k, d, lane) ? a.v[k] - mean : 0.f;
        q = fmaf(c, c, q);
    }
    const float rstd = 1.f / sqrtf(wave_sum(q) / (float)d + eps);
    float nn = 0.f;
    const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    const unsigned rkey = drop_row_key(seed, (unsigned long long)row);
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float o = (a.v[k] - mean) * rstd * g.v[k] + b.v[k];
        if (drop_p > 0.f) {
            const int e = (lane + 64 * (k / W)) * W + (k % W);
            o *= drop_scale(rkey, (unsigned)e, drop_p, inv_keep);
        }
        a.v[k] = o;
        nn += a.live(k, d, lane) ? o * o : 0.f;
    }
    if (y) a.store(y + row * ldy, d, lane);       // (nobody reads the LAST layer's y: only its normalised copy is kept)
    if (lane == 0) {
        save_mean[row] = mean;
        save_rstd[row] = rstd;
    }
    if (yn) {
        const float inv = 1.f / fmaxf(sqrtf(wave_sum(nn)), norm_eps);
#pragma unroll
        for (int k = 0; k < K; ++k) a.v[k] *= inv;
        a.store(yn + row * ldyn, d, lane);
    }
}

// Narrow rows (d <= 128 floats, 16-byte path): a whole wave per row would leave half (d = 128) to seven eighths (d = 32)
// of its lanes idle -- here LPR = 32 / 16 / 8 lanes hold a row and a wave carries 64 / LPR rows, the statistics are
// reductions inside the LPR-lane group.  Bit-identical to act_ln_fwd_kernel<4, 1> (whose idle lanes add exact zeros
// in the last butterfly steps).
template <int LPR>
__global__ __launch_bounds__(256) void act_ln_fwd_narrow_kernel(long n, int d, const float *__restrict__ z, long ldz,
                                                                 float slope, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float eps,
                                                                 float *__restrict__ y, long ldy, float *__restrict__ yn,
                                                                 long ldyn, float norm_eps, float *__restrict__ save_mean,
                                                                 float *__restrict__ save_rstd, float drop_p,
                                                                 unsigned long long seed) {
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, sl = lane % LPR;
    const long row_raw = ((long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) * RPW + lane / LPR;
    const bool valid = row_raw < n;                // (rows past the end are computed on a copy of the last row, never stored:
    const long row = valid ? row_raw : n - 1;      //  the group reductions want every lane of the wave active)
    const int e = sl * 4;
    const bool live = e < d;
    float a[4], g[4], b[4];
    {   // branch-free: lanes past the row's width load its first chunk (in bounds) and drop it
        const int ec = live ? e : 0;
        const float4 t = *reinterpret_cast<const float4 *>(z + row * ldz + ec);
        const float4 gg = *reinterpret_cast<const float4 *>(gamma + ec);
        const float4 bb = *reinterpret_cast<const float4 *>(beta + ec);
        a[0] = live ? t.x : 0.f; a[1] = live ? t.y : 0.f; a[2] = live ? t.z : 0.f; a[3] = live ? t.w : 0.f;
        g[0] = gg.x; g[1] = gg.y; g[2] = gg.z; g[3] = gg.w;
        b[0] = bb.x; b[1] = bb.y; b[2] = bb.z; b[3] = bb.w;
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float t = a[k];
        a[k] = t > 0.f ? t : t * slope;
        s += live ? a[k] : 0.f;
    }
    const float mean = group_sum<LPR>(s) / (float)d;
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float c = live ? a[k] - mean : 0.f;
        q = fmaf(c, c, q);
    }
    const float rstd = 1.f / sqrtf(group_sum<LPR>(q) / (float)d + eps);
    float nn = 0.f;
    const float inv_keep = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
    const unsigned rkey = drop_row_key(seed, (unsigned long long)row);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float o = (a[k] - mean) * rstd * g[k] + b[k];
        if (drop_p > 0.f) o *= drop_scale(rkey, (unsigned)(e + k), drop_p, inv_keep);
        a[k] = o;
        nn += live ? o * o : 0.f;
    }
    if (y && valid && live) *reinterpret_cast<float4 *>(y + row * ldy + e) = make_float4(a[0], a[1], a[2], a[3]);
    if (sl == 0 && valid) {
        save_mean[row] = mean;
        save_rstd[row] = rstd;
    }
    if (yn) {
        const float inv = 1.f / fmaxf(sqrtf(group_sum<LPR>(nn)), norm_eps);
        if (valid && live)
            *reinterpret_cast<float4 *>(yn + row * ldyn + e) = make_float4(a[0] * inv, a[1] * inv, a[2] * inv, a[3] * inv);
    }
}

// Backward.  With a = leaky(z), xh = (a - mean) * rstd, y = xh * gamma + beta, yn = y / max(|y|, e):
//   G   = g_y + (g_yn - yn * <yn, g_yn>) / max(|y|, e)      (second term only when |y| > e; else g_yn / e)
//   dxh = G * gamma ;  da = rstd * (dxh - mean(dxh) - xh * mean(dxh * xh)) ;  dz = da * leaky'(z)
//   g_gamma += sum_rows G * xh ;  g_beta += sum_rows G
template <int W, int CPL>
__global__ __launch_bounds__(256) void act_ln_bwd_kernel(long n, int d, const float *__restrict__ z, long ldz,
                                                          float slope, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta,
                                                          const float *__restrict__ y, long ldy,
                                                          const float *__restrict__ save_mean,
                                                          const float *__restrict__ save_rstd,
                                                          const float *__restrict__ g_y, long ldgy,
                                                          const float *__restrict__ g_yn, long ldgyn, float norm_eps,
                                                          float *__restrict__ g_z, long ldgz,
                                                          float *__restrict__ g_gamma, float *__restrict__ g_beta,
                                                          float drop_p, unsigned long long seed,
                                                          float *__restrict__ gz_rowmax,
                                                          const unsigned char *__restrict__ gyn_rows, int sparse_out,
                                                          const long *__restrict__ row_ids, long n_row_ids) {
    constexpr int K = CPL * W;
    __shared__ float red_g[3][K][64], red_b[3][K][64];
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
    RowRegs<W, CPL> gam;
    gam.load(gamma, d, lane);
    float acc_g[K], acc_b[K];
#pragma unroll
    for (int k = 0; k < K; ++k) acc_g[k] = acc_b[k] = 0.f;

    const long n_iter = row_ids ? n_row_ids : n;     // with a row list: only the listed rows (negative entries: padding)
    for (long it = wave; it < n_iter; it += nwaves) {
        const long row = row_ids ? row_ids[it] : it;
        if (row < 0) continue;
        RowRegs<W, CPL> zz, G, yy;
        const bool has_gyn = g_yn && (!gyn_rows || gyn_rows[row]);   // wave-uniform
        if (!g_y && !has_gyn) {   // no gradient reaches this row: g_z = 0, nothing to read or to add to g_gamma / g_beta
            if (sparse_out) continue;     // (g_z is a table kept all-zero outside the flagged rows: nothing to write either)
            zz.load(z, 0, lane);   // zeros
            zz.store(g_z + row * ldgz, d, lane);
            if (gz_rowmax && lane == 0) gz_rowmax[row] = 0.f;
            continue;
        }
        zz.load(z + row * ldz, d, lane);
        if (g_y)
            G.load(g_y + row * ldgy, d, lane);
        else
            G.load(z, 0, lane);   // zeros
        if (has_gyn) {
            RowRegs<W, CPL> gn;
            if (y) {
                yy.load(y + row * ldy, d, lane);
            } else {          // y was not kept (the last layer): the same arithmetic as the forward, for this row
                RowRegs<W, CPL> bb;
                bb.load(beta, d, lane);
                const float mean_ = save_mean[row], rstd_ = save_rstd[row];
                const float inv_keep_ = drop_p > 0.f ? 1.f / (1.f - drop_p) : 1.f;
                const unsigned rkey_ = drop_row_key(seed, (unsigned long long)row);
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float t_ = zz.v[k];
                    float o = ((t_ > 0.f ? t_ : t_ * slope) - mean_) * rstd_ * gam.v[k] + bb.v[k];
                    if (drop_p > 0.f) {
                        const int e = (lane + 64 * (k / W)) * W + (k % W);
                        o *= drop_scale(rkey_, (unsigned)e, drop_p, inv_keep_);
                    }
                    yy.v[k] = zz.live(k, d, lane) ? o : 0.f;
                }
            }
            gn.load(g_yn + row * ldgyn, d, lane);
            float n2 = 0.f, dt = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                n2 = fmaf(yy.v[k], yy.v[k], n2);
                dt = fmaf(yy.v[k], gn.v[k], dt);
            }
            const float nrm = sqrtf(wave_sum(n2));
            dt = wave_sum(dt);
            if (nrm > norm_eps) {
                const float inv = 1.f / nrm;
                const float proj = dt * inv * inv * inv;   // <y,g>/|y|^3
#pragma unroll
                for (int k = 0; k < K; ++k) G.v[k] += gn.v[k] * inv - yy.v[k] * proj;
            } else {
                const float inv = 1.f / norm_eps;
#pragma unroll
                for (int k = 0; k < K; ++k) G.v[k] += gn.v[k] * inv;
            }
        }
        if (drop_p > 0.f) {   // y (and g_y / g_yn) refer to the masked output: route G through the mask
            const float inv_keep = 1.f / (1.f - drop_p);
            const unsigned rkey = drop_row_key(seed, (unsigned long long)row);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const int e = (lane + 64 * (k / W)) * W + (k % W);
                G.v[k] *= drop_scale(rkey, (unsigned)e, drop_p, inv_keep);
            }
        }
        const float mean = save_mean[row], rstd = save_rstd[row];
        float s1 = 0.f, s2 = 0.f;
        float xh[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float t = zz.v[k];
            const float a = t > 0.f ? t : t * slope;
            const bool lv = zz.live(k, d, lane);
            xh[k] = lv ? (a - mean) * rstd : 0.f;
            const float dx = G.v[k] * gam.v[k];
            s1 += dx;
            s2 = fmaf(dx, xh[k], s2);
            acc_g[k] = fmaf(G.v[k], xh[k], acc_g[k]);
            acc_b[k] += G.v[k];
        }
        s1 = wave_sum(s1) / (float)d;
        s2 = wave_sum(s2) / (float)d;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float dx = G.v[k] * gam.v[k];
            const float da = rstd * (dx - s1 - xh[k] * s2);
            zz.v[k] = da * (zz.v[k] > 0.f ? 1.f : slope);
        }
        zz.store(g_z + row * ldgz, d, lane);
        if (gz_rowmax) {      // max |g_z[row, :]|: the row scale of the data-gradient GEMM that consumes g_z (lkg_gemm_tall_f32)
            float mx = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) mx = fmaxf(mx, zz.live(k, d, lane) ? fabsf(zz.v[k]) : 0.f);
            mx = wave_max(mx);
            if (lane == 0) gz_rowmax[row] = mx;
        }
    }
    // the four waves of the workgroup meet in LDS first: one atomic per workgroup per column (every workgroup
    // hits the same 2*d addresses, and contended float atomics are an order of magnitude slower)
    const int w = threadIdx.x >> 6;
    if (w > 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            red_g[w - 1][k][lane] = acc_g[k];
            red_b[w - 1][k][lane] = acc_b[k];
        }
    }
    __syncthreads();
    if (w == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int e = (lane + 64 * (k / W)) * W + (k % W);
            if (e < d) {
                atomicAdd(g_gamma + e, acc_g[k] + red_g[0][k][lane] + red_g[1][k][lane] + red_g[2][k][lane]);
                atomicAdd(g_beta + e, acc_b[k] + red_b[0][k][lane] + red_b[1][k][lane] + red_b[2][k][lane]);
            }
        }
    }
}

// Backward over narrow rows (d <= 128 floats, 16-byte path, dense output: the layers BELOW the last one of a deep narrow
// model -- the reference's default is eight layers of 32): LPR = 32 / 16 / 8 lanes per row, 64 / LPR rows per wave, like
// act_ln_fwd_narrow_kernel.  Per-row conditions are per sub-group here, so every lane runs every reduction (the DPP
// butterflies need all lanes) on masked values and only the stores are predicated.  y is required when g_yn is given
// (the rows-only recompute of the last layer stays on act_ln_bwd_kernel).  Same arithmetic as act_ln_bwd_kernel<4, 1>;
// g_gamma / g_beta partial sums meet across sub-groups by shuffles, across waves in LDS, one atomic per workgroup.
template <int LPR>
__global__ __launch_bounds__(256) void act_ln_bwd_narrow_kernel(long n, int d, const float *__restrict__ z, long ldz,
                                                                 float slope, const float *__restrict__ gamma,
                                                                 const float *__restrict__ y, long ldy,
                                                                 const float *__restrict__ save_mean,
                                                                 const float *__restrict__ save_rstd,
                                                                 const float *__restrict__ g_y, long ldgy,
                                                                 const float *__restrict__ g_yn, long ldgyn, float norm_eps,
                                                                 float *__restrict__ g_z, long ldgz,
                                                                 float *__restrict__ g_gamma, float *__restrict__ g_beta,
                                                                 float drop_p, unsigned long long seed,
                                                                 float *__restrict__ gz_rowmax,
                                                                 const unsigned char *__restrict__ gyn_rows) {
    constexpr int RPW = 64 / LPR;
    __shared__ float red_g[3][4][LPR], red_b[3][4][LPR];
    const int lane = threadIdx.x & 63, sl = lane % LPR, sub = lane / LPR;
    const long wave = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const long nwaves = (long)gridDim.x * (blockDim.x >> 6);
    const int e = sl * 4;
    const bool live = e < d;
    const int ec = live ? e : 0;                 // (lanes past the width load the row's first chunk and drop it)
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float gam[4];
    {
        const float4 t = *reinterpret_cast<const float4 *>(gamma + ec);
        gam[0] = live ? t.x : 0.f; gam[1] = live ? t.y : 0.f; gam[2] = live ? t.z : 0.f; gam[3] = live ? t.w : 0.f;
    }
    float acc_g[4] = {0.f, 0.f, 0.f, 0.f}, acc_b[4] = {0.f, 0.f, 0.f, 0.f};
    const long n_groups = (n + RPW - 1) / RPW;
    for (long it = wave; it < n_groups; it += nwaves) {
        const long row_raw = it * RPW + sub;
        const bool valid = row_raw < n;
        const long row = valid ? row_raw : n - 1;
        const bool has_gyn = g_yn && (!gyn_rows || gyn_rows[row]);
        const bool any = valid && (g_y || has_gyn);          // does a gradient reach this row at all?
        auto ld4 = [&](const float *base, long ld, bool on, float (&v)[4]) {
            const float4 t = on ? *reinterpret_cast<const float4 *>(base + row * ld + ec) : zero4;
            v[0] = (on && live) ? t.x : 0.f; v[1] = (on && live) ? t.y : 0.f;
            v[2] = (on && live) ? t.z : 0.f; v[3] = (on && live) ? t.w : 0.f;
        };
        float zz[4], G[4];
        ld4(z, ldz, any, zz);
        ld4(g_y, ldgy, any && g_y != nullptr, G);
        {
            float yy[4], gn[4];
            ld4(y, ldy, any && has_gyn, yy);
            ld4(g_yn, ldgyn, any && has_gyn, gn);
            float n2 = 0.f, dt = 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                n2 = fmaf(yy[k], yy[k], n2);
                dt = fmaf(yy[k], gn[k], dt);
            }
            const float nrm = sqrtf(group_sum<LPR>(n2));
            dt = group_sum<LPR>(dt);
            if (nrm > norm_eps) {                 // (rows without g_yn: yy = gn = 0, nrm = 0: the else branch adds zeros)
                const float inv = 1.f / nrm;
                const float proj = dt * inv * inv * inv;
#pragma unroll
                for (int k = 0; k < 4; ++k) G[k] += gn[k] * inv - yy[k] * proj;
            } else {
                const float inv = 1.f / norm_eps;
#pragma unroll
                for (int k = 0; k < 4; ++k) G[k] += gn[k] * inv;
            }
        }
        if (drop_p > 0.f) {
            const float inv_keep = 1.f / (1.f - drop_p);
            const unsigned rkey = drop_row_key(seed, (unsigned long long)row);
#pragma unroll
            for (int k = 0; k < 4; ++k) G[k] *= drop_scale(rkey, (unsigned)(e + k), drop_p, inv_keep);
        }
        const float mean = save_mean[row], rstd = save_rstd[row];
        float s1 = 0.f, s2 = 0.f, xh[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = zz[k];
            const float a = t > 0.f ? t : t * slope;
            xh[k] = (any && live) ? (a - mean) * rstd : 0.f;
            const float dx = G[k] * gam[k];
            s1 += dx;
            s2 = fmaf(dx, xh[k], s2);
            acc_g[k] = fmaf(G[k], xh[k], acc_g[k]);
            acc_b[k] += G[k];
        }
        s1 = group_sum<LPR>(s1) / (float)d;
        s2 = group_sum<LPR>(s2) / (float)d;
        float mx = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float dx = G[k] * gam[k];
            const float da = rstd * (dx - s1 - xh[k] * s2);
            zz[k] = (any && live) ? da * (zz[k] > 0.f ? 1.f : slope) : 0.f;
            mx = fmaxf(mx, fabsf(zz[k]));
        }
        if (valid && live) *reinterpret_cast<float4 *>(g_z + row * ldgz + e) = make_float4(zz[0], zz[1], zz[2], zz[3]);
        if (gz_rowmax) {
            mx = group_max<LPR>(mx);
            if (valid && sl == 0) gz_rowmax[row] = mx;
        }
    }
    // columns e .. e+3 are held by lane sl of every sub-group: fold the sub-groups, then the waves, then one atomic each
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int m = LPR; m < 64; m <<= 1) {
            acc_g[k] += __shfl_xor(acc_g[k], m, 64);
            acc_b[k] += __shfl_xor(acc_b[k], m, 64);
        }
    const int w = threadIdx.x >> 6;
    if (w > 0 && sub == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            red_g[w - 1][k][sl] = acc_g[k];
            red_b[w - 1][k][sl] = acc_b[k];
        }
    }
    __syncthreads();
    if (w == 0 && sub == 0 && live) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            atomicAdd(g_gamma + e + k, acc_g[k] + red_g[0][k][sl] + red_g[1][k][sl] + red_g[2][k][sl]);
            atomicAdd(g_beta + e + k, acc_b[k] + red_b[0][k][sl] + red_b[1][k][sl] + red_b[2][k][sl]);
        }
    }
}

// Literal-gate blend: rows are walked by groups of TPR = 2^k threads (TPR * W >= d when possible), so the
// (row, column) of an element needs shifts only and every access is a 16-byte one when rows are aligned.
template <int W>
__global__ __launch_bounds__(256) void gate_blend_fwd_kernel(long n, int d, int log_tpr, const float *__restrict__ x,
                                                              long ldx, const float *__restrict__ gpre, long ldg,
                                                              const float *__restrict__ zpre, long ldz,
                                                              float *__restrict__ out, long ldo) {
    const int tpr = 1 << log_tpr, rpb = 256 >> log_tpr;
    const int c0 = (threadIdx.x & (tpr - 1)) * W;
    for (long r = (long)blockIdx.x * rpb + (threadIdx.x >> log_tpr); r < n; r += (long)gridDim.x * rpb)
        for (int c = c0; c < d; c += tpr * W) {
            float xv[W], gv[W], zv[W], ov[W];
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(xv) = *reinterpret_cast<const float4 *>(x + r * ldx + c);
                *reinterpret_cast<float4 *>(gv) = *reinterpret_cast<const float4 *>(gpre + r * ldg + c);
                *reinterpret_cast<float4 *>(zv) = *reinterpret_cast<const float4 *>(zpre + r * ldz + c);
            } else {
                xv[0] = x[r * ldx + c];
                gv[0] = gpre[r * ldg + c];
                zv[0] = zpre[r * ldz + c];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float s = sigmoid_fast(zv[k]);
                ov[k] = (1.f - s) * xv[k] + s * tanh_fast(gv[k]);
            }
            if constexpr (W == 4)
                *reinterpret_cast<float4 *>(out + r * ldo + c) = *reinterpret_cast<float4 *>(ov);
            else
                out[r * ldo + c] = ov[0];
        }
}

template <int W>
__global__ __launch_bounds__(256) void gate_blend_bwd_kernel(long n, int d, int log_tpr, const float *__restrict__ x,
                                                              long ldx, const float *__restrict__ gpre, long ldg,
                                                              const float *__restrict__ zpre, long ldz,
                                                              const float *__restrict__ g_out, long ldgo,
                                                              float *__restrict__ g_x, long ldgx,
                                                              float *__restrict__ g_gpre, long ldgg,
                                                              float *__restrict__ g_zpre, long ldgz, int activated,
                                                              int *__restrict__ pre_rowmax) {
    const int tpr = 1 << log_tpr, rpb = 256 >> log_tpr;
    const int c0 = (threadIdx.x & (tpr - 1)) * W;
    for (long r = (long)blockIdx.x * rpb + (threadIdx.x >> log_tpr); r < n; r += (long)gridDim.x * rpb) {
        float rmax = 0.f;
        for (int c = c0; c < d; c += tpr * W) {
            float xv[W], gv[W], zv[W], go[W], ox[W], og[W], oz[W];
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(xv) = *reinterpret_cast<const float4 *>(x + r * ldx + c);
                *reinterpret_cast<float4 *>(gv) = *reinterpret_cast<const float4 *>(gpre + r * ldg + c);
                *reinterpret_cast<float4 *>(zv) = *reinterpret_cast<const float4 *>(zpre + r * ldz + c);
                *reinterpret_cast<float4 *>(go) = *reinterpret_cast<const float4 *>(g_out + r * ldgo + c);
            } else {
                xv[0] = x[r * ldx + c];
                gv[0] = gpre[r * ldg + c];
                zv[0] = zpre[r * ldz + c];
                go[0] = g_out[r * ldgo + c];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                // activated: gpre / zpre hold tanh(g) / sigmoid(z) as the fused gate epilogue kept them
                const float s = activated ? zv[k] : sigmoid_fast(zv[k]);
                const float tg = activated ? gv[k] : tanh_fast(gv[k]);
                ox[k] = go[k] * (1.f - s);
                og[k] = go[k] * s * (1.f - tg * tg);
                oz[k] = go[k] * (tg - xv[k]) * s * (1.f - s);
                rmax = fmaxf(rmax, fmaxf(fabsf(og[k]), fabsf(oz[k])));
            }
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(g_x + r * ldgx + c) = *reinterpret_cast<float4 *>(ox);
                *reinterpret_cast<float4 *>(g_gpre + r * ldgg + c) = *reinterpret_cast<float4 *>(og);
                *reinterpret_cast<float4 *>(g_zpre + r * ldgz + c) = *reinterpret_cast<float4 *>(oz);
            } else {
                g_x[r * ldgx + c] = ox[0];
                g_gpre[r * ldgg + c] = og[0];
                g_zpre[r * ldgz + c] = oz[0];
            }
        }
        if (pre_rowmax) {   // max |[g_gpre | g_zpre][r, :]|: the row scale of the data-gradient GEMM over the two (lkg_gemm_tall_f32)
            const int span = tpr < 64 ? tpr : 64;             // the row's threads inside this wave are consecutive lanes
            for (int m = 1; m < span; m <<= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, m, 64));
            if ((threadIdx.x & (span - 1)) == 0) atomicMax(pre_rowmax + r, __float_as_int(rmax));
        }
    }
}

// The same backward with the column statistics of what it reads and writes riding along, so that the weight / bias
// gradients that follow need no pass of their own over [g_gpre | g_zpre] (2 d wide) and x:
//   stats[0, 2d)        column sums of [g_gpre | g_zpre]          = the bias gradients of g and gate_*  (gate.py:24-25)
//   stats[2d, 4d)       column maxima |.| of [g_gpre | g_zpre]    } the column scales of the fp16 weight-gradient product
//   stats[4d, 5d)       column maxima |.| of x                    }   (lkg_gemm_wgrad_f32)
//   stats[5d + j 2d ..) sum_r [g_gpre | g_zpre][r, :] * w[r, j]    = the weight gradients of a NARROW literal panel w
//                                                                   (n_w <= 4 columns: the numeric literals)
// 16-byte path, one column chunk per thread (d <= 1024).  At most STAT_BLOCKS workgroups: every thread keeps running
// sums / maxima of its four columns over its rows, the block's row groups meet in LDS, the block writes ONE partial
// vector, and gate_stats_finish_kernel folds the partials (no atomics: deterministic).
constexpr int STAT_BLOCKS = 1024;
template <int NW>
__global__ __launch_bounds__(256) void gate_blend_bwd_stats_kernel(long n, int d, int log_tpr, const float *__restrict__ x,
                                                                    long ldx, const float *__restrict__ gpre, long ldg,
                                                                    const float *__restrict__ zpre, long ldz,
                                                                    const float *__restrict__ g_out, long ldgo,
                                                                    float *__restrict__ g_x, long ldgx,
                                                                    float *__restrict__ g_gpre, long ldgg,
                                                                    float *__restrict__ g_zpre, long ldgz, int activated,
                                                                    int *__restrict__ pre_rowmax,
                                                                    const float *__restrict__ w, long ldw,
                                                                    float *__restrict__ partial) {
    constexpr int W = 4, NV = 5 + 2 * NW;          // per column: sum og, sum oz, max og, max oz, max x, NW x (w og, w oz)
    __shared__ float red[NV][256][W];
    const int tpr = 1 << log_tpr, rpb = 256 >> log_tpr;
    const int c = (threadIdx.x & (tpr - 1)) * W;
    const bool has_col = c < d;
    float acc[NV][W];
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[v][k] = 0.f;
    for (long r = (long)blockIdx.x * rpb + (threadIdx.x >> log_tpr); r < n; r += (long)gridDim.x * rpb) {
        float rmax = 0.f;
        if (has_col) {
            float xv[W], gv[W], zv[W], go[W], ox[W], og[W], oz[W], wv[NW > 0 ? NW : 1];
            *reinterpret_cast<float4 *>(xv) = *reinterpret_cast<const float4 *>(x + r * ldx + c);
            *reinterpret_cast<float4 *>(gv) = *reinterpret_cast<const float4 *>(gpre + r * ldg + c);
            *reinterpret_cast<float4 *>(zv) = *reinterpret_cast<const float4 *>(zpre + r * ldz + c);
            *reinterpret_cast<float4 *>(go) = *reinterpret_cast<const float4 *>(g_out + r * ldgo + c);
#pragma unroll
            for (int j = 0; j < NW; ++j) wv[j] = w[r * ldw + j];
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float s = activated ? zv[k] : sigmoid_fast(zv[k]);
                const float tg = activated ? gv[k] : tanh_fast(gv[k]);
                ox[k] = go[k] * (1.f - s);
                og[k] = go[k] * s * (1.f - tg * tg);
                oz[k] = go[k] * (tg - xv[k]) * s * (1.f - s);
                rmax = fmaxf(rmax, fmaxf(fabsf(og[k]), fabsf(oz[k])));
                acc[0][k] += og[k];
                acc[1][k] += oz[k];
                acc[2][k] = fmaxf(acc[2][k], fabsf(og[k]));
                acc[3][k] = fmaxf(acc[3][k], fabsf(oz[k]));
                acc[4][k] = fmaxf(acc[4][k], fabsf(xv[k]));
#pragma unroll
                for (int j = 0; j < NW; ++j) {
                    acc[5 + 2 * j][k] = fmaf(og[k], wv[j], acc[5 + 2 * j][k]);
                    acc[6 + 2 * j][k] = fmaf(oz[k], wv[j], acc[6 + 2 * j][k]);
                }
            }
            *reinterpret_cast<float4 *>(g_x + r * ldgx + c) = *reinterpret_cast<float4 *>(ox);
            *reinterpret_cast<float4 *>(g_gpre + r * ldgg + c) = *reinterpret_cast<float4 *>(og);
            *reinterpret_cast<float4 *>(g_zpre + r * ldgz + c) = *reinterpret_cast<float4 *>(oz);
        }
        if (pre_rowmax) {
            const int span = tpr < 64 ? tpr : 64;
            for (int m = 1; m < span; m <<= 1) rmax = fmaxf(rmax, __shfl_xor(rmax, m, 64));
            if ((threadIdx.x & (span - 1)) == 0) atomicMax(pre_rowmax + r, __float_as_int(rmax));
        }
    }
    // the rpb row groups of the block hold the same columns: fold them, then one partial vector per block
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
        for (int k = 0; k < W; ++k) red[v][threadIdx.x][k] = acc[v][k];
    __syncthreads();
    if (threadIdx.x < tpr && has_col) {
        const int two_d = 2 * d;
        float *pb = partial + (long)blockIdx.x * ((5 + 2 * NW) * d);
#pragma unroll
        for (int k = 0; k < W; ++k) {
            float f[NV];
#pragma unroll
            for (int v = 0; v < NV; ++v) {
                float a = red[v][threadIdx.x][k];
                for (int g = 1; g < rpb; ++g) {
                    const float b = red[v][threadIdx.x + g * tpr][k];
                    a = (v >= 2 && v <= 4) ? fmaxf(a, b) : a + b;
                }
                f[v] = a;
            }
            const int col = c + k;
            pb[col] = f[0];                 // sums: og | oz
            pb[d + col] = f[1];
            pb[two_d + col] = f[2];         // maxima: og | oz
            pb[two_d + d + col] = f[3];
            pb[2 * two_d + col] = f[4];     // maxima of x
#pragma unroll
            for (int j = 0; j < NW; ++j) {
                pb[5 * d + j * two_d + col] = f[5 + 2 * j];
                pb[5 * d + j * two_d + d + col] = f[6 + 2 * j];
            }
        }
    }
}

// stats[i] = fold over the blocks' partial vectors: maxima for i in [2d, 5d), sums elsewhere.  64 statistics per
// workgroup, four threads each (interleaved blocks, eight loads in flight), folded in LDS in a fixed order.
__global__ __launch_bounds__(256) void gate_stats_finish_kernel(int n_stats, int d, int n_blocks, const float *__restrict__ partial,
                                                                float *__restrict__ stats) {
    __shared__ float red[4][64];
    const int q = threadIdx.x >> 6, i = blockIdx.x * 64 + (threadIdx.x & 63);
    const bool live = i < n_stats, is_max = i >= 2 * d && i < 5 * d;
    float a = 0.f;
    if (live) {
        int b = q;
        for (; b + 28 < n_blocks; b += 32) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = partial[(long)(b + 4 * u) * n_stats + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) a = is_max ? fmaxf(a, v[u]) : a + v[u];
        }
        for (; b < n_blocks; b += 4) {
            const float v = partial[(long)b * n_stats + i];
            a = is_max ? fmaxf(a, v) : a + v;
        }
    }
    red[q][threadIdx.x & 63] = a;
    __syncthreads();
    if (q == 0 && live) {
        const int l = threadIdx.x;
        stats[i] = is_max ? fmaxf(fmaxf(red[0][l], red[1][l]), fmaxf(red[2][l], red[3][l]))
                          : (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    }
}

// threads per row (log2) for a row of `units` access units
inline int log_threads_per_row(int units) {
    int l = 0;
    while ((1 << l) < units && l < 8) ++l;
    return l;
}

template <int W>
int pick_cpl(int d) {
    const int chunks = (d + W - 1) / W;
    const int cpl = (chunks + 63) / 64;
    return cpl;
}

}  // namespace

#define LKG_ROW_DISPATCH(KERNEL, GRID, ...)                                                                      \
    do {                                                                                                         \
        if (vec) {                                                                                               \
            switch (pick_cpl<4>(d)) {                                                                            \
                case 1: hipLaunchKernelGGL((KERNEL<4, 1>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                case 2: hipLaunchKernelGGL((KERNEL<4, 2>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                case 3: hipLaunchKernelGGL((KERNEL<4, 3>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                case 4: hipLaunchKernelGGL((KERNEL<4, 4>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                default: lkg_set_error("row width %d > 1024 not supported", d); return LKG_ERR_UNSUPPORTED;      \
            }                                                                                                    \
        } else {                                                                                                 \
            switch (pick_cpl<1>(d)) {                                                                            \
                case 1: hipLaunchKernelGGL((KERNEL<1, 1>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                case 2: hipLaunchKernelGGL((KERNEL<1, 2>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                case 3: hipLaunchKernelGGL((KERNEL<1, 3>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                case 4: hipLaunchKernelGGL((KERNEL<1, 4>), GRID, dim3(256), 0, s, __VA_ARGS__); break;           \
                default:                                                                                         \
                    lkg_set_error("row width %d > 256 needs 16-byte aligned rows (d %% 4 == 0)", d);             \
                    return LKG_ERR_UNSUPPORTED;                                                                  \
            }                                                                                                    \
        }                                                                                                        \
    } while (0)

extern "C" int lkg_act_layernorm_fwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, float slope,
                                         const float *gamma, const float *beta, float eps, float *y, int64_t ldy,
                                         float *yn, int64_t ldyn, float norm_eps, float *save_mean, float *save_rstd,
                                         float drop_p, uint64_t seed, void *stream) {
    LKG_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "lkg_act_layernorm_fwd_f32: dropout probability %g outside [0,1)", drop_p);
    LKG_REQUIRE(n >= 0 && d > 0 && ldz >= d && (!y || ldy >= d) && (!yn || ldyn >= d), "lkg_act_layernorm_fwd_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(z && gamma && beta && (y || yn) && save_mean && save_rstd, "lkg_act_layernorm_fwd_f32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = d % 4 == 0 && ldz % 4 == 0 && (!y || ldy % 4 == 0) && (!yn || ldyn % 4 == 0) && lkg_aligned16(z) &&
                     (!y || lkg_aligned16(y)) && lkg_aligned16(gamma) && lkg_aligned16(beta) && (!yn || lkg_aligned16(yn));
    static const bool narrow_off = getenv("LKG_ACTLN_NARROW_OFF") != nullptr;     // (A/B aid)
    if (vec && d <= 128 && !narrow_off) {      // several rows per wave
        const int lpr = d <= 32 ? 8 : d <= 64 ? 16 : 32;
        const int64_t rows_per_block = 4 * (64 / lpr);
        const dim3 grid_n((unsigned)((n + rows_per_block - 1) / rows_per_block));
#define LKG_NARROW(LPR_)                                                                                                  \
    hipLaunchKernelGGL((act_ln_fwd_narrow_kernel<LPR_>), grid_n, dim3(256), 0, s, (long)n, d, z, (long)ldz, slope, gamma, beta, \
                       eps, y, (long)ldy, yn, (long)ldyn, norm_eps, save_mean, save_rstd, drop_p, (unsigned long long)seed)
        if (lpr == 8) LKG_NARROW(8);
        else if (lpr == 16) LKG_NARROW(16);
        else LKG_NARROW(32);
#undef LKG_NARROW
        LKG_CHECK_LAUNCH("lkg_act_layernorm_fwd_f32");
        return LKG_OK;
    }
    const dim3 grid((unsigned)((n + 3) / 4));
    LKG_ROW_DISPATCH(act_ln_fwd_kernel, grid, (long)n, d, z, (long)ldz, slope, gamma, beta, eps, y, (long)ldy, yn,
                     (long)ldyn, norm_eps, save_mean, save_rstd, drop_p, (unsigned long long)seed);
    LKG_CHECK_LAUNCH("lkg_act_layernorm_fwd_f32");
    return LKG_OK;
}

extern "C" int lkg_act_layernorm_bwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, float slope,
                                         const float *gamma, const float *beta, const float *y, int64_t ldy,
                                         const float *save_mean,
                                         const float *save_rstd, const float *g_y, int64_t ldgy, const float *g_yn,
                                         int64_t ldgyn, float norm_eps, float *g_z, int64_t ldgz, float *g_gamma,
                                         float *g_beta, float drop_p, uint64_t seed, float *g_z_rowmax,
                                         const uint8_t *g_yn_rows, int32_t sparse_out, const int64_t *row_ids,
                                         int64_t n_row_ids, void *stream) {
    LKG_REQUIRE(!sparse_out || (!g_z_rowmax && (row_ids || (g_yn_rows && g_yn && !g_y))),
                "lkg_act_layernorm_bwd_f32: sparse_out needs a row list, or row flags and no g_y; and no row maxima");
    LKG_REQUIRE(!row_ids || (sparse_out && n_row_ids >= 0), "lkg_act_layernorm_bwd_f32: a row list needs sparse_out");
    LKG_REQUIRE(drop_p >= 0.f && drop_p < 1.f, "lkg_act_layernorm_bwd_f32: dropout probability %g outside [0,1)", drop_p);
    LKG_REQUIRE(n >= 0 && d > 0 && ldz >= d && ldgz >= d, "lkg_act_layernorm_bwd_f32: bad sizes");
    if (n == 0) return LKG_OK;             // (a rank without rows: empty operands may come as null pointers)
    LKG_REQUIRE(g_y || g_yn, "lkg_act_layernorm_bwd_f32: both upstream gradients are null");
    LKG_REQUIRE(z && gamma && save_mean && save_rstd && g_z && g_gamma && g_beta && (!g_yn || y || beta),
                "lkg_act_layernorm_bwd_f32: null pointer (g_yn needs y, or beta to recompute it)");
    hipStream_t s = (hipStream_t)stream;
    const bool vec = d % 4 == 0 && ldz % 4 == 0 && ldgz % 4 == 0 && (!g_y || ldgy % 4 == 0) &&
                     (!g_yn || (ldgyn % 4 == 0 && (!y || ldy % 4 == 0))) && lkg_aligned16(z) && lkg_aligned16(g_z) &&
                     lkg_aligned16(gamma) && (!g_y || lkg_aligned16(g_y)) &&
                     (!g_yn || (lkg_aligned16(g_yn) && (!y || lkg_aligned16(y)) && (y || lkg_aligned16(beta))));
    if (vec && d <= 128 && !sparse_out && !row_ids && (!g_yn || y) && n >= 4096) {      // several rows per wave
        const int lpr = d <= 32 ? 8 : d <= 64 ? 16 : 32;
        const int64_t groups = (n + 64 / lpr - 1) / (64 / lpr);
        const dim3 grid_n((unsigned)std::min<int64_t>((groups + 3) / 4, 2048));
#define LKG_NARROW(LPR_)                                                                                                   \
    hipLaunchKernelGGL((act_ln_bwd_narrow_kernel<LPR_>), grid_n, dim3(256), 0, s, (long)n, d, z, (long)ldz, slope, gamma, y,   \
                       (long)ldy, save_mean, save_rstd, g_y, (long)ldgy, g_yn, (long)ldgyn, norm_eps, g_z, (long)ldgz, g_gamma, \
                       g_beta, drop_p, (unsigned long long)seed, g_z_rowmax, g_yn ? g_yn_rows : nullptr)
        if (lpr == 8) LKG_NARROW(8);
        else if (lpr == 16) LKG_NARROW(16);
        else LKG_NARROW(32);
#undef LKG_NARROW
        LKG_CHECK_LAUNCH("lkg_act_layernorm_bwd_f32");
        return LKG_OK;
    }
    const int64_t n_work = row_ids ? n_row_ids : n;
    if (n_work == 0) return LKG_OK;
    const dim3 grid((unsigned)std::min<int64_t>((n_work + 3) / 4, 1024));
    LKG_ROW_DISPATCH(act_ln_bwd_kernel, grid, (long)n, d, z, (long)ldz, slope, gamma, beta, y, (long)ldy, save_mean,
                     save_rstd, g_y, (long)ldgy, g_yn, (long)ldgyn, norm_eps, g_z, (long)ldgz, g_gamma, g_beta, drop_p,
                     (unsigned long long)seed, g_z_rowmax, g_yn ? g_yn_rows : nullptr, sparse_out,
                     (const long *)row_ids, (long)n_row_ids);
    LKG_CHECK_LAUNCH("lkg_act_layernorm_bwd_f32");
    return LKG_OK;
}

extern "C" int lkg_gate_blend_fwd_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *gpre,
                                      int64_t ldg, const float *zpre, int64_t ldz, float *out, int64_t ldo,
                                      void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && ldx >= d && ldg >= d && ldz >= d && ldo >= d, "lkg_gate_blend_fwd_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(x && gpre && zpre && out, "lkg_gate_blend_fwd_f32: null pointer");
    const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldg % 4 == 0 && ldz % 4 == 0 && ldo % 4 == 0 && lkg_aligned16(x) &&
                     lkg_aligned16(gpre) && lkg_aligned16(zpre) && lkg_aligned16(out);
    const int lt = log_threads_per_row(vec ? d / 4 : d);
    const int64_t blocks = std::min<int64_t>((n + (256 >> lt) - 1) / (256 >> lt), 256 * 32);
    if (vec)
        hipLaunchKernelGGL(gate_blend_fwd_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n,
                           d, lt, x, (long)ldx, gpre, (long)ldg, zpre, (long)ldz, out, (long)ldo);
    else
        hipLaunchKernelGGL(gate_blend_fwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n,
                           d, lt, x, (long)ldx, gpre, (long)ldg, zpre, (long)ldz, out, (long)ldo);
    LKG_CHECK_LAUNCH("lkg_gate_blend_fwd_f32");
    return LKG_OK;
}

extern "C" int lkg_gate_blend_bwd_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *gpre,
                                      int64_t ldg, const float *zpre, int64_t ldz, const float *g_out, int64_t ldgo,
                                      float *g_x, int64_t ldgx, float *g_gpre, int64_t ldgg, float *g_zpre,
                                      int64_t ldgz, int32_t activated, float *g_pre_rowmax, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && ldx >= d && ldg >= d && ldz >= d && ldgo >= d && ldgx >= d && ldgg >= d && ldgz >= d,
                "lkg_gate_blend_bwd_f32: bad sizes");
    if (n == 0) return LKG_OK;
    if (g_pre_rowmax && hipMemsetAsync(g_pre_rowmax, 0, sizeof(float) * n, (hipStream_t)stream) != hipSuccess) {
        lkg_set_error("lkg_gate_blend_bwd_f32: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    LKG_REQUIRE(x && gpre && zpre && g_out && g_x && g_gpre && g_zpre, "lkg_gate_blend_bwd_f32: null pointer");
    const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldg % 4 == 0 && ldz % 4 == 0 && ldgo % 4 == 0 && ldgx % 4 == 0 &&
                     ldgg % 4 == 0 && ldgz % 4 == 0 && lkg_aligned16(x) && lkg_aligned16(gpre) && lkg_aligned16(zpre) &&
                     lkg_aligned16(g_out) && lkg_aligned16(g_x) && lkg_aligned16(g_gpre) && lkg_aligned16(g_zpre);
    const int lt = log_threads_per_row(vec ? d / 4 : d);
    const int64_t blocks = std::min<int64_t>((n + (256 >> lt) - 1) / (256 >> lt), 256 * 32);
    if (vec)
        hipLaunchKernelGGL(gate_blend_bwd_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n,
                           d, lt, x, (long)ldx, gpre, (long)ldg, zpre, (long)ldz, g_out, (long)ldgo, g_x, (long)ldgx,
                           g_gpre, (long)ldgg, g_zpre, (long)ldgz, activated, reinterpret_cast<int *>(g_pre_rowmax));
    else
        hipLaunchKernelGGL(gate_blend_bwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n,
                           d, lt, x, (long)ldx, gpre, (long)ldg, zpre, (long)ldz, g_out, (long)ldgo, g_x, (long)ldgx,
                           g_gpre, (long)ldgg, g_zpre, (long)ldgz, activated, reinterpret_cast<int *>(g_pre_rowmax));
    LKG_CHECK_LAUNCH("lkg_gate_blend_bwd_f32");
    return LKG_OK;
}

// The backward of the blend with the column statistics of [g_gpre | g_zpre] and x riding along (see
// gate_blend_bwd_stats_kernel): stats has (5 + 2 n_w) d floats, workspace STAT_BLOCKS = 1024 times that.
extern "C" int lkg_gate_blend_bwd_stats_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *gpre,
                                            int64_t ldg, const float *zpre, int64_t ldz, const float *g_out, int64_t ldgo,
                                            float *g_x, int64_t ldgx, float *g_gpre, int64_t ldgg, float *g_zpre,
                                            int64_t ldgz, int32_t activated, float *g_pre_rowmax, const float *w,
                                            int64_t ldw, int32_t n_w, float *workspace, int64_t workspace_floats,
                                            float *stats, void *stream) {
    LKG_REQUIRE(n > 0 && d > 0 && d % 4 == 0 && d <= 1024 && ldx >= d && ldg >= d && ldz >= d && ldgo >= d && ldgx >= d &&
                    ldgg >= d && ldgz >= d, "lkg_gate_blend_bwd_stats_f32: bad sizes (d a multiple of 4, <= 1024)");
    LKG_REQUIRE(n_w >= 0 && n_w <= 4 && (n_w == 0 || (w && ldw >= n_w)), "lkg_gate_blend_bwd_stats_f32: narrow panel of 0..4 columns");
    LKG_REQUIRE(x && gpre && zpre && g_out && g_x && g_gpre && g_zpre && workspace && stats, "lkg_gate_blend_bwd_stats_f32: null pointer");
    const bool vec = ldx % 4 == 0 && ldg % 4 == 0 && ldz % 4 == 0 && ldgo % 4 == 0 && ldgx % 4 == 0 && ldgg % 4 == 0 &&
                     ldgz % 4 == 0 && lkg_aligned16(x) && lkg_aligned16(gpre) && lkg_aligned16(zpre) && lkg_aligned16(g_out) &&
                     lkg_aligned16(g_x) && lkg_aligned16(g_gpre) && lkg_aligned16(g_zpre);
    LKG_REQUIRE(vec, "lkg_gate_blend_bwd_stats_f32: operands must be 16-byte aligned with row strides that are multiples of 4");
    hipStream_t s = (hipStream_t)stream;
    if (g_pre_rowmax && hipMemsetAsync(g_pre_rowmax, 0, sizeof(float) * n, s) != hipSuccess) {
        lkg_set_error("lkg_gate_blend_bwd_stats_f32: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    const int lt = log_threads_per_row(d / 4), rpb = 256 >> lt;
    const int n_stats = (5 + 2 * n_w) * d;
    const int blocks = (int)std::min<int64_t>((n + rpb - 1) / rpb, STAT_BLOCKS);
    LKG_REQUIRE(workspace_floats >= (int64_t)blocks * n_stats, "lkg_gate_blend_bwd_stats_f32: workspace of %lld floats, %lld needed",
                (long long)workspace_floats, (long long)blocks * n_stats);
#define LKG_GBS(NW)                                                                                                       \
    case NW:                                                                                                              \
        hipLaunchKernelGGL(gate_blend_bwd_stats_kernel<NW>, dim3((unsigned)blocks), dim3(256), 0, s, (long)n, d, lt, x,  \
                           (long)ldx, gpre, (long)ldg, zpre, (long)ldz, g_out, (long)ldgo, g_x, (long)ldgx, g_gpre,      \
                           (long)ldgg, g_zpre, (long)ldgz, activated, reinterpret_cast<int *>(g_pre_rowmax), w,          \
                           (long)ldw, workspace);                                                                        \
        break;
    switch (n_w) { LKG_GBS(0) LKG_GBS(1) LKG_GBS(2) LKG_GBS(3) LKG_GBS(4) }
#undef LKG_GBS
    LKG_CHECK_LAUNCH("lkg_gate_blend_bwd_stats_f32");
    hipLaunchKernelGGL(gate_stats_finish_kernel, dim3((unsigned)((n_stats + 63) / 64)), dim3(256), 0, s, n_stats, d, blocks,
                       workspace, stats);
    LKG_CHECK_LAUNCH("lkg_gate_blend_bwd_stats_f32");
    return LKG_OK;
}

namespace {
__global__ __launch_bounds__(256) void colsum_kernel(long n, int d, const float *__restrict__ x, long ldx,
                                                      float *__restrict__ out, long rows_per_block) {
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;   // four rows in flight per thread
        long r = r0;
        for (; r + 4 <= r1; r += 4) {
            s0 += x[r * ldx + c];
            s1 += x[(r + 1) * ldx + c];
            s2 += x[(r + 2) * ldx + c];
            s3 += x[(r + 3) * ldx + c];
        }
        for (; r < r1; ++r) s0 += x[r * ldx + c];
        atomicAdd(out + c, (s0 + s1) + (s2 + s3));
    }
}

// out_w[c, j] = sum_i x[i, c] * w[i, j] (j < NW <= 8) and, when asked, out_sum[c] = sum_i x[i, c] in the SAME pass over x:
// the weight gradient of a Linear's NARROW input panel (the 2-wide numeric literals of the gate: a long-k GEMM would
// spend a whole 128-wide MFMA tile and a full read of x on two columns) together with the bias gradient.
template <int NW>
__global__ __launch_bounds__(256) void colsum_weighted_kernel(long n, int d, const float *__restrict__ x, long ldx,
                                                               const float *__restrict__ w, long ldw,
                                                               float *__restrict__ out_sum, float *__restrict__ out_w,
                                                               long ld_out, long rows_per_block) {
    const long r0 = (long)blockIdx.x * rows_per_block, r1 = min(n, r0 + rows_per_block);
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float s[2] = {0.f, 0.f}, sw[2][NW];
#pragma unroll
        for (int j = 0; j < NW; ++j) sw[0][j] = sw[1][j] = 0.f;
        long r = r0;
        for (; r + 4 <= r1; r += 4) {            // four rows in flight per thread; w[r, :] is block-uniform (scalar loads)
            float v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = x[(r + u) * ldx + c];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                s[u & 1] += v[u];
#pragma unroll
                for (int j = 0; j < NW; ++j) sw[u & 1][j] = fmaf(v[u], w[(r + u) * ldw + j], sw[u & 1][j]);
            }
        }
        for (; r < r1; ++r) {
            const float v = x[r * ldx + c];
            s[0] += v;
#pragma unroll
            for (int j = 0; j < NW; ++j) sw[0][j] = fmaf(v, w[r * ldw + j], sw[0][j]);
        }
        if (out_sum) atomicAdd(out_sum + c, s[0] + s[1]);
#pragma unroll
        for (int j = 0; j < NW; ++j) atomicAdd(out_w + c * ld_out + j, sw[0][j] + sw[1][j]);
    }
}
}  // namespace

extern "C" int lkg_colsum_weighted_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *w, int64_t ldw,
                                       int32_t n_w, float *out_sum, float *out_w, int64_t ld_out_w, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && ldx >= d && n_w >= 1 && n_w <= 8 && ldw >= n_w && ld_out_w >= n_w && out_w,
                "lkg_colsum_weighted_f32: bad arguments (1 <= n_w <= 8)");
    hipStream_t s = (hipStream_t)stream;
    bool ok = !out_sum || hipMemsetAsync(out_sum, 0, sizeof(float) * d, s) == hipSuccess;
    ok = ok && (ld_out_w == n_w ? hipMemsetAsync(out_w, 0, sizeof(float) * d * n_w, s)
                                : hipMemset2DAsync(out_w, sizeof(float) * ld_out_w, 0, sizeof(float) * n_w, d, s)) == hipSuccess;
    if (!ok) {
        lkg_set_error("lkg_colsum_weighted_f32: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(x && w, "lkg_colsum_weighted_f32: null pointer");
    const long blocks = std::min<int64_t>((n + 63) / 64, 2048);
    const long rpb = (n + blocks - 1) / blocks;
#define LKG_CSW(NW)                                                                                                  \
    case NW:                                                                                                         \
        hipLaunchKernelGGL(colsum_weighted_kernel<NW>, dim3((unsigned)blocks), dim3(256), 0, s, (long)n, d, x,       \
                           (long)ldx, w, (long)ldw, out_sum, out_w, (long)ld_out_w, rpb);                            \
        break;
    switch (n_w) {
        LKG_CSW(1) LKG_CSW(2) LKG_CSW(3) LKG_CSW(4) LKG_CSW(5) LKG_CSW(6) LKG_CSW(7) LKG_CSW(8)
    }
#undef LKG_CSW
    LKG_CHECK_LAUNCH("lkg_colsum_weighted_f32");
    return LKG_OK;
}

extern "C" int lkg_colsum_f32(int64_t n, int32_t d, const float *x, int64_t ldx, float *out, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && ldx >= d && out, "lkg_colsum_f32: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(out, 0, sizeof(float) * d, s) != hipSuccess) {
        lkg_set_error("lkg_colsum_f32: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(x, "lkg_colsum_f32: null pointer");
    const long blocks = std::min<int64_t>((n + 63) / 64, 2048);
    const long rpb = (n + blocks - 1) / blocks;
    hipLaunchKernelGGL(colsum_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (long)n, d, x, (long)ldx, out, rpb);
    LKG_CHECK_LAUNCH("lkg_colsum_f32");
    return LKG_OK;
}

// ---------------------------------------------------------------------------------------------------
// f4  fused Adam step over one dense tensor (the N x D entity table gets a dense gradient every step,
// SURVEY.md 3.5-5): one pass, 4 reads + 3 writes per element, torch.optim.Adam's arithmetic
// (bias-corrected, eps added after the sqrt, optional L2 weight decay folded into the gradient).
namespace {
__global__ __launch_bounds__(256) void adam_kernel(long n, float *__restrict__ p, const float *__restrict__ g,
                                                    float *__restrict__ m, float *__restrict__ v, float lr,
                                                    float beta1, float beta2, float eps, float weight_decay,
                                                    float bc1, float bc2_sqrt) {
    const long n4 = n / 4;
    const long stride = (long)gridDim.x * blockDim.x;
    const float step_size = lr / bc1;
    auto upd = [&](float &pp, float gg, float &mm, float &vv) {
        gg = fmaf(weight_decay, pp, gg);
        mm = fmaf(beta1, mm, (1.f - beta1) * gg);
        vv = fmaf(beta2, vv, (1.f - beta2) * gg * gg);
        pp -= step_size * mm / (sqrtf(vv) / bc2_sqrt + eps);
    };
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
        float4 pp = reinterpret_cast<float4 *>(p)[i], mm = reinterpret_cast<float4 *>(m)[i],
               vv = reinterpret_cast<float4 *>(v)[i];
        const float4 gg = reinterpret_cast<const float4 *>(g)[i];
        upd(pp.x, gg.x, mm.x, vv.x);
        upd(pp.y, gg.y, mm.y, vv.y);
        upd(pp.z, gg.z, mm.z, vv.z);
        upd(pp.w, gg.w, mm.w, vv.w);
        reinterpret_cast<float4 *>(p)[i] = pp;
        reinterpret_cast<float4 *>(m)[i] = mm;
        reinterpret_cast<float4 *>(v)[i] = vv;
    }
    for (long i = n4 * 4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) upd(p[i], g[i], m[i], v[i]);
}
}  // namespace

extern "C" int lkg_adam_step_f32(int64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                                 float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                                 void *stream) {
    LKG_REQUIRE(n >= 0 && step >= 1, "lkg_adam_step_f32: n must be >= 0 and step >= 1");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(param && grad && exp_avg && exp_avg_sq, "lkg_adam_step_f32: null pointer");
    LKG_REQUIRE(lkg_aligned16(param) && lkg_aligned16(grad) && lkg_aligned16(exp_avg) && lkg_aligned16(exp_avg_sq),
                "lkg_adam_step_f32: tensors must be 16-byte aligned and contiguous");
    const double bc1 = 1.0 - std::pow((double)beta1, (double)step);
    const double bc2 = 1.0 - std::pow((double)beta2, (double)step);
    const int64_t blocks = std::min<int64_t>((n / 4 + 255) / 256 + 1, 256 * 16);
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, param, grad,
                       exp_avg, exp_avg_sq, lr, beta1, beta2, eps, weight_decay, (float)bc1, (float)std::sqrt(bc2));
    LKG_CHECK_LAUNCH("lkg_adam_step_f32");
    return LKG_OK;
}

// ---------------------------------------------------------------------------------------------------
// f1  MLP head (model.py:499-519, model_bce.py:255-260, 423-436):  y = BatchNorm1d(relu(z)) fused.
// A workgroup owns 64 columns; its four waves stride over the rows (coalesced 256-B row segments) and meet in
// LDS for the column statistics.  Training mode uses batch statistics (biased variance for the output, unbiased
// for the running estimate, like nn.BatchNorm1d) and updates the running buffers; eval mode uses the buffers.
// The column sums (mean, variance, g_gamma, g_beta) are ACCUMULATED IN FLOAT64 and rounded to float32 once: each of the four
// waves walks n / 4 rows of its column in one chain, and a float32 chain of 2 000 same-sign terms (n = 8 195, a column with
// a common offset) lost 5e-7 .. 8e-7 of the mean and 2e-6 of 1 / std -- several times torch's blocked sums
// (tests/test_rowwise_conditioning_gpu.py::test_relu_batchnorm).  The kernel is bound by its one workgroup per 64 columns
// reading n rows; the float64 adds do not show.
namespace {
__device__ __forceinline__ double col_reduce4(double v, double (*sm)[64], int g, int c) {
    sm[g][c] = v;
    __syncthreads();
    const double r = (sm[0][c] + sm[1][c]) + (sm[2][c] + sm[3][c]);
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void relu_bn_fwd_kernel(long n, int d, const float *__restrict__ z, long ldz,
                                                           const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, float eps, int training,
                                                           float momentum, float *__restrict__ running_mean,
                                                           float *__restrict__ running_var, float *__restrict__ y,
                                                           long ldy, float *__restrict__ save_mean,
                                                           float *__restrict__ save_invstd) {
    __shared__ double sm[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6, lc = threadIdx.x & 63;
    const bool ok = c < d;
    float mean, invstd;
    if (training) {
        double s = 0.0;
        for (long r = g; r < n; r += 4) s += ok ? (double)fmaxf(z[r * ldz + c], 0.f) : 0.0;
        mean = (float)(col_reduce4(s, sm, g, lc) / (double)n);
        double q = 0.0;
        for (long r = g; r < n; r += 4) {
            const double a = ok ? (double)(fmaxf(z[r * ldz + c], 0.f) - mean) : 0.0;
            q = fma(a, a, q);
        }
        const float var = (float)(col_reduce4(q, sm, g, lc) / (double)n);
        invstd = 1.f / sqrtf(var + eps);
        if (ok && g == 0) {
            running_mean[c] = (1.f - momentum) * running_mean[c] + momentum * mean;
            running_var[c] = (1.f - momentum) * running_var[c] + momentum * var * ((float)n / (float)max(n - 1, 1L));
        }
    } else {
        mean = ok ? running_mean[c] : 0.f;
        invstd = ok ? 1.f / sqrtf(running_var[c] + eps) : 0.f;
    }
    if (ok && g == 0) {
        save_mean[c] = mean;
        save_invstd[c] = invstd;
    }
    const float ga = ok ? gamma[c] : 0.f, be = ok ? beta[c] : 0.f;
    for (long r = g; r < n; r += 4)
        if (ok) y[r * ldy + c] = (fmaxf(z[r * ldz + c], 0.f) - mean) * invstd * ga + be;
}

__global__ __launch_bounds__(256) void relu_bn_bwd_kernel(long n, int d, const float *__restrict__ z, long ldz,
                                                           const float *__restrict__ gamma,
                                                           const float *__restrict__ save_mean,
                                                           const float *__restrict__ save_invstd, int training,
                                                           const float *__restrict__ g_y, long ldgy,
                                                           float *__restrict__ g_z, long ldgz,
                                                           float *__restrict__ g_gamma, float *__restrict__ g_beta) {
    __shared__ double sm[4][64];
    const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6, lc = threadIdx.x & 63;
    const bool ok = c < d;
    const float mean = ok ? save_mean[c] : 0.f, invstd = ok ? save_invstd[c] : 0.f, ga = ok ? gamma[c] : 0.f;
    double a1 = 0.0, a2 = 0.0;
    for (long r = g; r < n; r += 4) {
        const float dy = ok ? g_y[r * ldgy + c] : 0.f;
        const float xh = ok ? (fmaxf(z[r * ldz + c], 0.f) - mean) * invstd : 0.f;
        a1 += (double)dy;
        a2 = fma((double)dy, (double)xh, a2);
    }
    const float s1 = (float)col_reduce4(a1, sm, g, lc);
    const float s2 = (float)col_reduce4(a2, sm, g, lc);
    if (ok && g == 0) {
        g_beta[c] = s1;
        g_gamma[c] = s2;
    }
    const float inv_n = 1.f / (float)n;
    for (long r = g; r < n; r += 4) {
        if (!ok) continue;
        const float zz = z[r * ldz + c];
        const float dy = g_y[r * ldgy + c];
        float da;
        if (training) {
            const float xh = (fmaxf(zz, 0.f) - mean) * invstd;
            da = ga * invstd * (dy - s1 * inv_n - xh * s2 * inv_n);
        } else {
            da = ga * invstd * dy;
        }
        g_z[r * ldgz + c] = zz > 0.f ? da : 0.f;
    }
}
}  // namespace

extern "C" int lkg_relu_batchnorm_fwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, const float *gamma,
                                          const float *beta, float eps, int32_t training, float momentum,
                                          float *running_mean, float *running_var, float *y, int64_t ldy,
                                          float *save_mean, float *save_invstd, void *stream) {
    LKG_REQUIRE(n > 0 && d > 0 && ldz >= d && ldy >= d, "lkg_relu_batchnorm_fwd_f32: bad sizes (n=%lld, d=%d)",
                (long long)n, d);
    LKG_REQUIRE(!training || n > 1, "lkg_relu_batchnorm_fwd_f32: training mode needs more than one row per batch");
    LKG_REQUIRE(z && gamma && beta && running_mean && running_var && y && save_mean && save_invstd,
                "lkg_relu_batchnorm_fwd_f32: null pointer");
    hipLaunchKernelGGL(relu_bn_fwd_kernel, dim3((unsigned)((d + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (long)n,
                       d, z, (long)ldz, gamma, beta, eps, training, momentum, running_mean, running_var, y, (long)ldy,
                       save_mean, save_invstd);
    LKG_CHECK_LAUNCH("lkg_relu_batchnorm_fwd_f32");
    return LKG_OK;
}

extern "C" int lkg_relu_batchnorm_bwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, const float *gamma,
                                          const float *save_mean, const float *save_invstd, int32_t training,
                                          const float *g_y, int64_t ldgy, float *g_z, int64_t ldgz, float *g_gamma,
                                          float *g_beta, void *stream) {
    LKG_REQUIRE(n > 0 && d > 0 && ldz >= d && ldgy >= d && ldgz >= d, "lkg_relu_batchnorm_bwd_f32: bad sizes");
    LKG_REQUIRE(z && gamma && save_mean && save_invstd && g_y && g_z && g_gamma && g_beta,
                "lkg_relu_batchnorm_bwd_f32: null pointer");
    hipLaunchKernelGGL(relu_bn_bwd_kernel, dim3((unsigned)((d + 63) / 64)), dim3(256), 0, (hipStream_t)stream, (long)n,
                       d, z, (long)ldz, gamma, save_mean, save_invstd, training, g_y, (long)ldgy, g_z, (long)ldgz,
                       g_gamma, g_beta);
    LKG_CHECK_LAUNCH("lkg_relu_batchnorm_bwd_f32");
    return LKG_OK;
}

// ---------------------------------------------------------------------------------------------------
// Small element-wise steps of the aggregation layers that are not worth a fusion of their own: the GCNII residual
// mix (model.py:94-96), ego * side and the per-branch LeakyReLU sum of 'bi-interaction' (model.py:125-130), the
// row sums of 'gin' (model.py:146, 158), LeakyReLU after linear_gat (model.py:310).  One strided 2-D kernel,
// 2^k threads per row like the gate blend, 16-byte accesses when rows are aligned.
//   op 0  out = alpha * a + beta * b          (b == NULL: out = alpha * a + beta)
//   op 1  out = a * b
//   op 2  out = leaky(a, alpha) + leaky(b, alpha)          (b == NULL: out = leaky(a, alpha))
//   op 3  out = a * (b > 0 ? 1 : alpha)       (LeakyReLU backward: a = upstream gradient, b = pre-activation)
namespace {
template <int W>
__global__ __launch_bounds__(256) void eltwise_kernel(int op, long n, int d, int log_tpr, const float *__restrict__ a,
                                                       long lda, const float *__restrict__ b, long ldb, float alpha,
                                                       float beta, float *__restrict__ out, long ldo) {
    const int tpr = 1 << log_tpr, rpb = 256 >> log_tpr;
    const int c0 = (threadIdx.x & (tpr - 1)) * W;
    for (long r = (long)blockIdx.x * rpb + (threadIdx.x >> log_tpr); r < n; r += (long)gridDim.x * rpb)
        for (int c = c0; c < d; c += tpr * W) {
            float av[W], bv[W], ov[W];
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(av) = *reinterpret_cast<const float4 *>(a + r * lda + c);
                if (b) *reinterpret_cast<float4 *>(bv) = *reinterpret_cast<const float4 *>(b + r * ldb + c);
            } else {
                av[0] = a[r * lda + c];
                if (b) bv[0] = b[r * ldb + c];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float x = av[k], y = b ? bv[k] : 0.f;
                float o;
                if (op == 0)
                    o = b ? fmaf(alpha, x, beta * y) : fmaf(alpha, x, beta);
                else if (op == 1)
                    o = x * y;
                else if (op == 2)
                    o = (x > 0.f ? x : alpha * x) + (b ? (y > 0.f ? y : alpha * y) : 0.f);
                else
                    o = x * (y > 0.f ? 1.f : alpha);
                ov[k] = o;
            }
            if constexpr (W == 4)
                *reinterpret_cast<float4 *>(out + r * ldo + c) = *reinterpret_cast<float4 *>(ov);
            else
                out[r * ldo + c] = ov[0];
        }
}
}  // namespace

extern "C" int lkg_eltwise_f32(int32_t op, int64_t n, int32_t d, const float *a, int64_t lda, const float *b,
                               int64_t ldb, float alpha, float beta, float *out, int64_t ldo, void *stream) {
    LKG_REQUIRE(op >= 0 && op <= 3, "lkg_eltwise_f32: unknown op %d", op);
    LKG_REQUIRE(n >= 0 && d > 0 && lda >= d && ldo >= d && (!b || ldb >= d), "lkg_eltwise_f32: bad sizes");
    if (n == 0) return LKG_OK;             // (a rank without rows: its tensors are empty and their pointers null)
    LKG_REQUIRE(b || (op != 1 && op != 3), "lkg_eltwise_f32: op %d needs two operands", op);
    LKG_REQUIRE(a && out, "lkg_eltwise_f32: null pointer");
    const bool vec = d % 4 == 0 && lda % 4 == 0 && ldo % 4 == 0 && (!b || ldb % 4 == 0) && lkg_aligned16(a) &&
                     lkg_aligned16(out) && (!b || lkg_aligned16(b));
    const int lt = log_threads_per_row(vec ? d / 4 : d);
    const int64_t blocks = std::min<int64_t>((n + (256 >> lt) - 1) / (256 >> lt), 256 * 32);
    if (vec)
        hipLaunchKernelGGL(eltwise_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, op, (long)n, d, lt,
                           a, (long)lda, b, (long)ldb, alpha, beta, out, (long)ldo);
    else
        hipLaunchKernelGGL(eltwise_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, op, (long)n, d, lt,
                           a, (long)lda, b, (long)ldb, alpha, beta, out, (long)ldo);
    LKG_CHECK_LAUNCH("lkg_eltwise_f32");
    return LKG_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// bi-interaction's element-wise front (model.py:123-128, with the residual's mix of model.py:94): from ego, side (and the
// layer's projection h0p of the layer-0 table when the GCNII-style residual is on)
//     out_sum  = c (ego + side) + alpha h0p          out_prod = c (ego * side) + alpha h0p        c = 1 - alpha (1, 0 without h0p)
// in ONE pass (the reference's four: sum, product and two mixes), and its backward in one:
//     g_ego = c (g_sum + g_prod * side)     g_side = c (g_sum + g_prod * ego)     g_h0p = alpha (g_sum + g_prod)
// -- main.py's defaults (argument.py:52-58, 108) run this in each of eight 32-wide layers every step.
namespace {
template <int W>
__global__ __launch_bounds__(256) void bi_mix_fwd_kernel(long n, int d, int log_tpr, const float *__restrict__ ego, long lde,
                                                          const float *__restrict__ side, long lds,
                                                          const float *__restrict__ h0p, long ldh, float alpha,
                                                          float *__restrict__ out_sum, long ldos,
                                                          float *__restrict__ out_prod, long ldop) {
    const int tpr = 1 << log_tpr, rpb = 256 >> log_tpr;
    const int c0 = (threadIdx.x & (tpr - 1)) * W;
    const float c = h0p ? 1.f - alpha : 1.f;
    for (long r = (long)blockIdx.x * rpb + (threadIdx.x >> log_tpr); r < n; r += (long)gridDim.x * rpb)
        for (int col = c0; col < d; col += tpr * W) {
            float e[W], s[W], h[W], os[W], op[W];
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(e) = *reinterpret_cast<const float4 *>(ego + r * lde + col);
                *reinterpret_cast<float4 *>(s) = *reinterpret_cast<const float4 *>(side + r * lds + col);
                if (h0p) *reinterpret_cast<float4 *>(h) = *reinterpret_cast<const float4 *>(h0p + r * ldh + col);
            } else {
                e[0] = ego[r * lde + col];
                s[0] = side[r * lds + col];
                if (h0p) h[0] = h0p[r * ldh + col];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                const float hh = h0p ? alpha * h[k] : 0.f;
                os[k] = fmaf(c, e[k] + s[k], hh);
                op[k] = fmaf(c, e[k] * s[k], hh);
            }
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(out_sum + r * ldos + col) = *reinterpret_cast<float4 *>(os);
                *reinterpret_cast<float4 *>(out_prod + r * ldop + col) = *reinterpret_cast<float4 *>(op);
            } else {
                out_sum[r * ldos + col] = os[0];
                out_prod[r * ldop + col] = op[0];
            }
        }
}

template <int W>
__global__ __launch_bounds__(256) void bi_mix_bwd_kernel(long n, int d, int log_tpr, const float *__restrict__ ego, long lde,
                                                          const float *__restrict__ side, long lds,
                                                          const float *__restrict__ g_sum, long ldgs,
                                                          const float *__restrict__ g_prod, long ldgp, int has_h0, float alpha,
                                                          float *__restrict__ g_ego, float *__restrict__ g_side,
                                                          float *__restrict__ g_h0p) {
    const int tpr = 1 << log_tpr, rpb = 256 >> log_tpr;
    const int c0 = (threadIdx.x & (tpr - 1)) * W;
    const float c = has_h0 ? 1.f - alpha : 1.f;
    for (long r = (long)blockIdx.x * rpb + (threadIdx.x >> log_tpr); r < n; r += (long)gridDim.x * rpb)
        for (int col = c0; col < d; col += tpr * W) {
            float e[W], s[W], gs[W], gp[W], ge[W], gsd[W], gh[W];
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(e) = *reinterpret_cast<const float4 *>(ego + r * lde + col);
                *reinterpret_cast<float4 *>(s) = *reinterpret_cast<const float4 *>(side + r * lds + col);
                *reinterpret_cast<float4 *>(gs) = *reinterpret_cast<const float4 *>(g_sum + r * ldgs + col);
                *reinterpret_cast<float4 *>(gp) = *reinterpret_cast<const float4 *>(g_prod + r * ldgp + col);
            } else {
                e[0] = ego[r * lde + col];
                s[0] = side[r * lds + col];
                gs[0] = g_sum[r * ldgs + col];
                gp[0] = g_prod[r * ldgp + col];
            }
#pragma unroll
            for (int k = 0; k < W; ++k) {
                ge[k] = c * fmaf(gp[k], s[k], gs[k]);
                gsd[k] = c * fmaf(gp[k], e[k], gs[k]);
                gh[k] = alpha * (gs[k] + gp[k]);
            }
            const long o = r * (long)d + col;          // (the three gradients are dense n x d tensors of this call)
            if constexpr (W == 4) {
                *reinterpret_cast<float4 *>(g_ego + o) = *reinterpret_cast<float4 *>(ge);
                *reinterpret_cast<float4 *>(g_side + o) = *reinterpret_cast<float4 *>(gsd);
                if (g_h0p) *reinterpret_cast<float4 *>(g_h0p + o) = *reinterpret_cast<float4 *>(gh);
            } else {
                g_ego[o] = ge[0];
                g_side[o] = gsd[0];
                if (g_h0p) g_h0p[o] = gh[0];
            }
        }
}
}  // namespace

extern "C" int lkg_bi_mix_fwd_f32(int64_t n, int32_t d, const float *ego, int64_t lde, const float *side, int64_t lds,
                                  const float *h0p, int64_t ldh, float alpha, float *out_sum, int64_t ldos, float *out_prod,
                                  int64_t ldop, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && lde >= d && lds >= d && ldos >= d && ldop >= d && (!h0p || ldh >= d), "lkg_bi_mix_fwd_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(ego && side && out_sum && out_prod, "lkg_bi_mix_fwd_f32: null pointer");
    const bool vec = d % 4 == 0 && lde % 4 == 0 && lds % 4 == 0 && ldos % 4 == 0 && ldop % 4 == 0 && (!h0p || ldh % 4 == 0) &&
                     lkg_aligned16(ego) && lkg_aligned16(side) && lkg_aligned16(out_sum) && lkg_aligned16(out_prod) &&
                     (!h0p || lkg_aligned16(h0p));
    const int lt = log_threads_per_row(vec ? d / 4 : d);
    const int64_t blocks = std::min<int64_t>((n + (256 >> lt) - 1) / (256 >> lt), 256 * 32);
    if (vec)
        hipLaunchKernelGGL(bi_mix_fwd_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, d, lt, ego,
                           (long)lde, side, (long)lds, h0p, (long)ldh, alpha, out_sum, (long)ldos, out_prod, (long)ldop);
    else
        hipLaunchKernelGGL(bi_mix_fwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, d, lt, ego,
                           (long)lde, side, (long)lds, h0p, (long)ldh, alpha, out_sum, (long)ldos, out_prod, (long)ldop);
    LKG_CHECK_LAUNCH("lkg_bi_mix_fwd_f32");
    return LKG_OK;
}

extern "C" int lkg_bi_mix_bwd_f32(int64_t n, int32_t d, const float *ego, int64_t lde, const float *side, int64_t lds,
                                  const float *g_sum, int64_t ldgs, const float *g_prod, int64_t ldgp, int32_t has_h0,
                                  float alpha, float *g_ego, float *g_side, float *g_h0p, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && lde >= d && lds >= d && ldgs >= d && ldgp >= d, "lkg_bi_mix_bwd_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(ego && side && g_sum && g_prod && g_ego && g_side && (!has_h0 || g_h0p), "lkg_bi_mix_bwd_f32: null pointer");
    const bool vec = d % 4 == 0 && lde % 4 == 0 && lds % 4 == 0 && ldgs % 4 == 0 && ldgp % 4 == 0 && lkg_aligned16(ego) &&
                     lkg_aligned16(side) && lkg_aligned16(g_sum) && lkg_aligned16(g_prod) && lkg_aligned16(g_ego) &&
                     lkg_aligned16(g_side) && (!g_h0p || lkg_aligned16(g_h0p));
    const int lt = log_threads_per_row(vec ? d / 4 : d);
    const int64_t blocks = std::min<int64_t>((n + (256 >> lt) - 1) / (256 >> lt), 256 * 32);
    if (vec)
        hipLaunchKernelGGL(bi_mix_bwd_kernel<4>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, d, lt, ego,
                           (long)lde, side, (long)lds, g_sum, (long)ldgs, g_prod, (long)ldgp, (int)has_h0, alpha, g_ego, g_side,
                           has_h0 ? g_h0p : nullptr);
    else
        hipLaunchKernelGGL(bi_mix_bwd_kernel<1>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, d, lt, ego,
                           (long)lde, side, (long)lds, g_sum, (long)ldgs, g_prod, (long)ldgp, (int)has_h0, alpha, g_ego, g_side,
                           has_h0 ? g_h0p : nullptr);
    LKG_CHECK_LAUNCH("lkg_bi_mix_bwd_f32");
    return LKG_OK;
}

// lkg_preload(): HIP loads a translation unit's code object on the first use of one of its kernels; asking for a kernel's
// attributes is such a use (no launch).
int lkg_internal_preload_rowwise() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&gate_stats_finish_kernel)) == hipSuccess ? 0 : 1;
}
