// Relation-slot training loss (literalkg_amd/relation_loss.py): the cross-entropy of the true relation of a pair (h, ?, t)
// against the softmax over every relation.  With u_ij the pair's block under relation j (slab mode: u_ij = d_i W_j, row i
// of the product D @ Wcat, block j at u + i * ldu + j * rel_stride; shared mode, rel_stride == 0: u_ij = d_i for every j)
//     s_ij = sum_c (u_ijc + e_jc)^2,   z_ij = -scale s_ij,   loss_i = logsumexp_j z_ij - z_i,truth_i
// over the eligible relations: with a filter (lkg_known.h) every relation other than the truth under which the pair is
// known is stored as -inf.  DESIGN.md 3.6s.
//
// Tiling: one wave per pair, four waves per workgroup, a grid-stride loop under a grid cap.  A lane owns the 4-column units
// lane, lane + 64, ... of a k-wide block (one 16-byte load each where k, the strides and the pointers allow it; four
// guarded scalar loads otherwise, into the SAME lane and the SAME order: the two paths give the same bits).  Shared mode
// keeps the pair's row in registers across the relations (the first 512 columns; a wider row's remaining units are
// re-read through the cache).
//
// Forward, per relation: one fma chain per lane in unit order over u + e, one butterfly, lane 0 stores z_ij.  After a
// wavefront fence the filter's relations are overwritten with -inf (never the truth; duplicates write the same bits), and
// after another the wave reads its row of logits back in three lane-strided passes, each ended by a butterfly:
// m = max_j z_ij, sum = sum_j expf(z_ij - m), and z_t; then lse = m + logf(sum),
// loss = (m - z_t) + logf(sum) -- exactly 0 where the truth is the only eligible relation (m = z_t, sum = 1).  Any
// n_rel >= 1: the lanes loop, nothing is sized by the wave or by LDS.
//
// Backward: the wave takes m and sum from its stored row again, by the forward's own two passes (the same bits), and
// c_ij = cg (expf(z_ij - m) / sum - [j == truth_i]) with cg = fl(-2 scale * g_i), exactly 0 where z_ij = -inf (the stored
// -inf carries the filter: it is not looked up again).  expf(z_ij - lse_i) would be one operation less, and would carry
// half an ulp of lse -- 32 u at |lse| in [32, 64) -- into every softmax as a RELATIVE error.  Slab mode rewrites every
// block in place as c_ij (u_ij + e_j), each element loaded and stored once (a dropped relation's block is stored as
// zeros, not multiplied); shared mode adds
// c_ij (d_i + e_j) in increasing j into registers, per 512-column tile, and stores c.  No atomics; a pair's outputs depend
// on its own blocks, e, its truth and its filter entry alone.
// Floating-point contraction is off in this file: every rounding is one the references count.
#include "lkg_common.h"
#include "lkg_known.h"

#pragma clang fp contract(off)

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_WAVES = RL_THREADS / 64;   // pairs per workgroup and trip: one per wave
constexpr int RL_RU = 2;                    // 4-column units of a row a lane keeps in registers (2 x 64 x 4 = 512 columns)
constexpr long RL_GRID = 4096;              // workgroups at most (256 CUs x 8 resident, twice over)

// columns 4 u .. 4 u + 3 of a row, 4 u < k (zeros past k)
template <bool VEC>
__device__ __forceinline__ float4 load_unit(const float *__restrict__ row, int u, int k) {
    if constexpr (VEC) {
        return reinterpret_cast<const float4 *>(row)[u];
    } else {
        const int c = 4 * u, last = k - 1;              // (4 u < k; a column past k re-reads column k - 1 and is dropped:
        const float x = row[c];                         //  selects, no branches)
        const float y = row[c + 1 < k ? c + 1 : last], z = row[c + 2 < k ? c + 2 : last], w = row[c + 3 < k ? c + 3 : last];
        return make_float4(x, c + 1 < k ? y : 0.f, c + 2 < k ? z : 0.f, c + 3 < k ? w : 0.f);
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

// s += (a + b)^2 over the unit's four columns, in column order
__device__ __forceinline__ void sq_unit(float &s, const float4 &a, const float4 &b) {
    const float x = a.x + b.x, y = a.y + b.y, z = a.z + b.z, w = a.w + b.w;
    s = fmaf(x, x, s);
    s = fmaf(y, y, s);
    s = fmaf(z, z, s);
    s = fmaf(w, w, s);
}

// (m, sum) of a stored row of logits, as the forward kernel takes them: m = max_j z_j, sum = sum_j expf(z_j - m), a lane's
// entries j = lane, lane + 64, ... in order and one butterfly each
__device__ __forceinline__ void rl_row_stats(const float *zrow, int n_rel, int lane, float &m, float &sum) {
    m = -__builtin_inff();
    for (int j = lane; j < n_rel; j += 64) m = fmaxf(m, zrow[j]);
    m = wave_max(m);
    sum = 0.f;
    for (int j = lane; j < n_rel; j += 64) sum += expf(zrow[j] - m);
    sum = wave_sum(sum);
}

// c_ij of the kept logit; exactly 0 for a dropped relation
__device__ __forceinline__ float rl_coeff(float zij, float m, float sum, float cg, bool is_truth) {
    const float a = expf(zij - m) / sum - (is_truth ? 1.f : 0.f);
    return zij == -__builtin_inff() ? 0.f : cg * a;
}

template <bool VEC, bool SHARED>
__global__ __launch_bounds__(RL_THREADS) void relation_loss_fwd_kernel(
    long n, int n_rel, int k, const float *__restrict__ u, long ldu, long rel_stride, const float *__restrict__ e, long lde,
    const long *__restrict__ truth, const long *__restrict__ filter_row, const long *__restrict__ filter_col,
    const int *__restrict__ rowptr, const int *__restrict__ col, const int *__restrict__ eptr,
    const int *__restrict__ rel, float scale, float *z, long ldz, float *__restrict__ lse, float *__restrict__ loss) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nu = (k + 3) >> 2;
    for (long i = (long)blockIdx.x * RL_WAVES + wave; i < n; i += (long)gridDim.x * RL_WAVES) {   // (uniform in the wave)
        const float *urow = u + i * ldu;
        float *zrow = z + i * ldz;
        float4 dv[RL_RU];
        if constexpr (SHARED) {
#pragma unroll
            for (int a = 0; a < RL_RU; ++a) {
                const int x = lane + 64 * a;
                dv[a] = x < nu ? load_unit<VEC>(urow, x, k) : f4_zero();
            }
        }
        for (int j = 0; j < n_rel; ++j) {
            const float *blk = SHARED ? urow : urow + (long)j * rel_stride;
            const float *erow = e + (long)j * lde;
            float s = 0.f;
#pragma unroll
            for (int a = 0; a < RL_RU; ++a) {
                const int x = lane + 64 * a;
                if (x < nu) {
                    float4 v;
                    if constexpr (SHARED) v = dv[a];
                    else v = load_unit<VEC>(blk, x, k);
                    sq_unit(s, v, load_unit<VEC>(erow, x, k));
                }
            }
            for (int x = lane + 64 * RL_RU; x < nu; x += 64)      // (a block wider than 512 columns)
                sq_unit(s, load_unit<VEC>(blk, x, k), load_unit<VEC>(erow, x, k));
            s = wave_sum(s);
            if (lane == 0) zrow[j] = -(scale * s);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");        // the row of logits is in memory, visible to the wave
        const long tj = truth[i];
        if (rowptr) {
            const long f = filter_row[i];
            const long want = filter_col[i];
            int en;
            if (known_find(col, rowptr[f], rowptr[f + 1], want, en)) {
                const int x1 = eptr[en + 1];
                for (int x = eptr[en] + lane; x < x1; x += 64) {
                    const int rr = rel[x];
                    if (rr >= 0 && rr < n_rel && rr != tj) zrow[rr] = -__builtin_inff();   // (duplicates write the same bits)
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        float m, sum;
        rl_row_stats(zrow, n_rel, lane, m, sum);
        float zt = -__builtin_inff();
        for (int j = lane; j < n_rel; j += 64)
            if (j == tj) zt = zrow[j];
        zt = wave_max(zt);                                            // (one lane holds it, the others -inf)
        const float lg = logf(sum);
        if (lane == 0) {
            lse[i] = m + lg;
            loss[i] = (m - zt) + lg;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(RL_THREADS) void relation_loss_bwd_slab_kernel(
    long n, int n_rel, int k, float *__restrict__ u, long ldu, long rel_stride, const float *__restrict__ e, long lde,
    const long *__restrict__ truth, float scale, const float *__restrict__ g, const float *__restrict__ z, long ldz) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nu = (k + 3) >> 2;
    for (long i = (long)blockIdx.x * RL_WAVES + wave; i < n; i += (long)gridDim.x * RL_WAVES) {
        const float cg = (-2.f * scale) * g[i];
        const long tj = truth[i];
        const float *zrow = z + i * ldz;
        float m, sum;
        rl_row_stats(zrow, n_rel, lane, m, sum);
#pragma unroll 2
        for (int j = 0; j < n_rel; ++j) {
            float *blk = u + i * ldu + (long)j * rel_stride;
            const float *erow = e + (long)j * lde;
            const float zij = zrow[j];
            const float c = rl_coeff(zij, m, sum, cg, j == tj);
            const bool dropped = zij == -__builtin_inff();            // (uniform in the wave)
            for (int x = lane; x < nu; x += 64) {
                float4 o = f4_zero();
                if (!dropped) {
                    const float4 v = load_unit<VEC>(blk, x, k), ev = load_unit<VEC>(erow, x, k);
                    o = make_float4(c * (v.x + ev.x), c * (v.y + ev.y), c * (v.z + ev.z), c * (v.w + ev.w));
                }
                store_unit<VEC>(blk, x, k, o);
            }
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(RL_THREADS) void relation_loss_bwd_shared_kernel(
    long n, int n_rel, int k, const float *__restrict__ d, long ldd, const float *__restrict__ e, long lde,
    const long *__restrict__ truth, float scale, const float *__restrict__ g, const float *__restrict__ z, long ldz,
    float *__restrict__ gd, long ldgd, float *__restrict__ c, long ldc) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nu = (k + 3) >> 2;
    for (long i = (long)blockIdx.x * RL_WAVES + wave; i < n; i += (long)gridDim.x * RL_WAVES) {
        const float cg = (-2.f * scale) * g[i];
        const long tj = truth[i];
        const float *zrow = z + i * ldz;
        float m, sum;
        rl_row_stats(zrow, n_rel, lane, m, sum);
        const float *drow = d + i * ldd;
        for (int u0 = 0; u0 < nu; u0 += 64 * RL_RU) {                // 512 columns at a time
            float4 dv[RL_RU], acc[RL_RU];
#pragma unroll
            for (int a = 0; a < RL_RU; ++a) {
                const int x = u0 + lane + 64 * a;
                dv[a] = (gd && x < nu) ? load_unit<VEC>(drow, x, k) : f4_zero();
                acc[a] = f4_zero();
            }
#pragma unroll 2
            for (int j = 0; j < n_rel; ++j) {
                const float zij = zrow[j];
                const float cij = rl_coeff(zij, m, sum, cg, j == tj);
                if (c && u0 == 0 && lane == 0) c[i * ldc + j] = cij;
                if (!gd || zij == -__builtin_inff()) continue;       // (uniform) a dropped relation adds nothing
                const float *erow = e + (long)j * lde;
#pragma unroll
                for (int a = 0; a < RL_RU; ++a) {
                    const int x = u0 + lane + 64 * a;
                    if (x < nu) {
                        const float4 ev = load_unit<VEC>(erow, x, k);
                        acc[a].x += cij * (dv[a].x + ev.x);
                        acc[a].y += cij * (dv[a].y + ev.y);
                        acc[a].z += cij * (dv[a].z + ev.z);
                        acc[a].w += cij * (dv[a].w + ev.w);
                    }
                }
            }
            if (!gd) break;                                           // (uniform) only c was asked for
#pragma unroll
            for (int a = 0; a < RL_RU; ++a) {
                const int x = u0 + lane + 64 * a;
                if (x < nu) store_unit<VEC>(gd + i * ldgd, x, k, acc[a]);
            }
        }
    }
}

bool vec4_ok(int k, const void *ptr, int64_t ld) { return !ptr || (k % 4 == 0 && ld % 4 == 0 && lkg_aligned16(ptr)); }

dim3 rl_grid(int64_t n) {
    const long blocks = (n + RL_WAVES - 1) / RL_WAVES;
    return dim3((unsigned)(blocks < RL_GRID ? blocks : RL_GRID));
}

bool rl_sizes_ok(int64_t n, int32_t n_rel, int32_t k, int64_t ldu, int64_t rel_stride, int64_t lde, int64_t ldz) {
    return n >= 0 && n <= (int64_t)INT32_MAX - 1 && n_rel >= 1 && k >= 1 && rel_stride >= 0 && lde >= k && ldz >= n_rel &&
           (rel_stride == 0 ? ldu >= k : rel_stride >= k && ldu >= (int64_t)(n_rel - 1) * rel_stride + k);
}

}  // namespace

extern "C" int lkg_relation_loss_fwd_f32(int64_t n, int32_t n_rel, int32_t k, const float *u, int64_t ldu,
                                         int64_t rel_stride, const float *e, int64_t lde, const int64_t *truth,
                                         const int64_t *filter_row, const int64_t *filter_col, const int32_t *rowptr,
                                         const int32_t *col, const int32_t *eptr, const int32_t *rel, float scale, float *z,
                                         int64_t ldz, float *lse, float *loss, void *stream) {
    LKG_REQUIRE(rl_sizes_ok(n, n_rel, k, ldu, rel_stride, lde, ldz),
                "lkg_relation_loss_fwd_f32: bad sizes (n >= 0, n_rel >= 1, k >= 1, lde >= k, ldz >= n_rel; rel_stride 0 with "
                "ldu >= k, or rel_stride >= k with ldu >= (n_rel - 1) rel_stride + k)");
    LKG_REQUIRE(scale > 0.f && scale < __builtin_inff(), "lkg_relation_loss_fwd_f32: scale must be positive and finite");
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_col, col, eptr, rel),
                "lkg_relation_loss_fwd_f32: a filter needs filter_row, filter_col, col, eptr and rel (null pointer)");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(u && e && truth && z && lse && loss, "lkg_relation_loss_fwd_f32: null pointer");
    const dim3 grid = rl_grid(n), block(RL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec4_ok(k, u, ldu) && vec4_ok(k, e, lde) && rel_stride % 4 == 0;
#define LKG_RL_FWD(V, S)                                                                                               \
    hipLaunchKernelGGL((relation_loss_fwd_kernel<V, S>), grid, block, 0, s, (long)n, (int)n_rel, (int)k, u, (long)ldu, \
                       (long)rel_stride, e, (long)lde, (const long *)truth, (const long *)filter_row,                  \
                       (const long *)filter_col, rowptr, col, eptr, rel, scale, z, (long)ldz, lse, loss)
    if (vec) {
        if (rel_stride == 0) LKG_RL_FWD(true, true);
        else LKG_RL_FWD(true, false);
    } else {
        if (rel_stride == 0) LKG_RL_FWD(false, true);
        else LKG_RL_FWD(false, false);
    }
#undef LKG_RL_FWD
    LKG_CHECK_LAUNCH("lkg_relation_loss_fwd_f32");
    return LKG_OK;
}

extern "C" int lkg_relation_loss_bwd_f32(int64_t n, int32_t n_rel, int32_t k, float *u, int64_t ldu, int64_t rel_stride,
                                         const float *e, int64_t lde, const int64_t *truth, float scale, const float *g,
                                         const float *z, int64_t ldz, float *gd, int64_t ldgd, float *c, int64_t ldc,
                                         void *stream) {
    LKG_REQUIRE(rl_sizes_ok(n, n_rel, k, ldu, rel_stride, lde, ldz) && (!gd || ldgd >= k) && (!c || ldc >= n_rel),
                "lkg_relation_loss_bwd_f32: bad sizes (n >= 0, n_rel >= 1, k >= 1, lde >= k, ldz >= n_rel, ldgd >= k, "
                "ldc >= n_rel; rel_stride 0 with ldu >= k, or rel_stride >= k with ldu >= (n_rel - 1) rel_stride + k)");
    LKG_REQUIRE(scale > 0.f && scale < __builtin_inff(), "lkg_relation_loss_bwd_f32: scale must be positive and finite");
    LKG_REQUIRE(rel_stride == 0 || (!gd && !c),
                "lkg_relation_loss_bwd_f32: slab mode (rel_stride > 0) rewrites u in place and takes no gd and no c");
    if (n == 0 || (rel_stride == 0 && !gd && !c)) return LKG_OK;
    LKG_REQUIRE(u && e && truth && g && z, "lkg_relation_loss_bwd_f32: null pointer");
    const dim3 grid = rl_grid(n), block(RL_THREADS);
    hipStream_t s = (hipStream_t)stream;
    const bool vec = vec4_ok(k, u, ldu) && vec4_ok(k, e, lde) && vec4_ok(k, gd, ldgd) && rel_stride % 4 == 0;
    if (rel_stride != 0) {
        if (vec)
            hipLaunchKernelGGL(relation_loss_bwd_slab_kernel<true>, grid, block, 0, s, (long)n, (int)n_rel, (int)k, u,
                               (long)ldu, (long)rel_stride, e, (long)lde, (const long *)truth, scale, g, z, (long)ldz);
        else
            hipLaunchKernelGGL(relation_loss_bwd_slab_kernel<false>, grid, block, 0, s, (long)n, (int)n_rel, (int)k, u,
                               (long)ldu, (long)rel_stride, e, (long)lde, (const long *)truth, scale, g, z, (long)ldz);
    } else {
        if (vec)
            hipLaunchKernelGGL(relation_loss_bwd_shared_kernel<true>, grid, block, 0, s, (long)n, (int)n_rel, (int)k,
                               (const float *)u, (long)ldu, e, (long)lde, (const long *)truth, scale, g, z, (long)ldz,
                               gd, (long)ldgd, c, (long)ldc);
        else
            hipLaunchKernelGGL(relation_loss_bwd_shared_kernel<false>, grid, block, 0, s, (long)n, (int)n_rel, (int)k,
                               (const float *)u, (long)ldu, e, (long)lde, (const long *)truth, scale, g, z, (long)ldz,
                               gd, (long)ldgd, c, (long)ldc);
    }
    LKG_CHECK_LAUNCH("lkg_relation_loss_bwd_f32");
    return LKG_OK;
}

int lkg_internal_preload_relation_loss() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&relation_loss_fwd_kernel<true, false>)) == hipSuccess
               ? 0 : 1;
}
