// Ordered split-K fp32 GEMM: long reductions into small outputs, spread over the chip WITHOUT atomics, bit for bit repeatable
// (include/literalkg_hip.h states the contract).
//
//   C[m,n] = alpha * sum_k opA(A)[m,k] * opB(B)[k,n] + beta * C[m,n] (+ bias[n])
//
// Two launches.  The partial kernel runs a grid of (output tiles) x (S_eff k-splits); split z walks
// k in [z * per, min(k, (z + 1) * per)) on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: one k-ordered fmaf chain per
// element from 0.0, as lkg_gemm.hip's f32 engine) and stores its 128 x 128 partial with plain vector stores into
// workspace[z][m][n].  The reduce kernel then forms, per element, s = ((p_0 + p_1) + p_2) + ... in ascending z and applies
// ordered_finish() below.  With S_eff = 1 the partial kernel applies ordered_finish() itself and no workspace is touched.
// No atomics, no arrival counters, nothing spins: the order of every addition is fixed by (k, per) alone.
//
// Tiling and LDS images are those of lkg_gemm.hip's f32 engine (128 x 128 x 16 block tile, 4 waves in 2 x 2, each 2 x 2
// MFMA 32x32 accumulators; a K-contiguous operand as a [row][k] image of pitch 20, an M/N-contiguous one as [k][col] of
// pitch 132; inside a group of 8 k the four MFMAs take k = j on lanes 0-31 and k = 4 + j on lanes 32-63).  The two loader
// structs are restated here because lkg_gemm.hip's device code is pinned as it stands.  Every split starts on a multiple
// of 16 = BK, so a split's chain is the chain an unsplit product over the same k-slice runs: that is what "the partials,
// added in ascending z" can be tested against.
#include <algorithm>
#include <type_traits>

#include "lkg_common.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 16;
constexpr int EPT = BK / 2;      // floats per thread per operand tile (128 * BK / 256)
constexpr int PK = BK + 4;       // pitch of a [row][k] image
constexpr int PM = BM + 4;       // pitch of a [k][col] image
constexpr int IMG = (BM * PK > BK * PM) ? BM * PK : BK * PM;   // floats per operand image
constexpr int MAX_SPLITS = 256;
constexpr long MAX_WORKSPACE = 256L << 20;
typedef float f32x16 __attribute__((ext_vector_type(16)));

struct OrderedArgs {
    long m, n, k, per;
    float alpha, beta;
    const float *a;
    long lda;
    const float *b;
    long ldb;
    float *c;
    long ldc;
    const float *bias;
    float *ws;           // [s_eff][m][n], or null with s_eff == 1
    int s_eff;
    int tiles_n;
};

// The one float32 expression behind every output element (s: the ordered sum of the partials; bias 0.0f without one):
//     t   = fmaf(alpha, s, bias)
//     out = beta == 0 ? t : fmaf(beta, c_old, t)          (c_old is not read when beta == 0)
__device__ __forceinline__ float ordered_finish(float s, float alpha, float beta, float c_old, float bias) {
    const float t = fmaf(alpha, s, bias);
    return beta == 0.f ? t : fmaf(beta, c_old, t);
}

// K-contiguous operand: element (r, k) at src[r * ld + k]; LDS image [r][k].  Thread t owns row t/2 and EPT = 8 consecutive k.
struct KContig {
    float v[EPT];
    __device__ __forceinline__ void load(const float *src, long ld, long r0, long r_end, long k0, long k_end, int t, bool fast) {
        const long r = r0 + (t >> 1);
        const long k = k0 + (t & 1) * EPT;
        if (fast) {
            const float4 *p = reinterpret_cast<const float4 *>(src + r * ld + k);
#pragma unroll
            for (int q = 0; q < EPT / 4; ++q) {
                const float4 x = p[q];
                v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            }
        } else {
            // edge tile / unaligned operand: clamped address + select, no load outside [0, r_end) x [0, k_end)
            const float *row = src + min(r, r_end - 1) * ld;
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                const float x = row[min(k + j, k_end - 1)];
                v[j] = (r < r_end && k + j < k_end) ? x : 0.f;
            }
        }
    }
    __device__ __forceinline__ void store(float *lds, int t) const {
        float *p = lds + (t >> 1) * PK + (t & 1) * EPT;
#pragma unroll
        for (int q = 0; q < EPT / 4; ++q)
            *reinterpret_cast<float4 *>(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
    static __device__ __forceinline__ float4 frag(const float *lds, int r0, int g, int lane) {
        return *reinterpret_cast<const float4 *>(lds + (r0 + (lane & 31)) * PK + 8 * g + (lane >> 5) * 4);
    }
};

// M/N-contiguous operand: element (k, c) at src[k * ld + c]; LDS image [k][c].  Thread t owns k = t/16 and 8 consecutive columns.
struct MContig {
    static constexpr int TPK = BM / EPT;   // threads per k-row
    float v[EPT];
    __device__ __forceinline__ void load(const float *src, long ld, long c0, long c_end, long k0, long k_end, int t, bool fast) {
        const long k = k0 + t / TPK;
        const long c = c0 + (t % TPK) * EPT;
        if (fast) {
            const float4 *p = reinterpret_cast<const float4 *>(src + k * ld + c);
#pragma unroll
            for (int q = 0; q < EPT / 4; ++q) {
                const float4 x = p[q];
                v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            }
        } else {
            const float *row = src + min(k, k_end - 1) * ld;
#pragma unroll
            for (int j = 0; j < EPT; ++j) {
                const float x = row[min(c + j, c_end - 1)];
                v[j] = (k < k_end && c + j < c_end) ? x : 0.f;
            }
        }
    }
    __device__ __forceinline__ void store(float *lds, int t) const {
        float *p = lds + (t / TPK) * PM + (t % TPK) * EPT;
#pragma unroll
        for (int q = 0; q < EPT / 4; ++q)
            *reinterpret_cast<float4 *>(p + 4 * q) = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    }
    static __device__ __forceinline__ float4 frag(const float *lds, int c0, int g, int lane) {
        const float *p = lds + (8 * g + (lane >> 5) * 4) * PM + c0 + (lane & 31);
        return make_float4(p[0], p[PM], p[2 * PM], p[3 * PM]);
    }
};

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void ordered_partial_kernel(OrderedArgs g) {
    __shared__ __attribute__((aligned(16))) float As[2][IMG];
    __shared__ __attribute__((aligned(16))) float Bs[2][IMG];
    using LA = typename std::conditional<TA, MContig, KContig>::type;
    using LB = typename std::conditional<TB, KContig, MContig>::type;

    const int t = threadIdx.x;
    const int lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const long tm = blockIdx.x / g.tiles_n, tn = blockIdx.x % g.tiles_n;
    const int z = blockIdx.y;
    const long m0 = tm * BM, n0 = tn * BN;
    const long k_lo = (long)z * g.per;
    const long k_hi = min(g.k, k_lo + g.per);       // (k == 0: an empty range, the accumulators stay 0.0)

    // unguarded 16-byte loads: an aligned operand and a tile that lies inside it (k_lo and every k0 are multiples of 16)
    const bool a_al = (g.lda % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.a) & 15) == 0);
    const bool b_al = (g.ldb % 4 == 0) && ((reinterpret_cast<uintptr_t>(g.b) & 15) == 0);
    const bool m_full = m0 + BM <= g.m, n_full = n0 + BN <= g.n;

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    LA la;
    LB lb;
    auto fetch = [&](long k0) {
        const bool k_full = k0 + BK <= k_hi;
        la.load(g.a, g.lda, m0, g.m, k0, k_hi, t, a_al && m_full && k_full);
        lb.load(g.b, g.ldb, n0, g.n, k0, k_hi, t, b_al && n_full && k_full);
    };

    int buf = 0;
    if (k_lo < k_hi) {
        fetch(k_lo);
        la.store(As[0], t);
        lb.store(Bs[0], t);
    }
    __syncthreads();
    for (long k0 = k_lo; k0 < k_hi; k0 += BK) {
        const bool more = k0 + BK < k_hi;
        if (more) fetch(k0 + BK);
#pragma unroll
        for (int grp = 0; grp < BK / 8; ++grp) {
            const float4 a0 = LA::frag(As[buf], wm * 64, grp, lane), a1 = LA::frag(As[buf], wm * 64 + 32, grp, lane);
            const float4 b0 = LB::frag(Bs[buf], wn * 64, grp, lane), b1 = LB::frag(Bs[buf], wn * 64 + 32, grp, lane);
#define LKG_STEP(F)                                                                         \
    acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b0.F, acc[0][0], 0, 0, 0);       \
    acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0.F, b1.F, acc[0][1], 0, 0, 0);       \
    acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b0.F, acc[1][0], 0, 0, 0);       \
    acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1.F, b1.F, acc[1][1], 0, 0, 0);
            LKG_STEP(x) LKG_STEP(y) LKG_STEP(z) LKG_STEP(w)
#undef LKG_STEP
        }
        if (more) {
            la.store(As[buf ^ 1], t);
            lb.store(Bs[buf ^ 1], t);
        }
        __syncthreads();
        buf ^= 1;
    }

    // C/D map of the 32x32 MFMA: col = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5).
    const bool direct = g.s_eff <= 1;       // one split: finish here; otherwise the bare partial goes to workspace[z]
    float *dst = direct ? g.c : g.ws + (long)z * g.m * g.n;
    const long ldd = direct ? g.ldc : g.n;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const long col = n0 + wn * 64 + j * 32 + (lane & 31);
            if (col >= g.n) continue;
            const long row0 = m0 + wm * 64 + i * 32 + 4 * (lane >> 5);
            float *dst0 = dst + row0 * ldd + col;
            float out[16];
#pragma unroll
            for (int r = 0; r < 16; ++r) out[r] = acc[i][j][r];
            if (direct) {
                const float bv = g.bias ? g.bias[col] : 0.f;
                float old[16];
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int dr = (r & 3) + 8 * (r >> 2);
                    old[r] = (g.beta != 0.f && row0 + dr < g.m) ? dst0[dr * ldd] : 0.f;
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) out[r] = ordered_finish(out[r], g.alpha, g.beta, old[r], bv);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int dr = (r & 3) + 8 * (r >> 2);
                if (row0 + dr < g.m) dst0[dr * ldd] = out[r];
            }
        }
}

// one thread per output element: the partials of ascending z, then ordered_finish()
__global__ __launch_bounds__(256) void ordered_reduce_kernel(long m, long n, int s_eff, const float *__restrict__ ws, float alpha,
                                                             float beta, float *__restrict__ c, long ldc,
                                                             const float *__restrict__ bias) {
    const long e = (long)blockIdx.x * 256 + threadIdx.x;
    const long mn = m * n;
    if (e >= mn) return;
    const long row = e / n, col = e % n;
    const float *p = ws + e;
    float s = p[0];
#pragma unroll 8
    for (int z = 1; z < s_eff; ++z) s = s + p[(long)z * mn];
    float *out = c + row * ldc + col;
    const float old = beta != 0.f ? *out : 0.f;
    *out = ordered_finish(s, alpha, beta, old, bias ? bias[col] : 0.f);
}

long per_of(long k, long splits) {
    if (k <= 0) return 0;
    const long q = (k + splits - 1) / splits;
    return (q + BK - 1) / BK * BK;
}

}  // namespace

extern "C" int64_t lkg_gemm_ordered_partition(int64_t k, int32_t splits, int64_t *per) {
    LKG_REQUIRE(k >= 0 && splits >= 1 && splits <= MAX_SPLITS, "lkg_gemm_ordered_partition: k = %lld, splits = %d (1 .. %d)",
                (long long)k, (int)splits, MAX_SPLITS);
    const long p = per_of(k, splits);
    if (per) *per = p;
    return p ? (k + p - 1) / p : 0;
}

extern "C" int32_t lkg_gemm_ordered_splits(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k) {
    (void)trans_a; (void)trans_b;       // the tiling is the same for the four layouts
    if (m <= 0 || n <= 0 || k <= 0) return 1;
    const long tiles = ((m + BM - 1) / BM) * ((n + BN - 1) / BN);
    long s = 512 / tiles;                                   // about two workgroups for each of the 256 CUs
    s = std::min<long>(s, k / 512);                         // no split shorter than 512 k
    s = std::min<long>(s, MAX_WORKSPACE / (4 * m * n));     // the partials fit 256 MB
    return (int32_t)std::max<long>(1, std::min<long>(s, MAX_SPLITS));
}

extern "C" int64_t lkg_gemm_ordered_workspace(int64_t m, int64_t n, int64_t k, int32_t splits) {
    LKG_REQUIRE(m >= 0 && n >= 0, "lkg_gemm_ordered_workspace: negative size");
    const int64_t s_eff = lkg_gemm_ordered_partition(k, splits, nullptr);
    if (s_eff < 0) return s_eff;
    return s_eff <= 1 ? 0 : s_eff * m * n * (int64_t)sizeof(float);
}

extern "C" int lkg_gemm_ordered_f32(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, int32_t splits,
                                    float alpha, const float *a, int64_t lda, const float *b, int64_t ldb, float beta,
                                    float *c, int64_t ldc, const float *bias, void *workspace, int64_t workspace_bytes,
                                    void *stream) {
    LKG_REQUIRE(m >= 0 && n >= 0 && k >= 0, "lkg_gemm_ordered_f32: negative size");
    LKG_REQUIRE(splits >= 1 && splits <= MAX_SPLITS, "lkg_gemm_ordered_f32: splits = %d outside [1, %d]", (int)splits, MAX_SPLITS);
    if (m == 0 || n == 0) return LKG_OK;
    LKG_REQUIRE(c && ldc >= n, "lkg_gemm_ordered_f32: bad C (ldc=%lld, n=%lld)", (long long)ldc, (long long)n);
    LKG_REQUIRE(k == 0 || (a && b), "lkg_gemm_ordered_f32: null operand");
    LKG_REQUIRE(k == 0 || (lda >= (trans_a ? m : k) && ldb >= (trans_b ? k : n)), "lkg_gemm_ordered_f32: leading dimension too small");
    OrderedArgs g{};
    g.m = m; g.n = n; g.k = k; g.alpha = alpha; g.beta = beta;
    g.a = a; g.lda = lda; g.b = b; g.ldb = ldb; g.c = c; g.ldc = ldc; g.bias = bias;
    int64_t per = 0;
    g.s_eff = (int)lkg_gemm_ordered_partition(k, splits, &per);
    g.per = per;
    const int64_t need = g.s_eff <= 1 ? 0 : (int64_t)g.s_eff * m * n * (int64_t)sizeof(float);
    LKG_REQUIRE(need == 0 || (workspace && workspace_bytes >= need), "lkg_gemm_ordered_f32: %lld bytes of workspace for %d "
                "partials of %lld x %lld, %lld given", (long long)need, g.s_eff, (long long)m, (long long)n,
                (long long)(workspace ? workspace_bytes : 0));
    g.ws = need ? static_cast<float *>(workspace) : nullptr;
    const long tiles_m = (m + BM - 1) / BM;
    g.tiles_n = (int)((n + BN - 1) / BN);
    const long tiles = tiles_m * g.tiles_n;
    LKG_REQUIRE(tiles < INT32_MAX && m * n < (1L << 39), "lkg_gemm_ordered_f32: too many tiles");
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles, (unsigned)std::max(g.s_eff, 1));
    if (!trans_a && !trans_b)
        hipLaunchKernelGGL((ordered_partial_kernel<false, false>), grid, dim3(256), 0, s, g);
    else if (!trans_a && trans_b)
        hipLaunchKernelGGL((ordered_partial_kernel<false, true>), grid, dim3(256), 0, s, g);
    else if (trans_a && !trans_b)
        hipLaunchKernelGGL((ordered_partial_kernel<true, false>), grid, dim3(256), 0, s, g);
    else
        hipLaunchKernelGGL((ordered_partial_kernel<true, true>), grid, dim3(256), 0, s, g);
    LKG_CHECK_LAUNCH("lkg_gemm_ordered_f32 (partials)");
    if (need) {
        hipLaunchKernelGGL(ordered_reduce_kernel, dim3((unsigned)((m * n + 255) / 256)), dim3(256), 0, s, (long)m, (long)n,
                           g.s_eff, g.ws, alpha, beta, c, (long)ldc, bias);
        LKG_CHECK_LAUNCH("lkg_gemm_ordered_f32 (reduce)");
    }
    return LKG_OK;
}

int lkg_internal_preload_gemm_ordered() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&ordered_reduce_kernel)) == hipSuccess ? 0 : 1;
}
