// Explicit triples under the model's own score (literalkg_amd/triples.py: score_triples, fit_triple_thresholds,
// evaluate_triple_classification).  Triple i is (query row q_idx[i], candidate row c_idx[i]) of one table of rows p --
// P_r for 'transr', the inference table otherwise -- and its score is the one lkg_rank_count_f32 compares and
// lkg_topk_merge_f32 reports for that (query, candidate): the same bits.
//
// Arithmetic: load4 / mfma_chunk of lkg_rank_common.h with the unchanged lane -> k map and zero padding.  A wave owns 16
// triples per step; lane (r, s) = (l & 15, l >> 4) loads k-slice s of ITS triple r's query row and candidate row, so
// row r of the A operand is triple r's query and column r of B its candidate (the PmOwnX idea of lkg_pairmlp.hip).  The
// diagonal C[r][r] = q_r . p_r sits in lane (r, s = r >> 2), accumulator element r & 3.  Every output element of
// v_mfma_f32_16x16x4_f32 is a k-ordered fma chain that does not depend on its place in the tile, so the diagonal carries
// the bits the counting and selecting kernels compare; the 240 off-diagonal products are the price (the matrix pipe is
// not the bound: the kernel gathers two k-float rows per triple from HBM).
//
// The query is formed in-lane as fmaf(alpha, e_r[c], x[c]), the one rounding lkg_rank_queries_f32 makes.  |q|^2 for the
// reported squared distance reproduces lkg_rank_sqnorm_f32's order of operations on that row (lane c takes elements c,
// c + 64, ... as one fma chain, then wave_sum), one triple of the wave at a time: the rows were read a moment ago, so this
// second pass is served by the caches, and the queries are never materialised.
//
// No MFMA sits inside a divergent branch and the trip count is uniform in the workgroup: triples past the end are clamped
// to the last triple, computed, and neither stored nor counted.
#include "lkg_rank_common.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_TRIPLES = 64;                   // per workgroup and trip: 4 waves x 16
constexpr long TS_GRID = 4096;                   // workgroups at most

constexpr int TS_REPORTED = 1;                   // flags: out = |q|^2 + s (pn given) or -s / 2 (dot); else s itself
constexpr int TS_HIGHER = 2;                     //        positive iff out >= thr; else iff out <= thr

template <bool VEC>
__device__ __forceinline__ float4 query4(const float *__restrict__ x, const float *__restrict__ er, float alpha, int kk,
                                         int k) {
    float4 a = load4<VEC>(x, kk, k);
    if (er) {
        const float4 ev = load4<VEC>(er, kk, k);
        a.x = __builtin_fmaf(alpha, ev.x, a.x);
        a.y = __builtin_fmaf(alpha, ev.y, a.y);
        a.z = __builtin_fmaf(alpha, ev.z, a.z);
        a.w = __builtin_fmaf(alpha, ev.w, a.w);
    }
    return a;
}

// counts[0..4] += tp, fp, tn, fn, nan: per lane in registers, per workgroup in LDS, then one 64-bit atomic per non-zero
// count and workgroup (integers: no order enters).
template <bool VEC>
__global__ __launch_bounds__(TS_THREADS) void triple_scores_kernel(
    long n, int k, const float *__restrict__ p, long ldp, const long *__restrict__ q_idx, const long *__restrict__ c_idx,
    const float *__restrict__ pn, const float *__restrict__ e, long lde, const long *__restrict__ rel, float alpha,
    int flags, const unsigned char *__restrict__ labels, float thr, float *__restrict__ out,
    unsigned long long *__restrict__ counts) {
    __shared__ int cnt[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    if (tid < 5) cnt[tid] = 0;
    const bool want_qn = (flags & TS_REPORTED) && pn;                 // (uniform: kernel arguments)
    int n_tp = 0, n_fp = 0, n_tn = 0, n_fn = 0, n_nan = 0;
    for (long base = (long)blockIdx.x * TS_TRIPLES; base < n; base += (long)gridDim.x * TS_TRIPLES) {
        const long t0 = base + wave * 16;
        const long tr = t0 + r < n ? t0 + r : n - 1;
        const long qi = q_idx[tr], ci = c_idx[tr];
        const long ri = (e && rel) ? rel[tr] : 0L;
        const float *xrow = p + qi * ldp;
        const float *crow = p + ci * ldp;
        const float *erow = e ? e + ri * lde : nullptr;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        float4 a = query4<VEC>(xrow, erow, alpha, 4 * s, k);
        float4 b = load4<VEC>(crow, 4 * s, k);
        for (int k0 = 0; k0 < k; k0 += 16) {
            const int kn = k0 + 16 + 4 * s;
            const bool more = k0 + 16 < k;
            const float4 an = more ? query4<VEC>(xrow, erow, alpha, kn, k) : f4_zero();   // in flight during the MFMAs
            const float4 bn = more ? load4<VEC>(crow, kn, k) : f4_zero();
            mfma_chunk(acc, a, b);
            a = an;
            b = bn;
        }
        float qn = 0.f;
        if (want_qn) {
            for (int j = 0; j < 16; ++j) {                            // triple j of the wave, rank_sqnorm_kernel's order
                const long qj = __shfl(qi, j, 64), rj = __shfl(ri, j, 64);
                const float *x = p + qj * ldp;
                const float *er = e ? e + rj * lde : nullptr;
                float sq = 0.f;
                for (int c = lane; c < k; c += 64) {
                    const float y = er ? __builtin_fmaf(alpha, er[c], x[c]) : x[c];
                    sq = __builtin_fmaf(y, y, sq);
                }
                sq = wave_sum(sq);
                if (r == j) qn = sq;
            }
        }
        if (s == (r >> 2) && t0 + r < n) {                            // the diagonal: C[r][r] = acc[r & 3] of lane (r, r >> 2)
            const int v = r & 3;
            const float dot = v == 0 ? acc[0] : v == 1 ? acc[1] : v == 2 ? acc[2] : acc[3];
            const float sc = rank_score(dot, pn, ci);
            const float val = (flags & TS_REPORTED) ? (pn ? qn + sc : -0.5f * sc) : sc;
            if (out) out[t0 + r] = val;
            if (counts) {
                const bool one = labels[t0 + r] != 0, nan = val != val;
                const bool pos = (flags & TS_HIGHER) ? val >= thr : val <= thr;
                n_nan += nan;
                n_tp += !nan && pos && one;
                n_fp += !nan && pos && !one;
                n_tn += !nan && !pos && !one;
                n_fn += !nan && !pos && one;
            }
        }
    }
    if (!counts) return;                                              // (uniform: a kernel argument)
    __syncthreads();
    if (n_tp) atomicAdd(&cnt[0], n_tp);
    if (n_fp) atomicAdd(&cnt[1], n_fp);
    if (n_tn) atomicAdd(&cnt[2], n_tn);
    if (n_fn) atomicAdd(&cnt[3], n_fn);
    if (n_nan) atomicAdd(&cnt[4], n_nan);
    __syncthreads();
    if (tid < 5 && cnt[tid]) atomicAdd(counts + tid, (unsigned long long)cnt[tid]);
}

}  // namespace

extern "C" int lkg_triple_scores_f32(int64_t n, int32_t k, const float *p, int64_t ldp, const int64_t *q_idx,
                                     const int64_t *c_idx, const float *pn, const float *e, int64_t lde,
                                     const int64_t *rel, float alpha, int32_t flags, const uint8_t *labels, float thr,
                                     float *out, int64_t *counts, void *stream) {
    LKG_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX - 1 && k > 0 && ldp >= k && (!e || lde >= k),
                "lkg_triple_scores_f32: bad sizes");
    LKG_REQUIRE((flags & ~(TS_REPORTED | TS_HIGHER)) == 0, "lkg_triple_scores_f32: unknown flags");
    LKG_REQUIRE(out || counts, "lkg_triple_scores_f32: nothing to write (out and counts are both null)");
    LKG_REQUIRE(!counts || labels, "lkg_triple_scores_f32: counts need labels (null pointer)");
    LKG_REQUIRE(!counts || thr == thr, "lkg_triple_scores_f32: thr is NaN");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(p && q_idx && c_idx, "lkg_triple_scores_f32: null pointer");
    const long blocks = (n + TS_TRIPLES - 1) / TS_TRIPLES;
    const dim3 grid((unsigned)(blocks < TS_GRID ? blocks : TS_GRID)), block(TS_THREADS);
    vec_dispatch(vec_ok(p, ldp, e, e ? lde : 0), [&](auto vec) {
        hipLaunchKernelGGL(triple_scores_kernel<decltype(vec)::value>, grid, block, 0, (hipStream_t)stream, (long)n, k, p,
                           (long)ldp, (const long *)q_idx, (const long *)c_idx, pn, e, (long)lde, (const long *)rel, alpha,
                           (int)flags, labels, thr, out, (unsigned long long *)counts);
    });
    LKG_CHECK_LAUNCH("lkg_triple_scores_f32");
    return LKG_OK;
}

// lkg_preload(): HIP loads a translation unit's code object on the first use of one of its kernels; asking for a kernel's
// attributes is such a use (no launch).
int lkg_internal_preload_triples() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&triple_scores_kernel<true>)) == hipSuccess ? 0 : 1;
}
