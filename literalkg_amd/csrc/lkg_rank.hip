// Filtered link-prediction ranking (literalkg_amd/ranking.py): for every query q_i (one per held-out triple and side) count
// the candidates c in [0, N) whose score  s_c = pn_c - 2 q_i . p_c  lies strictly below / exactly at the truth's score.
// ||q_i||^2 is common to every candidate of a row and cancels; dot scoring passes pn = NULL (s_c = -2 q.p, exact).
//
// Arithmetic: the exact f32 MFMA v_mfma_f32_16x16x4_f32 -- every output element is a k-ordered chain of f32 fmas (one
// rounding per product, no wider accumulator), independent of its position in the 16 x 16 tile.  So a (query, candidate)
// pair scored in ANY tile position, with the same operands fed in the same k order, gives the same bits: the truth's
// score (the threshold) and the scores of filtered candidates come from rank_pair_scores (lkg_rank_common.h), which
// feeds the same lane -> k map as the counting kernel.  A candidate whose row is bit-identical to the truth's ties
// exactly.
//
// k order (both kernels, load4 / mfma_chunk of lkg_rank_common.h, shared with lkg_topk.hip): k is taken in chunks of 16;
// lane l holds elements 4(l>>4) .. 4(l>>4)+3 of the chunk for row l & 15; MFMA j of the chunk feeds element j.
//
// Counting: 256-thread workgroups over a 64-query x 256-candidate tile (4 waves, 64 x 64 each = 4 x 4 MFMA tiles);
// operands come straight from global memory (the 4 waves share the query tile through L1, consecutive workgroups share
// the candidate block through L2).  Per-row counts reduce in registers, across the 16 lanes of a row, across the waves
// in LDS, and leave with one atomic per row per workgroup.  The B x N scores are never stored.
#include "lkg_known.h"
#include "lkg_rank_common.h"

namespace {

constexpr int RK_THREADS = 256;
constexpr int RK_ROWS = 64;          // queries per workgroup
constexpr int RK_COLS = 256;         // candidates per workgroup (64 per wave)

template <bool VEC>
__global__ __launch_bounds__(RK_THREADS) void rank_count_kernel(long n_q, long n_c, int k, const float *__restrict__ q,
                                                                long ldq, const float *__restrict__ p, long ldp,
                                                                const float *__restrict__ pn, const float *__restrict__ thr,
                                                                const long *__restrict__ truth, int *__restrict__ better,
                                                                int *__restrict__ equal, long tiles_q) {
    __shared__ int cnt[2][RK_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * RK_ROWS, c0 = (bid / tiles_q) * RK_COLS + wave * 64;
    if (tid < RK_ROWS) {
        cnt[0][tid] = 0;
        cnt[1][tid] = 0;
    }
    const float *qrow[4], *prow[4];
    tile_rows(qrow, q, ldq, q0, n_q, r);
    tile_rows(prow, p, ldp, c0, n_c, r);
    f32x4 acc[4][4];
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
        for (int i = 0; i < 4; ++i) {          // next chunk in flight while this one runs on the matrix pipe
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
    __syncthreads();      // cnt cleared
    // acc[i][j][v]: query row q0 + 16 i + 4 s + v, candidate c0 + 16 j + r
    float pnv[4];
    long cid[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cid[j] = c0 + 16 * j + r;
        pnv[j] = (pn && cid[j] < n_c) ? pn[cid[j]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long row = q0 + 16 * i + 4 * s + v;
            const long rr = min(row, n_q - 1);
            const float t = thr[rr];
            const long tr = truth[rr];
            float nb = 0.f, ne = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float sc = __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                const bool ok = cid[j] < n_c && cid[j] != tr;
                nb += (ok && sc < t) ? 1.f : 0.f;
                ne += (ok && sc == t) ? 1.f : 0.f;
            }
            nb = group_sum<16>(nb);
            ne = group_sum<16>(ne);
            if (r == 0 && row < n_q) {
                if (nb != 0.f) atomicAdd(&cnt[0][16 * i + 4 * s + v], (int)nb);
                if (ne != 0.f) atomicAdd(&cnt[1][16 * i + 4 * s + v], (int)ne);
            }
        }
    }
    __syncthreads();
    if (tid < RK_ROWS && q0 + tid < n_q) {
        if (cnt[0][tid]) atomicAdd(better + q0 + tid, cnt[0][tid]);
        if (cnt[1][tid]) atomicAdd(equal + q0 + tid, cnt[1][tid]);
    }
}

// One wave per query: thr = the truth's score; better / equal = minus the filtered candidates (other than the truth)
// that the counting kernel will count, so that after it they hold the filtered counts.
template <bool VEC>
__global__ __launch_bounds__(RK_THREADS) void rank_prepare_kernel(
    long n_q, long n_c, int k, const float *__restrict__ q, long ldq, const float *__restrict__ p, long ldp,
    const float *__restrict__ pn, const long *__restrict__ truth, const long *__restrict__ frow,
    const long *__restrict__ frel, const int *__restrict__ rowptr, const int *__restrict__ col,
    const int *__restrict__ eptr, const int *__restrict__ rel, float *__restrict__ thr, int *__restrict__ better,
    int *__restrict__ equal) {
    const long i = (long)blockIdx.x * (RK_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n_q) return;                           // (a whole wave leaves: no cross-lane op is left half-populated)
    const int lane = threadIdx.x & 63, r = lane & 15;
    const float *qrow = q + i * ldq;
    const long tr = min(max(truth[i], 0L), n_c - 1);
    const float st = __shfl(rank_pair_scores<VEC>(qrow, p, ldp, pn, tr, k), 0);
    float nb = 0.f, ne = 0.f;
    if (rowptr) {
        const long f = min(max(frow[i], 0L), n_c - 1);      // (rowptr has n_cand + 1 entries)
        const int want = (int)frel[i];
        const int e0 = rowptr[f], e1 = rowptr[f + 1];
        for (int eb = e0; eb < e1; eb += 16) {       // 16 filter entries per pass (uniform trip count in the wave)
            const int e = eb + r;
            long c = tr;
            bool keep = false;
            if (e < e1) {
                c = col[e];
                if (c != tr && c >= 0 && c < n_c) keep = known_under_exact(eptr, rel, e, want);
                else c = tr;
            }
            const float sc = rank_pair_scores<VEC>(qrow, p, ldp, pn, c, k);
            if (lane < 16 && keep) {
                nb += sc < st ? 1.f : 0.f;
                ne += sc == st ? 1.f : 0.f;
            }
        }
    }
    nb = wave_sum(nb);
    ne = wave_sum(ne);
    if (lane == 0) {
        thr[i] = st;
        better[i] = -(int)nb;
        equal[i] = -(int)ne;
    }
}

__global__ __launch_bounds__(256) void rank_sqnorm_kernel(long n, int k, const float *__restrict__ p, long ldp,
                                                          float *__restrict__ out) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63;
    const float *x = p + row * ldp;
    float acc = 0.f;
    for (int c = lane; c < k; c += 64) acc = __builtin_fmaf(x[c], x[c], acc);
    acc = wave_sum(acc);
    if (lane == 0) out[row] = acc;
}

__global__ __launch_bounds__(256) void rank_queries_kernel(long n, int k, const float *__restrict__ p, long ldp,
                                                           const long *__restrict__ ids, const float *__restrict__ e,
                                                           long lde, const long *__restrict__ rel, float alpha,
                                                           float *__restrict__ q, long ldq) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const int lane = threadIdx.x & 63;
    const float *x = p + ids[row] * ldp;
    const float *er = e ? e + (rel ? rel[row] : 0L) * lde : nullptr;
    float *y = q + row * ldq;
    for (int c = lane; c < k; c += 64) y[c] = er ? __builtin_fmaf(alpha, er[c], x[c]) : x[c];
}

}  // namespace

extern "C" int lkg_rank_sqnorm_f32(int64_t n, int32_t k, const float *p, int64_t ldp, float *out, void *stream) {
    LKG_REQUIRE(n >= 0 && k > 0 && ldp >= k, "lkg_rank_sqnorm_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(p && out, "lkg_rank_sqnorm_f32: null pointer");
    hipLaunchKernelGGL(rank_sqnorm_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long)n, k,
                       p, (long)ldp, out);
    LKG_CHECK_LAUNCH("lkg_rank_sqnorm_f32");
    return LKG_OK;
}

extern "C" int lkg_rank_queries_f32(int64_t n, int32_t k, const float *p, int64_t ldp, const int64_t *ids,
                                    const float *e, int64_t lde, const int64_t *rel, float alpha, float *q, int64_t ldq,
                                    void *stream) {
    LKG_REQUIRE(n >= 0 && k > 0 && ldp >= k && ldq >= k && (!e || lde >= k), "lkg_rank_queries_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(p && ids && q, "lkg_rank_queries_f32: null pointer");
    hipLaunchKernelGGL(rank_queries_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long)n, k,
                       p, (long)ldp, (const long *)ids, e, (long)lde, (const long *)rel, alpha, q, (long)ldq);
    LKG_CHECK_LAUNCH("lkg_rank_queries_f32");
    return LKG_OK;
}

extern "C" int lkg_rank_prepare_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                    int64_t ldp, const float *pn, const int64_t *truth, const int64_t *filter_row,
                                    const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col,
                                    const int32_t *eptr, const int32_t *rel, float *thr, int32_t *better,
                                    int32_t *equal, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand > 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k,
                "lkg_rank_prepare_f32: bad sizes");
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(q && p && truth && thr && better && equal, "lkg_rank_prepare_f32: null pointer");
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "lkg_rank_prepare_f32: incomplete filter");
    const dim3 grid((unsigned)((n_q + 3) / 4)), block(RK_THREADS);
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL(rank_prepare_kernel<decltype(vec)::value>, grid, block, 0, (hipStream_t)stream, (long)n_q,
                           (long)n_cand, k, q, (long)ldq, p, (long)ldp, pn, (const long *)truth, (const long *)filter_row,
                           (const long *)filter_rel, rowptr, col, eptr, rel, thr, better, equal);
    });
    LKG_CHECK_LAUNCH("lkg_rank_prepare_f32");
    return LKG_OK;
}

extern "C" int lkg_rank_count_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                  int64_t ldp, const float *pn, const float *thr, const int64_t *truth, int32_t *better,
                                  int32_t *equal, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand >= 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k,
                "lkg_rank_count_f32: bad sizes");
    if (n_q == 0 || n_cand == 0) return LKG_OK;
    LKG_REQUIRE(q && p && thr && truth && better && equal, "lkg_rank_count_f32: null pointer");
    const long tiles_q = (n_q + RK_ROWS - 1) / RK_ROWS, tiles_c = (n_cand + RK_COLS - 1) / RK_COLS;
    LKG_REQUIRE(tiles_q * tiles_c < INT32_MAX, "lkg_rank_count_f32: too many tiles (split the queries)");
    const dim3 grid((unsigned)(tiles_q * tiles_c)), block(RK_THREADS);
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL(rank_count_kernel<decltype(vec)::value>, grid, block, 0, (hipStream_t)stream, (long)n_q,
                           (long)n_cand, k, q, (long)ldq, p, (long)ldp, pn, thr, (const long *)truth, better, equal, tiles_q);
    });
    LKG_CHECK_LAUNCH("lkg_rank_count_f32");
    return LKG_OK;
}

// lkg_preload(): HIP loads a translation unit's code object on the first use of one of its kernels; asking for a kernel's
// attributes is such a use (no launch).
int lkg_internal_preload_rank() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&rank_sqnorm_kernel)) == hipSuccess ? 0 : 1;
}
