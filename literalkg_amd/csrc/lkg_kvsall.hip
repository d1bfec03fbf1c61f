// KvsAll training loss (literalkg_amd/kvs_all.py): for every query row q_i the binary cross-entropy with logits of ALL n_c
// candidates against the multi-hot vector of the query's known answers,
//     L_i = sum_c [ softplus(z_ic) - y'_ic z_ic ],   y' = (1 - eps) y + eps / n,   z_ic = nsb * s_ic + bias_i,
// with the ranking kernels' score  s_ic = pn_c - 2 q_i . p_c  and  nsb = -scale (distance) or -scale / 2 (dot: pn = NULL).
// A sigmoid does not cancel the row constant ||q_i||^2 as a softmax does: it arrives as the per-row bias
// scale (margin - ||q_i||^2), and has a gradient of its own (the row sums of the weights).  DESIGN.md 3.6o.
//
// Arithmetic: the score is that of rank_count_kernel (lkg_rank_common.h: the exact f32 MFMA, the same lane -> k map, zero
// padding past k, the same final fma); the logit takes two more roundings, fl(fl(nsb * s) + bias).  A term is evaluated
// without cancellation: x = y ? -z : z,  sp = max(x, 0) + log1pf(expf(-|x|))  (softplus(z) - z = softplus(-z)), and with
// smoothing  + ce_y * z  with  ce_1 = eps (1 - 1 / n),  ce_0 = -eps / n  (formed in double by the entry point, rounded
// once).  With eps == 0 the product is not executed: the sum has the bits of the plain one.  Floating-point contraction is
// off in this file: every rounding above is one the references restate.
//
// Forward: the tile, the split scheme and the workspace of softmax_partial_kernel with MASKED (lkg_softmax.hip): a
// 256-thread workgroup owns 64 query rows and a contiguous range of 256-candidate tiles.  A lane keeps ONE running sum per
// row it holds (16 of them, over its 4 columns of every tile) -- no maximum to carry, so nothing crosses lanes inside the loop.
// The 16 lanes of a row meet once and the 4 waves meet once in LDS, after the last tile; the workgroup's sum goes to
// workspace [S][B], sigmoid_finish_kernel merges the S partials of a row in split order in float64.  No float atomics: for
// a given S every bit is the same from run to run.
//
// The positives of query i are the sorted candidate positions ycol[yptr[i] .. yptr[i + 1]) (lkg_softmax_excluded with
// truth = -1 builds them).  Lane = row of the wave's 64 walks its row's list with a cursor, turns the entries inside the
// wave's 64 columns into a 64-bit mask and leaves it in LDS for the lanes that hold the row's logits (wave-local: no
// workgroup barrier); a wave none of whose rows has a positive in the tile skips all of it.  The cursor and mask helpers
// are lkg_all_entity_common.h's, shared with lkg_softmax.hip; a call without lists (yptr NULL) seeks with no rows, so
// every list is empty and yptr is never read.
#include "lkg_all_entity_common.h"

#pragma clang fp contract(off)

namespace {

// softplus(x) without cancellation; NaN in, NaN out (fmaxf drops it, the logarithm keeps it)
__device__ __forceinline__ float softplus_f(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }

// sigma(x) on the side that does not cancel: 1 / (1 + e^-x) for x >= 0, e^x / (1 + e^x) below
__device__ __forceinline__ float sigmoid_f(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.f : e) / (1.f + e);
}

// (two workgroups per CU stated: without the hint the compiler took 260 registers, with it 225 and no spill)
template <bool VEC>
__global__ __launch_bounds__(AE_THREADS, 2) void sigmoid_partial_kernel(
    long n_q, long n_c, int k, const float *__restrict__ q, long ldq, const float *__restrict__ p, long ldp,
    const float *__restrict__ pn, const float *__restrict__ bias, float nsb, float ce1, float ce0, int smooth, int splits,
    long tiles_q, long tiles_c, float *__restrict__ ws, const int *__restrict__ yptr, const int *__restrict__ ycol,
    int m_total) {
    __shared__ unsigned long long sm_y[4][AE_ROWS];
    __shared__ float sm_b[AE_ROWS], sm_l[4][AE_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * AE_ROWS;
    const int split = (int)(bid / tiles_q);
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    if (tid < AE_ROWS) sm_b[tid] = (bias && q0 + tid < n_q) ? bias[q0 + tid] : 0.f;
    __syncthreads();
    const float *qrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qrow[i] = q + min(q0 + 16 * i + r, n_q - 1) * ldq;    // rows past the end: never written
    float l[4][4];                    // [i][v]: query row 16 i + 4 s + v, this lane's columns only
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) l[i][v] = 0.f;
    ListCursor x = list_seek(yptr, ycol, m_total, q0 + lane, yptr ? n_q : 0, t_lo * AE_COLS);

    for (long t = t_lo; t < t_hi; ++t) {
        const long c0 = t * AE_COLS + wave * 64;
        const float *prow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) prow[i] = p + min(c0 + 16 * i + r, n_c - 1) * ldp;
        f32x4 acc[4][4];
        rank_tile_dots<VEC>(acc, qrow, prow, k, s);
        // acc[i][j][v]: query row 16 i + 4 s + v, candidate c0 + 16 j + r
        const bool any = list_publish(x, ycol, c0, sm_y[wave], lane);      // wave-uniform: some row has a positive here
        float pnv[4];
        bool ok[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long c = c0 + 16 * j + r;
            ok[j] = c < n_c;
            pnv[j] = (pn && ok[j]) ? pn[c] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const float bi = sm_b[16 * i + 4 * s + v];
                unsigned long long mrow = 0ull;     // the row's positives among the wave's 64 columns
                if (any) mrow = sm_y[wave][16 * i + 4 * s + v];
                float term[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const bool y = (mrow >> (16 * j + r)) & 1ull;
                    const float z = nsb * __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]) + bi;
                    float tj = softplus_f(y ? -z : z);
                    if (smooth) tj = tj + (y ? ce1 : ce0) * z;
                    term[j] = ok[j] ? tj : 0.f;     // a column past the end contributes nothing
                }
                // the tile's four terms first, then the running sum: a quarter of the additions in the long chain
                l[i][v] += (term[0] + term[1]) + (term[2] + term[3]);
            }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const float sum = group_sum<16>(l[i][v]);
            if (r == 0) sm_l[wave][16 * i + 4 * s + v] = sum;
        }
    __syncthreads();
    if (tid < AE_ROWS && q0 + tid < n_q) {
        float lw = sm_l[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) lw += sm_l[w][tid];
        ws[(long)split * n_q + q0 + tid] = lw;
    }
}

// one thread per query: the S partials of a row (the forward's splits, or the tiles of the weights' row sums) in order in
// float64, rounded once
__global__ __launch_bounds__(AE_THREADS) void sigmoid_finish_kernel(long n_q, int splits, const float *__restrict__ ws,
                                                                    float *__restrict__ loss) {
    const long i = (long)blockIdx.x * AE_THREADS + threadIdx.x;
    if (i >= n_q) return;
    double sum = 0.0;
    for (int j = 0; j < splits; ++j) sum += (double)ws[(long)j * n_q + i];
    loss[i] = (float)sum;
}

// The backward's recompute: V[i, c] = sb g_i (sigma(z_ic) - y'_ic) for the n_c candidates of a chunk that starts at
// candidate c_base of the table (p, pn point at the chunk; the lists hold positions of the whole table).  One 64 x 256 tile
// per workgroup, stored straight from the accumulator layout: the 16 lanes of a row write 64 consecutive bytes.  With
// rowsum (nullable) the tile's share of rowsum(V) goes to rowsum[tile][row] -- the stored values added in registers, over
// the row's 16 lanes and over the 4 waves in LDS; sigmoid_finish_kernel adds the tiles in order (dbias = rowsum(V) / sb).
// A row sum through the dQ product's f32 MFMA chain (a column of ones next to P) was measured first: its terms all have
// one sign away from the positives, and the chain's error then grew with the length, not with its root.
template <bool VEC>
__global__ __launch_bounds__(AE_THREADS) void sigmoid_weights_kernel(
    long n_q, long n_c, int k, const float *__restrict__ q, long ldq, const float *__restrict__ p, long ldp,
    const float *__restrict__ pn, const float *__restrict__ bias, long c_base, const float *__restrict__ g, float nsb,
    float sb, float ce1, float ce0, float *__restrict__ vout, long ldv, long tiles_q, const int *__restrict__ yptr,
    const int *__restrict__ ycol, int m_total, float *__restrict__ rowsum) {
    __shared__ unsigned long long sm_y[4][AE_ROWS];
    __shared__ float sm_r[4][AE_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * AE_ROWS, c0 = (bid / tiles_q) * AE_COLS + wave * 64;
    const float *qrow[4], *prow[4];
    tile_rows(qrow, q, ldq, q0, n_q, r);
    tile_rows(prow, p, ldp, c0, n_c, r);
    f32x4 acc[4][4];
    rank_tile_dots<VEC>(acc, qrow, prow, k, s);
    ListCursor x = list_seek(yptr, ycol, m_total, q0 + lane, yptr ? n_q : 0, c_base + c0);
    const bool any = list_publish(x, ycol, c_base + c0, sm_y[wave], lane);
    float pnv[4];
    long cid[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cid[j] = c0 + 16 * j + r;
        pnv[j] = (pn && cid[j] < n_c) ? pn[cid[j]] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const long row = q0 + 16 * i + 4 * s + v;
            const long rr = min(row, n_q - 1);
            const float bi = bias ? bias[rr] : 0.f, coef = sb * g[rr];
            float *out = vout + rr * ldv;
            unsigned long long mrow = 0ull;
            if (any) mrow = sm_y[wave][16 * i + 4 * s + v];
            float vj[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool y = (mrow >> (16 * j + r)) & 1ull;
                const float z = nsb * __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]) + bi;
                // sigma(z) - y' on the side that does not cancel: ce_1 - sigma(-z) for a positive, sigma(z) + ce_0 otherwise
                const float w = y ? ce1 - sigmoid_f(-z) : sigmoid_f(z) + ce0;
                vj[j] = cid[j] < n_c ? coef * w : 0.f;
                if (row < n_q && cid[j] < n_c) out[cid[j]] = vj[j];
            }
            if (rowsum) {                           // (uniform) the tile's share of rowsum(V): lanes, then waves below
                const float sum = group_sum<16>((vj[0] + vj[1]) + (vj[2] + vj[3]));
                if (r == 0) sm_r[wave][16 * i + 4 * s + v] = sum;
            }
        }
    if (rowsum) {
        __syncthreads();
        if (tid < AE_ROWS && q0 + tid < n_q)
            rowsum[(bid / tiles_q) * n_q + q0 + tid] = ((sm_r[0][tid] + sm_r[1][tid]) + sm_r[2][tid]) + sm_r[3][tid];
    }
}

bool eps_ok(double eps) { return eps >= 0.0 && eps < 1.0; }

// the smoothing coefficients of a positive and of a negative column, in double, rounded once
float ce_pos(double eps, int64_t n) { return (float)(eps * (1.0 - 1.0 / (double)n)); }
float ce_neg(double eps, int64_t n) { return (float)(-eps / (double)n); }

}  // namespace

extern "C" int lkg_sigmoid_all_partial_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                           const float *p, int64_t ldp, const float *pn, const float *bias, float scale,
                                           double eps, int32_t splits, const int32_t *yptr, const int32_t *ycol,
                                           int64_t n_pos, float *ws, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand > 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k && n_pos >= 0 &&
                    n_pos < INT32_MAX,
                "lkg_sigmoid_all_partial_f32: bad sizes");
    LKG_REQUIRE(scale_ok(scale), "lkg_sigmoid_all_partial_f32: scale must be positive and finite");
    LKG_REQUIRE(eps_ok(eps), "lkg_sigmoid_all_partial_f32: eps must lie in [0, 1)");
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(splits >= 1 && splits == lkg_softmax_all_splits(n_q, n_cand, splits),
                "lkg_sigmoid_all_partial_f32: splits must come from lkg_softmax_all_splits");
    LKG_REQUIRE(q && p && ws && (!yptr || ycol || n_pos == 0), "lkg_sigmoid_all_partial_f32: null pointer");
    const long tiles_q = (n_q + AE_ROWS - 1) / AE_ROWS, tiles_c = (n_cand + AE_COLS - 1) / AE_COLS;
    LKG_REQUIRE(tiles_q * splits < INT32_MAX, "lkg_sigmoid_all_partial_f32: too many workgroups (split the queries)");
    const dim3 grid((unsigned)(tiles_q * splits)), block(AE_THREADS);
    const float nsb = neg_scale_beta(scale, pn);
    const int m_total = yptr ? (int)n_pos : 0;
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL(sigmoid_partial_kernel<decltype(vec)::value>, grid, block, 0, (hipStream_t)stream, (long)n_q,
                           (long)n_cand, k, q, (long)ldq, p, (long)ldp, pn, bias, nsb, ce_pos(eps, n_cand),
                           ce_neg(eps, n_cand), (int)(eps > 0.0), splits, tiles_q, tiles_c, ws, yptr, ycol, m_total);
    });
    LKG_CHECK_LAUNCH("lkg_sigmoid_all_partial_f32");
    return LKG_OK;
}

extern "C" int lkg_sigmoid_all_finish_f32(int64_t n_q, int32_t splits, const float *ws, float *loss, void *stream) {
    LKG_REQUIRE(n_q >= 0 && splits >= 1, "lkg_sigmoid_all_finish_f32: bad sizes");
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(ws && loss, "lkg_sigmoid_all_finish_f32: null pointer");
    const dim3 grid((unsigned)((n_q + AE_THREADS - 1) / AE_THREADS)), block(AE_THREADS);
    hipLaunchKernelGGL(sigmoid_finish_kernel, grid, block, 0, (hipStream_t)stream, (long)n_q, splits, ws, loss);
    LKG_CHECK_LAUNCH("lkg_sigmoid_all_finish_f32");
    return LKG_OK;
}

extern "C" int lkg_sigmoid_all_weights_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                           const float *p, int64_t ldp, const float *pn, const float *bias,
                                           int64_t c_base, int64_t n_total, const float *g, float scale, double eps,
                                           const int32_t *yptr, const int32_t *ycol, int64_t n_pos, float *v, int64_t ldv,
                                           float *rowsum, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand >= 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k && ldv >= n_cand &&
                    c_base >= 0 && n_total < INT32_MAX && c_base + n_cand <= n_total && n_total > 0 && n_pos >= 0 &&
                    n_pos < INT32_MAX,
                "lkg_sigmoid_all_weights_f32: bad sizes");
    LKG_REQUIRE(scale_ok(scale), "lkg_sigmoid_all_weights_f32: scale must be positive and finite");
    LKG_REQUIRE(eps_ok(eps), "lkg_sigmoid_all_weights_f32: eps must lie in [0, 1)");
    if (n_q == 0 || n_cand == 0) return LKG_OK;
    LKG_REQUIRE(q && p && g && v && (!yptr || ycol || n_pos == 0), "lkg_sigmoid_all_weights_f32: null pointer");
    const long tiles_q = (n_q + AE_ROWS - 1) / AE_ROWS, tiles_c = (n_cand + AE_COLS - 1) / AE_COLS;
    LKG_REQUIRE(tiles_q * tiles_c < INT32_MAX, "lkg_sigmoid_all_weights_f32: too many tiles (use smaller chunks)");
    const dim3 grid((unsigned)(tiles_q * tiles_c)), block(AE_THREADS);
    const float nsb = neg_scale_beta(scale, pn);
    const int m_total = yptr ? (int)n_pos : 0;
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL(sigmoid_weights_kernel<decltype(vec)::value>, grid, block, 0, (hipStream_t)stream, (long)n_q,
                           (long)n_cand, k, q, (long)ldq, p, (long)ldp, pn, bias, (long)c_base, g, nsb, -nsb,
                           ce_pos(eps, n_total), ce_neg(eps, n_total), v, (long)ldv, tiles_q, yptr, ycol, m_total, rowsum);
    });
    LKG_CHECK_LAUNCH("lkg_sigmoid_all_weights_f32");
    return LKG_OK;
}

int lkg_internal_preload_kvsall() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sigmoid_finish_kernel)) == hipSuccess ? 0 : 1;
}
