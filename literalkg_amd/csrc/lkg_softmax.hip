// 1-vs-all training loss (literalkg_amd/one_vs_all.py): for every query q_i the cross-entropy of the truth t_i against the
// softmax over ALL n_c candidates,  loss_i = logsumexp_c z_ic - z_i,t_i,  with the logit  z_ic = -scale * beta * s_ic  of the
// kernel score  s_ic = pn_c - 2 q_i . p_c  (beta = 1;  dot scoring: pn = NULL, s = -2 q.p, beta = 1/2, z = scale q.p).
// ||q_i||^2 is common to a row and cancels in the softmax as it cancels in ranking.  The B x N logits are never stored by
// the forward pass; the backward pass recomputes them chunk by chunk into the weights V.
//
// Arithmetic: exactly that of rank_count_kernel (lkg_rank_common.h: the exact f32 MFMA, the same lane -> k map, zero
// padding past k, the same final fma), then ONE rounded product nsb * s with nsb = -scale * beta.  The truth's logit comes
// from rank_pair_scores and the same product, so it has the bits it has inside a tile: with one candidate the loss is
// exactly 0.  Floating-point contraction is off in this file: z - m must subtract the ROUNDED z the maximum was taken of.
//
// Forward: a 256-thread workgroup owns 64 query rows and a contiguous range of 256-candidate tiles (split `split` of S, as
// lkg_topk.hip).  Every wave carries, per row, the running pair (m, l) of its own 64 columns of each tile: m the largest
// logit so far, l = sum exp(z - m), rescaled when m moves.  Per tile the reductions run in registers (the lane's 4
// columns of a row) and across the 16 lanes of a row (group_max / group_sum); the 4 waves meet in LDS once, after the last
// tile (a per-tile meeting would cost two barriers per tile and change nothing but the association).  The workgroup's (m, l)
// goes to workspace [S][B]; softmax_finish_kernel merges the S partials of a row in split order in float64.  No float
// atomics: for a given S every bit is the same from run to run.
//
// MASKED (template parameter of the partial and the weights kernel) is the filtered loss: the kernel then
// reads its last three arguments, the exclusion lists, which the unmasked launches pass as NULL, NULL, 0 and the unmasked
// instantiations never touch (they compile to the instructions of a kernel without the parameter).  Query i drops the
// sorted candidate positions xcol[xptr[i] .. xptr[i + 1]) from its softmax -- the other known answers of the query.  A
// dropped column gets z = -inf inside the tile, exactly as a column
// past n_c does, BEFORE the running (max, sum) sees it (subtracting the dropped mass afterwards is amplified by
// 1 / (1 - dropped mass) without bound); the weights kernel stores exactly 0 there.  Lane = row of the wave's 64 walks its
// row's list with a cursor, turns the entries inside the wave's 64 columns into a 64-bit mask and leaves it in LDS for the
// lanes that hold the row's logits (wave-local: no workgroup barrier); a wave none of whose rows drops a column of the
// tile skips all of it.  The truth is never in a list (softmax_excluded_kernel), so the finish kernel serves both.
#include "lkg_all_entity_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int SM_MAX_SPLITS = LKG_SOFTMAX_MAX_SPLITS;

// exp(z - m) must not see inf - inf: a pair that has met no candidate yet is (-inf, 0) and takes 0 as its reference
__device__ __forceinline__ float safe_ref(float m) { return m == -__builtin_inff() ? 0.f : m; }

template <bool VEC, bool MASKED>
__global__ __launch_bounds__(AE_THREADS) void softmax_partial_kernel(
    long n_q, long n_c, int k, const float *__restrict__ q, long ldq, const float *__restrict__ p, long ldp,
    const float *__restrict__ pn, float nsb, int splits, long tiles_q, long tiles_c, float *__restrict__ ws_m,
    float *__restrict__ ws_l, const int *__restrict__ xptr, const int *__restrict__ xcol, int m_total) {
    __shared__ unsigned long long sm_x[4][AE_ROWS];        // MASKED only (unused, it takes no LDS)
    __shared__ float sm_m[4][AE_ROWS], sm_l[4][AE_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * AE_ROWS;
    const int split = (int)(bid / tiles_q);
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    const float *qrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qrow[i] = q + min(q0 + 16 * i + r, n_q - 1) * ldq;    // rows past the end: never written
    float m[4][4], l[4][4];           // [i][v]: query row 16 i + 4 s + v, the same on the 16 lanes of the row
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            m[i][v] = -__builtin_inff();
            l[i][v] = 0.f;
        }
    ListCursor x{0, 0, INT_MAX};
    if constexpr (MASKED) x = list_seek(xptr, xcol, m_total, q0 + lane, n_q, t_lo * AE_COLS);

    for (long t = t_lo; t < t_hi; ++t) {
        const long c0 = t * AE_COLS + wave * 64;
        const float *prow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) prow[i] = p + min(c0 + 16 * i + r, n_c - 1) * ldp;
        f32x4 acc[4][4];
        rank_tile_dots<VEC>(acc, qrow, prow, k, s);
        // acc[i][j][v]: query row 16 i + 4 s + v, candidate c0 + 16 j + r
        bool any = false;                                   // wave-uniform: some row drops a column here
        if constexpr (MASKED) any = list_publish(x, xcol, c0, sm_x[wave], lane);
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
                float z[4], mt = -__builtin_inff();
                unsigned long long mrow = 0ull;     // the row's dropped columns of the wave's 64
                if constexpr (MASKED) {
                    if (any) mrow = sm_x[wave][16 * i + 4 * s + v];
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) {       // a column past the end, or a dropped one, is -inf: no maximum, exp = 0
                    const bool keep = ok[j] && !((mrow >> (16 * j + r)) & 1ull);
                    z[j] = keep ? nsb * __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]) : -__builtin_inff();
                    mt = fmaxf(mt, z[j]);           // (a NaN logit is skipped here and poisons l below)
                }
                mt = group_max<16>(mt);
                const float mn = fmaxf(m[i][v], mt), ref = safe_ref(mn);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) sum += expf(z[j] - ref);
                sum = group_sum<16>(sum);
                l[i][v] = l[i][v] * expf(m[i][v] - ref) + sum;
                m[i][v] = mn;
            }
    }
    if (r == 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                sm_m[wave][16 * i + 4 * s + v] = m[i][v];
                sm_l[wave][16 * i + 4 * s + v] = l[i][v];
            }
    }
    __syncthreads();
    if (tid < AE_ROWS && q0 + tid < n_q) {
        float mw = sm_m[0][tid];
#pragma unroll
        for (int w = 1; w < 4; ++w) mw = fmaxf(mw, sm_m[w][tid]);
        const float ref = safe_ref(mw);
        float lw = 0.f;
#pragma unroll
        for (int w = 0; w < 4; ++w) lw += sm_l[w][tid] * expf(sm_m[w][tid] - ref);
        const long o = (long)split * n_q + q0 + tid;
        ws_m[o] = mw;
        ws_l[o] = lw;
    }
}

// One wave per query: the truth's logit with the pair routine of the ranking kernels, the S partials merged in split
// order in float64, lse and loss rounded once each; lse_lo (nullable) is the remainder of lse's rounding, with which the
// backward's exp(z - lse) does not carry |lse| u / 2 into every weight of the row.
template <bool VEC>
__global__ __launch_bounds__(AE_THREADS) void softmax_finish_kernel(long n_q, long n_c, int k, const float *__restrict__ q,
                                                                    long ldq, const float *__restrict__ p, long ldp,
                                                                    const float *__restrict__ pn,
                                                                    const long *__restrict__ truth, float nsb, int splits,
                                                                    const float *__restrict__ ws_m,
                                                                    const float *__restrict__ ws_l, float *__restrict__ lse,
                                                                    float *__restrict__ lse_lo, float *__restrict__ loss) {
    const long i = (long)blockIdx.x * (AE_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n_q) return;                           // (a whole wave leaves)
    const int lane = threadIdx.x & 63;
    const long tr = min(max(truth[i], 0L), n_c - 1);
    const float st = __shfl(rank_pair_scores<VEC>(q + i * ldq, p, ldp, pn, tr, k), 0);
    const float zt = nsb * st;
    double mx = -__builtin_inf();
    for (int j = 0; j < splits; ++j) mx = fmax(mx, (double)ws_m[(long)j * n_q + i]);
    const double ref = mx == -__builtin_inf() ? 0.0 : mx;
    double sum = 0.0;
    for (int j = 0; j < splits; ++j) sum += (double)ws_l[(long)j * n_q + i] * exp((double)ws_m[(long)j * n_q + i] - ref);
    const double lsed = mx + log(sum);
    if (lane == 0) {
        const float hi = (float)lsed;
        lse[i] = hi;
        if (lse_lo) lse_lo[i] = (float)(lsed - (double)hi);     // what the rounding of lse dropped (NaN for a non-finite lse)
        loss[i] = (float)(lsed - (double)zt);
    }
}

// The backward's recompute: V[i, c] = sb g_i (exp((z_ic - lse_i) - lse_lo_i) - [c_base + c == t_i]) for the n_c candidates
// of a chunk that starts at candidate c_base of the table (p, pn point at the chunk).  One 64 x 256 tile per workgroup, stored
// straight from the accumulator layout: the 16 lanes of a row write 64 consecutive bytes.
// MASKED: a dropped column is stored as exactly 0; the lists hold table positions, c_base + the chunk's column.
template <bool VEC, bool MASKED>
__global__ __launch_bounds__(AE_THREADS) void softmax_weights_kernel(
    long n_q, long n_c, int k, const float *__restrict__ q, long ldq, const float *__restrict__ p, long ldp,
    const float *__restrict__ pn, long c_base, const long *__restrict__ truth, const float *__restrict__ lse,
    const float *__restrict__ lse_lo, const float *__restrict__ g, float nsb, float sb, float *__restrict__ vout, long ldv,
    long tiles_q, const int *__restrict__ xptr, const int *__restrict__ xcol, int m_total) {
    __shared__ unsigned long long sm_x[4][AE_ROWS];        // MASKED only (unused, it takes no LDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * AE_ROWS, c0 = (bid / tiles_q) * AE_COLS + wave * 64;
    const float *qrow[4], *prow[4];
    tile_rows(qrow, q, ldq, q0, n_q, r);
    tile_rows(prow, p, ldp, c0, n_c, r);
    f32x4 acc[4][4];
    rank_tile_dots<VEC>(acc, qrow, prow, k, s);
    bool any = false;
    if constexpr (MASKED) {
        ListCursor x = list_seek(xptr, xcol, m_total, q0 + lane, n_q, c_base + c0);
        any = list_publish(x, xcol, c_base + c0, sm_x[wave], lane);
    }
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
            const float ls = lse[rr], lo = lse_lo ? lse_lo[rr] : 0.f, coef = sb * g[rr];
            const long tl = truth[rr] - c_base;
            float *out = vout + rr * ldv;
            unsigned long long mrow = 0ull;
            if constexpr (MASKED) {
                if (any) mrow = sm_x[wave][16 * i + 4 * s + v];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool dropped = (mrow >> (16 * j + r)) & 1ull;
                const float z = nsb * __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                // exp(z - lse) with lse = ls + lo: d = fl(z - ls), its rounding error recovered exactly (TwoSum) and, with
                // lo, applied to first order -- neither subtraction's rounding (up to |z - lse| u each) reaches the weight
                const float d = z - ls, zp = d + ls, e = (z - zp) + (-ls - (d - zp));
                const float w = expf(d) * (1.f + (e - lo)) - (cid[j] == tl ? 1.f : 0.f);
                if (row < n_q && cid[j] < n_c) out[cid[j]] = dropped ? 0.f : coef * w;
            }
        }
}

// The exclusion lists of the filtered loss, one wave per query and two passes (FILL false: cnt[i] = the length of query
// i's list; a cumulative sum on the host side makes xptr; FILL true: the entries).  Query i walks the known row frow[i]
// (lkg_known.h) 64 entries at a time and keeps an entry iff it is known under relation frel[i], maps to a candidate through
// pos and is not the row's truth.  pos is monotone where it is not -1, so the kept positions come out ascending.
template <bool FILL>
__global__ __launch_bounds__(AE_THREADS) void softmax_excluded_kernel(
    long n_q, long n_rows, long n_c, const long *__restrict__ frow, const long *__restrict__ frel,
    const long *__restrict__ truth, const int *__restrict__ rowptr, const int *__restrict__ col,
    const int *__restrict__ eptr, const int *__restrict__ rel, const int *__restrict__ pos, int *__restrict__ cnt,
    const int *__restrict__ xptr, int *__restrict__ xcol) {
    const long i = (long)blockIdx.x * (AE_THREADS / 64) + (threadIdx.x >> 6);
    if (i >= n_q) return;                           // (a whole wave leaves)
    const int lane = threadIdx.x & 63;
    const long f = min(max(frow[i], 0L), n_rows - 1), tr = truth[i];
    const int want = (int)frel[i];
    const int e0 = rowptr[f], e1 = rowptr[f + 1];
    int base = FILL ? xptr[i] : 0;
    const int stop = FILL ? xptr[i + 1] : 0;
    for (int eb = e0; eb < e1; eb += 64) {          // (uniform trip count in the wave)
        const int e = eb + lane;
        bool keep = false;
        int c = -1;
        if (e < e1) {
            c = known_slot<int>(pos, col[e], n_rows);
            keep = c >= 0 && c < n_c && c != tr && known_under(eptr, rel, e, want);
        }
        const unsigned long long kept = __ballot(keep);
        if (FILL) {
            const int o = base + __popcll(kept & ((1ull << lane) - 1ull));
            if (keep && o < stop) xcol[o] = c;
        }
        base += __popcll(kept);
    }
    if (!FILL && lane == 0) cnt[i] = base;
}

}  // namespace

extern "C" int32_t lkg_softmax_all_splits(int64_t n_q, int64_t n_cand, int32_t requested) {
    if (n_q <= 0 || n_cand <= 0 || requested < 0 || requested > SM_MAX_SPLITS) return 0;
    const long tiles_q = (n_q + AE_ROWS - 1) / AE_ROWS, tiles_c = (n_cand + AE_COLS - 1) / AE_COLS;
    long s_ = requested > 0 ? requested : (2 * 256 + tiles_q - 1) / tiles_q;   // auto: >= 2 workgroups per CU
    s_ = s_ < SM_MAX_SPLITS ? s_ : SM_MAX_SPLITS;
    s_ = s_ < tiles_c ? s_ : tiles_c;
    return (int32_t)(s_ > 1 ? s_ : 1);
}

namespace {

// lkg_softmax_all_partial_f32 (MASKED false: no lists) and lkg_softmax_all_partial_masked_f32: the checks and the launch
template <bool MASKED>
int softmax_partial(const char *name, int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                    int64_t ldp, const float *pn, float scale, int32_t splits, const int32_t *xptr, const int32_t *xcol,
                    int64_t n_excl, float *ws_m, float *ws_l, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand > 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k &&
                    (!MASKED || (n_excl >= 0 && n_excl < INT32_MAX)),
                "%s: bad sizes", name);
    LKG_REQUIRE(scale_ok(scale), "%s: scale must be positive and finite", name);
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(splits >= 1 && splits == lkg_softmax_all_splits(n_q, n_cand, splits),
                "%s: splits must come from lkg_softmax_all_splits", name);
    LKG_REQUIRE(q && p && ws_m && ws_l && (!MASKED || (xptr && (xcol || n_excl == 0))), "%s: null pointer", name);
    const long tiles_q = (n_q + AE_ROWS - 1) / AE_ROWS, tiles_c = (n_cand + AE_COLS - 1) / AE_COLS;
    LKG_REQUIRE(tiles_q * splits < INT32_MAX, "%s: too many workgroups (split the queries)", name);
    const dim3 grid((unsigned)(tiles_q * splits)), block(AE_THREADS);
    const float nsb = neg_scale_beta(scale, pn);
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL((softmax_partial_kernel<decltype(vec)::value, MASKED>), grid, block, 0, (hipStream_t)stream,
                           (long)n_q, (long)n_cand, k, q, (long)ldq, p, (long)ldp, pn, nsb, splits, tiles_q, tiles_c, ws_m,
                           ws_l, xptr, xcol, (int)n_excl);
    });
    LKG_CHECK_LAUNCH(name);
    return LKG_OK;
}

// lkg_softmax_all_weights_f32 and lkg_softmax_all_weights_masked_f32, in the same way
template <bool MASKED>
int softmax_weights(const char *name, int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                    int64_t ldp, const float *pn, int64_t c_base, const int64_t *truth, const float *lse,
                    const float *lse_lo, const float *g, float scale, const int32_t *xptr, const int32_t *xcol,
                    int64_t n_excl, float *v, int64_t ldv, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand >= 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k && ldv >= n_cand &&
                    c_base >= 0 && (!MASKED || (c_base < INT32_MAX && n_excl >= 0 && n_excl < INT32_MAX)),
                "%s: bad sizes", name);
    LKG_REQUIRE(scale_ok(scale), "%s: scale must be positive and finite", name);
    if (n_q == 0 || n_cand == 0) return LKG_OK;
    LKG_REQUIRE(q && p && truth && lse && g && v && (!MASKED || (xptr && (xcol || n_excl == 0))), "%s: null pointer", name);
    const long tiles_q = (n_q + AE_ROWS - 1) / AE_ROWS, tiles_c = (n_cand + AE_COLS - 1) / AE_COLS;
    LKG_REQUIRE(tiles_q * tiles_c < INT32_MAX, "%s: too many tiles (use smaller chunks)", name);
    const dim3 grid((unsigned)(tiles_q * tiles_c)), block(AE_THREADS);
    const float nsb = neg_scale_beta(scale, pn);
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL((softmax_weights_kernel<decltype(vec)::value, MASKED>), grid, block, 0, (hipStream_t)stream,
                           (long)n_q, (long)n_cand, k, q, (long)ldq, p, (long)ldp, pn, (long)c_base, (const long *)truth,
                           lse, lse_lo, g, nsb, -nsb, v, (long)ldv, tiles_q, xptr, xcol, (int)n_excl);
    });
    LKG_CHECK_LAUNCH(name);
    return LKG_OK;
}

}  // namespace

extern "C" int lkg_softmax_all_partial_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                           const float *p, int64_t ldp, const float *pn, float scale, int32_t splits,
                                           float *ws_m, float *ws_l, void *stream) {
    return softmax_partial<false>("lkg_softmax_all_partial_f32", n_q, n_cand, k, q, ldq, p, ldp, pn, scale, splits,
                                  nullptr, nullptr, 0, ws_m, ws_l, stream);
}

extern "C" int lkg_softmax_all_partial_masked_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                                  const float *p, int64_t ldp, const float *pn, float scale,
                                                  int32_t splits, const int32_t *xptr, const int32_t *xcol, int64_t n_excl,
                                                  float *ws_m, float *ws_l, void *stream) {
    return softmax_partial<true>("lkg_softmax_all_partial_masked_f32", n_q, n_cand, k, q, ldq, p, ldp, pn, scale, splits,
                                 xptr, xcol, n_excl, ws_m, ws_l, stream);
}

extern "C" int lkg_softmax_all_finish_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                          const float *p, int64_t ldp, const float *pn, const int64_t *truth, float scale,
                                          int32_t splits, const float *ws_m, const float *ws_l, float *lse, float *lse_lo,
                                          float *loss, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand > 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k,
                "lkg_softmax_all_finish_f32: bad sizes");
    LKG_REQUIRE(scale_ok(scale), "lkg_softmax_all_finish_f32: scale must be positive and finite");
    LKG_REQUIRE(splits >= 1 && splits <= SM_MAX_SPLITS, "lkg_softmax_all_finish_f32: splits must lie in [1, %d]",
                SM_MAX_SPLITS);
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(q && p && truth && ws_m && ws_l && lse && loss, "lkg_softmax_all_finish_f32: null pointer");
    const dim3 grid((unsigned)((n_q + 3) / 4)), block(AE_THREADS);
    const float nsb = neg_scale_beta(scale, pn);
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL(softmax_finish_kernel<decltype(vec)::value>, grid, block, 0, (hipStream_t)stream, (long)n_q,
                           (long)n_cand, k, q, (long)ldq, p, (long)ldp, pn, (const long *)truth, nsb, splits, ws_m, ws_l,
                           lse, lse_lo, loss);
    });
    LKG_CHECK_LAUNCH("lkg_softmax_all_finish_f32");
    return LKG_OK;
}

extern "C" int lkg_softmax_all_weights_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                           const float *p, int64_t ldp, const float *pn, int64_t c_base,
                                           const int64_t *truth, const float *lse, const float *lse_lo, const float *g,
                                           float scale, float *v, int64_t ldv, void *stream) {
    return softmax_weights<false>("lkg_softmax_all_weights_f32", n_q, n_cand, k, q, ldq, p, ldp, pn, c_base, truth, lse,
                                  lse_lo, g, scale, nullptr, nullptr, 0, v, ldv, stream);
}

extern "C" int lkg_softmax_all_weights_masked_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                                  const float *p, int64_t ldp, const float *pn, int64_t c_base,
                                                  const int64_t *truth, const float *lse, const float *lse_lo,
                                                  const float *g, float scale, const int32_t *xptr, const int32_t *xcol,
                                                  int64_t n_excl, float *v, int64_t ldv, void *stream) {
    return softmax_weights<true>("lkg_softmax_all_weights_masked_f32", n_q, n_cand, k, q, ldq, p, ldp, pn, c_base, truth,
                                 lse, lse_lo, g, scale, xptr, xcol, n_excl, v, ldv, stream);
}

extern "C" int lkg_softmax_excluded(int64_t n_q, int64_t n_rows, int64_t n_cand, const int64_t *filter_row,
                                    const int64_t *filter_rel, const int64_t *truth, const int32_t *rowptr,
                                    const int32_t *col, const int32_t *eptr, const int32_t *rel, const int32_t *pos,
                                    int32_t *count, const int32_t *xptr, int32_t *xcol, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_rows > 0 && n_rows < INT32_MAX && n_cand > 0 && n_cand < INT32_MAX,
                "lkg_softmax_excluded: bad sizes");
    LKG_REQUIRE((count && !xptr && !xcol) || (!count && xptr && xcol),
                "lkg_softmax_excluded: either count (first pass) or xptr and xcol (second pass)");
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(filter_row && filter_rel && truth && rowptr && col && eptr && rel, "lkg_softmax_excluded: null pointer");
    const dim3 grid((unsigned)((n_q + 3) / 4)), block(AE_THREADS);
    if (count)
        hipLaunchKernelGGL(softmax_excluded_kernel<false>, grid, block, 0, (hipStream_t)stream, (long)n_q, (long)n_rows,
                           (long)n_cand, (const long *)filter_row, (const long *)filter_rel, (const long *)truth, rowptr,
                           col, eptr, rel, pos, count, xptr, xcol);
    else
        hipLaunchKernelGGL(softmax_excluded_kernel<true>, grid, block, 0, (hipStream_t)stream, (long)n_q, (long)n_rows,
                           (long)n_cand, (const long *)filter_row, (const long *)filter_rel, (const long *)truth, rowptr,
                           col, eptr, rel, pos, count, xptr, xcol);
    LKG_CHECK_LAUNCH("lkg_softmax_excluded");
    return LKG_OK;
}

int lkg_internal_preload_softmax() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&softmax_finish_kernel<true>)) == hipSuccess ? 0 : 1;
}
