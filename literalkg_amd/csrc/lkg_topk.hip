// Filtered top-k link prediction (literalkg_amd/topk.py): for every query q_i select the k candidates c with the smallest
// score  s_c = pn_c - 2 q_i . p_c  (dot scoring: pn = NULL, s_c = -2 q.p), ties broken by the smaller entity id, NaN never
// selected, candidates known for the query dropped.  The B x N scores are never stored.
//
// Arithmetic: exactly that of rank_count_kernel (lkg_rank_common.h: the exact f32 MFMA, the same lane -> k map, zero
// padding past k, the same final fma), so a score here has the bits the ranking kernels compare.
//
// Selection: a 256-thread workgroup owns 64 query rows and a contiguous range of 256-candidate tiles
// (split `split` of S).  Per row it keeps, in LDS, a sorted list of its best kk (s, id) so far -- padded with the
// sentinel (+inf, INT32_MAX), which sorts after every real candidate -- and a queue of TQ candidates waiting to enter it.
// The row's threshold is the list's last entry.  After each tile's MFMAs every lane compares its 64 scores with the
// thresholds of their rows; only those that pass are pushed (an LDS atomic per push).  When a queue fills, the
// workgroup merges every queue into its list: the filter check (known_lookup of lkg_known.h) and a merge by rank, one wave
// per row.  Candidates that did not fit are pushed again against the tightened thresholds.  At the end each list goes to
// workspace [S][n_q][kk]; topk_merge_kernel merges the S lists of a row into the final sorted, padded output.  The result
// is the kk smallest (s, id) of the whole candidate set -- a unique set, whatever S, the query batch or the launch shape.
// The list, the queue and their merge live in lkg_topk_common.h (lkg_pairmlp.hip selects with them too).
#include "lkg_rank_common.h"
#include "lkg_topk_common.h"

namespace {

template <bool VEC, int KC>
__global__ __launch_bounds__(TK_THREADS) void topk_select_kernel(
    long n_q, long n_c, int k, const float *__restrict__ q, long ldq, const float *__restrict__ p, long ldp,
    const float *__restrict__ pn, const long *__restrict__ cand, const long *__restrict__ frow,
    const long *__restrict__ frel, const int *__restrict__ rowptr, const int *__restrict__ col,
    const int *__restrict__ eptr, const int *__restrict__ rel, int kk, int splits, long tiles_q, long tiles_c,
    float *__restrict__ ws_s, int *__restrict__ ws_i) {
    __shared__ TopkSmem<KC> sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * TK_ROWS;
    const int split = (int)(bid / tiles_q);
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    for (int x = tid; x < TK_ROWS * KC; x += TK_THREADS) {
        (&sm.ls[0][0])[x] = __builtin_inff();
        (&sm.li[0][0])[x] = TK_NONE;
    }
    if (tid < TK_ROWS) sm.qn[tid] = 0;
    const float *qrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qrow[i] = q + min(q0 + 16 * i + r, n_q - 1) * ldq;   // rows past the end: never pushed
    unsigned rows_ok = 0;                       // bit 4 i + v: row 16 i + 4 s + v exists
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) rows_ok |= (q0 + 16 * i + 4 * s + v < n_q) ? 1u << (4 * i + v) : 0u;
    __syncthreads();

    for (long t = t_lo; t < t_hi; ++t) {
        const long c0 = t * TK_COLS + wave * 64;
        const float *prow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) prow[i] = p + min(c0 + 16 * i + r, n_c - 1) * ldp;
        f32x4 acc[4][4];
        rank_tile_dots<VEC>(acc, qrow, prow, k, s);
        // acc[i][j][v]: query row 16 i + 4 s + v, candidate c0 + 16 j + r
        float pnv[4];
        int cid[4];
        unsigned cols_ok = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long c = c0 + 16 * j + r;
            const bool ok = c < n_c;
            cols_ok |= ok ? 1u << j : 0u;
            pnv[j] = (pn && ok) ? pn[c] : 0.f;
            cid[j] = ok ? (int)(cand ? cand[c] : c) : TK_NONE;
        }
        // pending bit 4 (4 i + v) + j: the score of (row, candidate) passes its row's threshold and is not queued yet
        unsigned long long pend = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 16 * i + 4 * s + v;
                const float ts = sm.ls[row][kk - 1];
                const int ti = sm.li[row][kk - 1];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sc = __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                    const bool pass = ((rows_ok >> (4 * i + v)) & 1u) && ((cols_ok >> j) & 1u) &&
                                      tk_before(sc, cid[j], ts, ti);
                    pend |= pass ? 1ull << (4 * (4 * i + v) + j) : 0ull;
                }
            }
        while (true) {
            bool full = false;
            if (pend) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int v = 0; v < 4; ++v)
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned long long bit = 1ull << (4 * (4 * i + v) + j);
                            if (pend & bit) {
                                const int row = 16 * i + 4 * s + v;
                                const int slot = atomicAdd(&sm.qn[row], 1);
                                if (slot < TK_QUEUE) {
                                    sm.qs[row][slot] = __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                                    sm.qi[row][slot] = cid[j];
                                    pend &= ~bit;
                                }
                                full |= slot >= TK_QUEUE - 1;
                            }
                        }
            }
            if (!__syncthreads_or(full)) break;        // every push landed, no queue is full
            topk_merge_queues<KC>(sm, kk, q0, n_q, frow, frel, rowptr, col, eptr, rel);
            __syncthreads();
            if (pend) {                                 // re-test what did not land against the new thresholds
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int row = 16 * i + 4 * s + v;
                        const float ts = sm.ls[row][kk - 1];
                        const int ti = sm.li[row][kk - 1];
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const unsigned long long bit = 1ull << (4 * (4 * i + v) + j);
                            const float sc = __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                            if (!tk_before(sc, cid[j], ts, ti)) pend &= ~bit;
                        }
                    }
            }
        }
    }
    __syncthreads();
    topk_merge_queues<KC>(sm, kk, q0, n_q, frow, frel, rowptr, col, eptr, rel);
    __syncthreads();
    for (int x = tid; x < TK_ROWS * kk; x += TK_THREADS) {
        const int row = x / kk, j = x - row * kk;
        if (q0 + row < n_q) {
            const long o = ((long)split * n_q + q0 + row) * kk + j;
            ws_s[o] = sm.ls[row][j];
            ws_i[o] = sm.li[row][j];
        }
    }
}

// One wave per row: lane l < S holds the head of split l's sorted list; kk rounds of a wave-wide (s, id) minimum, the
// winner's lane advancing.  out_s = the kernel score, out_v = the reported one: qn + s (qn non-NULL: squared distance)
// or -s / 2 (the dot product, exact); ids -1 and NaN past the eligible candidates.
__global__ __launch_bounds__(256) void topk_merge_kernel(long n_q, int kk, int splits, const float *__restrict__ ws_s,
                                                         const int *__restrict__ ws_i, const float *__restrict__ qn,
                                                         long *__restrict__ out_id, float *__restrict__ out_s,
                                                         float *__restrict__ out_v) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n_q) return;                          // (a whole wave leaves)
    const int lane = threadIdx.x & 63;
    const float *ls = ws_s + ((long)lane * n_q + row) * kk;
    const int *li = ws_i + ((long)lane * n_q + row) * kk;
    int head = 0;
    float hs = __builtin_inff();
    int hi = TK_NONE;
    if (lane < splits) {
        hs = ls[0];
        hi = li[0];
    }
    const float qnr = qn ? qn[row] : 0.f;
    for (int j = 0; j < kk; ++j) {
        float ms = hs;
        int mi = hi;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const float os = __shfl_xor(ms, off);
            const int oi = __shfl_xor(mi, off);
            if (tk_before(os, oi, ms, mi)) {
                ms = os;
                mi = oi;
            }
        }
        const long o = row * kk + j;
        if (mi == TK_NONE) {                         // every list is exhausted: padding from here on
            for (int x = j + lane; x < kk; x += 64) {
                out_id[row * kk + x] = -1;
                out_s[row * kk + x] = __builtin_nanf("");
                out_v[row * kk + x] = __builtin_nanf("");
            }
            return;
        }
        if (lane == 0) {
            out_id[o] = mi;
            out_s[o] = ms;
            out_v[o] = qn ? qnr + ms : -0.5f * ms;
        }
        if (hi == mi) {                              // ids are distinct: exactly one lane advances
            ++head;
            hs = head < kk ? ls[head] : __builtin_inff();
            hi = head < kk ? li[head] : TK_NONE;
        }
    }
}

template <bool VEC, int KC>
void launch_select(dim3 grid, hipStream_t st, long n_q, long n_c, int k, const float *q, long ldq, const float *p,
                   long ldp, const float *pn, const long *cand, const long *frow, const long *frel, const int *rowptr,
                   const int *col, const int *eptr, const int *rel, int kk, int splits, long tiles_q, long tiles_c,
                   float *ws_s, int *ws_i) {
    hipLaunchKernelGGL((topk_select_kernel<VEC, KC>), grid, dim3(TK_THREADS), 0, st, n_q, n_c, k, q, ldq, p, ldp, pn,
                       cand, frow, frel, rowptr, col, eptr, rel, kk, splits, tiles_q, tiles_c, ws_s, ws_i);
}

template <bool VEC>
void launch_select_kc(dim3 grid, hipStream_t st, long n_q, long n_c, int k, const float *q, long ldq, const float *p,
                      long ldp, const float *pn, const long *cand, const long *frow, const long *frel,
                      const int *rowptr, const int *col, const int *eptr, const int *rel, int kk, int splits,
                      long tiles_q, long tiles_c, float *ws_s, int *ws_i) {
#define LKG_TOPK_LAUNCH(KC)                                                                                          \
    launch_select<VEC, KC>(grid, st, n_q, n_c, k, q, ldq, p, ldp, pn, cand, frow, frel, rowptr, col, eptr, rel, kk, \
                           splits, tiles_q, tiles_c, ws_s, ws_i)
    if (kk <= 16) LKG_TOPK_LAUNCH(16);
    else if (kk <= 32) LKG_TOPK_LAUNCH(32);
    else if (kk <= 64) LKG_TOPK_LAUNCH(64);
    else LKG_TOPK_LAUNCH(128);
#undef LKG_TOPK_LAUNCH
}

}  // namespace

extern "C" int32_t lkg_topk_splits(int64_t n_q, int64_t n_cand, int32_t requested) {
    if (n_q <= 0 || n_cand <= 0 || requested < 0 || requested > TK_MAX_SPLITS) return 0;
    const long tiles_q = (n_q + TK_ROWS - 1) / TK_ROWS, tiles_c = (n_cand + TK_COLS - 1) / TK_COLS;
    long s_ = requested > 0 ? requested : (2 * 256 + tiles_q - 1) / tiles_q;   // auto: >= 2 workgroups per CU
    s_ = s_ < TK_MAX_SPLITS ? s_ : TK_MAX_SPLITS;
    s_ = s_ < tiles_c ? s_ : tiles_c;
    return (int32_t)(s_ > 1 ? s_ : 1);
}

extern "C" int lkg_topk_select_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                   int64_t ldp, const float *pn, const int64_t *cand_ids, const int64_t *filter_row,
                                   const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col,
                                   const int32_t *eptr, const int32_t *rel, int32_t top_k, int32_t splits, float *ws_s,
                                   int32_t *ws_i, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand > 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k,
                "lkg_topk_select_f32: bad sizes");
    LKG_REQUIRE(top_k >= 1 && top_k <= LKG_TOPK_MAX, "lkg_topk_select_f32: top_k must lie in [1, %d]", LKG_TOPK_MAX);
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(splits >= 1 && splits == lkg_topk_splits(n_q, n_cand, splits),
                "lkg_topk_select_f32: splits must come from lkg_topk_splits");
    LKG_REQUIRE(q && p && ws_s && ws_i, "lkg_topk_select_f32: null pointer");
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "lkg_topk_select_f32: incomplete filter");
    const long tiles_q = (n_q + TK_ROWS - 1) / TK_ROWS, tiles_c = (n_cand + TK_COLS - 1) / TK_COLS;
    LKG_REQUIRE(tiles_q * splits < INT32_MAX, "lkg_topk_select_f32: too many workgroups (split the queries)");
    const dim3 grid((unsigned)(tiles_q * splits));
    const hipStream_t st = (hipStream_t)stream;
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        launch_select_kc<decltype(vec)::value>(grid, st, n_q, n_cand, k, q, ldq, p, ldp, pn, (const long *)cand_ids,
                                               (const long *)filter_row, (const long *)filter_rel, rowptr, col, eptr, rel,
                                               top_k, splits, tiles_q, tiles_c, ws_s, ws_i);
    });
    LKG_CHECK_LAUNCH("lkg_topk_select_f32");
    return LKG_OK;
}

extern "C" int lkg_topk_merge_f32(int64_t n_q, int32_t top_k, int32_t splits, const float *ws_s, const int32_t *ws_i,
                                  const float *qn, int64_t *out_ids, float *out_scores, float *out_values,
                                  void *stream) {
    LKG_REQUIRE(n_q >= 0 && top_k >= 1 && top_k <= LKG_TOPK_MAX && splits >= 1 && splits <= TK_MAX_SPLITS,
                "lkg_topk_merge_f32: bad sizes");
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(ws_s && ws_i && out_ids && out_scores && out_values, "lkg_topk_merge_f32: null pointer");
    hipLaunchKernelGGL(topk_merge_kernel, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long)n_q,
                       top_k, splits, ws_s, ws_i, qn, (long *)out_ids, out_scores, out_values);
    LKG_CHECK_LAUNCH("lkg_topk_merge_f32");
    return LKG_OK;
}

int lkg_internal_preload_topk() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&topk_merge_kernel)) == hipSuccess ? 0 : 1;
}
