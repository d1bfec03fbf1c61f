// Threshold retrieval (literalkg_amd/accepted.py): for every query q_i the candidates c whose REPORTED score passes the
// query's threshold and that are not known for it -- the sparse form of a B x N "score above the milestone" matrix, which
// is never stored.
//
// Arithmetic: exactly that of topk_select_kernel (lkg_rank_common.h: rank_tile_dots, the same lane -> k map, zero padding
// past k, the same final fma), so the kernel score s = pn_c - 2 q_i . p_c (dot scoring: pn = NULL, s = -2 q.p) has the
// bits lkg_topk_merge_f32 returns as `scores`; the reported score is formed as that kernel forms it, v = qn_i + s
// (qn non-NULL: the squared distance) or v = -s / 2 (the dot product), and the decision is one f32 compare on it:
// v <= thr_i, or v >= thr_i with `higher`.  A NaN compares false both ways.
//
// Two passes over the same loop.  A 256-thread workgroup owns 64 query rows and a contiguous range of
// 256-candidate tiles (split `split` of S).  After each tile's MFMAs every lane forms its 64 values and compares them
// with the thresholds of their rows (staged in LDS with qn); only a lane with a pass goes on to the filter check
// (known_lookup of lkg_known.h).
//   count: the lane adds its passes to the row's LDS counter; the workgroup leaves with one global add per row.
//   emit : the lane takes a slot from the row's global cursor and writes (id, s, v) at base[row] + slot.  The slot is
//          checked against the row's counted length first: a slot at or past it is NOT written and a flag is raised.
//          Both passes run the same instructions on the same operands, so the flag cannot be raised; the check keeps a
//          disagreement from becoming a store outside the buffer.
// Counts and cursors are integers: the counts are deterministic; a row's entries land in an arbitrary order, which
// lkg_accept_order (lkg_csr_device.hip) then fixes -- (s, id) is unique within a row.
#include "lkg_rank_common.h"
#include "lkg_topk_common.h"

namespace {

constexpr int AC_MAX_SPLITS = LKG_TOPK_MAX_SPLITS;

template <bool VEC, bool EMIT>
__global__ __launch_bounds__(TK_THREADS) void accept_kernel(
    long n_q, long n_c, int k, const float *__restrict__ q, long ldq, const float *__restrict__ p, long ldp,
    const float *__restrict__ pn, const float *__restrict__ qn, const float *__restrict__ thr, int higher,
    const long *__restrict__ cand, const long *__restrict__ frow, const long *__restrict__ frel,
    const int *__restrict__ rowptr, const int *__restrict__ col, const int *__restrict__ eptr,
    const int *__restrict__ rel, int splits, long tiles_q, long tiles_c, int *__restrict__ counts,
    const long *__restrict__ base, int *__restrict__ cursor, long *__restrict__ out_id, float *__restrict__ out_s,
    float *__restrict__ out_v, int *__restrict__ flag) {
    __shared__ float s_qn[TK_ROWS], s_thr[TK_ROWS];
    __shared__ int s_cnt[TK_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * TK_ROWS;
    const int split = (int)(bid / tiles_q);
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    if (tid < TK_ROWS) {
        const long row = min(q0 + tid, n_q - 1);
        s_qn[tid] = qn ? qn[row] : 0.f;
        s_thr[tid] = thr[row];
        s_cnt[tid] = 0;
    }
    const float *qrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qrow[i] = q + min(q0 + 16 * i + r, n_q - 1) * ldq;   // rows past the end: never accepted
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
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = 16 * i + 4 * s + v;
                const float qnr = s_qn[row], th = s_thr[row];
                unsigned pass = 0;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float sc = __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                    const float val = qn ? qnr + sc : -0.5f * sc;
                    const bool ok = higher ? val >= th : val <= th;
                    pass |= ok ? 1u << j : 0u;
                }
                pass &= cols_ok;
                if (!((rows_ok >> (4 * i + v)) & 1u)) pass = 0;
                if (pass) {                                      // rare at the selectivities this is built for
                    const long grow = q0 + row;
                    int n_ok = 0;
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (!((pass >> j) & 1u)) continue;
                        if (rowptr && known_lookup(rowptr, col, eptr, rel, frow[grow], (int)frel[grow], cid[j])) continue;
                        if (EMIT) {
                            const int slot = atomicAdd(cursor + grow, 1);
                            if (slot >= 0 && slot < counts[grow]) {
                                const long o = base[grow] + slot;
                                const float sc = __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                                out_id[o] = cid[j];
                                out_s[o] = sc;
                                out_v[o] = qn ? qnr + sc : -0.5f * sc;
                            } else {
                                atomicOr(flag, 1);
                            }
                        } else {
                            ++n_ok;
                        }
                    }
                    if (!EMIT && n_ok) atomicAdd(&s_cnt[row], n_ok);
                }
            }
    }
    if (!EMIT) {
        __syncthreads();
        if (tid < TK_ROWS && q0 + tid < n_q && s_cnt[tid]) atomicAdd(counts + q0 + tid, s_cnt[tid]);
    }
}

template <bool EMIT>
int launch_accept(const char *name, int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                  int64_t ldp, const float *pn, const float *qn, const float *thr, int32_t higher,
                  const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                  const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t splits, int32_t *counts,
                  const int64_t *base, int32_t *cursor, int64_t *out_ids, float *out_s, float *out_v, int32_t *flag,
                  void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_q < INT32_MAX && n_cand >= 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k,
                "%s: bad sizes", name);
    LKG_REQUIRE(splits >= 0 && splits <= AC_MAX_SPLITS, "%s: splits must lie in [0, %d]", name, AC_MAX_SPLITS);
    if (n_q == 0 || n_cand == 0) return LKG_OK;
    LKG_REQUIRE(q && p && thr && counts, "%s: null pointer", name);
    LKG_REQUIRE((pn == nullptr) == (qn == nullptr), "%s: pn and qn go together (both NULL: dot scoring)", name);
    LKG_REQUIRE(!EMIT || (base && cursor && out_ids && out_s && out_v && flag), "%s: null pointer", name);
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "%s: incomplete filter", name);
    const int s_ = lkg_topk_splits(n_q, n_cand, splits);          // the same split policy as the top-k launch
    LKG_REQUIRE(s_ >= 1, "%s: no split count for these sizes", name);
    const long tiles_q = (n_q + TK_ROWS - 1) / TK_ROWS, tiles_c = (n_cand + TK_COLS - 1) / TK_COLS;
    LKG_REQUIRE(tiles_q * s_ < INT32_MAX, "%s: too many workgroups (split the queries)", name);
    const dim3 grid((unsigned)(tiles_q * s_)), block(TK_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL((accept_kernel<decltype(vec)::value, EMIT>), grid, block, 0, st, (long)n_q, (long)n_cand, k, q,
                           (long)ldq, p, (long)ldp, pn, qn, thr, (int)(higher != 0), (const long *)cand_ids,
                           (const long *)filter_row, (const long *)filter_rel, rowptr, col, eptr, rel, s_, tiles_q, tiles_c,
                           counts, (const long *)base, cursor, (long *)out_ids, out_s, out_v, flag);
    });
    LKG_CHECK_LAUNCH(name);
    return LKG_OK;
}

}  // namespace

extern "C" int lkg_accept_count_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                    int64_t ldp, const float *pn, const float *qn, const float *thr, int32_t higher,
                                    const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                    const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                    int32_t splits, int32_t *counts, void *stream) {
    return launch_accept<false>("lkg_accept_count_f32", n_q, n_cand, k, q, ldq, p, ldp, pn, qn, thr, higher, cand_ids,
                                filter_row, filter_rel, rowptr, col, eptr, rel, splits, counts, nullptr, nullptr, nullptr,
                                nullptr, nullptr, nullptr, stream);
}

extern "C" int lkg_accept_emit_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                   int64_t ldp, const float *pn, const float *qn, const float *thr, int32_t higher,
                                   const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                   const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                   int32_t splits, const int32_t *counts, const int64_t *base, int32_t *cursor,
                                   int64_t *out_ids, float *out_scores, float *out_values, int32_t *flag, void *stream) {
    return launch_accept<true>("lkg_accept_emit_f32", n_q, n_cand, k, q, ldq, p, ldp, pn, qn, thr, higher, cand_ids,
                               filter_row, filter_rel, rowptr, col, eptr, rel, splits, const_cast<int32_t *>(counts), base,
                               cursor, out_ids, out_scores, out_values, flag, stream);
}

int lkg_internal_preload_accept() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&accept_kernel<true, false>)) == hipSuccess ? 0 : 1;
}
