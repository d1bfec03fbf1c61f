// Multi-answer retrieval (literalkg_amd/retrieval.py): the place of EVERY answer of a query in the query's ranked list of
// candidates, from one pass over the candidates per distinct query -- however many answers the query has.
//
// Arithmetic: that of topk_select_kernel / accept_kernel (lkg_rank_common.h: rank_tile_dots, the same lane -> k map, zero
// padding past k, the same final fma), so the kernel score s = pn_c - 2 q . p_c (dot scoring: pn = NULL) has the bits
// lkg_rank_count_f32 compares and lkg_triple_scores_f32 stores.  The answers' keys (s, id) come from
// lkg_triple_scores_f32, sorted by lkg_accept_order: ascending s by float comparison, then ascending id.
//
// A ROW of the kernels is a query vector with a SLICE of at most RT_SLICE consecutive keys of that query's sorted key list
// (DESIGN.md 3.6j).  Bucket g of a row counts the scores x with exactly g of the row's keys before x, for g below the key
// count: x past the last key is dropped, x equal to key g -- the answer itself, scored by the same arithmetic -- is
// skipped.  The inclusive prefix of the buckets up to g is then the number of listed non-answers ahead of key g:
//   prepare: one wave per row.  Bucket 0 starts at MINUS the query's keys in earlier slices (they sort before every key
//            of this slice: the count pass puts them into bucket 0; the keys of later slices fall past the last key).
//            Every filter entry of the query that is a candidate and not one of the query's answers (looked up in the
//            query's WHOLE key list) is scored and taken out of the bucket the count pass will put it into.
//   count  : 256-thread workgroups over 64 rows and a range of 256-candidate tiles; the rows' keys sit in LDS, the buckets
//            too, and leave with one global atomic per non-zero bucket per workgroup.  The scores are never stored.
//   finish : one wave per query: prefix sums inside each slice, position = 1 + before + index, then hits@k, DCG, AP, RR in
//            float64 from a host-built table of 1 / log2(1 + p): sums in an order fixed by the sorted positions.
#include "lkg_rank_common.h"
#include "lkg_topk_common.h"

namespace {

constexpr int RT_SLICE = LKG_RETRIEVAL_SLICE;      // keys per row
constexpr int RT_LD = RT_SLICE + 1;                // LDS row stride (odd: rows of one MFMA column group hit different banks)
static_assert(RT_SLICE >= 2 && (RT_SLICE & (RT_SLICE - 1)) == 0, "the bucket search halves its step");

template <bool VEC>
__global__ __launch_bounds__(TK_THREADS) void retrieval_count_kernel(
    long n_rows, long n_c, int k, const float *__restrict__ q, long ldq, const long *__restrict__ row_q,
    const float *__restrict__ p, long ldp, const float *__restrict__ pn, const long *__restrict__ cand,
    const long *__restrict__ key_off, const int *__restrict__ key_n, const float *__restrict__ key_s,
    const long *__restrict__ key_id, int splits, long tiles_q, long tiles_c, int *__restrict__ buckets) {
    __shared__ float s_ks[TK_ROWS][RT_LD];
    __shared__ int s_ki[TK_ROWS][RT_LD];
    __shared__ int s_cnt[TK_ROWS][RT_LD];
    __shared__ float s_ls[TK_ROWS];                 // the row's last key ((-inf, -1) for a row without keys: nothing passes)
    __shared__ int s_li[TK_ROWS], s_nk[TK_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * TK_ROWS;
    const int split = (int)(bid / tiles_q);
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    for (int x = tid; x < TK_ROWS * RT_SLICE; x += TK_THREADS) {
        const int row = x / RT_SLICE, j = x % RT_SLICE;
        const long grow = q0 + row;
        const int nk = grow < n_rows ? min(max(key_n[grow], 0), RT_SLICE) : 0;
        const bool real = j < nk;
        const long o = real ? key_off[grow] + j : 0;
        const float ks = real ? key_s[o] : __builtin_inff();
        const int ki = real ? (int)key_id[o] : TK_NONE;
        s_ks[row][j] = ks;
        s_ki[row][j] = ki;
        s_cnt[row][j] = 0;
        if (j == 0) {
            s_nk[row] = nk;
            if (nk == 0) {
                s_ls[row] = -__builtin_inff();
                s_li[row] = -1;
            }
        }
        if (real && j == nk - 1) {
            s_ls[row] = ks;
            s_li[row] = ki;
        }
    }
    const float *qrow[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) qrow[i] = q + row_q[min(q0 + 16 * i + r, n_rows - 1)] * ldq;
    __syncthreads();
    // the first step of the bucket search, the same for the whole workgroup: half the smallest power of two that is not
    // below the largest key count (the pads past a row's keys are (+inf, TK_NONE): nothing that passes is after them)
    int nk_max = 0;
    for (int x = 0; x < TK_ROWS; ++x) nk_max = max(nk_max, s_nk[x]);
    int top = 0;
    while (2 * top < nk_max) top = top ? 2 * top : 1;
    top = __builtin_amdgcn_readfirstlane(nk_max > 1 ? top : 0);

    for (long t = t_lo; t < t_hi; ++t) {
        const long c0 = t * TK_COLS + wave * 64;
        const float *prow[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) prow[i] = p + min(c0 + 16 * i + r, n_c - 1) * ldp;
        f32x4 acc[4][4];
        rank_tile_dots<VEC>(acc, qrow, prow, k, s);
        // acc[i][j][v]: row 16 i + 4 s + v, candidate c0 + 16 j + r
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
                const float ls = s_ls[row];
                const int li = s_li[row];
                float sc[4];
                unsigned pass = 0;                  // not NaN and not past the row's last key
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    sc[j] = __builtin_fmaf(-2.f, acc[i][j][v], pnv[j]);
                    pass |= (sc[j] < ls || (sc[j] == ls && cid[j] <= li)) ? 1u << j : 0u;
                }
                pass &= cols_ok;
                if (top == 0) {                     // at most one key per row: whatever passes and is not it, is before it
                    float c = 0.f;
#pragma unroll
                    for (int j = 0; j < 4; ++j) c += (((pass >> j) & 1u) && !(sc[j] == ls && cid[j] == li)) ? 1.f : 0.f;
                    c = group_sum<16>(c);
                    if (r == 0 && c != 0.f) atomicAdd(&s_cnt[row][0], (int)c);
                } else if (pass) {
                    // the keys before (sc, id) among the row's first 2 top - 1: four independent searches, step by step
                    int g[4] = {0, 0, 0, 0};
                    for (int step = top; step >= 1; step >>= 1) {
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const int x = g[j] + step - 1;
                            g[j] += tk_before(s_ks[row][x], s_ki[row][x], sc[j], cid[j]) ? step : 0;
                        }
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const bool self = s_ks[row][g[j]] == sc[j] && s_ki[row][g[j]] == cid[j];       // the answer itself
                        if (((pass >> j) & 1u) && !self) atomicAdd(&s_cnt[row][g[j]], 1);
                    }
                }
            }
    }
    __syncthreads();
    for (int x = tid; x < TK_ROWS * RT_SLICE; x += TK_THREADS) {
        const int row = x / RT_SLICE, j = x % RT_SLICE;
        const int c = s_cnt[row][j];
        if (c && j < s_nk[row]) atomicAdd(buckets + (q0 + row) * RT_SLICE + j, c);        // (nk > 0: the row exists)
    }
}

// lanes 0..15 return s(q, p[cand of lane]) with the counting arithmetic (rank_pair_scores of lkg_rank.hip)
template <bool VEC>
__device__ __forceinline__ float rt_pair_scores(const float *__restrict__ qrow, const float *__restrict__ p, long ldp,
                                                const float *__restrict__ pn, long cand, int k) {
    const int s = (threadIdx.x & 63) >> 4;
    const float *prow = p + cand * ldp;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int k0 = 0; k0 < k; k0 += 16) {
        const float4 a = load4<VEC>(qrow, k0 + 4 * s, k);
        const float4 b = load4<VEC>(prow, k0 + 4 * s, k);
        mfma_chunk(acc, a, b);
    }
    return rank_score(acc[0], pn, cand);
}

template <bool VEC>
__global__ __launch_bounds__(TK_THREADS) void retrieval_prepare_kernel(
    long n_rows, long n_c, int k, const float *__restrict__ q, long ldq, const long *__restrict__ row_q,
    const float *__restrict__ p, long ldp, const float *__restrict__ pn, long n_ids, const int *__restrict__ cand_slot,
    const long *__restrict__ key_off, const int *__restrict__ key_n, const long *__restrict__ qkey_off,
    const long *__restrict__ qkey_n, const float *__restrict__ key_s, const long *__restrict__ key_id,
    const long *__restrict__ frow, const long *__restrict__ frel, const int *__restrict__ rowptr,
    const int *__restrict__ col, const int *__restrict__ eptr, const int *__restrict__ rel, int *__restrict__ buckets) {
    __shared__ int s_b[TK_THREADS / 64][RT_SLICE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r = lane & 15;
    const long i = (long)blockIdx.x * (TK_THREADS / 64) + wave;
    const bool live = i < n_rows;                    // (uniform in the wave)
    long first = 0, koff = 0, qoff = 0, qn = 0;
    int nk = 0;
    if (live) {
        koff = key_off[i];
        nk = min(max(key_n[i], 0), RT_SLICE);
        qoff = qkey_off[i];
        qn = qkey_n[i];
        first = koff - qoff;                         // the query's keys in earlier slices
        if (lane < RT_SLICE) s_b[wave][lane] = lane == 0 ? -(int)first : 0;
    }
    __syncthreads();
    if (live && rowptr) {
        const float *qrow = q + row_q[i] * ldq;
        const long f = min(max(frow[i], 0L), n_ids - 1);
        const int want = (int)frel[i];
        const int e0 = rowptr[f], e1 = rowptr[f + 1];
        for (int eb = e0; eb < e1; eb += 16) {       // 16 filter entries per pass (uniform trip count in the wave)
            const int e = eb + r;
            long slot = 0;
            int id = -1;
            bool keep = false;
            if (e < e1) {
                id = col[e];
                if (id >= 0 && id < n_ids) {
                    const long sl = cand_slot ? cand_slot[id] : id;
                    if (sl >= 0 && sl < n_c) {
                        slot = sl;
                        keep = known_under(eptr, rel, e, want);
                    }
                }
            }
            const float sc = rt_pair_scores<VEC>(qrow, p, ldp, pn, slot, k);
            if (lane < 16 && keep && sc == sc) {
                long lo = 0, hi = qn;                // the query's keys before (sc, id)
                while (lo < hi) {
                    const long mid = (lo + hi) >> 1;
                    if (tk_before(key_s[qoff + mid], (int)key_id[qoff + mid], sc, id)) lo = mid + 1;
                    else hi = mid;
                }
                const bool answer = lo < qn && key_s[qoff + lo] == sc && (int)key_id[qoff + lo] == id;
                const long g = max(lo - first, 0L);
                if (!answer && g < nk) atomicAdd(&s_b[wave][g], -1);
            }
        }
    }
    __syncthreads();
    if (live && lane < RT_SLICE) buckets[i * RT_SLICE + lane] = s_b[wave][lane];
}

__device__ __forceinline__ double rt_wave_sum(double v) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
    return v;
}

// the number of listed non-answers before key `lane` of the slice held by `row`: the inclusive prefix of its buckets
__device__ __forceinline__ long rt_slice_before(const int *__restrict__ buckets, long row, int lane, bool mine) {
    long b = mine ? (long)buckets[row * RT_SLICE + lane] : 0L;
#pragma unroll
    for (int d = 1; d < RT_SLICE; d <<= 1) {
        const long o = __shfl_up(b, d);
        if (lane >= d) b += o;
    }
    return b;
}

// One wave per query; lane l < RT_SLICE holds key l of each slice in turn, so a lane's partial sums take the keys
// l, l + RT_SLICE, ... in order and the wave's partial sums meet in a fixed butterfly.
__global__ __launch_bounds__(256) void retrieval_finish_kernel(
    long n_q, const long *__restrict__ qkey_ptr, const long *__restrict__ row_base, const long *__restrict__ n_answers,
    const int *__restrict__ buckets, int n_ks, const long *__restrict__ ks, long k_tab, const double *__restrict__ disc,
    const double *__restrict__ icum, long *__restrict__ before, long *__restrict__ position, long *__restrict__ hits,
    double *__restrict__ ndcg, double *__restrict__ ap, double *__restrict__ rr) {
    const long u = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= n_q) return;                            // (a whole wave leaves)
    const int lane = threadIdx.x & 63;
    const long k0 = qkey_ptr[u], m_keys = qkey_ptr[u + 1] - k0, rb = row_base[u];
    double s_ap = 0.0, first_rr = 0.0;
    for (long j0 = 0; j0 < m_keys; j0 += RT_SLICE) {
        const bool mine = lane < RT_SLICE && j0 + lane < m_keys;
        const long b = rt_slice_before(buckets, rb + j0 / RT_SLICE, lane, mine);
        if (mine) {
            const long pos = 1 + b + j0 + lane;
            before[k0 + j0 + lane] = b;
            position[k0 + j0 + lane] = pos;
            s_ap += (double)(j0 + lane + 1) / (double)pos;
            if (j0 + lane == 0) first_rr = 1.0 / (double)pos;
        }
    }
    if (!hits) return;
    const long m = n_answers[u];
    s_ap = rt_wave_sum(s_ap);
    if (lane == 0) {
        ap[u] = m > 0 ? s_ap / (double)m : 0.0;
        rr[u] = first_rr;
    }
    for (int x = 0; x < n_ks; ++x) {
        const long kk = ks[x];
        long h = 0;
        double d = 0.0;
        for (long j0 = 0; j0 < m_keys; j0 += RT_SLICE) {
            const bool mine = lane < RT_SLICE && j0 + lane < m_keys;
            const long pos = 1 + rt_slice_before(buckets, rb + j0 / RT_SLICE, lane, mine) + j0 + lane;
            if (mine && pos <= kk) {
                ++h;
                d += disc[min(pos, k_tab)];
            }
        }
        d = rt_wave_sum(d);
#pragma unroll
        for (int mm = 1; mm < 64; mm <<= 1) h += __shfl_xor(h, mm);
        if (lane == 0) {
            hits[u * n_ks + x] = h;
            const long ideal = min(min(m, kk), k_tab);
            ndcg[u * n_ks + x] = ideal > 0 ? d / icum[ideal] : 0.0;
        }
    }
}

}  // namespace

extern "C" int lkg_retrieval_prepare_f32(int64_t n_rows, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                         const int64_t *row_q, const float *p, int64_t ldp, const float *pn,
                                         int64_t n_ids, const int32_t *cand_slot, const int64_t *key_off,
                                         const int32_t *key_n, const int64_t *qkey_off, const int64_t *qkey_n,
                                         const float *key_s, const int64_t *key_id, const int64_t *filter_row,
                                         const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col,
                                         const int32_t *eptr, const int32_t *rel, int32_t *buckets, void *stream) {
    LKG_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX && n_cand > 0 && n_cand < INT32_MAX && n_ids > 0 && n_ids < INT32_MAX &&
                    k > 0 && ldq >= k && ldp >= k,
                "lkg_retrieval_prepare_f32: bad sizes");
    if (n_rows == 0) return LKG_OK;
    LKG_REQUIRE(q && row_q && p && key_off && key_n && qkey_off && qkey_n && key_s && key_id && buckets,
                "lkg_retrieval_prepare_f32: null pointer");
    LKG_REQUIRE(cand_slot || n_ids == n_cand, "lkg_retrieval_prepare_f32: without cand_slot the ids are the candidate rows");
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "lkg_retrieval_prepare_f32: incomplete filter");
    const dim3 grid((unsigned)((n_rows + 3) / 4)), block(TK_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL(retrieval_prepare_kernel<decltype(vec)::value>, grid, block, 0, st, (long)n_rows, (long)n_cand,
                           k, q, (long)ldq, (const long *)row_q, p, (long)ldp, pn, (long)n_ids, cand_slot,
                           (const long *)key_off, key_n, (const long *)qkey_off, (const long *)qkey_n, key_s,
                           (const long *)key_id, (const long *)filter_row, (const long *)filter_rel, rowptr, col, eptr, rel,
                           buckets);
    });
    LKG_CHECK_LAUNCH("lkg_retrieval_prepare_f32");
    return LKG_OK;
}

extern "C" int lkg_retrieval_count_f32(int64_t n_rows, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                                       const int64_t *row_q, const float *p, int64_t ldp, const float *pn,
                                       const int64_t *cand_ids, const int64_t *key_off, const int32_t *key_n,
                                       const float *key_s, const int64_t *key_id, int32_t *buckets, void *stream) {
    LKG_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX && n_cand >= 0 && n_cand < INT32_MAX && k > 0 && ldq >= k && ldp >= k,
                "lkg_retrieval_count_f32: bad sizes");
    if (n_rows == 0 || n_cand == 0) return LKG_OK;
    LKG_REQUIRE(q && row_q && p && key_off && key_n && key_s && key_id && buckets, "lkg_retrieval_count_f32: null pointer");
    const int s_ = lkg_topk_splits(n_rows, n_cand, 0);            // the split policy of the top-k launch
    LKG_REQUIRE(s_ >= 1, "lkg_retrieval_count_f32: no split count for these sizes");
    const long tiles_q = (n_rows + TK_ROWS - 1) / TK_ROWS, tiles_c = (n_cand + TK_COLS - 1) / TK_COLS;
    LKG_REQUIRE(tiles_q * s_ < INT32_MAX, "lkg_retrieval_count_f32: too many workgroups (split the rows)");
    const dim3 grid((unsigned)(tiles_q * s_)), block(TK_THREADS);
    const hipStream_t st = (hipStream_t)stream;
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL(retrieval_count_kernel<decltype(vec)::value>, grid, block, 0, st, (long)n_rows, (long)n_cand, k,
                           q, (long)ldq, (const long *)row_q, p, (long)ldp, pn, (const long *)cand_ids,
                           (const long *)key_off, key_n, key_s, (const long *)key_id, s_, tiles_q, tiles_c, buckets);
    });
    LKG_CHECK_LAUNCH("lkg_retrieval_count_f32");
    return LKG_OK;
}

extern "C" int lkg_retrieval_finish(int64_t n_q, const int64_t *qkey_ptr, const int64_t *row_base,
                                    const int64_t *n_answers, const int32_t *buckets, int32_t n_ks, const int64_t *ks,
                                    int64_t k_tab, const double *disc, const double *icum, int64_t *before,
                                    int64_t *position, int64_t *hits, double *ndcg, double *ap, double *rr, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_q < INT32_MAX && n_ks >= 0 && k_tab >= 0, "lkg_retrieval_finish: bad sizes");
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(qkey_ptr && row_base && buckets && before && position, "lkg_retrieval_finish: null pointer");
    LKG_REQUIRE(!hits || (n_answers && ndcg && ap && rr && (n_ks == 0 || (ks && disc && icum))),
                "lkg_retrieval_finish: the metrics need n_answers, ks, the tables and every output");
    hipLaunchKernelGGL(retrieval_finish_kernel, dim3((unsigned)((n_q + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (long)n_q, (const long *)qkey_ptr, (const long *)row_base, (const long *)n_answers, buckets, n_ks,
                       (const long *)ks, (long)k_tab, disc, icum, (long *)before, (long *)position, (long *)hits, ndcg, ap,
                       rr);
    LKG_CHECK_LAUNCH("lkg_retrieval_finish");
    return LKG_OK;
}

int lkg_internal_preload_retrieval() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&retrieval_finish_kernel)) == hipSuccess ? 0 : 1;
}
