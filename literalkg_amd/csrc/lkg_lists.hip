// Per-query candidate lists (literalkg_amd/lists.py: score_lists, rank_in_lists, evaluate_list_ranking).  Query i owns
// the M slots lists[i][0 .. M): row numbers of one table of rows p -- P_r for 'transr', the inference table otherwise --
// a negative entry being an empty slot.  The score of (query i, slot j) is the one lkg_rank_count_f32 compares and
// lkg_triple_scores_f32 stores for that (query, candidate): the same bits.
//
// Arithmetic: load4 / mfma_chunk / rank_score of lkg_rank_common.h, unchanged, in rank_pair_scores' shape.  A wave owns
// one query and 16 slots per step: every row of the A operand is the query row q_i (made by lkg_rank_queries_f32),
// column r of B is the row of the slot of lane r = l & 15, and lane (r, s) = (l & 15, l >> 4) loads k-slice s of both.
// Every output element of v_mfma_f32_16x16x4_f32 is a k-ordered fma chain that does not depend on its place in the tile,
// so C[0][r] = acc[0] of lane (r, 0) carries the bits the other kernels produce; the other fifteen rows of C are the
// price (the matrix pipe is not the bound: the kernel gathers one k-float row per slot).  The query row is read again
// with every k-chunk (64 bytes a wave, served by the caches) and never held in registers: k reaches 2048.
//
// Work is cut by (query, slice of LS_SLICE slots): one workgroup of four waves per cut, 64 slots per trip.  Neither a
// few queries with long lists nor many queries with short ones leave the chip idle.  No MFMA sits inside a divergent
// branch and the trip count is uniform in the workgroup: an empty slot or a slot past the end is clamped to row 0,
// computed, and neither stored as a score nor counted.
//
// Counting (lkg_list_count_f32): in its first trip every wave scores the truth of its query beside its slots -- a second
// accumulator on the same query fragments whose B columns are all the truth's row, rank_pair_scores' chain -- the
// lanes (r, 0) compare their slot with it, the workgroup adds up in LDS and then makes one 64-bit atomic add per non-zero
// counter: slices of one query meet in counters the caller zeroed, integers, so no order enters.  No score is stored.
#include "lkg_rank_common.h"
#include "lkg_known.h"

namespace {

constexpr int LS_THREADS = 256;
constexpr int LS_STEP = 64;                      // slots per workgroup and trip: 4 waves x 16
constexpr int LS_SLICE = 256;                    // slots per workgroup: at most 4 trips

constexpr int LS_REPORTED = 1;                   // flags: out = qn + s (pn given) or -s / 2 (dot); else s itself

// One wave's 16 dot products q . p_(slot of lane r), and with TRUTH the dot product q . p_truth beside them on the same
// query fragments: each accumulator is the chain of rank_pair_scores (k-chunks in order, mfma_chunk per chunk).  The
// fragments of the next k-chunk are in flight while this one runs on the matrix pipe (two chunks ahead measured the same).
template <bool VEC, bool TRUTH>
__device__ __forceinline__ void list_dots(f32x4 &acc, f32x4 &acc_t, const float *__restrict__ qrow,
                                          const float *__restrict__ crow, const float *__restrict__ trow, int k, int s) {
    float4 a = load4<VEC>(qrow, 4 * s, k), b = load4<VEC>(crow, 4 * s, k);
    float4 t = TRUTH ? load4<VEC>(trow, 4 * s, k) : f4_zero();
    for (int k0 = 0; k0 < k; k0 += 16) {
        const int kn = k0 + 16 + 4 * s;
        const bool more = k0 + 16 < k;
        const float4 an = more ? load4<VEC>(qrow, kn, k) : f4_zero();
        const float4 bn = more ? load4<VEC>(crow, kn, k) : f4_zero();
        const float4 tn = TRUTH && more ? load4<VEC>(trow, kn, k) : f4_zero();
        mfma_chunk(acc, a, b);
        if (TRUTH) mfma_chunk(acc_t, a, t);
        a = an, b = bn, t = tn;
    }
}

template <bool VEC, bool COUNT>
__global__ __launch_bounds__(LS_THREADS) void list_kernel(
    long m, long n_rows, int k, long slices, const float *__restrict__ q, long ldq, const float *__restrict__ qn,
    const float *__restrict__ p, long ldp, const float *__restrict__ pn, const long *__restrict__ lists, long ld_lists,
    int flags, float *__restrict__ out, long ld_out, const long *__restrict__ truth, const long *__restrict__ cand_ids,
    const long *__restrict__ frow, const long *__restrict__ frel, const int *__restrict__ rowptr,
    const int *__restrict__ col, const int *__restrict__ eptr, const int *__restrict__ rel,
    unsigned long long *__restrict__ better, unsigned long long *__restrict__ equal, unsigned long long *__restrict__ kept) {
    __shared__ int cnt[3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long i = (long)blockIdx.x / slices;                         // the query ...
    const long j0 = ((long)blockIdx.x % slices) * LS_SLICE;           // ... and the first slot of the slice
    const long j1 = j0 + LS_SLICE < m ? j0 + LS_SLICE : m;
    const float *qrow = q + i * ldq;
    const long *list = lists + i * ld_lists;
    long tru = 0;
    if (COUNT) {
        if (tid < 3) cnt[tid] = 0;
        tru = truth[i];
        tru = tru >= 0 && tru < n_rows ? tru : 0L;                    // (the caller hands in rows of p: never out of it)
        __syncthreads();
    }
    const float *trow = p + tru * ldp;
    float thr = 0.f;
    int n_better = 0, n_equal = 0, n_kept = 0;
    for (long base = j0; base < j1; base += LS_STEP) {                // (uniform: the slice's bounds)
        const long j = base + wave * 16 + r;
        const long id = j < j1 ? list[j] : -1L;
        const bool full = id >= 0 && id < n_rows;
        const long row = full ? id : 0L;
        const float *crow = p + row * ldp;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
        if (COUNT && base == j0) {                                    // (uniform) the first trip scores the truth as well:
            f32x4 acc_t = f32x4{0.f, 0.f, 0.f, 0.f};                  // every column of its B operand is the truth's row
            list_dots<VEC, true>(acc, acc_t, qrow, crow, trow, k, s);
            thr = rank_score(acc_t[0], pn, tru);                      // every lane: s(q_i, truth)
        } else {
            list_dots<VEC, false>(acc, acc, qrow, crow, trow, k, s);
        }
        if (s == 0 && j < j1) {                                       // C[0][r] sits in lane (r, 0)
            const float sc = rank_score(acc[0], pn, row);
            if (COUNT) {
                bool keep = full && row != tru;                       // not empty, not the truth itself
                if (keep && rowptr)
                    keep = !known_lookup(rowptr, col, eptr, rel, frow[i], (int)frel[i],
                                         (int)(cand_ids ? cand_ids[row] : row));
                n_kept += keep;
                n_better += keep && sc < thr;                         // (a NaN on either side: neither)
                n_equal += keep && sc == thr;
            } else {
                const float val = (flags & LS_REPORTED) ? (pn ? qn[i] + sc : -0.5f * sc) : sc;
                out[i * ld_out + j] = full ? val : __builtin_nanf("");
            }
        }
    }
    if (!COUNT) return;
    if (n_kept) atomicAdd(&cnt[2], n_kept);
    if (n_better) atomicAdd(&cnt[0], n_better);
    if (n_equal) atomicAdd(&cnt[1], n_equal);
    __syncthreads();
    if (tid == 0 && cnt[0]) atomicAdd(better + i, (unsigned long long)cnt[0]);
    if (tid == 1 && cnt[1]) atomicAdd(equal + i, (unsigned long long)cnt[1]);
    if (tid == 2 && cnt[2]) atomicAdd(kept + i, (unsigned long long)cnt[2]);
}

template <bool COUNT>
int launch_lists(const char *name, int64_t n_q, int64_t m, int64_t n_rows, int32_t k, const float *q, int64_t ldq,
                 const float *qn, const float *p, int64_t ldp, const float *pn, const int64_t *lists, int64_t ld_lists,
                 int32_t flags, float *out, int64_t ld_out, const int64_t *truth, const int64_t *cand_ids,
                 const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col,
                 const int32_t *eptr, const int32_t *rel, int64_t *better, int64_t *equal, int64_t *kept, void *stream) {
    LKG_REQUIRE(n_q >= 0 && m >= 1 && n_rows >= 0 && n_rows < INT32_MAX && k > 0 && ldq >= k && ldp >= k && ld_lists >= m,
                "%s: bad sizes", name);
    LKG_REQUIRE((flags & ~LS_REPORTED) == 0, "%s: unknown flags", name);
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(n_rows >= 1, "%s: lists into an empty table", name);
    LKG_REQUIRE(q && p && lists, "%s: null pointer", name);
    if (COUNT) {
        LKG_REQUIRE(truth && better && equal && kept, "%s: null pointer", name);
        LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "%s: incomplete filter", name);
    } else {
        LKG_REQUIRE(out && ld_out >= m, "%s: null pointer or a row of out shorter than M", name);
        LKG_REQUIRE(!((flags & LS_REPORTED) && pn) || qn, "%s: the reported distance needs qn", name);
    }
    const long slices = (m + LS_SLICE - 1) / LS_SLICE;
    LKG_REQUIRE(slices <= INT32_MAX / n_q, "%s: too many workgroups (split the queries)", name);
    const dim3 grid((unsigned)(n_q * slices)), block(LS_THREADS);
    vec_dispatch(vec_ok(q, ldq, p, ldp), [&](auto vec) {
        hipLaunchKernelGGL((list_kernel<decltype(vec)::value, COUNT>), grid, block, 0, (hipStream_t)stream, (long)m,
                           (long)n_rows, k, slices, q, (long)ldq, qn, p, (long)ldp, pn, (const long *)lists, (long)ld_lists,
                           (int)flags, out, (long)ld_out, (const long *)truth, (const long *)cand_ids,
                           (const long *)filter_row, (const long *)filter_rel, rowptr, col, eptr, rel,
                           (unsigned long long *)better, (unsigned long long *)equal, (unsigned long long *)kept);
    });
    LKG_CHECK_LAUNCH(name);
    return LKG_OK;
}

}  // namespace

extern "C" int lkg_list_scores_f32(int64_t n_q, int64_t m, int64_t n_rows, int32_t k, const float *q, int64_t q_stride,
                                   const float *qn, const float *p, int64_t p_stride, const float *pn, const int64_t *lists,
                                   int64_t lists_stride, int32_t flags, float *out, int64_t out_stride, void *stream) {
    return launch_lists<false>("lkg_list_scores_f32", n_q, m, n_rows, k, q, q_stride, qn, p, p_stride, pn, lists, lists_stride, flags, out,
                               out_stride, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                               nullptr, nullptr, stream);
}

extern "C" int lkg_list_count_f32(int64_t n_q, int64_t m, int64_t n_rows, int32_t k, const float *q, int64_t q_stride,
                                  const float *p, int64_t p_stride, const float *pn, const int64_t *lists, int64_t lists_stride,
                                  const int64_t *truth, const int64_t *cand_ids, const int64_t *filter_row,
                                  const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col, const int32_t *eptr,
                                  const int32_t *rel, int64_t *better, int64_t *equal, int64_t *kept, void *stream) {
    return launch_lists<true>("lkg_list_count_f32", n_q, m, n_rows, k, q, q_stride, nullptr, p, p_stride, pn, lists, lists_stride, 0,
                              nullptr, 0, truth, cand_ids, filter_row, filter_rel, rowptr, col, eptr, rel, better, equal,
                              kept, stream);
}

int lkg_internal_preload_lists() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&list_kernel<true, true>)) == hipSuccess ? 0 : 1;
}
