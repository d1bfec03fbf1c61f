// The relation slot of a triple (literalkg_amd/relations.py: score_relations, rank_relations, predict_relations,
// evaluate_relation_prediction): the score of (h, j, t) for every relation j of a chunk in one launch, and the filtered
// counts / top-k over the stored row of scores.
//
// relation_scores_kernel is triple_scores_kernel (lkg_triples.hip) with TS_REPORTED and a relation loop inside: load4 /
// mfma_chunk of lkg_rank_common.h with the unchanged lane -> k map and zero padding, a wave owning 16 pairs, lane (r, s) =
// (l & 15, l >> 4) loading k-slice s of ITS pair r's query row and candidate row, the query formed in-lane as
// fmaf(alpha, e_j[c], x[c]), the diagonal C[r][r] read from lane (r, r >> 2), |q|^2 in lkg_rank_sqnorm_f32's order (lane c
// takes c, c + 64, ... as one fma chain, then wave_sum), the score rank_score's one fma and the reported distance one add.
// Every operation a pair's score goes through is the one lkg_triple_scores_f32 performs for (pair, relation j), in the
// same order: the bits are the same.  Relation j reads the table at p + j * rel_stride (rel_stride 0: one shared table)
// and the squared norms at pn + j * pn_stride.
//
// The rows of a pair are NOT held in registers across relations: a k = 300 row pair is 19 k-chunks x 8 floats = 152
// VGPRs per lane with a k known only at run time, which would need one kernel per width and leave no room for the loads in
// flight; for the shared table ('transe') relation j > 0 re-reads the two rows the wave fetched a moment ago, which the
// caches serve (each wave touches 32 rows x 1.2 KB = 38 KB between re-reads).  The projected tables ('transr') differ per
// relation, so nothing could be kept there.
//
// No MFMA sits inside a divergent branch; the trip count and the relation loop are uniform in the workgroup: pairs past the
// end are clamped to the last pair, computed and not stored.
//
// relation_order_kernel: one wave per pair, the pair's row of scores staged in LDS.  A relation under which the pair is
// known is dropped by overwriting its staged score with NaN -- a NaN is never selected and counts nowhere, so the dropped
// and the NaN relations share one rule, and duplicates or the order of the raw edges cannot matter.  The truth's own score
// is read from the stored row, so a known truth keeps it, and the truth is skipped by id.  The selection is top_k rounds
// of a wave arg-min over (score, id): every lane keeps the best of its own elements (j = lane, lane + 64, ...), the wave
// reduces, the winner's slot becomes NaN and only its lane rescans.  Compares and integer adds only: no rounding enters.
#include "lkg_known.h"
#include "lkg_rank_common.h"

#include <climits>

namespace {

constexpr int RS_THREADS = 256;
constexpr int RS_PAIRS = 64;                     // per workgroup and trip: 4 waves x 16
constexpr long RS_GRID = 4096;                   // workgroups at most

constexpr int RO_THREADS = 256;
constexpr int RO_WAVES = RO_THREADS / 64;        // pairs per workgroup and trip: one per wave
constexpr int RO_MAX_REL = LKG_RELATION_MAX;     // RO_WAVES rows of this many floats are the 64 KB of LDS a workgroup may ask for
constexpr long RO_GRID = 8192;                   // workgroups at most
constexpr int RO_NONE = INT_MAX;                 // the sentinel id: no eligible relation

template <bool VEC>
__device__ __forceinline__ float4 rel_query4(const float *__restrict__ x, const float *__restrict__ er, float alpha, int kk,
                                             int k) {
    float4 a = load4<VEC>(x, kk, k);
    const float4 ev = load4<VEC>(er, kk, k);
    a.x = __builtin_fmaf(alpha, ev.x, a.x);
    a.y = __builtin_fmaf(alpha, ev.y, a.y);
    a.z = __builtin_fmaf(alpha, ev.z, a.z);
    a.w = __builtin_fmaf(alpha, ev.w, a.w);
    return a;
}

template <bool VEC>
__global__ __launch_bounds__(RS_THREADS) void relation_scores_kernel(
    long n, int k, int n_rel, const float *__restrict__ p, long ldp, long rel_stride, const float *__restrict__ pn,
    long pn_stride, const long *__restrict__ q_idx, const long *__restrict__ c_idx, const float *__restrict__ e, long lde,
    float alpha, float *__restrict__ out, long ldo) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    for (long base = (long)blockIdx.x * RS_PAIRS; base < n; base += (long)gridDim.x * RS_PAIRS) {
        const long t0 = base + wave * 16;
        const long tr = t0 + r < n ? t0 + r : n - 1;
        const long qi = q_idx[tr], ci = c_idx[tr];
        for (int j = 0; j < n_rel; ++j) {                             // (uniform: a kernel argument)
            const float *pj = p + (long)j * rel_stride;
            const float *pnj = pn + (long)j * pn_stride;
            const float *erow = e + (long)j * lde;
            const float *xrow = pj + qi * ldp;
            const float *crow = pj + ci * ldp;
            f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
            float4 a = rel_query4<VEC>(xrow, erow, alpha, 4 * s, k);
            float4 b = load4<VEC>(crow, 4 * s, k);
            for (int k0 = 0; k0 < k; k0 += 16) {
                const int kn = k0 + 16 + 4 * s;
                const bool more = k0 + 16 < k;
                const float4 an = more ? rel_query4<VEC>(xrow, erow, alpha, kn, k) : f4_zero();   // in flight during the MFMAs
                const float4 bn = more ? load4<VEC>(crow, kn, k) : f4_zero();
                mfma_chunk(acc, a, b);
                a = an;
                b = bn;
            }
            float qn = 0.f;
            for (int i = 0; i < 16; ++i) {                            // pair i of the wave, rank_sqnorm_kernel's order
                const long qq = __shfl(qi, i, 64);
                const float *x = pj + qq * ldp;
                float sq = 0.f;
                for (int c = lane; c < k; c += 64) {
                    const float y = __builtin_fmaf(alpha, erow[c], x[c]);
                    sq = __builtin_fmaf(y, y, sq);
                }
                sq = wave_sum(sq);
                if (r == i) qn = sq;
            }
            if (s == (r >> 2) && t0 + r < n) {                        // the diagonal: C[r][r] = acc[r & 3] of lane (r, r >> 2)
                const int v = r & 3;
                const float dot = v == 0 ? acc[0] : v == 1 ? acc[1] : v == 2 ? acc[2] : acc[3];
                out[(t0 + r) * ldo + j] = qn + rank_score(dot, pnj, ci);
            }
        }
    }
}

// (a, ia) before (b, ib): ascending score, ties to the smaller id; false whenever a is NaN
__device__ __forceinline__ bool ro_before(float a, int ia, float b, int ib) { return a < b || (a == b && ia < ib); }

// the best (score, id) among the lane's own elements of the staged row; (+inf, RO_NONE) when it has none
__device__ __forceinline__ void ro_lane_best(const float *__restrict__ row, int n_rel, int lane, float &bs, int &bi) {
    bs = __builtin_inff();
    bi = RO_NONE;
    for (int j = lane; j < n_rel; j += 64) {
        const float x = row[j];
        if (ro_before(x, j, bs, bi)) {
            bs = x;
            bi = j;
        }
    }
}

__global__ __launch_bounds__(RO_THREADS) void relation_order_kernel(
    long n, int n_rel, const float *__restrict__ scores, long lds, const long *__restrict__ truth,
    const long *__restrict__ filter_row, const long *__restrict__ filter_col, const int *__restrict__ rowptr,
    const int *__restrict__ col, const int *__restrict__ eptr, const int *__restrict__ rel, int top_k,
    int *__restrict__ better, int *__restrict__ equal, long *__restrict__ top_ids, float *__restrict__ top_scores) {
    extern __shared__ float ro_rows[];                                // RO_WAVES rows of n_rel floats
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *row = ro_rows + (long)wave * n_rel;
    for (long i = (long)blockIdx.x * RO_WAVES + wave; i < n; i += (long)gridDim.x * RO_WAVES) {   // (uniform in the wave)
        const float *src = scores + i * lds;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");        // the previous pair's reads of the row are done
        for (int j = lane; j < n_rel; j += 64) row[j] = src[j];
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (rowptr) {
            const long f = filter_row[i];
            const long want = filter_col[i];
            int en;
            if (known_find(col, rowptr[f], rowptr[f + 1], want, en)) {
                const int x1 = eptr[en + 1];
                for (int x = eptr[en] + lane; x < x1; x += 64) {
                    const int rr = rel[x];
                    if (rr >= 0 && rr < n_rel) row[rr] = __builtin_nanf("");    // (duplicates write the same bits)
                }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        }
        if (truth) {
            const long tj = truth[i];
            const float ts = (tj >= 0 && tj < n_rel) ? src[tj] : __builtin_nanf("");   // a NaN truth compares false everywhere
            int nb = 0, ne = 0;
            for (int j = lane; j < n_rel; j += 64) {
                const float x = row[j];
                const bool other = j != tj;
                nb += (other && x < ts) ? 1 : 0;
                ne += (other && x == ts) ? 1 : 0;
            }
            for (int m = 1; m < 64; m <<= 1) {
                nb += __shfl_xor(nb, m, 64);
                ne += __shfl_xor(ne, m, 64);
            }
            if (lane == 0) {
                better[i] = nb;
                equal[i] = ne;
            }
        }
        if (top_k > 0) {
            float bs;
            int bi;
            ro_lane_best(row, n_rel, lane, bs, bi);
            bool live = true;                                         // (uniform in the wave)
            for (int round = 0; round < top_k; ++round) {
                float ws = bs;
                int wi = bi;
                if (live) {
                    for (int m = 1; m < 64; m <<= 1) {
                        const float os = __shfl_xor(ws, m, 64);
                        const int oi = __shfl_xor(wi, m, 64);
                        if (ro_before(os, oi, ws, wi)) {
                            ws = os;
                            wi = oi;
                        }
                    }
                    live = wi != RO_NONE;
                }
                if (!live) {                                          // fewer eligible relations than top_k: the padding
                    if (lane == 0) {
                        top_ids[i * top_k + round] = -1;
                        top_scores[i * top_k + round] = __builtin_nanf("");
                    }
                    continue;
                }
                if (lane == 0) {
                    top_ids[i * top_k + round] = wi;
                    top_scores[i * top_k + round] = ws;
                }
                if ((wi & 63) == lane) {                              // the winner leaves the row; its lane looks again
                    row[wi] = __builtin_nanf("");
                    ro_lane_best(row, n_rel, lane, bs, bi);
                }
            }
        }
    }
}

}  // namespace

extern "C" int lkg_relation_scores_f32(int64_t n, int32_t k, int32_t n_rel, const float *p, int64_t ldp,
                                       int64_t rel_stride, const float *pn, int64_t pn_stride, const int64_t *q_idx,
                                       const int64_t *c_idx, const float *e, int64_t lde, float alpha, float *out,
                                       int64_t ldo, void *stream) {
    LKG_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX - 1 && k > 0 && n_rel >= 0 && ldp >= k && lde >= k && ldo >= n_rel &&
                    rel_stride >= 0 && pn_stride >= 0,
                "lkg_relation_scores_f32: bad sizes");
    LKG_REQUIRE((rel_stride == 0) == (pn_stride == 0),
                "lkg_relation_scores_f32: rel_stride and pn_stride are both zero (one shared table) or both positive");
    if (n == 0 || n_rel == 0) return LKG_OK;
    LKG_REQUIRE(p && pn && q_idx && c_idx && e && out, "lkg_relation_scores_f32: null pointer");
    const long blocks = (n + RS_PAIRS - 1) / RS_PAIRS;
    const dim3 grid((unsigned)(blocks < RS_GRID ? blocks : RS_GRID)), block(RS_THREADS);
    vec_dispatch(vec_ok(p, ldp, e, lde) && rel_stride % 4 == 0, [&](auto vec) {
        hipLaunchKernelGGL(relation_scores_kernel<decltype(vec)::value>, grid, block, 0, (hipStream_t)stream, (long)n, k,
                           (int)n_rel, p, (long)ldp, (long)rel_stride, pn, (long)pn_stride, (const long *)q_idx,
                           (const long *)c_idx, e, (long)lde, alpha, out, (long)ldo);
    });
    LKG_CHECK_LAUNCH("lkg_relation_scores_f32");
    return LKG_OK;
}

extern "C" int lkg_relation_order_f32(int64_t n, int32_t n_rel, const float *scores, int64_t lds, const int64_t *truth,
                                      const int64_t *filter_row, const int64_t *filter_col, const int32_t *rowptr,
                                      const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t top_k,
                                      int32_t *better, int32_t *equal, int64_t *top_ids, float *top_scores,
                                      void *stream) {
    LKG_REQUIRE(n >= 0 && n <= (int64_t)INT32_MAX - 1 && n_rel >= 1 && n_rel <= RO_MAX_REL && lds >= n_rel,
                "lkg_relation_order_f32: bad sizes (1 <= n_rel <= %d: a workgroup stages %d rows of scores in 64 KB of LDS)",
                RO_MAX_REL, RO_WAVES);
    LKG_REQUIRE(top_k >= 0 && top_k <= LKG_TOPK_MAX, "lkg_relation_order_f32: top_k outside [0, %d]", LKG_TOPK_MAX);
    LKG_REQUIRE(truth || top_k > 0, "lkg_relation_order_f32: nothing to compute (no truth, top_k = 0)");
    LKG_REQUIRE(!truth || (better && equal), "lkg_relation_order_f32: a truth needs better and equal (null pointer)");
    LKG_REQUIRE(top_k == 0 || (top_ids && top_scores), "lkg_relation_order_f32: top_k needs top_ids and top_scores");
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_col, col, eptr, rel),
                "lkg_relation_order_f32: a filter needs filter_row, filter_col, col, eptr and rel (null pointer)");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(scores, "lkg_relation_order_f32: null pointer");
    const long blocks = (n + RO_WAVES - 1) / RO_WAVES;
    const dim3 grid((unsigned)(blocks < RO_GRID ? blocks : RO_GRID)), block(RO_THREADS);
    const size_t smem = (size_t)RO_WAVES * (size_t)n_rel * sizeof(float);
    hipLaunchKernelGGL(relation_order_kernel, grid, block, smem, (hipStream_t)stream, (long)n, (int)n_rel, scores,
                       (long)lds, (const long *)truth, (const long *)filter_row, (const long *)filter_col, rowptr, col, eptr,
                       rel, (int)top_k, better, equal, (long *)top_ids, top_scores);
    LKG_CHECK_LAUNCH("lkg_relation_order_f32");
    return LKG_OK;
}

// lkg_preload(): HIP loads a translation unit's code object on the first use of one of its kernels; asking for a kernel's
// attributes is such a use (no launch).
int lkg_internal_preload_relations() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&relation_scores_kernel<true>)) == hipSuccess ? 0 : 1;
}
