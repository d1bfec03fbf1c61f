// The MLP pair head at inference (literalkg_amd/pairmlp.py): logits of every (query, candidate) pair, and the filtered
// top-k of them per query, from the two PROJECTED tables of the head's first layer; and, further down, the filtered rank
// counts of held-out pairs (prepare + count), which compare those logits instead of storing them; and the logits and
// confusion counts of an explicit list of pairs (pairs), every row of the A operand a pair of its own.
//
// With BatchNorm in inference form folded forward the head is
//     x1 = relu(u_q + v_c)                      u = Uq row (128, bias included), v = V row (128)
//     x2 = relu(W2' x1 + b2')                   W2' 64 x 128
//     z  = w3' . x2 + b3'                       the logit
// fc2 is 16 384 FLOP per pair and runs on the exact-f32 MFMA v_mfma_f32_16x16x4_f32: the A operand is x1 for 16
// candidates of one query, formed on the fly, the B operand W2'^T, register-resident (32 k-steps x 4 column blocks = 128
// VGPRs per lane).  A wave owns 16 candidates at a time: their V rows sit in 32 VGPRs (lane (r, s) = (l & 15, l >> 4)
// holds elements 16 t + 4 s .. + 3, t = 0..7, of candidate r's row) while the wave walks the workgroup's query rows,
// whose u rows are staged once in LDS and read as broadcasts.  So a V row is read from memory once per workgroup and
// candidate, a u row once per workgroup, and the per-pair work touches registers and LDS only.
//
// Position independence: a pair's logit is a fixed sequence of f32 operations on (u row, v row, folded weights) --
// k order 16 t + {0, 4, 8, 12} + e for e = 0..3, t = 0..7 (the order of lkg_rank_common.h); the epilogue's in-lane fma
// chain over the 4 column blocks, then the xor butterfly over the 16 lanes of a row -- whatever tile, wave, row, split
// or launch computes it, and the same in every epilogue and for either source of the A rows (all go through
// pm_logits_of).
//
// Selection: the state and the merge of lkg_topk_common.h, fed s = -2 z (exact), so ascending s is descending logit and
// lkg_topk_merge_f32 reports -s / 2 = z.  After the lane reduction one lane holds a pair's logit; it is pushed when it
// passes its row's threshold.  A tile brings a row at most 64 candidates and the queues (64 slots) are merged after
// every tile, so a push always lands.
#include "lkg_rank_common.h"
#include "lkg_topk_common.h"

namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_H1 = 128;           // fc1 outputs = fc2 inputs
constexpr int PM_H2 = 64;            // fc2 outputs
constexpr int PM_ROWS = 64;          // query rows per workgroup (at most; TK_ROWS lists)
constexpr int PM_COLS = 64;          // candidates per tile: 16 per wave
constexpr int PM_STORE_TILES = 8;    // candidate tiles per workgroup of the store kernel
static_assert(PM_ROWS == TK_ROWS && PM_COLS <= TK_QUEUE, "one tile must fit the queues");

struct PairWeights {
    float4 b[PM_H1 / 16][PM_H2 / 16];   // b[t][j]: W2'[16 j + r][16 t + 4 s .. + 3]
    float b2[PM_H2 / 16], w3[PM_H2 / 16];   // element 16 j + r
    float b3;
};

__device__ __forceinline__ void pm_load_weights(PairWeights &w, const float *__restrict__ w2,
                                                const float *__restrict__ b2, const float *__restrict__ w3,
                                                const float *__restrict__ b3, int r, int s) {
#pragma unroll
    for (int t = 0; t < PM_H1 / 16; ++t)
#pragma unroll
        for (int j = 0; j < PM_H2 / 16; ++j)
            w.b[t][j] = *reinterpret_cast<const float4 *>(w2 + (16 * j + r) * PM_H1 + 16 * t + 4 * s);
#pragma unroll
    for (int j = 0; j < PM_H2 / 16; ++j) {
        w.b2[j] = b2[16 * j + r];
        w.w3[j] = w3[16 * j + r];
    }
    w.b3 = b3[0];
}

__device__ __forceinline__ float pm_relu(float x) { return x < 0.f ? 0.f : x; }      // (NaN stays NaN)

// the wave's 16 V rows: vf[t] = elements 16 t + 4 s .. + 3 of row `vrow`
__device__ __forceinline__ void pm_load_v(float4 (&vf)[PM_H1 / 16], const float *__restrict__ vrow, int s) {
#pragma unroll
    for (int t = 0; t < PM_H1 / 16; ++t) vf[t] = *reinterpret_cast<const float4 *>(vrow + 16 * t + 4 * s);
}

// Opens candidate tile t for the wave: vf = its 16 V rows (rows past the end repeat the last one: computed, never
// used), cw = the candidate that lane (r < 4, s) speaks for; true when the lane speaks for one
__device__ __forceinline__ bool pm_open_tile(float4 (&vf)[PM_H1 / 16], long &cw, long t, int wave, int r, int s,
                                             const float *__restrict__ vt, long ldv, long n_c) {
    const long c0 = t * PM_COLS + wave * 16;
    const long crow = c0 + r < n_c ? c0 + r : n_c - 1;
    pm_load_v(vf, vt + crow * ldv, s);
    cw = c0 + 4 * s + (r & 3);
    return r < 4 && cw < n_c;
}

// Where row r of the A operand comes from: x1(t) = elements 16 t + 4 s .. + 3 of relu(u + v) for the lane's row.
// PmBroadcastU: one u row in LDS for all 16 candidates (the query of the store / select / count / prepare kernels).
// PmOwnX: every row a pair of its own, its relu(u + v) already formed from the lane's own u and v fragments.
struct PmBroadcastU {
    const float *urow;
    const float4 (&vf)[PM_H1 / 16];
    int s;
    __device__ __forceinline__ float4 x1(int t) const {
        const float4 u = *reinterpret_cast<const float4 *>(urow + 16 * t + 4 * s);
        return make_float4(pm_relu(u.x + vf[t].x), pm_relu(u.y + vf[t].y), pm_relu(u.z + vf[t].z),
                           pm_relu(u.w + vf[t].w));
    }
};
struct PmOwnX {
    const float4 (&xf)[PM_H1 / 16];
    __device__ __forceinline__ float4 x1(int t) const { return xf[t]; }
};

// z[v] = the logit of row 4 s + v of the wave's 16 A rows, the same bits in all 16 lanes r of the row group: the one
// operation sequence of a logit, whatever feeds the rows.  Call with all lanes active.
template <typename ROWS>
__device__ __forceinline__ void pm_logits_of(float (&z)[4], const ROWS &rows, const PairWeights &w) {
    f32x4 acc[PM_H2 / 16];
#pragma unroll
    for (int j = 0; j < PM_H2 / 16; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < PM_H1 / 16; ++t) {
        const float4 x = rows.x1(t);
#pragma unroll
        for (int j = 0; j < PM_H2 / 16; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.x, w.b[t][j].x, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < PM_H2 / 16; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.y, w.b[t][j].y, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < PM_H2 / 16; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.z, w.b[t][j].z, acc[j], 0, 0, 0);
#pragma unroll
        for (int j = 0; j < PM_H2 / 16; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(x.w, w.b[t][j].w, acc[j], 0, 0, 0);
    }
    // acc[j][v]: row 4 s + v, fc2 output 16 j + r
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        float p = 0.f;
#pragma unroll
        for (int j = 0; j < PM_H2 / 16; ++j) p = __builtin_fmaf(w.w3[j], pm_relu(acc[j][v] + w.b2[j]), p);
        z[v] = group_sum<16>(p) + w.b3;
    }
}

// z[v] = the logit of (the query whose u row is at `urow` in LDS, the wave's candidate 4 s + v)
__device__ __forceinline__ void pm_pair_logits(float (&z)[4], const float *urow, const float4 (&vf)[PM_H1 / 16],
                                               const PairWeights &w, int s) {
    pm_logits_of(z, PmBroadcastU{urow, vf, s}, w);
}

// z[v] = the logit of the wave's pair 4 s + v, xf the lane's fragments of relu(u + v) of ITS pair r
__device__ __forceinline__ void pm_own_pair_logits(float (&z)[4], const float4 (&xf)[PM_H1 / 16], const PairWeights &w) {
    pm_logits_of(z, PmOwnX{xf}, w);
}

// lane r < 4 of a row group speaks for candidate 4 s + r
__device__ __forceinline__ float pm_pick(const float (&z)[4], int r) {
    return r == 0 ? z[0] : r == 1 ? z[1] : r == 2 ? z[2] : z[3];
}

// stage the u rows q0 .. q0 + nq - 1 in LDS
__device__ __forceinline__ void pm_stage_u(float *su, const float *__restrict__ uq, long ldu, long q0, int nq) {
    for (int x = threadIdx.x; x < nq * (PM_H1 / 4); x += PM_THREADS) {
        const int row = x / (PM_H1 / 4), c4 = x - row * (PM_H1 / 4);
        *reinterpret_cast<float4 *>(su + row * PM_H1 + 4 * c4) =
            *reinterpret_cast<const float4 *>(uq + (q0 + row) * ldu + 4 * c4);
    }
}

// out[q, c] = z(q, c): a workgroup owns 64 query rows and PM_STORE_TILES candidate tiles
__global__ __launch_bounds__(PM_THREADS) void pair_mlp_store_kernel(
    long n_q, long n_c, const float *__restrict__ uq, long ldu, const float *__restrict__ vt, long ldv,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, float *__restrict__ out, long ldo, long tiles_q, long tiles_c) {
    __shared__ __attribute__((aligned(16))) float su[PM_ROWS * PM_H1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * PM_ROWS;
    const long t_lo = (bid / tiles_q) * PM_STORE_TILES;
    const long t_hi = t_lo + PM_STORE_TILES < tiles_c ? t_lo + PM_STORE_TILES : tiles_c;
    const int nq = (int)(n_q - q0 < PM_ROWS ? n_q - q0 : PM_ROWS);
    pm_stage_u(su, uq, ldu, q0, nq);
    PairWeights w;
    pm_load_weights(w, w2, b2, w3, b3, r, s);
    __syncthreads();
    for (long t = t_lo; t < t_hi; ++t) {
        float4 vf[PM_H1 / 16];
        long cw;
        const bool mine = pm_open_tile(vf, cw, t, wave, r, s, vt, ldv, n_c);
        for (int qi = 0; qi < nq; ++qi) {
            float z[4];
            pm_pair_logits(z, su + qi * PM_H1, vf, w, s);
            if (mine) out[(q0 + qi) * ldo + cw] = pm_pick(z, r);
        }
    }
}

template <int KC>
struct PairSmem {
    TopkSmem<KC> tk;
    __attribute__((aligned(16))) float u[PM_ROWS * PM_H1];
};

// per split and query row the best kk (s = -2 z, id) of the split's candidates into ws [S][n_q][kk]; a workgroup owns
// qr <= 64 query rows and the split's candidate tiles
template <int KC>
__global__ __launch_bounds__(PM_THREADS) void pair_mlp_select_kernel(
    long n_q, long n_c, const float *__restrict__ uq, long ldu, const float *__restrict__ vt, long ldv,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, const long *__restrict__ cand, const long *__restrict__ frow,
    const long *__restrict__ frel, const int *__restrict__ rowptr, const int *__restrict__ col,
    const int *__restrict__ eptr, const int *__restrict__ rel, int kk, int splits, int qr, long tiles_q, long tiles_c,
    float *__restrict__ ws_s, int *__restrict__ ws_i) {
    __shared__ PairSmem<KC> sm;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * qr;
    const int split = (int)(bid / tiles_q);
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    const int nq = (int)(n_q - q0 < qr ? n_q - q0 : qr);
    for (int x = tid; x < TK_ROWS * KC; x += PM_THREADS) {
        (&sm.tk.ls[0][0])[x] = __builtin_inff();
        (&sm.tk.li[0][0])[x] = TK_NONE;
    }
    if (tid < TK_ROWS) sm.tk.qn[tid] = 0;
    pm_stage_u(sm.u, uq, ldu, q0, nq);
    PairWeights w;
    pm_load_weights(w, w2, b2, w3, b3, r, s);
    __syncthreads();
    for (long t = t_lo; t < t_hi; ++t) {
        // (pm_open_tile by hand: through the helper this kernel's registers are allocated differently)
        const long c0 = t * PM_COLS + wave * 16;
        const long crow = c0 + r < n_c ? c0 + r : n_c - 1;        // rows past the end: computed, never pushed
        float4 vf[PM_H1 / 16];
        pm_load_v(vf, vt + crow * ldv, s);
        const long cw = c0 + 4 * s + (r & 3);
        const bool mine = r < 4 && cw < n_c;
        const int cid = mine ? (int)(cand ? cand[cw] : cw) : TK_NONE;
        for (int qi = 0; qi < nq; ++qi) {
            float z[4];
            pm_pair_logits(z, sm.u + qi * PM_H1, vf, w, s);
            if (mine) {
                const float sv = -2.f * pm_pick(z, r);
                if (tk_before(sv, cid, sm.tk.ls[qi][kk - 1], sm.tk.li[qi][kk - 1])) {
                    const int slot = atomicAdd(&sm.tk.qn[qi], 1);
                    if (slot < TK_QUEUE) {                          // (always: at most PM_COLS pushes per row and tile)
                        sm.tk.qs[qi][slot] = sv;
                        sm.tk.qi[qi][slot] = cid;
                    }
                }
            }
        }
        __syncthreads();
        topk_merge_queues<KC, true>(sm.tk, kk, q0, n_q, frow, frel, rowptr, col, eptr, rel);
        __syncthreads();
    }
    for (int x = tid; x < nq * kk; x += PM_THREADS) {
        const int row = x / kk, j = x - row * kk;
        const long o = ((long)split * n_q + q0 + row) * kk + j;
        ws_s[o] = sm.tk.ls[row][j];
        ws_i[o] = sm.tk.li[row][j];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Filtered ranking under the head (rank_pairs_mlp): the store kernel's loop with compares in place of the store, and the
// "subtract, do not mask" filter correction of lkg_rank.hip (DESIGN.md sections 3.6a, 3.6d).

constexpr int PM_PREP_WAVES = PM_THREADS / 64;   // queries per workgroup pass of the prepare kernel
constexpr long PM_PREP_GRID = 1024;              // its workgroups at most: a wave keeps the weights for several queries
constexpr long PM_COUNT_WGS = 4096;              // workgroups the count kernel aims for (16 per CU: a smooth tail) ...
constexpr long PM_COUNT_MIN_TILES = 8;           // ... while each owns at least this many candidate tiles

// One wave per query: thr[i] = z(i, truth[i]); better[i] / equal[i] = minus the filtered candidates (other than the truth,
// inside the candidate set) that pair_mlp_count_kernel will count -- 0 without a filter.  Filter entries are entity ids;
// slot maps them to rows of vt (NULL: the identity), -1 = not a candidate.
__global__ __launch_bounds__(PM_THREADS) void pair_mlp_prepare_kernel(
    long n_q, long n_c, const float *__restrict__ uq, long ldu, const float *__restrict__ vt, long ldv,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, const long *__restrict__ truth, long n_rows, const int *__restrict__ slot,
    const long *__restrict__ frow, const long *__restrict__ frel, const int *__restrict__ rowptr,
    const int *__restrict__ col, const int *__restrict__ eptr, const int *__restrict__ rel, float *__restrict__ thr,
    int *__restrict__ better, int *__restrict__ equal) {
    __shared__ __attribute__((aligned(16))) float su[PM_PREP_WAVES * PM_H1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    PairWeights w;
    pm_load_weights(w, w2, b2, w3, b3, r, s);
    float *urow = su + wave * PM_H1;
    for (long base = (long)blockIdx.x * PM_PREP_WAVES; base < n_q; base += (long)gridDim.x * PM_PREP_WAVES) {
        const long i = base + wave;
        const bool active = i < n_q;                      // (uniform in the wave; `base` is uniform in the workgroup)
        __syncthreads();                                  // the previous pass has read its u rows
        if (active && lane < PM_H1 / 4)
            *reinterpret_cast<float4 *>(urow + 4 * lane) = *reinterpret_cast<const float4 *>(uq + i * ldu + 4 * lane);
        __syncthreads();
        if (!active) continue;
        const long tr = min(max(truth[i], 0L), n_c - 1);
        float4 vf[PM_H1 / 16];
        float z[4];
        pm_load_v(vf, vt + tr * ldv, s);                  // all 16 candidates are the truth
        pm_pair_logits(z, urow, vf, w, s);
        const float st = z[0];
        int nb = 0, ne = 0;
        if (rowptr) {
            const long f = min(max(frow[i], 0L), n_rows - 1);
            const int want = (int)frel[i];
            const int e0 = rowptr[f], e1 = rowptr[f + 1];
            for (int eb = e0; eb < e1; eb += 16) {        // 16 filter entries per pass (uniform trip count in the wave)
                const int e = eb + r;
                long c = tr;
                bool keep = false;
                if (e < e1) {
                    const long cs = known_slot<long>(slot, col[e], n_rows);
                    if (cs >= 0 && cs < n_c && cs != tr) {
                        c = cs;
                        keep = known_under(eptr, rel, e, want);
                    }
                }
                pm_load_v(vf, vt + c * ldv, s);
                pm_pair_logits(z, urow, vf, w, s);
                const unsigned long long kept = __ballot(keep);          // bit r (of the lanes s = 0): candidate r is kept
                const float zc = pm_pick(z, r);
                const bool on = r < 4 && ((kept >> (4 * s + r)) & 1ull);
                nb += __popcll(__ballot(on && zc > st));
                ne += __popcll(__ballot(on && zc == st));
            }
        }
        if (lane == 0) {
            thr[i] = st;
            better[i] = -nb;
            equal[i] = -ne;
        }
    }
}

// better[i] += #{c != truth[i] : z(i, c) > thr[i]}, equal[i] += #{c != truth[i] : z(i, c) == thr[i]}: a workgroup owns 64
// query rows and the candidate tiles of its split.  Lane qi of every wave keeps query qi's two counts over the wave's
// candidates in registers; they meet in LDS and leave with one atomic per row, count and workgroup.
__global__ __launch_bounds__(PM_THREADS) void pair_mlp_count_kernel(
    long n_q, long n_c, const float *__restrict__ uq, long ldu, const float *__restrict__ vt, long ldv,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, const float *__restrict__ thr, const long *__restrict__ truth,
    int *__restrict__ better, int *__restrict__ equal, long splits, long tiles_q, long tiles_c) {
    __shared__ __attribute__((aligned(16))) float su[PM_ROWS * PM_H1];
    __shared__ float sthr[PM_ROWS];
    __shared__ int struth[PM_ROWS];
    __shared__ int cnt[2][PM_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * PM_ROWS;
    const long split = bid / tiles_q;
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    const int nq = (int)(n_q - q0 < PM_ROWS ? n_q - q0 : PM_ROWS);
    if (tid < PM_ROWS) {
        const bool in = tid < nq;
        sthr[tid] = in ? thr[q0 + tid] : __builtin_nanf("");
        struth[tid] = in ? (int)min(max(truth[q0 + tid], -1L), (long)INT_MAX) : -1;
        cnt[0][tid] = 0;
        cnt[1][tid] = 0;
    }
    pm_stage_u(su, uq, ldu, q0, nq);
    PairWeights w;
    pm_load_weights(w, w2, b2, w3, b3, r, s);
    __syncthreads();
    // the epilogue is kept free of branches and LDS traffic: lane qi holds query qi's threshold and truth (read with
    // v_readlane, qi being uniform), and lane (r < 4, s) takes its candidate's logit z[r] through bit masks -- a lane that
    // speaks for no candidate (r >= 4, or past the end) takes a NaN, which compares false both ways
    const int my_thr = __float_as_int(sthr[lane]), my_truth = struth[lane];
    int pick[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) pick[x] = r == x ? -1 : 0;
    int nb = 0, ne = 0;
    for (long t = t_lo; t < t_hi; ++t) {
        float4 vf[PM_H1 / 16];
        long cw;
        const int none = pm_open_tile(vf, cw, t, wave, r, s, vt, ldv, n_c) ? 0 : 0x7fc00000;
        const int cwi = (int)cw;
        for (int qi = 0; qi < nq; ++qi) {
            float z[4];
            pm_pair_logits(z, su + qi * PM_H1, vf, w, s);
            const float tq = __int_as_float(__builtin_amdgcn_readlane(my_thr, qi));
            const int tr = __builtin_amdgcn_readlane(my_truth, qi);
            const float zc = __int_as_float((__float_as_int(z[0]) & pick[0]) | (__float_as_int(z[1]) & pick[1]) |
                                            (__float_as_int(z[2]) & pick[2]) | (__float_as_int(z[3]) & pick[3]) | none);
            const bool ok = cwi != tr;
            const int b = __popcll(__ballot(ok && zc > tq)), e = __popcll(__ballot(ok && zc == tq));
            nb += lane == qi ? b : 0;
            ne += lane == qi ? e : 0;
        }
    }
    if (lane < nq) {
        if (nb) atomicAdd(&cnt[0][lane], nb);
        if (ne) atomicAdd(&cnt[1][lane], ne);
    }
    __syncthreads();
    if (tid < nq) {
        if (cnt[0][tid]) atomicAdd(better + q0 + tid, cnt[0][tid]);
        if (cnt[1][tid]) atomicAdd(equal + q0 + tid, cnt[1][tid]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Explicit pairs (score_pairs_mlp, evaluate_mlp_classification): pair i = (row u_idx[i] of u, row v_idx[i] of v).  A wave
// owns 16 pairs per step and lane (r, s) forms relu(u + v) of ITS pair r from the two gathered rows, so the A operand has
// a pair of its own in every row; the rest is pm_logits_of, the operation sequence of every other logit in this file.
// The grid is capped so that a wave keeps the weights for many steps.  Pairs past the end are clamped to the last one:
// computed, never stored or counted.
constexpr long PM_PAIRS_GRID = 1024;             // workgroups at most: 64 pairs per workgroup and trip

// counts[0..4] += tp, fp, tn, fn, nan of the pairs against labels and the logit threshold thr: per lane in registers,
// per workgroup in LDS, then one 64-bit atomic per non-zero count and workgroup (integers: no order enters).
__global__ __launch_bounds__(PM_THREADS) void pair_mlp_pairs_kernel(
    long n_pairs, const float *__restrict__ u, long ldu, const float *__restrict__ v, long ldv,
    const long *__restrict__ u_idx, const long *__restrict__ v_idx, const float *__restrict__ w2,
    const float *__restrict__ b2, const float *__restrict__ w3, const float *__restrict__ b3,
    const unsigned char *__restrict__ labels, float thr, float *__restrict__ out,
    unsigned long long *__restrict__ counts) {
    __shared__ int cnt[5];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    if (tid < 5) cnt[tid] = 0;
    PairWeights w;
    pm_load_weights(w, w2, b2, w3, b3, r, s);
    int n_tp = 0, n_fp = 0, n_tn = 0, n_fn = 0, n_nan = 0;
    // (the trip count is uniform in the workgroup: a wave whose 16 pairs all lie past the end computes the last pair)
    for (long base = (long)blockIdx.x * PM_COLS; base < n_pairs; base += (long)gridDim.x * PM_COLS) {
        const long p0 = base + wave * 16;
        const long pr = p0 + r < n_pairs ? p0 + r : n_pairs - 1;
        const float *urow = u + (u_idx ? u_idx[pr] : pr) * ldu;
        const float *vrow = v + (v_idx ? v_idx[pr] : pr) * ldv;
        float4 xf[PM_H1 / 16];
#pragma unroll
        for (int t = 0; t < PM_H1 / 16; ++t) {
            const float4 a = *reinterpret_cast<const float4 *>(urow + 16 * t + 4 * s);
            const float4 b = *reinterpret_cast<const float4 *>(vrow + 16 * t + 4 * s);
            xf[t] = make_float4(pm_relu(a.x + b.x), pm_relu(a.y + b.y), pm_relu(a.z + b.z), pm_relu(a.w + b.w));
        }
        float z[4];
        pm_own_pair_logits(z, xf, w);
        const long pw = p0 + 4 * s + (r & 3);
        if (r < 4 && pw < n_pairs) {
            const float zp = pm_pick(z, r);
            if (out) out[pw] = zp;
            if (counts) {
                const bool one = labels[pw] != 0, nan = zp != zp, pos = zp > thr;
                n_nan += nan;
                n_tp += !nan && pos && one;
                n_fp += !nan && pos && !one;
                n_tn += !nan && !pos && !one;
                n_fn += !nan && !pos && one;
            }
        }
    }
    if (!counts) return;                                          // (uniform: a kernel argument)
    __syncthreads();
    if (n_tp) atomicAdd(&cnt[0], n_tp);
    if (n_fp) atomicAdd(&cnt[1], n_fp);
    if (n_tn) atomicAdd(&cnt[2], n_tn);
    if (n_fn) atomicAdd(&cnt[3], n_fn);
    if (n_nan) atomicAdd(&cnt[4], n_nan);
    __syncthreads();
    if (tid < 5 && cnt[tid]) atomicAdd(counts + tid, (unsigned long long)cnt[tid]);
}

// ---------------------------------------------------------------------------------------------------------------------
// Threshold retrieval under the head (predict_accepted_mlp, count_accepted_mlp; include/literalkg_hip.h):
// the count kernel's loop with ONE compare per logit, z > thr[row], and the filter lookup only on a pass.  Three modes
// share every instruction up to the decision:
//   PM_ACC_COUNT   the pass is added to the row's LDS counter; one integer global add per row and workgroup.
//   PM_ACC_APPEND  count, and the entry takes a slot from ONE global cursor: (row, id, z) is written when the slot lies
//                  below `capacity`, nothing otherwise -- the counts stay exact either way, and the host sees an
//                  overflow as sum(counts) > capacity.
//   PM_ACC_EMIT    the entry takes a slot from its row's cursor and is written at base[row] + slot when the slot lies
//                  inside the row's counted length; otherwise nothing is written and the flag is raised.
// Entries land in an arbitrary order, which lkg_accept_order fixes: (s = -2 z, id) is unique within a row.
enum { PM_ACC_COUNT = 0, PM_ACC_APPEND = 1, PM_ACC_EMIT = 2 };

template <int MODE>
__global__ __launch_bounds__(PM_THREADS) void pair_mlp_accept_kernel(
    long n_q, long n_c, const float *__restrict__ uq, long ldu, const float *__restrict__ vt, long ldv,
    const float *__restrict__ w2, const float *__restrict__ b2, const float *__restrict__ w3,
    const float *__restrict__ b3, const float *__restrict__ thr, const long *__restrict__ cand,
    const long *__restrict__ frow, const long *__restrict__ frel, const int *__restrict__ rowptr,
    const int *__restrict__ col, const int *__restrict__ eptr, const int *__restrict__ rel, int splits, int qr,
    long tiles_q, long tiles_c, int *__restrict__ counts, long capacity, unsigned long long *__restrict__ gcursor,
    int *__restrict__ out_row, int *__restrict__ out_id32, const long *__restrict__ base, int *__restrict__ cursor,
    long *__restrict__ out_id, float *__restrict__ out_s, float *__restrict__ out_z, int *__restrict__ flag) {
    __shared__ __attribute__((aligned(16))) float su[PM_ROWS * PM_H1];
    __shared__ float sthr[PM_ROWS];
    __shared__ int cnt[PM_ROWS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 15, s = lane >> 4;
    const long bid = blockIdx.x;
    const long q0 = (bid % tiles_q) * qr;
    const long split = bid / tiles_q;
    const long t_lo = split * tiles_c / splits, t_hi = (split + 1) * tiles_c / splits;
    const int nq = (int)(n_q - q0 < qr ? n_q - q0 : qr);
    if (tid < PM_ROWS) {
        sthr[tid] = tid < nq ? thr[q0 + tid] : __builtin_nanf("");
        cnt[tid] = 0;
    }
    pm_stage_u(su, uq, ldu, q0, nq);
    PairWeights w;
    pm_load_weights(w, w2, b2, w3, b3, r, s);
    __syncthreads();
    // as in pair_mlp_count_kernel: lane qi holds query qi's threshold (read with v_readlane, qi being uniform) and lane
    // (r < 4, s) takes its candidate's logit through bit masks; a lane that speaks for no candidate takes a NaN, which
    // never passes
    const int my_thr = __float_as_int(sthr[lane]);
    int pick[4];
#pragma unroll
    for (int x = 0; x < 4; ++x) pick[x] = r == x ? -1 : 0;
    for (long t = t_lo; t < t_hi; ++t) {
        float4 vf[PM_H1 / 16];
        long cw;
        const bool mine = pm_open_tile(vf, cw, t, wave, r, s, vt, ldv, n_c);
        const int none = mine ? 0 : 0x7fc00000;
        const int cid = mine ? (int)(cand ? cand[cw] : cw) : TK_NONE;
        for (int qi = 0; qi < nq; ++qi) {
            float z[4];
            pm_pair_logits(z, su + qi * PM_H1, vf, w, s);
            const float tq = __int_as_float(__builtin_amdgcn_readlane(my_thr, qi));
            const float zc = __int_as_float((__float_as_int(z[0]) & pick[0]) | (__float_as_int(z[1]) & pick[1]) |
                                            (__float_as_int(z[2]) & pick[2]) | (__float_as_int(z[3]) & pick[3]) | none);
            if (zc > tq) {                                           // rare at the selectivities this is built for
                const long grow = q0 + qi;
                if (rowptr && known_lookup(rowptr, col, eptr, rel, frow[grow], (int)frel[grow], cid)) continue;
                if (MODE != PM_ACC_EMIT) atomicAdd(&cnt[qi], 1);
                if (MODE == PM_ACC_APPEND) {
                    const unsigned long long slot = atomicAdd(gcursor, 1ull);
                    if (slot < (unsigned long long)capacity) {
                        out_row[slot] = (int)grow;
                        out_id32[slot] = cid;
                        out_z[slot] = zc;
                    }
                }
                if (MODE == PM_ACC_EMIT) {
                    const int slot = atomicAdd(cursor + grow, 1);
                    if (slot >= 0 && slot < counts[grow]) {
                        const long o = base[grow] + slot;
                        out_id[o] = cid;
                        out_s[o] = -2.f * zc;
                        out_z[o] = zc;
                    } else {
                        atomicOr(flag, 1);
                    }
                }
            }
        }
    }
    if (MODE != PM_ACC_EMIT) {
        __syncthreads();
        if (tid < nq && cnt[tid]) atomicAdd(counts + q0 + tid, cnt[tid]);
    }
}

// candidate splits of the count kernel: enough workgroups for a smooth tail, each with a long run of tiles, and never
// fewer than two workgroups per CU while there are tiles to hand out
long pm_count_splits(long tiles_q, long tiles_c) {
    const long fill = (2 * 256 + tiles_q - 1) / tiles_q, many = (PM_COUNT_WGS + tiles_q - 1) / tiles_q;
    long s_ = tiles_c / PM_COUNT_MIN_TILES < many ? tiles_c / PM_COUNT_MIN_TILES : many;
    s_ = s_ > fill ? s_ : fill;
    s_ = s_ < tiles_c ? s_ : tiles_c;
    return s_ > 1 ? s_ : 1;
}

// query rows per workgroup of the select kernel: fewer for small batches, so that the splits (at most 64) fill the chip
long pm_select_rows(long n_q) { return n_q >= 512 ? 64 : n_q >= 128 ? 32 : 16; }

bool pm_operands_ok(const float *uq, long ldu, const float *v, long ldv, const float *w2) {
    return lkg_aligned16(uq) && lkg_aligned16(v) && lkg_aligned16(w2) && ldu % 4 == 0 && ldv % 4 == 0 && ldu >= PM_H1 &&
           ldv >= PM_H1;
}

// What an entry point asks of its operands (`a`: its first table, `rest`: its other pointers that may not be null).
// Statements of the entry point's body, which read its parameters v, w2, b2, w3, b3, ldu, ldv by name.
#define PM_REQUIRE_OPERANDS(name, a, rest)                                                                             \
    LKG_REQUIRE(a && v && w2 && b2 && w3 && b3 && rest, name ": null pointer");                                        \
    LKG_REQUIRE(pm_operands_ok(a, ldu, v, ldv, w2),                                                                    \
                name ": " #a ", v and w2 must be 16-byte aligned with row strides that are multiples of 4 (at least 128)")

}  // namespace

extern "C" int32_t lkg_pair_mlp_splits(int64_t n_q, int64_t n_cand, int32_t requested) {
    if (n_q <= 0 || n_cand <= 0 || requested < 0 || requested > LKG_TOPK_MAX_SPLITS) return 0;
    const long qr = pm_select_rows(n_q);
    const long tiles_q = (n_q + qr - 1) / qr, tiles_c = (n_cand + PM_COLS - 1) / PM_COLS;
    long s_ = requested > 0 ? requested : (2 * 256 + tiles_q - 1) / tiles_q;   // auto: >= 2 workgroups per CU
    s_ = s_ < LKG_TOPK_MAX_SPLITS ? s_ : LKG_TOPK_MAX_SPLITS;
    s_ = s_ < tiles_c ? s_ : tiles_c;
    return (int32_t)(s_ > 1 ? s_ : 1);
}

extern "C" int lkg_pair_mlp_scores_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v,
                                       int64_t ldv, const float *w2, const float *b2, const float *w3, const float *b3,
                                       float *out, int64_t ldo, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand >= 0 && ldo >= n_cand, "lkg_pair_mlp_scores_f32: bad sizes");
    if (n_q == 0 || n_cand == 0) return LKG_OK;
    PM_REQUIRE_OPERANDS("lkg_pair_mlp_scores_f32", uq, out);
    const long tiles_q = (n_q + PM_ROWS - 1) / PM_ROWS, tiles_c = (n_cand + PM_COLS - 1) / PM_COLS;
    const long chunks = (tiles_c + PM_STORE_TILES - 1) / PM_STORE_TILES;
    LKG_REQUIRE(tiles_q * chunks < INT32_MAX, "lkg_pair_mlp_scores_f32: too many workgroups (split the queries)");
    hipLaunchKernelGGL(pair_mlp_store_kernel, dim3((unsigned)(tiles_q * chunks)), dim3(PM_THREADS), 0,
                       (hipStream_t)stream, (long)n_q, (long)n_cand, uq, (long)ldu, v, (long)ldv, w2, b2, w3, b3, out,
                       (long)ldo, tiles_q, tiles_c);
    LKG_CHECK_LAUNCH("lkg_pair_mlp_scores_f32");
    return LKG_OK;
}

extern "C" int lkg_pair_mlp_select_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v,
                                       int64_t ldv, const float *w2, const float *b2, const float *w3, const float *b3,
                                       const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                       const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                       int32_t top_k, int32_t splits, float *ws_s, int32_t *ws_i, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand > 0 && n_cand < INT32_MAX, "lkg_pair_mlp_select_f32: bad sizes");
    LKG_REQUIRE(top_k >= 1 && top_k <= LKG_TOPK_MAX, "lkg_pair_mlp_select_f32: top_k must lie in [1, %d]", LKG_TOPK_MAX);
    if (n_q == 0) return LKG_OK;
    LKG_REQUIRE(splits >= 1 && splits == lkg_pair_mlp_splits(n_q, n_cand, splits),
                "lkg_pair_mlp_select_f32: splits must come from lkg_pair_mlp_splits");
    PM_REQUIRE_OPERANDS("lkg_pair_mlp_select_f32", uq, ws_s && ws_i);
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "lkg_pair_mlp_select_f32: incomplete filter");
    const long qr = pm_select_rows(n_q);
    const long tiles_q = (n_q + qr - 1) / qr, tiles_c = (n_cand + PM_COLS - 1) / PM_COLS;
    LKG_REQUIRE(tiles_q * splits < INT32_MAX, "lkg_pair_mlp_select_f32: too many workgroups (split the queries)");
    const dim3 grid((unsigned)(tiles_q * splits));
    const hipStream_t st = (hipStream_t)stream;
#define LKG_PM_LAUNCH(KC)                                                                                              \
    hipLaunchKernelGGL((pair_mlp_select_kernel<KC>), grid, dim3(PM_THREADS), 0, st, (long)n_q, (long)n_cand, uq,       \
                       (long)ldu, v, (long)ldv, w2, b2, w3, b3, (const long *)cand_ids, (const long *)filter_row,      \
                       (const long *)filter_rel, rowptr, col, eptr, rel, top_k, splits, (int)qr, tiles_q, tiles_c,     \
                       ws_s, ws_i)
    if (top_k <= 16) LKG_PM_LAUNCH(16);
    else if (top_k <= 32) LKG_PM_LAUNCH(32);
    else if (top_k <= 64) LKG_PM_LAUNCH(64);
    else LKG_PM_LAUNCH(128);
#undef LKG_PM_LAUNCH
    LKG_CHECK_LAUNCH("lkg_pair_mlp_select_f32");
    return LKG_OK;
}

extern "C" int lkg_pair_mlp_prepare_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v,
                                        int64_t ldv, const float *w2, const float *b2, const float *w3, const float *b3,
                                        const int64_t *truth, int64_t n_rows, const int32_t *cand_slot,
                                        const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                                        const int32_t *col, const int32_t *eptr, const int32_t *rel, float *thr,
                                        int32_t *better, int32_t *equal, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand > 0 && n_cand < INT32_MAX, "lkg_pair_mlp_prepare_f32: bad sizes");
    if (n_q == 0) return LKG_OK;
    PM_REQUIRE_OPERANDS("lkg_pair_mlp_prepare_f32", uq, truth && thr && better && equal);
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "lkg_pair_mlp_prepare_f32: incomplete filter");
    LKG_REQUIRE(!rowptr || (n_rows > 0 && n_rows < INT32_MAX && (cand_slot || n_rows == n_cand)),
                "lkg_pair_mlp_prepare_f32: the filter's rows must be the candidates, or come with cand_slot");
    const long blocks = (n_q + PM_PREP_WAVES - 1) / PM_PREP_WAVES;
    hipLaunchKernelGGL(pair_mlp_prepare_kernel, dim3((unsigned)(blocks < PM_PREP_GRID ? blocks : PM_PREP_GRID)),
                       dim3(PM_THREADS), 0, (hipStream_t)stream, (long)n_q, (long)n_cand, uq, (long)ldu, v, (long)ldv, w2,
                       b2, w3, b3, (const long *)truth, (long)n_rows, cand_slot, (const long *)filter_row,
                       (const long *)filter_rel, rowptr, col, eptr, rel, thr, better, equal);
    LKG_CHECK_LAUNCH("lkg_pair_mlp_prepare_f32");
    return LKG_OK;
}

extern "C" int lkg_pair_mlp_count_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v,
                                      int64_t ldv, const float *w2, const float *b2, const float *w3, const float *b3,
                                      const float *thr, const int64_t *truth, int32_t *better, int32_t *equal,
                                      void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_cand >= 0 && n_cand < INT32_MAX, "lkg_pair_mlp_count_f32: bad sizes");
    if (n_q == 0 || n_cand == 0) return LKG_OK;
    PM_REQUIRE_OPERANDS("lkg_pair_mlp_count_f32", uq, thr && truth && better && equal);
    const long tiles_q = (n_q + PM_ROWS - 1) / PM_ROWS, tiles_c = (n_cand + PM_COLS - 1) / PM_COLS;
    const long splits = pm_count_splits(tiles_q, tiles_c);
    LKG_REQUIRE(tiles_q * splits < INT32_MAX, "lkg_pair_mlp_count_f32: too many workgroups (split the queries)");
    hipLaunchKernelGGL(pair_mlp_count_kernel, dim3((unsigned)(tiles_q * splits)), dim3(PM_THREADS), 0,
                       (hipStream_t)stream, (long)n_q, (long)n_cand, uq, (long)ldu, v, (long)ldv, w2, b2, w3, b3, thr,
                       (const long *)truth, better, equal, splits, tiles_q, tiles_c);
    LKG_CHECK_LAUNCH("lkg_pair_mlp_count_f32");
    return LKG_OK;
}

extern "C" int lkg_pair_mlp_pairs_f32(int64_t n_pairs, const float *u, int64_t ldu, const float *v, int64_t ldv,
                                      const int64_t *u_idx, const int64_t *v_idx, const float *w2, const float *b2,
                                      const float *w3, const float *b3, const uint8_t *labels, float thr, float *out,
                                      int64_t *counts, void *stream) {
    LKG_REQUIRE(n_pairs >= 0 && n_pairs <= (int64_t)INT32_MAX - 1, "lkg_pair_mlp_pairs_f32: bad sizes");
    LKG_REQUIRE(out || counts, "lkg_pair_mlp_pairs_f32: nothing to write (out and counts are both null)");
    LKG_REQUIRE(!counts || labels, "lkg_pair_mlp_pairs_f32: counts need labels (null pointer)");
    if (n_pairs == 0) return LKG_OK;
    PM_REQUIRE_OPERANDS("lkg_pair_mlp_pairs_f32", u, true);
    const long blocks = (n_pairs + PM_COLS - 1) / PM_COLS;
    hipLaunchKernelGGL(pair_mlp_pairs_kernel, dim3((unsigned)(blocks < PM_PAIRS_GRID ? blocks : PM_PAIRS_GRID)),
                       dim3(PM_THREADS), 0, (hipStream_t)stream, (long)n_pairs, u, (long)ldu, v, (long)ldv,
                       (const long *)u_idx, (const long *)v_idx, w2, b2, w3, b3, labels, thr, out,
                       (unsigned long long *)counts);
    LKG_CHECK_LAUNCH("lkg_pair_mlp_pairs_f32");
    return LKG_OK;
}

namespace {

template <int MODE>
int pm_launch_accept(const char *name, int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                     const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                     const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                     const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t splits, int32_t *counts,
                     int64_t capacity, int64_t *gcursor, int32_t *out_rows, int32_t *out_ids32, const int64_t *base,
                     int32_t *cursor, int64_t *out_ids, float *out_s, float *out_z, int32_t *flag, void *stream) {
    LKG_REQUIRE(n_q >= 0 && n_q < INT32_MAX && n_cand >= 0 && n_cand < INT32_MAX, "%s: bad sizes", name);
    LKG_REQUIRE(splits >= 0 && splits <= LKG_TOPK_MAX_SPLITS, "%s: splits must lie in [0, %d]", name, LKG_TOPK_MAX_SPLITS);
    LKG_REQUIRE(MODE != PM_ACC_APPEND || (capacity >= 0 && capacity < INT32_MAX), "%s: capacity must lie in [0, 2^31 - 1)",
                name);
    if (n_q == 0 || n_cand == 0) return LKG_OK;
    LKG_REQUIRE(uq && v && w2 && b2 && w3 && b3 && thr && counts, "%s: null pointer", name);
    LKG_REQUIRE(pm_operands_ok(uq, PM_H1, v, PM_H1, w2),
                "%s: uq, v and w2 must be 16-byte aligned", name);
    LKG_REQUIRE(MODE != PM_ACC_APPEND || (gcursor && (capacity == 0 || (out_rows && out_ids32 && out_z))),
                "%s: null pointer", name);
    LKG_REQUIRE(MODE != PM_ACC_EMIT || (base && cursor && out_ids && out_s && out_z && flag), "%s: null pointer", name);
    LKG_REQUIRE(known_filter_complete(rowptr, filter_row, filter_rel, col, eptr, rel), "%s: incomplete filter", name);
    const int s_ = lkg_pair_mlp_splits(n_q, n_cand, splits);      // the split policy of the select launch
    LKG_REQUIRE(s_ >= 1, "%s: no split count for these sizes", name);
    const long qr = pm_select_rows(n_q);
    const long tiles_q = (n_q + qr - 1) / qr, tiles_c = (n_cand + PM_COLS - 1) / PM_COLS;
    LKG_REQUIRE(tiles_q * s_ < INT32_MAX, "%s: too many workgroups (split the queries)", name);
    hipLaunchKernelGGL((pair_mlp_accept_kernel<MODE>), dim3((unsigned)(tiles_q * s_)), dim3(PM_THREADS), 0,
                       (hipStream_t)stream, (long)n_q, (long)n_cand, uq, (long)PM_H1, v, (long)PM_H1, w2, b2, w3, b3, thr,
                       (const long *)cand_ids, (const long *)filter_row, (const long *)filter_rel, rowptr, col, eptr, rel,
                       s_, (int)qr, tiles_q, tiles_c, counts, (long)capacity, (unsigned long long *)gcursor, out_rows,
                       out_ids32, (const long *)base, cursor, (long *)out_ids, out_s, out_z, flag);
    LKG_CHECK_LAUNCH(name);
    return LKG_OK;
}

}  // namespace

extern "C" int lkg_pair_mlp_accept_count_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                             const float *w2, const float *b2, const float *w3,
                                             const float *b3, const float *thr, const int64_t *cand_ids,
                                             const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                                             const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t splits,
                                             int32_t *counts, void *stream) {
    return pm_launch_accept<PM_ACC_COUNT>("lkg_pair_mlp_accept_count_f32", n_q, n_cand, uq, v, w2, b2, w3, b3, thr,
                                          cand_ids, filter_row, filter_rel, rowptr, col, eptr, rel, splits, counts, 0,
                                          nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                                          stream);
}

extern "C" int lkg_pair_mlp_accept_append_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                              const float *w2, const float *b2, const float *w3,
                                              const float *b3, const float *thr, const int64_t *cand_ids,
                                              const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                                              const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t splits,
                                              int32_t *counts, int64_t capacity, int64_t *cursor, int32_t *out_rows,
                                              int32_t *out_ids, float *out_logits, void *stream) {
    return pm_launch_accept<PM_ACC_APPEND>("lkg_pair_mlp_accept_append_f32", n_q, n_cand, uq, v, w2, b2, w3, b3,
                                           thr, cand_ids, filter_row, filter_rel, rowptr, col, eptr, rel, splits, counts,
                                           capacity, cursor, out_rows, out_ids, nullptr, nullptr, nullptr, nullptr,
                                           out_logits, nullptr, stream);
}

extern "C" int lkg_pair_mlp_accept_emit_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                            const float *w2, const float *b2, const float *w3,
                                            const float *b3, const float *thr, const int64_t *cand_ids,
                                            const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                                            const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t splits,
                                            const int32_t *counts, const int64_t *base, int32_t *cursor, int64_t *out_ids,
                                            float *out_scores, float *out_logits, int32_t *flag, void *stream) {
    return pm_launch_accept<PM_ACC_EMIT>("lkg_pair_mlp_accept_emit_f32", n_q, n_cand, uq, v, w2, b2, w3, b3, thr,
                                         cand_ids, filter_row, filter_rel, rowptr, col, eptr, rel, splits,
                                         const_cast<int32_t *>(counts), 0, nullptr, nullptr, nullptr, base, cursor, out_ids,
                                         out_scores, out_logits, flag, stream);
}

int lkg_internal_preload_pairmlp() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&pair_mlp_store_kernel)) == hipSuccess ? 0 : 1;
}
