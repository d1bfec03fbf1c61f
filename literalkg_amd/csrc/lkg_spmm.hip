// K3 / K4: neighbour aggregation  out[i,:] = sum_j val[j] * x[col[j],:]  over a CSR
// (forward, model.py:106) or the CSC of the same pattern (backward, A^T grad).
//
// HBM-bound gather.  Mapping for gfx950 (wave64):
//   * one wave per destination row (softmax rows and aggregation rows are the same unit);
//   * the row's (col, val) pairs are fetched with ONE coalesced load per 64 entries and
//     handed to the gathering lanes by cross-lane reads (readlane / ds_bpermute), so the
//     index stream costs one dword per entry, not one per lane;
//   * a source row is read as whole 16-byte chunks by consecutive lanes: D=256 is exactly one
//     global_load_dwordx4 per lane per edge (1 KiB per wave-instruction).  For narrower rows the
//     wave is split into 64/LPE sub-groups that gather different edges at once and are summed
//     with xor-shuffles at the end, so every lane always carries a 16-byte load;
//   * U edges are kept in flight per sub-group (unrolled, loads issued before the FMAs).
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "lkg_common.h"

namespace {

template <typename V>
struct vec_ops;
template <>
struct vec_ops<float4> {
    static constexpr int W = 4;
    static __device__ __forceinline__ float4 zero() { return f4_zero(); }
    static __device__ __forceinline__ void fma(float4 &a, float s, const float4 &x) { f4_fma(a, s, x); }
    static __device__ __forceinline__ float absmax(const float4 &a) {
        return fmaxf(fmaxf(fabsf(a.x), fabsf(a.y)), fmaxf(fabsf(a.z), fabsf(a.w)));
    }
    template <int M>
    static __device__ __forceinline__ void xor_add(float4 &a) {
        a.x = lane_xor_add<M>(a.x);
        a.y = lane_xor_add<M>(a.y);
        a.z = lane_xor_add<M>(a.z);
        a.w = lane_xor_add<M>(a.w);
    }
};
template <>
struct vec_ops<float> {
    static constexpr int W = 1;
    static __device__ __forceinline__ float zero() { return 0.f; }
    static __device__ __forceinline__ void fma(float &a, float s, const float &x) { a = fmaf(s, x, a); }
    static __device__ __forceinline__ float absmax(const float &a) { return fabsf(a); }
    template <int M>
    static __device__ __forceinline__ void xor_add(float &a) { a = lane_xor_add<M>(a); }
};

template <typename V, int LPE>
__device__ __forceinline__ void reduce_subgroups(V &a) {
    if constexpr (LPE <= 32) vec_ops<V>::template xor_add<32>(a);
    if constexpr (LPE <= 16) vec_ops<V>::template xor_add<16>(a);
    if constexpr (LPE <= 8) vec_ops<V>::template xor_add<8>(a);
}

// Accumulate entries [start, end) of one row into acc.  `wave_i` / `n_waves`: this wave takes the 64-entry
// chunks wave_i, wave_i + n_waves, ... (n_waves == 1 for the wave-per-row kernel).
//
// The edge loop is branch-free on purpose: a predicated gather (`ok ? load : 0`) makes hipcc emit a
// branch per load and, at the joins, a conservative s_waitcnt vmcnt(0) that serialises the U gathers.
// Instead the tail slots of the last group re-read the row's last valid source row (an L1 hit) with
// weight 0.
template <typename V, int LPE, int CPL, int U, bool FULL>
__device__ __forceinline__ void accumulate_entries(V (&acc)[CPL], int start, int end, int wave_i, int n_waves,
                                                   int lane, int nchunk, const int *__restrict__ col,
                                                   const float *__restrict__ val, const float *__restrict__ x,
                                                   long ldx) {
    using ops = vec_ops<V>;
    constexpr int EPW = 64 / LPE;
    const int sub = lane / LPE;
    const int sl = lane % LPE;
    for (int base = start + 64 * wave_i; base < end; base += 64 * n_waves) {
        const int cnt = min(64, end - base);
        const int last = cnt - 1;
        // one coalesced fetch of up to 64 (col, val) pairs; lanes past the row end copy its last entry
        // the index stream is touched once: streaming (nontemporal) loads keep it from displacing gathered rows in the L2
        // (with the result's streaming stores: forward 1.519 -> 1.508 ms at 1 M x 256, transpose 2.14 -> 2.10 ms at the N = 8
        // per-rank shape; -DLKG_SPMM_PLAIN restores plain accesses for A/B runs)
#ifndef LKG_SPMM_PLAIN
        const int c = __builtin_nontemporal_load(col + base + min(lane, last));
        const float v = __builtin_nontemporal_load(val + base + min(lane, last));
#else
        const int c = col[base + min(lane, last)];
        const float v = val[base + min(lane, last)];
#endif
        for (int k = 0; k < cnt; k += EPW * U) {
            int cc[U];
            float vv[U];
            V xv[U][CPL];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int idx = k + u * EPW + sub;
                const int idc = min(idx, last);
                if constexpr (LPE == 64) {   // idx is wave-uniform: scalar broadcast
                    cc[u] = __builtin_amdgcn_readlane(c, idc);
                    vv[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), idc));
                } else {
                    cc[u] = __shfl(c, idc, 64);
                    vv[u] = __shfl(v, idc, 64);
                }
                vv[u] = idx < cnt ? vv[u] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const V *src = reinterpret_cast<const V *>(x + (long)cc[u] * ldx);
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const int chunk = sl + i * LPE;
                    if constexpr (FULL)
                        xv[u][i] = src[chunk];
                    else
                        xv[u][i] = src[min(chunk, nchunk - 1)];   // clamped lanes are never stored
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int i = 0; i < CPL; ++i) ops::fma(acc[i], vv[u], xv[u][i]);
        }
    }
}

// The same over a ROW-SPARSE x: xflags[c] == 0 promises that row c of x is all zero, and such entries are skipped
// without touching x (the backward of the LAST aggregation layer: the loss's gradient reaches <= 3B of the N rows, so
// all but a fraction of a percent of the transpose SpMM's gathers would fetch zeros).  Per 64-entry chunk: one coalesced
// (col) load, one byte gather of the flags, a ballot; only chunks with a flagged entry load their values and gather
// (64 / LPE flagged entries at a time, one per sub-group).  Four chunks are in flight so that the dependent col -> flag
// round trips of a long row overlap.
template <typename V, int LPE, int CPL, bool FULL>
__device__ __forceinline__ bool accumulate_entries_flagged(V (&acc)[CPL], int start, int end, int wave_i, int n_waves,
                                                           int lane, int nchunk, const int *__restrict__ col,
                                                           const float *__restrict__ val, const float *__restrict__ x,
                                                           long ldx, const unsigned char *__restrict__ xflags) {
    using ops = vec_ops<V>;
    constexpr int EPW = 64 / LPE, G = 4;
    const int sub = lane / LPE;
    const int sl = lane % LPE;
    bool any = false;                              // did this wave meet a flagged entry?  (wave-uniform)
    for (int base0 = start + 64 * wave_i; base0 < end; base0 += 64 * n_waves * G) {
        int c[G];
        unsigned long long live[G];
#pragma unroll
        for (int gq = 0; gq < G; ++gq) {
            const int j = base0 + 64 * n_waves * gq + lane;
            c[gq] = col[min(j, end - 1)];
        }
#pragma unroll
        for (int gq = 0; gq < G; ++gq) {
            const int j = base0 + 64 * n_waves * gq + lane;
            live[gq] = __ballot(j < end && xflags[c[gq]] != 0);
        }
#pragma unroll
        for (int gq = 0; gq < G; ++gq) {
            unsigned long long m = live[gq];
            if (m == 0) continue;                                  // (wave-uniform)
            any = true;
            const int j = base0 + 64 * n_waves * gq + lane;
            const float v = val[min(j, end - 1)];
            while (m) {
                int cc = __builtin_amdgcn_readlane(c[gq], __builtin_ctzll(m));   // (a sub-group without an entry re-reads a live one, weight 0)
                float vv = 0.f;
#pragma unroll
                for (int e = 0; e < EPW; ++e) {                    // sub-group e takes the e-th flagged entry still pending
                    const bool have = m != 0;
                    const int b = have ? __builtin_ctzll(m) : 0;
                    const int ce = __builtin_amdgcn_readlane(c[gq], b);
                    const float ve = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b));
                    if (sub == e) {
                        cc = have ? ce : cc;
                        vv = have ? ve : 0.f;
                    }
                    m &= m - 1;
                }
                const V *src = reinterpret_cast<const V *>(x + (long)cc * ldx);
#pragma unroll
                for (int i = 0; i < CPL; ++i) {
                    const int chunk = sl + i * LPE;
                    ops::fma(acc[i], vv, FULL ? src[chunk] : src[min(chunk, nchunk - 1)]);
                }
            }
        }
    }
    return any;
}

// Optional row-wise extras of the epilogue (lkg_spmm_csr_fused_f32): a second addend and a row copy riding along.
struct SpmmExtra {
    const float *add2;       // out[i,:] += add2[i,:]
    long ld_add2;
    const unsigned char *add2_rows;   // nullable: add2 is zero (and not read) outside the rows flagged here
    const float *copy_src;   // copy_dst[i,:] = copy_src[i,:]
    long ld_copy_src;
    float *copy_dst;
    long ld_copy_dst;
    int *rowmax;             // rowmax[i] = max |out[i,:]| as the int bits of a non-negative float (atomicMax over the slabs)
    const unsigned char *x_rows;      // nullable: rows of x that may be non-zero (accumulate_entries_flagged)
    const unsigned char *self_rows;   // nullable: the same promise for `self`
    unsigned char *out_rows;          // nullable (with x_rows): out_rows[i] = 1 where row i received a contribution; the other
                                      //   rows are NOT written (out is a table the caller keeps all-zero there)
    const int *row_list;              // nullable: the ordinary waves take THESE rows (the rows that hold entries); the others are
    int n_list;                       //   spmm_listless_rows_kernel's
    __device__ __forceinline__ const float *add2_row(long row) const {
        return add2 && (!add2_rows || add2_rows[row]) ? add2 + row * ld_add2 : nullptr;
    }
    __device__ __forceinline__ void shift(long cols) {
        if (add2) add2 += cols;
        if (copy_dst) {
            copy_src += cols;
            copy_dst += cols;
        }
    }
};

// V: float4 (16-byte chunks) or float.  LPE: lanes per edge.  CPL: chunks per lane.  U: edges in flight.
// FULL: nchunk == LPE * CPL, i.e. no lane ever falls outside the row (drops the per-load guard).
//
// One launch, two kinds of workgroup (256 threads = 4 waves each):
//   blocks [0, n_long)   : one LONG row (> long_thresh entries, listed in long_rows) per workgroup -- the four
//                          waves take interleaved 64-entry chunks, partial sums meet in LDS and are added in a
//                          fixed order (deterministic, no atomics).  They are dispatched first, so the longest
//                          rows of a skewed graph overlap the bulk instead of being the tail of the launch.
//   blocks [n_long, ...) : four ordinary rows, one wave each (rows over the threshold are skipped here).
template <typename V, int LPE, int CPL, int U, bool FULL, bool XF>
__global__ __launch_bounds__(256) void spmm_csr_kernel(int n_rows, int nchunk,
                                                        const int *__restrict__ rowptr,
                                                        const int *__restrict__ col,
                                                        const float *__restrict__ val,
                                                        const float *__restrict__ x, long ldx,
                                                        float *__restrict__ out, long ldo,
                                                        const float *__restrict__ self, long ld_self,
                                                        const int *__restrict__ long_rows, int n_long,
                                                        int long_thresh, int blocks_per_slab, int slab_cols,
                                                        SpmmExtra ex) {
    using ops = vec_ops<V>;
    __shared__ V part[4][CPL][LPE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    // several equal column slabs in ONE launch, slab-major (all workgroups of slab 0, then slab 1, ...): the slabs keep
    // their temporal locality and the tail of one overlaps the start of the next (a separate launch costs ~25 us)
    const int slab = (int)blockIdx.x / blocks_per_slab;
    const int bid = (int)blockIdx.x - slab * blocks_per_slab;
    x += (long)slab * slab_cols;
    out += (long)slab * slab_cols;
    if (self) self += (long)slab * slab_cols;
    ex.shift((long)slab * slab_cols);
    const bool team = bid < n_long;     // workgroup-uniform
    int row;
    if (team) {
        row = long_rows[bid];
    } else {
        row = (bid - n_long) * 4 + w;
        if (ex.row_list) {               // a structure of mostly EMPTY rows: one wave per row that holds entries
            if (row >= ex.n_list) return;
            row = ex.row_list[row];
        } else if (row >= n_rows) {
            return;
        }
    }
    const int start = __builtin_amdgcn_readfirstlane(rowptr[row]);
    const int end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
    if (!team && n_long > 0 && end - start > long_thresh) return;
    V acc[CPL];
#pragma unroll
    for (int i = 0; i < CPL; ++i) acc[i] = ops::zero();
    bool any = true;
    if constexpr (XF)
        any = accumulate_entries_flagged<V, LPE, CPL, FULL>(acc, start, end, team ? w : 0, team ? 4 : 1, lane, nchunk, col,
                                                            val, x, ldx, ex.x_rows);
    else
        accumulate_entries<V, LPE, CPL, U, FULL>(acc, start, end, team ? w : 0, team ? 4 : 1, lane, nchunk, col, val, x,
                                                 ldx);
#pragma unroll
    for (int i = 0; i < CPL; ++i) reduce_subgroups<V, LPE>(acc[i]);
    if (team) {
        if (lane < LPE)
#pragma unroll
            for (int i = 0; i < CPL; ++i) part[w][i][lane] = acc[i];
        any = __syncthreads_or(any);
        if (w != 0) return;
        if (lane < LPE)
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                acc[i] = part[0][i][lane];
#pragma unroll
                for (int k = 1; k < 4; ++k) ops::fma(acc[i], 1.f, part[k][i][lane]);
            }
    }
    float rmax = 0.f;
    if (lane < LPE) {
        V *dst = reinterpret_cast<V *>(out + (long)row * ldo);
        const V *own = self && (!ex.self_rows || ex.self_rows[row]) ? reinterpret_cast<const V *>(self + (long)row * ld_self) : nullptr;
        const V *own2 = reinterpret_cast<const V *>(ex.add2_row(row));
        if constexpr (XF) {
            if (ex.out_rows) {       // row-sparse output: flag the rows that received anything, leave the others alone
                if (!(any || own || own2)) return;
                if (lane == 0) ex.out_rows[row] = 1;
            }
        }
        const V *csrc = ex.copy_dst ? reinterpret_cast<const V *>(ex.copy_src + (long)row * ex.ld_copy_src) : nullptr;
        V *cdst = ex.copy_dst ? reinterpret_cast<V *>(ex.copy_dst + (long)row * ex.ld_copy_dst) : nullptr;
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int chunk = lane + i * LPE;
            if (FULL || chunk < nchunk) {
                if (own) ops::fma(acc[i], 1.f, own[chunk]);   // out = self + A @ x  (ego + side, model.py:109)
                if (own2) ops::fma(acc[i], 1.f, own2[chunk]);
#ifndef LKG_SPMM_PLAIN
                if constexpr (std::is_same<V, float4>::value) {
                    typedef float nt4 __attribute__((ext_vector_type(4)));
                    const nt4 nv = {acc[i].x, acc[i].y, acc[i].z, acc[i].w};
                    __builtin_nontemporal_store(nv, reinterpret_cast<nt4 *>(dst + chunk));
                } else {
                    __builtin_nontemporal_store(acc[i], dst + chunk);
                }
#else
                dst[chunk] = acc[i];
#endif
                if (cdst) cdst[chunk] = csrc[chunk];
                rmax = fmaxf(rmax, ops::absmax(acc[i]));
            }
        }
    }
    if (ex.rowmax) {       // (workgroup-uniform; every lane of the wave is here)
        rmax = wave_max(rmax);
        if (lane == 0) atomicMax(ex.rowmax + row, __float_as_int(rmax));
    }
}

// Rows-per-wave form for NARROW rows (nchunk <= 32 chunks, i.e. at most 128 floats): the 64/LPE sub-groups of a
// wave each own a DIFFERENT row and walk its entries themselves, U gathers in flight per sub-group.  With one wave
// per row a 20-entry row of 128-byte source rows keeps < 1 KB in flight for a third of the wave's life (rowptr ->
// (col,val) -> gathers -> store are dependent round trips) and the launch is bound by wave turnover, not by HBM
// (measured on MI355X, 5 M rows x 100 M entries x 32 columns: 5.8 TB/s, against 7.1 TB/s for the same kernel on
// 100-entry rows).  Here one wave turnover serves 64/LPE rows and no cross-sub-group reduction is needed.
//   * every lane fetches one (col, val) of ITS row's current LPE-entry chunk (sub-groups read consecutive
//     segments of the entry stream, rows being consecutive) and the sub-group broadcasts them with ds_bpermute;
//   * the trip count is the longest row of the wave; finished sub-groups keep re-reading their last source row
//     with weight 0 (an L1 hit), so the loop stays branch-free like accumulate_entries;
//   * rows over long_thresh stay on the leading team workgroups.
// Measured (MI355X, zipf heads / uniform tails, U = 8): 5 M x 100 M x 32 columns forward 2.41 -> 2.17 ms, transpose
// 2.18 -> 2.10 ms (6.6-6.8 TB/s algorithmic).  At 64 columns and wider the wave-per-row kernel is already at
// 7.2-7.6 TB/s and this form is 2-4 % slower, so it is used for rows of at most 32 floats only.
template <typename V, int LPE, int U, bool FULL>
__global__ __launch_bounds__(256) void spmm_csr_grouped_kernel(int n_rows, int nchunk,
                                                                const int *__restrict__ rowptr,
                                                                const int *__restrict__ col,
                                                                const float *__restrict__ val,
                                                                const float *__restrict__ x, long ldx,
                                                                float *__restrict__ out, long ldo,
                                                                const float *__restrict__ self, long ld_self,
                                                                const int *__restrict__ long_rows, int n_long,
                                                                int long_thresh, SpmmExtra ex) {
    using ops = vec_ops<V>;
    static_assert(LPE <= 32 && LPE % U == 0, "grouped SpMM: 2+ rows per wave, whole U-groups per chunk");
    __shared__ V part[4][LPE];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    if ((int)blockIdx.x < n_long) {   // one long row per workgroup, exactly as in spmm_csr_kernel
        const int row = long_rows[blockIdx.x];
        const int start = __builtin_amdgcn_readfirstlane(rowptr[row]);
        const int end = __builtin_amdgcn_readfirstlane(rowptr[row + 1]);
        V acc[1] = {ops::zero()};
        accumulate_entries<V, LPE, 1, U, FULL>(acc, start, end, w, 4, lane, nchunk, col, val, x, ldx);
        reduce_subgroups<V, LPE>(acc[0]);
        if (lane < LPE) part[w][lane] = acc[0];
        __syncthreads();
        if (w != 0 || lane >= LPE || !(FULL || lane < nchunk)) return;
        V a = part[0][lane];
#pragma unroll
        for (int k = 1; k < 4; ++k) ops::fma(a, 1.f, part[k][lane]);
        if (self) ops::fma(a, 1.f, reinterpret_cast<const V *>(self + (long)row * ld_self)[lane]);
        if (const float *a2 = ex.add2_row(row)) ops::fma(a, 1.f, reinterpret_cast<const V *>(a2)[lane]);
        reinterpret_cast<V *>(out + (long)row * ldo)[lane] = a;
        if (ex.rowmax) atomicMax(ex.rowmax + row, __float_as_int(ops::absmax(a)));
        if (ex.copy_dst)
            reinterpret_cast<V *>(ex.copy_dst + (long)row * ex.ld_copy_dst)[lane] =
                reinterpret_cast<const V *>(ex.copy_src + (long)row * ex.ld_copy_src)[lane];
        return;
    }
    constexpr int RPW = 64 / LPE;
    const int sub = lane / LPE, sl = lane % LPE;
    const int slot = (((int)blockIdx.x - n_long) * 4 + w) * RPW + sub;
    const bool valid = slot < n_rows;
    const int row = valid ? slot : 0;
    int start = 0, len = 0;
    if (valid) {
        start = rowptr[row];
        len = rowptr[row + 1] - start;
    }
    const bool mine = valid && !(n_long > 0 && len > long_thresh);
    if (!mine) len = 0;
    int maxlen = len;
    // idle sub-groups (empty, skipped or out-of-range rows) gather, with weight 0, an entry of a LIVE row of this wave:
    // always a valid entry of this launch's row range (x may be a shifted view that only covers those, x_row_offset)
    int spare = len > 0 ? start : -1;
#pragma unroll
    for (int m = LPE; m < 64; m <<= 1) {
        maxlen = max(maxlen, __shfl_xor(maxlen, m, 64));
        spare = max(spare, __shfl_xor(spare, m, 64));
    }
    V acc = ops::zero();
    for (int k = 0; k < maxlen; k += LPE) {
        const int j = k + sl;
        const int jc = len > 0 ? start + min(j, len - 1) : spare;   // maxlen > 0: some row of the wave has entries
        const int c = col[jc];
        const float v = j < len ? val[jc] : 0.f;
        const int mcnt = min(LPE, maxlen - k);                    // wave-uniform
        for (int q = 0; q < mcnt; q += U) {
            int cc[U];
            float vv[U];
            V xv[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                cc[u] = __shfl(c, sub * LPE + q + u, 64);
                vv[u] = __shfl(v, sub * LPE + q + u, 64);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const V *src = reinterpret_cast<const V *>(x + (long)cc[u] * ldx);
                xv[u] = FULL ? src[sl] : src[min(sl, nchunk - 1)];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) ops::fma(acc, vv[u], xv[u]);
        }
    }
    const bool writes = mine && (FULL || sl < nchunk);
    if (writes) {
        if (len == 0) acc = ops::zero();   // an empty row is exactly 0 (0 * Inf/NaN of the spare gathers must not leak)
        if (self) ops::fma(acc, 1.f, reinterpret_cast<const V *>(self + (long)row * ld_self)[sl]);
        if (const float *a2 = ex.add2_row(row)) ops::fma(acc, 1.f, reinterpret_cast<const V *>(a2)[sl]);
        reinterpret_cast<V *>(out + (long)row * ldo)[sl] = acc;
        if (ex.copy_dst)
            reinterpret_cast<V *>(ex.copy_dst + (long)row * ex.ld_copy_dst)[sl] =
                reinterpret_cast<const V *>(ex.copy_src + (long)row * ex.ld_copy_src)[sl];
    }
    if (ex.rowmax) {       // (wave-uniform: every lane is here)  ONE atomic per row: the LPE lanes of a row meet first -- an
        const float rm = group_max<LPE>(writes ? ops::absmax(acc) : 0.f);   // atomic per lane cost the forward launches of
        if (mine && sl == 0) atomicMax(ex.rowmax + row, __float_as_int(rm));   // 32-wide layers 0.3 ms each (0.55 vs 0.23 ms)
    }
}

// Row-sparse x, FOUR rows per wave.  With almost nothing to gather a row is a chain of dependent round trips (rowptr ->
// col -> flag) and nothing else; one wave per row leaves the launch bound by wave turnover (1 M rows: 0.43 ms).  Here
// the four 16-lane quarters of a wave scan four consecutive rows at once -- 16 entries each per pass, one ballot for
// all four -- and the (rare) flagged entries are gathered by the whole wave, one at a time, into the accumulators of
// their row; then the wave writes the four rows (64 lanes x 16 bytes x CPL).  Rows over long_thresh entries are left
// to the team workgroups of spmm_csr_kernel (a second, tiny launch).
template <int CPL, bool FULL>
__global__ __launch_bounds__(256) void spmm_flagged4_kernel(int n_rows, int nchunk, const int *__restrict__ rowptr,
                                                             const int *__restrict__ col, const float *__restrict__ val,
                                                             const float *__restrict__ x, long ldx,
                                                             float *__restrict__ out, long ldo,
                                                             const float *__restrict__ self, long ld_self, int n_long,
                                                             int long_thresh, SpmmExtra ex) {
    const int lane = threadIdx.x & 63, q = lane >> 4, ql = lane & 15;
    const int task = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int row_q = task * 4 + q;                         // this quarter's row
    int start = 0, len = 0;
    if (row_q < n_rows) {
        start = rowptr[row_q];
        len = rowptr[row_q + 1] - start;
        if (n_long > 0 && len > long_thresh) len = 0;       // (a team workgroup's row)
    }
    int maxlen = len;
    maxlen = max(maxlen, __shfl_xor(maxlen, 16, 64));
    maxlen = max(maxlen, __shfl_xor(maxlen, 32, 64));
    float4 acc[4][CPL];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < CPL; ++i) acc[r][i] = f4_zero();
    unsigned any = 0;                                       // bit r: row r of the four met a flagged entry
    for (int p = 0; p < maxlen; p += 16) {
        const int j = p + ql;
        const bool in = j < len;
        const int jj = start + (in ? j : 0);
        const int c = len > 0 ? col[jj] : 0;
        unsigned long long m = __ballot(in && ex.x_rows[c] != 0);
        if (m == 0) continue;                               // (wave-uniform)
        const float v = in ? val[jj] : 0.f;
        while (m) {
            const int b = __builtin_ctzll(m);
            m &= m - 1;
            const int r = b >> 4;                           // (wave-uniform)
            const int cc = __builtin_amdgcn_readlane(c, b);
            const float vv = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), b));
            const float4 *src = reinterpret_cast<const float4 *>(x + (long)cc * ldx);
            any |= 1u << r;
#pragma unroll
            for (int i = 0; i < CPL; ++i) {
                const int chunk = lane + i * 64;
                const float4 xv = (FULL || chunk < nchunk) ? src[chunk] : f4_zero();
                if (r == 0) f4_fma(acc[0][i], vv, xv);
                else if (r == 1) f4_fma(acc[1][i], vv, xv);
                else if (r == 2) f4_fma(acc[2][i], vv, xv);
                else f4_fma(acc[3][i], vv, xv);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = task * 4 + r;
        if (row >= n_rows) break;
        const int rfull = rowptr[row + 1] - rowptr[row];    // (team rows: written by their workgroup, not here)
        if (n_long > 0 && rfull > long_thresh) continue;
        const float *own = self && (!ex.self_rows || ex.self_rows[row]) ? self + (long)row * ld_self : nullptr;
        const float *own2 = ex.add2_row(row);
        if (ex.out_rows) {
            if (!(((any >> r) & 1) || own || own2)) continue;
            if (lane == 0) ex.out_rows[row] = 1;
        }
        float4 *dst = reinterpret_cast<float4 *>(out + (long)row * ldo);
#pragma unroll
        for (int i = 0; i < CPL; ++i) {
            const int chunk = lane + i * 64;
            if (FULL || chunk < nchunk) {
                float4 a = acc[r][i];
                if (own) f4_fma(a, 1.f, reinterpret_cast<const float4 *>(own)[chunk]);
                if (own2) f4_fma(a, 1.f, reinterpret_cast<const float4 *>(own2)[chunk]);
                dst[chunk] = a;
            }
        }
    }
}

// The rows WITHOUT entries of a structure that is mostly such rows (BASELINE config[0]'s shape: 766 k entity rows, 84 % of them
// never a head): out = (self +) (add2 +) 0, the row copy and the row maximum -- a streaming pass, one 16-byte (or 4-byte)
// chunk per thread, instead of one wave (a workgroup slot, a rowptr round trip) per empty row: with one wave per row the
// launch was bound by the rate at which workgroups start, not by HBM (0.28 ms for 0.46 GB).
template <typename V, int LPR>
__global__ __launch_bounds__(256) void spmm_listless_rows_kernel(long n_list, const int *__restrict__ rows, int nchunk,
                                                                  float *__restrict__ out, long ldo,
                                                                  const float *__restrict__ self, long ld_self, SpmmExtra ex) {
    // LPR lanes per row (a power of two <= 64), 256 / LPR rows per workgroup; the row maximum meets inside the group (one
    // plain store per row: nobody else writes an empty row's maximum -- an atomic per chunk cost this pass 0.3 ms at 644 k rows)
    using ops = vec_ops<V>;
    const int sl = threadIdx.x % LPR;
    const long r = (long)blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    const bool live = r < n_list;
    const long row = live ? rows[r] : 0;
    float mx = 0.f;
    if (live) {
        const float *a2 = ex.add2_row(row);
        for (int chunk = sl; chunk < nchunk; chunk += LPR) {
            V acc = ops::zero();
            if (self) ops::fma(acc, 1.f, reinterpret_cast<const V *>(self + row * ld_self)[chunk]);
            if (a2) ops::fma(acc, 1.f, reinterpret_cast<const V *>(a2)[chunk]);
            reinterpret_cast<V *>(out + row * ldo)[chunk] = acc;
            if (ex.copy_dst)
                reinterpret_cast<V *>(ex.copy_dst + row * ex.ld_copy_dst)[chunk] =
                    reinterpret_cast<const V *>(ex.copy_src + row * ex.ld_copy_src)[chunk];
            mx = fmaxf(mx, ops::absmax(acc));
        }
    }
    if (ex.rowmax) {                       // (workgroup-uniform; every lane takes part in the group reduction)
        mx = group_max<LPR>(mx);
        if (live && sl == 0) ex.rowmax[row] = __float_as_int(mx);
    }
}

template <typename V, int LPE, int U, bool FULL>
int launch_grouped(int64_t n_rows, int nchunk, const int *rowptr, const int *col, const float *val, const float *x,
                   int64_t ldx, float *out, int64_t ldo, const float *self, int64_t ld_self, const int *long_rows,
                   int n_long, int long_thresh, const SpmmExtra &ex, hipStream_t s) {
    constexpr int rows_per_block = 4 * (64 / LPE);
    const int64_t blocks = (n_rows + rows_per_block - 1) / rows_per_block + n_long;
    LKG_REQUIRE(blocks * 256 < (int64_t)UINT32_MAX, "lkg_spmm_csr_f32: grid too large (%lld workgroups)", (long long)blocks);
    hipLaunchKernelGGL((spmm_csr_grouped_kernel<V, LPE, U, FULL>), dim3((unsigned)blocks), dim3(256), 0, s,
                       (int)n_rows, nchunk, rowptr, col, val, x, (long)ldx, out, (long)ldo, self, (long)ld_self,
                       long_rows, n_long, long_thresh, ex);
    LKG_CHECK_LAUNCH("lkg_spmm_csr_f32");
    return LKG_OK;
}

template <typename V, int LPE, int CPL, int U, bool FULL>
int launch(int64_t n_rows, int nchunk, const int *rowptr, const int *col, const float *val, const float *x,
           int64_t ldx, float *out, int64_t ldo, const float *self, int64_t ld_self, const int *long_rows, int n_long,
           int long_thresh, int n_slabs, int slab_cols, const SpmmExtra &ex, hipStream_t s) {
    const int64_t blocks = ((ex.row_list ? (int64_t)ex.n_list : n_rows) + 3) / 4 + n_long;
    LKG_REQUIRE(blocks * n_slabs * 256 < (int64_t)UINT32_MAX, "lkg_spmm_csr_f32: grid too large (%lld workgroups)",
                (long long)(blocks * n_slabs));
    // (the scalar path too: x_rows promises that the unflagged rows of x are not READ -- they may hold anything)
    if (ex.x_rows) {
        hipLaunchKernelGGL((spmm_csr_kernel<V, LPE, CPL, U, FULL, true>), dim3((unsigned)(blocks * n_slabs)), dim3(256), 0,
                           s, (int)n_rows, nchunk, rowptr, col, val, x, (long)ldx, out, (long)ldo, self,
                           (long)ld_self, long_rows, n_long, long_thresh, (int)blocks, slab_cols, ex);
        LKG_CHECK_LAUNCH("lkg_spmm_csr_f32");
        return LKG_OK;
    }
    hipLaunchKernelGGL((spmm_csr_kernel<V, LPE, CPL, U, FULL, false>), dim3((unsigned)(blocks * n_slabs)), dim3(256), 0, s,
                       (int)n_rows, nchunk, rowptr, col, val, x, (long)ldx, out, (long)ldo, self, (long)ld_self,
                       long_rows, n_long, long_thresh, (int)blocks, slab_cols, ex);
    LKG_CHECK_LAUNCH("lkg_spmm_csr_f32");
    return LKG_OK;
}

// Experiment switches, COMPILE-TIME only (LKG_EXTRA_HIPCC_FLAGS="-DLKG_SPMM_U=8" / "-DLKG_SPMM_GROUPED_CHUNKS=32" and a
// rebuild): the shipped library holds the measured defaults and nothing in its environment can select a variant that the
// parity suite never ran (round 3 measured all of them within noise of the defaults at the 5 M / 100 M shape).
#ifndef LKG_SPMM_U
#define LKG_SPMM_U 4                     /* gathers in flight per half-wave for 128-column rows: 2 | 4 | 8 */
#endif
#ifndef LKG_SPMM_GROUPED_CHUNKS
#define LKG_SPMM_GROUPED_CHUNKS 8        /* widest row (in 16-byte chunks) that takes several rows per wave: 8 | 16 | 32 */
#endif

template <typename V>
int dispatch(int64_t n_rows, int nchunk, const int *rowptr, const int *col, const float *val, const float *x,
             int64_t ldx, float *out, int64_t ldo, const float *self, int64_t ld_self, const int *long_rows, int n_long,
             int long_thresh, int n_slabs, int slab_cols, const SpmmExtra &ex, hipStream_t s) {
#define LKG_GO(LPE, CPL, U)                                                                              \
    return (nchunk == LPE * CPL)                                                                         \
               ? launch<V, LPE, CPL, U, true>(n_rows, nchunk, rowptr, col, val, x, ldx, out, ldo, self, ld_self, \
                                              long_rows, n_long, long_thresh, n_slabs, slab_cols, ex, s)  \
               : launch<V, LPE, CPL, U, false>(n_rows, nchunk, rowptr, col, val, x, ldx, out, ldo, self, ld_self, \
                                               long_rows, n_long, long_thresh, n_slabs, slab_cols, ex, s)
    // rows of <= 32 floats: 8 rows per wave (see spmm_csr_grouped_kernel); a row-sparse x -- the long rows behind
    // spmm_flagged4_kernel -- stays on the wave-per-row kernel's flagged form
    if (nchunk <= 8 && !ex.x_rows && !ex.row_list)
        return (nchunk == 8) ? launch_grouped<V, 8, 8, true>(n_rows, nchunk, rowptr, col, val, x, ldx, out, ldo, self,
                                                            ld_self, long_rows, n_long, long_thresh, ex, s)
                             : launch_grouped<V, 8, 8, false>(n_rows, nchunk, rowptr, col, val, x, ldx, out, ldo, self,
                                                             ld_self, long_rows, n_long, long_thresh, ex, s);
    if constexpr (std::is_same<V, float4>::value) {
#if LKG_SPMM_GROUPED_CHUNKS >= 16            // (experiment build: several rows per wave for 64- / 128-column rows too)
        if (!ex.x_rows && !ex.row_list && n_slabs == 1 && nchunk == 16)
            return launch_grouped<V, 16, 8, true>(n_rows, nchunk, rowptr, col, val, x, ldx, out, ldo, self, ld_self, long_rows,
                                                  n_long, long_thresh, ex, s);
#endif
#if LKG_SPMM_GROUPED_CHUNKS >= 32
        if (!ex.x_rows && !ex.row_list && n_slabs == 1 && nchunk == 32)
            return launch_grouped<V, 32, 8, true>(n_rows, nchunk, rowptr, col, val, x, ldx, out, ldo, self, ld_self, long_rows,
                                                  n_long, long_thresh, ex, s);
#endif
    }
    if (nchunk <= 16) LKG_GO(16, 1, 4);
    if (nchunk <= 32) {
        LKG_GO(32, 1, LKG_SPMM_U);
    }
    if (nchunk <= 64) LKG_GO(64, 1, 4);
    if (nchunk <= 128) LKG_GO(64, 2, 4);
    if (nchunk <= 192) LKG_GO(64, 3, 2);
    LKG_GO(64, 4, 2);
#undef LKG_GO
}

}  // namespace

extern "C" int lkg_spmm_csr_fused_f32(int64_t n_rows, int32_t d, const int32_t *rowptr, const int32_t *col,
                                      const float *val, const float *x, int64_t ldx, float *out, int64_t ldo,
                                      const float *self, int64_t ld_self, const float *add2, int64_t ld_add2,
                                      const uint8_t *add2_rows, const float *copy_src, int64_t ld_copy_src,
                                      float *copy_dst, int64_t ld_copy_dst, float *rowmax_out, const uint8_t *x_rows,
                                      const uint8_t *self_rows, uint8_t *out_rows, const int32_t *long_rows,
                                      int32_t n_long, int32_t long_thresh, const int32_t *rows_with_entries,
                                      int64_t n_rows_with_entries, const int32_t *rows_without_entries,
                                      int64_t n_rows_without_entries, void *stream) {
    LKG_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX, "lkg_spmm_csr_f32: n_rows %lld out of range", (long long)n_rows);
    LKG_REQUIRE(d > 0, "lkg_spmm_csr_f32: d must be positive (got %d)", d);
    LKG_REQUIRE(ldx >= d && ldo >= d, "lkg_spmm_csr_f32: row strides (%lld, %lld) smaller than d=%d", (long long)ldx,
                (long long)ldo, d);
    LKG_REQUIRE(n_long >= 0 && (n_long == 0 || (long_rows && long_thresh >= 64)),
                "lkg_spmm_csr_f32: long-row list needs a pointer and a threshold >= 64");
    if (n_rows == 0) return LKG_OK;
    LKG_REQUIRE(rowptr && x && out, "lkg_spmm_csr_f32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    LKG_REQUIRE(!self || ld_self >= d, "lkg_spmm_csr_f32: self stride %lld smaller than d=%d", (long long)ld_self, d);
    LKG_REQUIRE(!add2 || ld_add2 >= d || ld_add2 == 0, "lkg_spmm_csr_fused_f32: add2 stride %lld smaller than d=%d (0 = one row for "
                "every output row)", (long long)ld_add2, d);
    LKG_REQUIRE(!copy_dst || (copy_src && ld_copy_src >= d && ld_copy_dst >= d),
                "lkg_spmm_csr_fused_f32: the row copy needs a source and strides >= d=%d", d);
    const bool vec = (d % 4 == 0) && (ldx % 4 == 0) && (ldo % 4 == 0) && lkg_aligned16(x) && lkg_aligned16(out) &&
                     (!self || (ld_self % 4 == 0 && lkg_aligned16(self))) &&
                     (!add2 || (ld_add2 % 4 == 0 && lkg_aligned16(add2))) &&
                     (!copy_dst || (ld_copy_src % 4 == 0 && ld_copy_dst % 4 == 0 && lkg_aligned16(copy_src) &&
                                    lkg_aligned16(copy_dst)));
    if (rowmax_out && hipMemsetAsync(rowmax_out, 0, sizeof(float) * n_rows, s) != hipSuccess) {
        lkg_set_error("lkg_spmm_csr_fused_f32: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    LKG_REQUIRE(!out_rows || (x_rows && vec && !rowmax_out && !copy_dst && d <= 1024),
                "lkg_spmm_csr_fused_f32: out_rows needs x_rows, the 16-byte path (d %% 4 == 0, aligned rows, d <= 1024), no row "
                "copy and no rowmax_out");
    if (out_rows && hipMemsetAsync(out_rows, 0, n_rows, s) != hipSuccess) {
        lkg_set_error("lkg_spmm_csr_fused_f32: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    const bool listed = rows_with_entries != nullptr;
    LKG_REQUIRE(!listed || ((rows_without_entries || n_rows_without_entries == 0) && !x_rows && !out_rows &&
                            n_rows_with_entries >= 0 && n_rows_without_entries >= 0 &&
                            n_rows_with_entries + n_rows_without_entries == n_rows),
                "lkg_spmm_csr_fused_f32: the row lists must partition the %lld rows (and exclude x_rows / out_rows)",
                (long long)n_rows);
    const SpmmExtra ex{add2, (long)ld_add2, add2 ? add2_rows : nullptr, copy_dst ? copy_src : nullptr, (long)ld_copy_src, copy_dst,
                       (long)ld_copy_dst, reinterpret_cast<int *>(rowmax_out), x_rows, self ? self_rows : nullptr, out_rows,
                       listed ? rows_with_entries : nullptr, listed ? (int)n_rows_with_entries : 0};
    if (listed && n_rows_without_entries > 0) {      // the rows without entries: one streaming pass (all column slabs at once)
        const int nchunk_all = vec ? d / 4 : d;
        const int lpr = nchunk_all <= 8 ? 8 : nchunk_all <= 16 ? 16 : nchunk_all <= 32 ? 32 : 64;
        const int64_t blocks_e = (n_rows_without_entries + 256 / lpr - 1) / (256 / lpr);
        LKG_REQUIRE(blocks_e < (int64_t)UINT32_MAX, "lkg_spmm_csr_f32: grid too large");
#define LKG_LISTLESS(V_, LPR_)                                                                                          \
    hipLaunchKernelGGL((spmm_listless_rows_kernel<V_, LPR_>), dim3((unsigned)blocks_e), dim3(256), 0, s,                \
                       (long)n_rows_without_entries, rows_without_entries, nchunk_all, out, (long)ldo, self,            \
                       (long)ld_self, ex)
        if (vec) {
            if (lpr == 8) LKG_LISTLESS(float4, 8);
            else if (lpr == 16) LKG_LISTLESS(float4, 16);
            else if (lpr == 32) LKG_LISTLESS(float4, 32);
            else LKG_LISTLESS(float4, 64);
        } else {
            if (lpr == 8) LKG_LISTLESS(float, 8);
            else if (lpr == 16) LKG_LISTLESS(float, 16);
            else if (lpr == 32) LKG_LISTLESS(float, 32);
            else LKG_LISTLESS(float, 64);
        }
#undef LKG_LISTLESS
        LKG_CHECK_LAUNCH("lkg_spmm_csr_f32");
        if (n_rows_with_entries == 0 && n_long == 0) return LKG_OK;
    }
    // Column slabs.  Rows wider than 128 floats are aggregated 128 columns (512 B per gathered row) at a time:
    // measured on MI355X the slab form is 10-30 % faster than one full-width pass (1 M x 256: 1.83 -> 1.56 ms,
    // 1 M x 512: 4.13 -> 3.10 ms, 2 M x 256: 4.09 -> 3.70 ms) -- a half-wave per row keeps two rows per wave in
    // flight and a 128-column slab of the source table is 2-4x more likely to be served from the 256 MiB
    // Infinity Cache -- at the price of re-reading the (col, val) stream once per slab (+8 B per entry per slab).
    // The scalar (unaligned) path keeps up to 256 columns per launch.
    if (x_rows && vec && !copy_dst && !rowmax_out && d <= 1024) {
        // row-sparse x: four rows per wave (spmm_flagged4_kernel); the rows over long_thresh entries on team workgroups
        const int nchunk = d / 4, cpl = (nchunk + 63) / 64;
        const bool full = nchunk == 64 * cpl;
        const int64_t tasks = (n_rows + 3) / 4, blocks = (tasks + 3) / 4;
        LKG_REQUIRE(blocks * 256 < (int64_t)UINT32_MAX, "lkg_spmm_csr_f32: grid too large (%lld workgroups)", (long long)blocks);
#define LKG_F4(CPL_)                                                                                                   \
    case CPL_:                                                                                                         \
        if (full)                                                                                                      \
            hipLaunchKernelGGL((spmm_flagged4_kernel<CPL_, true>), dim3((unsigned)blocks), dim3(256), 0, s, (int)n_rows, \
                               nchunk, rowptr, col, val, x, (long)ldx, out, (long)ldo, self, (long)ld_self, n_long,     \
                               long_thresh, ex);                                                                       \
        else                                                                                                           \
            hipLaunchKernelGGL((spmm_flagged4_kernel<CPL_, false>), dim3((unsigned)blocks), dim3(256), 0, s, (int)n_rows, \
                               nchunk, rowptr, col, val, x, (long)ldx, out, (long)ldo, self, (long)ld_self, n_long,     \
                               long_thresh, ex);                                                                       \
        break;
        switch (cpl) { LKG_F4(1) LKG_F4(2) LKG_F4(3) LKG_F4(4) }
#undef LKG_F4
        LKG_CHECK_LAUNCH("lkg_spmm_csr_f32");
        if (n_long == 0) return LKG_OK;
        // the long rows: the team workgroups of the general kernel alone (n_rows = 0 leaves no ordinary row to it)
        for (int c0 = 0; c0 < d; c0 += 256) {
            const int dc = min(256, d - c0);
            const SpmmExtra exc{add2 ? add2 + c0 : nullptr, (long)ld_add2, add2 ? add2_rows : nullptr, nullptr, 0, nullptr, 0, nullptr,
                                x_rows, self ? self_rows : nullptr, out_rows, nullptr, 0};
            const int rc = dispatch<float4>(0, dc / 4, rowptr, col, val, x + c0, ldx, out + c0, ldo, self ? self + c0 : nullptr,
                                            ld_self, long_rows, n_long, long_thresh, 1, 0, exc, s);
            if (rc != LKG_OK) return rc;
        }
        return LKG_OK;
    }
    // (over a row-sparse x almost nothing is gathered: one pass over the entry stream per 256 columns, not per 128)
    const int block_cols = (vec && !x_rows) ? 128 : 256;
    const bool grouped_slabs = vec && !x_rows && block_cols / 4 <= LKG_SPMM_GROUPED_CHUNKS;   // (experiment: one launch per slab)
    if (d > block_cols && d % block_cols == 0 && !grouped_slabs)     // equal slabs: one launch, slab-major workgroup order
        return vec ? dispatch<float4>(n_rows, block_cols / 4, rowptr, col, val, x, ldx, out, ldo, self, ld_self,
                                      long_rows, n_long, long_thresh, d / block_cols, block_cols, ex, s)
                   : dispatch<float>(n_rows, block_cols, rowptr, col, val, x, ldx, out, ldo, self, ld_self, long_rows,
                                     n_long, long_thresh, d / block_cols, block_cols, ex, s);
    for (int c0 = 0; c0 < d; c0 += block_cols) {
        const int dc = min(block_cols, d - c0);
        const SpmmExtra exc{add2 ? add2 + c0 : nullptr, (long)ld_add2, add2 ? add2_rows : nullptr,
                            copy_dst ? copy_src + c0 : nullptr,
                            (long)ld_copy_src, copy_dst ? copy_dst + c0 : nullptr, (long)ld_copy_dst,
                            reinterpret_cast<int *>(rowmax_out), x_rows, self ? self_rows : nullptr, out_rows, ex.row_list, ex.n_list};
        int rc = vec ? dispatch<float4>(n_rows, dc / 4, rowptr, col, val, x + c0, ldx, out + c0, ldo,
                                        self ? self + c0 : nullptr, ld_self, long_rows, n_long, long_thresh, 1, 0, exc, s)
                     : dispatch<float>(n_rows, dc, rowptr, col, val, x + c0, ldx, out + c0, ldo,
                                       self ? self + c0 : nullptr, ld_self, long_rows, n_long, long_thresh, 1, 0, exc, s);
        if (rc != LKG_OK) return rc;
    }
    return LKG_OK;
}

extern "C" int lkg_spmm_csr_f32(int64_t n_rows, int32_t d, const int32_t *rowptr, const int32_t *col,
                                const float *val, const float *x, int64_t ldx, float *out, int64_t ldo,
                                const float *self, int64_t ld_self, const int32_t *long_rows, int32_t n_long,
                                int32_t long_thresh, void *stream) {
    return lkg_spmm_csr_fused_f32(n_rows, d, rowptr, col, val, x, ldx, out, ldo, self, ld_self, nullptr, 0, nullptr,
                                  nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, long_rows, n_long, long_thresh,
                                  nullptr, 0, nullptr, 0, stream);
}

// dst[i] = src[perm[i]].  An index outside [0, n_src) is never dereferenced (NaN is stored for it): a list that does not
// belong to `src` -- round 3's fault: a part's index list paired with the whole value array's length -- shows up as NaNs
// in the result instead of as a memory access fault of the device.
__global__ void permute_kernel(long n, long n_src, const int *__restrict__ perm, const float *__restrict__ src,
                               float *__restrict__ dst) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long stride = (long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        const long p = perm[i];
        dst[i] = (p >= 0 && p < n_src) ? src[p] : __builtin_nanf("");
    }
}

extern "C" int lkg_permute_f32(int64_t n, const int32_t *perm, int64_t n_src, const float *src, float *dst, void *stream) {
    LKG_REQUIRE(n >= 0 && n_src >= 0, "lkg_permute_f32: negative extent");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(perm && src && dst, "lkg_permute_f32: null pointer");
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 256 * 8);
    hipLaunchKernelGGL(permute_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n, (long)n_src, perm,
                       src, dst);
    LKG_CHECK_LAUNCH("lkg_permute_f32");
    return LKG_OK;
}

// ---------------------------------------------------------------------------------------------------
// Structure check: how many offsets / column ids of a CSR (a view into one: rowptr may start anywhere) would make an
// SpMM over it read outside its operands?  Counts rows whose offsets are not 0 <= rowptr[i] <= rowptr[i + 1] <= nnz and
// entries of the rows' range whose column id (minus col_offset) lies outside [0, n_cols).  One streaming pass.
__global__ __launch_bounds__(256) void csr_check_kernel(long n_rows, const int *__restrict__ rowptr, long nnz,
                                                        const int *__restrict__ col, long col_offset, long n_cols,
                                                        int *__restrict__ bad) {
    const long stride = (long)gridDim.x * blockDim.x;
    const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
    int mine = 0;
    for (long i = t0; i < n_rows; i += stride) {
        const long a = rowptr[i], b = rowptr[i + 1];
        mine += (a < 0 || a > b || b > nnz) ? 1 : 0;
    }
    // the entry range of the view, clamped to the arrays (a bad offset was counted above)
    long lo = rowptr[0], hi = rowptr[n_rows];
    lo = lo < 0 ? 0 : (lo > nnz ? nnz : lo);
    hi = hi < lo ? lo : (hi > nnz ? nnz : hi);
    for (long j = lo + t0; j < hi; j += stride) {
        const long c = (long)col[j] - col_offset;
        mine += (c < 0 || c >= n_cols) ? 1 : 0;
    }
    if (mine) atomicAdd(bad, mine);
}

extern "C" int lkg_csr_check_i32(int64_t n_rows, const int32_t *rowptr, int64_t nnz, const int32_t *col,
                                 int64_t col_offset, int64_t n_cols, int32_t *bad_out, void *stream) {
    LKG_REQUIRE(n_rows >= 0 && nnz >= 0 && n_cols >= 0, "lkg_csr_check_i32: negative extent");
    LKG_REQUIRE(rowptr && bad_out && (col || nnz == 0), "lkg_csr_check_i32: null pointer");
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(bad_out, 0, sizeof(int32_t), s) != hipSuccess) {
        lkg_set_error("lkg_csr_check_i32: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    const int64_t work = std::max<int64_t>(n_rows, nnz);
    const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((work + 255) / 256, 256 * 8));
    hipLaunchKernelGGL(csr_check_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (long)n_rows, rowptr, (long)nnz, col,
                       (long)col_offset, (long)n_cols, bad_out);
    LKG_CHECK_LAUNCH("lkg_csr_check_i32");
    return LKG_OK;
}

// ---------------------------------------------------------------------------------------------------
// Batch-pruned step (exact; see literalkg_amd/pruned.py): the loss reads <= 3B rows of the last layer, so
// layer k is only evaluated on the rows its consumers need.  Two helpers on the same CSR:
//   lkg_csr_extract_rows       copy the entries (col, val) of a sorted list of rows into a compact CSR
//   lkg_spmm_csr_scatter_bwd   backward of out = A_sub @ x for such a (small) sub-CSR without building its
//                              transpose every step:  g_x[col[j],:] += val[j] * g_out[row,:]  (f32 atomics,
//                              one 16-B-per-lane row segment per wave-instruction)
namespace {
__global__ __launch_bounds__(256) void extract_rows_kernel(long n_sel, const long *__restrict__ sel,
                                                            const int *__restrict__ rowptr,
                                                            const int *__restrict__ col, const float *__restrict__ val,
                                                            const int *__restrict__ out_rowptr,
                                                            int *__restrict__ out_col, float *__restrict__ out_val) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n_sel) return;
    const int src = rowptr[sel[i]], cnt = rowptr[sel[i] + 1] - src, dst = out_rowptr[i];
    for (int j = lane; j < cnt; j += 64) {
        out_col[dst + j] = col[src + j];
        out_val[dst + j] = val[src + j];
    }
}

__global__ __launch_bounds__(256) void spmm_scatter_bwd_kernel(long n_rows, int d, const int *__restrict__ rowptr,
                                                                const int *__restrict__ col,
                                                                const float *__restrict__ val,
                                                                const float *__restrict__ g_out, long ldg,
                                                                float *__restrict__ g_x, long ldx) {
    const int lane = threadIdx.x & 63;
    const long row = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_rows) return;
    const int start = rowptr[row], end = rowptr[row + 1];
    for (int c0 = 0; c0 < d; c0 += 64) {
        const int c = c0 + lane;
        const float g = c < d ? g_out[row * ldg + c] : 0.f;
        for (int j = start; j < end; ++j)
            if (c < d) atomicAdd(g_x + (long)col[j] * ldx + c, val[j] * g);
    }
}
}  // namespace

extern "C" int lkg_csr_extract_rows(int64_t n_sel, const int64_t *sel_rows, const int32_t *rowptr, const int32_t *col,
                                    const float *val, const int32_t *out_rowptr, int32_t *out_col, float *out_val,
                                    void *stream) {
    LKG_REQUIRE(n_sel >= 0, "lkg_csr_extract_rows: negative row count");
    if (n_sel == 0) return LKG_OK;
    LKG_REQUIRE(sel_rows && rowptr && col && val && out_rowptr && out_col && out_val,
                "lkg_csr_extract_rows: null pointer");
    hipLaunchKernelGGL(extract_rows_kernel, dim3((unsigned)((n_sel + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (long)n_sel, (const long *)sel_rows, rowptr, col, val, out_rowptr, out_col, out_val);
    LKG_CHECK_LAUNCH("lkg_csr_extract_rows");
    return LKG_OK;
}

extern "C" int lkg_spmm_csr_scatter_bwd_f32(int64_t n_rows, int32_t d, const int32_t *rowptr, const int32_t *col,
                                            const float *val, const float *g_out, int64_t ldg, float *g_x,
                                            int64_t ldx, void *stream) {
    LKG_REQUIRE(n_rows >= 0 && d > 0 && ldg >= d && ldx >= d, "lkg_spmm_csr_scatter_bwd_f32: bad sizes");
    if (n_rows == 0) return LKG_OK;
    LKG_REQUIRE(rowptr && col && val && g_out && g_x, "lkg_spmm_csr_scatter_bwd_f32: null pointer");
    hipLaunchKernelGGL(spmm_scatter_bwd_kernel, dim3((unsigned)((n_rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (long)n_rows, d, rowptr, col, val, g_out, (long)ldg, g_x, (long)ldx);
    LKG_CHECK_LAUNCH("lkg_spmm_csr_scatter_bwd_f32");
    return LKG_OK;
}

// lkg_preload(): HIP loads a translation unit's code object on the first use of one of its kernels; asking for a kernel's
// attributes is such a use (no launch).
int lkg_internal_preload_spmm() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&permute_kernel)) == hipSuccess ? 0 : 1;
}
