// Batch-side primitives of the TransR scoring path (model.py:371-395): grouping the batch by relation
// (so that W_r is applied as one GEMM per relation instead of a B x C x D gather), row gather of the
// batch's entity rows, and the scatter-add of their gradients (autograd of the three `index` ops).
#include <algorithm>

#include "lkg_common.h"
#include "lkg_known.h"

namespace {

constexpr int GB_WAVES = 16;

// Deterministic (stable) counting sort of `keys` by value, one workgroup.
//   perm[p] = position in the input of the p-th element in key order, seg[k] = first p of key k.
__global__ __launch_bounds__(1024) void group_by_key_kernel(long n, int n_keys, const long *__restrict__ keys,
                                                             int *__restrict__ perm, int *__restrict__ seg,
                                                             int *__restrict__ n_bad) {
    extern __shared__ int sm[];   // [n_keys][GB_WAVES] running offsets, then one counter of out-of-range keys
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int i = t; i < n_keys * GB_WAVES + 1; i += blockDim.x) sm[i] = 0;
    __syncthreads();
    const long chunk = ((n + GB_WAVES - 1) / GB_WAVES + 63) / 64 * 64;
    const long lo = min(n, (long)w * chunk), hi = min(n, lo + chunk);
    for (long i = lo + lane; i < hi; i += 64) {
        const long key = keys[i];
        // an out-of-range key is counted (the caller raises, like the reference's gat_trans_M[r] would) and grouped
        // with the nearest valid key only so that this launch and the ones queued behind it stay in bounds
        if (key < 0 || key >= n_keys) atomicAdd(&sm[n_keys * GB_WAVES], 1);
        const int k = (int)min(max(key, 0L), (long)n_keys - 1);
        atomicAdd(&sm[k * GB_WAVES + w], 1);
    }
    __syncthreads();
    if (t == 0) {
        if (n_bad) *n_bad = sm[n_keys * GB_WAVES];
        int run = 0;
        for (int k = 0; k < n_keys; ++k) {
            seg[k] = run;
            for (int j = 0; j < GB_WAVES; ++j) {
                const int c = sm[k * GB_WAVES + j];
                sm[k * GB_WAVES + j] = run;
                run += c;
            }
        }
        seg[n_keys] = run;
    }
    __syncthreads();
    for (long i0 = lo; i0 < hi; i0 += 64) {
        const long i = i0 + lane;
        const bool valid = i < hi;
        const int k = valid ? (int)min(max(keys[i], 0L), (long)n_keys - 1) : -1;
        unsigned long long todo = __ballot(valid);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int k0 = __shfl(k, leader, 64);
            const unsigned long long same = __ballot(k == k0);
            const int base = sm[k0 * GB_WAVES + w];
            if (k == k0) {
                const int rank = __popcll(same & ((1ull << lane) - 1ull));
                perm[base + rank] = (int)i;
            }
            // all lanes of the wave have read `base` before lane `leader` bumps it (same wave, in order)
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (lane == leader) sm[k0 * GB_WAVES + w] = base + __popcll(same);
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            todo &= ~same;
        }
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows_kernel(long n, int d, const float *__restrict__ src, long lds,
                                                           const long *__restrict__ idx, const int *__restrict__ perm,
                                                           float *__restrict__ dst, long ldd) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long p = perm ? perm[i] : i;
    const long r = idx ? idx[p] : p;
    if constexpr (VEC) {
        const float4 *s = reinterpret_cast<const float4 *>(src + r * lds);
        float4 *o = reinterpret_cast<float4 *>(dst + i * ldd);
        for (int c = lane; c < d / 4; c += 64) o[c] = s[c];
    } else {
        for (int c = lane; c < d; c += 64) dst[i * ldd + c] = src[r * lds + c];
    }
}

__global__ __launch_bounds__(256) void scatter_add_rows_kernel(long n, int d, const float *__restrict__ src, long lds,
                                                                const long *__restrict__ idx,
                                                                const int *__restrict__ perm, float *__restrict__ dst,
                                                                long ldd) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long p = perm ? perm[i] : i;
    const long r = idx ? idx[p] : p;
    for (int c = lane; c < d; c += 64) atomicAdd(dst + r * ldd + c, src[i * lds + c]);
}

// dst[idx[i], :] = value and, when given, flags[idx[i]] = flag: resets (or marks) the few rows a row-sparse gradient touched
// in a table that is otherwise kept all-zero between steps (duplicates in idx write the same bytes)
__global__ __launch_bounds__(256) void fill_rows_kernel(long n, int d, const long *__restrict__ idx, float *__restrict__ dst,
                                                         long ldd, float value, unsigned char *__restrict__ flags,
                                                         unsigned char flag) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long r = idx[i];
    if (r < 0) return;                 // (padding of a de-duplicated id list)
    if (dst)
        for (int c = lane; c < d; c += 64) dst[r * ldd + c] = value;
    if (flags && lane == 0) flags[r] = flag;
}

// Row-range forms for a table sharded by rows over ranks: this rank holds rows [lo, hi) (src / dst point at row lo).
//   gather : dst[i,:] = idx[i] in [lo, hi) ? src[idx[i] - lo, :] : 0     (the rows of other ranks arrive by all-reduce)
//   scatter: dst[idx[i] - lo, :] += src[i,:] for idx[i] in [lo, hi)      (f32 atomics)
__global__ __launch_bounds__(256) void gather_rows_range_kernel(long n, int d, const float *__restrict__ src, long lds,
                                                                 const long *__restrict__ idx, long lo, long hi,
                                                                 float *__restrict__ dst, long ldd) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long r = idx[i];
    const bool mine = r >= lo && r < hi;
    const float *s = src + (mine ? r - lo : 0) * lds;
    for (int c = lane; c < d; c += 64) dst[i * ldd + c] = mine ? s[c] : 0.f;
}

__global__ __launch_bounds__(256) void scatter_add_rows_range_kernel(long n, int d, const float *__restrict__ src,
                                                                      long lds, const long *__restrict__ idx, long lo,
                                                                      long hi, float *__restrict__ dst, long ldd) {
    const int lane = threadIdx.x & 63;
    const long i = (long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= n) return;
    const long r = idx[i];
    if (r < lo || r >= hi) return;
    for (int c = lane; c < d; c += 64) atomicAdd(dst + (r - lo) * ldd + c, src[i * lds + c]);
}

__global__ void gather_i64_kernel(long n, const long *__restrict__ src, const int *__restrict__ perm,
                                  long *__restrict__ dst) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        dst[i] = src[perm[i]];
}

// perm_out[p * k + j] = perm[p] * k + j, seg_out[s] = seg[s] * k: the row order of a batch of n groups x k rows whose
// GROUPS were sorted by key (the negatives of a grouped TransR batch follow their group)
__global__ void expand_groups_kernel(long n, int k, int n_seg, const int *__restrict__ perm, const int *__restrict__ seg,
                                     int *__restrict__ perm_out, int *__restrict__ seg_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (long)n_seg) seg_out[i] = seg[i] * k;
    if (i < n * k) perm_out[i] = perm[i / k] * k + (int)(i % k);
}

// mismatches of the a12 layout: rows j of group i that differ from the group's first row in h, r or t+
__global__ void check_grouped_kernel(long n, int k, const long *__restrict__ h, const long *__restrict__ r,
                                     const long *__restrict__ p, int *__restrict__ n_bad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const long f = i / k * k;
        bad = h[i] != h[f] || r[i] != r[f] || p[i] != p[f];
    }
    const unsigned long long m = __ballot(bad);   // taken by all lanes, before the divergent add
    if (m && (threadIdx.x & 63) == 0) atomicAdd(n_bad, (int)__popcll(m));
}

// out[i] = ids[i] when lo <= ids[i] < hi, else lo; *n_bad += the number of ids outside the range
__global__ __launch_bounds__(256) void sanitize_ids_kernel(long n, const long *__restrict__ ids, long lo, long hi,
                                                            long *__restrict__ out, int *__restrict__ n_bad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const long v = ids[i];
        bad = v < lo || v >= hi;
        out[i] = bad ? lo : v;
    }
    const unsigned long long m = __ballot(bad);   // taken by all lanes, before the divergent add
    if (m && (threadIdx.x & 63) == 0) atomicAdd(n_bad, (int)__popcll(m));
}

}  // namespace

extern "C" int lkg_expand_groups_i32(int64_t n_groups, int32_t rows_per_group, int32_t n_seg, const int32_t *perm,
                                     const int32_t *seg, int32_t *perm_out, int32_t *seg_out, void *stream) {
    LKG_REQUIRE(n_groups >= 0 && rows_per_group >= 1 && n_seg >= 1 && n_groups * rows_per_group < INT32_MAX,
                "lkg_expand_groups_i32: bad sizes");
    LKG_REQUIRE(seg && seg_out && (n_groups == 0 || (perm && perm_out)), "lkg_expand_groups_i32: null pointer");
    const int64_t n = std::max<int64_t>(n_groups * rows_per_group, n_seg);
    hipLaunchKernelGGL(expand_groups_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (long)n_groups, rows_per_group, n_seg, perm, seg, perm_out, seg_out);
    LKG_CHECK_LAUNCH("lkg_expand_groups_i32");
    return LKG_OK;
}

extern "C" int lkg_sanitize_ids_i64(int64_t n, const int64_t *ids, int64_t lo, int64_t hi, int64_t *out, int32_t *n_bad,
                                    void *stream) {
    LKG_REQUIRE(n >= 0 && lo < hi, "lkg_sanitize_ids_i64: bad sizes");
    LKG_REQUIRE(n_bad && (n == 0 || (ids && out)), "lkg_sanitize_ids_i64: null pointer");
    if (hipMemsetAsync(n_bad, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
        lkg_set_error("lkg_sanitize_ids_i64: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    if (n == 0) return LKG_OK;
    hipLaunchKernelGGL(sanitize_ids_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long)n,
                       (const long *)ids, (long)lo, (long)hi, (long *)out, n_bad);
    LKG_CHECK_LAUNCH("lkg_sanitize_ids_i64");
    return LKG_OK;
}

extern "C" int lkg_check_grouped_i64(int64_t n, int32_t rows_per_group, const int64_t *h, const int64_t *r,
                                     const int64_t *pos_t, int32_t *n_bad, void *stream) {
    LKG_REQUIRE(n >= 0 && rows_per_group >= 1, "lkg_check_grouped_i64: bad sizes");
    LKG_REQUIRE(n_bad && (n == 0 || (h && r && pos_t)), "lkg_check_grouped_i64: null pointer");
    if (hipMemsetAsync(n_bad, 0, sizeof(int32_t), (hipStream_t)stream) != hipSuccess) {
        lkg_set_error("lkg_check_grouped_i64: hipMemsetAsync failed");
        return LKG_ERR_HIP;
    }
    if (n == 0) return LKG_OK;
    hipLaunchKernelGGL(check_grouped_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (long)n, rows_per_group, (const long *)h, (const long *)r, (const long *)pos_t, n_bad);
    LKG_CHECK_LAUNCH("lkg_check_grouped_i64");
    return LKG_OK;
}

extern "C" int lkg_group_by_key_i64(int64_t n, int32_t n_keys, const int64_t *keys, int32_t *perm, int32_t *seg,
                                    int32_t *n_bad, void *stream) {
    LKG_REQUIRE(n >= 0 && n < INT32_MAX && n_keys >= 1, "lkg_group_by_key_i64: bad sizes");
    LKG_REQUIRE(n_keys <= 1024, "lkg_group_by_key_i64: at most 1024 distinct keys supported (got %d)", n_keys);
    LKG_REQUIRE(seg && (n == 0 || (keys && perm)), "lkg_group_by_key_i64: null pointer");
    const int lds = (int)sizeof(int) * (n_keys * GB_WAVES + 1);
    // n_keys = 1024 asks for 65 540 bytes, four over the 64 KiB a kernel may take as dynamic LDS unless its limit is raised
    // (the limit belongs to the kernel on ONE device: one flag per device of the process)
    static bool raised_on[64] = {};
    int dev = 0;
    if (lds > 64 * 1024 && (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64)) {
        lkg_set_error("lkg_group_by_key_i64: cannot tell the current device");
        return LKG_ERR_HIP;
    }
    bool &raised = raised_on[dev];
    if (!raised && lds > 64 * 1024) {
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(group_by_key_kernel),
                                hipFuncAttributeMaxDynamicSharedMemorySize, sizeof(int) * (1024 * GB_WAVES + 1)) != hipSuccess) {
            lkg_set_error("lkg_group_by_key_i64: cannot raise the dynamic LDS limit");
            return LKG_ERR_HIP;
        }
        raised = true;
    }
    hipLaunchKernelGGL(group_by_key_kernel, dim3(1), dim3(1024), lds,
                       (hipStream_t)stream, (long)n, n_keys, (const long *)keys, perm, seg, n_bad);
    LKG_CHECK_LAUNCH("lkg_group_by_key_i64");
    return LKG_OK;
}

extern "C" int lkg_gather_rows_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                                   const int32_t *perm, float *dst, int64_t ldd, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && lds >= d && ldd >= d, "lkg_gather_rows_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(src && dst, "lkg_gather_rows_f32: null pointer");
    const dim3 grid((unsigned)((n + 3) / 4));
    const bool vec = d % 4 == 0 && lds % 4 == 0 && ldd % 4 == 0 && lkg_aligned16(src) && lkg_aligned16(dst);
    if (vec)
        hipLaunchKernelGGL((gather_rows_kernel<true>), grid, dim3(256), 0, (hipStream_t)stream, (long)n, d, src,
                           (long)lds, (const long *)idx, perm, dst, (long)ldd);
    else
        hipLaunchKernelGGL((gather_rows_kernel<false>), grid, dim3(256), 0, (hipStream_t)stream, (long)n, d, src,
                           (long)lds, (const long *)idx, perm, dst, (long)ldd);
    LKG_CHECK_LAUNCH("lkg_gather_rows_f32");
    return LKG_OK;
}

extern "C" int lkg_scatter_add_rows_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                                        const int32_t *perm, float *dst, int64_t ldd, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && lds >= d && ldd >= d, "lkg_scatter_add_rows_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(src && dst, "lkg_scatter_add_rows_f32: null pointer");
    hipLaunchKernelGGL(scatter_add_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (long)n, d, src, (long)lds, (const long *)idx, perm, dst, (long)ldd);
    LKG_CHECK_LAUNCH("lkg_scatter_add_rows_f32");
    return LKG_OK;
}

extern "C" int lkg_fill_rows_f32(int64_t n, int32_t d, const int64_t *idx, float *dst, int64_t ldd, float value,
                                 uint8_t *flags, int32_t flag, void *stream) {
    LKG_REQUIRE(n >= 0 && d >= 0 && (!dst || (d > 0 && ldd >= d)), "lkg_fill_rows_f32: bad sizes");
    if (n == 0 || (!dst && !flags)) return LKG_OK;
    LKG_REQUIRE(idx, "lkg_fill_rows_f32: null row list");
    hipLaunchKernelGGL(fill_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (long)n, d,
                       (const long *)idx, dst, (long)ldd, value, flags, (unsigned char)(flag != 0));
    LKG_CHECK_LAUNCH("lkg_fill_rows_f32");
    return LKG_OK;
}

extern "C" int lkg_gather_rows_range_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                                         int64_t row_lo, int64_t row_hi, float *dst, int64_t ldd, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && lds >= d && ldd >= d && row_lo <= row_hi, "lkg_gather_rows_range_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(idx && dst && (src || row_lo == row_hi), "lkg_gather_rows_range_f32: null pointer");
    hipLaunchKernelGGL(gather_rows_range_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (long)n, d, src, (long)lds, (const long *)idx, (long)row_lo, (long)row_hi, dst, (long)ldd);
    LKG_CHECK_LAUNCH("lkg_gather_rows_range_f32");
    return LKG_OK;
}

extern "C" int lkg_scatter_add_rows_range_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                                              int64_t row_lo, int64_t row_hi, float *dst, int64_t ldd, void *stream) {
    LKG_REQUIRE(n >= 0 && d > 0 && lds >= d && ldd >= d && row_lo <= row_hi,
                "lkg_scatter_add_rows_range_f32: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(idx && src && (dst || row_lo == row_hi), "lkg_scatter_add_rows_range_f32: null pointer");
    hipLaunchKernelGGL(scatter_add_rows_range_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream,
                       (long)n, d, src, (long)lds, (const long *)idx, (long)row_lo, (long)row_hi, dst, (long)ldd);
    LKG_CHECK_LAUNCH("lkg_scatter_add_rows_range_f32");
    return LKG_OK;
}

extern "C" int lkg_gather_i64(int64_t n, const int64_t *src, const int32_t *perm, int64_t *dst, void *stream) {
    LKG_REQUIRE(n >= 0, "lkg_gather_i64: negative n");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(src && perm && dst, "lkg_gather_i64: null pointer");
    const int64_t blocks = std::min<int64_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(gather_i64_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (long)n,
                       (const long *)src, perm, (long *)dst);
    LKG_CHECK_LAUNCH("lkg_gather_i64");
    return LKG_OK;
}

// ---------------------------------------------------------------------------------------------------
// f2  device-side batch / negative sampler.  Semantics of DataLoader.generate_kg_batch
// (dataloader.py:249-330) on the sorted KG structure instead of Python dicts:
//   per sampled head: ONE positive triple drawn uniformly from the head's triples; neg_rate negative tails
//   drawn uniformly from `training_tails` (= the tail of a uniformly drawn triple, i.e. proportional to
//   in-degree), rejecting a candidate when (candidate, relation) is a positive of the head or when it
//   already is one of this head's negatives; h / r / t+ repeated neg_rate times (generate_batch_by_neg_rate).
// The reference re-draws forever; here a candidate is accepted after MAX_TRIES rejections (cannot happen on
// graphs with more than neg_rate + out-degree distinct tails).
namespace {

struct Draw {   // counter-based stream: value i of stream (seed, group)
    unsigned long long key;
    unsigned ctr;
    __device__ unsigned long long next() { return mix64(key + 0x9E3779B97F4A7C15ull * (++ctr)); }
    __device__ long below(long n) { return (long)(next() % (unsigned long long)n); }
};

// (eptr == nullptr: every entry is one raw edge)
__global__ void sample_kg_batch_kernel(long n_groups, int neg_rate, unsigned long long seed,
                                       const long *__restrict__ heads, long n_ent,
                                       const int *__restrict__ rowptr,
                                       const int *__restrict__ col, const int *__restrict__ eptr,
                                       const int *__restrict__ rel, int nnz, int n_raw, long *__restrict__ out_h,
                                       long *__restrict__ out_r, long *__restrict__ out_p, long *__restrict__ out_n) {
    constexpr int MAX_TRIES = 256;
    const long g = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n_groups) return;
    Draw d{mix64(seed ^ (0xD1B54A32D192ED03ull * (unsigned long long)(g + 1))), 0u};
    const long h = heads[g];
    const int j0 = (h >= 0 && h < n_ent) ? rowptr[h] : 0, j1 = (h >= 0 && h < n_ent) ? rowptr[h + 1] : 0;
    const int e0 = eptr ? eptr[j0] : j0, e1 = eptr ? eptr[j1] : j1;
    if (e1 <= e0) {   // a head without triples (the reference's kg_dict[h] raises KeyError): sentinel group, no draw
        for (int k = 0; k < neg_rate; ++k) {
            out_h[g * neg_rate + k] = h;
            out_r[g * neg_rate + k] = out_p[g * neg_rate + k] = out_n[g * neg_rate + k] = -1;
        }
        return;
    }
    // positive: uniform over the head's raw triples
    const int ep = e0 + (int)d.below(e1 - e0);
    const long r = rel[ep];
    const long tp = col[eptr ? known_entry_of_raw(eptr, nnz, ep) : ep];
    long *ng = out_n + g * neg_rate;
    for (int k = 0; k < neg_rate; ++k) {
        long cand = 0;
        for (int tries = 0; tries < MAX_TRIES; ++tries) {
            const int raw = (int)d.below(n_raw);
            cand = col[eptr ? known_entry_of_raw(eptr, nnz, raw) : raw];
            int en;   // is (cand, r) a positive of h?
            bool reject = known_find(col, j0, j1, cand, en) &&
                          known_among(rel, eptr ? eptr[en] : en, eptr ? eptr[en + 1] : en + 1, r);
            for (int q = 0; q < k && !reject; ++q) reject = (ng[q] == cand);
            if (!reject) break;
        }
        ng[k] = cand;
        out_h[g * neg_rate + k] = h;
        out_r[g * neg_rate + k] = r;
        out_p[g * neg_rate + k] = tp;
    }
}
}  // namespace

extern "C" int lkg_sample_kg_batch(int64_t n_groups, int32_t neg_rate, uint64_t seed, const int64_t *heads,
                                   int64_t n_entities, const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                   int64_t nnz, int64_t n_raw, int64_t *out_h, int64_t *out_r, int64_t *out_pos_t,
                                   int64_t *out_neg_t, void *stream) {
    LKG_REQUIRE(n_groups >= 0 && neg_rate >= 1 && n_entities > 0 && nnz > 0 && n_raw >= nnz && n_raw < INT32_MAX,
                "lkg_sample_kg_batch: bad sizes");
    if (n_groups == 0) return LKG_OK;
    LKG_REQUIRE(heads && rowptr && col && rel && out_h && out_r && out_pos_t && out_neg_t,
                "lkg_sample_kg_batch: null pointer");
    hipLaunchKernelGGL(sample_kg_batch_kernel, dim3((unsigned)((n_groups + 127) / 128)), dim3(128), 0,
                       (hipStream_t)stream, (long)n_groups, neg_rate, (unsigned long long)seed, (const long *)heads,
                       (long)n_entities, rowptr, col, eptr, rel, (int)nnz, (int)n_raw, (long *)out_h, (long *)out_r, (long *)out_pos_t,
                       (long *)out_neg_t);
    LKG_CHECK_LAUNCH("lkg_sample_kg_batch");
    return LKG_OK;
}

// lkg_preload(): HIP loads a translation unit's code object on the first use of one of its kernels; asking for a kernel's
// attributes is such a use (no launch).
int lkg_internal_preload_batch() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&group_by_key_kernel)) == hipSuccess ? 0 : 1;
}
