// Neighbour sampling for the batch-pruned step (include/literalkg_hip.h states the contract; pruned.py calls it
// in place of lkg_csr_extract_rows): a selected row keeps at most `fanout` of its stored entries, the ones with the smallest
// (value(j), j) of a counter-based hash of (seed, draw, row id, position).
//
// One wave per selected row, as extract_rows_kernel.  A short row (d <= fanout) is copied.  A long row
//   1. finds the bound T of its kept entries by a radix select over the 64-bit values, most significant byte first: a pass
//      hashes every position again (the values are a function of j alone -- no memory is read), counts the byte of the
//      values that share the decided prefix in a 256-bin histogram of the wave's own in LDS, and walks the bins to the one
//      that holds the fanout-th smallest.  A pass whose bin is kept WHOLE ends the search (the bound is the bin's largest
//      value): random values leave one entry per bin after ceil(log256 d) passes, so a row of 10^5 entries takes 3, not 8.
//   2. hashes the row once more in turns of 64 positions and keeps value < T, and of the entries with value == T the first
//      n_eq in ascending j (equal values: the smaller position wins).  A turn's kept lanes store at the running offset plus
//      the prefix popcount of their ballot, so the row leaves in CSR order -- one plain store per output element.
// LDS atomics only; nothing in global memory is added to, and there is no workspace.
#include "lkg_common.h"
#include "lkg_known.h"

namespace {

typedef unsigned long long u64;

constexpr u64 NS_GROUP = 0xD1B54A32D192ED03ull, NS_STEP = 0x9E3779B97F4A7C15ull;
constexpr int NS_WAVES = 4, NS_BINS = 256;

__device__ __forceinline__ u64 ns_value(u64 row_key, int j) { return mix64(row_key + NS_STEP * ((u64)j + 1ull)); }

// The bound of the f smallest (value, j) among positions [0, d), d > f >= 1: every value < T is kept, and of the values
// == T the first n_eq in ascending j.  hist: the wave's 256 bins.  Called by all 64 lanes of a wave.
__device__ __forceinline__ void ns_select(u64 row_key, int d, int f, unsigned *hist, int lane, u64 &T, int &n_eq) {
    u64 prefix = 0;                       // the bytes decided so far
    unsigned k = (unsigned)f;             // still to take among the values that carry them
    for (int shift = 56; shift >= 0; shift -= 8) {
        const u64 decided = shift == 56 ? 0ull : ~0ull << (shift + 8);
        *reinterpret_cast<uint4 *>(hist + 4 * lane) = make_uint4(0u, 0u, 0u, 0u);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int j = lane; j < d; j += 64) {
            const u64 v = ns_value(row_key, j);
            if ((v & decided) == prefix) atomicAdd(hist + (int)((v >> shift) & 255ull), 1u);
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const uint4 c = *reinterpret_cast<const uint4 *>(hist + 4 * lane);     // lane owns bins 4 lane .. 4 lane + 3
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                 // (read before the next pass clears them)
        const unsigned own = c.x + c.y + c.z + c.w;
        unsigned inc = own;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        const u64 reached = __ballot(inc >= k);          // never empty: the values under the prefix number at least k
        const int at = __ffsll((long long)reached) - 1;
        unsigned rem = k - __shfl(inc - own, at, 64);    // >= 1: its place inside the lane's four bins
        const unsigned b0 = __shfl(c.x, at, 64), b1 = __shfl(c.y, at, 64), b2 = __shfl(c.z, at, 64),
                       b3 = __shfl(c.w, at, 64);
        int digit = 0;
        unsigned cnt = b0;
        if (rem > cnt) { rem -= cnt; digit = 1; cnt = b1; }
        if (digit == 1 && rem > cnt) { rem -= cnt; digit = 2; cnt = b2; }
        if (digit == 2 && rem > cnt) { rem -= cnt; digit = 3; cnt = b3; }
        prefix |= (u64)(4 * at + digit) << shift;
        k = rem;
        if (k == cnt || shift == 0) {      // the bin is kept whole (or every byte is decided: the values left are equal)
            T = prefix | ((1ull << shift) - 1ull);
            n_eq = (int)k;
            return;
        }
    }
}

__global__ __launch_bounds__(NS_WAVES * 64) void sample_rows_kernel(long n_sel, const long *__restrict__ sel,
                                                                     const int *__restrict__ rowptr,
                                                                     const int *__restrict__ col,
                                                                     const float *__restrict__ val, int fanout, u64 epoch_key,
                                                                     int rescale, const int *__restrict__ out_rowptr,
                                                                     int *__restrict__ out_col, float *__restrict__ out_val) {
    __shared__ __attribute__((aligned(16))) unsigned hist[NS_WAVES][NS_BINS];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const long i = (long)blockIdx.x * NS_WAVES + w;
    if (i >= n_sel) return;
    const long row = sel[i];
    const int src = rowptr[row], d = rowptr[row + 1] - src, dst = out_rowptr[i];
    if (d <= fanout) {                                    // a short row: lkg_csr_extract_rows' copy
        for (int j = lane; j < d; j += 64) {
            out_col[dst + j] = col[src + j];
            out_val[dst + j] = val[src + j];
        }
        return;
    }
    const u64 row_key = mix64(epoch_key ^ (NS_GROUP * ((u64)row + 1ull)));
    u64 T;
    int n_eq;
    ns_select(row_key, d, fanout, hist[w], lane, T, n_eq);
    const float scale = __fdiv_rn((float)d, (float)fanout);
    const u64 below = (1ull << lane) - 1ull;
    int written = 0, eq_seen = 0;
    for (int j0 = 0; j0 < d && written < fanout; j0 += 64) {          // (uniform bounds: every ballot meets the whole wave)
        const int j = j0 + lane;
        const bool in = j < d;
        const u64 v = ns_value(row_key, in ? j : 0);
        const bool eq = in && v == T;
        const u64 m_eq = __ballot(eq);
        bool keep = in && (v < T || (eq && eq_seen + __popcll(m_eq & below) < n_eq));
        const u64 m_keep = __ballot(keep);
        const int at = written + __popcll(m_keep & below);
        if (keep && at < fanout) {                                    // (at < fanout by the bound's construction)
            const float x = val[src + j];
            out_col[dst + at] = col[src + j];
            out_val[dst + at] = rescale ? __fmul_rn(x, scale) : x;
        }
        written += __popcll(m_keep);
        eq_seen += __popcll(m_eq);
    }
}

}  // namespace

extern "C" int lkg_csr_sample_rows(int64_t n_sel, const int64_t *sel_rows, const int32_t *rowptr, const int32_t *col,
                                   const float *val, int32_t fanout, uint64_t seed, uint64_t draw, int32_t rescale,
                                   const int32_t *out_rowptr, int32_t *out_col, float *out_val, void *stream) {
    LKG_REQUIRE(n_sel >= 0, "lkg_csr_sample_rows: negative row count");
    LKG_REQUIRE(fanout >= 1, "lkg_csr_sample_rows: fanout %d is not positive", (int)fanout);
    if (n_sel == 0) return LKG_OK;
    LKG_REQUIRE(sel_rows && rowptr && col && val && out_rowptr && out_col && out_val, "lkg_csr_sample_rows: null pointer");
    LKG_REQUIRE((n_sel + NS_WAVES - 1) / NS_WAVES <= 0x7fffffffLL, "lkg_csr_sample_rows: %lld rows are too many",
                (long long)n_sel);
    // mix64 on the host: the one key every row of the launch shares
    u64 z = (u64)seed ^ (NS_GROUP * ((u64)draw + 1ull));
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    const u64 epoch_key = z ^ (z >> 31);
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)((n_sel + NS_WAVES - 1) / NS_WAVES)), dim3(NS_WAVES * 64), 0,
                       (hipStream_t)stream, (long)n_sel, (const long *)sel_rows, rowptr, col, val, (int)fanout, epoch_key,
                       (int)(rescale != 0), out_rowptr, out_col, out_val);
    LKG_CHECK_LAUNCH("lkg_csr_sample_rows");
    return LKG_OK;
}

// lkg_preload(): HIP loads a translation unit's code object on the first use of one of its kernels; asking for a kernel's
// attributes is such a use (no launch).
int lkg_internal_preload_neighbors() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sample_rows_kernel)) == hipSuccess ? 0 : 1;
}
