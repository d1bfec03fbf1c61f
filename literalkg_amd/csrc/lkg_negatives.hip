// Negative sampling for given positive triples (include/literalkg_hip.h; literalkg_amd/negatives.py): the draw itself,
// the per-relation cardinalities its Bernoulli side choice needs, and the per-triple answer counts of the subsampling
// weights.  Every structure is the known triples of lkg_known.h: rows = heads with their tails (the tail side) and rows =
// tails with their heads (the head side).
#include <algorithm>

#include "lkg_common.h"
#include "lkg_known.h"

namespace {

struct Structure {   // one side of the known triples
    const int *rowptr, *col, *eptr, *rel;
};
// the side's structure by value (pointer selects: a reference to a kernel argument would put it in scratch)
__device__ __forceinline__ Structure pick(bool head, const Structure &by_head, const Structure &by_tail) {
    return Structure{head ? by_tail.rowptr : by_head.rowptr, head ? by_tail.col : by_head.col,
                     head ? by_tail.eptr : by_head.eptr, head ? by_tail.rel : by_head.rel};
}

// One thread per (group, slot).  Counter 0 of the group's stream decides the side, counters 1 + slot * MAX_TRIES + try
// the candidates: a slot's value depends on (seed, group_offset + g, h, r, t, slot) and on nothing else.
__global__ __launch_bounds__(256) void sample_negatives_kernel(
    long n_groups, long n_slots, unsigned long long seed, unsigned long long group_offset, const long *__restrict__ h,
    const long *__restrict__ r, const long *__restrict__ t, long n_ent, long n_rel, int mode, bool filtered,
    bool any_relation, Structure by_head, Structure by_tail, const long *__restrict__ rel_heads,
    const long *__restrict__ rel_tails, const long *__restrict__ tail_pool, long tail_pool_len,
    const long *__restrict__ head_pool, long head_pool_len, long *__restrict__ neg, unsigned char *__restrict__ head_side,
    unsigned char *__restrict__ unfiltered) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n_groups * n_slots) return;
    const long g = idx / n_slots, j = idx - g * n_slots;
    const unsigned long long key = mix64(seed ^ (0xD1B54A32D192ED03ull * (group_offset + (unsigned long long)g + 1ull)));
    const long hg = h[g], rg = r[g], tg = t[g];
    bool head = mode == LKG_CORRUPT_HEAD;
    if (mode == LKG_CORRUPT_BOTH) {
        head = (mix64(key) & 1ull) != 0;
    } else if (mode == LKG_CORRUPT_BERNOULLI) {
        // TransH's tph / (tph + hpt) = Tl_r / (H_r + Tl_r) in integers; a relation nobody knows corrupts the tail
        const bool in_range = rg >= 0 && rg < n_rel;
        const unsigned long long nh = in_range ? (unsigned long long)rel_heads[rg] : 0ull;
        const unsigned long long nt = in_range ? (unsigned long long)rel_tails[rg] : 0ull;
        head = nh + nt != 0 && mix64(key) % (nh + nt) < nt;
    }
    const Structure s = pick(head, by_head, by_tail);
    const long row = head ? tg : hg, truth = head ? hg : tg;
    const long *pool = head ? head_pool : tail_pool;
    const unsigned long long span = (unsigned long long)(pool ? (head ? head_pool_len : tail_pool_len) : n_ent);
    int j0 = 0, j1 = 0;
    if (filtered && row >= 0 && row < n_ent) {   // (an id out of range is refused before the launch: an empty row here)
        j0 = s.rowptr[row];
        j1 = s.rowptr[row + 1];
    }
    long cand = 0;
    bool reject = true;
    const unsigned long long c0 = 1ull + (unsigned long long)j * LKG_SAMPLE_MAX_TRIES;
    for (int i = 0; i < LKG_SAMPLE_MAX_TRIES && reject; ++i) {
        const unsigned long long v = mix64(key + 0x9E3779B97F4A7C15ull * (c0 + (unsigned long long)i));
        cand = pool ? pool[v % span] : (long)(v % span);
        int e;   // known: an entry of the row [j0, j1) (empty unless filtered), alone (any_relation) or under rg
        reject = cand == truth ||
                 (known_find(s.col, j0, j1, cand, e) && (any_relation || known_under_exact(s.eptr, s.rel, e, rg)));
    }
    neg[idx] = cand;
    unfiltered[idx] = reject ? 1 : 0;
    if (j == 0) head_side[g] = head ? 1 : 0;
}

// ---- per-relation cardinalities ----------------------------------------------------------------------------------------
constexpr int CARD_WAVES = 4;
constexpr int CARD_BITMAP_WORDS = LKG_RELATION_MAX / 32;

// hist[r] += the number of rows that have a raw edge of relation r: one wave per row (a hub row's raw edges are walked 64 at
// a time), a bitmap of the row's relations in LDS -- the lane that sets a bit first counts the relation -- and a histogram
// per workgroup, added to the result once.  Integer adds only: the counts do not depend on the order.
__global__ __launch_bounds__(64 * CARD_WAVES) void rows_per_relation_kernel(long n_rows, int n_rel,
                                                                             const int *__restrict__ rowptr,
                                                                             const int *__restrict__ eptr,
                                                                             const int *__restrict__ rel,
                                                                             unsigned long long *__restrict__ out) {
    extern __shared__ unsigned sm[];   // [CARD_WAVES][CARD_BITMAP_WORDS] bitmaps, then [n_rel] counts
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    unsigned *bitmap = sm + w * CARD_BITMAP_WORDS, *hist = sm + CARD_WAVES * CARD_BITMAP_WORDS;
    const int words = (n_rel + 31) / 32;
    for (int i = threadIdx.x; i < CARD_WAVES * CARD_BITMAP_WORDS + n_rel; i += blockDim.x) sm[i] = 0u;
    __syncthreads();
    const long n_waves = (long)gridDim.x * CARD_WAVES;
    for (long row = (long)blockIdx.x * CARD_WAVES + w; row < n_rows; row += n_waves) {
        const int e0 = eptr[rowptr[row]], e1 = eptr[rowptr[row + 1]];
        if (e1 <= e0) continue;
        for (int e = e0 + lane; e < e1; e += 64) {
            const int q = rel[e];
            if (q < 0 || q >= n_rel) continue;
            const unsigned bit = 1u << (q & 31);
            if (!(atomicOr(&bitmap[q >> 5], bit) & bit)) atomicAdd(&hist[q], 1u);
        }
        // the wave's lanes run in step: every bit of this row has been set before the words are cleared for the next
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int i = lane; i < words; i += 64) bitmap[i] = 0u;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n_rel; q += blockDim.x)
        if (hist[q]) atomicAdd(&out[q], (unsigned long long)hist[q]);
}

// hist[r] += the number of (entry, r) with a raw edge of relation r in the entry: one thread per raw edge, which counts
// unless an EARLIER raw edge of its entry has the same relation (a duplicated triple counts once).
__global__ __launch_bounds__(256) void triples_per_relation_kernel(int n_raw, int nnz, int n_rel,
                                                                    const int *__restrict__ eptr,
                                                                    const int *__restrict__ rel,
                                                                    unsigned long long *__restrict__ out) {
    extern __shared__ unsigned sm[];   // [n_rel] counts
    for (int i = threadIdx.x; i < n_rel; i += blockDim.x) sm[i] = 0u;
    __syncthreads();
    for (long k = (long)blockIdx.x * blockDim.x + threadIdx.x; k < n_raw; k += (long)gridDim.x * blockDim.x) {
        const int q = rel[k];
        if (q < 0 || q >= n_rel) continue;
        bool first = true;
        for (int e = eptr[known_entry_of_raw(eptr, nnz, (int)k)]; e < (int)k; ++e) first &= (rel[e] != q);
        if (first) atomicAdd(&sm[q], 1u);
    }
    __syncthreads();
    for (int q = threadIdx.x; q < n_rel; q += blockDim.x)
        if (sm[q]) atomicAdd(&out[q], (unsigned long long)sm[q]);
}

// ---- per-triple answer counts ------------------------------------------------------------------------------------------
// One thread per (triple, side): the entries of its row known under the triple's relation (r < 0: every entry).
__global__ __launch_bounds__(256) void answer_counts_kernel(long n, const long *__restrict__ h, const long *__restrict__ r,
                                                             const long *__restrict__ t, long n_ent, Structure by_head,
                                                             Structure by_tail, long *__restrict__ n_tails,
                                                             long *__restrict__ n_heads) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= 2 * n) return;
    const bool head = idx >= n;
    const long g = head ? idx - n : idx;
    const Structure s = pick(head, by_head, by_tail);
    const long row = head ? t[g] : h[g], rg = r[g];
    long count = 0;
    if (row >= 0 && row < n_ent) {
        const int j0 = s.rowptr[row], j1 = s.rowptr[row + 1];
        if (rg < 0) {
            count = j1 - j0;
        } else {
            for (int j = j0; j < j1; ++j) {   // known_under_exact without its early exit: measured 19 % faster here
                bool found = false;
                for (int e = s.eptr[j]; e < s.eptr[j + 1]; ++e) found |= (s.rel[e] == rg);
                count += found;
            }
        }
    }
    (head ? n_heads : n_tails)[g] = count;
}

}  // namespace

extern "C" int lkg_sample_negatives(int64_t n_groups, int64_t n_slots, uint64_t seed, int64_t group_offset, const int64_t *h,
                                    const int64_t *r, const int64_t *t, int64_t n_entities, int64_t n_relations,
                                    int32_t mode, int32_t filtered, int32_t any_relation, const int32_t *head_rowptr,
                                    const int32_t *head_col, const int32_t *head_eptr, const int32_t *head_rel,
                                    const int32_t *tail_rowptr, const int32_t *tail_col, const int32_t *tail_eptr,
                                    const int32_t *tail_rel, const int64_t *rel_heads, const int64_t *rel_tails,
                                    const int64_t *tail_pool, int64_t tail_pool_len, const int64_t *head_pool,
                                    int64_t head_pool_len, int64_t *neg, uint8_t *head_side, uint8_t *unfiltered,
                                    void *stream) {
    LKG_REQUIRE(n_groups >= 0 && n_slots >= 1 && n_entities >= 1 && n_entities < INT32_MAX && n_relations >= 0 &&
                    group_offset >= 0 && tail_pool_len >= 0 && head_pool_len >= 0 &&
                    n_groups <= ((int64_t)1 << 38) / n_slots,
                "lkg_sample_negatives: bad sizes");
    LKG_REQUIRE(mode >= LKG_CORRUPT_TAIL && mode <= LKG_CORRUPT_BERNOULLI, "lkg_sample_negatives: unknown mode %d", mode);
    LKG_REQUIRE((tail_pool == nullptr || tail_pool_len >= 1) && (head_pool == nullptr || head_pool_len >= 1),
                "lkg_sample_negatives: empty pool");
    if (n_groups == 0) return LKG_OK;
    LKG_REQUIRE(h && r && t && neg && head_side && unfiltered, "lkg_sample_negatives: null pointer");
    const bool tails = mode != LKG_CORRUPT_HEAD, heads = mode != LKG_CORRUPT_TAIL;
    LKG_REQUIRE(!filtered || ((!tails || (head_rowptr && head_col && head_eptr && head_rel)) &&
                              (!heads || (tail_rowptr && tail_col && tail_eptr && tail_rel))),
                "lkg_sample_negatives: null structure of a filtered side");
    LKG_REQUIRE(mode != LKG_CORRUPT_BERNOULLI || (rel_heads && rel_tails), "lkg_sample_negatives: null relation counts");
    const Structure by_head{head_rowptr, head_col, head_eptr, head_rel}, by_tail{tail_rowptr, tail_col, tail_eptr, tail_rel};
    const int64_t total = n_groups * n_slots;
    hipLaunchKernelGGL(sample_negatives_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (long)n_groups, (long)n_slots, (unsigned long long)seed, (unsigned long long)group_offset,
                       (const long *)h, (const long *)r, (const long *)t, (long)n_entities, (long)n_relations, (int)mode,
                       filtered != 0, any_relation != 0, by_head, by_tail, (const long *)rel_heads, (const long *)rel_tails,
                       (const long *)tail_pool, (long)tail_pool_len, (const long *)head_pool, (long)head_pool_len,
                       (long *)neg, head_side, unfiltered);
    LKG_CHECK_LAUNCH("lkg_sample_negatives");
    return LKG_OK;
}

extern "C" int lkg_relation_cardinality(int64_t n_entities, int64_t n_relations, int64_t n_raw, const int32_t *head_rowptr,
                                        const int32_t *head_eptr, const int32_t *head_rel, int64_t head_nnz,
                                        const int32_t *tail_rowptr, const int32_t *tail_eptr, const int32_t *tail_rel,
                                        int64_t *n_triples, int64_t *n_heads, int64_t *n_tails, void *stream) {
    LKG_REQUIRE(n_entities >= 1 && n_entities < INT32_MAX && n_relations >= 0 && n_raw >= 0 && n_raw < INT32_MAX &&
                    head_nnz >= 0 && head_nnz <= n_raw,
                "lkg_relation_cardinality: bad sizes");
    LKG_REQUIRE(n_relations <= LKG_RELATION_MAX, "lkg_relation_cardinality: at most %d relations supported (got %lld)",
                LKG_RELATION_MAX, (long long)n_relations);
    if (n_relations == 0) return LKG_OK;
    LKG_REQUIRE(n_triples && n_heads && n_tails, "lkg_relation_cardinality: null pointer");
    for (int64_t *out : {n_triples, n_heads, n_tails})
        if (hipMemsetAsync(out, 0, sizeof(int64_t) * n_relations, (hipStream_t)stream) != hipSuccess) {
            lkg_set_error("lkg_relation_cardinality: hipMemsetAsync failed");
            return LKG_ERR_HIP;
        }
    if (n_raw == 0) return LKG_OK;
    LKG_REQUIRE(head_rowptr && head_eptr && head_rel && tail_rowptr && tail_eptr && tail_rel && head_nnz >= 1,
                "lkg_relation_cardinality: null pointer");
    const int n_rel = (int)n_relations;
    const unsigned row_blocks = (unsigned)std::min<int64_t>((n_entities + CARD_WAVES - 1) / CARD_WAVES, 4096);
    const size_t row_lds = sizeof(unsigned) * (CARD_WAVES * CARD_BITMAP_WORDS + n_rel);
    hipLaunchKernelGGL(rows_per_relation_kernel, dim3(row_blocks), dim3(64 * CARD_WAVES), row_lds, (hipStream_t)stream,
                       (long)n_entities, n_rel, head_rowptr, head_eptr, head_rel, (unsigned long long *)n_heads);
    hipLaunchKernelGGL(rows_per_relation_kernel, dim3(row_blocks), dim3(64 * CARD_WAVES), row_lds, (hipStream_t)stream,
                       (long)n_entities, n_rel, tail_rowptr, tail_eptr, tail_rel, (unsigned long long *)n_tails);
    const unsigned raw_blocks = (unsigned)std::min<int64_t>((n_raw + 255) / 256, 4096);
    hipLaunchKernelGGL(triples_per_relation_kernel, dim3(raw_blocks), dim3(256), sizeof(unsigned) * n_rel,
                       (hipStream_t)stream, (int)n_raw, (int)head_nnz, n_rel, head_eptr, head_rel,
                       (unsigned long long *)n_triples);
    LKG_CHECK_LAUNCH("lkg_relation_cardinality");
    return LKG_OK;
}

extern "C" int lkg_answer_counts(int64_t n, const int64_t *h, const int64_t *r, const int64_t *t, int64_t n_entities,
                                 const int32_t *head_rowptr, const int32_t *head_eptr, const int32_t *head_rel,
                                 const int32_t *tail_rowptr, const int32_t *tail_eptr, const int32_t *tail_rel,
                                 int64_t *n_tails, int64_t *n_heads, void *stream) {
    LKG_REQUIRE(n >= 0 && n < ((int64_t)1 << 38) && n_entities >= 1 && n_entities < INT32_MAX,
                "lkg_answer_counts: bad sizes");
    if (n == 0) return LKG_OK;
    LKG_REQUIRE(h && r && t && n_tails && n_heads && head_rowptr && head_eptr && head_rel && tail_rowptr && tail_eptr &&
                    tail_rel,
                "lkg_answer_counts: null pointer");
    const Structure by_head{head_rowptr, nullptr, head_eptr, head_rel}, by_tail{tail_rowptr, nullptr, tail_eptr, tail_rel};
    hipLaunchKernelGGL(answer_counts_kernel, dim3((unsigned)((2 * n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (long)n,
                       (const long *)h, (const long *)r, (const long *)t, (long)n_entities, by_head, by_tail, (long *)n_tails,
                       (long *)n_heads);
    LKG_CHECK_LAUNCH("lkg_answer_counts");
    return LKG_OK;
}

int lkg_internal_preload_negatives() {
    hipFuncAttributes attr;
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void *>(&sample_negatives_kernel)) == hipSuccess ? 0 : 1;
}
