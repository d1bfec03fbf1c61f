// What the all-entity training losses share (lkg_softmax.hip: 1-vs-all and its filtered form; lkg_kvsall.hip: KvsAll): the
// per-row walk through a sorted list of candidate positions -- the exclusion list of a filtered softmax row, the positives
// of a KvsAll row -- and the host-side checks of the temperature.  The tile arithmetic is lkg_rank_common.h's.
#pragma once
#include "lkg_known.h"
#include "lkg_rank_common.h"

#include <climits>

// the tile of every kernel of the two files (and what lkg_softmax_all_splits, which both use, divides by)
constexpr int AE_THREADS = 256;
constexpr int AE_ROWS = 64;           // queries per workgroup
constexpr int AE_COLS = 256;          // candidates per tile (64 per wave)

// A row's walk through its list: entries [cur, end) of col are still ahead, next = col[cur] (INT_MAX when none is left:
// positions are < n_c < INT32_MAX).  ptr is clamped into [0, m_total], so a bad list cannot be read past.
struct ListCursor {
    int cur, end, next;
};

// the list of query `row` (empty past n_q) from its first entry >= first (binary search).  ptr is read for every
// row < n_q: a caller whose lists may be absent hands in n_q = 0 with them.
__device__ __forceinline__ ListCursor list_seek(const int *__restrict__ ptr, const int *__restrict__ col, int m_total,
                                                long row, long n_q, long first) {
    ListCursor x{0, 0, INT_MAX};
    if (row < n_q) {
        x.cur = min(max(ptr[row], 0), m_total);
        x.end = min(max(ptr[row + 1], x.cur), m_total);
    }
    x.cur = known_lower_bound(col, x.cur, x.end, first);
    if (x.cur < x.end) x.next = col[x.cur];
    return x;
}

// bit b set: position c0 + b is in the list; the cursor moves past every entry below c0 + 64
__device__ __forceinline__ unsigned long long list_tile_mask(ListCursor &x, const int *__restrict__ col, long c0) {
    unsigned long long mk = 0ull;
    while ((long)x.next < c0 + 64) {
        if ((long)x.next >= c0) mk |= 1ull << ((long)x.next - c0);
        ++x.cur;
        x.next = x.cur < x.end ? col[x.cur] : INT_MAX;
    }
    return mk;
}

// The wave's masks of one tile: lane = row computes its row's, the wave leaves them in sm (its own 64 words) when any is
// non-zero.  Returns that wave-uniform "any".  LDS operations of one wave complete in order, so the rows' readers need no
// workgroup barrier; the wave barriers keep the compiler from moving the accesses across each other.
__device__ __forceinline__ bool list_publish(ListCursor &x, const int *__restrict__ col, long c0, unsigned long long *sm,
                                             int lane) {
    const unsigned long long mk = list_tile_mask(x, col, c0);
    const bool any = __ballot(mk != 0ull) != 0ull;
    if (any) {
        __builtin_amdgcn_wave_barrier();            // the previous tile's reads come first
        sm[lane] = mk;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    return any;
}

static inline bool scale_ok(float scale) { return scale > 0.f && scale < __builtin_inff(); }

// -scale * beta: beta = 1 with squared norms (minus the squared distance), 1/2 without (the dot product); exact
static inline float neg_scale_beta(float scale, const float *pn) { return pn ? -scale : -0.5f * scale; }
