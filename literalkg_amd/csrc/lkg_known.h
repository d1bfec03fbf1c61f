// Device-side access to the known triples: the (rowptr, col, eptr, rel) that lkg_csr_build_device produces and KnownTriples
// holds, read by every filtered query, filtered loss and sampler.  A row is an entity; its entries are
// col[rowptr[row] .. rowptr[row + 1]), ascending and unique inside the row.  Entry e stands for every triple
// (row, *, col[e]); its raw edges are eptr[e] .. eptr[e + 1], their relations rel[x] (in any order, duplicates allowed).
//
// Two rules say when entry e is known under a wanted relation:
//   known_under        want < 0 means any relation: known_lookup (top-k, accepted, the pair head's select) and the entry
//                      walks of pair_mlp_prepare_kernel, retrieval_prepare_kernel and softmax_excluded_kernel.
//   known_under_exact  a negative want matches nothing: rank_prepare_kernel (as include/literalkg_hip.h documents it) and
//                      sample_negatives_kernel, which takes "any relation" as a flag of its own.
// relation_order_kernel and relation_loss_fwd_kernel look an entry up (known_find) and then take EVERY relation of it.
// The comparisons are templates on the wanted value's type: int against int or int against long, as a site's arguments come.
#pragma once
#include <hip/hip_runtime.h>

// the first index in [lo, hi) whose col is >= want (hi when there is none)
template <typename T>
__device__ __forceinline__ int known_lower_bound(const int *__restrict__ col, int lo, int hi, T want) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < want) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// does the row [j0, j1) hold an entry whose col is id?  e: that entry (an empty row holds nothing and reads nothing)
template <typename T>
__device__ __forceinline__ bool known_find(const int *__restrict__ col, int j0, int j1, T id, int &e) {
    e = known_lower_bound(col, j0, j1, id);
    return e < j1 && col[e] == id;
}

// keep, or one of the raw edges [x0, x1) carries relation want
template <typename T>
__device__ __forceinline__ bool known_among(const int *__restrict__ rel, int x0, int x1, T want, bool keep = false) {
    for (int x = x0; x < x1 && !keep; ++x) keep = rel[x] == want;
    return keep;
}

template <typename T>
__device__ __forceinline__ bool known_under_exact(const int *__restrict__ eptr, const int *__restrict__ rel, int e, T want) {
    return known_among(rel, eptr[e], eptr[e + 1], want);
}

template <typename T>
__device__ __forceinline__ bool known_under(const int *__restrict__ eptr, const int *__restrict__ rel, int e, T want) {
    return known_among(rel, eptr[e], eptr[e + 1], want, want < 0);
}

// is (row f, relation want, id) a known triple?  known_under's rule, want tested ahead of the entry's raw edges
__device__ __forceinline__ bool known_lookup(const int *__restrict__ rowptr, const int *__restrict__ col,
                                             const int *__restrict__ eptr, const int *__restrict__ rel, long f, int want,
                                             int id) {
    int e;
    return known_find(col, rowptr[f], rowptr[f + 1], id, e) && (want < 0 || known_under_exact(eptr, rel, e, want));
}

// the candidate slot of entity id: map[id] (no map: id itself), -1 outside [0, n_rows); the caller range-checks the slot
template <typename S>
__device__ __forceinline__ S known_slot(const int *__restrict__ map, int id, long n_rows) {
    S slot = -1;
    if (id >= 0 && id < n_rows) slot = map ? map[id] : id;
    return slot;
}

// the entry that holds raw edge k: the last e in [0, nnz) with eptr[e] <= k
__device__ __forceinline__ int known_entry_of_raw(const int *__restrict__ eptr, int nnz, int k) {
    int lo = 0, hi = nnz;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (eptr[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// splitmix64's finaliser: the samplers' counter-based streams (include/literalkg_hip.h)
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// A filter is absent (rowptr null) or complete: the check of every entry point that takes the six filter arguments.
static inline bool known_filter_complete(const void *rowptr, const void *filter_row, const void *filter_key,
                                         const void *col, const void *eptr, const void *rel) {
    return !rowptr || (filter_row && filter_key && col && eptr && rel);
}
