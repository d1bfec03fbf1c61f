/*
 * literalkg_hip_sample.h -- negative sampling for given positive triples of the MI355X (gfx950) LiteralKG library, under
 * the conventions of literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no allocation, 0 on
 * success and a negative lkg_status with lkg_last_error() otherwise).  literalkg_amd/_native.py binds them from its fourth
 * table, SAMPLE_PROTOTYPES.
 *
 * The known triples are two structures of lkg_csr_build_device over n_entities rows, int32 (rowptr, col, eptr, rel): "head_*"
 * has rows = heads with their tails (it answers "is (h, r, c) known?", the tail side), "tail_*" rows = tails with their
 * heads ("is (c, r, t) known?", the head side).  n_raw is the number of raw triples either was built from (eptr[nnz]).
 */
#ifndef LITERALKG_HIP_SAMPLE_H
#define LITERALKG_HIP_SAMPLE_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LKG_SAMPLE_MAX_TRIES 64
#define LKG_CORRUPT_TAIL 0
#define LKG_CORRUPT_HEAD 1
#define LKG_CORRUPT_BOTH 2
#define LKG_CORRUPT_BERNOULLI 3

/* lkg_sample_negatives (lkg_negatives.hip; literalkg_amd/negatives.py): for the n_groups positives (h[g], r[g], t[g]) and
 * n_slots >= 1 slots each, neg int64[n_groups * n_slots], head_side uint8[n_groups] and unfiltered uint8[n_groups *
 * n_slots], every element stored once by plain stores.  The draw is counter-based; with mix64 splitmix64's finaliser, all
 * arithmetic mod 2^64 and gid = group_offset + g,
 *     key(seed, gid)      = mix64(seed ^ (0xD1B54A32D192ED03 * (gid + 1)))
 *     value(seed, gid, c) = mix64(key(seed, gid) + 0x9E3779B97F4A7C15 * c).
 * Counter 0 decides the side: LKG_CORRUPT_TAIL never the head, LKG_CORRUPT_HEAD always, LKG_CORRUPT_BOTH iff value % 2 == 1,
 * LKG_CORRUPT_BERNOULLI iff value % (H + Tl) < Tl with H = rel_heads[r[g]], Tl = rel_tails[r[g]] (the distinct heads and
 * tails of the relation, lkg_relation_cardinality; H + Tl == 0, or r[g] outside [0, n_relations): the tail).  Slot j, try i
 * (0 <= i < LKG_SAMPLE_MAX_TRIES) uses counter 1 + j * LKG_SAMPLE_MAX_TRIES + i; its candidate is pool[value % pool_len]
 * of the side's pool (tail_pool / head_pool, entity ids drawn by position), or value % n_entities with a NULL pool.  A
 * candidate is rejected when it equals the truth of the corrupted slot (t[g], or h[g] on the head side) or when filtered != 0
 * and (h[g], r[g], cand) -- head side: (cand, r[g], t[g]) -- is known; any_relation != 0: known under any relation.  The
 * first candidate that passes is stored; after LKG_SAMPLE_MAX_TRIES rejections the last candidate is stored with its
 * unfiltered flag set.  A candidate equal to the anchor entity and duplicates inside a group are NOT rejected: a slot
 * depends on (seed, gid, h, r, t, j) alone.  One thread per (group, slot); no atomics.  Only the structures of a side that
 * can be corrupted are read, and only with filtered != 0; an h / t outside [0, n_entities) reads no row (callers refuse
 * such ids before the launch).  n_groups == 0 launches nothing; n_groups * n_slots <= 2^38.                          */
int lkg_sample_negatives(int64_t n_groups, int64_t n_slots, uint64_t seed, int64_t group_offset, const int64_t *h,
                         const int64_t *r, const int64_t *t, int64_t n_entities, int64_t n_relations, int32_t mode,
                         int32_t filtered, int32_t any_relation, const int32_t *head_rowptr, const int32_t *head_col,
                         const int32_t *head_eptr, const int32_t *head_rel, const int32_t *tail_rowptr,
                         const int32_t *tail_col, const int32_t *tail_eptr, const int32_t *tail_rel,
                         const int64_t *rel_heads, const int64_t *rel_tails, const int64_t *tail_pool,
                         int64_t tail_pool_len, const int64_t *head_pool, int64_t head_pool_len, int64_t *neg,
                         uint8_t *head_side, uint8_t *unfiltered, void *stream);

/* lkg_relation_cardinality: per relation r of n_relations <= LKG_RELATION_MAX, n_triples[r] = the distinct known (h, r, t),
 * n_heads[r] = the distinct h and n_tails[r] = the distinct t among them, each int64[n_relations] (a duplicated triple
 * counts once; a relation id outside [0, n_relations) nowhere).  head_nnz = the entries of the head structure.  One wave per
 * row with a bitmap of the row's relations in LDS for the heads and the tails, one thread per raw triple for the triples;
 * integer atomics only, so the result does not depend on any order.  The outputs are zeroed on the stream first.    */
int lkg_relation_cardinality(int64_t n_entities, int64_t n_relations, int64_t n_raw, const int32_t *head_rowptr,
                             const int32_t *head_eptr, const int32_t *head_rel, int64_t head_nnz,
                             const int32_t *tail_rowptr, const int32_t *tail_eptr, const int32_t *tail_rel,
                             int64_t *n_triples, int64_t *n_heads, int64_t *n_tails, void *stream);

/* lkg_answer_counts: per triple g of n, n_tails[g] = the distinct known tails of (h[g], r[g], ?) and n_heads[g] = the
 * distinct known heads of (?, r[g], t[g]), int64[n] each, stored once; r[g] < 0: under any relation (the row's entry
 * count).  An h / t outside [0, n_entities) counts 0.  One thread per (triple, side); no atomics.                   */
int lkg_answer_counts(int64_t n, const int64_t *h, const int64_t *r, const int64_t *t, int64_t n_entities,
                      const int32_t *head_rowptr, const int32_t *head_eptr, const int32_t *head_rel,
                      const int32_t *tail_rowptr, const int32_t *tail_eptr, const int32_t *tail_rel, int64_t *n_tails,
                      int64_t *n_heads, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_SAMPLE_H */
