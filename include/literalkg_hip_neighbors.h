/*
 * literalkg_hip_neighbors.h -- neighbour sampling for the batch-pruned training step of the MI355X (gfx950) LiteralKG
 * library, under the conventions of literalkg_hip.h (plain pointers and sizes, the stream as void*, asynchronous, no
 * allocation, 0 on success and a negative lkg_status with lkg_last_error() otherwise).  literalkg_amd/_native.py binds it
 * from its seventh table, NEIGHBOR_PROTOTYPES.
 */
#ifndef LITERALKG_HIP_NEIGHBORS_H
#define LITERALKG_HIP_NEIGHBORS_H

#include "literalkg_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lkg_csr_extract_rows with a fixed fanout (lkg_neighbors.hip; literalkg_amd/pruned.py): of every selected row at most
 * `fanout` stored entries are copied into the compact CSR, chosen by a counter-based draw.  The argument conventions are
 * those of lkg_csr_extract_rows: sel_rows[n_sel] the (sorted) global row ids, (rowptr, col, val) the CSR they are taken
 * from, out_rowptr[n_sel + 1] the CALLER'S exclusive scan of min(d_i, fanout), out_col / out_val the destinations; col
 * keeps the original ids.
 *
 * The draw.  mix64 is splitmix64's finaliser, arithmetic is mod 2^64, G = 0xD1B54A32D192ED03, S = 0x9E3779B97F4A7C15.
 * For row i (its global id) with d stored entries at positions j = 0 .. d - 1 in CSR order:
 *     d <= fanout   every entry is kept, col and val unchanged to the bit (what lkg_csr_extract_rows writes)
 *     d >  fanout   epoch_key = mix64(seed ^ (G * (draw + 1)))
 *                   row_key   = mix64(epoch_key ^ (G * (i + 1)))
 *                   value(j)  = mix64(row_key + S * (j + 1))
 *                   kept: the `fanout` smallest entries under the order (value(j), j), written in ascending j
 *                   rescale != 0: a kept value is val[j] * scale, scale = float32(d) / float32(fanout) -- two conversions
 *                   to nearest even, one float32 division, one rounded product; rescale == 0: the value is copied
 * A row's sample is a function of (seed, draw, i, the row's entries, fanout, rescale) alone: not of the other selected
 * rows, of alignment, of the stream or of the run.  Every output element is stored once with a plain store; there are no
 * atomics on global memory and no workspace.
 *
 * fanout < 1, n_sel < 0 or (with n_sel > 0) a null pointer is LKG_ERR_INVALID_ARG before any launch; n_sel == 0 launches
 * nothing.                                                                                                                */
int lkg_csr_sample_rows(int64_t n_sel, const int64_t *sel_rows, const int32_t *rowptr, const int32_t *col,
                        const float *val, int32_t fanout, uint64_t seed, uint64_t draw, int32_t rescale,
                        const int32_t *out_rowptr, int32_t *out_col, float *out_val, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* LITERALKG_HIP_NEIGHBORS_H */
