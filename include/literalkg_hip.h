/*
 * literalkg_hip.h -- C ABI of the MI355X (gfx950) LiteralKG hot-path library.
 *
 * The reference (NSLab-CUK/LiteralKG) is pure Python on PyTorch and has NO native
 * boundary of its own.  Its "plugin API" for this path is the
 * nn.Module surface LiteralKG.forward(*input, device=, mode=) (model.py:521-532);
 * literalkg_amd/model.py mirrors that surface and binds the entry points below
 * with ctypes.  Each entry point names the reference lines whose ATen call
 * sequence it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only, no torch types; every device function takes
 *     the hipStream_t to launch on (as void*) and is asynchronous on it;
 *   - no allocation, no host sync inside device functions (graph-capturable);
 *   - return 0 on success, a negative lkg_status otherwise; lkg_last_error()
 *     returns a thread-local message for the last failure on the calling thread;
 *   - all floating point is fp32, entity/column ids in the KG structure are int32,
 *     batch triple ids are int64 (the dtype the reference's DataLoader hands over);
 *   - "ld*" arguments are row strides in ELEMENTS so that callers can address
 *     column slices of a concatenated table without a copy.
 */
#ifndef LITERALKG_HIP_H
#define LITERALKG_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
    LKG_OK = 0,
    LKG_ERR_INVALID_ARG = -1,
    LKG_ERR_HIP = -2,
    LKG_ERR_UNSUPPORTED = -3,
    LKG_ERR_NOMEM = -4
} lkg_status;

/* library version: major*10000 + minor*100 + patch */
int lkg_version(void);
const char *lkg_last_error(void);
/* Load every code object of the library on the CURRENT device now.  HIP loads a translation unit's device code on the first
 * launch of one of its kernels -- tens of milliseconds that would otherwise land inside the first call that needs them (the
 * reference's first mode='update_att', main_pretraining.py:139: a dozen sort / scan kernels of the structure build).  The
 * Python binding calls it once per process, before the first entry point that takes a stream.  No launch, no allocation. */
int lkg_preload(void);

/* ------------------------------------------------------------------ host --
 * KG structure build.  Replaces the per-relation torch.where / cat / stack /
 * sparse_coo_tensor / coalesce sequence of LiteralKG.update_attention
 * (model.py:451-468) and the scipy COO assembly of DataLoader
 * (dataloader.py:449-495): triples are sorted by (head, tail); duplicate
 * (head, tail) pairs under different relations are merged into ONE stored
 * entry (their logits are summed later, as coalesce() does).
 *
 * in : n_entities, n_edges, h/t/r int64[n_edges] (host; r may be NULL -> 0)
 * out: rowptr int32[n_entities+1], col int32[<=n_edges] (tails, ascending per row),
 *      eptr int32[<=n_edges+1] (entry j covers sorted raw edges eptr[j]..eptr[j+1]),
 *      rel int32[n_edges] (relation of each sorted raw edge),
 *      order int64[n_edges] (sorted raw edge k is input edge order[k]),
 *      *nnz_out = number of stored entries.
 * All out buffers are caller-allocated with the upper-bound sizes above.      */
int lkg_csr_build(int64_t n_entities, int64_t n_edges, const int64_t *h, const int64_t *t,
                  const int64_t *r, int32_t *rowptr, int32_t *col, int32_t *eptr, int32_t *rel,
                  int64_t *order, int64_t *nnz_out);

/* CSC of the same pattern, for the backward pass grad_ego = A^T grad_side
 * (autograd of model.py:106).  t_rowptr int32[n_cols+1], t_col int32[nnz]
 * (heads, ascending per tail), t_perm int32[nnz]: transposed entry k is CSR
 * entry t_perm[k].                                                          */
int lkg_csr_transpose(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *rowptr,
                      const int32_t *col, int32_t *t_rowptr, int32_t *t_col, int32_t *t_perm);

/* The same two builds on the DEVICE (lkg_csr_device.hip): h / t / r and every output are device pointers, outputs bit
 * for bit those of lkg_csr_build / lkg_csr_transpose (stable (head, tail) order, ties in input order; heads ascending
 * inside every tail of the CSC).  A hand-written LSD radix sort (8-bit digits) over the key head * n_entities + tail;
 * no allocation: `workspace` holds at least lkg_csr_*_device_workspace(...) bytes.  order is int32[n_edges] here.
 * counts (device int64[2]): counts[0] = number of stored entries, counts[1] = number of triples with an id outside
 * [0, n_entities) or a relation outside int32 (the host build rejects such input; callers must treat counts[1] > 0 as
 * the same error -- the outputs are then unspecified but in bounds).  The caller reads counts after the stream has
 * reached this point (one host sync per edge list) to size col / eptr.                                              */
int64_t lkg_csr_build_device_workspace(int64_t n_entities, int64_t n_edges);
int lkg_csr_build_device(int64_t n_entities, int64_t n_edges, const int64_t *h, const int64_t *t, const int64_t *r,
                         int32_t *rowptr, int32_t *col, int32_t *eptr, int32_t *rel, int32_t *order,
                         int64_t *counts, void *workspace, int64_t workspace_bytes, void *stream);
int64_t lkg_csr_transpose_device_workspace(int64_t n_cols, int64_t nnz);
int lkg_csr_transpose_device(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t *rowptr, const int32_t *col,
                             int32_t *t_rowptr, int32_t *t_col, int32_t *t_perm, void *workspace,
                             int64_t workspace_bytes, void *stream);

/* indices_out int64[2 * nnz] (device) = the [2, nnz] index tensor of the coalesced sparse COO A_in the reference keeps
 * (model.py:462-468, 257-261): row 0 the head of every stored entry, row 1 its tail, in the structure's entry order.   */
int lkg_csr_coo_indices_i64(int64_t n_rows, int64_t nnz, const int32_t *rowptr, const int32_t *col,
                            int64_t *indices_out, void *stream);

/* Cut [0, n_rows) into n_parts contiguous row ranges balanced by stored entries
 * (cuts only at row boundaries so a softmax row never straddles two GPUs,
 * SURVEY.md 8e).  cuts int64[n_parts+1].                                     */
int lkg_row_partition(int64_t n_rows, const int32_t *rowptr, int32_t n_parts, int64_t *cuts);

/* f3  graph ingestion.  Text file of "h r t" lines (single spaces), as
 * DataLoader.load_graph reads with pandas (dataloader.py:186-190).  Two calls: count, then read into
 * caller-sized int64 arrays.  A malformed line is an error (LKG_ERR_INVALID_ARG).              */
int lkg_triples_count(const char *path, int64_t *n_lines);
int lkg_triples_read(const char *path, int64_t capacity, int64_t *h, int64_t *r, int64_t *t,
                     int64_t *n_read);
/* drop_duplicates(keep='first') (dataloader.py:189): keep int64[<=n] lists, in input order, the first
 * occurrence of every distinct (h, r, t).                                                       */
int lkg_triples_dedup(int64_t n, const int64_t *h, const int64_t *r, const int64_t *t, int64_t *keep,
                      int64_t *n_keep);
/* Initial attention values of the loader, A_in = sum_r norm(A_r) (dataloader.py:449-495), written in
 * the entry order of the structure built by lkg_csr_build.  kind 0 = 'random-walk' (D_r^-1 A_r),
 * kind 1 = 'symmetric' (D_r^-1/2 A_r D_r^-1/2 with the ROW sums on both sides, as the reference).
 * All pointers are HOST memory.                                                                 */
int lkg_laplacian_f32(int64_t n_entities, int64_t n_raw, int64_t nnz, const int32_t *rowptr,
                      const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t kind,
                      float *val_out);
/* The same on the DEVICE, over the arrays lkg_csr_build_device left in HBM (all pointers device memory): n_rel = number of
 * relations (max relation id + 1), deg_workspace int32[n_entities * n_rel] scratch.  Same f64 arithmetic as the host form:
 * the values agree bit for bit.                                                                                      */
int lkg_laplacian_device_f32(int64_t n_entities, int64_t nnz, int32_t n_rel, const int32_t *rowptr, const int32_t *col,
                             const int32_t *eptr, const int32_t *rel, int32_t kind, int32_t *deg_workspace,
                             float *val_out, void *stream);

/* ---------------------------------------------------------------- device --
 * K3/K4  neighbour aggregation  out[i,:] = sum_{j in row i} val[j] * x[col[j],:]
 * Replaces torch.matmul(A_in, ego) (model.py:106); called with the CSC arrays
 * it is the backward A^T grad.  Rows without entries are written as zeros.
 * rowptr is int32[n_rows+1] holding offsets into col/val; x has >= max(col)+1 rows -- or is a SHIFTED view
 * (x - offset*ldx) that covers at least every col value stored in the entries rowptr[0]..rowptr[n_rows] of THIS call
 * (a row-range shard that holds only its own rows of x): the kernels never gather through an entry outside that range.
 * Rows without entries come out as exact zeros whatever x holds.  The grid is limited to 2^32 threads.
 * long_rows (nullable, device int32[n_long]): the rows (relative to rowptr) holding more than
 * long_thresh entries; each of them gets a whole workgroup instead of one wave so that a skewed
 * degree distribution does not leave one wave as the tail of the launch.  The list must contain
 * exactly the rows with > long_thresh entries (KGStructure builds it on the host).
 * self (nullable, n_rows x d, stride ld_self): out[i,:] = self[i,:] + sum ... , i.e. the
 * `ego + side` of the gcn / bi-interaction / gin layers (model.py:109, 123, 132) without a second
 * pass; in the backward the same flag adds the incoming gradient (d(ego+side)/d ego = I + A^T).
 * `self` may alias `out` (out += A x).  One kernel launch per call when d <= 128 or d is a multiple of 128
 * (128-column slabs in slab-major workgroup order), else one launch per 128-column slab; rows of at most 32 floats
 * take eight rows per wave.  Deterministic (no atomics): the same inputs give the same bits.          */
int lkg_spmm_csr_f32(int64_t n_rows, int32_t d, const int32_t *rowptr, const int32_t *col,
                     const float *val, const float *x, int64_t ldx, float *out, int64_t ldo,
                     const float *self, int64_t ld_self, const int32_t *long_rows, int32_t n_long,
                     int32_t long_thresh, void *stream);

/* The same with two optional row-wise extras in the epilogue (both nullable), so that an aggregation layer's
 * neighbours in the autograd graph cost no pass of their own:
 *   add2               out[i,:] += add2[i,:]  -- in the backward, the gradient that reaches `ego` through its OTHER use
 *                      (the concatenated table keeps a copy of the layer input, model.py:300-309), which autograd
 *                      would otherwise add in a separate N x D pass; ld_add2 = 0 adds the SAME row to every output
 *                      row: the bias of a gcn layer whose Linear was applied BEFORE the aggregation
 *                      ((ego + A ego) W^T + b = p + A p + b with p = ego W^T, model.py:108-111, when out_dim < in_dim);
 *   add2_rows          (nullable, uint8[n_rows]) add2 is read for the rows whose byte is non-zero only: the loss's
 *                      gradient of the concatenated table touches <= 3B rows (lkg_fill_rows_f32 keeps the flags);
 *   copy_src/copy_dst  copy_dst[i,:] = copy_src[i,:] -- in the forward, that copy itself (the raw entity table into
 *                      column slot 0 of the concatenated table when no gate is configured);
 *   rowmax_out         float[n_rows] (cleared here): max |out[i,:]| -- the row scale the tall GEMM of the layer's
 *                      Linear needs of its input (lkg_gemm_tall_f32), produced while the row is in registers;
 *   x_rows, self_rows  (nullable, uint8 per row of x / of self) a zero byte promises that the row is all zero: its
 *                      entries are skipped without touching x (on the scalar path too: an unflagged row may hold
 *                      anything, it is not read).  The backward of the
 *                      LAST aggregation layer: the loss's gradient reaches <= 3B of the N rows, so all but a fraction
 *                      of a percent of the transpose SpMM's gathers would fetch zeros;
 *   out_rows           (nullable, uint8[n_rows], cleared here; needs x_rows and the 16-byte path, d <= 1024) receives 1
 *                      for every row that got a contribution (a flagged entry, a flagged self / add2 row); the OTHER
 *                      rows of out are not written: out is a table the caller keeps all-zero there.  The set of
 *                      flagged rows is the gradient's next frontier, handed on to the layer below;
 *   rows_with_entries / rows_without_entries
 *                      (both nullable, int32 lists that together hold every row once; not with x_rows / out_rows) for a
 *                      structure whose rows are mostly EMPTY (the reference's data/Small: 766 k entity rows, 84 % never
 *                      a head): one wave per LISTED row with entries, the rows without entries in one streaming pass
 *                      (out = self + add2, copy, row maximum) -- one wave per empty row left the launch bound by the rate
 *                      at which workgroups start.                                                                  */
int lkg_spmm_csr_fused_f32(int64_t n_rows, int32_t d, const int32_t *rowptr, const int32_t *col,
                           const float *val, const float *x, int64_t ldx, float *out, int64_t ldo,
                           const float *self, int64_t ld_self, const float *add2, int64_t ld_add2,
                           const uint8_t *add2_rows, const float *copy_src, int64_t ld_copy_src, float *copy_dst,
                           int64_t ld_copy_dst, float *rowmax_out, const uint8_t *x_rows, const uint8_t *self_rows,
                           uint8_t *out_rows, const int32_t *long_rows, int32_t n_long, int32_t long_thresh,
                           const int32_t *rows_with_entries, int64_t n_rows_with_entries,
                           const int32_t *rows_without_entries, int64_t n_rows_without_entries, void *stream);

/* Batch-pruned step (exact; literalkg_amd/pruned.py): the loss reads <= 3B rows of the last layer, so a
 * layer only needs the rows its consumers read.  lkg_csr_extract_rows copies the entries of the (sorted,
 * int64) rows sel_rows into a compact CSR whose offsets out_rowptr int32[n_sel+1] the caller has already
 * computed (exclusive scan of the row lengths); col keeps the ORIGINAL ids.
 * lkg_spmm_csr_scatter_bwd_f32 is the backward of out = A_sub @ x for such a small sub-CSR without
 * building its transpose every step: g_x[col[j],:] += val[j] * g_out[row,:] (f32 atomics; g_x is
 * zero-initialised by the caller).                                                                */
int lkg_csr_extract_rows(int64_t n_sel, const int64_t *sel_rows, const int32_t *rowptr, const int32_t *col,
                         const float *val, const int32_t *out_rowptr, int32_t *out_col, float *out_val,
                         void *stream);
int lkg_spmm_csr_scatter_bwd_f32(int64_t n_rows, int32_t d, const int32_t *rowptr, const int32_t *col,
                                 const float *val, const float *g_out, int64_t ldg, float *g_x,
                                 int64_t ldx, void *stream);

/* K1+K2  attention refresh, fused: per stored entry
 *     v = sum over its raw edges e of  sum_d ent[t,d] * tanh(ent[h,d] + relemb[rel[e],d])
 * then softmax of v over the stored entries of each head row.
 * Replaces update_attention_batch + coalesce + torch.sparse.softmax(A.cpu(), dim=1)
 * (model.py:430-471).  eptr may be NULL when no (h,t) pair is duplicated
 * (then rel is indexed by entry, and rel_first / dup_* / nnz are ignored).  With eptr: rel_first
 * int32[nnz] holds rel[eptr[j]] per entry; dup_entries int32[n_dup] lists the entries covering more than
 * one raw edge and dup_rows their head rows (relative to row_offset); a pre-pass adds their further
 * relations' terms so that the main kernel's hot loop never chases eptr -> rel; [entry_lo, entry_hi) =
 * rowptr[0] .. rowptr[n_rows] (host-known) is the entry range this call refreshes: only those elements of
 * val_out are cleared and rewritten, the rest is left untouched.  logits_out (nullable) receives the merged
 * pre-softmax logits, val_out the attention values, both float[nnz].
 * row_offset: rowptr holds n_rows+1 offsets for head rows row_offset..row_offset+n_rows
 * (a row-range shard of a larger graph; ent always holds the full table).
 * long_rows / n_long / long_thresh: as for lkg_spmm_csr_f32 (one workgroup per long row).
 * n_rel: the rows of relemb (nn.Embedding(n_relations, relation_dim), model.py:276); every relation id in rel /
 * rel_first is below it (the caller checks).  A table of at most 16 KB is staged in LDS per workgroup;
 * 0 = unknown (the rows are fetched from global memory per entry).  */
int lkg_edge_softmax_f32(int64_t n_rows, int64_t row_offset, int32_t d, const int32_t *rowptr,
                         const int32_t *col, const int32_t *eptr, const int32_t *rel,
                         const int32_t *rel_first, const int32_t *dup_entries,
                         const int32_t *dup_rows, int32_t n_dup, int64_t entry_lo, int64_t entry_hi,
                         const float *ent, int64_t ld_ent, const float *relemb, int64_t ld_rel,
                         float *val_out, float *logits_out, const int32_t *long_rows, int32_t n_long,
                         int32_t long_thresh, int32_t n_rel, void *stream);

/* dst[i] = src[perm[i]] for i < n  (attention values into CSC order after a refresh, or into the entry order of a part
 * of the structure).  n_src = the extent of src: an index outside [0, n_src) is not dereferenced and NaN is stored for it,
 * so an index list that does not belong to src can never make the device read outside src.                       */
int lkg_permute_f32(int64_t n, const int32_t *perm, int64_t n_src, const float *src, float *dst, void *stream);

/* Structure check (a debugging / hardening aid; no counterpart in the reference, whose torch.sparse tensors validate
 * themselves): *bad_out (device int32, cleared here) receives the number of rows of the CSR view rowptr[0 .. n_rows] whose
 * offsets are not 0 <= rowptr[i] <= rowptr[i+1] <= nnz plus the number of entries of that view whose column id minus
 * col_offset lies outside [0, n_cols) -- i.e. 0 exactly when lkg_spmm_csr_f32 over (rowptr, col, val[nnz], x[n_cols rows]
 * handed over with that row offset) stays inside its operands.  literalkg_amd.ops.spmm_raw runs it before every launch
 * when LKG_CHECK_STRUCTURES=1 (the GPU test tier sets it).                                                          */
int lkg_csr_check_i32(int64_t n_rows, const int32_t *rowptr, int64_t nnz, const int32_t *col, int64_t col_offset,
                      int64_t n_cols, int32_t *bad_out, void *stream);

/* K8  TransE-form triple scoring (model_bce.py:329-368; same math baselines.py:33-61)
 *   pos_b = |e_h + r - e_p|^2, neg_b = |e_h + r - e_n|^2,
 *   reg_b = (|e_h|^2 + |r|^2 + |e_p|^2 + |e_n|^2)/2,  rank_b = -logsigmoid(neg_b - pos_b)
 * emb is the N x dim entity-side table (stride ld_emb), relemb the relation table.
 * Outputs are float[batch] each.                                               */
int lkg_transe_score_fwd_f32(int64_t batch, int32_t dim, const float *emb, int64_t ld_emb,
                             const float *relemb, int64_t ld_rel, const int64_t *h,
                             const int64_t *r, const int64_t *pos_t, const int64_t *neg_t,
                             float *pos, float *neg, float *reg, float *rank, void *stream);

/* loss = mean(rank) + lambda * mean(reg); one float written to loss_out.
 * Replaces torch.mean / _L2_loss_mean / add (model.py:8-9, 420-426).           */
int lkg_loss_reduce_f32(int64_t batch, const float *rank, const float *reg, float lambda,
                        float *loss_out, void *stream);

/* Backward of the two calls above.  g_loss is a device pointer to the upstream
 * scalar gradient.  Accumulates (atomic add) into g_emb (N x dim, stride ld_gemb)
 * and g_rel; both must be zero-initialised (or hold gradients to add to).       */
int lkg_transe_score_bwd_f32(int64_t batch, int32_t dim, const float *emb, int64_t ld_emb,
                             const float *relemb, int64_t ld_rel, const int64_t *h,
                             const int64_t *r, const int64_t *pos_t, const int64_t *neg_t,
                             const float *pos, const float *neg, float lambda,
                             const float *g_loss, float *g_emb, int64_t ld_gemb, float *g_rel,
                             int64_t ld_grel, void *stream);

/* K7  TransR projection W_r = gat_trans_M[r] (model.py:372, 390-395) without ever materialising the
 * B x C x D gather: the batch is grouped by relation (stable counting sort), its entity rows are
 * gathered in that order, and ONE grouped MFMA GEMM applies W_r per relation segment.
 *
 * lkg_group_by_key_i64: perm int32[n] lists input positions in key order (stable), seg int32[n_keys+1]
 * the first position of each key.  n_bad (nullable, device int32[1]) receives the number of keys outside
 * [0, n_keys): the reference's gat_trans_M[r] raises IndexError on such a batch, so callers must treat n_bad > 0 as
 * an error (ops.py checks it without a host sync, one call later); the kernel itself groups such a key with the
 * nearest valid one only to keep the launches queued behind it in bounds.                           */
int lkg_group_by_key_i64(int64_t n, int32_t n_keys, const int64_t *keys, int32_t *perm, int32_t *seg,
                         int32_t *n_bad, void *stream);
/* dst[i,:] = src[idx[perm[i]],:]   (idx and/or perm may be NULL = identity)                         */
int lkg_gather_rows_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                        const int32_t *perm, float *dst, int64_t ldd, void *stream);
/* dst[idx[perm[i]],:] += src[i,:]  (f32 atomics; autograd of the row gathers model.py:382-384)     */
int lkg_scatter_add_rows_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                             const int32_t *perm, float *dst, int64_t ldd, void *stream);
/* dst[idx[i],:] = value (dst nullable) and flags[idx[i]] = (flag != 0) (flags nullable, uint8 per table row): marks or
 * resets the <= 3B rows a loss gradient touches in an N-row table that is otherwise kept all-zero between steps, so that
 * no N x C fill runs per step (ops._RowScratch).  Negative ids are skipped (padding of de-duplicated lists).   */
int lkg_fill_rows_f32(int64_t n, int32_t d, const int64_t *idx, float *dst, int64_t ldd, float value, uint8_t *flags,
                      int32_t flag, void *stream);
/* Row-range forms for a table sharded by rows over the ranks of one node (literalkg_amd/distributed.py): this rank
 * holds rows [row_lo, row_hi) and src / dst point at row row_lo.
 *   gather : dst[i,:] = src[idx[i] - row_lo,:] when idx[i] is in the range, else 0 (the rows owned by other ranks are
 *            added by the all-reduce that follows);
 *   scatter: dst[idx[i] - row_lo,:] += src[i,:] for the idx[i] in the range (f32 atomics), the others are skipped.  */
int lkg_gather_rows_range_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                              int64_t row_lo, int64_t row_hi, float *dst, int64_t ldd, void *stream);
int lkg_scatter_add_rows_range_f32(int64_t n, int32_t d, const float *src, int64_t lds, const int64_t *idx,
                                   int64_t row_lo, int64_t row_hi, float *dst, int64_t ldd, void *stream);
/* dst[i] = src[perm[i]] for int64 ids                                                              */
int lkg_gather_i64(int64_t n, const int64_t *src, const int32_t *perm, int64_t *dst, void *stream);

/* f2  device-side batch / negative sampler with the semantics of
 * DataLoader.generate_kg_batch (dataloader.py:249-330): for each of the n_groups heads one positive
 * (relation, tail) drawn uniformly from the head's triples and neg_rate negative tails drawn like
 * random.choice(training_tails), rejecting (tail, relation) positives of the head and repeats inside the
 * group; h / r / pos_t are repeated neg_rate times.  Outputs are int64[n_groups * neg_rate].  A head outside
 * [0, n_entities) or without a triple (kg_dict[h] raises KeyError in the reference) yields a sentinel group:
 * r = pos_t = neg_t = -1, nothing is drawn.  Counter-based RNG: the batch is a pure function of (seed, heads).
 *
 * The stream (all arithmetic on unsigned 64-bit integers, wrapping):
 *   mix(z):  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9;  z = (z ^ (z >> 27)) * 0x94D049BB133111EB;  return z ^ (z >> 31)
 *   group g (0-based position in `heads`) has the key  mix(seed ^ (0xD1B54A32D192ED03 * (g + 1)))  and a counter that
 *   starts at 0; every draw increments the counter first and has the value  mix(key + 0x9E3779B97F4A7C15 * counter);
 *   "a number below n" is  value % n.
 * The raw triples are taken in the structure's sorted order (by head, then tail; lkg_csr_build's `order`), so those of a
 * head are consecutive.  Order of the draws of a group: FIRST the positive -- a number below the head's triple count picks
 * the head's triple at that offset (its relation and tail) -- THEN the candidates, one draw each: a number below n_raw
 * picks a raw triple, whose tail is the candidate.  A candidate is rejected when (head, candidate, the positive's
 * relation) is a triple or when it equals an earlier negative of the group; the next draw replaces it.  The 256th
 * candidate of one negative is kept whether or not it would be rejected (the reference would draw for ever: this happens
 * only when the head's triples and the group's negatives leave fewer free tails than neg_rate).  Negatives are drawn
 * one after the other, k = 0 .. neg_rate - 1, from the same stream.  */
int lkg_sample_kg_batch(int64_t n_groups, int32_t neg_rate, uint64_t seed, const int64_t *heads,
                        int64_t n_entities, const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                        int64_t nnz, int64_t n_raw, int64_t *out_h, int64_t *out_r, int64_t *out_pos_t,
                        int64_t *out_neg_t, void *stream);

/* Grouped fp32 MFMA GEMM over segments seg[g]..seg[g+1] (device int32[n_groups+1], no host sync):
 *  mode 1 (rows): C[seg rows,:] = alpha * A[seg rows,:] opB(B + (g % b_period)*stride_b) + beta*C   (A row-major)
 *                 max_seg_len bounds the longest segment (e.g. the batch size); b_period (0: = n_groups) lets several
 *                 row ranges share a B block: the head, positive-tail and negative-tail rows of a TransR batch, each
 *                 sorted by relation, are 3 R groups over the R matrices of gat_trans_M -- one launch.
 *  mode 2 (k)   : (C + g*stride_c)[m,n] = alpha * sum_{k in seg} A[k,m] B[k,n] + beta*C
 *                 (A given transposed, trans_a = 1; B k-major, trans_b = 0): g_W[r] = X_r^T G_r.   */
int lkg_grouped_gemm_f32(int32_t mode, int32_t n_groups, const int32_t *seg, int64_t max_seg_len,
                         int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, float alpha,
                         const float *a, int64_t lda, const float *b, int64_t ldb, int64_t stride_b,
                         int32_t b_period, float beta, float *c, int64_t ldc, int64_t stride_c, void *stream);

/* f1  fine-tuning head (model.py:316-348): dot-product BPR on table rows
 *   pos_b = <e_h, e_p>, neg_b = <e_h, e_n>, reg_b = (|e_h|^2 + |e_p|^2 + |e_n|^2)/2,
 *   rank_b = -logsigmoid(pos_b - neg_b);  loss via lkg_loss_reduce_f32 (lambda = fine_tuning_l2loss_lambda).
 * Backward accumulates (atomic) into g_emb (zero-initialised by the caller).          */
int lkg_dot_score_fwd_f32(int64_t batch, int32_t dim, const float *emb, int64_t ld_emb, const int64_t *h,
                          const int64_t *pos_t, const int64_t *neg_t, float *pos, float *neg, float *reg,
                          float *rank, void *stream);
int lkg_dot_score_bwd_f32(int64_t batch, int32_t dim, const float *emb, int64_t ld_emb, const int64_t *h,
                          const int64_t *pos_t, const int64_t *neg_t, const float *pos, const float *neg,
                          float lambda, const float *g_loss, float *g_emb, int64_t ld_gemb, void *stream);

/* f1  MLP head (model.py:499-519; model_bce.py:255-260, 423-436): y = BatchNorm1d(relu(z)) fused.
 * training != 0: batch statistics (needs n > 1), running_mean / running_var updated with `momentum` (unbiased
 * variance), like nn.BatchNorm1d; training == 0: the running buffers normalise.  save_mean / save_invstd
 * float[d] feed the backward, which writes g_z and OVERWRITES g_gamma / g_beta.                          */
int lkg_relu_batchnorm_fwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, const float *gamma,
                               const float *beta, float eps, int32_t training, float momentum,
                               float *running_mean, float *running_var, float *y, int64_t ldy,
                               float *save_mean, float *save_invstd, void *stream);
int lkg_relu_batchnorm_bwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, const float *gamma,
                               const float *save_mean, const float *save_invstd, int32_t training,
                               const float *g_y, int64_t ldgy, float *g_z, int64_t ldgz, float *g_gamma,
                               float *g_beta, void *stream);

/* Scores on already-projected rows (TransR form, model.py:413-426): same outputs
 * as lkg_transe_score_fwd_f32 but ph/pp/pn are dense matrices.
 * rows_per_group = K >= 1: the batch is batch/K groups of K consecutive rows that share (h, r, t+) -- the layout
 * DataLoader.generate_kg_batch produces (dataloader.py:318-330, each sampled head repeated neg_rate times).  Then
 * ph / pp / r (and g_ph / g_pp in the backward) hold ONE row per group (batch/K rows), pn / g_pn one row per triple:
 * the head and the positive tail are projected once per group instead of K times (2(2+K)/K B C D flops instead of
 * the reference's 6 B C D).  K = 1 is the general batch.  pos / neg / reg / rank are per triple either way.    */
int lkg_dense_score_fwd_f32(int64_t batch, int32_t rows_per_group, int32_t dim, const float *ph, const float *pp,
                            const float *pn, int64_t ld, const float *relemb, int64_t ld_rel,
                            const int64_t *r, float *pos, float *neg, float *reg, float *rank,
                            void *stream);
int lkg_dense_score_bwd_f32(int64_t batch, int32_t rows_per_group, int32_t dim, const float *ph, const float *pp,
                            const float *pn, int64_t ld, const float *relemb, int64_t ld_rel,
                            const int64_t *r, const float *pos, const float *neg, float lambda,
                            const float *g_loss, float *g_ph, float *g_pp, float *g_pn,
                            int64_t ldg, float *g_rel, int64_t ld_grel, void *stream);
/* Helpers of the grouped form.  lkg_check_grouped_i64: *n_bad (device int32) = number of rows that differ from the
 * first row of their group of rows_per_group in h, r or pos_t (0 = the batch has the layout above).
 * lkg_expand_groups_i32: from the key order of the GROUPS (perm / seg of lkg_group_by_key_i64 over one key per group)
 * the row order of the batch: perm_out[p*K + j] = perm[p]*K + j (int32[n_groups*K]), seg_out[s] = seg[s]*K
 * (int32[n_seg]).                                                                                                 */
int lkg_check_grouped_i64(int64_t n, int32_t rows_per_group, const int64_t *h, const int64_t *r,
                          const int64_t *pos_t, int32_t *n_bad, void *stream);
int lkg_expand_groups_i32(int64_t n_groups, int32_t rows_per_group, int32_t n_seg, const int32_t *perm,
                          const int32_t *seg, int32_t *perm_out, int32_t *seg_out, void *stream);

/* Caller-supplied row ids (the batch's h / pos_t / neg_t, model.py:366-372; head / tail ids of the scoring heads,
 * model.py:473-477) before any kernel gathers or scatters through them: out[i] = ids[i] when lo <= ids[i] < hi, else
 * lo (a valid row), and *n_bad (device int32, cleared here) = the number of ids outside the range.  The reference
 * raises IndexError / a device-side assert for such an id (its embedding lookups are bounds-checked by ATen); here
 * the kernels only ever see in-range ids and the host raises once it has read the counter (one call late, no sync
 * inside the step).                                                                                              */
int lkg_sanitize_ids_i64(int64_t n, const int64_t *ids, int64_t lo, int64_t hi, int64_t *out, int32_t *n_bad,
                         void *stream);

/* K5  row-wise epilogue of an aggregation layer (model.py:111, 161, 305):
 *   a   = leaky_relu(z, slope)                    (z = Linear output, n x d)
 *   y   = layer_norm(a) * gamma + beta            (eps)
 *   yn  = y / max(|y|_2, norm_eps)                (nullable: the L2-normalised copy)
 * save_mean / save_rstd float[n] are kept for the backward.
 * drop_p > 0: message dropout (nn.Dropout, model.py:28/161) is applied to y BEFORE the normalised
 *   copy is taken, y *= keep(seed, row*d + col) / (1 - drop_p) with a counter-based mask that the
 *   backward regenerates from the same seed.
 * y may be NULL (with yn given): the last layer's un-normalised output is read by nobody.   */
int lkg_act_layernorm_fwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, float slope,
                              const float *gamma, const float *beta, float eps, float *y,
                              int64_t ldy, float *yn, int64_t ldyn, float norm_eps,
                              float *save_mean, float *save_rstd, float drop_p, uint64_t seed,
                              void *stream);

/* Backward of the epilogue.  y may be NULL when the forward did not keep it (the last layer's output is read by
 * nobody: lkg_act_layernorm_fwd_f32 accepts y == NULL when yn is given); it is then recomputed from z, the saved
 * statistics, gamma, beta and the dropout seed for the rows that need it.  g_y and g_yn (nullable) are the upstream gradients of
 * the two outputs; writes g_z (n x d) and ACCUMULATES g_gamma / g_beta (atomic,
 * zero-initialised by the caller).  g_z_rowmax (nullable, float[n]) receives max |g_z[i,:]|:
 * the row scale of the data-gradient GEMM that consumes g_z (lkg_gemm_tall_f32), for free.
 * g_yn_rows (nullable, uint8[n]): g_yn is known to be zero outside the rows whose byte is non-zero (the loss's
 * row-sparse gradient, lkg_fill_rows_f32) -- those rows skip the g_yn / y reads, and with g_y == NULL the whole
 * row (g_z = 0, no z read either).  sparse_out != 0 (needs g_yn_rows, g_y == NULL, g_z_rowmax == NULL): g_z is a
 * table the caller keeps all-zero outside the flagged rows, so the zero rows are not written either; row_ids
 * (nullable, int64[n_row_ids], with sparse_out) then lists the rows to visit (negative entries = padding): the launch
 * is over the <= 3B rows the loss reaches -- or over the gradient's frontier, when g_y is row-sparse too (its rows
 * must then be in the list; g_y is read for every listed row) -- instead of N.                              */
int lkg_act_layernorm_bwd_f32(int64_t n, int32_t d, const float *z, int64_t ldz, float slope,
                              const float *gamma, const float *beta, const float *y, int64_t ldy,
                              const float *save_mean, const float *save_rstd, const float *g_y,
                              int64_t ldgy, const float *g_yn, int64_t ldgyn, float norm_eps,
                              float *g_z, int64_t ldgz, float *g_gamma, float *g_beta,
                              float drop_p, uint64_t seed, float *g_z_rowmax, const uint8_t *g_yn_rows,
                              int32_t sparse_out, const int64_t *row_ids, int64_t n_row_ids, void *stream);

/* K6  literal-gate blend (gate.py:24-26, 47-49) on the two pre-activations
 *   out = (1 - sigmoid(zpre)) * x + sigmoid(zpre) * tanh(gpre)
 * gpre / zpre already hold the Linear outputs INCLUDING their biases.              */
int lkg_gate_blend_fwd_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *gpre,
                           int64_t ldg, const float *zpre, int64_t ldz, float *out, int64_t ldo,
                           void *stream);
/* activated != 0: gpre / zpre hold tanh(g) / sigmoid(z) (what the fused gate epilogue of lkg_gemm_tall_f32 keeps).
 * g_pre_rowmax (nullable, float[n], cleared here): max over row i of |g_gpre[i,:]| and |g_zpre[i,:]| -- the row scale of
 * the two-panel data-gradient GEMM that consumes them (lkg_gemm_tall_f32), without a pass of its own.               */
int lkg_gate_blend_bwd_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *gpre,
                           int64_t ldg, const float *zpre, int64_t ldz, const float *g_out,
                           int64_t ldgo, float *g_x, int64_t ldgx, float *g_gpre, int64_t ldgg,
                           float *g_zpre, int64_t ldgz, int32_t activated, float *g_pre_rowmax, void *stream);

/* lkg_gate_blend_bwd_f32 (activated form) with the column statistics of what it reads and writes riding along, so that
 * the bias and weight gradients that follow need no pass of their own over [g_gpre | g_zpre] (2 d wide) and x:
 *   stats[0, 2d)         column sums of [g_gpre | g_zpre]        = the bias gradients of g and gate_* (gate.py:24-25)
 *   stats[2d, 4d)        column maxima |.| of [g_gpre | g_zpre]  }  the column scales of lkg_gemm_wgrad_f32
 *   stats[4d, 5d)        column maxima |.| of x                  }
 *   stats[5d + j 2d, ..) sum_r [g_gpre | g_zpre][r, :] * w[r, j] = the weight gradient of a NARROW literal panel w
 *                        (n_w <= 4 columns, nullable: the numeric literals, gate.py:23)
 * d a multiple of 4, <= 1024, 16-byte aligned operands.  workspace: 1024 (5 + 2 n_w) d floats (per-workgroup partial
 * vectors folded by a second tiny launch: no float atomics, the statistics are deterministic).                   */
int lkg_gate_blend_bwd_stats_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *gpre, int64_t ldg,
                                 const float *zpre, int64_t ldz, const float *g_out, int64_t ldgo, float *g_x,
                                 int64_t ldgx, float *g_gpre, int64_t ldgg, float *g_zpre, int64_t ldgz,
                                 int32_t activated, float *g_pre_rowmax, const float *w, int64_t ldw, int32_t n_w,
                                 float *workspace, int64_t workspace_floats, float *stats, void *stream);

/* Weight-gradient product on the fp16 matrix cores (lkg_gemm_wgrad.hip):  C[m, n] = sum over the k rows of
 * A[k, m] * B[k, n]  (both operands k-major: dW = dY^T X of nn.Linear with k = rows, model.py:93-149, gate.py:22-25),
 * f32 in / f32 out, C overwritten.  a_colmax / b_colmax (device float[m] / float[n]): max |A[:, j]| / max |B[:, j]| --
 * every column is scaled by the power of two that brings its maximum to [2^13, 2^14), split exactly into two fp16
 * halves and multiplied with three fp16 MFMAs per product (f32-accurate normwise; lkg_gemm_f32 uses six bf16 MFMAs and
 * needs no scales).  A bound that is too small by more than a factor 4 can overflow fp16: pass true maxima (emitted by
 * the operand's producer -- lkg_gate_blend_bwd_f32, lkg_row_absmax_f32 -- or lkg_col_absmax_f32 for constant tables). */
int lkg_gemm_wgrad_f32(int64_t m, int64_t n, int64_t k, const float *a, int64_t lda, const float *a_colmax,
                       const float *b, int64_t ldb, const float *b_colmax, float *c, int64_t ldc, void *stream);
/* The same product without scales ("bf16 x 3", six bf16 MFMAs per product as in lkg_gemm_f32) on a 256 x 128 tile per
 * CU with three tiles of loads in flight and the split hidden behind the MFMAs: the long-k engine of every wide weight
 * gradient of the path.  lkg_gemm_longk_ok tells whether it takes a product (k >= 8192 in whole 16-row tiles, widths and row strides
 * multiples of 4 floats, 16-byte aligned operands); otherwise lkg_gemm_f32(trans_a = 1) serves it.  C is overwritten.  */
int lkg_gemm_longk_ok(int64_t m, int64_t n, int64_t k, const float *a, int64_t lda, const float *b, int64_t ldb);
int lkg_gemm_longk_f32(int64_t m, int64_t n, int64_t k, const float *a, int64_t lda, const float *b, int64_t ldb,
                       float *c, int64_t ldc, void *stream);
/* The same product for a NARROW A (m <= 64: dW = dY^T X of an aggregation layer whose conv_dim is 32 or 64 -- the
 * reference's default stacks eight layers of 32, argument_pretraining.py:54-58): exact f32 FMAs on the VALU over LDS-staged
 * 32-row tiles, every thread an (m / 16) x 4 block of a 64-column chunk of C, slices of k combined by f32 atomics -- the
 * matrix-core engines would spend a 256 x 128 tile on it.  lkg_gemm_smallm_ok: m <= 64, k >= 4096, widths and strides
 * multiples of 4 floats, 16-byte aligned operands.  C is overwritten.                                                  */
int lkg_gemm_smallm_ok(int64_t m, int64_t n, int64_t k, const float *a, int64_t lda, const float *b, int64_t ldb);
int lkg_gemm_smallm_f32(int64_t m, int64_t n, int64_t k, const float *a, int64_t lda, const float *b, int64_t ldb,
                        float *c, int64_t ldc, void *stream);

/* The dense backward of a NARROW aggregation layer in one launch: y = Dropout(LayerNorm(LeakyReLU(x W^T + b))) with its
 * L2-normalised copy yn, 32 columns in and out (the reference's default conv_dim: model.py:108-111, 161, 305 over
 * argument_pretraining.py:54-58).  Replaces, for such a layer, lkg_act_layernorm_bwd_f32 + lkg_gemm_skinny_f32 (g_x = g_z W) +
 * lkg_gemm_smallm_f32 (g_W = g_z^T x) + lkg_colsum_f32 (g_b): g_z stays in LDS, both products run as f32 MFMAs.
 * x, z: the Linear's input and output rows as the forward pass kept them; y: required where g_yn is given; g_y and/or g_yn:
 * the incoming gradients (either may be null); g_yn_rows: optional row flags of g_yn (0 = that row of g_yn is zero).
 * Outputs: g_x [n, 32]; g_w [32 x 32, contiguous], g_bias (may be null), g_gamma, g_beta: OVERWRITTEN with the sums, which are
 * added up in a fixed order (every workgroup's partial sums go through `workspace`, lkg_narrow_layer_bwd_workspace(n) floats).
 * lkg_narrow_layer_bwd_ok: n >= 4096, d_in = d_out = 32, row strides multiples of 4 floats, 16-byte aligned operands. */
int64_t lkg_narrow_layer_bwd_workspace(int64_t n);
int lkg_narrow_layer_bwd_ok(int64_t n, int32_t d_in, int32_t d_out, const float *x, int64_t ldx, const float *z, int64_t ldz,
                            const float *y, int64_t ldy, const float *g_y, int64_t ldgy, const float *g_yn, int64_t ldgyn);
int lkg_narrow_layer_bwd_f32(int64_t n, int32_t d_in, int32_t d_out, const float *x, int64_t ldx, const float *w, int64_t ldw,
                             const float *z, int64_t ldz, float slope, const float *gamma, const float *y, int64_t ldy,
                             const float *save_mean, const float *save_rstd, const float *g_y, int64_t ldgy,
                             const float *g_yn, int64_t ldgyn, float norm_eps, float drop_p, uint64_t seed,
                             const uint8_t *g_yn_rows, float *g_x, int64_t ldgx, float *g_w, float *g_bias,
                             float *g_gamma, float *g_beta, float *workspace, int64_t workspace_floats, void *stream);
/* Skinny products over many rows: C[m, n] = A[m, k] . op(B) (+ bias) (+ beta C) for k, n <= 64 (op(B) = B[k, n], or
 * B[n, k]^T with trans_b: an nn.Linear weight) -- the 32 x 32 Linears, data gradients and residual mixes of narrow aggregation
 * layers (model.py:93-130 at the reference's default conv_dim 32).  Exact f32 FMAs on the VALU at streaming rate: op(B) stays
 * in LDS, 64 rows of A per turn, one row x n / 4 columns per thread.  lkg_gemm_skinny_ok: m >= 4096, k and n <= 64 in
 * multiples of 4, rows of A and C 16-byte aligned.                                                                  */
int lkg_gemm_skinny_ok(int64_t m, int64_t n, int64_t k, const float *a, int64_t lda, const float *c, int64_t ldc);
int lkg_gemm_skinny_f32(int64_t m, int64_t n, int64_t k, const float *a, int64_t lda, const float *b, int64_t ldb,
                        int32_t trans_b, float beta, float *c, int64_t ldc, const float *bias, void *stream);
/* out[c] = max_r |x[r,c]|  (out is overwritten)                                                     */
int lkg_col_absmax_f32(int64_t n, int32_t d, const float *x, int64_t ldx, float *out, void *stream);

/* out[c] = sum_r x[r,c]  (bias gradients of nn.Linear; out is overwritten)                       */
int lkg_colsum_f32(int64_t n, int32_t d, const float *x, int64_t ldx, float *out, void *stream);
/* out_w[c, j] = sum_r x[r,c] * w[r,j] for a NARROW w (1 <= n_w <= 8 columns) and, when out_sum != NULL,
 * out_sum[c] = sum_r x[r,c] in the same pass: the weight gradient of a Linear's narrow input panel (gate.py:22-25: the
 * 2 numeric literals) together with its bias gradient -- one read of x instead of a long-k GEMM that would spend a
 * 128-wide tile on n_w columns, plus a column-sum pass.  Both outputs are overwritten (f32 atomics inside).     */
int lkg_colsum_weighted_f32(int64_t n, int32_t d, const float *x, int64_t ldx, const float *w, int64_t ldw,
                            int32_t n_w, float *out_sum, float *out_w, int64_t ld_out_w, void *stream);

/* bi-interaction's element-wise front (model.py:123-128) fused with the GCNII-style residual's mix (model.py:94):
 *   out_sum = c (ego + side) + alpha h0p,  out_prod = c (ego * side) + alpha h0p,  c = 1 - alpha
 * (h0p NULL: c = 1 and no h0p term: the plain sum and product) in one pass over ego / side / h0p, and its backward
 *   g_ego = c (g_sum + g_prod * side),  g_side = c (g_sum + g_prod * ego),  g_h0p = alpha (g_sum + g_prod)
 * in one pass (g_ego, g_side, g_h0p: dense n x d outputs; g_h0p only with has_h0).  Replaces four element-wise ops of
 * the reference per layer (and eight-plus autograd kernels behind them).                                       */
int lkg_bi_mix_fwd_f32(int64_t n, int32_t d, const float *ego, int64_t lde, const float *side, int64_t lds,
                       const float *h0p, int64_t ldh, float alpha, float *out_sum, int64_t ldos, float *out_prod,
                       int64_t ldop, void *stream);
int lkg_bi_mix_bwd_f32(int64_t n, int32_t d, const float *ego, int64_t lde, const float *side, int64_t lds,
                       const float *g_sum, int64_t ldgs, const float *g_prod, int64_t ldgp, int32_t has_h0, float alpha,
                       float *g_ego, float *g_side, float *g_h0p, void *stream);

/* Small element-wise steps of the layers (row-major n x d, row strides in elements):
 *   op 0  out = alpha * a + beta * b   (b NULL: alpha * a + beta)   GCNII residual mix, model.py:94-96; 'gin' sums
 *   op 1  out = a * b                                                ego * side of 'bi-interaction', model.py:127
 *   op 2  out = leaky(a, alpha) + leaky(b, alpha)  (b NULL: one term) model.py:125-130, 310
 *   op 3  out = a * (b > 0 ? 1 : alpha)                              LeakyReLU backward (a gradient, b pre-activation) */
int lkg_eltwise_f32(int32_t op, int64_t n, int32_t d, const float *a, int64_t lda, const float *b,
                    int64_t ldb, float alpha, float beta, float *out, int64_t ldo, void *stream);

/* f4  one fused Adam step over a dense contiguous tensor (the reference runs dense torch.optim.Adam over
 * the N x D entity table every step, main_pretraining.py:47,119): torch.optim.Adam's arithmetic,
 * `step` is the 1-based step count used for the bias corrections; weight_decay is the L2 form.          */
int lkg_adam_step_f32(int64_t n, float *param, const float *grad, float *exp_avg, float *exp_avg_sq,
                      float lr, float beta1, float beta2, float eps, float weight_decay, int64_t step,
                      void *stream);

/* Dense fp32 GEMM on the matrix cores, row-major, f32 in / f32 out / f32 accumulation:
 *   C[m,n] = alpha * sum_k opA(A)[m,k] * opB(B)[k,n] + beta * C[m,n] (+ bias[n])
 * Engines (chosen from the shape, results agree to f32 rounding): the f32-input MFMA (v_mfma_f32_32x32x2_f32), and two
 * "bf16 x 3" engines that form the f32 product from six v_mfma_f32_32x32x16_bf16 over an exact three-way bf16 split
 * of every operand (A row-major with m >= 16384 and a small B -- Linear forward / data gradient; trans_a = 1,
 * trans_b = 0 with k >= 2048 -- weight gradients).  The first needs lkg_gemm_workspace(trans_a, m, n, k) bytes of
 * caller-provided device workspace for B's planes (0 = the engine does not apply to this shape); without it (NULL or
 * too small) the product runs on the f32-input MFMA.  No allocation inside.
 * LKG_GEMM_F32_ONLY=1 in the environment (read at the first call) keeps every product on the f32-input MFMA.
 * trans_a / trans_b: 0 = stored as written, 1 = stored transposed (A is k x m / B is n x k).
 * Used for nn.Linear forward (trans_b = 1), its data gradient and its weight
 * gradient (model.py:111 etc., gate.py:24-25, linear_gat model.py:309).          */
int64_t lkg_gemm_workspace(int32_t trans_a, int64_t m, int64_t n, int64_t k);
/* The engine lkg_gemm_f32 runs this product on, given workspace_bytes of workspace (the choice lkg_gemm_f32 itself makes):
 * 0 = the f32-input MFMA (a k-ordered chain), 1 = bf16 x 3 with A row-major, 2 = bf16 x 3 with both operands k-major. */
int lkg_gemm_f32_engine(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, int64_t workspace_bytes);

/* C[m,n] = opA(A)[m,k] opB(B)[k,n] with float64 accumulation, rounded to float32 once; SMALL products only (m n <= 2^24,
 * m n k <= 2^34).  The GCNII-style residual's weight fold W_lin (W')^T of the device path (model.py:95-98 evaluates
 * Linear(mixed @ W'); the device multiplies the two small matrices first and runs ONE N-row product): W' has near-equal
 * entries, and an fp32 fold's accumulated rounding is what ill-conditioned residual configurations' scores then see.   */
int lkg_gemm_f64acc_f32(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, const float *a, int64_t lda,
                        const float *b, int64_t ldb, float *c, int64_t ldc, void *stream);
int lkg_gemm_f32(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, float alpha,
                 const float *a, int64_t lda, const float *b, int64_t ldb, float beta, float *c,
                 int64_t ldc, const float *bias, void *workspace, int64_t workspace_bytes, void *stream);

/* Tall GEMM of the layers' dense part (lkg_gemm_tall.hip): m rows (entities), n <= a few hundred output columns,
 *   C[m, n] = epilogue( sum over K-panels p of  A_p[m, ka[p]] . B_p[n, ka[p]]^T )            f32 in, f32 out.
 * Arithmetic "f16 x 2": rows of A and of B are scaled by powers of two, every element split exactly into two fp16
 * (11 + 11 significant bits), three v_mfma_f32_32x32x16_f16 per 16 k into a main and a correction accumulator (f32),
 * unscaled exactly in the epilogue: within ~2x of an f32 GEMM's rounding error against f64, at 3/8 of the f32 MFMA's
 * instruction count on a 16x faster pipe.
 *   a / lda / ka       host arrays of n_panels (1..3) device pointers / row strides / widths: A's K-panels, possibly
 *                      from different arrays (nn.Linear over a concatenated input WITHOUT the concatenation:
 *                      gate.py:23 [x | num | txt], model.py:116 [ego | side]); any alignment, any width -- but a panel
 *                      must span one 16-byte window, (m - 1) lda[p] + ka[p] >= 4 floats (a single row narrower than 4,
 *                      two rows of one): the kernel loads whole windows clamped to the panel's last one, and a
 *                      shorter panel is LKG_ERR_INVALID_ARG before any launch;
 *   a_rowmax           device float[m]: max_k |A[i, k]| over all panels (lkg_row_absmax_f32; accumulate = 1 folds a
 *                      further panel in).  It only has to BOUND the row (a stale larger value costs precision, a
 *                      smaller one overflows fp16): callers cache it for constant panels;
 *   b / ldb            host arrays of n_groups * n_panels device pointers: block (group, panel) of B.  trans_b = 1:
 *                      stored [rows][ka[p]] (an nn.Linear weight or a column slice of one), 0: stored [ka[p]][rows]
 *                      (the data gradient  gy . W).  n_groups = 1: rows = n.  Epilogue 1 (gate): n_groups = 2 row
 *                      groups of n / 2 (the g and the z projection of gate.py:22-25), bias = [b_g | b_z], and
 *                      C[m, n/2] = (1 - sigmoid(z)) gate_x + sigmoid(z) tanh(g)   (gate.py:26; gate_x IS the first K-panel, a[0] --
 *                      its values are kept on chip while they pass through the staging registers) with tanh(g) / sigmoid(z)
 *                      optionally kept in gate_g / gate_z for lkg_gate_blend_bwd_f32(activated = 1);
 *   epilogue 0         C = alpha * product + beta * C + bias[n];
 *   epilogue bits 8-15 the tiling, chosen per call: 0 = the library's default ("256x1"), else 1 + {0 "256x2" (two
 *                      accumulators, 128 x 256 tiles), 1 "128x1" (one accumulator, 128 x 128 tiles), 2 "256x1" (one
 *                      accumulator, 128 x 256 tiles)}: tests and tools run them side by side; nothing in the environment
 *                      or the build selects code.  Any other value (4..6 named tilings that were removed) is an error;
 *   workspace          >= lkg_gemm_tall_workspace(n, n_panels, ka, epilogue) bytes (B's fp16 planes: no allocation here;
 *                      -1 for bad sizes or an unknown tiling). */
int lkg_row_absmax_f32(int64_t n, int32_t d, const float *x, int64_t ldx, float *out, int32_t accumulate,
                       void *stream);
int64_t lkg_gemm_tall_workspace(int32_t n, int32_t n_panels, const int32_t *ka, int32_t epilogue);
int lkg_gemm_tall_f32(int64_t m, int32_t n, int32_t n_panels, const float *const *a, const int64_t *lda,
                      const int32_t *ka, const float *a_rowmax, int32_t n_groups, const float *const *b,
                      const int64_t *ldb, int32_t trans_b, float alpha, float beta, float *c, int64_t ldc,
                      const float *bias, int32_t epilogue, const float *gate_x, int64_t ld_x, float *gate_g,
                      int64_t ld_g, float *gate_z, int64_t ld_z, void *workspace, int64_t workspace_bytes,
                      void *stream);

/* K5 as surveyed ("fused epilogue around an MFMA GEMM"): an aggregation layer's whole dense part in ONE launch,
 *     z  = sum_p A_p W_p^T + bias                      (nn.Linear over a column-concatenated input, model.py:108-110, 116-123)
 *     y  = Dropout_p(LayerNorm(LeakyReLU_slope(z)))    (model.py:111, 161; eps, gamma, beta: nn.LayerNorm's)
 *     yn = y / max(|y|_2, norm_eps)                    (F.normalize, model.py:305)
 * for output widths n <= 256 and at most two K-panels: the 128 x 256 tile of the tall GEMM holds whole rows; its epilogue
 * sends them through LDS in slabs of 16 rows, row-major, and runs the row-wise kernel's own arithmetic on them (one wave per
 * row, the same lane <-> column map and reduction tree), so y, yn, mean and rstd are BIT-IDENTICAL to lkg_gemm_tall_f32 (its
 * default tiling) followed by lkg_act_layernorm_fwd_f32 whenever that kernel takes its 16-byte path (n % 4 == 0, aligned
 * rows), and equal to fp32 rounding otherwise.  z is NOT written (nor read back by a second kernel): one HBM pass fewer.
 * y and yn are nullable (not both); save_mean / save_rstd float[m] are what lkg_act_layernorm_bwd_f32 needs beside a
 * recomputed z.  The dropout mask is lkg_act_layernorm_fwd_f32's (same seed, same mask).  Arguments a .. a_rowmax, workspace:
 * as for lkg_gemm_tall_f32 (w: one [n, ka[p]] block per panel, nn.Linear layout).                                         */
int64_t lkg_linear_act_layernorm_workspace(int32_t n, int32_t n_panels, const int32_t *ka);
int lkg_linear_act_layernorm_fwd_f32(int64_t m, int32_t n, int32_t n_panels, const float *const *a, const int64_t *lda,
                                     const int32_t *ka, const float *a_rowmax, const float *const *w, const int64_t *ldw,
                                     const float *bias, float slope, const float *gamma, const float *beta, float eps,
                                     float *y, int64_t ldy, float *yn, int64_t ldyn, float norm_eps, float *save_mean,
                                     float *save_rstd, float drop_p, uint64_t seed, void *workspace,
                                     int64_t workspace_bytes, void *stream);

/* Filtered link-prediction ranking (lkg_rank.hip; literalkg_amd/ranking.py).  Candidates are the n_cand rows of p (f32,
 * row stride ldp, k columns); a query row q_i (row stride ldq) scores candidate c as
 *     s(i, c) = pn[c] - 2 q_i . p_c          (lower is better; pn NULL = 0: dot scoring, s = -2 q.p)
 * the squared distance ||q_i - p_c||^2 less the row constant ||q_i||^2.  The dot product is the exact-f32 MFMA chain
 * (v_mfma_f32_16x16x4_f32, a fixed k order); every score below comes from that same arithmetic, bit for bit.
 *
 * lkg_rank_sqnorm_f32 : out[c] = ||p_c||^2.
 * lkg_rank_queries_f32: q[i,:] = p[ids[i],:] + alpha * e[rel[i],:]   (e nullable: a plain gather; rel nullable: row 0).
 * lkg_rank_prepare_f32: thr[i] = s(i, truth[i]) and, with a filter, better[i] / equal[i] = MINUS the number of filtered
 *     candidates c != truth[i] with s(i, c) < thr[i] / == thr[i] (else 0).  The filter is a structure of
 *     lkg_csr_build_device over n_cand rows (rowptr int32[n_cand+1], col, eptr, rel): query i drops every col[e] of
 *     row filter_row[i] that has a raw edge with relation filter_rel[i].  rowptr NULL = no filter.
 * lkg_rank_count_f32  : better[i] += #{c != truth[i] : s(i, c) < thr[i]}, equal[i] += #{c != truth[i] : s == thr[i]}
 *     (int32 atomics, one per row per workgroup; the n_q x n_cand scores are never stored).  After prepare + count,
 *     better / equal are the filtered counts.  A NaN score counts nowhere.  64-bit addressing throughout.      */
int lkg_rank_sqnorm_f32(int64_t n, int32_t k, const float *p, int64_t ldp, float *out, void *stream);
int lkg_rank_queries_f32(int64_t n, int32_t k, const float *p, int64_t ldp, const int64_t *ids, const float *e,
                         int64_t lde, const int64_t *rel, float alpha, float *q, int64_t ldq, void *stream);
int lkg_rank_prepare_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                         int64_t ldp, const float *pn, const int64_t *truth, const int64_t *filter_row,
                         const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col, const int32_t *eptr,
                         const int32_t *rel, float *thr, int32_t *better, int32_t *equal, void *stream);
int lkg_rank_count_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                       int64_t ldp, const float *pn, const float *thr, const int64_t *truth, int32_t *better,
                       int32_t *equal, void *stream);

/* Filtered top-k link prediction (lkg_topk.hip; literalkg_amd/topk.py).  Queries, candidates and the score s(i, c) as
 * for lkg_rank_* above, with the same arithmetic bit for bit.  For every query i the top_k candidates of smallest
 * (s(i, c), id(c)) -- float comparison, then the entity id id(c) = cand_ids[c] (cand_ids NULL: c), NaN never selected --
 * among those not dropped by the filter: query i drops every candidate whose id is a col of row filter_row[i] of the
 * lkg_csr_build_device structure (rowptr, col, eptr, rel) with a raw edge of relation filter_rel[i] (filter_rel[i] < 0:
 * of any relation).  rowptr NULL = no filter.  The n_q x n_cand scores are never stored.
 *
 * lkg_topk_splits    : the number S of candidate splits for n_q queries (requested in [1, LKG_TOPK_MAX_SPLITS], or 0 =
 *     automatic), clamped to the candidate tiles; 0 for bad arguments.  The result does not depend on S.
 * lkg_topk_select_f32: per split, each query's best top_k of that split's candidates, sorted, padded with
 *     (+inf, INT32_MAX), into ws_s / ws_i [S][n_q][top_k] (splits = lkg_topk_splits(n_q, n_cand, splits)).
 * lkg_topk_merge_f32 : out_ids[i, j] / out_scores[i, j] = the j-th best id / s over the S lists; out_values[i, j] =
 *     qn[i] + s (qn non-NULL: the squared distance, qn = ||q_i||^2) or -s / 2 (the dot product).  Fewer than top_k
 *     eligible candidates: ids -1, scores and values NaN past them.  top_k in [1, LKG_TOPK_MAX].                */
#define LKG_TOPK_MAX 128
#define LKG_TOPK_MAX_SPLITS 64
int32_t lkg_topk_splits(int64_t n_q, int64_t n_cand, int32_t requested);
int lkg_topk_select_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                        int64_t ldp, const float *pn, const int64_t *cand_ids, const int64_t *filter_row,
                        const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col, const int32_t *eptr,
                        const int32_t *rel, int32_t top_k, int32_t splits, float *ws_s, int32_t *ws_i, void *stream);
int lkg_topk_merge_f32(int64_t n_q, int32_t top_k, int32_t splits, const float *ws_s, const int32_t *ws_i,
                       const float *qn, int64_t *out_ids, float *out_scores, float *out_values, void *stream);

/* Threshold retrieval (lkg_accept.hip, lkg_csr_device.hip; literalkg_amd/accepted.py).  Queries, candidates, cand_ids, the
 * filter and the kernel score s(i, c) as for lkg_topk_select_f32, bit for bit.  The reported score is v(i, c) = qn[i] + s
 * (pn and qn given: the squared distance, qn = lkg_rank_sqnorm_f32 of the queries) or -s / 2 (pn and qn NULL: the dot
 * product) -- what lkg_topk_merge_f32 returns as `values`.  Candidate c of query i is ACCEPTED iff v(i, c) <= thr[i]
 * (higher != 0: v(i, c) >= thr[i]) in one f32 compare -- a NaN score never is -- and the filter does not drop it.
 * splits in [0, LKG_TOPK_MAX_SPLITS] (0 = automatic, as lkg_topk_splits chooses) is the number of candidate splits per 64
 * queries; no result depends on it.  n_q, n_cand <= INT32_MAX - 1; empty inputs launch nothing; addressing is 64-bit.
 *
 * lkg_accept_count_f32: counts[i] += the number of accepted candidates of query i (the caller zeroes counts).  Nothing
 *     of size n_q x n_cand, or of the size of the result, is written.
 * lkg_accept_emit_f32 : every accepted (i, c) is written as (id(c), s, v) at out_*[base[i] + slot], slot taken from
 *     cursor[i] (int32[n_q], zeroed by the caller), in no particular order inside the row.  counts is what
 *     lkg_accept_count_f32 gave for the same arguments and base its exclusive scan; a slot outside [0, counts[i]) is NOT
 *     written and *flag (zeroed by the caller) is set to 1 instead -- the two passes run the same arithmetic, so this
 *     cannot happen, and if it did it would not become a store outside the buffers.
 * lkg_accept_order    : rows of (id, s, v), row i owning the entries rowptr[i] .. rowptr[i + 1] (int64[n_q + 1],
 *     rowptr[n_q] = m), sorted inside every row by ascending s (float comparison: -0.0 == +0.0; no NaN) and then ascending
 *     id, into out_*.  ids lie in [0, id_bound), id_bound <= INT32_MAX; m <= INT32_MAX - 1.  workspace:
 *     lkg_accept_order_workspace(m, n_q) bytes of device memory; the call allocates nothing.  out_* must not alias the
 *     inputs.                                                                                                        */
int lkg_accept_count_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                         int64_t ldp, const float *pn, const float *qn, const float *thr, int32_t higher,
                         const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                         const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                         int32_t splits, int32_t *counts, void *stream);
int lkg_accept_emit_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                        int64_t ldp, const float *pn, const float *qn, const float *thr, int32_t higher,
                        const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                        const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                        int32_t splits, const int32_t *counts, const int64_t *base, int32_t *cursor, int64_t *out_ids,
                        float *out_scores, float *out_values, int32_t *flag, void *stream);
int64_t lkg_accept_order_workspace(int64_t m, int64_t n_q);
int lkg_accept_order(int64_t m, int64_t n_q, int64_t id_bound, const int64_t *rowptr, const int64_t *ids,
                     const float *scores, const float *values, int64_t *out_ids, float *out_scores, float *out_values,
                     void *workspace, int64_t workspace_bytes, void *stream);

/* The MLP pair head at inference (lkg_pairmlp.hip; literalkg_amd/pairmlp.py).  Queries are the n_q rows of uq, candidates
 * the n_cand rows of v (f32, 128 columns, row strides ldu / ldv: multiples of 4, 16-byte aligned bases): the two halves
 * of the head's first layer, already projected (the bias in either of them).  With the folded second and third layer --
 * w2 64 x 128 row-major contiguous, b2[64], w3[64], b3[1], BatchNorm in inference form folded in -- the logit of a pair is
 *     z(i, c) = w3 . relu(w2 relu(uq_i + v_c) + b2) + b3
 * on the exact-f32 MFMA in a fixed operation order: the same bits for a pair wherever and by whichever of the entry
 * points below it is computed.
 *
 * lkg_pair_mlp_scores_f32: out[i * ldo + c] = z(i, c).
 * lkg_pair_mlp_splits    : as lkg_topk_splits, for lkg_pair_mlp_select_f32.
 * lkg_pair_mlp_select_f32: as lkg_topk_select_f32 with s(i, c) = -2 z(i, c) (exact): per split each query's best top_k
 *     (s, id) into ws_s / ws_i [S][n_q][top_k], for lkg_topk_merge_f32 with qn NULL, whose values -s / 2 are the logits.
 *     The n_q x n_cand logits are never stored.  Filter, cand_ids, tie and NaN rules as for lkg_topk_select_f32.
 *
 * Filtered ranking under the head (higher logit is better), the counterpart of lkg_rank_prepare_f32 / lkg_rank_count_f32:
 * lkg_pair_mlp_prepare_f32: thr[i] = z(i, truth[i]) (truth[i] a row of v) and, with a filter, better[i] / equal[i] = MINUS
 *     the number of filtered candidates c != truth[i] with z(i, c) > thr[i] / == thr[i] (else 0).  The filter is a
 *     structure of lkg_csr_build_device over n_rows entity ids (rowptr int32[n_rows+1], col, eptr, rel): query i drops
 *     every col[e] of row filter_row[i] that has a raw edge with relation filter_rel[i] (filter_rel[i] < 0: any
 *     relation).  cand_slot int32[n_rows] maps an entity id to its row of v, -1 = not a candidate (such entries are
 *     skipped); cand_slot NULL = the identity, n_rows == n_cand.  rowptr NULL = no filter.  An entry counts once
 *     however many raw edges it has; an entry that names the truth is skipped.
 * lkg_pair_mlp_count_f32  : better[i] += #{c != truth[i] : z(i, c) > thr[i]}, equal[i] += #{c != truth[i] : z == thr[i]}
 *     over the n_cand rows of v (int32 atomics, one per row, count and workgroup: the result does not depend on the
 *     order of arrival or the launch shape; the n_q x n_cand logits are never stored).  After prepare + count, better /
 *     equal are the filtered counts.  Every logit compared -- threshold, counted, filtered -- has the bits
 *     lkg_pair_mlp_scores_f32 stores for that pair.  A NaN logit counts nowhere; a NaN threshold gives 0 / 0.  64-bit
 *     addressing throughout, n_cand < INT32_MAX.                                                                  */
int lkg_pair_mlp_scores_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v, int64_t ldv,
                            const float *w2, const float *b2, const float *w3, const float *b3, float *out, int64_t ldo,
                            void *stream);
int32_t lkg_pair_mlp_splits(int64_t n_q, int64_t n_cand, int32_t requested);
int lkg_pair_mlp_select_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v, int64_t ldv,
                            const float *w2, const float *b2, const float *w3, const float *b3, const int64_t *cand_ids,
                            const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                            const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t top_k, int32_t splits,
                            float *ws_s, int32_t *ws_i, void *stream);
int lkg_pair_mlp_prepare_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v, int64_t ldv,
                             const float *w2, const float *b2, const float *w3, const float *b3, const int64_t *truth,
                             int64_t n_rows, const int32_t *cand_slot, const int64_t *filter_row,
                             const int64_t *filter_rel, const int32_t *rowptr, const int32_t *col, const int32_t *eptr,
                             const int32_t *rel, float *thr, int32_t *better, int32_t *equal, void *stream);
int lkg_pair_mlp_count_f32(int64_t n_q, int64_t n_cand, const float *uq, int64_t ldu, const float *v, int64_t ldv,
                           const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                           const int64_t *truth, int32_t *better, int32_t *equal, void *stream);

/* Explicit pairs under the head (lkg_pairmlp.hip; score_pairs_mlp, evaluate_mlp_classification).  Pair i is (row u_idx[i]
 * of u, row v_idx[i] of v) of the two projected tables (as uq / v above: f32, 128 columns, row strides multiples of 4,
 * 16-byte aligned); a NULL index list means "pair i uses row i".  Row indices are trusted.
 *
 * lkg_pair_mlp_pairs_f32: out[i] = z(u_idx[i], v_idx[i]), the bits lkg_pair_mlp_scores_f32 stores for that pair, and / or
 *     counts[0..4] += tp, fp, tn, fn, nan against labels (uint8[n_pairs], 0 or 1) and the logit threshold thr: a pair is
 *     predicted positive iff z > thr (an f32 compare); a NaN logit is counted in nan and in none of the other four.
 *     out and counts are each nullable, at least one is given; counts needs labels.  The counts are ACCUMULATED (64-bit
 *     integer atomics, at most five per workgroup: the order of arrival does not enter), so batches add up; the caller
 *     zeroes them.  64-bit addressing, n_pairs <= INT32_MAX - 1; n_pairs == 0 launches nothing.                      */
int lkg_pair_mlp_pairs_f32(int64_t n_pairs, const float *u, int64_t ldu, const float *v, int64_t ldv,
                           const int64_t *u_idx, const int64_t *v_idx, const float *w2, const float *b2, const float *w3,
                           const float *b3, const uint8_t *labels, float thr, float *out, int64_t *counts, void *stream);

/* Exact tie-aware ROC AUC and average precision of n (score, label) pairs (lkg_csr_device.hip): scores f32[n], labels
 * uint8[n] (0 or 1).  out_counts int64[5] = n_pos, n_neg, n_nan, n_groups, auc2; out_ap double[1].
 *   ties      by float equality: -0.0 and +0.0 tie; +-inf are ordinary values
 *   NaN       scores are counted in n_nan and take part in nothing else (n_pos + n_neg + n_nan = n)
 *   n_groups  the number of distinct non-NaN scores
 *   auc2      sum over positives i of (2 #{negatives j: s_j < s_i} + #{negatives j: s_j == s_i}), an exact integer;
 *             ROC AUC = auc2 / (2 n_pos n_neg), formed by the caller
 *   ap        sum over the distinct scores in descending order of (TP_g - TP_(g-1)) / n_pos * TP_g / (TP_g + FP_g), the
 *             cumulative counts taken at the end of each tie group (average precision as a step function, not the
 *             trapezoid); float64, three roundings per term, summed in an order that is a fixed function of the sorted
 *             scores: the same bits from run to run and for any permutation of the input.  0.0 when n_pos == 0.
 * n <= INT32_MAX - 1; n == 0 gives all-zero outputs.  workspace: lkg_binary_curve_workspace(n) bytes of device memory. */
int64_t lkg_binary_curve_workspace(int64_t n);
int lkg_binary_curve_f32(int64_t n, const float *scores, const uint8_t *labels, int64_t *out_counts, double *out_ap,
                         void *workspace, int64_t workspace_bytes, void *stream);

/* Explicit triples under the model's own score (lkg_triples.hip; score_triples, evaluate_triple_classification).  Triple i
 * is (query row q_idx[i], candidate row c_idx[i]) of the n_rows x k table p (P_r for 'transr', the inference table
 * otherwise); its query is q = p[q_idx[i]] + alpha e[rel[i]] (e NULL: the row itself; rel NULL: row 0 of e), formed with
 * the one rounding lkg_rank_queries_f32 makes.  Row and relation indices are trusted; addressing is 64-bit.
 *
 * lkg_triple_scores_f32: out[i] = the kernel score s = pn[c_idx[i]] - 2 q.p_c (pn NULL: dot scoring, s = -2 q.p_c), the
 *     bits lkg_rank_count_f32 compares and lkg_topk_merge_f32 returns as `scores` for that (query, candidate) -- or, with
 *     flag 1, the reported score it returns as `values`: |q|^2 + s (pn given; |q|^2 with lkg_rank_sqnorm_f32's bits) or
 *     -s / 2 (dot).  And / or counts[0..4] += tp, fp, tn, fn, nan against labels (uint8[n], 0 or 1) and thr: a triple is
 *     predicted positive iff out[i] <= thr -- with flag 2, iff out[i] >= thr -- one f32 compare on the value out would
 *     hold; a NaN score is counted in nan alone.  out and counts are each nullable, at least one is given; counts needs
 *     labels and a thr that is not NaN.  The counts are ACCUMULATED (64-bit integer atomics, at most five per workgroup),
 *     so batches add up; the caller zeroes them.  n <= INT32_MAX - 1; n == 0 launches nothing.                        */
int lkg_triple_scores_f32(int64_t n, int32_t k, const float *p, int64_t ldp, const int64_t *q_idx, const int64_t *c_idx,
                          const float *pn, const float *e, int64_t lde, const int64_t *rel, float alpha, int32_t flags,
                          const uint8_t *labels, float thr, float *out, int64_t *counts, void *stream);

/* Exact tie-aware classification thresholds per relation (lkg_csr_device.hip; fit_triple_thresholds): scores f32[n],
 * labels uint8[n] (0 or 1), rel int64[n] in [0, n_relations) (NULL: every triple under relation 0, the pooled fit).
 * Within a relation the non-NaN scores are taken best first (lower_is_better: ascending, else descending) and grouped by
 * float equality (-0.0 == +0.0); with TP_g / FP_g the cumulative label counts at the end of group g, correct(0) = n_neg
 * and correct(g) = TP_g + n_neg - FP_g.  thr[rho] = the score of the smallest g that maximises correct (a zero as +0.0),
 * or, if that g is 0 (also: no scores), the sentinel -inf (lower_is_better) / +inf.  stats int64[n_relations][4] = n (all
 * triples of the relation), n_pos (among its non-NaN scores), correct (at the threshold; NaN scores are wrong), n_nan.
 * 1 <= n_relations < 2^29, n <= INT32_MAX - 1.  workspace: lkg_threshold_fit_workspace(n, n_relations) bytes of device
 * memory; the call allocates nothing.                                                                              */
int64_t lkg_threshold_fit_workspace(int64_t n, int64_t n_relations);
int lkg_threshold_fit_f32(int64_t n, int64_t n_relations, const float *scores, const uint8_t *labels, const int64_t *rel,
                          int32_t lower_is_better, float *thr, int64_t *stats, void *workspace, int64_t workspace_bytes,
                          void *stream);

/* The relation slot of a triple (lkg_relations.hip; literalkg_amd/relations.py: score_relations, rank_relations,
 * predict_relations).  Pair i is (query row q_idx[i], candidate row c_idx[i]); a chunk of n_rel relations is scored in one
 * launch and the stored row of scores is then filtered, counted and selected from.  Row indices are trusted; addressing
 * is 64-bit.
 *
 * lkg_relation_scores_f32: out[i * ldo + j] = the reported score of pair i under the chunk's relation j, the bits
 *     lkg_triple_scores_f32 writes with flag 1 for (q_idx[i], c_idx[i]) on that relation's operands: |q|^2 + (pn_j[c] -
 *     2 q.p_c) with q = p_j[q_idx[i]] + alpha e[j] (one rounding per element), |q|^2 with lkg_rank_sqnorm_f32's bits.
 *     Relation j's table of rows starts at p + j * rel_stride (row stride ldp), its squared norms at pn + j * pn_stride,
 *     its embedding is row j of e (row stride lde); rel_stride = pn_stride = 0: one table shared by all relations
 *     ('transe').  One launch whatever n_rel is; n <= INT32_MAX - 1; n == 0 or n_rel == 0 launches nothing.
 * lkg_relation_order_f32 : per pair i over scores[i * lds .. + n_rel): first every relation under which the pair is known
 *     is dropped -- the raw edges eptr[e] .. eptr[e+1] of the entry e whose col is filter_col[i] in row filter_row[i] of
 *     the lkg_csr_build_device structure (rowptr, col, eptr, rel); duplicates and order do not matter; rowptr NULL = no
 *     filter.  With truth non-NULL, better[i] / equal[i] = #{r' != truth[i], not dropped : s(i, r') < / == s(i, truth[i])}
 *     (the truth's own score is used whether or not it is known; a NaN score counts nowhere, a NaN truth gives 0 / 0).
 *     With top_k > 0, top_ids[i, j] / top_scores[i, j] = the j-th smallest (score, relation id) among the relations
 *     neither dropped nor NaN -- float comparison, then the id -- padded with -1 / NaN.  Compares and integer adds only.
 *     1 <= n_rel <= LKG_RELATION_MAX (a workgroup stages four rows of scores in 64 KB of LDS), top_k in
 *     [0, LKG_TOPK_MAX]; truth NULL and top_k == 0 together is an error.                                              */
#define LKG_RELATION_MAX 4096
int lkg_relation_scores_f32(int64_t n, int32_t k, int32_t n_rel, const float *p, int64_t ldp, int64_t rel_stride,
                            const float *pn, int64_t pn_stride, const int64_t *q_idx, const int64_t *c_idx,
                            const float *e, int64_t lde, float alpha, float *out, int64_t ldo, void *stream);
int lkg_relation_order_f32(int64_t n, int32_t n_rel, const float *scores, int64_t lds, const int64_t *truth,
                           const int64_t *filter_row, const int64_t *filter_col, const int32_t *rowptr,
                           const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t top_k, int32_t *better,
                           int32_t *equal, int64_t *top_ids, float *top_scores, void *stream);

/* Multi-answer retrieval (lkg_retrieval.hip; literalkg_amd/retrieval.py): the place of every answer of a query in the
 * query's ranked list.  Candidates, cand_ids, the filter structure and the kernel score s(i, c) as for lkg_topk_select_f32,
 * bit for bit.  The answers of the queries are given as KEYS (s, id): key_s / key_id, per query a contiguous run sorted by
 * ascending s (float comparison) and then ascending id, as lkg_accept_order sorts, the s from lkg_triple_scores_f32, no
 * NaN.  A ROW is a query vector (row row_q[i] of q) with a slice of key_n[i] <= LKG_RETRIEVAL_SLICE consecutive keys of its
 * query starting at key_off[i]; the query's whole run is qkey_off[i] .. + qkey_n[i] and its slices are cut every
 * LKG_RETRIEVAL_SLICE keys.  buckets is int32[n_rows][LKG_RETRIEVAL_SLICE].
 *
 * lkg_retrieval_prepare_f32: WRITES every bucket of every row: bucket 0 = -(key_off[i] - qkey_off[i]), the others 0, less
 *     one in bucket g for every filter entry of the query (row filter_row[i], relation filter_rel[i], < 0: any) that is a
 *     candidate, whose score is not NaN, that is not one of the query's keys, and that has g < key_n[i] of the row's keys
 *     before it.  cand_slot int32[n_ids] maps an entity id to its candidate row, -1 = not a candidate; NULL = the identity
 *     (n_ids == n_cand).  rowptr NULL = no filter.
 * lkg_retrieval_count_f32  : bucket g of row i += #{c : s(i, c) not NaN, (s, id(c)) not a key of the row, exactly g <
 *     key_n[i] of the row's keys before (s, id(c))} (int32 atomics, one per non-zero bucket per workgroup; the scores are
 *     never stored).  After prepare + count the inclusive prefix of a row's buckets up to g is the number of listed
 *     candidates that are not answers of the query ahead of key g.
 * lkg_retrieval_finish     : per query u with keys qkey_ptr[u] .. qkey_ptr[u + 1] (int64[n_q + 1]) and rows row_base[u] ..:
 *     before[j] = that prefix and position[j] = 1 + before[j] + (index of key j in its query), int64 per key.  With hits
 *     non-NULL also, per query and k = ks[x]: hits[u, x] = #{position <= k}; ndcg[u, x] = (sum over position <= k of
 *     disc[position]) / icum[min(n_answers[u], k)]; ap[u] = (sum_i i / position_i) / n_answers[u]; rr[u] = 1 / position_1
 *     (0 without keys) -- float64, summed in an order fixed by the sorted positions.  disc / icum: double[k_tab + 1], disc[p]
 *     = 1 / log2(1 + p), icum its running sums, k_tab >= min(max ks, the largest position).
 * n_rows, n_cand, n_ids <= INT32_MAX - 1; empty inputs launch nothing; addressing is 64-bit.                           */
#define LKG_RETRIEVAL_SLICE 32
int lkg_retrieval_prepare_f32(int64_t n_rows, int64_t n_cand, int32_t k, const float *q, int64_t ldq,
                              const int64_t *row_q, const float *p, int64_t ldp, const float *pn, int64_t n_ids,
                              const int32_t *cand_slot, const int64_t *key_off, const int32_t *key_n,
                              const int64_t *qkey_off, const int64_t *qkey_n, const float *key_s, const int64_t *key_id,
                              const int64_t *filter_row, const int64_t *filter_rel, const int32_t *rowptr,
                              const int32_t *col, const int32_t *eptr, const int32_t *rel, int32_t *buckets,
                              void *stream);
int lkg_retrieval_count_f32(int64_t n_rows, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const int64_t *row_q,
                            const float *p, int64_t ldp, const float *pn, const int64_t *cand_ids,
                            const int64_t *key_off, const int32_t *key_n, const float *key_s, const int64_t *key_id,
                            int32_t *buckets, void *stream);
int lkg_retrieval_finish(int64_t n_q, const int64_t *qkey_ptr, const int64_t *row_base, const int64_t *n_answers,
                         const int32_t *buckets, int32_t n_ks, const int64_t *ks, int64_t k_tab, const double *disc,
                         const double *icum, int64_t *before, int64_t *position, int64_t *hits, double *ndcg, double *ap,
                         double *rr, void *stream);

/* 1-vs-all training loss (lkg_softmax.hip; literalkg_amd/one_vs_all.py): cross-entropy of the truth against the softmax
 * over ALL candidates.  Queries, candidates and the kernel score s(i, c) as for lkg_rank_* above, bit for bit.  The logit is
 *     z(i, c) = -scale * beta * s(i, c)      (pn given: beta = 1, minus the squared distance up to the row constant
 *                                              ||q_i||^2, which cancels;  pn NULL: beta = 1/2, z = scale q_i . p_c)
 * one rounded product of the score; scale > 0, finite.  loss_i = logsumexp_c z(i, c) - z(i, truth[i]).
 *
 * lkg_softmax_all_splits     : as lkg_topk_splits.  The loss's last bits may depend on S; for a given S every output is
 *     the same from run to run (no float atomics anywhere).
 * lkg_softmax_all_partial_f32: per split j and query i the running pair ws_m[j * n_q + i] = the largest logit of the
 *     split's candidates and ws_l[j * n_q + i] = sum exp(z - that maximum) (splits = lkg_softmax_all_splits(n_q, n_cand,
 *     splits)).  The n_q x n_cand logits are never stored.
 * lkg_softmax_all_finish_f32 : the truth's logit (lkg_rank_prepare_f32's pair routine: the bits it has inside a tile), the
 *     S partials merged in split order in float64: lse[i] = fl32(M + log L), loss[i] = fl32((M + log L) - z_t), and
 *     (lse_lo nullable) lse_lo[i] = fl32((M + log L) - lse[i]), what lse's rounding dropped.  A NaN in query row i gives
 *     lse[i] = loss[i] = NaN and touches no other row.  truth is clamped into [0, n_cand).
 * lkg_softmax_all_weights_f32: the backward's recompute for a chunk of n_cand candidates that starts at candidate c_base
 *     of the table the forward pass ran over (p and pn point AT the chunk; truth, lse, lse_lo and g are per query):
 *         v[i * ldv + c] = scale * beta * g[i] * (exp(z(i, c_base + c) - lse[i] - lse_lo[i]) - [c_base + c == truth[i]]),
 *     ldv >= n_cand, lse_lo NULL = 0 (every weight of row i then carries lse[i]'s rounding, |lse| u / 2, relative).
 *     With it  dQ = 2 V P  and  dP = 2 V^T Q - 2 diag(colsum V) P  (the second term only with pn).
 * n_q == 0 launches nothing; addressing is 64-bit.                                                                    */
#define LKG_SOFTMAX_MAX_SPLITS 64
int32_t lkg_softmax_all_splits(int64_t n_q, int64_t n_cand, int32_t requested);
int lkg_softmax_all_partial_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *pn, float scale, int32_t splits, float *ws_m, float *ws_l,
                                void *stream);
int lkg_softmax_all_finish_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                               int64_t ldp, const float *pn, const int64_t *truth, float scale, int32_t splits,
                               const float *ws_m, const float *ws_l, float *lse, float *lse_lo, float *loss,
                               void *stream);
int lkg_softmax_all_weights_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *pn, int64_t c_base, const int64_t *truth, const float *lse,
                                const float *lse_lo, const float *g, float scale, float *v, int64_t ldv, void *stream);

/* The filtered 1-vs-all loss: query i drops the candidate POSITIONS xcol[xptr[i] .. xptr[i + 1]) (ascending, unique,
 * n_excl = xptr[n_q] < 2^31 entries in all) from its softmax -- a dropped candidate has logit -inf before the running
 * (max, sum) sees it, and weight exactly 0.  The truth of a query must not be in its list (lkg_softmax_excluded never puts
 * it there), so lkg_softmax_all_finish_f32 serves both routes.  With every list empty the masked entry points give the
 * bits of the unmasked ones for the same splits.  No float atomics.
 *
 * lkg_softmax_excluded: builds the lists from the known-triple structure of lkg_csr_build_device over n_rows entities
 *     (rowptr, col, eptr, rel), one wave per query, in two passes.  Query i walks row filter_row[i] and keeps an entry iff
 *     it is known under relation filter_rel[i] (< 0: under any relation), its entity maps to a candidate -- position
 *     pos[entity] (pos int32[n_rows], -1 = not a candidate; must be increasing over the candidates), or the entity id
 *     itself with pos NULL -- inside [0, n_cand), and that position is not truth[i].  First pass (count given, xptr and
 *     xcol NULL): count[i] = the list's length.  The caller forms xptr = the exclusive cumulative sum.  Second pass
 *     (count NULL): fills xcol.
 * lkg_softmax_all_partial_masked_f32 / lkg_softmax_all_weights_masked_f32: as the unmasked entry points; in the weights
 *     the lists hold positions of the whole table (c_base + the chunk's column).                                      */
int lkg_softmax_excluded(int64_t n_q, int64_t n_rows, int64_t n_cand, const int64_t *filter_row, const int64_t *filter_rel,
                         const int64_t *truth, const int32_t *rowptr, const int32_t *col, const int32_t *eptr,
                         const int32_t *rel, const int32_t *pos, int32_t *count, const int32_t *xptr, int32_t *xcol,
                         void *stream);
int lkg_softmax_all_partial_masked_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                       int64_t ldp, const float *pn, float scale, int32_t splits, const int32_t *xptr,
                                       const int32_t *xcol, int64_t n_excl, float *ws_m, float *ws_l, void *stream);
int lkg_softmax_all_weights_masked_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                       int64_t ldp, const float *pn, int64_t c_base, const int64_t *truth,
                                       const float *lse, const float *lse_lo, const float *g, float scale,
                                       const int32_t *xptr, const int32_t *xcol, int64_t n_excl, float *v, int64_t ldv,
                                       void *stream);

/* ------------------------------------------------- KvsAll training loss -- */

/* KvsAll training loss (lkg_kvsall.hip; literalkg_amd/kvs_all.py): binary cross-entropy with logits of EVERY candidate
 * against the multi-hot vector of a query's known answers.  Queries, candidates and the kernel score s(i, c) as for
 * lkg_rank_* / lkg_softmax_all_*, bit for bit.  The logit is
 *     z(i, c) = fl(fl(-scale * beta * s(i, c)) + bias[i])      (pn given: beta = 1; pn NULL: beta = 1/2, s = -2 q.p),
 * bias float[n_q] or NULL (= 0); scale > 0, finite.  The positives of query i are the candidate POSITIONS
 * ycol[yptr[i] .. yptr[i + 1]) (ascending, unique, n_pos = yptr[n_q] < 2^31 entries in all; lkg_softmax_excluded with
 * truth = -1 builds them); yptr NULL = every list empty, with the same bits.  With y = 1 on a positive and 0 elsewhere,
 *     loss_i = sum_c softplus(z) - y' z,      y' = (1 - eps) y + eps / n,      0 <= eps < 1  (label smoothing),
 * each term as softplus(y ? -z : z) + ce_y z with ce_1 = eps (1 - 1/n), ce_0 = -eps / n formed in double and rounded once;
 * with eps == 0 the product is not executed.  A NaN logit poisons its own row only.
 *
 * lkg_sigmoid_all_partial_f32: per split j and query i  ws[j * n_q + i] = the sum of the terms of the split's candidates
 *     (splits = lkg_softmax_all_splits(n_q, n_cand, splits); n = n_cand).  The n_q x n_cand logits are never stored.
 * lkg_sigmoid_all_finish_f32 : loss[i] = fl32(sum_j ws[j * n_q + i]), added in split order in float64 (any splits >= 1: it
 *     also adds the row sums of lkg_sigmoid_all_weights_f32 over that call's tiles).
 * lkg_sigmoid_all_weights_f32: the backward's recompute for a chunk of n_cand candidates that starts at candidate c_base
 *     of the n_total candidates the forward pass ran over (p and pn point AT the chunk; bias and g are per query; the lists
 *     hold positions of the whole table, and n of the smoothing is n_total, not the chunk's width):
 *         v[i * ldv + c] = scale * beta * g[i] * (sigma(z(i, c_base + c)) - y'(i, c_base + c)),
 *     evaluated as ce_1 - sigma(-z) for a positive and sigma(z) + ce_0 otherwise.  With it  dQ = 2 V P,
 *     dP = 2 V^T Q - 2 diag(colsum V) P  (the second term only with pn)  and  dbias = rowsum(V) / (scale * beta).
 *     rowsum (nullable) float[ceil(n_cand / 256) * n_q]: rowsum[t * n_q + i] = the sum of v[i, 256 t .. 256 t + 255] as
 *     stored, added in a fixed order in registers and LDS.
 * No float atomics: for a given number of splits every output repeats bit for bit.  n_q == 0 launches nothing;
 * addressing is 64-bit.                                                                                               */
int lkg_sigmoid_all_partial_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *pn, const float *bias, float scale, double eps, int32_t splits,
                                const int32_t *yptr, const int32_t *ycol, int64_t n_pos, float *ws, void *stream);
int lkg_sigmoid_all_finish_f32(int64_t n_q, int32_t splits, const float *ws, float *loss, void *stream);
int lkg_sigmoid_all_weights_f32(int64_t n_q, int64_t n_cand, int32_t k, const float *q, int64_t ldq, const float *p,
                                int64_t ldp, const float *pn, const float *bias, int64_t c_base, int64_t n_total,
                                const float *g, float scale, double eps, const int32_t *yptr, const int32_t *ycol,
                                int64_t n_pos, float *v, int64_t ldv, float *rowsum, void *stream);

/* ------------------------------- training objectives on sampled rows -- */

/* Self-adversarial negative-sampling loss on grouped rows (lkg_nssa.hip; literalkg_amd/self_adversarial.py).  n_groups
 * groups; group g has the anchor row q[g * ldq ..], the positive row p[g * ldp ..] and the n_neg >= 1 negative rows
 * n[(g * n_neg + j) * ldn ..], all of k float32 columns with free row strides.  With s(x) = sum_c (q_c - x_c)^2 summed
 * directly (distance != 0) or s(x) = sum_c q_c x_c (distance == 0), the logit of a row is
 *     z(x) = fl(scale * fl(margin - s(x)))   (distance)        z(x) = fl(scale * fl(margin + s(x)))   (dot),
 * scale > 0 and finite, margin finite.  The weights are  w_j = e_j / sum_j e_j,  e_j = exp(temperature z_j - max_j
 * temperature z_j),  temperature >= 0 and finite (0: every w_j = fl(1 / n_neg)); they are constants of the loss
 *     loss_g = softplus(-z+) + sum_j w_j softplus(z_j),
 * every softplus evaluated as max(x, 0) + log1p(exp(-|x|)).
 *
 * lkg_nssa_fwd_f32: z_pos[n_groups], z_neg[n_groups * n_neg], w[n_groups * n_neg] and loss[n_groups], each written once.
 * lkg_nssa_bwd_f32: from the upstream g[n_groups] and the kept z_pos, z_neg, w, with a_0 = -g sigma(-z+),
 *     a_j = g w_j sigma(z_j) (sigma on the side that does not cancel) and c_x = (distance ? 2 scale : scale) a_x:
 *         distance:  dp = c_0 (q - p),   dn_j = c_j (q - n_j),   dq = -sum_x c_x (q - x)
 *         dot:       dp = c_0 q,         dn_j = c_j q,           dq = sum_x c_x x
 *     into dq[g * lddq ..], dp[g * lddp ..], dn[(g * n_neg + j) * lddn ..], every element stored once.  dq, dp or dn may
 *     be NULL: that output is not computed, the others keep their bits.
 * A group's outputs depend on its own rows alone (not on n_groups, its position or other groups), the sums run in a fixed
 * order and there are no atomics: every output repeats bit for bit, and the 16-byte and the scalar load path give the
 * same bits.  n_groups == 0 launches nothing; addressing is 64-bit.                                                    */
int lkg_nssa_fwd_f32(int64_t n_groups, int64_t n_neg, int32_t k, const float *q, int64_t ldq, const float *p,
                     int64_t ldp, const float *n, int64_t ldn, int32_t distance, float margin, float scale,
                     float temperature, float *z_pos, float *z_neg, float *w, float *loss, void *stream);
int lkg_nssa_bwd_f32(int64_t n_groups, int64_t n_neg, int32_t k, const float *q, int64_t ldq, const float *p,
                     int64_t ldp, const float *n, int64_t ldn, int32_t distance, float scale, const float *g,
                     const float *z_pos, const float *z_neg, const float *w, float *dq, int64_t lddq, float *dp,
                     int64_t lddp, float *dn, int64_t lddn, void *stream);

/* ---------------------------- negative sampling for given positives --
 * The known triples are two structures of lkg_csr_build_device over n_entities rows, int32 (rowptr, col, eptr, rel): "head_*"
 * has rows = heads with their tails (it answers "is (h, r, c) known?", the tail side), "tail_*" rows = tails with their
 * heads ("is (c, r, t) known?", the head side).  n_raw is the number of raw triples either was built from (eptr[nnz]).
 */

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

/* ------------------------------- relation-slot training objective -- */

/* Softmax cross-entropy of the true relation of a pair against every relation (lkg_relation_loss.hip;
 * literalkg_amd/relation_loss.py).  n pairs, n_rel >= 1 relations, k >= 1 float32 columns per block.
 *
 * Slab mode (rel_stride > 0): pair i, relation j owns the block u[i * ldu + j * rel_stride ..] of k columns
 * (rel_stride >= k, ldu >= (n_rel - 1) * rel_stride + k).  Shared mode (rel_stride == 0): pair i owns the ONE row
 * u[i * ldu ..] of k columns, read for every relation (ldu >= k).  With e[j * lde ..] the relation's row (lde >= k),
 *     s_ij = sum_c (u_ijc + e_jc)^2   summed directly (one fma chain per lane over its 4-column units lane, lane + 64, ...,
 *                                     then one butterfly over the wave),
 *     z_ij = -fl(scale * s_ij),       scale > 0 and finite.
 * A filter (rowptr != NULL: the four arrays of lkg_csr_build_device, filter_row[n] and filter_col[n] in its row and column
 * ids, all in range) makes every relation rr != truth[i] listed under the entry (filter_row[i], filter_col[i]) ineligible:
 * z[i, rr] = -inf.  truth[i] in [0, n_rel) is never dropped; duplicates in the filter change nothing.  Then
 *     m_i = max_j z_ij,   sum_i = sum_j exp(z_ij - m_i),   lse_i = m_i + log(sum_i),
 *     loss_i = (m_i - z_i,truth_i) + log(sum_i)
 * (a pair whose only eligible relation is the truth: exactly 0).
 *
 * lkg_relation_loss_fwd_f32 stores z[i * ldz + j] (ldz >= n_rel), lse[n] and loss[n], each element once (a dropped
 * relation's logit twice: the value, then -inf).
 * lkg_relation_loss_bwd_f32 reads the upstream g[n], z and truth, takes m_i and sum_i from the stored row again (the
 * forward's own passes: the same bits; exp(z_ij - lse_i) would carry half an ulp of lse into every softmax) and forms
 *     c_ij = fl(fl(-2 scale * g_i) * (exp(z_ij - m_i) / sum_i - [j == truth_i])),      exactly 0.0 where z_ij = -inf.
 *   Slab mode: every block of u is OVERWRITTEN in place by c_ij (u_ij + e_j), each element stored once (zeros, not
 *     products, where z_ij = -inf); gd and c must be NULL.
 *   Shared mode: u is only read; gd[i * ldgd ..] = sum_j c_ij (u_i + e_j), added in increasing j (ldgd >= k), and
 *     c[i * ldc + j] = c_ij (ldc >= n_rel).  Either of gd, c may be NULL: it is not computed, the other keeps its bits.
 *
 * One wave per pair.  A pair's outputs depend on its own blocks, e, its truth and its filter entry alone -- not on n, on
 * its position or on other pairs -- the sums run in a fixed order and there are no atomics: every output repeats bit for
 * bit, and the 16-byte and the scalar load path (taken when k, a stride or a pointer is not a multiple of 4 elements /
 * 16 bytes) give the same bits.  n == 0 launches nothing; addressing is 64-bit.                                          */
int lkg_relation_loss_fwd_f32(int64_t n, int32_t n_rel, int32_t k, const float *u, int64_t ldu, int64_t rel_stride,
                              const float *e, int64_t lde, const int64_t *truth, const int64_t *filter_row,
                              const int64_t *filter_col, const int32_t *rowptr, const int32_t *col, const int32_t *eptr,
                              const int32_t *rel, float scale, float *z, int64_t ldz, float *lse, float *loss,
                              void *stream);
int lkg_relation_loss_bwd_f32(int64_t n, int32_t n_rel, int32_t k, float *u, int64_t ldu, int64_t rel_stride,
                              const float *e, int64_t lde, const int64_t *truth, float scale, const float *g,
                              const float *z, int64_t ldz, float *gd, int64_t ldgd, float *c, int64_t ldc,
                              void *stream);

/* ----------------------------------------------- ordered split-K GEMM -- */

/* C = alpha * op(A) op(B) + beta * C (+ bias[n]) in float32 for products with a SMALL output and a LONG reduction
 * (lkg_gemm_ordered.hip; literalkg_amd/gemm_ordered.py): the reduction is spread over the chip as lkg_gemm_f32's atomic
 * split does, but the pieces are added in a fixed order, so every output repeats bit for bit.  op(A) is m x k (A stored
 * k x m with trans_a), op(B) is k x n (B stored n x k with trans_b), row-major with free row strides; ldc >= n.
 *
 * The partition.  For `splits` = S in [1, 256]:
 *     per   = 16 * ceil(ceil(k / S) / 16)          (0 for k == 0)
 *     S_eff = ceil(k / per)                        (0 for k == 0; at most min(S, ceil(k / 16)))
 * and split z in [0, S_eff) covers k in [z * per, min(k, (z + 1) * per)): every boundary but the last is a multiple of
 * 16.  lkg_gemm_ordered_partition returns S_eff and stores per (per may be NULL); a negative lkg_status on bad arguments.
 *
 * The arithmetic.  A first launch of (output tiles) x S_eff workgroups computes, per element and split, the partial
 *     p_z = the k-ordered fmaf chain of the exact f32-input MFMA (v_mfma_f32_32x32x2_f32) over the split's k, from 0.0,
 *           one rounding per product -- the bits an UNSPLIT call over the k-slice alone produces with alpha = 1, beta = 0,
 * and stores it with plain vector stores into workspace[z][m][n] (float32, contiguous).  A second launch forms
 *     s   = ((p_0 + p_1) + p_2) + ...               float32 adds in ascending z
 *     t   = fmaf(alpha, s, bias[j])                 (bias NULL: 0.0f)
 *     out = beta == 0 ? t : fmaf(beta, C_old, t)    (C is not read when beta == 0)
 * With S_eff == 1 the first launch applies the last two lines to s = p_0 itself: no workspace, no second launch.  k == 0
 * gives s = 0.0, that is beta * C + bias.  There are no atomics, no counters and no in-launch combine.
 *
 * The property.  An output element is a function of its row of op(A), its column of op(B), k, per, alpha, beta, its old C
 * and its bias -- not of m, n, other rows or columns, alignment, strides, the stream, the workspace's previous contents
 * or the run.  The 16-byte load path and the clamped scalar one (edge tiles; an operand whose address is not a multiple of
 * 16 bytes or whose row stride is not a multiple of 4 elements) give the same bits.
 *
 * lkg_gemm_ordered_splits: the default S, a pure function of its five arguments (no device query, no environment):
 *     tiles = ceil(m / 128) * ceil(n / 128)
 *     S     = max(1, min(512 / tiles, k / 512, 2^26 / (m * n), 256))          (integer divisions)
 * about two workgroups per CU of a 256-CU device, no split shorter than 512 k, partials within 256 MB.
 * lkg_gemm_ordered_workspace: the bytes lkg_gemm_ordered_f32 needs for (m, n, k, splits): S_eff * m * n * 4, 0 for
 * S_eff <= 1; a negative lkg_status on bad arguments.
 * lkg_gemm_ordered_f32: splits outside [1, 256], a workspace shorter than that, a leading dimension smaller than the
 * stored row or a null operand is LKG_ERR_INVALID_ARG before any launch.  m == 0 or n == 0 launches nothing.               */
int32_t lkg_gemm_ordered_splits(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k);
int64_t lkg_gemm_ordered_partition(int64_t k, int32_t splits, int64_t *per);
int64_t lkg_gemm_ordered_workspace(int64_t m, int64_t n, int64_t k, int32_t splits);
int lkg_gemm_ordered_f32(int32_t trans_a, int32_t trans_b, int64_t m, int64_t n, int64_t k, int32_t splits, float alpha,
                         const float *a, int64_t lda, const float *b, int64_t ldb, float beta, float *c, int64_t ldc,
                         const float *bias, void *workspace, int64_t workspace_bytes, void *stream);

/* ---------------- neighbour sampling for the batch-pruned training step -- */

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

/* ------------------------ threshold retrieval under the MLP pair head --
 * literalkg_amd/pairmlp.py (predict_accepted_mlp, count_accepted_mlp) drives it. */

/* The three entry points below share their operands with lkg_pair_mlp_select_f32 (lkg_pairmlp.hip): uq[n_q x 128] the
 * projected query rows (fc1's bias included), v[n_cand x 128] the projected candidate rows, (w2, b2, w3, b3) the folded
 * head, cand_ids[n_cand] the entity id of every candidate row (NULL: the row number), and the known-triples filter
 * (filter_row[n_q], filter_rel[n_q], rowptr, col, eptr, rel) of lkg_csr_build_device over entity ids: query i drops the
 * candidates whose id is a col of row filter_row[i] under relation filter_rel[i] (-1: under any).  The filter is absent
 * (rowptr NULL) or complete.  thr[n_q] holds one float32 logit threshold per query.
 *
 * The decision.  z(i, c) is the logit lkg_pair_mlp_scores_f32 stores for the pair, bit for bit, whatever tile, wave,
 * split or launch computes it.  Candidate c of query i is ACCEPTED iff z(i, c) > thr[i] in one float32 compare, strictly
 * (a NaN logit or a NaN threshold accepts nothing; thr = +inf accepts nothing; thr = -inf accepts every logit that is
 * neither NaN nor -inf), and the filter does not drop it.  Only a candidate that passes the compare is looked up in the
 * filter.
 *
 *   lkg_pair_mlp_accept_count_f32    counts[i] += the number of accepted candidates of query i.  The caller zeroes
 *                                    counts.  Integer atomics only: the counts do not depend on the order of anything.
 *   lkg_pair_mlp_accept_append_f32   the same counts, and in the same pass every accepted entry takes a slot from the
 *                                    ONE 64-bit cursor (*cursor, zeroed by the caller).  A slot below `capacity` writes
 *                                    out_rows[slot] = i, out_ids[slot] = the id, out_logits[slot] = z; a slot at or past
 *                                    it writes nothing.  The counts are exact whether or not the buffer overflows, and
 *                                    overflow is sum(counts) > capacity (then *cursor == sum(counts) too).  The entries
 *                                    are in no particular order.  capacity == 0 needs no output buffers.
 *   lkg_pair_mlp_accept_emit_f32     the second pass of the two-pass route: counts[n_q] are those of a count over the
 *                                    same arguments, base[n_q] their exclusive scan (int64), cursor[n_q] zeroed by the
 *                                    caller.  Every accepted entry of query i takes slot = cursor[i]++ and writes
 *                                    out_ids / out_scores (s = -2 z, exact, the ascending key of lkg_accept_order) /
 *                                    out_logits at base[i] + slot when 0 <= slot < counts[i]; otherwise it writes
 *                                    nothing and sets *flag to 1.  With the counts of the same arguments the flag stays 0.
 *                                    A row's entries are in no particular order; (s, id) is unique within a row, so
 *                                    lkg_accept_order makes the result unique.
 *
 * splits: candidate splits per launch, 0 = automatic, else 1 .. LKG_TOPK_MAX_SPLITS; resolved by lkg_pair_mlp_splits.
 * No result depends on it.
 *
 * Conventions: uq and v hold DENSE rows of 128 floats -- row i starts at element 128 i; there is no row-stride argument
 * (the projections that feed these entry points are dense, and every row-strided operand of this library is an operand
 * that has to be exercised past 2^32 elements) -- and uq, v and w2 are 16-byte aligned; n_q, n_cand and capacity below
 * 2^31 - 1; n_q == 0 or n_cand == 0 launches nothing; a bad size, a null pointer, a misaligned operand or an incomplete
 * filter is LKG_ERR_INVALID_ARG before any launch.  No float atomics.                                                      */
int lkg_pair_mlp_accept_count_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                  const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                                  const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                  const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                  int32_t splits, int32_t *counts, void *stream);

int lkg_pair_mlp_accept_append_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                   const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                                   const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                   const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                   int32_t splits, int32_t *counts, int64_t capacity, int64_t *cursor, int32_t *out_rows,
                                   int32_t *out_ids, float *out_logits, void *stream);

int lkg_pair_mlp_accept_emit_f32(int64_t n_q, int64_t n_cand, const float *uq, const float *v,
                                 const float *w2, const float *b2, const float *w3, const float *b3, const float *thr,
                                 const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                                 const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                                 int32_t splits, const int32_t *counts, const int64_t *base, int32_t *cursor,
                                 int64_t *out_ids, float *out_scores, float *out_logits, int32_t *flag, void *stream);

/* ------------- scoring and ranking against per-query candidate lists --
 * literalkg_amd/lists.py (score_lists, rank_in_lists, evaluate_list_ranking) drives it. */

/* Operands of both entry points.  q[n_q x k] (row stride q_stride) the query rows lkg_rank_queries_f32 makes; p[n_rows x k]
 * (row stride p_stride) the candidate rows with their squared norms pn[n_rows] (lkg_rank_sqnorm_f32; NULL: dot scoring);
 * lists[n_q x m] (row stride lists_stride, m >= 1) the slots of every query: slot j of query i holds a row number of p, or a
 * negative value for an EMPTY slot.  A row number at or past n_rows is treated as an empty slot (nothing is read out of
 * bounds); callers check their ids beforehand.
 *
 * The kernel score of (query i, row c) is s = pn[c] - 2 q_i . p_c (dot scoring: -2 q_i . p_c), the bits
 * lkg_rank_count_f32 compares and lkg_triple_scores_f32 stores for that (query, candidate), whatever slot, slice, wave
 * or launch computes it.
 *
 *   lkg_list_scores_f32   out[i * out_stride + j] = the score of slot j of query i, NaN for an empty slot.  flags bit 0
 *                         (reported): qn[i] + s with pn given (qn[n_q]: lkg_rank_sqnorm_f32 over q, required then) or
 *                         -s / 2 for dot scoring; flags 0: s itself (qn is not read).
 *   lkg_list_count_f32    truth[n_q] holds the row of p that is query i's truth; its score comes from the same chain.
 *                         Slot j of query i is COUNTED unless it is empty, its row is truth[i], or the filter drops it:
 *                         (filter_row[n_q], filter_rel[n_q], rowptr, col, eptr, rel) of lkg_csr_build_device over entity
 *                         ids, query i dropping the slots whose entity id is a col of row filter_row[i] under relation
 *                         filter_rel[i] (negative: under any).  cand_ids[n_rows] is the entity id of every row of p
 *                         (NULL: the row number).  The filter is absent (rowptr NULL) or complete.
 *                         kept[i] += the counted slots, better[i] += those with s < s_truth, equal[i] += those with
 *                         s == s_truth, by float32 compares (a NaN on either side is neither).  The caller zeroes the
 *                         three int64 arrays; the additions are integer atomics, so no order enters.  No score is stored.
 *
 * The row strides are named *_stride, in elements: tests/test_lists_gpu.py places p itself past 2^31 and 2^32 elements
 * (the ledger of tests/wide_cases.py follows the arguments named ld* of the training and query entry points).
 *
 * Conventions: n_q * ceil(m / 256) below 2^31 - 1 (one workgroup per query and slice of 256 slots); n_rows below
 * 2^31 - 1; all row offsets are 64-bit; 16-byte loads are used only where q, p and their strides allow them; n_q == 0 launches
 * nothing; a bad size, a null pointer or an incomplete filter is LKG_ERR_INVALID_ARG before any launch.  No float
 * atomics.                                                                                                             */
int lkg_list_scores_f32(int64_t n_q, int64_t m, int64_t n_rows, int32_t k, const float *q, int64_t q_stride, const float *qn,
                        const float *p, int64_t p_stride, const float *pn, const int64_t *lists, int64_t lists_stride,
                        int32_t flags, float *out, int64_t out_stride, void *stream);

int lkg_list_count_f32(int64_t n_q, int64_t m, int64_t n_rows, int32_t k, const float *q, int64_t q_stride, const float *p,
                       int64_t p_stride, const float *pn, const int64_t *lists, int64_t lists_stride, const int64_t *truth,
                       const int64_t *cand_ids, const int64_t *filter_row, const int64_t *filter_rel,
                       const int32_t *rowptr, const int32_t *col, const int32_t *eptr, const int32_t *rel,
                       int64_t *better, int64_t *equal, int64_t *kept, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* LITERALKG_HIP_H */
