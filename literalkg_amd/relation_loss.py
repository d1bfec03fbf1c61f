"""Relation-slot training loss: the cross-entropy of the true relation of (h, ?, t) against the softmax over EVERY relation
(LibKGE's 1vsAll on the ``s_o`` query type), the objective whose filtered metric rank_relations /
evaluate_relation_prediction report.

With d_i = T[h_i] - T[t_i], u_ij = d_i W_j + e_j ('transe': d_i + e_j) and s_ij = sum_c u_ijc^2, the logit of relation j for
pair i is z_ij = -scale s_ij and

    loss_i = logsumexp_j z_ij - z_i,r_i

over the eligible relations: with ``known`` every j != r_i for which (h_i, j, t_i) is known is dropped (rank_relations'
rule; the truth is exempt, so ``known`` may or may not hold the trained triples).  Under 'transr' the projection is linear,
P_j[h] + e_j - P_j[t] = (T[h] - T[t]) W_j + e_j, so the head-side form gives the same number: the loss has no ``side``, it
reads two table rows per pair (``prune_to_batch`` applies) and every projection of a batch is ONE product
D [P x C] @ Wcat [C x R D] on ops.gemm.  s_ij is summed directly, as lkg_nssa.hip sums its distance: it is NOT built to
the bits of score_relations, which reports fl(|q|^2 + |p|^2 - 2 q.p).  ``reduction`` acts over the pairs; there is no L2 term
(weight decay is Adam's).  Device code: lkg_relation_loss.hip (one wave per pair, no atomics).

Determinism: no float atomics on the route, every accumulating product runs with beta = 1 onto an initialised output in a
fixed chunk order (ops.all_entity_backward's docstring has the reason), so for given arguments the loss and every gradient
repeat bit for bit.  The kernels' outputs for a pair depend on that pair's blocks alone; the GEMM in front of them
('transr') may change its engine with a chunk's row count, so the bits are promised across different ``chunk_bytes`` only
in shared mode ('transe'), where no slab exists and chunk_bytes bounds nothing.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function

from . import _native as N
from . import _objectives as O
from . import _queries as Q
from . import ops, pruned
from . import relations as R
from .gemm_ordered import accumulate_ordered, check_route, current_route, gemm_ordered, keyword_route

SHARDED_MESSAGE = ("the relation loss gathers its rows from a single-device table: the row-sharded model holds a block of it "
                   "per rank (train it on a single-device LiteralKG)")
CHUNK_BYTES = 256 << 20        # the slab U of a chunk of pairs: rows x R x D x 4 bytes


def chunk_rows(n_pairs: int, n_rel: int, k: int, chunk_bytes: int = CHUNK_BYTES) -> int:
    """Pairs per chunk of slab mode: as many as fit chunk_bytes; ValueError when one pair's slab alone does not."""
    one = int(n_rel) * int(k) * 4
    if one > int(chunk_bytes):
        raise ValueError(f"one pair's slab takes {one} bytes ({n_rel} relations x {k} columns x 4), chunk_bytes is "
                         f"{int(chunk_bytes)}: raise chunk_bytes to at least {one}")
    return max(1, min(int(n_pairs), int(chunk_bytes) // one))


def _operands(d, w, e, truth, filt, filter_row, filter_col):
    ops._need_gpu(d, w, e, truth, filter_row, filter_col)
    d, e = ops._f32_rows(d), ops._f32_rows(e)
    (p, c), (n_rel, k) = d.shape, e.shape
    if n_rel == 0 or k == 0:
        raise ValueError(f"relation_softmax_loss: e is {tuple(e.shape)} (at least one relation of at least one column)")
    if w is None:
        if c != k:
            raise ValueError(f"relation_softmax_loss: shared mode (w None) needs d ({tuple(d.shape)}) as wide as e "
                             f"({tuple(e.shape)})")
    else:
        if w.dtype != torch.float32:
            raise TypeError(f"expected float32, got {w.dtype}")
        if tuple(w.shape) != (n_rel, c, k):
            raise ValueError(f"relation_softmax_loss: w is {tuple(w.shape)}, d {tuple(d.shape)} and e {tuple(e.shape)} "
                             f"need ({n_rel}, {c}, {k})")
    truth = ops._i64(truth.reshape(-1))
    if truth.numel() != p:
        raise ValueError(f"relation_softmax_loss: {truth.numel()} truths for {p} pairs")
    if filt is not None and (filter_row is None or filter_col is None):
        raise ValueError("relation_softmax_loss: a filter needs filter_row and filter_col")
    return d, e, truth


def _wcat(w: torch.Tensor) -> torch.Tensor:
    """[C, R D]: column block j is W_j, so that row i of d @ Wcat lists d_i W_0, d_i W_1, ..."""
    n_rel, c, k = w.shape
    return w.permute(1, 0, 2).reshape(c, n_rel * k).contiguous()


def relation_softmax_forward(u: torch.Tensor, rel_stride: int, e: torch.Tensor, truth: torch.Tensor, scale: float = 1.0,
                             filt=None, filter_row=None, filter_col=None, z: Optional[torch.Tensor] = None):
    """(loss float32[P], z float32[P, R], lse float32[P]) of lkg_relation_loss_fwd_f32 on given blocks, no autograd: slab
    mode (rel_stride > 0: row i of u holds the R blocks of pair i, rel_stride elements apart) or shared mode (rel_stride
    0: row i of u is the one block of pair i).  z: where to store the logits (rows of any stride)."""
    ops._need_gpu(u, e, truth, filter_row, filter_col)
    u, e, truth = ops._f32_rows(u), ops._f32_rows(e), ops._i64(truth.reshape(-1))
    p, (n_rel, k), dev = u.shape[0], e.shape, u.device
    if z is None:
        z = torch.empty((p, n_rel), dtype=torch.float32, device=dev)
    lse, loss = (torch.empty(p, dtype=torch.float32, device=dev) for _ in range(2))
    fargs = ops._filter_args("relation_softmax_loss", filt, filter_row, filter_col, p)
    if p:
        N.call("lkg_relation_loss_fwd_f32", p, n_rel, k, N.ptr(u), ops._ld(u), int(rel_stride), N.ptr(e), ops._ld(e),
               N.ptr(truth), *fargs(), float(scale), N.ptr(z), ops._ld(z), N.ptr(lse), N.ptr(loss), ops._stream())
    return loss, z, lse


def relation_softmax_backward(u: torch.Tensor, rel_stride: int, e: torch.Tensor, truth: torch.Tensor, scale: float,
                              g: torch.Tensor, z: torch.Tensor, want_gd: bool = True, want_c: bool = True):
    """lkg_relation_loss_bwd_f32 on given blocks, no autograd.  Slab mode: u is OVERWRITTEN by G_ij = c_ij (u_ij + e_j) and
    returned.  Shared mode: (gd float32[P, k] or None, c float32[P, R] or None)."""
    ops._need_gpu(u, e, truth, g, z)
    e, truth = ops._f32_rows(e), ops._i64(truth.reshape(-1))
    p, (n_rel, k), dev = u.shape[0], e.shape, u.device
    if rel_stride and (u.dtype != torch.float32 or u.dim() != 2 or u.stride(1) != 1):
        raise ValueError("relation_softmax_backward: slab mode rewrites u in place and takes it as it is (float32 rows)")
    u = u if rel_stride else ops._f32_rows(u)
    g = g.reshape(-1).float().contiguous()
    gd = torch.empty((p, k), dtype=torch.float32, device=dev) if not rel_stride and want_gd else None
    c = torch.empty((p, n_rel), dtype=torch.float32, device=dev) if not rel_stride and want_c else None
    if p:
        N.call("lkg_relation_loss_bwd_f32", p, n_rel, k, N.ptr(u), ops._ld(u), int(rel_stride), N.ptr(e), ops._ld(e),
               N.ptr(truth), float(scale), N.ptr(g), N.ptr(z), ops._ld(z), N.ptr(gd), k, N.ptr(c), n_rel,
               ops._stream())
    return u if rel_stride else (gd, c)


DD_SLICE = ops.SOFTMAX_DQ_SLICE        # dd += G Wcat^T in reductions of about this many columns (whole relations): short
#                                        chains from the running sum, for the reason ops.SOFTMAX_DQ_SLICE states


class _RelationSoftmaxLoss(Function):
    """loss_i = logsumexp_j z_ij - z_i,truth_i over the eligible relations.  Forward keeps z and the inputs (the backward
    kernel takes a row's maximum and sum from z again); the slab of slab mode is recomputed per chunk of pairs in the
    backward pass."""

    @staticmethod
    def forward(ctx, d, w, e, truth, scale, filt, filter_row, filter_col, chunk_bytes):
        d, e, truth = _operands(d, w, e, truth, filt, filter_row, filter_col)
        (p, c), (n_rel, k), dev = d.shape, e.shape, d.device
        ctx.shapes = (d.shape, None if w is None else w.shape, e.shape)
        ctx.empty = p == 0
        ctx.route = current_route()                      # the backward follows the forward's choice wherever it is called
        if ctx.empty:
            return torch.empty(0, dtype=torch.float32, device=dev)
        if w is None:
            loss, z, _ = relation_softmax_forward(d, 0, e, truth, scale, filt, filter_row, filter_col)
        else:
            rows = chunk_rows(p, n_rel, k, chunk_bytes)
            wcat = _wcat(w)
            z = torch.empty((p, n_rel), dtype=torch.float32, device=dev)
            ubuf = torch.empty((rows, n_rel * k), dtype=torch.float32, device=dev)
            parts = []
            for lo in range(0, p, rows):                 # a fixed order
                hi = min(p, lo + rows)
                u = ops.gemm(d[lo:hi], wcat, out=ubuf[:hi - lo])
                parts.append(relation_softmax_forward(
                    u, k, e, truth[lo:hi], scale, filt, None if filt is None else filter_row[lo:hi],
                    None if filt is None else filter_col[lo:hi], z=z[lo:hi]))
            loss = torch.cat([x[0] for x in parts]) if len(parts) > 1 else parts[0][0]
            ctx.rows = rows
        ctx.save_for_backward(d, w, e, truth, z)
        ctx.scale = scale
        return loss

    @staticmethod
    def backward(ctx, g):
        want_d, want_w, want_e = ctx.needs_input_grad[:3]
        nothing = (None,) * 6
        dev = g.device
        ordered = ctx.route == "ordered"
        if ctx.empty or not (want_d or want_w or want_e):
            return tuple(torch.zeros(s, dtype=torch.float32, device=dev) if wnt and s is not None else None
                         for s, wnt in zip(ctx.shapes, (want_d, want_w, want_e))) + nothing
        d, w, e, truth, z = ctx.saved_tensors
        (p, c), (n_rel, k), scale = d.shape, e.shape, ctx.scale
        g = g.reshape(-1).float().contiguous()
        ones = torch.ones((p, 1), dtype=torch.float32, device=dev)
        if w is None:                                    # shared mode: no slab
            gd, cf = relation_softmax_backward(d, 0, e, truth, scale, g, z, want_d, want_e)
            de = None
            if want_e:
                # de = c^T d + diag(colsum c) e; the column sums ride in the product as a column of ones next to d
                # (lkg_colsum_f32 adds with float atomics)
                d1 = torch.cat((d, ones), dim=1)
                if ordered:                              # R x (k + 1) over P rows: split over the chip, added in order
                    t = gemm_ordered(cf, d1, trans_a=True)
                else:
                    t = torch.zeros((n_rel, k + 1), dtype=torch.float32, device=dev)
                    ops.gemm(cf, d1, trans_a=True, beta=1.0, out=t)
                de = torch.addcmul(t[:, :k], t[:, k:], e)
            return (gd, None, de) + nothing
        wcat = _wcat(w)
        rows = ctx.rows
        ubuf = torch.empty((rows, n_rel * k), dtype=torch.float32, device=dev)
        dd = torch.zeros((p, c), dtype=torch.float32, device=dev) if want_d else None
        acc = d1 = None
        if want_w or want_e:                             # [dWcat ; de] += [d | 1]^T G: ONE product for both
            acc = torch.zeros((c + 1, n_rel * k), dtype=torch.float32, device=dev)
            d1 = torch.cat((d, ones), dim=1)
        step = max(1, DD_SLICE // k) * k
        for lo in range(0, p, rows):                     # a fixed order: every sum below accumulates chunk after chunk
            hi = min(p, lo + rows)
            u = ops.gemm(d[lo:hi], wcat, out=ubuf[:hi - lo])
            gm = relation_softmax_backward(u, k, e, truth[lo:hi], scale, g[lo:hi], z[lo:hi])
            if want_d and ordered:                       # one product per chunk, no split longer than a slice
                accumulate_ordered(gm, wcat, dd[lo:hi], step, trans_b=True)
            elif want_d:
                for s0 in range(0, n_rel * k, step):
                    s1 = min(n_rel * k, s0 + step)
                    ops.gemm(gm[:, s0:s1], wcat[:, s0:s1], trans_b=True, beta=1.0, out=dd[lo:hi])
            if acc is not None:
                ops.gemm(d1[lo:hi], gm, trans_a=True, beta=1.0, out=acc)
        dw = acc[:c].view(c, n_rel, k).permute(1, 0, 2).contiguous() if want_w else None
        de = acc[c].view(n_rel, k).clone() if want_e else None
        return (dd, dw, de) + nothing


def relation_softmax_loss(d: torch.Tensor, w: Optional[torch.Tensor], e: torch.Tensor, truth: torch.Tensor,
                          scale: float = 1.0, filt=None, filter_row: Optional[torch.Tensor] = None,
                          filter_col: Optional[torch.Tensor] = None, chunk_bytes: int = CHUNK_BYTES,
                          products: str = "engine") -> torch.Tensor:
    """float32[P]: loss_i = logsumexp_j z_ij - z_i,truth_i with z_ij = -scale ||d_i W_j + e_j||^2 (w None, shared mode:
    ||d_i + e_j||^2, d as wide as e) for d float32[P, C], w float32[R, C, D] or None, e float32[R, D], truth int64[P] in
    [0, R).  filt = (rowptr, col, eptr, rel) of ops.csr_build_device: row i's softmax leaves out every relation other than
    truth[i] listed under the entry (filter_row[i], filter_col[i]); the ids must be rows / columns of the structure.
    Differentiable in d, w and e; a gradient nobody needs is None and its product or kernel is not launched (dw and de
    share ONE product, launched when either is needed), the others keep their bits.  Slab mode (w given) runs in chunks
    of pairs whose slab rows x R x D x 4 bytes fits chunk_bytes (ValueError when one pair's does not) and recomputes the
    slab in the backward pass; its bits may depend on chunk_bytes (the GEMM's engine may change with the row count), the
    loss from a given slab does not.  Shared mode has no slab: chunk_bytes bounds nothing there and changes no bit.
    products "ordered" (gemm_ordered.keyword_route): slab mode's dd += G Wcat^T is one gemm_ordered product per chunk
    (no split longer than a DD_SLICE slice), shared mode's c^T [d | 1] behind de runs on gemm_ordered; the loss and the
    other gradients keep their bits."""
    with keyword_route(products):                        # (a bad name: ValueError before any device work)
        scale, _, chunk_bytes = ops.check_softmax_args(scale, None, chunk_bytes)
        ops._need_gpu(d, w, e, truth, filter_row, filter_col)
        return _RelationSoftmaxLoss.apply(d, w, e, truth, scale, filt, filter_row, filter_col, chunk_bytes)


def relation_loss(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, known=None, scoring: Optional[str] = None,
                  scale: float = 1.0, reduction: str = "mean", chunk_bytes: int = CHUNK_BYTES,
                  products: str = "engine") -> torch.Tensor:
    """The cross-entropy of the true relations r of the pairs (h, t) (int64[P] each) against the softmax over every
    relation under the model (see the module docstring): scoring 'transr' / 'transe' (default: model.scoring; 'dot' and
    'mlp' are refused as relation prediction refuses them), scale > 0, reduction 'mean' / 'sum' / 'none' over the pairs,
    known a KnownTriples (the other known relations of a pair leave its softmax; the truth never does).  The logits are
    summed directly and are not the bits of score_relations.  Differentiable in every parameter the table, the relation
    embeddings and (transr) gat_trans_M depend on; the table is taken as self_adversarial_loss takes it (training or grad
    enabled: the graph-carrying table, prune_to_batch honoured; otherwise the kept one).  products as in
    relation_softmax_loss."""
    check_route(products)
    O.check_single_device(model, SHARDED_MESSAGE)
    scoring = R._check_scoring(model, scoring)
    reduction = O.check_reduction(reduction)
    scale, _, chunk_bytes = ops.check_softmax_args(scale, None, chunk_bytes)
    R._check_pairs(h, t, r)
    R._check_known(known, model)
    if scoring == "transr":
        chunk_rows(1, model.n_relations, model.gat_trans_M.shape[2], chunk_bytes)
    if h.numel() == 0:
        return O.empty_loss(model, reduction)
    dev = model.entity_embed.weight.device
    Q.check_known_device(known, dev)
    h, t = ops.checked_ids(model.n_entities, h.to(dev), t.to(dev))   # (out-of-range ids never reach a kernel)
    (r,) = ops.checked_ids(model.n_relations, r.to(dev), what="relation")
    model.device = dev
    table, (hp, tp) = model._embeddings_and_ids(h, t)                # the pruned table with positions, or the full one
    Q.check_table_shape(model, scoring, table)
    # ONE gather of the 2 P rows: its backward is one scatter into a table-sized gradient
    rows = pruned.gather_rows(table, torch.cat((hp, tp)))
    n = h.numel()
    d = ops.axpby(rows[:n], rows[n:], 1.0, -1.0)
    w = model.gat_trans_M if scoring == "transr" else None
    filt = known.by_head if known is not None else None              # (h, r', t): heads with their tails, raw entity ids
    loss = relation_softmax_loss(d, w, model.relation_embed.weight, r, scale, filt, h if filt is not None else None,
                                 t if filt is not None else None, chunk_bytes, products=products)
    return O.reduce(loss, reduction)
