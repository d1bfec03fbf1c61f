"""Self-adversarial negative-sampling loss (NSSA: RotatE's loss, PyKEEN's ``NSSALoss``, DGL-KE's default for TransE): one
positive scored against its K SAMPLED negatives with a margin, each negative weighted by the model's own softmax over the
group -- hard negatives dominate, at the cost of a sampled step.  It sits between the pairwise ``calc_triplet_loss`` (the K
negatives of a group as K unrelated pairs) and the all-entity objectives of ``one_vs_all.py`` / ``kvs_all.py``.

A group is an anchor query row q, a positive row p and K negative rows n_j.  For side 'tail' the negatives replace the
tail: q = T[h] + e_r, p = T[t]; for side 'head' they replace the head: q = T[t] - e_r, p = T[h] ('dot': q is the row alone,
r is ignored; 'transr': rows projected by gat_trans_M[r]).  The logits follow kvs_all.py's convention

    z+ = scale (margin - ||q - p||^2),   z_j = scale (margin - ||q - n_j||^2)      ('dot': scale (margin + q . x)),

the weights are w_j = softmax_j(temperature z_j) over the group's K negatives, CONSTANTS of the loss (no gradient flows
through them; temperature 0: w_j = 1 / K, the plain uniform negative-sampling loss), and

    L = softplus(-z+) + sum_j w_j softplus(z_j)

-- the positive and the negative half are NOT halved (PyKEEN halves them).  ``reduction`` acts over the groups; there is no
L2 term (weight decay is Adam's).  Device code: lkg_nssa.hip (one workgroup per group, the q row kept in registers, every
row gathered once, no atomics).  The table is taken the way calc_triplet_loss's general path takes it, so
``prune_to_batch`` applies: the loss reads only (2 + K) G rows, gathered ONCE (one table-sized scatter in the backward
pass); for 'transr' the groups are put in relation order, so that a relation's anchors, positives and negatives are one slice
of the gather and take one product with gat_trans_M[r].
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function

from . import _native as N
from . import _objectives as O
from . import _queries as Q
from . import ops, pruned
from ._objectives import check_margin, check_reduction

MLP_MESSAGE = ("scoring='mlp' has no self-adversarial loss: the pair head is trained by train_MLP on labelled pairs -- use "
               "'transr', 'transe' or 'dot'")
SHARDED_MESSAGE = ("the self-adversarial loss gathers its rows from a single-device table: the row-sharded model holds a "
                   "block of it per rank (train it on a single-device LiteralKG)")


def check_temperature(temperature) -> float:
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or \
            not 0.0 <= float(temperature) < float("inf"):
        raise ValueError(f"temperature must be a finite number >= 0, got {temperature!r}")
    return float(temperature)


def _operands(q, p, n):
    ops._need_gpu(q, p, n)
    q, p, n = ops._f32_rows(q), ops._f32_rows(p), ops._f32_rows(n)
    g, k = q.shape
    if p.shape != q.shape or n.shape[1] != k or k == 0 or (g == 0 and n.shape[0] != 0) or \
            (g > 0 and (n.shape[0] == 0 or n.shape[0] % g)):
        raise ValueError(f"sampled_sigmoid_loss: anchors {tuple(q.shape)}, positives {tuple(p.shape)}, negatives "
                         f"{tuple(n.shape)} (G x k, G x k and G K x k with K >= 1)")
    return q, p, n


def sampled_sigmoid_forward(q: torch.Tensor, p: torch.Tensor, n: torch.Tensor, distance: bool = True, margin: float = 0.0,
                            scale: float = 1.0, temperature: float = 1.0):
    """(loss float32[G], z_pos float32[G], z_neg float32[G K], w float32[G K]) of lkg_nssa_fwd_f32, no autograd: the
    losses, the logits of the positives and of the negatives, and the negatives' weights."""
    q, p, n = _operands(q, p, n)
    (g, k), dev = q.shape, q.device
    kn = n.shape[0] // g if g else 0
    loss, z_pos = (torch.empty(g, dtype=torch.float32, device=dev) for _ in range(2))
    z_neg, w = (torch.empty(g * kn, dtype=torch.float32, device=dev) for _ in range(2))
    if g:
        N.call("lkg_nssa_fwd_f32", g, kn, k, N.ptr(q), ops._ld(q), N.ptr(p), ops._ld(p), N.ptr(n), ops._ld(n), int(distance),
               margin, scale, temperature, N.ptr(z_pos), N.ptr(z_neg), N.ptr(w), N.ptr(loss), ops._stream())
    return loss, z_pos, z_neg, w


class _SampledSigmoidLoss(Function):
    """L_g = softplus(-z+) + sum_j w_j softplus(z_j) over groups of one positive and K negatives (lkg_nssa_fwd_f32); the
    backward (lkg_nssa_bwd_f32) reads the kept z+, z_j and w_j, writes every element of dq, dp and dn once and leaves out
    the gradients nobody needs (None), whose absence does not change the bits of the others."""

    @staticmethod
    def forward(ctx, q, p, n, distance, margin, scale, temperature):
        q, p, n = _operands(q, p, n)
        loss, z_pos, z_neg, w = sampled_sigmoid_forward(q, p, n, distance, margin, scale, temperature)
        ctx.empty = q.shape[0] == 0
        ctx.shapes = (q.shape, p.shape, n.shape)
        if not ctx.empty:
            ctx.save_for_backward(q, p, n, z_pos, z_neg, w)
            ctx.meta = (int(distance), scale, n.shape[0] // q.shape[0])
        return loss

    @staticmethod
    def backward(ctx, g):
        want = ctx.needs_input_grad[:3]
        nothing = (None,) * 4
        if ctx.empty:
            dev = g.device
            return tuple(torch.zeros(s, dtype=torch.float32, device=dev) if wnt else None
                         for s, wnt in zip(ctx.shapes, want)) + nothing
        q, p, n, z_pos, z_neg, w = ctx.saved_tensors
        distance, scale, kn = ctx.meta
        g = g.reshape(-1).float().contiguous()
        k = q.shape[1]
        dq, dp, dn = (torch.empty((x.shape[0], k), dtype=torch.float32, device=q.device) if wnt else None
                      for x, wnt in zip((q, p, n), want))
        N.call("lkg_nssa_bwd_f32", q.shape[0], kn, k, N.ptr(q), ops._ld(q), N.ptr(p), ops._ld(p), N.ptr(n), ops._ld(n),
               distance, scale, N.ptr(g), N.ptr(z_pos), N.ptr(z_neg), N.ptr(w), N.ptr(dq), k, N.ptr(dp), k, N.ptr(dn), k,
               ops._stream())
        return (dq, dp, dn) + nothing


def sampled_sigmoid_loss(q: torch.Tensor, p: torch.Tensor, n: torch.Tensor, distance: bool = True, margin: float = 0.0,
                         scale: float = 1.0, temperature: float = 1.0) -> torch.Tensor:
    """float32[G]: the self-adversarial negative-sampling loss of G groups -- anchor rows q[G, k], positive rows p[G, k] and
    negative rows n[G K, k], row g K + j negative j of group g (K = n.shape[0] // G >= 1).  distance True: logits
    scale (margin - ||q - x||^2), the distance summed directly; False: scale (margin + q . x).  The weights
    softmax_j(temperature z_j) are constants (temperature 0: 1 / K).  Differentiable in q, p and n; a gradient nobody needs
    is None and is not computed."""
    scale = ops.check_softmax_args(scale, None)[0]
    margin, temperature = check_margin(margin), check_temperature(temperature)
    ops._need_gpu(q, p, n)
    return _SampledSigmoidLoss.apply(q, p, n, bool(distance), margin, scale, temperature)


def group_sampled_batch(h: torch.Tensor, r: torch.Tensor, pos_t: torch.Tensor, neg_t: torch.Tensor, neg_rate: int):
    """(h[G], r[G], t[G], neg[G, K]) of a KGBatchSampler batch (generate_kg_batch's flat layout: K = neg_rate consecutive
    rows share (h, r, t+)), for self_adversarial_loss.  ValueError for a batch that is not whole groups."""
    if isinstance(neg_rate, bool) or not isinstance(neg_rate, int) or neg_rate < 1:
        raise ValueError(f"neg_rate must be a positive integer, got {neg_rate!r}")
    Q.check_triple_lists(h, r, pos_t)
    Q.check_id_pair(h, neg_t, ("h", "neg_t"))
    k = int(neg_rate)
    if h.numel() == 0 or h.numel() % k or (k > 1 and not ops.is_grouped_batch(h, r, pos_t, k)):
        raise ValueError(f"the batch of {h.numel()} rows is not whole groups of {k} consecutive rows that share (h, r, t+)")
    return h[::k].contiguous(), r[::k].contiguous(), pos_t[::k].contiguous(), neg_t.reshape(-1, k)


def _group_losses(scoring: str, side: str, w, rows, gr: int, e, margin, scale, temperature):
    """float32[gr]: the losses of the gr groups of one projection.  rows: their gathered table rows, the gr anchors, then the
    gr positives, then the gr K negatives; e: their relation rows (None for 'dot'); w: gat_trans_M[r] for 'transr' (ONE
    product projects the anchors, the positives and the negatives), else None."""
    rows = O.projected(rows, w)
    q, p, n = rows[:gr], rows[gr:2 * gr], rows[2 * gr:]
    distance = scoring != "dot"
    if distance:
        q = ops.axpby(q, e, 1.0, Q.side_alpha(side))
    return sampled_sigmoid_loss(q, p, n, distance=distance, margin=margin, scale=scale, temperature=temperature)


def _side_losses(model, scoring: str, side: str, table, h, r, t, neg, margin, scale, temperature):
    """float32[G], in the caller's order: the losses of the groups (h, r, t, neg) -- ids already checked and relabelled for
    ``table`` -- corrupted on ``side``."""
    anchor, pos = (h, t) if side == "tail" else (t, h)
    kn = neg.shape[1]
    perm, spans = O.relation_groups(model, scoring, r)      # relation order: a relation's rows are ONE slice of the gather
    anchor, pos, neg, r = O.in_group_order(perm, anchor, pos, neg, r)
    ids = [x for s0, s1, _ in spans for x in (anchor[s0:s1], pos[s0:s1], neg[s0:s1].reshape(-1))]
    # ONE gather of the (2 + K) G rows: its backward is one scatter into a table-sized gradient, not one per operand
    rows = pruned.gather_rows(table, torch.cat(ids))
    e = pruned.gather_rows(model.relation_embed.weight, r) if scoring != "dot" else None
    parts = []
    for s0, s1, rr in spans:
        w = model.gat_trans_M[rr] if rr is not None else None
        parts.append(_group_losses(scoring, side, w, rows[s0 * (2 + kn):s1 * (2 + kn)], s1 - s0,
                                   e[s0:s1] if e is not None else None,
                                   margin, scale, temperature))
    return O.in_caller_order(perm, parts)


def losses_by_side(model, scoring: str, h, r, t, neg, parts, margin, scale, temperature):
    """[float32[G_i]]: the per-group losses of the G > 0 groups (h, r, t, neg[G, K]) in parts -- ``parts`` lists
    (side, positions) with positions an index tensor into the groups (None: all of them) -- on ONE table: the ids are
    checked and the table is taken once (the encoder runs once, prune_to_batch sees every id), each part is gathered and
    scored for itself.  Arguments already validated (self_adversarial_loss, negatives.sampled_negative_loss)."""
    dev = model.entity_embed.weight.device
    h, t, neg = ops.checked_ids(model.n_entities, h.to(dev), t.to(dev), neg.to(dev))    # (out-of-range ids never reach a kernel)
    (r,) = ops.checked_ids(model.n_relations, r.to(dev), what="relation")
    model.device = dev
    table, (h, t, neg) = model._embeddings_and_ids(h, t, neg)        # the pruned table with positions, or the full one
    Q.check_table_shape(model, scoring, table)
    return [_side_losses(model, scoring, side, table, *((x if at is None else x[at]) for x in (h, r, t, neg)),
                         margin, scale, temperature) for side, at in parts]


def self_adversarial_loss(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, neg: torch.Tensor, side: str = "tail",
                          margin: float = 0.0, scale: float = 1.0, temperature: float = 1.0, reduction: str = "mean",
                          scoring: Optional[str] = None) -> torch.Tensor:
    """The self-adversarial negative-sampling loss of the triples (h, r, t) (int64[G]) against their sampled negatives
    neg (int64[G, K], K >= 1) under the model (see the module docstring): side 'tail' (the negatives replace the tail) or
    'head' (they replace the head), margin any finite number, scale > 0, temperature >= 0, reduction 'mean' / 'sum' /
    'none' over the groups, scoring 'transr' / 'transe' / 'dot' (default: model.scoring).  Differentiable in every
    parameter the table, the relation embeddings and (transr) gat_trans_M depend on."""
    O.check_single_device(model, SHARDED_MESSAGE)
    side = Q.check_one_side(side, "the negatives replace one side of the triple")
    scoring = Q.resolve_scoring(model, scoring, MLP_MESSAGE)
    reduction = check_reduction(reduction)
    scale = ops.check_softmax_args(scale, None)[0]
    margin, temperature = check_margin(margin), check_temperature(temperature)
    Q.check_triple_lists(h, r, t)
    if not isinstance(neg, torch.Tensor) or neg.dim() != 2 or neg.dtype.is_floating_point or neg.dtype == torch.bool or \
            neg.shape[0] != h.numel() or (h.numel() > 0 and neg.shape[1] < 1):
        raise ValueError(f"neg must be a 2-D tensor of integer ids with one row of K >= 1 negatives per triple "
                         f"({h.numel()} rows)")
    Q.check_transr_model(model, scoring)
    if h.numel() == 0:
        return O.empty_loss(model, reduction)
    return O.reduce(losses_by_side(model, scoring, h, r, t, neg, [(side, None)], margin, scale, temperature)[0], reduction)
