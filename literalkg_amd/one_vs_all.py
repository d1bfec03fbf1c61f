"""1-vs-all training: cross-entropy of the true entity against the softmax over EVERY entity (LibKGE's ``1vsAll``, PyKEEN's
LCWA) -- the objective filtered MRR measures, next to the sampled-negative losses of ``calc_triplet_loss``.

For a triple (h, r, t) and side 'tail' the query is q = P[h] + e_r and the truth t; for side 'head' q = P[t] - e_r and the
truth h ('dot': q = P[h] / P[t], no relation).  The logit of candidate c is

    z_c = -scale * ||q - P[c]||^2   ('transe', 'transr'; up to the row constant ||q||^2, which cancels)
    z_c =  scale * q . P[c]         ('dot')

and the loss of the triple is logsumexp_c z_c - z_truth over ALL N entities (ops.softmax_all_loss: lkg_softmax.hip, the
ranking kernels' tile with a running (max, sum) in place of their counts; the B x N logits are never stored by the forward
pass).  P is the full table of the step, ``gat_embeddings()`` with its autograd graph -- never the pruned frontier: every
row is a candidate, so ``prune_to_batch`` does not apply here.  'transr' groups the triples by relation and scores each
group against P_r = P W_r; every P_r (N x relation_dim floats) stays alive until the backward pass has used it.

There is no L2 term (lkg_adam_step_f32 carries weight decay), no ``known`` filter in the denominator (other true answers
stay negatives, as in plain 1vsAll), no ``candidates`` subset and no label smoothing.  Under ``torch.no_grad()`` in eval
mode the table is the cached inference table and ``reduction='none'`` gives the per-triple negative log-likelihood.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _queries as Q
from . import ops, pruned

REDUCTIONS = ("mean", "sum", "none")
MLP_MESSAGE = ("scoring='mlp' has no 1-vs-all loss: the pair head is trained by train_MLP on labelled pairs -- use "
               "'transr', 'transe' or 'dot'")


def check_reduction(reduction: str) -> str:
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    return reduction


def _side_losses(scoring: str, side: str, p, relemb, h, r, t, scale, splits):
    """float32[len(h)]: per triple the loss of the side (the mean of the two sides' for 'both') against the rows p."""
    total = None
    for s_ in Q.rank_sides(side):
        ent, truth = (h, t) if s_ == "tail" else (t, h)
        q = pruned.gather_rows(p, ent)
        if scoring != "dot":
            q = ops.axpby(q, pruned.gather_rows(relemb, r), 1.0, Q.side_alpha(s_))
        loss = ops.softmax_all_loss(q, p, truth, distance=scoring != "dot", scale=scale, splits=splits)
        total = loss if total is None else total + loss
    return total if side != "both" else 0.5 * total


def one_vs_all_loss(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, side: str = "tail", scale: float = 1.0,
                    reduction: str = "mean", scoring: Optional[str] = None, splits: Optional[int] = None) -> torch.Tensor:
    """The 1-vs-all loss of the triples (h, r, t) under the model (see the module docstring): side 'tail' / 'head' / 'both'
    (the mean of the two sides), scale > 0 a temperature on the logits, reduction 'mean' / 'sum' / 'none' (float32[B]),
    scoring 'transr' / 'transe' / 'dot' (default: model.scoring), splits the candidate splits of the forward kernel (None:
    automatic; the last bits of the loss may depend on it, for a given value they repeat from run to run).
    Differentiable in every parameter the table, the relation embeddings and (transr) gat_trans_M depend on."""
    side = Q.check_side(side)
    scoring = Q.resolve_scoring(model, scoring, MLP_MESSAGE)
    reduction = check_reduction(reduction)
    scale, splits, _ = ops.check_softmax_args(scale, splits)
    Q.check_triple_lists(h, r, t)
    Q.check_transr_model(model, scoring)
    dev = model.entity_embed.weight.device
    b = h.numel()
    if b == 0:
        return torch.zeros((0,) if reduction == "none" else (), dtype=torch.float32, device=dev)
    h, t = ops.checked_ids(model.n_entities, h.to(dev), t.to(dev))          # (out-of-range ids never reach a kernel)
    (r,) = ops.checked_ids(model.n_relations, r.to(dev), what="relation")
    model.device = dev
    table = model._table_for_inference()       # training or grad enabled: gat_embeddings() with its graph; else the kept table
    Q.check_table_shape(model, scoring, table)
    relemb = model.relation_embed.weight
    if scoring == "transr":
        perm, seg = ops.group_by_key(r, model.n_relations)
        perm, seg = perm.long(), seg.tolist()
        parts = []
        for rr in range(model.n_relations):
            if seg[rr + 1] > seg[rr]:
                pos = perm[seg[rr]:seg[rr + 1]]
                p_r = ops.matmul(table, model.gat_trans_M[rr])             # alive until the backward pass (N x relation_dim)
                parts.append(_side_losses(scoring, side, p_r, relemb, h[pos], r[pos], t[pos], scale, splits))
        back = torch.empty_like(perm)
        back[perm] = torch.arange(b, device=dev)
        loss = torch.cat(parts)[back]
    else:
        loss = _side_losses(scoring, side, table, relemb, h, r, t, scale, splits)
    if reduction == "mean":
        return loss.mean()
    return loss.sum() if reduction == "sum" else loss
