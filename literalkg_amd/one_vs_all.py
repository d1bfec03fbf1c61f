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

Filtered loss.  ``known`` (a KnownTriples) drops from the row of (h, r, ?) every candidate c != t with
(h, r, c) known -- from the row of (?, r, t) every c != h with (c, r, t) known; 'dot' ignores r and drops the entities
known under ANY relation -- so the other true answers of a query are no longer its negatives, which is what filtered MRR
measures.  The truth is exempt: ``known`` may or may not hold the trained triples.  The mask is applied inside the tile,
before the running (max, sum) sees the logit (ops.softmax_excluded builds the lists, the masked kernels of lkg_softmax.hip
apply them).  ``candidates`` (unique entity ids, sorted internally: the result has the same bits for any order) restricts
the softmax to those rows -- type-constrained training; one side at a time, every truth must be a candidate, the table's
gradient reaches only candidate and query rows, and 'transr' projects the gathered rows, not the N-row table.

There is no L2 term (lkg_adam_step_f32 carries weight decay) and no label smoothing of the softmax (its extra term
eps (z_t - mean z) has a closed form in column sums and would bring its own accuracy contract); multi-hot (KvsAll) targets,
with label smoothing of their own, are literalkg_amd/kvs_all.py.  Under
``torch.no_grad()`` in eval mode the table is the cached inference table and ``reduction='none'`` gives the per-triple
negative log-likelihood.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _objectives as O
from . import _queries as Q
from . import ops
from ._objectives import REDUCTIONS, check_reduction      # noqa: F401  (their home before _objectives.py)
from .gemm_ordered import check_route

MLP_MESSAGE = ("scoring='mlp' has no 1-vs-all loss: the pair head is trained by train_MLP on labelled pairs -- use "
               "'transr', 'transe' or 'dot'")


def one_vs_all_loss(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, side: str = "tail", scale: float = 1.0,
                    reduction: str = "mean", scoring: Optional[str] = None, splits: Optional[int] = None,
                    known=None, candidates: Optional[torch.Tensor] = None, products: str = "engine") -> torch.Tensor:
    """The 1-vs-all loss of the triples (h, r, t) under the model (see the module docstring): side 'tail' / 'head' / 'both'
    (the mean of the two sides), scale > 0 a temperature on the logits, reduction 'mean' / 'sum' / 'none' (float32[B]),
    scoring 'transr' / 'transe' / 'dot' (default: model.scoring), splits the candidate splits of the forward kernel (None:
    automatic; the last bits of the loss may depend on it, for a given value they repeat from run to run).  known: a
    KnownTriples whose other answers of each query leave its softmax; candidates: the unique entity ids the softmax runs
    over (one side only; every truth among them).  products as in ops.softmax_all_loss ("ordered": the backward's dQ
    product on gemm_ordered).  Differentiable in every parameter the table, the relation embeddings and (transr)
    gat_trans_M depend on."""
    check_route(products)
    side = Q.check_side(side)
    scoring = Q.resolve_scoring(model, scoring, MLP_MESSAGE)
    reduction = check_reduction(reduction)
    scale, splits, _ = ops.check_softmax_args(scale, splits)
    Q.check_triple_lists(h, r, t)
    Q.check_transr_model(model, scoring)
    Q.check_known_entities(known, model)
    if candidates is not None:
        Q.check_ids("candidates", candidates)
        if side == "both":
            raise ValueError("candidates restrict one side's answers: side must be 'tail' or 'head' with candidates, got "
                             "'both'")
    dev = model.entity_embed.weight.device
    b = h.numel()
    if b == 0:
        return O.empty_loss(model, reduction)
    h, t = ops.checked_ids(model.n_entities, h.to(dev), t.to(dev))          # (out-of-range ids never reach a kernel)
    (r,) = ops.checked_ids(model.n_relations, r.to(dev), what="relation")
    Q.check_known_device(known, dev)
    cand, pos = O.candidate_block(model, candidates, dev)
    if pos is not None:
        missing = int((pos[t if side == "tail" else h] < 0).sum())
        if missing:
            raise ValueError(f"{missing} of the {b} true {'tails' if side == 'tail' else 'heads'} are not among the "
                             "candidates: every truth must be a candidate")

    def score_group(table, rows, w, r, h, t):
        """per triple of one projection the loss of the side (the mean of the two sides' for 'both'); known / pos: the
        exclusion lists of ops.softmax_excluded per side"""
        p = O.projected(rows, w)                                # alive until the backward pass (transr: N x relation_dim)
        total = None
        for s_ in Q.rank_sides(side):
            ent, truth = (h, t) if s_ == "tail" else (t, h)
            q = O.query_rows(model, scoring, s_, table, p, w, ent, r, pos)
            if pos is not None:
                truth = pos[truth].long()                       # (every truth is a candidate: checked above)
            exclude = None
            if known is not None:
                exclude = ops.softmax_excluded(known.for_side(s_), ent, O.known_relations(scoring, r), truth, p.shape[0],
                                               pos)
            loss = ops.softmax_all_loss(q, p, truth, distance=scoring != "dot", scale=scale, splits=splits,
                                        exclude=exclude, products=products)
            total = loss if total is None else total + loss
        return total if side != "both" else 0.5 * total

    return O.all_entity_loss(model, scoring, r, (h, t), cand, reduction, score_group)
