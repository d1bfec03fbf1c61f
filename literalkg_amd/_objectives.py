"""The training front end shared by one_vs_all.py, kvs_all.py, self_adversarial.py and negatives.py, the sibling of
_queries.py: the argument checks the objectives have in common, the empty-batch result, the candidate block, the grouping
of a batch by relation ('transr' projects per relation) with the way back to the caller's order, the operands of a loss
over every entity, and the reduction.  Plain functions; each caller decides where it runs them, so its argument errors
still come before any device work.  No function here asks which loss called it: what differs between the losses arrives
as the closure that scores one group."""
from __future__ import annotations

from typing import Callable, Optional

import torch

from . import _queries as Q
from . import ops, pruned

REDUCTIONS = ("mean", "sum", "none")


def check_reduction(reduction: str) -> str:
    if reduction not in REDUCTIONS:
        raise ValueError(f"reduction must be one of {REDUCTIONS}, got {reduction!r}")
    return reduction


def check_margin(margin) -> float:
    if isinstance(margin, bool) or not isinstance(margin, (int, float)) or not abs(float(margin)) < float("inf"):
        raise ValueError(f"margin must be a finite number, got {margin!r}")
    return float(margin)


def check_single_device(model, message: str):
    if not hasattr(model, "_table_for_inference"):          # (ShardedLiteralKG: its table is a block per rank)
        raise NotImplementedError(message)


def reduce(loss: torch.Tensor, reduction: str) -> torch.Tensor:
    if reduction == "mean":
        return loss.mean()
    return loss.sum() if reduction == "sum" else loss


def empty_loss(model, reduction: str) -> torch.Tensor:
    """The loss of no rows at all: float32[0] for 'none', 0 otherwise, on the model's device."""
    return torch.zeros((0,) if reduction == "none" else (), dtype=torch.float32, device=model.entity_embed.weight.device)


def candidate_block(model, candidates: Optional[torch.Tensor], dev):
    """(cand, pos) of a ``candidates`` argument (None, None without one): the ids on the device, range-checked, unique and
    at least one, SORTED -- pos (int32[n_entities], -1 = not a candidate) is increasing over the candidates, so the bits
    ignore the order they were given in."""
    if candidates is None:
        return None, None
    (cand,) = ops.checked_ids(model.n_entities, candidates.to(dev), what="candidate entity")
    ops.check_deferred_errors()
    Q.check_unique(cand)
    if cand.numel() == 0:
        raise ValueError("candidates must hold at least one entity id")
    cand = torch.sort(cand).values
    pos = torch.full((model.n_entities,), -1, dtype=torch.int32, device=dev)
    pos[cand] = torch.arange(cand.numel(), dtype=torch.int32, device=dev)
    return cand, pos


def relation_groups(model, scoring: str, r: torch.Tensor):
    """(perm, spans): 'transr' scores a relation's rows against their own projection, so perm (int64) puts the rows in
    relation order and spans lists (s0, s1, relation) of every relation present, positions into the PERMUTED rows; any other
    scoring is one span (0, len(r), None) and perm None (the rows as they are)."""
    if scoring != "transr":
        return None, [(0, r.numel(), None)]
    perm, seg = ops.group_by_key(r, model.n_relations)
    seg = seg.tolist()
    return perm.long(), [(seg[rr], seg[rr + 1], rr) for rr in range(model.n_relations) if seg[rr + 1] > seg[rr]]


def in_group_order(perm: Optional[torch.Tensor], *xs):
    return xs if perm is None else tuple(x[perm] for x in xs)


def in_caller_order(perm: Optional[torch.Tensor], parts):
    """The spans' results, one after the other, back in the order the caller's rows came in."""
    if perm is None:
        return parts[0]
    back = torch.empty_like(perm)
    back[perm] = torch.arange(perm.numel(), device=perm.device)
    return torch.cat(parts)[back]


def projected(rows: torch.Tensor, w: Optional[torch.Tensor]) -> torch.Tensor:
    return rows if w is None else ops.matmul(rows, w)


def query_rows(model, scoring: str, side: str, table, p, w, ent, r, pos) -> torch.Tensor:
    """The query rows of the entities ent (relations r) on ``side`` against the candidate rows p = projected(rows, w):
    gathered from p -- or, with candidates (pos given: p holds only those), from the table and projected on their own --
    and shifted by the relation, q = P[ent] +- e_r (not for 'dot')."""
    q = pruned.gather_rows(p, ent) if pos is None else projected(pruned.gather_rows(table, ent), w)
    if scoring != "dot":
        q = ops.axpby(q, pruned.gather_rows(model.relation_embed.weight, r), 1.0, Q.side_alpha(side))
    return q


def known_relations(scoring: str, r: torch.Tensor) -> torch.Tensor:
    """The relation each row's known answers are looked up under: r, or -1 (any) for 'dot', which ignores r."""
    return r if scoring != "dot" else torch.full_like(r, -1)


def all_entity_loss(model, scoring: str, r: torch.Tensor, ids, cand: Optional[torch.Tensor], reduction: str,
                    score_group: Callable) -> torch.Tensor:
    """The driver of a loss over every entity (or every candidate: cand of candidate_block) for the checked rows (r, *ids)
    on the device: the table is taken once (training or grad enabled: gat_embeddings() with its graph; else the kept one),
    the candidate rows are gathered once for every relation group, and score_group(table, rows, w, r, *ids) gives
    float32[rows of the group] for each group of relation_groups -- w its gat_trans_M[relation] or None -- which go back
    into the caller's order and through ``reduction``."""
    model.device = model.entity_embed.weight.device
    table = model._table_for_inference()
    Q.check_table_shape(model, scoring, table)
    rows = table if cand is None else pruned.gather_rows(table, cand)
    perm, spans = relation_groups(model, scoring, r)
    r, *ids = in_group_order(perm, r, *ids)
    parts = [score_group(table, rows, None if rr is None else model.gat_trans_M[rr], r[s0:s1], *(x[s0:s1] for x in ids))
             for s0, s1, rr in spans]
    return reduce(in_caller_order(perm, parts), reduction)
