"""Filtered link-prediction ranking: MR, MRR and Hits@k of held-out triples under the model's own scoring function.

For a test triple (h, r, t) the tail side ranks the truth t among all N entities as the tail of (h, r, .), the head side
ranks h among all N as the head of (., r, t).  Lower distance is better ('transr': ||T_h W_r + e_r - T_c W_r||^2,
'transe': ||T_h + e_r - T_c||^2); for 'dot' (T_h . T_c, the calc_score head) higher is better.  A candidate other than
the truth that forms a ``known`` triple is dropped (the filtered setting); the truth is never compared with itself.
``better`` counts the kept candidates strictly better than the truth, ``equal`` the ties, and
rank = 1 + better + equal / 2 (ties share the mean of their positions; optimistic and pessimistic ranks follow from the two
counts).  A NaN score is neither better nor equal.

Every score is computed on the device by lkg_rank.hip: a GEMM whose output is never stored (its epilogue compares each
score with the truth's and counts), the truth's score and the filtered candidates' scores from the same exact-f32 MFMA
arithmetic, so a candidate whose table row equals the truth's ties exactly.  TransR projects the
table once per relation present in the queries (the tall GEMM), and that projection serves both sides.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import torch

from . import _queries as Q
from . import ops
from ._queries import (SCORINGS, SIDES, RankResult, metrics_from_counts,  # noqa: F401  (public under this module)
                       realistic_rank, scoring_groups)


def _check_triples(h, r, t):
    for name, x in (("h", h), ("r", r), ("t", t)):
        if not isinstance(x, torch.Tensor) or x.dim() != 1:
            raise ValueError(f"{name} must be a 1-D tensor of ids")
    if not h.numel() == r.numel() == t.numel():
        raise ValueError(f"h, r, t have different lengths ({h.numel()}, {r.numel()}, {t.numel()})")


class KnownTriples:
    """The filter: every (h, r, t) of the splits the caller wants to filter by, held on the device as two structures of
    lkg_csr_build_device -- rows = heads with their tails (the tail side drops the tails of (h, r, .)) and rows = tails with
    their heads (the head side) -- each entry listing the relations under which the pair is known.  Memory
    O(N + |known|); duplicates are merged."""

    def __init__(self, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, n_entities: int, n_relations: int):
        _check_triples(h, r, t)
        self.n_entities, self.n_relations = int(n_entities), int(n_relations)
        for ids, n, what in ((h, self.n_entities, "entity"), (t, self.n_entities, "entity"),
                             (r, self.n_relations, "relation")):
            bad = ops.count_ids_outside(n, ids)
            if bad:
                raise IndexError(f"KnownTriples: {bad} {what} id(s) outside [0, {n})")
        self.n_triples = h.numel()
        self.device = h.device
        self.by_head = ops.csr_build_device(self.n_entities, h, t, r)     # tail side
        self.by_tail = ops.csr_build_device(self.n_entities, t, h, r)     # head side

    def for_side(self, side: str):
        return self.by_head if side == "tail" else self.by_tail


def _count_group(model, scoring, side, p, pn, pos, h, r, t, known, batch_size, better, equal):
    """better / equal of one side for the queries at positions pos, against the candidate rows p (squared norms pn)."""
    q_ids, truth = (h, t) if side == "tail" else (t, h)
    filt = known.for_side(side) if known is not None else None
    ids, tru, rel = q_ids[pos], truth[pos], r[pos]
    q, _, _ = Q.side_queries(model, scoring, side, p, pn, ids, rel)
    for lo, hi in Q.batches(pos.numel(), batch_size):
        bb, ee, _ = ops.rank_count(q[lo:hi], p, pn, tru[lo:hi], filt, ids[lo:hi], rel[lo:hi])
        better[pos[lo:hi]] = bb
        equal[pos[lo:hi]] = ee


def rank_triples(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, side: str = "tail",
                 known: Optional[KnownTriples] = None, scoring: Optional[str] = None,
                 batch_size: Optional[int] = None) -> RankResult:
    """Filtered ranks of the triples (h, r, t) on the model's inference table (see the module docstring).  The model's
    mode is left as it is (evaluate_ranking switches to eval); nothing of the model is changed."""
    side = Q.check_side(side)
    scoring = Q.resolve_scoring(model, scoring)
    _check_triples(h, r, t)
    Q.check_batch_size(batch_size)
    Q.check_transr_model(model, scoring)
    Q.check_known_entities(known, model)
    dev = model.entity_embed.weight.device
    b = h.numel()
    better, equal = Q.count_buffers(side, b, dev)
    if b == 0:
        return Q.rank_result(better, equal, side)
    (h, t), r, _ = Q.ids_to_device(model, dev, (h, t), r, known=known)
    with torch.no_grad():
        table = model._table_for_inference().detach()
        for p, pn, pos in scoring_groups(model, scoring, table, r):
            for j, s_ in enumerate(Q.rank_sides(side)):
                _count_group(model, scoring, s_, p, pn, pos, h, r, t, known, batch_size, better[j], equal[j])
            del p, pn
    return Q.rank_result(better, equal, side)


def evaluate_ranking(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, known: Optional[KnownTriples] = None,
                     ks: Sequence[int] = (1, 3, 10), side: str = "both", scoring: Optional[str] = None,
                     batch_size: Optional[int] = None) -> Dict:
    """{'mr', 'mrr', 'hits@k'..., 'n', 'tail': {...}, 'head': {...}}: filtered ranking metrics of the triples; the top
    level is over every rank computed (2B for side='both').  Runs in eval mode, as the reference's evaluate does, and
    restores the model's previous mode."""
    ks = Q.check_ks(ks)
    side = Q.check_side(side)
    Q.resolve_scoring(model, scoring)
    with Q.eval_mode(model):
        res = rank_triples(model, h, r, t, side=side, known=known, scoring=scoring, batch_size=batch_size)
    return Q.ranking_metrics(res, ks)
