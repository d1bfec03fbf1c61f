"""Relation prediction: the relation slot of (h, ?, t) under the model's own score -- the score of a pair of entities
under every relation, the filtered rank of the true relation, the most likely relations that are not already known, and
MR / MRR / Hits@k of the true relation among all relations, overall and per relation (the third standard KG-completion
evaluation, next to ranking.py and triples.py).

score_relations(...)[i, j] is the number score_triples reports for (h_i, j, t_i) on that side, bit for bit: the squared
distance fl(|q|^2 + s) with s = |p_c|^2 - 2 q.p_c, where side='tail' scores t as a candidate of q = P_j[h] + e_j and
side='head' scores h as a candidate of q = P_j[t] - e_j ('transr': P_j = T W_j; 'transe': the table itself).  The bits do
not depend on batch_size, on relation_chunk, on the order of the pairs or on which rows are projected together
(lkg_relations.hip).  The order over relations is always taken on this reported float32 score:
|q|^2 differs between relations, so the kernel score s alone is not comparable across them.

Lower is better.  Ties go to the smaller relation id in predict_relations and count as half in rank_relations
(rank = 1 + better + equal / 2).  A NaN score is never selected and counts nowhere; a NaN truth compares false everywhere
(better = equal = 0).  With ``known`` (a ranking.KnownTriples), rank_relations drops every relation r' != r_i for which
(h_i, r', t_i) is known -- the truth is never dropped and never compared with itself -- and predict_relations drops every
known relation of (h_i, t_i); nothing is exempt there, as in predict_topk.

'dot' does not depend on the relation and the MLP pair head scores pairs, not triples: both are refused.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from . import _queries as Q
from . import ops
from . import triples as T
from .ranking import KnownTriples

PROJECT: Optional[str] = None      # 'transr' projections, as triples.PROJECT: None = the distinct rows of a batch when they
#                                    are fewer than the entities; 'distinct' / 'full' force a route (the choice changes no bit)


@dataclass
class RelationTopK:
    """P x k per pair, best first: ``ids`` (int64 relation ids, -1 where fewer than k relations are eligible) and
    ``scores`` (float32 reported scores, non-decreasing along the list, NaN where ids == -1)."""
    ids: torch.Tensor
    scores: torch.Tensor
    side: str


def _check_scoring(model, scoring: Optional[str]) -> str:
    if (scoring if scoring is not None else model.scoring) == "dot":
        raise ValueError("scoring='dot' has no relation prediction: the dot product does not depend on the relation")
    return T.check_scoring(model, scoring)


def _check_pairs(h, t, r=None):
    Q.check_ids("h", h)
    if r is not None:
        Q.check_ids("r", r)
    Q.check_ids("t", t)
    if h.numel() != t.numel() or (r is not None and r.numel() != h.numel()):
        lens = (h.numel(), t.numel()) if r is None else (h.numel(), r.numel(), t.numel())
        raise ValueError(f"{'h, t' if r is None else 'h, r, t'} have different lengths {lens}")


def _check_chunk(relation_chunk):
    if relation_chunk is not None and (isinstance(relation_chunk, bool) or int(relation_chunk) != relation_chunk
                                       or relation_chunk <= 0):
        raise ValueError(f"relation_chunk must be a positive integer, got {relation_chunk!r}")


def _check_n_relations(model):
    if model.n_relations > ops.RELATION_MAX:
        raise ValueError(f"the model has {model.n_relations} relations, relation prediction takes at most "
                         f"{ops.RELATION_MAX}: lkg_relation_order_f32 stages a pair's scores of every relation in LDS, "
                         f"four pairs per workgroup in its 64 KB")


def _check_known(known, model):
    if known is None:
        return
    if known.n_relations != model.n_relations:
        raise ValueError(f"known triples over {known.n_relations} relations, the model has {model.n_relations}")
    Q.check_known_entities(known, model)


def _check_common(model, scoring, side, h, t, r, known, batch_size, relation_chunk):
    """Every argument check that needs no device; (scoring, side)."""
    scoring = _check_scoring(model, scoring)
    side = Q.check_one_side(side, "a triple is scored from one side at a time")
    _check_pairs(h, t, r)
    Q.check_batch_size(batch_size)
    _check_chunk(relation_chunk)
    _check_n_relations(model)
    _check_known(known, model)
    return scoring, side


def _default_sizes(n_pairs: int, n_rel: int, k: int, batch_size, relation_chunk):
    """(pairs per batch, relations per chunk) of the 'transr' route: given values as they are; else the largest whose slab
    -- chunk x distinct rows (at most two per pair) x padded k x 4 bytes -- stays within ops.RELATION_WORKSPACE_BYTES."""
    row_bytes = 4 * ((k + 3) // 4 * 4)
    budget_rows = max(ops.RELATION_WORKSPACE_BYTES // row_bytes, 2)           # slab rows in all: chunk x distinct rows
    if batch_size is None:
        batch_size = max(1, min(n_pairs, budget_rows // 2))
    if relation_chunk is None:
        relation_chunk = max(1, min(n_rel, budget_rows // (2 * int(batch_size))))
    return int(batch_size), int(relation_chunk)


def _scan(model, scoring: str, side: str, h, t, batch_size, relation_chunk) -> torch.Tensor:
    """float32[P, n_relations] of the checked, non-empty pairs on the model's device (ids already there)."""
    dev = h.device
    qid, cid = (h, t) if side == "tail" else (t, h)
    alpha = Q.side_alpha(side)                           # q = P_j[h] + e_j  /  q = P_j[t] - e_j
    n, n_rel = h.numel(), model.n_relations
    out = torch.empty((n, n_rel), dtype=torch.float32, device=dev)
    with torch.no_grad():
        table = model._table_for_inference().detach()
        Q.check_table_shape(model, scoring, table)
        e = Q.relation_rows(model, scoring)
        if scoring == "transe":
            pn = ops.rank_sqnorm(table)
            chunk = n_rel if relation_chunk is None else int(relation_chunk)
            for lo, hi in Q.batches(n, batch_size):
                for r0 in range(0, n_rel, chunk):
                    r1 = min(r0 + chunk, n_rel)
                    ops.relation_scores(table, pn, qid[lo:hi], cid[lo:hi], e[r0:r1], alpha, out=out[lo:hi, r0:r1])
            return out
        w = model.gat_trans_M.detach()
        k = w.shape[2]
        kp = (k + 3) // 4 * 4                            # rows of the slab start 16 bytes apart: the kernel's float4 loads
        batch, chunk = _default_sizes(n, n_rel, k, batch_size, relation_chunk)
        rowmax = ops.row_absmax(table)
        for lo, hi in Q.batches(n, batch):
            rows, rm, qi, ci = Q.rows_to_project(table, rowmax, qid[lo:hi], cid[lo:hi], PROJECT)   # once per pair batch
            n_rows = rows.shape[0]
            for r0 in range(0, n_rel, chunk):
                r1 = min(r0 + chunk, n_rel)
                slab = torch.empty((r1 - r0, n_rows, kp), dtype=torch.float32, device=dev)[:, :, :k]
                pn = torch.empty((r1 - r0, n_rows), dtype=torch.float32, device=dev)
                for j in range(r0, r1):
                    ops.gemm_tall([rows], [[w[j]]], trans_b=False, out=slab[j - r0], rowmax=rm)
                    pn[j - r0] = ops.rank_sqnorm(slab[j - r0])
                ops.relation_scores(slab, pn, qi, ci, e[r0:r1], alpha, out=out[lo:hi, r0:r1])
                del slab, pn
    return out


def _prepare(model, h, t, r, known):
    """The ids on the model's device (checked), and the filter's device checked."""
    dev = model.entity_embed.weight.device
    Q.check_known_device(known, dev)
    (h, t), r, _ = Q.ids_to_device(model, dev, (h, t), r)
    return dev, h, t, r


def score_relations(model, h: torch.Tensor, t: torch.Tensor, scoring: Optional[str] = None, side: str = "tail",
                    batch_size: Optional[int] = None, relation_chunk: Optional[int] = None) -> torch.Tensor:
    """float32[P, n_relations]: s[i, j] is the score of (h_i, j, t_i) on the model's inference table, with the bits
    score_triples(model, h, full(j), t, side=side) returns for pair i (see the module docstring); every relation of a
    chunk is scored in one launch.  batch_size: pairs per launch; relation_chunk: relations per launch (None: as many as
    the workspace bound ops.RELATION_WORKSPACE_BYTES allows).  Neither changes a bit of the result.  The model's mode,
    parameters and caches are left as they are."""
    scoring, side = _check_common(model, scoring, side, h, t, None, None, batch_size, relation_chunk)
    dev = model.entity_embed.weight.device
    if h.numel() == 0:
        return torch.empty((0, model.n_relations), dtype=torch.float32, device=dev)
    dev, h, t, _ = _prepare(model, h, t, None, None)
    return _scan(model, scoring, side, h, t, batch_size, relation_chunk)


def rank_relations(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, known: Optional[KnownTriples] = None,
                   scoring: Optional[str] = None, side: str = "tail", batch_size: Optional[int] = None,
                   relation_chunk: Optional[int] = None) -> Q.RankResult:
    """The filtered rank of the true relation r_i among all relations of (h_i, ?, t_i): a RankResult for one side with
    better / equal int64[P] -- the relations r' != r_i, not known for (h_i, t_i), whose score_relations score is lower
    than / equal to the truth's -- and rank = 1 + better + equal / 2.  The counting runs on the device
    (lkg_relation_order_f32).  The model's mode is left as it is (evaluate_relation_prediction switches to eval)."""
    scoring, side = _check_common(model, scoring, side, h, t, r, known, batch_size, relation_chunk)
    dev = model.entity_embed.weight.device
    better, equal = Q.count_buffers(side, h.numel(), dev)
    if h.numel() == 0:
        return Q.rank_result(better, equal, side)
    dev, h, t, r = _prepare(model, h, t, r, known)
    scores = _scan(model, scoring, side, h, t, batch_size, relation_chunk)
    filt = known.by_head if known is not None else None              # (h, r', t): heads with their tails, on either side
    better[0], equal[0], _, _ = ops.relation_order(scores, truth=r, filt=filt, filter_row=h, filter_col=t)
    return Q.rank_result(better, equal, side)


def predict_relations(model, h: torch.Tensor, t: torch.Tensor, k: int = 1, known: Optional[KnownTriples] = None,
                      scoring: Optional[str] = None, side: str = "tail", batch_size: Optional[int] = None,
                      relation_chunk: Optional[int] = None) -> RelationTopK:
    """The k most likely relations of every pair (h_i, t_i) that are not already known for it: a RelationTopK, best
    (lowest score) first, ties to the smaller relation id, a NaN score never listed; rows with fewer than k eligible
    relations are padded with -1 / NaN.  k in [1, ops.TOPK_MAX].  The model's mode, parameters and caches are left as
    they are."""
    k = Q.check_k(k)
    scoring, side = _check_common(model, scoring, side, h, t, None, known, batch_size, relation_chunk)
    dev = model.entity_embed.weight.device
    if h.numel() == 0:
        return RelationTopK(torch.full((0, k), -1, dtype=torch.int64, device=dev),
                            torch.zeros((0, k), dtype=torch.float32, device=dev), side)
    dev, h, t, _ = _prepare(model, h, t, None, known)
    scores = _scan(model, scoring, side, h, t, batch_size, relation_chunk)
    filt = known.by_head if known is not None else None
    _, _, ids, top = ops.relation_order(scores, filt=filt, filter_row=h, filter_col=t, top_k=k)
    return RelationTopK(ids, top, side)


def relation_metrics(better: torch.Tensor, equal: torch.Tensor, r: torch.Tensor, n_relations: int,
                     ks: Sequence[int] = (1, 3, 10)) -> Dict:
    """The dict of evaluate_relation_prediction from the counts and the true relations: Q.metrics_from_counts overall,
    and under 'per_relation' n int64[R] with mr / mrr / hits@k float64[R] over the pairs whose truth is that relation
    (NaN where n == 0)."""
    ks = Q.check_ks(ks)
    better, equal, r = better.cpu().reshape(-1), equal.cpu().reshape(-1), r.cpu().reshape(-1).long()
    out = Q.metrics_from_counts(better, equal, ks)
    rank = Q.realistic_rank(better, equal)
    n = torch.bincount(r, minlength=n_relations)[:n_relations]
    cnt = n.double()

    def mean_by_relation(x):
        s = torch.zeros(n_relations, dtype=torch.float64).index_add_(0, r, x)
        return torch.where(n > 0, s / cnt, torch.full_like(s, float("nan")))

    per = {"n": n, "mr": mean_by_relation(rank), "mrr": mean_by_relation(1.0 / rank)}
    for k in ks:
        per[f"hits@{k}"] = mean_by_relation((rank <= k).double())
    out["per_relation"] = per
    return out


def evaluate_relation_prediction(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor,
                                 known: Optional[KnownTriples] = None, ks: Sequence[int] = (1, 3, 10),
                                 scoring: Optional[str] = None, batch_size: Optional[int] = None) -> Dict:
    """{'mr', 'mrr', 'hits@k'..., 'n', 'per_relation': {'n': int64[R], 'mr', 'mrr', 'hits@k': float64[R]}}: the filtered
    ranking metrics of the true relations (rank_relations, tail side), overall and over the pairs of every true relation
    (NaN where it has none).  Runs in eval mode and restores the model's previous mode."""
    ks = Q.check_ks(ks)
    _check_common(model, scoring, "tail", h, t, r, known, batch_size, None)
    with Q.eval_mode(model):
        res = rank_relations(model, h, r, t, known=known, scoring=scoring, batch_size=batch_size)
    return relation_metrics(res.better, res.equal, r, model.n_relations, ks)
