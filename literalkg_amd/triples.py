"""Explicit labelled triples under the model's own score: the score of (h, r, t), per-relation classification thresholds
fitted on a validation split, and triple-classification accuracy -- the second standard evaluation of a TransR / TransE
model (the protocol of the TransR paper), next to the ranking of ranking.py.

The score of a triple is the number every other inference entry point reports for it: score_triples returns what
predict_topk reports for that (query, candidate), bit for bit -- the squared distance fl(|q|^2 + s) with
s = |p_c|^2 - 2 q.p_c for 'transr' / 'transe' (lower is better), the dot product -s / 2 for 'dot' (higher is better);
kernel_scores=True returns s itself, the value lkg_rank_count_f32 compares.  side='tail' scores t as a candidate of the
query built from (h, r), q = P_r[h] + e_r; side='head' scores h as a candidate of q = P_r[t] - e_r.  The bits do not
depend on batch_size, on the order of the triples, or on which rows are projected together (lkg_triples.hip, DESIGN.md
section 3.6g).

Decisions are one float32 compare on the reported score: a triple is positive iff score <= thr[r] ('transr' / 'transe')
or score >= thr[r] ('dot'); a NaN score is counted in ``nan`` alone and is wrong for accuracy.  "Nothing is positive" is
the threshold -inf for distances and +inf for 'dot'.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Union

import torch

from . import _queries as Q
from . import ops
from .pairmlp import classification_metrics

PROJECT: Optional[str] = None      # 'transr' projections: None = the distinct rows when they are fewer than the entities;
#                                    'distinct' / 'full' force a route (tests run both: the choice changes no bit)


@dataclass
class TripleThresholds:
    """``thresholds`` float32[n_relations] on the model's device (a relation without a validation triple holds
    ``global_threshold``, the fit over all triples pooled), ``scoring`` the score they were fitted on, ``n`` /
    ``correct`` int64[n_relations]: the validation triples of every relation and how many of them its threshold
    classifies correctly."""
    thresholds: torch.Tensor
    global_threshold: float
    scoring: str
    n: torch.Tensor
    correct: torch.Tensor


def sentinel(scoring: str) -> float:
    """The threshold under which nothing is positive."""
    return float("-inf") if Q.lower_is_better(scoring) else float("inf")


def check_scoring(model, scoring: Optional[str]) -> str:
    scoring = Q.resolve_scoring(model, scoring, "scoring='mlp' has no triple score: the pair head scores (h, t) pairs -- "
                                "use score_pairs_mlp / evaluate_mlp_classification")
    Q.check_transr_model(model, scoring)
    return scoring


def _check_labels(labels, n: int) -> torch.Tensor:
    if not isinstance(labels, torch.Tensor):
        raise ValueError("labels must be a uint8 or bool tensor of 0 / 1")
    return ops._u8_labels("labels", labels, n)


def _groups(model, scoring: str, table: torch.Tensor, qid, cid, r, by_relation: bool):
    """A generator of (p, pn, e, q_idx, c_idx, rel, pos, relation): the table of rows the triples at positions pos index
    through q_idx / c_idx, its squared norms (None for dot), the relation embeddings (None for dot) with the triples'
    relations, and the relation the group belongs to (None: all of them).  'transr': one group per relation present,
    over P_r of the distinct rows its triples touch -- or of the whole table when those are not fewer -- a projected row
    being the same bits either way (the tall GEMM's row does not depend on the rows projected with it).  Otherwise the
    groups share the table: one per relation present with by_relation (the counts), else a single one."""
    Q.check_table_shape(model, scoring, table)
    e = Q.relation_rows(model, scoring)
    pn = ops.rank_sqnorm(table) if scoring == "transe" else None
    if scoring != "transr" and not by_relation:
        yield table, pn, e, qid, cid, r, None, None
        return
    perm, seg = ops.group_by_key(r, model.n_relations)
    perm, seg = perm.long(), seg.tolist()
    if scoring == "transr":
        w = model.gat_trans_M.detach()
        rowmax = ops.row_absmax(table)
    for rr in range(model.n_relations):
        if seg[rr + 1] == seg[rr]:
            continue
        pos = perm[seg[rr]:seg[rr + 1]]
        qi, ci, rel = qid[pos], cid[pos], r[pos]
        if scoring != "transr":
            yield table, pn, e, qi, ci, rel, pos, rr
            continue
        rows, rm, qi, ci = Q.rows_to_project(table, rowmax, qi, ci, PROJECT)
        p = ops.gemm_tall([rows], [[w[rr]]], trans_b=False, rowmax=rm)
        del rows, rm
        yield p, ops.rank_sqnorm(p), e, qi, ci, rel, pos, rr
        del p


def _scores(model, scoring, side, h, r, t, batch_size, kernel_scores=False, labels=None, thr=None):
    """(scores float32[P], counts int64[n_relations, 5] or None) of the checked, non-empty triples on the model's device
    (ids already there).  thr: one threshold per relation (a list of floats) for the counts against labels."""
    dev = h.device
    qid, cid = (h, t) if side == "tail" else (t, h)
    alpha = Q.side_alpha(side)
    n = h.numel()
    out = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.zeros((model.n_relations, 5), dtype=torch.int64, device=dev) if labels is not None else None
    with torch.no_grad():
        table = model._table_for_inference().detach()
        for p, pn, e, qi, ci, rel, pos, rr in _groups(model, scoring, table, qid, cid, r, labels is not None):
            m = qi.numel()
            sc = out if pos is None else torch.empty(m, dtype=torch.float32, device=dev)
            lab = None if labels is None else (labels if pos is None else labels[pos])
            for lo, hi in Q.batches(m, batch_size):
                ops.triple_scores(p, qi[lo:hi], ci[lo:hi], pn, e, rel[lo:hi], alpha, reported=not kernel_scores,
                                  higher_is_positive=not Q.lower_is_better(scoring),
                                  labels=None if lab is None else lab[lo:hi], thr=None if lab is None else thr[rr],
                                  out=sc[lo:hi], counts=None if lab is None else counts[rr])
            if pos is not None:
                out[pos] = sc
    return out, counts


def score_triples(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, scoring: Optional[str] = None,
                  side: str = "tail", batch_size: Optional[int] = None, kernel_scores: bool = False) -> torch.Tensor:
    """float32[P]: the score of every triple (h_i, r_i, t_i) on the model's inference table, with the bits
    predict_topk reports for that (query, candidate) on that side (see the module docstring): TopKResult.scores, or
    .kernel_scores with kernel_scores=True.  batch_size: triples per launch (None: all of a group); it changes nothing.
    The model's mode, parameters and caches are left as they are."""
    scoring = check_scoring(model, scoring)
    side = Q.check_one_side(side, "a triple is scored from one side at a time")
    Q.check_triple_lists(h, r, t)
    Q.check_batch_size(batch_size)
    dev = model.entity_embed.weight.device
    if h.numel() == 0:
        return torch.empty(0, dtype=torch.float32, device=dev)
    (h, t), r, _ = Q.ids_to_device(model, dev, (h, t), r)
    out, _ = _scores(model, scoring, side, h, r, t, batch_size, kernel_scores)
    return out


def fit_triple_thresholds(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, labels: torch.Tensor,
                          scoring: Optional[str] = None, per_relation: bool = True,
                          batch_size: Optional[int] = None) -> TripleThresholds:
    """The classification thresholds that fit the labelled validation triples best, exact, tie-aware and per relation
    (lkg_threshold_fit_f32).  Within relation rho the non-NaN scores of score_triples (tail side) are taken best first
    -- ascending for distances, descending for 'dot' -- and grouped by float equality (-0.0 == +0.0).  With TP_g / FP_g
    the cumulative label counts at the end of group g, correct(0) = n_neg and correct(g) = TP_g + n_neg - FP_g;
    thr[rho] is the score of the smallest g that maximises correct, or the sentinel (-inf / +inf: nothing is positive) if
    that g is 0.  The threshold is an OBSERVED score, not a midpoint between two scores, so every integer of the fit has
    an exact reference (a threshold of zero is returned as +0.0).  A relation without a validation triple takes
    ``global_threshold``, the same fit over all triples pooled, which per_relation=False puts everywhere.  labels: a
    uint8 or bool tensor of 0 / 1.  NaN scores are classified wrongly whatever the threshold.  Runs in eval mode and
    restores the model's previous mode."""
    scoring = check_scoring(model, scoring)
    Q.check_triple_lists(h, r, t)
    labels = _check_labels(labels, h.numel())
    Q.check_batch_size(batch_size)
    dev = model.entity_embed.weight.device
    n_rel = model.n_relations
    lower = Q.lower_is_better(scoring)
    if h.numel() == 0:
        s_ = sentinel(scoring)
        zeros = torch.zeros(n_rel, dtype=torch.int64, device=dev)
        return TripleThresholds(torch.full((n_rel,), s_, dtype=torch.float32, device=dev), s_, scoring, zeros,
                                zeros.clone())
    with Q.eval_mode(model):
        (h, t), r, _ = Q.ids_to_device(model, dev, (h, t), r)
        lab = labels.to(dev)
        scores, _ = _scores(model, scoring, "tail", h, r, t, batch_size)
        thr_g, _ = ops.threshold_fit(scores, lab, None, 1, lower)
        thr_r, stats = ops.threshold_fit(scores, lab, r, n_rel, lower)
        n = stats[:, 0].clone()
        if per_relation:
            thr = torch.where(n > 0, thr_r, thr_g.expand(n_rel))
            correct = stats[:, 2].clone()
        else:
            thr = thr_g.expand(n_rel).clone()
            pred = (scores <= thr_g) if lower else (scores >= thr_g)         # (one f32 compare; NaN compares false ...
            right = (pred == (lab != 0)) & ~torch.isnan(scores)              #  ... and is wrong either way)
            correct = torch.bincount(r[right], minlength=n_rel)
        return TripleThresholds(thr, float(thr_g.item()), scoring, n, correct)


def threshold_list(model, thresholds, scoring: str):
    """One Python float per relation from a TripleThresholds, a float or a float32[n_relations] tensor."""
    n_rel = model.n_relations
    if isinstance(thresholds, TripleThresholds):
        if thresholds.scoring != scoring:
            raise ValueError(f"the thresholds were fitted on scoring={thresholds.scoring!r}, the evaluation asks for "
                             f"{scoring!r}")
        thresholds = thresholds.thresholds
    if isinstance(thresholds, torch.Tensor):
        if thresholds.dtype != torch.float32 or thresholds.dim() != 1 or thresholds.numel() != n_rel:
            raise ValueError(f"thresholds must be a float32 tensor of {n_rel} elements (one per relation)")
        thr = thresholds.tolist()
    elif isinstance(thresholds, (int, float)) and not isinstance(thresholds, bool):
        thr = [float(torch.tensor(float(thresholds), dtype=torch.float32))] * n_rel
    else:
        raise ValueError("thresholds must be a TripleThresholds, a float or a float32 tensor [n_relations]")
    if any(x != x for x in thr):
        raise ValueError("a threshold is NaN")
    return thr


def triple_metrics(counts: torch.Tensor, n_pos: int, n_neg: int, curve=None) -> Dict:
    """The dict of evaluate_triple_classification from the per-relation counts int64[n_relations, 5] (tp, fp, tn, fn, nan
    per row), the label counts and binary_curve's six values (None: nothing was scored)."""
    counts = counts.cpu().to(torch.int64)
    tp, fp, tn, fn, nan = (int(x) for x in counts.sum(0).tolist())
    out = classification_metrics(tp, fp, tn, fn, nan, n_pos, n_neg, curve)
    per_n = counts.sum(1)
    used = per_n > 0
    acc = (counts[:, 0] + counts[:, 2])[used].double() / per_n[used].double()
    out["macro_accuracy"] = float(acc.mean()) if bool(used.any()) else 0.0
    out["per_relation"] = {name: counts[:, j].clone() for j, name in enumerate(("tp", "fp", "tn", "fn", "nan"))}
    return out


def evaluate_triple_classification(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, labels: torch.Tensor,
                                   thresholds: Union[TripleThresholds, float, torch.Tensor],
                                   scoring: Optional[str] = None, batch_size: Optional[int] = None) -> Dict:
    """Triple classification of the labelled triples under per-relation thresholds (fit_triple_thresholds, a float32
    tensor [n_relations], or one float everywhere):

        accuracy, precision, recall, f1        pairmlp.classification_metrics of the summed counts; accuracy is over all
                                               triples, so a NaN score is wrong
        macro_accuracy                         the mean of per-relation accuracy over the relations that have triples
        tp, fp, tn, fn, nan, n, n_pos, n_neg   the counts behind them; per_relation: the first five as int64[n_relations]
        roc_auc, average_precision             exact and tie-aware (ops.binary_curve) over all triples on the plausibility
                                               -- the negated distance (negation is exact) or the dot product; NaN when a
                                               class is empty

    The scores are those of score_triples (tail side), computed once for the counts (taken in the scoring kernel, one
    float32 compare each) and the curve.  labels: a uint8 or bool tensor of 0 / 1.  batch_size changes nothing.  Runs in
    eval mode and restores the model's previous mode."""
    scoring = check_scoring(model, scoring)
    Q.check_triple_lists(h, r, t)
    labels = _check_labels(labels, h.numel())
    Q.check_batch_size(batch_size)
    thr = threshold_list(model, thresholds, scoring)
    n_rel = model.n_relations
    if h.numel() == 0:
        return triple_metrics(torch.zeros((n_rel, 5), dtype=torch.int64), 0, 0)
    with Q.eval_mode(model):
        dev = model.entity_embed.weight.device
        (h, t), r, _ = Q.ids_to_device(model, dev, (h, t), r)
        lab = labels.to(dev)
        scores, counts = _scores(model, scoring, "tail", h, r, t, batch_size, labels=lab, thr=thr)
        curve = ops.binary_curve(-scores if Q.lower_is_better(scoring) else scores, lab)
        n_pos = int((lab != 0).sum())
    return triple_metrics(counts, n_pos, h.numel() - n_pos, curve)
