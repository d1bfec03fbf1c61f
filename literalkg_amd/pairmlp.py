"""The MLP pair head at inference: all-pairs logits (``mlp_scores``, the MLP counterpart of ``calc_score``), the backend
of ``predict_topk(scoring="mlp")``, filtered ranking of held-out pairs under the head (``rank_pairs_mlp``,
``evaluate_mlp_ranking``), and the head's downstream task itself: scores of an explicit list of pairs
(``score_pairs_mlp``) and their binary-classification metrics against labels (``evaluate_mlp_classification``).

The head of mode='mlp' is sigmoid(fc3(bn2(relu(fc2(bn1(relu(fc1([e_h | e_t])))))))).  At inference BatchNorm is affine per
feature, bn(x) = a x + c with a = gamma / sqrt(running_var + eps), c = beta - running_mean a, and since ReLU comes
before each BatchNorm both fold forward into the next Linear:

    u_h = W1[:, :C] e_h + b1                     v_t = W1[:, C:] e_t
    x1  = relu(u_h + v_t)
    x2  = relu(W2' x1 + b2')       W2' = W2 diag(a1),   b2' = W2 c1 + b2
    z   = w3' . x2 + b3'           w3' = w3 * a2,       b3' = w3 . c2 + b3
    p   = sigmoid(z)

fc1 separates over the two entities, so every entity is projected once (the tall GEMM) and the per-pair work -- fc2 on the
exact-f32 MFMA, fc3 in its epilogue -- runs in lkg_pairmlp.hip, which stores the logits or keeps a running filtered
top-k per query without storing them.  Everything orders by the logit z: the sigmoid is
monotone but saturates in f32.  A pair's logit has the same bits wherever it is computed: in ``mlp_scores``, in
``predict_topk`` on either side, in ``rank_pairs_mlp``, in ``score_pairs_mlp``, in any batch, split or candidate order.

BatchNorm always uses its running statistics here, whatever ``model.training`` says; the model's mode, parameters,
buffers and caches are left as they are.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from . import _queries as Q
from . import ops
from .ranking import KnownTriples, RankResult

_SIGMOID_CHUNK = 1 << 24      # elements per float64 temporary of _sigmoid_


@dataclass
class FoldedMLPHead:
    """The head with BatchNorm folded in, float32 on the model's device: w1h / w1t (128 x C, the head and tail halves of
    fc1), b1 (128), w2 (64 x 128), b2 (64), w3 (64), b3 (1)."""
    w1h: torch.Tensor
    w1t: torch.Tensor
    b1: torch.Tensor
    w2: torch.Tensor
    b2: torch.Tensor
    w3: torch.Tensor
    b3: torch.Tensor


def _bn_affine(bn, width: int, name: str):
    """(a, c) of bn(x) = a x + c in float64 from the running statistics."""
    if getattr(bn, "running_mean", None) is None or getattr(bn, "running_var", None) is None:
        raise ValueError(f"{name} keeps no running statistics (track_running_stats=False): the inference form of the "
                         "head is undefined")
    if bn.running_mean.numel() != width:
        raise ValueError(f"{name} has {bn.running_mean.numel()} features, the head needs {width}")
    one = torch.ones(width, dtype=torch.float64, device=bn.running_mean.device)
    gamma = bn.weight.detach().double() if bn.weight is not None else one
    beta = bn.bias.detach().double() if bn.bias is not None else torch.zeros_like(one)
    a = gamma / torch.sqrt(bn.running_var.detach().double() + bn.eps)
    return a, beta - bn.running_mean.detach().double() * a


def fold_mlp_head_f64(model):
    """The folded head in float64: (w1h, w1t, b1, w2, b2, w3, b3); see the module docstring."""
    for name in ("fc1", "norm1", "fc2", "norm2", "fc3"):
        if not hasattr(model, name):
            raise AttributeError("the model has no MLP head: call initialize_MLP() first")
    h1, h2 = ops.PAIR_MLP_H1, ops.PAIR_MLP_H2
    w1, w2, w3 = model.fc1.weight.detach(), model.fc2.weight.detach(), model.fc3.weight.detach()
    if w1.shape[0] != h1 or w1.shape[1] % 2 or tuple(w2.shape) != (h2, h1) or tuple(w3.shape) != (1, h2):
        raise ValueError(f"the pair-head kernels take the head 2C -> {h1} -> {h2} -> 1 that initialize_MLP builds (got fc1 "
                         f"{tuple(w1.shape)}, fc2 {tuple(w2.shape)}, fc3 {tuple(w3.shape)})")
    for lin, name in ((model.fc1, "fc1"), (model.fc2, "fc2"), (model.fc3, "fc3")):
        if lin.bias is None:
            raise ValueError(f"{name} has no bias: not the head initialize_MLP builds")
    a1, c1 = _bn_affine(model.norm1, h1, "norm1")
    a2, c2 = _bn_affine(model.norm2, h2, "norm2")
    c = w1.shape[1] // 2
    w1, w2, w3 = w1.double(), w2.double(), w3.double().reshape(-1)
    return (w1[:, :c].contiguous(), w1[:, c:].contiguous(), model.fc1.bias.detach().double(),
            w2 * a1[None, :], (w2 * c1[None, :]).sum(dim=1) + model.fc2.bias.detach().double(),
            w3 * a2, ((w3 * c2).sum() + model.fc3.bias.detach().double().reshape(())).reshape(1))


def fold_mlp_head(model) -> FoldedMLPHead:
    """The model's head with both BatchNorms (running statistics) folded forward, computed in float64 and rounded once to
    float32.  AttributeError without a head (initialize_MLP not called); ValueError for a BatchNorm without running
    statistics or a head other than 2C -> 128 -> 64 -> 1."""
    return FoldedMLPHead(*(t.to(torch.float32).contiguous() for t in fold_mlp_head_f64(model)))


def _sigmoid_(z: torch.Tensor) -> torch.Tensor:
    """sigmoid of float32 logits in place, evaluated in float64 and rounded once -- so the probability is monotone in the
    logit and within an ulp of the true value -- through temporaries of bounded size."""
    flat = z.view(-1) if z.is_contiguous() else None
    if flat is None:
        for row in z:
            _sigmoid_(row)
        return z
    for lo, hi in Q.batches(flat.numel(), _SIGMOID_CHUNK):
        part = flat[lo:hi]
        part.copy_(torch.sigmoid(part.double()))
    return z


def _table_width_ok(head: FoldedMLPHead, table: torch.Tensor):
    if table.shape[1] != head.w1h.shape[1]:
        raise ValueError(f"fc1 takes 2 x {head.w1h.shape[1]} inputs, the inference table is {table.shape[1]} wide")


def _project(rows: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rows @ w^T (+ bias): one half of fc1 over the given table rows, on the tall-GEMM engine."""
    if rows.shape[0] == 0:
        return torch.empty((0, w.shape[0]), dtype=torch.float32, device=rows.device)
    return ops.gemm_tall([rows], [[w]], trans_b=True, bias=bias)


def _project_sides(head: FoldedMLPHead, side: str, qrows: torch.Tensor, crows: torch.Tensor):
    """(uq, v) of the query rows and the candidate rows for a side.  'tail': the pairs are (query, c), so the queries take
    fc1's head half and its bias; 'head': the pairs are (c, query), so the candidates do."""
    if side == "tail":
        return _project(qrows, head.w1h, head.b1), _project(crows, head.w1t)
    return _project(qrows, head.w1t), _project(crows, head.w1h, head.b1)


def mlp_scores(model, head_ids: torch.Tensor, tail_ids: torch.Tensor, logits: bool = False) -> torch.Tensor:
    """The len(head_ids) x len(tail_ids) matrix of the head's probabilities p(h_i, t_j) -- or logits -- on the model's
    inference table: what model(h, t, mode='mlp') gives in eval mode for every pair, without forming the pairs.  Only
    the rows named are projected.  The result is one float32 tensor of the caller's choosing (rows x cols x 4 bytes)."""
    Q.check_ids("head_ids", head_ids)
    Q.check_ids("tail_ids", tail_ids)
    head = fold_mlp_head(model)
    (hid, tid), _, _ = Q.ids_to_device(model, model.entity_embed.weight.device, (head_ids, tail_ids))
    with torch.no_grad():
        table = model._table_for_inference().detach()
        _table_width_ok(head, table)
        uq = _project(ops.gather_rows(table, hid), head.w1h, head.b1)
        v = _project(ops.gather_rows(table, tid), head.w1t)
        out = ops.pair_mlp_scores(uq, v, head.w2, head.b2, head.w3, head.b3)
        return out if logits else _sigmoid_(out)


def predict_topk_mlp(model, head: FoldedMLPHead, ids, r, side, k, filt, cand, batch_size, splits):
    """predict_topk's backend for scoring='mlp' (arguments already checked and on the device): (ids, probabilities,
    logits), each B x k."""
    dev = ids.device
    b = ids.numel()
    with torch.no_grad():
        table = model._table_for_inference().detach()
        _table_width_ok(head, table)
        qrows = ops.gather_rows(table, ids)
        crows = table if cand is None else ops.gather_rows(table, cand)
        uq, v = _project_sides(head, side, qrows, crows)
        del qrows, crows
        frel = Q.filter_relations(r, b, dev)
        out_ids = torch.empty((b, k), dtype=torch.int64, device=dev)
        out_z = torch.empty((b, k), dtype=torch.float32, device=dev)
        for lo, hi in Q.batches(b, batch_size):
            ii, zz = ops.pair_mlp_topk(uq[lo:hi], v, head.w2, head.b2, head.w3, head.b3, k, filt, ids[lo:hi], frel[lo:hi],
                                       cand, splits)
            out_ids[lo:hi] = ii
            out_z[lo:hi] = zz
        return out_ids, _sigmoid_(out_z.clone()), out_z


def rank_pairs_mlp(model, h: torch.Tensor, t: torch.Tensor, r: Optional[torch.Tensor] = None, side: str = "tail",
                   known: Optional[KnownTriples] = None, candidates: Optional[torch.Tensor] = None,
                   batch_size: Optional[int] = None) -> RankResult:
    """Filtered ranks of the pairs (h, t) under the MLP pair head on the model's inference table (see the module
    docstring): side 'tail' / 'head' / 'both' (2 x B: row 0 the tail side, row 1 the head side).  r: the relation of every
    pair for the filter (None: a pair known under any relation is dropped).  candidates: optional 1-D tensor of unique
    entity ids to rank among -- every truth must be one of them; one side only.  batch_size: queries per launch (None:
    all); it does not change the result.  The model's mode, parameters, buffers and caches are left as they are."""
    side = Q.check_side(side)
    _check_pairs(h, t)
    if r is not None:
        Q.check_ids("r", r)
        if r.numel() != h.numel():
            raise ValueError(f"h and r have different lengths ({h.numel()}, {r.numel()})")
    if candidates is not None:
        Q.check_ids("candidates", candidates)
        if side == "both":
            raise ValueError("candidates go with side='tail' or side='head': the two sides of 'both' would need two sets")
        Q.check_unique(candidates)
        truth = t if side == "tail" else h
        missing = int((~torch.isin(truth.to(candidates.device), candidates)).sum())
        if missing:
            raise ValueError(f"{missing} of the {truth.numel()} true {'tails' if side == 'tail' else 'heads'} are not among "
                             "the candidates")
    Q.check_batch_size(batch_size)
    Q.check_known_entities(known, model)
    head = fold_mlp_head(model)                          # (AttributeError without initialize_MLP)
    dev = model.entity_embed.weight.device
    Q.check_known_device(known, dev)
    b = h.numel()
    better, equal = Q.count_buffers(side, b, dev)
    if b == 0:
        return Q.rank_result(better, equal, side)
    (h, t), r, cand = Q.ids_to_device(model, dev, (h, t), r, candidates)
    with torch.no_grad():
        table = model._table_for_inference().detach()
        _table_width_ok(head, table)
        crows = table if cand is None else ops.gather_rows(table, cand)
        slot = ops.pair_mlp_cand_slot(model.n_entities, cand) if cand is not None else None
        frel = Q.filter_relations(r, b, dev)
        for j, s_ in enumerate(Q.rank_sides(side)):
            q_ids, truth = (h, t) if s_ == "tail" else (t, h)
            uq, v = _project_sides(head, s_, ops.gather_rows(table, q_ids), crows)
            filt = known.for_side(s_) if known is not None else None
            truth_rows = truth if slot is None else slot[truth].long()
            for lo, hi in Q.batches(b, batch_size):
                bb, ee, _ = ops.pair_mlp_rank_count(uq[lo:hi], v, head.w2, head.b2, head.w3, head.b3, truth_rows[lo:hi],
                                                    filt, q_ids[lo:hi], frel[lo:hi], cand, slot)
                better[j, lo:hi] = bb
                equal[j, lo:hi] = ee
            del uq, v
    return Q.rank_result(better, equal, side)


def evaluate_mlp_ranking(model, h: torch.Tensor, t: torch.Tensor, r: Optional[torch.Tensor] = None,
                         known: Optional[KnownTriples] = None, ks: Sequence[int] = (1, 3, 10), side: str = "both",
                         candidates: Optional[torch.Tensor] = None, batch_size: Optional[int] = None) -> Dict:
    """{'mr', 'mrr', 'hits@k'..., 'n', 'tail': {...}, 'head': {...}}: filtered ranking metrics of the pairs under the MLP
    pair head (rank_pairs_mlp, ranking.metrics_from_counts); the top level is over every rank computed (2B for
    side='both').  Runs in eval mode, as evaluate_ranking does, and restores the model's previous mode."""
    ks = Q.check_ks(ks)
    side = Q.check_side(side)
    with Q.eval_mode(model):
        res = rank_pairs_mlp(model, h, t, r=r, side=side, known=known, candidates=candidates, batch_size=batch_size)
    return Q.ranking_metrics(res, ks)


# ----------------------------------------------------------------------------- explicit pairs and their classification
def _check_pairs(h, t):
    Q.check_ids("h", h)
    Q.check_ids("t", t)
    if h.numel() != t.numel():
        raise ValueError(f"h and t have different lengths ({h.numel()}, {t.numel()})")


def _pair_side(table: torch.Tensor, ids: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor],
               unique: Optional[bool] = None):
    """(rows, idx): one half of fc1 for a list of checked entity ids -- projected over the unique ids, idx the row of
    every pair, when those are fewer than the pairs; else over the gathered rows, idx None ("pair i uses row i").  A
    projected row does not depend on which rows are projected with it, so the choice (unique: None = by the counts,
    True / False force a route) does not change a bit."""
    uniq, inv = (None, None) if unique is False else torch.unique(ids, return_inverse=True)
    if unique is None:
        unique = uniq.numel() < ids.numel()
    if unique:
        return _project(ops.gather_rows(table, uniq), w, bias), inv
    return _project(ops.gather_rows(table, ids), w, bias), None


def _pair_logits(model, head: FoldedMLPHead, h, t, batch_size, labels=None, thr=None):
    """(logits float32[P], counts int64[5] or None) of the checked-for-shape, non-empty pair list on the model's device"""
    dev = model.entity_embed.weight.device
    (hid, tid), _, _ = Q.ids_to_device(model, dev, (h, t))
    p = hid.numel()
    with torch.no_grad():
        table = model._table_for_inference().detach()
        _table_width_ok(head, table)
        u, u_idx = _pair_side(table, hid, head.w1h, head.b1)
        v, v_idx = _pair_side(table, tid, head.w1t, None)
        z = torch.empty(p, dtype=torch.float32, device=dev)
        counts = torch.zeros(5, dtype=torch.int64, device=dev) if labels is not None else None
        for lo, hi in Q.batches(p, batch_size):
            ops.pair_mlp_pairs(u if u_idx is not None else u[lo:hi], v if v_idx is not None else v[lo:hi], head.w2,
                               head.b2, head.w3, head.b3, u_idx[lo:hi] if u_idx is not None else None,
                               v_idx[lo:hi] if v_idx is not None else None,
                               labels[lo:hi] if labels is not None else None, thr, True, z[lo:hi], counts)
    return z, counts


def score_pairs_mlp(model, h: torch.Tensor, t: torch.Tensor, logits: bool = False,
                    batch_size: Optional[int] = None) -> torch.Tensor:
    """float32[P]: the head's probability -- or logit -- of every pair (h_i, t_i) on the model's inference table: what
    model(h, t, mode='mlp') gives in eval mode, through the folded head (see the module docstring), each logit with the
    bits mlp_scores gives that pair.  Every distinct entity is projected once.  batch_size: pairs per launch (None: all);
    it does not change the result.  BatchNorm is in inference form whatever model.training says; the model's mode,
    parameters, buffers and caches are left as they are."""
    _check_pairs(h, t)
    Q.check_batch_size(batch_size)
    head = fold_mlp_head(model)                          # (AttributeError without initialize_MLP)
    if h.numel() == 0:
        return torch.empty(0, dtype=torch.float32, device=model.entity_embed.weight.device)
    z, _ = _pair_logits(model, head, h, t, batch_size)
    return z if logits else _sigmoid_(z)


def logit_of_probability(p: float) -> float:
    """float32(log(p / (1 - p))) formed in float64, as a Python float: the logit threshold of a probability threshold
    strictly inside (0, 1).  0.5 is the logit 0.0 exactly."""
    p = float(p)
    if not 0.0 < p < 1.0:
        raise ValueError(f"threshold must be a probability strictly inside (0, 1), got {p!r}")
    return float(torch.tensor(math.log(p / (1.0 - p)), dtype=torch.float64).to(torch.float32))


def classification_metrics(tp: int, fp: int, tn: int, fn: int, nan: int, n_pos: int, n_neg: int,
                           curve=None) -> Dict:
    """The dict of evaluate_mlp_classification from the confusion counts, the label counts and binary_curve's six
    values (None: no pair was scored).  accuracy, precision, recall and f1 follow the reference's utils/metric_utils.py:
    accuracy over ALL pairs (a NaN prediction is wrong), precision / recall 0 with an empty denominator, f1 0 when both
    are 0."""
    n = tp + fp + tn + fn + nan
    precision = tp / (tp + fp) if tp + fp else 0.0
    recall = tp / (tp + fn) if tp + fn else 0.0
    f1 = (2.0 * precision * recall) / (precision + recall) if precision + recall > 0 else 0.0
    roc_auc = average_precision = float("nan")
    if curve is not None:
        c_pos, c_neg, _, _, auc2, ap = curve
        if c_pos > 0 and c_neg > 0:
            roc_auc, average_precision = auc2 / (2 * c_pos * c_neg), ap
    return {"accuracy": (tp + tn) / n if n else 0.0, "precision": precision, "recall": recall, "f1": f1,
            "tp": tp, "fp": fp, "tn": tn, "fn": fn, "nan": nan, "n": n, "n_pos": n_pos, "n_neg": n_neg,
            "roc_auc": roc_auc, "average_precision": average_precision}


def _check_labels(labels, n):
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.is_complex():
        raise ValueError("labels must be a 1-D bool, integer or float tensor of 0 / 1")
    if labels.numel() != n:
        raise ValueError(f"h and labels have different lengths ({n}, {labels.numel()})")
    if labels.dtype != torch.bool and not bool(((labels == 0) | (labels == 1)).all()):
        raise ValueError("labels must be 0 or 1")


def evaluate_mlp_classification(model, h: torch.Tensor, t: torch.Tensor, labels: torch.Tensor, threshold: float = 0.5,
                                logit_threshold: Optional[float] = None, batch_size: Optional[int] = None) -> Dict:
    """Binary classification of the labelled pairs (h_i, t_i) under the MLP pair head, the reference's downstream
    evaluation (utils/model_utils.py:133-158) with its baselines' curve metrics:

        accuracy, precision, recall, f1        the formulas and zero conventions of utils/metric_utils.py; accuracy is
                                               over all pairs, so a NaN prediction is wrong
        tp, fp, tn, fn, nan, n, n_pos, n_neg   the counts behind them (nan: pairs whose logit is NaN; n_pos / n_neg: the
                                               labels, n = n_pos + n_neg = tp + fp + tn + fn + nan)
        roc_auc, average_precision             exact and tie-aware over the pairs whose logit is not NaN (tied scores
                                               count as halves; average precision is the step-function sum, not the
                                               trapezoid); NaN when either class is empty among them

    labels: a 1-D bool, integer or float tensor of 0 / 1.  threshold: a probability strictly inside (0, 1), applied on
    the logit as float32(log(p / (1 - p))) formed in float64 (0.5 is the logit 0.0 exactly); logit_threshold overrides
    it (any float but NaN).  A pair is positive iff its logit > that threshold.  The logits are those of
    score_pairs_mlp, computed once for the counts (taken in the scoring kernel) and the curve (lkg_binary_curve_f32).
    batch_size: pairs per launch; it changes nothing.  Runs in eval mode and restores the model's previous mode.

    One deliberate difference from the reference: decisions are taken on the logit, where the reference rounds the float32
    probability.  sigmoid(z) rounds to exactly 0.5 in float32 for 0 < z < ~6e-8, which .round() sends to 0; here such a
    pair is positive."""
    _check_pairs(h, t)
    _check_labels(labels, h.numel())
    Q.check_batch_size(batch_size)
    if logit_threshold is None:
        thr = logit_of_probability(threshold)
    else:
        thr = float(logit_threshold)
        if thr != thr:
            raise ValueError("logit_threshold is NaN")
    head = fold_mlp_head(model)                          # (AttributeError without initialize_MLP)
    with Q.eval_mode(model):
        if h.numel() == 0:
            return classification_metrics(0, 0, 0, 0, 0, 0, 0)
        dev = model.entity_embed.weight.device
        lab = (labels != 0).to(dev).view(torch.uint8)
        z, counts = _pair_logits(model, head, h, t, batch_size, lab, thr)
        curve = ops.binary_curve(z, lab)
        tp, fp, tn, fn, nan = (int(x) for x in counts.tolist())
        n_pos = int(lab.sum())
    return classification_metrics(tp, fp, tn, fn, nan, n_pos, h.numel() - n_pos, curve)
