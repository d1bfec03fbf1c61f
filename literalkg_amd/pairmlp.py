"""The MLP pair head at inference: all-pairs logits (``mlp_scores``, the MLP counterpart of ``calc_score``), the backend
of ``predict_topk(scoring="mlp")``, filtered ranking of held-out pairs under the head (``rank_pairs_mlp``,
``evaluate_mlp_ranking``), and the head's downstream task itself: scores of an explicit list of pairs
(``score_pairs_mlp``) and their binary-classification metrics against labels (``evaluate_mlp_classification``), and the
retrieval side of that decision: every pair the head accepts, per query (``predict_accepted_mlp``,
``count_accepted_mlp``).

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


# ----------------------------------------------------------------------------- threshold retrieval under the head
_ACCEPT_BUFFER = 1 << 22      # entries of the one-pass buffer (12 bytes each): a memory choice, not a measured optimum


def _check_cap(name: str, x) -> int:
    if isinstance(x, bool) or not isinstance(x, int) or x < 0:
        raise ValueError(f"{name} must be a non-negative integer, got {x!r}")
    return x


def _logit_thresholds(threshold, logit_threshold, b: int):
    """The per-query logit thresholds as given: a Python float, or the caller's float32[B] tensor."""
    if logit_threshold is None:
        return logit_of_probability(threshold)
    if isinstance(logit_threshold, torch.Tensor):
        if logit_threshold.dtype != torch.float32 or logit_threshold.dim() != 1 or logit_threshold.numel() != b:
            raise ValueError(f"a tensor logit_threshold must be a float32 tensor of {b} elements (one per query), got "
                             f"{logit_threshold.dtype} {tuple(logit_threshold.shape)}")
        return logit_threshold
    thr = float(logit_threshold)
    if thr != thr:
        raise ValueError("logit_threshold is NaN")
    return thr


def _accept_front(model, ids, r, threshold, logit_threshold, side, known, candidates, batch_size, splits):
    """The argument checks predict_topk(scoring='mlp') makes, through the same functions in the same order, then the
    thresholds; everything before any device work.  (side, folded head, thresholds, device)."""
    side = Q.check_one_side(side, "top-k ranks one side at a time")
    Q.check_query_lists(ids, r, "mlp")
    if candidates is not None:
        Q.check_ids("candidates", candidates)
    Q.check_batch_size(batch_size)
    Q.check_splits(splits)
    Q.check_known_entities(known, model)
    Q.check_unique(candidates)
    head = fold_mlp_head(model)                          # (AttributeError without initialize_MLP)
    dev = model.entity_embed.weight.device
    Q.check_known_device(known, dev)
    return side, head, _logit_thresholds(threshold, logit_threshold, ids.numel()), dev


def _accept_run(model, head: FoldedMLPHead, ids, r, thr, side, known, cand, batch_size, splits, max_total, buffer):
    """(counts int64[B], chunks, total) of the checked queries (ids on the device).  With max_total None only the count
    kernel runs.  Otherwise chunks holds per query batch (ids, logits), every row in order and the rows in query order:
    from the one-pass buffer where the batch's entries fit it, else from the emit pass into counted segments."""
    dev, b = ids.device, ids.numel()
    filt = known.for_side(side) if known is not None else None
    if isinstance(thr, torch.Tensor):
        thr_q = thr.to(dev).contiguous()
    else:
        thr_q = torch.full((b,), thr, dtype=torch.float32, device=dev)
    counts = torch.zeros(b, dtype=torch.int64, device=dev)
    chunks, total = [], 0
    with torch.no_grad():
        table = model._table_for_inference().detach()
        _table_width_ok(head, table)
        qrows = ops.gather_rows(table, ids)
        crows = table if cand is None else ops.gather_rows(table, cand)
        uq, v = _project_sides(head, side, qrows, crows)
        del qrows, crows
        frel = Q.filter_relations(r, b, dev)
        n_c = v.shape[0]
        for lo, hi in Q.batches(b, batch_size):
            args = (uq[lo:hi], v, head.w2, head.b2, head.w3, head.b3, thr_q[lo:hi])
            kw = dict(filt=filt, filter_row=ids[lo:hi], filter_rel=frel[lo:hi], cand_ids=cand, splits=splits)
            if max_total is None:
                counts[lo:hi] = ops.pair_mlp_accept_count(*args, **kw)
                continue
            cap = min(buffer, (hi - lo) * n_c)           # (no batch has more entries than pairs)
            if cap > 0:
                cnt, rows, ii, zz, n_w = ops.pair_mlp_accept_append(*args, **kw, capacity=cap)
                m = n_w if n_w < cap else int(cnt.sum(dtype=torch.int64))
            else:
                cnt = ops.pair_mlp_accept_count(*args, **kw)
                m = int(cnt.sum(dtype=torch.int64))
            total += m
            counts[lo:hi] = cnt
            if total > max_total:
                raise ValueError(f"more than max_total={max_total} accepted pairs: {total} so far (raise max_total, "
                                 "tighten the threshold, or ask count_accepted_mlp for the sizes)")
            if cap > 0 and m <= cap:                     # one pass: the buffer holds every entry; group them by row
                order = torch.argsort(rows[:m], stable=True)
                ii, zz = ii[:m][order].long(), zz[:m][order]
                rowptr = torch.zeros(hi - lo + 1, dtype=torch.int64, device=dev)
                torch.cumsum(cnt, 0, out=rowptr[1:])
                ss = -2.0 * zz                           # (exact) the ascending key, as the select kernel feeds the merge
            else:                                        # overflow, or no buffer: the second pass into counted segments
                rowptr, ii, ss, zz = ops.pair_mlp_accept_emit(*args, **kw, counts=cnt, total=m)
            ii, ss, zz = ops.accept_order(rowptr, ii, ss, zz, model.n_entities)
            chunks.append((ii, zz))
    return counts, chunks, total


def predict_accepted_mlp(model, ids: torch.Tensor, r: Optional[torch.Tensor] = None, threshold: float = 0.5,
                         logit_threshold=None, side: str = "tail", known: Optional[KnownTriples] = None,
                         candidates: Optional[torch.Tensor] = None, batch_size: Optional[int] = None, splits: int = 0,
                         max_total: int = 1 << 26, buffer: int = _ACCEPT_BUFFER):
    """Every pair the MLP pair head accepts, per query, in CSR form (accepted.AcceptedResult): the sparse form of the
    reference's mode='predict' under the head.

    Queries, sides, r, known and candidates are exactly those of predict_topk(scoring='mlp'): side 'tail' scores the
    pairs (query, c), side 'head' the pairs (c, query); r=None drops a candidate known with the query under ANY relation,
    r given only one known under that relation; nothing is exempt; candidates are unique entity ids and any order of them
    gives the same result.

    Candidate c of query i is accepted iff its logit z(i, c) -- the bits mlp_scores(..., logits=True) gives that pair --
    passes ONE float32 compare, z > thr_i, strictly (the decision of evaluate_mlp_classification), it is not dropped by
    ``known``, and it is among ``candidates`` when those are given.  A NaN logit is never accepted.  threshold is a
    probability strictly inside (0, 1), turned into a logit by logit_of_probability (0.5 is the logit 0.0 exactly);
    logit_threshold overrides it: a Python float, or a float32 tensor of B per-query logit thresholds.  +inf accepts
    nothing; -inf accepts every candidate whose logit is neither NaN nor -inf.

    Every list is ordered as predict_topk(scoring='mlp') orders: descending logit by float comparison (-0.0 == +0.0),
    then ascending entity id -- so a query's list is a prefix of its unbounded top-k list.  ``ids`` int64, ``scores``
    float32 probabilities (the float64 sigmoid of the logit rounded once, the bits of TopKResult.scores),
    ``kernel_scores`` float32 logits (the bits of TopKResult.kernel_scores); rowptr, counts, side, query_ids, r as in
    predict_accepted; pairs() gives the (h, t) lists.  The result is a unique object: it does not depend on batch_size,
    splits, buffer, the order of queries or candidates, the stream or the contents of any scratch; duplicate queries get
    equal lists.

    max_total caps the number of entries M as in predict_accepted: ValueError once the running total of the counts
    exceeds it, and the full-size outputs are allocated only after the counts are known.  buffer: the entries of the
    one-pass buffer (12 bytes each).  A query batch whose accepted entries fit it is scored ONCE (count and append in one
    kernel, lkg_pair_mlp_accept_append_f32); one that overflows it is scored a second time into counted segments
    (lkg_pair_mlp_accept_emit_f32); buffer=0 always takes the two passes.  BatchNorm enters in inference form whatever
    model.training says; the model's mode, parameters, buffers and caches are left as they are."""
    from .accepted import AcceptedResult, _empty
    side, head, thr, dev = _accept_front(model, ids, r, threshold, logit_threshold, side, known, candidates, batch_size,
                                         splits)
    buffer = min(_check_cap("buffer", buffer), 2 ** 31 - 2)
    max_total = _check_cap("max_total", max_total)
    b = ids.numel()
    if b == 0:
        return _empty(side, dev, ids, r)
    (ids,), r, cand = Q.ids_to_device(model, dev, (ids,), r, candidates, unique=True)
    counts, chunks, total = _accept_run(model, head, ids, r, thr, side, known, cand, batch_size, splits, max_total, buffer)
    rowptr = torch.zeros(b + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=rowptr[1:])
    if chunks:
        out_ids, out_z = torch.cat([c[0] for c in chunks]), torch.cat([c[1] for c in chunks])
    else:
        out_ids = torch.empty(0, dtype=torch.int64, device=dev)
        out_z = torch.empty(0, dtype=torch.float32, device=dev)
    return AcceptedResult(rowptr, out_ids, _sigmoid_(out_z.clone()), out_z, counts, side, ids, r)


def count_accepted_mlp(model, ids: torch.Tensor, r: Optional[torch.Tensor] = None, threshold: float = 0.5,
                       logit_threshold=None, side: str = "tail", known: Optional[KnownTriples] = None,
                       candidates: Optional[torch.Tensor] = None, batch_size: Optional[int] = None,
                       splits: int = 0) -> torch.Tensor:
    """int64[B]: the length of every list predict_accepted_mlp would return, from the count kernel alone
    (lkg_pair_mlp_accept_count_f32) -- there is no cap and nothing of the size of the lists is allocated."""
    side, head, thr, dev = _accept_front(model, ids, r, threshold, logit_threshold, side, known, candidates, batch_size,
                                         splits)
    if ids.numel() == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    (ids,), r, cand = Q.ids_to_device(model, dev, (ids,), r, candidates, unique=True)
    return _accept_run(model, head, ids, r, thr, side, known, cand, batch_size, splits, None, 0)[0]
