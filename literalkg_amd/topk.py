"""Filtered top-k link prediction: the k most likely tails of (h, r, ?) -- or heads of (?, r, t) -- that are not already
known, under the model's own scoring function.

side='tail': ``ids`` are heads and the tails are ranked; side='head': ``ids`` are tails and the heads are ranked.  The
queries are those of ranking.py: q = P_r[h] + e_r / q = P_r[t] - e_r ('transr', P_r = T W_r), the same without W_r
('transe'), T[id] ('dot').  Candidates are ordered by the kernel score s_c = |p_c|^2 - 2 q.p_c (dot: -2 q.p_c), the
value lkg_rank_count_f32 compares: ascending s is best first, ties go to the smaller entity id, a NaN score is never
selected.  The reported score is the squared distance fl(|q|^2 + s) for 'transr' / 'transe' (non-decreasing along the
list) and the dot product q.p = -s / 2 for 'dot' (exact, non-increasing).  A candidate c is dropped when (query, r, c)
-- tail side -- or (c, r, query) -- head side -- is in ``known``; nothing is exempt.  With scoring='dot', r may be None:
a pair known under any relation is dropped then.

scoring='mlp' ranks by the trained pair head of mode='mlp' instead (pairmlp.py, lkg_pairmlp.hip): candidates are
ordered by the head's logit z, descending, ties to the smaller id; ``scores`` is the probability sigmoid(z)
(non-increasing), ``kernel_scores`` the logit.  r may be None (any relation) or given (that relation only), as for 'dot'.

The selection runs on the device (lkg_topk.hip): a GEMM on the exact-f32 MFMA whose epilogue keeps a running top-k per
query instead of storing the B x N scores.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch

from . import _queries as Q
from . import ops
from .ranking import KnownTriples


@dataclass
class TopKResult:
    """B x k per query, best first: ``ids`` (int64 entity ids, -1 where fewer than k candidates are eligible),
    ``scores`` (float32 reported scores, NaN where ids == -1) and ``kernel_scores`` (float32 s = |p|^2 - 2 q.p, the value
    the selection and lkg_rank_count_f32 compare -- for scoring='mlp' the head's logit; NaN where ids == -1)."""
    ids: torch.Tensor
    scores: torch.Tensor
    side: str
    kernel_scores: torch.Tensor


def predict_topk(model, ids: torch.Tensor, r: Optional[torch.Tensor] = None, side: str = "tail", k: int = 10,
                 known: Optional[KnownTriples] = None, scoring: Optional[str] = None,
                 candidates: Optional[torch.Tensor] = None, batch_size: Optional[int] = None,
                 splits: int = 0) -> TopKResult:
    """The k best eligible candidates of every query on the model's inference table (see the module docstring).
    candidates: optional 1-D tensor of unique entity ids to select among (ids are still entity ids).  batch_size: queries
    per launch (None: as many as the workspace bound allows); splits: candidate splits per launch (0 = automatic).
    Neither changes the result.  The model's mode, parameters and caches are left as they are."""
    side = Q.check_one_side(side, "top-k ranks one side at a time")
    scoring = scoring if scoring is not None else model.scoring
    mlp = scoring == "mlp"                               # the pair head (pairmlp.py); Q.SCORINGS are the embedding scores
    if not mlp:
        scoring = Q.check_scoring(scoring)
    k = Q.check_k(k)
    Q.check_query_lists(ids, r, scoring)
    if candidates is not None:
        Q.check_ids("candidates", candidates)
    Q.check_batch_size(batch_size)
    Q.check_splits(splits)
    Q.check_transr_model(model, scoring)
    Q.check_known_entities(known, model)
    head = None
    if mlp:
        from .pairmlp import fold_mlp_head, predict_topk_mlp
        Q.check_unique(candidates)
        head = fold_mlp_head(model)                      # (AttributeError without initialize_MLP)
    dev = model.entity_embed.weight.device
    Q.check_known_device(known, dev)
    b = ids.numel()
    if b == 0:
        return TopKResult(torch.full((0, k), -1, dtype=torch.int64, device=dev),
                          torch.zeros((0, k), dtype=torch.float32, device=dev), side,
                          torch.zeros((0, k), dtype=torch.float32, device=dev))
    (ids,), r, cand = Q.ids_to_device(model, dev, (ids,), r, candidates, unique=True)
    filt = known.for_side(side) if known is not None else None
    if mlp:
        out_ids, out_p, out_z = predict_topk_mlp(model, head, ids, r, side, k, filt, cand, batch_size, splits)
        return TopKResult(out_ids, out_p, side, out_z)
    out_ids = torch.empty((b, k), dtype=torch.int64, device=dev)
    out_sc = torch.empty((b, k), dtype=torch.float32, device=dev)
    out_s = torch.empty((b, k), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for g in Q.query_groups(model, scoring, side, ids, r, cand):
            for lo, hi in Q.batches(g.pos.numel(), batch_size):
                ii, ss, vv = ops.topk_select(g.q[lo:hi], g.p, g.pn, k, filt, g.qid[lo:hi], g.frel[lo:hi], cand, splits)
                out_ids[g.pos[lo:hi]] = ii
                out_s[g.pos[lo:hi]] = ss
                out_sc[g.pos[lo:hi]] = vv
    return TopKResult(out_ids, out_sc, side, out_s)
