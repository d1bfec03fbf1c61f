"""Threshold retrieval: for every query (h, r, ?) -- or (?, r, t) -- the list of ALL candidates that a fitted classifier
accepts and that are not already known: the sparse form of the reference's mode='predict' (model.py:488-491), whose dense
B x N matrix of 0 / 1 cannot exist at the sizes this library runs.

Queries, candidates, sides, scoring ('transr' / 'transe' / 'dot'), ``known`` and ``candidates`` are those of predict_topk
(topk.py).  Candidate c of query i is accepted iff its reported score v(i, c) -- the bits score_triples returns for that
triple on that side, TopKResult.scores -- passes one float32 compare with the query's threshold, v <= thr[r_i] for
distances and v >= thr[r_i] for 'dot' (the decision of evaluate_triple_classification; a NaN score is never accepted), it
is not dropped by ``known`` (nothing is exempt; r=None with 'dot' drops pairs known under any relation) and it is in
``candidates`` if that is given.  Every list is ordered as predict_topk orders: ascending kernel score s by float
comparison, then ascending entity id.  The reported score is monotone in s, so a query's accepted list is a PREFIX of its
unbounded top-k list; the result is a unique object, whatever batch_size, splits or the order of queries and candidates.

The lists are built on the device in two passes over the exact-f32 MFMA scoring (lkg_accept.hip): a count, whose running
total is held against ``max_total`` before anything of the size of the result is allocated, then an emit into the
scanned segments and a radix sort inside them.
"""
from __future__ import annotations

from dataclasses import dataclass
from types import SimpleNamespace
from typing import Optional, Union

import torch

from . import _queries as Q
from . import ops
from .ranking import KnownTriples
from .triples import TripleThresholds, threshold_list


@dataclass
class AcceptedResult:
    """The accepted candidates of B queries in CSR form, on the model's device: query i owns [rowptr[i], rowptr[i + 1]) of
    ``ids`` (int64 entity ids, best first), ``scores`` (float32 reported scores, the bits of score_triples) and
    ``kernel_scores`` (float32 s, the ordering key, the bits of TopKResult.kernel_scores); ``counts`` = the lengths.
    ``query_ids`` / ``r`` are the queries as given (on the device), which triples() and pairs() pair the lists with.
    From predict_accepted_mlp (pairmlp.py) ``scores`` are probabilities and ``kernel_scores`` logits, as in a TopKResult
    under scoring='mlp'."""
    rowptr: torch.Tensor
    ids: torch.Tensor
    scores: torch.Tensor
    kernel_scores: torch.Tensor
    counts: torch.Tensor
    side: str
    query_ids: torch.Tensor
    r: Optional[torch.Tensor]

    def triples(self):
        """(h, r, t), int64[M] each: the proposed triples in list order."""
        if self.r is None:
            raise ValueError("the queries carry no relation (r=None): there are pairs here, not triples")
        rows = self._rows()
        q, r = self.query_ids[rows], self.r[rows]
        return (q, r, self.ids) if self.side == "tail" else (self.ids, r, q)

    def pairs(self):
        """(h, t), int64[M] each: the listed pairs in list order, whichever side was asked; works with r=None (the lists
        of predict_accepted_mlp, pairmlp.py, whose scores are probabilities and kernel_scores logits)."""
        q = self.query_ids[self._rows()]
        return (q, self.ids) if self.side == "tail" else (self.ids, q)

    def _rows(self):
        return torch.repeat_interleave(torch.arange(self.counts.numel(), device=self.counts.device), self.counts)


def _check_max_total(max_total) -> int:
    if isinstance(max_total, bool) or not isinstance(max_total, int) or max_total < 0:
        raise ValueError(f"max_total must be a non-negative integer, got {max_total!r}")
    return max_total


def _query_thresholds(model, thresholds, scoring: str, r: Optional[torch.Tensor]):
    """What _front hands on for the per-query thresholds: one Python float per relation, or a single float with r=None."""
    if r is None:
        if isinstance(thresholds, (TripleThresholds, torch.Tensor)):
            raise ValueError("without relations (r=None) the threshold must be one float")
        return threshold_list(SimpleNamespace(n_relations=1), thresholds, scoring)
    return threshold_list(model, thresholds, scoring)


def _front(model, ids, r, thresholds, side, known, scoring, candidates, batch_size, splits):
    """The argument checks predict_topk makes, through the same functions in the same order, and the thresholds;
    everything before any device work."""
    side = Q.check_one_side(side, "top-k ranks one side at a time")
    scoring = Q.resolve_scoring(model, scoring, "scoring='mlp' has no acceptance threshold here: the pair head's lists "
                                "come from predict_topk(scoring='mlp')")
    Q.check_query_lists(ids, r, scoring)
    if candidates is not None:
        Q.check_ids("candidates", candidates)
    Q.check_batch_size(batch_size)
    Q.check_splits(splits)
    Q.check_transr_model(model, scoring)
    thr = _query_thresholds(model, thresholds, scoring, r)
    Q.check_known_entities(known, model)
    Q.check_unique(candidates)
    dev = model.entity_embed.weight.device
    Q.check_known_device(known, dev)
    return side, scoring, thr, dev


def _run(model, ids, r, thr, side, known, scoring, cand, batch_size, splits, max_total):
    """(counts int64[B], chunks, total) of the checked queries (ids already on the device): with max_total not None,
    chunks holds per relation group and query batch (query positions, local rowptr, ids, s, v), every row in order, and
    total their entries; with max_total None only the count pass runs."""
    dev = ids.device
    b = ids.numel()
    higher = not Q.lower_is_better(scoring)
    filt = known.for_side(side) if known is not None else None
    thr_t = torch.tensor(thr, dtype=torch.float32, device=dev)
    thr_q = thr_t[r] if r is not None else thr_t.expand(b).contiguous()
    counts = torch.zeros(b, dtype=torch.int64, device=dev)
    chunks, total = [], 0
    with torch.no_grad():
        for g in Q.query_groups(model, scoring, side, ids, r, cand):
            pos = g.pos
            qn = ops.rank_sqnorm(g.q) if g.pn is not None else None
            tq = thr_q[pos]
            for lo, hi in Q.batches(pos.numel(), batch_size):
                args = (g.q[lo:hi], g.p, g.pn, tq[lo:hi])
                kw = dict(higher=higher, filt=filt, filter_row=g.qid[lo:hi], filter_rel=g.frel[lo:hi], cand_ids=cand,
                          splits=splits, qn=None if qn is None else qn[lo:hi])
                cnt = ops.accept_count(*args, **kw)
                m = int(cnt.sum())
                total += m
                counts[pos[lo:hi]] = cnt.long()
                if max_total is None:
                    continue
                if total > max_total:
                    raise ValueError(f"more than max_total={max_total} accepted candidates: {total} so far (raise "
                                     "max_total, tighten the thresholds, or ask count_accepted for the sizes)")
                rowptr, ii, ss, vv = ops.accept_emit(*args, cnt, total=m, **kw)
                ii, ss, vv = ops.accept_order(rowptr, ii, ss, vv, model.n_entities)
                chunks.append((pos[lo:hi], rowptr, ii, ss, vv))
    return counts, chunks, total


def _empty(side, dev, ids, r):
    z = torch.zeros(0, dtype=torch.float32, device=dev)
    return AcceptedResult(torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros(0, dtype=torch.int64, device=dev), z,
                          z.clone(), torch.zeros(0, dtype=torch.int64, device=dev), side, ids.to(dev).long(),
                          None if r is None else r.to(dev).long())


def predict_accepted(model, ids: torch.Tensor, r: Optional[torch.Tensor],
                     thresholds: Union[TripleThresholds, float, torch.Tensor], side: str = "tail",
                     known: Optional[KnownTriples] = None, scoring: Optional[str] = None,
                     candidates: Optional[torch.Tensor] = None, batch_size: Optional[int] = None, splits: int = 0,
                     max_total: int = 1 << 26) -> AcceptedResult:
    """Every eligible candidate of every query whose reported score passes the query's threshold, ordered as
    predict_topk orders (see the module docstring).  thresholds: a TripleThresholds fitted on this scoring, a float, or a
    float32[n_relations] tensor -- query i uses thr[r[i]]; with scoring='dot' and r=None only a float.  The sentinels
    work as they are: -inf accepts nothing under a distance, +inf every candidate whose score is not NaN.  max_total caps
    the number of entries M: the counts are taken first and the call raises ValueError as soon as their running total
    exceeds it, before the allocation that would hold them.  batch_size (queries per launch) and splits (candidate splits
    per launch, 0 = automatic) change nothing.  The model's mode, parameters and caches are left as they are."""
    max_total = _check_max_total(max_total)
    side, scoring, thr, dev = _front(model, ids, r, thresholds, side, known, scoring, candidates, batch_size, splits)
    b = ids.numel()
    if b == 0:
        return _empty(side, dev, ids, r)
    (ids,), r, cand = Q.ids_to_device(model, dev, (ids,), r, candidates, unique=True)
    counts, chunks, total = _run(model, ids, r, thr, side, known, scoring, cand, batch_size, splits, max_total)
    rowptr = torch.zeros(b + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=rowptr[1:])
    out_ids = torch.empty(total, dtype=torch.int64, device=dev)
    out_sc = torch.empty(total, dtype=torch.float32, device=dev)
    out_s = torch.empty(total, dtype=torch.float32, device=dev)
    for pos, rp, ii, ss, vv in chunks:                     # the rows back in query order
        if ii.numel() == 0:
            continue
        shift = rowptr[pos] - rp[:-1]
        dst = torch.arange(ii.numel(), device=dev) + torch.repeat_interleave(shift, rp[1:] - rp[:-1])
        out_ids[dst], out_s[dst], out_sc[dst] = ii, ss, vv
    return AcceptedResult(rowptr, out_ids, out_sc, out_s, counts, side, ids, r)


def count_accepted(model, ids: torch.Tensor, r: Optional[torch.Tensor],
                   thresholds: Union[TripleThresholds, float, torch.Tensor], side: str = "tail",
                   known: Optional[KnownTriples] = None, scoring: Optional[str] = None,
                   candidates: Optional[torch.Tensor] = None, batch_size: Optional[int] = None,
                   splits: int = 0) -> torch.Tensor:
    """int64[B]: the length of every list predict_accepted would return, from the count pass alone -- nothing of the size
    of the lists is allocated and there is no cap."""
    side, scoring, thr, dev = _front(model, ids, r, thresholds, side, known, scoring, candidates, batch_size, splits)
    if ids.numel() == 0:
        return torch.zeros(0, dtype=torch.int64, device=dev)
    (ids,), r, cand = Q.ids_to_device(model, dev, (ids,), r, candidates, unique=True)
    return _run(model, ids, r, thr, side, known, scoring, cand, batch_size, splits, None)[0]
