"""Scores and filtered ranks against per-query candidate lists: every held-out triple is judged against ITS OWN list of
negatives -- the protocol of ogbl-wikikg2 / ogbl-biokg (fixed, possibly type-constrained negatives per side) and of the
reference's ``evaluate(..., neg_rate=...)`` -- instead of one candidate set shared by all queries.

``lists`` is an int64[B, M] tensor, M >= 1; row i belongs to query i, a negative entry is an empty slot (ragged lists are
padded with -1), and a ``NegativeBatch.neg`` is accepted as it is.  Lists are taken as given: duplicate ids each count.

score_lists returns the bits of score_triples for every slot (NaN in an empty one).  rank_in_lists compares kernel scores,
as rank_triples does, and stores none: slot j of query i is counted unless it is empty, holds the truth's id (the truth is
never compared with itself), or -- with ``known`` -- forms a known triple with the query on that side under r[i] (under
any relation for 'dot' with r=None).  ``kept`` counts the counted slots, ``better`` those strictly better than the truth
(lower for distances, higher for 'dot'), ``equal`` the float ties; a NaN slot is kept and is neither, a NaN truth gives
better = equal = 0.  With lists[i] = arange(N) the counts are rank_triples'.  Nothing depends on batch_size, on the order
of the queries or of the slots, or on which rows are projected together (lkg_lists.hip).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from . import _queries as Q
from . import ops
from . import triples as T


@dataclass
class ListRanks:
    """Per query: ``better`` / ``equal`` / ``kept`` (int64) and ``rank`` = 1 + better + equal / 2 (float64) among the kept
    slots of its own list and the truth."""
    better: torch.Tensor
    equal: torch.Tensor
    kept: torch.Tensor
    rank: torch.Tensor
    side: str


def _check_scoring(model, scoring: Optional[str]) -> str:
    scoring = Q.resolve_scoring(model, scoring, "scoring='mlp' has no list score: the pair head scores explicit (h, t) "
                                "pairs -- use score_pairs_mlp")
    Q.check_transr_model(model, scoring)
    return scoring


def _check_lists(name: str, lists, b: int):
    if not isinstance(lists, torch.Tensor) or lists.dim() != 2 or lists.dtype != torch.int64:
        raise ValueError(f"{name} must be an int64 tensor [B, M] of entity ids (a negative entry: an empty slot)")
    if lists.shape[0] != b or lists.shape[1] < 1:
        raise ValueError(f"{name} must hold one row of M >= 1 slots per query: {b} queries, {name} {tuple(lists.shape)}")


def _check_triples(h, r, t, scoring: str):
    Q.check_id_pair(h, t, ("h", "t"))
    if r is None:
        Q.check_has_relations(r, scoring)
    else:
        Q.check_id_pair(h, r, ("h", "r"))


def _to_device(model, dev, entities, r, lists):
    """The checked ids and lists on the model's device; an id out of range raises here."""
    lists = ops.checked_list_ids(model.n_entities, lists.to(dev))
    entities, r, _ = Q.ids_to_device(model, dev, entities, r)
    return entities, r, lists


def _groups(model, scoring: str, side: str, ent, r, lists, truth=None, want_ids: bool = False):
    """A generator of (p, pn, q, rows, tru, cand_ids, pos): the table of rows the queries at positions pos (None: all of
    them, in order) score against, its squared norms (None for dot), their query rows q, their lists and truths as rows
    of p, and the entity id of every row of p (None: the row number; made only with want_ids).  'transr': one group per
    relation present, over P_r of the distinct rows its queries, truths and non-empty slots touch -- or of the whole
    table when those are not fewer -- as triples._groups projects."""
    table = model._table_for_inference().detach()
    Q.check_table_shape(model, scoring, table)
    e = Q.relation_rows(model, scoring)
    alpha = Q.side_alpha(side)
    if scoring != "transr":
        pn = ops.rank_sqnorm(table) if scoring == "transe" else None
        yield table, pn, ops.rank_queries(table, ent, e, r if e is not None else None, alpha), lists, truth, None, None
        return
    perm, seg = ops.group_by_key(r, model.n_relations)
    perm, seg = perm.long(), seg.tolist()
    w = model.gat_trans_M.detach()
    rowmax = ops.row_absmax(table)
    for rr in range(model.n_relations):
        if seg[rr + 1] == seg[rr]:
            continue
        pos = perm[seg[rr]:seg[rr + 1]]
        n = pos.numel()
        own = ent[pos] if truth is None else torch.cat((ent[pos], truth[pos]))
        rows = lists[pos]
        full = rows >= 0
        slots = rows[full]                                            # empty slots stay out of the unique
        src, srm, own_r, slots_r = Q.rows_to_project(table, rowmax, own, slots, T.PROJECT)
        cand_ids = None
        if src is not table:                                          # the distinct rows: renumber the lists into them
            rows = torch.full_like(rows, -1)
            rows[full] = slots_r
            if want_ids:
                cand_ids = torch.empty(src.shape[0], dtype=torch.int64, device=rows.device)
                cand_ids[torch.cat((own_r, slots_r))] = torch.cat((own, slots))
        p = ops.gemm_tall([src], [[w[rr]]], trans_b=False, rowmax=srm)
        del src, srm
        q = ops.rank_queries(p, own_r[:n], e, r[pos], alpha)
        yield p, ops.rank_sqnorm(p), q, rows, (None if truth is None else own_r[n:]), cand_ids, pos
        del p, q


def score_lists(model, ids: torch.Tensor, r: Optional[torch.Tensor], lists: torch.Tensor, side: str = "tail",
                scoring: Optional[str] = None, kernel_scores: bool = False,
                batch_size: Optional[int] = None) -> torch.Tensor:
    """float32[B, M]: the score of every slot of every query's own list on the model's inference table, NaN in an empty
    slot.  side='tail': [i, j] has the bits of score_triples(model, ids[i], r[i], lists[i, j], side='tail');
    side='head': of score_triples(model, lists[i, j], r[i], ids[i], side='head') -- reported scores, or kernel scores
    with kernel_scores=True.  r may be None for 'dot'.  batch_size: queries per launch (None: all of a group); it changes
    nothing.  The model's mode, parameters and caches are left as they are."""
    scoring = _check_scoring(model, scoring)
    side = Q.check_one_side(side, "a list is scored from one side at a time")
    Q.check_query_lists(ids, r, scoring)
    _check_lists("lists", lists, ids.numel())
    Q.check_batch_size(batch_size)
    dev = model.entity_embed.weight.device
    b, m = lists.shape
    out = torch.empty((b, m), dtype=torch.float32, device=dev)
    if b == 0:
        return out
    (ids,), r, lists = _to_device(model, dev, (ids,), r, lists)
    with torch.no_grad():
        for p, pn, q, rows, _, _, pos in _groups(model, scoring, side, ids, r, lists):
            n = q.shape[0]
            qn = ops.rank_sqnorm(q) if (pn is not None and not kernel_scores) else None
            sc = out if pos is None else torch.empty((n, m), dtype=torch.float32, device=dev)
            for lo, hi in Q.batches(n, batch_size):
                ops.list_scores(q[lo:hi], p, pn, rows[lo:hi], None if qn is None else qn[lo:hi],
                                reported=not kernel_scores, out=sc[lo:hi])
            if pos is not None:
                out[pos] = sc
    return out


def _rank(model, scoring, side, h, r, t, lists, known, batch_size):
    """(better, equal, kept) int64[B] of one side over checked ids and lists on the model's device."""
    dev = h.device
    b = h.numel()
    ent, truth = (h, t) if side == "tail" else (t, h)
    filt = known.for_side(side) if known is not None else None
    frel = Q.filter_relations(r, b, dev) if filt is not None else None
    better = torch.zeros(b, dtype=torch.int64, device=dev)
    equal = torch.zeros(b, dtype=torch.int64, device=dev)
    kept = torch.zeros(b, dtype=torch.int64, device=dev)
    with torch.no_grad():
        for p, pn, q, rows, tru, cand_ids, pos in _groups(model, scoring, side, ent, r, lists, truth, filt is not None):
            frow = None if filt is None else (ent if pos is None else ent[pos])
            fr = None if filt is None else (frel if pos is None else frel[pos])
            for lo, hi in Q.batches(q.shape[0], batch_size):
                bb, ee, kk = ops.list_count(q[lo:hi], p, pn, rows[lo:hi], tru[lo:hi], filt,
                                            None if filt is None else frow[lo:hi], None if filt is None else fr[lo:hi],
                                            cand_ids)
                at = slice(lo, hi) if pos is None else pos[lo:hi]
                better[at], equal[at], kept[at] = bb, ee, kk
    return better, equal, kept


def _check_rank_args(model, h, r, t, lists_by_name, known, scoring, batch_size):
    scoring = _check_scoring(model, scoring)
    _check_triples(h, r, t, scoring)
    for name, lists in lists_by_name:
        _check_lists(name, lists, h.numel())
    Q.check_batch_size(batch_size)
    Q.check_known_entities(known, model)
    Q.check_known_device(known, model.entity_embed.weight.device)
    return scoring


def rank_in_lists(model, h: torch.Tensor, r: Optional[torch.Tensor], t: torch.Tensor, lists: torch.Tensor,
                  side: str = "tail", known=None, scoring: Optional[str] = None,
                  batch_size: Optional[int] = None) -> ListRanks:
    """The rank of every triple's truth -- t as the tail of (h_i, r_i, .) on side 'tail', h as the head of (., r_i, t_i)
    on side 'head' -- among the slots of its own list lists[i, :] (see the module docstring): ListRanks(better, equal,
    kept, rank, side).  known: a ranking.KnownTriples filter.  No B x M scores are made.  r may be None for 'dot' (the
    filter then drops a slot known under any relation).  batch_size changes nothing; nothing of the model is changed."""
    side = Q.check_one_side(side, "a list is ranked from one side at a time")
    scoring = _check_rank_args(model, h, r, t, (("lists", lists),), known, scoring, batch_size)
    dev = model.entity_embed.weight.device
    if h.numel() == 0:
        z = torch.zeros(0, dtype=torch.int64, device=dev)
        return ListRanks(z, z.clone(), z.clone(), Q.realistic_rank(z, z), side)
    (h, t), r, lists = _to_device(model, dev, (h, t), r, lists)
    better, equal, kept = _rank(model, scoring, side, h, r, t, lists, known, batch_size)
    return ListRanks(better, equal, kept, Q.realistic_rank(better, equal), side)


def evaluate_list_ranking(model, h: torch.Tensor, r: Optional[torch.Tensor], t: torch.Tensor,
                          tail_lists: Optional[torch.Tensor] = None, head_lists: Optional[torch.Tensor] = None,
                          known=None, ks: Sequence[int] = (1, 3, 10), scoring: Optional[str] = None,
                          batch_size: Optional[int] = None) -> Dict:
    """{'mr', 'mrr', 'hits@k'..., 'n', 'tail': {...}, 'head': {...}}: ranking metrics of the triples against the given
    negatives, tail_lists[i, :] the candidate tails of (h_i, r_i, .) and head_lists[i, :] the candidate heads of
    (., r_i, t_i).  A side is present only if its lists were given; the top level is over every rank computed.  Runs in
    eval mode and restores the model's previous mode."""
    ks = Q.check_ks(ks)
    given = [(s_, name, x) for s_, name, x in (("tail", "tail_lists", tail_lists), ("head", "head_lists", head_lists))
             if x is not None]
    if not given:
        raise ValueError("evaluate_list_ranking needs tail_lists, head_lists or both")
    _check_rank_args(model, h, r, t, [(name, x) for _, name, x in given], known, scoring, batch_size)
    out, better, equal = {}, [], []
    with Q.eval_mode(model):
        for s_, _, x in given:
            res = rank_in_lists(model, h, r, t, x, side=s_, known=known, scoring=scoring, batch_size=batch_size)
            better.append(res.better.cpu())
            equal.append(res.equal.cpu())
            out[s_] = Q.metrics_from_counts(better[-1], equal[-1], ks)
    out.update(Q.metrics_from_counts(torch.cat(better), torch.cat(equal), ks))
    return out
