"""Multi-answer retrieval: the place of EVERY held-out answer of a query in the query's ranked list, and the per-query
retrieval metrics that follow from those places -- precision@k, recall@k, hit@k, NDCG@k, average precision, reciprocal
rank -- for data in which an (entity, relation) has several true answers (patient -> diseases, disease -> patients).

Sides and queries.  side='tail': a query is a distinct (h, r) among the evaluated triples and its answers A are the
distinct t with (h, r, t) evaluated; side='head': a distinct (t, r) with the heads as answers.  With scoring='dot', r may
be None: the query is the entity alone and the filter drops pairs known under any relation, as predict_topk does.  Query
vectors, candidate rows and TransR projections are those of rank_triples / predict_topk; the kernel score is
s = pn[c] - 2 q.p_c.

The list of a query holds every candidate c -- every entity, or ``candidates`` -- whose kernel score is not NaN and that
``known`` does not drop.  The query's answers are exempt from the filter: they are the held-out truth, so ``known`` may or
may not contain the evaluated triples and the result is the same.  The list is ordered as predict_topk orders: ascending
kernel score by float comparison (-0.0 == +0.0), then ascending entity id.

Per answer: ``position`` is its 1-based place in that list and ``before`` the number of non-answers ahead of it, so
position = 1 + before + (answers of the same query ahead of it).  An answer whose score is NaN has position = before = -1
and is counted in ``nan``: a miss at every k that adds 0 to every sum, but still counts in m = |A|.

Per query, with the positions p_1 < p_2 < ... and hits_k = #{p_i <= k}: precision@k = hits_k / k, recall@k = hits_k / m,
hit@k = hits_k > 0, ndcg@k = (sum over p_i <= k of 1 / log2(1 + p_i)) / (sum for i = 1 .. min(m, k) of 1 / log2(1 + i)),
ap = (sum_i i / p_i) / m (untruncated), rr = 1 / p_1.  Aggregates are means over the queries in float64.

Every distinct query is scored ONCE against the candidates, however many answers it has (lkg_retrieval.hip, DESIGN.md
section 3.6j): the answers' keys (s, id) come from the explicit-triple kernel, are sorted inside each query by
lkg_accept_order, and a counting GEMM on the exact-f32 MFMA places every candidate's score among the keys of its row.
Positions are exact at any depth; nothing of size B x N is stored.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from . import _queries as Q
from . import ops
from .ranking import KnownTriples


@dataclass
class AnswerRanks:
    """Per input triple, on the model's device: ``query`` (int64, index into the distinct queries), ``before`` and
    ``position`` (int64; -1 for a NaN answer) and ``nan`` (bool).  Per distinct query, ordered by (relation, entity id):
    ``q_ids``, ``q_rel`` (-1: any relation) and ``n_answers`` (its distinct answers, the NaN ones included), all int64.
    Per distinct answer, ordered by (query, entity id) so that query u owns n_answers[u] consecutive entries: ``a_query``,
    ``a_ids``, ``a_before``, ``a_position`` (int64).  With ``ks`` also per query: ``hits`` int64[Q, len(ks)], ``ndcg``
    float64[Q, len(ks)], ``ap`` and ``rr`` float64[Q]."""
    query: torch.Tensor
    before: torch.Tensor
    position: torch.Tensor
    nan: torch.Tensor
    q_ids: torch.Tensor
    q_rel: torch.Tensor
    n_answers: torch.Tensor
    side: str
    a_query: torch.Tensor
    a_ids: torch.Tensor
    a_before: torch.Tensor
    a_position: torch.Tensor
    ks: Optional[tuple] = None
    hits: Optional[torch.Tensor] = None
    ndcg: Optional[torch.Tensor] = None
    ap: Optional[torch.Tensor] = None
    rr: Optional[torch.Tensor] = None


def _front(model, h, r, t, side, known, scoring, candidates, batch_size):
    """Every argument check, before any device work; (side, scoring, device)."""
    side = Q.check_one_side(side, "top-k ranks one side at a time")
    scoring = Q.resolve_scoring(model, scoring, "scoring='mlp' has no kernel score to place answers by here: the pair "
                                "head's filtered ranks come from rank_pairs_mlp")
    Q.check_has_relations(r, scoring)
    if r is None:
        Q.check_id_pair(h, t, ("h", "t"))
    else:
        Q.check_triple_lists(h, r, t)
    if candidates is not None:
        Q.check_ids("candidates", candidates)
    Q.check_batch_size(batch_size)
    Q.check_transr_model(model, scoring)
    Q.check_known_entities(known, model)
    Q.check_unique(candidates)
    dev = model.entity_embed.weight.device
    Q.check_known_device(known, dev)
    return side, scoring, dev


def _empty(side, dev, ks):
    zi = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)       # noqa: E731
    zf = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)     # noqa: E731
    res = AnswerRanks(zi(0), zi(0), zi(0), torch.zeros(0, dtype=torch.bool, device=dev), zi(0), zi(0), zi(0), side, zi(0), zi(0),
                      zi(0), zi(0))
    if ks is not None:
        res.ks, res.hits, res.ndcg, res.ap, res.rr = ks, zi(0, len(ks)), zf(0, len(ks)), zf(0), zf(0)
    return res


def _group_answers(model, scoring, p, pn, e, alpha, q_ent, q_rel, a_query, a_ptr, a_id, pos):
    """The sorted keys of the distinct queries at ``pos``: (keys' answer index int64[M], key_s, key_id, counts int64[len
    (pos)], their rowptr) -- the answers a_ptr[u] .. a_ptr[u + 1] of each query, scored by the explicit-triple kernel, the NaN ones
    dropped, the rest in (score, id) order inside their query."""
    dev = pos.device
    lens = a_ptr[pos + 1] - a_ptr[pos]
    local = torch.repeat_interleave(torch.arange(pos.numel(), device=dev), lens)          # the key's query within pos
    start = torch.cumsum(lens, 0) - lens
    idx = a_ptr[pos][local] + (torch.arange(local.numel(), device=dev) - start[local])     # its answer, globally
    ent, ans = q_ent[a_query[idx]], a_id[idx]
    rel = q_rel[a_query[idx]] if e is not None else None
    s, _ = ops.triple_scores(p, ent, ans, pn, e, rel, alpha, reported=False)
    ok = ~torch.isnan(s)
    idx, local, s, ans = idx[ok], local[ok], s[ok], ans[ok]
    counts = torch.bincount(local, minlength=pos.numel())
    rowptr = torch.zeros(pos.numel() + 1, dtype=torch.int64, device=dev)
    torch.cumsum(counts, 0, out=rowptr[1:])
    key_id, key_s, _ = ops.accept_order(rowptr, ans, s, s, model.n_entities)
    # (query, id) is unique: the sorted key's answer is found among the scored ones, which ascend by (query, id)
    n = model.n_entities
    key_local = torch.repeat_interleave(torch.arange(pos.numel(), device=dev), counts)
    where = torch.searchsorted(local * n + ans, key_local * n + key_id)
    return idx[where], key_s, key_id, counts, rowptr


def _run(model, h, r, t, side, known, scoring, cand, batch_size, ks) -> AnswerRanks:
    """rank_answers of checked, non-empty triples whose ids are on the device."""
    dev = h.device
    n = model.n_entities
    tee = ops.RETRIEVAL_SLICE
    ent, ans = (h, t) if side == "tail" else (t, h)
    uq, query = torch.unique((r if r is not None else torch.zeros_like(ent)) * n + ent, return_inverse=True)
    n_q = uq.numel()
    q_ent = uq % n
    q_rel = uq // n if r is not None else torch.full_like(uq, -1)
    up, answer = torch.unique(query * n + ans, return_inverse=True)        # the distinct answers, by (query, id)
    a_query, a_id = up // n, up % n
    n_answers = torch.bincount(a_query, minlength=n_q)
    a_ptr = torch.zeros(n_q + 1, dtype=torch.int64, device=dev)
    torch.cumsum(n_answers, 0, out=a_ptr[1:])
    slot = None
    if cand is not None:
        slot = ops.pair_mlp_cand_slot(n, cand)
        if bool((slot[a_id] < 0).any()):
            raise ValueError("candidates must contain every answer (the evaluated entity of every triple)")
    filt = known.for_side(side) if known is not None else None
    a_before = torch.full((up.numel(),), -1, dtype=torch.int64, device=dev)
    a_position = torch.full((up.numel(),), -1, dtype=torch.int64, device=dev)
    res = AnswerRanks(query, None, None, None, q_ent, q_rel, n_answers, side, a_query, a_id, a_before, a_position)
    if ks is not None:
        res.ks = ks
        res.hits = torch.zeros((n_q, len(ks)), dtype=torch.int64, device=dev)
        res.ndcg = torch.zeros((n_q, len(ks)), dtype=torch.float64, device=dev)
        res.ap = torch.zeros(n_q, dtype=torch.float64, device=dev)
        res.rr = torch.zeros(n_q, dtype=torch.float64, device=dev)
    e, alpha = Q.relation_rows(model, scoring), Q.side_alpha(side)
    with torch.no_grad():
        for g in Q.query_groups(model, scoring, side, q_ent, q_rel if r is not None else None, cand):
            pos = g.pos
            key_ans, key_s, key_id, counts, qkey_ptr = _group_answers(model, scoring, g.table, g.table_n, e, alpha, q_ent,
                                                                      q_rel, a_query, a_ptr, a_id, pos)
            # one row per RETRIEVAL_SLICE keys of a query
            n_slices = (counts + tee - 1) // tee
            row_base = torch.cumsum(n_slices, 0) - n_slices
            row_q = torch.repeat_interleave(torch.arange(pos.numel(), device=dev), n_slices)
            n_rows = row_q.numel()
            in_query = torch.arange(n_rows, device=dev) - row_base[row_q]
            qkey_off, qkey_n = qkey_ptr[:-1][row_q], counts[row_q]
            key_off = qkey_off + in_query * tee
            key_n = torch.clamp(qkey_n - in_query * tee, max=tee).to(torch.int32)
            frow, frel = g.qid[row_q], g.frel[row_q]
            buckets = torch.empty((n_rows, tee), dtype=torch.int32, device=dev)
            for lo, hi in Q.batches(n_rows, batch_size):
                buckets[lo:hi] = ops.retrieval_count(g.q, row_q[lo:hi], g.p, g.pn, key_off[lo:hi], key_n[lo:hi],
                                                     qkey_off[lo:hi], qkey_n[lo:hi], key_s, key_id, filt, frow[lo:hi],
                                                     frel[lo:hi], cand, slot)
            before, position, metrics = ops.retrieval_finish(qkey_ptr, row_base, buckets, n_answers[pos], ks, g.p.shape[0])
            a_before[key_ans], a_position[key_ans] = before, position
            if ks is not None:
                res.hits[pos], res.ndcg[pos], res.ap[pos], res.rr[pos] = metrics
    res.before, res.position = a_before[answer], a_position[answer]
    res.nan = res.position < 0
    return res


def rank_answers(model, h: torch.Tensor, r: Optional[torch.Tensor], t: torch.Tensor, side: str = "tail",
                 known: Optional[KnownTriples] = None, scoring: Optional[str] = None,
                 candidates: Optional[torch.Tensor] = None, batch_size: Optional[int] = None,
                 ks: Optional[Sequence[int]] = None) -> AnswerRanks:
    """The place of every evaluated triple's answer in its query's list (see the module docstring): an AnswerRanks.
    Duplicate input triples get the same values and an answer counts once.  side is 'tail' or 'head'.  candidates:
    optional unique entity ids to rank among; they must contain every answer.  batch_size bounds the rows (a query and at
    most ops.RETRIEVAL_SLICE of its answers) per launch and changes nothing.  ks: also compute the per-query hits@k,
    NDCG@k, AP and RR on the device.  The model's mode, parameters and caches are left as they are."""
    ks = Q.check_ks(ks) if ks is not None else None
    side, scoring, dev = _front(model, h, r, t, side, known, scoring, candidates, batch_size)
    if h.numel() == 0:
        return _empty(side, dev, ks)
    (h, t), r, cand = Q.ids_to_device(model, dev, (h, t), r, candidates, unique=True)
    return _run(model, h, r, t, side, known, scoring, cand, batch_size, ks)


def retrieval_metrics(res: AnswerRanks) -> Dict:
    """The aggregates of evaluate_retrieval for one side from an AnswerRanks computed with ks."""
    ks = res.ks
    n_q = res.q_ids.numel()
    hits, m = res.hits.cpu(), res.n_answers.cpu().double()
    mean = lambda x: float(x.double().mean()) if n_q else 0.0                   # noqa: E731
    out: Dict = {}
    for j, k in enumerate(ks):
        hk = hits[:, j].double()
        out[f"precision@{k}"] = mean(hk / float(k))
        out[f"recall@{k}"] = mean(hk / m)
        out[f"hit@{k}"] = mean(hits[:, j] > 0)
        out[f"ndcg@{k}"] = mean(res.ndcg[:, j].cpu())
    out["map"], out["mrr"] = mean(res.ap.cpu()), mean(res.rr.cpu())
    listed = res.a_position > 0
    nan = int((~listed).sum())
    before = res.a_before[listed].cpu()
    out["n_queries"], out["n_answers"], out["nan"] = n_q, int(res.n_answers.sum()), nan
    out["per_answer"] = Q.metrics_from_counts(before, torch.zeros_like(before), ks)
    return out


def evaluate_retrieval(model, h: torch.Tensor, r: Optional[torch.Tensor], t: torch.Tensor,
                       known: Optional[KnownTriples] = None, ks: Sequence[int] = (1, 3, 10), side: str = "tail",
                       scoring: Optional[str] = None, candidates: Optional[torch.Tensor] = None,
                       batch_size: Optional[int] = None) -> Dict:
    """{'precision@k', 'recall@k', 'hit@k', 'ndcg@k' for each k, 'map', 'mrr', 'n_queries', 'n_answers', 'nan',
    'per_answer'}: the means over the distinct queries of the per-query retrieval metrics (see the module docstring);
    ``nan`` counts the distinct answers whose score is NaN, and ``per_answer`` is metrics_from_counts(before, 0, ks), the
    filtered link-prediction view of the same run over the distinct non-NaN answers.  side='both' averages over the
    queries of both sides and adds the 'tail' and 'head' sub-dicts, as evaluate_ranking does.  ks are positive integers
    without an upper bound.  Runs in eval mode and restores the model's previous mode."""
    ks = Q.check_ks(ks)
    side = Q.check_side(side)
    sides = Q.rank_sides(side)
    for s_ in sides:
        _front(model, h, r, t, s_, known, scoring, candidates, batch_size)
    with Q.eval_mode(model):
        per_side = {s_: retrieval_metrics(rank_answers(model, h, r, t, side=s_, known=known, scoring=scoring,
                                                       candidates=candidates, batch_size=batch_size, ks=ks))
                    for s_ in sides}
    if side != "both":
        return per_side[side]
    a, b = per_side["tail"], per_side["head"]
    na, nb = a["n_queries"], b["n_queries"]
    out: Dict = {}
    for key in a:
        if key == "per_answer":
            continue
        if key in ("n_queries", "n_answers", "nan"):
            out[key] = a[key] + b[key]
        else:
            out[key] = (a[key] * na + b[key] * nb) / (na + nb) if na + nb else 0.0
    pa, pb = a["per_answer"], b["per_answer"]
    n = pa["n"] + pb["n"]
    out["per_answer"] = {k_: (n if k_ == "n" else ((pa[k_] * pa["n"] + pb[k_] * pb["n"]) / n if n else 0.0)) for k_ in pa}
    out["tail"], out["head"] = a, b
    return out
