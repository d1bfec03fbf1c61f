"""The query front end shared by ranking.py, topk.py, accepted.py, retrieval.py, triples.py, relations.py and pairmlp.py:
the argument checks, the step that takes the ids to the model's device, the batch ranges, the scorings with the rows and
queries they score (scoring_groups, side_queries, query_groups, rows_to_project), and what the rankers (rank_triples,
rank_pairs_mlp) and their evaluate_* functions do with the counts.  Plain functions; each caller decides where it runs
them, so its argument errors still come before any device work."""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Dict, Optional, Sequence

import torch

from . import ops

SIDES = ("tail", "head", "both")
SCORINGS = ("transr", "transe", "dot")                   # the embedding scores; 'mlp' is the pair head (pairmlp.py)


def check_ids(name, x):
    if not isinstance(x, torch.Tensor) or x.dim() != 1 or x.dtype.is_floating_point or x.dtype == torch.bool:
        raise ValueError(f"{name} must be a 1-D tensor of integer ids")


def check_batch_size(batch_size):
    if batch_size is not None and (isinstance(batch_size, bool) or int(batch_size) != batch_size or batch_size <= 0):
        raise ValueError(f"batch_size must be a positive integer, got {batch_size!r}")


def check_side(side: str) -> str:
    if side not in SIDES:
        raise ValueError(f"side must be one of {SIDES}, got {side!r}")
    return side


def check_one_side(side: str, why: str) -> str:
    if side not in SIDES[:2]:
        raise ValueError(f"side must be one of {SIDES[:2]} ({why}), got {side!r}")
    return side


def check_scoring(scoring: str) -> str:
    if scoring not in SCORINGS:
        raise ValueError(f"scoring must be one of {SCORINGS}, got {scoring!r}")
    return scoring


def resolve_scoring(model, scoring: Optional[str], mlp_message: Optional[str] = None) -> str:
    """scoring, or the model's own; 'mlp' refused in the caller's words (mlp_message), anything else unknown in ours."""
    scoring = scoring if scoring is not None else model.scoring
    if mlp_message is not None and scoring == "mlp":
        raise ValueError(mlp_message)
    return check_scoring(scoring)


def check_transr_model(model, scoring: str):
    if scoring == "transr" and getattr(model, "gat_trans_M", None) is None:
        raise ValueError("scoring='transr' needs a model with gat_trans_M (built with scoring='transr')")


def lower_is_better(scoring: str) -> bool:
    return scoring != "dot"


def check_k(k) -> int:
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= ops.TOPK_MAX:
        raise ValueError(f"k must be an integer in [1, {ops.TOPK_MAX}], got {k!r}")
    return k


def check_splits(splits):
    if isinstance(splits, bool) or int(splits) != splits or not 0 <= splits <= ops.TOPK_MAX_SPLITS:
        raise ValueError(f"splits must be an integer in [0, {ops.TOPK_MAX_SPLITS}], got {splits!r}")


def check_has_relations(r, scoring: str):
    if r is None and scoring not in ("dot", "mlp"):
        raise ValueError(f"scoring={scoring!r} needs the relations r (only 'dot' can filter without them)")


def check_id_pair(a, b, names):
    """Two 1-D id lists of one length, both required."""
    check_ids(names[0], a)
    check_ids(names[1], b)
    if a.numel() != b.numel():
        raise ValueError(f"{names[0]} and {names[1]} have different lengths ({a.numel()}, {b.numel()})")


def check_query_lists(ids, r, scoring: str, names=("ids", "r")):
    """1-D ids; r the same and as long, or None where the scoring can do without (check_has_relations)."""
    if r is None:
        check_ids(names[0], ids)
        check_has_relations(r, scoring)
    else:
        check_id_pair(ids, r, names)


def check_triple_lists(h, r, t):
    check_ids("h", h)
    check_ids("r", r)
    check_ids("t", t)
    if not h.numel() == r.numel() == t.numel():
        raise ValueError(f"h, r, t have different lengths ({h.numel()}, {r.numel()}, {t.numel()})")


def check_ks(ks: Sequence[int]) -> tuple:
    ks = tuple(ks)
    for k in ks:
        if isinstance(k, bool) or int(k) != k or k <= 0:
            raise ValueError(f"Hits@k needs positive integers k, got {k!r}")
    return tuple(int(k) for k in ks)


def check_unique(candidates: Optional[torch.Tensor]):
    if candidates is not None and torch.unique(candidates).numel() != candidates.numel():
        raise ValueError("candidates must be unique entity ids")


def check_known_entities(known, model):
    if known is not None and known.n_entities != model.n_entities:
        raise ValueError(f"known triples over {known.n_entities} entities, the model has {model.n_entities}")


def check_known_device(known, dev):
    if known is not None and known.device != dev:
        raise ValueError(f"known triples live on {known.device}, the model on {dev}")


def batches(n: int, batch_size: Optional[int]):
    """(lo, hi) over n items, batch_size at a time (None: all at once); nothing for n = 0."""
    step = max(n, 1) if batch_size is None else int(batch_size)
    for lo in range(0, n, step):
        yield lo, min(lo + step, n)


def ids_to_device(model, dev, entities: Sequence[torch.Tensor], r: Optional[torch.Tensor] = None,
                  candidates: Optional[torch.Tensor] = None, known=None, unique: bool = False):
    """(entity id lists, r, candidates) on the model's device as ids that are safe to gather through (ops.checked_ids); an
    id out of range raises here (check_deferred_errors waits for it).  Then two checks for the callers that make them at
    this point (known: the filter's device, rank_triples; unique: the moved candidates, predict_topk) and model.device."""
    entities = ops.checked_ids(model.n_entities, *(x.to(dev) for x in entities))
    if r is not None:
        (r,) = ops.checked_ids(model.n_relations, r.to(dev), what="relation")
    if candidates is not None:
        (candidates,) = ops.checked_ids(model.n_entities, candidates.to(dev), what="candidate entity")
    ops.check_deferred_errors()
    check_known_device(known, dev)
    if unique:
        check_unique(candidates)
    model.device = dev
    return entities, r, candidates


def filter_relations(r: Optional[torch.Tensor], b: int, dev) -> torch.Tensor:
    """The relation of every query for the filter: r, or -1 ("under any relation") everywhere."""
    return r if r is not None else torch.full((b,), -1, dtype=torch.int64, device=dev)


def check_table_shape(model, scoring: str, table: torch.Tensor):
    c = table.shape[1]
    if scoring == "transe" and c != model.relation_dim:
        raise ValueError(f"scoring='transe' needs the table width ({c}) to equal relation_dim ({model.relation_dim})")
    if scoring == "transr" and model.gat_trans_M.shape[1] != c:
        raise ValueError(f"gat_trans_M is {tuple(model.gat_trans_M.shape)} for a table of width {c}")


def side_alpha(side: str) -> float:
    return 1.0 if side == "tail" else -1.0               # q = P_r[h] + e_r  /  q = P_r[t] - e_r


def relation_rows(model, scoring: str) -> Optional[torch.Tensor]:
    """The relation embeddings e the queries are shifted by (None for dot)."""
    return None if scoring == "dot" else model.relation_embed.weight.detach()


def scoring_groups(model, scoring: str, table: torch.Tensor, r: Optional[torch.Tensor], b: Optional[int] = None):
    """Check the table's width against the scoring and return a generator of (p, pn, pos): the candidate rows, their
    squared norms (None for dot) and the positions of the queries they serve.  TransR: one projection P_r = T W_r per
    relation present in r (the tall GEMM, one rowmax for all), each alive while the caller uses it; otherwise the table
    itself, serving all b = len(r) queries (r may be None then).  Every one-sided entry point scores through this, so
    all of them score with the same P_r, bit for bit."""
    dev = table.device
    check_table_shape(model, scoring, table)
    if scoring == "transr":
        w = model.gat_trans_M.detach()
        perm, seg = ops.group_by_key(r, model.n_relations)
        perm, seg = perm.long(), seg.tolist()
        rowmax = ops.row_absmax(table)

        def groups():
            for rr in range(model.n_relations):
                if seg[rr + 1] > seg[rr]:
                    p = ops.gemm_tall([table], [[w[rr]]], trans_b=False, rowmax=rowmax)
                    yield p, ops.rank_sqnorm(p), perm[seg[rr]:seg[rr + 1]]
    else:
        n = r.numel() if b is None else int(b)

        def groups():
            yield table, (ops.rank_sqnorm(table) if scoring == "transe" else None), torch.arange(n, device=dev)
    return groups()


def side_queries(model, scoring: str, side: str, p, pn, ent, rel, cand=None):
    """(q, p_c, pn_c): the query rows of the entities ent (relations rel) on that side of the rows p, and the candidate
    operands -- p, pn themselves, or with cand the gathered rows, scored with the same bits, and their squared norms."""
    q = ops.rank_queries(p, ent, relation_rows(model, scoring), rel, side_alpha(side))
    if cand is not None:
        p = ops.gather_rows(p, cand)
        pn = ops.rank_sqnorm(p) if pn is not None else None
    return q, p, pn


@torch.no_grad()
def query_groups(model, scoring: str, side: str, ent: torch.Tensor, r: Optional[torch.Tensor], cand=None):
    """The operand loop of the one-sided entry points over the checked queries (ent, r) on the device: per group of
    scoring_groups on the model's inference table one record g with pos, qid = ent[pos], rel = r[pos] (None without r),
    frel (the filter column: rel, or -1 everywhere), the query rows q, the group's rows table / table_n and the candidate
    operands p / pn of side_queries.  A record lives for one turn of the caller's loop: it is emptied before the next
    projection is made, so no group's rows outlive their turn, whatever the caller still holds.  Gradients are off
    only while this generator's own frame runs: a caller keeps its launches under its own torch.no_grad()."""
    table = model._table_for_inference().detach()
    for p, pn, pos in scoring_groups(model, scoring, table, r, ent.numel()):
        g = SimpleNamespace(pos=pos, qid=ent[pos], rel=r[pos] if r is not None else None, table=p, table_n=pn)
        g.frel = filter_relations(g.rel, pos.numel(), pos.device)
        g.q, g.p, g.pn = side_queries(model, scoring, side, p, pn, g.qid, g.rel, cand)
        del p, pn
        yield g
        vars(g).clear()


def rows_to_project(table: torch.Tensor, rowmax: torch.Tensor, qi: torch.Tensor, ci: torch.Tensor, project: Optional[str]):
    """(rows, their rowmax, qi, ci) for a 'transr' projection that only the rows qi / ci are read from: the distinct rows
    of cat(qi, ci) with the ids renumbered into them, or the whole table with the ids as they are when the distinct rows
    are not fewer (project None) or when forced (project 'full'; any other value forces the distinct rows).  A projected
    row has the same bits either way: the tall GEMM's row does not depend on the rows projected with it."""
    if project != "full":
        uniq, inv = torch.unique(torch.cat((qi, ci)), return_inverse=True)
        if project is not None or uniq.numel() < table.shape[0]:
            return ops.gather_rows(table, uniq), rowmax[uniq], inv[:qi.numel()], inv[qi.numel():]
    return table, rowmax, qi, ci


@contextmanager
def eval_mode(model):
    """The model in eval mode, its previous mode restored on the way out (also after an error)."""
    was_training = model.training
    model.eval()
    try:
        yield
    finally:
        model.train(was_training)


@dataclass
class RankResult:
    """Per query: ``better`` / ``equal`` (int64) and ``rank`` = 1 + better + equal / 2 (float64).  For side='both' the
    tensors are 2 x B: row 0 the tail side, row 1 the head side."""
    better: torch.Tensor
    equal: torch.Tensor
    rank: torch.Tensor
    side: str


def realistic_rank(better: torch.Tensor, equal: torch.Tensor) -> torch.Tensor:
    return 1.0 + better.double() + 0.5 * equal.double()


def metrics_from_counts(better: torch.Tensor, equal: torch.Tensor, ks: Sequence[int] = (1, 3, 10)) -> Dict[str, float]:
    """{'mr', 'mrr', 'hits@k'..., 'n'} of the ranks 1 + better + equal / 2 (all zero for an empty set, 'n' = 0)."""
    ks = check_ks(ks)
    rank = realistic_rank(torch.as_tensor(better).reshape(-1), torch.as_tensor(equal).reshape(-1))
    n = rank.numel()
    out = {"n": n}
    if n == 0:
        out.update({"mr": 0.0, "mrr": 0.0}, **{f"hits@{k}": 0.0 for k in ks})
        return out
    out["mr"] = float(rank.mean())
    out["mrr"] = float((1.0 / rank).mean())
    for k in ks:
        out[f"hits@{k}"] = float((rank <= k).double().mean())
    return out


def rank_sides(side: str) -> tuple:
    return ("tail", "head") if side == "both" else (side,)


def count_buffers(side: str, b: int, dev):
    """better, equal: int32, one row per side of rank_sides(side), for the kernels' counts of b queries."""
    shape = (len(rank_sides(side)), b)
    return torch.empty(shape, dtype=torch.int32, device=dev), torch.empty(shape, dtype=torch.int32, device=dev)


def rank_result(better: torch.Tensor, equal: torch.Tensor, side: str) -> RankResult:
    """The RankResult of filled count_buffers (b = 0: the empty result)."""
    better, equal = better.long(), equal.long()
    if side != "both":
        better, equal = better[0], equal[0]
    return RankResult(better, equal, realistic_rank(better, equal), side)


def ranking_metrics(res: RankResult, ks: Sequence[int]) -> Dict:
    """metrics_from_counts over every rank of res, and per side under 'tail' / 'head'."""
    sides = rank_sides(res.side)
    better, equal = res.better.cpu().reshape(len(sides), -1), res.equal.cpu().reshape(len(sides), -1)
    out = metrics_from_counts(better, equal, ks)
    for j, s_ in enumerate(sides):
        out[s_] = metrics_from_counts(better[j], equal[j], ks)
    return out
