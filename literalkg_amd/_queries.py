"""The query front end shared by ranking.py, topk.py and pairmlp.py: the argument checks, the step that takes the ids to
the model's device, the batch ranges, and what the two rankers (rank_triples, rank_pairs_mlp) and their evaluate_*
functions do with the counts.  Plain functions; each caller decides where it runs them, so its argument errors still come
before any device work."""
from __future__ import annotations

from contextlib import contextmanager
from dataclasses import dataclass
from typing import Dict, Optional, Sequence

import torch

from . import ops

SIDES = ("tail", "head", "both")


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
