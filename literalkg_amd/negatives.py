"""Negatives for GIVEN positive triples, drawn on the device (lkg_negatives.hip; include/literalkg_hip.h): either
side corrupted ('tail', 'head', 'both' by a fair coin per triple, 'bernoulli' by TransH's tph / (tph + hpt) per relation),
false negatives filtered against every known triple of the corrupted side, candidates from all entities or from a pool, and
the subsampling weights RotatE and DGL-KE pair with the self-adversarial loss.  It is the sampling half of
self_adversarial.py; KGBatchSampler (sampler.py) stays the restatement of the reference's generate_kg_batch.

The draw is counter-based: with mix64 splitmix64's finaliser, arithmetic mod 2^64 and gid = group_offset + g,

    key(seed, gid)      = mix64(seed ^ (0xD1B54A32D192ED03 * (gid + 1)))
    value(seed, gid, c) = mix64(key(seed, gid) + 0x9E3779B97F4A7C15 * c)

counter 0 decides the side, counter 1 + j * MAX_TRIES + i is try i of slot j.  A candidate is rejected when it is the truth
of the corrupted slot or (filtered) forms a known triple; after MAX_TRIES rejections the last candidate is kept and flagged
``unfiltered``.  A candidate equal to the anchor entity and duplicates inside a group are NOT rejected, so a group's row
depends on (seed, gid, h, r, t) alone: the first K' columns of a K-draw are the K'-draw, and a batch cut anywhere with
group_offset carried gives the bits of the whole.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional, Tuple, Union

import torch

from . import _native as N
from . import _queries as Q
from . import ops
from ._objectives import check_margin, check_reduction, check_single_device
from .ranking import KnownTriples

MAX_TRIES = 64                                     # LKG_SAMPLE_MAX_TRIES
CORRUPT = ("tail", "head", "both", "bernoulli")    # LKG_CORRUPT_*: the position is the mode
RELATION_MAX = ops.RELATION_MAX                    # lkg_relation_cardinality's bitmap


def _check_known(known, what: str):
    if not isinstance(known, KnownTriples):
        raise ValueError(f"{what} needs the known triples as a KnownTriples, got {type(known).__name__}")
    return known


def _structure(s):
    """(rowptr, eptr, rel) pointers of a KnownTriples side, for the entry points that do not search the cols"""
    return [N.ptr(s[0]), N.ptr(s[2]), N.ptr(s[3])]


@dataclass
class RelationCardinalities:
    """Per relation, over the distinct known triples: ``triples`` T_r, distinct ``heads`` H_r and distinct ``tails`` Tl_r
    (int64[R] on the device).  tails_per_head = T_r / H_r (TransH's tph) and heads_per_tail = T_r / Tl_r (hpt) in float64,
    NaN for a relation without a triple."""
    triples: torch.Tensor
    heads: torch.Tensor
    tails: torch.Tensor

    @property
    def tails_per_head(self) -> torch.Tensor:
        return self.triples.double() / self.heads.double()

    @property
    def heads_per_tail(self) -> torch.Tensor:
        return self.triples.double() / self.tails.double()


def relation_cardinalities(known: KnownTriples) -> RelationCardinalities:
    """The cardinalities of every relation of ``known`` (lkg_relation_cardinality); a duplicated triple counts once."""
    known = _check_known(known, "relation_cardinalities")
    if known.n_relations > RELATION_MAX:
        raise ValueError(f"relation_cardinalities: at most {RELATION_MAX} relations, the known triples have "
                         f"{known.n_relations}")
    ops._need_gpu(known.by_head[0])
    out = torch.empty((3, known.n_relations), dtype=torch.int64, device=known.device)
    nnz = known.by_head[1].numel() if known.n_triples else 0
    N.call("lkg_relation_cardinality", known.n_entities, known.n_relations, known.n_triples, *_structure(known.by_head), nnz,
           *_structure(known.by_tail), N.ptr(out[0]), N.ptr(out[1]), N.ptr(out[2]), ops._stream())
    return RelationCardinalities(out[0], out[1], out[2])


def _outside(n_rows: int, ids: torch.Tensor) -> torch.Tensor:
    """int32[1] on the device: how many of ids lie outside [0, n_rows) -- ops.count_ids_outside without its host read"""
    bad = torch.empty(1, dtype=torch.int32, device=ids.device)
    scratch = torch.empty_like(ids)
    N.call("lkg_sanitize_ids_i64", ids.numel(), N.ptr(ids), 0, int(n_rows), N.ptr(scratch), N.ptr(bad), ops._stream())
    return bad


def _triples_on_device(what: str, h, r, t, dev=None):
    Q.check_triple_lists(h, r, t)
    ops._need_gpu(h, r, t)
    if dev is not None and h.device != dev:
        raise ValueError(f"{what}: the triples live on {h.device}, the known triples on {dev}")
    return ops._i64(h), ops._i64(r), ops._i64(t)


def answer_counts(known: KnownTriples, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, any_relation: bool = False
                  ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(n_tails, n_heads), int64[G] each: the distinct known tails of (h, r, ?) and the distinct known heads of (?, r, t)
    of every triple (lkg_answer_counts); any_relation: under any relation.  IndexError for an id out of range."""
    known = _check_known(known, "answer_counts")
    h, r, t = _triples_on_device("answer_counts", h, r, t, known.device)
    g = h.numel()
    out = torch.empty((2, g), dtype=torch.int64, device=known.device)
    if g == 0:
        return out[0], out[1]
    bad_e, bad_r = ops.count_ids_outside(known.n_entities, torch.cat((h, t))), ops.count_ids_outside(known.n_relations, r)
    if bad_e or bad_r:
        raise IndexError(f"answer_counts: {bad_e} entity id(s) outside [0, {known.n_entities}), {bad_r} relation id(s) "
                         f"outside [0, {known.n_relations})")
    rel = torch.full_like(r, -1) if any_relation else r
    N.call("lkg_answer_counts", g, N.ptr(h), N.ptr(rel), N.ptr(t), known.n_entities, *_structure(known.by_head),
           *_structure(known.by_tail), N.ptr(out[0]), N.ptr(out[1]), ops._stream())
    return out[0], out[1]


def subsampling_weights(known: KnownTriples, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, start: float = 4.0
                        ) -> torch.Tensor:
    """float32[G]: RotatE's / DGL-KE's subsampling weight 1 / sqrt(start + n_tails + n_heads) of every triple, from
    answer_counts -- computed in float64 and rounded once.  start > 0 and finite."""
    if isinstance(start, bool) or not isinstance(start, (int, float)) or not 0.0 < float(start) < float("inf"):
        raise ValueError(f"start must be a finite number > 0, got {start!r}")
    n_tails, n_heads = answer_counts(known, h, r, t)
    return (1.0 / torch.sqrt(float(start) + (n_tails + n_heads).double())).float()


@dataclass
class NegativeBatch:
    """The negatives of G positives: ``neg`` int64[G, K]; ``head_side`` bool[G], whether the group's negatives replace the
    head; ``unfiltered`` bool[G, K], the slots that kept their last candidate after MAX_TRIES rejections; ``n_unfiltered``
    their number on the host."""
    neg: torch.Tensor
    head_side: torch.Tensor
    unfiltered: torch.Tensor
    n_unfiltered: int


def _check_pool(pool, n_entities: int, which: str):
    if not isinstance(pool, torch.Tensor) or pool.dim() != 1 or pool.dtype != torch.int64 or pool.numel() == 0:
        raise ValueError(f"the {which} pool must be a non-empty 1-D int64 tensor of entity ids")
    bad = ops.count_ids_outside(n_entities, pool) if pool.is_cuda else int(((pool < 0) | (pool >= n_entities)).sum())
    if bad:
        raise IndexError(f"the {which} pool has {bad} entity id(s) outside [0, {n_entities})")
    return pool.contiguous()


class NegativeSampler:
    """Draws K negatives for each given positive (h, r, t) on the device (see the module docstring).

    corrupt      'tail', 'head', 'both' (a fair coin per triple) or 'bernoulli' (the head with probability
                 tph / (tph + hpt) of the triple's relation over ``known``; a relation without a known triple: the tail).
    known        the KnownTriples to filter by and to count the relations of; needed by filtered=True and by 'bernoulli'.
    filtered     reject a candidate that forms a known triple on the corrupted side (default: known is not None).
    any_relation "known" means known under any relation -- the rule of the 'dot' scoring, which ignores r.
    pool         an int64 tensor of entity ids, or a (tail_pool, head_pool) pair: the candidates, DRAWN BY POSITION
                 (pool[value % len(pool)]).  Duplicates are allowed and weigh an entity by its count (the reference's
                 training_tails distribution is pool = the training tails); a type constraint is a pool of unique ids.  The
                 result depends on the pool's ORDER: the same ids in another order give other negatives."""

    def __init__(self, n_entities: int, known: Optional[KnownTriples] = None, corrupt: str = "tail",
                 pool: Union[None, torch.Tensor, Tuple[torch.Tensor, torch.Tensor]] = None,
                 filtered: Optional[bool] = None, any_relation: bool = False):
        if isinstance(n_entities, bool) or not isinstance(n_entities, int) or not 1 <= n_entities < 2 ** 31 - 1:
            raise ValueError(f"n_entities must be an integer in [1, 2^31 - 1), got {n_entities!r}")
        if corrupt not in CORRUPT:
            raise ValueError(f"corrupt must be one of {CORRUPT}, got {corrupt!r}")
        if known is not None:
            _check_known(known, "NegativeSampler")
            if known.n_entities != n_entities:
                raise ValueError(f"known triples over {known.n_entities} entities, the sampler over {n_entities}")
        filtered = known is not None if filtered is None else bool(filtered)
        if filtered and known is None:
            raise ValueError("filtered=True needs the known triples (known=)")
        if corrupt == "bernoulli" and known is None:
            raise ValueError("corrupt='bernoulli' needs the known triples (known=) to count the relations of")
        if isinstance(pool, (tuple, list)):
            if len(pool) != 2:
                raise ValueError("pool must be a tensor of entity ids or a (tail_pool, head_pool) pair")
            pool = (_check_pool(pool[0], n_entities, "tail"), _check_pool(pool[1], n_entities, "head"))
        elif pool is not None:
            pool = (_check_pool(pool, n_entities, "candidate"),) * 2
        self.n_entities, self.known, self.corrupt, self.pool = n_entities, known, corrupt, pool
        self.filtered, self.any_relation = filtered, bool(any_relation)
        self.cardinalities = relation_cardinalities(known) if corrupt == "bernoulli" else None

    def sample(self, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, k: int, seed: Optional[int] = None,
               group_offset: int = 0) -> NegativeBatch:
        """K = k negatives for each of the G positives (h, r, t) (int64[G] on the device).  seed: an integer in
        [0, 2^64) (None: ops.new_seed()); group_offset: the index of the batch's first group in the stream -- a batch cut
        out of a longer list with its offset carried has the bits it has inside the whole.  IndexError for an id out of
        range.  One host sync: the error counts and n_unfiltered are read together."""
        for name, v, lo in (("k", k, 1), ("group_offset", group_offset, 0)):
            if isinstance(v, bool) or not isinstance(v, int) or v < lo:
                raise ValueError(f"{name} must be an integer >= {lo}, got {v!r}")
        if seed is not None and (isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 64):
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        known = self.known
        h, r, t = _triples_on_device("NegativeSampler.sample", h, r, t, known.device if known is not None else None)
        g, dev = h.numel(), h.device
        seed = ops.new_seed() if seed is None else seed
        out = torch.empty(g + g * k, dtype=torch.uint8, device=dev)     # head_side, then unfiltered
        neg = torch.empty((g, k), dtype=torch.int64, device=dev)
        head_side, unfiltered = out[:g].view(torch.bool), out[g:g + g * k].view(torch.bool).view(g, k)
        if g == 0:
            return NegativeBatch(neg, head_side, unfiltered, 0)
        bad = [_outside(self.n_entities, torch.cat((h, t)))]
        if known is not None:
            bad.append(_outside(known.n_relations, r))
        pools = [None, 0, None, 0]
        if self.pool is not None:
            self.pool = tuple(p.to(dev) for p in self.pool)
            pools = [N.ptr(self.pool[0]), self.pool[0].numel(), N.ptr(self.pool[1]), self.pool[1].numel()]
        sides = [N.ptr(x) for s in (known.by_head, known.by_tail) for x in s] if known is not None else [None] * 8
        card = self.cardinalities
        N.call("lkg_sample_negatives", g, k, seed, group_offset, N.ptr(h), N.ptr(r), N.ptr(t), self.n_entities,
               known.n_relations if known is not None else 0, CORRUPT.index(self.corrupt), int(self.filtered),
               int(self.any_relation), *sides, N.ptr(card.heads) if card else None, N.ptr(card.tails) if card else None,
               *pools, N.ptr(neg), N.ptr(out), N.ptr(out[g:]), ops._stream())
        counts = torch.cat([b.long() for b in bad] + [out[g:g + g * k].sum(dtype=torch.int64).reshape(1)]).tolist()
        if any(counts[:-1]):
            raise IndexError(f"NegativeSampler.sample: {counts[0]} entity id(s) outside [0, {self.n_entities})" +
                             (f", {counts[1]} relation id(s) outside [0, {known.n_relations})" if known is not None else ""))
        return NegativeBatch(neg, head_side, unfiltered, int(counts[-1]))


class TripleEpoch:
    """One epoch over the training triples: an iterator of (h, r, t, group_offset) batches of ``batch_groups`` positives
    (the last one shorter) in an order shuffled by ``seed``.  group_offset is the batch's position in that order, so
    NegativeSampler.sample(h, r, t, k, seed, group_offset) draws for a triple what it would draw under any other
    batch_groups: cutting the epoch into batches of 683 or of 8192 changes no negative."""

    def __init__(self, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, batch_groups: int, seed: int):
        Q.check_triple_lists(h, r, t)
        if isinstance(batch_groups, bool) or not isinstance(batch_groups, int) or batch_groups < 1:
            raise ValueError(f"batch_groups must be a positive integer, got {batch_groups!r}")
        if isinstance(seed, bool) or not isinstance(seed, int) or not 0 <= seed < 2 ** 63:
            raise ValueError(f"seed must be an integer in [0, 2^63), got {seed!r}")
        self.batch_groups, self.seed = batch_groups, seed
        order = torch.randperm(h.numel(), generator=torch.Generator().manual_seed(seed)).to(h.device)
        self.h, self.r, self.t = h[order], r[order], t[order]

    def __len__(self) -> int:
        return math.ceil(self.h.numel() / self.batch_groups)

    def __iter__(self):
        for lo in range(0, self.h.numel(), self.batch_groups):
            hi = lo + self.batch_groups
            yield self.h[lo:hi], self.r[lo:hi], self.t[lo:hi], lo


def sampled_negative_loss(model, h: torch.Tensor, r: torch.Tensor, t: torch.Tensor, batch: NegativeBatch,
                          weights: Optional[torch.Tensor] = None, margin: float = 0.0, scale: float = 1.0,
                          temperature: float = 1.0, reduction: str = "mean", scoring: Optional[str] = None) -> torch.Tensor:
    """The self-adversarial loss of the triples (h, r, t) against a NegativeBatch whose groups may be corrupted on either
    side.  A batch corrupted on one side only IS self_adversarial_loss(..., side, reduction='none') on it.  A mixed batch
    splits its groups by batch.head_side: the ids are checked and the table is taken ONCE (one encoder pass), each side's
    groups are gathered, projected and scored for themselves exactly as self_adversarial_loss does on that side's groups
    alone -- the same bits, group for group -- and the two results go back into group order.  weights (float[G], e.g.
    subsampling_weights; None: all 1): 'none' returns the unweighted float32[G], 'sum' is sum(w L), 'mean' is
    sum(w L) / sum(w).  margin, scale, temperature, scoring and the refusals ('mlp', ShardedLiteralKG) are
    self_adversarial_loss's."""
    from .self_adversarial import (MLP_MESSAGE, SHARDED_MESSAGE, check_temperature, losses_by_side,
                                   self_adversarial_loss)
    check_single_device(model, SHARDED_MESSAGE)
    scoring = Q.resolve_scoring(model, scoring, MLP_MESSAGE)
    Q.check_transr_model(model, scoring)
    reduction = check_reduction(reduction)
    scale = ops.check_softmax_args(scale, None)[0]
    margin, temperature = check_margin(margin), check_temperature(temperature)
    Q.check_triple_lists(h, r, t)
    g = h.numel()
    if not isinstance(batch, NegativeBatch) or batch.neg.dim() != 2 or batch.neg.shape[0] != g or \
            batch.neg.dtype.is_floating_point or (g > 0 and batch.neg.shape[1] < 1) or batch.head_side.shape != (g,) or \
            batch.head_side.dtype != torch.bool:
        raise ValueError(f"batch must be the NegativeBatch of these {g} triples (neg [G, K] with K >= 1, head_side bool[G])")
    if weights is not None and (not isinstance(weights, torch.Tensor) or weights.shape != (g,) or
                                not weights.dtype.is_floating_point):
        raise ValueError(f"weights must be a float tensor with one weight per triple ({g})")
    dev = model.entity_embed.weight.device
    h, r, t, neg, head_side = (x.to(dev) for x in (h, r, t, batch.neg, batch.head_side))
    head = head_side.nonzero()[:, 0]
    if head.numel() in (0, g):                       # one side only: the groups as they are
        loss = self_adversarial_loss(model, h, r, t, neg, side="head" if g and head.numel() == g else "tail", margin=margin,
                                     scale=scale, temperature=temperature, reduction="none", scoring=scoring)
    else:
        tail = (~head_side).nonzero()[:, 0]
        parts = losses_by_side(model, scoring, h, r, t, neg, [("tail", tail), ("head", head)], margin, scale, temperature)
        back = torch.empty(g, dtype=torch.int64, device=dev)
        back[torch.cat((tail, head))] = torch.arange(g, device=dev)
        loss = torch.cat(parts)[back]
    if reduction == "none":
        return loss
    if weights is None:
        return loss.mean() if reduction == "mean" else loss.sum()
    weights = weights.to(loss.device, torch.float32)
    total = (weights * loss).sum()
    return total / weights.sum() if reduction == "mean" else total
