"""KvsAll training: one row per query (h, r, ?) scored against EVERY entity, the target the multi-hot vector of all the
query's known answers, the loss binary cross-entropy with logits (ConvE, LibKGE's ``KvsAll``) -- the objective for graphs
where a query has many true answers, next to the softmax objectives of ``one_vs_all.py``, which learn from one answer per
row and pay one row per triple.

For a query (ent, r) and side 'tail' the row is q = P[ent] + e_r and the positives are the known tails of (ent, r, ?); for
side 'head' q = P[ent] - e_r and the positives are the known heads of (?, r, ent) ('dot': q = P[ent], no relation, the
positives known under ANY relation).  The logit of candidate c is

    z_c = scale * (margin - ||q - P[c]||^2)     ('transe', 'transr')
    z_c = scale * (margin + q . P[c])           ('dot')

and the loss of the row is  sum_c softplus(z_c) - y'_c z_c  with  y' = (1 - label_smoothing) y + label_smoothing / n  over
the n candidates -- the SUM over candidates (LibKGE's convention); ``reduction`` acts over the rows.  A sigmoid does not
cancel the row constant ||q||^2 as a softmax does: it goes in as the per-row bias  scale (margin - ||q||^2)  of
``sigmoid_all_loss``, differentiable like q itself.

Device code: lkg_kvsall.hip -- the ranking kernels' tile with a running sum of softplus terms (forward, two launches,
nothing of size B x N stored) and the weights V = scale beta g (sigma(z) - y') recomputed chunk by chunk in the backward
pass.  The positives' lists come from ops.softmax_excluded with truth = -1 (no entry is exempt, so it returns every known
answer that is a candidate, sorted and unique).  ``candidates`` restricts the rows scored exactly as in one_vs_all_loss; a
positive that is not a candidate is simply absent.  P is the full table of the step: ``prune_to_batch`` does not apply.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd import Function

from . import _native as N
from . import _objectives as O
from . import _queries as Q
from . import ops
from ._objectives import check_margin      # noqa: F401  (its home before _objectives.py)
from .gemm_ordered import check_route, current_route, keyword_route

MLP_MESSAGE = ("scoring='mlp' has no KvsAll loss: the pair head is trained by train_MLP on labelled pairs -- use 'transr', "
               "'transe' or 'dot'")
SHARDED_MESSAGE = ("the KvsAll loss scores every entity of the whole table: the row-sharded model holds a block of it per "
                   "rank (train KvsAll on a single-device LiteralKG)")


def check_label_smoothing(eps) -> float:
    if isinstance(eps, bool) or not isinstance(eps, (int, float)) or not 0.0 <= float(eps) < 1.0:
        raise ValueError(f"label_smoothing must be a number in [0, 1), got {eps!r}")
    return float(eps)


def sigmoid_all_forward(q: torch.Tensor, p: torch.Tensor, pn: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                        positives=None, scale: float = 1.0, label_smoothing: float = 0.0,
                        splits: Optional[int] = None) -> torch.Tensor:
    """loss float32[B] of lkg_sigmoid_all_partial_f32 + lkg_sigmoid_all_finish_f32, no autograd: the logits are
    z = -scale (pn[c] - 2 q.p_c) + bias with pn = ops.rank_sqnorm(p), or scale q.p_c + bias with pn None (bias None: 0);
    loss_i = sum_c softplus(z) - y' z with y = 1 on the positions positives = (yptr, ycol) list for row i."""
    q, p, _, bias = ops.all_entity_operands("sigmoid_all_forward", q, p, pn, bias=bias)
    scale, splits, _ = ops.check_softmax_args(scale, splits)
    eps = check_label_smoothing(label_smoothing)
    (b, k), n, dev = q.shape, p.shape[0], q.device
    yptr, ycol = ops.list_pair("sigmoid_all_forward", "positives", positives, b)
    loss = torch.empty(b, dtype=torch.float32, device=dev)
    if b == 0:
        return loss
    s_ = ops.softmax_all_splits(b, n, splits)
    ws = torch.empty((s_, b), dtype=torch.float32, device=dev)
    N.call("lkg_sigmoid_all_partial_f32", b, n, k, N.ptr(q), ops._ld(q), N.ptr(p), ops._ld(p), N.ptr(pn), N.ptr(bias), scale,
           eps, s_, N.ptr(yptr), N.ptr(ycol), ycol.numel() if ycol is not None else 0, N.ptr(ws), ops._stream())
    N.call("lkg_sigmoid_all_finish_f32", b, s_, N.ptr(ws), N.ptr(loss), ops._stream())
    return loss


def sigmoid_all_weights(q: torch.Tensor, p: torch.Tensor, pn: Optional[torch.Tensor], bias: Optional[torch.Tensor],
                        g: torch.Tensor, positives=None, scale: float = 1.0, label_smoothing: float = 0.0, c0: int = 0,
                        c1: Optional[int] = None, out: Optional[torch.Tensor] = None,
                        rowsum: Optional[torch.Tensor] = None) -> torch.Tensor:
    """V[:, c0:c1] of lkg_sigmoid_all_weights_f32 (B x (c1 - c0), into ``out`` when given, whose row stride is free):
    V[i, c] = scale beta g[i] (sigma(z_ic) - y'_ic), beta = 1 with pn, 1/2 without.  The lists hold positions of the whole
    table and the n of the smoothing is the whole table's, whatever the chunk.  rowsum (optional, contiguous float32
    [ceil((c1 - c0) / 256), B]): receives per 256-candidate tile of the chunk the sum of V's row over that tile."""
    q, p, _, bias = ops.all_entity_operands("sigmoid_all_weights", q, p, pn, bias=bias)
    ops._need_gpu(g, out)
    scale = ops.check_softmax_args(scale, 0)[0]
    eps = check_label_smoothing(label_smoothing)
    (b, k), n = q.shape, p.shape[0]
    yptr, ycol = ops.list_pair("sigmoid_all_weights", "positives", positives, b)
    c0, c1 = ops.chunk_range("sigmoid_all_weights", c0, c1, n)
    g = g.reshape(-1).contiguous()
    if g.numel() != b or g.dtype != torch.float32:
        raise ValueError(f"sigmoid_all_weights: g must be float32[{b}]")
    out = ops.weights_out("sigmoid_all_weights", out, b, c1 - c0, q.device)
    if b == 0:
        return out
    if rowsum is not None:
        ops._need_gpu(rowsum)
        if tuple(rowsum.shape) != ((c1 - c0 + 255) // 256, b) or rowsum.dtype != torch.float32 or not rowsum.is_contiguous():
            raise ValueError(f"sigmoid_all_weights: rowsum must be a contiguous float32 {(c1 - c0 + 255) // 256} x {b} tensor")
    N.call("lkg_sigmoid_all_weights_f32", b, c1 - c0, k, N.ptr(q), ops._ld(q), N.ptr(p[c0:c1]), ops._ld(p),
           N.ptr(pn[c0:c1]) if pn is not None else None, N.ptr(bias), c0, n, N.ptr(g), scale, eps, N.ptr(yptr),
           N.ptr(ycol), ycol.numel() if ycol is not None else 0, N.ptr(out), max(ops._ld(out), c1 - c0), N.ptr(rowsum),
           ops._stream())
    return out


class _SigmoidAllLoss(Function):
    """loss_i = sum_c softplus(z_ic) - y'_ic z_ic over ALL rows of p.  Forward: two launches, nothing of size B x N.  Backward:
    ops.all_entity_backward, the loop of the softmax loss, with the weights V of lkg_sigmoid_all_weights_f32; its
    per-chunk hook adds dbias = rowsum(V) / (scale beta).  The weights kernel leaves
    the row sums of its tiles as it stores them, lkg_sigmoid_all_finish_f32 adds a chunk's tiles in float64, the chunks are
    added in float64 (a column of ones next to P in the dQ product was tried first: away from the positives V has one
    sign, and the f32 MFMA chain's error grew with the chain's length).  V has the same bits with or without the row
    sums, so no gradient's bits depend on which others are needed; a gradient nobody needs is None and its product is not
    launched."""

    @staticmethod
    def forward(ctx, q, p, bias, yptr, ycol, distance, scale, eps, splits, chunk_bytes):
        q_, p_, _, bias_ = ops.all_entity_operands("sigmoid_all_loss", q, p, bias=bias)
        pn = ops.rank_sqnorm(p_) if distance else None
        positives = (yptr, ycol) if yptr is not None else None
        loss = sigmoid_all_forward(q_, p_, pn, bias_, positives, scale, eps, splits)
        ctx.save_for_backward(q_, p_, pn, bias_, yptr, ycol)
        ctx.meta = (scale, eps, chunk_bytes, bias.shape if bias is not None else None)
        ctx.route = current_route()              # the backward follows the forward's choice wherever it is called
        return loss

    @staticmethod
    def backward(ctx, g):
        q, p, pn, bias, yptr, ycol = ctx.saved_tensors
        positives = (yptr, ycol) if yptr is not None else None
        scale, eps, chunk_bytes, bias_shape = ctx.meta
        want_q, want_p = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        want_b = bias is not None and ctx.needs_input_grad[2]
        b, dev = q.shape[0], q.device
        g = g.reshape(-1).float().contiguous()
        width = ops.softmax_chunk_width(b, p.shape[0], chunk_bytes)
        if want_b:
            rows = torch.zeros(b, dtype=torch.float64, device=dev)
            tiles = torch.empty(((width + 255) // 256, b), dtype=torch.float32, device=dev)
            part = torch.empty(b, dtype=torch.float32, device=dev)

        def fill(c0, c1, out):
            return sigmoid_all_weights(q, p, pn, bias, g, positives, scale, eps, c0, c1, out=out,
                                       rowsum=tiles[:(c1 - c0 + 255) // 256] if want_b else None)

        def add_row_sums(c0, c1):
            N.call("lkg_sigmoid_all_finish_f32", b, (c1 - c0 + 255) // 256, N.ptr(tiles), N.ptr(part), ops._stream())
            rows.add_(part)

        dq, dp = ops.all_entity_backward(q, p, pn, width, want_q, want_p, fill, add_row_sums if want_b else None,
                                         route=ctx.route)
        sb = scale if pn is not None else 0.5 * scale
        dbias = (rows / sb).float().reshape(bias_shape) if want_b else None
        return (dq, dp, dbias) + (None,) * 7


def sigmoid_all_loss(q: torch.Tensor, p: torch.Tensor, bias: Optional[torch.Tensor], positives=None, distance: bool = True,
                     scale: float = 1.0, label_smoothing: float = 0.0, splits: Optional[int] = None,
                     chunk_bytes: int = ops.SOFTMAX_CHUNK_BYTES, products: str = "engine") -> torch.Tensor:
    """float32[B]: binary cross-entropy with logits of ALL N rows of p for query row q[i], summed over the candidates, the
    target 1 on the positions positives = (yptr int32[B + 1], ycol int32[M]) list for the row (sorted, unique; None: no
    positive anywhere) and 0 elsewhere, smoothed to (1 - label_smoothing) y + label_smoothing / N.  distance True: logits
    z = -scale (||p_c||^2 - 2 q.p_c) + bias_i -- hand in bias_i = scale (margin - ||q_i||^2) for scale (margin -
    ||q_i - p_c||^2); False: z = scale q.p_c + bias_i.  bias float32[B] or None (0).  Differentiable in q, p and bias; the
    gradient of p is a dense N x k table.  splits: candidate splits of the forward pass (None: automatic) -- the last bits
    of the loss may depend on it, for a given value they do not change from run to run.  chunk_bytes bounds the backward's
    B x Nc weights.  products "ordered": the backward's dQ product runs on gemm_ordered (gemm_ordered.keyword_route;
    ops.all_entity_backward says what changes); the loss, dP and dbias keep their bits."""
    with keyword_route(products):
        scale, splits, chunk_bytes = ops.check_softmax_args(scale, splits, chunk_bytes)
        eps = check_label_smoothing(label_smoothing)
        ops._need_gpu(q, p, bias)
        yptr, ycol = ops.list_pair("sigmoid_all_loss", "positives", positives, q.shape[0])
        return _SigmoidAllLoss.apply(q, p, bias, yptr, ycol, bool(distance), scale, eps, splits, chunk_bytes)


def distinct_queries(ent: torch.Tensor, r: torch.Tensor):
    """(ent, r) of the distinct pairs, ordered by (relation, entity): the rows a KvsAll step scores for a batch of triples
    -- a query with m answers in the batch is one row, not m."""
    Q.check_id_pair(ent, r, ("ent", "r"))
    pairs = torch.unique(torch.stack((r.long(), ent.long()), dim=1), dim=0)
    return pairs[:, 1].contiguous(), pairs[:, 0].contiguous()


def kvs_all_loss(model, ent: torch.Tensor, r: torch.Tensor, known, side: str = "tail", margin: float = 0.0,
                 scale: float = 1.0, label_smoothing: float = 0.0, reduction: str = "mean", scoring: Optional[str] = None,
                 splits: Optional[int] = None, candidates: Optional[torch.Tensor] = None,
                 products: str = "engine") -> torch.Tensor:
    """The KvsAll loss of the queries (ent, r) under the model (see the module docstring): one row per GIVEN query
    (duplicates get equal values; distinct_queries gives the unique pairs of a batch), side 'tail' ((ent, r, ?), the
    positives known's tails) or 'head' ((?, r, ent), its heads), margin any finite number, scale > 0, label_smoothing in
    [0, 1), reduction 'mean' / 'sum' / 'none' over the rows (a row is the SUM over its candidates), scoring 'transr' /
    'transe' / 'dot' (default: model.scoring), splits as in one_vs_all_loss.  known: the KnownTriples the positives are
    read from.  candidates: the unique entity ids scored (n = their number; a positive that is not among them is simply
    absent).  products as in sigmoid_all_loss.  Differentiable in every parameter the table, the relation embeddings and
    (transr) gat_trans_M depend on."""
    check_route(products)
    O.check_single_device(model, SHARDED_MESSAGE)
    side = Q.check_one_side(side, "a KvsAll row is one side's query")
    scoring = Q.resolve_scoring(model, scoring, MLP_MESSAGE)
    reduction = O.check_reduction(reduction)
    scale, splits, _ = ops.check_softmax_args(scale, splits)
    margin, eps = check_margin(margin), check_label_smoothing(label_smoothing)
    Q.check_id_pair(ent, r, ("ent", "r"))
    Q.check_transr_model(model, scoring)
    if known is None or not hasattr(known, "for_side"):
        raise ValueError("known must be the KnownTriples the positives of each query are read from")
    Q.check_known_entities(known, model)
    if candidates is not None:
        Q.check_ids("candidates", candidates)
    dev = model.entity_embed.weight.device
    if ent.numel() == 0:
        return O.empty_loss(model, reduction)
    (ent,) = ops.checked_ids(model.n_entities, ent.to(dev))                 # (out-of-range ids never reach a kernel)
    (r,) = ops.checked_ids(model.n_relations, r.to(dev), what="relation")
    Q.check_known_device(known, dev)
    cand, pos = O.candidate_block(model, candidates, dev)
    distance = scoring != "dot"

    def score_group(table, rows, w, r, ent):
        """the loss of the queries (ent, r) of one projection"""
        p = O.projected(rows, w)                                # alive until the backward pass (transr: N x relation_dim)
        q = O.query_rows(model, scoring, side, table, p, w, ent, r, pos)
        if distance:
            bias = scale * (margin - (q * q).sum(1))            # ||q||^2 does not cancel under a sigmoid: differentiable
        else:
            bias = torch.full((ent.numel(),), scale * margin, dtype=torch.float32, device=ent.device)
        none = torch.full_like(ent, -1)                          # no truth to exempt: every known answer is listed
        positives = ops.softmax_excluded(known.for_side(side), ent, O.known_relations(scoring, r), none, p.shape[0], pos)
        return sigmoid_all_loss(q, p, bias, positives, distance=distance, scale=scale, label_smoothing=eps, splits=splits,
                                products=products)

    return O.all_entity_loss(model, scoring, r, (ent,), cand, reduction, score_group)
