"""Drop-in ``LiteralKG`` module for MI355X: the reference's nn.Module surface
(``LiteralKG(args, n_entities, n_relations, A_in, numerical_literals, text_literals)``;
``model(*input, device=, mode=)``; same ``state_dict`` keys, model.py:167-263, 521-532) over the
HIP kernels of ``include/literalkg_hip.h``.

Differences in *structure* (results are the reference's):
  * ``A_in`` stays a sparse COO ``nn.Parameter`` for ``state_dict`` / checkpoint interchange, but the
    kernels read a destination-sorted int32 CSR (+ CSC for the backward) built once per pattern and a
    flat fp32 value array that aliases ``A_in``'s values (``graph.py``);
  * ``update_att`` runs fused on the device (no ``.cpu()`` round trip, model.py:470);
  * ``gat_trans_M[r]`` is never gathered into a B x C x D tensor (model.py:372): the batch is grouped
    by relation and projected by one grouped MFMA GEMM;
  * the gate never concatenates ``[x | num | txt]`` (gate.py:23).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import torch
import torch.nn as nn

from . import ops, pruned
from .gate import Gate, GateMul
from .graph import KGStructure


class AttentionCSR:
    """What an aggregation layer needs of A_in on the device: pattern + values in CSR and CSC order."""

    def __init__(self, graph: KGStructure, val: torch.Tensor, val_t: Optional[torch.Tensor] = None):
        self.graph = graph
        self.val = val
        self.val_t = val_t if val_t is not None else (
            ops.permute_values(val, graph.t_perm) if graph.t_perm is not None and val.is_cuda else None)

    def aggregate(self, ego: torch.Tensor, plus_self: bool = False, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A_in @ ego  (plus_self: ego + A_in @ ego in the same pass; bias: a row added to every output row)."""
        return ops.aggregate(ego, self.graph, self.val, self.val_t, plus_self, bias)


class _KeepingAttention:
    """A_in for the FIRST layer: its aggregation also produces the copy of the layer input that gat_embeddings keeps
    as slot 0 of the concatenated table (ops._AggregateKeep), forward copy and backward sum fused into the SpMM."""

    def __init__(self, att: AttentionCSR, keep_dst: torch.Tensor):
        self.att, self.keep_dst, self.kept = att, keep_dst, None

    def aggregate(self, ego: torch.Tensor, plus_self: bool = False) -> torch.Tensor:
        a = self.att
        if self.kept is not None:                 # a layer that aggregates twice keeps once
            return a.aggregate(ego, plus_self)
        side, self.kept = ops.aggregate_keep(ego, a.graph, a.val, a.val_t, plus_self, self.keep_dst)
        return side


def _xavier(linear: nn.Linear) -> nn.Linear:
    nn.init.xavier_uniform_(linear.weight)
    return linear


class Aggregator(nn.Module):
    """One aggregation layer (model.py:12-164): side = A_in @ ego, then the type-specific dense part,
    LeakyReLU, LayerNorm, dropout.  Parameter names/shapes are the reference's."""

    def __init__(self, in_dim, out_dim, dropout, aggregator_type, use_residual=False, args=None):
        super().__init__()
        self.in_dim, self.out_dim = in_dim, out_dim
        self.dropout = dropout
        self.aggregator_type = aggregator_type
        self.use_residual = bool(use_residual)
        kind = aggregator_type
        if kind not in ("gcn", "graphsage", "bi-interaction", "gin"):
            raise NotImplementedError(kind)
        mix_dim = args.mlp_hidden_dim if kind == "gin" else in_dim
        # identity-mapping matrix of the GCNII-style residual; always registered (model.py:21, 61)
        self.weight = nn.Parameter(torch.empty(mix_dim, mix_dim))
        bound = 1.0 / math.sqrt(out_dim)
        nn.init.uniform_(self.weight, -bound, bound)   # reference leaves the gin variant uninitialised
        if self.use_residual or kind == "gin":
            self.linear_h0 = _xavier(nn.Linear(args.embed_dim, mix_dim))
        self.layer_normalize = nn.LayerNorm(out_dim)
        if kind == "gcn":
            self.linear = _xavier(nn.Linear(in_dim, out_dim))
        elif kind == "graphsage":
            if self.use_residual:
                self.linear_h = _xavier(nn.Linear(2 * in_dim, in_dim))
                self.linear = _xavier(nn.Linear(in_dim, out_dim))
            else:
                self.linear = _xavier(nn.Linear(2 * in_dim, out_dim))
        elif kind == "bi-interaction":
            self.linear1 = _xavier(nn.Linear(in_dim, out_dim))
            self.linear2 = _xavier(nn.Linear(in_dim, out_dim))
        else:   # gin: an MLP on (ego + side); its Linears keep torch's default init like the reference
            self.num_layers = args.n_mlp_layers
            if self.num_layers == 1:
                self.linear = nn.Linear(in_dim, out_dim)
            else:
                hid = args.mlp_hidden_dim
                self.inp_linear = nn.Linear(in_dim, hid)
                self.linears = nn.ModuleList(nn.Linear(hid, hid) for _ in range(self.num_layers - 1))
                self.out_linear = nn.Linear(hid, out_dim)
                self.mlp_layer_norms = nn.ModuleList(nn.LayerNorm(hid) for _ in range(self.num_layers - 1))
        # reference_association (args, default False): evaluate a residual layer as the reference writes it --
        # Linear(mixed @ W') with W' = (1 - b) + b W (model.py:95-98), two N-row products -- instead of the device's fold
        # mixed @ (W_lin W'^T)^T.  Same function; a parity run on an ill-conditioned residual configuration (W' has near-equal
        # entries, LayerNorm removes their common part) then rounds where the reference rounds.
        self.reference_association = bool(getattr(args, "reference_association", False))
        self.last_normalized = None
        self.h0_projection = None   # set by the encoder for the duration of a pass: linear_h0(h0) of this layer
        self.norm_out = None   # set by the encoder: the concat-buffer slice the normalised copy goes to
        self.want_output = True   # ... and False for the last layer: nobody reads its un-normalised output

    # (1-a) hi + a W0 h0, then @ ((1-b) + b W)   -- (1-b) lands on every entry of W (model.py:96)
    def residual_connection(self, hi, h0, lamda, alpha, l):
        if not self.use_residual:
            return hi
        # linear_h0(h0): handed in by the encoder (all layers' projections of the same h0 as ONE product, and one copy for
        # both branches of bi-interaction) or computed here
        h0p = self.h0_projection if self.h0_projection is not None else \
            ops.linear(h0, self.linear_h0.weight, self.linear_h0.bias)
        mixed = ops.axpby(hi, h0p, 1 - alpha, alpha)
        beta = math.log(lamda / l + 1)
        return ops.matmul(mixed, ops.axpby(self.weight, None, beta, 1 - beta))

    @staticmethod
    def _lin(mod: nn.Linear, x):
        return ops.linear(x, mod.weight, mod.bias)

    def _identity_map(self, lamda, l):
        """(1 - b) + b W, b = ln(lamda / l + 1): the GCNII-style identity mapping (model.py:95-96)."""
        beta = math.log(lamda / l + 1)
        return ops.axpby(self.weight, None, beta, 1 - beta)

    def _lin_mapped(self, mod: nn.Linear, mixed, wp):
        """mod(mixed @ wp) as ONE product over the rows: mixed @ (wp @ W^T) + b -- the two weight matrices are multiplied
        first (d x d x out: nothing), the N-row product runs once, at the Linear's output width (for the 300-wide first layer
        of main.py's defaults: 1 M x 300 x 32 instead of 1 M x 300 x 300 and then 1 M x 300 x 32, forward and backward).
        Same value up to fp32 rounding order."""
        if self.reference_association:
            return ops.linear(ops.matmul(mixed, wp), mod.weight, mod.bias)
        # (the fold of the two small matrices in float64, rounded once: its fp32 dot products' accumulated rounding would be the
        #  device path's own contribution to the error of an ill-conditioned configuration)
        return ops.linear(mixed, ops.fold_nt(mod.weight, wp) if mixed.is_cuda else ops.matmul(mod.weight, wp.t()), mod.bias)

    def _res_lin(self, mod: nn.Linear, hi, h0, lamda, alpha, l):
        """mod(residual_connection(hi)), with the identity mapping folded into the Linear's weight on the device path."""
        if not self.use_residual:
            return self._lin(mod, hi)
        h0p = self.h0_projection if self.h0_projection is not None else \
            ops.linear(h0, self.linear_h0.weight, self.linear_h0.bias)
        return self._lin_mapped(mod, ops.axpby(hi, h0p, 1 - alpha, alpha), self._identity_map(lamda, l))

    def _finish(self, z, extra_sum=None, slope=ops.LEAKY_SLOPE):
        """LeakyReLU -> LayerNorm -> message dropout, plus the L2-normalised copy of the result that
        gat_embeddings concatenates (model.py:161, 305) -- one fused kernel."""
        ln = self.layer_normalize
        p = float(self.dropout) if self.training else 0.0
        if extra_sum is not None:   # gin skip-sum: LN(act(z)) + earlier layers, then LN again (model.py:151-161)
            inner, _ = ops.act_layernorm(z, ln.weight, ln.bias, want_norm=False)
            z = inner
            for e in extra_sum:
                z = ops.axpby(z, e)
            slope = 1.0   # the second LayerNorm has no activation in front: slope 1 = identity
        y, yn = ops.act_layernorm(z, ln.weight, ln.bias, want_norm=True, slope=slope, drop_p=p, yn_out=self.norm_out,
                                  want_y=self.want_output)
        self.last_normalized = yn
        return y

    def _linear_finish(self, xs, ws, bias):
        """_finish(sum_i x_i @ w_i^T + bias): ONE launch where ops.fused_layer_wanted says so (by default: evaluation, rows of
        129-256 columns), else the tall GEMM followed by the row-wise kernel (same bits either way)."""
        ln = self.layer_normalize
        if len(xs) == 1 and ops.narrow_layer_ok(xs[0], ws[0]):      # 32 -> 32: the dense backward in one launch
            p = float(self.dropout) if self.training else 0.0
            y, yn = ops.narrow_layer(xs[0], ws[0], bias, ln.weight, ln.bias, want_norm=True, drop_p=p, yn_out=self.norm_out,
                                     want_y=self.want_output)
            self.last_normalized = yn
            return y
        if ops.fused_layer_wanted(xs, ws, (bias, ln.weight, ln.bias)):
            p = float(self.dropout) if self.training else 0.0
            y, yn = ops.linear_act_layernorm(xs, ws, bias, ln.weight, ln.bias, want_norm=True, drop_p=p, yn_out=self.norm_out,
                                             want_y=self.want_output)
            self.last_normalized = yn
            return y
        return self._finish(ops.multi_linear(xs, ws, bias))

    def narrows(self) -> bool:
        """A gcn layer of at most half its input's width (the reference's default 300 -> 32): it projects first and aggregates
        out_dim columns (forward below)."""
        return self.aggregator_type == "gcn" and not self.use_residual and 2 * self.out_dim <= self.in_dim

    def forward(self, ego_embeddings, A_in: AttentionCSR, all_layers, lamda, alpha, l):
        ego = ego_embeddings
        h0 = all_layers[0]
        kind = self.aggregator_type
        if kind == "gcn":   # ego + side comes out of the SpMM directly
            att = getattr(A_in, "att", A_in)         # (layer 1 arrives wrapped: _KeepingAttention)
            if self.narrows() and isinstance(att, AttentionCSR):
                # a layer that narrows (the reference's default: 300 -> 32): (ego + A ego) W^T + b = p + A p + b with
                # p = ego W^T -- the aggregation gathers out_dim columns per entry instead of in_dim, forward and backward.
                # Same sums in another order (fp32 rounding only); the bias rides in the SpMM's epilogue.
                p = ops.linear(ego, self.linear.weight, None)
                return self._finish(att.aggregate(p, True, bias=self.linear.bias))
            if not self.use_residual:
                return self._linear_finish((A_in.aggregate(ego, True),), (self.linear.weight,), self.linear.bias)
            z = self._res_lin(self.linear, A_in.aggregate(ego, True), h0, lamda, alpha, l)
            return self._finish(z)
        if kind == "gin":
            return self._gin(ego, A_in.aggregate(ego, True), h0, all_layers, lamda, alpha, l)
        side = A_in.aggregate(ego)
        if kind == "graphsage":
            if self.use_residual:
                wh = self.linear_h.weight
                hi = ops.multi_linear((ego, side), (wh[:, :self.in_dim], wh[:, self.in_dim:]), self.linear_h.bias)
                z = self._res_lin(self.linear, hi, h0, lamda, alpha, l)
            else:   # Linear over [ego | side] as two accumulating GEMMs, no cat
                w = self.linear.weight
                return self._linear_finish((ego, side), (w[:, :self.in_dim], w[:, self.in_dim:]), self.linear.bias)
            return self._finish(z)
        if kind == "bi-interaction":
            # sum, product and (with the residual) both mixes (1 - a) hi + a linear_h0(h0) in ONE kernel, one for their
            # backward; the identity-mapping matrix (1 - b) + b W once for both branches
            h0p = None
            if self.use_residual:
                h0p = self.h0_projection if self.h0_projection is not None else \
                    ops.linear(h0, self.linear_h0.weight, self.linear_h0.bias)
            ms, mp = ops.bi_mix(ego, side, h0p, alpha)
            if self.use_residual:
                wp = self._identity_map(lamda, l)
                s, b = self._lin_mapped(self.linear1, ms, wp), self._lin_mapped(self.linear2, mp, wp)
            else:
                s, b = self._lin(self.linear1, ms), self._lin(self.linear2, mp)
            # LeakyReLU is applied per branch BEFORE the sum (model.py:125-130): one kernel, then a slope-1
            # epilogue for the LayerNorm
            return self._finish(ops.leaky_relu_sum(b, s), slope=1.0)
        raise NotImplementedError(kind)

    def _gin(self, ego, ego_plus_side, h0, all_layers, lamda, alpha, l):
        """model.py:131-158"""
        if self.num_layers == 1:
            raise AttributeError("gin with n_mlp_layers == 1 cannot run in the reference either "
                                 "(inp_linear/out_linear are never created, model.py:66-68, 133)")
        stack = self._lin(self.inp_linear, ego)
        h = self._lin(self.inp_linear, ego_plus_side)
        for lin, norm in zip(self.linears, self.mlp_layer_norms):
            h, _ = ops.act_layernorm(self._lin(lin, h), norm.weight, norm.bias, want_norm=False)
            stack = ops.axpby(stack, h)
        z = self._res_lin(self.out_linear, stack, h0, lamda, alpha, l)
        if len(all_layers) > 1:
            return self._finish(z, extra_sum=list(all_layers[1:]))
        return self._finish(z)


class LiteralKG(nn.Module):
    """See module docstring.  ``scoring``: 'transr' = model.py:364-428 (default), 'transe' =
    model_bce.py:329-368 (no ``gat_trans_M``; needs the encoder width to equal ``relation_dim``)."""

    def __init__(self, args, n_entities, n_relations, A_in=None, numerical_literals=None, text_literals=None,
                 scoring: str = "transr"):
        super().__init__()
        if scoring not in ("transr", "transe"):
            raise ValueError(scoring)
        self.scoring = scoring
        self.args = args
        self.use_pretrain = args.use_pretrain
        self.device = args.device
        self.n_entities, self.n_relations = n_entities, n_relations
        self.id_space = n_entities        # ids callers may hand in: [0, id_space) (a row-sharded module: the GLOBAL entity count)
        self.embed_dim, self.relation_dim = args.embed_dim, args.relation_dim
        self.scale_gat_dim = args.scale_gat_dim
        self.use_residual, self.alpha, self.lamda = args.use_residual, args.alpha, args.lamda
        self.aggregation_type = args.aggregation_type
        self.n_layers = args.n_conv_layers
        self.conv_dim_list = [args.embed_dim] + [args.conv_dim] * self.n_layers
        self.total_conv_dim = sum(self.conv_dim_list)
        self.mess_dropout = [args.mess_dropout] * self.n_layers
        self.kg_l2loss_lambda = args.kg_l2loss_lambda
        self.prediction_l2loss_lambda = args.fine_tuning_l2loss_lambda
        self.pre_training_neg_rate = args.pre_training_neg_rate
        self.fine_tuning_neg_rate = args.fine_tuning_neg_rate
        self.n_num_lit, self.n_txt_lit = args.num_lit_dim, args.txt_lit_dim
        self.milestone_score = args.milestone_score

        self.entity_embed = nn.Embedding(n_entities, self.embed_dim)
        self.relation_embed = nn.Embedding(n_relations, self.relation_dim)
        out_width = self.total_conv_dim
        if self.scale_gat_dim is not None:
            self.linear_gat = _xavier(nn.Linear(self.total_conv_dim, self.scale_gat_dim))
            out_width = self.scale_gat_dim
        self.out_width = out_width
        if scoring == "transr":
            self.gat_trans_M = nn.Parameter(torch.empty(n_relations, out_width, self.relation_dim))
            nn.init.xavier_uniform_(self.gat_trans_M)
        nn.init.xavier_uniform_(self.entity_embed.weight)
        nn.init.xavier_uniform_(self.relation_embed.weight)

        self.numerical_literals_embed = numerical_literals
        self.text_literals_embed = text_literals
        if args.use_num_lit and args.use_txt_lit:
            self.emb_mul_lit = GateMul(self.embed_dim, self.n_num_lit, self.n_txt_lit)
        elif args.use_num_lit:
            self.emb_num_lit = Gate(self.embed_dim, self.n_num_lit)
        elif args.use_txt_lit:
            self.emb_txt_lit = Gate(self.embed_dim, self.n_txt_lit)

        self.aggregator_layers = nn.ModuleList(
            Aggregator(self.conv_dim_list[k], self.conv_dim_list[k + 1], self.mess_dropout[k], self.aggregation_type,
                       self.use_residual, args) for k in range(self.n_layers))

        if scoring == "transe" and self.scale_gat_dim is not None:
            self.initialize_MLP()     # model_bce.py builds the MLP head in its constructor (255-260)

        # sparse, non-trainable, rides in state_dict like the reference's (model.py:257-261)
        empty = torch.sparse_coo_tensor(torch.zeros((2, 0), dtype=torch.int64), torch.zeros(0), (n_entities, n_entities))
        self.A_in = nn.Parameter(empty, requires_grad=False)
        if A_in is not None:
            self.A_in.data = A_in
        # opt-in: evaluate every layer only on the rows the batch needs (exact, see pruned.py); then
        # self.gat_embed holds the rows self.gat_rows instead of all N
        self.prune_to_batch = bool(getattr(args, "prune_to_batch", False))
        self.prune_max_fraction = 0.5     # frontier larger than this share of the entities: the dense path is cheaper
        # opt-in, inside the pruned path and in training mode only: a row aggregates at most neighbor_fanout of its stored
        # neighbours per step (pruned.sample_rows: the draw is a function of (neighbor_seed, neighbor_draw, row id)); every
        # sampled subgraph build uses neighbor_draw and then increments it -- set it back to repeat a step
        self.neighbor_fanout = getattr(args, "neighbor_fanout", None)
        self.neighbor_seed = 0
        self.neighbor_draw = 0
        self.neighbor_rescale = True      # kept values times d / fanout: the sampled neighbour sum estimates the full one
        self.last_step_sampled = False    # did the last subgraph build sample (False: exact, or the dense fall-back)
        self.gat_rows = None
        self.group_reuse = True           # TransR: project (h, t+) once per group of pre_training_neg_rate rows
        # linear_gat on the rows the loss reads instead of all N (calc_triplet_loss); LKG_ROWS_ONLY_PROJECTION=0: as the reference
        self.project_batch_rows_only = os.environ.get("LKG_ROWS_ONLY_PROJECTION", "1") not in ("", "0")
        self.group_reuse_min_rate = 2     # ... from this many negatives per positive on (the layout check is the step's one
                                          #     host sync; measured at K = 3, B = 2049: the reuse still wins 0.3-0.5 ms)
        self._att: Optional[AttentionCSR] = None
        self._att_key = None
        self._triple_graph = None
        self._triple_key = None
        self.last_scores = {}

    # ------------------------------------------------------------------ A_in <-> CSR
    def _attention(self) -> AttentionCSR:
        """CSR/CSC view of the current ``A_in`` (rebuilt only when ``A_in`` was replaced or moved)."""
        a = self.A_in.data
        if not a.is_coalesced():
            a = a.coalesce()
            self.A_in.data = a
        vals = a._values()
        key = (a._indices().data_ptr(), vals.data_ptr(), vals._version, str(vals.device), a._nnz())
        if self._att is not None and self._att_key == key:
            return self._att
        graph = KGStructure.from_coo(a, device=vals.device)
        self._att = AttentionCSR(graph, vals.contiguous())
        self._att_key = key
        return self._att

    # ------------------------------------------------------------------ a6/a7 encoder
    def _gate(self, ent, num, txt, out=None):
        a = self.args
        if a.use_num_lit and a.use_txt_lit:
            return self.emb_mul_lit(ent, num, txt, out)
        if a.use_num_lit:
            return self.emb_num_lit(ent, num, out)
        if a.use_txt_lit:
            return self.emb_txt_lit(ent, txt, out)
        return ent

    def _literals(self):
        a = self.args
        if a.use_num_lit:
            self.numerical_literals_embed = self.numerical_literals_embed.to(self.device)
        if a.use_txt_lit:
            self.text_literals_embed = self.text_literals_embed.to(self.device)
        for name, lit, width in (("numerical_literals", self.numerical_literals_embed if a.use_num_lit else None, self.n_num_lit),
                                 ("text_literals", self.text_literals_embed if a.use_txt_lit else None, self.n_txt_lit)):
            if lit is not None and tuple(lit.shape) != (self.n_entities, width):     # (the gate reads them row for row)
                raise ValueError(f"{name} has shape {tuple(lit.shape)}, expected ({self.n_entities}, {width})")
        return (self.numerical_literals_embed if a.use_num_lit else None,
                self.text_literals_embed if a.use_txt_lit else None)

    def gate_embeddings(self):
        return self._gate(self.entity_embed.weight, *self._literals())

    def gat_embeddings(self, defer_slot0: bool = False, project: bool = True):
        """The concatenated table (model.py:298-314).  defer_slot0 (no gate, no linear_gat): the copy of the raw entity
        table into column slot 0 is NOT made -- returns (table with slot 0 pending, raw table); a reader of <= 3B rows
        (the TransR loss) takes those columns from the raw table, anybody else goes through the ``gat_embed`` property,
        which completes the table first.  project = False: linear_gat + its activation (model.py:309-310) are NOT applied --
        the caller applies them to the rows it reads (calc_triplet_loss)."""
        att = self._attention()
        # every producer writes its column slice of the concatenated table directly (no torch.cat pass)
        cb = ops.CatBuffer(self.n_entities, self.conv_dim_list, self.entity_embed.weight.device)
        cur = self._gate(self.entity_embed.weight, *self._literals(), out=cb.slot(0))
        defer = (defer_slot0 and cur is self.entity_embed.weight and self.scale_gat_dim is None
                 and isinstance(att, AttentionCSR))
        kept = [cur]
        res_layers = [layer for layer in self.aggregator_layers if layer.use_residual]
        if len(res_layers) > 1:      # every layer projects the SAME h0 (model.py:93): one stacked product
            projections = ops.stacked_linear(cur, [layer.linear_h0.weight for layer in res_layers],
                                             [layer.linear_h0.bias for layer in res_layers])
            for layer, proj in zip(res_layers, projections):
                layer.h0_projection = proj        # (cleared layer by layer below; all of them if a layer raises)
        if (self.aggregator_layers and self.aggregator_layers[0].narrows() and cur is not self.entity_embed.weight
                and isinstance(att, AttentionCSR)):
            # the gate's output has two consumers here -- column slot 0 of the concatenated table and the first layer's Linear
            # (a narrowing layer projects before it aggregates) -- whose gradients are both zero outside a few rows in a
            # one-layer model: joined by ops.fanout their sum stays row-sparse and the gate's backward runs on those rows
            kept[0], cur = ops.fanout(cur)
        for idx, layer in enumerate(self.aggregator_layers):
            layer.norm_out = cb.slot(idx + 1)
            layer.want_output = idx + 1 < len(self.aggregator_layers)     # (the last layer's y is read by nobody)
            # layer 1 on the device structure: its SpMM also leaves the layer input in slot 0 (no copy pass) and its
            # backward sums the two gradients of that input in the same launch
            a_k = (_KeepingAttention(att, None if defer else cb.slot(0))
                   if (idx == 0 and isinstance(att, AttentionCSR)) else att)
            try:
                cur = layer(cur, a_k, kept, self.lamda, self.alpha, idx + 1)
            except BaseException:
                for other in self.aggregator_layers:
                    other.h0_projection = None
                raise
            finally:
                layer.norm_out = None
                layer.want_output = True
                layer.h0_projection = None
            if a_k is not att and a_k.kept is not None:
                kept[0] = a_k.kept
            kept.append(layer.last_normalized)   # F.normalize of the (dropped-out) layer output, fused
        if defer_slot0:
            cat = ops.assemble_cat(cb, kept, pending=(0,) if defer else ())
            if self.scale_gat_dim is not None:
                cat = ops.leaky_relu(ops.linear(cat, self.linear_gat.weight, self.linear_gat.bias))
            return cat, (self.entity_embed.weight if defer else None)
        cat = ops.assemble_cat(cb, kept)
        if self.scale_gat_dim is not None and project:
            return ops.leaky_relu(ops.linear(cat, self.linear_gat.weight, self.linear_gat.bias))
        return cat

    def _can_prune(self) -> bool:
        # gin sums earlier layers' outputs row by row (model.py:151-158): not wired for compact rows
        # (a frontier that outgrew prune_max_fraction -- deep models: the reference's eight layers reach everything from 2 049
        # triples -- is not tried again for PRUNE_RETRY_EVERY calls of forward(): an attempt costs two levels of index bookkeeping)
        return self.prune_to_batch and self.aggregation_type != "gin" and self.__dict__.get("_prune_skip", 0) == 0

    PRUNE_RETRY_EVERY = 64

    def _neighbor_sampling(self) -> Optional[int]:
        """The fanout the next subgraph build samples with, or None: sampling is active in training mode with
        ``neighbor_fanout`` set (eval mode runs the exact path, as dropout is off there).  A fanout that is no int >= 1, or set
        where the pruned path does not run (``prune_to_batch`` off, 'gin'), is a ValueError -- raised here, ahead of any
        device work of the call."""
        if self.neighbor_fanout is None or not self.training:
            return None
        fanout = pruned.checked_fanout(self.neighbor_fanout)
        if not self.prune_to_batch:
            raise ValueError("neighbor_fanout needs prune_to_batch = True: neighbours are sampled inside the batch-pruned step")
        if self.aggregation_type == "gin":
            raise ValueError("neighbor_fanout does not apply to aggregation_type 'gin': the batch-pruned step does not support it")
        return fanout

    def gat_embeddings_for(self, ids: torch.Tensor):
        """Rows `unique(ids)` of gat_embeddings(), computed on the batch's L-hop frontier only (pruned.py).
        Returns (compact table, BatchSubgraph), or (None, None) when the frontier covers more than
        ``prune_max_fraction`` of the entities (large batches x many layers: the dense path is cheaper then).
        With neighbour sampling active the frontier is that of the sampled matrix (draw ``neighbor_draw``, which is then
        incremented) and ``last_step_sampled`` says whether the returned subgraph is a sampled one."""
        fanout = self._neighbor_sampling()
        att = self._attention()
        sub = pruned.build_batch_subgraph(att.graph, att.val, ids, self.n_layers,
                                          max_rows=int(self.prune_max_fraction * self.n_entities), fanout=fanout,
                                          seed=self.neighbor_seed, draw=self.neighbor_draw, rescale=self.neighbor_rescale)
        if fanout is not None:
            self.neighbor_draw += 1
        self.last_step_sampled = fanout is not None and sub is not None
        if sub is None:
            return None, None
        top = self.n_layers
        num, txt = self._literals()
        r0 = sub.rows[0]
        g0 = self._gate(pruned.gather_rows(self.entity_embed.weight, r0),
                        ops.gather_rows(num, r0) if num is not None else None,
                        ops.gather_rows(txt, r0) if txt is not None else None)
        kept = [pruned.gather_rows(g0, sub.rows_in(top, 0))]
        cur = g0
        for k, layer in enumerate(self.aggregator_layers, start=1):
            sl = sub.layers[k]
            ego = pruned.gather_rows(cur, sl.self_pos)
            h0 = pruned.gather_rows(g0, sub.rows_in(k, 0)) if layer.use_residual else g0
            cur = layer(ego, pruned.CompactAttention(sl, cur), [h0], self.lamda, self.alpha, k)
            norm = layer.last_normalized
            kept.append(norm if k == top else pruned.gather_rows(norm, sub.rows_in(top, k)))
        cat = torch.cat(kept, dim=1)
        if self.scale_gat_dim is not None:
            cat = ops.leaky_relu(ops.linear(cat, self.linear_gat.weight, self.linear_gat.bias))
        return cat, sub

    def _eval_key(self):
        """What the encoder's output depends on: every parameter (address and in-place version; A_in by its value array) and
        the literal tables."""
        key = []
        for p in self.parameters():
            t_ = p.data._values() if p.is_sparse else p
            key.append((t_.data_ptr(), t_._version, tuple(t_.shape)))
        for lit in (self.numerical_literals_embed, self.text_literals_embed):
            if isinstance(lit, torch.Tensor):
                key.append((lit.data_ptr(), lit._version, str(lit.device)))
        return tuple(key)

    def _table_for_inference(self):
        """gat_embeddings() for the inference heads.  The reference's evaluate() calls mode='predict' once per batch of heads
        (utils/model_utils.py:55-60) and every call recomputes the whole encoder (model.py:475); in eval mode under no_grad
        the table is a pure function of the parameters, A_in and the literals, so it is kept until one of them changes
        (optimizer step, load_state_dict, update_att, an in-place edit: all of them bump a version or move a tensor)."""
        if self.training or torch.is_grad_enabled():
            self._eval_cache = None
            return self.gat_embeddings()
        key = self._eval_key()
        cached = self.__dict__.get("_eval_cache")
        if cached is not None and cached[0] == key:
            return cached[1]
        table = self.gat_embeddings()
        self._eval_cache = (self._eval_key(), table)      # (keyed AFTER the pass: it may have moved the literals to the device)
        return table

    def train(self, mode: bool = True):
        """nn.Module.train; entering training mode drops the table the inference heads keep (N x C floats)."""
        if mode:
            self._eval_cache = None
        return super().train(mode)

    def _embeddings_and_ids(self, *id_lists):
        """(table, relabelled ids): the full table with the ids as given, or the pruned table with positions."""
        self._neighbor_sampling()                 # (a fanout that cannot apply raises before anything is launched)
        if not self._can_prune():
            self.gat_rows = None
            self.last_step_sampled = False
            return self._table_for_inference(), id_lists
        table, sub = self.gat_embeddings_for(torch.cat([i.reshape(-1) for i in id_lists]))
        if table is None:
            self.gat_rows = None
            self._prune_skip = self.PRUNE_RETRY_EVERY
            return self.gat_embeddings(), id_lists
        self.gat_rows = sub.rows[-1]
        return table, tuple(sub.positions(i) for i in id_lists)

    # ------------------------------------------------------------------ a8/a9 loss
    def calc_triplet_loss(self, h, r, pos_t, neg_t):
        # generate_kg_batch repeats every sampled (h, r, t+) pre_training_neg_rate times (dataloader.py:318-330): such
        # a batch projects h and t+ once per group.  Checked on the ids (any other batch takes the general path).
        self._neighbor_sampling()
        h, pos_t, neg_t = ops.checked_ids(self.id_space, h, pos_t, neg_t)     # (out-of-range ids never reach a kernel)
        (r,) = ops.checked_ids(self.n_relations, r, what="relation")
        check, k = None, int(self.pre_training_neg_rate)
        if self.scoring == "transr" and self.group_reuse and k >= self.group_reuse_min_rate:
            check = ops.GroupedCheck(h, r, pos_t, k)      # queued now, answered just before the loss (no idle device)
        keep = self.last_scores if not self.training else None
        if self.training or torch.is_grad_enabled():
            self._eval_cache = None           # a training step is under way: the inference heads' kept table goes
        if self.scoring == "transr" and self._rows_only_projection_applies():
            # The loss reads <= 3B rows of linear_gat's output and a row of it depends on the same row of the concatenated table
            # only: the projection (model.py:309-310) runs on those rows -- 1 M x 556 -> 300 was 2.5 of the reference-default
            # step's 10.6 forward ms -- and the N-row table the reference leaves in self.gat_embed (model.py:380) is projected
            # only if somebody reads that attribute.  Same loss, same gradients (the projection's backward already ran on
            # these rows only).
            cat = self._unprojected_table()         # (the encoder is queued before the layout check is waited for)
            group = k if (check is not None and check.result()) else 1
            rows, (at_h, at_p, at_n) = self._projected_rows(cat, h[::group], pos_t[::group], neg_t)
            return ops.transr_loss(rows, self.relation_embed.weight, self.gat_trans_M, at_h.repeat_interleave(group), r,
                                   at_p.repeat_interleave(group), at_n, self.kg_l2loss_lambda, keep, group, False)
        if self._rows_only_projection_applies():          # TransE on the same footing
            rows, (h, pos_t, neg_t) = self._projected_rows(self._unprojected_table(), h, pos_t, neg_t)
            return ops.transe_loss(rows, self.relation_embed.weight, h, r, pos_t, neg_t, self.kg_l2loss_lambda, keep, False)
        if self.scoring == "transr" and not self._can_prune():
            # the loss reads <= 3B rows: the N-row copy of the raw entity table into slot 0 of the concatenated table is
            # deferred (made only if somebody asks for self.gat_embed), its columns are read from the raw table
            self.gat_rows = None
            self.last_step_sampled = False
            table, raw = self.gat_embeddings(defer_slot0=True)
            self._gat_state = (table, raw)        # (a tuple: nn.Module would register a bare Parameter attribute)
            group = k if (check is not None and check.result()) else 1
            self._raise_bad_ids()
            return ops.transr_loss(table, self.relation_embed.weight, self.gat_trans_M, h, r, pos_t, neg_t,
                                   self.kg_l2loss_lambda, keep, group, self._table_grad_stays_inside(), slot0=raw)
        self.gat_embed, (h, pos_t, neg_t) = self._embeddings_and_ids(h, pos_t, neg_t)
        self._raise_bad_ids()
        sparse = self._table_grad_stays_inside()
        if self.scoring == "transr":
            group = k if (check is not None and check.result()) else 1
            return ops.transr_loss(self.gat_embed, self.relation_embed.weight, self.gat_trans_M, h, r, pos_t, neg_t,
                                   self.kg_l2loss_lambda, keep, group, sparse)
        return ops.transe_loss(self.gat_embed, self.relation_embed.weight, h, r, pos_t, neg_t,
                               self.kg_l2loss_lambda, keep, sparse)

    def calc_one_vs_all_loss(self, h, r, t, side: str = "tail", scale: float = 1.0, reduction: str = "mean",
                             scoring: Optional[str] = None, splits: Optional[int] = None, known=None, candidates=None,
                             products: str = "engine"):
        """1-vs-all training loss of the triples (h, r, t) (literalkg_amd/one_vs_all.py): cross-entropy of the true tail
        (side 'tail'), head ('head') or the mean of both ('both') against the softmax over EVERY entity under scoring
        'transr' / 'transe' / 'dot' (default: self.scoring).  Always on the full table of the step (prune_to_batch does
        not apply); no L2 term (weight decay is the optimizer's).  known (a KnownTriples): the other known answers of a
        query leave its softmax (the filtered loss); candidates (unique entity ids, one side only): the softmax runs over
        those entities alone.  products "ordered": the backward's long reduction runs on the ordered split-K GEMM
        (literalkg_amd/gemm_ordered.py).  Also ``model(h, r, t, device=, mode='one_vs_all')``, the plain call."""
        from .one_vs_all import one_vs_all_loss
        return one_vs_all_loss(self, h, r, t, side=side, scale=scale, reduction=reduction, scoring=scoring, splits=splits,
                               known=known, candidates=candidates, products=products)

    def calc_kvs_all_loss(self, ent, r, known, side: str = "tail", margin: float = 0.0, scale: float = 1.0,
                          label_smoothing: float = 0.0, reduction: str = "mean", scoring: Optional[str] = None,
                          splits: Optional[int] = None, candidates=None, products: str = "engine"):
        """KvsAll training loss of the queries (ent, r) (literalkg_amd/kvs_all.py): one row per query scored against EVERY
        entity, binary cross-entropy with logits against the multi-hot vector of the query's answers in known (a
        KnownTriples), summed over the candidates; side 'tail' ((ent, r, ?)) or 'head' ((?, r, ent)), logits
        scale (margin - ||q - p||^2) ('dot': scale (margin + q.p)), optional label smoothing.  Always on the full table of
        the step (prune_to_batch does not apply).  products as in calc_one_vs_all_loss.  There is no mode= string for it."""
        from .kvs_all import kvs_all_loss
        return kvs_all_loss(self, ent, r, known, side=side, margin=margin, scale=scale, label_smoothing=label_smoothing,
                            reduction=reduction, scoring=scoring, splits=splits, candidates=candidates, products=products)

    def calc_self_adversarial_loss(self, h, r, t, neg, side: str = "tail", margin: float = 0.0, scale: float = 1.0,
                                   temperature: float = 1.0, reduction: str = "mean", scoring: Optional[str] = None):
        """Self-adversarial negative-sampling loss of the triples (h, r, t) against their K sampled negatives neg[G, K]
        (literalkg_amd/self_adversarial.py): softplus(-z+) + sum_j w_j softplus(z_j) with the logits
        scale (margin - ||q - x||^2) ('dot': scale (margin + q.x)) and the constant weights softmax_j(temperature z_j);
        side 'tail' (the negatives replace the tail) or 'head'.  Reads only the (2 + K) G rows it scores, so
        prune_to_batch applies; no L2 term.  There is no mode= string for it."""
        from .self_adversarial import self_adversarial_loss
        self._neighbor_sampling()
        return self_adversarial_loss(self, h, r, t, neg, side=side, margin=margin, scale=scale, temperature=temperature,
                                     reduction=reduction, scoring=scoring)

    def calc_sampled_negative_loss(self, h, r, t, batch, weights=None, margin: float = 0.0, scale: float = 1.0,
                                   temperature: float = 1.0, reduction: str = "mean", scoring: Optional[str] = None):
        """The self-adversarial loss of the triples (h, r, t) against a NegativeBatch of NegativeSampler.sample, whose groups
        may be corrupted on either side (literalkg_amd/negatives.py): each side's groups scored as
        calc_self_adversarial_loss scores them alone (one table for both), the per-group losses back in group order,
        weighted by ``weights`` (e.g. subsampling_weights): 'mean' is sum(w L) / sum(w)."""
        from .negatives import sampled_negative_loss
        self._neighbor_sampling()
        return sampled_negative_loss(self, h, r, t, batch, weights=weights, margin=margin, scale=scale,
                                     temperature=temperature, reduction=reduction, scoring=scoring)

    def calc_relation_loss(self, h, r, t, known=None, scoring: Optional[str] = None, scale: float = 1.0,
                           reduction: str = "mean", chunk_bytes: int = 256 << 20, products: str = "engine"):
        """Relation-slot loss of the triples (h, r, t) (literalkg_amd/relation_loss.py): the cross-entropy of r against the
        softmax over every relation of (h, ?, t), logits -scale ||(T[h] - T[t]) W_j + e_j||^2 ('transe': no W_j), with
        ``known`` (a KnownTriples) the pair's other known relations left out -- the objective of
        evaluate_relation_prediction's filtered metric.  Reads two table rows per pair, so prune_to_batch applies; no L2
        term.  products as in calc_one_vs_all_loss.  There is no mode= string for it."""
        from .relation_loss import relation_loss
        self._neighbor_sampling()
        return relation_loss(self, h, r, t, known=known, scoring=scoring, scale=scale, reduction=reduction,
                             chunk_bytes=chunk_bytes, products=products)

    def _rows_only_projection_applies(self) -> bool:
        """A loss that reads a few rows of linear_gat's output and has to run the encoder anyway (a training step, or any call
        with autograd on: the inference heads' kept table is for eval mode under no_grad)."""
        return (self.project_batch_rows_only and self.scale_gat_dim is not None and not self._can_prune()
                and (self.training or torch.is_grad_enabled() or self.scoring == "transr"))

    def _unprojected_table(self):
        """The concatenated table without linear_gat; it stays behind self.gat_embed, projected on first access."""
        self.gat_rows = None
        self.last_step_sampled = False
        cat = self.gat_embeddings(project=False)
        self._gat_state = (cat, None, True)
        self._raise_bad_ids()
        return cat

    def _projected_rows(self, cat, *id_lists):
        """(linear_gat + activation of the rows of cat that the lists name, the lists as positions in them).  The lists hold
        n_g, n_g, ..., n_g * K ids (one head / positive per group, its K negatives): the rows are laid out GROUP BY GROUP --
        head, positive, negatives of group 0, then group 1 ... -- so that every sum over these rows downstream (linear_gat's
        weight and bias gradients) meets a group's nearly cancelling terms next to each other, as autograd's per-sample sums do
        in the reference (model.py:380-397); block after block -- all heads, then all positives -- the same sums were 60 x
        further from float64 than the fp32 reference on ill-conditioned configurations.  What this layout fixed is
        gat_trans_M's gradient at fuzz seed 44053.  Seed 81374 (linear_gat's gradients off next to a LeakyReLU kink) is not
        an audited op's error: every audited GEMM / weight-gradient / column-sum call of its step is within its per-op bound
        against float64 (tests/test_op_audit_gpu.py); its end-to-end case is a strict xfail."""
        lists = [i.reshape(-1) for i in id_lists]
        n_g = min(i.numel() for i in lists)
        per = [i.numel() // max(n_g, 1) for i in lists]                  # ids of a group in each list: 1, 1, K
        total = sum(per)
        ids = torch.cat([i.view(n_g, m) for i, m in zip(lists, per)], dim=1).reshape(-1) if n_g else torch.cat(lists)
        half = ids.numel() // 2
        a, b = ops.gather_rows_pair(cat, ids[:half], ids[half:], self._table_grad_stays_inside())
        rows = ops.leaky_relu(ops.linear(torch.cat([a, b]), self.linear_gat.weight, self.linear_gat.bias))
        base = torch.arange(n_g, device=ids.device).view(n_g, 1) * total
        positions, at = [], 0
        for m in per:
            positions.append((base + at + torch.arange(m, device=ids.device)).reshape(-1))
            at += m
        return rows, tuple(positions)

    @staticmethod
    def _raise_bad_ids():
        """The ids a caller handed in were sanitised on the device at the start of the call (ops.checked_ids).  By now the
        encoder's launches are queued BEHIND that kernel, so waiting for its event costs the device nothing -- and an id
        outside its table raises IndexError inside the call, before a loss or a score exists and before anything is updated
        (the reference's lookups raise at model.py:366-384 / 475-476)."""
        ops.check_deferred_errors()

    @property
    def gat_embed(self):
        """The table of the last encoder pass (the reference keeps it as an attribute, model.py:366).  A slot-0 copy that
        the loss deferred is made here, on first access."""
        table, raw, *pending = self.__dict__.get("_gat_state", (None, None))
        if table is not None and pending and pending[0]:       # linear_gat was applied to the batch's rows only: all rows now
            with torch.no_grad():
                table = ops.leaky_relu(ops.linear(table.detach(), self.linear_gat.weight, self.linear_gat.bias))
            self._gat_state = (table, None)
        if table is not None and raw is not None:
            ops.fill_slot(table, 0, raw)
            self._gat_state = (table, None)
        return table

    @gat_embed.setter
    def gat_embed(self, table):
        self._gat_state = (table, None)

    def _table_grad_stays_inside(self) -> bool:
        """Is ``self.gat_embed`` the full N-row table of gat_embeddings()?  Its gradient (<= 3B non-zero rows) is then
        consumed during the backward pass by this package's Functions only -- column slices of the concatenated table
        (>= 2 slots, so no slice can become a parameter's .grad as it is) or linear_gat's backward -- and the loss may
        hand back the shared all-zero table of ops._RowScratch instead of filling N x C zeros per step."""
        return self.gat_rows is None and len(self.conv_dim_list) >= 2     # (gat_rows: set by the pruned path)

    # ------------------------------------------------------------------ a4/a5 attention refresh
    def _structure_for(self, h_list, t_list, r_list, relations) -> KGStructure:
        # content, not identity: a driver re-uploads the lists every epoch (main_pretraining.py:135-137) and the
        # allocator may hand the same address to a different list -- so the cached structure is reused only when the
        # three lists EQUAL the device copies kept from the build (an exact compare, ~0.1 ms at 10 M triples)
        rel_key = tuple(int(x) for x in relations) if relations is not None else None
        dev = self.A_in.device
        c = self._triple_key
        if (self._triple_graph is not None and c is not None and c[0] == rel_key and c[1] == str(dev)
                and all(a.shape == b.shape and a.dtype == b.dtype and a.device == b.device and torch.equal(a, b)
                        for a, b in zip((h_list, t_list, r_list), c[2]))):
            return self._triple_graph
        h, t, r = h_list, t_list, r_list
        if relations is not None:      # the reference only visits `relations` (model.py:451): other triples are dropped
            every = sorted(set(rel_key)) == list(range(self.n_relations))
            # (the usual call visits EVERY relation: then the filter keeps exactly the triples with a valid relation id, which
            # the id sanitiser counts -- no torch.isin over the edge list, whose first use alone costs the first refresh 25 ms)
            if not (every and r.is_cuda and ops.count_ids_outside(self.n_relations, r) == 0):
                rel_ids = torch.as_tensor(list(relations), dtype=r.dtype, device=r.device)
                keep = torch.isin(r, rel_ids)
                if not bool(keep.all()):
                    h, t, r = h[keep], t[keep], r[keep]
        g = KGStructure.from_triples(self.n_entities, h, t, r, device=dev)
        self._triple_graph = g
        self._triple_key = (rel_key, str(dev), tuple(x.detach().clone() for x in (h_list, t_list, r_list)))
        return g

    def update_attention(self, h_list, t_list, r_list, relations):
        if relations is not None and any(not 0 <= int(x) < self.n_relations for x in relations):
            raise IndexError(f"update_att: relation id outside [0, {self.n_relations}) in `relations` "
                             "(relation_embed.weight[r_idx], model.py:441)")
        if relations is None and r_list.is_cuda:      # (no list to filter by: every triple's relation id is used as it is)
            (r_list,) = ops.checked_ids(self.n_relations, r_list, what="relation")
        g = self._structure_for(h_list, t_list, r_list, relations)
        val, _ = ops.edge_softmax(g, self.entity_embed.weight.detach(), self.relation_embed.weight.detach())
        new = torch.sparse_coo_tensor(g.coo_indices(), val, (self.n_entities, self.n_entities), is_coalesced=True)
        self.A_in.data = new
        vals = new._values()
        self._att = AttentionCSR(g, vals)
        self._att_key = (new._indices().data_ptr(), vals.data_ptr(), vals._version, str(vals.device), new._nnz())

    # ------------------------------------------------------------------ f1 heads
    def calc_score(self, head_ids, tail_ids):
        self._neighbor_sampling()
        head_ids, tail_ids = ops.checked_ids(self.id_space, head_ids, tail_ids)
        emb, (head_ids, tail_ids) = self._embeddings_and_ids(head_ids, tail_ids)
        self._raise_bad_ids()
        return ops.gemm(ops.gather_rows(emb.detach(), head_ids), ops.gather_rows(emb.detach(), tail_ids),
                        trans_b=True)

    def predict_links(self, head_ids, tail_ids):
        s = self.calc_score(head_ids, tail_ids)
        lo, hi = s.min(), s.max()
        return ((s - lo) / (hi - lo) > self.milestone_score).int()

    def rank_triples(self, h, r, t, side: str = "tail", known=None, scoring: Optional[str] = None,
                     batch_size: Optional[int] = None):
        """Filtered link-prediction ranks of the triples (h, r, t) on the inference table (literalkg_amd/ranking.py):
        side 'tail' / 'head' / 'both', scoring 'transr' / 'transe' / 'dot' (default: self.scoring), known a
        ranking.KnownTriples filter.  Returns a ranking.RankResult (better, equal, rank)."""
        from .ranking import rank_triples
        return rank_triples(self, h, r, t, side=side, known=known, scoring=scoring, batch_size=batch_size)

    def predict_topk(self, ids, r=None, side: str = "tail", k: int = 10, known=None, scoring: Optional[str] = None,
                     candidates=None, batch_size: Optional[int] = None, splits: int = 0):
        """The k best tails of (ids, r, ?) (side 'tail') or heads of (?, r, ids) (side 'head') on the inference table,
        known triples dropped (literalkg_amd/topk.py): scoring 'transr' / 'transe' / 'dot' (default: self.scoring) or 'mlp'
        (the trained pair head, literalkg_amd/pairmlp.py), known a ranking.KnownTriples filter, candidates an optional subset of entity ids.  Returns a topk.TopKResult
        (ids, scores, side)."""
        from .topk import predict_topk
        return predict_topk(self, ids, r, side=side, k=k, known=known, scoring=scoring, candidates=candidates,
                            batch_size=batch_size, splits=splits)

    def mlp_scores(self, head_ids, tail_ids, logits: bool = False):
        """The len(head_ids) x len(tail_ids) probabilities (or logits) of the MLP pair head on the inference table: what
        mode='mlp' gives in eval mode for every pair, without forming the pairs (literalkg_amd/pairmlp.py)."""
        from .pairmlp import mlp_scores
        return mlp_scores(self, head_ids, tail_ids, logits=logits)

    def rank_pairs(self, h, t, r=None, side: str = "tail", known=None, candidates=None,
                   batch_size: Optional[int] = None):
        """Filtered ranks of the pairs (h, t) under the MLP pair head on the inference table (literalkg_amd/pairmlp.py,
        rank_pairs_mlp): side 'tail' / 'head' / 'both', r the pairs' relations for the filter (None: any relation), known
        a ranking.KnownTriples filter, candidates an optional subset of entity ids.  Returns a ranking.RankResult."""
        from .pairmlp import rank_pairs_mlp
        return rank_pairs_mlp(self, h, t, r=r, side=side, known=known, candidates=candidates, batch_size=batch_size)

    def score_pairs(self, h, t, logits: bool = False, batch_size: Optional[int] = None):
        """float32[P]: the MLP pair head's probability (or logit) of every pair (h_i, t_i) on the inference table, each
        logit with the bits mlp_scores gives that pair (literalkg_amd/pairmlp.py, score_pairs_mlp)."""
        from .pairmlp import score_pairs_mlp
        return score_pairs_mlp(self, h, t, logits=logits, batch_size=batch_size)

    def score_triples(self, h, r, t, scoring: Optional[str] = None, side: str = "tail",
                      batch_size: Optional[int] = None, kernel_scores: bool = False):
        """float32[P]: the score of every triple (h_i, r_i, t_i) on the inference table, with the bits predict_topk
        reports for that (query, candidate) (literalkg_amd/triples.py, score_triples)."""
        from .triples import score_triples
        return score_triples(self, h, r, t, scoring=scoring, side=side, batch_size=batch_size,
                             kernel_scores=kernel_scores)

    def fit_triple_thresholds(self, h, r, t, labels, scoring: Optional[str] = None, per_relation: bool = True,
                              batch_size: Optional[int] = None):
        """The exact per-relation classification thresholds of the labelled validation triples
        (literalkg_amd/triples.py, fit_triple_thresholds).  Returns a triples.TripleThresholds."""
        from .triples import fit_triple_thresholds
        return fit_triple_thresholds(self, h, r, t, labels, scoring=scoring, per_relation=per_relation,
                                     batch_size=batch_size)

    def evaluate_triple_classification(self, h, r, t, labels, thresholds, scoring: Optional[str] = None,
                                       batch_size: Optional[int] = None):
        """Triple-classification metrics of the labelled triples under per-relation thresholds
        (literalkg_amd/triples.py, evaluate_triple_classification)."""
        from .triples import evaluate_triple_classification
        return evaluate_triple_classification(self, h, r, t, labels, thresholds, scoring=scoring,
                                              batch_size=batch_size)

    def score_lists(self, ids, r, lists, side: str = "tail", scoring: Optional[str] = None, kernel_scores: bool = False,
                    batch_size: Optional[int] = None):
        """float32[B, M]: the score of every slot of every query's own candidate list int64[B, M] (a negative entry: an
        empty slot, NaN), with the bits score_triples returns for it (literalkg_amd/lists.py, score_lists)."""
        from .lists import score_lists
        return score_lists(self, ids, r, lists, side=side, scoring=scoring, kernel_scores=kernel_scores,
                           batch_size=batch_size)

    def rank_in_lists(self, h, r, t, lists, side: str = "tail", known=None, scoring: Optional[str] = None,
                      batch_size: Optional[int] = None):
        """The filtered rank of every triple's truth among the slots of its own candidate list
        (literalkg_amd/lists.py, rank_in_lists).  Returns a lists.ListRanks (better, equal, kept, rank)."""
        from .lists import rank_in_lists
        return rank_in_lists(self, h, r, t, lists, side=side, known=known, scoring=scoring, batch_size=batch_size)

    def evaluate_list_ranking(self, h, r, t, tail_lists=None, head_lists=None, known=None, ks=(1, 3, 10),
                              scoring: Optional[str] = None, batch_size: Optional[int] = None):
        """MR, MRR and Hits@k of the triples against given negatives per side
        (literalkg_amd/lists.py, evaluate_list_ranking)."""
        from .lists import evaluate_list_ranking
        return evaluate_list_ranking(self, h, r, t, tail_lists=tail_lists, head_lists=head_lists, known=known, ks=ks,
                                     scoring=scoring, batch_size=batch_size)

    def score_relations(self, h, t, scoring: Optional[str] = None, side: str = "tail", batch_size: Optional[int] = None,
                        relation_chunk: Optional[int] = None):
        """float32[P, n_relations]: the score of (h_i, j, t_i) under every relation j, with the bits score_triples
        returns for it (literalkg_amd/relations.py, score_relations)."""
        from .relations import score_relations
        return score_relations(self, h, t, scoring=scoring, side=side, batch_size=batch_size,
                               relation_chunk=relation_chunk)

    def rank_relations(self, h, r, t, known=None, scoring: Optional[str] = None, side: str = "tail",
                       batch_size: Optional[int] = None, relation_chunk: Optional[int] = None):
        """The filtered rank of the true relation r_i among all relations of (h_i, ?, t_i)
        (literalkg_amd/relations.py, rank_relations).  Returns a RankResult."""
        from .relations import rank_relations
        return rank_relations(self, h, r, t, known=known, scoring=scoring, side=side, batch_size=batch_size,
                              relation_chunk=relation_chunk)

    def predict_relations(self, h, t, k: int = 1, known=None, scoring: Optional[str] = None, side: str = "tail",
                          batch_size: Optional[int] = None, relation_chunk: Optional[int] = None):
        """The k most likely relations of every pair (h_i, t_i) that are not already known
        (literalkg_amd/relations.py, predict_relations).  Returns a relations.RelationTopK."""
        from .relations import predict_relations
        return predict_relations(self, h, t, k=k, known=known, scoring=scoring, side=side, batch_size=batch_size,
                                 relation_chunk=relation_chunk)

    def predict_accepted(self, ids, r, thresholds, side: str = "tail", known=None, scoring: Optional[str] = None,
                         candidates=None, batch_size: Optional[int] = None, splits: int = 0, max_total: int = 1 << 26):
        """Every tail of (ids, r, ?) (side 'tail') or head of (?, r, ids) (side 'head') whose score passes the thresholds
        and that is not already known, best first (literalkg_amd/accepted.py, predict_accepted).  Returns an
        accepted.AcceptedResult (rowptr, ids, scores, kernel_scores, counts)."""
        from .accepted import predict_accepted
        return predict_accepted(self, ids, r, thresholds, side=side, known=known, scoring=scoring, candidates=candidates,
                                batch_size=batch_size, splits=splits, max_total=max_total)

    def count_accepted(self, ids, r, thresholds, side: str = "tail", known=None, scoring: Optional[str] = None,
                       candidates=None, batch_size: Optional[int] = None, splits: int = 0):
        """int64[B]: how many candidates predict_accepted would list for every query (literalkg_amd/accepted.py,
        count_accepted); nothing of the size of the lists is allocated."""
        from .accepted import count_accepted
        return count_accepted(self, ids, r, thresholds, side=side, known=known, scoring=scoring, candidates=candidates,
                              batch_size=batch_size, splits=splits)

    def predict_accepted_pairs(self, ids, r=None, threshold: float = 0.5, logit_threshold=None, side: str = "tail",
                               known=None, candidates=None, batch_size: Optional[int] = None, splits: int = 0,
                               max_total: int = 1 << 26, buffer: int = 1 << 22):
        """Every pair (ids, ?) (side 'tail') or (?, ids) (side 'head') that the MLP pair head accepts -- logit > threshold
        -- and that is not already known, best first (literalkg_amd/pairmlp.py, predict_accepted_mlp).  Returns an
        accepted.AcceptedResult whose scores are probabilities and whose kernel_scores are logits."""
        from .pairmlp import predict_accepted_mlp
        return predict_accepted_mlp(self, ids, r=r, threshold=threshold, logit_threshold=logit_threshold, side=side,
                                    known=known, candidates=candidates, batch_size=batch_size, splits=splits,
                                    max_total=max_total, buffer=buffer)

    def count_accepted_pairs(self, ids, r=None, threshold: float = 0.5, logit_threshold=None, side: str = "tail",
                             known=None, candidates=None, batch_size: Optional[int] = None, splits: int = 0):
        """int64[B]: how many pairs predict_accepted_pairs would list for every query (literalkg_amd/pairmlp.py,
        count_accepted_mlp); nothing of the size of the lists is allocated."""
        from .pairmlp import count_accepted_mlp
        return count_accepted_mlp(self, ids, r=r, threshold=threshold, logit_threshold=logit_threshold, side=side,
                                  known=known, candidates=candidates, batch_size=batch_size, splits=splits)

    def rank_answers(self, h, r, t, side: str = "tail", known=None, scoring: Optional[str] = None, candidates=None,
                     batch_size: Optional[int] = None, ks=None):
        """The place of every answer of every distinct query (h, r, ?) -- or (?, r, t) -- in the query's ranked list, each
        query scored once however many answers it has (literalkg_amd/retrieval.py, rank_answers).  Returns a
        retrieval.AnswerRanks."""
        from .retrieval import rank_answers
        return rank_answers(self, h, r, t, side=side, known=known, scoring=scoring, candidates=candidates,
                            batch_size=batch_size, ks=ks)

    def evaluate_retrieval(self, h, r, t, known=None, ks=(1, 3, 10), side: str = "tail", scoring: Optional[str] = None,
                           candidates=None, batch_size: Optional[int] = None):
        """precision@k / recall@k / hit@k / NDCG@k, MAP and MRR over the distinct queries of the triples, every answer
        placed exactly at any depth (literalkg_amd/retrieval.py, evaluate_retrieval)."""
        from .retrieval import evaluate_retrieval
        return evaluate_retrieval(self, h, r, t, known=known, ks=ks, side=side, scoring=scoring, candidates=candidates,
                                  batch_size=batch_size)

    def evaluate_relation_prediction(self, h, r, t, known=None, ks=(1, 3, 10), scoring: Optional[str] = None,
                                     batch_size: Optional[int] = None):
        """MR / MRR / Hits@k of the true relations among all relations, filtered, overall and per relation
        (literalkg_amd/relations.py, evaluate_relation_prediction)."""
        from .relations import evaluate_relation_prediction
        return evaluate_relation_prediction(self, h, r, t, known=known, ks=ks, scoring=scoring, batch_size=batch_size)

    def initialize_MLP(self):
        """The pair-classification head of model.py:499-504 (same module names, so checkpoints interchange)."""
        self.fc1 = nn.Linear(self.scale_gat_dim * 2, 128)
        self.norm1 = nn.BatchNorm1d(128)
        self.fc2 = nn.Linear(128, 64)
        self.norm2 = nn.BatchNorm1d(64)
        self.fc3 = nn.Linear(64, 1)
        dev = self.entity_embed.weight.device
        for mod in (self.fc1, self.norm1, self.fc2, self.norm2, self.fc3):
            mod.to(dev)

    def train_MLP(self, head_ids, tail_ids):
        """mode='mlp' (model.py:506-519): sigmoid(fc3(bn2(relu(fc2(bn1(relu(fc1([e_h | e_t])))))))) ."""
        if not hasattr(self, "fc1"):
            raise AttributeError("call initialize_MLP() first (model.py:499)")
        self._neighbor_sampling()
        head_ids, tail_ids = ops.checked_ids(self.id_space, head_ids, tail_ids)
        self.gat_embed, (head_ids, tail_ids) = self._embeddings_and_ids(head_ids, tail_ids)
        self._raise_bad_ids()
        eh, et = ops.gather_rows_pair(self.gat_embed, head_ids, tail_ids, self._table_grad_stays_inside())
        c = eh.shape[1]
        w1 = self.fc1.weight
        x = ops.multi_linear((eh, et), (w1[:, :c], w1[:, c:]), self.fc1.bias)       # fc1 over [e_h | e_t], no cat
        x = ops.relu_batchnorm(x, self.norm1)
        x = ops.relu_batchnorm(ops.linear(x, self.fc2.weight, self.fc2.bias), self.norm2)
        return torch.sigmoid(ops.linear(x, self.fc3.weight, self.fc3.bias))

    def get_final_embeddings(self, entity_ids):
        return self.gat_embeddings()[entity_ids]

    def forward(self, *input, device, mode):
        self.device = device
        if self.__dict__.get("_prune_skip", 0) > 0 and mode != "update_att":
            self._prune_skip -= 1
        if mode in ("pre_training", "fine_tuning", "mlp", "one_vs_all") and (self.training or torch.is_grad_enabled()):
            self._eval_cache = None           # a training step: whatever table the inference heads kept is about to be stale
        if mode == "pre_training":
            return self.calc_triplet_loss(*input)
        if mode == "one_vs_all":
            return self.calc_one_vs_all_loss(*input)
        if mode == "update_att":
            return self.update_attention(*input)
        if mode == "predict":
            return self.predict_links(*input)
        if mode == "fine_tuning":
            return self.calculate_prediction_loss(*input)
        if mode == "mlp":
            return self.train_MLP(*input)
        return None   # unknown modes fall through silently, as in the reference (model.py:521-532)

    def calculate_prediction_loss(self, head_ids, tail_pos_ids, tail_neg_ids):
        """f1: dot-product BPR fine-tuning loss (model.py:316-348)."""
        self._neighbor_sampling()
        head_ids, tail_pos_ids, tail_neg_ids = ops.checked_ids(self.id_space, head_ids, tail_pos_ids, tail_neg_ids)
        if self._rows_only_projection_applies() and (self.training or torch.is_grad_enabled()):
            rows, (head_ids, tail_pos_ids, tail_neg_ids) = self._projected_rows(self._unprojected_table(), head_ids, tail_pos_ids,
                                                                                  tail_neg_ids)
            return ops.dot_loss(rows, head_ids, tail_pos_ids, tail_neg_ids, self.prediction_l2loss_lambda, False)
        self.gat_embed, (head_ids, tail_pos_ids, tail_neg_ids) = self._embeddings_and_ids(
            head_ids, tail_pos_ids, tail_neg_ids)
        self._raise_bad_ids()
        return ops.dot_loss(self.gat_embed, head_ids, tail_pos_ids, tail_neg_ids, self.prediction_l2loss_lambda,
                            self._table_grad_stays_inside())
