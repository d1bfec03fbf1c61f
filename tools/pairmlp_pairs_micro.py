#!/usr/bin/env python3
"""The MLP pair head on explicit labelled pairs (score_pairs_mlp / evaluate_mlp_classification, lkg_pair_mlp_pairs_f32 and
lkg_binary_curve_f32) on the GPU box; one JSON line per measurement (--out FILE: also written there, default
profiles/pairmlp_pairs_micro.jsonl).  One process; times are medians of HIP-event intervals after a warm-up, the two sides
of a comparison alternated.  Per P in {100 k, 1 M, 10 M} random pairs on a random normalised 1 M x 300 table (a stand-in
for the encoder's output, which is in neither route) with a random head:
  1. the pairs kernel on projected tables over the unique ids: logits + counts, logits only, counts only; the line carries
     the gathered bytes per second (1 KB of rows per pair) and the TFLOP/s (2 x 128 x 64 FLOP per pair);
  2. the curve kernel (ops.binary_curve) against a torch.sort-based AUC (rank sum, no tie handling) on the same logits;
  3. evaluate_mlp_classification end to end against the route without it: the eval-mode mode='mlp' forward
     (LiteralKG.train_MLP: gather, multi_linear, relu_batchnorm, linear, sigmoid) under no_grad, .round(), the compares and
     sums in torch on the device, and the torch.sort AUC.  The line says how many decisions differ between the routes."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import LiteralKG, ops, pairmlp  # noqa: E402
from pairmlp_rank_micro import TableModel, alternated, dev, emit, lines, timed  # noqa: E402

FLOP_PER_PAIR = 2 * 128 * 64
BYTES_PER_PAIR = 2 * 128 * 4


class EagerModel(TableModel):
    """TableModel with what LiteralKG.train_MLP reads besides the head: the table stands for the encoder pass"""
    gat_rows = None

    def __init__(self, table, gen):
        super().__init__(table, 1, gen)
        self.id_space = table.shape[0]

    def _embeddings_and_ids(self, *id_lists):
        return self.T, id_lists

    @staticmethod
    def _raise_bad_ids():
        ops.check_deferred_errors()

    def _table_grad_stays_inside(self):
        return False


def sort_auc(p, y):
    """rank-sum AUC of the scores p (ties not handled) against 0 / 1 labels"""
    order = torch.sort(p).indices
    ranks = torch.empty_like(order)
    ranks[order] = torch.arange(1, p.numel() + 1, device=p.device)
    pos = y.bool()
    n_pos = pos.sum()
    return (ranks[pos].sum() - n_pos * (n_pos + 1) // 2).double() / (n_pos * (p.numel() - n_pos)).double()


def parent_route(model, h, t, y):
    with torch.no_grad():
        p = LiteralKG.train_MLP(model, h, t).reshape(-1)
    pred = p.round()
    yb = y.bool()
    one = pred == 1
    tp, fp, tn, fn = (one & yb).sum(), (one & ~yb).sum(), (~one & ~yb).sum(), (~one & yb).sum()
    auc = sort_auc(p, y)
    vals = torch.stack([tp, fp, tn, fn]).tolist()
    return vals, float(auc), pred


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairmlp_pairs_micro.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, nargs="*", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--c", type=int, default=300)
    a = ap.parse_args()
    torch.manual_seed(2026)              # (the heads' biases come from the global generator)
    gen = torch.Generator().manual_seed(2026)
    dgen = torch.Generator(device=dev).manual_seed(2026)
    n = a.n
    table = torch.nn.functional.normalize(torch.randn(n, a.c, device=dev, generator=dgen), dim=1)
    model = EagerModel(table, gen)
    head = pairmlp.fold_mlp_head(model)
    w = (head.w2, head.b2, head.w3, head.b3)
    for p in a.pairs:
        h = torch.randint(0, n, (p,), device=dev, generator=dgen)
        t = torch.randint(0, n, (p,), device=dev, generator=dgen)
        y = (torch.rand(p, device=dev, generator=dgen) < 0.5).to(torch.uint8)
        # 1. the kernel
        u, u_idx = pairmlp._pair_side(table, h, head.w1h, head.b1)
        v, v_idx = pairmlp._pair_side(table, t, head.w1t, None)
        z = torch.empty(p, dtype=torch.float32, device=dev)
        cnt = torch.zeros(5, dtype=torch.int64, device=dev)
        both = timed(lambda: ops.pair_mlp_pairs(u, v, *w, u_idx, v_idx, y, 0.0, True, z, cnt), reps=5)
        logits_only = timed(lambda: ops.pair_mlp_pairs(u, v, *w, u_idx, v_idx, out=z), reps=5)
        counts_only = timed(lambda: ops.pair_mlp_pairs(u, v, *w, u_idx, v_idx, y, 0.0, False, None, cnt), reps=5)
        emit(what="pairs_kernel", pairs=p, n=n, c=a.c, rows_u=u.shape[0], rows_v=v.shape[0],
             logits_and_counts_ms=round(both, 4), logits_only_ms=round(logits_only, 4), counts_only_ms=round(counts_only, 4),
             gathered_gb_per_s=round(p * BYTES_PER_PAIR / (both * 1e-3) / 1e9, 1),
             tflops=round(p * FLOP_PER_PAIR / (both * 1e-3) / 1e12, 2))
        del u, v, u_idx, v_idx
        # 2. the curve kernel against a torch.sort AUC
        t_curve, t_sort = alternated(lambda: ops.binary_curve(z, y), lambda: float(sort_auc(z, y)), reps=5)
        curve = ops.binary_curve(z, y)
        emit(what="curve_kernel", pairs=p, binary_curve_ms=round(statistics.median(t_curve), 3),
             torch_sort_auc_ms=round(statistics.median(t_sort), 3), n_groups=curve[3],
             roc_auc=curve[4] / (2 * curve[0] * curve[1]), torch_sort_auc=float(sort_auc(z, y)), average_precision=curve[5])
        # 3. end to end
        got = {}
        t_new, t_old = alternated(
            lambda: got.__setitem__("new", pairmlp.evaluate_mlp_classification(model, h, t, y)),
            lambda: got.__setitem__("old", parent_route(model, h, t, y)), reps=3)
        m, (old_counts, old_auc, pred) = got["new"], got["old"]
        differ = int(((pairmlp.score_pairs_mlp(model, h, t, logits=True) > 0) != (pred == 1)).sum())
        emit(what="end_to_end", pairs=p, n=n, c=a.c, evaluate_mlp_classification_ms=round(statistics.median(t_new), 2),
             mode_mlp_route_ms=round(statistics.median(t_old), 2),
             speedup=round(statistics.median(t_old) / statistics.median(t_new), 2),
             counts=[m["tp"], m["fp"], m["tn"], m["fn"], m["nan"]], mode_mlp_counts=old_counts, decisions_that_differ=differ,
             roc_auc=m["roc_auc"], mode_mlp_auc=old_auc, average_precision=m["average_precision"])
        del got, pred, h, t, y, z
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
