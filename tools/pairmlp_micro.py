#!/usr/bin/env python3
"""The MLP pair head at inference (lkg_pairmlp.hip, literalkg_amd/pairmlp.py) on the GPU box; one JSON line per shape
(--out FILE: also written there, default profiles/pairmlp_micro.jsonl).

For N_c in {100 k, 1 M} candidates, table width C in {256, 300}, B in {64, 1024} queries and k in {10, 100}, in one
process, on a random normalised N_c x C table with a random head (the encoder pass is in neither route):
  new       predict_topk(scoring='mlp'): gather + both fc1 projections (tall GEMM), lkg_pair_mlp_select_f32,
            lkg_topk_merge_f32, sigmoid of the B x k logits;
  baseline  the route without it: LiteralKG.train_MLP under eval() / no_grad() over the explicit B x N_c (h, t) pairs in
            chunks that fit memory, then torch.topk over the collected probabilities.  At B = 1024 the baseline is timed
            on the first 64 query rows and scaled by 16 (its cost per pair does not depend on B); the line says so.
Also per line: the projection alone, the select and the store kernel alone on the projected tables (ops level), their
ratio (the cost of selecting instead of storing), and the kernels' TFLOP/s counted as 2 x 128 x 64 per pair.
Times are medians of HIP-event intervals after a warm-up."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import LiteralKG, ops, pairmlp, topk  # noqa: E402

PEAK_F32 = 157.3
FLOP_PER_PAIR = 2 * 128 * 64
BASELINE_ROWS = 64
BASELINE_CHUNK = 1 << 21          # pairs per train_MLP call (2 gathered C-wide rows + 128 + 64 activations per pair)
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def timed(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


class TableModel:
    """What predict_topk / train_MLP read of a LiteralKG, over a given table."""

    def __init__(self, table, gen):
        c = table.shape[1]
        self.T = table
        self.entity_embed = SimpleNamespace(weight=table)
        self.n_entities = self.id_space = table.shape[0]
        self.n_relations, self.scoring, self.training = 1, "dot", False
        self.fc1, self.fc2, self.fc3 = torch.nn.Linear(2 * c, 128), torch.nn.Linear(128, 64), torch.nn.Linear(64, 1)
        self.norm1, self.norm2 = torch.nn.BatchNorm1d(128), torch.nn.BatchNorm1d(64)
        with torch.no_grad():
            for fc in (self.fc1, self.fc2, self.fc3):
                torch.nn.init.xavier_uniform_(fc.weight, generator=gen)
            for bn in (self.norm1, self.norm2):
                bn.running_mean.copy_(0.2 * torch.randn(bn.num_features, generator=gen))
                bn.running_var.copy_(0.5 + torch.rand(bn.num_features, generator=gen))
        for mod in (self.fc1, self.fc2, self.fc3, self.norm1, self.norm2):
            mod.to(dev).eval()

    def _table_for_inference(self):
        return self.T

    # what train_MLP calls on the model
    def _embeddings_and_ids(self, *id_lists):
        return self.T, id_lists

    def _raise_bad_ids(self):
        ops.check_deferred_errors()

    def _table_grad_stays_inside(self):
        return False


def baseline_topk(model, q, k):
    """the parent's route: every (h, t) pair through mode='mlp' in eval mode, then torch.topk"""
    n = model.n_entities
    rows_per_chunk = max(1, BASELINE_CHUNK // n)
    every = torch.arange(n, device=dev)
    probs = torch.empty((q.numel(), n), dtype=torch.float32, device=dev)
    with torch.no_grad():
        for lo in range(0, q.numel(), rows_per_chunk):
            qq = q[lo:lo + rows_per_chunk]
            h, t = qq.repeat_interleave(n), every.repeat(qq.numel())
            probs[lo:lo + qq.numel()] = LiteralKG.train_MLP(model, h, t).reshape(qq.numel(), n)
    return torch.topk(probs, k, dim=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairmlp_micro.jsonl"))
    ap.add_argument("--n", type=int, nargs="*", default=[100_000, 1_000_000])
    a = ap.parse_args()
    gen = torch.Generator().manual_seed(2026)
    dgen = torch.Generator(device=dev).manual_seed(2026)
    for n in a.n:
        for c in (256, 300):
            table = torch.nn.functional.normalize(torch.randn(n, c, device=dev, generator=dgen), dim=1)
            model = TableModel(table, gen)
            head = pairmlp.fold_mlp_head(model)
            v = ops.gemm_tall([table], [[head.w1t]], trans_b=True)
            proj_ms = timed(lambda: ops.gemm_tall([table], [[head.w1t]], trans_b=True))
            for b in (64, 1024):
                q = torch.randint(0, n, (b,), device=dev, generator=dgen)
                uq = ops.gemm_tall([ops.gather_rows(table, q)], [[head.w1h]], trans_b=True, bias=head.b1)
                w = (head.w2, head.b2, head.w3, head.b3)
                out = torch.empty((b, n), dtype=torch.float32, device=dev)
                store_ms = timed(lambda: ops.pair_mlp_scores(uq, v, *w, out=out))
                del out
                for k in (10, 100):
                    select_ms = timed(lambda: ops.pair_mlp_topk(uq, v, *w, k))
                    new_ms = timed(lambda: topk.predict_topk(model, q, None, k=k, scoring="mlp"))
                    rows = min(b, BASELINE_ROWS)
                    base_ms = timed(lambda: baseline_topk(model, q[:rows], k), reps=3 if n * rows <= (1 << 25) else 1)
                    scale = b / rows
                    res = topk.predict_topk(model, q[:rows], None, k=k, scoring="mlp")
                    base = baseline_topk(model, q[:rows], k)
                    pairs = float(b) * n
                    emit(what="pair_mlp_topk", n_cand=n, c=c, b=b, top_k=k, new_ms=round(new_ms, 3),
                         baseline_ms=round(base_ms * scale, 3),
                         baseline_note=("timed in full" if scale == 1 else
                                        f"timed on {rows} query rows ({round(base_ms, 3)} ms) and scaled by {scale:g}"),
                         speedup=round(base_ms * scale / new_ms, 1), projection_ms=round(proj_ms, 3),
                         select_ms=round(select_ms, 3), store_ms=round(store_ms, 3),
                         select_over_store=round(select_ms / store_ms, 3),
                         select_tflops=round(pairs * FLOP_PER_PAIR / (select_ms * 1e-3) / 1e12, 1),
                         store_tflops=round(pairs * FLOP_PER_PAIR / (store_ms * 1e-3) / 1e12, 1),
                         select_frac_of_f32_peak=round(pairs * FLOP_PER_PAIR / (select_ms * 1e-3) / 1e12 / PEAK_F32, 3),
                         same_top1_as_baseline=round(float((res.ids[:, 0] == base.indices[:, 0]).double().mean()), 3))
                del uq
            del table, model, v
    if a.out:
        with open(a.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
