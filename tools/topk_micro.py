#!/usr/bin/env python3
"""Filtered top-k (lkg_topk.hip, literalkg_amd/topk.py) on the GPU box; one JSON line per measurement (--out FILE: also
written there).
  1. the selection kernels alone (lkg_topk_select_f32 + lkg_topk_merge_f32, no filter) at N = 1 M, k_dim in {256, 300},
     B in {1024, 8192}, top-k in {10, 100}, and in the same process the counting kernel (lkg_rank_prepare_f32 +
     lkg_rank_count_f32) at the same shape: times and their ratio;
  2. predict_topk end to end against rank_triples(side='tail') on the same 10 k tail queries, TransR, top-10, filtered by
     every triple: the synthetic 1 M entity / 10 M triple graph (16 relations) and the reference KG fixture
     (tests/golden/kg_pre_training_train.npz).
The table is a random N x C stand-in for the encoder's output (the encoder pass is not what is measured here)."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import ops, ranking, synth, topk  # noqa: E402

PEAK_F32 = 157.3
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def timed(fn, reps=5, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


class TableModel:
    def __init__(self, table, relemb, trans_m):
        self.T, self.gat_trans_M = table, trans_m
        self.entity_embed = SimpleNamespace(weight=table)
        self.relation_embed = SimpleNamespace(weight=relemb)
        self.n_entities, self.n_relations = table.shape[0], relemb.shape[0]
        self.relation_dim, self.scoring, self.training = relemb.shape[1], "transr", False

    def _table_for_inference(self):
        return self.T


def kernel_sweep(n):
    for kd in (256, 300):
        p = torch.randn(n, kd, device=dev)
        pn = ops.rank_sqnorm(p)
        for b in (1024, 8192):
            q = torch.randn(b, kd, device=dev)
            truth = torch.randint(0, n, (b,), device=dev)
            reps = 3 if b == 8192 else 5
            count_ms = timed(lambda: ops.rank_count(q, p, pn, truth), reps=reps)
            for k in (10, 100):
                sel_ms = timed(lambda: ops.topk_select(q, p, pn, k), reps=reps)
                tf = 2.0 * b * n * kd / (sel_ms * 1e-3) / 1e12
                emit(what="select_kernel", n=n, k_dim=kd, b=b, top_k=k, select_ms=round(sel_ms, 3),
                     count_ms=round(count_ms, 3), ratio=round(sel_ms / count_ms, 3), tflops=round(tf, 1),
                     frac_of_f32_peak=round(tf / PEAK_F32, 3))
        del p, pn


def end_to_end(name, n, h, r, t, n_rel, n_test, c=300, kdim=300, seed=7):
    g = torch.Generator(device=dev).manual_seed(seed)
    table = torch.randn(n, c, device=dev, generator=g) * 0.1
    relemb = torch.randn(n_rel, kdim, device=dev, generator=g) * 0.1
    trans_m = torch.randn(n_rel, c, kdim, device=dev, generator=g) / c ** 0.5
    model = TableModel(table, relemb, trans_m)
    pick = torch.randperm(h.numel(), device=dev, generator=g)[:n_test]
    th, tr, tt = h[pick], r[pick], t[pick]
    known = ranking.KnownTriples(h, r, t, n, n_rel)
    rank_ms = timed(lambda: ranking.rank_triples(model, th, tr, tt, side="tail", known=known), reps=2, warm=1)
    topk_ms = timed(lambda: topk.predict_topk(model, th, tr, side="tail", k=10, known=known), reps=2, warm=1)
    res = topk.predict_topk(model, th, tr, side="tail", k=10, known=known)
    emit(what="end_to_end", graph=name, n=n, known=int(h.numel()), n_rel=n_rel, test=n_test, c=c, k_dim=kdim, top_k=10,
         rank_triples_tail_ms=round(rank_ms, 2), predict_topk_ms=round(topk_ms, 2), ratio=round(topk_ms / rank_ms, 3),
         padded=int((res.ids < 0).sum()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--n", type=int, default=1_000_000)
    a = ap.parse_args()
    kernel_sweep(a.n)
    h, t, r = synth.make_kg_device(1_000_000, 10_000_000, "zipf", 2022, dev)[:3]
    end_to_end("synthetic_1M_10M", 1_000_000, h, r % 16, t, 16, 10_000)
    del h, r, t
    kg = np.load(os.path.join(ROOT, "tests", "golden", "kg_pre_training_train.npz"))
    h, r, t = (torch.from_numpy(kg[x]).long().to(dev) for x in ("h", "r", "t"))
    n = int(max(h.max(), t.max())) + 1
    end_to_end("kg_pre_training_train", n, h, r, t, int(r.max()) + 1, 10_000)
    if a.out:
        with open(a.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
