#!/usr/bin/env python3
"""Filtered ranking (lkg_rank.hip, literalkg_amd/ranking.py) on the GPU box; one JSON line per measurement (--out FILE: also
written there).
  1. the counting kernel alone (lkg_rank_prepare_f32 + lkg_rank_count_f32, no filter) at N = 1 M, k in {64, 256, 300},
     B_r in {64, 1024, 8192}: time and TFLOP/s (2 B_r N k) against the 157.3 TF f32 matrix peak;
  2. rank_triples end to end, TransR, both sides, filtered by every triple: the synthetic 1 M entity / 10 M edge graph
     (16 relations, 10 k test triples drawn from it) and the reference KG fixture (tests/golden/kg_pre_training_train.npz),
     with the filter build, the projections (tall GEMM + squared norms) and the counting reported separately.
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
from literalkg_amd import ops, ranking, synth  # noqa: E402

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
    for k in (64, 256, 300):
        p = torch.randn(n, k, device=dev)
        pn = ops.rank_sqnorm(p)
        for b in (64, 1024, 8192):
            q = torch.randn(b, k, device=dev)
            truth = torch.randint(0, n, (b,), device=dev)
            ms = timed(lambda: ops.rank_count(q, p, pn, truth), reps=3 if b == 8192 else 5)
            tf = 2.0 * b * n * k / (ms * 1e-3) / 1e12
            emit(what="count_kernel", n=n, k=k, b_r=b, ms=round(ms, 3), tflops=round(tf, 1),
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
    known = [None]
    filt_ms = timed(lambda: known.__setitem__(0, ranking.KnownTriples(h, r, t, n, n_rel)), reps=1, warm=1)
    rowmax = ops.row_absmax(table)
    present = torch.unique(tr).tolist()

    def projections():
        for rr in present:
            p = ops.gemm_tall([table], [[trans_m[rr]]], trans_b=False, rowmax=rowmax)
            ops.rank_sqnorm(p)
    proj_ms = timed(projections, reps=1, warm=1)
    total_ms = timed(lambda: ranking.rank_triples(model, th, tr, tt, side="both", known=known[0]), reps=1, warm=1)
    res = ranking.rank_triples(model, th, tr, tt, side="both", known=known[0])
    flop = 2.0 * 2 * n_test * n * kdim
    emit(what="end_to_end", graph=name, n=n, known=int(h.numel()), n_rel=n_rel, test=n_test, c=c, k=kdim,
         filter_build_ms=round(filt_ms, 2), projection_ms=round(proj_ms, 2),
         counting_ms=round(total_ms - proj_ms, 2), rank_triples_ms=round(total_ms, 2),
         count_tflops=round(flop / ((total_ms - proj_ms) * 1e-3) / 1e12, 1),
         mean_rank=float(res.rank.mean()))


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
