#!/usr/bin/env python3
"""Filtered ranking under the MLP pair head (rank_pairs_mlp / evaluate_mlp_ranking, the prepare and count kernels of
lkg_pairmlp.hip) on the GPU box; one JSON line per measurement (--out FILE: also written there, default
profiles/pairmlp_rank_micro.jsonl).  One process; times are medians of HIP-event intervals after a warm-up, the two sides
of a comparison alternated.
  1. the count kernel (lkg_pair_mlp_count_f32) against the store kernel (lkg_pair_mlp_scores_f32) on the same projected
     tables: N_c in {100 k, 1 M}, B in {64, 1024}, C = 300.  Both do 2 x 128 x 64 FLOP per pair through the same
     pm_pair_logits; the line carries the ratio, the spread (max - min) / median of the store kernel's own timings, the
     TFLOP/s and the share of the 157.3 TF f32 matrix peak (matrix-bound), and the prepare kernel's time without a filter.
  2. evaluate_mlp_ranking end to end, 10 k pairs, both sides, filtered by every known triple, on the synthetic 1 M entity /
     10 M edge graph (16 relations) and on the reference KG fixture (tests/golden/kg_pre_training_train.npz), against the
     route without it: mlp_scores(logits=True) over query chunks that fit memory, the known pairs masked, the compares and
     sums in torch.  Both use only the public API; their counts must be equal (the line says so).  The split of the new
     route -- projections, prepare, count -- is timed at the ops level on the same operands.
The table is a random normalised N x C stand-in for the encoder's output with a random head (the encoder pass is in neither
route)."""
import argparse
import json
import os
import statistics
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import _native as N  # noqa: E402
from literalkg_amd import ops, pairmlp, ranking, synth  # noqa: E402

PEAK_F32 = 157.3
FLOP_PER_PAIR = 2 * 128 * 64
BASELINE_BYTES = 4 << 30              # stored logits per chunk of queries on the route without the count kernel
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def interval(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def timed(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    return statistics.median(interval(fn) for _ in range(reps))


def alternated(f, g, reps=5, warm=1):
    """all timings of f and of g, taken in turns"""
    for _ in range(warm):
        f()
        g()
    tf, tg = [], []
    for _ in range(reps):
        tf.append(interval(f))
        tg.append(interval(g))
    return tf, tg


class TableModel:
    """What mlp_scores / rank_pairs_mlp / evaluate_mlp_ranking read of a LiteralKG, over a given table."""

    def __init__(self, table, n_rel, gen):
        c = table.shape[1]
        self.T = table
        self.entity_embed = SimpleNamespace(weight=table)
        self.n_entities, self.n_relations, self.scoring, self.training = table.shape[0], n_rel, "dot", False
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

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        self.training = mode
        return self


def kernel_sweep(ns, c=300):
    gen = torch.Generator().manual_seed(2026)
    dgen = torch.Generator(device=dev).manual_seed(2026)
    for n in ns:
        table = torch.nn.functional.normalize(torch.randn(n, c, device=dev, generator=dgen), dim=1)
        model = TableModel(table, 1, gen)
        head = pairmlp.fold_mlp_head(model)
        w = (head.w2, head.b2, head.w3, head.b3)
        v = ops.gemm_tall([table], [[head.w1t]], trans_b=True)
        for b in (64, 1024):
            q = torch.randint(0, n, (b,), device=dev, generator=dgen)
            truth = torch.randint(0, n, (b,), device=dev, generator=dgen)
            uq = ops.gemm_tall([ops.gather_rows(table, q)], [[head.w1h]], trans_b=True, bias=head.b1)
            out = torch.empty((b, n), dtype=torch.float32, device=dev)
            better, equal, thr = ops.pair_mlp_rank_count(uq, v, *w, truth)
            args = (b, n, N.ptr(uq), uq.stride(0), N.ptr(v), v.stride(0), *(N.ptr(x) for x in w))
            st = torch.cuda.current_stream().cuda_stream

            def count():
                N.call("lkg_pair_mlp_count_f32", *args, N.ptr(thr), N.ptr(truth), N.ptr(better), N.ptr(equal), st)

            def prepare():
                N.call("lkg_pair_mlp_prepare_f32", *args, N.ptr(truth), n, None, None, None, None, None, None, None,
                       N.ptr(thr), N.ptr(better), N.ptr(equal), st)

            t_store, t_count = alternated(lambda: ops.pair_mlp_scores(uq, v, *w, out=out), count)
            store_ms, count_ms = statistics.median(t_store), statistics.median(t_count)
            prepare_ms = timed(prepare)
            wb, we, _ = ops.pair_mlp_rank_count(uq, v, *w, truth)           # (the timed launches added to better / equal)
            zt = out.gather(1, truth[:, None])
            same = bool(torch.equal(wb.long(), (out > zt).sum(1)) and torch.equal(we.long(), (out == zt).sum(1) - 1))
            tf = lambda ms: float(b) * n * FLOP_PER_PAIR / (ms * 1e-3) / 1e12
            emit(what="count_vs_store_kernel", n_cand=n, c=c, b=b, count_ms=round(count_ms, 3), store_ms=round(store_ms, 3),
                 count_over_store=round(count_ms / store_ms, 4),
                 store_spread=round((max(t_store) - min(t_store)) / store_ms, 4),
                 count_spread=round((max(t_count) - min(t_count)) / count_ms, 4),
                 count_tflops=round(tf(count_ms), 1), store_tflops=round(tf(store_ms), 1),
                 count_frac_of_f32_matrix_peak=round(tf(count_ms) / PEAK_F32, 3), bound="matrix",
                 prepare_ms=round(prepare_ms, 3), counts_equal_stored_logits=same)
            del out, uq
        del table, model, v


class TorchFilter:
    """the known pairs of one side, sorted by (query end, relation), for the route that masks stored logits"""

    def __init__(self, a, rel, b_, n_rel):
        key = a * n_rel + rel
        order = torch.argsort(key)
        self.key, self.b, self.n_rel = key[order].contiguous(), b_[order].contiguous(), n_rel

    def pairs(self, q, r):
        k = q * self.n_rel + r
        lo, hi = torch.searchsorted(self.key, k), torch.searchsorted(self.key, k, right=True)
        cnt = hi - lo
        rows = torch.repeat_interleave(torch.arange(q.numel(), device=dev), cnt)
        offs = torch.arange(int(cnt.sum()), device=dev) - torch.repeat_interleave(torch.cumsum(cnt, 0) - cnt, cnt)
        return rows, self.b[torch.repeat_interleave(lo, cnt) + offs]


def stored_logits_route(model, h, r, t, filters):
    """(better, equal), 2 x B, from mlp_scores(logits=True) over chunks of queries, in torch"""
    n, b = model.n_entities, h.numel()
    every = torch.arange(n, device=dev)
    step = max(1, BASELINE_BYTES // (4 * n))
    better = torch.empty((2, b), dtype=torch.int64, device=dev)
    equal = torch.empty((2, b), dtype=torch.int64, device=dev)
    for j, (q, truth) in enumerate(((h, t), (t, h))):
        for lo in range(0, b, step):
            qq, tt, rr = q[lo:lo + step], truth[lo:lo + step], r[lo:lo + step]
            rows = torch.arange(qq.numel(), device=dev)
            kr, kc = filters[j].pairs(qq, rr)
            if j == 0:                           # rows = queries
                d = pairmlp.mlp_scores(model, qq, every, logits=True)
                zt = d[rows, tt][:, None].clone()
                d[kr, kc] = -float("inf")
                d[rows, tt] = -float("inf")
                better[j, lo:lo + step], equal[j, lo:lo + step] = (d > zt).sum(1), (d == zt).sum(1)
            else:                                # the pairs (c, query): columns = queries
                d = pairmlp.mlp_scores(model, every, qq, logits=True)
                zt = d[tt, rows][None, :].clone()
                d[kc, kr] = -float("inf")
                d[tt, rows] = -float("inf")
                better[j, lo:lo + step], equal[j, lo:lo + step] = (d > zt).sum(0), (d == zt).sum(0)
            del d
    return better, equal


def end_to_end(name, n, h, r, t, n_rel, n_test, c=300, seed=7):
    g = torch.Generator(device=dev).manual_seed(seed)
    table = torch.nn.functional.normalize(torch.randn(n, c, device=dev, generator=g), dim=1)
    model = TableModel(table, n_rel, torch.Generator().manual_seed(seed))
    pick = torch.randperm(h.numel(), device=dev, generator=g)[:n_test]
    th, tr, tt = h[pick], r[pick], t[pick]
    known = ranking.KnownTriples(h, r, t, n, n_rel)
    filters = (TorchFilter(h, r, t, n_rel), TorchFilter(t, r, h, n_rel))
    head = pairmlp.fold_mlp_head(model)
    w = (head.w2, head.b2, head.w3, head.b3)

    def projections():
        return [(pairmlp._project(ops.gather_rows(table, th), head.w1h, head.b1), pairmlp._project(table, head.w1t)),
                (pairmlp._project(ops.gather_rows(table, tt), head.w1t), pairmlp._project(table, head.w1h, head.b1))]
    proj_ms = timed(projections, reps=3)
    sides = projections()
    st = torch.cuda.current_stream().cuda_stream
    bufs = [torch.empty(n_test, dtype=torch.int32, device=dev) for _ in range(2)] + \
        [torch.empty(n_test, dtype=torch.float32, device=dev)]

    def prepare():
        for (uq, v), q, truth, filt in zip(sides, (th, tt), (tt, th), (known.by_head, known.by_tail)):
            N.call("lkg_pair_mlp_prepare_f32", n_test, n, N.ptr(uq), uq.stride(0), N.ptr(v), v.stride(0),
                   *(N.ptr(x) for x in w), N.ptr(truth), n, None, N.ptr(q), N.ptr(tr), *(N.ptr(x) for x in filt),
                   N.ptr(bufs[2]), N.ptr(bufs[0]), N.ptr(bufs[1]), st)
    prepare_ms = timed(prepare, reps=3)

    def count():
        for (uq, v), q, truth, filt in zip(sides, (th, tt), (tt, th), (known.by_head, known.by_tail)):
            ops.pair_mlp_rank_count(uq, v, *w, truth, filt, q, tr)
    both_ms = timed(count, reps=1)
    del sides
    kw = dict(known=known, ks=(1, 3, 10), side="both")
    got = {}
    t_new, t_old = alternated(lambda: got.__setitem__("new", pairmlp.evaluate_mlp_ranking(model, th, tt, tr, **kw)),
                              lambda: got.__setitem__("old", stored_logits_route(model, th, tr, tt, filters)), reps=1, warm=1)
    res = pairmlp.rank_pairs_mlp(model, th, tt, tr, side="both", known=known)
    (wb, we), m = got["old"], got["new"]
    assert m == {**ranking.metrics_from_counts(res.better.cpu(), res.equal.cpu()),
                 "tail": ranking.metrics_from_counts(res.better[0].cpu(), res.equal[0].cpu()),
                 "head": ranking.metrics_from_counts(res.better[1].cpu(), res.equal[1].cpu())}
    flop = 2.0 * n_test * n * FLOP_PER_PAIR
    emit(what="end_to_end", graph=name, n=n, known=int(h.numel()), n_rel=n_rel, pairs=n_test, c=c,
         evaluate_mlp_ranking_ms=round(t_new[0], 2), stored_logits_route_ms=round(t_old[0], 2),
         speedup=round(t_old[0] / t_new[0], 2), projection_ms=round(proj_ms, 2), prepare_ms=round(prepare_ms, 2),
         count_ms=round(both_ms - prepare_ms, 2), count_tflops=round(flop / ((both_ms - prepare_ms) * 1e-3) / 1e12, 1),
         counts_equal=bool(torch.equal(res.better, wb) and torch.equal(res.equal, we)),
         mr=round(m["mr"], 2), mrr=round(m["mrr"], 5), hits10=round(m["hits@10"], 5))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairmlp_rank_micro.jsonl"))
    ap.add_argument("--n", type=int, nargs="*", default=[100_000, 1_000_000])
    ap.add_argument("--pairs", type=int, default=10_000)
    ap.add_argument("--skip-synthetic", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(2026)              # (the heads' biases come from the global generator)
    kernel_sweep(a.n)
    if not a.skip_synthetic:
        h, t, r = synth.make_kg_device(1_000_000, 10_000_000, "zipf", 2022, dev)[:3]
        end_to_end("synthetic_1M_10M", 1_000_000, h, r % 16, t, 16, a.pairs)
        del h, r, t
    kg = np.load(os.path.join(ROOT, "tests", "golden", "kg_pre_training_train.npz"))
    h, r, t = (torch.from_numpy(kg[x]).long().to(dev) for x in ("h", "r", "t"))
    n = int(max(h.max(), t.max())) + 1
    end_to_end("kg_pre_training_train", n, h, r, t, int(r.max()) + 1, a.pairs)
    if a.out:
        with open(a.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
