#!/usr/bin/env python3
"""Threshold retrieval under the MLP pair head (lkg_pairmlp.hip: pair_mlp_accept_kernel; literalkg_amd/pairmlp.py:
predict_accepted_mlp) on the GPU box; one JSON line per measurement, all of them also written to
profiles/pair_accepted_micro.jsonl (--out FILE: elsewhere).  One process, a warm-up, device events, the routes taken in
turns.  Everything at 1024 queries x 1 M candidates, C = 300, on a random table (the encoder pass is not measured here).
  1. the kernels alone: lkg_pair_mlp_accept_count_f32 and lkg_pair_mlp_accept_append_f32 against lkg_pair_mlp_count_f32
     (the ranking count: the same loop, two compares and no filter) on the same operands, at per-query thresholds set for
     about 10 / 100 / 1000 accepted candidates (quantiles of each query's logits against 65 536 sampled candidates);
  2. one pass against two: predict_accepted_mlp with the default buffer against buffer=0 at the same three thresholds;
  3. end to end against the route there was: mlp_scores(logits=True) in chunks of queries, a compare, the known filter
     and an order in torch, held to the same lists -- unfiltered and filtered by every known triple, on the synthetic
     1 M entity / 10 M triple graph and on the reference KG fixture (tests/golden/kg_pre_training_train.npz)."""
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
DENSE_BYTES = 1 << 30                 # stored logits per chunk of queries on the torch route
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


def in_turns(fns, reps=5, warm=1):
    """{name: [ms, ...]}: all timings of every route, the routes taken in turns"""
    for _ in range(warm):
        for f in fns.values():
            f()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(interval(f))
    return out


def stats(ts):
    return dict(median_ms=round(statistics.median(ts), 3), min_ms=round(min(ts), 3), max_ms=round(max(ts), 3))


class TableModel:
    """What mlp_scores / predict_topk(scoring='mlp') / predict_accepted_mlp read of a LiteralKG, over a given table."""

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


def thresholds_for(model, q, targets, gen, sample=65536):
    """{target: float32[B]}: per query the logit that about `target` of the n candidates exceed, from a sample"""
    n = model.n_entities
    cols = torch.randperm(n, device=dev, generator=gen)[:min(sample, n)]
    z = pairmlp.mlp_scores(model, q, cols, logits=True)
    z = torch.sort(z, dim=1, descending=True).values
    out = {}
    for t in targets:
        k = min(z.shape[1] - 1, max(0, round(t * z.shape[1] / n)))
        out[t] = z[:, k].contiguous()
    return out


def kernel_level(model, q, thr_by_target):
    head = pairmlp.fold_mlp_head(model)
    table = model.T
    uq, v = pairmlp._project_sides(head, "tail", ops.gather_rows(table, q), table)
    b, n = uq.shape[0], v.shape[0]
    w = (head.w2, head.b2, head.w3, head.b3)
    flop = float(FLOP_PER_PAIR) * b * n
    truth = torch.full((b,), -1, dtype=torch.int64, device=dev)            # the ranking count leaves no candidate out
    better = torch.zeros(b, dtype=torch.int32, device=dev)
    equal = torch.zeros(b, dtype=torch.int32, device=dev)
    for target, thr in thr_by_target.items():
        def rank_count():
            N.call("lkg_pair_mlp_count_f32", b, n, N.ptr(uq), 128, N.ptr(v), 128, *(N.ptr(x) for x in w), N.ptr(thr),
                   N.ptr(truth), N.ptr(better), N.ptr(equal), ops._stream())
        cnt = ops.pair_mlp_accept_count(uq, v, *w, thr)
        m = int(cnt.sum())
        cap = 1 << 22
        ts = in_turns({"rank_count": rank_count, "accept_count": lambda: ops.pair_mlp_accept_count(uq, v, *w, thr),
                       "accept_append": lambda: ops.pair_mlp_accept_append(uq, v, *w, thr, capacity=cap)})
        med = {k: statistics.median(x) for k, x in ts.items()}
        emit(what="accept_kernels", b=b, n=n, target_per_query=target, accepted=m, mean_per_query=round(m / b, 2),
             fits_buffer=m <= cap, rank_count=stats(ts["rank_count"]), accept_count=stats(ts["accept_count"]),
             accept_append=stats(ts["accept_append"]),
             accept_count_over_rank_count=round(med["accept_count"] / med["rank_count"], 4),
             accept_append_over_rank_count=round(med["accept_append"] / med["rank_count"], 4),
             rank_count_spread=round(max(ts["rank_count"]) / min(ts["rank_count"]), 4),
             accept_count_tflops=round(flop / (med["accept_count"] * 1e-3) / 1e12, 1),
             accept_count_frac_of_f32_peak=round(flop / (med["accept_count"] * 1e-3) / 1e12 / PEAK_F32, 3))


def one_pass_against_two(model, q, thr_by_target):
    for target, thr in thr_by_target.items():
        one = lambda: pairmlp.predict_accepted_mlp(model, q, logit_threshold=thr)              # noqa: E731
        two = lambda: pairmlp.predict_accepted_mlp(model, q, logit_threshold=thr, buffer=0)    # noqa: E731
        a, c = one(), two()
        same = all(torch.equal(getattr(a, k), getattr(c, k)) for k in ("rowptr", "ids")) and \
            torch.equal(a.kernel_scores.view(torch.int32), c.kernel_scores.view(torch.int32))
        ts = in_turns({"one_pass": one, "two_pass": two}, reps=4)
        emit(what="one_pass_against_two", b=q.numel(), n=model.n_entities, target_per_query=target,
             accepted=int(a.ids.numel()), same_lists=bool(same), one_pass=stats(ts["one_pass"]),
             two_pass=stats(ts["two_pass"]),
             one_over_two=round(statistics.median(ts["one_pass"]) / statistics.median(ts["two_pass"]), 4))


def torch_route(model, q, thr, known_keys):
    """(counts, ids, logits) of the accepted lists through stored logits: mlp_scores in chunks of queries, a compare,
    the known filter (a sorted array of h * n + t keys, any relation) and the order (-z, id) in torch"""
    n, b = model.n_entities, q.numel()
    every = torch.arange(n, device=dev)
    chunk = max(1, DENSE_BYTES // (4 * n))
    ids, zs, counts = [], [], []
    for lo in range(0, b, chunk):
        qq = q[lo:lo + chunk]
        z = pairmlp.mlp_scores(model, qq, every, logits=True)
        hit = torch.nonzero(z > thr[lo:lo + chunk, None])                     # (row, id) in row-major order
        rows, cols = hit[:, 0], hit[:, 1]
        zz = z[rows, cols]
        if known_keys is not None and known_keys.numel():
            key = qq[rows] * n + cols
            at = torch.searchsorted(known_keys, key).clamp_max(known_keys.numel() - 1)
            keep = known_keys[at] != key
            rows, cols, zz = rows[keep], cols[keep], zz[keep]
        o = torch.sort(-zz, stable=True).indices                              # ids ascending already: ties keep them
        o = o[torch.sort(rows[o], stable=True).indices]
        ids.append(cols[o])
        zs.append(zz[o])
        counts.append(torch.bincount(rows, minlength=qq.numel()))
    return torch.cat(counts), torch.cat(ids), torch.cat(zs)


def end_to_end(name, n, h, r, t, n_rel, b, gen, c=300, target=100):
    table = torch.randn(n, c, device=dev, generator=gen) * 0.1
    model = TableModel(table, n_rel, torch.Generator().manual_seed(11))
    q = h[torch.randperm(h.numel(), device=dev, generator=gen)[:b]].contiguous()
    thr = thresholds_for(model, q, [min(target, max(1, n // 20))], gen)
    thr = next(iter(thr.values()))
    known = ranking.KnownTriples(h, r, t, n, n_rel)
    keys = torch.unique(h * n + t)
    for what, kn, kk in (("unfiltered", None, None), ("filtered", known, keys)):
        mine = lambda: pairmlp.predict_accepted_mlp(model, q, logit_threshold=thr, known=kn)   # noqa: E731
        theirs = lambda: torch_route(model, q, thr, kk)                                        # noqa: E731
        a, (cnt, ids, zz) = mine(), theirs()
        same = torch.equal(a.counts, cnt) and torch.equal(a.ids, ids) and \
            torch.equal(a.kernel_scores.view(torch.int32), zz.view(torch.int32))
        ts = in_turns({"predict_accepted_mlp": mine, "torch_route": theirs}, reps=3)
        emit(what="end_to_end", graph=name, filter=what, n=n, known=int(h.numel()), b=int(q.numel()), c=c,
             accepted=int(a.ids.numel()), mean_per_query=round(a.ids.numel() / q.numel(), 2),
             max_per_query=int(a.counts.max()), same_lists=bool(same),
             predict_accepted_mlp=stats(ts["predict_accepted_mlp"]), torch_route=stats(ts["torch_route"]),
             torch_over_ours=round(statistics.median(ts["torch_route"]) / statistics.median(ts["predict_accepted_mlp"]), 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pair_accepted_micro.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--b", type=int, default=1024)
    ap.add_argument("--skip-synthetic", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(2026)              # (the heads' biases come from the global generator)
    gen = torch.Generator(device=dev).manual_seed(5)
    table = torch.randn(a.n, 300, device=dev, generator=gen) * 0.1
    model = TableModel(table, 16, torch.Generator().manual_seed(11))
    q = torch.randint(0, a.n, (a.b,), device=dev, generator=gen)
    thr = thresholds_for(model, q, (10, 100, 1000), gen)
    kernel_level(model, q, thr)
    one_pass_against_two(model, q, thr)
    del model, table
    if not a.skip_synthetic:
        h, t, r = synth.make_kg_device(1_000_000, 10_000_000, "zipf", 2022, dev)[:3]
        end_to_end("synthetic_1M_10M", 1_000_000, h, r % 16, t, 16, a.b, gen)
        del h, r, t
    kg = np.load(os.path.join(ROOT, "tests", "golden", "kg_pre_training_train.npz"))
    h, r, t = (torch.from_numpy(kg[x]).long().to(dev) for x in ("h", "r", "t"))
    n = int(max(h.max(), t.max())) + 1
    end_to_end("kg_pre_training_train", n, h, r, t, int(r.max()) + 1, a.b, gen)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
