#!/usr/bin/env python3
"""Threshold retrieval (lkg_accept.hip, literalkg_amd/accepted.py) on the GPU box; one JSON line per measurement, all of
them also written to profiles/accepted_micro.jsonl (--out FILE: elsewhere).
  1. the kernels alone at N = 1 M, k_dim = 300, B = 8192, 'transe' operands, no filter: lkg_accept_count_f32 against the
     counting kernel of filtered ranking (lkg_rank_prepare_f32 + lkg_rank_count_f32: the same loop, a cheaper epilogue)
     in the same process, then count / emit / order at per-query thresholds set for about 10, 100 and 1000 accepted
     candidates -- the 10th and 100th best score of lkg_topk_select_f32, and a bisection on the count pass itself;
  2. predict_accepted end to end on 10 k TransR tail queries of the synthetic 1 M entity / 10 M triple graph (16
     relations), filtered by every triple, against predict_topk(k=10) on the same queries and against the only route
     there was for lists longer than 128: a chunked dense  P_r q^T  in torch with a compare and nonzero.  The two routes
     round differently; the (query, candidate) decisions on which they differ are counted.
The table is a random N x C stand-in for the encoder's output (the encoder pass is not what is measured here)."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import accepted, ops, ranking, synth, topk  # noqa: E402

PEAK_F32 = 157.3
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def timed(fn, reps=3, warm=1):
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


def kernel_level(n, kd, b):
    g = torch.Generator(device=dev).manual_seed(3)
    p = torch.randn(n, kd, device=dev, generator=g)
    q = torch.randn(b, kd, device=dev, generator=g)
    pn, qn = ops.rank_sqnorm(p), ops.rank_sqnorm(q)
    truth = torch.randint(0, n, (b,), device=dev, generator=g)
    flop = 2.0 * b * n * kd
    rank_ms = timed(lambda: ops.rank_count(q, p, pn, truth))
    top = ops.topk_select(q, p, pn, 100)[2]                       # the reported scores, best first
    none = torch.full((b,), float("-inf"), device=dev)
    lo, hi = top[:, 99].clone(), top[:, 99] + 4.0 * (top[:, 99] - top[:, 9])
    for _ in range(8):                                            # hi: at least 1000 accepted everywhere
        short = ops.accept_count(q, p, pn, hi, qn=qn) < 1000
        if not bool(short.any()):
            break
        hi = torch.where(short, hi + 2.0 * (hi - lo), hi)
    for _ in range(14):                                           # bisection per query on the count pass
        mid = 0.5 * (lo + hi)
        enough = ops.accept_count(q, p, pn, mid, qn=qn) >= 1000
        lo, hi = torch.where(enough, lo, mid), torch.where(enough, mid, hi)
    for target, thr in ((0, none), (10, top[:, 9].contiguous()), (100, top[:, 99].contiguous()), (1000, hi)):
        cnt = ops.accept_count(q, p, pn, thr, qn=qn)
        m = int(cnt.sum())
        count_ms = timed(lambda: ops.accept_count(q, p, pn, thr, qn=qn))
        rec = dict(what="accept_kernels", n=n, k_dim=kd, b=b, target_per_query=target, accepted=m,
                   mean_per_query=round(m / b, 2), count_ms=round(count_ms, 3), rank_count_ms=round(rank_ms, 3),
                   count_over_rank_count=round(count_ms / rank_ms, 3),
                   count_tflops=round(flop / (count_ms * 1e-3) / 1e12, 1),
                   rank_count_tflops=round(flop / (rank_ms * 1e-3) / 1e12, 1),
                   count_frac_of_f32_peak=round(flop / (count_ms * 1e-3) / 1e12 / PEAK_F32, 3))
        if m:
            emit_ms = timed(lambda: ops.accept_emit(q, p, pn, thr, cnt, qn=qn, total=m))
            rowptr, ii, ss, vv = ops.accept_emit(q, p, pn, thr, cnt, qn=qn, total=m)
            order_ms = timed(lambda: ops.accept_order(rowptr, ii, ss, vv, n))
            rec.update(emit_ms=round(emit_ms, 3), order_ms=round(order_ms, 3),
                       all_three_over_rank_count=round((count_ms + emit_ms + order_ms) / rank_ms, 3))
        emit(**rec)


def dense_route(model, ids, r, thr_rel, chunk=512):
    """(rowptr-free) per relation: P_r = T W_r, q = P_r[h] + e_r, d = |q|^2 + |p|^2 - 2 P_r q^T in torch, chunked over the
    queries; d <= thr; nonzero.  Returns the accepted (query position, candidate) pairs, unfiltered."""
    out_q, out_c = [], []
    for rr in torch.unique(r).tolist():
        pos = torch.nonzero(r == rr, as_tuple=True)[0]
        p = model.T @ model.gat_trans_M[rr]
        pn = (p * p).sum(1)
        q = p[ids[pos]] + model.relation_embed.weight[rr]
        qn = (q * q).sum(1)
        for lo in range(0, pos.numel(), chunk):
            qq = q[lo:lo + chunk]
            d = qn[lo:lo + chunk, None] + pn[None, :] - 2.0 * (qq @ p.T)
            hit = torch.nonzero(d <= thr_rel[rr])
            out_q.append(pos[lo + hit[:, 0]])
            out_c.append(hit[:, 1])
    return torch.cat(out_q), torch.cat(out_c)


def end_to_end(n, h, r, t, n_rel, n_test, c=300, kdim=300, seed=7):
    g = torch.Generator(device=dev).manual_seed(seed)
    table = torch.randn(n, c, device=dev, generator=g) * 0.1
    relemb = torch.randn(n_rel, kdim, device=dev, generator=g) * 0.1
    trans_m = torch.randn(n_rel, c, kdim, device=dev, generator=g) / c ** 0.5
    model = TableModel(table, relemb, trans_m)
    pick = torch.randperm(h.numel(), device=dev, generator=g)[:n_test]
    th, tr = h[pick], r[pick]
    known = ranking.KnownTriples(h, r, t, n, n_rel)
    top = topk.predict_topk(model, th, tr, side="tail", k=10, known=known)
    thr = torch.stack([top.scores[tr == rr, 9].median() if bool((tr == rr).any()) else top.scores[:, 9].median()
                       for rr in range(n_rel)]).float()          # per relation: the median 10th-best score
    topk_ms = timed(lambda: topk.predict_topk(model, th, tr, side="tail", k=10, known=known), reps=2)
    acc_ms = timed(lambda: accepted.predict_accepted(model, th, tr, thr, known=known), reps=2)
    cnt_ms = timed(lambda: accepted.count_accepted(model, th, tr, thr, known=known), reps=2)
    res = accepted.predict_accepted(model, th, tr, thr, known=known)
    dense_ms = timed(lambda: dense_route(model, th, tr, thr), reps=1)
    dq, dc = dense_route(model, th, tr, thr)
    raw = accepted.predict_accepted(model, th, tr, thr)            # unfiltered, as the dense route is
    rows = torch.repeat_interleave(torch.arange(n_test, device=dev), raw.counts)
    mine, theirs = torch.unique(rows * n + raw.ids), torch.unique(dq * n + dc)
    both = torch.isin(mine, theirs).sum().item()
    emit(what="end_to_end", graph="synthetic_1M_10M", n=n, known=int(h.numel()), n_rel=n_rel, test=n_test, c=c,
         k_dim=kdim, accepted=int(res.ids.numel()), mean_per_query=round(res.ids.numel() / n_test, 2),
         max_per_query=int(res.counts.max()), predict_accepted_ms=round(acc_ms, 2), count_accepted_ms=round(cnt_ms, 2),
         predict_topk10_ms=round(topk_ms, 2), dense_torch_ms=round(dense_ms, 2),
         accepted_over_topk=round(acc_ms / topk_ms, 3), dense_over_accepted=round(dense_ms / acc_ms, 3),
         unfiltered_accepted=int(mine.numel()), dense_accepted=int(theirs.numel()),
         decisions_only_here=int(mine.numel() - both), decisions_only_dense=int(theirs.numel() - both))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accepted_micro.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--b", type=int, default=8192)
    ap.add_argument("--test", type=int, default=10_000)
    a = ap.parse_args()
    kernel_level(a.n, 300, a.b)
    h, t, r = synth.make_kg_device(1_000_000, 10_000_000, "zipf", 2022, dev)[:3]
    end_to_end(1_000_000, h, r % 16, t, 16, a.test)
    with open(a.out, "w") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
