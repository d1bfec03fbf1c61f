#!/usr/bin/env python3
"""Multi-answer retrieval (lkg_retrieval.hip, literalkg_amd/retrieval.py) on the GPU box; one JSON line per measurement,
all of them also written to profiles/retrieval_micro.jsonl (--out FILE: elsewhere).  N = 1 M entities, k_dim = 300,
'transe' operands, 8192 answers in all, spread as m = 1, 4, 16, 64 and 512 answers per query (8192 / m queries):
  a. the kernels alone: lkg_retrieval_prepare_f32 + lkg_retrieval_count_f32 over the rows of those queries (a query with
     m answers is ceil(m / RETRIEVAL_SLICE) rows) against lkg_rank_prepare_f32 + lkg_rank_count_f32 on the SAME rows in
     the same process -- at m = 1 the price of the bucket epilogue -- and against the rank kernels over all 8192 answers,
     which is what the route without this kernel has to launch;
  b. end to end: rank_answers against that route -- rank_triples over all answers with the evaluated triples in
     ``known``, the answers' kernel scores from score_triples and the position arithmetic in torch.  The ``before``
     values of the two routes must be equal wherever rank_triples reports no tie, and inside its interval better ..
     better + equal elsewhere (the run stops otherwise).
One process, one warm-up, the mean of 3 timed calls; min and max of the three are the spread.  The table is a random
N x 300 stand-in for the encoder's output (the encoder pass is not what is measured here)."""
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
from literalkg_amd import ops, ranking, retrieval, triples  # noqa: E402

dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def timed(fn, reps=3, warm=1):
    """(mean, min, max) ms of reps calls, each ended by a device synchronise"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sum(ts) / reps, min(ts), max(ts)


class TableModel:
    def __init__(self, table, relemb):
        self.T, self.gat_trans_M = table, None
        self.entity_embed = SimpleNamespace(weight=table)
        self.relation_embed = SimpleNamespace(weight=relemb)
        self.n_entities, self.n_relations = table.shape[0], relemb.shape[0]
        self.relation_dim, self.scoring, self.training = relemb.shape[1], "transe", False

    def _table_for_inference(self):
        return self.T


def parent_route(model, h, r, t, known):
    """(before, position) without the retrieval kernels: one GEMM row per answer."""
    n = model.n_entities
    rk = ranking.rank_triples(model, h, r, t, side="tail", known=known, scoring="transe")
    s = triples.score_triples(model, h, r, t, scoring="transe", kernel_scores=True)
    query = torch.unique(r * n + h, return_inverse=True)[1]
    order = torch.argsort(t, stable=True)
    order = order[torch.argsort(s[order] + 0.0, stable=True)]
    order = order[torch.argsort(query[order], stable=True)]            # by (query, score, id)
    first = torch.zeros(int(query.max()) + 2, dtype=torch.int64, device=dev)
    first[1:] = torch.cumsum(torch.bincount(query), 0)
    index = torch.empty_like(order)
    index[order] = torch.arange(order.numel(), device=dev) - first[query[order]]
    return rk.better, 1 + rk.better + index, rk.equal                   # (before = better where nothing ties)


def measure(model, p, pn, m, total, gen):
    n, kd = p.shape
    tee = ops.RETRIEVAL_SLICE
    n_q = total // m
    h = torch.randperm(n, device=dev, generator=gen)[:n_q].repeat_interleave(m)
    r = torch.randint(0, model.n_relations, (n_q,), device=dev, generator=gen).repeat_interleave(m)
    base = torch.randint(0, n, (n_q, 1), device=dev, generator=gen)
    stride = torch.randint(1, max(n // m, 2), (n_q, 1), device=dev, generator=gen)
    t = ((base + stride * torch.arange(m, device=dev)[None, :]) % n).reshape(-1)      # m distinct answers per query
    known = ranking.KnownTriples(h, r, t, n, model.n_relations)
    # a. the kernels on the rows rank_answers builds
    res = retrieval.rank_answers(model, h, r, t, known=known, scoring="transe")
    e = model.relation_embed.weight
    q = ops.rank_queries(p, res.q_ids, e, res.q_rel, 1.0)
    key_ans, key_s, key_id, counts, qkey_ptr = retrieval._group_answers(
        model, "transe", p, pn, e, 1.0, res.q_ids, res.q_rel, res.a_query,
        torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(res.n_answers, 0)]), res.a_ids,
        torch.arange(res.q_ids.numel(), device=dev))
    n_slices = (counts + tee - 1) // tee
    row_base = torch.cumsum(n_slices, 0) - n_slices
    row_q = torch.repeat_interleave(torch.arange(counts.numel(), device=dev), n_slices)
    in_query = torch.arange(row_q.numel(), device=dev) - row_base[row_q]
    qkey_off, qkey_n = qkey_ptr[:-1][row_q], counts[row_q]
    key_off = qkey_off + in_query * tee
    key_n = torch.clamp(qkey_n - in_query * tee, max=tee).to(torch.int32)
    rows = row_q.numel()
    q_rows, truth_rows = q[row_q].contiguous(), key_id[key_off]
    count = timed(lambda: ops.retrieval_count(q, row_q, p, pn, key_off, key_n, qkey_off, qkey_n, key_s, key_id))
    rank_rows = timed(lambda: ops.rank_count(q_rows, p, pn, truth_rows))
    q_all = ops.rank_queries(p, h, e, r, 1.0)
    rank_all = timed(lambda: ops.rank_count(q_all, p, pn, t))
    flop = 2.0 * rows * n * kd
    emit(what="retrieval_kernels", n=n, k_dim=kd, answers=total, m=m, queries=n_q, rows=rows,
         retrieval_count_ms=round(count[0], 3), retrieval_count_min_max_ms=[round(count[1], 3), round(count[2], 3)],
         rank_count_same_rows_ms=round(rank_rows[0], 3),
         rank_count_same_rows_min_max_ms=[round(rank_rows[1], 3), round(rank_rows[2], 3)],
         retrieval_over_rank_same_rows=round(count[0] / rank_rows[0], 3),
         rank_count_all_answers_ms=round(rank_all[0], 3), retrieval_over_rank_all_answers=round(count[0] / rank_all[0], 3),
         retrieval_count_tflops=round(flop / (count[0] * 1e-3) / 1e12, 1))
    # b. end to end
    # at this size some answers tie with a candidate in float32: there rank_triples gives an interval, not a place
    before, position, equal = parent_route(model, h, r, t, known)
    clear = equal == 0
    if not torch.equal(before[clear], res.before[clear]) or bool((res.before < before).any()) or \
            bool((res.before > before + equal).any()):
        raise SystemExit(f"m = {m}: the two routes disagree")
    ours = timed(lambda: retrieval.rank_answers(model, h, r, t, known=known, scoring="transe"))
    theirs = timed(lambda: parent_route(model, h, r, t, known))
    emit(what="end_to_end", n=n, k_dim=kd, answers=total, m=m, queries=n_q, before_equal=True,
         answers_tied_with_a_candidate=int((~clear).sum()),
         rank_answers_ms=round(ours[0], 2), rank_answers_min_max_ms=[round(ours[1], 2), round(ours[2], 2)],
         parent_route_ms=round(theirs[0], 2), parent_route_min_max_ms=[round(theirs[1], 2), round(theirs[2], 2)],
         parent_over_rank_answers=round(theirs[0] / ours[0], 3),
         wins_beyond_parent_spread=bool(ours[0] < theirs[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "retrieval_micro.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--answers", type=int, default=8192)
    ap.add_argument("--m", type=int, nargs="*", default=[1, 4, 16, 64, 512])
    a = ap.parse_args()
    gen = torch.Generator(device=dev).manual_seed(3)
    table = torch.randn(a.n, 300, device=dev, generator=gen)
    relemb = torch.randn(4, 300, device=dev, generator=gen) * 0.3
    model = TableModel(table, relemb)
    pn = ops.rank_sqnorm(table)
    for m in a.m:
        measure(model, table, pn, m, a.answers, gen)
    with open(a.out, "w") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
