#!/usr/bin/env python3
"""Relation prediction (score_relations / rank_relations, lkg_relation_scores_f32 and lkg_relation_order_f32) on the GPU
box; one JSON line per measurement (--out FILE: also written there, default profiles/relations_micro.jsonl; --append keeps
what the file holds, so that every P runs as a process of its own under its own time limit).  Times are medians of
HIP-event intervals after a warm-up, the two sides of a comparison alternated.  Per P in {10 k, 100 k, 1 M} random pairs
on a random 1 M x 300 table (a stand-in for the encoder's output, which is in neither route), k = 300, R = 16 relations:
  a. the scan kernel (one launch over the R relations, the shared table of 'transe') against R launches of
     lkg_triple_scores_f32 on the same operands, with identical bits; the line carries the time of reading two k-float
     rows per pair ONCE at the HBM rate a float4 copy reaches here (6.29 TB/s);
  b. the order kernel on the P x R matrix: counts alone, counts with a filter, top-1 and top-10;
  c. rank_relations end to end, 'transe' and 'transr', against the route without it: a Python loop of score_triples over
     the relations, then the compares and sums in torch on the device -- with equal counts."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import ops, relations, triples  # noqa: E402
from literalkg_amd.ranking import KnownTriples  # noqa: E402
from pairmlp_rank_micro import alternated, dev, emit, lines, timed  # noqa: E402
from triples_micro import HBM_COPY_TB_S, TripleModel  # noqa: E402


def loop_route(model, h, r, t, scoring):
    """better, equal by the route without rank_relations: one score_triples per relation, compares in torch"""
    n_rel = model.n_relations
    s = torch.stack([triples.score_triples(model, h, torch.full_like(h, j), t, scoring=scoring) for j in range(n_rel)], 1)
    ts = s.gather(1, r[:, None])
    other = torch.arange(n_rel, device=h.device)[None, :] != r[:, None]
    return ((s < ts) & other).sum(1), ((s == ts) & other).sum(1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relations_micro.jsonl"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--pairs", type=int, nargs="*", default=[10_000, 100_000, 1_000_000])
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--relations", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dgen = torch.Generator(device=dev).manual_seed(2026)
    n, k, n_rel = a.n, a.k, a.relations
    table = torch.randn(n, k, device=dev, generator=dgen)
    relemb = torch.randn(n_rel, k, device=dev, generator=dgen) * 0.3
    trans_m = torch.randn(n_rel, k, k, device=dev, generator=dgen) / math.sqrt(k)
    pn = ops.rank_sqnorm(table)
    for p in a.pairs:
        h = torch.randint(0, n, (p,), device=dev, generator=dgen)
        t = torch.randint(0, n, (p,), device=dev, generator=dgen)
        r = torch.randint(0, n_rel, (p,), device=dev, generator=dgen)
        # a. the scan kernel against R launches of the triple kernel
        s_new = torch.empty((p, n_rel), dtype=torch.float32, device=dev)
        s_old = torch.empty((n_rel, p), dtype=torch.float32, device=dev)
        rels = [torch.full_like(h, j) for j in range(n_rel)]

        def launches():
            for j in range(n_rel):
                ops.triple_scores(table, h, t, pn, relemb, rels[j], out=s_old[j])
        t_new, t_old = alternated(lambda: ops.relation_scores(table, pn, h, t, relemb, 1.0, out=s_new), launches,
                                  reps=a.reps)
        once = p * 2 * k * 4 / (HBM_COPY_TB_S * 1e12) * 1e3
        emit(what="scan_kernel", pairs=p, n=n, k=k, relations=n_rel, relation_scores_ms=round(statistics.median(t_new), 4),
             triple_scores_launches_ms=round(statistics.median(t_old), 4),
             speedup=round(statistics.median(t_old) / statistics.median(t_new), 2),
             identical_bits=bool(torch.equal(s_new.view(torch.int32), s_old.t().contiguous().view(torch.int32))),
             rows_once_at_hbm_copy_rate_ms=round(once, 4), times_that_floor=round(statistics.median(t_new) / once, 2))
        del s_old, rels
        # b. the order kernel
        known = KnownTriples(h, r, t, n, n_rel)                          # every truth known: the filter is looked up per pair
        filt = known.by_head
        emit(what="order_kernel", pairs=p, relations=n_rel,
             counts_ms=round(timed(lambda: ops.relation_order(s_new, truth=r), reps=a.reps), 4),
             filtered_counts_ms=round(timed(lambda: ops.relation_order(s_new, truth=r, filt=filt, filter_row=h,
                                                                       filter_col=t), reps=a.reps), 4),
             top1_ms=round(timed(lambda: ops.relation_order(s_new, top_k=1), reps=a.reps), 4),
             top10_ms=round(timed(lambda: ops.relation_order(s_new, top_k=10), reps=a.reps), 4),
             matrix_read_at_hbm_copy_rate_ms=round(p * n_rel * 4 / (HBM_COPY_TB_S * 1e12) * 1e3, 5))
        del s_new, known, filt
        # c. end to end
        for scoring in ("transe", "transr"):
            model = TripleModel(table, relemb, trans_m if scoring == "transr" else None, scoring)
            got = {}
            t_new, t_old = alternated(lambda: got.__setitem__("new", relations.rank_relations(model, h, r, t)),
                                      lambda: got.__setitem__("old", loop_route(model, h, r, t, scoring)),
                                      reps=3 if scoring == "transr" else a.reps)
            res, (ob, oe) = got["new"], got["old"]
            assert torch.equal(res.better, ob) and torch.equal(res.equal, oe), "the two routes count differently"
            emit(what="end_to_end_rank", scoring=scoring, pairs=p, n=n, k=k, relations=n_rel,
                 rank_relations_ms=round(statistics.median(t_new), 3), loop_route_ms=round(statistics.median(t_old), 3),
                 speedup=round(statistics.median(t_old) / statistics.median(t_new), 2), equal_counts=True,
                 mean_rank=float(res.rank.mean()))
            del got, res, ob, oe
            torch.cuda.empty_cache()
        del h, t, r
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
