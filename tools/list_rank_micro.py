#!/usr/bin/env python3
"""Ranking against per-query candidate lists (score_lists / rank_in_lists, lkg_list_scores_f32 and lkg_list_count_f32) on
the GPU box; one JSON line per measurement (--out FILE: also written there, default profiles/list_rank_micro.jsonl;
--append keeps what the file holds, so that every part can run as a step of its own under its own time limit).  One
process per invocation; times are medians of HIP-event intervals after a warm-up, the routes of a comparison alternated.
  1. --kernels: on a random 1 M x 300 table under 'transe', B x M = 100 k x 500, 1 M x 50 and 64 x 100 k: the counting
     kernel, the scoring kernel, and lkg_triple_scores_f32 over the same slots flattened into B M explicit triples (the
     route without this module: the baseline).  Each line carries the kernel's bytes-per-slot bound computed from the
     shapes -- one k-float row, one 8-byte id, and 4 bytes where the score is stored -- as a time at the HBM rate a float4
     copy reaches here (6.29 TB/s), and the share of it the kernel reaches.
  2. --end-to-end: on the synthetic 1 M entity / 10 M edge graph under 'transr', rank_in_lists of 100 k triples x 500
     negatives, tail side, filtered by every known triple, against flattened score_triples + torch compares + a torch
     known-filter (sorted keys and searchsorted).  The counts of the two routes must be identical: the tool fails if not."""
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
from literalkg_amd import lists as LS, ops, ranking, synth, triples  # noqa: E402
from pairmlp_rank_micro import alternated, dev, emit, lines, timed  # noqa: E402
from triples_micro import HBM_COPY_TB_S, TripleModel  # noqa: E402

SHAPES = ((100_000, 500), (1_000_000, 50), (64, 100_000))


def bound_ms(slots, bytes_per_slot):
    return slots * bytes_per_slot / (HBM_COPY_TB_S * 1e12) * 1e3


def kernels(n, k, n_rel, shapes):
    g = torch.Generator(device=dev).manual_seed(2026)
    table = torch.randn(n, k, device=dev, generator=g)
    relemb = torch.randn(n_rel, k, device=dev, generator=g) * 0.3
    pn = ops.rank_sqnorm(table)
    for b, m in shapes:
        ids = torch.randint(0, n, (b,), device=dev, generator=g)
        truth = torch.randint(0, n, (b,), device=dev, generator=g)
        r = torch.randint(0, n_rel, (b,), device=dev, generator=g)
        lst = torch.randint(0, n, (b, m), device=dev, generator=g)
        out = torch.empty((b, m), dtype=torch.float32, device=dev)
        q = ops.rank_queries(table, ids, relemb, r, 1.0)
        qn = ops.rank_sqnorm(q)
        prep = timed(lambda: ops.rank_sqnorm(ops.rank_queries(table, ids, relemb, r, 1.0)), reps=5)
        q_idx = ids[:, None].expand(b, m).reshape(-1)
        rel = r[:, None].expand(b, m).reshape(-1)
        c_idx = lst.reshape(-1)
        flat_out = out.view(-1)
        t_count, t_flat = alternated(lambda: ops.list_count(q, table, pn, lst, truth),
                                     lambda: ops.triple_scores(table, q_idx, c_idx, pn, relemb, rel, out=flat_out), reps=5)
        t_scores, t_flat2 = alternated(lambda: ops.list_scores(q, table, pn, lst, qn, out=out),
                                       lambda: ops.triple_scores(table, q_idx, c_idx, pn, relemb, rel, out=flat_out), reps=5)
        count_ms, scores_ms = statistics.median(t_count), statistics.median(t_scores)
        flat_ms = statistics.median(t_flat + t_flat2)
        # the same bits, the same counts
        want = ops.triple_scores(table, q_idx, c_idx, pn, relemb, rel)[0].view(b, m)
        same_bits = bool(torch.equal(ops.list_scores(q, table, pn, lst, qn).view(torch.int32), want.view(torch.int32)))
        slots = b * m
        emit(what="kernels", queries=b, slots_per_query=m, n=n, k=k,
             list_count_ms=round(count_ms, 4), list_scores_ms=round(scores_ms, 4), flattened_triple_scores_ms=round(flat_ms, 4),
             query_rows_and_norms_ms=round(prep, 4),
             count_bytes_per_slot=4 * k + 8, scores_bytes_per_slot=4 * k + 12, flattened_bytes_per_slot=8 * k + 28,
             count_bound_ms=round(bound_ms(slots, 4 * k + 8), 4), scores_bound_ms=round(bound_ms(slots, 4 * k + 12), 4),
             count_share_of_bound=round(bound_ms(slots, 4 * k + 8) / count_ms, 3),
             scores_share_of_bound=round(bound_ms(slots, 4 * k + 12) / scores_ms, 3),
             flattened_over_count=round(flat_ms / count_ms, 2), flattened_over_scores=round(flat_ms / scores_ms, 2),
             identical_score_bits=same_bits)
        del ids, truth, r, lst, out, q, qn, q_idx, rel, c_idx, flat_out, want
        torch.cuda.empty_cache()


def flattened_route(model, h, r, t, lst, keys, n_rel, chunk):
    """(better, equal, kept) of the tail side by score_triples over explicit triples, compares and a known-filter in torch"""
    n = model.n_entities
    b, m = lst.shape
    better = torch.empty(b, dtype=torch.int64, device=dev)
    equal, kept = torch.empty_like(better), torch.empty_like(better)
    truth_scores = triples.score_triples(model, h, r, t, kernel_scores=True)
    for lo in range(0, b, chunk):
        hh, rr, tt, ll = h[lo:lo + chunk], r[lo:lo + chunk], t[lo:lo + chunk], lst[lo:lo + chunk]
        c = ll.shape[0]
        fh, fr = hh[:, None].expand(c, m).reshape(-1), rr[:, None].expand(c, m).reshape(-1)
        s = triples.score_triples(model, fh, fr, ll.reshape(-1), kernel_scores=True).view(c, m)
        key = ((fh * n_rel + fr) * n + ll.reshape(-1))
        at = torch.searchsorted(keys, key).clamp(max=keys.numel() - 1)
        keep = ((keys[at] != key).view(c, m)) & (ll != tt[:, None])
        ts = truth_scores[lo:lo + chunk, None]
        better[lo:lo + chunk] = ((s < ts) & keep).sum(1)
        equal[lo:lo + chunk] = ((s == ts) & keep).sum(1)
        kept[lo:lo + chunk] = keep.sum(1)
    return better, equal, kept


def end_to_end(n, edges, k, n_rel, b, m, chunk):
    g = torch.Generator(device=dev).manual_seed(7)
    h, t, r = synth.make_kg_device(n, edges, "zipf", 2022, dev)[:3]
    h, t, r = h.long(), t.long(), r.long() % n_rel
    table = torch.randn(n, k, device=dev, generator=g)
    relemb = torch.randn(n_rel, k, device=dev, generator=g) * 0.3
    trans_m = torch.randn(n_rel, k, k, device=dev, generator=g) / math.sqrt(k)
    model = TripleModel(table, relemb, trans_m, "transr")
    known = ranking.KnownTriples(h, r, t, n, n_rel)
    keys = torch.unique((h * n_rel + r) * n + t)
    pick = torch.randperm(h.numel(), device=dev, generator=g)[:b]
    th, tr, tt = h[pick], r[pick], t[pick]
    lst = torch.randint(0, n, (b, m), device=dev, generator=g)
    lst[::3, 0] = tt[::3]                                                     # the truth inside its own list
    lst[1::3, 1] = t[(pick[1::3] + 1) % h.numel()]                            # tails that are often known with the query
    got = {}
    t_new, t_old = alternated(lambda: got.__setitem__("new", LS.rank_in_lists(model, th, tr, tt, lst, known=known)),
                              lambda: got.__setitem__("old", flattened_route(model, th, tr, tt, lst, keys, n_rel, chunk)),
                              reps=3)
    new, old = got["new"], got["old"]
    identical = all(bool(torch.equal(a, b_)) for a, b_ in zip((new.better, new.equal, new.kept), old))
    emit(what="end_to_end_rank_in_lists", n=n, edges=edges, k=k, relations=n_rel, triples=b, negatives=m, side="tail",
         filtered=True, rank_in_lists_ms=round(statistics.median(t_new), 2),
         flattened_route_ms=round(statistics.median(t_old), 2),
         speedup=round(statistics.median(t_old) / statistics.median(t_new), 2), identical_counts=identical,
         slots_dropped=int(b * m - int(new.kept.sum())), mean_rank=float(new.rank.mean()))
    return identical


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "list_rank_micro.jsonl"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--end-to-end", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--relations", type=int, default=16)
    ap.add_argument("--triples", type=int, default=100_000)
    ap.add_argument("--negatives", type=int, default=500)
    ap.add_argument("--chunk", type=int, default=20_000, help="queries per chunk of the flattened route")
    a = ap.parse_args()
    both = not (a.kernels or a.end_to_end)
    ok = True
    if a.kernels or both:
        kernels(a.n, a.k, a.relations, SHAPES)
    if a.end_to_end or both:
        ok = end_to_end(a.n, a.edges, a.k, a.relations, a.triples, a.negatives, a.chunk)
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")
    if not ok:
        sys.exit("the counts of rank_in_lists and of the flattened route differ")


if __name__ == "__main__":
    main()
