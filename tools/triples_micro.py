#!/usr/bin/env python3
"""Triple classification under the model's own score (score_triples / fit_triple_thresholds /
evaluate_triple_classification, lkg_triple_scores_f32 and lkg_threshold_fit_f32) on the GPU box; one JSON line per
measurement (--out FILE: also written there, default profiles/triples_micro.jsonl; --append keeps what the file holds, so
that every P can run as a step of its own under its own time limit).  One process per invocation; times are medians of
HIP-event intervals after a warm-up, the two sides of a comparison alternated.  Per P in {100 k, 1 M, 10 M} random triples
over 16 relations on a random 1 M x 300 table (a stand-in for the encoder's output, which is in neither route), k = 300:
  1. the scoring kernel alone over the table (the 'transe' launch: |q|^2 + s with e_r added in-lane): scores only, scores
     + counts, kernel scores only (no |q|^2 pass); the line carries the gathered bytes per second (two k-float rows per
     triple) and the time of that gather at the HBM rate a float4 copy reaches here (6.29 TB/s);
  2. the fit kernel (ops.threshold_fit, per relation + pooled) against a torch.sort-based per-relation tie-aware fit on the
     device, with identical thresholds;
  3. 'transr' end to end: evaluate_triple_classification and fit_triple_thresholds against the route without them:
     table[h] @ W_r, table[t] @ W_r per relation in torch on the device, the squared distance, compares and sums in torch,
     and a torch.sort AUC.  The line says how many decisions differ between the routes."""
import argparse
import json
import math
import os
import statistics
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import ops, triples  # noqa: E402
from pairmlp_pairs_micro import sort_auc  # noqa: E402
from pairmlp_rank_micro import alternated, dev, emit, lines, timed  # noqa: E402

HBM_COPY_TB_S = 6.29


class TripleModel:
    """What the triple entry points read of a LiteralKG, over a given table."""

    def __init__(self, table, relemb, trans_m, scoring):
        self.T = table
        self.entity_embed = SimpleNamespace(weight=table)
        self.relation_embed = SimpleNamespace(weight=relemb)
        self.gat_trans_M = trans_m
        self.n_entities, self.n_relations, self.relation_dim = table.shape[0], relemb.shape[0], relemb.shape[1]
        self.scoring, self.training = scoring, False

    def _table_for_inference(self):
        return self.T

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode


def torch_fit(scores, y, r, n_rel):
    """per relation the tie-aware best threshold of distances by torch.sort (ascending): float32[n_rel], -inf = none"""
    out = torch.full((n_rel,), -math.inf, dtype=torch.float32, device=scores.device)
    for rho in range(n_rel):
        m = r == rho
        s, order = torch.sort(scores[m])
        if s.numel() == 0:
            continue
        d = torch.cumsum(2 * y[m][order].long() - 1, 0)                       # TP - FP
        end = torch.ones_like(s, dtype=torch.bool)
        end[:-1] = s[1:] != s[:-1]
        d_end, s_end = d[end], s[end]
        best = int(torch.argmax(d_end))                                       # (first maximal: torch.argmax on ties ...
        best = int(torch.nonzero(d_end == d_end[best])[0])                    #  ... is not specified: take the first)
        if int(d_end[best]) > 0:
            out[rho] = s_end[best]
    return out


def torch_scores(table, relemb, trans_m, h, r, t):
    scores = torch.empty(h.numel(), dtype=torch.float32, device=h.device)
    for rho in range(trans_m.shape[0]):
        idx = torch.nonzero(r == rho, as_tuple=True)[0]
        if idx.numel() == 0:
            continue
        q = table[h[idx]] @ trans_m[rho] + relemb[rho]
        p = table[t[idx]] @ trans_m[rho]
        scores[idx] = ((q - p) ** 2).sum(1)
    return scores


def parent_route(table, relemb, trans_m, h, r, t, y, thr):
    """scores, counts and AUC in torch on the device"""
    scores = torch_scores(table, relemb, trans_m, h, r, t)
    pos = scores <= thr[r]
    yb = y.bool()
    counts = torch.stack([(pos & yb).sum(), (pos & ~yb).sum(), (~pos & ~yb).sum(), (~pos & yb).sum()]).tolist()
    return scores, counts, float(sort_auc(-scores, y))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triples_micro.jsonl"))
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--triples", type=int, nargs="*", default=[100_000, 1_000_000, 10_000_000])
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--relations", type=int, default=16)
    a = ap.parse_args()
    dgen = torch.Generator(device=dev).manual_seed(2026)
    n, k, n_rel = a.n, a.k, a.relations
    table = torch.randn(n, k, device=dev, generator=dgen)
    relemb = torch.randn(n_rel, k, device=dev, generator=dgen) * 0.3
    trans_m = torch.randn(n_rel, k, k, device=dev, generator=dgen) / math.sqrt(k)
    transr = TripleModel(table, relemb, trans_m, "transr")
    pn = ops.rank_sqnorm(table)
    for p in a.triples:
        h = torch.randint(0, n, (p,), device=dev, generator=dgen)
        t = torch.randint(0, n, (p,), device=dev, generator=dgen)
        r = torch.randint(0, n_rel, (p,), device=dev, generator=dgen)
        y = (torch.rand(p, device=dev, generator=dgen) < 0.5).to(torch.uint8)
        # 1. the kernel
        z = torch.empty(p, dtype=torch.float32, device=dev)
        cnt = torch.zeros(5, dtype=torch.int64, device=dev)
        thr0 = 2.0 * k
        scores_only = timed(lambda: ops.triple_scores(table, h, t, pn, relemb, r, out=z), reps=5)
        both = timed(lambda: ops.triple_scores(table, h, t, pn, relemb, r, labels=y, thr=thr0, out=z, counts=cnt), reps=5)
        kernel_only = timed(lambda: ops.triple_scores(table, h, t, pn, relemb, r, reported=False, out=z), reps=5)
        gathered = p * 2 * k * 4
        emit(what="scores_kernel", triples=p, n=n, k=k, scores_only_ms=round(scores_only, 4),
             scores_and_counts_ms=round(both, 4), kernel_scores_only_ms=round(kernel_only, 4),
             gathered_gb_per_s=round(gathered / (both * 1e-3) / 1e9, 1),
             kernel_scores_gathered_gb_per_s=round(gathered / (kernel_only * 1e-3) / 1e9, 1),
             gather_at_hbm_copy_rate_ms=round(gathered / (HBM_COPY_TB_S * 1e12) * 1e3, 4),
             times_the_floor=round(both / (gathered / (HBM_COPY_TB_S * 1e12) * 1e3), 2))
        # 2. the fit kernel against torch.sort
        ops.triple_scores(table, h, t, pn, relemb, r, out=z)
        got = {}
        t_fit, t_sort = alternated(
            lambda: got.__setitem__("new", (ops.threshold_fit(z, y, r, n_rel, True), ops.threshold_fit(z, y, None, 1, True))),
            lambda: got.__setitem__("old", torch_fit(z, y, r, n_rel)), reps=5)
        same = bool(torch.equal(got["new"][0][0].view(torch.int32), got["old"].view(torch.int32)))
        emit(what="fit_kernel", triples=p, relations=n_rel, threshold_fit_ms=round(statistics.median(t_fit), 3),
             torch_sort_fit_ms=round(statistics.median(t_sort), 3),
             speedup=round(statistics.median(t_sort) / statistics.median(t_fit), 2), identical_thresholds=same)
        # 3. end to end, 'transr'
        fit = triples.fit_triple_thresholds(transr, h, r, t, y)
        t_new, t_old = alternated(
            lambda: got.__setitem__("m", triples.evaluate_triple_classification(transr, h, r, t, y, fit)),
            lambda: got.__setitem__("p", parent_route(table, relemb, trans_m, h, r, t, y, fit.thresholds)), reps=3)
        m, (old_scores, old_counts, old_auc) = got["m"], got["p"]
        new_scores = triples.score_triples(transr, h, r, t)
        differ = int(((new_scores <= fit.thresholds[r]) != (old_scores <= fit.thresholds[r])).sum())
        worst = float(((new_scores.double() - old_scores.double()).abs() / new_scores.double().abs()).max())
        distinct = int(sum(torch.unique(torch.cat((h[r == x], t[r == x]))).numel() for x in range(n_rel)))
        emit(what="end_to_end_evaluate", triples=p, n=n, k=k, relations=n_rel, distinct_rows_projected=distinct,
             rows_of_the_torch_route=2 * p, evaluate_triple_classification_ms=round(statistics.median(t_new), 2),
             torch_route_ms=round(statistics.median(t_old), 2),
             speedup=round(statistics.median(t_old) / statistics.median(t_new), 2),
             counts=[m["tp"], m["fp"], m["tn"], m["fn"], m["nan"]], torch_counts=old_counts, decisions_that_differ=differ,
             worst_relative_score_difference=worst, roc_auc=m["roc_auc"], torch_sort_auc=old_auc)
        del got["p"], old_scores, new_scores

        def old_fit():
            return torch_fit(torch_scores(table, relemb, trans_m, h, r, t), y, r, n_rel)
        t_new, t_old = alternated(lambda: triples.fit_triple_thresholds(transr, h, r, t, y), old_fit, reps=3)
        emit(what="end_to_end_fit", triples=p, fit_triple_thresholds_ms=round(statistics.median(t_new), 2),
             torch_route_ms=round(statistics.median(t_old), 2),
             speedup=round(statistics.median(t_old) / statistics.median(t_new), 2))
        del got, h, t, r, y, z
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "a" if a.append else "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
