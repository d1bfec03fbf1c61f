#!/usr/bin/env python3
"""The negative sampler (lkg_negatives.hip, literalkg_amd/negatives.py) on the GPU box: one JSON line per measurement,
written to profiles/negatives_micro.jsonl (--out).  One process, a warm-up per shape, device events, the two routes of a
comparison alternating.  On the synthetic graph of --entities / --edges (default 1 M / 10 M, 16 relations):
  1. NegativeSampler.sample at G in {683, 8192}, K in {3, 64, 256} -- unfiltered, filtered, Bernoulli (filtered) -- against
     KGBatchSampler.sample at the same group count and rate (tail-only, rejects against the head's own row, sequential in K)
     and, for the unfiltered draw, against torch.randint.  A call includes its host read (n_unfiltered and the id check);
  2. relation_cardinalities and answer_counts over all the triples against a torch.unique route that gives the same
     integers (the run stops if they differ);
and on examples/pretrain_synthetic.py's model (--step-entities / --step-edges, default 200 k / 2 M):
  3. one --objective self_adversarial training step with the new sampler (tail unfiltered; tail filtered; Bernoulli filtered
     with subsampling weights) against the same step with the batch of the old route (synth.make_batch on the host, copied
     over, group_sampled_batch), at neg-rate 3 and 64; and the loss step alone on a mixed-side batch against the same
     positives corrupted on the tail only -- what scoring the two sides of a mixed batch separately costs (one table, two
     gathers, for 'transr' the per-relation products twice)."""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import (KGStructure, KnownTriples, LiteralKG, NegativeSampler, answer_counts,  # noqa: E402
                           group_sampled_batch, relation_cardinalities, subsampling_weights)
from literalkg_amd.sampler import KGBatchSampler  # noqa: E402
from literalkg_amd.synth import make_batch, make_kg  # noqa: E402

dev = torch.device("cuda:0")
lines = []
out_path = [None]
N_REL = 16


def emit(**kw):
    """print the line and rewrite the output file: a run cut short keeps what it measured"""
    lines.append(kw)
    print(json.dumps(kw), flush=True)
    if out_path[0]:
        with open(out_path[0], "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


def timed_pair(fa, fb, reps=5, warm=2):
    """mean milliseconds of fa and of fb between device events, after a warm-up, the two alternating"""
    for _ in range(warm):
        fa()
        fb()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps + 1)]
    ev[0].record()
    for i in range(reps):
        fa()
        ev[2 * i + 1].record()
        fb()
        ev[2 * i + 2].record()
    torch.cuda.synchronize()
    ta = sum(ev[2 * i].elapsed_time(ev[2 * i + 1]) for i in range(reps)) / reps
    tb = sum(ev[2 * i + 1].elapsed_time(ev[2 * i + 2]) for i in range(reps)) / reps
    return ta, tb


def draw_sweep(n, h, r, t, known, graph, inner=5):
    order = torch.randperm(h.numel(), generator=torch.Generator().manual_seed(1)).to(dev)
    routes = {"unfiltered": NegativeSampler(n), "filtered": NegativeSampler(n, known),
              "bernoulli": NegativeSampler(n, known, corrupt="bernoulli")}
    for g in (683, 8192):
        at = order[:g]
        ph, pr, pt = h[at].contiguous(), r[at].contiguous(), t[at].contiguous()
        for k in (3, 64, 256):
            old = KGBatchSampler(graph, k)
            for name, sampler in routes.items():
                stats = sampler.sample(ph, pr, pt, k, seed=1)

                def new():
                    for i in range(inner):
                        sampler.sample(ph, pr, pt, k, seed=i)

                def kg_batch():
                    for i in range(inner):
                        old.sample(g * k, seed=i)
                new_ms, old_ms = (x / inner for x in timed_pair(new, kg_batch))
                line = dict(what="draw", route=name, g=g, k=k, sample_ms=round(new_ms, 4),
                            kg_batch_sampler_ms=round(old_ms, 4), kg_batch_sampler_over_new=round(old_ms / new_ms, 3),
                            n_unfiltered=stats.n_unfiltered, head_side_groups=int(stats.head_side.sum()))
                if name == "unfiltered":
                    def randint():
                        for i in range(inner):
                            torch.randint(n, (g, k), device=dev)
                    new_ms2, rand_ms = (x / inner for x in timed_pair(new, randint))
                    line.update(torch_randint_ms=round(rand_ms, 4), sample_ms_beside_randint=round(new_ms2, 4))
                emit(**line)


def torch_unique_counts(n, h, r, t):
    """(T_r, H_r, Tl_r, n_tails, n_heads) of all the triples by torch.unique: the integers of the two kernels"""
    triples = torch.unique((r * n + h) * n + t)                 # sorted: by (r, h), then t
    rh = triples // n
    card = [torch.bincount(rh // n, minlength=N_REL)]
    rh_u, tails_of = torch.unique_consecutive(rh, return_counts=True)
    card.append(torch.bincount(rh_u // n, minlength=N_REL))
    by_tail = torch.unique((r * n + t) * n + h)
    rt_u, heads_of = torch.unique_consecutive(by_tail // n, return_counts=True)
    card.append(torch.bincount(rt_u // n, minlength=N_REL))
    n_tails = tails_of[torch.searchsorted(rh_u, r * n + h)]
    n_heads = heads_of[torch.searchsorted(rt_u, r * n + t)]
    return card + [n_tails, n_heads]


def statistics(n, h, r, t, known):
    want = torch_unique_counts(n, h, r, t)
    card = relation_cardinalities(known)
    got = [card.triples, card.heads, card.tails, *answer_counts(known, h, r, t)]
    same = all(torch.equal(a, b) for a, b in zip(got, want))
    emit(what="statistics_agree", triples=h.numel(), same_integers=same)
    if not same:
        sys.exit("the kernels and the torch.unique route give different integers")
    card_ms, _ = timed_pair(lambda: relation_cardinalities(known), lambda: None)
    ans_ms, _ = timed_pair(lambda: answer_counts(known, h, r, t), lambda: None)
    both_ms, uniq_ms = timed_pair(lambda: (relation_cardinalities(known), answer_counts(known, h, r, t)),
                                  lambda: torch_unique_counts(n, h, r, t), reps=3, warm=1)
    emit(what="statistics", triples=h.numel(), relation_cardinalities_ms=round(card_ms, 3), answer_counts_ms=round(ans_ms, 3),
         both_ms=round(both_ms, 3), torch_unique_route_ms=round(uniq_ms, 3), torch_over_ours=round(uniq_ms / both_ms, 2))


def training_step(entities, edges, dim, groups, margin, temperature):
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    args = SimpleNamespace(use_pretrain=0, device=dev, embed_dim=dim, relation_dim=dim, scale_gat_dim=None,
                           use_residual=False, alpha=0.1, lamda=0.5, aggregation_type="gcn", n_conv_layers=1, conv_dim=dim,
                           mess_dropout=0.1, kg_l2loss_lambda=1e-5, fine_tuning_l2loss_lambda=1e-5,
                           pre_training_neg_rate=3, fine_tuning_neg_rate=3, num_lit_dim=2, txt_lit_dim=300,
                           use_num_lit=True, use_txt_lit=False, milestone_score=0.5, n_mlp_layers=2, mlp_hidden_dim=64)
    from pretrain_synthetic import initial_a_in
    torch.manual_seed(2022)
    h, t, r = make_kg(entities, edges)
    model = LiteralKG(args, entities, N_REL, initial_a_in(entities, h, t, r), torch.rand(entities, 2), None).to(dev)
    h, r, t = (torch.from_numpy(x).to(dev) for x in (h, r, t))
    known = KnownTriples(h, r, t, entities, N_REL)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    model.train()
    at = torch.randperm(h.numel(), generator=torch.Generator().manual_seed(2))[:groups].to(dev)
    ph, pr, pt = h[at].contiguous(), r[at].contiguous(), t[at].contiguous()
    kw = dict(margin=margin, temperature=temperature)
    for rate in (3, 64):
        def old_route():
            opt.zero_grad()
            bh, br, bp, bn = (torch.from_numpy(x).to(dev) for x in make_batch(entities, groups, rate, seed=1))
            model.calc_self_adversarial_loss(*group_sampled_batch(bh, br, bp, bn, rate), **kw).backward()
            opt.step()
        for name, sampler, weighted in (("tail_unfiltered", NegativeSampler(entities), False),
                                        ("tail_filtered", NegativeSampler(entities, known), False),
                                        ("bernoulli_filtered_subsampling", NegativeSampler(entities, known, corrupt="bernoulli"),
                                         True)):
            def new_route():
                opt.zero_grad()
                batch = sampler.sample(ph, pr, pt, rate, seed=1)
                w = subsampling_weights(known, ph, pr, pt) if weighted else None
                model.calc_sampled_negative_loss(ph, pr, pt, batch, weights=w, **kw).backward()
                opt.step()
            new_ms, old_ms = timed_pair(new_route, old_route, reps=10, warm=3)
            emit(what="training_step", route=name, entities=entities, edges=edges, dim=dim, scoring=model.scoring,
                 groups=groups, neg_rate=rate, new_sampler_step_ms=round(new_ms, 3), old_sampler_step_ms=round(old_ms, 3),
                 new_over_old=round(new_ms / old_ms, 3))
        tail = NegativeSampler(entities, known).sample(ph, pr, pt, rate, seed=1)
        mixed = NegativeSampler(entities, known, corrupt="both").sample(ph, pr, pt, rate, seed=1)

        def loss_step(batch):
            def step():
                opt.zero_grad()
                model.calc_sampled_negative_loss(ph, pr, pt, batch, **kw).backward()
                opt.step()
            return step
        mixed_ms, tail_ms = timed_pair(loss_step(mixed), loss_step(tail), reps=10, warm=3)
        emit(what="mixed_side_step", scoring=model.scoring, groups=groups, neg_rate=rate,
             head_side_groups=int(mixed.head_side.sum()), mixed_step_ms=round(mixed_ms, 3), tail_only_step_ms=round(tail_ms, 3),
             mixed_over_tail_only=round(mixed_ms / tail_ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "negatives_micro.jsonl"))
    ap.add_argument("--entities", type=int, default=1_000_000)
    ap.add_argument("--edges", type=int, default=10_000_000)
    ap.add_argument("--step-entities", type=int, default=200_000)
    ap.add_argument("--step-edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    ap.add_argument("--margin", type=float, default=8.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_path[0] = a.out
    hn, tn, rn = make_kg(a.entities, a.edges)
    h, r, t = (torch.from_numpy(x).to(dev) for x in (hn, rn, tn))
    known = KnownTriples(h, r, t, a.entities, N_REL)
    graph = KGStructure.from_triples(a.entities, hn, tn, rn, device=dev)
    draw_sweep(a.entities, h, r, t, known, graph)
    statistics(a.entities, h, r, t, known)
    del known, graph
    training_step(a.step_entities, a.step_edges, a.dim, a.batch_groups, a.margin, a.temperature)


if __name__ == "__main__":
    main()
