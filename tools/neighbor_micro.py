#!/usr/bin/env python3
"""Neighbour sampling (lkg_neighbors.hip, literalkg_amd/pruned.py) on the GPU box: one JSON line per measurement, written to
profiles/neighbor_micro.jsonl (--out).  One process, a warm-up, device events, the routes of a comparison alternating.
  kernel  lkg_csr_sample_rows at fanout 4, 16 and 64 next to lkg_csr_extract_rows on the same selected rows (2 k and 200 k)
          of the synthetic 1 M-entity / 10 M-triple graph, and on one planted hub row of 10^5 entries alone;
  step    one training step (forward, backward, Adam) of examples/pretrain_synthetic.py's model (200 k entities, 2 M edges,
          dim 128, 683 groups) at --layers 2 and 3 with prune_to_batch, the sampled objective and self_adversarial, at
          neighbor_fanout None (the exact pruned step, with its dense fall-back where the frontier outgrows
          prune_max_fraction) against 4, 8 and 16; the frontier size at every level beside it.
--part kernel | step runs one of the two alone (each with its own --out), so that the command that runs them can give every
part a time limit of its own."""
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
from literalkg_amd import KGStructure, LiteralKG, group_sampled_batch, ops, pruned  # noqa: E402
from literalkg_amd import _native as N  # noqa: E402
from literalkg_amd.synth import make_batch, make_kg, make_kg_device  # noqa: E402

dev = torch.device("cuda:0")
lines = []
out_path = [None]
FANOUTS = (4, 16, 64)


def emit(**kw):
    """print the line and rewrite the output file: a run cut short keeps what it measured"""
    lines.append(kw)
    print(json.dumps(kw), flush=True)
    if out_path[0]:
        with open(out_path[0], "w") as f:
            for x in lines:
                f.write(json.dumps(x) + "\n")


def timed(fns, reps=20, warm=3):
    """mean milliseconds of each of fns between device events, after a warm-up, the routes alternating"""
    for _ in range(warm):
        for f in fns:
            f()
    torch.cuda.synchronize()
    n = len(fns)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n * reps + 1)]
    ev[0].record()
    for i in range(reps):
        for j, f in enumerate(fns):
            f()
            ev[n * i + j + 1].record()
    torch.cuda.synchronize()
    return [sum(ev[n * i + j].elapsed_time(ev[n * i + j + 1]) for i in range(reps)) / reps for j in range(n)]


def kernel_case(what, rowptr, col, val, rows):
    """extract and the three fanouts on the same rows, into buffers sized once"""
    deg = (rowptr[rows + 1] - rowptr[rows]).long()
    total = int(deg.sum())
    out_col = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
    out_val = torch.empty(max(total, 1), dtype=torch.float32, device=dev)

    def scan(d):
        rp = torch.zeros(rows.numel() + 1, dtype=torch.int32, device=dev)
        rp[1:] = torch.cumsum(d, 0)
        return rp
    rp_all = scan(deg)
    rp_f = {f: scan(deg.clamp(max=f)) for f in FANOUTS}
    head = (rows.numel(), N.ptr(rows), N.ptr(rowptr), N.ptr(col), N.ptr(val))

    def extract():
        N.call("lkg_csr_extract_rows", *head, N.ptr(rp_all), N.ptr(out_col), N.ptr(out_val), ops._stream())

    def sample(f):
        return lambda: N.call("lkg_csr_sample_rows", *head, f, 2022, 0, 1, N.ptr(rp_f[f]), N.ptr(out_col), N.ptr(out_val),
                              ops._stream())
    ms = timed([extract] + [sample(f) for f in FANOUTS])
    emit(what=what, rows=rows.numel(), entries=total, longest_row=int(deg.max()), extract_ms=round(ms[0], 4),
         **{f"sample_f{f}_ms": round(x, 4) for f, x in zip(FANOUTS, ms[1:])},
         **{f"kept_f{f}": int(rp_f[f][-1]) for f in FANOUTS},
         **{f"rows_longer_than_{f}": int((deg > f).sum()) for f in FANOUTS},
         **{f"sample_f{f}_over_extract": round(x / ms[0], 3) for f, x in zip(FANOUTS, ms[1:])})


def kernel(entities, edges, hub):
    h, t, r = make_kg_device(entities, edges, "zipf", 2022, dev)
    g = KGStructure.from_triples(entities, h, t, r, device=dev, with_transpose=False)
    val = torch.rand(g.nnz, device=dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    for n_sel in (2_000, 200_000):
        rows = torch.sort(torch.randperm(entities, generator=gen, device=dev)[:n_sel]).values
        kernel_case(f"{n_sel} rows of the {entities}-entity / {edges}-triple graph", g.rowptr, g.col, val, rows)
    rowptr = torch.tensor([0, hub], dtype=torch.int32, device=dev)
    col = torch.arange(hub, dtype=torch.int32, device=dev)
    kernel_case(f"one hub row of {hub} entries", rowptr, col, torch.rand(hub, device=dev), torch.zeros(1, dtype=torch.int64, device=dev))


def level_sizes(model, ids, fanout):
    att = model._attention()
    sub = pruned.build_batch_subgraph(att.graph, att.val, ids, model.n_layers, fanout=fanout, seed=model.neighbor_seed, draw=0)
    return [int(x.numel()) for x in reversed(sub.rows)], [int(sub.layers[k].col.numel()) for k in range(model.n_layers, 0, -1)]


def training_step(entities, edges, dim, groups, layers, reps):
    """examples/pretrain_synthetic.py's model and batch; the configurations share one model and alternate"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    args = SimpleNamespace(use_pretrain=0, device=dev, embed_dim=dim, relation_dim=dim, scale_gat_dim=None,
                           use_residual=False, alpha=0.1, lamda=0.5, aggregation_type="gcn", n_conv_layers=layers, conv_dim=dim,
                           mess_dropout=0.1, kg_l2loss_lambda=1e-5, fine_tuning_l2loss_lambda=1e-5,
                           pre_training_neg_rate=3, fine_tuning_neg_rate=3, num_lit_dim=2, txt_lit_dim=300,
                           use_num_lit=True, use_txt_lit=False, milestone_score=0.5, n_mlp_layers=2, mlp_hidden_dim=64)
    from pretrain_synthetic import initial_a_in
    torch.manual_seed(2022)
    h, t, r = make_kg(entities, edges)
    model = LiteralKG(args, entities, 16, initial_a_in(entities, h, t, r), torch.rand(entities, 2), None).to(dev)
    model.prune_to_batch = True
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    model.train()
    bh, br, bp, bn = (torch.from_numpy(x).to(dev) for x in make_batch(entities, groups, 3, seed=1))
    grouped = group_sampled_batch(bh, br, bp, bn, 3)
    objectives = {"sampled": lambda: model(bh, br, bp, bn, device=dev, mode="pre_training"),
                  "self_adversarial": lambda: model.calc_self_adversarial_loss(*grouped, margin=8.0)}
    ids = torch.cat([bh, bp, bn])
    configs = (None, 4, 8, 16)
    sizes = {f: level_sizes(model, ids, f) for f in configs}
    for name, loss in objectives.items():
        skip = {f: 0 for f in configs}             # the dense back-off of one configuration must not leak into the next
        sampled = {f: [] for f in configs}

        def step(f):
            def run():
                model.neighbor_fanout, model._prune_skip = f, skip[f]
                opt.zero_grad()
                loss().backward()
                opt.step()
                sampled[f].append(model.gat_rows is not None)
                skip[f] = model.__dict__.get("_prune_skip", 0)
            return run
        ms = timed([step(f) for f in configs], reps=reps, warm=2)
        for f, x in zip(configs, ms):
            emit(what="training_step", objective=name, layers=layers, entities=entities, edges=edges, dim=dim, groups=groups,
                 neighbor_fanout=f, ms_per_step=round(x, 3), over_exact_pruned_step=round(x / ms[0], 3),
                 steps_on_the_pruned_path=sum(sampled[f]), steps=len(sampled[f]),
                 frontier_rows_top_to_input=sizes[f][0], entries_top_to_input=sizes[f][1],
                 prune_max_rows=int(model.prune_max_fraction * entities))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "neighbor_micro.jsonl"))
    ap.add_argument("--part", choices=("kernel", "step", "all"), default="all")
    ap.add_argument("--kernel-entities", type=int, default=1_000_000)
    ap.add_argument("--kernel-edges", type=int, default=10_000_000)
    ap.add_argument("--hub", type=int, default=100_000)
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_path[0] = a.out
    if a.part in ("kernel", "all"):
        kernel(a.kernel_entities, a.kernel_edges, a.hub)
    if a.part in ("step", "all"):
        for layers in (2, 3):
            training_step(a.entities, a.edges, a.dim, a.batch_groups, layers, a.reps)


if __name__ == "__main__":
    main()
