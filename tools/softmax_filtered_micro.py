#!/usr/bin/env python3
"""The FILTERED 1-vs-all loss (the masked kernels of lkg_softmax.hip, ops.softmax_excluded, one_vs_all_loss(known=,
candidates=)) on the GPU box: one JSON line per measurement, written to profiles/softmax_filtered_micro.jsonl (--out).
One process, a warm-up per shape, device events.  On a random table at N = 1 M, k = 300, B in {1024, 8192}:
  1. the masked forward pair and the masked weights kernel (over every chunk of the backward pass) against the unmasked
     ones, alternating, with exclusion lists of 0, 10 and 1000 positions per row;
and one training step of examples/pretrain_synthetic.py's model under mode='one_vs_all':
  2. all entities, unfiltered and with known = the training triples (list building included);
  3. candidates = the batch's truths and a 10 k subset of the entities, with the same filter."""
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
from literalkg_amd import KnownTriples, LiteralKG, ops  # noqa: E402
from literalkg_amd.synth import make_batch, make_kg  # noqa: E402

dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def timed_pair(fa, fb, reps=3, warm=1):
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


def timed(fn, reps=3, warm=1):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def lists_of(b, n, per_row, truth):
    """(xptr, xcol): per row `per_row` ascending, distinct positions, one drawn from each of per_row equal strata of
    [0, n), never the row's truth"""
    if per_row == 0:
        return torch.zeros(b + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    w = n // per_row
    pos = torch.arange(per_row, device=dev)[None, :] * w + torch.randint(0, w, (b, per_row), device=dev)
    step = torch.where((pos + 1) % w != 0, 1, -1)
    pos = torch.where(pos == truth[:, None], pos + step, pos)
    xptr = (torch.arange(b + 1, device=dev) * per_row).int()
    return xptr, pos.reshape(-1).int()


def kernel_sweep(n, kd, scale, chunk_bytes):
    p = torch.randn(n, kd, device=dev) * 0.1
    pn = ops.rank_sqnorm(p)
    for b in (1024, 8192):
        q = torch.randn(b, kd, device=dev) * 0.1
        truth = torch.randint(0, n, (b,), device=dev)
        g = torch.full((b,), 1.0 / b, device=dev)
        width = ops.softmax_chunk_width(b, n, chunk_bytes)
        vbuf = torch.empty((b, width), device=dev)
        for per_row in (0, 10, 1000):
            ex = lists_of(b, n, per_row, truth)
            lse, _ = ops.softmax_all_forward(q, p, pn, truth, scale, exclude=ex)

            def weights(exclude):
                for c0 in range(0, n, width):
                    c1 = min(n, c0 + width)
                    ops.softmax_all_weights(q, p, pn, truth, lse, g, scale, c0, c1, out=vbuf[:, :c1 - c0], exclude=exclude)
            f_ms, fm_ms = timed_pair(lambda: ops.softmax_all_forward(q, p, pn, truth, scale),
                                     lambda: ops.softmax_all_forward(q, p, pn, truth, scale, exclude=ex))
            w_ms, wm_ms = timed_pair(lambda: weights(None), lambda: weights(ex))
            emit(what="masked_kernels", n=n, k_dim=kd, b=b, excluded_per_row=per_row, splits=ops.softmax_all_splits(b, n),
                 forward_ms=round(f_ms, 3), masked_forward_ms=round(fm_ms, 3), forward_ratio=round(fm_ms / f_ms, 4),
                 weights_ms=round(w_ms, 3), masked_weights_ms=round(wm_ms, 3), weights_ratio=round(wm_ms / w_ms, 4))
        del vbuf


def training_step(entities, edges, dim, groups, n_cand):
    """examples/pretrain_synthetic.py's model and batch under mode='one_vs_all': plain, filtered, and over a subset"""
    sys.path.insert(0, os.path.join(ROOT, "examples"))
    args = SimpleNamespace(use_pretrain=0, device=dev, embed_dim=dim, relation_dim=dim, scale_gat_dim=None,
                           use_residual=False, alpha=0.1, lamda=0.5, aggregation_type="gcn", n_conv_layers=1, conv_dim=dim,
                           mess_dropout=0.1, kg_l2loss_lambda=1e-5, fine_tuning_l2loss_lambda=1e-5,
                           pre_training_neg_rate=3, fine_tuning_neg_rate=3, num_lit_dim=2, txt_lit_dim=300,
                           use_num_lit=True, use_txt_lit=False, milestone_score=0.5, n_mlp_layers=2, mlp_hidden_dim=64)
    from pretrain_synthetic import initial_a_in
    torch.manual_seed(2022)
    h, t, r = make_kg(entities, edges)
    model = LiteralKG(args, entities, 16, initial_a_in(entities, h, t, r), torch.rand(entities, 2), None).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    model.train()
    bh, br, bp, _ = (torch.from_numpy(x).to(dev)[::3] for x in make_batch(entities, groups, 3, seed=1))
    known = KnownTriples(*(torch.from_numpy(x).to(dev) for x in (h, r, t)), entities, 16)
    cand = torch.unique(torch.cat((bp, torch.randperm(entities, device=dev)[:n_cand])))

    def step(**kw):
        def run():
            opt.zero_grad()
            model.calc_one_vs_all_loss(bh, br, bp, **kw).backward()
            opt.step()
        return run
    plain_ms = timed(step(), reps=3, warm=1)
    known_ms = timed(step(known=known), reps=3, warm=1)
    cand_ms = timed(step(known=known, candidates=cand), reps=5, warm=2)
    cand_only_ms = timed(step(candidates=cand), reps=5, warm=2)
    emit(what="training_step", entities=entities, edges=edges, dim=dim, scoring=model.scoring, positives=int(bh.numel()),
         relations_in_batch=int(br.unique().numel()), candidates=int(cand.numel()), one_vs_all_step_ms=round(plain_ms, 2),
         filtered_step_ms=round(known_ms, 2), filtered_over_plain=round(known_ms / plain_ms, 3),
         candidates_filtered_step_ms=round(cand_ms, 2), candidates_step_ms=round(cand_only_ms, 2),
         plain_over_candidates=round(plain_ms / cand_only_ms, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_filtered_micro.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    ap.add_argument("--candidates", type=int, default=10_000)
    a = ap.parse_args()
    kernel_sweep(a.n, a.k, 1.0, ops.SOFTMAX_CHUNK_BYTES)
    training_step(a.entities, a.edges, a.dim, a.batch_groups, a.candidates)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
