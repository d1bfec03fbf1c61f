#!/usr/bin/env python3
"""The self-adversarial negative-sampling loss (lkg_nssa.hip, literalkg_amd/self_adversarial.py) on the GPU box: one JSON
line per measurement, written to profiles/self_adversarial_micro.jsonl (--out).  One process, a warm-up per shape, device
events, the two routes of a comparison alternating.  On random rows at k = 300, G in {683, 8192}, K in {3, 64, 256}:
  1. the forward and the backward launch, with the achieved bytes/s of the G (2 + K) k 4 bytes of rows a pass reads (the
     backward also writes as many: reported as read + written);
  2. forward + backward of sampled_sigmoid_loss against a torch composite of the same op (broadcast difference, softmax,
     softplus, autograd);
and one training step of examples/pretrain_synthetic.py's model:
  3. calc_self_adversarial_loss on a grouped batch at neg-rate 3 and 64 against the sampled step (mode='pre_training') on
     the same batch at the same rate."""
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
from literalkg_amd import LiteralKG, group_sampled_batch, self_adversarial  # noqa: E402
from literalkg_amd.synth import make_batch, make_kg  # noqa: E402

dev = torch.device("cuda:0")
lines = []
out_path = [None]


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


def torch_composite(q, p, n, up, margin, scale, temperature):
    """forward + backward of the same op in torch ops: the broadcast difference, softmax, softplus, autograd"""
    q_, p_, n_ = (x.detach().requires_grad_(True) for x in (q, p, n))
    zp = scale * (margin - ((q_ - p_) ** 2).sum(1))
    zn = scale * (margin - ((q_[:, None] - n_.view(q.shape[0], -1, q.shape[1])) ** 2).sum(2))
    w = torch.softmax(temperature * zn, dim=1).detach()
    sp = torch.nn.functional.softplus
    (sp(-zp) + (w * sp(zn)).sum(1)).backward(up)
    return q_.grad, p_.grad, n_.grad


def op_sweep(k, margin, scale, temperature, inner=10):
    for g in (683, 8192):
        for kn in (3, 64, 256):
            q, p = torch.randn(g, k, device=dev) * 0.1, torch.randn(g, k, device=dev) * 0.1
            n = torch.randn(g * kn, k, device=dev) * 0.1
            up = torch.full((g,), 1.0 / g, device=dev)
            row_bytes = g * (2 + kn) * k * 4

            def forward():
                for _ in range(inner):
                    self_adversarial.sampled_sigmoid_forward(q, p, n, True, margin, scale, temperature)
            leaves = [x.detach().requires_grad_(True) for x in (q, p, n)]
            loss = self_adversarial.sampled_sigmoid_loss(*leaves, margin=margin, scale=scale, temperature=temperature)

            def backward():
                for _ in range(inner):
                    torch.autograd.grad(loss, leaves, up, retain_graph=True)
            f_ms, b_ms = (t / inner for t in timed_pair(forward, backward))
            emit(what="kernels", g=g, neg=kn, k_dim=k, row_bytes=row_bytes, forward_ms=round(f_ms, 4),
                 backward_ms=round(b_ms, 4), forward_read_TBps=round(row_bytes / f_ms / 1e9, 3),
                 backward_read_plus_written_TBps=round(2 * row_bytes / b_ms / 1e9, 3))

            def ours():
                ls = [x.detach().requires_grad_(True) for x in (q, p, n)]
                self_adversarial.sampled_sigmoid_loss(*ls, margin=margin, scale=scale, temperature=temperature).backward(up)
            ours_ms, torch_ms = timed_pair(ours, lambda: torch_composite(q, p, n, up, margin, scale, temperature))
            emit(what="forward_backward", g=g, neg=kn, k_dim=k, sampled_sigmoid_loss_ms=round(ours_ms, 4),
                 torch_composite_ms=round(torch_ms, 4), torch_over_ours=round(torch_ms / ours_ms, 3))


def training_step(entities, edges, dim, groups, margin, temperature):
    """examples/pretrain_synthetic.py's model and batch: --objective self_adversarial against the sampled step"""
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
    for rate in (3, 64):
        model.pre_training_neg_rate = rate
        bh, br, bp, bn = (torch.from_numpy(x).to(dev) for x in make_batch(entities, groups, rate, seed=1))

        def nssa():
            opt.zero_grad()
            model.calc_self_adversarial_loss(*group_sampled_batch(bh, br, bp, bn, rate), margin=margin,
                                             temperature=temperature).backward()
            opt.step()

        def sampled():
            opt.zero_grad()
            model(bh, br, bp, bn, device=dev, mode="pre_training").backward()
            opt.step()
        nssa_ms, sampled_ms = timed_pair(nssa, sampled, reps=10, warm=3)
        emit(what="training_step", entities=entities, edges=edges, dim=dim, scoring=model.scoring, groups=groups,
             neg_rate=rate, self_adversarial_step_ms=round(nssa_ms, 3), sampled_step_ms=round(sampled_ms, 3),
             self_adversarial_over_sampled=round(nssa_ms / sampled_ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "self_adversarial_micro.jsonl"))
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    ap.add_argument("--margin", type=float, default=8.0)
    ap.add_argument("--temperature", type=float, default=1.0)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_path[0] = a.out
    op_sweep(a.k, 2.0 * a.k * 0.01, 1.0, a.temperature)
    training_step(a.entities, a.edges, a.dim, a.batch_groups, a.margin, a.temperature)


if __name__ == "__main__":
    main()
