#!/usr/bin/env python3
"""The 1-vs-all loss (lkg_softmax.hip, ops.softmax_all_loss, literalkg_amd/one_vs_all.py) on the GPU box: one JSON line
per measurement, written to profiles/softmax_loss_micro.jsonl (--out).  One process, a warm-up per shape, device events.
On a random table at N = 1 M, k = 300, B in {1024, 8192}:
  1. the forward pair (lkg_softmax_all_partial_f32 + lkg_softmax_all_finish_f32) against the counting pair
     (lkg_rank_prepare_f32 + lkg_rank_count_f32) at the same shape;
  2. the weights kernel (lkg_softmax_all_weights_f32 over every chunk of the backward pass) against the same;
  3. the whole backward pass (weights, both products, the norm term);
  4. forward + backward against the dense torch route: chunked q @ p.T, logsumexp, autograd;
and one training step of examples/pretrain_synthetic.py's model under mode='one_vs_all' against its sampled-negative
step (mode='pre_training') on the same batch of triples."""
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
from literalkg_amd import LiteralKG, ops  # noqa: E402
from literalkg_amd.synth import make_batch, make_kg  # noqa: E402

PEAK_F32 = 157.3
dev = torch.device("cuda:0")
lines = []


def emit(**kw):
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def timed(fn, reps=3, warm=1):
    """mean milliseconds of fn between two device events, after a warm-up"""
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


def torch_dense(q, p, truth, g, scale, chunk_bytes):
    """forward + backward (upstream gradient g) of the same loss in dense torch ops: logits chunk by chunk (q @ p.T),
    logsumexp, autograd"""
    b, n = q.shape[0], p.shape[0]
    width = ops.softmax_chunk_width(b, n, chunk_bytes)

    def logits(c0, c1):
        pc = p[c0:c1]
        return -scale * ((pc * pc).sum(1)[None, :] - 2.0 * (q @ pc.t()))
    with torch.no_grad():
        lse = torch.full((b,), -float("inf"), device=q.device)
        for c0 in range(0, n, width):
            lse = torch.logaddexp(lse, torch.logsumexp(logits(c0, min(n, c0 + width)), 1))
        pt = p[truth]
        zt = -scale * ((pt * pt).sum(1) - 2.0 * (q * pt).sum(1))
    for c0 in range(0, n, width):         # d(lse) = sum_c softmax_c dz_c = d(sum_c exp(z_c - lse)) with lse held
        c1 = min(n, c0 + width)
        z = logits(c0, c1)
        inside = (truth >= c0) & (truth < c1)
        part = torch.exp(z - lse[:, None]).sum(1) - torch.where(
            inside, z.gather(1, (truth - c0).clamp(0, c1 - c0 - 1)[:, None])[:, 0], torch.zeros_like(lse))
        (part * g).sum().backward()
    return lse - zt


def kernel_sweep(n, kd, scale, chunk_bytes):
    p = torch.randn(n, kd, device=dev) * 0.1
    pn = ops.rank_sqnorm(p)
    for b in (1024, 8192):
        q = torch.randn(b, kd, device=dev) * 0.1
        truth = torch.randint(0, n, (b,), device=dev)
        g = torch.full((b,), 1.0 / b, device=dev)
        flop = 2.0 * b * n * kd
        count_ms = timed(lambda: ops.rank_count(q, p, pn, truth))
        fwd_ms = timed(lambda: ops.softmax_all_forward(q, p, pn, truth, scale))
        lse, _ = ops.softmax_all_forward(q, p, pn, truth, scale)
        width = ops.softmax_chunk_width(b, n, chunk_bytes)
        vbuf = torch.empty((b, width), device=dev)

        def weights():
            for c0 in range(0, n, width):
                c1 = min(n, c0 + width)
                ops.softmax_all_weights(q, p, pn, truth, lse, g, scale, c0, c1, out=vbuf[:, :c1 - c0])
        w_ms = timed(weights)
        del vbuf
        qg, pg = q.clone().requires_grad_(True), p.clone().requires_grad_(True)
        loss = ops.softmax_all_loss(qg, pg, truth, scale=scale, chunk_bytes=chunk_bytes)

        def backward():
            qg.grad = pg.grad = None
            loss.backward(g, retain_graph=True)
        bwd_ms = timed(backward)
        ws = min(width, ops.SOFTMAX_DQ_SLICE)
        e_q = ops.gemm_engine(torch.empty((b, ws), device=dev), p[:ws], alpha=2.0, beta=1.0,
                              out=torch.empty((b, kd), device=dev))
        e_p = ops.gemm_engine(torch.empty((b, width), device=dev), torch.empty((b, kd + 1), device=dev), trans_a=True,
                              alpha=2.0, beta=1.0, out=torch.empty((width, kd + 1), device=dev))
        del loss

        def ours():
            qg.grad = pg.grad = None
            ops.softmax_all_loss(qg, pg, truth, scale=scale, chunk_bytes=chunk_bytes).backward(g)

        def dense():
            qg.grad = pg.grad = None
            torch_dense(qg, pg, truth, g, scale, chunk_bytes)
        ours_ms = timed(ours, reps=2)
        dq, dp = qg.grad.clone(), pg.grad.clone()
        dense_ms = timed(dense, reps=2)
        emit(what="softmax_all_kernels", n=n, k_dim=kd, b=b, scale=scale, splits=ops.softmax_all_splits(b, n),
             chunk_width=width, chunks=-(-n // width), rank_count_ms=round(count_ms, 3), forward_ms=round(fwd_ms, 3),
             forward_over_count=round(fwd_ms / count_ms, 3), forward_tflops=round(flop / fwd_ms / 1e9, 1),
             forward_frac_of_f32_peak=round(flop / fwd_ms / 1e9 / PEAK_F32, 3), weights_ms=round(w_ms, 3),
             weights_over_count=round(w_ms / count_ms, 3), backward_ms=round(bwd_ms, 3), dq_engine=e_q, dp_engine=e_p,
             fwd_bwd_ms=round(ours_ms, 3), torch_dense_fwd_bwd_ms=round(dense_ms, 3),
             fwd_bwd_over_torch_dense=round(ours_ms / dense_ms, 3),
             dq_max_rel_diff_vs_dense=float((dq - qg.grad).abs().max() / qg.grad.abs().max()),
             dp_max_rel_diff_vs_dense=float((dp - pg.grad).abs().max() / pg.grad.abs().max()))
        del qg, pg, dq, dp


def training_step(entities, edges, dim, groups):
    """examples/pretrain_synthetic.py's model and batch: the sampled-negative step against the 1-vs-all step"""
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
    bh, br, bp, bn = (torch.from_numpy(x).to(dev) for x in make_batch(entities, groups, 3, seed=1))

    def sampled():
        opt.zero_grad()
        model(bh, br, bp, bn, device=dev, mode="pre_training").backward()
        opt.step()

    def one_vs_all():
        opt.zero_grad()
        model(bh[::3], br[::3], bp[::3], device=dev, mode="one_vs_all").backward()       # the batch's distinct positives
        opt.step()
    s_ms = timed(sampled, reps=5, warm=2)
    o_ms = timed(one_vs_all, reps=3, warm=1)
    emit(what="training_step", entities=entities, edges=edges, dim=dim, scoring=model.scoring, batch=int(bh.numel()),
         positives=int(bh[::3].numel()), relations_in_batch=int(br.unique().numel()), sampled_negative_step_ms=round(s_ms, 2),
         one_vs_all_step_ms=round(o_ms, 2), ratio=round(o_ms / s_ms, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "softmax_loss_micro.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    a = ap.parse_args()
    kernel_sweep(a.n, a.k, 1.0, ops.SOFTMAX_CHUNK_BYTES)
    training_step(a.entities, a.edges, a.dim, a.batch_groups)
    with open(a.out, "w") as f:
        for x in lines:
            f.write(json.dumps(x) + "\n")


if __name__ == "__main__":
    main()
