#!/usr/bin/env python3
"""The KvsAll loss (lkg_kvsall.hip, literalkg_amd/kvs_all.py) on the GPU box: one JSON line per measurement, written to
profiles/kvs_all_micro.jsonl (--out).  One process, a warm-up per shape, device events, the two routes of a comparison
alternating.  On a random table at N = 1 M, k = 300, B in {1024, 8192}, lists of 0, 10 and 1000 positions per row:
  1. the sigmoid forward pair and the sigmoid weights kernel (over every chunk of the backward pass, with and without its
     row sums) against the MASKED softmax ones on the same operands and the same lists;
  2. forward + backward of sigmoid_all_loss against a dense torch route: chunked q @ p.T, BCE-with-logits sum, autograd
     (the targets of a chunk scattered from the same lists);
and one training step of examples/pretrain_synthetic.py's model:
  3. calc_kvs_all_loss over the distinct queries of a batch against calc_one_vs_all_loss(known=) over the batch's triples,
     list building included in both; the number of distinct queries is reported next to the number of triples."""
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
from literalkg_amd import KnownTriples, LiteralKG, distinct_queries, kvs_all, ops  # noqa: E402
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


def lists_of(b, n, per_row, truth):
    """(ptr, col): per row `per_row` ascending, distinct positions, one drawn from each of per_row equal strata of
    [0, n), never the row's truth (so that the same lists serve the masked softmax)"""
    if per_row == 0:
        return torch.zeros(b + 1, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    w = n // per_row
    pos = torch.arange(per_row, device=dev)[None, :] * w + torch.randint(0, w, (b, per_row), device=dev)
    step = torch.where((pos + 1) % w != 0, 1, -1)
    pos = torch.where(pos == truth[:, None], pos + step, pos)
    ptr = (torch.arange(b + 1, device=dev) * per_row).int()
    return ptr, pos.reshape(-1).int()


def dense_torch_step(q, p, bias, lists, per_row, scale, g, width):
    """forward + backward of the same loss in dense torch ops, chunk by chunk (nothing of size B x N alive)"""
    q_ = q.detach().requires_grad_(True)
    p_ = p.detach().requires_grad_(True)
    b_ = bias.detach().requires_grad_(True)
    b, n = q.shape[0], p.shape[0]
    cols = lists[1].long().view(b, per_row) if per_row else None
    pn = (p_ * p_).sum(1)
    bce = torch.nn.functional.binary_cross_entropy_with_logits
    for c0 in range(0, n, width):
        c1 = min(n, c0 + width)
        z = -scale * (pn[c0:c1][None, :] - 2.0 * (q_ @ p_[c0:c1].t())) + b_[:, None]
        y = torch.zeros_like(z)
        if cols is not None:
            inside = (cols >= c0) & (cols < c1)
            rows = torch.arange(b, device=dev)[:, None].expand_as(cols)[inside]
            y[rows, cols[inside] - c0] = 1.0
        (bce(z, y, reduction="none").sum(1) * g).sum().backward(retain_graph=True)
    return q_.grad, p_.grad, b_.grad


def kernel_sweep(n, kd, scale, chunk_bytes):
    p = torch.randn(n, kd, device=dev) * 0.1
    pn = ops.rank_sqnorm(p)
    for b in (1024, 8192):
        q = torch.randn(b, kd, device=dev) * 0.1
        bias = scale * (2.0 * kd * 0.01 - (q * q).sum(1))
        truth = torch.randint(0, n, (b,), device=dev)
        g = torch.full((b,), 1.0 / b, device=dev)
        width = ops.softmax_chunk_width(b, n, chunk_bytes)
        vbuf = torch.empty((b, width), device=dev)
        tiles = torch.empty(((width + 255) // 256, b), device=dev)
        for per_row in (0, 10, 1000):
            ls = lists_of(b, n, per_row, truth)
            lse, _ = ops.softmax_all_forward(q, p, pn, truth, scale, exclude=ls)

            def softmax_weights():
                for c0 in range(0, n, width):
                    c1 = min(n, c0 + width)
                    ops.softmax_all_weights(q, p, pn, truth, lse, g, scale, c0, c1, out=vbuf[:, :c1 - c0], exclude=ls)

            def sigmoid_weights(with_rows):
                def run():
                    for c0 in range(0, n, width):
                        c1 = min(n, c0 + width)
                        rs = tiles[:(c1 - c0 + 255) // 256] if with_rows else None
                        kvs_all.sigmoid_all_weights(q, p, pn, bias, g, ls, scale, 0.1, c0, c1, out=vbuf[:, :c1 - c0],
                                                    rowsum=rs)
                return run
            fm_ms, fs_ms = timed_pair(lambda: ops.softmax_all_forward(q, p, pn, truth, scale, exclude=ls),
                                      lambda: kvs_all.sigmoid_all_forward(q, p, pn, bias, ls, scale, 0.1))
            _, fs0_ms = timed_pair(lambda: ops.softmax_all_forward(q, p, pn, truth, scale, exclude=ls),
                                   lambda: kvs_all.sigmoid_all_forward(q, p, pn, bias, ls, scale, 0.0))
            wm_ms, ws_ms = timed_pair(softmax_weights, sigmoid_weights(False))
            _, wsr_ms = timed_pair(softmax_weights, sigmoid_weights(True))
            emit(what="sigmoid_kernels", n=n, k_dim=kd, b=b, positives_per_row=per_row, splits=ops.softmax_all_splits(b, n),
                 masked_softmax_forward_ms=round(fm_ms, 3), sigmoid_forward_ms=round(fs_ms, 3),
                 sigmoid_forward_eps0_ms=round(fs0_ms, 3), forward_ratio=round(fs_ms / fm_ms, 4),
                 masked_softmax_weights_ms=round(wm_ms, 3), sigmoid_weights_ms=round(ws_ms, 3),
                 sigmoid_weights_rowsum_ms=round(wsr_ms, 3), weights_ratio=round(ws_ms / wm_ms, 4),
                 weights_rowsum_ratio=round(wsr_ms / wm_ms, 4))

            def ours():
                q_, p_, b_ = (x.detach().requires_grad_(True) for x in (q, p, bias))
                kvs_all.sigmoid_all_loss(q_, p_, b_, ls, scale=scale, chunk_bytes=chunk_bytes).backward(g)
            ours_ms, torch_ms = timed_pair(ours, lambda: dense_torch_step(q, p, bias, ls, per_row, scale, g, width),
                                           reps=2, warm=1)
            emit(what="forward_backward", n=n, k_dim=kd, b=b, positives_per_row=per_row, chunk_width=width,
                 sigmoid_all_loss_ms=round(ours_ms, 2), dense_torch_ms=round(torch_ms, 2),
                 torch_over_ours=round(torch_ms / ours_ms, 3))
        del vbuf, tiles


def training_step(entities, edges, dim, groups):
    """examples/pretrain_synthetic.py's model and batch: kvs_all over the distinct queries, one_vs_all --filtered over the
    triples"""
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
    n_queries = int(distinct_queries(bh, br)[0].numel())

    def kvs():
        opt.zero_grad()
        ent, rel = distinct_queries(bh, br)
        model.calc_kvs_all_loss(ent, rel, known, margin=8.0, label_smoothing=0.1).backward()
        opt.step()

    def ova():
        opt.zero_grad()
        model.calc_one_vs_all_loss(bh, br, bp, known=known).backward()
        opt.step()
    kvs_ms, ova_ms = timed_pair(kvs, ova, reps=3, warm=1)
    emit(what="training_step", entities=entities, edges=edges, dim=dim, scoring=model.scoring, triples=int(bh.numel()),
         distinct_queries=n_queries, kvs_all_step_ms=round(kvs_ms, 2), one_vs_all_filtered_step_ms=round(ova_ms, 2),
         kvs_over_filtered=round(kvs_ms / ova_ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kvs_all_micro.jsonl"))
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=300)
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_path[0] = a.out
    kernel_sweep(a.n, a.k, 1.0, ops.SOFTMAX_CHUNK_BYTES)
    training_step(a.entities, a.edges, a.dim, a.batch_groups)


if __name__ == "__main__":
    main()
