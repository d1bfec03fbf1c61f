#!/usr/bin/env python3
"""The relation-slot loss (lkg_relation_loss.hip, literalkg_amd/relation_loss.py) on the GPU box: one JSON line per
measurement, written to profiles/relation_loss_micro.jsonl (--out).  One process, a warm-up per shape, device events, the
two routes of a comparison alternating.  On random rows at P in {683, 8192}, R in {16, 256}, C = D in {128, 300}, slab
mode ('transr') and shared mode ('transe'), 0 and 4 known relations per pair:
  1. the forward and the backward launch alone, with the achieved bytes/s over the P R D 4 bytes of the slab a pass reads
     (the slab-mode backward writes as many again: reported as read + written; shared mode has no slab: its R D 4 bytes of
     e per pair come from the caches, and the same P R D 4 is reported as the bytes it walks);
  2. forward + backward of relation_softmax_loss against the route there was, the dense torch head (einsum, squared norm,
     masked cross_entropy, autograd), and the two routes' gradient agreement (max |a - b| / max |b| per gradient);
and one training step of examples/pretrain_synthetic.py's model:
  3. calc_relation_loss on one triple per group against the sampled step (mode='pre_training') on the same batch."""
import argparse
import json
import math
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

ge.build()
import importlib  # noqa: E402

from literalkg_amd import KnownTriples, LiteralKG, ops  # noqa: E402
from literalkg_amd.synth import make_batch, make_kg  # noqa: E402

rl = importlib.import_module("literalkg_amd.relation_loss")      # (literalkg_amd.relation_loss is the function)
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


def dense_head(d, w, e, truth, mask, scale, up):
    """forward + backward of the same loss in torch ops; (dd, dw or None, de)"""
    d_, e_ = d.detach().requires_grad_(True), e.detach().requires_grad_(True)
    w_ = None if w is None else w.detach().requires_grad_(True)
    u3 = d_[:, None, :] if w_ is None else torch.einsum("pc,rcd->prd", d_, w_)
    z = -scale * ((u3 + e_[None]) ** 2).sum(2)
    if mask is not None:
        z = z.masked_fill(mask, -math.inf)
    torch.nn.functional.cross_entropy(z, truth, reduction="none").backward(up)
    return d_.grad, None if w_ is None else w_.grad, e_.grad


def known_filter(p, n_rel, truth, n_known):
    """(filt, filter_row, filter_col, mask): pair i is (2 i, 2 i + 1), known under truth + 1 .. truth + n_known"""
    if not n_known:
        return None, None, None, None
    h = torch.arange(p, device=dev) * 2
    rel = (truth[:, None] + torch.arange(1, n_known + 1, device=dev)[None]) % n_rel
    filt = ops.csr_build_device(2 * p, h.repeat_interleave(n_known), (h + 1).repeat_interleave(n_known), rel.reshape(-1))
    mask = torch.zeros((p, n_rel), dtype=torch.bool, device=dev)
    mask.scatter_(1, rel, True)
    mask[torch.arange(p, device=dev), truth] = False
    return filt, h, h + 1, mask


def op_sweep(scale, inner):
    for p in (683, 8192):
        for n_rel in (16, 256):
            for k in (128, 300):
                for shared in (False, True):
                    for n_known in (0, 4):
                        one_shape(p, n_rel, k, shared, n_known, scale, inner)


def one_shape(p, n_rel, k, shared, n_known, scale, inner):
    gen = torch.Generator(device=dev).manual_seed(p + n_rel + k)
    d = torch.randn(p, k, device=dev, generator=gen) * 0.1
    e = torch.randn(n_rel, k, device=dev, generator=gen) * 0.1
    w = None if shared else torch.randn(n_rel, k, k, device=dev, generator=gen) * (1.0 / math.sqrt(k))
    truth = torch.randint(0, n_rel, (p,), device=dev, generator=gen)
    up = torch.full((p,), 1.0 / p, device=dev)
    filt, frow, fcol, mask = known_filter(p, n_rel, truth, n_known)
    mode = "shared" if shared else "slab"
    slab_bytes = p * n_rel * k * 4
    u, rs = (d, 0) if shared else (ops.gemm(d, rl._wcat(w)), k)
    _, z, _ = rl.relation_softmax_forward(u, rs, e, truth, scale, filt, frow, fcol)

    def forward():
        for _ in range(inner):
            rl.relation_softmax_forward(u, rs, e, truth, scale, filt, frow, fcol, z=z)

    def backward():                            # (slab mode rewrites u in place: the next launch reads what this one wrote)
        for _ in range(inner):
            rl.relation_softmax_backward(u, rs, e, truth, scale, up, z)
    f_ms, b_ms = (t / inner for t in timed_pair(forward, backward))
    moved = slab_bytes if shared else 2 * slab_bytes
    emit(what="kernels", mode=mode, pairs=p, relations=n_rel, k_dim=k, known_per_pair=n_known, slab_bytes=slab_bytes,
         forward_ms=round(f_ms, 4), backward_ms=round(b_ms, 4), forward_TBps=round(slab_bytes / f_ms / 1e9, 3),
         backward_TBps=round(moved / b_ms / 1e9, 3), backward_bytes="read" if shared else "read + written")
    del u

    def ours():
        leaves = [None if x is None else x.detach().requires_grad_(True) for x in (d, w, e)]
        rl.relation_softmax_loss(*leaves, truth, scale, filt, frow, fcol).backward(up)
        return [None if x is None else x.grad for x in leaves]
    ours_ms, torch_ms = timed_pair(ours, lambda: dense_head(d, w, e, truth, mask, scale, up))
    agree = {}
    for name, a, b in zip(("dd", "dw", "de"), ours(), dense_head(d, w, e, truth, mask, scale, up)):
        if a is not None:
            agree[name] = float((a - b).abs().max() / b.abs().max())
    emit(what="forward_backward", mode=mode, pairs=p, relations=n_rel, k_dim=k, known_per_pair=n_known,
         relation_softmax_loss_ms=round(ours_ms, 4), dense_torch_head_ms=round(torch_ms, 4),
         torch_over_ours=round(torch_ms / ours_ms, 3), gradient_agreement={k_: float(f"{v:.3g}") for k_, v in agree.items()})


def training_step(entities, edges, dim, groups):
    """examples/pretrain_synthetic.py's model and batch: --objective relation against the sampled step"""
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
    known = KnownTriples(*(torch.from_numpy(x).to(dev) for x in (h, r, t)), entities, 16)
    opt = torch.optim.Adam(model.parameters(), lr=1e-4)
    model.train()
    bh, br, bp, bn = (torch.from_numpy(x).to(dev) for x in make_batch(entities, groups, 3, seed=1))
    for filtered in (False, True):
        def relation():
            opt.zero_grad()
            model.calc_relation_loss(bh[::3], br[::3], bp[::3], known=known if filtered else None).backward()
            opt.step()

        def sampled():
            opt.zero_grad()
            model(bh, br, bp, bn, device=dev, mode="pre_training").backward()
            opt.step()
        rel_ms, sampled_ms = timed_pair(relation, sampled, reps=10, warm=3)
        emit(what="training_step", entities=entities, edges=edges, dim=dim, scoring=model.scoring, groups=groups,
             filtered=filtered, relation_step_ms=round(rel_ms, 3), sampled_step_ms=round(sampled_ms, 3),
             relation_over_sampled=round(rel_ms / sampled_ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relation_loss_micro.jsonl"))
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed interval of the kernels alone")
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_path[0] = a.out
    op_sweep(a.scale, a.inner)
    training_step(a.entities, a.edges, a.dim, a.batch_groups)


if __name__ == "__main__":
    main()
