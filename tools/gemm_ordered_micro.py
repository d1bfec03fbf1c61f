#!/usr/bin/env python3
"""The ordered split-K GEMM (lkg_gemm_ordered.hip, literalkg_amd/gemm_ordered.py) on the GPU box: one JSON line per
measurement, written to profiles/gemm_ordered_micro.jsonl (--out).  One process, a warm-up per shape, device events, the
routes of a comparison alternating.
  1. the products the training losses wait for, as they launch them -- accumulating onto an initialised output -- on the
     "ordered" route (accumulate_ordered: one gemm_ordered call), on the "engine" route (ops.gemm in beta = 1 slices) and
     as ONE torch.addmm:  dQ += 2 V P of a 256 MB chunk of V at B = 1024 (1024 x 300 x 65 536; 16 chunks make N = 1 M) and
     at B = 8192 (8192 x 300 x 8192; 128 chunks), and dd += G Wcat^T at 873 x 300 x 32 768 and 873 x 300 x 76 800;
  2. forward + backward of softmax_all_loss and sigmoid_all_loss (B = 1024, N = 1 M, k = 300) and of relation_softmax_loss
     (slab and shared mode) under both routes, the dense torch head next to the first and the last;
  3. one training step of examples/pretrain_synthetic.py's model per objective under both routes.
--part products | losses | step runs one of the three alone (each with its own --out), so that the command that runs them
can give every part a time limit of its own, e.g. `timeout 150 python tools/gemm_ordered_micro.py --part products ...`."""
import argparse
import importlib
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
from literalkg_amd import KnownTriples, LiteralKG, distinct_queries, ops, product_route  # noqa: E402
from literalkg_amd.synth import make_batch, make_kg  # noqa: E402

GO = importlib.import_module("literalkg_amd.gemm_ordered")       # (literalkg_amd.gemm_ordered is the function)
kv = importlib.import_module("literalkg_amd.kvs_all")
rl = importlib.import_module("literalkg_amd.relation_loss")
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


def timed(fns, reps=5, warm=2):
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


def product(what, m, n, k, trans_b, max_chain, alpha, note):
    gen = torch.Generator(device=dev).manual_seed(m + n + k)
    a = torch.randn(m, k, device=dev, generator=gen) * 0.1
    b = torch.randn((n, k) if trans_b else (k, n), device=dev, generator=gen) * 0.1
    outs = [torch.zeros(m, n, device=dev) for _ in range(3)]

    def ordered():
        GO.accumulate_ordered(a, b, outs[0], max_chain, trans_b=trans_b, alpha=alpha)

    def engine():                                     # the slice loop of ops.all_entity_backward / relation_loss.py
        for s0 in range(0, k, max_chain):
            s1 = min(k, s0 + max_chain)
            ops.gemm(a[:, s0:s1], b[:, s0:s1] if trans_b else b[s0:s1], trans_b=trans_b, alpha=alpha, beta=1.0, out=outs[1])

    def dense():
        outs[2].addmm_(a, b.t() if trans_b else b, alpha=alpha)
    o_ms, e_ms, t_ms = timed([ordered, engine, dense])
    for o in outs:
        o.zero_()
    ordered(), engine(), dense()
    ref = alpha * (a.double() @ (b.double().t() if trans_b else b.double()))
    err = [float((o.double() - ref).abs().max() / ref.abs().max()) for o in outs]
    f = max(16, max_chain // 16 * 16)
    s_eff, per = GO.partition(k, max(1, -(-k // f)))
    emit(what=what, m=m, n=n, k=k, trans_b=trans_b, note=note, splits=s_eff, per=per, slices_on_engine_route=-(-k // max_chain),
         ordered_ms=round(o_ms, 4), engine_ms=round(e_ms, 4), torch_addmm_ms=round(t_ms, 4),
         engine_over_ordered=round(e_ms / o_ms, 3), torch_over_ordered=round(t_ms / o_ms, 3),
         max_error_over_max_entry=dict(ordered=float(f"{err[0]:.3g}"), engine=float(f"{err[1]:.3g}"), torch=float(f"{err[2]:.3g}")))


def products():
    product("dQ", 1024, 300, 65536, False, ops.SOFTMAX_DQ_SLICE, 2.0, "one 256 MB chunk of V at B = 1024; N = 1 M is 16 of them")
    product("dQ", 8192, 300, 8192, False, ops.SOFTMAX_DQ_SLICE, 2.0, "one 256 MB chunk of V at B = 8192; N = 1 M is 128 of them")
    product("dd", 873, 300, 32768, True, max(1, rl.DD_SLICE // 128) * 128, 1.0, "R = 256, D = 128")
    product("dd", 873, 300, 76800, True, max(1, rl.DD_SLICE // 300) * 300, 1.0, "R = 256, D = 300")


def both_routes(run):
    """milliseconds of run() under product_route('engine') and ('ordered'), alternating"""
    def under(name):
        def f():
            with product_route(name):
                run()
        return f
    return timed([under("engine"), under("ordered")], reps=3, warm=1)


def all_entity(b, n, k):
    gen = torch.Generator(device=dev).manual_seed(b + k)
    q = torch.randn(b, k, device=dev, generator=gen) * 0.1
    p = torch.randn(n, k, device=dev, generator=gen) * 0.1
    truth = torch.randint(0, n, (b,), device=dev, generator=gen)
    up = torch.full((b,), 1.0 / b, device=dev)

    def softmax():
        q_, p_ = q.detach().requires_grad_(True), p.detach().requires_grad_(True)
        ops.softmax_all_loss(q_, p_, truth).backward(up)

    def dense():
        q_, p_ = q.detach().requires_grad_(True), p.detach().requires_grad_(True)
        z = -(torch.cdist(q_, p_) ** 2)
        torch.nn.functional.cross_entropy(z, truth, reduction="none").backward(up)
    e_ms, o_ms = both_routes(softmax)
    (t_ms,) = timed([dense], reps=3, warm=1)
    emit(what="one_vs_all forward+backward", queries=b, candidates=n, k_dim=k, engine_ms=round(e_ms, 3), ordered_ms=round(o_ms, 3),
         dense_torch_head_ms=round(t_ms, 3), engine_over_ordered=round(e_ms / o_ms, 3), torch_over_ordered=round(t_ms / o_ms, 3))
    bias = torch.zeros(b, device=dev)
    yptr = torch.arange(b + 1, dtype=torch.int32, device=dev)
    ycol = truth.int()

    def sigmoid():
        q_, p_, b_ = (x.detach().requires_grad_(True) for x in (q, p, bias))
        kv.sigmoid_all_loss(q_, p_, b_, (yptr, ycol)).backward(up)
    e_ms, o_ms = both_routes(sigmoid)
    emit(what="kvs_all forward+backward", queries=b, candidates=n, k_dim=k, engine_ms=round(e_ms, 3), ordered_ms=round(o_ms, 3),
         engine_over_ordered=round(e_ms / o_ms, 3))


def relation(p, n_rel, k, shared):
    gen = torch.Generator(device=dev).manual_seed(p + n_rel + k)
    d = torch.randn(p, k, device=dev, generator=gen) * 0.1
    e = torch.randn(n_rel, k, device=dev, generator=gen) * 0.1
    w = None if shared else torch.randn(n_rel, k, k, device=dev, generator=gen) * (1.0 / math.sqrt(k))
    truth = torch.randint(0, n_rel, (p,), device=dev, generator=gen)
    up = torch.full((p,), 1.0 / p, device=dev)

    def ours():
        leaves = [None if x is None else x.detach().requires_grad_(True) for x in (d, w, e)]
        rl.relation_softmax_loss(*leaves, truth).backward(up)

    def dense():
        d_, e_ = d.detach().requires_grad_(True), e.detach().requires_grad_(True)
        w_ = None if w is None else w.detach().requires_grad_(True)
        u3 = d_[:, None, :] if w_ is None else torch.einsum("pc,rcd->prd", d_, w_)
        z = -((u3 + e_[None]) ** 2).sum(2)
        torch.nn.functional.cross_entropy(z, truth, reduction="none").backward(up)
    e_ms, o_ms = both_routes(ours)
    (t_ms,) = timed([dense], reps=3, warm=1)
    emit(what="relation_loss forward+backward", mode="shared" if shared else "slab", pairs=p, relations=n_rel, k_dim=k,
         engine_ms=round(e_ms, 3), ordered_ms=round(o_ms, 3), dense_torch_head_ms=round(t_ms, 3),
         engine_over_ordered=round(e_ms / o_ms, 3), torch_over_ordered=round(t_ms / o_ms, 3))


def training_step(entities, edges, dim, groups):
    """examples/pretrain_synthetic.py's model and batch, one step per objective under both routes"""
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
    bh, br, bp, _ = (torch.from_numpy(x).to(dev) for x in make_batch(entities, groups, 3, seed=1))
    bh, br, bp = bh[::3], br[::3], bp[::3]
    ent, rel = distinct_queries(bh, br)
    losses = {"one_vs_all": lambda: model.calc_one_vs_all_loss(bh, br, bp),
              "kvs_all": lambda: model.calc_kvs_all_loss(ent, rel, known, margin=8.0, label_smoothing=0.1),
              "relation": lambda: model.calc_relation_loss(bh, br, bp)}
    for name, loss in losses.items():
        def step():
            opt.zero_grad()
            loss().backward()
            opt.step()
        e_ms, o_ms = both_routes(step)
        emit(what="training_step", objective=name, entities=entities, edges=edges, dim=dim, scoring=model.scoring, groups=groups,
             engine_ms=round(e_ms, 3), ordered_ms=round(o_ms, 3), engine_over_ordered=round(e_ms / o_ms, 3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gemm_ordered_micro.jsonl"))
    ap.add_argument("--part", choices=("products", "losses", "step", "all"), default="all")
    ap.add_argument("--candidates", type=int, default=1_000_000)
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batch-groups", type=int, default=683)
    a = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    out_path[0] = a.out
    if a.part in ("products", "all"):
        products()
    if a.part in ("losses", "all"):
        all_entity(1024, a.candidates, 300)
        for p, n_rel, k, shared in ((873, 256, 128, False), (873, 256, 300, False), (8192, 256, 128, False), (8192, 256, 300, True)):
            relation(p, n_rel, k, shared)
    if a.part in ("step", "all"):
        training_step(a.entities, a.edges, a.dim, a.batch_groups)


if __name__ == "__main__":
    main()
