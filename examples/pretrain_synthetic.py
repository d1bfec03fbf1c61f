#!/usr/bin/env python3
"""A driver shaped like the reference's pre_training_train (main_pretraining.py:67-167) that calls the
MI355X module through the SAME surface: ctor, model.to(device), Adam over model.parameters(),
model(h, r, pos_t, neg_t, device=, mode='pre_training'), NaN check, loss.backward(), optimizer.step(),
model(h_list, t_list, r_list, relations, device=, mode='update_att') once per epoch, state_dict checkpoint.
Only the data source differs (synthetic KG instead of the reference's DataLoader, which is out of scope).

    python examples/pretrain_synthetic.py --entities 200000 --edges 2000000 --dim 128 --epochs 2 --iters 20
"""
import argparse
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as ge  # noqa: E402

ge.build()
from literalkg_amd import LiteralKG                      # noqa: E402  (the one-line change vs `from model import LiteralKG`)
from literalkg_amd import KnownTriples, distinct_queries   # noqa: E402  (--filtered, --objective kvs_all)
from literalkg_amd import product_route                  # noqa: E402  (--ordered-products)
from literalkg_amd import group_sampled_batch            # noqa: E402  (--objective self_adversarial)
from literalkg_amd import NegativeSampler, TripleEpoch, subsampling_weights   # noqa: E402  (--sampler triples, --eval-sampled)
from literalkg_amd.synth import make_batch, make_kg      # noqa: E402


def initial_a_in(n, h, t, r):
    """Random-walk Laplacian summed over relations, as the reference's loader builds it
    (dataloader.py:449-495): value 1/outdeg_r(h) per (h, r, t), summed over relations per (h, t)."""
    key = h * (int(r.max()) + 1) + r
    _, inv, cnt = np.unique(key, return_inverse=True, return_counts=True)
    w = 1.0 / cnt[inv]
    idx = torch.from_numpy(np.stack([h, t]))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(w.astype(np.float32)), (n, n)).coalesce()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entities", type=int, default=200_000)
    ap.add_argument("--edges", type=int, default=2_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--layers", type=int, default=1)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batch-groups", type=int, default=683)
    ap.add_argument("--lr", type=float, default=1e-4)
    ap.add_argument("--objective", choices=("sampled", "one_vs_all", "kvs_all", "self_adversarial", "relation"),
                    default="sampled",
                    help="sampled: the reference's loss over pre_training_neg_rate sampled negatives (mode='pre_training'); "
                         "one_vs_all: cross-entropy of the true tail against the softmax over every entity "
                         "(mode='one_vs_all'; the sampled negatives of the batch are not used); "
                         "kvs_all: one row per DISTINCT query (h, r, ?) of the batch against every entity, binary "
                         "cross-entropy against all its known tails among the training triples (calc_kvs_all_loss); "
                         "self_adversarial: each positive against its --neg-rate sampled negatives, weighted by the model's "
                         "own softmax over the group at --temperature (calc_self_adversarial_loss); "
                         "relation: cross-entropy of the true relation of (h, ?, t) against the softmax over every relation "
                         "(calc_relation_loss; one triple per group, the sampled negatives are not used)")
    ap.add_argument("--neg-rate", type=int, default=3, help="sampled negatives per positive (the reference's "
                                                            "pre_training_neg_rate)")
    ap.add_argument("--temperature", type=float, default=1.0,
                    help="with --objective self_adversarial: the weights are softmax(temperature * logits); 0: uniform")
    ap.add_argument("--label-smoothing", type=float, default=0.1, help="with --objective kvs_all")
    ap.add_argument("--margin", type=float, default=8.0,
                    help="with --objective kvs_all or self_adversarial: the logits are margin - ||q - p||^2")
    ap.add_argument("--filtered", action="store_true",
                    help="with --objective one_vs_all: the other known tails of (h, r, ?) among the training triples leave "
                         "the row's softmax (calc_one_vs_all_loss(known=...)), as filtered MRR drops them; with --objective "
                         "relation: the other known relations of (h, ?, t) do (calc_relation_loss(known=...))")
    ap.add_argument("--sampler", choices=("batch", "triples"), default="batch",
                    help="batch: the synthetic generate_kg_batch stand-in (tail negatives, made on the host); triples: with "
                         "--objective self_adversarial, an epoch over the shuffled training triples (TripleEpoch) with the "
                         "negatives drawn on the device (NegativeSampler, calc_sampled_negative_loss)")
    ap.add_argument("--corrupt", choices=("tail", "head", "both", "bernoulli"), default="tail",
                    help="with --sampler triples: the side the negatives replace")
    ap.add_argument("--filter-negatives", action="store_true",
                    help="with --sampler triples: reject a negative that forms a training triple")
    ap.add_argument("--subsampling", action="store_true",
                    help="with --sampler triples: weight every triple by 1 / sqrt(4 + its known tails + its known heads)")
    ap.add_argument("--ordered-products", action="store_true",
                    help="with --objective one_vs_all, kvs_all or relation: the backward's long reductions run on the ordered "
                         "split-K GEMM (literalkg_amd.product_route('ordered')); the other objectives have none")
    ap.add_argument("--prune-to-batch", action="store_true",
                    help="evaluate every layer on the batch's frontier only (model.prune_to_batch; the objectives that read a "
                         "few thousand rows: sampled, self_adversarial, relation)")
    ap.add_argument("--fanout", type=int, default=None,
                    help="with --prune-to-batch: a row aggregates at most this many of its stored neighbours per training "
                         "step, drawn anew every step (model.neighbor_fanout)")
    ap.add_argument("--neighbor-seed", type=int, default=0, help="with --fanout: the seed of the neighbour draws")
    ap.add_argument("--eval-sampled", type=int, default=0, metavar="K",
                    help="after training, rank a held-out slice of the triples against K filtered negatives per side, "
                         "drawn under a fixed seed (evaluate_list_ranking: the protocol of ogbl-wikikg2 / ogbl-biokg)")
    a = ap.parse_args()
    if a.fanout is not None and not a.prune_to_batch:
        ap.error("--fanout goes with --prune-to-batch")
    if a.filtered and a.objective not in ("one_vs_all", "relation"):
        ap.error("--filtered goes with --objective one_vs_all or relation")
    if a.sampler == "triples" and a.objective != "self_adversarial":
        ap.error("--sampler triples goes with --objective self_adversarial")
    if a.sampler != "triples" and (a.corrupt != "tail" or a.filter_negatives or a.subsampling):
        ap.error("--corrupt, --filter-negatives and --subsampling go with --sampler triples")
    device = torch.device("cuda:0")
    args = SimpleNamespace(use_pretrain=0, device=device, embed_dim=a.dim, relation_dim=a.dim, scale_gat_dim=None,
                           use_residual=False, alpha=0.1, lamda=0.5, aggregation_type="gcn", n_conv_layers=a.layers,
                           conv_dim=a.dim, mess_dropout=0.1, kg_l2loss_lambda=1e-5, fine_tuning_l2loss_lambda=1e-5,
                           pre_training_neg_rate=a.neg_rate, fine_tuning_neg_rate=3, num_lit_dim=2, txt_lit_dim=300,
                           use_num_lit=True, use_txt_lit=False, milestone_score=0.5, n_mlp_layers=2,
                           mlp_hidden_dim=64)
    torch.manual_seed(2022)
    h, t, r = make_kg(a.entities, a.edges)
    num = torch.rand(a.entities, 2)
    model = LiteralKG(args, a.entities, 16, initial_a_in(a.entities, h, t, r), num, None)
    model.prune_to_batch = a.prune_to_batch
    model.neighbor_fanout, model.neighbor_seed = a.fanout, a.neighbor_seed
    optimizer = torch.optim.Adam(model.parameters(), lr=a.lr)
    model.to(device)
    h_list, t_list, r_list = (torch.from_numpy(x).to(device) for x in (h, t, r))
    relations = list(range(16))
    need_known = a.filtered or a.objective == "kvs_all" or a.filter_negatives or a.subsampling or a.corrupt == "bernoulli"
    known = KnownTriples(h_list, r_list, t_list, a.entities, 16) if need_known else None
    sampler = None
    if a.sampler == "triples":
        sampler = NegativeSampler(a.entities, known, corrupt=a.corrupt, filtered=a.filter_negatives)
    for epoch in range(1, a.epochs + 1):
        model.train()
        t0, total = time.time(), 0.0
        batches = iter(TripleEpoch(h_list, r_list, t_list, a.batch_groups, seed=epoch)) if sampler is not None else None
        for it in range(a.iters):
            k = a.neg_rate
            if sampler is not None:
                bh, br, bp, offset = next(batches)
                batch = sampler.sample(bh, br, bp, k, seed=epoch, group_offset=offset)
                weights = subsampling_weights(known, bh, br, bp) if a.subsampling else None
            else:
                bh, br, bp, bn = (torch.from_numpy(x).to(device)
                                  for x in make_batch(a.entities, a.batch_groups, a.neg_rate, seed=epoch * 10_000 + it))
            optimizer.zero_grad()
            with product_route("ordered" if a.ordered_products else "engine"):     # read by the loss in its forward
                if sampler is not None:
                    loss = model.calc_sampled_negative_loss(bh, br, bp, batch, weights=weights, margin=a.margin,
                                                            temperature=a.temperature)
                elif a.objective == "self_adversarial":
                    loss = model.calc_self_adversarial_loss(*group_sampled_batch(bh, br, bp, bn, k), margin=a.margin,
                                                            temperature=a.temperature)
                elif a.objective == "kvs_all":
                    ent, rel = distinct_queries(bh[::k], br[::k])
                    loss = model.calc_kvs_all_loss(ent, rel, known, margin=a.margin, label_smoothing=a.label_smoothing)
                elif a.objective == "relation":
                    loss = model.calc_relation_loss(bh[::k], br[::k], bp[::k], known=known)    # (known is None without --filtered)
                elif a.filtered:
                    loss = model.calc_one_vs_all_loss(bh[::k], br[::k], bp[::k], known=known)
                elif a.objective == "one_vs_all":
                    loss = model(bh[::k], br[::k], bp[::k], device=device, mode="one_vs_all")   # one triple per group
                else:
                    loss = model(bh, br, bp, bn, device=device, mode="pre_training")
            if np.isnan(loss.cpu().detach().numpy()):
                sys.exit("ERROR (Pre-training): loss is nan")
            loss.backward()
            optimizer.step()
            total += loss.item()
        t1 = time.time()
        model(h_list, t_list, r_list, relations, device=device, mode="update_att")
        torch.cuda.synchronize()
        print(f"epoch {epoch}: mean loss {total / a.iters:.4f} | {a.iters} iters {t1 - t0:.2f} s "
              f"({(t1 - t0) / a.iters * 1e3:.1f} ms/iter) | update_att {time.time() - t1:.3f} s")
    if a.eval_sampled > 0:
        every = known if known is not None else KnownTriples(h_list, r_list, t_list, a.entities, 16)
        eh, er, et = (x[-min(10_000, x.numel()):] for x in (h_list, r_list, t_list))      # the held-out slice
        neg_t = NegativeSampler(a.entities, every, corrupt="tail").sample(eh, er, et, a.eval_sampled, seed=2022)
        neg_h = NegativeSampler(a.entities, every, corrupt="head").sample(eh, er, et, a.eval_sampled, seed=2022)
        m = model.evaluate_list_ranking(eh, er, et, tail_lists=neg_t.neg, head_lists=neg_h.neg, known=every)
        print(f"sampled ranking, {eh.numel()} triples x {a.eval_sampled} filtered negatives per side: " +
              " | ".join(f"{k_} {v:.4f}" for k_, v in m.items() if isinstance(v, float)))
    path = "/tmp/pre-training_model_epoch%d.pth" % a.epochs
    torch.save({"model_state_dict": model.state_dict(), "epoch": a.epochs}, path)
    back = LiteralKG(args, a.entities, 16)
    back.load_state_dict(torch.load(path, map_location="cpu")["model_state_dict"])
    print("checkpoint round trip ok:", path, "A_in nnz", back.A_in._nnz())


if __name__ == "__main__":
    main()
