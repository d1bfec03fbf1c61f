"""A training-mode step -- message dropout ON, the configuration the model is trained in -- against the float64 oracle.

The device's masks are a stated function of (seed, row, column) (dropout_cases.py holds the host port), so a step with
dropout has an exact reference: every layer's seed is recorded by wrapping ops.new_seed, the port rebuilds each layer's scale
tensor (0 or 1 / (1 - p)), and oracle/literalkg_oracle.py applies THAT instead of F.dropout (gat_embeddings' dropout_scales).
Loss and every parameter gradient of one pre_training step and one fine_tuning step are then judged as test_gpu_fuzz.py
judges the eval-mode step of the same configuration, by the same helpers and factors: within 1e-4 (loss) / 2e-3 (gradients)
of the float32 oracle's largest entry, or no further from the float64 oracle than 10 x the float32 oracle is.

Rows of the mask.  On the full table a layer's mask row is the entity id.  Under prune_to_batch layer k runs on the compact
rows R_k = BatchSubgraph.rows[k], and the mask row is the POSITION inside R_k: the port's scale of positions 0 .. |R_k| - 1 is
scattered to the entity ids R_k for the oracle (1 elsewhere: the loss reads nothing of those rows).  That is the contract
'only the dropout mask indexes compact rows' of literalkg_amd/pruned.py, held here.

Configurations (n = 600: dense backward; n = 16389: the row-sparse backward machinery is active):
  gcn 300 -> 32          the narrowing layer (projects, then aggregates): forward narrow form, last layer (y not kept)
  gcn 64 -> 32 -> 32     the one-launch narrow layer (from 4096 rows on) under a narrowing one
  gcn 200 -> 200         a 200-wide layer: the general 16-byte form
  gcn 64, residual       two residual layers
  gin 32, 2 layers       the skip-sum: two LayerNorms per layer, dropout on the second only
and the first two again with prune_to_batch at n = 16389."""
import numpy as np
import pytest
import torch

import dropout_cases as D
import test_gpu_fuzz as F

pytestmark = pytest.mark.gpu

BASE = dict(residual=False, gate=None, txt_dim=300, scale=None, scoring="transr", rel_dim=16, n_rel=3, batch=200, neg=3, prune=False,
            mlp_hidden=24, skew="zipf", weight_scale=1.0, batch_pool=0)
KINDS = {
    "gcn 300->32": dict(agg="gcn", layers=1, dim=300, conv=32),
    "gcn 64->32->32": dict(agg="gcn", layers=2, dim=64, conv=32),
    "gcn 200->200": dict(agg="gcn", layers=1, dim=200, conv=200),
    "gcn 64 residual": dict(agg="gcn", layers=2, dim=64, conv=64, residual=True),
    "gin 32 x2": dict(agg="gin", layers=2, dim=32, conv=32),
}
CASES = [(kind, n, False) for kind in KINDS for n in (600, 16389)] + [(kind, 16389, True) for kind in ("gcn 300->32", "gcn 64->32->32")]


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def O():
    from oracle import literalkg_oracle
    return literalkg_oracle


def in_f64(O, loss_of, params, a_in, num, txt, scales):
    """the oracle in float64 on the same inputs and the same masks, evaluated once and only when a comparison asks for it
    (test_gpu_fuzz.run_case's, with the masks)"""
    memo = {}

    def run():
        if not memo:
            dd = lambda x: None if x is None else x.double()
            p64 = {k: (v.double() if v.is_floating_point() else v).clone().requires_grad_(v.is_floating_point())
                   for k, v in params.items()}
            seen, act = [], O._act

            def spy(x):
                seen.append(float(x.detach().abs().min() / (x.detach().abs().max() + 1e-300)))
                return act(x)
            O._act = spy
            try:
                loss = loss_of(p64, a_in.double(), dd(num), dd(txt), [s.double() for s in scales])
                loss.backward()
            finally:
                O._act = act
            memo.update(p64)
            memo["loss"] = loss.detach()
            memo["smallest relative LeakyReLU input"] = min(seen) if seen else 1.0
        return memo
    return run


def port_scales(seeds, widths, p, n, sub):
    """one float32 [n, width] tensor per layer: the port's scale on the rows the layer's kernel numbered"""
    out = []
    for k, (seed, w) in enumerate(zip(seeds, widths), start=1):
        if sub is None:
            out.append(torch.from_numpy(D.scale(seed, np.arange(n), np.arange(w), p)))
        else:           # compact rows: position i of R_k is entity R_k[i]
            rk = sub.rows[k].cpu()
            full = torch.ones(n, w)
            full[rk] = torch.from_numpy(D.scale(seed, np.arange(rk.numel()), np.arange(w), p))
            out.append(full)
    return out


def dropout_step(L, O, gpu_device, monkeypatch, kind, n, prune, p, value_seed):
    from literalkg_amd import ops, pruned
    c = dict(BASE, **KINDS[kind], n=n, e=3 * n, prune=prune, cfg=dict(mess_dropout=p))
    if prune:
        c.update(batch=30)               # (a frontier of some 1700 rows: well below prune_max_fraction of the entities)
    k = F.build_case(L, O, gpu_device, c, 4242, value_seed)
    m, cfg, widths = k.m, k.cfg, [c["conv"]] * c["layers"]
    assert [float(layer.dropout) for layer in m.aggregator_layers] == [p] * c["layers"]
    seeds, subs = [], []
    real_seed, real_sub = ops.new_seed, pruned.build_batch_subgraph

    def new_seed():
        seeds.append(real_seed())
        return seeds[-1]

    def build_batch_subgraph(*a, **kw):
        subs.append(real_sub(*a, **kw))
        return subs[-1]
    monkeypatch.setattr(ops, "new_seed", new_seed)
    monkeypatch.setattr(pruned, "build_batch_subgraph", build_batch_subgraph)
    dev = lambda *xs: [x.to(gpu_device) for x in xs]
    steps = (("pre_training", (k.bh, k.br, k.bp, k.bn),
              lambda q, a, nu, tx, sc: O.triple_loss_transr(q, cfg, O.gat_embeddings(q, cfg, a, nu, tx, dropout_scales=sc),
                                                            k.bh, k.br, k.bp, k.bn)),
             ("fine_tuning", (k.bh, k.bp, k.bn),
              lambda q, a, nu, tx, sc: O.prediction_loss(cfg, O.gat_embeddings(q, cfg, a, nu, tx, dropout_scales=sc), k.bh, k.bp, k.bn)))
    m.train()
    try:
        for mode, batch, loss_of in steps:
            del seeds[:], subs[:]
            m.zero_grad(set_to_none=True)
            torch.manual_seed(value_seed + 11)
            loss = m(*dev(*batch), device=gpu_device, mode=mode)
            loss.backward()
            assert len(seeds) == c["layers"] and len(set(seeds)) == len(seeds), (mode, seeds)      # one seed per layer, all different
            sub = subs[-1] if subs else None
            if prune:
                assert sub is not None and m.gat_rows is not None, "the pruned path did not run"
                assert all(sub.rows[j].numel() < n // 2 for j in range(1, c["layers"] + 1))
            else:
                assert sub is None and m.gat_rows is None
            scales = port_scales(seeds, widths, p, n, sub)
            p32 = {kk: v.clone().requires_grad_(v.is_floating_point()) for kk, v in k.params.items()}
            want = loss_of(p32, k.a_in, k.num, k.txt, scales)
            want.backward()
            ref64 = in_f64(O, loss_of, k.params, k.a_in, k.num, k.txt, scales)
            tag = f"{kind} n {n}{' pruned' if prune else ''} p {p} {mode}"
            print(f"{tag}: loss {float(loss):.7g} oracle32 {float(want):.7g}; seeds {[hex(s) for s in seeds]}")
            F.within_reference_noise(loss.detach().cpu().reshape(1), want.detach().reshape(1), lambda: ref64()["loss"].reshape(1),
                                     1e-4, (tag, "loss"))
            F.close_grads(m.named_parameters(), p32, ref64, tag, None, 2e-3)
    finally:
        m.eval()
        ops._RowScratch._tables.clear()


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("kind,n,prune", CASES, ids=lambda v: str(v).replace(" ", "_"))
def test_training_step_with_dropout_matches_the_float64_oracle(L, O, gpu_device, monkeypatch, kind, n, prune, p):
    for attempt in range(3):            # (a LeakyReLU input within rounding reach of zero: other values, as test_gpu_fuzz does)
        try:
            return dropout_step(L, O, gpu_device, monkeypatch, kind, n, prune, p, 77 + 7919 * attempt)
        except F.NearKink as e:
            if attempt == 2:
                raise
            print("near a LeakyReLU kink:", e, "\n-> the same configuration with other values")
