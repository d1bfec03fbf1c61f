"""Neighbour sampling in the module (LiteralKG.neighbor_fanout, literalkg_amd/pruned.py): a sampled step is the exact step of
the sampled matrix A' = sample_neighbors(A, seed, draw), so every check has an exact or a dense reference.

Tiny models: 400 entities, entity 0 a hub of 150 tails, mess_dropout 0, train mode, prune_max_fraction 1.  Tolerances are
the ones the project holds the exact pruned step against the dense one to (test_gpu_parity.py): the loss within
1e-6 max(1, |loss|), gradients within rtol 1e-4 / atol 1e-7 (the scatter backward adds with float atomics)."""
import numpy as np
import pytest
import torch

import invariance as V

pytestmark = pytest.mark.gpu

N_ENT, N_REL, HUB_DEGREE = 400, 3, 150


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


def triples():
    rng = np.random.default_rng(11)
    h, t, r = rng.integers(0, N_ENT, 1800), rng.integers(0, N_ENT, 1800), rng.integers(0, N_REL, 1800)
    h = np.concatenate([h, np.zeros(HUB_DEGREE, np.int64)])
    t = np.concatenate([t, rng.choice(N_ENT, HUB_DEGREE, replace=False)])
    r = np.concatenate([r, rng.integers(0, N_REL, HUB_DEGREE)])
    trip = np.unique(np.stack([h, r, t], 1), axis=0)
    return trip[:, 0].copy(), trip[:, 1].copy(), trip[:, 2].copy()


def build(L, device, aggregation="gcn", layers=2, **attrs):
    from literalkg_amd import io
    from oracle import literalkg_oracle as O
    h, r, t = triples()
    cfg = O.default_cfg(embed_dim=32, relation_dim=32, conv_dim=16, n_conv_layers=layers, aggregation_type=aggregation,
                        scale_gat_dim=24, use_num_lit=True, mess_dropout=0.0, pre_training_neg_rate=1, device=device)
    torch.manual_seed(0)
    m = L.LiteralKG(cfg, N_ENT, N_REL, io.initial_a_in(N_ENT, h, t, r), torch.rand(N_ENT, 2), None).to(device).train()
    m.prune_to_batch, m.prune_max_fraction = True, 1.0
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def batch(device):
    rng = np.random.default_rng(3)
    h = np.concatenate([[0, 0], rng.integers(0, N_ENT, 14)])            # the hub among the heads
    cols = (h, rng.integers(0, N_REL, 16), rng.integers(0, N_ENT, 16), rng.integers(0, N_ENT, 16))
    return [torch.tensor(c, device=device) for c in cols]


def calls(device):
    h, r, p, n = batch(device)
    return (("pre_training", [h, r, p, n]), ("fine_tuning", [h, p, n]))


def step(m, mode, args, device):
    m.zero_grad(set_to_none=True)
    loss = m(*args, device=device, mode=mode)
    loss.backward()
    return loss.detach().clone(), {k: v.grad.clone() for k, v in m.named_parameters() if v.grad is not None}


def close(loss, grads, want_loss, want_grads):
    assert abs(float(loss) - float(want_loss)) <= 1e-6 * max(1.0, abs(float(want_loss))), (float(loss), float(want_loss))
    assert grads.keys() == want_grads.keys()
    for k in want_grads:
        torch.testing.assert_close(grads[k], want_grads[k], rtol=1e-4, atol=1e-7, msg=k)


def max_degree(m):
    return int(m._attention().graph.rowptr.diff().max())


def sampled_matrix(L, m, fanout, seed, draw, rescale=True):
    """A' as the sparse tensor a dense model takes for A_in"""
    att = m._attention()
    rowptr, col, val = L.sample_neighbors(att.graph, att.val, fanout, seed=seed, draw=draw, rescale=rescale)
    rows = torch.repeat_interleave(torch.arange(N_ENT, device=val.device), rowptr.diff().long())
    return torch.sparse_coo_tensor(torch.stack([rows, col.long()]), val, (N_ENT, N_ENT), is_coalesced=True)


def test_a_fanout_no_row_exceeds_is_the_exact_step(L, gpu_device):
    from literalkg_amd import pruned
    m = build(L, gpu_device)
    assert max_degree(m) >= HUB_DEGREE
    att, ids = m._attention(), torch.cat(batch(gpu_device)[:1] + batch(gpu_device)[2:])
    for fanout in (max_degree(m), 2 ** 31 - 1):
        exact = pruned.build_batch_subgraph(att.graph, att.val, ids, 2)
        got = pruned.build_batch_subgraph(att.graph, att.val, ids, 2, fanout=fanout, seed=5, draw=3)
        for k in range(3):
            assert V.same_bits(got.rows[k], exact.rows[k], f"rows[{k}]")
        for k in (1, 2):
            for name in ("rowptr", "col", "val", "self_pos"):
                assert V.same_bits(getattr(got.layers[k], name), getattr(exact.layers[k], name), f"layers[{k}].{name}")
    for mode, args in calls(gpu_device):
        m.neighbor_fanout = None
        want_loss, want_grads = step(m, mode, args, gpu_device)
        assert m.last_step_sampled is False
        m.neighbor_fanout = max_degree(m)
        loss, grads = step(m, mode, args, gpu_device)
        assert m.last_step_sampled is True
        assert V.same_bits(loss, want_loss, mode)
        close(loss, grads, want_loss, want_grads)


@pytest.mark.parametrize("rescale", [True, False])
@pytest.mark.parametrize("fanout", [2, 4])
@pytest.mark.parametrize("aggregation,layers", [("gcn", 2), ("bi-interaction", 1), ("graphsage", 1)])
def test_a_sampled_step_is_the_dense_step_of_the_sampled_matrix(L, gpu_device, aggregation, layers, fanout, rescale):
    m = build(L, gpu_device, aggregation, layers, neighbor_fanout=fanout, neighbor_seed=2022, neighbor_rescale=rescale)
    dense = build(L, gpu_device, aggregation, layers, prune_to_batch=False)       # (the same seed: the same parameters)
    for draw, (mode, args) in enumerate(calls(gpu_device), start=4):
        m.neighbor_draw = draw
        loss, grads = step(m, mode, args, gpu_device)
        assert m.last_step_sampled is True and m.neighbor_draw == draw + 1
        a_prime = sampled_matrix(L, m, fanout, 2022, draw, rescale)
        assert a_prime._nnz() < m.A_in._nnz() and int(a_prime._indices()[0].bincount().max()) == fanout
        dense.A_in.data = a_prime
        want_loss, want_grads = step(dense, mode, args, gpu_device)
        assert dense.gat_rows is None
        close(loss, grads, want_loss, want_grads)


def test_draw_counter_and_eval_mode(L, gpu_device):
    m = build(L, gpu_device, neighbor_fanout=2, neighbor_seed=9)
    mode, args = calls(gpu_device)[0]
    assert m.neighbor_draw == 0
    first, _ = step(m, mode, args, gpu_device)
    second, _ = step(m, mode, args, gpu_device)
    assert m.neighbor_draw == 2 and not torch.equal(first, second)
    dense = build(L, gpu_device, prune_to_batch=False)                   # (the same seed: the same parameters)
    for draw, got in ((0, first), (1, second)):                         # the two steps used draws 0 and 1
        dense.A_in.data = sampled_matrix(L, m, 2, 9, draw)
        want, _ = step(dense, mode, args, gpu_device)
        assert abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want))), draw
    m.neighbor_draw = 0
    again, _ = step(m, mode, args, gpu_device)
    assert V.same_bits(again, first) and m.neighbor_draw == 1
    m.neighbor_seed = 10
    m.neighbor_draw = 0
    assert not torch.equal(step(m, mode, args, gpu_device)[0], first)
    exact = build(L, gpu_device)                                         # (nothing was updated: the same parameters)
    m.eval(), exact.eval()
    with torch.no_grad():
        before = m.neighbor_draw
        got, want = m(*args, device=gpu_device, mode=mode), exact(*args, device=gpu_device, mode=mode)
    assert V.same_bits(got, want) and m.last_step_sampled is False and m.neighbor_draw == before


def test_fallback_and_argument_errors(L, gpu_device):
    m = build(L, gpu_device, neighbor_fanout=2)
    dense = build(L, gpu_device, prune_to_batch=False)                   # (the same seed: the same parameters)
    mode, args = calls(gpu_device)[0]
    want, _ = step(dense, mode, args, gpu_device)
    m.prune_max_fraction = 0.01                                          # 4 rows: the batch alone is over it
    got, _ = step(m, mode, args, gpu_device)
    assert m.last_step_sampled is False and m.gat_rows is None
    assert abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    m.prune_max_fraction = 1.0                                           # the back-off: dense for the next calls all the same
    got, _ = step(m, mode, args, gpu_device)
    assert m.last_step_sampled is False and abs(float(got) - float(want)) <= 1e-6 * max(1.0, abs(float(want)))
    # argument errors come before any device work: the ids are HOST tensors here, which no kernel of the step accepts
    host_args = [a.cpu() for a in args]
    for bad in (0, -3, True, 4.0, "4"):
        m = build(L, gpu_device, neighbor_fanout=bad)
        with pytest.raises(ValueError, match="fanout"):
            m(*host_args, device=gpu_device, mode=mode)
        with pytest.raises(ValueError, match="fanout"):
            m.calc_self_adversarial_loss(host_args[0], host_args[1], host_args[2], host_args[3].view(-1, 1))
        assert m.neighbor_draw == 0
    m = build(L, gpu_device, neighbor_fanout=4, prune_to_batch=False)
    with pytest.raises(ValueError, match="prune_to_batch"):
        m(*host_args, device=gpu_device, mode=mode)
    m = build(L, gpu_device, aggregation="gin", neighbor_fanout=4)
    with pytest.raises(ValueError, match="gin"):
        m(*host_args, device=gpu_device, mode=mode)
    m.eval()                                                             # (eval mode does not sample: nothing to refuse)
    with torch.no_grad():
        assert torch.isfinite(m(*args, device=gpu_device, mode=mode))


def test_training_under_sampling_lowers_the_exact_loss(L, gpu_device):
    m = build(L, gpu_device, neighbor_fanout=2, neighbor_seed=1)
    mode, args = calls(gpu_device)[0]

    def exact_loss():
        m.eval()
        with torch.no_grad():
            out = float(m(*args, device=gpu_device, mode=mode))
        m.train()
        return out

    before = exact_loss()
    opt = torch.optim.Adam([p for p in m.parameters() if p.requires_grad], lr=1e-2)
    for _ in range(20):
        opt.zero_grad(set_to_none=True)
        m(*args, device=gpu_device, mode=mode).backward()
        assert m.last_step_sampled is True
        opt.step()
    after = exact_loss()
    print(f"exact loss {before:.6f} -> {after:.6f} after 20 sampled Adam steps")
    assert m.neighbor_draw == 20 and after < before
