"""GPU: the MLP pair head at inference (literalkg_amd/pairmlp.py, lkg_pairmlp.hip) against float64.

The float64 reference is the head restated here on a float64 copy of the same f32 table and parameters (BatchNorm in
inference form; oracle.literalkg_oracle.mlp_head is used where a whole model exists).  Next to every float64 logit the
reference carries a running error bound E for the device's logit, computed in float64 from absolute values, u = 2^-24:

    du = 2 (C + 4) u |e_h| |W1h|^T + u |u|         the tall GEMM and the rounding of + b1
    dv = 2 (C + 4) u |e_t| |W1t|^T
    d1 = du + dv + u |u + v|                        x1 = relu(u + v): one more rounding, relu is 1-Lipschitz
    d2 = |W2'| d1 + (128 + 2) u |W2'| x1            the fc2 fma chain and + b2'
         + u |W2'| x1 + u |b2'| + u |pre2|          one rounding per folded parameter
    E  = |w3'| . d2 + (64 + 2) u |w3'| . x2         the fc3 reduction and + b3'
         + u |w3'| . x2 + u |b3'| + u |z|           one rounding per folded parameter

Probabilities: E / 4 (the sigmoid's slope) plus 2 ulp of a number in [1/2, 1).  The bound holds for every pair.  Exact
behaviour (ties, filter, padding, candidate ids) is checked on small-integer data where every f32 step is exact.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from conftest import golden_cfg, golden_params, load_golden

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
ULP = 2.0 ** -24             # of a probability in [1/2, 1)


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def R(L):
    from literalkg_amd import ranking
    return ranking


@pytest.fixture(scope="module")
def ops(L):
    from literalkg_amd import ops
    return ops


# ----------------------------------------------------------------------------- a model to test on
class StandIn:
    """What mlp_scores / predict_topk(scoring='mlp') read of a LiteralKG, over a given table."""

    def __init__(self, table, head, n_rel=5):
        self.T = table
        self.entity_embed = SimpleNamespace(weight=table)
        self.n_entities, self.n_relations = table.shape[0], n_rel
        self.scoring = "dot"
        self.training = False
        for k, v in head.items():
            setattr(self, k, v)

    def _table_for_inference(self):
        return self.T


def random_head(gen, c, dev):
    """xavier weights, BatchNorm affine and running statistics away from 0 / 1"""
    fc1, fc2, fc3 = torch.nn.Linear(2 * c, 128), torch.nn.Linear(128, 64), torch.nn.Linear(64, 1)
    norm1, norm2 = torch.nn.BatchNorm1d(128), torch.nn.BatchNorm1d(64)
    with torch.no_grad():
        for fc in (fc1, fc2, fc3):
            torch.nn.init.xavier_uniform_(fc.weight, generator=gen)
            fc.bias.copy_(0.2 * torch.randn(fc.bias.shape, generator=gen))
        for bn in (norm1, norm2):
            d = bn.num_features
            bn.weight.copy_(0.5 + torch.rand(d, generator=gen))
            bn.bias.copy_(0.3 * torch.randn(d, generator=gen))
            bn.running_mean.copy_(0.2 + 0.2 * torch.randn(d, generator=gen))
            bn.running_var.copy_(0.3 + 1.5 * torch.rand(d, generator=gen))
            bn.num_batches_tracked.fill_(7)
    return {k: m.to(dev).eval() for k, m in dict(fc1=fc1, norm1=norm1, fc2=fc2, norm2=norm2, fc3=fc3).items()}


def random_model(seed, n, c, dev):
    gen = torch.Generator().manual_seed(seed)
    table = torch.nn.functional.normalize(torch.randn(n, c, generator=gen), dim=1).to(dev)
    return StandIn(table, random_head(gen, c, dev)), gen


# ----------------------------------------------------------------------------- float64 reference with its bound
def head64(model):
    """the head's parameters in float64 with BatchNorm in inference form folded forward (the four lines of pairmlp.py)"""
    d = lambda t: t.detach().double()
    w1, w2, w3 = d(model.fc1.weight), d(model.fc2.weight), d(model.fc3.weight).reshape(-1)
    c = w1.shape[1] // 2
    ac = []
    for bn in (model.norm1, model.norm2):
        a = d(bn.weight) / torch.sqrt(d(bn.running_var) + bn.eps)
        ac.append((a, d(bn.bias) - d(bn.running_mean) * a))
    (a1, c1), (a2, c2) = ac
    return SimpleNamespace(w1h=w1[:, :c], w1t=w1[:, c:], b1=d(model.fc1.bias), w2=w2 * a1[None, :],
                           b2=w2 @ c1 + d(model.fc2.bias), w3=w3 * a2, b3=(w3 @ c2 + d(model.fc3.bias).reshape(())))


def ref64(model, hid, tid, chunk=8):
    """(Z, E): float64 logits z(h_i, t_j) and the device's error bound (module docstring), len(hid) x len(tid)"""
    p = head64(model)
    t64 = model._table_for_inference().detach().double()
    eh, et = t64[hid], t64[tid]
    c = eh.shape[1]
    eps_p = 2.0 * (c + 4) * U
    u, v = eh @ p.w1h.T + p.b1, et @ p.w1t.T
    du = eps_p * (eh.abs() @ p.w1h.abs().T) + U * u.abs()
    dv = eps_p * (et.abs() @ p.w1t.abs().T)
    aw2, aw3 = p.w2.abs(), p.w3.abs()
    zs, es = [], []
    for lo in range(0, hid.numel(), chunk):
        pre1 = u[lo:lo + chunk, None, :] + v[None, :, :]
        d1 = du[lo:lo + chunk, None, :] + dv[None, :, :] + U * pre1.abs()
        x1 = pre1.clamp_min(0)
        pre2 = x1 @ p.w2.T + p.b2
        ax = x1 @ aw2.T
        d2 = d1 @ aw2.T + (128 + 2) * U * ax + U * ax + U * p.b2.abs() + U * pre2.abs()
        x2 = pre2.clamp_min(0)
        z = x2 @ p.w3 + p.b3
        ax2 = x2 @ aw3
        es.append(d2 @ aw3 + (64 + 2) * U * ax2 + U * ax2 + U * p.b3.abs() + U * z.abs())
        zs.append(z)
    return torch.cat(zs), torch.cat(es)


SHAPES = [(700, 37), (3000, 48), (20000, 96)]
N_QUERIES = 256


@pytest.fixture(scope="module")
def cases(L, gpu_device):
    """per shape: the model, the 256 query ids, and for both roles the float64 logits / bounds and the device's logits.
    Role 'tail': row i, column c = the pair (query_i, c); role 'head': the pair (c, query_i)."""
    made = {}

    def get(n, c):
        if (n, c) not in made:
            model, gen = random_model(100 + n + c, n, c, gpu_device)
            q = torch.randint(0, n, (N_QUERIES,), generator=gen).to(gpu_device)
            every = torch.arange(n, device=gpu_device)
            zt, et = ref64(model, q, every)
            zh, eh = ref64(model, every, q, chunk=512)
            dev_t = L.mlp_scores(model, q, every, logits=True)
            dev_h = L.mlp_scores(model, every, q, logits=True).T.contiguous()
            made[(n, c)] = SimpleNamespace(model=model, gen=gen, q=q, n=n, Z=dict(tail=zt, head=zh.T.contiguous()),
                                           E=dict(tail=et, head=eh.T.contiguous()), D=dict(tail=dev_t, head=dev_h))
        return made[(n, c)]
    return get


# ----------------------------------------------------------------------------- 4. exact op test
def int_head(gen, dev):
    """small integers: every product and partial sum of the kernel is an integer far below 2^24"""
    w2 = torch.randint(-2, 3, (64, 128), generator=gen).float()
    b2 = torch.randint(-60, -20, (64,), generator=gen).float()      # few fc2 outputs survive: ties are frequent
    w3 = torch.randint(-2, 3, (64,), generator=gen).float()
    b3 = torch.randint(-3, 4, (1,), generator=gen).float()
    return tuple(t.to(dev) for t in (w2, b2, w3, b3))


def int_logits(uq, v, w2, b2, w3, b3):
    uq, v, w2, b2, w3, b3 = (t.cpu().to(torch.int64) for t in (uq, v, w2, b2, w3, b3))
    x1 = (uq[:, None, :] + v[None, :, :]).clamp_min(0)
    x2 = (x1 @ w2.T + b2).clamp_min(0)
    return x2 @ w3 + b3[0]


@pytest.mark.parametrize("n_q,n_c,k", [(50, 300, 20), (1, 777, 10), (65, 64, 7), (130, 1000, 128), (3, 5, 10),
                                       (600, 200, 3)])
def test_exact_integer_op(L, R, ops, gpu_device, n_q, n_c, k):
    gen = torch.Generator().manual_seed(n_q * 1000 + n_c + k)
    uq = torch.randint(-3, 4, (n_q, 128), generator=gen).float().to(gpu_device)
    v = torch.randint(-3, 4, (n_c, 128), generator=gen).float().to(gpu_device)
    head = int_head(gen, gpu_device)
    want = int_logits(uq, v, *head)
    assert int(want.abs().max()) < 2 ** 16                                                 # exact in f32 with room
    if want.numel() > 1000:
        assert want.unique().numel() < want.numel() // 4                                   # and with many ties
    got = ops.pair_mlp_scores(uq, v, *head)
    assert got.shape == (n_q, n_c) and torch.equal(got.cpu().to(torch.int64), want) and bool((got == got.round()).all())
    # into a strided output
    wide = torch.full((n_q, n_c + 3), -7.0, device=gpu_device)
    ops.pair_mlp_scores(uq, v, *head, out=wide[:, :n_c])
    assert torch.equal(wide[:, :n_c], got) and bool((wide[:, n_c:] == -7.0).all())

    def expect(elig, ids_of):
        rows_i, rows_z = [], []
        for i in range(n_q):
            order = sorted((j for j in range(n_c) if elig(i, j)), key=lambda j: (-int(want[i, j]), ids_of[j]))[:k]
            rows_i.append([ids_of[j] for j in order] + [-1] * (k - len(order)))
            rows_z.append([float(want[i, j]) for j in order] + [math.nan] * (k - len(order)))
        return rows_i, rows_z

    def same(res, exp):
        ids, z = res
        assert ids.dtype == torch.int64 and z.dtype == torch.float32 and ids.shape == (n_q, k) == z.shape
        assert ids.cpu().tolist() == exp[0]
        np.testing.assert_array_equal(z.cpu().numpy(), np.array(exp[1], dtype=np.float32))

    plain = list(range(n_c))
    same(ops.pair_mlp_topk(uq, v, *head, k), expect(lambda i, j: True, plain))
    # entity ids through cand_ids (a permutation with gaps), and the known-pair filter over entity ids
    n_ent, n_rel = 2 * n_c + 11, 3
    cand = torch.randperm(n_ent, generator=gen)[:n_c]
    cand_l = cand.tolist()
    same(ops.pair_mlp_topk(uq, v, *head, k, cand_ids=cand.to(gpu_device)), expect(lambda i, j: True, cand_l))
    frow = torch.randint(0, n_ent, (n_q,), generator=gen)
    m = 40 * n_q
    kh = frow[torch.randint(0, n_q, (m,), generator=gen)]
    kt = cand[torch.randint(0, n_c, (m,), generator=gen)]
    kr = torch.randint(0, n_rel, (m,), generator=gen)
    if n_c > 8:                      # query 0 is known with all but 4 candidates under relation 1: padded
        kh = torch.cat([kh, frow[0].repeat(n_c - 4)])
        kt = torch.cat([kt, cand[4:]])
        kr = torch.cat([kr, torch.ones(n_c - 4, dtype=torch.int64)])
    known = R.KnownTriples(kh.to(gpu_device), kr.to(gpu_device), kt.to(gpu_device), n_ent, n_rel)
    trip = set(zip(kh.tolist(), kr.tolist(), kt.tolist()))
    pair = set((a, c) for a, _, c in trip)
    frow_l = frow.tolist()
    for frel in (torch.full((n_q,), -1, dtype=torch.int64), torch.ones(n_q, dtype=torch.int64),
                 torch.randint(0, n_rel, (n_q,), generator=gen)):
        frel_l = frel.tolist()
        exp = expect(lambda i, j: ((frow_l[i], cand_l[j]) not in pair) if frel_l[i] < 0
                     else ((frow_l[i], frel_l[i], cand_l[j]) not in trip), cand_l)
        for splits in (0, 1, 3):
            same(ops.pair_mlp_topk(uq, v, *head, k, known.by_head, frow.to(gpu_device), frel.to(gpu_device),
                                   cand.to(gpu_device), splits), exp)
        if n_c > 8 and frel_l[0] in (-1, 1):
            assert exp[0][0][4:] == [-1] * (k - 4) if k > 4 else True
    with pytest.raises(ValueError):
        ops.pair_mlp_topk(uq, v, *head, 0)
    with pytest.raises(ValueError):
        ops.pair_mlp_topk(uq, v, *head, 129)
    with pytest.raises(ValueError):
        ops.pair_mlp_topk(uq, v, *head, 5, splits=65)
    with pytest.raises(ValueError):
        ops.pair_mlp_scores(uq[:, :100], v, *head)
    with pytest.raises(ValueError):
        ops.pair_mlp_scores(uq, v, head[0][:32], *head[1:])


# ----------------------------------------------------------------------------- 5. per-pair error bound
@pytest.mark.parametrize("n,c", SHAPES)
@pytest.mark.parametrize("role", ["tail", "head"])
def test_every_logit_within_its_bound(L, cases, gpu_device, n, c, role):
    cs = cases(n, c)
    z, e, d = cs.Z[role], cs.E[role], cs.D[role]
    err = (d.double() - z).abs()
    print(f"\n[{n} x {c} {role}] max |logit error| {float(err.max()):.3e}, max bound {float(e.max()):.3e}, "
          f"max error / bound {float((err / e).max()):.3f}, logits in [{float(z.min()):.2f}, {float(z.max()):.2f}]")
    assert bool((err <= e).all())
    every = torch.arange(n, device=gpu_device)
    p = L.mlp_scores(cs.model, cs.q, every) if role == "tail" else L.mlp_scores(cs.model, every, cs.q).T
    perr = (p.double() - torch.sigmoid(z)).abs()
    print(f"[{n} x {c} {role}] max |probability error| {float(perr.max()):.3e}")
    assert bool((perr <= e / 4 + 2 * ULP).all())
    assert torch.equal(p, torch.sigmoid(d.double()).float())          # the probability is the rounded sigmoid of the logit


# ----------------------------------------------------------------------------- 6. agreement with mode='mlp'
def _golden_mlp_model(L, name, dev):
    gd = load_golden(name)
    scoring = "transr" if bool(gd["init_mlp"]) else "transe"
    cfg = golden_cfg(gd)
    n = int(gd["n"])
    a_in = torch.sparse_coo_tensor(torch.from_numpy(gd["a_indices"]), torch.from_numpy(gd["a_values"]), (n, n)).coalesce()
    m = L.LiteralKG(cfg, n, int(gd["n_rel"]), a_in, scoring=scoring)
    if scoring == "transr":
        m.initialize_MLP()
    m.load_state_dict(golden_params(gd), strict=False)
    m.load_state_dict({k[6:]: torch.from_numpy(v) for k, v in gd.items() if k.startswith("after/")}, strict=False)
    return m.to(dev).eval(), gd


def eager_bound(model, table64, h, t):
    """(z64, bound) of the unfused eval-mode path model(h, t, mode='mlp') for the pairs (h_i, t_i): every Linear within
    the engines' 2 (K + 4) u |x| |W|^T plus the bias rounding, every BatchNorm (x - mean) * invstd * gamma + beta within
    4 roundings of its largest intermediate, errors carried forward through |W| and relu."""
    d = lambda t_: t_.detach().double()
    x = torch.cat([table64[h], table64[t]], dim=1)
    err = torch.zeros_like(x)
    for fc, bn in ((model.fc1, model.norm1), (model.fc2, model.norm2), (model.fc3, None)):
        w, b = d(fc.weight), d(fc.bias)
        y = x @ w.T + b
        err = err @ w.abs().T + 2.0 * (w.shape[1] + 4) * U * (x.abs() @ w.abs().T) + U * y.abs()
        if bn is None:
            return y.reshape(-1), err.reshape(-1)
        y = y.clamp_min(0)
        a = d(bn.weight) / torch.sqrt(d(bn.running_var) + bn.eps)
        x = (y - d(bn.running_mean)) * a + d(bn.bias)
        err = err * a.abs() + 4 * U * ((y.abs() + d(bn.running_mean).abs()) * a.abs() + d(bn.bias).abs() + x.abs())


@pytest.mark.parametrize("name", ["mlp_model_gcn_l1_scale", "mlp_bce_gcn_l2_scale"])
def test_agrees_with_mode_mlp_and_the_reference_fixture(L, gpu_device, name):
    import oracle.literalkg_oracle as O
    m, gd = _golden_mlp_model(L, name, gpu_device)
    heads, tails = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("heads", "tails"))
    n = m.n_entities
    # the reference's own eval-mode numbers on its 96 pairs
    sc = m.mlp_scores(heads, tails)
    assert sc.shape == (96, 96) and sc.dtype == torch.float32
    np.testing.assert_allclose(sc.diagonal().cpu().numpy(), gd["out_eval"], rtol=1e-4, atol=1e-5)
    res = m.predict_topk(heads, None, side="tail", k=min(n, 128), scoring="mlp", candidates=torch.unique(tails))
    for i in range(96):
        at = torch.nonzero(res.ids[i] == tails[i]).reshape(-1)
        assert at.numel() == 1, i
        np.testing.assert_allclose(float(res.scores[i, at[0]]), gd["out_eval"][i], rtol=1e-4, atol=1e-5)
        assert float(res.scores[i, at[0]]) == float(sc[i, i])
    # explicit pairs through mode='mlp' (eval, no_grad) and through mlp_scores: both within their bound of float64
    gen = torch.Generator().manual_seed(5)
    hs, ts = (torch.randint(0, n, (40,), generator=gen).to(gpu_device) for _ in range(2))
    hh, tt = hs.repeat_interleave(40), ts.repeat(40)
    with torch.no_grad():
        eager = m(hh, tt, device=gpu_device, mode="mlp").reshape(40, 40)
        table = m._table_for_inference().detach()
    fused = m.mlp_scores(hs, ts)
    z64, e_fused = ref64(m, hs, ts)
    zz, e_eager = eager_bound(m, table.double(), hh, tt)
    p64 = torch.sigmoid(z64)
    assert float((zz.reshape(40, 40) - z64).abs().max()) < 1e-12
    p_or = O.mlp_head({k: (v.detach().double() if v.is_floating_point() else v.detach()) for k, v in m.state_dict().items()
                       if not v.is_sparse}, table.double(), hh, tt, training=False).reshape(40, 40)
    assert float((p_or - p64).abs().max()) < 1e-12
    b_fused, b_eager = e_fused / 4 + 2 * ULP, e_eager.reshape(40, 40) / 4 + 4 * ULP
    assert bool(((fused.double() - p64).abs() <= b_fused).all())
    assert bool(((eager.double() - p64).abs() <= b_eager).all())
    assert bool(((fused.double() - eager.double()).abs() <= b_fused + b_eager).all())


# ----------------------------------------------------------------------------- 7. top-k against float64 with margins
def eligibility(n, side, q, cand, known, r):
    """B x len(cand) bool: the pair is not known (under r[i], or under any relation when r is None)"""
    elig = torch.ones((q.numel(), cand.numel()), dtype=torch.bool, device=q.device)
    if known is None:
        return elig
    kh, kr, kt = known
    a, b_ = (kh, kt) if side == "tail" else (kt, kh)              # a: the query's end, b_: the candidate's
    for i in range(q.numel()):
        hit = a == q[i]
        if r is not None:
            hit &= kr == r[i]
        elig[i] &= ~torch.isin(cand, b_[hit])
    return elig


def check_topk(res, cs, side, k, cand, elig, what):
    n, dev = cs.n, cs.q.device
    z, e, d = (x[side][:, cand] for x in (cs.Z, cs.E, cs.D))
    ids, ks, sc = res.ids, res.kernel_scores, res.scores
    b = ids.shape[0]
    assert ids.shape == (b, k) == ks.shape == sc.shape and res.side == side
    valid = ids >= 0
    m = valid.sum(1)
    assert torch.equal(m, elig.sum(1).clamp_max(k)), what                                 # min(k, #eligible) exactly
    assert bool((valid == (torch.arange(k, device=dev)[None, :] < m[:, None])).all()), what     # padding at the end
    assert bool(torch.isnan(ks[~valid]).all()) and bool(torch.isnan(sc[~valid]).all()), what
    pos_of = torch.full((n,), -1, dtype=torch.int64, device=dev)
    pos_of[cand] = torch.arange(cand.numel(), device=dev)
    pos = pos_of[ids.clamp_min(0)]
    assert bool((pos[valid] >= 0).all()), what
    inside = torch.zeros_like(elig)
    rows = torch.arange(b, device=dev)[:, None].expand(b, k)
    inside[rows[valid], pos[valid]] = True
    assert torch.equal(inside.sum(1), m), what                                            # no id twice
    assert bool(elig[inside].all()), (what, "a returned id is not eligible")
    # bit for bit the logits of mlp_scores; ordered by (logit descending, id ascending); probabilities follow
    assert torch.equal(ks[valid], d[rows[valid], pos[valid]]), what
    for j in range(k - 1):
        both = valid[:, j + 1]
        a_, b_ = ks[both, j], ks[both, j + 1]
        assert bool(((a_ > b_) | ((a_ == b_) & (ids[both, j] < ids[both, j + 1]))).all()), (what, j)
        assert bool((sc[both, j] >= sc[both, j + 1]).all()), (what, j)
    assert torch.equal(sc[valid], torch.sigmoid(ks[valid].double()).float()), what
    # nothing eligible that was left out beats the k-th returned one by more than the two bounds together
    has = m > 0
    last = pos[torch.arange(b, device=dev), (m - 1).clamp_min(0)]
    z_last, e_last = z.gather(1, last[:, None]), e.gather(1, last[:, None])
    out = elig & ~inside & has[:, None]
    assert bool((z[out] <= (z_last + e_last + e).expand_as(z)[out]).all()), what
    # the cap: margins must not hide a broken selection
    want = torch.topk(z.masked_fill(~elig, -math.inf), k, dim=1).indices
    full = m == k
    got = pos[full]
    if k <= 10:
        share = float((got == want[full]).all(1).double().mean())
    else:
        share = float((got.sort(1).values == want[full].sort(1).values).all(1).double().mean())
    print(f"[{what}] share of queries with float64's {'list' if k <= 10 else 'set'}: {share:.4f}")
    assert share >= 0.9, (what, share)


def draw_known(cs, side, r, n_rel, cand):
    """known triples that bite: for every query some of float64's best candidates (under the query's relation, another
    relation, or both), plus random ones"""
    gen, dev, n = cs.gen, cs.q.device, cs.n
    top = torch.topk(cs.Z[side], 12, dim=1).indices                       # entity ids (the columns are all entities)
    pick = torch.rand(top.shape, generator=gen).to(dev) < 0.4
    qq = cs.q[:, None].expand_as(top)[pick]
    cc = top[pick]
    rr = r[:, None].expand_as(top)[pick]
    other = torch.rand(rr.shape, generator=gen).to(dev) < 0.3
    rr = torch.where(other, (rr + 1) % n_rel, rr)
    m = 2000
    xa, xb = (torch.randint(0, n, (m,), generator=gen).to(dev) for _ in range(2))
    xr = torch.randint(0, n_rel, (m,), generator=gen).to(dev)
    a, b_ = torch.cat([qq, xa]), torch.cat([cc, xb])
    return (a, torch.cat([rr, xr]), b_) if side == "tail" else (b_, torch.cat([rr, xr]), a)


@pytest.mark.parametrize("n,c", SHAPES)
@pytest.mark.parametrize("side", ["tail", "head"])
def test_topk_against_float64(L, R, cases, gpu_device, n, c, side):
    cs = cases(n, c)
    n_rel = cs.model.n_relations
    r = torch.randint(0, n_rel, (N_QUERIES,), generator=cs.gen).to(gpu_device)
    every = torch.arange(n, device=gpu_device)
    subset = torch.randperm(n, generator=cs.gen)[: (2 * n) // 3].to(gpu_device)       # unsorted entity ids
    known = draw_known(cs, side, r, n_rel, every)
    kt_ = R.KnownTriples(*known, n, n_rel)
    for k in (10, 100):
        for kn in (None, "any", "rel"):
            for cand in (None, subset):
                what = f"{n} x {c} {side} k={k} known={kn} candidates={'subset' if cand is not None else 'all'}"
                res = L.predict_topk(cs.model, cs.q, r if kn == "rel" else None, side=side, k=k, scoring="mlp",
                                     known=kt_ if kn else None, candidates=cand)
                cc = every if cand is None else cand
                elig = eligibility(n, side, cs.q, cc, known if kn else None, r if kn == "rel" else None)
                check_topk(res, cs, side, k, cc, elig, what)
                if kn:
                    assert int((~elig).sum()) > N_QUERIES          # the filter did bite


# ----------------------------------------------------------------------------- 8. invariance
def test_invariance(L, R, cases, gpu_device):
    cs = cases(3000, 48)
    n, n_rel = cs.n, cs.model.n_relations
    q = cs.q[:100]
    r = torch.randint(0, n_rel, (100,), generator=cs.gen).to(gpu_device)
    known = R.KnownTriples(*draw_known(cs, "tail", torch.randint(0, n_rel, (N_QUERIES,), generator=cs.gen).to(gpu_device),
                                       n_rel, None), n, n_rel)
    for side in ("tail", "head"):
        for k in (10, 100):
            kw = dict(side=side, k=k, scoring="mlp", known=known)
            base = L.predict_topk(cs.model, q, r, **kw)
            for extra in (dict(splits=1), dict(splits=3), dict(splits=64), dict(batch_size=1), dict(batch_size=7),
                          dict(batch_size=7, splits=5)):
                if k == 100 and extra.get("batch_size") == 1:
                    continue
                res = L.predict_topk(cs.model, q, r, **kw, **extra)
                assert torch.equal(res.ids, base.ids), (side, k, extra)
                assert torch.equal(res.kernel_scores.view(torch.int32), base.kernel_scores.view(torch.int32)), (side, k, extra)
                assert torch.equal(res.scores.view(torch.int32), base.scores.view(torch.int32)), (side, k, extra)
            perm = torch.randperm(100, generator=cs.gen).to(gpu_device)
            res = L.predict_topk(cs.model, q[perm], r[perm], **kw)
            assert torch.equal(res.ids, base.ids[perm]) and \
                torch.equal(res.kernel_scores.view(torch.int32), base.kernel_scores[perm].view(torch.int32)), (side, k)
            res = L.predict_topk(cs.model, q, r, candidates=torch.randperm(n, generator=cs.gen).to(gpu_device), **kw)
            assert torch.equal(res.ids, base.ids) and \
                torch.equal(res.kernel_scores.view(torch.int32), base.kernel_scores.view(torch.int32)), (side, k)
            # the store epilogue gives the same bits as the select epilogue, whatever rows the matrix is asked for
            some = torch.randperm(n, generator=cs.gen)[:777].to(gpu_device)
            sub = L.mlp_scores(cs.model, q, some, logits=True) if side == "tail" else \
                L.mlp_scores(cs.model, some, q, logits=True).T
            assert torch.equal(sub.contiguous().view(torch.int32), cs.D[side][:100][:, some].contiguous().view(torch.int32))
            valid = base.ids >= 0
            rows = torch.arange(100, device=gpu_device)[:, None].expand_as(base.ids)
            assert torch.equal(base.kernel_scores[valid], cs.D[side][:100][rows[valid], base.ids[valid]])


# ----------------------------------------------------------------------------- 9. filter semantics
def test_filter_semantics(L, R, gpu_device):
    n, n_rel = 300, 3
    model, gen = random_model(9, n, 24, gpu_device)
    model.n_relations = n_rel
    q = torch.tensor([5, 17, 100, 299], device=gpu_device)
    r = torch.tensor([0, 1, 2, 1], device=gpu_device)
    free = L.predict_topk(model, q, None, k=8, scoring="mlp")
    best = free.ids[:, 0]                                                 # each query's best tail ...
    kh, kr, kt = q.clone(), (r + 1) % n_rel, best.clone()                 # ... known under ANOTHER relation than r
    heavy = torch.arange(n, device=gpu_device)
    heavy = heavy[heavy % 60 != 0]                                        # query 3: all but 5 tails known under its r
    kh, kr, kt = torch.cat([kh, q[3].repeat(heavy.numel())]), torch.cat([kr, r[3].repeat(heavy.numel())]), \
        torch.cat([kt, heavy])
    known = R.KnownTriples(kh, kr, kt, n, n_rel)
    any_rel = L.predict_topk(model, q, None, k=8, scoring="mlp", known=known)
    own_rel = L.predict_topk(model, q, r, k=8, scoring="mlp", known=known)
    for i in range(3):
        assert int(best[i]) not in any_rel.ids[i].tolist()               # r=None: known under any relation -> dropped
        assert any_rel.ids[i, :7].tolist() == free.ids[i, 1:].tolist()
        assert own_rel.ids[i].tolist() == free.ids[i].tolist()           # r given: only that relation counts
    for res in (any_rel, own_rel):
        left = [c for c in range(0, n, 60) if not (res is any_rel and c == int(best[3]))]
        assert sorted(res.ids[3, :len(left)].tolist()) == left
        assert res.ids[3, len(left):].tolist() == [-1] * (8 - len(left))
        assert bool(torch.isnan(res.scores[3, len(left):]).all()) and bool(torch.isnan(res.kernel_scores[3, len(left):]).all())
    # the head side reads the other structure: (c, r, query)
    hres = L.predict_topk(model, best[:3], (r + 1)[:3] % n_rel, side="head", k=8, scoring="mlp", known=known)
    for i in range(3):
        assert int(q[i]) not in hres.ids[i].tolist()
    # a query that is the head of no known triple (an empty filter row) keeps its free list
    lone = torch.tensor([41], device=gpu_device)
    assert not bool((kh == 41).any())
    assert torch.equal(L.predict_topk(model, lone, r[:1], k=8, scoring="mlp", known=known).ids,
                       L.predict_topk(model, lone, None, k=8, scoring="mlp").ids)
    # fewer candidates than k
    few = L.predict_topk(model, q, None, k=8, scoring="mlp", candidates=torch.tensor([7, 3, 250], device=gpu_device))
    assert bool((few.ids[:, 3:] == -1).all()) and sorted(few.ids[0, :3].tolist()) == [3, 7, 250]
    with pytest.raises(ValueError):
        L.predict_topk(model, q, r, scoring="mlp", known=R.KnownTriples(kh, kr, kt, n + 1, n_rel))
    with pytest.raises(ValueError):
        L.predict_topk(model, q, r, scoring="mlp", known=SimpleNamespace(n_entities=n, device=torch.device("cpu")))
    with pytest.raises(IndexError):
        L.predict_topk(model, torch.tensor([0, n], device=gpu_device), None, scoring="mlp")
    with pytest.raises(IndexError):
        L.mlp_scores(model, q, torch.tensor([-1], device=gpu_device))
    ok = L.predict_topk(model, q, r, k=5, scoring="mlp")                   # nothing left pending
    assert ok.ids.shape == (4, 5)
    with pytest.raises(ValueError):
        R.rank_triples(model, q, r, q, scoring="mlp")


# ----------------------------------------------------------------------------- 10. large shape, once
def test_two_million_candidates(L, gpu_device):
    n, c, k = 1 << 21, 32, 10
    gen = torch.Generator().manual_seed(2026)
    dgen = torch.Generator(device=gpu_device).manual_seed(2026)
    table = torch.nn.functional.normalize(torch.randn(n, c, generator=dgen, device=gpu_device), dim=1)
    model = StandIn(table, random_head(gen, c, gpu_device))
    q = torch.cat([torch.tensor([0, n - 1, 1 << 20]), torch.randint(0, n, (61,), generator=gen)]).to(gpu_device)
    table[n - 64:] = table[q] * 1.5                    # rows past 2^31 / 4 / k and past 2^31 / 128 that stand out
    res = L.predict_topk(model, q, None, k=k, scoring="mlp")
    assert bool((res.ids >= 0).all())
    sample = torch.randint(0, n, (5000,), generator=gen).to(gpu_device)
    for lo in range(0, 64, 8):
        rows = slice(lo, lo + 8)
        cols = torch.unique(torch.cat([res.ids[rows].reshape(-1), sample, torch.arange(n - 64, n, device=gpu_device)]))
        at = torch.searchsorted(cols, res.ids[rows])
        z, e = ref64(model, q[rows], cols)
        zr, er = z.gather(1, at), e.gather(1, at)
        assert bool(((res.kernel_scores[rows].double() - zr).abs() <= er).all())
        assert bool((res.kernel_scores[rows][:, 1:] <= res.kernel_scores[rows][:, :-1]).all())
        inside = torch.zeros_like(z, dtype=torch.bool)
        inside.scatter_(1, at, True)
        worst = z.masked_fill(inside, -math.inf)
        assert bool((worst <= zr[:, -1:] + er[:, -1:] + e).all())         # nothing sampled beats the k-th
        dev_rows = L.mlp_scores(model, q[rows], cols, logits=True)
        assert torch.equal(dev_rows.gather(1, at), res.kernel_scores[rows])
    full = L.mlp_scores(model, q[:1100 % 64 + 2], torch.arange(n, device=gpu_device), logits=True)   # rows x 2^21 > 2^31 / 64
    assert full.shape[1] == n and torch.equal(full.gather(1, res.ids[:full.shape[0]]), res.kernel_scores[:full.shape[0]])


# ----------------------------------------------------------------------------- 11. the model's state is untouched
@pytest.mark.parametrize("training", [False, True])
def test_model_state_untouched(L, R, gpu_device, training):
    m, gd = _golden_mlp_model(L, "mlp_model_gcn_l1_scale", gpu_device)
    heads, tails = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("heads", "tails"))
    with torch.no_grad():
        m._table_for_inference()
    m.train(training)
    cache = m.__dict__.get("_eval_cache")
    assert (cache is None) == training
    before = {k: (v, v._version, v.detach().clone()) for k, v in list(m.named_parameters()) + list(m.named_buffers())
              if not v.is_sparse}
    assert "norm1.num_batches_tracked" in before and "norm2.running_var" in before
    known = R.KnownTriples(heads, torch.zeros_like(heads), tails, m.n_entities, m.n_relations)
    p = m.mlp_scores(heads, tails)
    res = m.predict_topk(heads, None, k=5, scoring="mlp", known=known)
    res_h = L.predict_topk(m, tails, torch.zeros_like(tails), side="head", k=5, scoring="mlp", known=known)
    assert m.training == training
    for mod in (m.norm1, m.norm2, m.fc1):
        assert mod.training == training
    assert m.__dict__.get("_eval_cache") is cache
    after = dict(list(m.named_parameters()) + list(m.named_buffers()))
    for k, (v, ver, val) in before.items():
        assert after[k] is v and v._version == ver and torch.equal(v.detach(), val), k
    if not training:                 # the running statistics are what was used (the eval-mode forward agrees)
        with torch.no_grad():
            eager = m(heads, tails, device=gpu_device, mode="mlp").reshape(-1)
        np.testing.assert_allclose(p.diagonal().cpu().numpy(), eager.cpu().numpy(), rtol=1e-4, atol=1e-5)
    assert bool((res.ids >= 0).all()) and bool((res_h.ids >= 0).all())
