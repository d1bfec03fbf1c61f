"""GPU: the MLP pair head on explicit labelled pairs -- score_pairs_mlp, evaluate_mlp_classification
(literalkg_amd/pairmlp.py), lkg_pair_mlp_pairs_f32 (lkg_pairmlp.hip) and lkg_binary_curve_f32 (lkg_csr_device.hip).

Logits are held to the bits of mlp_scores and to the float64 reference with its per-pair bound of tests/test_pairmlp_gpu.py;
counts, auc2 and the group counts to the exact references of tests/pair_cases.py; the average precision to

    |ap - ap_exact| <= (G + 4) 2^-53 ap_exact,      G = n_groups

-- three roundings per term (two quotients, one product) and at most G - 1 additions over any term in a sum of
non-negative terms -- against the exact fractions.Fraction value.

The pairs kernel caps its grid at 1024 workgroups of 64 pairs: SECOND_TRIP = 65 561 pairs make workgroup 0 take a second
trip whose wave 0 is full, wave 1 holds 9 pairs and waves 2 and 3 lie past the end.
"""
import math
import struct
from fractions import Fraction

import numpy as np
import pytest
import torch

import pair_cases as PC
from test_pairmlp_gpu import StandIn, _golden_mlp_model, eager_bound, random_model, ref64

pytestmark = pytest.mark.gpu

HEAD = ("fc1", "norm1", "fc2", "norm2", "fc3")
SHAPES = [(12, 50), (300, 500)]                 # table width C, entities
SIZES = [1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 4099]
SECOND_TRIP = 65_561


@pytest.fixture(scope="module")
def L(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    import literalkg_amd
    return literalkg_amd


@pytest.fixture(scope="module")
def ops(L):
    from literalkg_amd import ops
    return ops


@pytest.fixture(scope="module")
def PM(L):
    from literalkg_amd import pairmlp
    return pairmlp


class Model(StandIn):
    """StandIn with the two mode switches evaluate_mlp_classification uses"""

    def eval(self):
        return self.train(False)

    def train(self, mode=True):
        self.training = mode
        return self


def make_model(seed, n, c, dev):
    base, gen = random_model(seed, n, c, dev)
    return Model(base.T, {k: getattr(base, k) for k in HEAD}), gen


def draw_pairs(gen, n, p):
    """p pairs over n entities with repeated heads and tails, a pair (a, a) and a pair that occurs twice"""
    pool = torch.randint(0, n, (max(1, min(n, p // 3 + 1)),), generator=gen)
    h = pool[torch.randint(0, pool.numel(), (p,), generator=gen)]
    t = torch.randint(0, n, (p,), generator=gen)
    if p >= 3:
        t[1] = h[1]
        h[2], t[2] = h[0], t[0]
    return h, t


def bits(x):
    return x.contiguous().view(torch.int32)


def all_pairs_logits(L, model, h, t):
    """mlp_scores over the unique ids, read at every pair"""
    uh, hi = torch.unique(h, return_inverse=True)
    ut, ti = torch.unique(t, return_inverse=True)
    return L.mlp_scores(model, uh, ut, logits=True)[hi, ti]


@pytest.fixture(scope="module")
def cases(L, gpu_device):
    """per (C, n): the model; per P the pairs, the logits of score_pairs_mlp and those of mlp_scores"""
    made = {}

    def get(c, n, p=None):
        if (c, n) not in made:
            model, gen = make_model(7 * c + n, n, c, gpu_device)
            made[(c, n)] = dict(model=model, gen=gen)
        cs = made[(c, n)]
        if p is not None and p not in cs:
            h, t = (x.to(gpu_device) for x in draw_pairs(cs["gen"], n, p))
            cs[p] = dict(h=h, t=t, z=L.score_pairs_mlp(cs["model"], h, t, logits=True),
                         want=all_pairs_logits(L, cs["model"], h, t))
        return cs if p is None else (cs["model"], cs["gen"], cs[p])
    return get


# ----------------------------------------------------------------------------- 1. the bits of mlp_scores
@pytest.mark.parametrize("c,n", SHAPES)
def test_same_bits_as_mlp_scores(L, ops, PM, cases, gpu_device, c, n):
    for p in SIZES + [SECOND_TRIP]:
        model, gen, cs = cases(c, n, p)
        h, t, z = cs["h"], cs["t"], cs["z"]
        assert z.shape == (p,) and z.dtype == torch.float32
        assert torch.equal(bits(z), bits(cs["want"])), p
        perm = torch.randperm(p, generator=gen).to(gpu_device)
        assert torch.equal(bits(L.score_pairs_mlp(model, h[perm], t[perm], logits=True)), bits(z[perm])), p
        for bs in ((1, 7, p) if p <= 4099 else (40_000,)):
            assert torch.equal(bits(L.score_pairs_mlp(model, h, t, logits=True, batch_size=bs)), bits(z)), (p, bs)
        assert torch.equal(bits(L.score_pairs_mlp(model, h, t)), bits(torch.sigmoid(z.double()).float())), p
        if p in (17, 257, 4099):               # both projection routes, forced, in every combination
            head = PM.fold_mlp_head(model)
            for uu in (True, False):
                for vu in (True, False):
                    u, u_idx = PM._pair_side(model.T, h, head.w1h, head.b1, unique=uu)
                    v, v_idx = PM._pair_side(model.T, t, head.w1t, None, unique=vu)
                    assert (u_idx is not None) == uu and (v_idx is not None) == vu
                    got, none = ops.pair_mlp_pairs(u, v, head.w2, head.b2, head.w3, head.b3, u_idx, v_idx)
                    assert none is None and torch.equal(bits(got), bits(z)), (p, uu, vu)
    # distinct ids: the gathered route is the one score_pairs_mlp takes by itself
    model, gen = cases(c, n)["model"], cases(c, n)["gen"]
    head = PM.fold_mlp_head(model)
    for p in (1, 17, n):
        h, t = (torch.randperm(n, generator=gen)[:p].to(gpu_device) for _ in range(2))
        assert PM._pair_side(model.T, h, head.w1h, head.b1)[1] is None
        z = L.score_pairs_mlp(model, h, t, logits=True)
        assert torch.equal(bits(z), bits(L.mlp_scores(model, h, t, logits=True).diagonal())), p


# ----------------------------------------------------------------------------- 2. float64, every logit
@pytest.mark.parametrize("c,n", SHAPES)
def test_every_logit_within_its_float64_bound(cases, c, n):
    for p in SIZES + [SECOND_TRIP]:
        model, gen, cs = cases(c, n, p)
        uh, hi = torch.unique(cs["h"], return_inverse=True)
        ut, ti = torch.unique(cs["t"], return_inverse=True)
        z64, e = ref64(model, uh, ut)
        err = (cs["z"].double() - z64[hi, ti]).abs()
        print(f"\n[C={c} P={p}] max |logit error| {float(err.max()):.3e}, max error / bound "
              f"{float((err / e[hi, ti]).max()):.3f}")
        assert bool((err <= e[hi, ti]).all()), p


# ----------------------------------------------------------------------------- 3. the counts of the stored logits
COUNT_KEYS = ("tp", "fp", "tn", "fn", "nan", "n", "n_pos", "n_neg")


def same_metrics(got, want, n_groups):
    assert set(got) == set(want)
    for k, w in want.items():
        g = got[k]
        if k == "average_precision" and not (isinstance(w, float) and math.isnan(w)):
            print(f"[ap] device {g!r}, exact {float(w)!r}, error {float(abs(Fraction(g) - w)):.3e}, "
                  f"bound {float((n_groups + 4) * Fraction(1, 2 ** 53) * w):.3e}")
            assert abs(Fraction(g) - w) <= (n_groups + 4) * Fraction(1, 2 ** 53) * w, (g, float(w))
        elif isinstance(w, float) and math.isnan(w):
            assert isinstance(g, float) and math.isnan(g), k
        else:
            assert g == w and (k not in COUNT_KEYS or isinstance(g, int)), (k, g, w)


@pytest.mark.parametrize("c,n,p", [(12, 50, 4099), (300, 500, 257)])
def test_counts_are_the_counts_of_the_stored_logits(L, ops, PM, cases, gpu_device, c, n, p):
    model, gen, cs = cases(c, n, p)
    h, t, z = cs["h"], cs["t"], cs["z"]
    zn = z.cpu().numpy()
    assert not np.isnan(zn).any()
    rand = torch.randint(0, 2, (p,), generator=gen)
    ones, zeros = torch.ones(p, dtype=torch.int64), torch.zeros(p, dtype=torch.int64)
    thresholds = [0.0, float(zn[5]), math.inf, -math.inf, float(zn.max()), float(zn.min())]
    for thr in thresholds:
        for y in (zeros, ones, rand):
            got = L.evaluate_mlp_classification(model, h, t, y.to(gpu_device), logit_threshold=thr)
            want = PC.confusion_counts(zn, y.numpy(), thr)
            assert (got["tp"], got["fp"], got["tn"], got["fn"], got["nan"]) == want, (thr, want)
            assert got["n"] == p and got["n_pos"] == int(y.sum()) and got["n_neg"] == p - int(y.sum())
    # a logit equal to the threshold is not positive
    one = L.evaluate_mlp_classification(model, h[5:6], t[5:6], torch.ones(1), logit_threshold=float(zn[5]))
    assert (one["tp"], one["fn"]) == (0, 1)
    # label types; batches
    base = L.evaluate_mlp_classification(model, h, t, rand.to(gpu_device), logit_threshold=float(np.median(zn)))
    assert min(base["tp"], base["fp"], base["tn"], base["fn"]) > 0
    for y in (rand.bool(), rand.to(torch.int32), rand, rand.float(), rand.bool().to(gpu_device)):
        for bs in (None, 7 if p < 1000 else 1000, p):
            got = L.evaluate_mlp_classification(model, h, t, y, logit_threshold=float(np.median(zn)), batch_size=bs)
            assert set(got) == set(base) and all(got[k] == base[k] for k in base), (y.dtype, bs)
    # the probability threshold is applied on the logit
    for prob in (0.5, 0.35):
        got = L.evaluate_mlp_classification(model, h, t, rand, threshold=prob)
        thr = struct.unpack("f", struct.pack("f", math.log(prob / (1.0 - prob))))[0]
        assert (got["tp"], got["fp"], got["tn"], got["fn"], got["nan"]) == PC.confusion_counts(zn, rand.numpy(), thr)
    # two calls on one counter add up
    head = PM.fold_mlp_head(model)
    u, u_idx = PM._pair_side(model.T, h, head.w1h, head.b1, unique=True)
    v, v_idx = PM._pair_side(model.T, t, head.w1t, None, unique=True)
    lab = rand.to(torch.uint8).to(gpu_device)
    counter = torch.zeros(5, dtype=torch.int64, device=gpu_device)
    cut = p // 3
    for lo, hi in ((0, cut), (cut, p)):
        zz, cc = ops.pair_mlp_pairs(u, v, head.w2, head.b2, head.w3, head.b3, u_idx[lo:hi], v_idx[lo:hi], lab[lo:hi], 0.0,
                                    want_logits=False, counts=counter)
        assert zz is None and cc is counter
    assert tuple(counter.tolist()) == PC.confusion_counts(zn, rand.numpy(), 0.0)
    zz, cc = ops.pair_mlp_pairs(u, v, head.w2, head.b2, head.w3, head.b3, u_idx, v_idx, lab, 0.0, counts=counter)
    assert torch.equal(bits(zz), bits(z)) and tuple(counter.tolist()) == tuple(2 * x for x in
                                                                                 PC.confusion_counts(zn, rand.numpy(), 0.0))
    with pytest.raises(ValueError):
        ops.pair_mlp_pairs(u, v, head.w2, head.b2, head.w3, head.b3, u_idx, v_idx, want_logits=False)
    with pytest.raises(ValueError):
        ops.pair_mlp_pairs(u, v, head.w2, head.b2, head.w3, head.b3, u_idx, v_idx, labels=lab)
    with pytest.raises(ValueError):
        ops.pair_mlp_pairs(u, v, head.w2, head.b2, head.w3, head.b3, u_idx, v_idx[:-1])


def test_a_nan_row_lands_exactly_its_pairs_in_nan(L, cases, gpu_device):
    c, n, p = 12, 50, 4099
    model, gen, cs = cases(c, n, p)
    h, t = cs["h"], cs["t"]
    row = int(h[0])
    table = model.T.clone()
    table[row] = math.nan
    sick = Model(table, {k: getattr(model, k) for k in HEAD})
    touched = ((h == row) | (t == row)).cpu().numpy()
    assert 0 < touched.sum() < p
    z = L.score_pairs_mlp(sick, h, t, logits=True)
    zn = z.cpu().numpy()
    assert np.array_equal(np.isnan(zn), touched)
    assert torch.equal(bits(z[~torch.from_numpy(touched).to(gpu_device)]),
                       bits(cs["z"][~torch.from_numpy(touched).to(gpu_device)]))
    y = torch.randint(0, 2, (p,), generator=gen)
    curve = PC.curve_reference(zn, y.numpy())
    want = PC.metrics_reference(zn, y.numpy(), 0.0, curve)
    for bs in (None, 100):
        got = L.evaluate_mlp_classification(sick, h, t, y, batch_size=bs)
        assert got["nan"] == int(touched.sum()) == want["nan"]
        same_metrics(got, want, curve[3])
        assert got["accuracy"] == (got["tp"] + got["tn"]) / p            # a NaN prediction is wrong


# ----------------------------------------------------------------------------- 4. the curve kernel, driven directly
NEG_NAN = np.array([0xFFC00001], dtype=np.uint32).view(np.float32)[0]


def curve_draws(rng, n):
    """(name, float32 scores, uint8 labels)"""
    y = rng.integers(0, 2, n).astype(np.uint8)
    normal = rng.standard_normal(n).astype(np.float32)
    yield "normal", normal, y
    yield "five values", rng.choice(np.array([-1.5, 0.0, 0.25, 2.0, 7.0], dtype=np.float32), n), y
    yield "all equal", np.full(n, 0.75, dtype=np.float32), y
    yield "only positives", normal, np.ones(n, dtype=np.uint8)
    yield "only negatives", normal, np.zeros(n, dtype=np.uint8)
    s = normal.copy()
    s[rng.random(n) < 0.2] = np.inf
    s[rng.random(n) < 0.2] = -np.inf
    yield "infinities", s, y
    neg = rng.random(n) < 0.5
    s = np.where(neg, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    yield "signed zeros, opposite labels", s, neg.astype(np.uint8)
    s = np.where(rng.random(n) < 0.3, normal, s).astype(np.float32)
    yield "signed zeros among others", s, y
    yield "subnormals", (rng.integers(-40, 41, n) * 2.0 ** -149).astype(np.float32), y
    s = normal.copy()
    s[rng.random(n) < 0.1] = np.nan
    s[rng.random(n) < 0.05] = NEG_NAN
    yield "planted NaNs", s, y
    yield "only NaNs", np.full(n, np.nan, dtype=np.float32), y


@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 2047, 2048, 2049, 4097, 70_001])
def test_binary_curve_kernel(ops, gpu_device, n):
    rng = np.random.default_rng(1000 + n)
    for name, s, y in curve_draws(rng, n):
        want = PC.curve_reference(s, y)
        st, yt = torch.from_numpy(s).to(gpu_device), torch.from_numpy(y).to(gpu_device)
        got = ops.binary_curve(st, yt)
        assert all(isinstance(x, int) for x in got[:5]) and isinstance(got[5], float)
        assert got[:5] == want[:5], (name, n, got, want[:5])
        assert got[0] + got[1] + got[2] == n
        err, bound = abs(Fraction(got[5]) - want[5]), (want[3] + 4) * Fraction(1, 2 ** 53) * want[5]
        print(f"[n={n} {name}] ap {got[5]!r} error {float(err):.3e} bound {float(bound):.3e} groups {want[3]}")
        assert err <= bound, (name, n)
        if want[0] == 0:
            assert got[5] == 0.0
        perm = torch.from_numpy(rng.permutation(n)).to(gpu_device)
        for again in (ops.binary_curve(st, yt), ops.binary_curve(st[perm], yt[perm]), ops.binary_curve(st, yt.bool())):
            assert again[:5] == got[:5] and struct.pack("d", again[5]) == struct.pack("d", got[5]), (name, n)
    with pytest.raises(ValueError):
        ops.binary_curve(torch.zeros(3, device=gpu_device), torch.zeros(4, dtype=torch.uint8, device=gpu_device))
    with pytest.raises(ValueError):
        ops.binary_curve(torch.zeros(3, device=gpu_device).double(), torch.zeros(3, dtype=torch.uint8, device=gpu_device))


# ----------------------------------------------------------------------------- 5. end to end
@pytest.mark.parametrize("c,n,p", [(12, 50, 4099), (300, 500, 4099), (300, 500, SECOND_TRIP)])
def test_evaluate_equals_the_references_on_the_stored_logits(L, cases, gpu_device, c, n, p):
    model, gen, cs = cases(c, n, p)
    h, t, z = cs["h"], cs["t"], cs["z"]
    # every pair twice, the copy with the opposite label: exact ties (test 1) that enter auc2 as halves
    y = torch.randint(0, 2, (p,), generator=gen)
    hh, tt, yy = torch.cat([h, h]), torch.cat([t, t]), torch.cat([y, 1 - y])
    zn, z1 = torch.cat([z, z]).cpu().numpy(), z.cpu().numpy()
    curve = PC.curve_reference(zn, yy.numpy())
    assert curve[3] <= p and curve[4] == p * p              # the copies tie: every positive's own copy counts as a half
    choices = ((dict(), 0.0), (dict(threshold=0.7), struct.unpack("f", struct.pack("f", math.log(0.7 / (1.0 - 0.7))))[0]),
               (dict(logit_threshold=float(np.median(zn))), float(np.median(zn))))
    for thr_kw, thr in choices[:1 if p > 10_000 else 3]:
        got = L.evaluate_mlp_classification(model, hh, tt, yy.to(gpu_device), **thr_kw)
        same_metrics(got, PC.metrics_reference(zn, yy.numpy(), thr, curve), curve[3])
        assert got["roc_auc"] == 0.5 and got["n_pos"] == p == got["n_neg"]
    if p > 10_000:
        return
    curve = PC.curve_reference(z1, y.numpy())
    got = L.evaluate_mlp_classification(model, h, t, y.bool(), batch_size=1000)
    same_metrics(got, PC.metrics_reference(z1, y.numpy(), 0.0, curve), curve[3])
    assert 0.0 < got["roc_auc"] < 1.0 and 0.0 < got["average_precision"] <= 1.0
    # an empty class: the curve metrics are NaN, the rest stays defined
    for fill in (0, 1):
        y1 = torch.full((p,), fill, dtype=torch.int64)
        got = L.evaluate_mlp_classification(model, h, t, y1)
        assert math.isnan(got["roc_auc"]) and math.isnan(got["average_precision"])
        same_metrics(got, PC.metrics_reference(z1, y1.numpy(), 0.0), 0)
        assert got["accuracy"] == (got["tp"] + got["tn"]) / p and got["n_pos"] == fill * p


# ----------------------------------------------------------------------------- 6. agreement with mode='mlp'
@pytest.mark.parametrize("name", ["mlp_bce_gcn_l2_scale", "mlp_model_gcn_l1_scale"])
def test_decisions_agree_with_mode_mlp_where_float64_is_clear(L, gpu_device, name):
    """On the pairs whose float64 logit is further from 0 than the bounds of both routes together, the decision is
    model(h, t, mode='mlp').round().  The share of such pairs was computed beforehand on the CPU from the float64
    reference alone (the oracle's table, ref64 and eager_bound; 600 pairs of seed 6): 0.993 with 69 % positives for
    mlp_bce_gcn_l2_scale, 1.0 (all negative) for mlp_model_gcn_l1_scale -- the fixtures' own heads, no redraw needed."""
    m, gd = _golden_mlp_model(L, name, gpu_device)
    n = m.n_entities
    gen = torch.Generator().manual_seed(6)
    hs, ts = (torch.randint(0, n, (600,), generator=gen).to(gpu_device) for _ in range(2))
    with torch.no_grad():
        eager = m(hs, ts, device=gpu_device, mode="mlp").reshape(-1)
        table = m._table_for_inference().detach()
    uh, hi = torch.unique(hs, return_inverse=True)
    ut, ti = torch.unique(ts, return_inverse=True)
    z64, e_fused = ref64(m, uh, ut)
    z64, e_fused = z64[hi, ti], e_fused[hi, ti]
    zz, e_eager = eager_bound(m, table.double(), hs, ts)
    assert float((zz - z64).abs().max()) < 1e-12
    clear = z64.abs() > e_fused + e_eager
    print(f"\n[{name}] clear pairs {int(clear.sum())} of 600, positive among them {int((z64[clear] > 0).sum())}")
    assert int(clear.sum()) >= 300
    z = m.score_pairs(hs, ts, logits=True)
    assert torch.equal(bits(z), bits(L.score_pairs_mlp(m, hs, ts, logits=True)))
    assert torch.equal((z > 0)[clear], eager.round().bool()[clear])
    assert torch.equal((z > 0)[clear], (z64 > 0)[clear])
    got = L.evaluate_mlp_classification(m, hs[clear], ts[clear], eager.round()[clear])      # the kernel's own compare
    assert got["fp"] == got["fn"] == got["nan"] == 0 and got["accuracy"] == 1.0
    assert got["tp"] == int((z64[clear] > 0).sum()) and got["tn"] == int(clear.sum()) - got["tp"]
    np.testing.assert_allclose(m.score_pairs(hs, ts).cpu().numpy(), eager.cpu().numpy(), rtol=1e-4, atol=1e-5)


# ----------------------------------------------------------------------------- 7. the model's state is untouched
@pytest.mark.parametrize("training", [False, True])
def test_model_state_untouched(L, gpu_device, training):
    m, gd = _golden_mlp_model(L, "mlp_model_gcn_l1_scale", gpu_device)
    heads, tails = (torch.from_numpy(gd[k]).to(gpu_device) for k in ("heads", "tails"))
    labels = torch.from_numpy(gd["labels"]).to(gpu_device)
    with torch.no_grad():
        m._table_for_inference()
    want_z = m.score_pairs(heads, tails, logits=True)
    want_d = L.evaluate_mlp_classification(m, heads, tails, labels, threshold=0.48)
    m.train(training)
    cache = m.__dict__.get("_eval_cache")
    assert (cache is None) == training
    before = {k: (v, v._version, v.detach().clone()) for k, v in list(m.named_parameters()) + list(m.named_buffers())
              if not v.is_sparse}
    assert "norm1.num_batches_tracked" in before and "norm2.running_var" in before
    z = m.score_pairs(heads, tails, logits=True)
    p = L.score_pairs_mlp(m, heads, tails, batch_size=10)
    d = L.evaluate_mlp_classification(m, heads, tails, labels, threshold=0.48)
    assert m.training == training
    for mod in (m.norm1, m.norm2, m.fc1):
        assert mod.training == training
    assert m.__dict__.get("_eval_cache") is cache
    after = dict(list(m.named_parameters()) + list(m.named_buffers()))
    for k, (v, ver, val) in before.items():
        assert after[k] is v and v._version == ver and torch.equal(v.detach(), val), k
    # the same results in both modes: the running statistics are what is used.  (In training mode the table itself comes
    # from the encoder's training pass, which owes the eval pass no bits: score_pairs is compared within 1e-5 there.)
    assert torch.equal(bits(p), bits(torch.sigmoid(z.double()).float()))
    if training:
        np.testing.assert_allclose(z.cpu().numpy(), want_z.cpu().numpy(), rtol=1e-4, atol=1e-5)
    else:
        assert torch.equal(bits(z), bits(want_z))
    assert set(d) == set(want_d)
    for k in d:
        assert d[k] == want_d[k] or (math.isnan(d[k]) and math.isnan(want_d[k])), k
    assert d["n"] == 96 and d["nan"] == 0
    np.testing.assert_allclose(p.cpu().numpy(), gd["out_eval"], rtol=1e-4, atol=1e-5)       # the reference's own numbers
