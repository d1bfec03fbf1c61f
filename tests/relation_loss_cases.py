"""Draws, float64 references, measures, bounds and planted faults of the relation-slot loss (lkg_relation_loss.hip,
literalkg_amd/relation_loss.py), shared by test_relation_loss_host.py (on the CPU: the checks accept a float32 restatement
of the kernels' steps and reject planted faults), test_relation_loss_gpu.py and test_relation_loss_model_gpu.py.

Contract (include/literalkg_hip.h): P pairs, R relations, blocks of D columns.  A slab u3[P, R, D] holds
u_ij = d_i W_j (slab mode) or d_i for every j (shared mode); s_ij = sum_c (u_ijc + e_jc)^2, z_ij = -scale s_ij, a dropped
relation (mask[i, j]; never the truth) has z_ij = -inf, loss_i = logsumexp_j z_ij - z_i,t_i.  Gradient: c_ij =
-2 scale g_i (softmax_ij - [j == t_i]), G_ij = c_ij (u_ij + e_j); shared mode gd_i = sum_j G_ij; the whole op
dd = sum_j G_ij W_j^T, dW_j = sum_i d_i^T G_ij, de_j = sum_i G_ij.

Measures.  The loss per pair r = |L - L64| / (|lse64| + |z_t|) against loss_bound = max(3 r_torch32, N_loss u); a gradient
per element r = |got - x64| / (the |.|-sum of the element's terms, with |softmax| + [j == t] for the coefficient's
difference and |u| + |e| for the block's sum) against grad_bound = max(3 r_torch32, N_grad u), u = 2^-24, r_torch32 the
same quantity evaluated by float32 torch, on exact-logit cases: small-integer d, W, e and a power-of-two scale, so that
d W + e, s and z are exact in float32 and the argument of every exponential is exact.  exact_case also makes every
|z_ij| >= 1, so that |lse64| + |z_t| >= 1 and a rounding that is absolute (the additions of the sum of exponentials, whose
result lies in [1, R]) is no more than that many u of the measure's denominator.

The counts N, from the kernels' own expressions (expf and logf within 1 ulp = 2 u each, every other operation u; as
DESIGN 3.6p counts, the conditioning of an exponential's argument is NOT counted: it is what 3 r_torch32 carries).  A sum
over the R relations runs over a lane's ceil(R / 64) entries in order and then six butterfly steps: at most
d(R) = ceil(R / 64) - 1 + 6 additions deep.  A logit (not exact on general inputs): the sum u + e 1, its square 2, a
lane's chain of 4 ceil(ceil(D / 4) / 64) fmas and six butterfly steps, the product with scale 1: zN(D).
  lse = m + logf(sum):        expf 2, the additions d, logf 2, the addition 1                                    = 5 + d
  loss = (m - z_t) + logf(sum): the same with the difference m - z_t 1, and twice a logit's own roundings (the truth's
                              and the softmax-weighted mean of the others')                               = 6 + d + 2 zN
  c = cg (expf(z - m) / sum - [j == t]): the numerator 3 (the difference, expf), the denominator 3 + d, the quotient 1,
                              the one-hot 1, cg 1, the product 1                                                  = 10 + d
  a G element c (u + e):      the sum 1, the product 1                                                            = 12 + d
  a gd element:               its R terms as G's, added in increasing j (the first addition to zero is exact)  = 11 + d + R
"""
import math

import torch

import self_adversarial_cases as S
import softmax_cases as C

U = C.U
FAULTS_LOSS = ("mask_ignored", "truth_masked", "scale_ignored", "e_not_added", "next_relation")
FAULTS_GRAD = FAULTS_LOSS + ("no_onehot",)
MAX_SPREAD = 60.0

PS = (1, 2, 5, 33)
RS = (1, 2, 3, 64, 65, 130)
DS = (1, 3, 4, 17, 64, 300, 600)
CS = ("D", 5, 300)                  # slab mode: the width of d (the table), "D" = as wide as the blocks
ALIGNED = (True, False)
FILTERED = (True, False)

# (P, R, D, C, aligned, filtered): slab mode
SLAB_CASES = S._pairwise_cover((PS, RS, DS, CS, ALIGNED, FILTERED))
# (P, R, D, aligned, filtered): shared mode
SHARED_CASES = S._pairwise_cover((PS, RS, DS, ALIGNED, FILTERED))


def slab_id(case) -> str:
    p, r, d, c, aligned, filtered = case
    return f"P{p}-R{r}-D{d}-C{c}-{'aligned' if aligned else 'scalar'}-{'filtered' if filtered else 'all'}"


def shared_id(case) -> str:
    p, r, d, aligned, filtered = case
    return f"P{p}-R{r}-D{d}-{'aligned' if aligned else 'scalar'}-{'filtered' if filtered else 'all'}"


def width_of(c, d: int) -> int:
    return d if c == "D" else int(c)


# ----------------------------------------------------------------------------- draws
def random_mask(p: int, n_rel: int, truth: torch.Tensor, gen, rate: float = 0.3) -> torch.Tensor:
    """bool[P, R]: the relations dropped per pair, never the truth; pair 0 (R > 1) drops every relation but its truth and
    the last pair drops none"""
    mask = torch.rand((p, n_rel), generator=gen) < rate
    mask[0] = True
    if p > 1:
        mask[-1] = False
    mask[torch.arange(p), truth] = False
    return mask


def exact_case(p: int, n_rel: int, k: int, c, seed: int, filtered: bool = False):
    """dict(d[P, C], w[R, C, D] or None (c None: shared mode), e[R, D], truth[P], mask[P, R] or None, scale): small
    integers -- d and e in [-2, 2], every column of a W_j with at most two entries +-1 -- so that d W + e (|.| <= 6 + the
    offset below) and s are exact in float32, and a power-of-two scale <= 1 chosen from the draw so that the spread
    scale (max s - min s) over a pair's relations is at most 32 before the offset and, asserted, <= MAX_SPREAD after.
    Column 0 carries the offset that makes every |z| >= 1: d (shared) or W (slab) is zero there and e[:, 0] = +-(q + b)
    with q = ceil(scale^-1/2), b in {0, 1}."""
    gen = torch.Generator().manual_seed(seed)
    shared = c is None
    cw = k if shared else width_of(c, k)
    d = torch.randint(-2, 3, (p, cw), generator=gen).float()
    e = torch.randint(-2, 3, (n_rel, k), generator=gen).float()
    w = None
    if shared:
        d[:, 0] = 0.0
    else:
        w = torch.zeros((n_rel, cw, k))
        rows = torch.randint(0, cw, (n_rel, 2, k), generator=gen)
        sign = (torch.randint(0, 2, (n_rel, 2, k), generator=gen) * 2 - 1).float()
        for a in range(2):
            w.scatter_(1, rows[:, a:a + 1], sign[:, a:a + 1])           # (a second hit on the same row overwrites: still +-1)
        w[:, :, 0] = 0.0
    e[:, 0] = 0.0
    s = score(slab_of(d, w, n_rel), e)
    spread = float((s.max(1).values - s.min(1).values).max())
    scale = 1.0 if spread <= 32.0 else 2.0 ** math.floor(math.log2(32.0 / spread))
    q = math.ceil(scale ** -0.5)
    e[:, 0] = (torch.randint(0, 2, (n_rel,), generator=gen) * 2 - 1).float() * \
        (q + torch.randint(0, 2, (n_rel,), generator=gen)).float()
    truth = torch.randint(0, n_rel, (p,), generator=gen)
    if p >= 2:
        truth[0], truth[1] = 0, n_rel - 1
    mask = random_mask(p, n_rel, truth, gen) if filtered else None
    s = score(slab_of(d, w, n_rel), e)
    assert float(s.max()) < 2.0 ** 24 and float(scale * s.min()) >= 1.0, (p, n_rel, k, c)
    s_hi = s.clone() if mask is None else s.masked_fill(mask, -math.inf)
    s_lo = s.clone() if mask is None else s.masked_fill(mask, math.inf)
    spread = scale * float((s_hi.max(1).values - s_lo.min(1).values).max())
    assert spread <= MAX_SPREAD, (p, n_rel, k, c, spread)
    return dict(d=d, w=w, e=e, truth=truth, mask=mask, scale=scale)


def random_case(p: int, n_rel: int, k: int, c, seed: int, filtered: bool = False, std: float = 0.5):
    """the same dict with random rows, scale 0.37, and the upstream gradient g in [0.5, 1.5)"""
    gen = torch.Generator().manual_seed(seed)
    shared = c is None
    cw = k if shared else width_of(c, k)
    d = torch.randn((p, cw), generator=gen) * std
    e = torch.randn((n_rel, k), generator=gen) * std
    w = None if shared else torch.randn((n_rel, cw, k), generator=gen) * (std / math.sqrt(cw))
    truth = torch.randint(0, n_rel, (p,), generator=gen)
    mask = random_mask(p, n_rel, truth, gen) if filtered else None
    return dict(d=d, w=w, e=e, truth=truth, mask=mask, scale=0.37, g=torch.rand((p,), generator=gen) + 0.5)


def upstream(p: int, seed: int) -> torch.Tensor:
    return torch.rand((p,), generator=torch.Generator().manual_seed(seed)) + 0.5


# ----------------------------------------------------------------------------- the filter
def dropped_mask(kh, kr, kt, h, r, t, n_rel: int) -> torch.Tensor:
    """bool[P, R]: mask[i, j] = (h_i, j, t_i) is among the known triples (kh, kr, kt) and j != r_i -- rank_relations' rule,
    vectorised; duplicates among the known triples change nothing"""
    hit = (kh[None, :] == h[:, None]) & (kt[None, :] == t[:, None])             # [P, K]
    mask = torch.zeros((h.numel(), n_rel), dtype=torch.bool)
    at = hit.nonzero()
    mask[at[:, 0], kr[at[:, 1]]] = True
    mask[torch.arange(h.numel()), r] = False
    return mask


def triples_of_mask(mask, truth, n_entities_offset: int = 0):
    """(kh, kr, kt, h, t): pair i is (h_i, t_i) = (2 i, 2 i + 1) (+ offset), known under every dropped relation, every
    second pair also under its truth (the truth is exempt), the first dropped triple listed twice (a duplicate)"""
    p = mask.shape[0]
    h = torch.arange(p) * 2 + n_entities_offset
    t = h + 1
    at = mask.nonzero()
    kh, kr, kt = h[at[:, 0]], at[:, 1].clone(), t[at[:, 0]]
    own = torch.arange(0, p, 2)
    kh, kr, kt = torch.cat((kh, h[own], kh[:1])), torch.cat((kr, truth[own], kr[:1])), torch.cat((kt, t[own], kt[:1]))
    return kh, kr, kt, h, t


def tails_around(h, t, n_entities: int):
    """(kh, kt): rows that are not empty and do not hold (h_i, t_i).  Every row h_i holds the tail h_i (< t_i: the row's
    last entry lies below the wanted one) and every second row also t_i + 1 where that is an entity (an entry above it)."""
    up = t[::2] + 1
    ok = up < n_entities
    return torch.cat((h, h[::2][ok])), torch.cat((h, up[ok]))


# ----------------------------------------------------------------------------- references
def slab_of(d, w, n_rel: int, dtype=torch.float64):
    """u3[P, R, D] in dtype: d_i W_j, or d_i for every j without w"""
    d = d.to(dtype)
    if w is None:
        return d[:, None, :].expand(d.shape[0], n_rel, d.shape[1])
    return torch.einsum("pc,rcd->prd", d, w.to(dtype))


def score(u3, e, dtype=torch.float64):
    return ((u3.to(dtype) + e.to(dtype)[None]) ** 2).sum(2)


def _faulty(u3, e, mask, truth, scale, fault):
    """the operands the planted fault sees"""
    if fault == "mask_ignored":
        mask = None
    if fault == "scale_ignored":
        scale = 1.0
    if fault == "e_not_added":
        e = torch.zeros_like(e)
    if fault == "next_relation":                       # relation j reading relation j + 1's block (shared mode: its e row)
        if bool((u3[:, :1] == u3).all()):
            e = torch.roll(e, -1, dims=0)
        else:
            u3 = torch.roll(u3, -1, dims=1)
    return u3, e, mask, scale


def logits(u3, e, truth, mask, scale: float, dtype=torch.float64, fault=None):
    """z[P, R] in dtype, -inf where dropped"""
    u3, e, mask, scale = _faulty(u3, e, mask, truth, scale, fault)
    z = -scale * score(u3, e, dtype)
    if mask is not None:
        z = z.masked_fill(mask.to(z.device), -math.inf)
    if fault == "truth_masked":
        z = z.clone()
        z[torch.arange(z.shape[0]), truth] = -math.inf
    return z


def loss_eval(u3, e, truth, mask, scale: float, dtype=torch.float64, fault=None):
    """(lse, z_t, loss) in dtype.  float64: the reference; float32, fault None: torch's evaluation (r_torch32)."""
    z = logits(u3, e, truth, mask, scale, dtype, fault)
    zt = -scale * score(u3, e, dtype).gather(1, truth.to(z.device)[:, None])[:, 0] if fault == "truth_masked" else \
        z.gather(1, truth.to(z.device)[:, None])[:, 0]
    lse = torch.logsumexp(z, dim=1)
    return lse, zt, lse - zt


def loss_measure(loss, ref):
    """r per pair against ref = (lse64, zt64, loss64); 0 / 0 = 0 (a loss that is exactly right), NaN / inf count as inf"""
    lse64, zt64, loss64 = (x.cpu() for x in ref)
    diff = (loss.double().cpu() - loss64).abs()
    r = torch.where(diff == 0, torch.zeros_like(diff), diff / (lse64.abs() + zt64.abs()).clamp_min(1e-300))
    return torch.nan_to_num(r, nan=math.inf)


def grads_eval(u3, d, w, e, truth, mask, scale: float, g, dtype=torch.float64, fault=None):
    """dict(c, G, gd, dd, dw, de and their scales) in dtype from the contract's closed form.  u3: the slab the kernels are
    given (d and w may be None then: only c, G and gd come out)."""
    z = logits(u3, e, truth, mask, scale, dtype, fault)
    u3, e_, _, scale_ = _faulty(u3, e, mask, truth, scale, fault)
    soft = torch.softmax(z, dim=1)
    hot = torch.zeros_like(soft)
    if fault != "no_onehot":
        hot[torch.arange(z.shape[0]), truth.to(z.device)] = 1.0
    gq = g.to(dtype)[:, None]
    c = -2.0 * scale_ * gq * (soft - hot)
    c_scale = 2.0 * scale_ * gq.abs() * (soft + hot)
    b = u3.to(dtype) + e_.to(dtype)[None]
    b_scale = u3.to(dtype).abs() + e_.to(dtype).abs()[None]
    big, big_scale = c[:, :, None] * b, c_scale[:, :, None] * b_scale
    out = dict(c=c, c_scale=c_scale, G=big, G_scale=big_scale, gd=big.sum(1), gd_scale=big_scale.sum(1),
               de=big.sum(0), de_scale=big_scale.sum(0))
    if w is not None:
        w_, d_ = w.to(dtype), d.to(dtype)
        out.update(dd=torch.einsum("prd,rcd->pc", big, w_), dd_scale=torch.einsum("prd,rcd->pc", big_scale, w_.abs()),
                   dw=torch.einsum("pc,prd->rcd", d_, big), dw_scale=torch.einsum("pc,prd->rcd", d_.abs(), big_scale))
    else:
        out.update(dd=out["gd"], dd_scale=out["gd_scale"])
    return out


def autograd_eval(d, w, e, truth, mask, scale: float, g, dtype):
    """(dd, dw or None, de) of sum_i g_i loss_i by torch autograd in dtype on the operands' device: the dense head
    (einsum, squared norm, masked cross_entropy)"""
    d_ = d.detach().to(dtype).requires_grad_(True)
    e_ = e.detach().to(dtype).requires_grad_(True)
    w_ = None if w is None else w.detach().to(dtype).requires_grad_(True)
    u3 = d_[:, None, :] if w_ is None else torch.einsum("pc,rcd->prd", d_, w_)
    z = -scale * ((u3 + e_[None]) ** 2).sum(2)
    if mask is not None:
        z = z.masked_fill(mask.to(z.device), -math.inf)
    loss = torch.nn.functional.cross_entropy(z, truth.to(z.device), reduction="none")
    (loss * g.to(dtype)).sum().backward()
    return d_.grad, None if w_ is None else w_.grad, e_.grad


# ----------------------------------------------------------------------------- bounds
def depth(n_rel: int) -> int:
    """additions deep of a sum over R relations: a lane's ceil(R / 64) entries in order, six butterfly steps"""
    return (n_rel + 63) // 64 - 1 + 6


def logit_roundings(k: int) -> int:
    return 1 + 2 + 4 * (((k + 3) // 4 + 63) // 64) + 6 + 1


def loss_roundings(n_rel: int, k: int) -> int:
    return 6 + depth(n_rel) + 2 * logit_roundings(k)


def grad_roundings(n_rel: int, k: int, name: str) -> int:
    n = 10 + depth(n_rel)
    return {"c": n, "G": n + 2, "gd": n + 1 + n_rel}[name]


def loss_bound(r_torch32: float, n_rel: int, k: int) -> float:
    return max(3.0 * r_torch32, loss_roundings(n_rel, k) * U)


def grad_bound(r_torch32: float, n_rel: int, k: int, name: str) -> float:
    return max(3.0 * r_torch32, grad_roundings(n_rel, k, name) * U)


# ----------------------------------------------------------------------------- the kernels' steps in float32 torch
def _fma(a, b, c):
    """fl(a b + c) of float32 operands: the product is exact in float64, the sum rounded once to float64 and once more to
    float32 (a double rounding differs from the fused one only on a tie of the second)"""
    return (a.double() * b.double() + c.double()).float()


def kernel_scores(u3, e):
    """s[P, R] in float32 by the kernel's steps: lane l adds the 4-column units l, l + 64, ... as ONE fma chain over
    (u + e)^2 in column order, then a butterfly over the 64 lanes"""
    p, n_rel, k = u3.shape
    b = u3.float() + e.float()[None]
    turns = ((k + 3) // 4 + 63) // 64
    b = torch.cat((b, torch.zeros((p, n_rel, turns * 256 - k))), dim=2).view(p, n_rel, turns, 64, 4)
    acc = torch.zeros((p, n_rel, 64))
    for t in range(turns):
        for col in range(4):
            acc = _fma(b[:, :, t, :, col], b[:, :, t, :, col], acc)
    while acc.shape[2] > 1:
        acc = acc[:, :, 0::2] + acc[:, :, 1::2]
    return acc[:, :, 0]


def kernel_loss_eval(u3, e, truth, mask, scale: float):
    """(loss, z, lse) in float32 by the forward kernel's steps"""
    z = -(torch.tensor(scale, dtype=torch.float32) * kernel_scores(u3, e))
    if mask is not None:
        z = z.masked_fill(mask, -math.inf)
    m = z.max(1).values
    zt = z.gather(1, truth[:, None])[:, 0]
    lg = torch.log(S._lane_sum(torch.exp(z - m[:, None])))
    return (m - zt) + lg, z, m + lg


def kernel_grads_eval(u3, e, truth, mask, scale: float, g):
    """dict(c, G, gd) in float32 by the backward kernels' steps: cg = fl(-2 scale g), c = cg (expf(z - m) / sum - [j == t])
    with the forward's m and sum, exactly 0 where dropped; G = c (u + e) (zeros where dropped); gd adds its terms in
    increasing j"""
    _, z, _ = kernel_loss_eval(u3, e, truth, mask, scale)
    m = z.max(1).values
    soft = torch.exp(z - m[:, None]) / S._lane_sum(torch.exp(z - m[:, None]))[:, None]
    hot = torch.zeros_like(z)
    hot[torch.arange(z.shape[0]), truth] = 1.0
    cg = torch.tensor(-2.0 * scale, dtype=torch.float32) * g.float()
    dropped = z == -math.inf
    c = torch.where(dropped, torch.zeros_like(z), cg[:, None] * (soft - hot))
    big = torch.where(dropped[:, :, None], torch.zeros(()), c[:, :, None] * (u3.float() + e.float()[None]))
    gd = torch.zeros((z.shape[0], u3.shape[2]))
    for j in range(z.shape[1]):
        gd = gd + big[:, j]
    return dict(c=c, G=big, gd=gd)
