"""Draws, list patterns, float64 references, measures and bounds of the KvsAll loss (lkg_kvsall.hip,
literalkg_amd/kvs_all.py), shared by test_kvs_all_host.py (on the CPU: the checks accept a float32 restatement of the
kernel's algorithm and reject planted faults), test_kvs_all_gpu.py and test_kvs_all_surface_gpu.py.

Contract (include/literalkg_hip.h): s_ic = |p_c|^2 - 2 q_i.p_c (dot: -2 q_i.p_c), z_ic = -scale beta s_ic + bias_i with
beta = 1 (distance) or 1/2 (dot), L_i = sum_c softplus(z_ic) - y'_ic z_ic, y' = (1 - eps) y + eps / n;
V_ic = scale beta g_i (sigma(z_ic) - y'_ic), dQ = 2 V P, dP = 2 V^T Q - 2 diag(colsum V) P (the second term with distance
only), dbias = rowsum(V) / (scale beta) = g_i sum_c (sigma - y').  bias is an input of its own: dQ holds no term of it.

Measures: the loss per query r = |L - L64| / sum_c |term64_c| against softmax_cases.loss_bound(r_torch32) = max(3 r_torch32,
3e-7), r_torch32 the same expression evaluated by float32 torch, on tables whose logits are exact in float32 (integer
entries, integer margin, power-of-two scale); a gradient per element r = |got - x64| / (the |.|-sum of the float64
expression's terms) against the bound of the engine that ran the product (softmax_cases.gemm_bound); dbias, which no
product computes (the weights kernel adds its own row sums), against dbias_bound."""
import math

import torch

import softmax_cases as C

TILE = 256
N_PATTERNS = 10
FAULTS_LOSS = ("positives_ignored", "lists_shifted", "bias_dropped", "smoothing_sign")
FAULTS_GRAD = ("weights_without_positives", "dbias_dropped")
SHAPES = [(1, 1, 1), (65, 257, 17), (130, 255, 32), (130, 1000, 300), (65, 70001, 17)]


# ----------------------------------------------------------------------------- the lists
def pattern(j: int, n: int, gen) -> list:
    if j == 0:
        return []                                                   # an empty row
    if j == 1:
        return [0]                                                  # position 0
    if j == 2:
        return [n - 1]                                              # position n - 1
    if j == 3:
        return [63, 64, 255, 256]                                   # wave and tile edges
    if j == 4:
        return list(range(64, 128))                                 # a whole wave's 64 columns
    if j == 5:
        return list(range(256, 512))                                # a whole 256-column tile
    if j == 6:
        return list(range(n // 2 - 600, n // 2 + 600))              # a run across tile (and split) boundaries
    if j == 7:
        return list(range(n))                                       # every candidate a positive
    if j == 8:
        return torch.nonzero(torch.rand(n, generator=gen) < 0.5)[:, 0].tolist()      # a long list ...
    return torch.randint(0, n, (5,), generator=gen).tolist()        # ... next to a short one (and the empty row 0)


def patterns(b: int, n: int, seed: int, offset: int = 0) -> list:
    """per row the sorted, duplicate-free positive positions in [0, n): row i gets pattern (i + offset) mod N_PATTERNS"""
    gen = torch.Generator().manual_seed(seed)
    return [sorted({c for c in pattern((i + offset) % N_PATTERNS, n, gen) if 0 <= c < n}) for i in range(b)]


def to_lists(rows: list, device="cpu"):
    """(yptr int32[B + 1], ycol int32[M]) of per-row lists"""
    yptr = [0]
    for row in rows:
        yptr.append(yptr[-1] + len(row))
    ycol = [c for row in rows for c in row]
    return (torch.tensor(yptr, dtype=torch.int32, device=device), torch.tensor(ycol, dtype=torch.int32, device=device))


def mask_of(rows: list, n: int, device="cpu") -> torch.Tensor:
    """bool[B, n]: True where the candidate is a positive of the row"""
    m = torch.zeros((len(rows), n), dtype=torch.bool)
    for i, row in enumerate(rows):
        if row:
            m[i, torch.tensor(row)] = True
    return m.to(device)


# ----------------------------------------------------------------------------- exact-logit draws
def exact_case(b: int, n: int, k: int, distance: bool, seed: int):
    """(q, p, bias, scale): integer tables, an integer margin (4 k with a distance: the middle of ||q - p||^2, so the
    sigmoids are in their active range; 1 with dot) and a power-of-two scale -- bias = scale (margin - ||q||^2), or
    scale margin, and every logit are exact in float32"""
    q, p, _ = C.integer_tables(b, n, k, seed)
    scale = C.exact_scale(k)
    if distance:
        bias = scale * (4.0 * k - (q * q).sum(1))
    else:
        bias = torch.full((b,), scale * 1.0)
    return q, p, bias.float(), scale


def random_case(b: int, n: int, k: int, seed: int, std: float = 0.5):
    """(q, p, bias, g): random tables, a bias that centres the logits, upstream gradients in [0.5, 1.5)"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn((b, k), generator=gen) * std
    p = torch.randn((n, k), generator=gen) * std
    bias = torch.randn((b,), generator=gen) * 0.5 + 2.0 * k * std * std
    return q, p, bias, torch.rand((b,), generator=gen) + 0.5


# ----------------------------------------------------------------------------- references
def logits(q, p, bias, distance: bool, scale: float, dtype=torch.float64):
    z = C.logits(q, p, distance, scale, dtype)
    return z if bias is None else z + bias.to(dtype)[:, None]


def softplus(x):
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def smoothing(eps: float, n: int):
    """(ce_1, ce_0): the coefficients of z in a positive's and in a negative's term"""
    return eps * (1.0 - 1.0 / n), -eps / n


def terms_eval(z, mask, eps: float):
    """softplus(z) - y' z per element, each without cancellation (the contract's form)"""
    ce1, ce0 = smoothing(eps, z.shape[1])
    t = softplus(torch.where(mask, -z, z))
    if eps > 0:
        t = t + torch.where(mask, torch.full_like(z, ce1), torch.full_like(z, ce0)) * z
    return t


def loss_eval(q, p, bias, mask, distance: bool, scale: float, eps: float, dtype=torch.float64, fault=None):
    """(loss, denom) in dtype: the row sums of the terms and of their magnitudes.  float64: the reference; float32, fault
    None: torch's evaluation (r_torch32).  Faults (FAULTS_LOSS) are the mistakes the checks must reject."""
    if fault == "positives_ignored":
        mask = torch.zeros_like(mask)
    if fault == "lists_shifted":
        mask = torch.roll(mask, 1, dims=1)
    z = logits(q, p, None if fault == "bias_dropped" else bias, distance, scale, dtype)
    t = _wrong_sign_terms(z, mask, eps) if fault == "smoothing_sign" else terms_eval(z, mask, eps)
    return t.sum(1), t.abs().sum(1)


def _wrong_sign_terms(z, mask, eps):
    ce1, ce0 = smoothing(eps, z.shape[1])
    return softplus(torch.where(mask, -z, z)) - torch.where(mask, torch.full_like(z, ce1), torch.full_like(z, ce0)) * z


def loss_measure(loss, ref):
    """r per query against the float64 reference ref = (loss64, denom64); a NaN / inf difference counts as inf"""
    loss64, denom64 = ref
    r = (loss.double().cpu() - loss64.cpu()).abs() / (denom64.cpu() + 1e-300)
    return torch.nan_to_num(r, nan=math.inf)


def dbias_bound(r_torch32: float) -> float:
    """dbias = rowsum(V) / (scale beta) relative to g sum_c |sigma - y'|.  A stored weight carries at most 7 roundings of
    u = 2^-24 (expf within 1 ulp = 2 u, 1 + e, the quotient, the sum with ce, scale beta g, the product), the row sum is a
    tree 9 float32 additions deep (2 in a lane, 4 over the row's 16 lanes, 3 over the waves) before it continues in
    float64: 16 u.  On top comes what the rounding of the float32 logits themselves brings, which torch's float32
    evaluation carries as well: 3 r_torch32, as for the loss."""
    return 3.0 * r_torch32 + 16.0 * C.U


def tiled_eval(q, p, bias, mask, distance: bool, scale: float, eps: float, splits: int = 1):
    """The kernel's algorithm in float32 torch: z = fl(fl(nsb s) + bias); 256-wide tiles, a wave's 64 columns as 4 x 16;
    per (wave, lane of the row) one running float32 sum that takes the tile's 4 terms added as (t0 + t1) + (t2 + t3); a
    tree over the 16 lanes, the 4 waves in order, the splits in order in float64, rounded once."""
    b, n = q.shape[0], p.shape[0]
    z = C.logits(q, p, distance, scale, torch.float32)
    z = z + bias[:, None] if bias is not None else z
    ce1, ce0 = (torch.tensor(c, dtype=torch.float64).float() for c in smoothing(eps, n))
    t = softplus(torch.where(mask, -z, z))
    if eps > 0:
        t = t + torch.where(mask, ce1, ce0) * z
    tiles = (n + TILE - 1) // TILE
    t = torch.cat((t, torch.zeros((b, tiles * TILE - n))), dim=1).view(b, tiles, 4, 4, 16)      # [tile][wave][j][r]
    total = torch.zeros(b, dtype=torch.float64)
    for s_ in range(splits):
        acc = torch.zeros((b, 4, 16))
        for ti in range(s_ * tiles // splits, (s_ + 1) * tiles // splits):
            x = t[:, ti]
            acc = acc + ((x[:, :, 0] + x[:, :, 1]) + (x[:, :, 2] + x[:, :, 3]))
        while acc.shape[2] > 1:
            acc = acc[:, :, 0::2] + acc[:, :, 1::2]
        acc = acc[:, :, 0]
        total = total + (((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]).double()
    return total.float()


def grads_eval(q, p, bias, mask, g, distance: bool, scale: float, eps: float, dtype=torch.float64, fault=None):
    """dict(v, dq, dp, dbias and their scales) in dtype from the contract's closed form.  Faults (FAULTS_GRAD): the weights
    computed as if no column were a positive; dbias left at zero."""
    sb = scale * C.beta_of(distance)
    n = p.shape[0]
    z = logits(q, p, bias, distance, scale, dtype)
    y = torch.zeros_like(mask) if fault == "weights_without_positives" else mask
    ce1, ce0 = smoothing(eps, n)
    q, p, g = q.to(dtype), p.to(dtype), g.to(dtype)
    # sigma(z) - y' on the side that does not cancel (sigma(z) - 1 = -sigma(-z)), as the contract states it: in float32
    # the plain difference loses a well-fitted positive's weight to the rounding of sigma(z) near 1
    d = torch.where(y, ce1 - torch.sigmoid(-z), torch.sigmoid(z) + ce0)
    v = sb * g[:, None] * d
    out = dict(v=v, dq=2.0 * (v @ p), dq_scale=2.0 * (v.abs() @ p.abs()))
    dp = 2.0 * (v.t() @ q)
    dp_scale = 2.0 * (v.abs().t() @ q.abs())
    if distance:
        dp = dp - 2.0 * v.sum(0)[:, None] * p
        dp_scale = dp_scale + 2.0 * v.abs().sum(0)[:, None] * p.abs()
    dbias = g * d.sum(1)
    out.update(dp=dp, dp_scale=dp_scale, dbias=torch.zeros_like(dbias) if fault == "dbias_dropped" else dbias,
               dbias_scale=g.abs() * d.abs().sum(1))
    return out


def autograd_eval(q, p, bias, mask, g, distance: bool, scale: float, eps: float, dtype):
    """(dq, dp, dbias) of sum_i g_i L_i by torch autograd in dtype on the operands' device, bias a leaf of its own"""
    q_ = q.detach().to(dtype).requires_grad_(True)
    p_ = p.detach().to(dtype).requires_grad_(True)
    b_ = bias.detach().to(dtype).requires_grad_(True)
    z = C.logits(q_, p_, distance, scale, dtype) + b_[:, None]
    loss = terms_eval(z, mask, eps).sum(1)          # (softplus(z) - y' z written so that its derivative does not cancel)
    (loss * g.to(dtype)).sum().backward()
    return q_.grad, p_.grad, b_.grad
