"""Draws, float64 references, measures and bounds of the 1-vs-all loss (lkg_softmax.hip, ops.softmax_all_loss), shared by
test_softmax_measures_host.py (on the CPU: the checks accept a float32 evaluation and reject planted faults) and
test_one_vs_all_gpu.py (the kernels on the device).

Contract (include/literalkg_hip.h): s_ic = |p_c|^2 - 2 q_i.p_c (dot: -2 q_i.p_c), z_ic = -scale beta s_ic with beta = 1
(distance) or 1/2 (dot), loss_i = logsumexp_c z_ic - z_i,t_i;  V_ic = scale beta g_i (softmax_ic - [c == t_i]),
dQ = 2 V P,  dP = 2 V^T Q - 2 diag(colsum V) P (the second term with distance only).

Measures: the loss per query r = |loss - loss64| / (|lse64| + |z_t|) against max(3 r_torch32, 3e-7) (the "red." bound of
DESIGN 3.5a); a gradient per element r = |got - x64| / scale with scale the |.|-sum of the float64 expression's terms,
against the bound of the engine that ran the product (tests/op_audit.py)."""
import math

import torch

U = 2.0 ** -24
TILE = 256
FAULTS_LOSS = ("max_not_carried", "beta", "drop_last")
FAULTS_GRAD = ("truth_in_weights", "no_diag", "beta")


def beta_of(distance: bool) -> float:
    return 1.0 if distance else 0.5


def exact_scale(k: int) -> float:
    """a power of two that keeps the logits of integer tables in [-2, 2] exact and their spread at 8-24"""
    return 2.0 ** -6 if k >= 100 else (2.0 ** -3 if k >= 16 else 0.5)


def strided(t: torch.Tensor, ld: int) -> torch.Tensor:
    """the same values as rows of a wider buffer (row stride ld >= columns)"""
    buf = torch.zeros((t.shape[0], ld), dtype=t.dtype, device=t.device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]]


def aligned_ld(k: int) -> int:
    return (k + 3) // 4 * 4 + 4          # a multiple of 4 floats: the 16-byte path (with a scalar tail when k % 4)


def unaligned_ld(k: int) -> int:
    return k + 1 if (k + 1) % 4 else k + 2


def truths(b: int, n: int, gen) -> torch.Tensor:
    """candidate 0, candidate n - 1, the last column of a full tile, then random"""
    t = torch.randint(0, n, (b,), generator=gen)
    special = [0, n - 1, (n // TILE) * TILE - 1 if n >= TILE else n - 1]
    for i, v in enumerate(special[:b]):
        t[i] = v
    return t


def integer_tables(b: int, n: int, k: int, seed: int):
    """q, p with integer entries in [-2, 2] (float32), truths: every score and, with a power-of-two scale, every logit is
    exact in float32"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randint(-2, 3, (b, k), generator=gen).float()
    p = torch.randint(-2, 3, (n, k), generator=gen).float()
    return q, p, truths(b, n, gen)


def random_tables(b: int, n: int, k: int, seed: int, std: float = 0.5):
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn((b, k), generator=gen) * std
    p = torch.randn((n, k), generator=gen) * std
    return q, p, truths(b, n, gen), torch.rand((b,), generator=gen) + 0.5


def logits(q, p, distance: bool, scale: float, dtype=torch.float64, beta=None):
    """z in dtype, by the contract's expression"""
    q, p = q.to(dtype), p.to(dtype)
    s = -2.0 * (q @ p.t())
    if distance:
        s = s + (p * p).sum(1)[None, :]
    return -(scale * (beta_of(distance) if beta is None else beta)) * s


def loss_eval(q, p, truth, distance: bool, scale: float, dtype=torch.float64, fault=None):
    """(lse, z_t, loss) in dtype.  float64: the reference.  float32 with fault None: torch's evaluation (r_torch32).
    Faults (FAULTS_LOSS) are the mistakes the checks must reject."""
    beta = None
    if fault == "beta":
        beta = 1.5 - beta_of(distance)            # the other scoring's
    z = logits(q, p, distance, scale, dtype, beta)
    zt = z.gather(1, truth.to(z.device)[:, None])[:, 0]
    if fault == "drop_last":
        z = z[:, :-1] if z.shape[1] > 1 else z
    lse = torch.logsumexp(z, dim=1)
    return lse, zt, lse - zt


def online_eval(q, p, truth, distance: bool, scale: float, fault=None):
    """The kernel's algorithm in float32 torch: 256-wide tiles, a running (m, l) per row, rescaled when m moves.
    fault 'max_not_carried': the maximum is taken per tile but l is not rescaled to the new one."""
    z = logits(q, p, distance, scale, torch.float32)
    zt = z.gather(1, truth[:, None])[:, 0]
    m = torch.full((z.shape[0],), -math.inf)
    l_ = torch.zeros(z.shape[0])
    for c0 in range(0, z.shape[1], TILE):
        zt_ = z[:, c0:c0 + TILE]
        mt = zt_.max(1).values
        mn = torch.maximum(m, mt)
        part = torch.exp(zt_ - mn[:, None]).sum(1)
        l_ = (l_ if fault == "max_not_carried" else l_ * torch.exp(m - mn)) + part
        m = mn
    lse = m + torch.log(l_)
    return lse, zt, lse - zt


def loss_measure(loss, ref):
    """r per query against the float64 reference ref = (lse64, zt64, loss64); a NaN / inf difference counts as inf"""
    lse64, zt64, loss64 = ref
    r = (loss.double().cpu() - loss64.cpu()).abs() / (lse64.abs().cpu() + zt64.abs().cpu() + 1e-300)
    return torch.nan_to_num(r, nan=math.inf)


def loss_bound(r_torch32: float) -> float:
    return max(3.0 * r_torch32, 3e-7)


def reduce_eval(loss, reduction: str, fault=None):
    if reduction == "none":
        return loss
    if reduction == "sum":
        return loss.sum()
    return loss.sum() / (loss.numel() + 1 if fault == "mean_count" else loss.numel())


def grads_eval(q, p, truth, g, distance: bool, scale: float, dtype=torch.float64, fault=None):
    """dict(v, dq, dp, dq_scale, dp_scale) in dtype from the contract's closed form; the scales are the |.|-sums of the
    terms.  Faults (FAULTS_GRAD): the truth's term left in the weights, the diag(colsum V) P term dropped, the other
    scoring's beta."""
    sb = scale * (beta_of(distance) if fault != "beta" else 1.5 - beta_of(distance))
    z = logits(q, p, distance, scale, dtype)
    soft = torch.softmax(z, dim=1)
    if fault != "truth_in_weights":
        soft = soft.clone()
        soft[torch.arange(q.shape[0]), truth] -= 1.0
    q, p, g = q.to(dtype), p.to(dtype), g.to(dtype)
    v = sb * g[:, None] * soft
    out = dict(v=v, dq=2.0 * (v @ p), dq_scale=2.0 * (v.abs() @ p.abs()))
    dp = 2.0 * (v.t() @ q)
    dp_scale = 2.0 * (v.abs().t() @ q.abs())
    if distance:
        if fault != "no_diag":
            dp = dp - 2.0 * v.sum(0)[:, None] * p
        dp_scale = dp_scale + 2.0 * v.abs().sum(0)[:, None] * p.abs()
    out.update(dp=dp, dp_scale=dp_scale)
    return out


def autograd_eval(q, p, truth, g, distance: bool, scale: float, dtype):
    """(dq, dp) of sum_i g_i loss_i by torch autograd in dtype on the operands' device"""
    q_ = q.detach().to(dtype).requires_grad_(True)
    p_ = p.detach().to(dtype).requires_grad_(True)
    z = logits(q_, p_, distance, scale, dtype)
    loss = torch.logsumexp(z, dim=1) - z.gather(1, truth[:, None])[:, 0]
    (loss * g.to(dtype)).sum().backward()
    return q_.grad, p_.grad


def worst(got, want64, scale64) -> float:
    """max over the elements of |got - want| / scale (0 / 0 = 0: an element with no term at all must be exactly 0)"""
    diff = (got.double() - want64).abs()
    r = torch.where(diff == 0, torch.zeros_like(diff), diff / scale64.clamp_min(1e-300))
    r = torch.nan_to_num(r, nan=math.inf)
    return float(r.max()) if r.numel() else 0.0


def gemm_bound(engine: str, r_torch32: float, k: int) -> float:
    """the bound of the engine that ran a gradient product (tests/op_audit.py): lkg_gemm_f32's f32 MFMA is
    max(2 r_torch32, 3e-7, 2 sqrt(K) u)"""
    import op_audit
    return op_audit.bound_for(engine, r_torch32, k)


def shapes(ks):
    """(b, n, k): every b of {1, 63, 64, 65, 130}, n of {1, 255, 256, 257, 1000, 70 001} and k of ks appears with every
    value of the other two lists in turn (a third of the full product), the largest of all three together included"""
    bs, ns = (1, 63, 64, 65, 130), (1, 255, 256, 257, 1000, 70001)
    out = [(b, n, k) for bi, b in enumerate(bs) for ni, n in enumerate(ns) for ki, k in enumerate(ks)
           if (bi + ni + ki) % 3 == 0]
    if (bs[-1], ns[-1], ks[-1]) not in out:
        out.append((bs[-1], ns[-1], ks[-1]))
    return out
