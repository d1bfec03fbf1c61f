"""Draws, float64 references, measures, bounds and planted faults of the self-adversarial negative-sampling loss
(lkg_nssa.hip, literalkg_amd/self_adversarial.py), shared by test_self_adversarial_host.py (on the CPU: the checks accept a
float32 restatement of the kernel's algorithm and reject planted faults), test_self_adversarial_gpu.py and
test_self_adversarial_model_gpu.py.

Contract (include/literalkg_hip.h): G groups of an anchor row q_g, a positive row p_g and K negative rows n_gj
(row g K + j of n); z+ = scale (margin - ||q - p||^2), z_j = scale (margin - ||q - n_j||^2) (dot: scale (margin + q.x));
w_j = softmax_j(temperature z_j), constants; L_g = softplus(-z+) + sum_j w_j softplus(z_j).  Gradient: a_0 = -g sigma(-z+),
a_j = g w_j sigma(z_j), c_x = cs a_x with cs = 2 scale (dot: scale); distance: dp = c_0 (q - p), dn_j = c_j (q - n_j),
dq = -sum_x c_x (q - x); dot: dp = c_0 q, dn_j = c_j q, dq = sum_x c_x x.

Measures.  The loss per group r = |L - L64| / sum |term64| against loss_bound = max(3 r_torch32, N u), a gradient per
element r = |got - x64| / (the |.|-sum of the element's terms) against grad_bound = max(3 r_torch32, N u), u = 2^-24,
r_torch32 the same quantity evaluated by float32 torch, on tables whose logits are exact in float32 (integer entries,
integer margin, power-of-two scale and temperature) so that the argument of every exponential is exact.

The counts N, from the kernel's own expressions (expf and log1pf within 1 ulp = 2 u each, every other operation u).  A
sum over the K negatives runs over a lane's ceil(K / 64) entries in order and then six butterfly steps: at most
d(K) = ceil(K / 64) - 1 + 6 additions deep.
  a weight w_j = e_j / sum e:      expf 2, the denominator 2 + d (its terms' expf, the additions), the quotient 1   = 5 + d
  softplus(z):                     expf 2, log1pf 2, the addition 1                                                 = 5
  a loss term w_j softplus(z_j):   (5 + d) + 5 + the product 1, accumulated over the negatives and added to the
                                   positive's term: d + 1                                                           = 12 + 2 d
  sigma(z):                        expf 2, 1 + e 1, the quotient 1                                                  = 4
  a dn element cs (g (w sigma)) (q - n): (5 + d) + 4 + three products 3 + the difference 1 + the product 1          = 14 + d
  a dp element: 4 + two products 2 + the difference 1 + the product 1 = 8 <= the dn count, which is used for it
  a dq element: its terms as dn's, added over a wave's ceil((K + 1) / 4) rows in order (the first addition to zero is
                exact) and over the four waves in order: ceil((K + 1) / 4) - 1 + 3 more                    = 14 + d + R + 2
"""
import itertools
import math

import torch

import softmax_cases as C

U = C.U
FAULTS_LOSS = ("temperature_ignored", "positive_sign", "next_group_negatives", "divided_by_k")
FAULTS_GRAD = ("weights_not_detached",) + FAULTS_LOSS

KS_COLS = (1, 3, 17, 64, 300, 600)            # k: 300 is 75 16-byte units for 64 lanes; 600 goes past a lane's registers
KS_NEG = (1, 2, 3, 5, 64, 65, 257)            # K: a wave's 64 lanes, one more, several turns of the lanes' loop
GS = (1, 2, 33)
ALIGNED = (True, False)
DISTANCE = (True, False)
TEMPERATURES = (0.0, 0.25, 1.0)
MAX_SPREAD = 60.0


def _pairwise_cover(lists):
    """a short list of combinations in which every value of every list meets every value of every other list (greedy,
    deterministic: the combination that covers the most pairs not met yet, the first of equals)"""
    need = {(a, x, b, y) for a, b in itertools.combinations(range(len(lists)), 2) for x in lists[a] for y in lists[b]}
    out = []
    product = list(itertools.product(*lists))
    while need:
        def gain(combo):
            return sum((a, combo[a], b, combo[b]) in need for a, b in itertools.combinations(range(len(lists)), 2))
        best = max(product, key=gain)
        out.append(best)
        need -= {(a, best[a], b, best[b]) for a, b in itertools.combinations(range(len(lists)), 2)}
    return out


# (k, K, G, aligned, distance, temperature)
CASES = _pairwise_cover((KS_COLS, KS_NEG, GS, ALIGNED, DISTANCE, TEMPERATURES))


def case_id(case) -> str:
    k, kn, g, aligned, distance, temp = case
    return f"k{k}-K{kn}-G{g}-{'aligned' if aligned else 'scalar'}-{'dist' if distance else 'dot'}-t{temp}"


# ----------------------------------------------------------------------------- draws
def exact_case(g: int, kn: int, k: int, distance: bool, seed: int, temperature: float = 1.0):
    """(q[G, k], p[G, k], n[G K, k], margin, scale): the integer tables of softmax_cases.integer_tables, margin 4 k (the
    middle of ||q - x||^2; 1 with dot) and softmax_cases.exact_scale(k): every logit is exact in float32, and with a
    power-of-two temperature so is every exponent.  No weight is near underflow: temperature (max_j z_j - min_j z_j)
    <= MAX_SPREAD in every group, asserted here."""
    q, rows, _ = C.integer_tables(g, g + g * kn, k, seed)
    p, n = rows[:g].clone(), rows[g:].clone()
    margin, scale = (4.0 * k if distance else 1.0), C.exact_scale(k)
    _, zn = logits(q, p, n, distance, margin, scale)
    spread = float((zn.max(1).values - zn.min(1).values).max()) * temperature
    assert spread <= MAX_SPREAD, (g, kn, k, distance, spread)
    return q, p, n, margin, scale


def random_case(g: int, kn: int, k: int, seed: int, std: float = 0.5):
    """(q, p, n, upstream g in [0.5, 1.5)): random rows"""
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn((g, k), generator=gen) * std
    p = torch.randn((g, k), generator=gen) * std
    n = torch.randn((g * kn, k), generator=gen) * std
    return q, p, n, torch.rand((g,), generator=gen) + 0.5


def extreme_case(seed: int = 7, g: int = 5, kn: int = 70, k: int = 64):
    """(q, p, n, margin, scale, temperature): integer tables at scale 4 and temperature 16 -- logits from about -500 to
    +400 (exact integers), so softplus and sigma run far into both tails and most weights of a group underflow to 0"""
    q, rows, _ = C.integer_tables(g, g + g * kn, k, seed)
    return q, rows[:g].clone(), rows[g:].clone(), 4.0 * k, 4.0, 16.0


# ----------------------------------------------------------------------------- references
def softplus(x):
    return x.clamp_min(0) + torch.log1p(torch.exp(-x.abs()))


def logits(q, p, n, distance: bool, margin: float, scale: float, dtype=torch.float64):
    """(z+[G], z[G, K]) in dtype, the distance summed directly"""
    q, p, n = q.to(dtype), p.to(dtype), n.to(dtype)
    n = n.reshape(q.shape[0], -1, q.shape[1])
    if distance:
        return scale * (margin - ((q - p) ** 2).sum(1)), scale * (margin - ((q[:, None] - n) ** 2).sum(2))
    return scale * (margin + (q * p).sum(1)), scale * (margin + (q[:, None] * n).sum(2))


def weights(zn, temperature: float, fault=None):
    if fault == "temperature_ignored":
        temperature = 0.0
    w = torch.softmax(temperature * zn, dim=1)
    return w / zn.shape[1] if fault == "divided_by_k" else w


def _faulty_rows(n, g: int, fault):
    """group g reading group g + 1's negatives"""
    if fault == "next_group_negatives":
        return torch.roll(n.reshape(g, -1, n.shape[1]), -1, dims=0).reshape(n.shape)
    return n


def loss_eval(q, p, n, distance: bool, margin: float, scale: float, temperature: float, dtype=torch.float64, fault=None):
    """(loss[G], denom[G]) in dtype: the sum of a group's K + 1 terms and of their magnitudes.  float64: the reference;
    float32, fault None: torch's evaluation (r_torch32).  Faults (FAULTS_LOSS): the mistakes the checks must reject."""
    zp, zn = logits(q, p, _faulty_rows(n, q.shape[0], fault), distance, margin, scale, dtype)
    w = weights(zn, temperature, fault)
    pos = softplus(zp if fault == "positive_sign" else -zp)
    neg = w * softplus(zn)
    return pos + neg.sum(1), pos.abs() + neg.abs().sum(1)


def loss_measure(loss, ref):
    """r per group against the float64 reference ref = (loss64, denom64); a NaN / inf difference counts as inf"""
    loss64, denom64 = ref
    r = (loss.double().cpu() - loss64.cpu()).abs() / (denom64.cpu() + 1e-300)
    return torch.nan_to_num(r, nan=math.inf)


def grads_eval(q, p, n, g, distance: bool, margin: float, scale: float, temperature: float, dtype=torch.float64,
               fault=None):
    """dict(dq, dp, dn and their scales) in dtype from the contract's closed form (the weights constants); the scales are
    the |.|-sums of the elements' terms.  Faults as for the loss."""
    gq = q.shape[0]
    n = _faulty_rows(n, gq, fault)
    zp, zn = logits(q, p, n, distance, margin, scale, dtype)
    w = weights(zn, temperature, fault)
    q, p, g = q.to(dtype), p.to(dtype), g.to(dtype)
    n3 = n.to(dtype).reshape(gq, -1, q.shape[1])
    a0 = g * torch.sigmoid(zp) if fault == "positive_sign" else -g * torch.sigmoid(-zp)
    aj = g[:, None] * w * torch.sigmoid(zn)
    cs = 2.0 * scale if distance else scale
    if distance:
        dp = cs * a0[:, None] * (q - p)
        dn = cs * aj[:, :, None] * (q[:, None] - n3)
        dq, dq_scale = -(dp + dn.sum(1)), dp.abs() + dn.abs().sum(1)
    else:
        dp = cs * a0[:, None] * q
        dn = cs * aj[:, :, None] * q[:, None]
        tp, tn = cs * a0[:, None] * p, cs * aj[:, :, None] * n3
        dq, dq_scale = tp + tn.sum(1), tp.abs() + tn.abs().sum(1)
    dn = dn.reshape(n.shape)
    return dict(dq=dq, dp=dp, dn=dn, dq_scale=dq_scale, dp_scale=dp.abs(), dn_scale=dn.abs())


def autograd_eval(q, p, n, g, distance: bool, margin: float, scale: float, temperature: float, dtype, detach: bool = True):
    """(dq, dp, dn) of sum_g g_g L_g by torch autograd in dtype on the operands' device, the weights detached (detach
    False: the planted fault 'weights_not_detached', the dw term left in the gradients)"""
    q_, p_, n_ = (x.detach().to(dtype).requires_grad_(True) for x in (q, p, n))
    zp, zn = logits(q_, p_, n_, distance, margin, scale, dtype)
    w = torch.softmax(temperature * zn, dim=1)
    sp = torch.nn.functional.logsigmoid          # softplus(x) = -logsigmoid(-x): differentiable at an exact 0 as well
    loss = -sp(zp) - ((w.detach() if detach else w) * sp(-zn)).sum(1)
    (loss * g.to(dtype)).sum().backward()
    return q_.grad, p_.grad, n_.grad


# ----------------------------------------------------------------------------- bounds
def depth(kn: int) -> int:
    """additions deep of a sum over K negatives: a lane's ceil(K / 64) entries in order, six butterfly steps"""
    return (kn + 63) // 64 - 1 + 6


def loss_roundings(kn: int) -> int:
    return 12 + 2 * depth(kn)


def grad_roundings(kn: int, name: str) -> int:
    n = 14 + depth(kn)
    return n + (kn + 1 + 3) // 4 + 2 if name == "dq" else n


def loss_bound(r_torch32: float, kn: int) -> float:
    return max(3.0 * r_torch32, loss_roundings(kn) * U)


def grad_bound(r_torch32: float, kn: int, name: str) -> float:
    return max(3.0 * r_torch32, grad_roundings(kn, name) * U)


# ----------------------------------------------------------------------------- the kernel's algorithm in float32 torch
def _lane_sum(x):
    """sum over dim 1 of x[G, K] the way a wave adds K values: lane l adds entries l, l + 64, ... in order, then a butterfly
    (a pairwise tree) over the 64 lanes"""
    g, kn = x.shape
    turns = (kn + 63) // 64
    x = torch.cat((x, torch.zeros((g, turns * 64 - kn), dtype=x.dtype)), dim=1).view(g, turns, 64)
    acc = torch.zeros((g, 64), dtype=x.dtype)
    for t in range(turns):
        acc = acc + x[:, t]
    while acc.shape[1] > 1:
        acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


def kernel_loss_eval(q, p, n, distance: bool, margin: float, scale: float, temperature: float):
    """(loss, w) in float32, by the kernel's steps: m = max t z, e = exp(t z - m), w = e / sum e (the sum in lane order),
    the loss's sum in lane order, the positive's term added last"""
    zp, zn = logits(q, p, n, distance, margin, scale, torch.float32)
    tz = torch.tensor(temperature, dtype=torch.float32) * zn
    e = torch.exp(tz - tz.max(1, keepdim=True).values)
    w = e / _lane_sum(e)[:, None]
    return softplus(-zp) + _lane_sum(w * softplus(zn)), w


def kernel_grads_eval(q, p, n, g, distance: bool, margin: float, scale: float, temperature: float):
    """dict(dq, dp, dn) in float32 by the kernel's steps: c_x = cs (g (w sigma)), a row's gradient c (q - x) (dot: c q),
    dq over rows 0 (the positive), 1 .. K: wave v adds rows v, v + 4, ... in order, the waves are added in order"""
    gq, k = q.shape
    zp, zn = logits(q, p, n, distance, margin, scale, torch.float32)
    _, w = kernel_loss_eval(q, p, n, distance, margin, scale, temperature)
    cs = torch.tensor(2.0 * scale if distance else scale, dtype=torch.float32)
    c = torch.cat(((cs * (g * -torch.sigmoid(-zp)))[:, None], cs * (g[:, None] * (w * torch.sigmoid(zn)))), dim=1)
    x = torch.cat((p[:, None], n.reshape(gq, -1, k)), dim=1)                   # [G, K + 1, k]
    own = c[:, :, None] * (q[:, None] - x) if distance else c[:, :, None] * q[:, None].expand_as(x)
    terms = own if distance else c[:, :, None] * x
    rows = terms.shape[1]
    turns = (rows + 3) // 4
    terms = torch.cat((terms, torch.zeros((gq, turns * 4 - rows, k))), dim=1).view(gq, turns, 4, k)
    acc = torch.zeros((gq, 4, k))
    for t in range(turns):
        acc = acc + terms[:, t]
    dq = ((acc[:, 0] + acc[:, 1]) + acc[:, 2]) + acc[:, 3]
    return dict(dq=-dq if distance else dq, dp=own[:, 0], dn=own[:, 1:].reshape(n.shape))
