"""Exclusion patterns and float64 references of the FILTERED 1-vs-all loss (the masked kernels of lkg_softmax.hip,
ops.softmax_excluded, one_vs_all_loss(known=, candidates=)), shared by test_softmax_filtered_host.py (on the CPU: the
checks accept a correct float32 masked evaluation and reject planted faults) and test_one_vs_all_filtered_gpu.py.

The reference is softmax_cases.logits in float64 with -inf at the excluded positions; measures and bounds are those of
softmax_cases (loss_measure / loss_bound, worst / gemm_bound), unchanged.  Faults: FAULTS_MASK."""
import math

import torch

import softmax_cases as C

FAULTS_MASK = ("mask_ignored", "truth_masked", "mask_shifted", "weights_unmasked")
N_PATTERNS = 10


def pattern(j: int, n: int, t: int, gen) -> list:
    """the j-th exclusion pattern for a row with truth t over n candidates (before the truth is taken out)"""
    if j == 0:
        return []                                                   # an empty list
    if j == 1:
        return [0]                                                  # the first column
    if j == 2:
        return [n - 1]                                              # the last column
    if j == 3:
        return [63, 64, 255, 256]                                   # wave and tile edges
    if j == 4:
        return list(range(64, 128))                                 # a whole wave's 64 columns
    if j == 5:
        return list(range(256, 512))                                # a whole 256-column tile
    if j == 6:
        return list(range(n // 2 - 600, n // 2 + 600))              # a run across tile (and split) boundaries
    if j == 7:
        return [t - 1, t + 1]                                       # the truth's neighbours
    if j == 8:
        return torch.nonzero(torch.rand(n, generator=gen) < 0.5)[:, 0].tolist()      # a long list
    return torch.randint(0, n, (5,), generator=gen).tolist()        # a few


def patterns(b: int, n: int, truth: torch.Tensor, seed: int, offset: int = 0) -> list:
    """per row the sorted, duplicate-free excluded positions in [0, n) without the row's truth: row i gets pattern
    (i + offset) mod N_PATTERNS, so a long list (8) stands next to an empty one (0 of the next round) and rows with few"""
    gen = torch.Generator().manual_seed(seed)
    out = []
    for i in range(b):
        t = int(truth[i])
        cols = {c for c in pattern((i + offset) % N_PATTERNS, n, t, gen) if 0 <= c < n and c != t}
        out.append(sorted(cols))
    return out


def all_but_truth(n: int, truth: torch.Tensor) -> list:
    return [[c for c in range(n) if c != int(t)] for t in truth]


def to_lists(excl: list, device="cpu"):
    """(xptr int32[B + 1], xcol int32[M]) of per-row lists"""
    xptr = [0]
    for row in excl:
        xptr.append(xptr[-1] + len(row))
    xcol = [c for row in excl for c in row]
    return (torch.tensor(xptr, dtype=torch.int32, device=device), torch.tensor(xcol, dtype=torch.int32, device=device))


def mask_of(excl: list, n: int, device="cpu") -> torch.Tensor:
    """bool[B, n]: True where the candidate is excluded"""
    m = torch.zeros((len(excl), n), dtype=torch.bool)
    for i, row in enumerate(excl):
        if row:
            m[i, torch.tensor(row)] = True
    return m.to(device)


def _fault_mask(mask, truth, fault):
    if fault == "mask_ignored":
        return torch.zeros_like(mask)
    if fault == "truth_masked":
        m = mask.clone()
        m[torch.arange(mask.shape[0], device=mask.device), truth] = True
        return m
    if fault == "mask_shifted":
        return torch.roll(mask, 1, dims=1)
    return mask


def masked_logits(q, p, mask, distance, scale, dtype=torch.float64):
    return C.logits(q, p, distance, scale, dtype).masked_fill(mask, -math.inf)


def loss_eval(q, p, truth, mask, distance: bool, scale: float, dtype=torch.float64, fault=None):
    """(lse, z_t, loss) in dtype over the candidates that are not masked.  float64: the reference; float32, fault None:
    torch's evaluation (r_torch32).  z_t is the truth's own logit, never masked (a masked truth shows in lse alone)."""
    z = C.logits(q, p, distance, scale, dtype)
    zt = z.gather(1, truth[:, None])[:, 0]
    lse = torch.logsumexp(z.masked_fill(_fault_mask(mask, truth, fault), -math.inf), dim=1)
    return lse, zt, lse - zt


def grads_eval(q, p, truth, g, mask, distance: bool, scale: float, dtype=torch.float64, fault=None):
    """dict(v, dq, dp, dq_scale, dp_scale) in dtype from the closed form with the masked softmax (exact zeros at the
    masked positions).  Fault 'weights_unmasked': the forward pass masks, the weights do not -- V = sb g (exp(z - lse_masked)
    - [c == t]) at EVERY column; the other faults change the mask of both passes."""
    sb = scale * C.beta_of(distance)
    z = C.logits(q, p, distance, scale, dtype)
    fm = _fault_mask(mask, truth, fault)
    lse = torch.logsumexp(z.masked_fill(fm, -math.inf), dim=1)
    soft = torch.exp((z if fault == "weights_unmasked" else z.masked_fill(fm, -math.inf)) - lse[:, None])
    soft[torch.arange(q.shape[0], device=q.device), truth] -= 1.0
    q, p, g = q.to(dtype), p.to(dtype), g.to(dtype)
    v = sb * g[:, None] * soft
    out = dict(v=v, dq=2.0 * (v @ p), dq_scale=2.0 * (v.abs() @ p.abs()))
    dp = 2.0 * (v.t() @ q)
    dp_scale = 2.0 * (v.abs().t() @ q.abs())
    if distance:
        dp = dp - 2.0 * v.sum(0)[:, None] * p
        dp_scale = dp_scale + 2.0 * v.abs().sum(0)[:, None] * p.abs()
    out.update(dp=dp, dp_scale=dp_scale)
    return out


def autograd_eval(q, p, truth, g, mask, distance: bool, scale: float, dtype):
    """(dq, dp) of sum_i g_i loss_i by torch autograd in dtype on the operands' device"""
    q_ = q.detach().to(dtype).requires_grad_(True)
    p_ = p.detach().to(dtype).requires_grad_(True)
    z = C.logits(q_, p_, distance, scale, dtype)
    loss = torch.logsumexp(z.masked_fill(mask, -math.inf), dim=1) - z.gather(1, truth[:, None])[:, 0]
    (loss * g.to(dtype)).sum().backward()
    return q_.grad, p_.grad


def excluded_reference(filt, filter_row, filter_rel, truth, n_cand: int, pos=None) -> list:
    """per query the list ops.softmax_excluded must give, by a Python double loop over the known structure
    (rowptr, col, eptr, rel): an entry is kept iff its relation matches (filter_rel < 0: any), it maps to a candidate
    position in [0, n_cand) and that position is not the query's truth"""
    rowptr, col, eptr, rel = (x.cpu().tolist() for x in filt)
    pos = pos.cpu().tolist() if pos is not None else None
    out = []
    for f, want, t in zip(filter_row.cpu().tolist(), filter_rel.cpu().tolist(), truth.cpu().tolist()):
        row = []
        for e in range(rowptr[f], rowptr[f + 1]):
            c = pos[col[e]] if pos is not None else col[e]
            if 0 <= c < n_cand and c != t and (want < 0 or want in rel[eptr[e]:eptr[e + 1]]):
                row.append(c)
        out.append(row)
    return out


# The smallest structure that reaches every branch of a walk over a known row: 5 entities, 6 triples (h, r, t), the pair
# (0, 1) under both relations, entity 4 in no triple.  On either side the queries (row, relation, truth) meet: an empty row;
# a row with one entry under the wanted relation and one under the other only; any relation; the truth among the entries.
TINY_TRIPLES = ([0, 0, 0, 2, 2, 3], [0, 1, 0, 1, 0, 1], [1, 1, 3, 3, 0, 2])
TINY_QUERIES = ([4, 0, 2, 3], [0, 1, -1, 0], [0, 4, 0, 4])


def shapes(ks=(1, 17, 300)):
    """(b, n, k): every b of {1, 65, 130}, n of {1, 255, 257, 1000, 70 001} and k of ks with every value of the other two
    lists in turn (a third of the product), the largest of all three together included"""
    bs, ns = (1, 65, 130), (1, 255, 257, 1000, 70001)
    out = [(b, n, k) for bi, b in enumerate(bs) for ni, n in enumerate(ns) for ki, k in enumerate(ks)
           if (bi + ni + ki) % 3 == 0]
    if (bs[-1], ns[-1], ks[-1]) not in out:
        out.append((bs[-1], ns[-1], ks[-1]))
    return out
