"""Ordered split-K GEMM (include/literalkg_hip.h, lkg_gemm_ordered.hip): a product with a small output and a
long reduction, spread over the chip in k-splits whose partial outputs are added in a fixed order -- no float atomics, so
for given arguments (``splits`` among them) the result repeats bit for bit.

    gemm_ordered      out = alpha op(a) op(b) + beta out (+ bias), ops.gemm's arguments plus ``splits``
    matmul_ordered    a @ b with autograd, both gradients on gemm_ordered
    product_route     which of the two the training losses run their long reductions on: "engine" (ops.gemm in slices,
                      the default) or "ordered"; a thread-local context manager, read by current_route()

DESIGN.md 3.5c has the contract and the error bound (the chain of an element is ``per`` products plus ``s_eff`` adds).
"""
from __future__ import annotations

import contextlib
import threading
from typing import Optional, Tuple

import torch
from torch.autograd import Function

from . import _native as N
from . import ops

MAX_SPLITS = 256
ROUTES = ("engine", "ordered")

_local = threading.local()


def check_route(name) -> str:
    """``name`` when it is one of ROUTES; ValueError otherwise.  Host only."""
    if not isinstance(name, str) or name not in ROUTES:
        raise ValueError(f"products must be one of {ROUTES}, got {name!r}")
    return name


def current_route() -> str:
    """The route in force on this thread ("engine" outside every product_route())."""
    return getattr(_local, "route", "engine")


@contextlib.contextmanager
def product_route(name: str):
    """Run the long reductions of the training losses called inside on ``name`` ("engine" or "ordered").  Thread-local,
    nests, restored on exception.  A loss reads it in its forward and keeps it for its backward."""
    check_route(name)
    before = current_route()
    _local.route = name
    try:
        yield
    finally:
        _local.route = before


def keyword_route(products: str):
    """The context a public ``products`` keyword stands for: "ordered" enters product_route("ordered") around the call;
    "engine", the default of every such keyword, leaves the route in force as it is -- "engine" outside every
    product_route(), so a call that names nothing inside product_route("ordered") stays ordered.  Any other value:
    ValueError, before any device work."""
    return product_route("ordered") if check_route(products) == "ordered" else contextlib.nullcontext()


def _check_splits(splits) -> Optional[int]:
    if splits is None:
        return None
    if isinstance(splits, bool) or not isinstance(splits, int) or not 1 <= splits <= MAX_SPLITS:
        raise ValueError(f"gemm_ordered: splits must be None or an integer in [1, {MAX_SPLITS}], got {splits!r}")
    return splits


def partition(k: int, splits: int) -> Tuple[int, int]:
    """(s_eff, per) of lkg_gemm_ordered_partition: split z of s_eff covers k in [z per, min(k, (z + 1) per)), per a
    multiple of 16; (0, 0) for k == 0."""
    if int(k) < 0 or _check_splits(int(splits)) is None:
        raise ValueError(f"partition: k = {k!r}, splits = {splits!r}")
    per = N.i64(0)
    s_eff = int(N.load().lkg_gemm_ordered_partition(int(k), int(splits), N.C.byref(per)))
    return s_eff, int(per.value)


def gemm_ordered_splits(m: int, n: int, k: int, trans_a: bool = False, trans_b: bool = False) -> int:
    """The default ``splits`` of an m x n x k product (lkg_gemm_ordered_splits: a pure function of the shape)."""
    return int(N.load().lkg_gemm_ordered_splits(int(trans_a), int(trans_b), int(m), int(n), int(k)))


def gemm_ordered(a: torch.Tensor, b: torch.Tensor, trans_a: bool = False, trans_b: bool = False, alpha: float = 1.0,
                 beta: float = 0.0, out: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None,
                 splits: Optional[int] = None) -> torch.Tensor:
    """out = alpha * op(a) @ op(b) + beta * out (+ bias) on lkg_gemm_ordered_f32.  a, b: row-major 2-D fp32 (row stride
    free).  splits: how many k-splits to ask for (None: gemm_ordered_splits); partition(k, splits) tells what they are.
    The bits depend on the operands' values, k and ``per`` alone."""
    splits = _check_splits(splits)
    a, b = ops._f32_rows(a), ops._f32_rows(b)
    m, k = (a.shape[1], a.shape[0]) if trans_a else a.shape
    kb, n = (b.shape[1], b.shape[0]) if trans_b else b.shape
    if k != kb:
        raise ValueError(f"gemm_ordered: inner dimensions differ ({k} vs {kb})")
    if out is None:
        if beta != 0.0:
            raise ValueError("gemm_ordered: beta != 0 needs out")
    elif tuple(out.shape) != (m, n) or out.dtype != torch.float32 or out.stride(1) != 1:
        raise ValueError(f"gemm_ordered: out must be a float32 {m} x {n} tensor with unit column stride (got {tuple(out.shape)})")
    if bias is not None and bias.numel() != n:
        raise ValueError(f"gemm_ordered: bias of {bias.numel()} elements for {n} output columns")
    ops._need_gpu(a, b, out, bias)
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a.device)
    if splits is None:
        splits = gemm_ordered_splits(m, n, k, trans_a, trans_b)
    need = int(N.load().lkg_gemm_ordered_workspace(m, n, k, splits))
    ws = torch.empty(need // 4, dtype=torch.float32, device=a.device) if need else None      # the partials
    N.call("lkg_gemm_ordered_f32", int(trans_a), int(trans_b), m, n, k, splits, float(alpha), N.ptr(a), ops._ld(a), N.ptr(b),
           ops._ld(b), float(beta), N.ptr(out), ops._ld(out), N.ptr(bias), N.ptr(ws), need, ops._stream())
    return out


def accumulate_ordered(a: torch.Tensor, b: torch.Tensor, out: torch.Tensor, max_chain: int, trans_a: bool = False,
                       trans_b: bool = False, alpha: float = 1.0) -> torch.Tensor:
    """out += alpha * op(a) @ op(b) with no k-split longer than max_chain: ONE gemm_ordered call with
    ceil(k / f) splits, f = max_chain rounded down to a multiple of 16 (so per <= f <= max_chain) -- or, past MAX_SPLITS
    splits, one call per MAX_SPLITS * f of k, in ascending k.  What the training losses run under the "ordered" route
    in place of their loops of beta = 1 slices."""
    k = a.shape[0] if trans_a else a.shape[1]
    f = max(16, int(max_chain) // 16 * 16)
    step = MAX_SPLITS * f
    for s0 in range(0, max(k, 1), step):
        s1 = min(k, s0 + step)
        a_s = a[s0:s1] if trans_a else a[:, s0:s1]
        b_s = b[:, s0:s1] if trans_b else b[s0:s1]
        gemm_ordered(a_s, b_s, trans_a, trans_b, alpha=alpha, beta=1.0, out=out, splits=max(1, -(-(s1 - s0) // f)))
    return out


class _MatMulOrdered(Function):
    @staticmethod
    def forward(ctx, a, b):
        ops._need_gpu(a, b)
        ctx.save_for_backward(a, b)
        return gemm_ordered(a, b)

    @staticmethod
    def backward(ctx, gc):
        a, b = ctx.saved_tensors
        gc = ops._f32_rows(gc)
        ga = gemm_ordered(gc, b, trans_b=True) if ctx.needs_input_grad[0] else None
        gb = gemm_ordered(a, gc, trans_a=True) if ctx.needs_input_grad[1] else None
        return ga, gb


def matmul_ordered(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """a @ b on gemm_ordered, differentiable: dA = g b^T and dB = a^T g run on gemm_ordered too; a gradient nobody needs is
    None and is not launched."""
    return _MatMulOrdered.apply(a, b)
