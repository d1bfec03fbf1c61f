"""What no op may depend on: the contents of memory it asked for uninitialised, and the stream it happens to run on.

Two context managers perturb the environment of the code run inside them, one comparison judges the outcome:

  poisoned(byte)       every uninitialised allocation (UNINITIALISED below, the torch functions and the Tensor methods) comes
                       back with each of its bytes set to `byte`, filled on the current stream.  0xFF reads as NaN in float32
                       and float64, -1 in int32 and int64, 255 in uint8; 0x7F as 3.39e38 / 1.4e306 and as 0x7F7F.. > 2e9.
  side_stream(sleep)   the body runs under torch.cuda.stream(S) for a fresh S, and every device allocation of UNINITIALISED and of
                       INITIALISED first enqueues torch.cuda._sleep(sleep) on the current stream and then its fill: S stays
                       behind the host, also after a host sync of the op.  A launch that goes to another stream by mistake
                       writes before the pending fill (which then overwrites it) or reads what has not been produced yet.
  same_bits(a, b)      dtype, shape and raw bytes; names the first element that differs.

The two combine (side_stream() with poisoned(0xFF) inside or outside it).  Nothing here provokes a fault: poison reaches only
memory the code under test asked for uninitialised, which a correct op never reads before it has written it."""
import contextlib

import numpy as np
import torch

UNINITIALISED = ("empty", "empty_like", "empty_strided")
INITIALISED = ("zeros", "zeros_like", "ones", "ones_like", "full", "full_like")
TENSOR_UNINITIALISED = ("new_empty", "new_empty_strided")
TENSOR_INITIALISED = ("new_zeros", "new_ones", "new_full")
# every spelling the harness patches, as a source file writes it
PATCHED = frozenset("torch." + n for n in UNINITIALISED + INITIALISED) | \
    frozenset("." + n for n in TENSOR_UNINITIALISED + TENSOR_INITIALISED)

# torch.cuda._sleep argument of side_stream(): 0.42 ms on the MI355X by events.  The smallest value at which every planted
# fault of test_invariance_gpu.py (test_planted_fault_is_caught_and_its_twin_passes) was caught is 3 x 10^5 (0.129 ms, in
# two runs of two; 10^5 = 0.045 ms leaves the host no lead).  10^6 is that value with a safety factor of 3.3 on top: the
# lead has to hold on a busy host too, and a planted fault that slips through once is a failing suite.  DESIGN.md 3.6m.
SLEEP_CYCLES = 1_000_000

_state = {"depth": 0, "poison": None, "sleep": 0, "saved": None}
_orig = {n: getattr(torch, n) for n in UNINITIALISED + INITIALISED}


def _on_gpu(args, kwargs):
    """whether the allocation asked for goes to the device: its device argument, else the tensor it is modelled on"""
    device = kwargs.get("device")
    if device is not None:
        return torch.device(device).type == "cuda"
    return bool(args) and isinstance(args[0], torch.Tensor) and args[0].is_cuda


def _delay(args=(), kwargs=None):
    """the bounded device-side delay in front of a device allocation's fill (a host buffer needs none)"""
    if _state["sleep"] and (kwargs is None or _on_gpu(args, kwargs)):
        torch.cuda._sleep(_state["sleep"])


def _poison(t):
    byte = _state["poison"]
    if byte is None or not isinstance(t, torch.Tensor) or t.layout != torch.strided or t.device.type == "meta" or t.numel() == 0:
        return t
    with torch.no_grad():
        d = t.detach()
        if d.dtype == torch.bool:
            d.fill_(True)
        elif d.is_contiguous():
            d.reshape(-1).view(torch.uint8).fill_(byte)
        else:                                   # (a strided request: one element of poison, broadcast)
            one = _orig["full"]((d.element_size(),), byte, dtype=torch.uint8, device=d.device).view(d.dtype)
            d.copy_(one[0])
    return t


def _wrap(fn, uninitialised):
    def patched(*args, **kwargs):
        _delay(args, kwargs)                    # the fill (torch's own, or the poison) is enqueued behind the delay
        t = fn(*args, **kwargs)
        return _poison(t) if uninitialised else t
    patched.__name__ = getattr(fn, "__name__", "patched")
    patched.__wrapped__ = fn
    return patched


def _install():
    saved = []
    for names, un in ((UNINITIALISED, True), (INITIALISED, False)):
        for n in names:
            saved.append((torch, n, True, getattr(torch, n)))
            setattr(torch, n, _wrap(getattr(torch, n), un))
    for names, un in ((TENSOR_UNINITIALISED, True), (TENSOR_INITIALISED, False)):
        for n in names:
            own = n in torch.Tensor.__dict__
            saved.append((torch.Tensor, n, own, torch.Tensor.__dict__.get(n)))
            setattr(torch.Tensor, n, _wrap(getattr(torch.Tensor, n), un))
    return saved


def _restore(saved):
    for obj, n, own, fn in reversed(saved):
        if own:
            setattr(obj, n, fn)
        else:
            delattr(obj, n)


@contextlib.contextmanager
def _perturbed(**change):
    before = {k: _state[k] for k in change}
    if _state["depth"] == 0:
        _state["saved"] = _install()
    _state["depth"] += 1
    _state.update(change)
    try:
        yield
    finally:
        _state.update(before)
        _state["depth"] -= 1
        if _state["depth"] == 0:
            saved, _state["saved"] = _state["saved"], None
            _restore(saved)


def active():
    """(poison byte or None, sleep cycles or 0) in force at the moment."""
    return _state["poison"], _state["sleep"]


@contextlib.contextmanager
def poisoned(byte=0xFF):
    if not 0 <= int(byte) <= 255:
        raise ValueError("poisoned(byte): a byte value")
    with _perturbed(poison=int(byte)):
        yield


MAX_DRAWS = 8
DRAWS = []                                      # streams drawn per side_stream() so far


def independent_stream(sleep):
    """A fresh stream behind which the null stream does not wait.  The runtime spreads its streams over a few hardware
    queues (4 by default) and serialises two streams that share one: on such a stream a launch that went to the null stream
    by mistake is ordered behind the delay like a correct one, and no perturbation can show it.  Each candidate is probed
    once -- delay and a store on the candidate, then a store from the null stream: the candidate's store must land last --
    and the first that passes is taken."""
    probe = _orig["zeros"](1, dtype=torch.int32, device="cuda")
    null = torch.cuda.default_stream()
    for draw in range(1, MAX_DRAWS + 1):
        s = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            torch.cuda._sleep(int(sleep))
            probe.fill_(1)
        with torch.cuda.stream(null):
            probe.fill_(2)
        torch.cuda.synchronize()
        if int(probe.item()) == 1:
            DRAWS.append(draw)
            return s
    raise RuntimeError(f"none of {MAX_DRAWS} fresh streams runs beside the null stream: side_stream() could see nothing")


@contextlib.contextmanager
def side_stream(sleep=SLEEP_CYCLES):
    torch.cuda.synchronize()                    # the operands made before the body are complete
    s = independent_stream(sleep)
    with torch.cuda.stream(s), _perturbed(sleep=int(sleep)):
        try:
            _delay()
            yield s
        finally:
            s.synchronize()


def _raw(x):
    """(dtype name, shape, bytes as a flat uint8 array, a printable flat view) of a tensor, an array or a scalar."""
    if isinstance(x, torch.Tensor):
        t = x.detach()
        if t.layout != torch.strided:
            raise TypeError("same_bits compares strided tensors: pass the indices and the values of a sparse one")
        t = t.cpu().contiguous().reshape(-1)
        raw = t.view(torch.uint8).numpy() if t.numel() else np.zeros(0, np.uint8)
        return str(x.dtype), tuple(x.shape), raw, t
    a = np.ascontiguousarray(x)
    flat = a.reshape(-1)
    return "numpy." + str(a.dtype), tuple(np.shape(x)), flat.view(np.uint8), flat


def same_bits(a, b, what=""):
    """True when a and b have the same dtype, shape and bytes (so NaN payloads and the sign of zero count); an
    AssertionError that names the first differing element otherwise."""
    da, sa, ra, fa = _raw(a)
    db, sb, rb, fb = _raw(b)
    head = f"{what}: " if what else ""
    assert da == db, f"{head}dtype {da} != {db}"
    assert sa == sb, f"{head}shape {sa} != {sb}"
    if ra.size == 0:
        return True
    diff = np.flatnonzero(ra != rb)
    if diff.size:
        item = ra.size // max(len(fa), 1)
        e = int(diff[0]) // item
        n_el = int(np.unique(diff // item).size)
        idx = tuple(int(i) for i in np.unravel_index(e, sa)) if sa else ()
        ha, hb = bytes(ra[e * item:(e + 1) * item][::-1]).hex(), bytes(rb[e * item:(e + 1) * item][::-1]).hex()
        raise AssertionError(f"{head}{n_el} of {len(fa)} elements differ, the first at {idx}: "
                             f"{fa[e].item()!r} (0x{ha}) != {fb[e].item()!r} (0x{hb})")
    return True
