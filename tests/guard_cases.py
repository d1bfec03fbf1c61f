"""Guard bands around every tensor a launch receives: the flush placement, its checks, the header ledger, the harness.

wide_cases.py asks where a kernel's ROW offsets go; this module asks whether a kernel stays inside its buffers at all, for
every pointer argument of every device entry point: id lists, rowptr / col / val, per-row vectors, counters, split buffers
and workspaces as much as the strided float tables.

THE PLACEMENT.  For one launch, one fresh buffer (the arena) holds a placement per argument:  band | extent | band.  The
whole arena is 0xFF first (NaN as float32 and float64, -1 as int32 and int64), then the caller's bytes are copied into each
extent -- for a row-strided operand the (n, d, ld) row view that wide_cases.Harness._rows resolves, column gaps included;
for every other argument the tensor whose address the caller passed.  The extent's first byte is congruent to the caller's
address modulo 512 (every alignment predicate of the dispatch code answers as it did), its last byte is followed by the
band at once, with no rounding.  band = max(64 KiB, 2 x the largest row stride in bytes among the launch's operands),
rounded up to 512: a wrong `row - 1` or `row + n` stays inside memory the test owns.  Arguments whose byte ranges overlap
or touch inside one caller storage (g_gpre | g_zpre side by side, in-place operands, column slabs of one table) share one
placement, the union of their ranges with their relative offsets kept; such an argument is recorded as `shared`.  An empty
argument (the stand-in address of _native.ptr) is a placement of extent 0: band | band.  The tall GEMM's host arrays of
pointers and strides stay host arrays; the device tensors they point to are placed.

AFTER THE LAUNCH every byte of the arena that is not a cell of a non-const argument carries what it was given: both bands
of every placement (the failure names the entry point, the parameter, the side and the first byte offset that changed),
the column gaps of strided placements, and every const argument.  Then every extent with a non-const argument is copied
back to the caller's tensor.

THE TWO PASSES.  A case runs once plain -- the boundary only records, launch by launch, a checksum of what the launch reads
and the bits of what it writes -- and once flush.  In the flush pass every output of every launch must be same_bits with
the plain pass: an over-read returns NaN or -1 where the plain pass read whatever the allocator had there, so a result
that was right by accident becomes wrong bits.  The exemptions are the wide harness's: the outputs of wide_cases.WAIVED are
left to the family's float64 bound, which the case body applies in both passes (a NaN read from a band fails it); a launch
whose input checksums differ from the plain pass's lies downstream of such an output and is counted as skipped; arguments
named `workspace` are scratch (wide_cases.SCRATCH: partial results in no stated layout), held by their bands and not
compared.  Every case runs once before the plain pass, so both passes start from the state a whole run leaves behind;
launch order and count must then be the plain pass's.  Where several views start at one address the widest is the extent.

THE LIMIT.  Every check here is a comparison of values.  An over-read whose value is masked away by a select -- the fourth
lane of a 16-byte load past an odd length, multiplied by nothing and stored nowhere -- changes no value and is not seen:
no value-based check can see it (test_guard_bands_host.py plants one and states that it passes).

Nothing here provokes a fault: a correct kernel never touches a band, and a wrong kernel's first step lands in memory the
test owns, where it shows as wrong values.  The code is generic over numpy (host tier, stand-in entry points over raw
addresses) and torch (device tier)."""
import contextlib
import ctypes
from collections import namedtuple

import numpy as np

import wide_cases as W

ALIGN = 512
MIN_BAND = 64 * 1024
NOT_MEMORY = ("stream", "dbg")

# ----------------------------------------------------------------------------- the ledger, from the header alone
# entry points that launch nothing and take no device memory of the caller's choosing: no stream parameter
HOST_ONLY = (
    "lkg_version", "lkg_last_error", "lkg_preload", "lkg_csr_build", "lkg_csr_transpose", "lkg_row_partition",
    "lkg_triples_count", "lkg_triples_read", "lkg_triples_dedup", "lkg_laplacian_f32",
    "lkg_csr_build_device_workspace", "lkg_csr_transpose_device_workspace", "lkg_gemm_tall_workspace",
    "lkg_linear_act_layernorm_workspace", "lkg_gemm_workspace", "lkg_narrow_layer_bwd_workspace",
    "lkg_binary_curve_workspace", "lkg_threshold_fit_workspace", "lkg_accept_order_workspace", "lkg_topk_splits",
    "lkg_pair_mlp_splits", "lkg_softmax_all_splits", "lkg_gemm_longk_ok", "lkg_gemm_smallm_ok", "lkg_gemm_skinny_ok",
    "lkg_narrow_layer_bwd_ok", "lkg_gemm_f32_engine", "lkg_gemm_ordered_splits", "lkg_gemm_ordered_partition",
    "lkg_gemm_ordered_workspace",
)
KINDS = ("host-only", "not memory", "host array")


def host_arrays(entry, params):
    """the parameters of `entry` that are host arrays: an array of pointers (`const float *const *a`) and the arrays of
    strides and widths that go with it (lda / ldb / ldw, ka), one element per panel"""
    if not any("*const *" in p.ctype.replace("* const", "*const") for p in params):
        return set()
    return {p.name for p in params if p.pointer and ("*const *" in p.ctype.replace("* const", "*const") or
                                                     p.name in ("lda", "ldb", "ldw", "ka"))}


def exempt_kind(entry, p, params):
    """the kind of exemption of (entry point, pointer parameter), or None: the pair is required"""
    if not any(q.name == "stream" for q in params):
        return "host-only"
    if p.name in NOT_MEMORY:
        return "not memory"
    if p.name in host_arrays(entry, params):
        return "host array"
    return None


def ledger(protos=None):
    """(required, exempt): the (entry point, pointer parameter) pairs of include/*.h that must be placed flush, and
    {pair: kind} of the others"""
    required, exempt = set(), {}
    for entry, params in (protos or W.prototypes()).items():
        for p in params:
            if not p.pointer:
                continue
            kind = exempt_kind(entry, p, params)
            if kind is None:
                required.add((entry, p.name))
            else:
                exempt[(entry, p.name)] = kind
    return required, exempt


EXEMPT = ledger()[1]


# ----------------------------------------------------------------------------- memory: numpy (host) or torch (device)
def _np(x):
    return isinstance(x, np.ndarray)


def span_bytes(t):
    """the bytes from the first to the last element of a tensor or an array (0 when empty)"""
    if _np(t):
        return 0 if t.size == 0 else sum((s - 1) * st for s, st in zip(t.shape, t.strides)) + t.itemsize
    return 0 if t.numel() == 0 else (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size()


def storage_of(t):
    return W.address(W.owner(t)) if _np(t) else t.untyped_storage().data_ptr()


def caller_bytes(t, lo, n):
    """the n bytes at address lo, inside the storage of t, as a flat uint8 view"""
    if _np(t):
        return np.ctypeslib.as_array((ctypes.c_uint8 * n).from_address(lo)) if n else np.empty(0, np.uint8)
    import torch
    st = t.untyped_storage()
    assert st.data_ptr() <= lo and lo + n <= st.data_ptr() + st.nbytes(), "an extent outside its tensor's storage"
    return torch.empty(0, dtype=torch.uint8, device=t.device).set_(st, lo - st.data_ptr(), (n,), (1,))


def new_arena(n, like):
    """n bytes of 0xFF whose first byte is 512-aligned"""
    if _np(like):
        raw = np.empty(n + ALIGN, dtype=np.uint8)
        off = -raw.ctypes.data % ALIGN
    else:
        import torch
        raw = torch.empty(n + ALIGN, dtype=torch.uint8, device=like.device)
        off = -raw.data_ptr() % ALIGN
    arena = raw[off:off + n]
    arena[...] = 0xFF
    return arena


def _zeros_bool(arena):
    if _np(arena):
        return np.zeros(arena.shape[0], dtype=bool)
    import torch
    return torch.zeros(arena.shape[0], dtype=torch.bool, device=arena.device)


def _mark_rows(mask, off, n, d, ld):
    """the cells of an (n, d) float32 row view of stride ld that starts at byte `off`"""
    if _np(mask):
        np.lib.stride_tricks.as_strided(mask[off:], shape=(n, 4 * d), strides=(4 * ld, 1))[...] = True
    else:
        import torch
        torch.as_strided(mask, (n, 4 * d), (4 * ld, 1), off).fill_(True)


def _copy(x):
    return x.copy() if _np(x) else x.clone()


def _first(flags):
    """the index of the first set flag, or None"""
    if _np(flags):
        i = np.flatnonzero(flags)
        return int(i[0]) if i.size else None
    if not bool(flags.any()):
        return None
    at = 0
    for c in flags.chunk(64):
        hit = c.nonzero()
        if hit.numel():
            return at + int(hit[0])
        at += c.numel()


def checksum(x):
    """a 0-d int64 over the bytes of a tensor's or an array's values that depends on where each byte stands: two tables that
    differ by a rounding here and the opposite rounding there (float atomics in another order) must not agree"""
    if _np(x):
        v = np.ascontiguousarray(x).reshape(-1).view(np.uint8)
        return (v.astype(np.int64) * (np.arange(v.size, dtype=np.int64) % 65521 + 1)).sum()
    import torch
    v = x.contiguous().reshape(-1).view(torch.uint8)
    if v.numel() % 4 == 0 and v.storage_offset() % 4 == 0:
        v = v.view(torch.int32)
    return (v.to(torch.int64) * (torch.arange(v.numel(), dtype=torch.int64, device=v.device) % 65521 + 1)).sum()


def band_bytes(lds):
    """max(64 KiB, 2 x the largest row stride in bytes), rounded up to 512"""
    return -(-max(MIN_BAND, 2 * 4 * max(list(lds) + [0])) // ALIGN) * ALIGN


# one pointer argument of one launch.  slot: its position in the argument list, (position, j) for panel j of a host array;
# rows: its (n, d) row view on the caller's memory when it came with a row stride; values: the caller's tensor otherwise
Item = namedtuple("Item", "param slot lo nbytes const rows values storage scratch")
# one placement: the caller's byte range [lo, hi) of one storage, the items inside it, where its extent starts in the arena
Group = namedtuple("Group", "lo hi items start")


def unions(items):
    """the items grouped by the union rule: ranges of one storage that overlap or touch share a group; an empty range
    shares nothing.  -> [(lo, hi, [item index])] in order of address"""
    out = []
    for i in sorted(range(len(items)), key=lambda i: (items[i].storage, items[i].lo, -items[i].nbytes)):
        it = items[i]
        g = out[-1] if out else None
        if g is not None and it.nbytes and g[1] > g[0] and g[3] == it.storage and it.lo <= g[1]:
            g[1] = max(g[1], it.lo + it.nbytes)
            g[2].append(i)
        else:
            out.append([it.lo, it.lo + it.nbytes, [i], it.storage])
    return [(lo, hi, idx) for lo, hi, idx, _ in out]


def layout(ranges, band):
    """where each (lo, hi) range starts in an arena whose first byte is 512-aligned, and the arena's size: every extent
    between two bands of its own, its first byte congruent to lo modulo 512"""
    starts, cursor = [], 0
    for lo, hi in ranges:
        start = cursor + band
        start += (lo - start) % ALIGN
        starts.append(start)
        cursor = start + (hi - lo) + band
    return starts, cursor


class Placed:
    """the arena of one launch"""

    def __init__(self, items, like):
        self.items = items
        self.band = band_bytes([it.rows.strides[0] // 4 if _np(it.rows) else it.rows.stride(0)
                                for it in items if it.rows is not None])
        grouped = unions(items)
        starts, size = layout([(lo, hi) for lo, hi, _ in grouped], self.band)
        self.groups = [Group(lo, hi, idx, s) for (lo, hi, idx), s in zip(grouped, starts)]
        self.arena = new_arena(size, like)
        self.base = W.address(self.arena)
        assert self.base % ALIGN == 0
        self.mask = _zeros_bool(self.arena)                         # the bytes the launch may write
        self.address = {}                                           # item index -> the address the launch receives
        self.shared = set()
        for g in self.groups:
            first = items[g.items[0]]
            if g.hi > g.lo:
                owner = first.values if first.rows is None else first.rows
                self.arena[g.start:g.start + g.hi - g.lo] = caller_bytes(owner, g.lo, g.hi - g.lo)
            for i in g.items:
                it = items[i]
                at = g.start + it.lo - g.lo
                self.address[i] = self.base + at
                assert self.address[i] % ALIGN == it.lo % ALIGN
                if len(g.items) > 1:
                    self.shared.add(i)
                if it.const or not it.nbytes:
                    continue
                if it.rows is not None:
                    n, d = it.rows.shape
                    _mark_rows(self.mask, at, n, d, it.rows.strides[0] // 4 if _np(it.rows) else it.rows.stride(0))
                else:
                    self.mask[at:at + it.nbytes] = True
        self.given = _copy(self.arena)

    def inside(self, addr, n=1):
        return self.base <= addr and addr + n <= self.base + self.arena.shape[0]

    def fault(self):
        """None, or (parameters, where, byte offset) of the first byte outside the writable cells that changed"""
        at = _first((self.arena != self.given) & ~self.mask)
        if at is None:
            return None
        for g in self.groups:
            ext = g.hi - g.lo
            names = "|".join(self.items[i].param for i in g.items)
            if g.start - self.band <= at < g.start:
                return names, "the band in front", at - g.start
            if g.start + ext <= at < g.start + ext + self.band:
                return names, "the band behind", at - (g.start + ext)
            if g.start <= at < g.start + ext:
                inner = [self.items[i] for i in g.items if self.items[i].lo - g.lo <= at - g.start < self.items[i].lo - g.lo + self.items[i].nbytes]
                it = next((x for x in inner if x.const), inner[0])
                what = "const input" if it.const else "column gap"
                return it.param, what, at - g.start - (it.lo - g.lo)
        return "?", "the arena's padding", at

    def copy_back(self):
        for g in self.groups:
            if g.hi > g.lo and any(not self.items[i].const for i in g.items):
                first = self.items[g.items[0]]
                owner = first.values if first.rows is None else first.rows
                caller_bytes(owner, g.lo, g.hi - g.lo)[...] = self.arena[g.start:g.start + g.hi - g.lo]


# ----------------------------------------------------------------------------- the harness
class Reordered(AssertionError):
    """the flush pass's launches are not the plain pass's, name by name"""


class Pass:
    def __init__(self, flush):
        self.flush = flush
        self.log = []                           # per launch: (entry point, input checksums, [(parameter, bits)])
        self.unresolved = {}                    # (entry point, parameter) -> launches whose address no tensor answered for
        self.launches = self.compared = self.waived = self.skipped = 0
        self.placed = None                      # the arena of the launch under way (the stand-ins' address table)
        self.reordered = None                   # the first launch that was not the plain pass's, in words


class Flush(W.Harness):
    """See the module docstring.  `native` is literalkg_amd._native on the device; on the host any object with call(name,
    *args) and ptr(array), whose entry points `protos` declares (the header's Param rows)."""

    def __init__(self, native, protos=None, sigs=None, host=False):
        self.host = host
        self.torch = None if host else __import__("torch")
        self.N = native
        self.protos = protos if protos is not None else W.prototypes()
        self.sigs = sigs if sigs is not None else W.strided_operands(self.protos)
        self.registry = {}
        self.tally = {}                         # (entry, parameter) -> {held, shared, compared, waived, skipped, scratch}
        self.panels = {}                        # (entry, 'a[0]') -> launches: the tensors behind the host arrays
        self.unresolved = {}
        self.passes = 0
        self.current = None

    # -- resolving
    def _rows(self, addr, ld, stacked=None):
        if not self.host:
            return super()._rows(addr, ld, stacked)
        for a in sorted(self.registry.get(addr, ()), key=lambda x: x.size):
            if a.dtype == np.float32 and a.ndim == 2 and a.shape[0] >= 2 and a.strides == (4 * ld, 4) and ld >= a.shape[1]:
                return a
        return None

    def _device(self, t):
        return _np(t) if self.host else (isinstance(t, self.torch.Tensor) and t.is_cuda)

    def _flat(self, addr):
        """the tensor the caller passed at this address: the widest when several views start there"""
        found = [t if self.host else t.data for t in self.registry.get(addr, ()) if self._device(t)]
        return max(found, key=span_bytes) if found else None

    def _item(self, name, slot, addr, const, rows):
        if rows is not None:
            n, d = rows.shape
            ld = rows.strides[0] // 4 if _np(rows) else rows.stride(0)
            return Item(name, slot, addr, 4 * ((n - 1) * ld + d), const, rows, None, storage_of(rows), False)
        t = self._flat(addr)
        if t is None:
            return None
        return Item(name, slot, addr, span_bytes(t), const, None, t, storage_of(t), name in W.SCRATCH)

    def _items(self, ps, name, args):
        params = self.protos[name]
        arrays = host_arrays(name, params)
        items, handled = [], set()

        def pointer(a):
            return isinstance(a, int) and not isinstance(a, bool) and a != 0

        for op in self.sigs.get(name, ()):
            if op.array:
                ptrs, lds = args[op.ptr_index[0]], args[op.ld_index]
                if ptrs is None or lds is None:
                    continue
                for j in range(len(ptrs)):
                    if ptrs[j]:
                        it = self._item(f"{op.label}[{j}]", (op.ptr_index[0], j), int(ptrs[j]), True,
                                        self._rows(int(ptrs[j]), int(lds[j])))
                        if it is None:
                            ps.unresolved[(name, f"{op.label}[{j}]")] = ps.unresolved.get((name, f"{op.label}[{j}]"), 0) + 1
                        else:
                            items.append(it)
                continue
            coupled = W.COUPLED.get((name, op.label))
            stacked = args[self.index(name, coupled)] if coupled else None
            for i, const, nm in zip(op.ptr_index, op.const, op.names):
                if pointer(args[i]):
                    rows = self._rows(args[i], args[op.ld_index], stacked)
                    if rows is not None:
                        handled.add(i)
                        items.append(self._item(nm, i, args[i], const, rows))
        for p in params:
            if not p.pointer or p.index in handled or p.name in NOT_MEMORY or p.name in arrays or not pointer(args[p.index]):
                continue
            it = self._item(p.name, p.index, args[p.index], p.const, None)
            if it is None:
                it = self._inner(p, args[p.index], items) or self._within(p, args[p.index])
            if it is None:
                ps.unresolved[(name, p.name)] = ps.unresolved.get((name, p.name), 0) + 1
            else:
                items.append(it)
        return items

    @staticmethod
    def _inner(p, addr, items):
        """an address no tensor answers for that lies inside another argument's tensor (seg.data_ptr() + 4 * (n_rel + 1):
        the counter behind the offsets): it follows that argument into its placement, from the address to the tensor's end"""
        for it in items:
            if it.lo <= addr < it.lo + it.nbytes:
                n = it.lo + it.nbytes - addr    # (its values: the caller's bytes from the address on, compared as bytes)
                return Item(p.name, p.index, addr, n, p.const, None, caller_bytes(it.values if it.rows is None else it.rows, addr, n),
                            it.storage, False)
        return None

    def _within(self, p, addr):
        """an address inside a tensor the caller took the address of for this launch (N.ptr(g.rowptr) + 4 * row_lo: the row
        range of a structure): the extent runs from the address to that tensor's end"""
        for ts in self.registry.values():
            for t in ts:
                if self._device(t) and not _np(t) and t.is_contiguous() and t.data_ptr() < addr < t.data_ptr() + span_bytes(t):
                    return Item(p.name, p.index, addr, t.data_ptr() + span_bytes(t) - addr, p.const, None, t.data, storage_of(t),
                                False)._replace(values=t.data.reshape(-1)[(addr - t.data_ptr()) // t.element_size():])
        return None

    # -- one launch
    def _launch(self, ps, plain, real_call, name, args):
        import invariance as V
        params = self.protos.get(name)
        if params is None or not any(p.name == "stream" for p in params):
            return real_call(name, *args)                               # (host-only: nothing is launched)
        items = self._items(ps, name, args)
        sums = [checksum(it.rows if it.rows is not None else it.values) for it in items if it.nbytes and not it.scratch]
        if not sums:
            checks = []
        elif self.host:
            checks = [int(s) for s in sums]
        else:
            checks = self.torch.stack(sums).tolist()
        args_in = tuple(args)
        placed = None
        if ps.flush and items:
            placed = Placed(items, items[0].rows if items[0].rows is not None else items[0].values)
            new_arrays = {}
            for i, it in enumerate(items):
                if isinstance(it.slot, tuple):
                    k, j = it.slot
                    if k not in new_arrays:
                        new_arrays[k] = (ctypes.c_void_p * len(args[k]))(*list(args[k]))
                    new_arrays[k][j] = placed.address[i]
                else:
                    args[it.slot] = placed.address[i]
            for k, arr in new_arrays.items():
                args[k] = arr
        ps.placed = placed
        try:
            real_call(name, *args)
        finally:
            ps.placed = None
        if not self.host:
            self.torch.cuda.synchronize()
        if placed is not None:
            fault = placed.fault()
            assert fault is None, (f"launch {len(ps.log)} {name}: parameter {fault[0]}: {fault[1]} was written, the first byte "
                                   f"at offset {fault[2]} (band {placed.band} bytes)")
            placed.copy_back()
            for i, it in enumerate(items):
                key = (name, it.param)
                if isinstance(it.slot, tuple):
                    self.panels[key] = self.panels.get(key, 0) + 1
                    continue
                t = self.tally.setdefault(key, dict(held=0, shared=0, compared=0, waived=0, skipped=0, scratch=0))
                t["shared" if i in placed.shared else "held"] += 1
        ps.launches += 1
        by_name = {p.name: a for p, a in zip(params, args_in)}
        kept = []
        for it in items:
            if it.const or isinstance(it.slot, tuple):
                continue
            when = W.WAIVED.get((name, it.param), (False,))[0]
            if it.scratch:
                self._count(ps, name, it.param, "scratch")
            elif when is None or (when and when(by_name)):
                self._count(ps, name, it.param, "waived")
            else:
                kept.append((it.param, _copy(it.rows if it.rows is not None else it.values)))
        idx = len(ps.log)
        ps.log.append((name, checks, kept if plain is None else None))
        if plain is not None and ps.reordered is None:
            p_name, p_checks, p_outs = plain.log[idx] if idx < len(plain.log) else (None, None, None)
            if p_name != name:                  # (the body runs on to its end, uncompared: an exception here would leave
                ps.reordered = f"launch {idx} is {name}, {p_name} in the plain pass"       # its caches half written)
            elif p_checks != checks:
                for nm, _ in kept:
                    self._count(ps, name, nm, "skipped")                # (downstream of an output added with atomics)
            else:
                assert [nm for nm, _ in kept] == [nm for nm, _ in p_outs], \
                    f"launch {idx} {name}: outputs {[nm for nm, _ in kept]}, {[nm for nm, _ in p_outs]} in the plain pass"
                for (nm, got), (_, want) in zip(kept, p_outs):
                    V.same_bits(got, want, f"flush, launch {idx} {name}: {nm}")
                    self._count(ps, name, nm, "compared")

    def _count(self, ps, name, param, what):
        if ps.flush:
            setattr(ps, what, getattr(ps, what, 0) + 1)
            t = self.tally.setdefault((name, param), dict(held=0, shared=0, compared=0, waived=0, skipped=0, scratch=0))
            t[what] += 1

    # -- passes and cases
    @contextlib.contextmanager
    def boundary(self, ps, plain):
        if not self.host:
            with super().boundary(ps, plain):
                yield
            return
        N = self.N
        real_call, real_ptr = N.call, N.ptr
        self.registry = {}

        def ptr(a):
            p = real_ptr(a)
            if _np(a) and p:
                self.registry.setdefault(p, []).append(a)
            return p

        def call(name, *args):
            try:
                return self._launch(ps, plain, real_call, name, list(args))
            finally:
                self.registry = {}

        N.call, N.ptr = call, ptr
        try:
            yield
        finally:
            N.call, N.ptr = real_call, real_ptr
            self.registry = {}

    @contextlib.contextmanager
    def running(self, flush, plain=None):
        """one pass: plain (the boundary records) or flush (every argument on its placement, compared against `plain`)"""
        ps = Pass(flush)
        self.current = ps
        if self.host:
            with self.boundary(ps, plain):
                yield ps
        else:
            import invariance as V
            self.torch.cuda.synchronize()
            self.torch.manual_seed(0)
            with self.boundary(ps, plain), V.poisoned(0xFF):
                yield ps
            self.torch.cuda.synchronize()
        self.current = None
        self.passes += 1
        for key, n in ps.unresolved.items():
            self.unresolved[key] = self.unresolved.get(key, 0) + n
        if plain is not None and ps.reordered is None and len(ps.log) != len(plain.log):
            ps.reordered = f"{len(ps.log)} launches, {len(plain.log)} in the plain pass"

    @contextlib.contextmanager
    def warming(self):
        if self.host:
            yield
            return
        import invariance as V
        self.torch.manual_seed(0)
        with V.poisoned(0xFF):
            yield
        self.torch.cuda.synchronize()

    def case(self, run, judge=None, what=""):
        """run() once to warm up, then once plain and once flush; the flush pass's launches must be the plain pass's, name
        by name (the body runs on to its end after a mismatch, uncompared, and the case fails then).  judge(result, mode) holds a run to its family's float64 oracle and returns
        {name: tensor} of the deterministic results, which must carry the plain pass's bits; a body that judges itself (run
        returns None) needs no judge.  -> the flush pass"""
        import invariance as V
        with self.warming():                    # (a first run fills what a body keeps between runs -- a structure's transpose,
            run()                               # a zero table kept between steps -- and launches what no later run does)
        with self.running(False) as pl:
            res = run()
        base = judge(res, "plain") if judge is not None else {}
        with self.running(True, pl) as fl:
            res = run()
        if fl.reordered is not None:
            raise Reordered(f"{what}: {fl.reordered}")
        out = judge(res, "flush") if judge is not None else {}
        assert out.keys() == base.keys(), what
        for name in base:
            V.same_bits(out[name], base[name], f"{what} flush: {name}")
        return fl

    # -- the stand-ins' address table
    def table(self, addr, n, slabs=()):
        """the n bytes at `addr` as a uint8 view, bounds-checked: inside the arena of the launch under way, or inside one
        of `slabs` (the buffers the caller owns).  A stand-in entry point reaches memory through this alone."""
        ps = self.current
        if ps is not None and ps.placed is not None and ps.placed.inside(addr, n):
            at = addr - ps.placed.base
            return ps.placed.arena[at:at + n]
        for s in slabs:
            lo = W.address(s)
            size = s.nbytes if _np(s) else s.numel() * s.element_size()
            if lo <= addr and addr + n <= lo + size:
                flat = s.reshape(-1).view(np.uint8) if _np(s) else s.reshape(-1).view(self.torch.uint8)
                return flat[addr - lo:addr - lo + n]
        raise MemoryError(f"a stand-in entry point left the memory the test owns at {addr:#x}")

    # -- the ledger
    def report(self):
        """(counts, unheld, uncompared, shared_only): the ledger over everything this harness has run"""
        required, exempt = ledger(self.protos)
        protos = self.protos
        held = {k for k, t in self.tally.items() if t["held"]}
        shared_only = sorted(k for k, t in self.tally.items() if t["shared"] and not t["held"])
        unheld = sorted(required - held - set(shared_only))
        const = {(e, p.name): p.const for e, ps in protos.items() for p in ps}
        uncompared = sorted(k for k in required & set(self.tally) if not const[k] and
                            not (self.tally[k]["compared"] or self.tally[k]["waived"] or self.tally[k]["scratch"]))
        kinds = {k: sum(1 for v in exempt.values() if v == k) for k in KINDS}
        counts = dict(required=len(required), held=len(required & held), shared_only=len(shared_only),
                      compared=sum(1 for k in required if self.tally.get(k, {}).get("compared")),
                      waived=sum(1 for k in required if self.tally.get(k, {}).get("waived")),
                      scratch=sum(1 for k in required if self.tally.get(k, {}).get("scratch")),
                      skipped_launch_outputs=sum(t["skipped"] for t in self.tally.values()),
                      exempt=kinds, passes=self.passes)
        return counts, unheld, uncompared, shared_only
