"""Row-strided operands spread over more than 2^32 elements: the placement, its checks, the header ledger, the harness.

Every C entry point takes its tables as (pointer, row stride).  The stride is free, so a table of 9 or 257 rows can be laid
over 20 GB of memory of which only its own cells are ever given values: the kernels run at the small tile-edge shapes the
suite already uses, and their row offsets cross every 32-bit boundary.

THE STORE.  One flat float32 buffer: a front pad of 2^(b-1) elements, then a span of 2^b * 8/7 elements plus a slack of
2^(b-6) ("a little over") plus a tail of max(2^(b-10), 1024) elements for the last row's cells; b = wrap_bits is 32 on the
device (about 28 GB) and 16 in the host test (a numpy array of 436 KB).  Before each use every byte is 0xFF: NaN as float32,
-1 as int32.  The view's base is the end of the pad (16-byte aligned), the row stride ld a multiple of 4.

WHERE THE ROWS FALL (check_geometry asserts it; offsets in elements from the base, B = 2^b):
  row 0 at 0; at least two rows at >= B; at least two in [B/2, B); at least two at a byte offset in [B, 2B), that is
  elements in [B/4, B/2); and rows at a byte offset in [B/2, B), elements in [B/8, B/4): at least two for n >= 15 and at
  least one for 9 <= n < 15.  All five with two rows each cannot hold below 15 rows under one stride: rows k and k + 1
  both in [B/8, B/4) mean k ld >= B/8 and (k + 1) ld < B/4; k = 1 contradicts itself, so k >= 2 and ld < B/12; two rows
  at >= B need (n - 2) ld >= B, hence n - 2 > 12.  (test_wide_placement_host.py confirms it by exhaustion at 16 bits.)
  From 9 to 14 rows the last band holds one row; each of the four wrap models below still moves at least two rows of
  such a table, which is what the bands are for.

THE FOUR WRAP MODELS, and why a wrong kernel gives wrong values and no fault.  An index product that is too narrow sends
the element offset o of a row through int32 or uint32, or its byte offset 4 o through int32 or uint32 (wrapped()).  For
every row and every model check_geometry asserts that
  - no row's cells contain a multiple of B/8 past their first cell: the four maps are translations between such multiples,
    so a row moves as one block, whether the product of row and stride wraps or the sum with the column does;
  - the image of a row that moves lies inside the store: a negative image is >= -B/2, inside the pad, and ends at or
    before the base; a non-negative one is below the row itself;
  - the image meets no row's own cells: it lies in the gap between two rows (d <= image mod ld <= ld - d).
So a wrapped read returns poison (NaN) and a wrapped write lands in poison, which is checked after the op; neither leaves
the allocation.  geometry() walks ld down in steps of 4 from the widest stride that fits until all of this holds.

THE TWIN.  The same values in a buffer of their own, row stride 4 ceil(d / 4) + 4, base 16-byte aligned: both placements
take the same load path of every kernel (vector where d % 4 == 0, scalar otherwise).

Operands that share one stride argument (ph / pp / pn of the dense scores) are placed together, side by side in one
placement, each in a slot of 4 ceil(d / 4) + 4 columns.

THE HARNESS (Harness, device only).  A case is an existing test body or a (run, judge) pair.  It runs inside a wrapper of
_native.call and _native.ptr (in the style of autograd_cases.launches) that replaces, at the C boundary, every resolved
(pointer, stride) pair by the twin placement of the operand -- the twin pass -- and, in one further pass per operand, that
operand alone by its wide placement.  The operand's rows are those of the tensor whose address the caller passed: nothing
is read or written outside tensors the caller owns.  After each launch outputs are copied back to the caller's tensor,
inputs must carry the bits they were given, the wide cells are set back to 0xFF; after each pass the whole store must be
0xFF.  Every launch's outputs (strided and flat) are kept in the twin pass and compared bit for bit in the wide pass
(same_bits), output by output: only the outputs of WAIVED -- those a kernel adds into with float atomics, in the launches
that do so, and buffers filled through an atomic slot counter -- are left to the family's float64 bound, which the body
itself applies in the twin pass and in every wide pass.  A launch is compared only if everything it reads (checksums of
every tensor argument, taken before the launch) equals the twin pass's: a launch downstream of a waived output may differ
and is counted as skipped, not compared.  The ledger credits an operand only with comparisons of launches that received it
wide.  An operand that an id list gathers (GATHERED) fails its pass unless the case's ids select a row at >= 2^32 elements
and one in [2^31, 2^32).  A pass fails unless a launch received an address inside the store
for the operand under test."""
import contextlib
import functools
import glob
import os
import re
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- geometry (plain integers, no store)
def pad_elems(b):
    return 1 << (b - 1)


def span_elems(b):
    """the furthest start of a last row: a little over 2^b * 8/7"""
    return (((1 << b) * 8 + 6) // 7 + 3) // 4 * 4 + (1 << (b - 6))


def tail_elems(b):
    return max(1 << (b - 10), 1024)


def store_elems(b):
    return pad_elems(b) + span_elems(b) + tail_elems(b)


WRAPS = ("int element", "uint element", "int byte", "uint byte")


def wrapped(o, model, b):
    """the element offset a kernel reaches when it sends o (element) or 4 o (byte) through a b-bit integer"""
    o = np.asarray(o, dtype=np.int64)
    full, half = np.int64(1) << b, np.int64(1) << (b - 1)
    if model == "int element":
        return (o + half) % full - half
    if model == "uint element":
        return o % full
    if model == "int byte":
        return ((4 * o + half) % full - half) // 4
    if model == "uint byte":
        return (4 * o % full) // 4
    raise ValueError(model)


def bands(n, ld, b):
    """how many rows start in each of the four bands"""
    o = np.arange(n, dtype=np.int64) * ld
    full = np.int64(1) << b
    return {"elements >= 2^b": int((o >= full).sum()),
            "elements in [2^(b-1), 2^b)": int(((o >= full // 2) & (o < full)).sum()),
            "bytes in [2^b, 2^(b+1))": int(((4 * o >= full) & (4 * o < 2 * full)).sum()),
            "bytes in [2^(b-1), 2^b)": int(((4 * o >= full // 2) & (4 * o < full)).sum())}


def geometry_faults(n, d, ld, b):
    """every way (n, d, ld) misses the placement's contract at b wrap bits; empty when it holds"""
    out = []
    if n < 9:
        return [f"n = {n} < 9 rows"]
    if ld % 4 or ld < d + 1:
        out.append(f"ld {ld} is no multiple of 4 or leaves no gap behind d {d}")
    o = np.arange(n, dtype=np.int64) * ld
    if int(o[-1]) > span_elems(b) or int(o[-1]) + d > span_elems(b) + tail_elems(b):
        out.append(f"the last row starts at {int(o[-1])}, outside the span")
    block = np.int64(1) << (b - 3)
    if bool((o // block != (o + d - 1) // block).any()):
        out.append("a row contains a multiple of 2^(b-3) past its first cell")
    got = bands(n, ld, b)
    for i, (name, count) in enumerate(got.items()):
        need = 1 if (i == 3 and n < 15) else 2
        if count < need:
            out.append(f"{count} rows with {name}, {need} needed")
    for model in WRAPS:
        w = wrapped(o, model, b)
        moved = w != o
        if not bool(moved.any()):
            out.append(f"no row moves under the {model} wrap")
        neg = moved & (w < 0)
        if bool((w[neg] < -pad_elems(b)).any()) or bool((w[neg] + d > 0).any()):
            out.append(f"{model}: a negative image leaves the pad")
        pos = moved & (w >= 0)
        r = w[pos] % ld
        if bool((w[pos] >= o[pos]).any()) or bool(((r < d) | (r + d > ld)).any()):
            out.append(f"{model}: an image meets a row's cells")
    return out


def check_geometry(n, d, ld, b=32):
    faults = geometry_faults(n, d, ld, b)
    assert not faults, (n, d, ld, b, faults)
    return True


@functools.lru_cache(maxsize=None)
def geometry(n, d, b=32):
    """the row stride of the wide placement of an (n, d) operand: the widest multiple of 4 that meets check_geometry"""
    if n < 9:
        raise ValueError(f"a wide placement needs at least 9 rows (got {n})")
    ld = span_elems(b) // (n - 1) // 4 * 4
    floor = max(-(-(1 << b) // (n - 2)), d + 1)
    tries = 0
    while ld >= floor and tries < 4096:
        if not geometry_faults(n, d, ld, b):
            return ld
        ld -= 4
        tries += 1
    raise ValueError(f"no row stride places {n} x {d} at {b} wrap bits")


def twin_ld(d):
    return 4 * -(-d // 4) + 4


# ----------------------------------------------------------------------------- stores: numpy (host) or torch (device)
def _is_numpy(x):
    return isinstance(x, np.ndarray)


def new_store(b, device=None):
    """an unfilled store; poison() fills it"""
    if device is None:
        raw = np.empty(store_elems(b) + 4, dtype=np.float32)
        off = (-raw.ctypes.data % 16) // 4
        return raw[off:off + store_elems(b)]
    import torch
    return torch.empty(store_elems(b), dtype=torch.float32, device=device)


def address(x):
    return x.ctypes.data if _is_numpy(x) else x.data_ptr()


def inside(store, addr):
    """whether a raw address lies inside the store"""
    lo = address(store)
    return lo <= addr < lo + 4 * store.size if _is_numpy(store) else lo <= addr < lo + 4 * store.numel()


def poison(store):
    if _is_numpy(store):
        store.view(np.uint8)[:] = 0xFF
    else:
        store.view(__import__("torch").int32).fill_(-1)
    return store


def all_poison(store):
    """one pass over the store: every byte 0xFF"""
    if _is_numpy(store):
        return bool((store.view(np.int32) == -1).all())
    import torch
    words = store.view(torch.int64) if store.numel() % 2 == 0 else store.view(torch.int32)
    bad = [c.ne(-1).any() for c in words.chunk(16)]               # (the comparison's bools: a sixteenth of the store at a time)
    return not bool(torch.stack(bad).any().item())


def first_stain(store, b):
    """the element offset (from the base) of the first cell that is not poison, for the message of a failed check"""
    if _is_numpy(store):
        i = np.flatnonzero(store.view(np.int32) != -1)
        return int(i[0]) - pad_elems(b) if i.size else None
    import torch
    at = 0
    for c in store.view(torch.int32).chunk(64):
        hit = c.ne(-1).nonzero()
        if hit.numel():
            return at + int(hit[0]) - pad_elems(b)
        at += c.numel()
    return None


def _strided(flat, offset, n, d, ld):
    if _is_numpy(flat):
        return np.lib.stride_tricks.as_strided(flat[offset:], shape=(n, d), strides=(4 * ld, 4))
    import torch
    return torch.as_strided(flat, (n, d), (ld, 1), offset)


def _assign(view, values):
    if _is_numpy(view):
        view[...] = values
    else:
        view.copy_(values)


def place(store, values, wrap_bits=32):
    """a row-strided (n, d) view of `store` that holds `values`: torch.as_strided (numpy's as_strided on a numpy store), so
    the last row needs only its d cells.  The geometry is asserted here, for the stride in use."""
    n, d = values.shape
    ld = geometry(n, d, wrap_bits)
    check_geometry(n, d, ld, wrap_bits)
    assert (store.size if _is_numpy(store) else store.numel()) == store_elems(wrap_bits), "the store of another wrap width"
    base = pad_elems(wrap_bits)
    assert (address(store) + 4 * base) % 16 == 0, "the view's base is not 16-byte aligned"
    view = _strided(store, base, n, d, ld)
    _assign(view, values)
    return view


def twin(values):
    """the same values in a buffer of their own, row stride 4 ceil(d / 4) + 4, base 16-byte aligned"""
    n, d = values.shape
    ld = twin_ld(d)
    if _is_numpy(values):
        flat = np.empty(n * ld + 4, dtype=np.float32)
        off = (-flat.ctypes.data % 16) // 4
    else:
        import torch
        flat = torch.empty(n * ld + 4, dtype=torch.float32, device=values.device)
        off = (-flat.data_ptr() % 16) // 4
    flat.view(np.int32 if _is_numpy(flat) else __import__("torch").int32)[...] = -1
    view = _strided(flat, off, n, d, ld)
    assert address(view) % 16 == 0
    _assign(view, values)
    return view


def owner(view):
    """the flat numpy buffer a placement lives in"""
    a = view
    while getattr(a, "base", None) is not None:
        a = a.base
    return a


def clear(view):
    """a placement's cells back to 0xFF"""
    if _is_numpy(view):
        view.view(np.int32)[...] = -1
    else:
        view.view(__import__("torch").int32).fill_(-1)


def carries(view, values):
    """whether the view's cells hold exactly the bits of `values`"""
    if _is_numpy(view):
        return bool(np.array_equal(np.ascontiguousarray(view).view(np.int32), np.ascontiguousarray(values).view(np.int32)))
    import torch
    return bool(torch.equal(view.view(torch.int32), values.contiguous().view(torch.int32)))


# every (n, d) the device module places wide (test_ledger of test_wide_placement_gpu.py asserts that it is; the host test
# asserts the geometry of each without a store)
SHAPES = [(9, 5), (9, 7), (9, 8), (9, 17), (9, 64), (9, 66), (9, 68), (9, 69), (9, 257), (9, 260), (10, 5), (10, 7),
          (10, 8), (10, 17), (10, 66), (10, 68), (10, 69), (11, 3), (11, 7), (11, 8), (11, 17), (11, 32), (11, 33),
          (11, 37), (11, 66), (12, 5), (12, 7), (12, 8), (12, 66), (12, 68), (12, 69), (13, 5), (13, 7), (13, 8),
          (13, 66), (13, 68), (13, 69), (14, 5), (14, 7), (14, 8), (14, 66), (14, 68), (14, 69), (15, 17), (17, 3),
          (17, 32), (23, 7), (23, 66), (24, 300), (30, 7), (30, 66), (32, 17), (32, 32), (32, 37), (33, 3), (33, 64),
          (33, 65), (33, 128), (33, 129), (33, 130), (33, 300), (33, 301), (33, 600), (33, 2210), (33, 4096), (33, 4160),
          (35, 7), (35, 132), (39, 8), (40, 1), (40, 5), (40, 24), (40, 32), (40, 64), (40, 130), (40, 300), (47, 66),
          (48, 80), (50, 8), (50, 64), (53, 37), (53, 128), (55, 7), (55, 66), (59, 37), (59, 128), (64, 64), (64, 4096),
          (64, 4160), (65, 1), (65, 11), (65, 17), (65, 18), (65, 32), (65, 33), (65, 37), (65, 64), (65, 128),
          (65, 256), (65, 257), (65, 300), (65, 301), (65, 4160), (66, 32), (66, 600), (68, 32), (68, 37), (69, 17),
          (69, 32), (69, 37), (70, 32), (70, 37), (72, 2), (73, 32), (73, 37), (88, 3), (88, 32), (95, 3), (95, 7),
          (95, 66), (95, 132), (96, 112), (96, 128), (96, 130), (99, 3), (99, 70), (100, 64), (119, 3), (119, 20),
          (119, 32), (119, 104), (120, 32), (128, 16), (128, 33), (128, 37), (128, 64), (128, 96), (128, 128), (129, 33),
          (129, 130), (129, 300), (129, 4097), (129, 8003), (129, 76800), (130, 17), (130, 32), (130, 33), (130, 255),
          (130, 4097), (130, 8003), (136, 3), (136, 32), (137, 30), (153, 3), (153, 32), (160, 136), (174, 37),
          (174, 128), (200, 17), (200, 32), (210, 33), (255, 32), (255, 33), (256, 17), (256, 18), (256, 32), (256, 33),
          (256, 96), (257, 3), (257, 5), (257, 17), (257, 18), (257, 32), (257, 37), (257, 64), (257, 65), (257, 128),
          (257, 257), (257, 260), (257, 300), (300, 24), (300, 40), (300, 2210), (300, 76800), (301, 2210), (352, 32),
          (429, 8), (500, 3), (600, 5), (600, 130), (700, 1), (700, 8), (700, 32), (700, 130), (700, 256), (757, 33),
          (757, 70), (800, 4), (800, 30), (800, 64), (800, 128), (1025, 4), (1027, 1), (1027, 2), (1027, 64),
          (1027, 100), (1032, 5), (1032, 7), (1032, 8), (1032, 66), (1032, 68), (1032, 69), (1036, 5), (1036, 7),
          (1036, 8), (1036, 66), (1036, 68), (1036, 69), (2054, 24), (2054, 40), (2145, 64), (3000, 96), (3000, 130),
          (4097, 129), (4097, 130), (4099, 32), (4103, 32), (4800, 48), (4800, 80), (7001, 1), (7001, 2), (7001, 64),
          (7001, 100), (8003, 96), (8003, 112), (8003, 129), (8003, 130), (8320, 96), (8320, 128), (16389, 32),
          (16389, 64), (16389, 128), (16461, 16), (16461, 64), (16461, 96), (16461, 128), (16461, 256), (20000, 32),
          (20000, 37), (20000, 40), (20000, 70), (20000, 96), (20000, 128), (40000, 136), (40000, 160), (40005, 136),
          (40005, 160), (200000, 64), (300001, 2), (300001, 72)]


# ----------------------------------------------------------------------------- the headers: who takes a row stride
Param = namedtuple("Param", "index name ctype pointer const")
# one operand of an entry point: `names` share the stride argument `ld` (one name, but for the dense scores); `array` marks
# the tall GEMM's host arrays of pointers and strides
Operand = namedtuple("Operand", "label names ptr_index ld_index const array")

# stride arguments that several pointers share (include/literalkg_hip.h: "ph / pp / pn ... row stride ld")
SHARED = {
    ("lkg_dense_score_fwd_f32", "ld"): ("ph", "pp", "pn"),
    ("lkg_dense_score_bwd_f32", "ld"): ("ph", "pp", "pn"),
    ("lkg_dense_score_bwd_f32", "ldg"): ("g_ph", "g_pp", "g_pn"),
}


def prototypes(include=None):
    """{entry point: [Param]} of every declaration in include/*.h"""
    out = {}
    for path in sorted(glob.glob(os.path.join(include or os.path.join(ROOT, "include"), "*.h"))):
        with open(path) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        for m in re.finditer(r"\b(lkg_\w+)\s*\(([^;{()]*)\)\s*;", text, re.S):
            params = []
            for i, p in enumerate(x.strip() for x in m.group(2).split(",")):
                p = re.sub(r"\s+", " ", p)
                if p in ("", "void"):
                    continue
                name = re.split(r"[\s*]+", p)[-1]
                ctype = p[: len(p) - len(name)].strip()
                params.append(Param(i, name, ctype, "*" in ctype, ctype.startswith("const")))
            out[m.group(1)] = params
    return out


def strided_operands(protos=None):
    """{entry point: [Operand]} for every entry point that declares a parameter named ld* (int64_t, or the arrays
    `const int64_t *ld*` of the tall GEMM and the fused layer)"""
    out = {}
    for entry, params in (protos or prototypes()).items():
        ops = []
        for p in params:
            if not p.name.startswith("ld"):
                continue
            if p.pointer:                                           # const int64_t *lda: an array of strides, one per panel
                prev = params[p.index - 1]
                assert prev.pointer and "*const *" in prev.ctype.replace("* const", "*const"), (entry, p, prev)
                ops.append(Operand(prev.name, (prev.name,), (prev.index,), p.index, (True,), True))
                continue
            names = SHARED.get((entry, p.name))
            if names is None:
                prev = params[p.index - 1]
                assert prev.pointer and "float" in prev.ctype, (entry, p.name, "follows no float pointer", prev)
                names = (prev.name,)
            by_name = {q.name: q for q in params}
            group = [by_name[x] for x in names]
            ops.append(Operand("+".join(names), tuple(names), tuple(q.index for q in group), p.index,
                               tuple(q.const for q in group), False))
        if ops:
            out[entry] = ops
    return out


def ledger_pairs(protos=None):
    return {(entry, op.label) for entry, ops in strided_operands(protos).items() for op in ops}


# Outputs that are not a function of the launch's inputs alone, read from the kernels: (entry point, output) -> (when, why).
# `when` takes the launch's arguments by name and says whether THIS launch adds with atomics; None: always.  Everything
# else a launch writes is compared bit for bit.
def _k_at_least(k_min, also_beta0=False):
    def when(a):
        return a["k"] >= k_min and (not also_beta0 or a["beta"] == 0.0)
    return when


WAIVED = {
    # float atomicAdd into global memory
    ("lkg_scatter_add_rows_f32", "dst"): (None, "lkg_batch.hip scatter_add_rows_kernel: atomicAdd(dst + r * ldd + c, ...)"),
    ("lkg_scatter_add_rows_range_f32", "dst"): (None, "lkg_batch.hip: atomicAdd(dst + (r - lo) * ldd + c, ...)"),
    ("lkg_spmm_csr_scatter_bwd_f32", "g_x"): (None, "lkg_spmm.hip: atomicAdd(g_x + col[j] * ldx + c, val[j] * g)"),
    ("lkg_transe_score_bwd_f32", "g_emb"): (None, "lkg_score.hip score_bwd_kernel: atomicAdd(gh / gp / gn + k, ...)"),
    ("lkg_transe_score_bwd_f32", "g_rel"): (None, "lkg_score.hip score_bwd_kernel: atomicAdd(gr + k, ...)"),
    ("lkg_dot_score_bwd_f32", "g_emb"): (None, "lkg_score.hip dot_bwd_kernel: atomicAdd(gh / gp / gn + k, ...)"),
    ("lkg_dense_score_bwd_f32", "g_rel"): (None, "lkg_score.hip score_bwd_grouped_kernel: atomicAdd(g_rel + r[grp] * ld_grel + c, ...)"),
    ("lkg_gemm_f32", "c"): (_k_at_least(2048, also_beta0=True),
                            "lkg_gemm.hip lkg_gemm_f32: splits > 1 (K-slices added with atomicAdd) only with beta == 0 and "
                            "k >= 2048; every other launch is a k-ordered chain and is compared"),
    ("lkg_gemm_wgrad_f32", "c"): (_k_at_least(8192), "lkg_gemm_wgrad.hip: splits > 1 (atomic_out) only with k >= 8192"),
    ("lkg_gemm_longk_f32", "c"): (_k_at_least(2048), "lkg_gemm_wgrad.hip lkg_gemm_longk_f32: splits = min(.., k / 1024) > 1: atomic_out"),
    ("lkg_gemm_smallm_f32", "c"): (None, "lkg_gemm_wgrad.hip smallm_wgrad_kernel: C is zeroed, then atomicAdd(c + row * ldc + col, ...)"),
    ("lkg_act_layernorm_bwd_f32", "g_gamma"): (None, "lkg_rowwise.hip: atomicAdd(g_gamma + e, ...)"),
    ("lkg_act_layernorm_bwd_f32", "g_beta"): (None, "lkg_rowwise.hip: atomicAdd(g_beta + e, ...)"),
    ("lkg_colsum_f32", "out"): (None, "lkg_rowwise.hip: atomicAdd(out + c, ...)"),
    ("lkg_colsum_weighted_f32", "out_sum"): (None, "lkg_rowwise.hip: atomicAdd(out_sum + c, ...)"),
    ("lkg_colsum_weighted_f32", "out_w"): (None, "lkg_rowwise.hip: atomicAdd(out_w + c * ld_out + j, ...)"),
    # slots handed out by an atomic counter: the order of a buffer's entries, not their set, depends on the schedule
    ("lkg_topk_select_f32", "ws_s"): (None, "lkg_topk.hip: slot = atomicAdd(&sm.qn[row], 1)"),
    ("lkg_topk_select_f32", "ws_i"): (None, "lkg_topk.hip: slot = atomicAdd(&sm.qn[row], 1)"),
    ("lkg_pair_mlp_select_f32", "ws_s"): (None, "lkg_pairmlp.hip: slot = atomicAdd(&sm.tk.qn[qi], 1)"),
    ("lkg_pair_mlp_select_f32", "ws_i"): (None, "lkg_pairmlp.hip: slot = atomicAdd(&sm.tk.qn[qi], 1)"),
    ("lkg_accept_emit_f32", "out_ids"): (None, "lkg_accept.hip: slot = atomicAdd(cursor + grow, 1)"),
    ("lkg_accept_emit_f32", "out_scores"): (None, "lkg_accept.hip: slot = atomicAdd(cursor + grow, 1)"),
    ("lkg_accept_emit_f32", "out_values"): (None, "lkg_accept.hip: slot = atomicAdd(cursor + grow, 1)"),
    **{("lkg_pair_mlp_accept_append_f32", out): (None, "lkg_pairmlp.hip: slot = atomicAdd(gcursor, 1ull)")
       for out in ("out_rows", "out_ids", "out_logits")},
    **{("lkg_pair_mlp_accept_emit_f32", out): (None, "lkg_pairmlp.hip: slot = atomicAdd(cursor + grow, 1)")
       for out in ("out_ids", "out_scores", "out_logits")},
}

# Operands whose rows an id list selects: (entry point, operand) -> the id arguments.  A wide pass of such an operand must
# have ids that hit a row at >= 2^32 elements and a row in [2^31, 2^32) elements, or the pass proves nothing and fails.
GATHERED = {
    ("lkg_transe_score_fwd_f32", "emb"): ("h", "pos_t", "neg_t"), ("lkg_transe_score_bwd_f32", "emb"): ("h", "pos_t", "neg_t"),
    ("lkg_dot_score_fwd_f32", "emb"): ("h", "pos_t", "neg_t"), ("lkg_dot_score_bwd_f32", "emb"): ("h", "pos_t", "neg_t"),
    ("lkg_gather_rows_f32", "src"): ("idx",), ("lkg_gather_rows_range_f32", "src"): ("idx",),
    ("lkg_rank_queries_f32", "p"): ("ids",), ("lkg_triple_scores_f32", "p"): ("q_idx", "c_idx"),
    ("lkg_relation_scores_f32", "p"): ("q_idx", "c_idx"),
    ("lkg_spmm_csr_f32", "x"): ("col",), ("lkg_spmm_csr_fused_f32", "x"): ("col",),
}

# a block stride that goes with an operand's row stride: blocks inside a row (0 < stride < ld) need nothing; blocks stacked
# one behind the other (stride = rows per block * ld) get the stride of the placement in use
COUPLED = {
    ("lkg_grouped_gemm_f32", "b"): "stride_b", ("lkg_grouped_gemm_f32", "c"): "stride_c",
    ("lkg_relation_scores_f32", "p"): "rel_stride",
    ("lkg_relation_loss_fwd_f32", "u"): "rel_stride", ("lkg_relation_loss_bwd_f32", "u"): "rel_stride",
}

# operands that are another operand by contract ("the gate blends its FIRST K-panel: gate_x must be a[0]"): they follow it
ALIASED = {("lkg_gemm_tall_f32", "gate_x"): "a"}

# flat arguments that are scratch, not results
SCRATCH = ("workspace", "stream", "dbg")


# ----------------------------------------------------------------------------- the harness (device)
class Pass:
    def __init__(self, target):
        self.target = target                    # (entry point, operand label), None for the twin pass
        self.log = []                           # per launch: (entry point, input checksums, [(name, bits)])
        self.pairs = []                         # the (entry point, operand label) resolved, in order of first launch
        self.hits = []                          # addresses inside the store handed to a launch for the target
        self.unresolved = {}
        self.sigs = {}                          # (entry point, operand label) -> the scalar arguments of its launches
        self.shapes = set()                     # the (n, d) placed wide
        self.aliased = None                     # the operand that followed the target by contract (gate_x = a[0])
        self.compared = 0                       # outputs of launches that received the wide operand, compared bit for bit
        self.waived = 0                         # ... and not compared, by WAIVED
        self.skipped = 0                        # ... and not compared because the launch's inputs differed from the twin pass's
        self.bands = [False, False]             # a gathered operand: an id hit a row at >= 2^b / in [2^(b-1), 2^b) elements
        self.ids_seen = 0


class Harness:
    """See the module docstring.  `native` is literalkg_amd._native, `store` the device store of new_store(32, device)."""

    def __init__(self, native, store, wrap_bits=32):
        import torch
        self.torch, self.N, self.store, self.b = torch, native, store, wrap_bits
        self.sigs = strided_operands()
        self.protos = prototypes()
        self.covered = {}                       # (entry, label) -> shapes run wide, in passes that were judged and passed
        self.judged = {}                        # (entry, label) -> [compared, waived, skipped]: outputs of the launches
                                                # that received the operand wide
        self.passes = 0
        self.done = {}                          # (entry, label) -> the launches (scalar arguments) already run wide
        self.registry = {}

    def index(self, entry, param):
        return next(p.index for p in self.protos[entry] if p.name == param)

    # -- resolving a raw address to the caller's tensor
    def _rows(self, addr, ld, stacked=None):
        """the (n, d) row view of the float32 tensor the caller passed at this address, or None.  `stacked`: the value of the
        block stride that goes with this operand (COUPLED): a (blocks, rows, d) tensor of uniformly stacked blocks is taken
        as blocks * rows rows."""
        torch = self.torch
        for t in sorted(self.registry.get(addr, ()), key=lambda x: x.numel()):
            t = t.data                          # (not .detach(): the copy back must not count as an in-place change)
            if t.dtype != torch.float32 or t.dim() < 2 or t.numel() == 0:
                continue
            if stacked and stacked >= ld:
                if t.dim() == 3 and t.stride(2) == 1 and t.stride(1) == ld and t.stride(0) == stacked == t.shape[1] * ld \
                        and ld >= t.shape[2]:
                    return torch.as_strided(t, (t.shape[0] * t.shape[1], t.shape[2]), (ld, 1), t.storage_offset())
                continue
            if t.shape[0] < 2:
                continue
            d = int(np.prod(t.shape[1:]))
            if not t[0].is_contiguous() or t.stride(0) != ld or ld < d:
                continue
            return torch.as_strided(t, (t.shape[0], d), (ld, 1), t.storage_offset())
        return None

    def _overlapped(self, rows, args_in, own):
        """whether an argument other than these operands' own pointers lies inside their tensors: a second output written
        into the same tensor (g_gpre | g_zpre side by side) would be overwritten by the copy back"""
        for r in rows:
            lo = r.data_ptr()
            hi = lo + 4 * ((r.shape[0] - 1) * r.stride(0) + r.shape[1])
            for i, a in enumerate(args_in):
                if i not in own and isinstance(a, int) and not isinstance(a, bool) and lo <= a < hi and a > 2 ** 32:
                    return True
        return False

    def _block(self, rows_list):
        """one (n, D) block of the operands that share a stride: a single operand as it is, several side by side"""
        torch = self.torch
        if len(rows_list) == 1:
            return rows_list[0], [0]
        n = rows_list[0].shape[0]
        offs, at = [], 0
        for r in rows_list:
            offs.append(at)
            at += twin_ld(r.shape[1])
        block = torch.full((n, at - 4), -1, dtype=torch.int32, device=rows_list[0].device).view(torch.float32)
        for r, o in zip(rows_list, offs):
            block[:, o:o + r.shape[1]] = r
        return block, offs

    @contextlib.contextmanager
    def boundary(self, ps, twin_pass):
        """the C boundary for the length of one pass: _native.ptr records which tensor each address came from, _native.call
        hands every launch to self._launch, ops._f32_rows records the tall GEMM's panels"""
        torch, N = self.torch, self.N
        real_call, real_ptr = N.call, N.ptr
        self.registry = {}

        def ptr(t):
            p = real_ptr(t)
            if isinstance(t, torch.Tensor) and t.is_cuda and p:
                self.registry.setdefault(p, []).append(t)
            return p

        def call(name, *args):
            try:
                with torch.no_grad():
                    return self._launch(ps, twin_pass, real_call, name, list(args))
            finally:
                self.registry = {}

        from literalkg_amd import ops
        real_rows = ops._f32_rows

        def f32_rows(t):                        # (the tall GEMM's panels reach the library in host arrays of .data_ptr())
            r = real_rows(t)
            if r.is_cuda and r.numel():
                self.registry.setdefault(r.data_ptr(), []).append(r)
            return r

        N.call, N.ptr, ops._f32_rows = call, ptr, f32_rows
        try:
            yield
        finally:
            N.call, N.ptr, ops._f32_rows = real_call, real_ptr, real_rows
            self.registry = {}

    @contextlib.contextmanager
    def running(self, target, twin_pass=None):
        """one pass: the twin pass (target None) or the pass with `target` wide, compared against `twin_pass`"""
        import invariance as V
        torch = self.torch
        ps = Pass(target)
        torch.cuda.synchronize()
        if target is not None:
            poison(self.store)
        torch.manual_seed(0)
        with self.boundary(ps, twin_pass), V.poisoned(0xFF):
            yield ps
        torch.cuda.synchronize()
        self.passes += 1
        if target is not None:
            assert ps.hits, f"{target}: no launch received an address inside the store for this operand"
            if not all_poison(self.store):
                raise AssertionError(f"{target}: a cell outside the operand was written: element offset "
                                     f"{first_stain(self.store, self.b)} from the base is no longer 0xFF")
            assert twin_pass is None or len(ps.log) == len(twin_pass.log), \
                f"{target}: {len(ps.log)} launches, {len(twin_pass.log)} in the twin pass"
            if target in GATHERED:
                assert ps.ids_seen and all(ps.bands), \
                    (f"{target}: the id lists of this case ({ps.ids_seen} ids) select no row at >= 2^{self.b} elements or none "
                     f"in [2^{self.b - 1}, 2^{self.b}) of the wide operand (hit: {ps.bands}): the pass proves nothing")

    def _launch(self, ps, twin_pass, real_call, name, args):
        import invariance as V
        torch = self.torch
        ops = self.sigs.get(name)
        if ops is None:
            return real_call(name, *args)
        after, shapes = [], None
        args_in = tuple(args)
        for op in ops:
            key = (name, op.label)
            if op.array:
                self._arrays(ps, op, name, args, after)
                continue
            ld = args[op.ld_index]
            addrs = [args[i] for i in op.ptr_index]
            alias = ALIASED.get(key)
            if alias and addrs[0]:                                      # (the gate's x IS the first panel, by contract)
                a_in, a_now = args_in[self.index(name, alias)], args[self.index(name, alias)]
                if a_in is not None and int(a_in[0] or 0) == addrs[0]:
                    args[op.ptr_index[0]], args[op.ld_index] = int(a_now[0]), int(args[self.index(name, "ld" + alias)][0])
                    if ps.target == (name, alias + "[0]") and inside(self.store, args[op.ptr_index[0]]):
                        ps.aliased = key
                    continue
            if any(a is None or a == 0 for a in addrs):
                continue
            coupled = COUPLED.get(key)
            c_index = next(p.index for p in self.protos[name] if p.name == coupled) if coupled else None
            stacked = args[c_index] if coupled else None
            rows = [self._rows(a, ld, stacked) for a in addrs]
            if any(r is None for r in rows):
                ps.unresolved[key] = ps.unresolved.get(key, 0) + 1
                continue
            if not all(op.const) and self._overlapped(rows, args_in, op.ptr_index):
                ps.unresolved[key] = ps.unresolved.get(key, 0) + 1      # (another argument points into this output's tensor)
                continue
            short = min(r.shape[0] for r in rows)                       # (ph / pp / pn: views of one tensor, a third each)
            rows = [r[:short] for r in rows]
            block, offs = self._block(rows)
            wide = ps.target == key and block.shape[0] >= 9
            if block.shape[0] >= 9 and key not in ps.pairs:
                ps.pairs.append(key)
            view = place(self.store, block, self.b) if wide else twin(block)
            for i, r, o in zip(op.ptr_index, rows, offs):
                args[i] = view.data_ptr() + 4 * o
            args[op.ld_index] = view.stride(0)
            if stacked and stacked >= ld:
                args[c_index] = stacked // ld * view.stride(0)
            sig = (name,) + tuple((a is None) if p.pointer else a for p, a in zip(self.protos[name], args_in))
            if block.shape[0] >= 9:
                ps.sigs.setdefault(key, set()).add(sig)
            if wide:
                ps.hits += [args[i] for i in op.ptr_index if inside(self.store, args[i])]
                shapes = tuple(block.shape)
            for r, o, const, nm in zip(rows, offs, op.const, op.names):
                after.append((nm, r, view[:, o:o + r.shape[1]], const, wide))
            if wide:
                after.append((None, None, view, None, True))            # (the placement itself, cleared last)
        flat = []                                                       # the flat arguments the caller passed as tensors
        done = {i for op in ops for i in op.ptr_index}
        for p in self.protos[name]:
            if p.pointer and p.index not in done and p.name not in SCRATCH and "void" not in p.ctype \
                    and isinstance(args[p.index], int) and not isinstance(args[p.index], bool):
                for t in self.registry.get(args[p.index], ())[:1]:
                    flat.append((p, t.data))
        # what the launch reads, outputs that are added into included: the twin pass's launch is comparable only if these agree
        sums = [r.view(torch.int32).sum(dtype=torch.int64) for nm, r, v, const, w in after if nm is not None] + \
               [t.reshape(-1).contiguous().view(torch.uint8).sum(dtype=torch.int64) for p, t in flat if t.numel()]
        checks = torch.stack(sums).tolist() if sums else []
        received = any(w for nm, r, v, const, w in after if nm is None) or ps.aliased is not None and ps.target is not None \
            and ps.target[0] == name
        if received and ps.target in GATHERED:
            self._bands(ps, name, args_in, next(v for nm, r, v, const, w in after if nm is None))
        real_call(name, *args)
        outs = []
        for nm, r, v, const, wide in after:
            if nm is None:
                clear(v)
            elif const:
                assert not wide or carries(v, r), f"{name}: the input {nm} no longer carries the bits it was given"
            else:
                r.copy_(v)
                outs.append((nm, r.clone()))
        outs += [(p.name, t.clone()) for p, t in flat if not p.const]
        by_name = {p.name: a for p, a in zip(self.protos[name], args_in)}
        kept = []
        for nm, bits in outs:
            when = WAIVED.get((name, nm), (False,))[0]
            if when is None or (when and when(by_name)):
                ps.waived += received
            else:
                kept.append((nm, bits))
        idx = len(ps.log)
        ps.log.append((name, checks, kept if twin_pass is None else None))
        if twin_pass is not None and idx < len(twin_pass.log):
            t_name, t_checks, t_outs = twin_pass.log[idx]
            assert t_name == name, f"launch {idx} is {name}, {t_name} in the twin pass"
            if t_checks != checks:
                ps.skipped += received * len(kept)                      # (downstream of an output that is added with atomics)
            else:
                assert [nm for nm, _ in kept] == [nm for nm, _ in t_outs], \
                    f"launch {idx} {name}: outputs {[nm for nm, _ in kept]}, {[nm for nm, _ in t_outs]} in the twin pass"
                for (nm, got), (_, want) in zip(kept, t_outs):
                    V.same_bits(got, want, f"{ps.target} wide, launch {idx} {name}: {nm}")
                    ps.compared += received
        if shapes is not None:
            ps.shapes.add(shapes)

    def _bands(self, ps, name, args_in, view):
        """which rows of the wide gathered operand this launch's id lists select"""
        torch = self.torch
        by_name = {p.name: a for p, a in zip(self.protos[name], args_in)}
        n, ld = view.shape[0], view.stride(0)
        ids = []
        for param in GATHERED[ps.target]:
            for t in self.registry.get(by_name[param] or 0, ())[:1]:
                ids.append(t.data.reshape(-1).long())
        if name == "lkg_gather_rows_f32" and not ids:                   # (idx NULL: the rows are perm's, or 0 .. n - 1)
            perm = self.registry.get(by_name["perm"] or 0, ())[:1]
            ids = [perm[0].data.reshape(-1).long()] if perm else [torch.arange(by_name["n"], device=view.device)]
        if not ids:
            return
        rows = torch.cat(ids)
        if name == "lkg_gather_rows_range_f32":
            rows = rows[(rows >= by_name["row_lo"]) & (rows < by_name["row_hi"])] - by_name["row_lo"]
        if name == "lkg_relation_scores_f32" and by_name["rel_stride"] >= by_name["ldp"]:
            per = by_name["rel_stride"] // by_name["ldp"]               # (stacked blocks: every relation's copy of the row)
            rows = (rows[:, None] + per * torch.arange(n // per, device=rows.device)[None, :]).reshape(-1)
        off = rows[(rows >= 0) & (rows < n)] * ld
        ps.ids_seen += int(off.numel())
        ps.bands[0] |= bool((off >= 1 << self.b).any())
        ps.bands[1] |= bool(((off >= 1 << (self.b - 1)) & (off < 1 << self.b)).any())

    def _arrays(self, ps, op, name, args, after):
        """the tall GEMM's panels: a host array of pointers and one of strides, each panel an operand of its own label"""
        import ctypes as C
        torch = self.torch
        ptrs, lds = args[op.ptr_index[0]], args[op.ld_index]
        if ptrs is None or lds is None:
            return
        new_p, new_l = (C.c_void_p * len(ptrs))(*list(ptrs)), (C.c_int64 * len(lds))(*list(lds))
        for j in range(len(ptrs)):
            addr, ld = int(ptrs[j] or 0), int(lds[j])
            if not addr:
                continue
            key = (name, f"{op.label}[{j}]")
            rows = self._rows(addr, ld)
            if rows is None:
                ps.unresolved[key] = ps.unresolved.get(key, 0) + 1
                continue
            wide = ps.target == key and rows.shape[0] >= 9
            if rows.shape[0] >= 9:
                if key not in ps.pairs:
                    ps.pairs.append(key)
                ps.sigs.setdefault(key, set()).add((name,) + tuple(a for p, a in zip(self.protos[name], args)
                                                                   if not p.pointer))
            view = place(self.store, rows, self.b) if wide else twin(rows)
            new_p[j], new_l[j] = view.data_ptr(), view.stride(0)
            after.append((f"{op.label}[{j}]", rows, view, True, wide))
            if wide:
                ps.hits.append(view.data_ptr())
                ps.shapes.add(tuple(rows.shape))
                after.append((None, None, view, None, True))
        args[op.ptr_index[0]], args[op.ld_index] = new_p, new_l

    # -- cases
    def case(self, run, judge=None, what=""):
        """run() once with every operand on its twin placement and once per strided operand with that operand alone wide.
        judge(result, mode) holds a run to its family's float64 oracle and returns {name: tensor} of the deterministic
        results, which must carry the twin pass's bits; a body that judges itself (run returns None) needs no judge."""
        import invariance as V
        with self.running(None) as tw:
            res = run()
        base = judge(res, f"{what} twin") if judge is not None else {}
        assert tw.pairs or tw.unresolved, f"{what}: no launch took a row-strided operand"
        for target in tw.pairs:
            if tw.sigs.get(target, set()) <= self.done.get(target, set()):
                continue                        # every launch of this operand ran wide before, with the same scalar arguments
            with self.running(target, tw) as ps:
                res = run()
            mode = f"{what} wide {target[0]} {target[1]}"
            out = judge(res, mode) if judge is not None else {}
            assert out.keys() == base.keys(), mode
            for name in base:
                V.same_bits(out[name], base[name], f"{mode}: {name}")
            for pair in (target,) + ((ps.aliased,) if ps.aliased else ()):
                self.covered.setdefault(pair, set()).update(ps.shapes)
                tally = self.judged.setdefault(pair, [0, 0, 0])
                for k, v in enumerate((ps.compared, ps.waived, ps.skipped)):
                    tally[k] += v
            self.done.setdefault(target, set()).update(tw.sigs.get(target, ()))
        return tw
