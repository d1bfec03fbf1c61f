"""CPU: the wide placement's geometry for every shape the GPU module runs, the header ledger's parser, and the placement's
checks against planted faults at wrap_bits = 16 (a numpy store of 436 KB), in the manner of test_index_measures_host.py.

The stand-in kernels address a small model of memory (Mem: the store and the twin buffers, each access bounds-checked) by
raw address, row stride and an offset function, as a HIP kernel does: the correct one computes offsets in int64, the
faulty ones send the element offset through np.int16 / np.uint16 or the byte offset through the same.  protocol() is the
device harness's sequence in small: a twin run, then one run per operand with that operand alone wide, and after each the
pointer record, the inputs' bits, the result's bits against the twin run, the poison of the whole store, and the twin run
against float64."""
import numpy as np
import pytest

import wide_cases as W

B = 16


# ----------------------------------------------------------------------------- geometry
@pytest.mark.parametrize("n,d", W.SHAPES)
def test_geometry_of_every_device_shape(n, d):
    """No store is allocated: the row stride geometry() picks meets every property of the placement (W.check_geometry)."""
    ld = W.geometry(n, d, 32)
    assert W.check_geometry(n, d, ld, 32)
    assert ld % 4 == 0 and (n - 1) * ld + d <= W.span_elems(32) + W.tail_elems(32)
    got = list(W.bands(n, ld, 32).values())
    assert all(c >= 2 for c in got[:3]) and got[3] >= (2 if n >= 15 else 1), got
    o = np.arange(n, dtype=np.int64) * ld
    for model in W.WRAPS:
        w = W.wrapped(o, model, 32)
        moved = np.flatnonzero(w != o)
        assert moved.size >= 2, model                               # every wrap model moves at least two rows
        for i in moved[[0, -1]]:                                    # ... into the store, and off every row's cells
            assert -W.pad_elems(32) <= w[i] and w[i] + d <= W.span_elems(32) + W.tail_elems(32)
            assert w[i] + d <= 0 or (d <= w[i] % ld <= ld - d), (model, int(i))


def test_five_bands_of_two_rows_need_fifteen_rows():
    """The arithmetic of the module docstring, by exhaustion at 16 bits: below 15 rows no stride of the span has two rows
    in each band; from 15 rows on geometry() finds one."""
    for n in range(9, 15):
        for ld in range(4, W.span_elems(B) // (n - 1) + 1, 4):
            assert min(W.bands(n, ld, B).values()) < 2, (n, ld)
    for n in (15, 16, 33, 257):
        assert min(W.bands(n, W.geometry(n, 5, B), B).values()) >= 2
    assert W.store_elems(32) * 4 < 28.6e9 and W.span_elems(32) > 2 ** 32 * 8 // 7 and W.pad_elems(32) == 2 ** 31


def test_wrap_models_are_numpys_casts():
    o = np.arange(0, W.span_elems(B) + 300, 7, dtype=np.int64)
    assert np.array_equal(W.wrapped(o, "int element", B), o.astype(np.int16).astype(np.int64))
    assert np.array_equal(W.wrapped(o, "uint element", B), o.astype(np.uint16).astype(np.int64))
    assert np.array_equal(W.wrapped(o, "int byte", B), (4 * o).astype(np.int16).astype(np.int64) // 4)
    assert np.array_equal(W.wrapped(o, "uint byte", B), (4 * o).astype(np.uint16).astype(np.int64) // 4)


def test_a_bad_stride_is_refused():
    n, d = 33, 7
    ld = W.geometry(n, d, B)
    assert not W.geometry_faults(n, d, ld, B)
    assert W.geometry_faults(n, d, ld + 2, B)                                       # no multiple of 4
    assert W.geometry_faults(n, d, 4 * -(-d // 4) + 4, B)                           # the twin's stride: no row past 2^b
    assert any("image" in f for f in W.geometry_faults(n, d, (1 << B) // 16, B))   # rows that wrap onto each other
    with pytest.raises(ValueError):
        W.geometry(8, d, B)


# ----------------------------------------------------------------------------- the headers
def test_header_ledger_parser():
    ops = W.strided_operands()
    pairs = W.ledger_pairs()
    assert len(ops) >= 72 and len(pairs) >= 204
    assert ("lkg_gather_rows_f32", "src") in pairs and ("lkg_gather_rows_f32", "dst") in pairs
    assert ("lkg_softmax_all_weights_f32", "v") in pairs and ("lkg_nssa_bwd_f32", "dn") in pairs
    assert ("lkg_dense_score_fwd_f32", "ph+pp+pn") in pairs and ("lkg_gemm_tall_f32", "a") in pairs
    tall = {o.label: o for o in ops["lkg_gemm_tall_f32"]}
    assert tall["a"].array and tall["b"].array and not tall["c"].array and tall["c"].const == (False,)
    gather = {o.label: o for o in ops["lkg_gather_rows_f32"]}
    assert gather["src"].const == (True,) and gather["dst"].const == (False,)
    from literalkg_amd import _native as N
    tables = N.PROTOTYPES
    protos = W.prototypes()
    for entry in ops:                                               # the argument positions are those of the ctypes table
        assert len(protos[entry]) == len(tables[entry]), entry
        for o in ops[entry]:
            assert tables[entry][o.ld_index] is (N.vp if o.array else N.i64), (entry, o)
            assert all(tables[entry][i] is N.vp for i in o.ptr_index), (entry, o)
    for entry, out in W.WAIVED:                                      # every waived output is an output of its entry point
        assert any(q.name == out and q.pointer and not q.const for q in protos[entry]), (entry, out)
    for (entry, operand), ids in W.GATHERED.items():
        assert (entry, operand) in pairs and all(any(q.name == i for q in protos[entry]) for i in ids), (entry, operand)


# ----------------------------------------------------------------------------- planted faults
class Mem:
    """the address space of the stand-in kernels: a few flat float32 arrays; an access outside all of them raises"""

    def __init__(self, *flats):
        self.flats = list(flats)

    def row(self, addr, d):
        for f in self.flats:
            lo = f.ctypes.data
            if lo <= addr and addr + 4 * d <= lo + 4 * f.size:
                i = (addr - lo) // 4
                return f[i:i + d]
        raise MemoryError(f"a stand-in kernel left its allocations at {addr:#x}")


OFFSETS = {
    "int64": lambda o: o,
    "int element": lambda o: int(np.array(o).astype(np.int16)),
    "uint element": lambda o: int(np.array(o).astype(np.uint16)),
    "int byte": lambda o: int(np.array(4 * o).astype(np.int16)) // 4,
    "uint byte": lambda o: int(np.array(4 * o).astype(np.uint16)) // 4,
}


def k_gather(mem, off, n, d, src, lds, idx, dst, ldd, extra=0):
    for i in range(n):
        mem.row(dst + 4 * off(i * ldd), d)[:] = mem.row(src + 4 * off(int(idx[i]) * lds), d)


def k_map(mem, off, n, d, src, lds, idx, dst, ldd, extra=0):
    for i in range(n):
        mem.row(dst + 4 * off(i * ldd), d)[:] = mem.row(src + 4 * off(i * lds), d) * np.float32(2) + np.float32(1)


def k_write(mem, off, n, d, src, lds, idx, dst, ldd, extra=0):
    for i in range(n):
        row = mem.row(dst + 4 * off(i * ldd), d + extra)
        row[:d] = np.float32(i) + np.arange(d, dtype=np.float32) / 8
        row[d:] = 0.0                                               # (extra cells past d: the planted overrun)


KERNELS = {"gather": k_gather, "map": k_map, "write": k_write}


def reference(kind, x, idx):
    x64 = x.astype(np.float64)
    if kind == "gather":
        return x64[idx]
    if kind == "map":
        return x64 * 2 + 1
    return np.arange(x.shape[0])[:, None] + np.arange(x.shape[1])[None, :] / 8.0


def protocol(kind, n, d, offsets="int64", copies=False, extra=0, seed=0):
    """the device harness in small; returns the reasons the checks found ({} when all passed), per wide operand"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(np.float32)
    idx = rng.integers(0, n, n)
    idx[:4] = (n - 1, n - 2, n // 2, n // 2 + 1)                     # ids that hit the rows past 2^b and in [2^(b-1), 2^b)
    store = W.poison(W.new_store(B))
    off = OFFSETS[offsets]

    def run(wide):
        xs = W.place(store, x, B) if wide == "src" else W.twin(x)
        out0 = np.empty((n, d), dtype=np.float32)
        W.clear(out0)
        os_ = W.place(store, out0, B) if wide == "dst" else W.twin(out0)
        mem = Mem(store, W.owner(xs), W.owner(os_))
        src = xs
        if copies:                                                   # a wrapper that packs its operand first
            src = np.ascontiguousarray(xs)
            mem.flats.append(src.reshape(-1))
        args = (W.address(src), src.strides[0] // 4, idx, W.address(os_), os_.strides[0] // 4)
        launches = [{"src": args[0], "dst": args[3]}]                # the pointer record
        KERNELS[kind](mem, off, n, d, *args, extra=extra)
        got = np.array(os_)
        found = set()
        if wide is not None:
            if not any(W.inside(store, rec[wide]) for rec in launches):
                found.add("pointer")
            if not W.carries(xs, x):
                found.add("input")
            W.clear(xs if wide == "src" else os_)
            if not W.all_poison(store):
                found.add(f"poison at {W.first_stain(store, B)}")
                W.poison(store)
        return got, found

    twin_out, _ = run(None)
    ref = reference(kind, x, idx)
    assert np.array_equal(twin_out.astype(np.float64), ref.astype(np.float32).astype(np.float64)), "the twin against float64"
    reasons = {}
    for wide in ("src", "dst"):
        got, found = run(wide)
        if not np.array_equal(got.view(np.int32), twin_out.view(np.int32)):
            found.add("bits")
        if found:
            reasons[wide] = found
    return reasons


SHAPES16 = [(9, 5), (33, 8), (257, 5)]


@pytest.mark.parametrize("n,d", SHAPES16)
@pytest.mark.parametrize("kind", list(KERNELS))
def test_correct_stand_ins_pass(kind, n, d):
    assert protocol(kind, n, d) == {}


@pytest.mark.parametrize("n,d", SHAPES16)
@pytest.mark.parametrize("offsets", ["int element", "uint element", "int byte", "uint byte"])
@pytest.mark.parametrize("kind", list(KERNELS))
def test_a_narrow_offset_is_caught(kind, offsets, n, d):
    """A wrapped read returns poison: the result's bits differ.  A wrapped write lands in poison: the result's rows are
    missing and the store is stained.  Never a MemoryError: the wrapped access stays inside the store."""
    reasons = protocol(kind, n, d, offsets=offsets)
    if kind != "write":
        assert "bits" in reasons.get("src", ()), reasons
    assert "bits" in reasons.get("dst", ()) and any(r.startswith("poison") for r in reasons["dst"]), reasons
    assert not any("pointer" in r or "input" in r for v in reasons.values() for r in v), reasons


@pytest.mark.parametrize("kind", ["gather", "map"])
def test_a_silent_copy_is_caught_by_the_pointer_record(kind):
    assert protocol(kind, 33, 8, copies=True) == {"src": {"pointer"}}


def test_a_write_past_d_is_caught_by_the_poison_check():
    reasons = protocol("write", 33, 8, extra=1)
    assert set(reasons) == {"dst"} and reasons["dst"] == {"poison at 8"}, reasons


def test_placement_on_the_numpy_store():
    store = W.poison(W.new_store(B))
    assert store.nbytes < 500_000 and W.all_poison(store)
    x = np.arange(33 * 8, dtype=np.float32).reshape(33, 8)
    v = W.place(store, x, B)
    assert W.address(v) % 16 == 0 and v.strides[0] % 16 == 0 and W.carries(v, x) and W.inside(store, W.address(v))
    assert 32 * v.strides[0] // 4 >= 1 << B and not W.all_poison(store)
    t = W.twin(x)
    assert t.strides[0] == 4 * 12 and W.address(t) % 16 == 0 and W.carries(t, x) and not W.inside(store, W.address(t))
    W.clear(v)
    assert W.all_poison(store)
