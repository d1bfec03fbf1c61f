"""CPU: the flush pass of guard_cases.py can tell -- planted faults with correct twins, the placement's geometry, the union
rule, and the ledger's derivation from include/literalkg_hip.h, in the manner of test_wide_placement_host.py.

The stand-in entry points are numpy over raw addresses (np.ctypeslib.as_array behind Flush.table, which bounds-checks
every access against the arena of the launch and the slabs the test owns).  The caller's arrays are slices of slabs with a
margin of ordinary numbers on both sides -- "whatever the allocator had there" -- so a planted over-run of the plain pass
stays inside the slab, reads plausible values and is not noticed there, as on the device; the flush pass must notice.

The masked over-read (a 16-byte load whose last lane runs past an odd length and is selected away) PASSES, by design: its
value reaches nothing, and the harness compares values.  test_a_masked_over_read_passes states it."""
import numpy as np
import pytest

import guard_cases as G
import wide_cases as W

HEADER = """
int lkg_t_map_f32(int64_t n, const float *src, float *dst, int64_t fault, int64_t home, void *stream);
int lkg_t_rows_f32(int64_t n, int32_t d, const float *src, int64_t lds, float *dst, int64_t ldd, int64_t fault, void *stream);
int lkg_t_count_i64(int64_t n, const int64_t *ids, int64_t *counts, int32_t *cursor, int64_t fault, void *stream);
int lkg_t_shape(int64_t n, const float *src);
"""
MARGIN = 64                                     # elements of ordinary numbers on both sides of every caller array


class Native:
    """call / ptr of a library whose entry points are Python functions over addresses"""

    def __init__(self):
        self.entries = {}
        self.launched = []
        self.stand_in = np.zeros(64, np.float32)            # (as _native.ptr: an empty operand's address, never dereferenced)

    def ptr(self, a):
        if a is None:
            return None
        return a.ctypes.data if a.size else self.stand_in.ctypes.data

    def call(self, name, *args):
        self.launched.append(name)
        self.entries[name](*args)


@pytest.fixture(scope="module")
def protos(tmp_path_factory):
    d = tmp_path_factory.mktemp("include")
    (d / "standins.h").write_text(HEADER)
    return W.prototypes(str(d))


def world(protos):
    """a harness over the stand-in library; slabs: the buffers the test owns"""
    N = Native()
    H = G.Flush(N, protos, W.strided_operands(protos), host=True)
    slabs = []

    def f32(addr, n):
        return H.table(addr, 4 * n, slabs).view(np.float32)

    def k_map(n, src, dst, fault, home, stream):
        x = f32(src, n).copy()
        if fault == "read past the end":
            x[n - 1] = f32(src + 4 * n, 1)[0]
        if fault == "read before the start":
            x[0] = f32(src - 4, 1)[0]
        if fault in ("float4 used", "float4 masked"):
            n4 = -(-n // 4) * 4
            lanes = f32(src, n4).copy()                                     # whole 16-byte groups: the last runs past n
            keep = np.arange(n4) < n
            if fault == "float4 masked":
                lanes = np.where(keep, lanes, np.float32(0))                # selected away: the value reaches nothing
            x = (lanes.reshape(-1, 4) + np.float32(0) * lanes.reshape(-1, 4)[:, 3:4]).reshape(-1)[:n] \
                if fault == "float4 used" else lanes[:n]
        out = x * np.float32(2) + np.float32(1)
        f32(home if fault == "write to the caller's address" else dst, n)[:] = out
        if fault == "write past the end":
            f32(dst + 4 * n, 1)[0] = 0.0
        if fault == "write before the start":
            f32(dst - 4, 1)[0] = 0.0
        if fault == "modify a const input":
            f32(src, n)[0] += np.float32(1)

    def k_rows(n, d, src, lds, dst, ldd, fault, stream):
        for i in range(n):
            f32(dst + 4 * i * ldd, d)[:] = f32(src + 4 * i * lds, d) * np.float32(2) + np.float32(1)
            if fault == "write in the column gap" and i == 0:
                f32(dst + 4 * (i * ldd + d), 1)[0] = 0.0

    def k_count(n, ids, counts, cursor, fault, stream):
        i64 = H.table(ids, 8 * n, slabs).view(np.int64)
        c = H.table(counts, 8 * n, slabs).view(np.int64)
        c[:] = np.bincount(i64, minlength=n)[:n]
        cur = H.table(cursor, 4, slabs).view(np.int32)
        cur[0] = n
        if fault == "cursor one slot on":
            H.table(cursor + 4, 4, slabs).view(np.int32)[0] = n

    N.entries = {"lkg_t_map_f32": k_map, "lkg_t_rows_f32": k_rows, "lkg_t_count_i64": k_count,
                 "lkg_t_shape": lambda n, src: None}
    return N, H, slabs


def carve(slabs, n, dtype=np.float32, seed=0, fill=None, off=0):
    """an n-element array in the middle of a slab of ordinary numbers, `off` elements off the slab's own alignment"""
    rng = np.random.default_rng(seed)
    slab = rng.standard_normal(n + 2 * MARGIN + off).astype(dtype) if fill is None else np.full(n + 2 * MARGIN + off, fill, dtype)
    slabs.append(slab)
    return slab[MARGIN + off:MARGIN + off + n]


def run_map(protos, n, fault, off=0):
    N, H, slabs = world(protos)

    def run():
        src = carve(slabs, n, seed=n, off=off)
        dst = carve(slabs, n, fill=0.0, off=off)
        N.call("lkg_t_map_f32", n, N.ptr(src), N.ptr(dst), fault, N.ptr(dst), None)
        return src, dst

    def judge(res, mode):
        return dict(dst=res[1])

    fl = H.case(run, judge, f"map {fault}")
    return H, fl


MAP_FAULTS = {
    "write past the end": r"lkg_t_map_f32: parameter dst: the band behind was written, the first byte at offset 0 ",
    "write before the start": r"lkg_t_map_f32: parameter dst: the band in front was written, the first byte at offset -4 ",
    "read past the end": "elements differ",
    "read before the start": "elements differ",
    "float4 used": "elements differ",
    "modify a const input": r"lkg_t_map_f32: parameter src: const input was written, the first byte at offset [0-3] ",
    "write to the caller's address": "elements differ",
}


@pytest.mark.parametrize("n", [1, 3, 5, 65, 257])
def test_the_correct_twin_passes(protos, n):
    for off in (0, 1):                                                      # (16-byte grid, and 4 bytes off it)
        H, fl = run_map(protos, n, 0, off)
        assert fl.launches == 1 and fl.compared == 1 and not H.unresolved
        assert H.tally[("lkg_t_map_f32", "src")]["held"] == 1 and H.tally[("lkg_t_map_f32", "dst")]["held"] == 1


@pytest.mark.parametrize("n", [1, 3, 5, 65, 257])
@pytest.mark.parametrize("fault", list(MAP_FAULTS))
def test_a_planted_fault_is_caught(protos, fault, n):
    with pytest.raises(AssertionError, match=MAP_FAULTS[fault]):
        run_map(protos, n, fault)


@pytest.mark.parametrize("n", [1, 3, 5, 65, 257])
def test_a_masked_over_read_passes(protos, n):
    """THE LIMIT of the harness, stated: the last lane of a 16-byte load runs past an odd-length array and is selected
    away.  No value changes, so the flush pass passes; the same load with the lane used is caught (above)."""
    H, fl = run_map(protos, n, "float4 masked")
    assert fl.compared == 1


def run_rows(protos, n, d, ld, fault):
    N, H, slabs = world(protos)

    def run():
        src = carve(slabs, n * ld, seed=d).reshape(n, ld)[:, :d]
        dst = carve(slabs, n * ld, seed=d + 1).reshape(n, ld)[:, :d]
        N.call("lkg_t_rows_f32", n, d, N.ptr(src), ld, N.ptr(dst), ld, fault, None)
        return dst

    return H, H.case(run, lambda res, mode: dict(dst=res), f"rows {fault}")


@pytest.mark.parametrize("n,d,ld", [(2, 3, 4), (9, 5, 8), (33, 17, 24)])
def test_a_write_in_the_column_gap_is_caught_and_the_twin_passes(protos, n, d, ld):
    H, fl = run_rows(protos, n, d, ld, 0)
    assert fl.compared == 1 and H.tally[("lkg_t_rows_f32", "dst")]["held"] == 1
    with pytest.raises(AssertionError, match=rf"parameter dst: column gap was written, the first byte at offset {4 * d} "):
        run_rows(protos, n, d, ld, "write in the column gap")


def test_the_band_follows_the_widest_row_stride(protos):
    assert G.band_bytes([]) == 64 * 1024 and G.band_bytes([8]) == 64 * 1024
    assert G.band_bytes([76800]) == 2 * 4 * 76800 and G.band_bytes([8193]) == 65536 + 512


def test_every_dtype_a_counter_and_an_empty_array(protos):
    """int64 ids and counts, an int32 cursor (4 bytes: one slot on is the band), an empty id list through the stand-in
    address: extent 0, a placement of two bands."""
    for n in (0, 1, 3, 64, 65):
        for fault in (0, "cursor one slot on"):
            N, H, slabs = world(protos)
            slabs.append(N.stand_in)

            def run():
                ids = carve(slabs, n, np.int64, fill=0)
                ids[:] = np.arange(n)[::-1] % max(n, 1) if n else 0
                counts = carve(slabs, n, np.int64, fill=7)
                cursor = carve(slabs, 1, np.int32, fill=0)
                N.call("lkg_t_count_i64", n, N.ptr(ids), N.ptr(counts), N.ptr(cursor), fault, None)
                return counts, cursor

            judge = lambda res, mode: dict(counts=res[0], cursor=res[1])
            if fault:
                with pytest.raises(AssertionError, match=r"parameter cursor: the band behind was written, the first byte at offset 0 "):
                    H.case(run, judge)
            else:
                fl = H.case(run, judge)
                assert fl.launches == 1 and not H.unresolved
                assert H.tally[("lkg_t_count_i64", "cursor")]["held"] == 1 and H.tally[("lkg_t_count_i64", "ids")]["held"] == 1


def test_a_host_only_entry_point_is_passed_through(protos):
    N, H, slabs = world(protos)
    src = carve(slabs, 5)
    H.case(lambda: N.call("lkg_t_shape", 5, N.ptr(src)))
    assert N.launched == ["lkg_t_shape"] * 3 and not H.tally      # (warm-up, plain, flush)


# ----------------------------------------------------------------------------- geometry
def _item(a, name="x", const=False):
    return G.Item(name, 0, a.ctypes.data, G.span_bytes(a), const, None, a, G.storage_of(a), False)


@pytest.mark.parametrize("ext,itemsize", [(e, i) for e in (0, 1, 3, 4, 5, 511, 512, 513) for i in (1, 2, 4, 8) if e % i == 0])
def test_placement_is_congruent_and_flush(ext, itemsize):
    dtype = {1: np.uint8, 2: np.int16, 4: np.float32, 8: np.float64}[itemsize]
    slab = np.arange(1024 + ext // itemsize, dtype=np.int64).astype(dtype)
    for shift in (0, 1, 3, 16, 129):                                        # (elements off the slab's start)
        a = slab[shift:shift + ext // itemsize]
        lo = a.ctypes.data if ext else slab.ctypes.data + shift * itemsize
        it = G.Item("x", 0, lo, ext, False, None, a, G.storage_of(slab), False)
        p = G.Placed([it], slab)
        at = p.address[0] - p.base
        assert p.address[0] % 512 == lo % 512 and p.band == 64 * 1024 and p.fault() is None
        assert at >= p.band and at + ext + p.band == p.arena.shape[0]       # a whole band on both sides, nothing behind
        assert bytes(p.arena[at:at + ext]) == a.tobytes()
        assert (p.arena[:at] == 0xFF).all() and (p.arena[at + ext:] == 0xFF).all()
        p.arena[at + ext] = 0                                               # the byte right behind the extent is band
        assert p.fault() == ("x", "the band behind", 0)
        p.arena[at + ext] = 0xFF
        p.arena[at - 1] = 0
        assert p.fault() == ("x", "the band in front", -1)


def test_the_union_rule():
    slab = np.arange(64, dtype=np.float32)
    a, b, c, d = slab[0:8], slab[4:12], slab[12:16], slab[17:20]           # overlap, touch, 4 bytes apart
    items = [_item(d, "d"), _item(b, "b"), _item(a, "a", const=True), _item(c, "c")]
    groups = G.unions(items)
    assert [[items[i].param for i in idx] for _, _, idx in groups] == [["a", "b", "c"], ["d"]]
    assert groups[0][:2] == (slab.ctypes.data, slab.ctypes.data + 64) and groups[1][:2] == (slab.ctypes.data + 68, slab.ctypes.data + 80)
    p = G.Placed(items, slab)
    assert p.shared == {1, 2, 3} and p.address[1] - p.address[2] == 16 and p.address[3] - p.address[2] == 48
    assert abs(p.address[0] - p.address[3]) > p.band                       # a placement of its own, bands between
    other = np.arange(8, dtype=np.float32)                                  # another storage never joins, wherever it lies
    assert len(G.unions([_item(a), _item(other)])) == 2
    empty = slab[8:8]
    assert len(G.unions([_item(a), G.Item("e", 0, slab.ctypes.data + 32, 0, False, None, empty, G.storage_of(slab), False)])) == 2
    # in place: a const view and an output over the same bytes share one placement, and the output's cells may change
    p = G.Placed([_item(a, "x", const=True), _item(a, "out")], slab)
    at = p.address[0] - p.base
    p.arena[at:at + 4] = 0
    assert p.shared == {0, 1} and p.address[0] == p.address[1] and p.fault() is None


# ----------------------------------------------------------------------------- the ledger, from the header
def test_ledger_derivation():
    protos = W.prototypes()
    required, exempt = G.ledger(protos)
    assert G.EXEMPT == exempt and set(exempt.values()) == set(G.KINDS)
    pointers = {(e, p.name) for e, ps in protos.items() for p in ps if p.pointer}
    assert required | set(exempt) == pointers and not required & set(exempt)
    no_stream = {e for e, ps in protos.items() if not any(p.name == "stream" for p in ps)}
    assert no_stream == set(G.HOST_ONLY)
    named = {"lkg_csr_build", "lkg_csr_transpose", "lkg_row_partition", "lkg_triples_count", "lkg_triples_read",
             "lkg_triples_dedup", "lkg_laplacian_f32", "lkg_last_error"}
    assert named <= no_stream and "lkg_csr_coo_indices_i64" not in no_stream     # (it takes a stream: device-side, required)
    from literalkg_amd import _native as N
    for (entry, param), kind in exempt.items():
        p = next(q for q in protos[entry] if q.name == param)
        if kind == "host-only":
            assert entry in no_stream
        elif kind == "not memory":
            assert param in ("stream", "dbg") and p.ctype == "void *"
        else:
            assert kind == "host array" and entry in ("lkg_gemm_tall_f32", "lkg_linear_act_layernorm_fwd_f32")
            assert param in ("a", "lda", "ka", "b", "ldb", "w", "ldw") and p.const
        assert kind == "host-only" or N.PROTOTYPES[entry][p.index] is N.vp
    assert len(required) >= 786
    for pair in (("lkg_permute_f32", "perm"), ("lkg_gather_i64", "perm"), ("lkg_spmm_csr_fused_f32", "rowptr"),
                 ("lkg_adam_step_f32", "exp_avg_sq"), ("lkg_gemm_tall_f32", "workspace"), ("lkg_gemm_tall_f32", "gate_x"),
                 ("lkg_topk_select_f32", "ws_i"), ("lkg_csr_coo_indices_i64", "rowptr"), ("lkg_csr_check_i32", "rowptr")):
        assert pair in required, pair
    for entry, out in W.WAIVED:
        assert (entry, out) in required
