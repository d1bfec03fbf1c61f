"""CPU: the harness of invariance.py itself -- same_bits, poisoned(), a planted leak, and the coverage of the patch by
construction: every allocation spelling of literalkg_amd/*.py is one the harness patches."""
import ast
import glob
import os
import re
import struct

import numpy as np
import pytest
import torch

import invariance as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- same_bits
def f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def test_same_bits_tells_nan_payloads_zeros_and_dtypes_apart():
    quiet, other = np.array([1.0, f32(0x7FC00000)], np.float32), np.array([1.0, f32(0x7FC00001)], np.float32)
    assert V.same_bits(torch.from_numpy(quiet), torch.from_numpy(quiet.copy()))      # NaN equals the same NaN
    with pytest.raises(AssertionError, match=r"first at \(1,\).*0x7fc00000.*0x7fc00001"):
        V.same_bits(torch.from_numpy(quiet), torch.from_numpy(other))
    with pytest.raises(AssertionError, match=r"first at \(0, 2\)"):
        V.same_bits(torch.tensor([[1.0, 2.0, 0.0]]), torch.tensor([[1.0, 2.0, -0.0]]))
    assert torch.equal(torch.tensor([0.0]), torch.tensor([-0.0]))                    # (what torch.equal lets through)
    with pytest.raises(AssertionError, match="dtype"):
        V.same_bits(torch.zeros(3, dtype=torch.int32), torch.zeros(3, dtype=torch.float32))
    with pytest.raises(AssertionError, match="dtype"):
        V.same_bits(torch.zeros(3, dtype=torch.int64), torch.zeros(6, dtype=torch.int32))
    with pytest.raises(AssertionError, match="shape"):
        V.same_bits(torch.zeros(2, 3), torch.zeros(3, 2))
    with pytest.raises(AssertionError, match="shape"):
        V.same_bits(torch.zeros(()), torch.zeros(1))
    assert V.same_bits(torch.zeros(0, 4), torch.zeros(0, 4)) and V.same_bits(torch.tensor(3), torch.tensor(3))
    assert V.same_bits(np.arange(5), np.arange(5)) and V.same_bits(torch.arange(6).view(2, 3).t(), torch.arange(6).view(2, 3).t())
    with pytest.raises(AssertionError, match=r"2 of 4 elements differ, the first at \(1, 0\): 3 .* != 7 "):
        V.same_bits(torch.tensor([[1, 2], [3, 4]]), torch.tensor([[1, 2], [7, 5]]), "ids")


# ----------------------------------------------------------------------------- the sources
def package_sources():
    return sorted(glob.glob(os.path.join(ROOT, "literalkg_amd", "*.py")))


SPELLING = re.compile(r"torch\.(?:empty|zeros|full|ones)\w*|\.new_\w+")
# matches of the pattern that allocate nothing
NOT_AN_ALLOCATION = {".new_seed"}                # torch.Generator.new_seed() (sampler.py)


def test_every_allocation_spelling_of_the_package_is_patched():
    found = {}
    for path in package_sources():
        with open(path) as f:
            for m in SPELLING.finditer(f.read()):
                found.setdefault(m.group(0), os.path.basename(path))
    assert {"torch.empty", "torch.zeros", "torch.full", "torch.empty_like"} <= set(found)    # the pattern finds them at all
    missing = {s: where for s, where in found.items() if s not in V.PATCHED and s not in NOT_AN_ALLOCATION}
    assert not missing, f"allocation spellings the harness does not patch: {missing}"
    assert NOT_AN_ALLOCATION <= set(found)
    # nobody binds an allocator by name (from torch import empty), which a patch of the module attribute would miss
    for path in package_sources():
        with open(path) as f:
            tree = ast.parse(f.read())
        for node in ast.walk(tree):
            if isinstance(node, ast.ImportFrom) and node.module == "torch":
                assert not {a.name for a in node.names} & set(V.UNINITIALISED + V.INITIALISED), path


def package_dtypes():
    """every torch dtype a package source names"""
    names = set()
    for path in package_sources():
        with open(path) as f:
            names |= set(re.findall(r"torch\.(float\d+|bfloat16|int\d+|uint8|bool|long|int|float|double|half)\b", f.read()))
    return sorted({getattr(torch, n) for n in names}, key=str)


# ----------------------------------------------------------------------------- poisoned
WANT = {0xFF: {torch.float32: "nan", torch.float64: "nan", torch.int32: -1, torch.int64: -1, torch.uint8: 255},
        0x7F: {torch.float32: f32(0x7F7F7F7F), torch.int32: 0x7F7F7F7F, torch.int64: 0x7F7F7F7F7F7F7F7F, torch.uint8: 127}}


@pytest.mark.parametrize("byte", [0xFF, 0x7F])
def test_poisoned_fills_every_dtype_the_package_allocates(byte):
    dtypes = package_dtypes()
    assert {torch.float32, torch.float64, torch.int32, torch.int64, torch.uint8} <= set(dtypes)
    like = torch.arange(12.0).view(3, 4)
    with V.poisoned(byte):
        for dt in dtypes:
            made = [torch.empty(7, dtype=dt), torch.empty((2, 3), dtype=dt), torch.empty((), dtype=dt), torch.empty(0, dtype=dt),
                    torch.empty_like(like, dtype=dt), torch.empty_like(like.t(), dtype=dt), like.new_empty((5,), dtype=dt),
                    torch.empty_strided((3, 2), (1, 3), dtype=dt)]
            for t in made:
                assert t.dtype == dt
                if dt == torch.bool:
                    assert bool(t.all())
                    continue
                raw = t.contiguous().reshape(-1).view(torch.uint8)
                assert bool((raw == byte).all()), (dt, tuple(t.shape))
                want = WANT[byte].get(dt)
                if want == "nan":
                    assert bool(torch.isnan(t).all())
                elif want is not None and t.numel():
                    assert t.reshape(-1)[0].item() == want, (dt, t.reshape(-1)[0].item())
        grad = torch.empty(4, requires_grad=True)                  # (a leaf that requires grad is filled all the same)
        assert grad.requires_grad and bool((grad.detach().view(torch.uint8) == byte).all())
        assert float(torch.zeros(3).sum()) == 0.0 and float(torch.full((3,), 2.0).sum()) == 6.0 and float(like.new_zeros(2).sum()) == 0.0
    assert f32(0x7F7F7F7F) > 3.39e38


def test_poisoned_restores_the_originals_also_after_an_exception():
    names = V.UNINITIALISED + V.INITIALISED
    before = {n: getattr(torch, n) for n in names}
    methods = {n: getattr(torch.Tensor, n) for n in V.TENSOR_UNINITIALISED + V.TENSOR_INITIALISED}
    with pytest.raises(KeyError):
        with V.poisoned(0xFF):
            assert all(getattr(torch, n) is not before[n] for n in names)
            with V.poisoned(0x7F):                                  # nested: the inner byte, then the outer one again
                assert torch.empty(1, dtype=torch.uint8).item() == 0x7F
            assert torch.empty(1, dtype=torch.uint8).item() == 0xFF
            raise KeyError("inside")
    assert all(getattr(torch, n) is before[n] for n in names)
    assert all(getattr(torch.Tensor, n) == methods[n] for n in methods)
    assert all(n not in torch.Tensor.__dict__ for n in methods)
    assert V.active() == (None, 0)
    with pytest.raises(ValueError):
        with V.poisoned(256):
            pass


# ----------------------------------------------------------------------------- a planted leak
def leaky(x):
    """x + 1, written to every second element only: the others keep what the buffer held."""
    out = torch.empty_like(x)
    out[::2] = x[::2] + 1
    return out


def sound(x):
    out = torch.empty_like(x)
    out[::2] = x[::2] + 1
    out[1::2] = x[1::2] + 1
    return out


def test_a_planted_leak_is_caught_under_both_bytes_and_passes_on_lucky_memory(monkeypatch):
    x = torch.arange(64, dtype=torch.float32)
    want = x + 1
    # unpoisoned, on memory that happens to hold the right values (a cached block of the same op's last run): it passes
    lucky = want.clone()
    real = torch.empty_like
    monkeypatch.setattr(torch, "empty_like", lambda *a, **k: lucky)
    assert V.same_bits(leaky(x), want)
    monkeypatch.setattr(torch, "empty_like", real)
    for byte in (0xFF, 0x7F):
        with V.poisoned(byte):
            got, twin = leaky(x), sound(x)
        with pytest.raises(AssertionError, match=r"32 of 64 elements differ, the first at \(1,\)"):
            V.same_bits(got, want)
        assert V.same_bits(twin, want)


def test_side_stream_delays_device_allocations_only():
    """the delay goes in front of an allocation on the device, by its device argument or the tensor it is modelled on"""
    like = torch.zeros(3)
    assert not V._on_gpu((3,), {}) and not V._on_gpu((3,), {"device": "cpu"}) and not V._on_gpu((like,), {})
    assert V._on_gpu((3,), {"device": "cuda"}) and V._on_gpu((3,), {"device": torch.device("cuda:0")})
    assert not V._on_gpu((like,), {"device": None})


# ----------------------------------------------------------------------------- the ledger
def test_the_ledger_partitions_the_entry_points():
    """REQUIRED, HOST_ONLY, NOT_REACHED and ELSEWHERE of test_invariance_gpu.py hold every entry point of
    _native.PROTOTYPES -- the whole ABI -- exactly once: a new entry point must be classified before the suite passes."""
    import test_invariance_gpu as G
    from literalkg_amd import _native
    G.check_ledger_partition(_native.PROTOTYPES)
    assert len(G.NOT_REACHED) <= 8 and not set(G.NOT_REACHED) & G.QUERY_SIDE
    assert len(_native.PROTOTYPES) >= 129 and len(G.ELSEWHERE) == 17


def _definitions(path):
    """(source, {name: [node]}) of every function and class a file defines, at any depth"""
    with open(path) as f:
        src = f.read()
    found = {}
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)):
            found.setdefault(node.name, []).append(node)
    return src, found


def _names(node):
    return {n.id for n in ast.walk(node) if isinstance(n, ast.Name)} | \
           {n.attr for n in ast.walk(node) if isinstance(n, ast.Attribute)}


# an autograd Function's passes are entered through its class (X.apply), never by these names alone
NOT_FOLLOWED = {"forward", "backward", "apply"}


def _reached_literals(test_node, local, package):
    """every string constant of the test, of the functions of its own module and of the package's functions and classes
    that it reaches by name, transitively"""
    seen, todo, strings = set(), [test_node], set()
    while todo:
        node = todo.pop()
        if id(node) in seen:
            continue
        seen.add(id(node))
        strings |= {c.value for c in ast.walk(node) if isinstance(c, ast.Constant) and isinstance(c.value, str)}
        for name in _names(node) - NOT_FOLLOWED:
            todo += local.get(name, []) + package.get(name, [])
    return strings


def test_every_entry_point_listed_elsewhere_has_its_case_there():
    """ELSEWHERE names, per entry point, the test of another module that runs it under poisoned scratch and on a side
    stream.  Each such test exists, enters poisoned( and side_stream( -- itself or through its module's perturbation(
    helper -- and reaches, by the names it calls, a function of the package that passes the entry point's name to the
    library."""
    import test_invariance_gpu as G
    package = {}
    for path in package_sources():
        for name, nodes in _definitions(path)[1].items():
            package.setdefault(name, []).extend(nodes)
    here = os.path.dirname(os.path.abspath(__file__))
    modules = {}
    for entry, where in G.ELSEWHERE.items():
        file, test = where.split("::")
        path = os.path.join(here, file)
        assert os.path.exists(path), (entry, file)
        if file not in modules:
            modules[file] = _definitions(path)
        src, local = modules[file]
        assert len(local.get(test, [])) == 1, f"{entry}: {file} does not define {test} (once)"
        node = local[test][0]
        assert "pytest.mark.gpu" in src
        text = ast.get_source_segment(src, node)
        if "perturbation(" in text:
            text += "".join(ast.get_source_segment(src, h) for h in local["perturbation"])
        assert "poisoned(" in text and "side_stream(" in text, f"{entry}: {where} does not enter both perturbations"
        assert entry in _reached_literals(node, local, package), f"{entry}: {where} reaches no caller of it"
    # the check can fail: a test that calls nothing of the family reaches no caller
    src, local = modules["test_neighbors_gpu.py"]
    assert "lkg_csr_sample_rows" not in _reached_literals(local["test_draw_and_seed_change_the_hubs_sample"][0], {}, package)
    assert "lkg_list_count_f32" not in _reached_literals(local["test_a_rows_sample_depends_on_the_row_alone"][0], local, package)
