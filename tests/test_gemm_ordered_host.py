"""CPU tier of the ordered split-K GEMM (literalkg_amd/gemm_ordered.py, include/literalkg_hip.h; the device
tier is test_gemm_ordered_gpu.py): the entry points are declared and bound, the partition tiles [0, k) as the
header states it, the default split count is a pure bounded function, product_route() is a thread-local stack, and the
argument errors that need no device."""
import importlib
import math
import os
import threading

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["lkg_gemm_ordered_f32", "lkg_gemm_ordered_partition", "lkg_gemm_ordered_splits", "lkg_gemm_ordered_workspace"]
KS = (0, 1, 15, 16, 17, 4096, 4097, 76800)
SPLITS = (1, 2, 3, 7, 256)


@pytest.fixture(scope="module")
def GO():
    import __graft_entry__ as ge
    ge.build()
    return importlib.import_module("literalkg_amd.gemm_ordered")      # (the package attribute of that name is the function)


def test_the_entry_points_are_declared_and_bound_and_the_package_exports_the_api(GO):
    from literalkg_amd import _native, build
    from wide_cases import prototypes
    assert "lkg_gemm_ordered.hip" in build.SOURCES
    assert os.path.exists(os.path.join(ROOT, "literalkg_amd", "csrc", "lkg_gemm_ordered.hip"))
    assert set(NAMES) <= set(_native.PROTOTYPES) and set(NAMES) <= set(prototypes())
    import literalkg_amd as L
    for name in ("gemm_ordered", "gemm_ordered_splits", "matmul_ordered", "product_route", "current_route"):
        assert name in L.__all__ and getattr(L, name) is getattr(GO, name)


def stated_partition(k, splits):
    """the header's rule, restated"""
    if k == 0:
        return 0, 0
    per = 16 * math.ceil(math.ceil(k / splits) / 16)
    return math.ceil(k / per), per


@pytest.mark.parametrize("k", KS)
def test_partition_tiles_the_reduction_once(GO, k):
    for splits in SPLITS:
        s_eff, per = GO.partition(k, splits)
        assert (s_eff, per) == stated_partition(k, splits), (k, splits)
        ranges = [(z * per, min(k, (z + 1) * per)) for z in range(s_eff)]
        covered = [i for lo, hi in ranges for i in range(lo, hi)]
        assert covered == list(range(k)), (k, splits)                 # every k once, in order
        assert all(lo < hi for lo, hi in ranges)                      # no empty split
        assert all(hi % 16 == 0 for _, hi in ranges[:-1]), (k, splits)
        assert s_eff <= min(splits, math.ceil(k / 16)), (k, splits, s_eff)
        from literalkg_amd import _native
        ws = int(_native.load().lkg_gemm_ordered_workspace(5, 7, k, splits))
        assert ws == (0 if s_eff <= 1 else s_eff * 5 * 7 * 4)


def test_partition_refuses_bad_arguments(GO):
    for k, splits in ((-1, 1), (16, 0), (16, 257)):
        with pytest.raises(ValueError):
            GO.partition(k, splits)
    from literalkg_amd import _native
    lib = _native.load()
    assert lib.lkg_gemm_ordered_partition(16, 0, None) < 0 and b"splits" in lib.lkg_last_error()
    assert lib.lkg_gemm_ordered_workspace(4, 4, 16, 300) < 0


SHAPES = [(1, 1, 1), (1024, 300, 1 << 20), (8192, 300, 1 << 20), (873, 300, 32768), (873, 300, 76800), (17, 129, 5000),
          (128, 128, 1 << 30), (100000, 4096, 1 << 20), (1, 300, 511), (1, 300, 512 * 256 + 1), (1 << 20, 1 << 12, 4096)]


@pytest.mark.parametrize("m,n,k", SHAPES)
def test_default_splits_are_a_bounded_pure_function(GO, m, n, k):
    for ta in (False, True):
        for tb in (False, True):
            s = GO.gemm_ordered_splits(m, n, k, ta, tb)
            assert s == GO.gemm_ordered_splits(m, n, k, ta, tb)       # twice: the same value
            assert 1 <= s <= 256
            s_eff, per = GO.partition(k, s)
            assert s_eff <= 1 or s_eff * m * n * 4 <= 256 << 20, (m, n, k, s)
            assert s == 1 or per >= 512                               # no split shorter than a few hundred k


def test_default_splits_spread_the_shapes_they_are_for(GO):
    tiles = lambda m, n: math.ceil(m / 128) * math.ceil(n / 128)
    for m, n, k in ((1024, 300, 1 << 20), (873, 300, 32768), (873, 300, 76800), (17, 301, 1 << 16)):
        s = GO.gemm_ordered_splits(m, n, k)
        assert 200 <= s * tiles(m, n) <= 512, (m, n, k, s)            # a few hundred workgroups


def test_product_route_default_nesting_and_restoration(GO):
    assert GO.current_route() == "engine"
    with GO.product_route("ordered"):
        assert GO.current_route() == "ordered"
        with GO.product_route("engine"):
            assert GO.current_route() == "engine"
            with GO.product_route("ordered"):
                assert GO.current_route() == "ordered"
            assert GO.current_route() == "engine"
        assert GO.current_route() == "ordered"
    assert GO.current_route() == "engine"
    with pytest.raises(KeyError):
        with GO.product_route("ordered"):
            raise KeyError("inside")
    assert GO.current_route() == "engine"                             # restored on exception
    for bad in ("Ordered", "", None, 1, "atomic"):
        with pytest.raises(ValueError):
            with GO.product_route(bad):
                pass
        assert GO.current_route() == "engine"
    # the public keyword: "ordered" enters the route, "engine" (every default) leaves the one in force
    with GO.keyword_route("ordered"):
        assert GO.current_route() == "ordered"
        with GO.keyword_route("engine"):
            assert GO.current_route() == "ordered"
    with GO.keyword_route("engine"):
        assert GO.current_route() == "engine"
    with pytest.raises(ValueError):
        GO.keyword_route("both")


def test_product_route_is_per_thread(GO):
    inside, go_on = threading.Event(), threading.Event()
    seen = {}

    def other():
        seen["before"] = GO.current_route()
        with GO.product_route("ordered"):
            seen["in"] = GO.current_route()
            inside.set()
            go_on.wait(10)
        seen["after"] = GO.current_route()

    th = threading.Thread(target=other)
    th.start()
    assert inside.wait(10)
    assert GO.current_route() == "engine"                             # the other thread's choice is not this one's
    with GO.product_route("ordered"):
        pass
    go_on.set()
    th.join(10)
    assert seen == {"before": "engine", "in": "ordered", "after": "engine"}


def test_argument_errors_that_need_no_device(GO):
    a, b = torch.zeros(3, 5), torch.zeros(4, 2)
    with pytest.raises(ValueError, match="inner dimensions"):
        GO.gemm_ordered(a, b)
    with pytest.raises(ValueError, match="inner dimensions"):
        GO.gemm_ordered(a, torch.zeros(5, 2), trans_a=True)
    with pytest.raises(ValueError, match="beta != 0 needs out"):
        GO.gemm_ordered(a, torch.zeros(5, 2), beta=1.0)
    for bad in (0, 257, -1, 2.0, True, "4"):
        with pytest.raises(ValueError, match="splits"):
            GO.gemm_ordered(a, torch.zeros(5, 2), splits=bad)
    with pytest.raises(ValueError, match="out must be"):
        GO.gemm_ordered(a, torch.zeros(5, 2), out=torch.zeros(3, 3))
    with pytest.raises(ValueError, match="bias"):
        GO.gemm_ordered(a, torch.zeros(5, 2), bias=torch.zeros(3))
    with pytest.raises(TypeError):
        GO.gemm_ordered(a.double(), torch.zeros(5, 2))
    with pytest.raises(RuntimeError, match="no CPU"):                  # well-formed CPU operands: refused, not computed
        GO.gemm_ordered(a, torch.zeros(5, 2))


def test_c_entry_point_refuses_before_any_launch(GO):
    from literalkg_amd import _native
    lib = _native.load()
    one = 0x1000                                                       # (never dereferenced: every call below is refused)
    ok = dict(ta=0, tb=0, m=4, n=4, k=64, splits=2, lda=64, ldb=4, ldc=4, ws=one, ws_bytes=2 * 4 * 4 * 4)

    def call(**kw):
        c = dict(ok, **kw)
        return lib.lkg_gemm_ordered_f32(c["ta"], c["tb"], c["m"], c["n"], c["k"], c["splits"], 1.0, one, c["lda"], one,
                                        c["ldb"], 0.0, one, c["ldc"], None, c["ws"], c["ws_bytes"], None)
    for kw, word in ((dict(splits=0), b"splits"), (dict(splits=257), b"splits"), (dict(ws_bytes=2 * 4 * 4 * 4 - 1), b"workspace"),
                     (dict(ws=None), b"workspace"), (dict(lda=63), b"leading"), (dict(ldb=3), b"leading"),
                     (dict(ldc=3), b"bad C"), (dict(m=-1), b"negative"), (dict(ta=1, lda=3), b"leading"),
                     (dict(tb=1, ldb=63), b"leading")):
        assert call(**kw) < 0, kw
        assert word in lib.lkg_last_error(), (kw, lib.lkg_last_error())
    assert call(m=0) == 0                                             # an empty output launches nothing


@pytest.mark.parametrize("fn", ["one_vs_all_loss", "kvs_all_loss", "relation_loss"])
def test_a_bad_products_name_is_refused_before_anything_else(GO, fn):
    import literalkg_amd as L
    with pytest.raises(ValueError, match="products"):
        getattr(L, fn)(None, None, None, None, products="atomic")
    from literalkg_amd import ops
    with pytest.raises(ValueError, match="products"):
        ops.softmax_all_loss(torch.zeros(1, 2), torch.zeros(3, 2), torch.zeros(1, dtype=torch.long), products="fast")
    with pytest.raises(ValueError, match="products"):
        L.sigmoid_all_loss(torch.zeros(1, 2), torch.zeros(3, 2), None, products="fast")
    with pytest.raises(ValueError, match="products"):
        L.relation_softmax_loss(torch.zeros(1, 2), None, torch.zeros(3, 2), torch.zeros(1, dtype=torch.long), products="fast")
    with pytest.raises(ValueError, match="products"):
        ops.all_entity_backward(torch.zeros(1, 2), torch.zeros(3, 2), None, 256, True, True, None, route="fast")
