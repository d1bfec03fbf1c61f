"""lkg_csr_sample_rows on the device against the numpy reference of neighbor_cases.py -- entry for entry, values by their bits,
no tolerance anywhere.  Destinations are allocated longer than written and pre-filled with a sentinel; the checker asserts that
the bytes behind the written region still hold it.

  rows of 0, 1, 3, 4, 5, 63, 64, 65, 129 and 5000 entries (a copy below the fanout, a select above: one, two and three
  histogram passes; 64-entry turns with and without a tail), a row with repeated columns, the last row of the matrix
  selections: all 600 rows (150 workgroups), rows with gaps, the hub alone, none
  fanout 1, 2, 4, 64, 65, 100, 5000 (the hub is copied), 2^31 - 1; three (seed, draw) pairs; rescale on and off"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import index_cases as I
import invariance as V
import neighbor_cases as NC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def N(ops):
    from literalkg_amd import _native
    return _native


@pytest.fixture(scope="module")
def dev(gpu_device):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu_device)


@pytest.fixture(scope="module")
def device_graph(dev):
    return tuple(dev(a.copy()) for a in NC.graph())                  # (the cached arrays are read-only)


def host(t):
    return t.cpu().numpy()


def run(ops, N, dev, device_graph, rows, f, seed, draw, rescale, entry="lkg_csr_sample_rows", operands=None):
    """one launch into guarded destinations -> (out_col, out_val) on the host, guards included"""
    rowptr = NC.graph()[0]
    rp, cl, vl = operands or device_graph
    out_rowptr = NC.out_rowptr_of(rowptr, rows, f)
    m = int(out_rowptr[-1])
    oc = torch.full((m + I.PAD,), I.ISENT, dtype=torch.int32, device=rp.device)
    ov = torch.full((m + I.PAD,), I.SENTINEL, dtype=torch.float32, device=rp.device)
    sel, orp = dev(np.asarray(rows, np.int64)), dev(out_rowptr)
    head = (rows.size, N.ptr(sel) if rows.size else None, N.ptr(rp), N.ptr(cl), N.ptr(vl))
    tail = (N.ptr(orp), N.ptr(oc), N.ptr(ov), ops._stream())
    if entry == "lkg_csr_sample_rows":
        N.call(entry, *head, f, seed, draw, int(rescale), *tail)
    else:
        N.call(entry, *head, *tail)
    return host(oc), host(ov)


@pytest.mark.parametrize("f", NC.FANOUTS)
@pytest.mark.parametrize("sel", list(NC.SELECTIONS))
def test_sample_equals_the_reference(ops, N, dev, device_graph, sel, f):
    rowptr, col, val = NC.graph()
    rows = NC.SELECTIONS[sel]()
    for seed, draw in NC.SEED_DRAWS:
        for rescale in (True, False):
            oc, ov = run(ops, N, dev, device_graph, rows, f, seed, draw, rescale)
            NC.check_sample(f"{sel}, f = {f}, seed {seed}, draw {draw}, rescale {rescale}", rowptr, col, val, rows, f, seed,
                            draw, rescale, oc, ov)


@pytest.mark.parametrize("f", [5000, 2 ** 31 - 1])
@pytest.mark.parametrize("sel", list(NC.SELECTIONS))
def test_a_fanout_no_row_exceeds_is_the_extraction(ops, N, dev, device_graph, sel, f):
    rows = NC.SELECTIONS[sel]()
    ec, ev = run(ops, N, dev, device_graph, rows, f, 0, 0, True, entry="lkg_csr_extract_rows")
    for rescale in (True, False):
        oc, ov = run(ops, N, dev, device_graph, rows, f, 2022, 7, rescale)
        assert V.same_bits(oc, ec, "col") and V.same_bits(ov, ev, "val")


def rows_of(rowptr, rows, f, oc, ov, wanted):
    """{row id: (col, val bits)} of the wanted rows of one result"""
    orp = NC.out_rowptr_of(rowptr, rows, f)
    at = {int(r): k for k, r in enumerate(rows)}
    return {r: (oc[orp[at[r]]:orp[at[r] + 1]].copy(), I.bits(ov[orp[at[r]]:orp[at[r] + 1]]).copy()) for r in wanted}


@pytest.mark.parametrize("f", [1, 4, 64, 100])
def test_a_rows_sample_depends_on_the_row_alone(ops, N, dev, device_graph, gpu_device, f):
    """the same entries for a row whether it is selected alone, in a subset or with every row, from misaligned copies of col
    and val, under poisoned scratch on a side stream, and in a second run"""
    from literalkg_amd import pruned
    rowptr, col, val = NC.graph()
    wanted = [5, 7, 8, NC.HUB, NC.DUP, NC.N_ROWS - 1]
    seed, draw = 2022, 7
    every = NC.SELECTIONS["all"]()
    base = rows_of(rowptr, every, f, *run(ops, N, dev, device_graph, every, f, seed, draw, True), wanted)

    def same(what, got):
        for r in wanted:
            assert (got[r][0] == base[r][0]).all() and (got[r][1] == base[r][1]).all(), (what, r)

    same("second run", rows_of(rowptr, every, f, *run(ops, N, dev, device_graph, every, f, seed, draw, True), wanted))
    gaps = NC.SELECTIONS["gaps"]()
    same("subset", rows_of(rowptr, gaps, f, *run(ops, N, dev, device_graph, gaps, f, seed, draw, True), wanted))
    for r in wanted:
        alone = np.array([r])
        got = rows_of(rowptr, alone, f, *run(ops, N, dev, device_graph, alone, f, seed, draw, True), [r])
        assert (got[r][0] == base[r][0]).all() and (got[r][1] == base[r][1]).all(), ("alone", r)
    for shift in (1, 3):                                   # col and val at addresses that are no multiple of 16 bytes
        cl = torch.full((col.size + shift,), I.ISENT, dtype=torch.int32, device=gpu_device)
        vl = torch.full((val.size + shift,), I.SENTINEL, dtype=torch.float32, device=gpu_device)
        cl[shift:], vl[shift:] = device_graph[1], device_graph[2]
        moved = (device_graph[0], cl[shift:], vl[shift:])
        assert cl[shift:].data_ptr() % 16 and vl[shift:].data_ptr() % 16
        same(f"shifted by {shift}", rows_of(rowptr, every, f, *run(ops, N, dev, device_graph, every, f, seed, draw, True,
                                                                   operands=moved), wanted))
    # the package's own call: every buffer it asks for uninitialised is poisoned, the launch goes to a delayed side stream
    g = SimpleNamespace(rowptr=device_graph[0], col=device_graph[1], n=NC.N_ROWS)
    sel = dev(every.astype(np.int64))
    with V.side_stream(), V.poisoned(0xFF):
        orp, oc, ov = pruned.sample_rows(g, device_graph[2], sel, f, seed, draw, True)
        orp, oc, ov = host(orp), host(oc), host(ov)
    want_rp, want_c, want_v = NC.sample_ref(rowptr, col, val, every, f, seed, draw, True)
    assert V.same_bits(orp, want_rp) and V.same_bits(oc, want_c) and V.same_bits(ov, want_v)
    same("poisoned, side stream", rows_of(rowptr, every, f, oc, ov, wanted))


def test_draw_and_seed_change_the_hubs_sample(ops, N, dev, device_graph):
    rows = NC.SELECTIONS["single"]()
    got = {(s, d): run(ops, N, dev, device_graph, rows, 64, s, d, False)[0] for s, d in ((0, 0), (0, 1), (1, 0), (1, 1))}
    for a in got:
        for b in got:
            if a < b:
                assert not (got[a] == got[b]).all(), (a, b)
    assert (run(ops, N, dev, device_graph, rows, 64, 0, 0, False)[0] == got[(0, 0)]).all()


def test_bad_arguments_launch_nothing(ops, N, dev, device_graph, gpu_device):
    rp, cl, vl = device_graph
    rows = NC.SELECTIONS["gaps"]()
    sel, orp = dev(rows.astype(np.int64)), dev(NC.out_rowptr_of(NC.graph()[0], rows, 4))
    oc = torch.full((400,), I.ISENT, dtype=torch.int32, device=gpu_device)
    ov = torch.full((400,), I.SENTINEL, dtype=torch.float32, device=gpu_device)
    lib = N.load()
    ptrs = (N.ptr(sel), N.ptr(rp), N.ptr(cl), N.ptr(vl))
    for fanout in (0, -1):
        assert lib.lkg_csr_sample_rows(rows.size, *ptrs, fanout, 0, 0, 1, N.ptr(orp), N.ptr(oc), N.ptr(ov), ops._stream()) == -1
        assert b"fanout" in lib.lkg_last_error()
    assert lib.lkg_csr_sample_rows(rows.size, *ptrs, 4, 0, 0, 1, N.ptr(orp), None, N.ptr(ov), ops._stream()) == -1
    assert b"null pointer" in lib.lkg_last_error()
    assert lib.lkg_csr_sample_rows(-1, *ptrs, 4, 0, 0, 1, N.ptr(orp), N.ptr(oc), N.ptr(ov), ops._stream()) == -1
    with pytest.raises(N.LkgError, match="fanout"):
        N.call("lkg_csr_sample_rows", rows.size, *ptrs, 0, 0, 0, 1, N.ptr(orp), N.ptr(oc), N.ptr(ov), ops._stream())
    assert lib.lkg_csr_sample_rows(0, None, None, None, None, 4, 0, 0, 1, None, None, None, ops._stream()) == 0   # n_sel = 0
    torch.cuda.synchronize()
    assert bool((oc == I.ISENT).all()) and bool((ov == I.SENTINEL).all())
