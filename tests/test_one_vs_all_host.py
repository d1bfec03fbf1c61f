"""No GPU: the argument checks of the 1-vs-all loss in their order (in the manner of test_query_checks_host.py: every
argument wrong at once, one repair per step), the refusal of CPU tensors, the mode dispatch and the ABI's new rows."""
from types import SimpleNamespace

import pytest
import torch

from literalkg_amd import _native, ops
from literalkg_amd.one_vs_all import one_vs_all_loss

DEVICE = "MI355X|no CPU"
IDS, R, T = torch.tensor([0, 1, 2]), torch.tensor([0, 1, 2]), torch.tensor([3, 4, 5])
EMPTY = torch.zeros(0, dtype=torch.int64)


def stand_in(scoring="mlp", n=40, c=8, n_rel=3):
    """a model without gat_trans_M whose table must not be asked for"""
    gen = torch.Generator().manual_seed(5)

    def no_table():
        raise AssertionError("the table was asked for")
    return SimpleNamespace(entity_embed=SimpleNamespace(weight=torch.randn(n, c, generator=gen)),
                           relation_embed=SimpleNamespace(weight=torch.randn(n_rel, c, generator=gen)),
                           gat_trans_M=None, n_entities=n, n_relations=n_rel, relation_dim=c, scoring=scoring,
                           training=False, _table_for_inference=no_table, gat_embeddings=no_table)


def test_argument_errors_come_in_order_and_before_any_device_work():
    model = stand_in()
    state = dict(h=IDS.float(), r=R == 0, t=T[:2].float(), side="left", scale=0.0, reduction="max", scoring=None, splits=65)
    steps = [("side must be one of", dict(side="both")),
             ("scoring='mlp' has no 1-vs-all loss", dict(scoring="distmult")),
             ("scoring must be one of", dict(scoring="transr")),
             ("reduction must be one of", dict(reduction="none")),
             ("scale must be a positive finite number", dict(scale=float("inf"))),
             ("scale must be a positive finite number", dict(scale=2.0)),
             ("splits must be", dict(splits=2.5)),
             ("splits must be", dict(splits=None)),
             ("h must be a 1-D tensor of integer ids", dict(h=IDS)),
             ("r must be a 1-D tensor of integer ids", dict(r=R)),
             ("t must be a 1-D tensor of integer ids", dict(t=T[:2])),
             ("h, r, t have different lengths", dict(t=T)),
             ("needs a model with gat_trans_M", dict(scoring="transe"))]
    for match, repair in steps:
        with pytest.raises(ValueError, match=match):
            one_vs_all_loss(model, **state)
        state.update(repair)
    empty = one_vs_all_loss(model, **dict(state, h=EMPTY, r=EMPTY, t=EMPTY))
    assert empty.shape == (0,) and empty.dtype == torch.float32
    assert one_vs_all_loss(model, **dict(state, h=EMPTY, r=EMPTY, t=EMPTY, reduction="mean")).shape == ()
    with pytest.raises(RuntimeError, match=DEVICE):          # a CPU model: refused by the id check, the table never asked for
        one_vs_all_loss(model, **state)


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    q, p, truth = torch.randn(3, 8), torch.randn(10, 8), torch.tensor([0, 1, 2])
    with pytest.raises(RuntimeError, match=DEVICE):
        ops.softmax_all_loss(q, p, truth)
    with pytest.raises(RuntimeError, match=DEVICE):
        ops.softmax_all_forward(q, p, None, truth)
    with pytest.raises(RuntimeError, match=DEVICE):
        ops.softmax_all_weights(q, p, None, truth, torch.zeros(3), torch.ones(3))
    for bad in (dict(scale=-1.0), dict(scale=float("nan")), dict(scale=True), dict(splits=-1), dict(splits=65),
                dict(chunk_bytes=0), dict(chunk_bytes=1.5)):
        with pytest.raises(ValueError):
            ops.check_softmax_args(**{**dict(scale=1.0, splits=None, chunk_bytes=1 << 20), **bad})
    assert ops.check_softmax_args(2, None) == (2.0, 0, ops.SOFTMAX_CHUNK_BYTES)


def test_chunk_width_is_whole_tiles_within_the_budget():
    assert ops.softmax_chunk_width(1024, 1_000_000) == 65536                   # 256 MB of 1024-row columns
    assert ops.softmax_chunk_width(130, 70001, 130 * 4 * 20000) == 19968       # whole tiles
    assert ops.softmax_chunk_width(130, 70001, 1) == 256                       # one tile at least
    assert ops.softmax_chunk_width(130, 100, 1) == 100                         # never beyond the table


def test_splits_helper_and_the_abi_rows():
    for name in ("lkg_softmax_all_splits", "lkg_softmax_all_partial_f32", "lkg_softmax_all_finish_f32",
                 "lkg_softmax_all_weights_f32"):
        assert name in _native.PROTOTYPES
    import __graft_entry__ as ge
    ge.build()
    assert ops.softmax_all_splits(64, 70001, 1) == 1 and ops.softmax_all_splits(64, 70001, 2) == 2
    assert ops.softmax_all_splits(64, 70001) == 64                             # automatic: capped at the maximum
    assert ops.softmax_all_splits(64, 300, 64) == 2                            # never more than candidate tiles
    assert ops.softmax_all_splits(64, 0) == 0 and ops.softmax_all_splits(64, 10, 65) == 0
    # the entry points refuse bad sizes and a scale that is not positive before touching a pointer
    with pytest.raises(_native.LkgError, match="bad sizes"):
        _native.call("lkg_softmax_all_partial_f32", 1, 0, 4, None, 4, None, 4, None, 1.0, 1, None, None, None)
    with pytest.raises(_native.LkgError, match="scale must be positive"):
        _native.call("lkg_softmax_all_finish_f32", 1, 5, 4, None, 4, None, 4, None, None, 0.0, 1, None, None, None, None,
                     None, None)
    with pytest.raises(_native.LkgError, match="null pointer"):
        _native.call("lkg_softmax_all_weights_f32", 1, 5, 4, None, 4, None, 4, None, 0, None, None, None, None, 1.0, None,
                     5, None)
    _native.call("lkg_softmax_all_weights_f32", 0, 5, 4, None, 4, None, 4, None, 0, None, None, None, None, 1.0, None, 5,
                 None)                                                          # n_q = 0 returns at once


def test_mode_dispatch_and_the_sharded_refusal():
    import literalkg_amd as L
    from literalkg_amd.distributed import ShardedLiteralKG
    assert L.one_vs_all_loss is one_vs_all_loss
    seen = {}

    class Probe(L.LiteralKG):
        def __init__(self):                                   # (no tables: only forward's dispatch is exercised)
            torch.nn.Module.__init__(self)

        def calc_one_vs_all_loss(self, *a, **kw):
            seen["args"] = a
            return "loss"
    m = Probe()
    assert m(IDS, R, T, device=torch.device("cpu"), mode="one_vs_all") == "loss" and len(seen["args"]) == 3
    assert m(IDS, R, T, device=torch.device("cpu"), mode="no_such_mode") is None
    sharded = ShardedLiteralKG.__new__(ShardedLiteralKG)
    torch.nn.Module.__init__(sharded)
    with pytest.raises(NotImplementedError, match="one_vs_all"):
        sharded(IDS, R, T, device=torch.device("cpu"), mode="one_vs_all")
