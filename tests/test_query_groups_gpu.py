"""GPU: the operand loop of the one-sided entry points (literalkg_amd/_queries.py: query_groups, side_queries,
scoring_groups) against the ops wrappers it is made of, on int32 views -- no tolerance.

300 entities; table width 20 with TransR output width 12 (neither row stride is a multiple of 16 bytes) and one case at
width 16; 3 relations of which 2 occur; 70 queries (past one 64-row tile); 130 shuffled candidate ids; both sides; r=None
for 'dot'."""
import math
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

N, B, N_REL, N_CAND = 300, 70, 3, 130


@pytest.fixture(scope="module")
def lib(gpu_device):
    import __graft_entry__ as ge
    ge.build()
    from literalkg_amd import _queries, ops
    return SimpleNamespace(Q=_queries, ops=ops)


class StandIn:
    """What query_groups reads of a LiteralKG, over a given table."""

    def __init__(self, table, relemb, trans_m, scoring):
        self.T = table
        self.entity_embed = SimpleNamespace(weight=table)
        self.relation_embed = SimpleNamespace(weight=relemb)
        self.gat_trans_M = trans_m
        self.n_entities, self.n_relations = table.shape[0], relemb.shape[0]
        self.relation_dim, self.scoring, self.training = relemb.shape[1], scoring, False

    def _table_for_inference(self):
        return self.T


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and \
        torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("with_cand", [False, True], ids=["all", "cand"])
@pytest.mark.parametrize("side", ["tail", "head"])
@pytest.mark.parametrize("scoring,c,k,with_r", [("transr", 20, 12, True), ("transr", 16, 16, True), ("transe", 20, 20, True),
                                                ("dot", 20, 20, True), ("dot", 20, 20, False)])
def test_every_group_carries_the_bits_of_the_wrappers(lib, scoring, c, k, with_r, side, with_cand):
    Q, ops = lib.Q, lib.ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(11)
    table = torch.randn(N, c, generator=gen).to(dev)
    relemb = (torch.randn(N_REL, k, generator=gen) * 0.3).to(dev)
    trans_m = (torch.randn(N_REL, c, k, generator=gen) / math.sqrt(c)).to(dev) if scoring == "transr" else None
    model = StandIn(table, relemb, trans_m, scoring)
    ent = torch.randint(0, N, (B,), generator=gen).to(dev)
    r = (2 * torch.randint(0, 2, (B,), generator=gen)).to(dev) if with_r else None        # relations 0 and 2 occur
    cand = torch.randperm(N, generator=gen)[:N_CAND].to(dev) if with_cand else None
    alpha = 1.0 if side == "tail" else -1.0
    e = None if scoring == "dot" else relemb
    seen, last = [], None
    for g in Q.query_groups(model, scoring, side, ent, r, cand):
        assert last is None or vars(last) == {}                # the turn before this one holds nothing any more
        last = g
        seen.append(g.pos.cpu())
        assert torch.equal(g.qid, ent[g.pos])
        if r is None:
            assert g.rel is None and g.frel.dtype == torch.int64 and g.frel.tolist() == [-1] * g.pos.numel()
        else:
            assert torch.equal(g.rel, r[g.pos]) and torch.equal(g.frel, r[g.pos])
        if scoring == "transr":
            rr = int(g.rel[0])
            assert bool((g.rel == rr).all())
            assert same_bits(g.table, ops.gemm_tall([table], [[trans_m[rr]]], trans_b=False, rowmax=ops.row_absmax(table)))
        else:
            assert g.table.data_ptr() == table.data_ptr() and g.table.shape == table.shape
        if scoring == "dot":
            assert g.table_n is None and g.pn is None
        else:
            assert same_bits(g.table_n, ops.rank_sqnorm(g.table))
        assert same_bits(g.q, ops.rank_queries(g.table, g.qid, e, g.rel, alpha))
        if cand is None:
            assert g.p is g.table and g.pn is g.table_n
        else:
            assert same_bits(g.p, ops.gather_rows(g.table, cand))
            assert (g.pn is None) == (scoring == "dot")
            assert g.pn is None or same_bits(g.pn, ops.rank_sqnorm(g.p))
    assert vars(last) == {}
    assert len(seen) == (2 if scoring == "transr" else 1)
    assert torch.cat(seen).sort().values.tolist() == list(range(B))
