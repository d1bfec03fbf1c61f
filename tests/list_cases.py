"""Plain-torch references for ranking against per-query candidate lists (literalkg_amd/lists.py), on GIVEN scores: which
slots of a B x M list are counted, the counts better / equal / kept against the truths' scores, the metrics, and the
comparator that holds a ListRanks to them.  Nothing here computes a score: test_lists_gpu.py feeds it the device's own
float32 scores (or exact integers), so every count has one right value."""
import torch


def keep_mask(lists, truth, queries=None, r=None, known=None, side="tail"):
    """bool[B, M]: slot j of query i is counted unless it is empty (a negative entry), holds the truth's id, or -- with
    `known`, a Python set of (h, r, t) triples -- forms a known triple with the query on that side under relation r[i]
    (r None: under any relation)."""
    lists, truth = torch.as_tensor(lists).cpu(), torch.as_tensor(truth).cpu()
    keep = (lists >= 0) & (lists != truth[:, None])
    if known:
        q = torch.as_tensor(queries).cpu().tolist()
        rel = None if r is None else torch.as_tensor(r).cpu().tolist()
        pairs = {}
        for h, rr, t in known:
            pairs.setdefault((h, t) if side == "tail" else (t, h), set()).add(rr)
        for i, row in enumerate(lists.tolist()):
            for j, c in enumerate(row):
                rels = pairs.get((q[i], c))
                if c >= 0 and rels is not None and (rel is None or rel[i] in rels):
                    keep[i, j] = False
    return keep


def counts(scores, truth_scores, keep, higher=False):
    """(better, equal, kept) int64[B] from a B x M score matrix, the truths' scores [B] and a keep mask: float compares,
    so a NaN slot is kept and is neither better nor equal, and a NaN truth gives better = equal = 0.  higher: a higher
    score is better (reported 'dot' scores); kernel scores are always lower-is-better."""
    s, t = torch.as_tensor(scores).cpu(), torch.as_tensor(truth_scores).cpu()[:, None]
    keep = torch.as_tensor(keep).cpu()
    better = ((s > t) if higher else (s < t)) & keep
    equal = (s == t) & keep
    return better.sum(1), equal.sum(1), keep.sum(1)


def metrics(by_side, ks=(1, 3, 10)):
    """The dict of evaluate_list_ranking from {side: (better, equal)}: Q.metrics_from_counts per side and over all."""
    from literalkg_amd import _queries as Q
    out = {s: Q.metrics_from_counts(b, e, ks) for s, (b, e) in by_side.items()}
    out.update(Q.metrics_from_counts(torch.cat([torch.as_tensor(b).reshape(-1) for b, _ in by_side.values()]),
                                     torch.cat([torch.as_tensor(e).reshape(-1) for _, e in by_side.values()]), ks))
    return out


def check_ranks(res, ref, what=""):
    """Hold a ListRanks (anything with better / equal / kept / rank) to the reference (better, equal, kept): every
    integer equal, int64, and rank = 1 + better + equal / 2 in float64."""
    for name, want in zip(("better", "equal", "kept"), ref):
        got = getattr(res, name)
        assert got.dtype == torch.int64, f"{what}: {name} is {got.dtype}"
        got, want = got.cpu(), torch.as_tensor(want).cpu()
        assert got.shape == want.shape, f"{what}: {name} has shape {tuple(got.shape)}, {tuple(want.shape)} wanted"
        bad = torch.nonzero(got != want).reshape(-1)
        assert bad.numel() == 0, (f"{what}: {name} differs at {bad.numel()} of {got.numel()} queries, the first {int(bad[0])}: "
                                  f"{int(got[bad[0]])} != {int(want[bad[0]])}")
    want = 1.0 + ref[0].double() + 0.5 * ref[1].double()
    assert res.rank.dtype == torch.float64 and torch.equal(res.rank.cpu(), want), f"{what}: rank"
    return True
