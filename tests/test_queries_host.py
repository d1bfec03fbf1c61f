"""No GPU: the pieces of the shared query front end (literalkg_amd/_queries.py) that have a contract of their own -- the
batch ranges, the batch-size check and the eval-mode context."""
import pytest

from literalkg_amd import _queries as Q


@pytest.mark.parametrize("n", [0, 1, 5])
@pytest.mark.parametrize("batch_size", [None, 1, 2, 5, 7])
def test_batches_cover_the_range_once_and_in_order(n, batch_size):
    ranges = list(Q.batches(n, batch_size))
    assert [i for lo, hi in ranges for i in range(lo, hi)] == list(range(n))
    assert all(0 < hi - lo <= (n if batch_size is None else batch_size) for lo, hi in ranges)     # no empty batch
    if batch_size is None:
        assert len(ranges) == (1 if n else 0)


def test_batch_size_check():
    Q.check_batch_size(3)
    Q.check_batch_size(None)
    for bad in (0, -1, 2.5, True, False):
        with pytest.raises(ValueError, match="batch_size must be a positive integer"):
            Q.check_batch_size(bad)


class Model:
    def __init__(self, training):
        self.training, self.calls = training, []

    def eval(self):
        self.calls.append("eval")
        self.training = False

    def train(self, mode):
        self.calls.append(mode)
        self.training = mode


@pytest.mark.parametrize("was_training", [True, False])
def test_eval_mode_restores_the_mode(was_training):
    m = Model(was_training)
    with Q.eval_mode(m):
        assert m.training is False
    assert m.training is was_training and m.calls == ["eval", was_training]
    m = Model(was_training)
    with pytest.raises(KeyError):
        with Q.eval_mode(m):
            assert m.training is False
            raise KeyError("inside")
    assert m.training is was_training and m.calls == ["eval", was_training]
