"""The collective sequence of a fused training step (TrainerState._exchange), on CPU tensors with stub phases and recorded
collectives: every rank must make the same sequence of collective calls whatever its row count, or the others hang in RCCL.
No GPU and no library load."""
import pytest
import torch

from wild_visual_navigation_amd.traversability_estimator import trainer
from wild_visual_navigation_amd.traversability_estimator.trainer import TrainerState

METHODS = ("latest_measurement", "running_mean", "kalman_filter", "moving_average")


def _trainer(method, calls, with_minmax=True):
    tr = TrainerState(model=None, lr=1e-3, method=method, process_group="the group")
    tr.stats = torch.full((4,), 7.0, dtype=torch.float64)
    tr.grads = torch.full((11,), 7.0)
    if with_minmax:
        tr.minmax = torch.zeros(2)
    tr.ran = []
    tr.phase_a = lambda: (tr.ran.append("A"), calls.append("A"))
    tr.phase_b = lambda: (tr.ran.append("B"), calls.append("B"))
    return tr


@pytest.fixture
def calls(monkeypatch):
    rec = []

    def record(op):
        def collective(t, group=None):
            assert group == "the group"
            rec.append((op, t))
            return t
        return collective

    monkeypatch.setattr(trainer, "allreduce_sum_", record("sum"))
    monkeypatch.setattr(trainer, "allreduce_max_", record("max"))
    return rec


def _sequence(tr, calls):
    names = {id(tr.stats): "stats", id(tr.grads): "grads", id(tr.minmax): "minmax"}
    return [c if isinstance(c, str) else f"{c[0]}({names[id(c[1])]})" for c in calls]


def _expected(method):
    return ["A", "sum(stats)"] + (["max(minmax)"] if method == "moving_average" else []) + ["B", "sum(grads)"]


@pytest.mark.parametrize("method", METHODS)
def test_local_rows(calls, method):
    tr = _trainer(method, calls)
    tr._exchange(tr.phase_a, tr.phase_b, launch=True)
    assert _sequence(tr, calls) == _expected(method)
    assert tr.ran == ["A", "B"]
    assert torch.all(tr.stats == 7.0) and torch.all(tr.grads == 7.0) and torch.all(tr.minmax == 0.0)   # left to the phases


@pytest.mark.parametrize("method", METHODS)
def test_empty_shard_that_skips_its_launches(calls, method):
    tr = _trainer(method, calls)
    tr._exchange(tr.phase_a, tr.phase_b, launch=False)
    assert tr.ran == []
    assert _sequence(tr, calls) == [c for c in _expected(method) if c not in ("A", "B")]
    assert torch.all(tr.stats == 0.0) and torch.all(tr.grads == 0.0)
    if method == "moving_average":
        assert torch.all(tr.minmax == -float("inf"))
    else:
        assert torch.all(tr.minmax == 0.0)


def test_substitutes_are_in_place_before_their_collective(calls, monkeypatch):
    """What an empty shard contributes is what the collective sees: zeros to the sums, -inf to the max."""
    seen = []
    monkeypatch.setattr(trainer, "allreduce_sum_", lambda t, group=None: seen.append(("sum", t.clone())))
    monkeypatch.setattr(trainer, "allreduce_max_", lambda t, group=None: seen.append(("max", t.clone())))
    tr = _trainer("moving_average", calls)
    tr._exchange(tr.phase_a, tr.phase_b, launch=False)
    assert [op for op, _ in seen] == ["sum", "max", "sum"]
    assert torch.all(seen[0][1] == 0.0) and torch.all(seen[1][1] == -float("inf")) and torch.all(seen[2][1] == 0.0)


@pytest.mark.parametrize("method", METHODS)
def test_empty_shard_that_launches_anyway(calls, method):
    """RnvpTrainer: no minmax, the phases run with zero rows; no MAX collective for any method."""
    tr = _trainer(method, calls, with_minmax=False)
    tr._exchange(tr.phase_a, tr.phase_b, launch=True)
    assert tr.ran == ["A", "B"]
    assert _sequence(tr, calls) == ["A", "sum(stats)", "B", "sum(grads)"]


@pytest.mark.parametrize("launch", (True, False))
@pytest.mark.parametrize("method", ("latest_measurement", "moving_average"))
def test_two_timed_pairs_per_step(calls, monkeypatch, method, launch):
    """comm_events = [] collects one (start, end) pair around each SUM, none around the MAX; each pair brackets its collective."""
    class Event:
        def __init__(self, enable_timing=False):
            assert enable_timing

        def record(self):
            calls.append(self)

    monkeypatch.setattr(torch.cuda, "Event", Event)
    tr = _trainer(method, calls)
    tr.comm_events = []
    for step in (1, 2):
        tr._exchange(tr.phase_a, tr.phase_b, launch=launch)
        assert len(tr.comm_events) == 2 * step
    for (a, b), t in zip(tr.comm_events, (tr.stats, tr.grads, tr.stats, tr.grads)):
        i = next(k for k, c in enumerate(calls) if c is a)
        assert calls[i + 1][0] == "sum" and calls[i + 1][1] is t and calls[i + 2] is b
    assert sum(1 for c in calls if isinstance(c, Event)) == 8
