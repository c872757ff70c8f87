"""The stepping engine (pxmcmc_amd/mcmc/engine.py) on CPU tensors: a step that adds 1, fake graphs that replay pairs of
it.  Every schedule of two consecutive advances lands on the requested iteration, whichever side the first one left the
state on, with and without graphs and with predictions written by the step or formed on demand.  No GPU needed."""
import itertools

import pytest
import torch

from pxmcmc_amd.mcmc import Engine, _Counter


class _FakeGraph:
    """stands in for a captured graph of ``pairs`` A -> B -> A pairs of the engine's step"""

    def __init__(self, eng, log, pairs):
        self.eng, self.log, self.pairs = eng, log, pairs

    def replay(self):
        self.log["replaying"] = True
        for _ in range(self.pairs):
            self.eng.one(self.eng.XA, self.eng.XB)
            self.eng.one(self.eng.XB, self.eng.XA)
        self.log["replaying"] = False
        self.log["replays"] += 1


def _engine(graphs, lazy):
    X = torch.zeros((2, 3), dtype=torch.float64)
    P = torch.zeros((2, 4), dtype=torch.float64)
    eng = Engine(X, P, _Counter(0, host=True))
    log = {"eager": 0, "replays": 0, "form": 0, "replaying": False}

    def forward(X):  # "predictions" of a state: its value, in P's shape
        return X[:, :1].expand(-1, 4)

    def one(src, dst):
        torch.add(src, 1, out=dst)
        if not lazy:
            eng.P.copy_(forward(dst))
        eng.cnt.add(1)
        log["eager"] += not log["replaying"]

    def form_preds(X):
        eng.P.copy_(forward(X))
        log["form"] += 1

    eng.one = one
    if lazy:
        eng.form_preds = form_preds
    eng.ready(X, P, 0, graph_ok=False)
    if graphs:
        eng.graph, eng.graph_long = _FakeGraph(eng, log, 1), _FakeGraph(eng, log, Engine.GRAPH_PAIRS)
    return eng, log


@pytest.mark.parametrize("lazy", [False, True], ids=["eager_preds", "lazy_preds"])
@pytest.mark.parametrize("graphs", [False, True], ids=["no_graphs", "graphs"])
def test_two_advances_reach_the_requested_iteration(graphs, lazy):
    for k1, k2 in itertools.product(range(20), repeat=2):
        eng, log = _engine(graphs, lazy)
        done = 0
        for k in (k1, k2):
            before = dict(log)
            eng.advance(k)
            done += k
            eager, replays = log["eager"] - before["eager"], log["replays"] - before["replays"]
            if k == 0:
                assert eager == 0 and replays == 0, (k1, k2)  # advance(0) launches nothing
            if graphs:
                assert eager <= 2, (k1, k2, eager)  # one realign step and one odd step
            else:
                assert eager == k and replays == 0, (k1, k2)
            X, P = eng.state()
            assert X.shape == (2, 3) and P.shape == (2, 4)
            assert bool((X == done).all()) and bool((P == done).all()), (k1, k2, X, P)
            assert eng.cnt.i == done, (k1, k2)
            assert X is (eng.XA if done % 2 == 0 else eng.XB) and eng.side == "AB"[done % 2]
            formed = log["form"] - before["form"]
            assert formed == (1 if lazy and k > 0 else 0), (k1, k2, formed)
            eng.state()  # a second look at the same state forms nothing
            assert log["form"] - before["form"] == formed


@pytest.mark.parametrize("graphs", [False, True], ids=["no_graphs", "graphs"])
def test_stop_keeps_the_flags_and_drops_the_rest(graphs):
    closed = []

    class Counter(_Counter):
        def close(self):
            closed.append(self)

    eng, _ = _engine(graphs, lazy=True)
    eng.cnt = cnt = Counter(0, host=True)
    eng.ring, eng.pairs, eng.graph_error = True, True, None if graphs else "RuntimeError('no capture')"
    assert eng["ring"] is eng.ring and eng["cnt"] is cnt  # eng[name] is eng.name, reading ...
    eng["plan"] = plan = object()  # ... and writing
    assert eng.plan is plan
    eng.advance(3)
    eng.stop()
    assert closed == [cnt]
    for name in ("cnt", "one", "XA", "XB", "P", "form_preds", "reset", "cnt0", "plan", "graph_long", "unpack"):
        assert eng[name] is None, name
    assert eng["ring"] is True and eng["pairs"] is True and eng["graph"] is graphs
    assert eng["graph_error"] == (None if graphs else "RuntimeError('no capture')") and eng["side"] == "B"
    eng.stop()  # a stopped engine stops again without touching the counter
    assert closed == [cnt] and eng["graph"] is graphs
