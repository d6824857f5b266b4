"""GPU tests (MI355X) for the round driver's ``eval_overlap`` option
(``GOSSIPY_RD_EVAL_OVERLAP=1``; off by default): a
sampled evaluation's rows are gathered behind the round's kernels and the
eval kernel runs on a stream of its own over that copy, beside the next
round's first launches. Whatever the streams do, a simulator that runs
through the driver must leave exactly what the Python round path
(``GOSSIPY_NO_ROUND_DRIVER=1``) leaves: parameters, ages, the pool, every
round's reported metrics and the message counters. All marked ``gpu``."""

import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from gossipy_amd.core import AntiEntropyProtocol, UniformDelay
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
    PegasosSpec,
    SlotPool,
)
from gossipy_amd.simul import SimulationReport

CUDA = torch.device("cuda:0")
D_IN, N_EVAL = 9, 33
ON = "GOSSIPY_RD_EVAL_OVERLAP"
OTHERS = ["GOSSIPY_RD_NO_MAPPED_EVAL", "GOSSIPY_RD_NO_SIDE_UPLOAD"]


@pytest.fixture(autouse=True)
def overlap_on(monkeypatch):
    for s in OTHERS:
        monkeypatch.delenv(s, raising=False)
    monkeypatch.setenv(ON, "1")


def _data(n, k=2, pm1=False):
    g = torch.Generator().manual_seed(17)
    w = torch.randn(D_IN, k, generator=g)

    def draw(m):
        X = torch.randn(m, D_IN, generator=g)
        if k == 2:
            y = ((X @ w[:, 0]) > 0).float()
            return X, (2 * y - 1 if pm1 else y)
        return X, (X @ w).argmax(1).float()

    return DataArena.from_shards(
        [draw(3 + (5 * i) % 7) for i in range(n)], CUDA,
        global_eval=draw(N_EVAL))


def _sim(n, spec, data, delta=10, pool_capacity=None, **kw):
    kw.setdefault("protocol", AntiEntropyProtocol.PUSH)
    cfg = EngineConfig(n_nodes=n, delta=delta, model_size=spec.D, seed=5, **kw)
    sim = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes(seed=3)
    if pool_capacity is not None:
        sim.pool = SlotPool(spec.D, CUDA, capacity=pool_capacity)
    return sim, rep


def _run(sim, n, driver, monkeypatch):
    if driver:
        monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    else:
        monkeypatch.setenv("GOSSIPY_NO_ROUND_DRIVER", "1")
    sim.start(n_rounds=n)


def _assert_same(a, rep_a, b, rep_b, rounds, rows=None):
    torch.cuda.synchronize()
    assert a.rounds_done == b.rounds_done == rounds
    assert torch.equal(a.state.params, b.state.params)
    assert torch.equal(a.state.ages, b.state.ages)
    assert torch.equal(a.pool.slots, b.pool.slots)
    assert torch.equal(a.pool.slot_ages, b.pool.slot_ages)
    ev_a, ev_b = rep_a.get_evaluation(False), rep_b.get_evaluation(False)
    assert len(ev_a) == rounds
    assert ev_a == ev_b  # every round's metrics, with their timestamps
    assert (rep_a._sent_messages, rep_a._failed_messages, rep_a._total_size) == (
        rep_b._sent_messages, rep_b._failed_messages, rep_b._total_size)
    assert rep_a._sent_messages > 0


def _pair(n, spec, data, rounds, monkeypatch, **kw):
    a, rep_a = _sim(n, spec, data, **kw)
    b, rep_b = _sim(n, spec, data, **kw)
    _run(a, rounds, True, monkeypatch)
    _run(b, rounds, False, monkeypatch)
    assert getattr(a, "_rd", None) is not None
    assert getattr(b, "_rd", None) is None
    _assert_same(a, rep_a, b, rep_b, rounds)
    return a, rep_a


def _logreg(k):
    return LogRegSpec(d_in=D_IN, n_classes=k, lr=0.1, batch_size=4)


@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("sampling", [0.1, 0.03], ids=["4rows", "1row"])
def test_logreg_equals_python_path(k, sampling, monkeypatch):
    assert max(int(40 * sampling), 1) == (4 if sampling == 0.1 else 1)
    _pair(40, _logreg(k), _data(40, k), 8, monkeypatch,
          sampling_eval=sampling)


def test_pegasos_through_the_linear_plan(monkeypatch):
    _pair(40, PegasosSpec(d_in=D_IN), _data(40, pm1=True), 8, monkeypatch,
          sampling_eval=0.1)


def test_evaluated_nodes_rewritten_by_the_next_round(monkeypatch):
    # 8 nodes, 4 evaluated per round, every node fires every round: the next
    # round's first launches rewrite the rows the evaluation reads
    _pair(8, _logreg(2), _data(8), 30, monkeypatch, sampling_eval=0.5)


@pytest.mark.parametrize("other", [None] + OTHERS)
def test_overlap_on_equals_off(other, monkeypatch):
    # the option on against the default (off), alone and with each of the
    # two other options switched off on both sides
    spec, data = _logreg(2), _data(40)
    kw = dict(protocol=AntiEntropyProtocol.PUSH_PULL,
              delay=UniformDelay(1, 5), sampling_eval=0.1)
    if other:
        monkeypatch.setenv(other, "1")
    a, rep_a = _sim(40, spec, data, **kw)
    _run(a, 6, True, monkeypatch)
    monkeypatch.delenv(ON)
    b, rep_b = _sim(40, spec, data, **kw)
    _run(b, 6, True, monkeypatch)
    assert a._rd is not None and b._rd is not None
    _assert_same(a, rep_a, b, rep_b, 6)


def test_sampling_zero_evaluates_every_node(monkeypatch):
    a, rep_a = _pair(40, _logreg(2), _data(40), 4, monkeypatch,
                     sampling_eval=0.0)
    # the in-stream path: a gather of the whole population buys nothing
    assert a._rd is not None


def test_split_start_and_pool_growth(monkeypatch):
    spec, data = _logreg(2), _data(40)
    kw = dict(protocol=AntiEntropyProtocol.PUSH_PULL,
              delay=UniformDelay(1, 5), sampling_eval=0.1)
    a, rep_a = _sim(40, spec, data, **kw)
    b, rep_b = _sim(40, spec, data, **kw)
    _run(a, 3, True, monkeypatch)
    assert len(rep_a.get_evaluation(False)) == 3  # drained at the boundary
    _run(a, 2, True, monkeypatch)
    _run(b, 5, True, monkeypatch)
    _assert_same(a, rep_a, b, rep_b, 5)
    # a pool too small at round 0: the held-round retry, overlap on
    c, rep_c = _sim(40, spec, data, pool_capacity=8, **kw)
    grown = []
    ensure = c.pool.ensure

    def spy(n):
        assert n > c.pool.slots.shape[0]
        ensure(n)
        grown.append(c.rounds_done)

    c.pool.ensure = spy
    _run(c, 5, True, monkeypatch)
    assert grown and grown[0] == 0
    d, rep_d = _sim(40, spec, data, pool_capacity=8, **kw)
    _run(d, 5, False, monkeypatch)
    _assert_same(c, rep_c, d, rep_d, 5)


def test_construct_destroy_twenty(monkeypatch):
    spec, data = _logreg(2), _data(40)
    monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    from gossipy_amd import ops

    live = ops.load_extension().round_driver_live
    gc.collect()
    base = live()
    for _ in range(20):
        sim, rep = _sim(40, spec, data, sampling_eval=0.1)
        sim.start(n_rounds=3)
        assert sim._rd is not None
        held = live()
        # ring, staging and upload events plus the two gather events; the
        # upload stream and the eval stream
        assert held[2] - base[2] == 4 + 2 + 1 + 2 and held[3] - base[3] == 2
        # the two stages' gathered rows and the identity index array
        assert held[1] - base[1] >= 3
        del sim, rep
        gc.collect()
        assert live() == base
