"""GPU tests (MI355X) for the scheduler's level packer: a simulator whose
rounds are packed by dependency level (``GOSSIPY_PACK_LEVELS``) must leave,
bit for bit, what the default packer leaves from the same seed. Every
delivery runs the same arithmetic on the same inputs; only the order of
independent deliveries differs. Small odd shapes: 64 nodes (32 for the MLP),
16 ticks, d=9, shards of 3 to 9 samples against a batch of 4, 33 eval
samples, 3 rounds. All marked ``gpu``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
    MLPSpec,
)
from gossipy_amd.engine.schedule import NativeSchedulerAdapter
from gossipy_amd.simul import SimulationReport

CUDA = torch.device("cuda:0")
DELTA, D_IN, N_EVAL, ROUNDS = 16, 9, 33, 3


def _data(n):
    g = torch.Generator().manual_seed(11)
    sizes = [3 + (5 * i) % 7 for i in range(n)]
    w = torch.randn(D_IN, generator=g)

    def draw(m):
        X = torch.randn(m, D_IN, generator=g)
        return X, ((X @ w) > 0).float()

    return DataArena.from_shards(
        [draw(m) for m in sizes], CUDA, global_eval=draw(N_EVAL)
    )


def _run(n, spec, data, levels, monkeypatch):
    """3 rounds with GOSSIPY_PACK_LEVELS=levels (None: unset)."""
    if levels is None:
        monkeypatch.delenv("GOSSIPY_PACK_LEVELS", raising=False)
    else:
        monkeypatch.setenv("GOSSIPY_PACK_LEVELS", str(levels))
    cfg = EngineConfig(
        n_nodes=n, delta=DELTA, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.1, seed=5,
    )
    sim = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes(seed=3)
    sim.start(n_rounds=ROUNDS)
    torch.cuda.synchronize()
    return sim, rep, cfg


def _assert_packer_ran(sim, cfg, cap):
    # the scheduler may have packed rounds ahead of the ones that ran
    packed, refused = sim.scheduler.pack_level_stats()
    assert packed >= ROUNDS and refused == 0
    # launch groups of the rounds that ran: more than one each, and what a
    # scheduler of its own gives for the same configuration
    twin = NativeSchedulerAdapter(cfg)
    twin.set_pack_levels(cap)
    groups = 0
    for r in range(ROUNDS):
        twin.next_round_flat(r)
        p = twin.last_flat["packed"]
        assert len(p["recv_tptr"]) - 1 > 1, f"round {r}"
        assert len(p["rep_nodes"]) == 0, f"round {r}"
        groups += len(p["recv_tptr"]) - 1
    assert twin.pack_level_stats() == (ROUNDS, 0)
    if getattr(sim, "_rd", None) is not None:
        assert sim.merge_stats == (ROUNDS * DELTA, groups)
    else:  # the Python round path has merged the round after the last too
        assert sim.merge_stats[1] > groups


def _assert_same(a, rep_a, b, rep_b):
    assert a.rounds_done == b.rounds_done == ROUNDS
    assert torch.equal(a.gather_params(), b.gather_params())
    assert torch.equal(a.gather_ages(), b.gather_ages())
    assert int(a.gather_ages().max()) > 0
    ev_a, ev_b = rep_a.get_evaluation(False), rep_b.get_evaluation(False)
    assert len(ev_a) == ROUNDS
    assert ev_a[-1] == ev_b[-1]
    assert (rep_a._sent_messages, rep_a._failed_messages) == (
        rep_b._sent_messages, rep_b._failed_messages)


def _on_off(n, spec, on, monkeypatch, cap=1):
    data = _data(n)
    a, rep_a, cfg = _run(n, spec, data, on, monkeypatch)
    b, rep_b, _ = _run(n, spec, data, 0, monkeypatch)
    _assert_packer_ran(a, cfg, cap)
    assert b.scheduler.pack_level_stats() == (0, 0)
    _assert_same(a, rep_a, b, rep_b)
    return a, b


def _logreg(**kw):
    return LogRegSpec(d_in=D_IN, n_classes=2, lr=0.1, batch_size=4, **kw)


@pytest.mark.parametrize("on", [None, 2], ids=["default", "cap2"])
def test_logreg(on, monkeypatch):
    monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    cap = BatchedGossipSimulator.PACK_LEVELS_DEFAULT if on is None else on
    a, b = _on_off(64, _logreg(), on, monkeypatch, cap)
    assert getattr(a, "_rd", None) is not None  # through the round driver


def test_limited_merge(monkeypatch):
    monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    _on_off(64, _logreg(age_diff_threshold=2), 1, monkeypatch)


def test_python_round_path(monkeypatch):
    monkeypatch.setenv("GOSSIPY_NO_ROUND_DRIVER", "1")
    a, b = _on_off(64, _logreg(), 1, monkeypatch)
    assert getattr(a, "_rd", None) is None


def test_mlp(monkeypatch):
    spec = MLPSpec(d_in=D_IN, n_classes=2, hidden=(8,), lr=0.1, batch_size=4)
    _on_off(32, spec, 1, monkeypatch)


def test_where_it_is_on_by_default(monkeypatch):
    monkeypatch.delenv("GOSSIPY_PACK_LEVELS", raising=False)
    on = BatchedGossipSimulator.PACK_LEVELS_DEFAULT
    assert on >= 1
    mlp = dict(d_in=D_IN, n_classes=2, hidden=(8,), lr=0.1, batch_size=4)
    for n, spec, want in (
        (64, _logreg(), on),
        (64, _logreg(age_diff_threshold=2), on),
        (64, _logreg(n_parts=4), 0),
        (32, MLPSpec(**mlp), on),
        (32, MLPSpec(age_diff_threshold=2, **mlp), 0),
    ):
        cfg = EngineConfig(
            n_nodes=n, delta=DELTA, protocol=AntiEntropyProtocol.PUSH,
            model_size=spec.D, n_parts=getattr(spec, "n_parts", 0), seed=5,
        )
        sim = BatchedGossipSimulator(cfg, spec, _data(n), device=CUDA)
        assert sim._pack_levels_cap() == want, spec
        monkeypatch.setenv("GOSSIPY_PACK_LEVELS", "0")
        assert sim._pack_levels_cap() == 0
        monkeypatch.setenv("GOSSIPY_PACK_LEVELS", "3")
        assert sim._pack_levels_cap() == 3
        monkeypatch.delenv("GOSSIPY_PACK_LEVELS")
