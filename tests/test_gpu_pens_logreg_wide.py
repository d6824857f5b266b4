"""GPU tests (MI355X) of ``tick_pens_wide_kernel``: the cases of
``pens_logreg_wide_cases.py`` against their float64 replay, the path query
and its knob, the PENS runner end to end on a shape only this kernel takes."""

from dataclasses import replace

import pytest
import torch

pytestmark = pytest.mark.gpu

import pens_logreg_wide_cases as pc
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (
    BatchedPENSGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
)
from gossipy_amd.engine.backend import HIPBackend

CUDA = torch.device("cuda:0")
KNOB = "GOSSIPY_LOGREG_WIDE"


def _run(case):
    state, data, pool, counts = pc.build(case, CUDA)
    assert HIPBackend().pens_tick_path(case.spec, data) == "wide"
    pc.run_backend(HIPBackend(), case, state, data, pool, counts)
    torch.cuda.synchronize()
    return state, counts


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_wide_pens_event_matches_replay(name, monkeypatch):
    pc.check_inputs(name)
    case = pc.BY_NAME[name]
    monkeypatch.delenv(KNOB, raising=False)
    if case.knob:
        monkeypatch.setenv(KNOB, case.knob)
    state, counts = _run(case)
    pc.compare(name, state, counts)
    again, counts2 = _run(case)
    assert torch.equal(state.params, again.params)
    assert torch.equal(state.ages, again.ages)
    assert torch.equal(counts, counts2)


def _path(spec, smax):
    x = torch.empty(2, smax, spec.d_in)
    return HIPBackend().pens_tick_path(spec, DataArena(x, x[:, :, 0], None))


def test_path_query_and_knob(monkeypatch):
    row = "the wide kernel keeps one model row and one dz block in LDS"
    big = LogRegSpec(784, 10, lr=0.1, batch_size=64)
    for knob in (None, "1", "0"):
        monkeypatch.delenv(KNOB, raising=False)
        if knob:
            monkeypatch.setenv(KNOB, knob)
        small = "wide" if knob == "1" else "lds"
        with pytest.raises(RuntimeError, match=row):
            _path(LogRegSpec(4096, 16), 40)
        assert _path(LogRegSpec(784, 10, batch_size=32), 70) == small
        assert _path(LogRegSpec(57, 2), 46) == small
        if knob != "0":
            assert _path(big, 70) == "wide"
    # knob "0" is still set: past the budget the event raises before a launch
    case = replace(pc.BY_NAME["ragged"], spec=big, shards=(70,) * 6)
    state, data, pool, counts = pc.build(case, CUDA)
    before = state.params.clone()
    with pytest.raises(RuntimeError, match="pens LDS budget exceeded: 234664"):
        _path(big, 70)
    with pytest.raises(RuntimeError, match="pens LDS budget exceeded: 234664"):
        pc.run_backend(HIPBackend(), case, state, data, pool, counts)
    torch.cuda.synchronize()
    assert torch.equal(before, state.params)


def test_pens_runner_end_to_end_past_the_budget(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    g = torch.Generator().manual_seed(11)
    xs = torch.randn(25, 80, 561, generator=g)  # the last shard: the eval set
    ys = (xs @ torch.randn(561, 6, generator=g)).argmax(dim=2).float()
    data = DataArena.from_shards(
        [(xs[i], ys[i]) for i in range(24)], CUDA, global_eval=(xs[24], ys[24]))
    spec = LogRegSpec(561, 6, lr=0.1, batch_size=0)
    cfg = EngineConfig(n_nodes=24, delta=10, protocol=AntiEntropyProtocol.PUSH,
                       model_size=spec.D, sampling_eval=0.0, seed=37)
    sim = BatchedPENSGossipSimulator(cfg, spec, data, n_sampled=3, m_top=2,
                                     step1_rounds=6, device=CUDA)
    assert sim.backend.pens_tick_path(spec, data) == "wide"
    sim.init_nodes()
    sim.start(n_rounds=8)  # 6 rounds of step 1, 2 of step 2
    torch.cuda.synchronize()
    assert int(sim.counts.sum()) > 0  # step-1 events ran
    assert sim.scheduler.best_nodes is not None  # and step 2 followed
    assert torch.isfinite(sim.local_params()).all()
    assert int(sim.state.ages.min()) > 0
