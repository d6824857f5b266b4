"""GPU tests (MI355X) of the wide MLP PENS route, ``pens_mlp_score_kernel`` +
``tick_pens_mlp_wide_kernel`` under ``GOSSIPY_PENS_MLP_WIDE=1``: the cases of
``pens_mlp_wide_cases.py`` against their float64 replay, bit-equality with
``tick_pens_mlp_kernel`` on the shapes both take, the path query and its
knob, the PENS runner end to end on 784-100-10."""

from dataclasses import replace

import pytest
import torch

pytestmark = pytest.mark.gpu

import pens_mlp_cases as small
import pens_mlp_wide_cases as pc
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (
    BatchedPENSGossipSimulator, DataArena, EngineConfig, MLPSpec)
from gossipy_amd.engine.backend import HIPBackend

CUDA = torch.device("cuda:0")
KNOB = "GOSSIPY_PENS_MLP_WIDE"
MNIST = MLPSpec(784, 10, (100,), lr=0.1, batch_size=32)


def _run(mod, case, path):
    state, data, pool, counts = mod.build(case, CUDA)
    assert HIPBackend().pens_tick_path(case.spec, data) == path
    mod.run_backend(HIPBackend(), case, state, data, pool, counts)
    torch.cuda.synchronize()
    return state, counts


def _same(a, b):
    return (torch.equal(a[0].params, b[0].params)
            and torch.equal(a[0].ages, b[0].ages) and torch.equal(a[1], b[1]))


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_wide_pens_event_matches_replay(name, monkeypatch):
    pc.check_inputs(name)
    monkeypatch.setenv(KNOB, "1")
    first = _run(pc, pc.BY_NAME[name], "wide")
    pc.compare(name, *first)
    assert _same(first, _run(pc, pc.BY_NAME[name], "wide"))


# B: 530 rows at batch 0, nine row blocks: a scorer that misses rows past one
# block, or mis-sums the partials, picks {1, 2}
@pytest.mark.parametrize("name", ["A", "A_bs0", "B"])
def test_wide_route_returns_the_lds_kernels_bits(name, monkeypatch):
    small.check_inputs(name)
    monkeypatch.delenv(KNOB, raising=False)
    lds = _run(small, small.CASES[name], "lds")
    monkeypatch.setenv(KNOB, "1")
    wide = _run(small, small.CASES[name], "wide")
    assert _same(lds, wide)
    small.compare(name, *wide)


def _path(spec, smax):
    x = torch.empty(2, smax, spec.d_in)
    return HIPBackend().pens_tick_path(spec, DataArena(x, x[:, :, 0], None))


def test_path_query_and_knob(monkeypatch):
    pinned = ("pens mlp LDS budget exceeded.*wide kernel covers the plain MLP"
              " tick only.*" + KNOB)
    tiny = MLPSpec(20, 3, (24,), lr=0.1, batch_size=16)
    for knob in (None, "0"):
        monkeypatch.delenv(KNOB, raising=False)
        if knob:
            monkeypatch.setenv(KNOB, knob)
        assert _path(tiny, 37) == "lds"
        with pytest.raises(RuntimeError, match=pinned):
            _path(MNIST, 40)
    # still off: past the budget the event raises before a launch
    case = pc.BY_NAME["mnist"]
    state, data, pool, counts = pc.build(case, CUDA)
    before = state.params.clone()
    with pytest.raises(RuntimeError, match=pinned):
        pc.run_backend(HIPBackend(), case, state, data, pool, counts)
    torch.cuda.synchronize()
    assert torch.equal(before, state.params) and int(counts.sum()) == 0
    monkeypatch.setenv(KNOB, "1")
    assert _path(tiny, 37) == _path(MNIST, 40) == "wide"
    with pytest.raises(RuntimeError, match="pens mlp wide LDS budget.*hidden"):
        _path(MLPSpec(784, 10, (5000,)), 40)
    with pytest.raises(ValueError, match="plain LogRegSpec or MLPSpec"):
        _path(replace(tiny, n_parts=2), 37)


def test_pens_runner_end_to_end_on_mnist_shape(monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    g = torch.Generator().manual_seed(11)
    xs = torch.randn(25, 40, 784, generator=g)  # the last shard: the eval set
    ys = (xs @ torch.randn(784, 10, generator=g)).argmax(dim=2).float()
    data = DataArena.from_shards(
        [(xs[i], ys[i]) for i in range(24)], CUDA, global_eval=(xs[24], ys[24]))
    cfg = EngineConfig(n_nodes=24, delta=10, protocol=AntiEntropyProtocol.PUSH,
                       model_size=MNIST.D, sampling_eval=0.0, seed=37)
    sim = BatchedPENSGossipSimulator(cfg, MNIST, data, n_sampled=3, m_top=2,
                                     step1_rounds=6, device=CUDA)
    assert sim.backend.pens_tick_path(MNIST, data) == "wide"
    sim.init_nodes()
    sim.start(n_rounds=8)  # 6 rounds of step 1, 2 of step 2
    torch.cuda.synchronize()
    assert int(sim.counts.sum()) > 0  # step-1 events ran
    assert sim.scheduler.best_nodes is not None  # and step 2 followed
    assert torch.isfinite(sim.local_params()).all()
    assert int(sim.state.ages.min()) > 0
