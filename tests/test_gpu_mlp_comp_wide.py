"""GPU tests (MI355X) of ``tick_mlp_comp_wide_kernel``, which
``GOSSIPY_MLP_COMP_WIDE=1`` selects for a partitioned or sampled ``MLPSpec``:
every case of ``mlp_comp_wide_cases.py`` against the float64 reference; the
LDS kernel's bits where that one fits; the budget error without the knob;
the whole-round executor against the tick-by-tick route. All marked ``gpu``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import mlp_comp_wide_cases as cw
import tick_cases as tc
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (BatchedGossipSimulator, DataArena,
                                EngineConfig, MLPSpec)
from gossipy_amd.engine.backend import HIPBackend

CUDA = torch.device("cuda:0")
KNOB = "GOSSIPY_MLP_COMP_WIDE"
NAMES = [c.name for c in cw.CASES]


@pytest.fixture(autouse=True)
def _knob_unset(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def _run(case):
    state, data, pool = tc.build(case, CUDA)
    path = HIPBackend().mlp_comp_tick_path(case.spec, data)
    tc.run_backend(HIPBackend(), case, state, data, pool)
    torch.cuda.synchronize()
    return path, state, pool


@pytest.mark.parametrize("name", NAMES)
def test_wide_tick_matches_reference(name, monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    case = cw.BY_NAME[name]
    path, state, pool = _run(case)
    assert path == "wide"
    dev = tc.deviation(case, cw.reference(name), state, pool)
    print(f"dev {name} {dev:.3e} tol {case.tol:.1e}")
    assert dev <= case.tol, (name, dev)
    # the kernel only reads the delivered slots
    nd, sent = tc.n_deliveries(case), tc.build(case)[2]
    assert torch.equal(sent.slots[:nd], pool.slots[:nd].cpu())
    assert torch.equal(sent.slot_ages[:nd], pool.slot_ages[:nd].cpu())


@pytest.mark.parametrize("name", [n for n in NAMES if "784" not in n])
def test_forced_wide_equals_the_lds_kernel_bit_for_bit(name, monkeypatch):
    path, s_lds, p_lds = _run(cw.BY_NAME[name])
    assert path == "lds"
    monkeypatch.setenv(KNOB, "1")
    path, s_wide, p_wide = _run(cw.BY_NAME[name])
    assert path == "wide"
    assert torch.equal(s_lds.params, s_wide.params)
    assert torch.equal(s_lds.ages, s_wide.ages)
    assert torch.equal(p_lds.slots, p_wide.slots)
    assert torch.equal(p_lds.slot_ages, p_wide.slot_ages)


@pytest.mark.parametrize("name", ["wide_784_part4", "wide_784_samp01"])
def test_without_the_knob_the_budget_error_stays(name):
    case = cw.BY_NAME[name]
    built = tc.build(case, CUDA)
    with pytest.raises(RuntimeError,
                       match="mlp LDS budget exceeded.*wide kernel covers"
                             " the plain MLP tick only.*" + KNOB):
        tc.run_backend(HIPBackend(), case, *built)
    assert torch.equal(tc.build(case)[0].params, built[0].params.cpu())


def _sim(kw, cfg_kw):
    g = torch.Generator().manual_seed(21)
    shards = [(torch.randn(c, 784, generator=g),
               torch.randint(0, 10, (c,), generator=g).float())
              for c in (33, 40, 47, 54, 61, 33, 40, 47)]  # partial batches
    data = DataArena.from_shards(shards, CUDA)
    spec = MLPSpec(d_in=784, n_classes=10, hidden=(100,), lr=0.1,
                   batch_size=32, **kw)
    cfg = EngineConfig(n_nodes=8, delta=8, protocol=AntiEntropyProtocol.PUSH,
                       model_size=spec.D, seed=5, sampling_eval=0.0, **cfg_kw)
    sim = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
    sim.init_nodes(seed=3)
    return sim


@pytest.mark.parametrize(
    "kw, cfg_kw",
    [(dict(n_parts=4), dict(n_parts=4)),
     (dict(sample_size=0.1), dict(sampled=True))], ids=["part", "samp"])
def test_round_executor_equals_the_tick_by_tick_route(kw, cfg_kw, monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    a = _sim(kw, cfg_kw)
    assert a._fast_path_ok()
    a.start(n_rounds=2)
    b = _sim(kw, cfg_kw)  # every phase one tick call from Python
    b._fast_path_ok = b._flat_exec_ok = lambda: False
    b.start(n_rounds=2)
    torch.cuda.synchronize()
    assert torch.equal(a.state.params, b.state.params)
    assert torch.equal(a.state.ages, b.state.ages)
    assert int(a.state.ages.max()) > 0
    assert torch.isfinite(a.state.params).all()
