"""GPU tests (MI355X) of ``tick_logreg_wide_kernel``, the batch-streaming
logreg tick ``logreg_plan`` picks past the LDS budget: the cases of
``logreg_wide_cases.py`` and, forced by ``GOSSIPY_LOGREG_WIDE=1``, the plain
logreg cases of the standing table (k 2 to 16, d 9 to 129, batches of 127 to
330 rows) against the float64 reference; equal bits run to run; the round
executors against tick-by-tick launches; what stays a budget error."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import logreg_wide_cases as wc
import tick_cases as tc
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
)
from gossipy_amd.engine.backend import HIPBackend
from gossipy_amd.simul import SimulationReport

CUDA = torch.device("cuda:0")
# (case, knob): the wide table as planned, the standing plain logreg forced
TABLE = [(c, None) for c in wc.CASES] + [
    (c, "1") for c in tc.CASES
    if c.spec.family == "logreg" and not c.spec.n_parts
    and not c.spec.sample_size
]


def _run(case, knob, monkeypatch):
    monkeypatch.delenv("GOSSIPY_LOGREG_WIDE", raising=False)
    if knob:
        monkeypatch.setenv("GOSSIPY_LOGREG_WIDE", knob)
    state, data, pool = tc.build(case, CUDA)
    assert HIPBackend().logreg_tick_path(case.spec, data) == "wide"
    tc.run_backend(HIPBackend(), case, state, data, pool)
    torch.cuda.synchronize()
    return state, pool


@pytest.mark.parametrize("case,knob", TABLE, ids=[c.name for c, _ in TABLE])
def test_wide_tick_matches_reference(case, knob, monkeypatch):
    state, pool = _run(case, knob, monkeypatch)
    ref = tc.run_ref(case) if knob else wc.reference(case.name)
    dev = tc.deviation(case, ref, state, pool)
    print(f"dev {case.name} {dev:.3e} tol {case.tol:.1e}")
    assert dev <= case.tol, (case.name, dev)


def test_two_runs_return_the_same_bits(monkeypatch):
    case = wc.BY_NAME["784_update_merge"]
    s1, p1 = _run(case, None, monkeypatch)
    s2, p2 = _run(case, None, monkeypatch)
    assert torch.equal(s1.params, s2.params)
    assert torch.equal(s1.ages, s2.ages)
    assert torch.equal(p1.slots, p2.slots)


def _sim(mode):
    g = torch.Generator().manual_seed(21)
    shards = [(torch.randn(c, 784, generator=g),
               torch.randint(0, 10, (c,), generator=g).float())
              for c in (33, 40, 47, 54, 61, 33)]  # a partial second batch
    data = DataArena.from_shards(
        shards, CUDA,
        global_eval=(torch.randn(40, 784, generator=g),
                     torch.randint(0, 10, (40,), generator=g).float()))
    spec = LogRegSpec(784, 10, lr=0.1, batch_size=32, mode=mode)
    cfg = EngineConfig(n_nodes=6, delta=8, protocol=AntiEntropyProtocol.PUSH,
                       model_size=spec.D, seed=5, sampling_eval=0.0)
    sim = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
    assert sim.backend.logreg_tick_path(spec, data) == "wide"
    sim.add_receiver(SimulationReport())
    sim.init_nodes(seed=3)
    return sim


@pytest.mark.parametrize("mode", sorted(tc.MODES))
def test_round_executor_equals_the_python_round_path(mode, monkeypatch):
    monkeypatch.delenv("GOSSIPY_LOGREG_WIDE", raising=False)
    monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    a = _sim(tc.MODES[mode])
    assert a._fast_path_ok()
    a.start(n_rounds=2)
    monkeypatch.setenv("GOSSIPY_NO_ROUND_DRIVER", "1")
    b = _sim(tc.MODES[mode])
    b.start(n_rounds=2)
    # every phase one tick_logreg call from Python (its pools are numbered
    # by another scheduler output and are not compared)
    c = _sim(tc.MODES[mode])
    c._fast_path_ok = lambda: False
    c._flat_exec_ok = lambda: False
    c.start(n_rounds=2)
    torch.cuda.synchronize()
    for other in (b, c):
        assert torch.equal(a.state.params, other.state.params)
        assert torch.equal(a.state.ages, other.state.ages)
    assert torch.equal(a.pool.slots, b.pool.slots)
    assert mode == "pass" or int(a.state.ages.max()) > 0  # PASS never trains


@pytest.mark.parametrize("knob,case,match", [
    ("0", wc.BY_NAME["784_merge_update"], "logreg LDS budget exceeded: 164432"),
    (None, tc.Case("row", LogRegSpec(4096, 16), [3, 2], 1e-4, seed=4100),
     "logreg LDS budget exceeded.*the wide kernel keeps one model row and one"
     " dz block in LDS"),
], ids=["knob_off", "row_past_lds"])
def test_what_stays_a_budget_error(knob, case, match, monkeypatch):
    monkeypatch.delenv("GOSSIPY_LOGREG_WIDE", raising=False)
    if knob:
        monkeypatch.setenv("GOSSIPY_LOGREG_WIDE", knob)
    state, data, pool = tc.build(case, CUDA)
    before = state.params.clone()
    with pytest.raises(RuntimeError, match=match):
        tc.run_backend(HIPBackend(), case, state, data, pool)
    torch.cuda.synchronize()
    assert torch.equal(before, state.params)
