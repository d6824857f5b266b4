"""GPU tests (MI355X) of the global-resident MLP tick
(``tick_mlp_wide_kernel``), the kernel ``mlp_plan`` picks for a plain MLP
whose model row and staged minibatch miss one workgroup's 160 KB of LDS:

* every case of ``mlp_wide_cases.py`` (784-100-10 in every mode, limited
  merge, pass-through coins, a full batch of 200 rows, a row that overflows
  alone, three layers) against the float64 reference within the case's
  ``tol``, the delivered slots only read;
* the path query names the kernel each configuration gets;
* with ``GOSSIPY_MLP_WIDE=1`` every plain MLP case of the standing table
  (MFMA buckets, ragged tiles, rows past the block, limited merge) returns
  the bits of the LDS kernel;
* a simulator's rounds through the whole-round executor equal its rounds
  with ``GOSSIPY_NO_ROUND_DRIVER=1`` and its rounds launched tick by tick,
  which also runs the workspace across launches;
* ``GOSSIPY_MLP_WIDE=0`` restores the budget error, and the partitioned,
  sampled and PENS MLP ticks keep theirs.

All marked ``gpu``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import mlp_wide_cases as wc
import tick_cases as tc
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    MLPSpec,
)
from gossipy_amd.engine.backend import HIPBackend

CUDA = torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _auto_path(monkeypatch):
    monkeypatch.delenv("GOSSIPY_MLP_WIDE", raising=False)


def _run(case):
    state, data, pool = tc.build(case, CUDA)
    tc.run_backend(HIPBackend(), case, state, data, pool)
    torch.cuda.synchronize()
    return state, pool


@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_wide_tick_matches_reference(name):
    case = wc.BY_NAME[name]
    state, data, pool = tc.build(case, CUDA)
    assert HIPBackend().mlp_tick_path(case.spec, data) == "wide"
    nd = tc.n_deliveries(case)
    sent = pool.slots[:nd].clone()
    sent_ages = pool.slot_ages[:nd].clone()
    tc.run_backend(HIPBackend(), case, state, data, pool)
    torch.cuda.synchronize()
    dev = tc.deviation(case, wc.reference(name), state, pool)
    print(f"dev {name} {dev:.3e} tol {case.tol:.1e}")
    assert dev <= case.tol, (name, dev)
    # the kernel only reads the delivered slots
    assert torch.equal(sent, pool.slots[:nd])
    assert torch.equal(sent_ages, pool.slot_ages[:nd])


def test_flagship_mlp_keeps_the_lds_kernel():
    spec = MLPSpec(d_in=57, n_classes=2, hidden=(100,), batch_size=32)
    x = torch.zeros(2, 46, 57, device=CUDA)
    data = DataArena(x, x[:, :, 0], torch.zeros(2, dtype=torch.int32))
    assert HIPBackend().mlp_tick_path(spec, data) == "lds"


PLAIN_MLP = [
    c.name for c in tc.CASES
    if c.spec.family == "mlp" and not c.spec.n_parts
    and not c.spec.sample_size
]


@pytest.mark.parametrize("name", PLAIN_MLP)
def test_forced_wide_equals_the_lds_kernel_bit_for_bit(name, monkeypatch):
    case = tc.BY_NAME[name]
    _, data, _ = tc.build(case, CUDA)
    assert HIPBackend().mlp_tick_path(case.spec, data) == "lds"
    s_lds, p_lds = _run(case)
    monkeypatch.setenv("GOSSIPY_MLP_WIDE", "1")
    assert HIPBackend().mlp_tick_path(case.spec, data) == "wide"
    s_wide, p_wide = _run(case)
    assert torch.equal(s_lds.params, s_wide.params)
    assert torch.equal(s_lds.ages, s_wide.ages)
    nd = tc.n_deliveries(case)
    assert torch.equal(p_lds.slots[nd:], p_wide.slots[nd:])
    assert torch.equal(p_lds.slot_ages[nd:], p_wide.slot_ages[nd:])
    assert torch.equal(p_lds.slots[:nd], p_wide.slots[:nd])


def test_the_bit_equality_table_reaches_the_edges():
    assert len(PLAIN_MLP) >= 30
    for part in ("mfma_fwd_k129", "mfma_ragged", "rows_mlp", "mlp_limited",
                 "mlp_wd_epochs_pass", "mlp_one_layer"):
        assert any(part in n for n in PLAIN_MLP), part


# ---- runner level -------------------------------------------------------------------

def _sim(mode):
    n = 8
    g = torch.Generator().manual_seed(21)
    sizes = [33 + 7 * (i % 5) for i in range(n)]  # 33 .. 61: a partial batch
    shards = [(torch.randn(c, 784, generator=g),
               torch.randint(0, 10, (c,), generator=g).float())
              for c in sizes]
    data = DataArena.from_shards(
        shards, CUDA,
        global_eval=(torch.randn(40, 784, generator=g),
                     torch.randint(0, 10, (40,), generator=g).float()))
    spec = MLPSpec(d_in=784, n_classes=10, hidden=(100,), lr=0.1,
                   batch_size=32, mode=mode)
    cfg = EngineConfig(n_nodes=n, delta=8, protocol=AntiEntropyProtocol.PUSH,
                       model_size=spec.D, seed=5, sampling_eval=0.0)
    sim = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
    assert sim.backend.mlp_tick_path(spec, data) == "wide"
    sim.init_nodes(seed=3)
    return sim


def _same(a, b):
    torch.cuda.synchronize()
    assert a.rounds_done == b.rounds_done == 2
    assert torch.equal(a.state.params, b.state.params)
    assert torch.equal(a.state.ages, b.state.ages)
    assert torch.equal(a.pool.slots, b.pool.slots)
    assert torch.equal(a.pool.slot_ages, b.pool.slot_ages)
    assert int(a.state.ages.max()) > 0


@pytest.mark.parametrize("mode", ["merge_update", "update_merge"])
def test_round_executor_equals_the_python_round_path(mode, monkeypatch):
    monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    a = _sim(tc.MODES[mode])
    assert a._fast_path_ok()
    a.start(n_rounds=2)
    monkeypatch.setenv("GOSSIPY_NO_ROUND_DRIVER", "1")
    b = _sim(tc.MODES[mode])
    b.start(n_rounds=2)
    _same(a, b)
    assert torch.isfinite(a.state.params).all()
    # that knob leaves an MLP round on the executor (the native driver has
    # no MLP plan), so a third run closes both whole-round routes: every
    # phase is then one tick_mlp call from Python. The same kernel sees the
    # same deliveries in the same order per receiver, so the models agree
    # bit for bit (the pools are numbered by another scheduler output and
    # are not compared)
    c = _sim(tc.MODES[mode])
    c._fast_path_ok = lambda: False
    c._flat_exec_ok = lambda: False
    ticks = []
    run_tick = c._run_tick
    c._run_tick = lambda phase: (ticks.append(1), run_tick(phase))[1]
    c.start(n_rounds=2)
    torch.cuda.synchronize()
    assert ticks
    assert torch.equal(a.state.params, c.state.params)
    assert torch.equal(a.state.ages, c.state.ages)


# ---- what stays bound to the LDS budget ----------------------------------------------

def test_knob_off_restores_the_budget_error(monkeypatch):
    monkeypatch.setenv("GOSSIPY_MLP_WIDE", "0")
    case = wc.BY_NAME["wide_mlp_784_merge_update"]
    state, data, pool = tc.build(case, CUDA)
    with pytest.raises(RuntimeError, match="mlp LDS budget exceeded"):
        tc.run_backend(HIPBackend(), case, state, data, pool)


@pytest.mark.parametrize("kw", [dict(n_parts=4), dict(sample_size=0.1)],
                         ids=["part", "samp"])
def test_compressed_ticks_keep_their_budget_error(kw):
    spec = MLPSpec(d_in=784, n_classes=10, hidden=(100,), lr=0.1,
                   batch_size=32, **kw)
    case = tc.Case("c", spec, [40, 33, 7], 1e-4, seed=3001)
    state, data, _ = tc.build(case, CUDA)
    before = state.params.clone()
    with pytest.raises(RuntimeError,
                       match="mlp LDS budget exceeded.*wide kernel covers"
                             " the plain MLP tick only"):
        HIPBackend().update(state, data, spec, torch.arange(3))
    torch.cuda.synchronize()
    assert torch.equal(before, state.params)


def test_pens_tick_keeps_its_budget_error():
    spec = MLPSpec(d_in=784, n_classes=10, hidden=(100,), lr=0.1,
                   batch_size=32)
    case = tc.Case("p", spec, [40, 33, 7], 1e-4, rows=tc.ROWS3, seed=3002)
    state, data, pool = tc.build(case, CUDA)
    counts = torch.zeros(3, 3, dtype=torch.int32, device=CUDA)
    with pytest.raises(RuntimeError,
                       match="pens mlp LDS budget exceeded.*wide kernel"
                             " covers the plain MLP tick only"):
        HIPBackend().deliver_pens(
            state, pool, data, spec, torch.tensor([0]), torch.tensor([0, 2]),
            torch.tensor([0, 1]), torch.tensor([0, 1]), counts, 2)
