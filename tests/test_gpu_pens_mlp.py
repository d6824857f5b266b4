"""GPU tests (MI355X) of PENS step 1 for the MLP family: ``tick_pens_mlp``
against the ``TorchBackend`` oracle on identical state for the cases of
``pens_mlp_cases.py`` (params at 1e-4, ages and winner counts exactly), the
PENS runner with an ``MLPSpec`` end to end on both devices, and the host
checks of ``HIPBackend.deliver_pens``. All marked ``gpu``.

Top-m selection is discrete, so each equality test first asserts, from a
float64 forward, that no head-logit gap of its inputs is below 1e-4 (the
fp32 forward error at these shapes is about 5e-6) and that the selection is
not the trivial one (see ``pens_mlp_cases.check_inputs``)."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import pens_mlp_cases as pc
from gossipy_amd import ops
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedPENSGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
    MLPSpec,
    NodeStateArena,
    SlotPool,
)
from gossipy_amd.engine.backend import HIPBackend, TorchBackend
from gossipy_amd.simul import SimulationReport

CUDA = torch.device("cuda:0")
CPU = torch.device("cpu")
_ORACLE = {}


def oracle(name):
    """The TorchBackend result of the case, computed once and only read."""
    if name not in _ORACLE:
        case = pc.CASES[name]
        state, data, pool, counts = pc.build(case)
        pc.run_backend(TorchBackend(), case, state, data, pool, counts)
        _ORACLE[name] = (state, counts)
    return _ORACLE[name]


# A: 16 + 16 + 5 row chunks, ragged MFMA tiles, a three-way tie at the cut;
# A_bs0: the same as one 37-row chunk; B: 530-row chunks, more rows than the
# block has threads
@pytest.mark.parametrize("name", ["A", "A_bs0", "B"])
def test_pens_mlp_event_matches_oracle(name):
    pc.check_inputs(name)
    case = pc.CASES[name]
    want, want_counts = oracle(name)
    state, data, pool, counts = pc.build(case, CUDA)
    sent, sent_ages = pool.slots.clone(), pool.slot_ages.clone()
    pc.run_backend(HIPBackend(), case, state, data, pool, counts)
    torch.cuda.synchronize()
    dev = float((state.params.cpu() - want.params).abs().max())
    print(f"dev {name} vs oracle {dev:.3e} tol {pc.TOL:.1e}")
    assert dev <= pc.TOL, (name, dev)
    assert torch.equal(want.ages, state.ages.cpu())
    assert torch.equal(want_counts, counts.cpu())
    # and against the float64 replay itself
    pc.compare(name, state, counts)
    # the kernel only reads the candidates
    assert torch.equal(sent, pool.slots)
    assert torch.equal(sent_ages, pool.slot_ages)


def _run_pens(device):
    # the config of TestPENSGPU.test_pens_gpu_learns
    X, y = make_synthetic_classification((640, 57, 2), seed=0, margin=2.0)
    idx = np.random.default_rng(0).permutation(640)
    shards = [(X[s], y[s]) for s in np.array_split(idx[:576], 24)]
    data = DataArena.from_shards(
        shards, device, global_eval=(X[idx[576:]], y[idx[576:]])
    )
    spec = MLPSpec(d_in=57, n_classes=2, hidden=(16,), lr=0.1)
    cfg = EngineConfig(
        n_nodes=24, delta=10, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.25, seed=37,
    )
    sim = BatchedPENSGossipSimulator(
        cfg, spec, data, n_sampled=4, m_top=2, step1_rounds=5, device=device,
    )
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes()
    sim.start(n_rounds=12)
    return sim, rep.get_evaluation(False)[-1][1]["accuracy"]


def test_pens_mlp_gpu_end_to_end():
    gsim, gacc = _run_pens(CUDA)
    torch.cuda.synchronize()
    assert gsim.backend.name == "hip"
    csim, cacc = _run_pens(CPU)
    print(f"accuracy gpu {gacc:.4f} cpu {cacc:.4f}")
    # step 1 bumps m_top counters per event, and the schedule fixes the events
    assert int(gsim.counts.sum()) == int(csim.counts.sum()) > 0
    assert gsim.scheduler.best_nodes is not None
    assert csim.scheduler.best_nodes is not None
    assert torch.isfinite(gsim.local_params()).all()
    # selections may diverge after the first near-tie: no parameter equality
    assert gacc >= cacc - 0.05


# ---- host checks ---------------------------------------------------------------

def _tiny(spec, n_slots=2):
    g = torch.Generator().manual_seed(1)
    shards = [(torch.randn(8, spec.d_in, generator=g),
               torch.randint(0, 2, (8,), generator=g).float())
              for _ in range(2)]
    cd = DataArena.from_shards(shards, CPU)
    data = DataArena(cd.x.to(CUDA), cd.y.to(CUDA), cd.counts.to(CUDA))
    state = NodeStateArena(2, spec.D, CUDA)
    state.params.copy_(torch.randn(2, spec.D, generator=g) * 0.1)
    pool = SlotPool(spec.D, CUDA, n_slots)
    pool.slots.copy_(torch.randn(pool.slots.shape, generator=g) * 0.1)
    counts = torch.zeros(2, 2, dtype=torch.int32, device=CUDA)
    return state, data, pool, counts


@pytest.mark.parametrize("spec", [
    LogRegSpec(d_in=5, n_classes=2, lr=0.1),
    MLPSpec(d_in=5, n_classes=2, hidden=(4,), lr=0.1),
], ids=["logreg", "mlp"])
def test_too_many_candidates_raise_before_launch(spec):
    n = int(ops.load_extension().PENS_MAX_CAND) + 1
    assert n == 65
    state, data, pool, counts = _tiny(spec)
    before = state.params.clone()
    with pytest.raises(ValueError, match="65 candidates"):
        HIPBackend().deliver_pens(
            state, pool, data, spec, torch.tensor([0]), torch.tensor([0, n]),
            torch.zeros(n, dtype=torch.int64),
            torch.zeros(n, dtype=torch.int64), counts, 2)
    torch.cuda.synchronize()
    assert torch.equal(before, state.params)
    assert int(counts.sum()) == 0


def test_over_budget_mlp_gets_the_lds_message():
    # D = 30722 floats (120 KB) + 51040 floats of scratch: twice the budget
    spec = MLPSpec(d_in=57, n_classes=2, hidden=(512,), lr=0.1, batch_size=32)
    state, data, pool, counts = _tiny(spec)
    with pytest.raises(RuntimeError,
                       match="pens mlp LDS budget exceeded.*shrink"):
        HIPBackend().deliver_pens(
            state, pool, data, spec, torch.tensor([0]), torch.tensor([0, 2]),
            torch.tensor([0, 1]), torch.tensor([0, 1]), counts, 2)
