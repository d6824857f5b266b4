"""GPU tests (MI355X) of ``tick_kmeans_match_kernel`` and its routing by
``GOSSIPY_KMEANS_MATCH_KERNEL``, on the cases of ``kmeans_match_cases.py``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import kmeans_match_cases as kc
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import BatchedGossipSimulator, EngineConfig, KMeansSpec
from gossipy_amd.engine.backend import HIPBackend
from gossipy_amd.simul import SimulationReport

CUDA = torch.device("cuda:0")
KNOB = "GOSSIPY_KMEANS_MATCH_KERNEL"
MU_CASES, UM_CASES = kc.CASES[::2], kc.CASES[1::2]  # the modes alternate


@pytest.fixture(autouse=True)
def _knob_unset(monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)


def _run(case):
    state, pool, data = kc.build(case, CUDA)
    path = HIPBackend().kmeans_match_path(kc.spec(case), data)
    kc.deliver(HIPBackend(), case, state, pool, data)
    torch.cuda.synchronize()
    return path, state, pool


@pytest.mark.parametrize("case", kc.CASES, ids=kc.IDS)
def test_kernel_matches_replay(case, monkeypatch):
    monkeypatch.setenv(KNOB, "1")
    path, state, pool = _run(case)
    assert path == "kernel"
    dev = kc.deviation(kc.replay(case), state, pool)
    print(f"dev kernel {dev:.3e} tol {kc.TOL:.1e}")
    assert dev <= kc.TOL
    sent = kc.build(case)[1]  # the kernel only reads the delivered slots
    assert torch.equal(sent.slots[:5], pool.slots[:5].cpu())
    assert torch.equal(sent.slot_ages[:5], pool.slot_ages[:5].cpu())


@pytest.mark.parametrize("case", MU_CASES, ids=kc.IDS[::2])
def test_kernel_equals_the_host_route_bit_for_bit(case, monkeypatch):
    monkeypatch.setenv(KNOB, "0")
    path, s_host, p_host = _run(case)
    assert path == "host"
    print(f"dev host {kc.deviation(kc.replay(case), s_host, p_host):.3e}")
    monkeypatch.setenv(KNOB, "1")
    path, s_ker, p_ker = _run(case)
    assert path == "kernel"
    assert torch.equal(s_host.params, s_ker.params)
    assert torch.equal(s_host.ages, s_ker.ages)
    assert torch.equal(p_host.slots, p_ker.slots)
    assert torch.equal(p_host.slot_ages, p_ker.slot_ages)


def test_update_merge_takes_the_kernel_unless_it_is_off(monkeypatch):
    case = UM_CASES[1]
    path, state, pool = _run(case)
    assert path == "kernel"
    assert kc.deviation(kc.replay(case), state, pool) <= kc.TOL
    monkeypatch.setenv(KNOB, "0")
    with pytest.raises(ValueError, match="UPDATE_MERGE.*unsupported.*" + KNOB):
        kc.deliver(HIPBackend(), case, *kc.build(case, CUDA))


def test_update_merge_clusters():
    from tests.test_engine import _blob_arena

    cfg = EngineConfig(n_nodes=16, delta=10, protocol=AntiEntropyProtocol.PUSH,
                       model_size=24, sampling_eval=0.0, seed=29)
    spec = KMeansSpec(k=3, dim=8, alpha=0.1, mode=kc.UM, matching="hungarian")
    sim = BatchedGossipSimulator(cfg, spec, _blob_arena(device=CUDA),
                                 device=CUDA)
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes()
    sim.start(n_rounds=10)
    torch.cuda.synchronize()
    assert rep.get_evaluation(False)[-1][1]["nmi"] > 0.6
