"""GPU tests (MI355X) for partitioned and sampled MLP gossip: the
tick_mlp_part / tick_mlp_samp kernels vs the fp32 torch oracle, the
whole-round executors vs the per-tick path, CPU <-> GPU end to end, and the
host-side error checks. All marked ``gpu``."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gossipy_amd.core import AntiEntropyProtocol, CreateModelMode
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    MLPSpec,
    NodeStateArena,
    RandomTape,
    SlotPool,
)
from gossipy_amd.engine.backend import HIPBackend, TorchBackend

CUDA = torch.device("cuda:0")
CPU = torch.device("cpu")

MODES = [
    CreateModelMode.MERGE_UPDATE,
    CreateModelMode.UPDATE,
    CreateModelMode.UPDATE_MERGE,
]

# delivery pattern shared by the deliver tests: receiver 2 gets two
# messages (the first asks for a reply), 5 and 9 one each
RECV = torch.tensor([2, 5, 9], dtype=torch.int64)
PTR = torch.tensor([0, 2, 3, 4], dtype=torch.int64)
SLOTS = torch.tensor([1, 4, 7, 10], dtype=torch.int64)
REPLY = torch.tensor([12, -1, 13, -1], dtype=torch.int64)
PIDS = torch.tensor([0, 3, 1, 2], dtype=torch.int64)
SEEDS = torch.tensor([123456, 777, 2**30 + 5, 42], dtype=torch.int64)


def _close(a, b, tol=1e-4):
    return torch.allclose(a.cpu(), b.cpu(), atol=tol, rtol=tol)


def _err(a, b):
    return float((a.cpu() - b.cpu()).abs().max())


def _pair(n, spec, samples=160, seed=3):
    """(cpu, gpu) copies of identical state/data; ages are [n, P] when the
    spec is partitioned, [n] otherwise."""
    A = spec.age_width
    cs = NodeStateArena(n, spec.D, CPU, age_width=A)
    TorchBackend().init_params(cs, spec, RandomTape(seed), n)
    cs.ages += (
        torch.arange(n * A, dtype=torch.int32).reshape(cs.ages.shape) % 5
    )
    gs = NodeStateArena(n, spec.D, CUDA, age_width=A)
    gs.params.copy_(cs.params)
    gs.ages.copy_(cs.ages)
    X, y = make_synthetic_classification(
        (samples, spec.d_in, spec.n_classes), seed=seed
    )
    shards = [(X[s], y[s]) for s in np.array_split(np.arange(samples), n)]
    cd = DataArena.from_shards(shards, CPU, global_eval=(X, y))
    gd = DataArena(
        cd.x.to(CUDA), cd.y.to(CUDA), cd.counts.to(CUDA),
        gx=cd.gx.to(CUDA), gy=cd.gy.to(CUDA),
    )
    return cs, gs, cd, gd


def _pools(spec, cap=16):
    """Slot pools holding MLP-scaled random models and distinct ages."""
    A = spec.age_width
    cpool = SlotPool(spec.D, CPU, cap, age_width=A)
    gpool = SlotPool(spec.D, CUDA, cap, age_width=A)
    cpool.slots.normal_(generator=torch.Generator().manual_seed(5))
    cpool.slots.mul_(0.2)
    cpool.slot_ages.copy_(
        torch.arange(cap * A, dtype=torch.int32).reshape(cpool.slot_ages.shape)
        % 7
    )
    gpool.slots.copy_(cpool.slots)
    gpool.slot_ages.copy_(cpool.slot_ages)
    return cpool, gpool


def _check_deliver(spec, cs, gs, cpool, gpool):
    print(
        f"params err {_err(cs.params, gs.params):.3e}"
        f" reply-slot err {_err(cpool.slots[12:14], gpool.slots[12:14]):.3e}"
    )
    assert _close(cs.params, gs.params)
    assert torch.equal(cs.ages, gs.ages.cpu())
    assert _close(cpool.slots[12:14], gpool.slots[12:14])
    assert torch.equal(cpool.slot_ages[12:14], gpool.slot_ages[12:14].cpu())


SHAPES = {
    # full batch, one hidden layer; D = 303, uneven partition split
    "11-20-3_fullbatch": dict(hidden=(20,), batch_size=0),
    # shards of 13/14 rows -> batches of 8 + a ragged 5/6, two epochs;
    # weight decay on so the rescale-then-decay order is exercised
    "11-20-3_bs8": dict(
        hidden=(20,), batch_size=8, local_epochs=2, weight_decay=0.01
    ),
    # two hidden layers; D = 531
    "11-20-12-3": dict(hidden=(20, 12), batch_size=0),
}


class TestPartitionedMLP:
    @pytest.mark.parametrize("shape", sorted(SHAPES))
    @pytest.mark.parametrize("mode", MODES, ids=lambda m: m.name)
    def test_deliver_matches_oracle(self, mode, shape):
        spec = MLPSpec(11, 3, lr=0.1, n_parts=4, mode=mode, **SHAPES[shape])
        cs, gs, cd, gd = _pair(12, spec)
        assert cs.ages.shape == (12, 4)
        cpool, gpool = _pools(spec)
        TorchBackend().deliver(cs, cpool, cd, spec, RECV, PTR, SLOTS, REPLY, PIDS)
        HIPBackend().deliver(gs, gpool, gd, spec, RECV, PTR, SLOTS, REPLY, PIDS)
        torch.cuda.synchronize()
        _check_deliver(spec, cs, gs, cpool, gpool)

    def test_giaretta_shape_update_mode(self):
        """57->100->2, bs 32: the 512-thread block, the K>64 padded MFMA
        loop and ~94 KB of LDS, in the mode that holds two model slabs."""
        spec = MLPSpec(
            57, 2, hidden=(100,), lr=0.1, batch_size=32, n_parts=4,
            mode=CreateModelMode.UPDATE,
        )
        cs, gs, cd, gd = _pair(4, spec, samples=160)
        assert cd.counts.tolist() == [40] * 4
        cpool, gpool = _pools(spec, cap=8)
        recv = torch.arange(4, dtype=torch.int64)
        ptr = torch.arange(5, dtype=torch.int64)
        slots = torch.tensor([0, 1, 2, 3], dtype=torch.int64)
        reply = torch.tensor([4, -1, 5, -1], dtype=torch.int64)
        pids = torch.tensor([0, 3, 1, 2], dtype=torch.int64)
        TorchBackend().deliver(cs, cpool, cd, spec, recv, ptr, slots, reply, pids)
        HIPBackend().deliver(gs, gpool, gd, spec, recv, ptr, slots, reply, pids)
        torch.cuda.synchronize()
        print(f"params err {_err(cs.params, gs.params):.3e}")
        assert _close(cs.params, gs.params)
        assert torch.equal(cs.ages, gs.ages.cpu())
        assert _close(cpool.slots[4:6], gpool.slots[4:6])
        assert torch.equal(cpool.slot_ages[4:6], gpool.slot_ages[4:6].cpu())

    @pytest.mark.parametrize("shape", ["11-20-3_bs8", "11-20-12-3"])
    def test_update_only(self, shape):
        spec = MLPSpec(11, 3, lr=0.1, n_parts=4, **SHAPES[shape])
        cs, gs, cd, gd = _pair(12, spec)
        nodes = torch.arange(12)
        TorchBackend().update(cs, cd, spec, nodes)
        HIPBackend().update(gs, gd, spec, nodes)
        torch.cuda.synchronize()
        print(f"params err {_err(cs.params, gs.params):.3e}")
        assert _close(cs.params, gs.params)
        assert torch.equal(cs.ages, gs.ages.cpu())


class TestSampledMLP:
    @pytest.mark.parametrize("sample_size", [0.3, 1.0])
    @pytest.mark.parametrize("mode", MODES, ids=lambda m: m.name)
    def test_deliver_matches_oracle(self, mode, sample_size):
        """samp_count 91 (resp. 303) draws with replacement from 303
        coordinates: duplicate indices are certain, and all of them must
        read the pre-merge value."""
        spec = MLPSpec(
            11, 3, hidden=(20,), lr=0.1, batch_size=0,
            sample_size=sample_size, mode=mode,
        )
        assert spec.samp_count() == (91 if sample_size == 0.3 else 303)
        cs, gs, cd, gd = _pair(12, spec)
        assert cs.ages.shape == (12,)
        cpool, gpool = _pools(spec)
        TorchBackend().deliver(cs, cpool, cd, spec, RECV, PTR, SLOTS, REPLY, SEEDS)
        HIPBackend().deliver(gs, gpool, gd, spec, RECV, PTR, SLOTS, REPLY, SEEDS)
        torch.cuda.synchronize()
        _check_deliver(spec, cs, gs, cpool, gpool)

    def test_update_only(self):
        spec = MLPSpec(
            11, 3, hidden=(20,), lr=0.1, batch_size=8, sample_size=0.3
        )
        cs, gs, cd, gd = _pair(12, spec)
        nodes = torch.arange(12)
        TorchBackend().update(cs, cd, spec, nodes)
        HIPBackend().update(gs, gd, spec, nodes)
        torch.cuda.synchronize()
        assert _close(cs.params, gs.params)
        assert torch.equal(cs.ages, gs.ages.cpu())


def _sim_data(n_nodes, device, seed=0):
    X, y = make_synthetic_classification((640, 57, 2), seed=seed, margin=2.0)
    idx = np.random.default_rng(seed).permutation(640)
    shards = [(X[s], y[s]) for s in np.array_split(idx[:576], n_nodes)]
    return DataArena.from_shards(
        shards, device, global_eval=(X[idx[576:]], y[idx[576:]])
    )


class TestRoundExecutors:
    @pytest.mark.parametrize("variant", ["partitioned", "sampled"])
    def test_fast_matches_tick_path(self, variant):
        data = _sim_data(64, CUDA)
        if variant == "partitioned":
            spec = MLPSpec(57, 2, hidden=(16,), lr=0.1, n_parts=4)
            kw = dict(n_parts=4)
        else:
            spec = MLPSpec(57, 2, hidden=(16,), lr=0.1, sample_size=0.3)
            kw = dict(sampled=True)
        cfg = EngineConfig(
            n_nodes=64, delta=10, protocol=AntiEntropyProtocol.PUSH_PULL,
            model_size=spec.D, sampling_eval=0.0, seed=3, **kw,
        )
        calls = {}

        def counted(sim, tag, name):
            orig = getattr(sim, name)

            def wrapper(*a, **kw):
                calls[tag, name] = calls.get((tag, name), 0) + 1
                return orig(*a, **kw)

            setattr(sim, name, wrapper)

        fast = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
        assert fast._fast_path_ok()
        counted(fast, "fast", "_run_round_fast")
        counted(fast, "fast", "_run_tick")
        fast.init_nodes()
        fast.start(n_rounds=4)

        # the per-tick arm: with only _fast_path_ok off, start() would still
        # flatten the python-scheduled round into the same C++ executor, so
        # that route is closed too and every phase goes through _run_tick
        # (HIPBackend.deliver -> tick_mlp_part / tick_mlp_samp)
        slow = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
        slow._fast_path_ok = lambda: False
        slow._flat_exec_ok = lambda: False
        counted(slow, "slow", "_run_round_fast")
        counted(slow, "slow", "_run_tick")
        slow.init_nodes()
        slow.start(n_rounds=4)
        torch.cuda.synchronize()
        assert calls.get(("fast", "_run_round_fast"), 0) == 4
        assert ("fast", "_run_tick") not in calls
        assert ("slow", "_run_round_fast") not in calls
        assert calls.get(("slow", "_run_tick"), 0) > 0
        print(f"fast vs tick err {_err(fast.local_params(), slow.local_params()):.3e}")
        assert torch.allclose(
            fast.local_params(), slow.local_params(), atol=1e-5, rtol=1e-5
        )
        assert torch.equal(fast.state.ages, slow.state.ages)
        assert int(fast.state.ages.max()) > 0

    @pytest.mark.parametrize("variant", ["partitioned", "sampled"])
    def test_gpu_matches_cpu_run(self, variant):
        """The learning configs of the CPU suite (40 nodes, 57->16->2, PUSH;
        partitioned: lr 0.5, P=4; sampled: lr 0.1, sample_size 0.3), cut to
        5 rounds: the GPU whole-round executor against the CPU oracle's
        per-tick run."""
        sims = {}
        for dev in (CPU, CUDA):
            data = _sim_data(40, dev, seed=1)
            if variant == "partitioned":
                spec = MLPSpec(57, 2, hidden=(16,), lr=0.5, n_parts=4)
                kw = dict(n_parts=4)
            else:
                spec = MLPSpec(57, 2, hidden=(16,), lr=0.1, sample_size=0.3)
                kw = dict(sampled=True)
            cfg = EngineConfig(
                n_nodes=40, delta=10, protocol=AntiEntropyProtocol.PUSH,
                model_size=spec.D, sampling_eval=0.25, seed=7, **kw,
            )
            sim = BatchedGossipSimulator(cfg, spec, data, device=dev)
            sim.init_nodes()
            sim.start(n_rounds=5)
            sims[dev.type] = sim
        torch.cuda.synchronize()
        assert sims["cuda"].backend.name == "hip"
        c, g = sims["cpu"].local_params(), sims["cuda"].local_params().cpu()
        print(f"cpu vs gpu err {_err(c, g):.3e}")
        assert torch.allclose(c, g, atol=1e-4, rtol=1e-4)
        assert torch.equal(sims["cpu"].state.ages, sims["cuda"].state.ages.cpu())


class TestHostChecks:
    """Both failures come from the launcher's host-side checks, before any
    kernel launch: state is untouched."""

    @pytest.mark.parametrize("variant", ["partitioned", "sampled"])
    def test_pass_mode_rejected(self, variant):
        kw = dict(n_parts=4) if variant == "partitioned" else dict(sample_size=0.3)
        spec = MLPSpec(
            11, 3, hidden=(20,), batch_size=0, mode=CreateModelMode.PASS, **kw
        )
        cs, gs, cd, gd = _pair(12, spec)
        cpool, gpool = _pools(spec)
        before = gs.params.clone()
        with pytest.raises(RuntimeError, match="PASS"):
            HIPBackend().deliver(
                gs, gpool, gd, spec, RECV, PTR, SLOTS, REPLY, PIDS
            )
        torch.cuda.synchronize()
        assert torch.equal(before, gs.params)

    @pytest.mark.parametrize("variant", ["partitioned", "sampled"])
    def test_lds_budget_rejected(self, variant):
        """11->4000->3 is a 60003-float (240 KB) model row: over the
        160 KiB block budget before activations are even counted."""
        kw = dict(n_parts=4) if variant == "partitioned" else dict(sample_size=0.3)
        spec = MLPSpec(11, 3, hidden=(4000,), batch_size=8, **kw)
        cs, gs, cd, gd = _pair(12, spec)
        before = gs.params.clone()
        with pytest.raises(RuntimeError, match="LDS budget"):
            HIPBackend().update(gs, gd, spec, torch.arange(12))
        torch.cuda.synchronize()
        assert torch.equal(before, gs.params)
