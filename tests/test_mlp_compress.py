"""Partitioned and sampled gossip for the MLP family on the CPU oracle:
spec surface, fidelity vs the object layer (PartitionedTMH over TorchMLP,
which mirrors gossipy/model/handler.py:455-525), end-to-end learning,
determinism, the tokenized / 2-rank / checkpoint paths and the example."""

import multiprocessing as mp
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from gossipy_amd.core import AntiEntropyProtocol, CreateModelMode, UniformDelay
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    BatchedTokenizedGossipSimulator,
    DataArena,
    EngineConfig,
    MLPSpec,
)
from gossipy_amd.engine.arena import NodeStateArena, SlotPool
from gossipy_amd.engine.backend import TorchBackend
from gossipy_amd.simul import SimulationReport

CPU = torch.device("cpu")


def _make_data(n_nodes, seed=1):
    """640x57 two-class data, margin 2.0: 576 train samples split evenly
    over the nodes, the remaining 64 as the global eval set."""
    X, y = make_synthetic_classification((640, 57, 2), seed=seed, margin=2.0)
    idx = np.random.default_rng(seed).permutation(640)
    shards = [(X[s], y[s]) for s in np.array_split(idx[:576], n_nodes)]
    return shards, (X[idx[576:]], y[idx[576:]])


def _arena_for_rank(shards, geval, rank, world):
    n = len(shards)
    lo, hi = rank * n // world, (rank + 1) * n // world
    return DataArena.from_shards(shards[lo:hi], CPU, global_eval=geval)


def _obj_handler(d, k, hidden, n_parts=4, lr=0.1):
    from gossipy_amd.model.handler import PartitionedTMH
    from gossipy_amd.model.nn import TorchMLP
    from gossipy_amd.model.sampling import TorchModelPartition

    net = TorchMLP(d, k, hidden)
    return PartitionedTMH(
        net,
        TorchModelPartition(net, n_parts),
        torch.optim.SGD,
        {"lr": lr},
        torch.nn.CrossEntropyLoss(),
        local_epochs=1,
        batch_size=0,
        create_model_mode=CreateModelMode.MERGE_UPDATE,
    )


def _row_from_model(net) -> torch.Tensor:
    """Arena row of a TorchMLP: per layer W (row-major) then b."""
    out = []
    for m in net.model.modules():
        if isinstance(m, torch.nn.Linear):
            out += [m.weight.detach().reshape(-1), m.bias.detach()]
    return torch.cat(out).clone()


class TestSpec:
    def test_geometry(self):
        spec = MLPSpec(11, 3, hidden=(20,), n_parts=4)
        assert spec.D == 303
        assert spec.part_ptr().tolist() == [0, 76, 152, 228, 303]
        assert spec.age_width == 4
        assert MLPSpec(11, 3, hidden=(20, 12), n_parts=4).D == 531

    @pytest.mark.parametrize("hidden", [(20,), (20, 12)])
    def test_cover_matches_object_layer(self, hidden):
        """part_perm/ptr == TorchModelPartition's cover in arena offsets."""
        d, k, P = 11, 3, 4
        h = _obj_handler(d, k, hidden, P)
        spec = MLPSpec(d, k, hidden=hidden, n_parts=P)
        perm, ptr = spec.part_perm(), spec.part_ptr()
        offs = spec.layer_offsets()
        seen = []
        for p in range(P):
            arena = []
            for li, (w_off, b_off, fin, fout) in enumerate(offs):
                ids_w = h.tm_partition.partitions[p][2 * li]
                if ids_w is not None:
                    arena.extend((w_off + ids_w[0] * fin + ids_w[1]).tolist())
                ids_b = h.tm_partition.partitions[p][2 * li + 1]
                if ids_b is not None:
                    arena.extend((b_off + ids_b[0]).tolist())
            assert sorted(arena) == sorted(perm[ptr[p] : ptr[p + 1]].tolist())
            seen += arena
        assert sorted(seen) == list(range(spec.D))
        apart = spec.arena_part()
        for p in range(P):
            assert (apart[perm[ptr[p] : ptr[p + 1]]] == p).all()

    def test_validation(self):
        with pytest.raises(ValueError):
            MLPSpec(11, 3, hidden=(8,), n_parts=4, sample_size=0.3)
        with pytest.raises(ValueError):
            MLPSpec(11, 3, hidden=(8,), n_parts=4, pass_through=True)
        with pytest.raises(ValueError):
            MLPSpec(11, 3, hidden=(8,), sample_size=0.3, pass_through=True)
        # the plain combinations stay legal
        MLPSpec(11, 3, hidden=(8,), pass_through=True)
        MLPSpec(11, 3, hidden=(8,), n_parts=4)

    def test_samp_count(self):
        spec = MLPSpec(11, 3, hidden=(20,), sample_size=0.3)
        assert spec.samp_count() == max(1, int(round(0.3 * 303))) == 91
        assert MLPSpec(11, 3, hidden=(20,)).sample_size == 0.0

    def test_positional_construction_unchanged(self):
        spec = MLPSpec(
            11, 3, (20,), 0.2, 0.0, 1, 8, CreateModelMode.UPDATE, 4, False
        )
        assert (spec.n_parts, spec.pass_through, spec.sample_size) == (4, False, 0.0)


class TestOracleVsObjectLayer:
    @pytest.mark.parametrize("hidden", [(20,), (20, 12)])
    def test_update_matches_object_layer(self, hidden):
        """Three successive full-batch partitioned local steps: the engine
        oracle == the object layer's autograd path (age increment + grad
        age-rescale)."""
        d, k, P = 11, 3, 4
        h = _obj_handler(d, k, hidden, P)
        h.n_updates[:] = [2, 0, 5, 1]
        spec = MLPSpec(
            d, k, hidden=hidden, lr=0.1, local_epochs=1, batch_size=0, n_parts=P
        )
        X, y = make_synthetic_classification((20, d, k), seed=3)
        state = NodeStateArena(1, spec.D, CPU, age_width=P)
        state.params[0] = _row_from_model(h.model)
        state.ages[0] = torch.tensor([2, 0, 5, 1], dtype=torch.int32)
        data = DataArena.from_shards([(X, y)], CPU)
        be = TorchBackend()
        for step in range(3):
            be.update(state, data, spec, torch.tensor([0]))
            h._update((X, y))
            assert np.array_equal(state.ages[0].numpy(), h.n_updates)
            err = (state.params[0] - _row_from_model(h.model)).abs().max()
            assert err <= 1e-6, f"step {step}: max abs {err:.3e}"

    def test_merge_matches_object_layer(self):
        d, k, P, hidden = 11, 3, 4, (20,)
        h1 = _obj_handler(d, k, hidden, P)
        h2 = _obj_handler(d, k, hidden, P)
        with torch.no_grad():
            for p_ in h2.model.parameters():
                p_.add_(torch.randn_like(p_))
        h1.n_updates[:] = [3, 0, 2, 7]
        h2.n_updates[:] = [1, 0, 4, 7]  # partition 1: both ages 0
        spec = MLPSpec(d, k, hidden=hidden, n_parts=P)
        state = NodeStateArena(1, spec.D, CPU, age_width=P)
        state.params[0] = _row_from_model(h1.model)
        state.ages[0] = torch.tensor(h1.n_updates, dtype=torch.int32)
        pool = SlotPool(spec.D, CPU, 4, age_width=P)
        pool.slots[2] = _row_from_model(h2.model)
        pool.slot_ages[2] = torch.tensor(h2.n_updates, dtype=torch.int32)
        be = TorchBackend()
        for pid in (0, 1, 3):
            be._merge_part(state, pool, spec, 0, 2, pid)
            h1._merge(h2, pid)
            assert torch.allclose(
                state.params[0], _row_from_model(h1.model), atol=1e-6
            ), f"partition {pid}"
            assert np.array_equal(state.ages[0].numpy(), h1.n_updates)

    def test_perm_cache_is_keyed_by_value(self):
        """Two specs with different covers must not share a perm table,
        whatever their ids; equal specs share one."""
        be = TorchBackend()
        a = MLPSpec(11, 3, hidden=(20,), n_parts=4)
        b = MLPSpec(11, 3, hidden=(20, 12), n_parts=4)
        pa, _, _ = be._part(a, CPU)
        pb, _, _ = be._part(b, CPU)
        assert len(pa) == a.D and len(pb) == b.D
        assert be._part(MLPSpec(11, 3, hidden=(20,), n_parts=4), CPU)[0] is pa


def _part_sim(rounds, mode=CreateModelMode.MERGE_UPDATE, lr=0.5, sim_cls=None,
              **cfg_kw):
    shards, geval = _make_data(40)
    data = DataArena.from_shards(shards, CPU, global_eval=geval)
    spec = MLPSpec(57, 2, hidden=(16,), lr=lr, n_parts=4, mode=mode)
    base = dict(
        n_nodes=40, delta=10, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.25, seed=7, n_parts=4,
    )
    base.update(cfg_kw)
    sim = BatchedGossipSimulator(EngineConfig(**base), spec, data, device=CPU)
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes()
    sim.start(n_rounds=rounds)
    return sim, rep


class TestEngineCPU:
    def test_partitioned_learns(self):
        sim, rep = _part_sim(30)
        acc = rep.get_evaluation(False)[-1][1]["accuracy"]
        print(f"partitioned MLP accuracy after 30 rounds: {acc:.4f}")
        assert acc > 0.9
        assert sim.state.ages.shape == (40, 4)

    @pytest.mark.parametrize(
        "mode", [CreateModelMode.MERGE_UPDATE, CreateModelMode.UPDATE_MERGE]
    )
    def test_sampled_learns(self, mode):
        shards, geval = _make_data(40)
        data = DataArena.from_shards(shards, CPU, global_eval=geval)
        spec = MLPSpec(57, 2, hidden=(16,), lr=0.1, sample_size=0.3, mode=mode)
        cfg = EngineConfig(
            n_nodes=40, delta=10, protocol=AntiEntropyProtocol.PUSH,
            model_size=spec.D, sampling_eval=0.25, seed=7, sampled=True,
        )
        sim = BatchedGossipSimulator(cfg, spec, data, device=CPU)
        rep = SimulationReport()
        sim.add_receiver(rep)
        sim.init_nodes()
        sim.start(n_rounds=15)
        acc = rep.get_evaluation(False)[-1][1]["accuracy"]
        print(f"sampled MLP ({mode.name}) accuracy after 15 rounds: {acc:.4f}")
        assert acc > 0.9
        assert sim.state.ages.dim() == 1

    def test_partitioned_deterministic(self):
        s1, _ = _part_sim(5)
        s2, _ = _part_sim(5)
        assert torch.equal(s1.local_params(), s2.local_params())
        assert torch.equal(s1.state.ages, s2.state.ages)

    def test_partitioned_tokenized_update_mode(self):
        from gossipy_amd.flow_control import RandomizedTokenAccount

        shards, geval = _make_data(40)
        data = DataArena.from_shards(shards, CPU, global_eval=geval)
        spec = MLPSpec(
            57, 2, hidden=(16,), lr=0.1, n_parts=4, mode=CreateModelMode.UPDATE
        )
        cfg = EngineConfig(
            n_nodes=40, delta=10, protocol=AntiEntropyProtocol.PUSH,
            model_size=spec.D, sampling_eval=0.25, seed=11, n_parts=4,
        )
        sim = BatchedTokenizedGossipSimulator(
            cfg, spec, data, token_account=RandomizedTokenAccount(C=20, A=10),
            device=CPU,
        )
        sim.init_nodes()
        sim.start(n_rounds=3)
        assert sim.state.ages.shape == (40, 4)
        assert int(sim.state.ages.max()) > 0
        assert torch.isfinite(sim.local_params()).all()

    def test_save_load_partitioned(self, tmp_path):
        kw = dict(
            protocol=AntiEntropyProtocol.PUSH_PULL, sampling_eval=0.0, seed=21,
            delay=UniformDelay(0, 12),
        )
        ref, _ = _part_sim(4, lr=0.1, **kw)
        sim, _ = _part_sim(2, lr=0.1, **kw)
        f = str(tmp_path / "ckpt_mlp_part.dill")
        sim.save(f)
        restored = BatchedGossipSimulator.load(f, device=CPU)
        assert restored.rounds_done == 2
        assert restored.spec.n_parts == 4 and restored.spec.family == "mlp"
        restored.start(n_rounds=2)
        assert torch.equal(ref.local_params(), restored.local_params())
        assert torch.equal(ref.state.ages, restored.state.ages)


def _two_rank_cfg_spec():
    spec = MLPSpec(57, 2, hidden=(16,), lr=0.1, n_parts=4)
    cfg = EngineConfig(
        n_nodes=40, delta=10, protocol=AntiEntropyProtocol.PUSH_PULL,
        model_size=spec.D, sampling_eval=0.25, seed=7, n_parts=4,
        delay=UniformDelay(0, 4),
    )
    return cfg, spec


def _mlp_part_worker(rank, world, port, q):
    import torch.distributed as dist

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        shards, geval = _make_data(40)
        data = _arena_for_rank(shards, geval, rank, world)
        cfg, spec = _two_rank_cfg_spec()
        sim = BatchedGossipSimulator(cfg, spec, data, device=CPU)
        sim.init_nodes()
        sim.start(n_rounds=5)
        full = sim.gather_params()
        if rank == 0:
            q.put(full.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_partitioned_mlp_two_rank_matches_single_rank():
    shards, geval = _make_data(40)
    data = DataArena.from_shards(shards, CPU, global_eval=geval)
    cfg, spec = _two_rank_cfg_spec()
    ref = BatchedGossipSimulator(cfg, spec, data, device=CPU)
    ref.init_nodes()
    ref.start(n_rounds=5)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [
        ctx.Process(target=_mlp_part_worker, args=(r, 2, 29561, q))
        for r in range(2)
    ]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
    assert np.array_equal(ref.local_params().numpy(), got)


@pytest.mark.timeout(300)
def test_hegedus_example_runs_with_mlp():
    r = subprocess.run(
        [sys.executable, "examples/main_hegedus_2021.py", "--model", "mlp",
         "--nodes", "30", "--rounds", "3"],
        capture_output=True,
        text=True,
        timeout=280,
    )
    assert r.returncode == 0, f"failed:\n{r.stdout}\n{r.stderr}"
