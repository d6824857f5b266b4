"""Limited-merge gossip (Danner 2023) on the CPU oracle: the
``age_diff_threshold`` spec field, ``TorchBackend._merge_limited`` against
the object layer's ``LimitedMergeTMH._merge`` (which mirrors
gossipy/model/handler.py:690-715), the vectorized torchmod wave, end-to-end
runs, the tokenized / 2-rank / checkpoint paths and the example."""

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
    BatchedAll2AllGossipSimulator,
    BatchedGossipSimulator,
    BatchedPENSGossipSimulator,
    BatchedTokenizedGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
    MLPSpec,
    TorchModuleSpec,
)
from gossipy_amd.engine.arena import NodeStateArena, SlotPool
from gossipy_amd.engine.backend import TorchBackend
from gossipy_amd.simul import SimulationReport

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# ---------------------------------------------------------------------------
# spec
# ---------------------------------------------------------------------------


class TestSpec:
    def test_default_is_plain_mean(self):
        assert LogRegSpec(5, 3).age_diff_threshold is None
        assert MLPSpec(5, 3).age_diff_threshold is None
        assert TorchModuleSpec(_tiny_module, (6,)).age_diff_threshold is None

    def test_zero_threshold_accepted(self):
        assert LogRegSpec(5, 3, age_diff_threshold=0).age_diff_threshold == 0
        assert MLPSpec(5, 3, age_diff_threshold=0).age_diff_threshold == 0
        spec = TorchModuleSpec(_tiny_module, (6,), age_diff_threshold=0)
        assert spec.age_diff_threshold == 0

    @pytest.mark.parametrize(
        "build",
        [
            lambda: LogRegSpec(5, 3, age_diff_threshold=-1),
            lambda: MLPSpec(5, 3, age_diff_threshold=-1),
            lambda: TorchModuleSpec(_tiny_module, (6,), age_diff_threshold=-1),
        ],
    )
    def test_negative_rejected(self, build):
        with pytest.raises(ValueError, match="age_diff_threshold"):
            build()

    @pytest.mark.parametrize("cls", [LogRegSpec, MLPSpec])
    @pytest.mark.parametrize(
        "other", [dict(n_parts=4), dict(sample_size=0.3)], ids=lambda d: next(iter(d))
    )
    def test_compressed_variants_rejected(self, cls, other):
        field = next(iter(other))
        with pytest.raises(ValueError) as ei:
            cls(5, 3, age_diff_threshold=2, **other)
        assert "age_diff_threshold" in str(ei.value) and field in str(ei.value)

    def test_pass_through_is_orthogonal(self):
        LogRegSpec(5, 3, pass_through=True, age_diff_threshold=2)
        MLPSpec(5, 3, pass_through=True, age_diff_threshold=2)

    def test_positional_construction_unchanged(self):
        spec = LogRegSpec(
            5, 3, 0.2, 0.01, 2, 8, CreateModelMode.UPDATE, 4, 0.0, False
        )
        assert (spec.n_parts, spec.sample_size, spec.pass_through) == (4, 0.0, False)
        assert spec.age_diff_threshold is None
        spec = MLPSpec(
            11, 3, (20,), 0.2, 0.0, 1, 8, CreateModelMode.UPDATE, 4, False, 0.0
        )
        assert (spec.n_parts, spec.pass_through, spec.sample_size) == (4, False, 0.0)
        assert spec.age_diff_threshold is None

    def test_last_field(self):
        import dataclasses

        for cls in (LogRegSpec, MLPSpec):
            assert dataclasses.fields(cls)[-1].name == "age_diff_threshold"

    @pytest.mark.parametrize(
        "sim_cls", [BatchedPENSGossipSimulator, BatchedAll2AllGossipSimulator]
    )
    def test_pens_and_all2all_refuse(self, sim_cls):
        shards, geval = _make_data(8)
        data = DataArena.from_shards(shards, CPU, global_eval=geval)
        spec = LogRegSpec(57, 2, age_diff_threshold=2)
        cfg = EngineConfig(
            n_nodes=8, delta=5, protocol=AntiEntropyProtocol.PUSH,
            model_size=spec.D,
        )
        with pytest.raises(ValueError, match="age_diff_threshold"):
            sim_cls(cfg, spec, data, device=CPU)


# ---------------------------------------------------------------------------
# oracle vs object layer
# ---------------------------------------------------------------------------


def _row(net) -> torch.Tensor:
    """Arena row of a LogisticRegression / TorchMLP: per layer W
    (row-major) then b — the ``parameters()`` order."""
    return torch.cat([p.detach().reshape(-1) for p in net.parameters()]).clone()


def _handler(kind, L):
    from gossipy_amd.model.handler import LimitedMergeTMH
    from gossipy_amd.model.nn import LogisticRegression, TorchMLP

    net = LogisticRegression(5, 3) if kind == "logreg" else TorchMLP(5, 3, (4,))
    h = LimitedMergeTMH(
        net, torch.optim.SGD, {"lr": 0.1}, torch.nn.CrossEntropyLoss(),
        create_model_mode=CreateModelMode.MERGE_UPDATE, age_diff_threshold=L,
    )
    with torch.no_grad():
        for p in h.model.parameters():
            p.copy_(torch.randn_like(p))
    return h


def _branch(a, b, L):
    return "keep" if a > b + L else ("adopt" if b > a + L else "weighted")


# (receiver age, received age) per threshold: keep, adopt, weighted, and the
# two boundaries a == b + L and b == a + L (both weighted)
AGE_PAIRS = {
    0: [(5, 4), (4, 5), (3, 3), (7, 7)],
    2: [(9, 3), (3, 9), (4, 5), (1, 2), (6, 4), (4, 6), (1000001, 999999)],
}


class TestOracleVsObjectLayer:
    @pytest.mark.parametrize("kind", ["logreg", "mlp"])
    @pytest.mark.parametrize("L", [0, 2])
    def test_merge_matches_object_layer(self, kind, L):
        torch.manual_seed(11)
        be = TorchBackend()
        seen = set()
        for a, b in AGE_PAIRS[L]:
            h1, h2 = _handler(kind, L), _handler(kind, L)
            h1.n_updates, h2.n_updates = a, b
            D = len(_row(h1.model))
            state = NodeStateArena(2, D, CPU)
            pool = SlotPool(D, CPU, 4)
            state.params[1] = _row(h1.model)
            state.ages[1] = a
            pool.slots[2] = _row(h2.model)
            pool.slot_ages[2] = b
            own, recv = state.params[1].clone(), pool.slots[2].clone()
            be._merge_limited(state, pool, 1, 2, L)
            h1._merge(h2)
            err = float((state.params[1] - _row(h1.model)).abs().max())
            assert err <= 1e-6, f"ages {(a, b)}: max abs {err:.3e}"
            assert int(state.ages[1]) == h1.n_updates == max(a, b)
            br = _branch(a, b, L)
            seen.add(br)
            if br == "keep":
                assert torch.equal(state.params[1], own)
            elif br == "adopt":
                assert torch.equal(state.params[1], recv)
        assert seen == {"keep", "adopt", "weighted"}
        if L == 2:
            assert _branch(6, 4, L) == _branch(4, 6, L) == "weighted"

    def test_zero_zero_is_plain_mean(self):
        """a + b == 0: the reference divides by zero; the engine averages."""
        torch.manual_seed(3)
        state = NodeStateArena(1, 18, CPU)
        pool = SlotPool(18, CPU, 2)
        state.params[0] = torch.randn(18)
        pool.slots[1] = torch.randn(18)
        want = (state.params[0] + pool.slots[1]) * 0.5
        TorchBackend()._merge_limited(state, pool, 0, 1, 2)
        assert torch.equal(state.params[0], want)
        assert int(state.ages[0]) == 0

    @pytest.mark.parametrize("mode", [
        CreateModelMode.MERGE_UPDATE, CreateModelMode.UPDATE_MERGE,
    ], ids=lambda m: m.name)
    def test_deliver_uses_the_rule(self, mode):
        """A delivery whose receiver is far ahead keeps its model under a
        threshold and averages without one; UPDATE_MERGE applies the rule
        to the post-training ages."""
        X, y = make_synthetic_classification((20, 5, 3), seed=3)

        def run(L):
            spec = LogRegSpec(5, 3, lr=0.0, mode=mode, age_diff_threshold=L)
            state = NodeStateArena(1, spec.D, CPU)
            pool = SlotPool(spec.D, CPU, 2)
            g = torch.Generator().manual_seed(1)
            state.params[0] = torch.randn(spec.D, generator=g)
            pool.slots[1] = torch.randn(spec.D, generator=g)
            state.ages[0] = 9
            pool.slot_ages[1] = 3
            before = state.params[0].clone()
            data = DataArena.from_shards([(X, y)], CPU)
            TorchBackend().deliver(
                state, pool, data, spec, torch.tensor([0]),
                torch.tensor([0, 1]), torch.tensor([1]), torch.tensor([-1]),
            )
            return before, state

        before, st = run(2)
        assert torch.equal(st.params[0], before)
        assert int(st.ages[0]) == 10
        before, st = run(None)
        assert not torch.equal(st.params[0], before)
        assert int(st.ages[0]) == 10


# ---------------------------------------------------------------------------
# torchmod: vectorized wave == per-message loop
# ---------------------------------------------------------------------------


def _tiny_module():
    return torch.nn.Sequential(
        torch.nn.Linear(6, 4), torch.nn.ReLU(), torch.nn.Linear(4, 3)
    )


class TestTorchmod:
    def test_vectorized_wave_matches_loop(self, monkeypatch):
        L = 2
        spec = TorchModuleSpec(
            _tiny_module, input_shape=(6,), lr=0.1, batch_size=0,
            age_diff_threshold=L,
        )
        X, y = make_synthetic_classification((40, 6, 3), seed=2)
        shards = [(X[s], y[s]) for s in np.array_split(np.arange(40), 4)]
        data = DataArena.from_shards(shards, CPU)
        node_ages = [9, 1, 4, 0]
        slot_ages = [3, 8, 5, 0, 6]
        recv = torch.tensor([0, 1, 2, 3])
        ptr = torch.tensor([0, 1, 2, 4, 5])
        dslots = torch.tensor([0, 1, 2, 4, 3])
        reply = torch.tensor([-1, 5, -1, 6, -1])
        first = [(9, 3), (1, 8), (4, 5), (0, 0)]
        assert {_branch(a, b, L) for a, b in first} == {"keep", "adopt", "weighted"}

        def run(loop):
            if loop:
                monkeypatch.setenv("GOSSIPY_TORCHMOD_LOOP", "1")
            else:
                monkeypatch.delenv("GOSSIPY_TORCHMOD_LOOP", raising=False)
            g = torch.Generator().manual_seed(7)
            state = NodeStateArena(4, spec.D, CPU)
            state.params.copy_(torch.randn(4, spec.D, generator=g) * 0.3)
            state.ages.copy_(torch.tensor(node_ages, dtype=torch.int32))
            pool = SlotPool(spec.D, CPU, 8)
            pool.slots.copy_(torch.randn(8, spec.D, generator=g) * 0.3)
            pool.slot_ages[:5] = torch.tensor(slot_ages, dtype=torch.int32)
            TorchBackend().deliver(
                state, pool, data, spec, recv, ptr, dslots, reply
            )
            return state, pool

        vs, vp = run(False)
        ls, lp = run(True)
        assert torch.equal(vs.ages, ls.ages)
        assert torch.equal(vp.slot_ages, lp.slot_ages)
        assert torch.allclose(vs.params, ls.params, atol=1e-6)
        assert torch.allclose(vp.slots, lp.slots, atol=1e-6)
        # node 0 kept its model: one SGD step from the prior row either way
        assert int(vs.ages[0]) == 10 and int(vs.ages[1]) == 9


# ---------------------------------------------------------------------------
# engine on CPU
# ---------------------------------------------------------------------------


def _sim(rounds, spec=None, sim_cls=BatchedGossipSimulator, n=20, sim_kw=None,
         **cfg_kw):
    shards, geval = _make_data(n)
    data = DataArena.from_shards(shards, CPU, global_eval=geval)
    if spec is None:
        spec = LogRegSpec(57, 2, lr=0.1, batch_size=8, age_diff_threshold=2)
    base = dict(
        n_nodes=n, delta=10, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=1.0, seed=7,
    )
    base.update(cfg_kw)
    sim = sim_cls(EngineConfig(**base), spec, data, device=CPU, **(sim_kw or {}))
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes()
    if rounds:
        sim.start(n_rounds=rounds)
    return sim, rep


def _accuracy(sim):
    scores = sim.backend.scores(
        sim.state, sim.spec, torch.arange(sim.n_local), sim.data.gx
    )
    pred = scores.argmax(dim=-1)
    return float((pred == sim.data.gy.long()[None, :]).float().mean())


class TestEngineCPU:
    @pytest.mark.parametrize("family", ["logreg", "mlp"])
    def test_learns(self, family):
        spec = (
            LogRegSpec(57, 2, lr=0.1, batch_size=8, age_diff_threshold=2)
            if family == "logreg"
            else MLPSpec(57, 2, hidden=(16,), lr=0.1, batch_size=8,
                         age_diff_threshold=2)
        )
        sim, _ = _sim(0, spec=spec)
        start = _accuracy(sim)
        sim.start(n_rounds=10)
        end = _accuracy(sim)
        print(f"{family}: accuracy {start:.4f} -> {end:.4f}")
        assert end > start
        assert int(sim.state.ages.max()) > 0

    def test_deterministic(self):
        s1, _ = _sim(4)
        s2, _ = _sim(4)
        assert torch.equal(s1.local_params(), s2.local_params())
        assert torch.equal(s1.state.ages, s2.state.ages)

    def test_threshold_changes_the_run(self):
        """The rule is live end to end: same config without a threshold
        ends elsewhere."""
        lim, _ = _sim(4)
        plain, _ = _sim(4, spec=LogRegSpec(57, 2, lr=0.1, batch_size=8))
        assert not torch.equal(lim.local_params(), plain.local_params())

    def test_tokenized(self):
        from gossipy_amd.flow_control import RandomizedTokenAccount

        sim, _ = _sim(
            3, sim_cls=BatchedTokenizedGossipSimulator,
            sim_kw=dict(token_account=RandomizedTokenAccount(C=20, A=10)),
        )
        assert int(sim.state.ages.max()) > 0
        assert torch.isfinite(sim.local_params()).all()

    def test_save_load(self, tmp_path):
        kw = dict(
            protocol=AntiEntropyProtocol.PUSH_PULL, sampling_eval=0.0, seed=21,
            delay=UniformDelay(0, 12),
        )
        ref, _ = _sim(4, **kw)
        sim, _ = _sim(2, **kw)
        f = str(tmp_path / "ckpt_limited.dill")
        sim.save(f)
        restored = BatchedGossipSimulator.load(f, device=CPU)
        assert restored.rounds_done == 2
        assert restored.spec.age_diff_threshold == 2
        restored.start(n_rounds=2)
        assert torch.equal(ref.local_params(), restored.local_params())
        assert torch.equal(ref.state.ages, restored.state.ages)

    def test_spec_without_the_attribute_still_runs(self):
        """A spec unpickled from an older checkpoint has no such attribute."""
        spec = LogRegSpec(57, 2, lr=0.1, batch_size=8)
        del spec.__dict__["age_diff_threshold"]
        assert "age_diff_threshold" not in vars(spec)
        old, _ = _sim(2, spec=spec)
        new, _ = _sim(2, spec=LogRegSpec(57, 2, lr=0.1, batch_size=8))
        assert torch.equal(old.local_params(), new.local_params())

    @pytest.mark.parametrize("family", ["logreg", "mlp"])
    def test_none_equals_spec_without_argument(self, family):
        if family == "logreg":
            a = LogRegSpec(57, 2, lr=0.1, batch_size=8)
            b = LogRegSpec(57, 2, lr=0.1, batch_size=8, age_diff_threshold=None)
        else:
            a = MLPSpec(57, 2, hidden=(16,), lr=0.1)
            b = MLPSpec(57, 2, hidden=(16,), lr=0.1, age_diff_threshold=None)
        sa, _ = _sim(3, spec=a, protocol=AntiEntropyProtocol.PUSH_PULL)
        sb, _ = _sim(3, spec=b, protocol=AntiEntropyProtocol.PUSH_PULL)
        assert torch.equal(sa.local_params(), sb.local_params())
        assert torch.equal(sa.state.ages, sb.state.ages)


# ---------------------------------------------------------------------------
# two gloo ranks == one rank
# ---------------------------------------------------------------------------


def _two_rank_cfg_spec():
    spec = LogRegSpec(57, 2, lr=0.1, batch_size=8, age_diff_threshold=2)
    cfg = EngineConfig(
        n_nodes=40, delta=10, protocol=AntiEntropyProtocol.PUSH_PULL,
        model_size=spec.D, sampling_eval=0.25, seed=7,
        delay=UniformDelay(0, 4),
    )
    return cfg, spec


def _limited_worker(rank, world, port, q):
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
def test_limited_two_rank_matches_single_rank():
    shards, geval = _make_data(40)
    data = DataArena.from_shards(shards, CPU, global_eval=geval)
    cfg, spec = _two_rank_cfg_spec()
    ref = BatchedGossipSimulator(cfg, spec, data, device=CPU)
    ref.init_nodes()
    ref.start(n_rounds=5)

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [
        ctx.Process(target=_limited_worker, args=(r, 2, 29567, q))
        for r in range(2)
    ]
    for p in procs:
        p.start()
    got = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
    assert np.array_equal(ref.local_params().numpy(), got)


# ---------------------------------------------------------------------------
# example
# ---------------------------------------------------------------------------


@pytest.mark.timeout(300)
@pytest.mark.parametrize("model", ["logreg", "mlp"])
def test_danner_example_runs_on_the_engine(model):
    r = subprocess.run(
        [sys.executable, "examples/main_danner_2023.py", "--engine",
         "--model", model, "--hidden", "16", "--nodes", "10", "--rounds", "2"],
        capture_output=True,
        text=True,
        timeout=280,
        cwd=ROOT,
    )
    assert r.returncode == 0, f"failed:\n{r.stdout}\n{r.stderr}"
    assert "final global eval" in r.stdout
