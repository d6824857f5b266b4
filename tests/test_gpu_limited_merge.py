"""GPU tests (MI355X) for limited-merge gossip (``age_diff_threshold``):
the LIM instantiations of tick_logreg / tick_mlp against the fp32 torch
oracle branch by branch and delivery by delivery, the whole-round executor
against the per-tick route, CPU <-> GPU end to end, and the host-side
checks. All marked ``gpu``."""

import os
import subprocess
import sys

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
    LogRegSpec,
    MLPSpec,
    NodeStateArena,
    PegasosSpec,
    RandomTape,
    SlotPool,
)
from gossipy_amd.engine.backend import HIPBackend, TorchBackend

CUDA = torch.device("cuda:0")
CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

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


def _close(a, b, tol=1e-4):
    return torch.allclose(a.cpu(), b.cpu(), atol=tol, rtol=tol)


def _err(a, b):
    return float((a.cpu() - b.cpu()).abs().max())


def _to_gpu(cs, cd):
    gs = NodeStateArena(cs.params.shape[0], cs.params.shape[1], CUDA)
    gs.params.copy_(cs.params)
    gs.ages.copy_(cs.ages)
    gd = DataArena(
        cd.x.to(CUDA), cd.y.to(CUDA), cd.counts.to(CUDA),
        gx=cd.gx.to(CUDA), gy=cd.gy.to(CUDA),
    )
    return gs, gd


def _pair(n, spec, samples=160, seed=3):
    """(cpu, gpu) copies of identical state/data."""
    cs = NodeStateArena(n, spec.D, CPU)
    TorchBackend().init_params(cs, spec, RandomTape(seed), n)
    # logreg rows start at zero: give every node a model of its own
    cs.params.add_(
        torch.randn(n, spec.D, generator=torch.Generator().manual_seed(9)) * 0.2
    )
    cs.ages += torch.arange(n, dtype=torch.int32) % 5
    X, y = make_synthetic_classification(
        (samples, spec.d_in, spec.n_classes), seed=seed
    )
    shards = [(X[s], y[s]) for s in np.array_split(np.arange(samples), n)]
    cd = DataArena.from_shards(shards, CPU, global_eval=(X, y))
    gs, gd = _to_gpu(cs, cd)
    return cs, gs, cd, gd


def _pools(spec, cap=16):
    """Slot pools holding model-scaled random rows and distinct ages."""
    cpool = SlotPool(spec.D, CPU, cap)
    gpool = SlotPool(spec.D, CUDA, cap)
    cpool.slots.normal_(generator=torch.Generator().manual_seed(5))
    cpool.slots.mul_(0.2)
    cpool.slot_ages.copy_(torch.arange(cap, dtype=torch.int32) % 7)
    gpool.slots.copy_(cpool.slots)
    gpool.slot_ages.copy_(cpool.slot_ages)
    return cpool, gpool


def _check_deliver(cs, gs, cpool, gpool):
    print(
        f"params err {_err(cs.params, gs.params):.3e}"
        f" reply-slot err {_err(cpool.slots[12:14], gpool.slots[12:14]):.3e}"
    )
    assert _close(cs.params, gs.params)
    assert torch.equal(cs.ages, gs.ages.cpu())
    assert _close(cpool.slots[12:14], gpool.slots[12:14])
    assert torch.equal(cpool.slot_ages[12:14], gpool.slot_ages[12:14].cpu())


# ---------------------------------------------------------------------------
# branch exactness
# ---------------------------------------------------------------------------

# With lr = 0 SGD leaves every parameter bit-unchanged while the age still
# grows by one per full-batch step, so each delivery's effect on the row is
# the merge rule alone. Four receivers; node 3 has an EMPTY shard (its age
# never grows), which is the only way a later delivery can see ages (0, 0).
BR_L = 2
BR_NODE_AGES = [10, 1, 5, 0]
BR_COUNTS = [7, 6, 5, 0]
#            receiver 0      receiver 1   receiver 2   receiver 3
BR_PTR = [0, 3, 5, 7, 10]
BR_SLOTS = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
BR_SLOT_AGES = [3, 20, 20, 9, 4, 6, 7, 0, 0, 5]
BR_REPLY = [-1, -1, 12, -1, 13, 14, -1, -1, 15, -1]


def _branch(a, b, L):
    if a > b + L:
        return "keep"
    if b > a + L:
        return "adopt"
    return "zero" if a + b == 0 else "weighted"


def _expected_branches():
    """Per receiver, the (branch, age after the delivery) of each of its
    deliveries under MERGE_UPDATE with one step per delivery."""
    out = []
    for i, a in enumerate(BR_NODE_AGES):
        step = 1 if BR_COUNTS[i] > 0 else 0
        seq = []
        for j in range(BR_PTR[i], BR_PTR[i + 1]):
            b = BR_SLOT_AGES[j]
            br = _branch(a, b, BR_L)
            a = max(a, b) + step
            seq.append((br, a))
        out.append(seq)
    return out


def _branch_spec(family):
    if family == "logreg":
        # D = 1048 > 8 * 128: the fused path's tail loop runs as well
        return LogRegSpec(
            130, 8, lr=0.0, batch_size=0, age_diff_threshold=BR_L
        )
    return MLPSpec(
        11, 3, hidden=(20,), lr=0.0, batch_size=0, age_diff_threshold=BR_L
    )


def _branch_setup(spec):
    g = torch.Generator().manual_seed(17)
    cs = NodeStateArena(4, spec.D, CPU)
    cs.params.copy_(torch.randn(4, spec.D, generator=g) * 0.3)
    cs.ages.copy_(torch.tensor(BR_NODE_AGES, dtype=torch.int32))
    X, y = make_synthetic_classification(
        (sum(BR_COUNTS), spec.d_in, spec.n_classes), seed=4
    )
    cuts = np.cumsum([0] + BR_COUNTS)
    shards = [(X[cuts[i] : cuts[i + 1]], y[cuts[i] : cuts[i + 1]]) for i in range(4)]
    cd = DataArena.from_shards(shards, CPU, global_eval=(X, y))
    assert cd.counts.tolist() == BR_COUNTS
    cpool = SlotPool(spec.D, CPU, 16)
    cpool.slots.copy_(torch.randn(16, spec.D, generator=g) * 0.3)
    cpool.slot_ages.zero_()
    cpool.slot_ages[:10] = torch.tensor(BR_SLOT_AGES, dtype=torch.int32)
    return cs, cd, cpool


class TestBranchExactness:
    def test_pattern_covers_every_branch_in_both_positions(self):
        seqs = _expected_branches()
        first = {s[0][0] for s in seqs}
        later = {br for s in seqs for br, _ in s[1:]}
        every = {"keep", "adopt", "weighted", "zero"}
        assert first == every, first
        assert later == every, later
        # one receiver with three deliveries, one of them with a reply slot
        assert any(
            BR_PTR[i + 1] - BR_PTR[i] >= 3
            and any(r >= 0 for r in BR_REPLY[BR_PTR[i] : BR_PTR[i + 1]])
            for i in range(4)
        )

    @pytest.mark.parametrize("family", ["logreg", "mlp"])
    def test_each_delivery_takes_its_branch(self, family):
        """Deliver the first p messages of every receiver, p = 1, 2, 3, each
        from the same start state: delivery p is then the LAST of one launch
        (p = 1: the logreg fused path; p > 1: a later delivery, behind the
        register prefetch), and its effect is the difference between the
        runs p - 1 and p."""
        spec = _branch_spec(family)
        seqs = _expected_branches()
        hip, oracle = HIPBackend(), TorchBackend()
        recv = torch.arange(4, dtype=torch.int64)
        cs0, cd, cpool0 = _branch_setup(spec)
        prev = cs0.params.clone()
        for p in (1, 2, 3):
            cnt = [min(p, BR_PTR[i + 1] - BR_PTR[i]) for i in range(4)]
            sel = [BR_PTR[i] + w for i in range(4) for w in range(cnt[i])]
            ptr = torch.tensor(np.cumsum([0] + cnt), dtype=torch.int64)
            dslots = torch.tensor([BR_SLOTS[j] for j in sel], dtype=torch.int64)
            reply = torch.tensor([BR_REPLY[j] for j in sel], dtype=torch.int64)
            cs, cd, cpool = _branch_setup(spec)
            gs, gd = _to_gpu(cs, cd)
            gpool = SlotPool(spec.D, CUDA, 16)
            gpool.slots.copy_(cpool.slots)
            gpool.slot_ages.copy_(cpool.slot_ages)
            oracle.deliver(cs, cpool, cd, spec, recv, ptr, dslots, reply)
            hip.deliver(gs, gpool, gd, spec, recv, ptr, dslots, reply)
            torch.cuda.synchronize()
            got = gs.params.cpu()
            for i in range(4):
                if len(seqs[i]) < p:
                    continue
                br, age = seqs[i][p - 1]
                j = BR_PTR[i] + p - 1
                tag = f"receiver {i} delivery {p} ({br})"
                if br == "keep":
                    assert torch.equal(got[i], prev[i]), tag
                elif br == "adopt":
                    assert torch.equal(got[i], cpool0.slots[BR_SLOTS[j]]), tag
                else:
                    err = _err(got[i], cs.params[i])
                    print(f"{tag}: err vs oracle {err:.3e}")
                    assert torch.allclose(
                        got[i], cs.params[i], atol=1e-6, rtol=0
                    ), tag
                    if br == "zero":
                        want = (prev[i] + cpool0.slots[BR_SLOTS[j]]) * 0.5
                        assert torch.allclose(got[i], want, atol=1e-6, rtol=0)
                assert int(gs.ages[i]) == age, tag
                r = BR_REPLY[j]
                if r >= 0:
                    # the reply snapshot is the row right after delivery p
                    assert torch.equal(gpool.slots[r].cpu(), got[i]), tag
                    assert int(gpool.slot_ages[r]) == age, tag
            assert torch.equal(cs.ages, gs.ages.cpu())
            assert torch.equal(cpool.slot_ages, gpool.slot_ages.cpu())
            assert torch.allclose(cs.params, got, atol=1e-6, rtol=0)
            assert torch.allclose(
                cpool.slots, gpool.slots.cpu(), atol=1e-6, rtol=0
            )
            prev = got.clone()


# ---------------------------------------------------------------------------
# deliver against the oracle
# ---------------------------------------------------------------------------

LOGREG_SHAPES = {
    # shards of 13/14 rows -> batches of 8 + a ragged 5/6, two epochs: the
    # staged batch does not survive across deliveries
    "5x3_bs8": dict(d_in=5, n_classes=3, batch_size=8, local_epochs=2),
    # the flagship row, single batch
    "57x2": dict(d_in=57, n_classes=2),
    # D = 1048 > 8 * 128 prefetched elements: the fused path's tail loop
    "130x8": dict(d_in=130, n_classes=8, weight_decay=0.01),
}

MLP_SHAPES = {
    "11-20-3_fullbatch": dict(hidden=(20,), batch_size=0),
    "11-20-3_bs8": dict(
        hidden=(20,), batch_size=8, local_epochs=2, weight_decay=0.01
    ),
    "11-20-12-3": dict(hidden=(20, 12), batch_size=0),
}


class TestDeliverMatchesOracle:
    @pytest.mark.parametrize("L", [0, 2])
    @pytest.mark.parametrize("shape", sorted(LOGREG_SHAPES))
    @pytest.mark.parametrize("mode", MODES, ids=lambda m: m.name)
    def test_logreg(self, mode, shape, L):
        spec = LogRegSpec(
            lr=0.1, mode=mode, age_diff_threshold=L, **LOGREG_SHAPES[shape]
        )
        cs, gs, cd, gd = _pair(12, spec)
        cpool, gpool = _pools(spec)
        TorchBackend().deliver(cs, cpool, cd, spec, RECV, PTR, SLOTS, REPLY)
        HIPBackend().deliver(gs, gpool, gd, spec, RECV, PTR, SLOTS, REPLY)
        torch.cuda.synchronize()
        _check_deliver(cs, gs, cpool, gpool)

    @pytest.mark.parametrize("L", [0, 2])
    @pytest.mark.parametrize("shape", sorted(MLP_SHAPES))
    @pytest.mark.parametrize("mode", MODES, ids=lambda m: m.name)
    def test_mlp(self, mode, shape, L):
        spec = MLPSpec(
            11, 3, lr=0.1, mode=mode, age_diff_threshold=L, **MLP_SHAPES[shape]
        )
        cs, gs, cd, gd = _pair(12, spec)
        cpool, gpool = _pools(spec)
        TorchBackend().deliver(cs, cpool, cd, spec, RECV, PTR, SLOTS, REPLY)
        HIPBackend().deliver(gs, gpool, gd, spec, RECV, PTR, SLOTS, REPLY)
        torch.cuda.synchronize()
        _check_deliver(cs, gs, cpool, gpool)

    def test_logreg_pass_through_mixed_coins(self):
        """PASS deliveries adopt, the others use the limited rule — in the
        first (the fused path must step aside for a PASS first delivery)
        and in later positions."""
        spec = LogRegSpec(
            57, 2, lr=0.1, pass_through=True, age_diff_threshold=2
        )
        recv = torch.tensor([2, 5, 9], dtype=torch.int64)
        ptr = torch.tensor([0, 3, 5, 6], dtype=torch.int64)
        slots = torch.tensor([1, 4, 7, 10, 3, 6], dtype=torch.int64)
        reply = torch.tensor([12, -1, -1, 13, -1, -1], dtype=torch.int64)
        coins = torch.tensor([0, 1, 0, 1, 0, 1], dtype=torch.int64)
        cs, gs, cd, gd = _pair(12, spec)
        cpool, gpool = _pools(spec)
        TorchBackend().deliver(cs, cpool, cd, spec, recv, ptr, slots, reply, coins)
        HIPBackend().deliver(gs, gpool, gd, spec, recv, ptr, slots, reply, coins)
        torch.cuda.synchronize()
        _check_deliver(cs, gs, cpool, gpool)
        # node 9's only delivery is a PASS: adopted bit for bit, never trained
        assert torch.equal(gs.params[9].cpu(), cpool.slots[6])
        assert int(gs.ages[9]) == int(cpool.slot_ages[6])

    @pytest.mark.parametrize("family", ["logreg", "mlp"])
    def test_threshold_none_is_the_plain_kernel(self, family):
        """Same call, threshold None vs a huge threshold: a huge L never
        keeps or adopts, so only the weights differ — and with equal ages
        they are (1/2, 1/2) too."""
        kw = dict(lr=0.1, batch_size=0)
        mk = (
            (lambda **k: LogRegSpec(57, 2, **kw, **k))
            if family == "logreg"
            else (lambda **k: MLPSpec(11, 3, hidden=(20,), **kw, **k))
        )
        out = []
        ptr = torch.tensor([0, 1, 2, 3], dtype=torch.int64)  # one message each
        for spec in (mk(), mk(age_diff_threshold=1 << 20)):
            cs, gs, cd, gd = _pair(12, spec)
            gs.ages.fill_(4)
            cpool, gpool = _pools(spec)
            gpool.slot_ages.fill_(4)
            HIPBackend().deliver(
                gs, gpool, gd, spec, RECV, ptr, SLOTS[:3], REPLY[:3]
            )
            torch.cuda.synchronize()
            out.append((gs.params.cpu(), gs.ages.cpu()))
        assert torch.equal(out[0][1], out[1][1])
        assert torch.allclose(out[0][0], out[1][0], atol=1e-6, rtol=0)


# ---------------------------------------------------------------------------
# whole-round executor, end to end
# ---------------------------------------------------------------------------


def _sim_data(n_nodes, device, seed=0):
    X, y = make_synthetic_classification((640, 57, 2), seed=seed, margin=2.0)
    idx = np.random.default_rng(seed).permutation(640)
    shards = [(X[s], y[s]) for s in np.array_split(idx[:576], n_nodes)]
    return DataArena.from_shards(
        shards, device, global_eval=(X[idx[576:]], y[idx[576:]])
    )


# L = 1 with 9-row shards in batches of 4 (3 steps per update): ages move in
# threes, so gaps beyond L and ties within it both occur from round one
E2E_ROUNDS = 4


def _e2e_spec(family):
    if family == "logreg":
        return LogRegSpec(57, 2, lr=0.1, batch_size=4, age_diff_threshold=1)
    return MLPSpec(
        57, 2, hidden=(16,), lr=0.1, batch_size=4, age_diff_threshold=1
    )


def _e2e_cfg(spec):
    return EngineConfig(
        n_nodes=64, delta=10, protocol=AntiEntropyProtocol.PUSH_PULL,
        model_size=spec.D, sampling_eval=0.0, seed=3,
    )


def _cpu_replay(family):
    """CPU oracle run of the end-to-end config, counting the branch every
    merge takes through a thin wrapper around ``_merge_limited``."""
    spec = _e2e_spec(family)
    sim = BatchedGossipSimulator(
        _e2e_cfg(spec), spec, _sim_data(64, CPU), device=CPU
    )
    counts = {"keep": 0, "adopt": 0, "weighted": 0, "zero": 0}
    orig = sim.backend._merge_limited

    def counting(state, pool, node, slot, L):
        a, b = int(state.ages[node]), int(pool.slot_ages[slot])
        counts[_branch(a, b, L)] += 1
        return orig(state, pool, node, slot, L)

    sim.backend._merge_limited = counting
    sim.init_nodes()
    sim.start(n_rounds=E2E_ROUNDS)
    return sim, counts


_REPLAYS = {}


@pytest.fixture
def cpu_replay():
    """The CPU reference run per family, computed once and left unchanged."""

    def get(family):
        if family not in _REPLAYS:
            _REPLAYS[family] = _cpu_replay(family)
        return _REPLAYS[family]

    return get


class TestRoundExecutors:
    @pytest.mark.parametrize("family", ["logreg", "mlp"])
    def test_replay_takes_every_branch(self, family, cpu_replay):
        _, counts = cpu_replay(family)
        print(f"{family}: merges by branch {counts}")
        assert counts["keep"] > 0 and counts["adopt"] > 0
        assert counts["weighted"] + counts["zero"] > 0

    @pytest.mark.parametrize("family", ["logreg", "mlp"])
    def test_fast_matches_tick_path(self, family):
        data = _sim_data(64, CUDA)
        spec = _e2e_spec(family)
        cfg = _e2e_cfg(spec)
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
        fast.start(n_rounds=E2E_ROUNDS)

        # the per-tick arm: both whole-round routes closed, so every phase
        # goes through _run_tick (HIPBackend.deliver -> tick_logreg/tick_mlp)
        slow = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
        slow._fast_path_ok = lambda: False
        slow._flat_exec_ok = lambda: False
        counted(slow, "slow", "_run_round_fast")
        counted(slow, "slow", "_run_tick")
        slow.init_nodes()
        slow.start(n_rounds=E2E_ROUNDS)
        torch.cuda.synchronize()
        assert calls.get(("fast", "_run_round_fast"), 0) == E2E_ROUNDS
        assert ("fast", "_run_tick") not in calls
        assert ("slow", "_run_round_fast") not in calls
        assert calls.get(("slow", "_run_tick"), 0) > 0
        print(f"fast vs tick err {_err(fast.local_params(), slow.local_params()):.3e}")
        assert torch.allclose(
            fast.local_params(), slow.local_params(), atol=1e-5, rtol=1e-5
        )
        assert torch.equal(fast.state.ages, slow.state.ages)
        assert int(fast.state.ages.max()) > 0

    @pytest.mark.parametrize("family", ["logreg", "mlp"])
    def test_gpu_matches_cpu_run(self, family, cpu_replay):
        cpu_sim, _ = cpu_replay(family)
        spec = _e2e_spec(family)
        sim = BatchedGossipSimulator(
            _e2e_cfg(spec), spec, _sim_data(64, CUDA), device=CUDA
        )
        assert sim.backend.name == "hip"
        sim.init_nodes()
        sim.start(n_rounds=E2E_ROUNDS)
        torch.cuda.synchronize()
        c, g = cpu_sim.local_params(), sim.local_params().cpu()
        print(f"cpu vs gpu err {_err(c, g):.3e}")
        assert torch.allclose(c, g, atol=1e-4, rtol=1e-4)
        assert torch.equal(cpu_sim.state.ages, sim.state.ages.cpu())


# ---------------------------------------------------------------------------
# host checks
# ---------------------------------------------------------------------------

_COOP_CHILD = """
import numpy as np, torch
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedGossipSimulator, DataArena, EngineConfig, LogRegSpec,
)
dev = torch.device("cuda:0")
X, y = make_synthetic_classification((640, 57, 2), seed=0, margin=2.0)
shards = [(X[s], y[s]) for s in np.array_split(np.arange(576), 32)]
data = DataArena.from_shards(shards, dev, global_eval=(X[576:], y[576:]))
spec = LogRegSpec(57, 2, lr=0.1, batch_size=4, age_diff_threshold=1)
cfg = EngineConfig(n_nodes=32, delta=10, protocol=AntiEntropyProtocol.PUSH,
                   model_size=spec.D, sampling_eval=0.0, seed=3)
sim = BatchedGossipSimulator(cfg, spec, data, device=dev)
assert sim._fast_path_ok()
sim.init_nodes()
sim.start(n_rounds=2)
torch.cuda.synchronize()
assert torch.isfinite(sim.local_params()).all()
assert int(sim.state.ages.max()) > 0
print("COOP_LIMITED_OK")
"""


class TestHostChecks:
    def test_family_without_kernel_rejected(self):
        """Pegasos has no limited-merge kernel: _family_call raises before
        any launch, state untouched."""
        spec = PegasosSpec(11)
        spec.age_diff_threshold = 2
        n = 12
        gs = NodeStateArena(n, spec.D, CUDA)
        gs.params.normal_()
        X, y = make_synthetic_classification((48, 11, 2), seed=3)
        shards = [(X[s], 2 * y[s] - 1) for s in np.array_split(np.arange(48), n)]
        gd = DataArena.from_shards(shards, CUDA)
        gpool = SlotPool(spec.D, CUDA, 16)
        before = gs.params.clone()
        with pytest.raises(ValueError, match="limited merge.*pegasos"):
            HIPBackend().deliver(gs, gpool, gd, spec, RECV, PTR, SLOTS, REPLY)
        torch.cuda.synchronize()
        assert torch.equal(before, gs.params)

    def test_merge_limit_validated_by_the_extension(self):
        """The overload itself refuses a threshold below -1."""
        spec = LogRegSpec(5, 3, age_diff_threshold=2)
        cs, gs, cd, gd = _pair(12, spec)
        cpool, gpool = _pools(spec)
        spec.age_diff_threshold = -5
        with pytest.raises(RuntimeError, match="merge_limit"):
            HIPBackend().deliver(gs, gpool, gd, spec, RECV, PTR, SLOTS, REPLY)

    def test_coop_env_with_threshold_still_runs(self):
        """GOSSIPY_COOP=1 selects the cooperative round for plain logreg;
        with a threshold the runner must stay on the stream executor."""
        env = dict(os.environ, GOSSIPY_COOP="1")
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run(
            [sys.executable, "-c", _COOP_CHILD],
            capture_output=True, text=True, timeout=120, cwd=ROOT, env=env,
        )
        assert r.returncode == 0, f"failed:\n{r.stdout}\n{r.stderr}"
        assert "COOP_LIMITED_OK" in r.stdout
