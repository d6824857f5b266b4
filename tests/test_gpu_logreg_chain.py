"""GPU tests (MI355X) for the logreg tick's batched-read loops: the forward
pass spread over (sample, class) pairs, the chunked staging and the SGD
reductions, against the fp32 torch oracle. Shapes sit on the loops' block
boundaries: feature counts around the read block of 8, more (sample, class)
pairs than threads, shards of 0 / 1 / exactly one batch / three batches with
a short last one, receiver rows of 1, 2 and 5 deliveries with reply
snapshots in between. All marked ``gpu``."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gossipy_amd.core import CreateModelMode
from gossipy_amd.engine import DataArena, LogRegSpec, NodeStateArena, SlotPool
from gossipy_amd.engine.backend import HIPBackend, TorchBackend

CUDA = torch.device("cuda:0")
CPU = torch.device("cpu")
TOL = 1e-4  # atol = rtol, as TestKernelNumerics in tests/test_gpu.py

# one launch: node -> shard size. 0 = nothing to train on, 1 = one sample,
# 32 = exactly one batch of 32, 70 = three batches, the last of 6 (the batch
# buffer must be restaged for every delivery), the rest odd sizes
SHARDS = [0, 1, 32, 70, 5, 33, 4, 12]
# receiver rows of 5, 2, 1, 2 and 1 deliveries; replies asked for by the
# first and fourth delivery of the long row, and in the zero-sample row
RECV = torch.tensor([3, 0, 1, 2, 5], dtype=torch.int64)
PTR = torch.tensor([0, 5, 7, 8, 10, 11], dtype=torch.int64)
SLOTS = torch.arange(11, dtype=torch.int64)
REPLY = torch.tensor(
    [11, -1, -1, 12, -1, 13, -1, -1, -1, 14, 15], dtype=torch.int64
)
POOL_CAP = 16
MODES = [
    CreateModelMode.MERGE_UPDATE,
    CreateModelMode.UPDATE,
    CreateModelMode.UPDATE_MERGE,
    CreateModelMode.PASS,
]


def make_inputs(spec, seed=0):
    """CPU state, data and slot pool for ``spec`` on the SHARDS layout."""
    g = torch.Generator().manual_seed(seed)
    n, d, k = len(SHARDS), spec.d_in, spec.n_classes
    state = NodeStateArena(n, spec.D, CPU)
    state.params.copy_(torch.randn(n, spec.D, generator=g) * 0.3)
    state.ages.copy_(torch.arange(n, dtype=torch.int32) % 5)
    shards = []
    for c in SHARDS:
        shards.append((
            torch.randn(c, d, generator=g),
            torch.randint(0, k, (c,), generator=g).float(),
        ))
    data = DataArena.from_shards(shards, CPU)
    pool = SlotPool(spec.D, CPU, POOL_CAP)
    pool.slots.copy_(torch.randn(POOL_CAP, spec.D, generator=g) * 0.3)
    pool.slot_ages.copy_(torch.arange(POOL_CAP, dtype=torch.int32) * 2 % 7)
    return state, data, pool


def to_gpu(spec, state, data, pool):
    gs = NodeStateArena(state.params.shape[0], spec.D, CUDA)
    gs.params.copy_(state.params)
    gs.ages.copy_(state.ages)
    gd = DataArena(data.x.to(CUDA), data.y.to(CUDA), data.counts.to(CUDA))
    gp = SlotPool(spec.D, CUDA, POOL_CAP)
    gp.slots.copy_(pool.slots)
    gp.slot_ages.copy_(pool.slot_ages)
    return gs, gd, gp


def oracle_deliver(spec, state, data, pool):
    TorchBackend().deliver(state, pool, data, spec, RECV, PTR, SLOTS, REPLY)


def _close(a, b):
    return torch.allclose(a.cpu(), b.cpu(), atol=TOL, rtol=TOL)


def _deliver_both(spec, seed=0):
    cs, cd, cp = make_inputs(spec, seed)
    gs, gd, gp = to_gpu(spec, cs, cd, cp)
    sent = cp.slots[:11].clone()
    oracle_deliver(spec, cs, cd, cp)
    HIPBackend().deliver(gs, gp, gd, spec, RECV, PTR, SLOTS, REPLY)
    torch.cuda.synchronize()
    assert _close(cs.params, gs.params), float(
        (cs.params - gs.params.cpu()).abs().max())
    assert torch.equal(cs.ages, gs.ages.cpu())
    # every reply snapshot holds the row as it stood right after ITS
    # delivery, not after the receiver's last one
    assert _close(cp.slots[11:16], gp.slots[11:16])
    assert torch.equal(cp.slot_ages[11:16], gp.slot_ages[11:16].cpu())
    # the kernel only reads the delivered slots (the oracle may train a
    # received model in place, so the comparison is with the input)
    assert torch.equal(sent, gp.slots[:11].cpu())


SPECS = {
    # feature counts around the read block of 8, and its tail
    **{
        f"d{d}": LogRegSpec(d_in=d, n_classes=2, lr=0.1, batch_size=32)
        for d in (1, 7, 8, 9, 57)
    },
    # class counts: k = 16 has 32 * 16 = 512 (sample, class) pairs
    **{
        f"k{k}": LogRegSpec(d_in=9, n_classes=k, lr=0.1, batch_size=32)
        for k in (3, 16)
    },
    "k16_d57": LogRegSpec(d_in=57, n_classes=16, lr=0.1, batch_size=32),
    "full_batch": LogRegSpec(d_in=57, n_classes=2, lr=0.1, batch_size=0),
    "epochs2": LogRegSpec(
        d_in=57, n_classes=2, lr=0.1, batch_size=32, local_epochs=2
    ),
    "weight_decay": LogRegSpec(
        d_in=57, n_classes=3, lr=0.1, batch_size=32, weight_decay=0.05
    ),
    "limited_merge": LogRegSpec(
        d_in=57, n_classes=2, lr=0.1, batch_size=32, age_diff_threshold=2
    ),
}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_deliver_matches_oracle(name):
    _deliver_both(SPECS[name], seed=sorted(SPECS).index(name))


@pytest.mark.parametrize("mode", MODES, ids=[m.name for m in MODES])
@pytest.mark.parametrize("k", [2, 16])
def test_modes_match_oracle(mode, k):
    spec = LogRegSpec(d_in=9, n_classes=k, lr=0.1, batch_size=32, mode=mode)
    _deliver_both(spec, seed=20 + k)


@pytest.mark.parametrize("mode", MODES[:3], ids=[m.name for m in MODES[:3]])
def test_limited_merge_modes(mode):
    spec = LogRegSpec(
        d_in=57, n_classes=2, lr=0.1, batch_size=32, mode=mode,
        age_diff_threshold=1,
    )
    _deliver_both(spec, seed=40)


@pytest.mark.parametrize("name", ["d9", "k16_d57", "full_batch", "epochs2"])
def test_update_only(name):
    spec = SPECS[name]
    cs, cd, cp = make_inputs(spec, seed=50)
    gs, gd, _ = to_gpu(spec, cs, cd, cp)
    nodes = torch.arange(len(SHARDS))
    TorchBackend().update(cs, cd, spec, nodes)
    HIPBackend().update(gs, gd, spec, nodes)
    torch.cuda.synchronize()
    assert _close(cs.params, gs.params)
    assert torch.equal(cs.ages, gs.ages.cpu())


def test_reply_between_deliveries_differs_from_final():
    # guards the check above: in the oracle itself the long row's two reply
    # snapshots differ from each other and from the row's final state
    spec = SPECS["d57"]
    cs, cd, cp = make_inputs(spec, 0)
    oracle_deliver(spec, cs, cd, cp)
    assert not np.allclose(cp.slots[11], cp.slots[12], atol=1e-3)
    assert not np.allclose(cp.slots[12], cs.params[3], atol=1e-3)
