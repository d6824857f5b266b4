"""GPU tests (MI355X): the HIP tick kernels and the fused evaluation kernel
against the float64 numpy reference (``ref64.py``) on the cases of
``tick_cases.py``: batches with more rows than the block has threads, the
MFMA K-loop's padded buckets and its dynamic loop, ragged MFMA tiles, logreg
rows wider than the 1024 prefetched floats, limited merge, every mode, and
integer-valued evaluation sets whose metrics are exact. Each case's bound is
the literal ``tol`` of the table, which ``test_ref64.py`` ties to the fp32
oracle's own deviation from the reference. All marked ``gpu``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import tick_cases as tc
from gossipy_amd import ops
from gossipy_amd.engine import DataArena, LogRegSpec, NodeStateArena, SlotPool
from gossipy_amd.engine.backend import HIPBackend, TorchBackend

CUDA = torch.device("cuda:0")
CPU = torch.device("cpu")
KEYS = ("accuracy", "precision", "recall", "f1_score", "auc")
_REF = {}


def reference(name):
    """The case's reference result, computed once and only read."""
    if name not in _REF:
        _REF[name] = tc.run_ref(tc.BY_NAME[name])
    return _REF[name]


@pytest.mark.parametrize("name", [c.name for c in tc.CASES])
def test_tick_matches_reference(name):
    case = tc.BY_NAME[name]
    state, data, pool = tc.build(case, CUDA)
    nd = tc.n_deliveries(case)
    sent = pool.slots[:nd].clone()
    sent_ages = pool.slot_ages[:nd].clone()
    tc.run_backend(HIPBackend(), case, state, data, pool)
    torch.cuda.synchronize()
    dev = tc.deviation(case, reference(name), state, pool)
    print(f"dev {name} {dev:.3e} tol {case.tol:.1e}")
    assert dev <= case.tol, (name, dev)
    # the kernels only read the delivered slots
    assert torch.equal(sent, pool.slots[:nd])
    assert torch.equal(sent_ages, pool.slot_ages[:nd])


def test_sampled_logreg_130_rows():
    # the sampling draws are not part of the float64 reference: the fp32
    # oracle at the bound of the sampled fuzz (tests/test_fuzz_gpu.py)
    spec = LogRegSpec(d_in=9, n_classes=2, lr=0.1, batch_size=0,
                      sample_size=0.3)
    g = torch.Generator().manual_seed(9)
    counts = [130, 129, 64]
    shards = [(torch.randn(c, 9, generator=g),
               torch.randint(0, 2, (c,), generator=g).float())
              for c in counts]
    cd = DataArena.from_shards(shards, CPU)
    gd = DataArena(cd.x.to(CUDA), cd.y.to(CUDA), cd.counts.to(CUDA))
    cs, gs = NodeStateArena(3, spec.D, CPU), NodeStateArena(3, spec.D, CUDA)
    cs.params.copy_(torch.randn(3, spec.D, generator=g) * 0.3)
    gs.params.copy_(cs.params)
    cp, gp = SlotPool(spec.D, CPU, 6), SlotPool(spec.D, CUDA, 6)
    cp.slots.copy_(torch.randn(6, spec.D, generator=g) * 0.3)
    cp.slot_ages.copy_(torch.arange(6, dtype=torch.int32))
    gp.slots.copy_(cp.slots)
    gp.slot_ages.copy_(cp.slot_ages)
    recv, ptr = torch.tensor([0, 1, 2]), torch.tensor([0, 2, 3, 4])
    slots = torch.arange(4)
    reply = torch.tensor([4, -1, 5, -1])
    seeds = torch.tensor([123456, 777, 2**30 + 5, 42])
    for backend, (s, d, p) in ((TorchBackend(), (cs, cd, cp)),
                               (HIPBackend(), (gs, gd, gp))):
        backend.update(s, d, spec, torch.arange(3))
        backend.deliver(s, p, d, spec, recv, ptr, slots, reply, seeds)
    torch.cuda.synchronize()
    assert torch.allclose(cs.params, gs.params.cpu(), atol=2e-3, rtol=2e-3)
    assert torch.allclose(cp.slots[4:], gp.slots[4:].cpu(), atol=2e-3,
                          rtol=2e-3)
    assert torch.equal(cs.ages, gs.ages.cpu())
    assert torch.equal(cp.slot_ages[4:], gp.slot_ages[4:].cpu())


# ---- evaluation kernel ------------------------------------------------------------

EVAL = {c.name: c for c in tc.eval_cases()}


def _same(want, got, name):
    assert set(want) == set(got), (name, want, got)
    for key in want:
        assert abs(want[key] - got[key]) <= tc.EVAL_TOL, (
            name, key, want[key], got[key])


def _state(case):
    gs = NodeStateArena(case.params.shape[0], case.spec.D, CUDA)
    gs.params.copy_(case.params)
    return gs


@pytest.mark.parametrize("name", sorted(EVAL))
def test_eval_kernel_matches_reference(name):
    case = EVAL[name]
    R = case.params.shape[0]
    got = HIPBackend().eval_metrics_fast(
        _state(case), case.spec, torch.arange(R), case.X.to(CUDA),
        case.y.to(CUDA))
    assert len(got) == R
    for r in range(R):
        _same(tc.eval_reference(case, case.params[r]), got[r], name)
    if "zero_model" in name or "all_ties" in name or "all_label" in name:
        assert all(g["auc"] == 0.5 for g in got)


@pytest.mark.parametrize("name", ["eval_repeats_n257", "eval_zero_model_n257"])
def test_eval_per_node_shards(name):
    # counts 0, 1, the full stride and 37: node i scores rows of its own
    # shard only, and the empty shard's row is dropped
    base = EVAL[name]
    stride = 64
    counts = [0, 1, stride, 37]
    g = torch.Generator().manual_seed(11)
    d = base.spec.d_in
    tx = torch.randint(-2, 3, (4, stride, d), generator=g).float()
    ty = torch.randint(0, 2, (4, stride), generator=g).float()
    params = base.params[[0, 1, 2, 0]].clone()
    params[3] = -params[3]
    gs = NodeStateArena(4, base.spec.D, CUDA)
    gs.params.copy_(params)
    got = HIPBackend().eval_local_fast(
        gs, base.spec, torch.arange(4), tx.to(CUDA), ty.to(CUDA),
        torch.tensor(counts, dtype=torch.int32, device=CUDA))
    kept = [i for i, c in enumerate(counts) if c]
    assert len(got) == len(kept)
    for res, i in zip(got, kept):
        c = counts[i]
        _same(tc.eval_reference(base, params[i], tx[i, :c], ty[i, :c]), res,
              (name, i))


@pytest.mark.parametrize("name", [
    "eval_zero_model_n257", "eval_repeats_n65", "eval_repeats_n700",
    "eval_2048_all_ties", "eval_2048_all_distinct", "eval_k3_missing_classes",
    "eval_margin_n257",
])
def test_eval_precomputed_scores(name):
    import ref64

    case = EVAL[name]
    spec, R = case.spec, case.params.shape[0]
    ext = ops.load_extension()
    if spec.family == "logreg":
        sc = torch.stack([
            torch.from_numpy(ref64.logreg_scores(
                case.params[r].numpy(), case.X.numpy(), spec.d_in,
                spec.n_classes)).float()
            for r in range(R)
        ])  # integers: the cast is exact
        out = ext.eval_metrics_scores(
            sc.to(CUDA).contiguous(), case.y.to(CUDA), spec.n_classes, False)
    else:
        sc = case.params @ case.X.t()
        out = ext.eval_metrics_scores(
            sc.to(CUDA).contiguous(), case.y.to(CUDA), 1, True)
    rows = out.cpu().numpy()
    for r in range(R):
        got = {k: float(v) for k, v in zip(KEYS, rows[r]) if v >= 0}
        _same(tc.eval_reference(case, case.params[r]), got, name)
