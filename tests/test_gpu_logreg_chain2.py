"""GPU tests (MI355X) for the pipelined forward loop of the logreg tick
(``dot_chain``: two register sets, an exact-length tail), the exact-length
batch reductions (``col_chain``) and the register path of the dLoss/dz stage
for two classes, against the float64 reference of ``ref64.py`` at the 1e-4 of
``tick_cases.py``. Feature counts sit on the chunk boundaries of the loop
(8 per chunk, two chunks per trip), class counts take the two-class path and
the generic one, shards have 0, 1, 5 and 32 rows, receiver rows 1, 2 and 5
deliveries with reply snapshots between them. The snapshot op, whose
kernel is unchanged and which the round driver's ``eval_overlap`` option
also uses as a gather without ages, is compared with torch indexing,
exactly. All marked ``gpu``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

import tick_cases as tc
from gossipy_amd import ops
from gossipy_amd.engine import LogRegSpec
from gossipy_amd.engine.backend import HIPBackend

CUDA = torch.device("cuda:0")
TOL = 1e-4  # as tick_cases.py: the fp32 oracle itself is within TOL / 8

DS = (1, 2, 7, 8, 9, 15, 16, 17, 24, 25, 57)
KS = (2, 3, 16)
# node -> shard rows; the 32-row node is exactly one batch
SHARDS = [0, 1, 5, 32]
# receiver rows of 5, 1, 2 and 1 deliveries; reply snapshots after the first
# and the fourth delivery of the long row and after the zero-row node's only
ROWS = [(3, 5, (0, 3)), (0, 1, (0,)), (1, 2, ()), (2, 1, ())]


def _case(name, spec, shards=SHARDS, rows=ROWS, seed=1):
    return tc.Case(name, spec, list(shards), TOL, rows=rows, seed=seed)


def _check(case):
    ref = tc.run_ref(case)
    state, data, pool = tc.build(case, CUDA)
    nd = tc.n_deliveries(case)
    sent = pool.slots[:nd].clone()
    tc.run_backend(HIPBackend(), case, state, data, pool)
    torch.cuda.synchronize()
    dev = tc.deviation(case, ref, state, pool)
    print(f"dev {case.name} {dev:.3e} tol {case.tol:.1e}")
    assert dev <= case.tol, (case.name, dev)
    assert torch.equal(sent, pool.slots[:nd])  # delivered slots are only read


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("d", DS)
def test_forward_chunks_and_class_paths(d, k):
    spec = LogRegSpec(d_in=d, n_classes=k, lr=0.1, batch_size=32)
    _check(_case(f"d{d}_k{k}", spec, seed=100 * k + d))


@pytest.mark.parametrize("mode", ["merge_update", "update", "update_merge"])
@pytest.mark.parametrize("d,k", [(57, 2), (17, 3)])
def test_modes(mode, d, k):
    spec = LogRegSpec(d_in=d, n_classes=k, lr=0.1, batch_size=32,
                      mode=tc.MODES[mode])
    _check(_case(f"{mode}_d{d}_k{k}", spec, seed=7))


def test_limited_merge():
    spec = LogRegSpec(d_in=57, n_classes=2, lr=0.1, batch_size=32,
                      age_diff_threshold=2)
    _check(_case("limited", spec, seed=8))


def test_batch_above_128_rows():
    # one batch of 130 rows: the per-sample stage strides over the batch
    spec = LogRegSpec(d_in=17, n_classes=2, lr=0.1, batch_size=0)
    _check(_case("big", spec, shards=[130, 5, 1],
                 rows=[(0, 2, (0,)), (1, 1, ()), (2, 1, ())], seed=9))


@pytest.mark.parametrize("k,limit", [(2, None), (3, None), (2, 2)])
def test_wide_launch_equals_thin_launches(k, limit):
    # The host runs the pipelined instantiation for launches of at most one
    # wave per SIMD and the plain one above. Both do the same arithmetic in
    # the same order, so one launch above the threshold must leave exactly
    # what the same rows leave in two launches below it, and both must meet
    # the reference.
    prop = torch.cuda.get_device_properties(0)
    thin = prop.multi_processor_count * 4 // 2  # 128 threads = 2 waves
    n = thin + 88
    kw = {} if limit is None else {"age_diff_threshold": limit}
    spec = LogRegSpec(d_in=9, n_classes=k, lr=0.1, batch_size=32, **kw)
    rows = [(i, 1 + i % 3, (0,) if i % 5 == 0 else ()) for i in range(n)]
    case = tc.Case(f"wide_k{k}", spec, [i % 6 for i in range(n)], TOL,
                   rows=rows, update=False, seed=11)
    recv, ptr, slots, reply, pids, _ = tc.events(case)
    assert len(recv) > thin and len(recv) - n // 2 <= thin
    one = tc.build(case, CUDA)
    two = tc.build(case, CUDA)
    HIPBackend().deliver(one[0], one[2], one[1], spec, recv, ptr, slots,
                         reply, pids)
    h = n // 2
    for r0, r1 in ((0, h), (h, n)):
        j0, j1 = int(ptr[r0]), int(ptr[r1])
        HIPBackend().deliver(two[0], two[2], two[1], spec, recv[r0:r1],
                             ptr[r0:r1 + 1] - j0, slots[j0:j1],
                             reply[j0:j1], pids)
    torch.cuda.synchronize()
    assert torch.equal(one[0].params, two[0].params)
    assert torch.equal(one[0].ages, two[0].ages)
    assert torch.equal(one[2].slots, two[2].slots)
    assert torch.equal(one[2].slot_ages, two[2].slot_ages)
    dev = tc.deviation(case, tc.run_ref(case), one[0], one[2])
    print(f"dev {case.name} {dev:.3e} tol {case.tol:.1e}")
    assert dev <= case.tol, (case.name, dev)


@pytest.mark.parametrize("aw", [0, 1])
@pytest.mark.parametrize("src_off", [0, 2, 4])
@pytest.mark.parametrize("W", [1, 3, 4, 116, 130])
def test_snapshot_small(W, src_off, aw):
    _snapshot(5, W, src_off, aw)
    _snapshot(1, W, src_off, aw)


def test_snapshot_strided_rows():
    # 5000 rows of 116 floats: more than the grid covers in one pass
    _snapshot(5000, 116, 0, 1)


def _snapshot(n, W, src_off, aw):
    g = torch.Generator().manual_seed(n + W + src_off)
    n_nodes, cap = n + 3, n + 5
    Dp = W + src_off + (4 if src_off else 0)  # a row wider than the slot
    params = torch.randn(n_nodes, Dp, generator=g).to(CUDA)
    ages = torch.randint(0, 99, (n_nodes,), generator=g,
                         dtype=torch.int32).to(CUDA)
    slots = torch.full((cap, W), -7.0, device=CUDA)
    slot_ages = torch.full((cap,), -7, dtype=torch.int32, device=CUDA)
    nodes = torch.randint(0, n_nodes, (n,), generator=g)
    slot_ids = torch.randperm(cap, generator=g)[:n]
    ops.load_extension().snapshot(
        params, ages, slots, slot_ages, nodes.to(torch.int32).to(CUDA),
        slot_ids.to(torch.int32).to(CUDA), aw, src_off)
    torch.cuda.synchronize()
    want = torch.full((cap, W), -7.0)
    want[slot_ids] = params.cpu()[nodes, src_off:src_off + W]
    want_ages = torch.full((cap,), -7, dtype=torch.int32)
    if aw:
        want_ages[slot_ids] = ages.cpu()[nodes]
    assert torch.equal(slots.cpu(), want)
    assert torch.equal(slot_ages.cpu(), want_ages)
