"""GPU tests (MI355X) for the native round driver (``RoundDriver`` in the
HIP extension): a simulator that runs its rounds through the driver must
leave exactly what the Python round path (``GOSSIPY_NO_ROUND_DRIVER=1``)
leaves from the same seed: parameters, ages, the slot pool, the report's
evaluations with their timestamps, and the message counters. Small odd
shapes: 64 nodes, 8 ticks, d=5, shards of 3 to 9 samples against a batch of
4 (partial batches), 33 eval samples. All marked ``gpu``."""

import gc

import pytest
import torch

pytestmark = pytest.mark.gpu

from gossipy_amd.core import AntiEntropyProtocol, UniformDelay
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
    PegasosSpec,
    SlotPool,
)
from gossipy_amd.simul import SimulationReport

CUDA = torch.device("cuda:0")
N, DELTA, D_IN, N_EVAL, ROUNDS = 64, 8, 5, 33, 6


def _data(pm1=False):
    g = torch.Generator().manual_seed(11)
    sizes = [3 + (5 * i) % 7 for i in range(N)]
    # one partial batch, a full and a partial one, two full and a partial
    assert min(sizes) == 3 and max(sizes) == 9 and set(sizes) == set(range(3, 10))
    w = torch.randn(D_IN, generator=g)

    def draw(n):
        X = torch.randn(n, D_IN, generator=g)
        y = ((X @ w) > 0).float()
        return X, (2 * y - 1 if pm1 else y)

    return DataArena.from_shards(
        [draw(n) for n in sizes], CUDA, global_eval=draw(N_EVAL)
    )


def _spec(**kw):
    return LogRegSpec(d_in=D_IN, n_classes=2, lr=0.1, batch_size=4, **kw)


def _cfg(spec, **kw):
    kw.setdefault("protocol", AntiEntropyProtocol.PUSH)
    kw.setdefault("sampling_eval", 0.1)
    return EngineConfig(n_nodes=N, delta=DELTA, model_size=spec.D, seed=5, **kw)


def _sim(cfg, spec, data, pool_capacity=None):
    sim = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes(seed=3)
    if pool_capacity is not None:
        sim.pool = SlotPool(spec.D, CUDA, capacity=pool_capacity)
    return sim, rep


def _run(sim, n, driver, monkeypatch):
    if driver:
        monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    else:
        monkeypatch.setenv("GOSSIPY_NO_ROUND_DRIVER", "1")
    sim.start(n_rounds=n)


def _used_driver(sim):
    return getattr(sim, "_rd", None) is not None


def _assert_same(a, rep_a, b, rep_b):
    torch.cuda.synchronize()
    assert a.rounds_done == b.rounds_done
    assert torch.equal(a.state.params, b.state.params)
    assert torch.equal(a.state.ages, b.state.ages)
    assert torch.equal(a.pool.slots, b.pool.slots)
    assert torch.equal(a.pool.slot_ages, b.pool.slot_ages)
    assert rep_a.get_evaluation(False) == rep_b.get_evaluation(False)
    assert [t for t, _ in rep_a.get_evaluation(False)] == sorted(
        t for t, _ in rep_a.get_evaluation(False))
    assert (rep_a._sent_messages, rep_a._failed_messages, rep_a._total_size) == (
        rep_b._sent_messages, rep_b._failed_messages, rep_b._total_size)
    assert rep_a._sent_messages > 0


CASES = {
    "push_sync": (dict(), dict()),
    "push_pull_uniform": (
        dict(protocol=AntiEntropyProtocol.PUSH_PULL, delay=UniformDelay(1, 5)),
        dict(),
    ),
    "faults": (dict(drop_prob=0.3, online_prob=0.7), dict()),
    "limited_merge": (dict(), dict(age_diff_threshold=2)),
    "eval_every_node": (dict(sampling_eval=0.0), dict()),
    "eval_duplicate_draws": (dict(sampling_eval=0.5), dict()),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_driver_equals_python_path(name, monkeypatch):
    cfg_kw, spec_kw = CASES[name]
    spec = _spec(**spec_kw)
    cfg, data = _cfg(spec, **cfg_kw), _data()
    a, rep_a = _sim(cfg, spec, data)
    b, rep_b = _sim(cfg, spec, data)
    _run(a, ROUNDS, True, monkeypatch)
    _run(b, ROUNDS, False, monkeypatch)
    assert _used_driver(a) and not _used_driver(b)
    _assert_same(a, rep_a, b, rep_b)
    evs = rep_a.get_evaluation(False)
    assert [t for t, _ in evs] == [(r + 1) * DELTA - 1 for r in range(ROUNDS)]


@pytest.mark.parametrize(
    "off", ["GOSSIPY_RD_NO_MAPPED_EVAL", "GOSSIPY_RD_NO_SIDE_UPLOAD"]
)
def test_driver_options_off(off, monkeypatch):
    # the copied-out metrics and the same-stream upload stay selectable
    monkeypatch.setenv(off, "1")
    spec = _spec()
    cfg = _cfg(spec, protocol=AntiEntropyProtocol.PUSH_PULL,
               delay=UniformDelay(1, 5), sampling_eval=0.5)
    data = _data()
    a, rep_a = _sim(cfg, spec, data)
    b, rep_b = _sim(cfg, spec, data)
    _run(a, ROUNDS, True, monkeypatch)
    _run(b, ROUNDS, False, monkeypatch)
    assert _used_driver(a) and not _used_driver(b)
    _assert_same(a, rep_a, b, rep_b)


def test_pegasos_through_the_linear_plan(monkeypatch):
    spec = PegasosSpec(d_in=D_IN)
    cfg, data = _cfg(spec), _data(pm1=True)
    a, rep_a = _sim(cfg, spec, data)
    b, rep_b = _sim(cfg, spec, data)
    _run(a, ROUNDS, True, monkeypatch)
    _run(b, ROUNDS, False, monkeypatch)
    assert _used_driver(a) and not _used_driver(b)
    _assert_same(a, rep_a, b, rep_b)


def test_small_pool_grows_through_the_retry(monkeypatch):
    # 8 slots: round 0 already needs 106, and replies in flight push the
    # demand past twice the capacity again in rounds 1, 2 and 3 (231, 361,
    # 484 slots), so the held-round retry and set_pool run four times
    spec = _spec()
    cfg = _cfg(spec, protocol=AntiEntropyProtocol.PUSH_PULL,
               delay=UniformDelay(1, 5))
    data = _data()
    a, rep_a = _sim(cfg, spec, data, pool_capacity=8)
    b, rep_b = _sim(cfg, spec, data, pool_capacity=8)
    caps = []
    ensure = a.pool.ensure

    def spy(n):
        # the driver path calls ensure only from the retry (step held the
        # round and asked for n slots)
        before = a.pool.slots.shape[0]
        assert n > before
        ensure(n)
        caps.append((a.rounds_done, a.pool.slots.shape[0]))

    a.pool.ensure = spy
    _run(a, ROUNDS, True, monkeypatch)
    _run(b, ROUNDS, False, monkeypatch)
    assert _used_driver(a)
    assert [r for r, _ in caps] == [0, 1, 2, 3], caps
    assert caps[0][1] > 8 and caps[-1][1] == a.pool.slots.shape[0]
    _assert_same(a, rep_a, b, rep_b)


def test_split_start_equals_one_start(monkeypatch):
    spec = _spec()
    cfg = _cfg(spec, protocol=AntiEntropyProtocol.PUSH_PULL,
               delay=UniformDelay(1, 5))
    data = _data()
    a, rep_a = _sim(cfg, spec, data)
    b, rep_b = _sim(cfg, spec, data)
    _run(a, 3, True, monkeypatch)
    assert len(rep_a.get_evaluation(False)) == 3  # drained at the boundary
    _run(a, 3, True, monkeypatch)
    _run(b, ROUNDS, True, monkeypatch)
    _assert_same(a, rep_a, b, rep_b)


def test_save_load_midway(tmp_path, monkeypatch):
    spec = _spec()
    cfg = _cfg(spec, protocol=AntiEntropyProtocol.PUSH_PULL,
               delay=UniformDelay(1, 5))
    data = _data()
    a, rep_a = _sim(cfg, spec, data)
    b, rep_b = _sim(cfg, spec, data)
    _run(a, 3, True, monkeypatch)
    ck = str(tmp_path / "ck.dill")
    a.save(ck)
    a2 = BatchedGossipSimulator.load(ck, device=CUDA)
    a2.add_receiver(rep_a)
    _run(a2, 3, True, monkeypatch)
    _run(b, ROUNDS, True, monkeypatch)
    assert _used_driver(a2)
    _assert_same(a2, rep_a, b, rep_b)


@pytest.mark.parametrize("first", [True, False], ids=["driver_then_python",
                                                      "python_then_driver"])
def test_switching_paths_on_one_simulator(first, monkeypatch):
    spec = _spec()
    cfg = _cfg(spec, protocol=AntiEntropyProtocol.PUSH_PULL,
               delay=UniformDelay(1, 5))
    data = _data()
    a, rep_a = _sim(cfg, spec, data)
    b, rep_b = _sim(cfg, spec, data)
    _run(a, 3, first, monkeypatch)
    _run(a, 3, not first, monkeypatch)
    _run(b, ROUNDS, False, monkeypatch)
    assert _used_driver(a)
    _assert_same(a, rep_a, b, rep_b)


def test_out_of_order_step_raises_and_enqueues_nothing(monkeypatch):
    spec = _spec()
    a, _ = _sim(_cfg(spec), spec, _data())
    _run(a, 1, True, monkeypatch)
    torch.cuda.synchronize()
    before = a.state.params.clone()
    with pytest.raises(ValueError):
        a._rd.step(5)
    torch.cuda.synchronize()
    assert torch.equal(a.state.params, before)
    _run(a, 1, True, monkeypatch)  # the refused request consumed nothing
    assert a.rounds_done == 2


def test_set_pool_rejects_a_pool_the_plan_cannot_write(monkeypatch):
    spec = _spec()
    a, _ = _sim(_cfg(spec), spec, _data())
    _run(a, 1, True, monkeypatch)
    ages = torch.zeros(16, device=CUDA, dtype=torch.int32)
    ok = torch.zeros(16, spec.D, device=CUDA)
    for slots, slot_ages in (
        (torch.zeros(16, spec.D - 1, device=CUDA), ages),  # narrower rows
        (torch.zeros(16, spec.D + 1, device=CUDA), ages),
        (ok, ages[:8]),                                    # fewer ages
        (ok, ages.to(torch.int64)),
        (ok.cpu(), ages),
    ):
        with pytest.raises(RuntimeError):
            a._rd.set_pool(slots, slot_ages)
    _run(a, 1, True, monkeypatch)  # the driver kept its pool
    assert a.rounds_done == 2


def _tiny_round():
    """8 nodes, a pool of 8 slots, one group: node 2 snapshots into slot 3,
    node 5 receives it. Returns a fresh simulator and the round's flat
    dict."""
    import numpy as np

    n = 8
    g = torch.Generator().manual_seed(4)
    shards = [
        (torch.randn(3 + i % 4, D_IN, generator=g),
         torch.randint(0, 2, (3 + i % 4,), generator=g).float())
        for i in range(n)
    ]
    spec = _spec()
    cfg = EngineConfig(n_nodes=n, delta=4, model_size=spec.D, seed=5,
                       protocol=AntiEntropyProtocol.PUSH)
    sim = BatchedGossipSimulator(
        cfg, spec, DataArena.from_shards(shards, CUDA), device=CUDA)
    sim.init_nodes(seed=3)
    sim.pool = SlotPool(spec.D, CUDA, capacity=8)
    i32 = lambda *v: np.array(v, np.int32)
    flat = {
        "snap_nodes": i32(2), "snap_slots": i32(3), "snap_tptr": i32(0, 1),
        "recv_nodes": i32(5), "recv_nptr": i32(0, 1), "recv_tptr": i32(0, 1),
        "del_slots": i32(3), "reply_slots": i32(-1),
        "pull_tptr": i32(0, 0), "rep_nptr": i32(0), "rep_tptr": i32(0, 0),
    }
    return sim, flat


def test_run_round_takes_the_upload_and_refuses_a_bad_one():
    """``run_round_*`` take the one upload buffer, its lengths and the four
    tick pointers. A direct call leaves what ``_run_round_fast`` leaves from
    the same flat dict; a buffer, lengths or tick pointers that do not fit
    together raise before anything is launched."""
    import numpy as np

    from gossipy_amd import ops

    ext = ops.load_extension()
    a, flat = _tiny_round()
    b, _ = _tiny_round()
    start = b.state.params.clone()
    a._run_round_fast(flat)

    empty = np.zeros(0, np.int32)
    parts = [flat.get(n, empty) for n in ext.ROUND_ARRAY_NAMES]
    lens = [len(p) for p in parts]
    assert sum(lens) == 8 and lens[-1] == 0
    buf = torch.from_numpy(np.concatenate(parts)).to(CUDA)
    tptr = [torch.from_numpy(flat[n]) for n in ext.ROUND_TPTR_NAMES]
    name, args, _ = b.backend._family_call(b.spec, CUDA)
    assert name == "logreg"

    def call(buf, lens, tptr):
        ext.run_round_logreg(
            b.state.params, b.state.ages, b.pool.slots, b.pool.slot_ages,
            buf, lens, *tptr, b.data.x, b.data.y, b.data.counts, *args)

    def state():
        torch.cuda.synchronize()
        return [t.clone() for t in (b.state.params, b.state.ages,
                                    b.pool.slots, b.pool.slot_ages)]

    # every bad call changes the last array only (rep_reply_slots, which a
    # round without replies never reads) or a tick pointer's tail
    before = state()
    bad = {
        "lens one short": (buf, lens[:-1], tptr),
        "negative length": (buf, lens[:-1] + [-1], tptr),
        "lens past the buffer": (buf, lens[:-1] + [1], tptr),
        "lens far past the buffer": (buf, lens[:-1] + [2 ** 62], tptr),
        "host buffer": (buf.cpu(), lens, tptr),
        "unequal tick pointers": (
            buf, lens, tptr[:-1] + [torch.zeros(3, dtype=torch.int32)]),
        "empty tick pointers": (
            buf, lens, [torch.zeros(0, dtype=torch.int32)] * 4),
    }
    for what, (bb, ll, tt) in bad.items():
        with pytest.raises(RuntimeError):
            call(bb, ll, tt)
        for x, y in zip(before, state()):
            assert torch.equal(x, y), what

    call(buf, lens, tptr)
    torch.cuda.synchronize()
    assert not torch.equal(b.state.params, start)  # node 5 merged and trained
    assert torch.equal(b.state.params[:5], start[:5])
    assert torch.equal(a.state.params, b.state.params)
    assert torch.equal(a.state.ages, b.state.ages)
    assert torch.equal(a.pool.slots, b.pool.slots)
    assert torch.equal(a.pool.slot_ages, b.pool.slot_ages)


def test_construct_destroy_twenty(monkeypatch):
    spec = _spec()
    cfg, data = _cfg(spec, sampling_eval=0.5), _data()
    monkeypatch.delenv("GOSSIPY_NO_ROUND_DRIVER", raising=False)
    from gossipy_amd import ops

    # (pinned host buffers, device buffers, events, streams) the drivers of
    # this process hold, counted where they are allocated and freed
    live = ops.load_extension().round_driver_live
    gc.collect()
    base = live()
    for i in range(20):
        sim, rep = _sim(cfg, spec, data)
        sim.start(n_rounds=i % 3)  # 0 rounds: buffers never allocated
        assert _used_driver(sim)
        assert len(rep.get_evaluation(False)) == i % 3
        held = live()
        # ring events + staging events + upload event, and the side stream
        assert held[2] - base[2] == 4 + 2 + 1 and held[3] - base[3] == 1
        if i % 3:
            assert held[0] > base[0] and held[1] > base[1]
        del sim, rep
        gc.collect()
        assert live() == base
