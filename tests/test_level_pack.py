"""The scheduler's level packer (csrc/round_levels.h): launches ordered by
dependency level compute what the flat schedule computes, in as many
launches as the round's critical path is long.

The check is symbolic: a node's state is a hash of its previous state and
the slot content it merged, a slot's content is its owner's state at the
snapshot. Replaying the flat arrays tick by tick and the packed arrays
launch by launch must give the same states and slots."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from gossipy_amd import ops
from gossipy_amd.core import AntiEntropyProtocol, UniformDelay
from gossipy_amd.engine import EngineConfig
from gossipy_amd.engine.schedule import NativeSchedulerAdapter

pytestmark = pytest.mark.skipif(
    ops.load_sched() is None, reason="_gossip_sched.so not built"
)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROUNDS = 4


def _cfg(kind):
    base = dict(n_nodes=120, model_size=10, delta=90, seed=13)
    if kind == "plain":
        return EngineConfig(protocol=AntiEntropyProtocol.PUSH, **base)
    proto = (AntiEntropyProtocol.PUSH if kind == "faults"
             else AntiEntropyProtocol.PUSH_PULL)
    return EngineConfig(protocol=proto, delay=UniformDelay(0, 7),
                        drop_prob=0.15, online_prob=0.9, **base)


def _sched(kind, cap, prefetch=False):
    s = NativeSchedulerAdapter(_cfg(kind))
    s.set_pack_levels(cap)
    s.set_prefetch(prefetch)
    return s


def _rounds(kind, cap, n=N_ROUNDS, prefetch=False):
    s = _sched(kind, cap, prefetch)
    out = []
    for r in range(n):
        s.next_round_flat(r)
        out.append(s.last_flat)
    return out, s


def _mix(a, b):
    return hash((a, b))


class _World:
    def __init__(self, n_nodes):
        self.state = [_mix(-1, i) for i in range(n_nodes)]
        self.slots = {}

    def snap(self, node, slot):
        self.slots[slot] = self.state[node]

    def deliver(self, node, slot):
        self.state[node] = _mix(self.state[node], self.slots[slot])


def _replay_flat(w, f):
    """Tick order: the snapshots of a tick, then its deliveries."""
    st, rt, nptr = f["snap_tptr"], f["recv_tptr"], f["recv_nptr"]
    assert len(f["pull_nodes"]) == 0 and len(f["rep_nodes"]) == 0
    assert (np.asarray(f["reply_slots"]) < 0).all()
    for t in range(len(st) - 1):
        for i in range(st[t], st[t + 1]):
            w.snap(int(f["snap_nodes"][i]), int(f["snap_slots"][i]))
        for r in range(rt[t], rt[t + 1]):
            for d in range(nptr[r], nptr[r + 1]):
                w.deliver(int(f["recv_nodes"][r]), int(f["del_slots"][d]))


def _replay_packed(w, p):
    """Launch order, as stream_round issues it: a group's snapshot launch,
    then its tick launch, whose rows run side by side. Asserts what lets
    them: one row per receiver, and no slot read in a launch that the same
    launch writes (a row reads its next slot before it writes a reply)."""
    st, rt, nptr = p["snap_tptr"], p["recv_tptr"], p["recv_nptr"]
    assert len(p["rep_nodes"]) == 0 and len(p["pull_nodes"]) == 0
    assert len(rt) == len(st) == len(p["pull_tptr"]) == len(p["rep_tptr"])
    seen = 0
    for g in range(len(st) - 1):
        for i in range(st[g], st[g + 1]):
            w.snap(int(p["snap_nodes"][i]), int(p["snap_slots"][i]))
        rows = range(rt[g], rt[g + 1])
        nodes = [int(p["recv_nodes"][r]) for r in rows]
        assert len(set(nodes)) == len(nodes), f"group {g}: a node twice"
        d0, d1 = nptr[rt[g]], nptr[rt[g + 1]]
        reads = set(int(s) for s in p["del_slots"][d0:d1])
        writes = [int(s) for s in p["reply_slots"][d0:d1] if s >= 0]
        assert len(set(writes)) == len(writes), f"group {g}: slot written twice"
        assert not reads & set(writes), f"group {g}: read/write hazard"
        for r in rows:
            x = int(p["recv_nodes"][r])
            assert nptr[r + 1] > nptr[r], "empty row"
            for d in range(nptr[r], nptr[r + 1]):
                w.deliver(x, int(p["del_slots"][d]))
                if p["reply_slots"][d] >= 0:
                    w.snap(x, int(p["reply_slots"][d]))
        seen += d1 - d0
    assert seen == len(p["del_slots"])


def _depth_and_features(f):
    """Critical depth of the round's deliveries, from the flat arrays alone:
    a delivery comes after the previous one to its receiver and after the
    delivery that made the state its slot holds. Also whether the round has
    a receiver with 3+ deliveries and a sender that received before it
    sent."""
    st, rt, nptr = f["snap_tptr"], f["recv_tptr"], f["recv_nptr"]
    node_level, node_count = {}, {}
    slot_level = {}
    late_snapshot = False
    depth = 0
    for t in range(len(st) - 1):
        for i in range(st[t], st[t + 1]):
            x = int(f["snap_nodes"][i])
            slot_level[int(f["snap_slots"][i])] = node_level.get(x, 0)
            late_snapshot |= node_count.get(x, 0) > 0
        for r in range(rt[t], rt[t + 1]):
            x = int(f["recv_nodes"][r])
            for d in range(nptr[r], nptr[r + 1]):
                lv = 1 + max(node_level.get(x, 0),
                             slot_level.get(int(f["del_slots"][d]), 0))
                node_level[x] = lv
                node_count[x] = node_count.get(x, 0) + 1
                depth = max(depth, lv)
    return depth, max(node_count.values(), default=0), late_snapshot


def _rows(p):
    return np.diff(np.asarray(p["recv_nptr"]))


def _check_same_dataflow(kind, cap):
    rounds, s = _rounds(kind, cap)
    n = _cfg(kind).n_nodes
    flat, packed = _World(n), _World(n)
    for r, f in enumerate(rounds):
        _replay_flat(flat, f)
        _replay_packed(packed, f["packed"])
        assert flat.state == packed.state, f"round {r}: node states"
        # every slot, so whatever a later round reads
        assert flat.slots == packed.slots, f"round {r}: slot contents"
        assert sorted(f["packed"]["del_slots"]) == sorted(f["del_slots"])
    assert s.pack_level_stats() == (len(rounds), 0)
    return rounds


@pytest.mark.parametrize("cap", [1, 2, 3])
@pytest.mark.parametrize("kind", ["plain", "faults"])
def test_same_dataflow(kind, cap):
    rounds = _check_same_dataflow(kind, cap)
    if kind == "faults":
        # delayed slots cross rounds: some round reads a slot it did not
        # write
        assert any(
            set(f["del_slots"].tolist()) - set(f["snap_slots"].tolist())
            for f in rounds[1:]
        )


@pytest.mark.parametrize("kind", ["plain", "faults"])
def test_chain_length_is_the_critical_depth(kind):
    rounds, _ = _rounds(kind, 1)
    for r, f in enumerate(rounds):
        p = f["packed"]
        assert (_rows(p) == 1).all(), f"round {r}"
        depth, _, _ = _depth_and_features(f)
        assert len(p["recv_tptr"]) - 1 == depth, f"round {r}"
        # one snapshot launch, at the head of the round
        assert (np.asarray(p["snap_tptr"])[1:] == len(p["snap_nodes"])).all()


@pytest.mark.parametrize("kind", ["plain", "faults"])
def test_cap_two(kind):
    one, _ = _rounds(kind, 1)
    two, _ = _rounds(kind, 2)
    some_pair = False
    for r, (a, b) in enumerate(zip(one, two)):
        rows = _rows(b["packed"])
        assert rows.max() <= 2 and rows.min() >= 1, f"round {r}"
        some_pair |= bool((rows == 2).any())
        assert len(b["packed"]["recv_tptr"]) <= len(a["packed"]["recv_tptr"])
    assert some_pair


def test_plain_schedule_has_the_features():
    # what the other tests lean on: without these the packer is not tried
    rounds, _ = _rounds("plain", 1)
    feats = [_depth_and_features(f) for f in rounds]
    assert max(d for d, _, _ in feats) >= 3
    assert max(c for _, c, _ in feats) >= 3
    assert any(late for _, _, late in feats)
    # and the late snapshots did become reply slots
    assert any((np.asarray(f["packed"]["reply_slots"]) >= 0).any()
               for f in rounds)


def test_push_pull_falls_back():
    from gossipy_amd.engine.runner import BatchedGossipSimulator

    s = _sched("push_pull", 1)
    for r in range(N_ROUNDS):
        s.next_round_flat(r)
        f = s.last_flat
        want = BatchedGossipSimulator._pack_flat(f)
        for k, v in want.items():
            if k == "eval_nodes":
                continue
            np.testing.assert_array_equal(np.asarray(f["packed"][k]), v,
                                          err_msg=k)
        assert s.pack_level_stats() == (0, r + 1)


def test_off_is_the_default_packer():
    on, _ = _rounds("plain", 0)
    default = NativeSchedulerAdapter(_cfg("plain"))
    for r, f in enumerate(on):
        default.next_round_flat(r)
        _same(f["packed"], default.last_flat["packed"], f"round {r}")
    assert default.pack_level_stats() == (0, 0)


def _same(a, b, where):
    assert list(a.keys()) == list(b.keys()), where
    for k in a:
        assert np.array_equal(a[k], b[k]), f"{where}: {k}"


@pytest.mark.parametrize("kind", ["plain", "faults"])
def test_prefetch_gives_the_same_rounds(kind):
    sync, _ = _rounds(kind, 1, n=6)
    pre, s = _rounds(kind, 1, n=6, prefetch=True)
    for r, (a, b) in enumerate(zip(sync, pre)):
        _same(a["packed"], b["packed"], f"round {r}")
    s.set_prefetch(False)


@pytest.mark.parametrize("prefetch", [False, True], ids=["sync", "prefetch"])
def test_switching_on_changes_only_later_rounds(prefetch):
    n, k = 12, 3
    off, _ = _rounds("plain", 0, n=n)
    on, _ = _rounds("plain", 1, n=n)
    s = _sched("plain", 0, prefetch)
    # the workers hold at most 6 rounds generated before the call: two
    # finished and one in the making, in each of the two stages
    ahead = 6 if prefetch else 0
    switched = False
    for r in range(n):
        if r == k:
            s.set_pack_levels(1)
        s.next_round_flat(r)
        got = s.last_flat["packed"]
        # the level packer leaves no reply launches, the default one does
        is_on = len(got["rep_nodes"]) == 0
        assert len(off[r]["packed"]["rep_nodes"]) > 0
        _same(got, (on if is_on else off)[r]["packed"], f"round {r}")
        if r < k:
            assert not is_on, f"round {r} was generated before the call"
        if r >= k + ahead:
            assert is_on, f"round {r} was generated after the call"
        assert is_on or not switched, f"round {r}: back to the old packer"
        switched |= is_on
    s.set_prefetch(False)


def test_level_packer_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "round_levels_san")
    src = os.path.join(ROOT, "tests", "native", "round_levels_san.cpp")
    build = subprocess.run(
        # the sanitizer runtimes are linked statically: the program then
        # needs nothing preloaded and minds nothing that is
        [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
         "-fno-sanitize-recover=undefined", "-static-libasan",
         "-static-libubsan", src, "-o", exe],
        capture_output=True, text=True, timeout=120,
    )
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "Sanitizer" not in run.stderr, run.stderr[-4000:]
    assert "runtime error" not in run.stderr, run.stderr[-4000:]
    assert "round_levels_san OK" in run.stdout
