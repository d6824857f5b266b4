"""The native scheduler's hand-over to the round driver, checked without a
GPU: ``next_round_packed_into`` writes the driver's upload layout
(``csrc/round_layout.h``) and must agree with what ``next_round`` hands to
the Python path, with the worker thread on or off and with the two entry
points mixed. The layout writer and the driver's ring-slot bookkeeping
(``csrc/round_ring.h``) are also driven by a stand-alone
address/undefined-behaviour sanitizer build."""

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
N_ROUNDS = 30

# the upload order, pinned here: the table of csrc/round_source.h has to
# say the same (test_array_table_is_the_one_definition)
DEV_NAMES = (
    "snap_nodes", "snap_slots", "recv_nodes", "recv_nptr", "del_slots",
    "reply_slots", "pull_nodes", "pull_slots", "rep_nodes", "rep_nptr",
    "rep_slots", "del_pids", "rep_pids", "rep_reply_slots",
)
TPTRS = ("snap_tptr", "recv_tptr", "pull_tptr", "rep_tptr")


def test_array_table_is_the_one_definition():
    import inspect

    from gossipy_amd.engine.runner import BatchedGossipSimulator

    # both extensions export the table they were compiled with
    for mod in (ops.load_sched(), ops.load_extension()):
        assert mod.ROUND_ARRAY_NAMES == DEV_NAMES
        assert mod.ROUND_TPTR_NAMES == TPTRS
    # and the Python path's upload reads it from the extension it calls,
    # with no list of its own
    src = inspect.getsource(BatchedGossipSimulator._run_round_fast)
    assert "for n in ext.ROUND_ARRAY_NAMES" in src
    assert "for n in ext.ROUND_TPTR_NAMES" in src
    for name in DEV_NAMES + TPTRS:
        assert name not in src, name


def _cfgs():
    # the five of tests/test_sched_prefetch.py, and one whose eval draw
    # (30 of 60 ids, with replacement) has duplicates in every round
    push = dict(protocol=AntiEntropyProtocol.PUSH, model_size=116, seed=9)
    return {
        "push": EngineConfig(n_nodes=200, delta=20, sampling_eval=0.05, **push),
        "push_pull_uniform": EngineConfig(
            n_nodes=60, delta=12, model_size=116, seed=9,
            protocol=AntiEntropyProtocol.PUSH_PULL, delay=UniformDelay(1, 5),
        ),
        "faults": EngineConfig(
            n_nodes=60, delta=12, drop_prob=0.3, online_prob=0.7, **push
        ),
        "parts": EngineConfig(n_nodes=60, delta=12, n_parts=4, **push),
        "sampled": EngineConfig(n_nodes=60, delta=12, sampled=True, **push),
        "dup_eval": EngineConfig(n_nodes=60, delta=12, sampling_eval=0.5, **push),
    }


CFGS = _cfgs()
BUF = np.empty(1 << 16, np.int32)


def _native(cfg, prefetch):
    s = NativeSchedulerAdapter(cfg)
    s.set_lean(True)
    s.set_prefetch(prefetch)
    return s._native


def _check_packed(got, buf, f, where):
    """``got``/``buf`` from next_round_packed_into against the dict ``f`` of
    a twin scheduler's next_round."""
    lens, tptrs, counters, ids = got
    assert len(lens) == len(DEV_NAMES), where
    off = 0
    for name, n in zip(DEV_NAMES, lens):
        want = f["packed"].get(name, np.zeros(0, np.int32))
        assert np.array_equal(buf[off:off + n], want), where + name
        off += n
    for name, t in zip(TPTRS, tptrs):
        assert t.dtype == np.int32, where + name
        assert np.array_equal(t, f["packed"][name]), where + name
    assert tuple(counters) == (
        f["sent"], f["failed"], f["total_size"], f["n_slots"]), where
    assert ids.dtype == np.int32, where
    if f["eval_nodes"] is None:
        assert len(ids) == 0, where
    else:
        assert np.array_equal(ids, np.unique(f["eval_nodes"])), where
        # and they sit right after the event arrays
        assert np.array_equal(buf[off:off + len(ids)], ids), where


@pytest.mark.parametrize("prefetch", [False, True], ids=["sync", "prefetch"])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_packed_into_equals_dict_path(name, prefetch):
    twin, sch = _native(CFGS[name], False), _native(CFGS[name], prefetch)
    dups = False
    for r in range(N_ROUNDS):
        f = twin.next_round(r)
        BUF.fill(-9)
        got = sch.next_round_packed_into(r, BUF)
        _check_packed(got, BUF, f, f"{name} round {r}: ")
        if f["eval_nodes"] is not None:
            dups |= len(np.unique(f["eval_nodes"])) < len(f["eval_nodes"])
    if name == "dup_eval":
        assert dups  # the case the config is there for


def _same(a, b, where):
    assert list(a.keys()) == list(b.keys()), where
    for k in a:
        if isinstance(a[k], dict):
            _same(a[k], b[k], where + k + ".")
        elif isinstance(a[k], np.ndarray):
            assert np.array_equal(a[k], b[k]), where + k
        else:
            assert a[k] == b[k], where + k


@pytest.mark.parametrize("prefetch", [False, True], ids=["sync", "prefetch"])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_interleaved_with_next_round(name, prefetch):
    # one sequence whichever entry point asks: rounds alternate in an
    # irregular pattern between the dict path and the packed one
    twin, sch = _native(CFGS[name], False), _native(CFGS[name], prefetch)
    for r in range(N_ROUNDS):
        f = twin.next_round(r)
        if (r * 7) % 5 < 2:
            _same(f, sch.next_round(r), f"{name} round {r}: ")
        else:
            got = sch.next_round_packed_into(r, BUF)
            _check_packed(got, BUF, f, f"{name} round {r}: ")


@pytest.mark.parametrize("prefetch", [False, True], ids=["sync", "prefetch"])
def test_small_buffer_raises_and_keeps_the_round(prefetch):
    twin, sch = _native(CFGS["push"], False), _native(CFGS["push"], prefetch)
    small = np.full(8, -9, np.int32)
    for r in range(6):
        f = twin.next_round(r)
        with pytest.raises(ValueError):
            sch.next_round_packed_into(r, small)
        assert (small == -9).all()  # nothing written
        if r % 2:  # the refused round is still the next one, for both
            _same(f, sch.next_round(r), f"round {r}: ")
        else:
            got = sch.next_round_packed_into(r, BUF)
            _check_packed(got, BUF, f, f"round {r}: ")
    # and the worker can be stopped and restarted around a refusal
    with pytest.raises(ValueError):
        sch.next_round_packed_into(6, small)
    sch.set_prefetch(False)
    _same(twin.next_round(6), sch.next_round(6), "round 6: ")


@pytest.mark.parametrize("prefetch", [False, True], ids=["sync", "prefetch"])
def test_out_of_order_raises(prefetch):
    twin, sch = _native(CFGS["push"], False), _native(CFGS["push"], prefetch)
    for r in (2, -1):
        with pytest.raises(ValueError):
            sch.next_round_packed_into(r, BUF)
    _check_packed(sch.next_round_packed_into(0, BUF), BUF, twin.next_round(0), "")
    for r in (0, 2):
        with pytest.raises(ValueError):
            sch.next_round_packed_into(r, BUF)
    # the refused requests consumed nothing
    _check_packed(sch.next_round_packed_into(1, BUF), BUF, twin.next_round(1), "")


def test_bad_buffers_raise():
    sch = _native(CFGS["push"], False)
    with pytest.raises((ValueError, TypeError)):
        sch.next_round_packed_into(0, np.empty((4, 1 << 12), np.int32))
    ro = np.empty(1 << 16, np.int32)
    ro.setflags(write=False)
    with pytest.raises((ValueError, TypeError)):
        sch.next_round_packed_into(0, ro)
    with pytest.raises((ValueError, TypeError)):
        sch.next_round_packed_into(0, np.empty(1 << 17, np.int32)[::2])
    sch.next_round_packed_into(0, BUF)  # none of them consumed round 0


def test_layout_and_ring_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "round_layout_san")
    src = os.path.join(ROOT, "tests", "native", "round_layout_san.cpp")
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
    assert "round_layout_san OK" in run.stdout


def test_two_stage_prefetch_under_thread_sanitizer(tmp_path):
    # set_prefetch chains two RoundPrefetch workers (generate, then pack);
    # the chain's stop, drain and destruction orders get a run of their own
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "prefetch_chain_tsan")
    src = os.path.join(ROOT, "tests", "native", "prefetch_chain_tsan.cpp")
    build = subprocess.run(
        [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread",
         src, "-o", exe],
        capture_output=True, text=True, timeout=120,
    )
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    # as in tests/test_sched_prefetch.py: an older sanitizer runtime cannot
    # place its shadow memory under wide address randomisation and stops
    # before main(); run the same binary with randomisation off for this one
    # process, and skip only if the runtime cannot start that way either
    cannot_start = "unexpected memory mapping"
    if run.returncode != 0 and cannot_start in run.stderr:
        setarch = shutil.which("setarch")
        if setarch is not None:
            run = subprocess.run(
                [setarch, os.uname().machine, "-R", exe],
                capture_output=True, text=True, timeout=60,
            )
        if run.returncode != 0 and (
            cannot_start in run.stderr or "setarch" in run.stderr
        ):
            pytest.skip("the thread-sanitizer runtime cannot start here")
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert "ThreadSanitizer" not in run.stderr, run.stderr[-4000:]
    assert "prefetch_chain_tsan OK" in run.stdout
