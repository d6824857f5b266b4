"""The native scheduler's prefetch worker (``set_prefetch``) must hand out
exactly the rounds the synchronous path generates, in order, whatever
``set_lean`` says at the time a round is converted, and must start and stop
cleanly. The prefetcher itself (``csrc/round_prefetch.h``) is also driven by
a stand-alone thread-sanitizer build."""

import os
import shutil
import subprocess
import sys
import textwrap

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


def _cfgs():
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
    }


CFGS = _cfgs()


def _assert_same(a, b, where=""):
    assert list(a.keys()) == list(b.keys()), where
    for k in a:
        x, y = a[k], b[k]
        if isinstance(x, dict):
            assert isinstance(y, dict), where + k
            _assert_same(x, y, where + k + ".")
        elif isinstance(x, np.ndarray):
            assert isinstance(y, np.ndarray) and x.dtype == y.dtype, where + k
            assert np.array_equal(x, y), where + k
        else:
            assert type(x) is type(y) and x == y, where + k


def _pair(cfg, lean):
    sync, pre = NativeSchedulerAdapter(cfg), NativeSchedulerAdapter(cfg)
    sync.set_lean(lean)
    pre.set_lean(lean)
    pre.set_prefetch(True)
    return sync, pre


@pytest.mark.parametrize("lean", [False, True], ids=["full", "lean"])
@pytest.mark.parametrize("name", sorted(CFGS))
def test_prefetch_equals_sync(name, lean):
    sync, pre = _pair(CFGS[name], lean)
    for r in range(N_ROUNDS):
        a, b = sync._native.next_round(r), pre._native.next_round(r)
        _assert_same(a, b, f"round {r}: ")
        assert "packed" in a and ("merge_bounds" in a) == (not lean)


@pytest.mark.parametrize("name", ["push", "push_pull_uniform"])
def test_set_lean_toggle_mid_run(name):
    # rounds 10 and 11 were generated before the toggle reaches the worker
    sync, pre = _pair(CFGS[name], False)
    for r in range(N_ROUNDS):
        if r in (10, 20):
            sync.set_lean(r == 10)
            pre.set_lean(r == 10)
        a, b = sync._native.next_round(r), pre._native.next_round(r)
        _assert_same(a, b, f"round {r}: ")
        assert ("snap_nodes" in b) == (not 10 <= r < 20)


def test_adapter_objects_match():
    # through the adapter's own entry points, summary objects included
    sync, pre = _pair(CFGS["push"], True)
    for r in range(N_ROUNDS):
        s, p = sync.next_round_flat(r), pre.next_round_flat(r)
        assert (s.n_slots, s.sent_messages, s.failed_messages, s.total_size) == (
            p.n_slots, p.sent_messages, p.failed_messages, p.total_size)
        assert np.array_equal(s.eval_nodes, p.eval_nodes)
        _assert_same(sync.last_flat, pre.last_flat)


def test_out_of_order_request_raises():
    _, pre = _pair(CFGS["push"], True)
    pre._native.next_round(0)
    with pytest.raises(ValueError):
        pre._native.next_round(2)
    with pytest.raises(ValueError):
        pre._native.next_round(0)
    pre._native.next_round(1)  # the refused requests consumed nothing


def test_prefetch_off_drains_and_continues():
    sync, pre = _pair(CFGS["faults"], False)
    for r in range(5):
        _assert_same(sync._native.next_round(r), pre._native.next_round(r))
    pre.set_prefetch(False)  # rounds generated ahead are served first
    for r in range(5, 12):
        _assert_same(sync._native.next_round(r), pre._native.next_round(r))
    pre.set_prefetch(True)  # and back on, right after a round was taken
    for r in range(12, 18):
        _assert_same(sync._native.next_round(r), pre._native.next_round(r))


def test_construct_destroy_many():
    code = textwrap.dedent(
        """
        from gossipy_amd.core import AntiEntropyProtocol
        from gossipy_amd.engine import EngineConfig
        from gossipy_amd.engine.schedule import NativeSchedulerAdapter
        cfg = EngineConfig(n_nodes=200, delta=20, model_size=116, seed=3,
                           protocol=AntiEntropyProtocol.PUSH)
        for i in range(200):
            s = NativeSchedulerAdapter(cfg)
            s.set_prefetch(True)
            for r in range((0, 1, 3)[i % 3]):
                s.next_round_flat(r)
            del s
        print("done")
        """
    )
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    out = subprocess.run(
        [sys.executable, "-c", code], env=env, cwd=ROOT, timeout=60,
        capture_output=True, text=True,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    assert out.stdout.strip().endswith("done")


def test_prefetcher_under_thread_sanitizer(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "prefetch_tsan")
    src = os.path.join(ROOT, "tests", "native", "prefetch_tsan.cpp")
    build = subprocess.run(
        [gxx, "-std=c++17", "-O1", "-g", "-fsanitize=thread", "-pthread",
         src, "-o", exe],
        capture_output=True, text=True, timeout=120,
    )
    assert build.returncode == 0, build.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    # Older sanitizer runtimes cannot place their shadow memory under a
    # kernel with wide address randomisation and stop before main(); that
    # says nothing about the code, so run the same binary with
    # randomisation off for this one process, and skip only if the runtime
    # cannot start that way either.
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
    assert "prefetch_tsan OK" in run.stdout
