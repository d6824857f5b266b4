"""CPU tests of ``logreg_wide_cases.py``: the fp32 ``TorchBackend`` oracle
is within ``tol / 8`` of the float64 reference with equal ages; every shape
misses the LDS plan; the extension's path query (host code, no GPU) follows
that budget and ``GOSSIPY_LOGREG_WIDE``; the example runs."""

import subprocess
import sys

import pytest
import torch

import logreg_wide_cases as wc
import mlp_wide_cases
import tick_cases as tc
from gossipy_amd.engine import DataArena, LogRegSpec
from gossipy_amd.engine.backend import HIPBackend, TorchBackend

LDS = 160 * 1024


@pytest.mark.parametrize("name", [c.name for c in wc.CASES])
def test_oracle_within_an_eighth_of_tol(name):
    case = wc.BY_NAME[name]
    assert case.tol == 1e-4
    state, data, pool = tc.build(case)
    tc.run_backend(TorchBackend(), case, state, data, pool)
    e32 = tc.deviation(case, wc.reference(name), state, pool)
    print(f"e32 {name} {e32:.3e} tol {case.tol:.1e}")
    assert e32 <= case.tol / 8, (name, e32)


def test_every_case_misses_the_lds_plan_and_seeds_are_its_own():
    for c in wc.CASES:
        assert c.spec.family == "logreg" and not c.spec.n_parts
        assert wc.lds_plan_bytes(c) > LDS, c.name
    assert wc.lds_plan_bytes(wc.BY_NAME["784_update"]) == 164432
    others = {c.seed for c in tc.CASES} | {c.seed for c in mlp_wide_cases.CASES}
    seeds = {c.seed for c in wc.CASES}
    assert len(seeds) == len(wc.CASES) and min(seeds) == 4001
    assert not seeds & others


def _path(spec, smax):
    x = torch.empty(2, smax, spec.d_in)
    return HIPBackend().logreg_tick_path(spec, DataArena(x, x[:, :, 0], None))


def test_path_query_follows_the_lds_budget(monkeypatch):
    monkeypatch.delenv("GOSSIPY_LOGREG_WIDE", raising=False)
    for c in wc.CASES:
        assert _path(c.spec, max(c.shards)) == "wide", c.name
    assert _path(LogRegSpec(784, 10, batch_size=31), 70) == "lds"
    assert _path(LogRegSpec(784, 10, batch_size=32), 70) == "wide"
    assert _path(LogRegSpec(57, 2), 46) == "lds"
    # the threshold itself: d x 10 and 32 rows, d around the budget's width
    seen = set()
    for d in range(760, 800):
        spec = LogRegSpec(d, 10, batch_size=32)
        over = 4 * (2 * spec.D + 32 * d + 32 * 10) > LDS
        seen.add(over)
        assert _path(spec, 40) == ("wide" if over else "lds"), d
    assert seen == {True, False}


def test_path_query_obeys_the_knob(monkeypatch):
    big, small = LogRegSpec(784, 10, batch_size=32), LogRegSpec(57, 2)
    monkeypatch.setenv("GOSSIPY_LOGREG_WIDE", "1")
    assert _path(small, 46) == "wide" and _path(big, 70) == "wide"
    monkeypatch.setenv("GOSSIPY_LOGREG_WIDE", "0")
    assert _path(small, 46) == "lds"
    with pytest.raises(RuntimeError, match="logreg LDS budget exceeded: 164432"):
        _path(big, 70)


def test_path_query_wants_a_plain_logreg():
    for kw in (dict(n_parts=4), dict(sample_size=0.1)):
        with pytest.raises(ValueError):
            _path(LogRegSpec(784, 10, **kw), 70)


@pytest.mark.timeout(300)
def test_example_runs():
    r = subprocess.run(
        [sys.executable, "examples/main_wide_logreg.py", "--nodes", "8",
         "--rounds", "2"],
        capture_output=True, text=True, timeout=280,
    )
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr}"
    assert "tick path" in r.stdout and "final global eval" in r.stdout
