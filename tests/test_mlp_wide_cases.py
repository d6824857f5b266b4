"""CPU tests of the wide-MLP case table (``mlp_wide_cases.py``): for every
case the fp32 ``TorchBackend`` oracle is within ``tol / 8`` of the float64
reference with exactly equal ages, as ``test_ref64.py`` asks of the standing
table; the shapes miss the LDS plan's budget for the reason each case is
named after; the extension's path query, which needs no GPU, picks the kernel
by that budget and obeys ``GOSSIPY_MLP_WIDE``; and the example runs."""

import subprocess
import sys

import pytest
import torch

import mlp_wide_cases as wc
import tick_cases as tc
from gossipy_amd import ops
from gossipy_amd.engine import DataArena, MLPSpec
from gossipy_amd.engine.backend import _MODE_ID, HIPBackend, TorchBackend

NAMES = [c.name for c in wc.CASES]
LDS = 160 * 1024


def lds_plan_bytes(spec, rows):
    """Bytes of LDS ``tick_mlp_kernel`` needs: model slabs, the staged
    batch with every layer's output, two gradient buffers."""
    dims = spec.dims
    slabs = 2 if spec.mode == tc.UM else 1
    return 4 * (slabs * spec.D + rows * sum(dims) + 2 * rows * max(dims))


def batch_rows(case):
    return min(case.spec.batch_size or max(case.shards), max(case.shards))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_within_an_eighth_of_tol(name):
    case = wc.BY_NAME[name]
    assert case.tol >= 1e-4
    state, data, pool = tc.build(case)
    tc.run_backend(TorchBackend(), case, state, data, pool)
    e32 = tc.deviation(case, wc.reference(name), state, pool)
    print(f"e32 {name} {e32:.3e} tol {case.tol:.1e}")
    assert e32 <= case.tol / 8, (name, e32)


def test_the_table_reaches_what_it_is_for():
    assert len({c.seed for c in wc.CASES} | {c.seed for c in tc.CASES}) == \
        len(wc.CASES) + len(tc.CASES)
    for c in wc.CASES:
        assert c.spec.family == "mlp" and not c.spec.n_parts
        assert lds_plan_bytes(c.spec, batch_rows(c)) > LDS, c.name
    d_only = wc.BY_NAME["wide_mlp_D_only"].spec
    assert 4 * d_only.D > LDS
    assert lds_plan_bytes(d_only, 16) - 4 * d_only.D < LDS // 2
    mnist = wc.BY_NAME["wide_mlp_784_merge_update"].spec
    assert lds_plan_bytes(mnist, 32) - 4 * mnist.D > LDS  # the batch too
    full = wc.BY_NAME["wide_mlp_full_batch"]
    dims = full.spec.dims
    # without the input and the layer-0 dX the batch still misses the budget
    assert 4 * 200 * (sum(dims[1:]) + 2 * max(dims[1:])) > LDS
    assert {c.spec.mode for c in wc.CASES} == set(tc.MODES.values())
    assert 0 in wc.BY_NAME["wide_mlp_784_update"].shards
    assert wc.BY_NAME["wide_mlp_pass_through"].flags
    assert wc.BY_NAME["wide_mlp_limited"].spec.age_diff_threshold == 2
    assert len(wc.BY_NAME["wide_mlp_three_layers"].spec.dims) == 4


# ---- the path query: host code of the extension, no GPU needed --------------------

def _path(spec, smax):
    # of the data only the shard stride matters
    x = torch.empty(2, smax, spec.d_in)
    return HIPBackend().mlp_tick_path(spec, DataArena(x, x[:, :, 0], None))


def test_path_query_follows_the_lds_budget(monkeypatch):
    monkeypatch.delenv("GOSSIPY_MLP_WIDE", raising=False)
    for c in wc.CASES:
        assert _path(c.spec, max(c.shards)) == "wide", c.name
    small = MLPSpec(d_in=57, n_classes=2, hidden=(100,), batch_size=32)
    assert _path(small, 46) == "lds"
    # the threshold itself: 11-h-3 with a batch of 32 rows, h around the
    # width whose plan is exactly the budget
    ext = ops.load_extension()
    for mode in (tc.MU, tc.UM):
        paths = {}
        for h in range(250, 450):  # the budget is met up to h = 364 / 321
            spec = MLPSpec(d_in=11, n_classes=3, hidden=(h,), batch_size=32,
                           mode=mode)
            over = lds_plan_bytes(spec, 32) > LDS
            paths[over] = paths.get(over, 0) + 1
            got = ext.mlp_tick_path(list(spec.dims), 32, 40, _MODE_ID[mode])
            assert got == ("wide" if over else "lds"), (h, mode)
        assert paths[True] and paths[False]


def test_path_query_obeys_the_knob(monkeypatch):
    big = wc.BY_NAME["wide_mlp_784_merge_update"].spec
    small = MLPSpec(d_in=57, n_classes=2, hidden=(100,), batch_size=32)
    monkeypatch.setenv("GOSSIPY_MLP_WIDE", "1")
    assert _path(small, 46) == "wide" and _path(big, 70) == "wide"
    monkeypatch.setenv("GOSSIPY_MLP_WIDE", "0")
    assert _path(small, 46) == "lds"
    with pytest.raises(RuntimeError, match="mlp LDS budget exceeded"):
        _path(big, 70)


def test_path_query_wants_a_plain_mlp():
    with pytest.raises(ValueError):
        _path(MLPSpec(d_in=784, n_classes=10, n_parts=4), 70)


@pytest.mark.timeout(300)
def test_example_runs():
    r = subprocess.run(
        [sys.executable, "examples/main_wide_mlp.py", "--nodes", "8",
         "--rounds", "2"],
        capture_output=True, text=True, timeout=280,
    )
    assert r.returncode == 0, f"{r.stdout}\n{r.stderr}"
    assert "tick path" in r.stdout and "final global eval" in r.stdout
