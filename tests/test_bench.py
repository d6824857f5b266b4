"""bench.py's contract: ``--steps`` sets the timed rounds, the result line
carries ``ms_per_step``, and ``--dump-outputs`` writes the timed path's
outputs reproducibly (same arguments => same arrays)."""

import importlib.util
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(monkeypatch, capsys, *argv):
    spec = importlib.util.spec_from_file_location(
        "_bench_under_test", os.path.join(ROOT, "bench.py")
    )
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    for var in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(var, raising=False)
    capsys.readouterr()
    bench.main()
    lines = [
        ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")
    ]
    assert len(lines) == 1, "exactly one JSON result line"
    return json.loads(lines[0])


@pytest.mark.timeout(120)
def test_dump_outputs_reproducible(monkeypatch, capsys, tmp_path):
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1",
            "--nodes-per-gpu", "100"]
    outs = []
    for name in ("a", "b"):
        d = tmp_path / name
        res = _run_bench(monkeypatch, capsys, *args, "--dump-outputs", str(d))
        assert res["steps"] == 3 and res["warmup"] == 1
        assert res["ms_per_step"] > 0
        assert res["value"] == pytest.approx(
            100 * 1000.0 / res["ms_per_step"], rel=0.05
        )
        outs.append({f: np.load(d / f) for f in sorted(os.listdir(d))})
    a, b = outs
    assert set(a) == {"params.npy", "ages.npy", "rows.npy", "eval_last.npy"}
    assert a["params.npy"].shape == (100, 116)
    assert a["ages.npy"].shape == (100,)
    assert np.array_equal(a["rows.npy"], np.arange(100))
    # 1 init update + at least one update per received model over 4 rounds
    assert (a["ages.npy"] >= 1).all()
    for f in a:
        assert a[f].dtype in (np.float32, np.float64), f
        assert np.isfinite(a[f]).all(), f
        assert np.array_equal(a[f], b[f]), f"{f} differs between runs"


@pytest.mark.timeout(120)
def test_full_flag_accepted(monkeypatch, capsys):
    res = _run_bench(
        monkeypatch, capsys, "--gpus", "1", "--steps", "2", "--warmup", "0",
        "--nodes-per-gpu", "100", "--full",
    )
    for key in ("metric", "value", "unit", "higher_is_better", "dtype",
                "ms_per_step"):
        assert key in res
    assert res["steps"] == 2
