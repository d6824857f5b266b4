"""GPU tests (MI355X) of ``eval_mlp``, the one-launch test-shard evaluation
of the MLP family: every case of ``mlp_eval_cases.py`` against the float64
reference at ``tick_cases.EVAL_TOL`` (per-node cases through
``HIPBackend.eval_local_fast``, shared-set cases through ``ext.eval_mlp``),
the two ways back to the per-node loop (a shape that does not fit, the
``GOSSIPY_NO_MLP_EVAL_KERNEL`` knob), and the runner end to end with the
kernel against the same run without it. All marked ``gpu``."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import mlp_eval_cases as mc
from gossipy_amd.engine import MLPSpec, NodeStateArena
from gossipy_amd.engine.backend import HIPBackend, metric_rows_to_dicts
from tick_cases import EVAL_TOL

CUDA = torch.device("cuda:0")
NAMES = sorted(mc.CASES)
_NO_COUNTS = torch.empty(0, dtype=torch.int32)


def _state(case):
    state = NodeStateArena(case.params.shape[0], case.spec.D, CUDA)
    state.params.copy_(case.params)
    return state


def _tile(be, spec, n):
    return be.ext.eval_mlp_tile(spec.D, spec.d_in, sum(spec.dims[1:]), n)


@pytest.mark.parametrize("name", NAMES)
def test_eval_mlp_matches_float64(name):
    case = mc.CASES[name]
    be = HIPBackend()
    state = _state(case)
    X, y = case.X.to(CUDA), case.y.to(CUDA)
    if case.per_node:
        got = be.eval_local_fast(state, case.spec, torch.tensor(case.ids),
                                 X, y, case.counts.to(CUDA))
        assert got is not None
    else:
        R = case.params.shape[0]
        out = be.ext.eval_mlp(
            state.params, torch.arange(R, dtype=torch.int32, device=CUDA),
            X, y, be._mlp_layout(case.spec, CUDA),
            len(case.spec.layer_offsets()), _NO_COUNTS)
        assert out.shape == (R, 5)
        got = metric_rows_to_dicts(out.cpu().numpy())
    mc.compare(name, got, EVAL_TOL)
    if name == "mlp_5_8_2_zero_model":
        assert all(d["auc"] == 0.5 for d in got)
    if not case.has_auc:
        assert all("auc" not in d for d in got)


def test_tile_below_n():
    """The 256-64-2 case runs in more than one chunk, the last one ragged."""
    case = mc.CASES["mlp_256_64_2_tile_below_n"]
    n = case.X.shape[0]
    tile = _tile(HIPBackend(), case.spec, n)
    assert 0 < tile < n
    assert n % tile


def test_tile_limits():
    be = HIPBackend()
    spec = mc.CASES["mlp_5_8_2_n2048"].spec
    assert _tile(be, spec, 2048) == 512
    assert _tile(be, spec, 2049) == 0   # the pair count of the AUC
    assert _tile(be, spec, 1) == 1


class _NoLaunch:
    """The extension with an ``eval_mlp`` that must not be called."""

    def __init__(self, ext):
        self._ext = ext

    def __getattr__(self, name):
        assert name != "eval_mlp", "eval_mlp launched"
        return getattr(self._ext, name)


def _small_shards(spec, n_local=3, stride=4):
    g = torch.Generator().manual_seed(5)
    state = NodeStateArena(n_local, spec.D, CUDA)
    state.params.copy_(torch.randn(n_local, spec.D, generator=g))
    tx = torch.randn(n_local, stride, spec.d_in, generator=g).to(CUDA)
    ty = torch.randint(0, 2, (n_local, stride), generator=g).float().to(CUDA)
    tc = torch.full((n_local,), stride, dtype=torch.int32, device=CUDA)
    return state, torch.arange(n_local), tx, ty, tc


def test_oversize_shape_falls_back():
    """A model that leaves fewer than 16 rows of forward scratch: ``None``
    (the runner's per-node loop serves it), no launch, no exception."""
    spec = MLPSpec(d_in=512, n_classes=2, hidden=(64,))
    be = HIPBackend()
    assert _tile(be, spec, 4) == 0
    be.ext = _NoLaunch(be.ext)
    state, ids, tx, ty, tc = _small_shards(spec)
    assert be.eval_local_fast(state, spec, ids, tx, ty, tc) is None


def test_knob_turns_the_kernel_off(monkeypatch):
    spec = MLPSpec(d_in=6, n_classes=2, hidden=(8,))
    be = HIPBackend()
    state, ids, tx, ty, tc = _small_shards(spec)
    assert be.eval_local_fast(state, spec, ids, tx, ty, tc) is not None
    monkeypatch.setenv("GOSSIPY_NO_MLP_EVAL_KERNEL", "1")
    be.ext = _NoLaunch(be.ext)
    assert be.eval_local_fast(state, spec, ids, tx, ty, tc) is None


def test_runner_kernel_against_loop(monkeypatch):
    """The same 2-round run with the kernel and with the per-node loop: the
    same entries and keys; accuracy, precision, recall and F1 within 1e-6
    once no evaluated sample's two logits are closer than 1e-4 (the two
    forwards round differently, about 1e-5 at K <= 57, so a nearer pair
    could flip a prediction); AUC within 1e-4, since two scores apart by
    rounding noise may swap ranks and a swap moves the AUC by at most
    1 / (npos * nneg)."""
    calls = []
    real = HIPBackend.eval_local_fast

    def counted(self, *a):
        got = real(self, *a)
        calls.append(got is not None)
        return got

    monkeypatch.setattr(HIPBackend, "eval_local_fast", counted)
    sim, kern = mc.e2e_run(CUDA)
    assert sim.backend.name == "hip"
    assert calls == [True] * mc.E2E_ROUNDS
    gap = mc.e2e_min_gap(sim, kern)
    assert gap >= mc.MARGIN, f"smallest top-2 logit gap {gap:.3e}"

    monkeypatch.setenv("GOSSIPY_NO_MLP_EVAL_KERNEL", "1")
    sim2, loop = mc.e2e_run(CUDA)
    assert calls[mc.E2E_ROUNDS:] == [False] * mc.E2E_ROUNDS
    gap2 = mc.e2e_min_gap(sim2, loop)
    assert gap2 >= mc.MARGIN, f"smallest top-2 logit gap {gap2:.3e}"

    worst = {"prf": 0.0, "auc": 0.0}
    for a, b in zip(kern, loop):
        assert np.array_equal(a["nodes"], b["nodes"])
        assert len(a["evals"]) == len(b["evals"]) > 0
        for da, db in zip(a["evals"], b["evals"]):
            assert set(da) == set(db) and "auc" in da
            for key in da:
                kind = "auc" if key == "auc" else "prf"
                worst[kind] = max(worst[kind], abs(da[key] - db[key]))
    print(f"kernel vs loop: prf {worst['prf']:.3e} auc {worst['auc']:.3e}"
          f" gap {gap:.3e}")
    assert worst["prf"] <= 1e-6
    assert worst["auc"] <= 1e-4
