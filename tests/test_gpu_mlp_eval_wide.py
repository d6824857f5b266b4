"""``eval_mlp_wide``, the MLP evaluation past the LDS budget, against the
float64 reference at ``tick_cases.EVAL_TOL``: the case table of
``mlp_eval_cases.py`` through the wide kernel (``GOSSIPY_MLP_EVAL_WIDE=1``),
the shapes only it takes (a model row that misses LDS, the scalar-load path,
a second column-group pass, the edges of a row block, shards that span two
blocks), the routing, and the runner end to end against the per-node loop.
The cases hold small integers, so every logit is exact in fp32 in any
summation order (``test_wide_cases_are_exact``, which needs no GPU)."""

import numpy as np
import pytest
import torch

import mlp_eval_cases as mc
import ref64
from gossipy_amd.engine import MLPSpec, NodeStateArena
from gossipy_amd.engine.backend import HIPBackend, metric_rows_to_dicts
from tick_cases import EVAL_TOL

gpu = pytest.mark.gpu
NAMES = sorted(mc.CASES)
_NO_COUNTS = torch.empty(0, dtype=torch.int32)
WIDE_DIMS = (640, 64, 2)  # D * 4 = 164.6 KB: the row alone misses LDS


def _wide_cases():
    out = [
        mc._shared("wide_640_64_2", WIDE_DIMS, 37, 900, R=2, in_mag=1),
        # d_in % 4 != 0: scalar loads, a ragged last K panel of 2 columns
        mc._shared("wide_642_64_2", (642, 64, 2), 37, 901, R=2, in_mag=1),
        # 16-byte loads and a ragged last K panel (644 = 20 * 32 + 4)
        mc._shared("wide_644_64_2", (644, 64, 2), 37, 902, R=2, in_mag=1),
        # 136 > 128 outputs: a second column-group pass; two hidden layers
        mc._shared("wide_640_136_24_3", (640, 136, 24, 3), 37, 903, R=2,
                   in_mag=1),
        # an empty shard, one that spans two row blocks, rows behind a count
        mc._shards("wide_640_64_2_shards", WIDE_DIMS, 70, [0, 1, 70, 37],
                   [3, 1, 0, 2], 904),
    ]
    for n in (63, 64, 65, 129):  # the row-block edges of RB = 64
        out.append(mc._shared(f"wide_640_64_2_n{n}", WIDE_DIMS, n, 910 + n,
                              R=2, in_mag=1))
    return {c.name: c for c in out}


WIDE = _wide_cases()


def _evaluate(case):
    """The case's metric dicts from ``eval_local_wide`` (per-node) or
    ``ext.eval_mlp_wide`` (shared set)."""
    cuda = torch.device("cuda:0")
    be = HIPBackend()
    state = NodeStateArena(case.params.shape[0], case.spec.D, cuda)
    state.params.copy_(case.params)
    X, y = case.X.to(cuda), case.y.to(cuda)
    if case.per_node:
        got = be.eval_local_wide(state, case.spec, torch.tensor(case.ids),
                                 X, y, case.counts.to(cuda))
        assert got is not None
        return got
    R = case.params.shape[0]
    out = be.ext.eval_mlp_wide(
        state.params, torch.arange(R, dtype=torch.int32, device=cuda), X, y,
        be._mlp_layout(case.spec, cuda), len(case.spec.dims) - 1, _NO_COUNTS)
    assert out.shape == (R, 5)
    return metric_rows_to_dicts(out.cpu().numpy())


@gpu
@pytest.mark.parametrize("name", NAMES)
def test_case_table_through_wide_kernel(name, monkeypatch):
    monkeypatch.setenv("GOSSIPY_MLP_EVAL_WIDE", "1")
    mc.compare(name, _evaluate(mc.CASES[name]), EVAL_TOL)


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_cases_are_exact(name):
    assert mc.logit_bound(WIDE[name]) < 2 ** 24


@gpu
@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_only_cases_match_float64(name):
    case = WIDE[name]
    got = _evaluate(case)
    want = [ref64.class_metrics(
                mc.forward64(case.spec, case.params[r].numpy(), x.numpy()),
                y.numpy())
            for r, x, y in mc.evaluations(case)]
    assert len(got) == len(want)
    worst = 0.0
    for g, w in zip(got, want):
        assert set(g) == set(w)
        worst = max(worst, max(abs(g[key] - w[key]) for key in w))
    print(f"dev {name} {worst:.3e} tol {EVAL_TOL:.1e}")
    assert worst <= EVAL_TOL


class _NoLaunch:
    """The extension with an ``eval_mlp_wide`` that must not be called."""

    def __init__(self, ext):
        self._ext = ext

    def __getattr__(self, name):
        assert name != "eval_mlp_wide", "eval_mlp_wide launched"
        return getattr(self._ext, name)


def _shards_of(spec, n_local=3, stride=4):
    cuda = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    state = NodeStateArena(n_local, spec.D, cuda)
    state.params.copy_(torch.randn(n_local, spec.D, generator=g))
    tx = torch.randn(n_local, stride, spec.d_in, generator=g).to(cuda)
    ty = torch.randint(0, 2, (n_local, stride), generator=g).float().to(cuda)
    tc = torch.full((n_local,), stride, dtype=torch.int32, device=cuda)
    return state, torch.arange(n_local), tx, ty, tc


@gpu
def test_routing(monkeypatch):
    be = HIPBackend()
    wide = MLPSpec(d_in=640, n_classes=2, hidden=(64,))
    args = _shards_of(wide)
    assert be.eval_local_fast(args[0], wide, *args[1:]) is None
    assert len(be.eval_local_wide(args[0], wide, *args[1:])) == 3
    assert not be.ext.eval_mlp_wide_fits([640, 64, 2], 2049)
    assert be.ext.eval_mlp_wide_fits([640, 64, 2], 2048)
    assert not be.ext.eval_mlp_wide_fits([640, 2048, 2], 4)  # < 16 rows

    # a spec that fits LDS never reaches the wide op with no knob set
    small = MLPSpec(d_in=6, n_classes=2, hidden=(8,))
    sargs = _shards_of(small)
    be.ext = _NoLaunch(be.ext)
    assert be.eval_local_wide(sargs[0], small, *sargs[1:]) is None
    assert len(be.eval_metrics_fast(sargs[0], small, sargs[1], sargs[2][0],
                                    sargs[3][0])) == 3

    monkeypatch.setenv("GOSSIPY_NO_MLP_EVAL_KERNEL", "1")
    assert be.eval_local_fast(args[0], wide, *args[1:]) is None
    assert be.eval_local_wide(args[0], wide, *args[1:]) is None


E2E_NODES = 12


def _e2e_data(device):
    from gossipy_amd.data import make_synthetic_classification
    from gossipy_amd.engine import DataArena

    n_test = np.random.default_rng(mc.E2E_SEED).integers(0, 8, size=E2E_NODES)
    n_test[5] = 0
    X, y = make_synthetic_classification(
        (int(30 * E2E_NODES + n_test.sum()), WIDE_DIMS[0], 2),
        seed=mc.E2E_SEED)
    shards, tests, at = [], [], 0
    for c in n_test:
        shards.append((X[at:at + 30], y[at:at + 30]))
        tests.append((X[at + 30:at + 30 + c], y[at + 30:at + 30 + c]))
        at += 30 + int(c)
    return DataArena.from_shards(shards, device, test_shards=tests)


@gpu
def test_runner_wide_kernel_against_loop(monkeypatch):
    """``test_gpu_mlp_eval.test_runner_kernel_against_loop`` on 640-64-2,
    whose evaluation only the wide kernel takes: same entries and keys,
    P/R/F1 within 1e-6 and AUC within 1e-4 once no evaluated sample's two
    logits are closer than ``mc.MARGIN`` (the argument is that test's)."""
    monkeypatch.setattr(mc, "E2E_NODES", E2E_NODES)
    monkeypatch.setattr(mc, "e2e_data", _e2e_data)
    monkeypatch.setattr(mc, "e2e_spec", lambda: MLPSpec(
        d_in=WIDE_DIMS[0], n_classes=2, hidden=(64,), lr=0.1, batch_size=16))
    calls = []
    real = HIPBackend.eval_local_wide

    def counted(self, *a):
        got = real(self, *a)
        calls.append(got is not None)
        return got

    monkeypatch.setattr(HIPBackend, "eval_local_wide", counted)
    cuda = torch.device("cuda:0")
    sim, kern = mc.e2e_run(cuda)
    assert calls == [True] * mc.E2E_ROUNDS
    monkeypatch.setenv("GOSSIPY_NO_MLP_EVAL_KERNEL", "1")
    sim2, loop = mc.e2e_run(cuda)
    assert calls[mc.E2E_ROUNDS:] == [False] * mc.E2E_ROUNDS
    gap = min(mc.e2e_min_gap(sim, kern), mc.e2e_min_gap(sim2, loop))
    assert gap >= mc.MARGIN, f"smallest top-2 logit gap {gap:.3e}"

    worst = {"prf": 0.0, "auc": 0.0}
    for a, b in zip(kern, loop):
        assert np.array_equal(a["nodes"], b["nodes"])
        assert len(a["evals"]) == len(b["evals"]) > 0
        for da, db in zip(a["evals"], b["evals"]):
            assert set(da) == set(db) and "auc" in da
            for key in da:
                kind = "auc" if key == "auc" else "prf"
                worst[kind] = max(worst[kind], abs(da[key] - db[key]))
    print(f"wide kernel vs loop: prf {worst['prf']:.3e}"
          f" auc {worst['auc']:.3e} gap {gap:.3e}")
    assert worst["prf"] <= 1e-6
    assert worst["auc"] <= 1e-4
