"""GPU tests (MI355X) for the fused evaluation kernel's batched-read
scoring loop and its label-compacted pairwise AUC: every staging mode
(in-kernel scoring, per-node shards, precomputed scores) against the torch
metric implementations, at the eval-set sizes where the tile staging and the
pair split change shape, and on inputs that are all ties. All marked
``gpu``."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from gossipy_amd import ops
from gossipy_amd.engine import DataArena, LogRegSpec, NodeStateArena, PegasosSpec
from gossipy_amd.engine.backend import HIPBackend, TorchBackend
from gossipy_amd.engine.metrics import (
    binary_margin_metrics,
    classification_metrics_shared,
)

CUDA = torch.device("cuda:0")
CPU = torch.device("cpu")
D_IN = 57
KEYS = ("accuracy", "precision", "recall", "f1_score", "auc")
TOL = 1e-3  # the bound of TestEvalKernel in tests/test_gpu.py


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _eval_set(n, seed=0, pm1=False):
    """n samples whose label follows a fixed direction, 10% flipped."""
    g = _gen(seed)
    X = torch.randn(n, D_IN, generator=g)
    w = torch.randn(D_IN, generator=g)
    y = ((X @ w) > 0).float()
    flip = torch.rand(n, generator=g) < 0.1
    y = torch.where(flip, 1 - y, y)
    return X, (2 * y - 1 if pm1 else y)


def _states(R, D, seed=1, scale=0.1):
    cs = NodeStateArena(R, D, CPU)
    cs.params.copy_(torch.randn(R, D, generator=_gen(seed)) * scale)
    gs = NodeStateArena(R, D, CUDA)
    gs.params.copy_(cs.params)
    return cs, gs


def _check(want, got):
    assert len(want) == len(got)
    for w, g in zip(want, got):
        for key in KEYS:
            assert abs(w[key] - g[key]) < TOL, (key, w[key], g[key])


def _logreg_case(R, X, y, zero=False):
    spec = LogRegSpec(d_in=D_IN, n_classes=2)
    cs, gs = _states(R, spec.D)
    if zero:
        cs.params.zero_()
        gs.params.zero_()
    ids = torch.arange(R)
    want = classification_metrics_shared(TorchBackend().scores(cs, spec, ids, X), y)
    got = HIPBackend().eval_metrics_fast(gs, spec, ids, X.to(CUDA), y.to(CUDA))
    torch.cuda.synchronize()
    return want, got


@pytest.mark.parametrize("R", [1, 10])
@pytest.mark.parametrize("n_eval", [1, 2, 255, 256, 257, 600])
def test_logreg_sizes(n_eval, R):
    X, y = _eval_set(n_eval, seed=n_eval)
    _check(*_logreg_case(R, X, y))


@pytest.mark.parametrize("label", [0.0, 1.0])
def test_single_class_labels(label):
    X, _ = _eval_set(257, seed=3)
    want, got = _logreg_case(4, X, torch.full((257,), label))
    _check(want, got)
    assert all(g["auc"] == 0.5 for g in got)


def test_all_zero_params_all_ties():
    X, y = _eval_set(300, seed=4)
    want, got = _logreg_case(3, X, y, zero=True)
    _check(want, got)
    assert all(g["auc"] == 0.5 for g in got)


def test_duplicated_samples_tie():
    # 8 samples appear twice, once with each label: each pair is an exact
    # (positive, negative) tie worth half a win
    X, y = _eval_set(248, seed=5)
    X = torch.cat([X, X[:8]])
    y = torch.cat([y, 1 - y[:8]])
    _check(*_logreg_case(5, X, y))


def test_two_samples_exact():
    # one positive, one negative, same row: the single pair is a tie
    x = torch.randn(1, D_IN, generator=_gen(6))
    _, got = _logreg_case(2, torch.cat([x, x]), torch.tensor([1.0, 0.0]))
    assert all(g["auc"] == 0.5 for g in got)


@pytest.mark.parametrize("n_eval", [2, 257, 600])
def test_margin_family(n_eval):
    spec = PegasosSpec(d_in=D_IN, lam=0.01)
    X, y = _eval_set(n_eval, seed=7 + n_eval, pm1=True)
    cs, gs = _states(6, spec.D, scale=1.0)
    ids = torch.arange(6)
    sc = TorchBackend().scores(cs, spec, ids, X)
    want = binary_margin_metrics(sc[:, :, 0], y)
    got = HIPBackend().eval_metrics_fast(gs, spec, ids, X.to(CUDA), y.to(CUDA))
    _check(want, got)


def test_per_node_shards():
    # eval_counts = [0, 1, 5, full]: the empty shard is skipped
    spec = LogRegSpec(d_in=D_IN, n_classes=2)
    full = 70
    counts = [0, 1, 5, full]
    cs, gs = _states(4, spec.D)
    X, y = _eval_set(4 * full, seed=8)
    tx = X.view(4, full, D_IN).clone()
    ty = y.view(4, full).clone()
    tc = torch.tensor(counts, dtype=torch.int32)
    want = []
    for li, c in enumerate(counts):
        if c == 0:
            continue
        sc = TorchBackend().scores(cs, spec, torch.tensor([li]), tx[li, :c])
        want.extend(classification_metrics_shared(sc, ty[li, :c]))
    got = HIPBackend().eval_local_fast(
        gs, spec, torch.arange(4), tx.to(CUDA), ty.to(CUDA), tc.to(CUDA)
    )
    _check(want, got)


@pytest.mark.parametrize("R", [1, 10])
@pytest.mark.parametrize("n_eval", [1, 256, 600])
def test_precomputed_scores(n_eval, R):
    ext = ops.load_extension()
    _, y = _eval_set(n_eval, seed=9)
    sc = torch.randn(R, n_eval, 2, generator=_gen(10))
    sc[:, : n_eval // 4] = sc[:, : n_eval // 4].round()  # plenty of ties
    want = classification_metrics_shared(sc, y)
    out = ext.eval_metrics_scores(sc.to(CUDA).contiguous(), y.to(CUDA), 2, False)
    got = [dict(zip(KEYS, map(float, row))) for row in out.cpu().numpy()]
    _check(want, got)


def test_precomputed_margin_scores():
    ext = ops.load_extension()
    _, y = _eval_set(257, seed=11, pm1=True)
    m = torch.randn(3, 257, generator=_gen(12))
    m[:, :60] = m[:, :60].round()
    want = binary_margin_metrics(m, y)
    out = ext.eval_metrics_scores(m.to(CUDA).contiguous(), y.to(CUDA), 1, True)
    got = [dict(zip(KEYS, map(float, row))) for row in out.cpu().numpy()]
    _check(want, got)
