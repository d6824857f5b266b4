"""GPU tests (MI355X) of the chunk-sorted evaluation (``GOSSIPY_EVAL_RANK=1``:
``eval_metrics_rank`` / ``eval_metrics_rank_scores``) against the float64
reference of ``ref64.py`` on integer-valued eval sets past the pairwise
kernel's 2048 rows: chunk borders, ties across them, chunks of one class,
more pairs than fp32 counts, three classes, margins, signed zeros, and the
bits of the pairwise kernel where both routes run. Bound: ``EVAL_TOL`` on
every entry (scores are exact in fp32, the AUC is integer until its last
division). All marked ``gpu``."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import ref64
import tick_cases as tc
from gossipy_amd import ops
from gossipy_amd.engine import LogRegSpec, MLPSpec, NodeStateArena
from gossipy_amd.engine.backend import HIPBackend

CUDA = torch.device("cuda:0")
CH = 2048  # ext.EVAL_RANK_CH, asserted in test_paths
KEYS = ("accuracy", "precision", "recall", "f1_score", "auc")
EVAL = {c.name: c for c in tc.eval_cases()}


def _distinct(n):
    # tick_cases._big_eval(distinct=True) at n rows: the class-1 score of
    # model 0 is a permutation of 0..n-1, model 1 ranks it backwards
    case = tc._logreg_eval(f"distinct_n{n}", n, 4, 2, 77, R=2, zero=True)
    g = torch.Generator().manual_seed(78)
    case.X[:, 0] = torch.randperm(n, generator=g).float()
    case.params[:, 4] = 1.0
    case.params[1, 4] = -1.0
    case.params[:, 8] = 1000.0
    case.y = (torch.randperm(n, generator=g) < n // 2).float()
    return case


def _one_class_chunks():
    # chunk 0 holds only positives (an empty run), chunk 1 only negatives
    # (an empty positive list), chunk 2 both
    case = tc._logreg_eval("one_class_chunks", 3 * CH, 4, 2, 31)
    case.y[:CH] = 1.0
    case.y[CH:2 * CH] = 0.0
    return case


CASES = [tc._logreg_eval(f"edges_n{n}", n, 4, 2, 700 + i)
         for i, n in enumerate((2049, 2 * CH, 2 * CH + 1, 3 * CH + 17))]
CASES += [_distinct(4097), _distinct(8193), _one_class_chunks()]
CASES += [tc._logreg_eval("all_ties", 2049, 4, 2, 41, zero=True)]
CASES += [tc._logreg_eval(f"all_label{v}", 2049, 4, 2, 42 + v, labels=float(v))
          for v in (0, 1)]
CASES += [tc._logreg_eval(f"k3_n{n}", n, 4, 3, 50, never=1, absent=2)
          for n in (2049, 2 * CH + 1)]
CASES += [tc._margin_eval("margin_n2049", 2049, 3, 60)]
CASES = {c.name: c for c in CASES}


def _same(want, got, name):
    assert set(want) == set(got), (name, want, got)
    for key in want:
        assert abs(want[key] - got[key]) <= tc.EVAL_TOL, (
            name, key, want[key], got[key])


def _state(case):
    gs = NodeStateArena(case.params.shape[0], case.spec.D, CUDA)
    gs.params.copy_(case.params)
    return gs


@pytest.mark.parametrize("name", sorted(CASES))
def test_rank_route_matches_reference(name, monkeypatch):
    monkeypatch.setenv("GOSSIPY_EVAL_RANK", "1")
    case = CASES[name]
    R = case.params.shape[0]
    got = HIPBackend().eval_metrics_fast(
        _state(case), case.spec, torch.arange(R), case.X.to(CUDA),
        case.y.to(CUDA))
    assert got is not None and len(got) == R
    for r in range(R):
        _same(tc.eval_reference(case, case.params[r]), got[r], name)
    if name.startswith("all_"):
        assert all(g["auc"] == 0.5 for g in got)
    if name.startswith("k3"):
        assert all("auc" not in g for g in got)
    if name.startswith("distinct"):
        assert abs(got[0]["auc"] + got[1]["auc"] - 1.0) <= 2 * tc.EVAL_TOL


@pytest.mark.parametrize("family", ["logreg", "margin"])
def test_rank_scores_mode_signed_zeros(family):
    # float64 reference scores cast to fp32 (integers: exact); zero scores
    # become -0.0 in the positive class and stay +0.0 in the negative one,
    # and must still count as ties
    ext = ops.load_extension()
    if family == "logreg":
        case = tc._logreg_eval("scores_logreg", 2049, 3, 2, 81)
        sc = np.stack([ref64.logreg_scores(p.numpy(), case.X.numpy(), 3, 2)
                       for p in case.params])
        s1, pos = sc[:, :, 1], case.y.numpy() == 1
    else:
        case = tc._margin_eval("scores_margin", 2049, 3, 82)
        sc = case.X.double().numpy() @ case.params.double().numpy().T
        sc = np.ascontiguousarray(sc.T)
        s1, pos = sc, case.y.numpy() > 0
    flip = (s1 == 0) & pos[None, :]
    assert flip.any() and ((s1 == 0) & ~pos[None, :]).any()
    s1[flip] = -0.0
    dev = torch.from_numpy(sc).float().to(CUDA).contiguous()
    assert torch.signbit(dev).any()
    if family == "logreg":
        out = ext.eval_metrics_rank_scores(dev, case.y.to(CUDA), 2, False)
        want = [ref64.class_metrics(s, case.y.numpy()) for s in sc]
    else:
        out = ext.eval_metrics_rank_scores(dev, case.y.to(CUDA), 1, True)
        want = [ref64.margin_metrics(s, case.y.numpy()) for s in sc]
    rows = out.cpu().numpy()
    for r, w in enumerate(want):
        _same(w, {k: float(v) for k, v in zip(KEYS, rows[r]) if v >= 0},
              (family, r))


@pytest.mark.parametrize("name", [
    "eval_repeats_n700", "eval_2048_all_ties", "eval_2048_all_distinct",
    "eval_margin_n257", "eval_k3_missing_classes",
])
def test_rank_bits_equal_pairwise(name, monkeypatch):
    case = EVAL[name]
    be, gs = HIPBackend(), _state(case)
    ids = torch.arange(case.params.shape[0])
    rows = {}
    for knob in ("0", "1"):
        monkeypatch.setenv("GOSSIPY_EVAL_RANK", knob)
        buf, ev, valid = be.eval_metrics_launch(
            gs, case.spec, ids, case.X.to(CUDA), case.y.to(CUDA))
        ev.synchronize()
        rows[knob] = buf[:valid].clone()
    assert torch.equal(rows["0"], rows["1"]), (rows["0"], rows["1"])


def test_paths(monkeypatch):
    be = HIPBackend()
    assert be.ext.EVAL_RANK_CH == CH
    specs = (LogRegSpec(d_in=4), MLPSpec(d_in=4, hidden=(8,), n_classes=2))
    monkeypatch.delenv("GOSSIPY_EVAL_RANK", raising=False)
    for spec in specs:
        assert be.eval_metrics_path(spec, 2048) == "pairwise"
        assert be.eval_metrics_path(spec, 2049) == "torch"
    monkeypatch.setenv("GOSSIPY_EVAL_RANK", "1")
    for spec in specs:
        assert be.eval_metrics_path(spec, 256) == "rank"
        assert be.eval_metrics_path(spec, 10_000) == "rank"


@pytest.mark.parametrize("family", ["logreg", "mlp"])
def test_runner_rank_route_pipelined_equals_blocking(family, monkeypatch):
    from gossipy_amd.core import AntiEntropyProtocol
    from gossipy_amd.data import make_synthetic_classification
    from gossipy_amd.engine import (BatchedGossipSimulator, DataArena,
                                    EngineConfig)
    from gossipy_amd.simul import SimulationReport

    monkeypatch.setenv("GOSSIPY_EVAL_RANK", "1")
    n_nodes, n_eval = 100, 2100
    X, y = make_synthetic_classification((400 + n_eval, 8, 2), seed=3,
                                         margin=1.0)
    shards = [(X[i * 4:(i + 1) * 4], y[i * 4:(i + 1) * 4])
              for i in range(n_nodes)]
    data = DataArena.from_shards(shards, CUDA, global_eval=(X[400:], y[400:]))
    spec = (LogRegSpec(d_in=8, n_classes=2, lr=0.1) if family == "logreg"
            else MLPSpec(d_in=8, hidden=(16,), n_classes=2, lr=0.1))
    reports = []
    for pipe_off in ("0", "1"):
        monkeypatch.setenv("GOSSIPY_NO_EVAL_PIPE", pipe_off)
        cfg = EngineConfig(n_nodes=n_nodes, delta=10,
                           protocol=AntiEntropyProtocol.PUSH,
                           model_size=spec.D, sampling_eval=0.1, seed=4)
        sim = BatchedGossipSimulator(cfg, spec, data, device=CUDA)
        assert sim.backend.eval_metrics_path(spec, n_eval) == "rank"
        rep = SimulationReport()
        sim.add_receiver(rep)
        sim.init_nodes()
        sim.start(n_rounds=3)
        reports.append(rep.get_evaluation(False))
    assert len(reports[0]) == 3 and reports[0] == reports[1]
    assert all(0.0 <= m["auc"] <= 1.0 for _, m in reports[0])
