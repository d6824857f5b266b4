"""CPU tests of the MLP family's test-shard evaluation: the conditions the GPU
tests' bound of 1e-6 rests on (``mlp_eval_cases.py``), the
``--engine --local-test`` path of the Onoszko example, and what the runner
reports for ragged test shards under sampled evaluation."""

import subprocess
import sys

import numpy as np
import pytest
import torch

import mlp_eval_cases as mc
from gossipy_amd.engine import NodeStateArena
from gossipy_amd.engine.backend import TorchBackend
from gossipy_amd.engine.metrics import classification_metrics_shared
from tick_cases import EVAL_TOL

CPU = torch.device("cpu")
NAMES = sorted(mc.CASES)
EXAMPLE = [sys.executable, "examples/main_onoszko_2021.py", "--engine",
           "--model", "mlp", "--nodes", "8", "--rounds", "4"]


def _scores32(case, r, x):
    state = NodeStateArena(case.params.shape[0], case.spec.D, CPU)
    state.params.copy_(case.params)
    return TorchBackend().scores(state, case.spec, torch.tensor([r]), x)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_forward_is_exact(name):
    """Every logit is an integer below 2**24, so the fp32 forward equals the
    float64 one in any summation order."""
    case = mc.CASES[name]
    assert mc.logit_bound(case) < 2 ** 24, mc.logit_bound(case)
    evs = mc.evaluations(case)
    assert evs
    for r, x, _ in evs:
        assert float(x.abs().max()) <= case.in_mag
        h64 = mc.forward64(case.spec, case.params[r].numpy(), x.numpy())
        assert np.array_equal(h64, np.round(h64))
        assert np.abs(h64).max() < 2 ** 24
        h32 = _scores32(case, r, x)[0].double().numpy()
        assert np.array_equal(h32, h64), name


def test_case_shapes():
    """What each case is there for."""
    c = mc.CASES["mlp_6_16_16_missing_classes"]
    h = mc.forward64(c.spec, c.params[0].numpy(), c.X.numpy())
    assert 1 not in set(h.argmax(axis=1).tolist())
    assert 15 not in set(c.y.tolist()) and c.spec.n_classes == 16
    c = mc.CASES["mlp_5_8_2_zero_model"]
    assert all(d["auc"] == 0.5 for d in mc.reference(c.name))
    c = mc.CASES["mlp_5_8_2_n2048"]
    assert int(c.y.sum()) == 1024 and c.y.numel() == 2048
    c = mc.CASES["mlp_5_8_2_shards"]
    assert c.ids != tuple(range(len(c.ids)))
    assert len(mc.reference(c.name)) == len(c.ids) - 1  # the empty shard
    assert all("auc" not in d for d in mc.reference("mlp_20_24_3"))


@pytest.mark.parametrize(
    "name", [n for n in NAMES if mc.CASES[n].has_auc and n != "mlp_5_8_2_n1"])
def test_auc_cases_have_ties(name):
    """Both labels and a tied positive/negative pair in every evaluation of
    at least two rows (one row cannot hold both labels), so the 0.5 branch
    of the pairwise AUC counts; and the float64 reference agrees with the
    project's own metrics on them."""
    case = mc.CASES[name]
    for (r, x, y), want in zip(mc.evaluations(case), mc.reference(name)):
        if len(y) < 2:
            continue
        s = mc.forward64(case.spec, case.params[r].numpy(), x.numpy())[:, 1]
        pos, neg = s[y.numpy() == 1], s[y.numpy() == 0]
        assert len(pos) and len(neg)
        assert np.intersect1d(pos, neg).size
        got = classification_metrics_shared(_scores32(case, r, x), y)[0]
        assert set(got) == set(want)
        for key in want:
            assert abs(got[key] - want[key]) <= EVAL_TOL, (name, key)


def _example(*extra):
    return subprocess.run([*EXAMPLE, *extra], capture_output=True, text=True,
                          timeout=280)


@pytest.mark.timeout(300)
def test_onoszko_engine_local_test():
    r = _example("--local-test")
    assert r.returncode == 0, f"failed:\n{r.stdout}\n{r.stderr}"
    assert "final local eval: {" in r.stdout
    assert "final global eval: {" in r.stdout


@pytest.mark.timeout(300)
def test_onoszko_engine_without_flag_prints_no_local_eval():
    r = _example()
    assert r.returncode == 0, f"failed:\n{r.stdout}\n{r.stderr}"
    assert "final local eval" not in r.stdout
    assert "final global eval: {" in r.stdout


def test_runner_reports_sampled_nonempty_shards():
    """The CPU backend's behaviour the kernel path has to reproduce: one
    entry per sampled node with a non-empty test shard, every round."""
    sim, rounds = mc.e2e_run(CPU)
    tc = sim.data.tcounts
    assert int((tc == 0).sum()) == 2
    assert len(rounds) == mc.E2E_ROUNDS
    for rd in rounds:
        assert 0 < len(rd["nodes"]) < mc.E2E_NODES
        want = sum(1 for n in rd["nodes"] if int(tc[n]) > 0)
        assert len(rd["evals"]) == want > 0
        assert all(set(d) == {"accuracy", "precision", "recall", "f1_score",
                              "auc"} for d in rd["evals"])
    # the seed of the end-to-end GPU comparison: no near-tie of the two
    # head logits on this trajectory
    assert mc.e2e_min_gap(sim, rounds) >= mc.MARGIN
