"""CPU tests of the float64 reference (``ref64.py``) and of the shared case
table (``tick_cases.py``): the reference's gradients against finite
differences, its AUC against the pair count, and, for every case, the fp32
``TorchBackend`` oracle within ``tol / 8`` of the reference with exactly
equal ages. The cases with more batch rows than block threads must also be
able to see a per-sample stage that stops at the block size."""

import numpy as np
import pytest
import torch

import ref64
import tick_cases as tc
from gossipy_amd.engine import LogRegSpec, MLPSpec
from gossipy_amd.engine.backend import TorchBackend
from gossipy_amd.engine.metrics import (
    binary_margin_metrics,
    classification_metrics_shared,
)

NAMES = [c.name for c in tc.CASES]
_REF = {}


def reference(name):
    """The case's reference result, computed once and only read."""
    if name not in _REF:
        _REF[name] = tc.run_ref(tc.BY_NAME[name])
    return _REF[name]


# ---- the reference itself -------------------------------------------------------

def _loss(spec, row, x, y):
    if spec.family == "logreg":
        z = ref64.logreg_scores(row, x, spec.d_in, spec.n_classes)
        h = 1.0 / (1.0 + np.exp(-z))
    else:
        h = x
        offs = spec.layer_offsets()
        for li, (w_off, b_off, fin, fout) in enumerate(offs):
            h = h @ row[w_off:b_off].reshape(fout, fin).T + row[b_off:b_off + fout]
            if li < len(offs) - 1:
                h = np.maximum(h, 0.0)
    h = h - h.max(axis=1, keepdims=True)
    logp = h - np.log(np.exp(h).sum(axis=1, keepdims=True))
    return -logp[np.arange(len(y)), y].mean()


@pytest.mark.parametrize("spec", [
    LogRegSpec(d_in=5, n_classes=3),
    MLPSpec(d_in=5, n_classes=3, hidden=(4, 6)),
    MLPSpec(d_in=5, n_classes=4, hidden=()),
], ids=["logreg", "mlp3", "mlp1"])
def test_reference_gradient_is_the_loss_gradient(spec):
    rng = np.random.default_rng(3)
    row = rng.normal(size=spec.D) * 0.5
    x = rng.normal(size=(7, spec.d_in))
    y = rng.integers(0, spec.n_classes, size=7)
    grad = ref64._logreg_grad if spec.family == "logreg" else ref64._mlp_grad
    g = grad(spec, row, x, y, None)
    num = np.empty_like(g)
    h = 1e-6
    for e in range(spec.D):
        up, dn = row.copy(), row.copy()
        up[e] += h
        dn[e] -= h
        num[e] = (_loss(spec, up, x, y) - _loss(spec, dn, x, y)) / (2 * h)
    assert np.abs(g - num).max() < 1e-8


def test_rank_auc_is_the_pair_count():
    rng = np.random.default_rng(4)
    s = rng.integers(-3, 4, size=90).astype(np.float64)  # many ties
    pos = rng.random(90) < 0.4
    wins = sum((a > b) + 0.5 * (a == b) for a in s[pos] for b in s[~pos])
    assert ref64.rank_auc(s, pos) == pytest.approx(
        wins / (pos.sum() * (~pos).sum()), abs=1e-12)
    assert ref64.rank_auc(s, np.zeros(90, bool)) == 0.5
    assert ref64.rank_auc(s, np.ones(90, bool)) == 0.5
    assert ref64.rank_auc(np.zeros(90), pos) == 0.5


def test_metrics_follow_the_engine_conventions():
    rng = np.random.default_rng(5)
    for k in (2, 3, 16):
        sc = rng.integers(-2, 3, size=(70, k)).astype(np.float32)
        sc[:, k - 1] = -9.0  # a class that is never predicted
        y = rng.integers(0, max(1, k - 1), size=70)
        y[y == 0] = 1 if k > 2 else 0  # k > 2: class 0 absent from labels
        want = classification_metrics_shared(
            torch.from_numpy(sc)[None], torch.from_numpy(y).float())[0]
        got = ref64.class_metrics(sc, y)
        assert set(want) == set(got)
        for key in want:
            assert abs(want[key] - got[key]) < 1e-6, (k, key)
    m = rng.integers(-2, 3, size=80).astype(np.float32)  # zeros included
    y = np.where(rng.random(80) < 0.5, 1.0, -1.0).astype(np.float32)
    want = binary_margin_metrics(torch.from_numpy(m)[None],
                                 torch.from_numpy(y))[0]
    got = ref64.margin_metrics(m, y)
    for key in want:
        assert abs(want[key] - got[key]) < 1e-6, key


# ---- every case: fp32 oracle against the reference --------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_oracle_within_an_eighth_of_tol(name):
    case = tc.BY_NAME[name]
    assert case.tol >= 1e-4
    state, data, pool = tc.build(case)
    tc.run_backend(TorchBackend(), case, state, data, pool)
    e32 = tc.deviation(case, reference(name), state, pool)
    print(f"e32 {name} {e32:.3e} tol {case.tol:.1e}")
    assert e32 <= case.tol / 8, (name, e32)


def test_the_table_reaches_what_it_is_for():
    # the cases listed in the module docstring exist with the shapes that
    # take the paths they are named after
    rows = [c for c in tc.CASES if c.block]
    assert all(max(c.shards) > c.block for c in rows)
    wide = [c for c in tc.CASES if c.name.startswith("wide_logreg")]
    assert wide and all(c.spec.D > 1024 for c in wide)
    assert {c.spec.d_in for c in tc.CASES if c.name.startswith("mfma_fwd")} \
        == {31, 32, 33, 63, 64, 65, 127, 128, 129, 132, 133, 136, 141}
    assert all(len(c.shards) <= 6 for c in tc.CASES)


# ---- the batch-row cases can see a stage that stops at the block size -------------

def _batches(case, c):
    bs = case.spec.batch_size or c
    return [min(bs, c - s) for s in range(0, c, bs)]


@pytest.mark.parametrize("kind", ["zero", "scores"])
@pytest.mark.parametrize("name", [c.name for c in tc.CASES if c.block])
def test_batch_row_cases_see_a_truncated_stage(name, kind):
    case = tc.BY_NAME[name]
    good = reference(name).params
    with np.errstate(over="ignore"):  # raw scores as gradients may blow up
        bad = tc.run_ref(case, broken=(case.block, kind)).params
    hit = [i for i, c in enumerate(case.shards)
           if c and max(_batches(case, c)) > case.block]
    assert hit
    for i, c in enumerate(case.shards):
        dev = np.abs(good[i] - bad[i]).max()
        print(f"sens {name} {kind} node {i} rows {c} dev {dev:.3e}")
        if i in hit:
            # every node with a batch past the block size moves by 10 * tol
            assert dev >= 10 * case.tol, (name, kind, i, dev)
        else:
            assert dev == 0.0


# ---- evaluation cases: fp32 metrics against the reference -------------------------

EVAL = {c.name: c for c in tc.eval_cases()}


@pytest.mark.parametrize("name", sorted(EVAL))
def test_eval_oracle_within_an_eighth_of_tol(name):
    case = EVAL[name]
    spec, R = case.spec, case.params.shape[0]
    if spec.family == "logreg":
        d, k = spec.d_in, spec.n_classes
        # raw fp32 scores (integers, exact): the oracle's sigmoid would
        # saturate large ones into ties that the kernel does not have
        sc = torch.einsum("nd,rkd->rnk", case.X,
                          case.params[:, :k * d].view(R, k, d))
        sc = sc + case.params[:, None, k * d:]
        want = classification_metrics_shared(sc, case.y)
    else:
        want = binary_margin_metrics(case.params @ case.X.t(), case.y)
    e32 = 0.0
    for r in range(R):
        ref = tc.eval_reference(case, case.params[r])
        assert set(ref) == set(want[r])
        e32 = max(e32, max(abs(ref[key] - want[r][key]) for key in ref))
    print(f"e32 {name} {e32:.3e} tol {tc.EVAL_TOL:.1e}")
    assert e32 <= tc.EVAL_TOL / 8


def test_eval_cases_hit_their_edges():
    zero = EVAL["eval_zero_model_n257"]
    assert tc.eval_reference(zero, zero.params[0])["auc"] == 0.5
    for lab in (0, 1):
        c = EVAL[f"eval_all_label{lab}"]
        assert tc.eval_reference(c, c.params[0])["auc"] == 0.5
    big = EVAL["eval_2048_all_distinct"]
    assert int(big.y.sum()) == 1024
    s = ref64.logreg_scores(big.params[0].numpy(), big.X.numpy(), 4, 2)[:, 1]
    assert len(np.unique(s)) == 2048
    a0 = tc.eval_reference(big, big.params[0])["auc"]
    a1 = tc.eval_reference(big, big.params[1])["auc"]
    assert a0 + a1 == pytest.approx(1.0, abs=1e-12) and a0 != 0.5
    # some margin scores are exactly 0, some repeated scores tie across labels
    m = EVAL["eval_margin_n257"]
    assert ((m.X @ m.params[0]) == 0).any()
    for k in (3, 16):
        c = EVAL[f"eval_k{k}_missing_classes"]
        sc = ref64.logreg_scores(c.params[0].numpy(), c.X.numpy(), 4, k)
        assert 1 not in set(sc.argmax(axis=1)) and (c.y != k - 1).all()
