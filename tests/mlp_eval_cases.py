"""The evaluation cases of the MLP family that ``test_mlp_eval.py`` (CPU) and
``test_gpu_mlp_eval.py`` (GPU) share, in the style of
``tick_cases.eval_cases()``. Not a test module (no ``test_`` prefix).

Models, inputs and biases are small integers (at most 2 in magnitude). The
ReLU of an integer is an integer, so every activation and every head logit is
an integer, exact in fp32 in any summation order as long as the sum of the
magnitudes of a dot product's terms stays below 2**24 (``logit_bound``
computes that sum's largest possible value per case; the CPU test checks it
and the exact equality of the fp32 torch forward with the float64 one). No
argmax and no rank can then differ from float64, and what is left is the
rounding of the five output floats: the bound is ``tick_cases.EVAL_TOL``.

The reference is a float64 numpy forward (``forward64``) fed to
``ref64.class_metrics``, computed once per case and only read.

A case is either a shared set (``counts is None``: ``X`` is ``[n, d]``, every
model row of ``params`` scores the same rows) or per-node shards (``X`` is
``[n_local, S, d]``, ``counts[node]`` rows of shard ``node`` are live, the
rows behind them hold values a kernel must not read, and ``ids`` lists the
evaluated local rows in an order that is not ``arange``).
"""

from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

import ref64
from gossipy_amd.engine import MLPSpec

EVAL_ROWS = (1, 15, 16, 17, 257, 2048)


@dataclass
class MlpEvalCase:
    name: str
    spec: MLPSpec
    params: torch.Tensor            # [R, D]
    X: torch.Tensor                 # [n, d] or [n_local, S, d]
    y: torch.Tensor                 # [n] or [n_local, S]
    counts: Optional[torch.Tensor] = None  # [n_local] int32: per-node mode
    ids: Optional[tuple] = None     # evaluated local rows (per-node mode)
    in_mag: int = 2                 # largest input magnitude

    @property
    def per_node(self):
        return self.counts is not None

    @property
    def has_auc(self):
        return self.spec.n_classes == 2


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _tie_pair(X, y):
    """Rows 0 and 1 become one input under both labels: a positive and a
    negative sample with the same score, whatever the model."""
    if X.shape[0] >= 2:
        X[1] = X[0]
        y[0], y[1] = 0.0, 1.0


def _shared(name, dims, n, seed, R=3, zero=False, never=None, absent=None,
            in_mag=2, balanced=False):
    g = torch.Generator().manual_seed(seed)
    spec = MLPSpec(d_in=dims[0], n_classes=dims[-1], hidden=tuple(dims[1:-1]))
    k = spec.n_classes
    params = _ints(g, (R, spec.D), -2, 2)
    if zero:
        params.zero_()
    if never is not None:  # class `never` loses every argmax
        w_off, b_off, fin, _ = spec.layer_offsets()[-1]
        params[:, w_off + never * fin:w_off + (never + 1) * fin] = 0.0
        params[:, b_off + never] = -1000.0
    X = _ints(g, (n, dims[0]), -in_mag, in_mag)
    y = torch.randint(0, k, (n,), generator=g).float()
    if balanced:  # n // 2 positives: one in the tie pair, the rest behind it
        y[2:] = (torch.randperm(n - 2, generator=g) < n // 2 - 1).float()
    if absent is not None:  # class `absent` has no sample
        y[y == absent] = float((absent + 1) % k)
    if k == 2:
        _tie_pair(X, y)
    return MlpEvalCase(name, spec, params, X, y, in_mag=in_mag)


def _shards(name, dims, stride, counts, ids, seed):
    g = torch.Generator().manual_seed(seed)
    spec = MLPSpec(d_in=dims[0], n_classes=dims[-1], hidden=tuple(dims[1:-1]))
    n_local = len(counts)
    params = _ints(g, (n_local, spec.D), -2, 2)
    params[3] = -params[0]
    # the rows behind a shard's count hold other integers, with label 1
    X = _ints(g, (n_local, stride, dims[0]), -2, 2)
    y = torch.ones(n_local, stride)
    for node, c in enumerate(counts):
        y[node, :c] = torch.randint(0, 2, (c,), generator=g).float()
        if c >= 2:
            Xn, yn = X[node], y[node]
            _tie_pair(Xn, yn)
    return MlpEvalCase(name, spec, params, X, y,
                       counts=torch.tensor(counts, dtype=torch.int32),
                       ids=tuple(ids))


def _build():
    out = [
        # ragged MFMA tiles (20 = 16 + 4, 24 = 16 + 8, 3 of 16), k > 2
        _shared("mlp_20_24_3", (20, 24, 3), 37, 700),
        # two hidden layers; K = 132 runs the dynamic K loop past MLP_KPAD
        _shared("mlp_4_132_24_2", (4, 132, 24, 2), 37, 701),
        # k = EVAL_KMAX; class 1 never predicted, class 15 without a sample
        _shared("mlp_6_16_16_missing_classes", (6, 16, 16), 257, 702,
                never=1, absent=15),
        # every logit 0: all predictions class 0, all scores tied
        _shared("mlp_5_8_2_zero_model", (5, 8, 2), 257, 703, zero=True),
        # the LDS budget leaves a tile below n = 300 and a ragged last chunk
        _shared("mlp_256_64_2_tile_below_n", (256, 64, 2), 300, 704, R=2,
                in_mag=1),
        # per-node shards: an empty one, a single row, a full stride, ragged
        _shards("mlp_5_8_2_shards", (5, 8, 2), 64, [0, 1, 64, 37],
                [3, 1, 0, 2], 705),
    ]
    for n in EVAL_ROWS:
        # 2048 rows: 1024 positives x 1024 negatives, the pair-count limit
        out.append(_shared(f"mlp_5_8_2_n{n}", (5, 8, 2), n, 800 + n,
                           balanced=(n == 2048)))
    return out


CASES = {c.name: c for c in _build()}


def logit_bound(case):
    """The largest value the sum of magnitudes of any dot product's terms
    (bias included) can take in the case's forward, for inputs of at most
    ``in_mag`` in magnitude: layer by layer, the largest of
    ``sum_j |W[i, j]| * a + |b[i]|`` over the units ``i`` and the models."""
    p = case.params.double().abs()
    a = float(case.in_mag)
    for (w_off, b_off, fin, fout) in case.spec.layer_offsets():
        W = p[:, w_off:b_off].reshape(-1, fout, fin)
        a = float((W.sum(dim=2) * a + p[:, b_off:b_off + fout]).max())
    return a


def forward64(spec, row, x):
    """Head logits ``[n, k]`` of one model row, in float64."""
    row = np.asarray(row, dtype=np.float64)
    h = np.asarray(x, dtype=np.float64)
    offs = spec.layer_offsets()
    for li, (w_off, b_off, fin, fout) in enumerate(offs):
        h = h @ row[w_off:b_off].reshape(fout, fin).T + row[b_off:b_off + fout]
        if li < len(offs) - 1:
            h = np.maximum(h, 0.0)
    return h


def evaluations(case):
    """``(params row index, X rows, y rows)`` of every evaluation the case
    asks for, in result order; an empty shard gives none."""
    if not case.per_node:
        return [(r, case.X, case.y) for r in range(case.params.shape[0])]
    out = []
    for node in case.ids:
        c = int(case.counts[node])
        if c:
            out.append((node, case.X[node, :c], case.y[node, :c]))
    return out


_REF = {}


def reference(name):
    """The case's float64 metric dicts, computed once and only read."""
    if name not in _REF:
        case = CASES[name]
        _REF[name] = [
            ref64.class_metrics(
                forward64(case.spec, case.params[r].numpy(), x.numpy()),
                y.numpy())
            for r, x, y in evaluations(case)
        ]
    return _REF[name]


def compare(name, got, tol):
    """``got`` (a list of metric dicts) against the float64 reference: the
    same entries, the same keys, every value within ``tol``."""
    want = reference(name)
    assert len(got) == len(want), (name, len(got), len(want))
    worst = 0.0
    for i, (g, w) in enumerate(zip(got, want)):
        assert set(g) == set(w), (name, i, sorted(g), sorted(w))
        for key in w:
            worst = max(worst, abs(g[key] - w[key]))
    print(f"dev {name} {worst:.3e} tol {tol:.1e}")
    assert worst <= tol, (name, worst)


# ---- the end-to-end run of the runner tests ----------------------------------
# 40 nodes on MLP 57 -> 32 -> 2, ragged test shards of 0..7 rows (nodes 5 and
# 23 have none), half of the nodes evaluated each round.
E2E_NODES = 40
E2E_ROUNDS = 2
E2E_SEED = 11
MARGIN = 1e-4  # as pens_mlp_cases.MARGIN: the fp32 forward error is ~1e-5


def e2e_spec():
    return MLPSpec(d_in=57, n_classes=2, hidden=(32,), lr=0.1, batch_size=16)


def e2e_data(device):
    from gossipy_amd.data import make_synthetic_classification
    from gossipy_amd.engine import DataArena

    rng = np.random.default_rng(E2E_SEED)
    n_test = rng.integers(1, 8, size=E2E_NODES)
    n_test[[5, 23]] = 0
    total = int(30 * E2E_NODES + n_test.sum())
    X, y = make_synthetic_classification((total, 57, 2), seed=E2E_SEED)
    shards, tests, at = [], [], 0
    for i in range(E2E_NODES):
        c = 30 + int(n_test[i])
        shards.append((X[at:at + 30], y[at:at + 30]))
        tests.append((X[at + 30:at + c], y[at + 30:at + c]))
        at += c
    return DataArena.from_shards(shards, device, test_shards=tests)


def e2e_run(device):
    """Runs the simulation on ``device`` and returns, per round, a dict with
    the evaluated node ids (``nodes``), the models they were evaluated with
    (``params``, on the CPU) and the local metric dicts the runner reported
    (``evals``)."""
    from gossipy_amd.core import AntiEntropyProtocol
    from gossipy_amd.engine import BatchedGossipSimulator, EngineConfig
    from gossipy_amd.simul import SimulationEventReceiver

    spec = e2e_spec()
    cfg = EngineConfig(
        n_nodes=E2E_NODES, delta=20, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.5, seed=E2E_SEED,
    )
    sim = BatchedGossipSimulator(cfg, spec, e2e_data(device), device=device)
    rounds = []

    class Keep(SimulationEventReceiver):
        def update_message(self, failed, msg=None):
            pass

        def update_evaluation(self, round, on_user, evaluation):
            assert on_user
            rounds[-1]["evals"] = list(evaluation)

        def update_end(self):
            pass

        def update_timestep(self, t):
            pass

    inner = sim._evaluate

    def evaluate(sched, t):
        rounds.append({
            "nodes": np.unique(sched.eval_nodes),
            "params": sim.state.params.detach().cpu().clone(),
            "evals": [],
        })
        inner(sched, t)

    sim._evaluate = evaluate
    sim.add_receiver(Keep())
    sim.init_nodes()
    sim.start(n_rounds=E2E_ROUNDS)
    return sim, rounds


def e2e_min_gap(sim, rounds):
    """The smallest top-2 head-logit gap, from a float64 forward, over every
    (node, test sample) pair the run evaluated."""
    tx, tc = sim.data.tx.cpu(), sim.data.tcounts.cpu()
    gap = np.inf
    for rd in rounds:
        for node in rd["nodes"]:
            c = int(tc[node])
            if c:
                h = forward64(sim.spec, rd["params"][node].numpy(),
                              tx[node, :c].numpy())
                gap = min(gap, float(np.abs(h[:, 1] - h[:, 0]).min()))
    return gap
