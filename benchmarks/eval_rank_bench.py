"""Shared eval set of 10 000 rows, 1000 nodes: the chunk-sorted evaluation
(``GOSSIPY_EVAL_RANK=1``: ``eval_metrics_rank`` / ``eval_metrics_rank_scores``)
against the route such a set takes without the knob (torch scores and the
hipGraph-captured tensor metrics chain), both in one process, alternating.

Per family (logreg 57x2, MLP 57-100-2) and ``sampling_eval`` (0.1: about 100
evaluated models a round, 0.01: about 10):

* rounds/s of one simulator with the knob unset and set, in turn;
* the evaluation alone: ``eval_metrics_launch`` (scores, metrics and the
  enqueued D2H of the result rows) on the sampled number of models, timed
  by device events around a batch of calls.

A window is as many calls as fill ``--min-seconds`` after a warm-up of both
routes; the best and all windows are reported so the spread is visible. The
largest difference of the two routes' result rows is printed next to the
times: the torch chain sums ranks in fp32, so its AUC is not exact at this
size. A run without a GPU fails: a CPU time says nothing here.

Prints one JSON line.

Usage: python benchmarks/eval_rank_bench.py [--repeat 3]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
    MLPSpec,
)
from gossipy_amd.simul import SimulationReport

N_NODES = 1000
TRAIN_ROWS = 10
EVAL_ROWS = 10_000
KNOB = "GOSSIPY_EVAL_RANK"


def _windows(fns, repeat, min_seconds):
    """Per name, ``repeat`` windows (seconds per call) of ``fns``, taken in
    turn; every ``fn`` returns the seconds its one call took."""
    runs = {name: [] for name in fns}
    for fn in fns.values():
        fn()  # warm-up of every route
    for _ in range(repeat):
        for name, fn in fns.items():
            done, spent, t0 = 0, 0.0, time.perf_counter()
            while time.perf_counter() - t0 < min_seconds:
                spent += fn()
                done += 1
            runs[name].append(spent / done)
    return runs


def _sim(device, spec, X, y, sampling):
    n_train = N_NODES * TRAIN_ROWS
    shards = [(X[i * TRAIN_ROWS:(i + 1) * TRAIN_ROWS],
               y[i * TRAIN_ROWS:(i + 1) * TRAIN_ROWS]) for i in range(N_NODES)]
    data = DataArena.from_shards(
        shards, device, global_eval=(X[n_train:], y[n_train:]))
    cfg = EngineConfig(
        n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=sampling, seed=42,
    )
    sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    sim.add_receiver(SimulationReport())
    sim.init_nodes()
    return sim


def bench(device, spec, X, y, sampling, args):
    sim = _sim(device, spec, X, y, sampling)
    be, data = sim.backend, sim.data
    R = max(1, round(N_NODES * sampling))
    ids = torch.randperm(N_NODES, generator=torch.Generator().manual_seed(1))[:R]
    paths, rows = {}, {}

    def rounds(knob):
        def run():
            os.environ[KNOB] = knob
            t0 = time.perf_counter()
            sim.start(n_rounds=args.steps)
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        return run

    def call(knob, reps=20):
        def run():
            os.environ[KNOB] = knob
            paths[knob] = be.eval_metrics_path(spec, EVAL_ROWS)
            e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in "ab")
            e0.record()
            for _ in range(reps):
                h = be.eval_metrics_launch(sim.state, spec, ids, data.gx,
                                           data.gy)
            e1.record()
            e1.synchronize()
            rows[knob] = h[0][:h[2]].clone()
            return e0.elapsed_time(e1) * 1e-3 / reps
        return run

    out = {"R": R}
    runs = _windows({"torch": rounds("0"), "rank": rounds("1")}, args.repeat,
                    args.min_seconds)
    out["rounds_per_s"] = {
        name: {"best": round(args.steps / min(v), 2),
               "runs": [round(args.steps / x, 2) for x in v]}
        for name, v in runs.items()}
    runs = _windows({"torch": call("0"), "rank": call("1")}, args.repeat,
                    args.min_seconds)
    out["eval_call_us"] = {
        name: {"best": round(min(v) * 1e6, 1),
               "runs": [round(x * 1e6, 1) for x in v]}
        for name, v in runs.items()}
    assert paths == {"0": "torch", "1": "rank"}, paths
    out["max_abs_diff"] = float((rows["0"] - rows["1"]).abs().max())
    os.environ.pop(KNOB, None)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    device = torch.device("cuda:0")
    X, y = make_synthetic_classification(
        (N_NODES * TRAIN_ROWS + EVAL_ROWS, 57, 2), seed=0, margin=2.0)
    specs = {
        "logreg-57x2": LogRegSpec(d_in=57, n_classes=2, lr=0.1),
        "mlp-57-100-2": MLPSpec(d_in=57, n_classes=2, hidden=(100,), lr=0.05),
    }
    res = {"config": f"{N_NODES}n-eval{EVAL_ROWS}"}
    for name, spec in specs.items():
        for sampling in (0.1, 0.01):
            res[f"{name}-samp{sampling}"] = bench(device, spec, X, y,
                                                  sampling, args)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
