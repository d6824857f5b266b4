"""Evaluation of the MNIST-shaped MLP (784-100-10, 100 nodes), whose model
row misses the LDS of ``eval_mlp_kernel``: ``eval_mlp_wide`` against what it
replaces, both in one process, alternating.

(a) Per-node test shards of about 60 rows (ragged, 55..65), every node
    evaluated each round (``sampling_eval = 1.0``): rounds/s of one
    simulator with ``eval_local_wide`` and, under
    ``GOSSIPY_NO_MLP_EVAL_KERNEL=1``, with the runner's per-node loop; and
    the time of one ``eval_local_wide`` call (it ends in the D2H of the
    metric rows).
(b) A shared set of 600 rows, R = 10 and R = 100 evaluated models:
    ``ext.eval_mlp_wide`` against ``scores()`` + ``eval_metrics_scores``,
    each call followed by a device synchronise; the largest difference of
    the two results is printed next to the times.

A window is as many calls as fill ``--min-seconds`` after a warm-up of every
shape; the best and all windows are reported so the spread is visible. A
run without a GPU fails: a CPU time says nothing here.

Prints one JSON line.

Usage: python benchmarks/mlp_wide_eval_bench.py [--repeat 5]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    MLPSpec,
)
from gossipy_amd.simul import SimulationReport

N_NODES = 100
TRAIN_ROWS = 60
SHARED_ROWS = 600
KNOB = "GOSSIPY_NO_MLP_EVAL_KERNEL"


def _window(fn, min_seconds):
    """Seconds per call of ``fn`` over one window; ``fn`` ends synchronised."""
    done, t0 = 0, time.perf_counter()
    while True:
        fn()
        done += 1
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return dt / done


def _alternate(fns, repeat, min_seconds):
    """Per name, the windows (seconds per call) of ``fns``, taken in turn."""
    runs = {name: [] for name in fns}
    for fn in fns.values():
        fn()  # warm-up of every shape
    for _ in range(repeat):
        for name, fn in fns.items():
            runs[name].append(_window(fn, min_seconds))
    return runs


def _summary(runs, scale, digits):
    return {name: {"best": round(min(v) * scale, digits),
                   "runs": [round(x * scale, digits) for x in v]}
            for name, v in runs.items()}


def _shard_sim(device, spec):
    rng = np.random.default_rng(0)
    n_test = rng.integers(55, 66, size=N_NODES)
    total = int(N_NODES * TRAIN_ROWS + n_test.sum())
    X, y = make_synthetic_classification((total, 784, 10), seed=0, margin=2.0)
    shards, tests, at = [], [], 0
    for c in n_test:
        shards.append((X[at:at + TRAIN_ROWS], y[at:at + TRAIN_ROWS]))
        tests.append((X[at + TRAIN_ROWS:at + TRAIN_ROWS + c],
                      y[at + TRAIN_ROWS:at + TRAIN_ROWS + c]))
        at += TRAIN_ROWS + int(c)
    cfg = EngineConfig(
        n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=1.0, seed=42,
    )
    data = DataArena.from_shards(shards, device, test_shards=tests)
    sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    sim.add_receiver(SimulationReport())
    sim.init_nodes()
    return sim


def bench_shards(device, spec, args):
    sim = _shard_sim(device, spec)
    be, data = sim.backend, sim.data
    ids = torch.arange(N_NODES)

    def rounds(knob):
        def run():
            os.environ[KNOB] = knob
            sim.start(n_rounds=args.steps)
            torch.cuda.synchronize()
            os.environ.pop(KNOB)
        return run

    def call():
        got = be.eval_local_wide(sim.state, spec, ids, data.tx, data.ty,
                                 data.tcounts)
        assert got is not None and len(got) == N_NODES

    runs = _alternate({"kernel": rounds("0"), "loop": rounds("1")},
                      args.repeat, args.min_seconds)
    out = {"ms_per_round": _summary(runs, 1e3 / args.steps, 3)}
    out["eval_local_wide_call_ms"] = _summary(
        _alternate({"call": call}, args.repeat, args.min_seconds), 1e3, 4
    )["call"]
    return out


def bench_shared(device, spec, R, args):
    from gossipy_amd.engine import NodeStateArena
    from gossipy_amd.engine.backend import HIPBackend

    g = torch.Generator().manual_seed(R)
    state = NodeStateArena(N_NODES, spec.D, device)
    state.params.copy_(0.05 * torch.randn(N_NODES, spec.D, generator=g))
    gx = torch.randn(SHARED_ROWS, 784, generator=g).to(device)
    gy = torch.randint(0, 10, (SHARED_ROWS,), generator=g).float().to(device)
    ids = torch.randperm(N_NODES, generator=g)[:R]
    ids_dev = ids.to(device, torch.int32)
    be = HIPBackend()
    layout, n_layers = be._mlp_layout(spec, device), len(spec.dims) - 1
    empty = torch.empty(0, dtype=torch.int32)
    outs = {}

    def wide():
        outs["wide"] = be.ext.eval_mlp_wide(state.params, ids_dev, gx, gy,
                                            layout, n_layers, empty)
        torch.cuda.synchronize()

    def torch_path():
        sc = be.scores(state, spec, ids, gx)
        outs["torch"] = be.ext.eval_metrics_scores(sc.contiguous(), gy,
                                                   sc.shape[-1], False)
        torch.cuda.synchronize()

    runs = _alternate({"wide": wide, "torch": torch_path}, args.repeat,
                      args.min_seconds)
    out = _summary(runs, 1e6, 1)
    out["max_abs_diff"] = float((outs["wide"] - outs["torch"]).abs().max())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=0.5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    device = torch.device("cuda:0")
    spec = MLPSpec(d_in=784, n_classes=10, hidden=(100,), lr=0.05,
                   batch_size=32)
    res = {"config": f"mlp-784-100-10-{N_NODES}n-eval"}
    res["shards_60_rows"] = bench_shards(device, spec, args)
    for R in (10, 100):
        res[f"shared_600_rows_R{R}_us"] = bench_shared(device, spec, R, args)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
