"""Round throughput of the MLP family when every node is evaluated on its
own test shard each round (``DataArena`` with ``test_shards``, no global
set): the accuracy-on-the-node's-own-distribution metric of Onoszko 2021.

Shape: 1000 nodes, MLP 57 -> 100 -> 2, delta 100, PUSH, ``sampling_eval =
1.0``; synthetic 57-feature data, about 40 train and 5 test rows per node
(test shards are ragged, 3..7 rows).

Reports rounds/s, best of ``--repeat`` windows on one simulator after
``--warmup`` rounds; a window is calls of ``--steps`` rounds, each ending in
a device synchronise, until ``--min-seconds`` have passed. Every window is
printed so the spread is visible. The script uses only API that
predates the one-launch MLP shard evaluation, so the same file measures the
commit before it; ``GOSSIPY_NO_MLP_EVAL_KERNEL=1`` turns the kernel off on a
commit that has it. A run without a GPU fails: a CPU time says nothing here.

Prints one JSON line.

Usage: python benchmarks/mlp_local_eval_bench.py [--steps 20] [--warmup 2]
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

N_NODES = 1000
TRAIN_ROWS = 40


def _data(device):
    rng = np.random.default_rng(0)
    n_test = rng.integers(3, 8, size=N_NODES)  # ragged, mean 5
    total = int(N_NODES * TRAIN_ROWS + n_test.sum())
    X, y = make_synthetic_classification((total, 57, 2), seed=0, margin=2.0)
    X = torch.as_tensor(X, dtype=torch.float32)
    y = torch.as_tensor(y, dtype=torch.float32)
    perm = rng.permutation(total)
    shards, tests = [], []
    at = 0
    for i in range(N_NODES):
        tr = perm[at:at + TRAIN_ROWS]
        te = perm[at + TRAIN_ROWS:at + TRAIN_ROWS + int(n_test[i])]
        at += TRAIN_ROWS + int(n_test[i])
        shards.append((X[tr], y[tr]))
        tests.append((X[te], y[te]))
    return DataArena.from_shards(shards, device, test_shards=tests)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    device = torch.device("cuda:0")
    spec = MLPSpec(d_in=57, n_classes=2, hidden=(100,), lr=0.05, batch_size=32)
    cfg = EngineConfig(
        n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=1.0, seed=42,
    )
    sim = BatchedGossipSimulator(cfg, spec, _data(device), device=device)
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes()
    sim.start(n_rounds=args.warmup)
    torch.cuda.synchronize()
    runs, rounds = [], args.warmup
    for _ in range(args.repeat):
        # a window is whole calls of --steps rounds, as many as it takes to
        # fill --min-seconds: the rate spans two orders of magnitude between
        # the per-node loop and the kernel
        done, t0 = 0, time.perf_counter()
        while True:
            sim.start(n_rounds=args.steps)
            torch.cuda.synchronize()
            done += args.steps
            dt = time.perf_counter() - t0
            if dt >= args.min_seconds:
                break
        runs.append(round(done / dt, 3))
        rounds += done
    evals = rep.get_evaluation(True)
    assert len(evals) == rounds, (len(evals), rounds)
    best = max(runs)
    print(json.dumps({
        "config": f"mlp-57-100-2-{N_NODES}n-push-local-eval",
        "backend": sim.backend.name,
        "no_mlp_eval_kernel_env":
            os.environ.get("GOSSIPY_NO_MLP_EVAL_KERNEL") == "1",
        "steps": args.steps,
        "rounds_per_sec": best,
        "rounds_per_sec_runs": runs,
        "node_evals_per_sec": round(best * N_NODES, 0),
        "final_local_accuracy": round(float(evals[-1][1]["accuracy"]), 4),
    }), flush=True)


if __name__ == "__main__":
    main()
