"""Engine throughput of limited-merge gossip (Danner 2023) next to the plain
mean merge.

Two shapes, each run plain and with ``age_diff_threshold = 10`` (the
threshold of the reference's main_danner_2023.py):

* the flagship logreg config of ``bench.py`` (1000 nodes, d = 57, k = 2,
  PUSH, delta 100, batch size 32, on the flagship's dataset: 4601 samples
  over 1000 nodes, so four or five rows and one SGD step per update);
* the ``mlp_bench`` shape of ``benchmarks/config_bench.py`` (57 -> 100 -> 2
  MLP, 1000 nodes, delta 100, PUSH, batch size 32).

Prints one JSON line per row. ``--repeat N`` times every row N times, each
on a fresh simulator, and reports every run, so the spread is visible.

Usage: python benchmarks/limited_merge_bench.py [--steps 20] [--warmup 3]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from config_bench import _data, timed
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
    MLPSpec,
)

L_DANNER = 10

ROWS = {
    "logreg-plain": ("logreg", None),
    "logreg-limited": ("logreg", L_DANNER),
    "mlp-plain": ("mlp", None),
    "mlp-limited": ("mlp", L_DANNER),
}


def _flagship_data(device):
    """The dataset of ``bench.py`` at one GPU: 4601 spambase-shaped samples,
    seed 7, 256 of them the global eval set, the rest split over 1000
    nodes."""
    X, y = make_synthetic_classification((4601, 57, 2), seed=7)
    idx = np.random.default_rng(7).permutation(4601)
    eval_idx, train_idx = idx[:256], idx[256:]
    shards = [(X[s], y[s]) for s in np.array_split(train_idx, 1000)]
    return DataArena.from_shards(
        shards, device, global_eval=(X[eval_idx], y[eval_idx])
    )


def _spec(family, L):
    if family == "logreg":
        return LogRegSpec(
            d_in=57, n_classes=2, lr=0.1, local_epochs=1, batch_size=32,
            age_diff_threshold=L,
        )
    return MLPSpec(
        d_in=57, n_classes=2, hidden=(100,), lr=0.05, batch_size=32,
        age_diff_threshold=L,
    )


def row(name, steps, warmup, repeat, device):
    family, L = ROWS[name]
    runs = []
    for _ in range(repeat):
        spec = _spec(family, L)
        cfg = EngineConfig(
            n_nodes=1000, delta=100, protocol=AntiEntropyProtocol.PUSH,
            model_size=spec.D, sampling_eval=0.01, seed=42,
        )
        data = (
            _flagship_data(device) if family == "logreg"
            else _data(1000, device)
        )
        sim = BatchedGossipSimulator(cfg, spec, data, device=device)
        runs.append(round(timed(sim, steps, warmup, device), 2))
    best = max(runs)
    shape = "logreg-57x2" if family == "logreg" else "mlp-57-100-2"
    return {
        "config": f"{shape}-1000n-push-{'L%d' % L if L is not None else 'plain'}",
        "age_diff_threshold": L,
        "backend": sim.backend.name,
        "fast_path": bool(sim._fast_path_ok()),
        "rounds_per_sec": best,
        "rounds_per_sec_runs": runs,
        "node_rounds_per_sec": round(best * 1000, 0),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--rows", nargs="+", default=list(ROWS), choices=list(ROWS))
    args = ap.parse_args()
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    for name in args.rows:
        print(
            json.dumps(row(name, args.steps, args.warmup, args.repeat, device)),
            flush=True,
        )


if __name__ == "__main__":
    main()
