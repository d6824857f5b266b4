"""Round throughput of Hungarian-matched k-means gossip on its two GPU
routes, next to naive matching.

Rows per shape, ``k=16, dim=32`` and ``k=64, dim=8``:

* ``naive``: ``tick_kmeans_kernel``, the plain centroid mean, as the
  yardstick of what a k-means tick costs without any matching;
* ``host``: ``GOSSIPY_KMEANS_MATCH_KERNEL=0``, per delivery wave a device
  cdist, scipy's assignment on the host and the update kernel;
* ``kernel``: ``GOSSIPY_KMEANS_MATCH_KERNEL=1``, ``tick_kmeans_match_kernel``,
  one launch per tick.

Shape: 1000 nodes, delta 100, PUSH, MERGE_UPDATE; Gaussian blobs around k
centres, 30 rows per node, no evaluation (the rounds are all gossip).

Reports rounds/s per row: best of ``--repeat`` windows after ``--warmup``
rounds, a window being calls of ``--steps`` rounds, each ending in a device
synchronise, until ``--min-seconds`` have passed. The rows' windows
alternate, so drift of the machine hits all alike; every window is printed.
A run without a GPU fails: a CPU time says nothing here.

Prints one JSON line.

Usage: python benchmarks/kmeans_match_bench.py [--steps 2] [--warmup 1]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gossipy_amd.core import AntiEntropyProtocol, CreateModelMode
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    KMeansSpec,
)

N_NODES = 1000
KNOB = "GOSSIPY_KMEANS_MATCH_KERNEL"
SHAPES = {"k16d32": (16, 32), "k64d8": (64, 8)}
#: route -> (matching, knob value)
ROUTES = {"naive": ("naive", "0"), "host": ("hungarian", "0"),
          "kernel": ("hungarian", "1")}


def _data(k, dim, device):
    rng = np.random.default_rng(0)
    centers = rng.normal(0, 4, size=(k, dim))
    shards = []
    for _ in range(N_NODES):
        lb = rng.integers(0, k, size=30)
        x = centers[lb] + rng.normal(0, 0.4, size=(30, dim))
        shards.append((torch.from_numpy(x).float(),
                       torch.from_numpy(lb).float()))
    return DataArena.from_shards(shards, device)


def _sim(spec, data, device):
    cfg = EngineConfig(
        n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.0, seed=42,
    )
    sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    sim.init_nodes()
    return sim


def _window(sim, steps, min_seconds):
    done, t0 = 0, time.perf_counter()
    while True:
        sim.start(n_rounds=steps)
        torch.cuda.synchronize()
        done += steps
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            return round(done / dt, 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    device = torch.device("cuda:0")
    sims, knobs, paths = {}, {}, {}
    for shape, (k, dim) in SHAPES.items():
        data = _data(k, dim, device)
        for route, (matching, knob) in ROUTES.items():
            name = f"{shape}_{route}"
            spec = KMeansSpec(k=k, dim=dim, alpha=0.1, matching=matching,
                              mode=CreateModelMode.MERGE_UPDATE)
            os.environ[KNOB] = knobs[name] = knob  # read at every delivery
            sims[name] = _sim(spec, data, device)
            if matching == "hungarian":
                paths[name] = sims[name].backend.kmeans_match_path(spec, data)
                assert paths[name] == route, (name, paths[name])
            sims[name].start(n_rounds=args.warmup)
            torch.cuda.synchronize()
    runs = {name: [] for name in sims}
    for _ in range(args.repeat):
        for name, sim in sims.items():
            os.environ[KNOB] = knobs[name]
            runs[name].append(_window(sim, args.steps, args.min_seconds))
    out = {"config": f"kmeans-match-{N_NODES}n-push-merge_update",
           "steps": args.steps, "match_paths": paths}
    for name in sims:
        out[f"{name}_rounds_per_sec"] = max(runs[name])
        out[f"{name}_rounds_per_sec_runs"] = runs[name]
    for shape in SHAPES:
        out[f"{shape}_kernel_over_host"] = round(
            out[f"{shape}_kernel_rounds_per_sec"]
            / out[f"{shape}_host_rounds_per_sec"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
