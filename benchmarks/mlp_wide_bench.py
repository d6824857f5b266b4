"""Round throughput of the MNIST-shaped MLP, 784-100-10, on the batched
engine: the global-resident wide tick kernel (``MLPSpec``, which the LDS
kernel cannot run at this size) against the only GPU route there was before
it, ``TorchModuleSpec`` wrapping the same three-layer module (node-batched
vmap/autograd SGD).

Shape: 1000 nodes, delta 100, PUSH, MERGE_UPDATE, ``batch_size=32``;
synthetic data from ``make_synthetic_classification((N, 784, 10))``, about
54 train rows per node, a global evaluation set of 1000 rows sampled on a
tenth of the nodes each round.

Reports rounds/s per route: best of ``--repeat`` windows after ``--warmup``
rounds, a window being calls of ``--steps`` rounds, each ending in a device
synchronise, until ``--min-seconds`` have passed. The two routes' windows
alternate, so drift of the machine hits both alike; every window is
printed. A run without a GPU fails: a CPU time says nothing here.

Prints one JSON line.

Usage: python benchmarks/mlp_wide_bench.py [--steps 2] [--warmup 1]
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
    TorchModuleSpec,
)
from gossipy_amd.simul import SimulationReport

N_NODES = 1000
D_IN, HIDDEN, K = 784, 100, 10


def _module():
    return torch.nn.Sequential(
        torch.nn.Linear(D_IN, HIDDEN), torch.nn.ReLU(),
        torch.nn.Linear(HIDDEN, K),
    )


def _data(device):
    X, y = make_synthetic_classification((61 * N_NODES, D_IN, K), seed=0,
                                         margin=2.0)
    idx = np.random.default_rng(0).permutation(len(y))
    cut = len(y) - 1000
    shards = [(X[s], y[s]) for s in np.array_split(idx[:cut], N_NODES)]
    return DataArena.from_shards(
        shards, device, global_eval=(X[idx[cut:]], y[idx[cut:]]))


def _sim(spec, data, device):
    cfg = EngineConfig(
        n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.1, seed=42,
    )
    sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    rep = SimulationReport()
    sim.add_receiver(rep)
    sim.init_nodes()
    return sim, rep


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
    data = _data(device)
    routes = {
        "mlp_wide": MLPSpec(d_in=D_IN, n_classes=K, hidden=(HIDDEN,), lr=0.1,
                            batch_size=32),
        "torchmod": TorchModuleSpec(_module, (D_IN,), lr=0.1, batch_size=32),
    }
    sims = {name: _sim(spec, data, device) for name, spec in routes.items()}
    path = sims["mlp_wide"][0].backend.mlp_tick_path(routes["mlp_wide"], data)
    assert path == "wide", path
    for sim, _ in sims.values():
        sim.start(n_rounds=args.warmup)
        torch.cuda.synchronize()
    runs = {name: [] for name in sims}
    for _ in range(args.repeat):
        for name, (sim, _) in sims.items():
            runs[name].append(_window(sim, args.steps, args.min_seconds))
    out = {
        "config": f"mlp-{D_IN}-{HIDDEN}-{K}-{N_NODES}n-push-bs32",
        "tick_path": path,
        "steps": args.steps,
    }
    for name, (sim, rep) in sims.items():
        out[f"{name}_rounds_per_sec"] = max(runs[name])
        out[f"{name}_rounds_per_sec_runs"] = runs[name]
        out[f"{name}_accuracy"] = round(
            float(rep.get_evaluation(False)[-1][1]["accuracy"]), 4)
    out["wide_over_torchmod"] = round(
        out["mlp_wide_rounds_per_sec"] / out["torchmod_rounds_per_sec"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
