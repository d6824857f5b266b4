"""Round throughput of MNIST-shaped logistic regression, 784x10, on the
batched engine:

* ``wide32``   ``LogRegSpec(784, 10, batch_size=32)``, which misses the LDS
  kernels' budget by 592 bytes and runs ``tick_logreg_wide_kernel``;
* ``torchmod`` the only GPU route that shape had before, ``TorchModuleSpec``
  wrapping the same module (node-batched vmap/autograd SGD);
* ``lds31`` / ``wide31``  ``batch_size=31``, which fits LDS, on the LDS
  kernels and with ``GOSSIPY_LOGREG_WIDE=1`` on the wide one.

Shape: 1000 nodes, delta 100, PUSH, MERGE_UPDATE; synthetic data from
``make_synthetic_classification((N, 784, 10))``, about 54 train rows per
node, a global evaluation set of 1000 rows sampled on a tenth of the nodes
each round.

Reports rounds/s per route: best of ``--repeat`` windows after ``--warmup``
rounds, a window being calls of ``--steps`` rounds, each ending in a device
synchronise, until ``--min-seconds`` have passed. The routes' windows
alternate, so drift of the machine hits all alike; every window is printed.
A run without a GPU fails: a CPU time says nothing here.

Prints one JSON line.

Usage: python benchmarks/logreg_wide_bench.py [--steps 2] [--warmup 1]
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
    LogRegSpec,
    TorchModuleSpec,
)
from gossipy_amd.simul import SimulationReport

N_NODES = 1000
D_IN, K = 784, 10
KNOB = "GOSSIPY_LOGREG_WIDE"


def _module():
    # LogRegSpec's model: softmax-CE on sigmoid(W x + b)
    return torch.nn.Sequential(torch.nn.Linear(D_IN, K), torch.nn.Sigmoid())


def _data(device):
    X, y = make_synthetic_classification((55 * N_NODES, D_IN, K), seed=0,
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


def _set_knob(value):
    # the extension reads the knob whenever it plans a launch
    if value is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = value


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

    def logreg(bs):
        return LogRegSpec(d_in=D_IN, n_classes=K, lr=0.1, batch_size=bs)

    # route -> (spec, knob value, expected tick path)
    routes = {
        "wide32": (logreg(32), None, "wide"),
        "torchmod": (TorchModuleSpec(_module, (D_IN,), lr=0.1, batch_size=32),
                     None, None),
        "lds31": (logreg(31), None, "lds"),
        "wide31": (logreg(31), "1", "wide"),
    }
    sims = {}
    for name, (spec, knob, want) in routes.items():
        _set_knob(knob)
        sims[name] = _sim(spec, data, device)
        if want:
            path = sims[name][0].backend.logreg_tick_path(spec, data)
            assert path == want, (name, path)
        sims[name][0].start(n_rounds=args.warmup)
        torch.cuda.synchronize()
    runs = {name: [] for name in sims}
    for _ in range(args.repeat):
        for name, (sim, _) in sims.items():
            _set_knob(routes[name][1])
            runs[name].append(_window(sim, args.steps, args.min_seconds))
    _set_knob(None)
    out = {
        "config": f"logreg-{D_IN}x{K}-{N_NODES}n-push",
        "steps": args.steps,
    }
    for name, (sim, rep) in sims.items():
        out[f"{name}_rounds_per_sec"] = max(runs[name])
        out[f"{name}_rounds_per_sec_runs"] = runs[name]
        out[f"{name}_accuracy"] = round(
            float(rep.get_evaluation(False)[-1][1]["accuracy"]), 4)
    out["wide32_over_torchmod"] = round(
        out["wide32_rounds_per_sec"] / out["torchmod_rounds_per_sec"], 3)
    out["wide31_over_lds31"] = round(
        out["wide31_rounds_per_sec"] / out["lds31_rounds_per_sec"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
