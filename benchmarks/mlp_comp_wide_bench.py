"""Round throughput of compressed (partitioned / sampled) MLP gossip on
``tick_mlp_comp_wide_kernel``, which ``GOSSIPY_MLP_COMP_WIDE=1`` selects.

* 784-100-10, the MNIST-shaped MLP whose row misses the LDS kernel's budget:
  ``n_parts=4`` and ``sample_size=0.25`` under the knob, next to the plain
  wide tick (``tick_mlp_wide_kernel``) as the yardstick. There is no earlier
  GPU route for the two compressed rows.
* 57-100-2, which the LDS kernel takes: ``n_parts=4`` and
  ``sample_size=0.25`` on ``tick_mlp_comp_kernel`` and with the wide kernel
  forced. These rows say what the global-resident operands cost where LDS
  would do; no routing threshold rests on them.

Shape: 1000 nodes, delta 100, PUSH, MERGE_UPDATE, ``batch_size=32``;
synthetic data from ``make_synthetic_classification``, about 54 train rows
per node, a global evaluation set of 1000 rows sampled on a tenth of the
nodes each round.

Reports rounds/s per row: best of ``--repeat`` windows after ``--warmup``
rounds, a window being calls of ``--steps`` rounds, each ending in a device
synchronise, until ``--min-seconds`` have passed. The rows' windows
alternate, so drift of the machine hits all alike; every window is printed.
A run without a GPU fails: a CPU time says nothing here.

Prints one JSON line.

Usage: python benchmarks/mlp_comp_wide_bench.py [--steps 2] [--warmup 1]
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

N_NODES = 1000
KNOB = "GOSSIPY_MLP_COMP_WIDE"
SHAPES = {"784": (784, 10), "57": (57, 2)}
#: row -> (shape, MLPSpec fields, EngineConfig fields, knob value)
ROWS = {
    "784_plain_wide": ("784", {}, {}, "0"),
    "784_part4_wide": ("784", dict(n_parts=4), dict(n_parts=4), "1"),
    "784_samp025_wide": ("784", dict(sample_size=0.25), dict(sampled=True),
                         "1"),
    "57_part4_lds": ("57", dict(n_parts=4), dict(n_parts=4), "0"),
    "57_part4_wide": ("57", dict(n_parts=4), dict(n_parts=4), "1"),
    "57_samp025_lds": ("57", dict(sample_size=0.25), dict(sampled=True), "0"),
    "57_samp025_wide": ("57", dict(sample_size=0.25), dict(sampled=True),
                        "1"),
}


def _data(d_in, k, device):
    X, y = make_synthetic_classification((61 * N_NODES, d_in, k), seed=0,
                                         margin=2.0)
    idx = np.random.default_rng(0).permutation(len(y))
    cut = len(y) - 1000
    shards = [(X[s], y[s]) for s in np.array_split(idx[:cut], N_NODES)]
    return DataArena.from_shards(
        shards, device, global_eval=(X[idx[cut:]], y[idx[cut:]]))


def _sim(spec, cfg_kw, data, device):
    cfg = EngineConfig(
        n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.1, seed=42, **cfg_kw,
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
    data = {s: _data(d, k, device) for s, (d, k) in SHAPES.items()}
    sims, paths = {}, {}
    for name, (shape, kw, cfg_kw, knob) in ROWS.items():
        d, k = SHAPES[shape]
        spec = MLPSpec(d_in=d, n_classes=k, hidden=(100,), lr=0.1,
                       batch_size=32, **kw)
        os.environ[KNOB] = knob  # read by the extension at every launch
        sims[name] = _sim(spec, cfg_kw, data[shape], device)
        query = (sims[name].backend.mlp_comp_tick_path if kw
                 else sims[name].backend.mlp_tick_path)
        paths[name] = query(spec, data[shape])
        assert paths[name] == name.rsplit("_", 1)[1], (name, paths[name])
        sims[name].start(n_rounds=args.warmup)
        torch.cuda.synchronize()
    runs = {name: [] for name in sims}
    for _ in range(args.repeat):
        for name, sim in sims.items():
            os.environ[KNOB] = ROWS[name][3]
            runs[name].append(_window(sim, args.steps, args.min_seconds))
    out = {"config": f"mlp-comp-{N_NODES}n-push-bs32", "steps": args.steps,
           "tick_paths": paths}
    for name in sims:
        out[f"{name}_rounds_per_sec"] = max(runs[name])
        out[f"{name}_rounds_per_sec_runs"] = runs[name]
    for name in ("784_part4_wide", "784_samp025_wide"):
        out[f"{name}_over_plain"] = round(
            out[f"{name}_rounds_per_sec"]
            / out["784_plain_wide_rounds_per_sec"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
