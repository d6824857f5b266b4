"""MNIST-shaped MLP gossip on the batched engine.

The canonical decentralised-learning classifier, 784-100-10, has 79,510
parameters: 318 KB per model row, twice one workgroup's LDS. On the GPU the
plain MLP tick therefore runs the global-resident wide kernel
(``tick_mlp_wide_kernel``: rows in device memory, the minibatch read from
the data arena); on a CPU-only machine the same script runs the TorchBackend
oracle. Synthetic MNIST-shaped data (784 features, 10 classes).

``--hidden`` sets the hidden widths, ``--mode`` the CreateModelMode. The
script prints the tick path the configuration gets and the last global
evaluation.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import argparse

import numpy as np
import torch

from gossipy_amd.core import AntiEntropyProtocol, CreateModelMode
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    DataArena,
    EngineConfig,
    MLPSpec,
)
from gossipy_amd.simul import SimulationReport

MODES = {m.name.lower(): m for m in CreateModelMode}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument(
        "--hidden", type=int, nargs="*", default=[100],
        help="hidden layer widths (none: a linear softmax classifier)",
    )
    ap.add_argument("--mode", choices=sorted(MODES), default="merge_update")
    args = ap.parse_args()

    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    n, d, k = args.nodes, 784, 10
    X, y = make_synthetic_classification((60 * n, d, k), seed=42, margin=2.0)
    idx = np.random.default_rng(42).permutation(len(y))
    cut = int(0.9 * len(y))
    shards = [(X[s], y[s]) for s in np.array_split(idx[:cut], n)]
    data = DataArena.from_shards(
        shards, device, global_eval=(X[idx[cut:]], y[idx[cut:]])
    )
    spec = MLPSpec(
        d_in=d, n_classes=k, hidden=tuple(args.hidden), lr=0.1,
        batch_size=32, mode=MODES[args.mode],
    )
    cfg = EngineConfig(
        n_nodes=n,
        delta=100,
        protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D,
        sync=False,
        sampling_eval=0.1,
        seed=42,
    )
    sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    if sim.backend.name == "hip":
        path = sim.backend.mlp_tick_path(spec, data)
    else:
        path = "torch (no GPU)"
    print(f"MLP {'-'.join(map(str, spec.dims))}, D = {spec.D}: tick path {path}")
    report = SimulationReport()
    sim.add_receiver(report)
    sim.init_nodes()
    sim.start(n_rounds=args.rounds)
    print(f"final global eval: {report.get_evaluation(False)[-1][1]}")


if __name__ == "__main__":
    main()
