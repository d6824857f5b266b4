"""MNIST-shaped logistic-regression gossip on the batched engine.

``LogRegSpec(784, 10)`` with minibatches of 32 needs 164,432 bytes for the
LDS-resident logreg kernels, 592 more than one workgroup has. On the GPU its
plain tick therefore runs the wide kernel (``tick_logreg_wide_kernel``: one
model row in LDS, the minibatch streamed from the data arena through MFMA
tiles); on a CPU-only machine the same script runs the TorchBackend oracle.
Synthetic MNIST-shaped data (784 features, 10 classes).

``--batch-size`` sets the minibatch (31 still fits the LDS kernels),
``--mode`` the CreateModelMode. The script prints the tick path the
configuration gets and the last global evaluation.

``--pens`` runs PENS neighbour selection (``BatchedPENSGossipSimulator``) on
the same data with minibatches of 64 unless ``--batch-size`` says otherwise:
from there on the step-1 event misses the LDS plan of ``tick_pens_kernel``
(``4 * (D + rows * 784 + rows * 10)`` bytes; 32 rows still fit) and runs
``tick_pens_wide_kernel``, which scores all candidates in one MFMA GEMM. The
script then prints the PENS event path as well.

``--eval-rank`` sets ``GOSSIPY_EVAL_RANK=1``: the shared eval set is measured
by the chunk-sorted kernels (``eval_metrics_rank``), which take any number of
rows; the script prints the evaluation path either way.
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
    BatchedPENSGossipSimulator,
    DataArena,
    EngineConfig,
    LogRegSpec,
)
from gossipy_amd.simul import SimulationReport

MODES = {m.name.lower(): m for m in CreateModelMode}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=None,
                    help="default 32, or 64 with --pens")
    ap.add_argument("--mode", choices=sorted(MODES), default="merge_update")
    ap.add_argument("--pens", action="store_true",
                    help="PENS neighbour selection (MERGE_UPDATE only)")
    ap.add_argument("--eval-rank", action="store_true",
                    help="chunk-sorted evaluation kernels at any eval-set"
                         " size (sets GOSSIPY_EVAL_RANK=1)")
    args = ap.parse_args()
    if args.batch_size is None:
        args.batch_size = 64 if args.pens else 32
    if args.eval_rank:
        os.environ["GOSSIPY_EVAL_RANK"] = "1"

    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    n, d, k = args.nodes, 784, 10
    X, y = make_synthetic_classification((60 * n, d, k), seed=42, margin=2.0)
    idx = np.random.default_rng(42).permutation(len(y))
    cut = int(0.9 * len(y))
    shards = [(X[s], y[s]) for s in np.array_split(idx[:cut], n)]
    data = DataArena.from_shards(
        shards, device, global_eval=(X[idx[cut:]], y[idx[cut:]])
    )
    spec = LogRegSpec(
        d_in=d, n_classes=k, lr=0.1, batch_size=args.batch_size,
        mode=MODES[args.mode],
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
    if args.pens:
        sim = BatchedPENSGossipSimulator(
            cfg, spec, data, n_sampled=4, m_top=2,
            step1_rounds=max(1, args.rounds // 2), device=device,
        )
    else:
        sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    hip = sim.backend.name == "hip"
    path = sim.backend.logreg_tick_path(spec, data) if hip else "torch (no GPU)"
    print(f"logreg {d}x{k}, batch {args.batch_size}: tick path {path}")
    if args.pens:
        path = sim.backend.pens_tick_path(spec, data) if hip else "torch (no GPU)"
        print(f"pens_tick_path {path}")
    if hip:
        n_eval = data.gx.shape[0]
        print(f"eval_metrics_path ({n_eval} rows)"
              f" {sim.backend.eval_metrics_path(spec, n_eval)}")
    report = SimulationReport()
    sim.add_receiver(report)
    sim.init_nodes()
    sim.start(n_rounds=args.rounds)
    print(f"final global eval: {report.get_evaluation(False)[-1][1]}")


if __name__ == "__main__":
    main()
