"""MNIST-shaped MLP gossip on the batched engine.

The canonical decentralised-learning classifier, 784-100-10, has 79,510
parameters: 318 KB per model row, twice one workgroup's LDS. On the GPU the
plain MLP tick therefore runs the global-resident wide kernel
(``tick_mlp_wide_kernel``: rows in device memory, the minibatch read from
the data arena); on a CPU-only machine the same script runs the TorchBackend
oracle. Synthetic MNIST-shaped data (784 features, 10 classes).

Evaluation on per-node test shards (``--test-shards``) follows the same
split: past the budget every evaluated node's own test split is forwarded by
``eval_mlp_wide_kernel`` (a row-blocked MFMA forward that streams the
weights through LDS) in place of a per-node Python loop.

``--pens`` runs PENS neighbour selection (``BatchedPENSGossipSimulator``) on
the same data. The LDS kernel of the step-1 event cannot hold a 784-100-10
row, so the script selects the wide route (``GOSSIPY_PENS_MLP_WIDE=1``
unless the variable is already set): ``pens_mlp_score_kernel`` forwards every
candidate of every event over a (row block, candidate) grid, and
``tick_pens_mlp_wide_kernel`` selects, merges and updates. The script then
prints the PENS event path as well.

``--n-parts P`` and ``--sample-size F`` run partitioned and sampled gossip
(Hegedűs 2021). Their LDS kernel cannot hold a 784-100-10 row either, so the
script selects ``tick_mlp_comp_wide_kernel`` (``GOSSIPY_MLP_COMP_WIDE=1``
unless the variable is already set), which works on the rows in device
memory, merges a partition as coalesced column bands and a sample behind an
LDS bitmap. The tick path printed is then that of the compressed tick.

``--hidden`` sets the hidden widths, ``--mode`` the CreateModelMode,
``--test-shards`` gives every node a test split of its own in place of the
shared set. The script prints the tick path the configuration gets and the
last global (or, with ``--test-shards``, local) evaluation.
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
    ap.add_argument(
        "--test-shards", action="store_true",
        help="evaluate every node on a test split of its own (a tenth of"
             " its rows) instead of one shared set",
    )
    ap.add_argument("--pens", action="store_true",
                    help="PENS neighbour selection (MERGE_UPDATE only), on"
                         " the wide route of the step-1 event")
    ap.add_argument("--n-parts", type=int, default=0, metavar="P",
                    help="partitioned gossip over P partitions, on the wide"
                         " compressed kernel")
    ap.add_argument("--sample-size", type=float, default=0.0, metavar="F",
                    help="sampled gossip over a fraction F of the parameters,"
                         " on the wide compressed kernel")
    args = ap.parse_args()
    comp = args.n_parts > 0 or args.sample_size > 0
    if comp and args.pens:
        ap.error("--pens needs whole-model gossip")
    if args.pens:
        os.environ.setdefault("GOSSIPY_PENS_MLP_WIDE", "1")
    if comp:
        os.environ.setdefault("GOSSIPY_MLP_COMP_WIDE", "1")

    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    n, d, k = args.nodes, 784, 10
    X, y = make_synthetic_classification((60 * n, d, k), seed=42, margin=2.0)
    idx = np.random.default_rng(42).permutation(len(y))
    cut = int(0.9 * len(y))
    if args.test_shards:
        parts = np.array_split(idx, n)
        cuts = [int(0.9 * len(s)) for s in parts]
        shards = [(X[s[:c]], y[s[:c]]) for s, c in zip(parts, cuts)]
        tests = [(X[s[c:]], y[s[c:]]) for s, c in zip(parts, cuts)]
        data = DataArena.from_shards(shards, device, test_shards=tests)
    else:
        shards = [(X[s], y[s]) for s in np.array_split(idx[:cut], n)]
        data = DataArena.from_shards(
            shards, device, global_eval=(X[idx[cut:]], y[idx[cut:]])
        )
    spec = MLPSpec(
        d_in=d, n_classes=k, hidden=tuple(args.hidden), lr=0.1,
        batch_size=32, mode=MODES[args.mode], n_parts=args.n_parts,
        sample_size=args.sample_size,
    )
    cfg = EngineConfig(
        n_nodes=n,
        delta=100,
        protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D,
        sync=False,
        sampling_eval=0.1,
        seed=42,
        n_parts=args.n_parts,
        sampled=args.sample_size > 0,
    )
    if args.pens:
        sim = BatchedPENSGossipSimulator(
            cfg, spec, data, n_sampled=4, m_top=2,
            step1_rounds=max(1, args.rounds // 2), device=device,
        )
    else:
        sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    hip = sim.backend.name == "hip"
    if not hip:
        path = "torch (no GPU)"
    elif comp:
        path = sim.backend.mlp_comp_tick_path(spec, data)
    else:
        path = sim.backend.mlp_tick_path(spec, data)
    print(f"MLP {'-'.join(map(str, spec.dims))}, D = {spec.D}: tick path {path}")
    if args.pens:
        path = sim.backend.pens_tick_path(spec, data) if hip else "torch (no GPU)"
        print(f"pens_tick_path {path}")
    report = SimulationReport()
    sim.add_receiver(report)
    sim.init_nodes()
    sim.start(n_rounds=args.rounds)
    if args.test_shards:
        if sim.backend.name == "hip":
            how = sim.backend.mlp_eval_path(spec, data.tx.shape[1])
            print(f"local evaluation path: {how}")
        print(f"final local eval: {report.get_evaluation(True)[-1][1]}")
    else:
        print(f"final global eval: {report.get_evaluation(False)[-1][1]}")


if __name__ == "__main__":
    main()
