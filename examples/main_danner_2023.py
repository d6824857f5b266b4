"""Danner et al. 2023 — limited-divergence merge gossip.

Equivalent of the reference's main_danner_2023.py (100 nodes,
LimitedMergeTMH logistic regression: if the age gap exceeds L keep the
newer model, else age-weighted average — gossipy/model/handler.py:690-739).
Synthetic spambase-shaped data. The default invocation runs the object
layer (LimitedMergeTMH handlers, one python object per node); ``--engine``
runs the same experiment on the batched engine, where the rule is the
``age_diff_threshold`` field of the spec and executes inside the HIP tick
kernels, so it scales to the node counts the other engine examples reach.
``--model mlp`` (engine only) swaps the logistic regression for an MLP with
``--hidden`` widths; ``--L`` sets the age-gap threshold.
"""

import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import argparse

import torch

from gossipy_amd import set_seed
from gossipy_amd.core import AntiEntropyProtocol, CreateModelMode, StaticP2PNetwork
from gossipy_amd.data import DataDispatcher, make_synthetic_classification
from gossipy_amd.data.handler import ClassificationDataHandler
from gossipy_amd.model.handler import LimitedMergeTMH
from gossipy_amd.model.nn import LogisticRegression
from gossipy_amd.node import GossipNode
from gossipy_amd.simul import GossipSimulator, SimulationReport


def run_engine(args):
    import numpy as np

    from gossipy_amd.engine import (
        BatchedGossipSimulator,
        DataArena,
        EngineConfig,
        LogRegSpec,
        MLPSpec,
    )

    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    n, d = args.nodes, 57
    X, y = make_synthetic_classification((46 * n, d, 2), seed=42, margin=2.0)
    idx = np.random.default_rng(42).permutation(len(y))
    cut = int(0.9 * len(y))
    shards = [(X[s], y[s]) for s in np.array_split(idx[:cut], n)]
    data = DataArena.from_shards(
        shards, device, global_eval=(X[idx[cut:]], y[idx[cut:]])
    )
    if args.model == "mlp":
        spec = MLPSpec(
            d_in=d, n_classes=2, hidden=tuple(args.hidden), lr=0.1,
            age_diff_threshold=args.L,
        )
    else:
        spec = LogRegSpec(
            d_in=d, n_classes=2, lr=0.1, age_diff_threshold=args.L
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
    report = SimulationReport()
    sim.add_receiver(report)
    sim.init_nodes()
    sim.start(n_rounds=args.rounds)
    print(f"final global eval: {report.get_evaluation(False)[-1][1]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument(
        "--engine", action="store_true",
        help="run on the batched engine (cuda:0 when available, else CPU)",
    )
    ap.add_argument("--model", choices=("logreg", "mlp"), default="logreg")
    ap.add_argument(
        "--hidden", type=int, nargs="+", default=[100],
        help="hidden layer widths of the MLP (--engine --model mlp)",
    )
    ap.add_argument("--L", type=int, default=10, help="age-gap threshold")
    args = ap.parse_args()

    if args.engine:
        run_engine(args)
        return
    if args.model != "logreg":
        ap.error("--model mlp needs --engine")

    set_seed(98765)
    X, y = make_synthetic_classification((46 * args.nodes, 57, 2), seed=42, margin=2.0)
    handler = ClassificationDataHandler(X, y, test_size=0.1, seed=42)
    dispatcher = DataDispatcher(handler, n=args.nodes, eval_on_user=False)

    topology = StaticP2PNetwork(args.nodes)
    nodes = GossipNode.generate(
        data_dispatcher=dispatcher,
        p2p_net=topology,
        model_proto=LimitedMergeTMH(
            net=LogisticRegression(57, 2),
            optimizer=torch.optim.SGD,
            optimizer_params={"lr": 0.1},
            criterion=torch.nn.CrossEntropyLoss(),
            create_model_mode=CreateModelMode.MERGE_UPDATE,
            age_diff_threshold=args.L,
        ),
        round_len=100,
        sync=False,
    )
    simulator = GossipSimulator(
        nodes=nodes,
        data_dispatcher=dispatcher,
        delta=100,
        protocol=AntiEntropyProtocol.PUSH,
        sampling_eval=0.1,
    )
    report = SimulationReport()
    simulator.add_receiver(report)
    simulator.init_nodes(seed=42)
    simulator.start(n_rounds=args.rounds)
    print(f"final global eval: {report.get_evaluation(False)[-1][1]}")


if __name__ == "__main__":
    main()
