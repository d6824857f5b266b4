"""Engine throughput of compressed MLP gossip (Hegedus 2021's two schemes
on the MLP family).

Rows 1-3 run the ``mlp_bench`` shape of ``benchmarks/config_bench.py``
(57 -> 100 -> 2 MLP, 1000 nodes, delta 100, PUSH, batch size 32) three ways:
plain, partitioned (``n_parts=4``) and sampled (``sample_size=0.25``).
Row 4 is the tokenized Hegedus-2021 row of ``config_bench.py`` (100 nodes,
20-regular graph, RandomizedTokenAccount(C=20, A=10), UPDATE, 4 partitions)
with the MLP in place of logistic regression.

Prints one JSON line per row. No CPU-reference speed-up is quoted: the
reference has not been measured on these rows.

Usage: python benchmarks/mlp_compress_bench.py [--steps 20] [--warmup 3]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

from config_bench import _data, timed
from examples.main_hegedus_2021 import k_regular_csr
from gossipy_amd.core import AntiEntropyProtocol, CreateModelMode
from gossipy_amd.engine import (
    BatchedGossipSimulator,
    BatchedTokenizedGossipSimulator,
    EngineConfig,
    MLPSpec,
)
from gossipy_amd.flow_control import RandomizedTokenAccount

VARIANTS = {
    "plain": (dict(), dict()),
    "partitioned-4": (dict(n_parts=4), dict(n_parts=4)),
    "sampled-0.25": (dict(sample_size=0.25), dict(sampled=True)),
}


def gossip_row(name, steps, warmup, device):
    spec_kw, cfg_kw = VARIANTS[name]
    spec = MLPSpec(
        d_in=57, n_classes=2, hidden=(100,), lr=0.05, batch_size=32, **spec_kw
    )
    cfg = EngineConfig(
        n_nodes=1000, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.01, seed=42, **cfg_kw,
    )
    sim = BatchedGossipSimulator(cfg, spec, _data(1000, device), device=device)
    r = timed(sim, steps, warmup, device)
    return {
        "config": f"giaretta-shaped-mlp-57-100-2-1000n-{name}",
        "mode": spec.mode.name,
        "backend": sim.backend.name,
        "fast_path": bool(sim._fast_path_ok()),
        "rounds_per_sec": round(r, 2),
        "node_rounds_per_sec": round(r * 1000, 0),
    }


def tokenized_row(steps, warmup, device):
    indptr, indices = k_regular_csr(100, 20)
    spec = MLPSpec(
        d_in=57, n_classes=2, hidden=(100,), lr=0.1, batch_size=32, n_parts=4,
        mode=CreateModelMode.UPDATE,
    )
    cfg = EngineConfig(
        n_nodes=100, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.1, seed=42, n_parts=4,
        peers_indptr=indptr, peers_indices=indices,
    )
    sim = BatchedTokenizedGossipSimulator(
        cfg, spec, _data(100, device),
        token_account=RandomizedTokenAccount(C=20, A=10),
        utility_fun=1,  # constant utility -> native tokenized scheduler
        device=device,
    )
    r = timed(sim, steps, warmup, device)
    return {
        "config": "hegedus2021-tokenized-partitioned-mlp-57-100-2-100n-20regular",
        "mode": spec.mode.name,
        "backend": sim.backend.name,
        "fast_path": bool(sim._fast_path_ok()),
        "rounds_per_sec": round(r, 2),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument(
        "--rows", nargs="+", default=[*VARIANTS, "tokenized"],
        choices=[*VARIANTS, "tokenized"],
    )
    args = ap.parse_args()
    device = torch.device("cuda:0" if torch.cuda.is_available() else "cpu")
    for row in args.rows:
        if row == "tokenized":
            out = tokenized_row(args.steps, args.warmup, device)
        else:
            out = gossip_row(row, args.steps, args.warmup, device)
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
