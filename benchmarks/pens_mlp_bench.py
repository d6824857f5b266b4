"""Engine throughput of PENS (Onoszko 2021) for the logreg and the MLP
family: rounds/s of step-1 rounds (candidate scoring + top-m merge events,
``tick_pens`` / ``tick_pens_mlp``) and of step-2 rounds (plain gossip over
the selected neighbours, the family's tick kernel).

Shape: 1000 nodes, delta 100, PUSH, ``n_sampled = 10``, ``m_top = 2`` (the
reference's main_onoszko_2021.py), batch size 32, on the dataset of
``benchmarks/config_bench.py`` (46 samples of 57 features per node);
logreg 57 -> 2, MLP 57 -> 100 -> 2 (the ``mlp_bench`` shape).

A node learns in step 1 only when its candidate cache is full, about once in
``n_sampled`` rounds, so every row first runs ``LEAD = 2 * n_sampled``
step-1 rounds: the caches fill and the events spread over the rounds (about
``n_nodes / n_sampled`` a round; each row reports the figure of its timed
rounds). A step-1 row keeps the step boundary beyond the timed rounds; a
step-2 row puts it right after the lead (the counts read and the neighbour
selection happen there), runs ``--warmup`` more rounds and times step-2
rounds alone.

Prints one JSON line per row. ``--repeat N`` times every row N times, each
on a fresh simulator, and reports every run, so the spread is visible.

Usage: python benchmarks/pens_mlp_bench.py [--steps 20] [--warmup 3]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

from config_bench import _data
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (
    BatchedPENSGossipSimulator,
    EngineConfig,
    LogRegSpec,
    MLPSpec,
)

N_NODES = 1000
N_SAMPLED = 10
M_TOP = 2
LEAD = 2 * N_SAMPLED  # step-1 rounds ahead of every measurement

ROWS = {
    "logreg-step1": ("logreg", 1),
    "logreg-step2": ("logreg", 2),
    "mlp-step1": ("mlp", 1),
    "mlp-step2": ("mlp", 2),
}


def _spec(family):
    if family == "logreg":
        return LogRegSpec(d_in=57, n_classes=2, lr=0.1, batch_size=32)
    return MLPSpec(d_in=57, n_classes=2, hidden=(100,), lr=0.05, batch_size=32)


def _sync(device):
    if device.type == "cuda":
        torch.cuda.synchronize()


def _timed(sim, step, steps, warmup, device):
    sim.init_nodes()
    sim.start(n_rounds=LEAD + warmup)
    assert (sim.scheduler.best_nodes is not None) == (step == 2)
    _sync(device)
    before = int(sim.counts.sum())
    t0 = time.perf_counter()
    sim.start(n_rounds=steps)
    _sync(device)
    dt = time.perf_counter() - t0
    # winner counters move in step 1 only: m_top per event
    events = (int(sim.counts.sum()) - before) // M_TOP
    return steps / dt, events / steps


def row(name, steps, warmup, repeat, device):
    family, step = ROWS[name]
    runs = []
    for _ in range(repeat):
        spec = _spec(family)
        cfg = EngineConfig(
            n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
            model_size=spec.D, sampling_eval=0.01, seed=42,
        )
        sim = BatchedPENSGossipSimulator(
            cfg, spec, _data(N_NODES, device), n_sampled=N_SAMPLED,
            m_top=M_TOP,
            step1_rounds=(LEAD + warmup + steps + 1) if step == 1 else LEAD,
            device=device,
        )
        rps, events = _timed(sim, step, steps, warmup, device)
        runs.append(round(rps, 2))
    best = max(runs)
    shape = "logreg-57x2" if family == "logreg" else "mlp-57-100-2"
    return {
        "config": f"pens-{shape}-{N_NODES}n-push-step{step}",
        "n_sampled": N_SAMPLED,
        "m_top": M_TOP,
        "backend": sim.backend.name,
        "pens_events_per_round": round(events, 1),
        "rounds_per_sec": best,
        "rounds_per_sec_runs": runs,
        "node_rounds_per_sec": round(best * N_NODES, 0),
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
