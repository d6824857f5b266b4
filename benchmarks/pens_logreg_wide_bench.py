"""Step-1 round throughput of PENS (Onoszko 2021) on MNIST-shaped logistic
regression, 784x10, on the batched engine:

* ``wide_full``  ``LogRegSpec(784, 10, batch_size=0)``: full-batch shards of
  about 54 rows miss the LDS plan of ``tick_pens_kernel`` and run
  ``tick_pens_wide_kernel``;
* ``torchmod_full``  the only GPU route that shape had before,
  ``TorchModuleSpec`` wrapping the same module (vmap candidate scoring,
  autograd SGD);
* ``lds32`` / ``wide32``  ``batch_size=32``, which fits the LDS plan, on
  ``tick_pens_kernel`` and with ``GOSSIPY_LOGREG_WIDE=1`` on the wide kernel.

Shape: 1000 nodes, delta 100, PUSH, ``n_sampled = 10``, ``m_top = 2``, the
data of ``logreg_wide_bench.py``. As in ``pens_mlp_bench.py`` every route
first runs ``LEAD = 2 * n_sampled`` step-1 rounds, so the candidate caches
are full and the events (about ``n_nodes / n_sampled`` a round) spread over
the rounds; the step boundary lies beyond every timed round.

Reports rounds/s per route: best of ``--repeat`` windows after the lead and
``--warmup`` rounds, a window being calls of ``--steps`` rounds, each ending
in a device synchronise, until ``--min-seconds`` have passed. The routes'
windows alternate; every window is printed. A run without a GPU fails.

Prints one JSON line.

Usage: python benchmarks/pens_logreg_wide_bench.py [--steps 2] [--warmup 1]
"""

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch

from logreg_wide_bench import D_IN, K, N_NODES, _data, _module, _set_knob
from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.engine import (
    BatchedPENSGossipSimulator,
    EngineConfig,
    LogRegSpec,
    TorchModuleSpec,
)

N_SAMPLED = 10
M_TOP = 2
LEAD = 2 * N_SAMPLED  # step-1 rounds ahead of every measurement


def _sim(spec, data, device):
    cfg = EngineConfig(
        n_nodes=N_NODES, delta=100, protocol=AntiEntropyProtocol.PUSH,
        model_size=spec.D, sampling_eval=0.01, seed=42,
    )
    sim = BatchedPENSGossipSimulator(
        cfg, spec, data, n_sampled=N_SAMPLED, m_top=M_TOP,
        step1_rounds=10 ** 6, device=device,
    )
    sim.init_nodes()
    return sim


def _window(sim, steps, min_seconds):
    """``(rounds/s, PENS events per round)`` of one timed window."""
    before = int(sim.counts.sum())
    done, t0 = 0, time.perf_counter()
    while True:
        sim.start(n_rounds=steps)
        torch.cuda.synchronize()
        done += steps
        dt = time.perf_counter() - t0
        if dt >= min_seconds:
            break
    # winner counters move m_top per event
    events = (int(sim.counts.sum()) - before) / M_TOP / done
    return round(done / dt, 3), round(events, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--routes", nargs="+", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this benchmark needs a GPU"
    device = torch.device("cuda:0")
    data = _data(device)

    def logreg(bs):
        return LogRegSpec(d_in=D_IN, n_classes=K, lr=0.1, batch_size=bs)

    # route -> (spec, knob value, expected PENS event path)
    routes = {
        "wide_full": (logreg(0), None, "wide"),
        "torchmod_full": (
            TorchModuleSpec(_module, (D_IN,), lr=0.1, batch_size=0), None, None),
        "lds32": (logreg(32), None, "lds"),
        "wide32": (logreg(32), "1", "wide"),
    }
    if args.routes:
        routes = {name: routes[name] for name in args.routes}
    sims, events = {}, {}
    for name, (spec, knob, want) in routes.items():
        _set_knob(knob)
        sims[name] = sim = _sim(spec, data, device)
        if want:
            path = sim.backend.pens_tick_path(spec, data)
            assert path == want, (name, path)
        sim.start(n_rounds=LEAD + args.warmup)
        torch.cuda.synchronize()
        assert sim.scheduler.best_nodes is None  # still step 1
    runs = {name: [] for name in sims}
    for _ in range(args.repeat):
        for name, sim in sims.items():
            _set_knob(routes[name][1])
            rps, events[name] = _window(sim, args.steps, args.min_seconds)
            runs[name].append(rps)
    _set_knob(None)
    out = {
        "config": f"pens-logreg-{D_IN}x{K}-{N_NODES}n-push-step1",
        "n_sampled": N_SAMPLED, "m_top": M_TOP, "steps": args.steps,
    }
    for name in sims:
        out[f"{name}_rounds_per_sec"] = max(runs[name])
        out[f"{name}_rounds_per_sec_runs"] = runs[name]
        out[f"{name}_pens_events_per_round"] = events[name]
    if "wide_full" in sims and "torchmod_full" in sims:
        out["wide_full_over_torchmod_full"] = round(
            out["wide_full_rounds_per_sec"]
            / out["torchmod_full_rounds_per_sec"], 3)
    if "wide32" in sims and "lds32" in sims:
        out["wide32_over_lds32"] = round(
            out["wide32_rounds_per_sec"] / out["lds32_rounds_per_sec"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
