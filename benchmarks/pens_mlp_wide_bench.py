"""Step-1 round throughput of PENS (Onoszko 2021) for the MLP family on the
batched engine, with the wide route of ``tick_pens_mlp``
(``pens_mlp_score_kernel`` + ``tick_pens_mlp_wide_kernel``, selected by
``GOSSIPY_PENS_MLP_WIDE=1``):

* ``wide``  ``MLPSpec(784, 10, (100,), batch_size=32)`` under the knob: the
  MNIST-shaped MLP, whose row alone misses the LDS plan of
  ``tick_pens_mlp_kernel``;
* ``torchmod``  the only GPU route that shape had before, ``TorchModuleSpec``
  wrapping the same module (vmap candidate scoring, autograd SGD);
* ``lds_small`` / ``wide_small``  ``MLPSpec(57, 2, (16,), batch_size=32)``,
  which fits the LDS plan, on ``tick_pens_mlp_kernel`` and under the knob.

Shape: 1000 nodes, delta 100, PUSH, ``n_sampled = 10``, ``m_top = 2``, about
54 rows per node (the data of ``mlp_wide_bench.py``, and the same recipe at
57 features and 2 classes). As in ``pens_mlp_bench.py`` every route first
runs ``LEAD = 2 * n_sampled`` step-1 rounds, so the candidate caches are full
and the events (about ``n_nodes / n_sampled`` a round) spread over the
rounds; the step boundary lies beyond every timed round.

Reports rounds/s per route: best of ``--repeat`` windows after the lead and
``--warmup`` rounds, a window being calls of ``--steps`` rounds, each ending
in a device synchronise, until ``--min-seconds`` have passed. The routes'
windows alternate; every window is printed. A run without a GPU fails.

Prints one JSON line.

Usage: python benchmarks/pens_mlp_wide_bench.py [--steps 2] [--warmup 1]
"""

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import numpy as np
import torch

from mlp_wide_bench import D_IN, HIDDEN, K, N_NODES, _data, _module
from pens_logreg_wide_bench import LEAD, M_TOP, N_SAMPLED, _sim, _window
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import DataArena, MLPSpec, TorchModuleSpec

KNOB = "GOSSIPY_PENS_MLP_WIDE"
SMALL = (57, 16, 2)  # d_in, hidden, classes of the shape that fits LDS


def _set_knob(value):
    os.environ.pop(KNOB, None)
    if value is not None:
        os.environ[KNOB] = value


def _small_data(device):
    X, y = make_synthetic_classification((61 * N_NODES, SMALL[0], SMALL[2]),
                                         seed=0, margin=2.0)
    idx = np.random.default_rng(0).permutation(len(y))
    cut = len(y) - 1000
    shards = [(X[s], y[s]) for s in np.array_split(idx[:cut], N_NODES)]
    return DataArena.from_shards(
        shards, device, global_eval=(X[idx[cut:]], y[idx[cut:]]))


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
    big, small = _data(device), _small_data(device)
    mnist = MLPSpec(d_in=D_IN, n_classes=K, hidden=(HIDDEN,), lr=0.1,
                    batch_size=32)
    tiny = MLPSpec(d_in=SMALL[0], n_classes=SMALL[2], hidden=(SMALL[1],),
                   lr=0.1, batch_size=32)

    # route -> (spec, data, knob value, expected PENS event path)
    routes = {
        "wide": (mnist, big, "1", "wide"),
        "torchmod": (
            TorchModuleSpec(_module, (D_IN,), lr=0.1, batch_size=32), big,
            None, None),
        "lds_small": (tiny, small, None, "lds"),
        "wide_small": (tiny, small, "1", "wide"),
    }
    if args.routes:
        routes = {name: routes[name] for name in args.routes}
    sims, events = {}, {}
    for name, (spec, data, knob, want) in routes.items():
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
            _set_knob(routes[name][2])
            rps, events[name] = _window(sim, args.steps, args.min_seconds)
            runs[name].append(rps)
    _set_knob(None)
    out = {
        "config": f"pens-mlp-{D_IN}-{HIDDEN}-{K}-{N_NODES}n-push-step1",
        "n_sampled": N_SAMPLED, "m_top": M_TOP, "steps": args.steps,
    }
    for name in sims:
        out[f"{name}_rounds_per_sec"] = max(runs[name])
        out[f"{name}_rounds_per_sec_runs"] = runs[name]
        out[f"{name}_pens_events_per_round"] = events[name]
    for a, b in (("wide", "torchmod"), ("wide_small", "lds_small")):
        if a in sims and b in sims:
            out[f"{a}_over_{b}"] = round(
                out[f"{a}_rounds_per_sec"] / out[f"{b}_rounds_per_sec"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
