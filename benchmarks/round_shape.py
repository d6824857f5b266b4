"""The shape of the flagship round's tick launches, and the fit of their
measured durations against it.

Runs on the CPU and reads no GPU. It builds the simulator of ``bench.py``
(same data, seeds and sizes), replays the schedule from round 0 and, for the
rounds ``--r0..--r1``, prints one line per ``tick_logreg_kernel`` launch in
stream order: kind (deliver or reply), receiver rows, the largest number of
deliveries a row has, the deliveries in all. Then the sums per round. The
launches come from ``scheduler.next_round_flat(r)`` followed by
``_maybe_merge(scheduler.last_flat)``: rows from ``recv_tptr``/``rep_tptr``,
deliveries per row from ``recv_nptr``/``rep_nptr``.

``--trace CSV`` joins the list with a ``rocprofv3 --kernel-trace`` of
``bench.py --gpus 1 --steps S --warmup W`` (give ``--r0 0 --r1 W+S-1``): the
tick dispatches in start order against the launches in stream order, after a
check that every round has the expected number. It then fits
duration = a + b * (largest deliveries per row) by least squares and reports
the thin launches, the per-round totals and how often a round's evaluation
kernel ends after the next round's first tick launch begins. ``--timed-from
W`` leaves the warm-up rounds out of those figures. ``--pack-levels CAP``
replays with the level packer at that row cap (0: the default packer); give
the value the traced run used."""
import argparse
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from gossipy_amd.core import AntiEntropyProtocol
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import (BatchedGossipSimulator, DataArena,
                                EngineConfig, LogRegSpec)


def bench_simulator():
    """bench.py's simulator at one rank, on the CPU."""
    n_nodes, n_samples = 1000, 4601
    X, y = make_synthetic_classification((n_samples, 57, 2), seed=7)
    idx = np.random.default_rng(7).permutation(n_samples)
    n_eval = max(256, n_samples // 100)
    eval_idx, train_idx = idx[:n_eval], idx[n_eval:]
    shards = [(X[s], y[s]) for s in np.array_split(train_idx, n_nodes)]
    device = torch.device("cpu")
    data = DataArena.from_shards(
        shards, device, global_eval=(X[eval_idx], y[eval_idx]))
    cfg = EngineConfig(n_nodes=n_nodes, delta=100,
                       protocol=AntiEntropyProtocol.PUSH, model_size=116,
                       sampling_eval=0.01, seed=42, sync=True)
    spec = LogRegSpec(d_in=57, n_classes=2, lr=0.1, local_epochs=1,
                      batch_size=32)
    sim = BatchedGossipSimulator(cfg, spec, data, device=device)
    sim.init_nodes()
    return sim


def round_launches(flat):
    """[(kind, rows, max deliveries per row, deliveries)] in stream order."""
    out = []
    rt, nptr = np.asarray(flat["recv_tptr"]), np.asarray(flat["recv_nptr"])
    qt, qptr = np.asarray(flat["rep_tptr"]), np.asarray(flat["rep_nptr"])
    for g in range(len(rt) - 1):
        for kind, t, p in (("deliver", rt, nptr), ("reply", qt, qptr)):
            r0, r1 = int(t[g]), int(t[g + 1])
            if r1 > r0:
                per_row = np.diff(p[r0:r1 + 1])
                out.append((kind, r1 - r0, int(per_row.max()),
                            int(per_row.sum())))
    return out


def replay(r1, pack_levels=None):
    """The launches of rounds 0..r1. ``pack_levels``: the level packer's row
    cap (0: off); None takes what the runner's ``start()`` would set."""
    sim = bench_simulator()
    if pack_levels is None:
        pack_levels = sim._pack_levels_cap()
    sim.scheduler.set_pack_levels(pack_levels)
    rounds = []
    for r in range(r1 + 1):
        sim.scheduler.next_round_flat(r)
        rounds.append(round_launches(sim._maybe_merge(sim.scheduler.last_flat)))
    packed, refused = sim.scheduler.pack_level_stats()
    print(f"level packer: row cap {pack_levels}, packed {packed} rounds, "
          f"left {refused} to the default packer")
    return rounds


def read_trace(path):
    """{kernel short name: [(start ns, end ns)] in start order}."""
    ks = {"tick": [], "snap": [], "eval": []}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            name = row["Kernel_Name"]
            # the plain tick kernel or its thin instantiation
            for key, pat in (("tick", r"tick_logreg_(thin_)?kernel"),
                             ("snap", "snapshot_kernel"),
                             ("eval", "eval_metrics_kernel")):
                if re.search(pat, name):
                    ks[key].append((int(row["Start_Timestamp"]),
                                    int(row["End_Timestamp"])))
    for v in ks.values():
        v.sort()
    return ks


def join_and_fit(rounds, trace, timed_from):
    ks = read_trace(trace)
    ticks, snaps, evals = ks["tick"], ks["snap"], ks["eval"]
    # a round begins with a run of snapshot launches with no tick between
    # them (the round's own snapshot; before it the previous round's gather)
    marks = sorted([(s, 0) for s, _ in snaps] + [(s, 1) for s, _ in ticks])
    per_round, prev, early = [], 1, 0
    for _, is_tick in marks:
        if not is_tick and prev:
            per_round.append(0)
        elif is_tick and not per_round:
            early += 1  # before round 0: the nodes' initial local update
        elif is_tick:
            per_round[-1] += 1
        prev = is_tick
    if early:
        print(f"{early} tick dispatches before the first snapshot left out")
        ticks = ticks[early:]
    want = [len(x) for x in rounds]
    if per_round and per_round[-1] == 0:  # the last round's gather
        per_round.pop()
    if per_round != want:
        bad = [i for i, (a, b) in enumerate(zip(per_round, want)) if a != b]
        print(f"tick dispatches per round do not match the replay: "
              f"{len(per_round)} rounds in the trace, {len(want)} replayed, "
              f"first differing rounds {bad[:5]}; no join")
        return 1
    shape = [x for rnd in rounds for x in rnd]
    rnd_of = [r for r, rnd in enumerate(rounds) for _ in rnd]
    dur = np.array([(e - s) / 1000.0 for s, e in ticks])
    keep = np.array([r >= timed_from for r in rnd_of])
    mx = np.array([x[2] for x in shape], dtype=float)
    rows = np.array([x[1] for x in shape])
    A = np.stack([np.ones(keep.sum()), mx[keep]], axis=1)
    (a, b), *_ = np.linalg.lstsq(A, dur[keep], rcond=None)
    res = dur[keep] - A @ np.array([a, b])
    n_rounds = len(rounds) - timed_from
    print(f"rounds {timed_from}..{len(rounds) - 1}: {keep.sum()} tick "
          f"launches, {keep.sum() / n_rounds:.2f} per round")
    print(f"fit duration = a + b * max deliveries: a = {a:.2f} us, "
          f"b = {b:.2f} us, residual std {res.std():.2f} us")
    thin = keep & (rows <= 10)
    print(f"launches with at most 10 rows: {thin.sum()}, mean "
          f"{dur[thin].mean():.2f} us")
    for m in sorted(set(mx[keep].astype(int))):
        sel = keep & (mx == m)
        print(f"  max deliveries {m}: {sel.sum():5d} launches, mean "
              f"{dur[sel].mean():6.2f} us")
    print(f"tick time per round {dur[keep].sum() / n_rounds:.2f} us, sum of "
          f"max deliveries per round {mx[keep].sum() / n_rounds:.2f}")
    for key in ("tick", "snap", "eval"):
        d = np.array([(e - s) / 1000.0 for s, e in ks[key]])
        print(f"{key}: {len(d)} dispatches, mean {d.mean():.2f} us")
    # first tick of every round, in round order
    first = {}
    for i, r in enumerate(rnd_of):
        first.setdefault(r, ticks[i][0])
    if len(evals) == len(rounds):
        late = sum(1 for r in range(timed_from, len(rounds) - 1)
                   if evals[r][1] > first[r + 1])
        print(f"eval of round r ends after the first tick of round r+1 "
              f"begins: {late} of {len(rounds) - 1 - timed_from} rounds")
    else:
        print(f"{len(evals)} eval dispatches for {len(rounds)} rounds: "
              f"overlap not counted")
    # the first timed round opens with its snapshot launch, just before its
    # first tick
    t1 = ticks[-1][1]
    t0 = max((s for s, _ in snaps if s <= first[timed_from]),
             default=first[timed_from])
    allk = [(s, e) for v in ks.values() for s, e in v if s >= t0]
    busy = sum(e - s for s, e in allk) / 1000.0
    print(f"from the opening snapshot of round {timed_from} to the last tick: "
          f"{(t1 - t0) / 1000.0 / n_rounds:.2f} us per round, kernels "
          f"{busy / n_rounds:.2f} us per round")
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--r0", type=int, default=10)
    ap.add_argument("--r1", type=int, default=59)
    ap.add_argument("--trace", default=None,
                    help="kernel-trace CSV of the bench line to join")
    ap.add_argument("--timed-from", type=int, default=0,
                    help="first round that counts in the fit (bench warm-up)")
    ap.add_argument("--pack-levels", type=int, default=None,
                    help="row cap of the level packer, 0 for the default "
                         "packer (default: what the runner sets, which "
                         "GOSSIPY_PACK_LEVELS overrides)")
    ap.add_argument("--quiet", action="store_true",
                    help="no line per launch, sums only")
    args = ap.parse_args()
    rounds = replay(args.r1, args.pack_levels)
    tot = []
    for r in range(args.r0, args.r1 + 1):
        for kind, rows, mx, n in rounds[r]:
            if not args.quiet:
                print(f"round {r:4d} {kind:7s} rows {rows:4d} max {mx:2d} "
                      f"deliveries {n:4d}")
        rl = rounds[r]
        tot.append((len(rl), sum(x[2] for x in rl), sum(x[3] for x in rl)))
        print(f"round {r:4d} launches {tot[-1][0]} sum of max {tot[-1][1]} "
              f"deliveries {tot[-1][2]}")
    t = np.array(tot, dtype=float)
    print(f"mean over rounds {args.r0}..{args.r1}: launches "
          f"{t[:, 0].mean():.2f}, sum of max {t[:, 1].mean():.2f}, "
          f"deliveries {t[:, 2].mean():.1f}")
    if args.trace:
        if args.r0 != 0:
            print("--trace needs the replay from round 0 (--r0 0)")
            return 2
        return join_and_fit(rounds, args.trace, args.timed_from)
    return 0


if __name__ == "__main__":
    sys.exit(main())
