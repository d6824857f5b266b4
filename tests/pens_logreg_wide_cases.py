"""Cases of the logreg PENS step-1 event on ``tick_pens_wide_kernel`` for
``test_pens_logreg_wide_cases.py`` (CPU) and ``test_gpu_pens_logreg_wide.py``
(MI355X), with a plain float64 numpy replay of one ``deliver_pens`` call:
``ref64.logreg_scores``, arg-max counts, stable top-m, the mean, then
``ref64.update``. Not a test module; ``events`` and ``run_backend`` are those
of ``pens_mlp_cases``.

State, shards and slots are those ``tick_cases.build`` draws from the seed;
slot ``b`` of a pair in ``dups`` copies slot ``a``, an exact tie. Seeds were
picked on the CPU so that the float64 forward alone meets ``check_inputs``.
Measured on the CPU: smallest top-2 score gap 5.5e-4 (many) to 3.1e-2
(cifar); fp32 ``TorchBackend.deliver_pens`` within 1.7e-8 (rows) to 8.4e-8
(cifar) of the replay, under TOL / 8 = 1.25e-5.
"""

import functools
from dataclasses import dataclass

import numpy as np
import torch

import ref64
import tick_cases as tc
from gossipy_amd.engine import LogRegSpec
from pens_mlp_cases import MARGIN, TOL, _stable_top, events, run_backend  # noqa: F401


@dataclass
class PensCase:
    name: str
    spec: LogRegSpec
    shards: tuple        # rows per node
    nodes: tuple         # event receivers
    ptr: tuple           # candidate ranges over slots 0.., arrival order
    seed: int
    dups: tuple          # (a, b): slot b is a copy of slot a
    knob: str            # GOSSIPY_LOGREG_WIDE of the GPU run, or None
    want_counts: tuple   # float64 correct counts per event
    want_picks: tuple    # picked candidate positions per event, pick order
    trunc_rows: tuple = ()  # a scorer that stops at these rows picks otherwise
    m_top: int = 2


def _spec(d, k, bs):
    return LogRegSpec(d_in=d, n_classes=k, lr=0.1, batch_size=bs)


CASES = [
    # d % 4 != 0, ragged K panel and row tile (16 + 16 + 5), 3 of 16 class
    # lanes, 5 and 7 candidates over 4 waves
    PensCase("ragged", _spec(70, 3, 16), (37,) * 6, (1, 4), (0, 5, 12),
             5006, ((1, 3), (7, 10)), "1",
             ((12, 11, 15, 11, 12), (13, 12, 9, 12, 11, 9, 13)),
             ((2, 0), (0, 6))),
    # d below a panel, more rows than threads
    PensCase("rows", _spec(4, 3, 0), (530, 530), (0, 1), (0, 3, 6),
             5156, ((0, 1), (3, 4)), "1",
             ((182, 182, 183), (173, 173, 175)), ((2, 0), (2, 0)),
             trunc_rows=(256, 512)),
    # full class tile, VEC, 19 candidates = a pass of 16 and one of 3, and an
    # event with fewer candidates than m_top
    PensCase("many", _spec(72, 16, 32), (40,) * 3, (0, 2), (0, 19, 20),
             5204, ((4, 17),), "1",
             ((3, 2, 6, 2, 2, 1, 7, 0, 1, 3, 4, 1, 4, 3, 2, 2, 3, 2, 6), (3,)),
             ((6, 2), (0,))),
    # 320 KB LDS plan, 159 KB wide geometry; a shard smaller than a batch
    PensCase("cifar", _spec(3072, 10, 16), (20, 33, 7), (1, 2), (0, 3, 7),
             5302, ((0, 2),), None,
             ((2, 4, 2), (0, 0, 2, 1)), ((1, 0), (2, 3))),
    # a 200-row batch, d % 4 != 0, an event on the empty shard
    PensCase("har", _spec(561, 6, 0), (200, 33, 0), (0, 1, 2), (0, 4, 7, 9),
             5407, ((0, 3),), None,
             ((31, 37, 29, 31), (9, 4, 10), (0, 0)),
             ((1, 0), (2, 0), (0, 1))),
]
BY_NAME = {c.name: c for c in CASES}


def build(case, device=tc.CPU):
    """``(state, data, pool, counts)`` of the case on ``device``: the values
    ``tick_cases.build`` generates on the CPU from the case's seed."""
    rows = [(n, hi - lo, ()) for n, lo, hi
            in zip(case.nodes, case.ptr, case.ptr[1:])]
    state, data, pool = tc.build(
        tc.Case(case.name, case.spec, list(case.shards), TOL, rows=rows,
                seed=case.seed), device)
    for a, b in case.dups:
        pool.slots[b] = pool.slots[a]
    counts = torch.zeros(len(case.shards), case.ptr[-1], dtype=torch.int32,
                         device=device)
    return state, data, pool, counts


def replay64(case, rows=None):
    """The float64 replay on the case's CPU inputs: final ``params``, ``ages``
    and ``counts`` matrix, and per event the ``correct`` counts, the ``picks``
    and the smallest top-2 score ``gap``. ``rows`` stops the scorer there."""
    spec, (state, data, pool, wins) = case.spec, build(case)
    rs, wins = ref64.RefState(state, data, pool), wins.long().numpy()
    nodes, ptr, slots, owners = (t.tolist() for t in events(case))
    out = {"correct": [], "picks": [], "gap": []}
    for i, node in enumerate(nodes):
        x, y = rs.shard(node)
        cand, own = slots[ptr[i]:ptr[i + 1]], owners[ptr[i]:ptr[i + 1]]
        correct, gap = [], np.inf
        for s in cand:
            z = ref64.logreg_scores(rs.slots[s], x, spec.d_in, spec.n_classes)
            top = np.sort(z, axis=1)
            gap = min([gap, *(top[:, -1] - top[:, -2])])
            correct.append(int((z.argmax(axis=1) == y)[:rows].sum()))
        picks = _stable_top(correct, case.m_top)
        row, age = rs.params[node].copy(), int(rs.ages[node])
        for c in picks:
            row += rs.slots[cand[c]]
            age = max(age, int(rs.slot_ages[cand[c]]))
            wins[node, own[c]] += 1
        rs.params[node], rs.ages[node] = row / (len(picks) + 1), age
        out["correct"].append(tuple(correct))
        out["picks"].append(tuple(picks))
        out["gap"].append(gap)
    ref64.update(spec, rs, nodes)
    out.update(params=rs.params, ages=rs.ages, counts=wins)
    return out


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's float64 result, computed once and only read."""
    return replay64(BY_NAME[name])


def check_inputs(name):
    """What makes the discrete selection comparable between fp32 and float64
    and not trivial, with the recorded float64 counts and picks."""
    case, ref = BY_NAME[name], reference(name)
    assert tuple(ref["correct"]) == case.want_counts, ref["correct"]
    assert tuple(ref["picks"]) == case.want_picks, ref["picks"]
    assert min(ref["gap"]) >= MARGIN, ref["gap"]
    # some event's top-m is not its first m arrivals, some event has a tie
    # between its last pick and a candidate left out
    first = tuple(range(case.m_top))
    assert any(tuple(sorted(p)) != first for p in ref["picks"])
    assert any(c[j] == c[p[-1]] for c, p in zip(ref["correct"], ref["picks"])
               for j in range(len(c)) if j not in p)
    for T in case.trunc_rows:  # a scorer that stops after T rows
        cut = replay64(case, rows=T)["picks"]
        assert any(set(a) != set(b) for a, b in zip(cut, ref["picks"])), T


def compare(name, state, counts):
    """A backend's result against the replay: params at TOL, ages and winner
    counts exactly. Returns the deviation."""
    ref = reference(name)
    dev = float(np.abs(state.params.cpu().double().numpy()
                       - ref["params"]).max())
    print(f"dev {name} {dev:.3e} tol {TOL:.1e}")
    assert dev <= TOL, (name, dev)
    assert np.array_equal(state.ages.cpu().numpy().ravel(), ref["ages"].ravel())
    assert np.array_equal(counts.cpu().numpy(), ref["counts"])
    return dev
