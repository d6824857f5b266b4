"""Cases of the Hungarian-matched k-means delivery and a plain float64 replay
of it. Events: node 1 receives slots 0 and 2 and answers the first into slot
5, node 6 (an empty shard) receives slot 4; all values uniform in [0, 1).

A discrete choice must not hide behind a tolerance: ``replay`` also returns,
over every merge, the gap between the best assignment's total and the best
total with one matched edge forbidden, relative to the best; and over every
sample, the gap between its two nearest centroids, relative to the nearer.
The seeds keep both at or above ``MARGIN``.

``TOL``: four times ``HOST_DEV``, the largest deviation of the host route
(``GOSSIPY_KMEANS_MATCH_KERNEL=0``) from the replay on the MERGE_UPDATE cases,
measured on an MI355X (per case in ``profiles/kmeans_match.md``)."""

import functools
from collections import namedtuple

import numpy as np
import torch
from scipy.optimize import linear_sum_assignment

from gossipy_amd.core import CreateModelMode
from gossipy_amd.engine import DataArena, KMeansSpec
from gossipy_amd.engine.arena import NodeStateArena, SlotPool

MU, UM = CreateModelMode.MERGE_UPDATE, CreateModelMode.UPDATE_MERGE
MARGIN = 1e-4
HOST_DEV = 9.194e-8  # at (33, 8); 6.855e-8 to 8.866e-8 on the other shapes
TOL = 4 * HOST_DEV
N_NODES, N_SLOTS, ROWS, ALPHA = 8, 6, 12, 0.1
RECV, PTR, DSLOTS, REPLY = [1, 6], [0, 2, 3], [0, 2, 4], [5, -1, -1]

Case = namedtuple("Case", "k dim mode seed")
#: (k, dim): seed for MERGE_UPDATE, seed for UPDATE_MERGE
_SEEDS = {
    (1, 4): (7001, 7001),    # the trivial assignment
    (3, 8): (7001, 7001),    # the shape the existing test uses
    (5, 7): (7001, 7002),    # odd in both dimensions
    (16, 32): (7003, 7002),  # the bank-conflict stride
    (33, 8): (7002, 7002),   # columns past lane 31, with idle lanes
    (64, 8): (7097, 7015),   # a full wave; margins 2.1e-4 and 3.3e-4
}
CASES = [Case(k, d, m, s[m is UM]) for (k, d), s in _SEEDS.items()
         for m in (MU, UM)]
IDS = [f"k{c.k}_d{c.dim}_{c.mode.name}" for c in CASES]


def spec(case):
    return KMeansSpec(k=case.k, dim=case.dim, alpha=ALPHA, mode=case.mode,
                      matching="hungarian")


def build(case, device=torch.device("cpu")):
    """Fresh ``(state, pool, data)`` of a case on ``device``."""
    g = torch.Generator().manual_seed(case.seed)
    D = case.k * case.dim
    state, pool = NodeStateArena(N_NODES, D, device), SlotPool(D, device, N_SLOTS)
    state.params.copy_(torch.rand(N_NODES, D, generator=g))
    state.ages.copy_(torch.arange(N_NODES, dtype=torch.int32) + 2)
    pool.slots.copy_(torch.rand(N_SLOTS, D, generator=g))
    pool.slot_ages.copy_(torch.arange(N_SLOTS, dtype=torch.int32) + 20)
    counts = torch.tensor([ROWS] * 6 + [0, ROWS], dtype=torch.int32)
    x = torch.rand(N_NODES, ROWS, case.dim, generator=g)
    data = DataArena(x.to(device), torch.zeros(N_NODES, ROWS, device=device),
                     counts.to(device))
    return state, pool, data


def deliver(backend, case, state, pool, data):
    t = lambda v: torch.tensor(v, dtype=torch.int64)
    backend.deliver(state, pool, data, spec(case), t(RECV), t(PTR), t(DSLOTS),
                    t(REPLY))


def _dist(A, B):
    return np.sqrt(((A[:, None, :] - B[None, :, :]) ** 2).sum(-1))


@functools.lru_cache(maxsize=None)
def replay(case):
    """``(params, ages, slots, slot_ages, assignment margin, arg-min margin)``"""
    state, pool, data = build(case)
    P = state.params.double().numpy().reshape(N_NODES, case.k, case.dim)
    S = pool.slots.double().numpy().reshape(N_SLOTS, case.k, case.dim)
    ages, sages = state.ages.numpy().copy(), pool.slot_ages.numpy().copy()
    margins = [np.inf, np.inf]

    def update(C, x):
        if not len(x):
            return 0
        d = _dist(x, C)
        if case.k > 1:
            near = np.sort(d, axis=1)
            margins[1] = min(margins[1],
                             ((near[:, 1] - near[:, 0]) / near[:, 0]).min())
        # every sample is assigned first; per centroid the last one lands
        for j, s in {j: s for s, j in enumerate(d.argmin(1))}.items():
            C[j] = C[j] * (1 - ALPHA) + ALPHA * x[s]
        return 1

    def merge(C, O):
        cost = _dist(C, O)
        rows, perm = linear_sum_assignment(cost)
        best = cost[rows, perm].sum()
        for i in range(case.k if case.k > 1 else 0):
            c = cost.copy()
            c[i, perm[i]] = 1e9
            alt = c[linear_sum_assignment(c)].sum()
            margins[0] = min(margins[0], (alt - best) / best)
        C[:] = 0.5 * (C + O[perm])

    for i, node in enumerate(RECV):
        x = data.x[node, : int(data.counts[node])].double().numpy()
        for j in range(PTR[i], PTR[i + 1]):
            if case.mode is MU:
                merge(P[node], S[DSLOTS[j]])
                ages[node] += update(P[node], x)
            else:
                ages[node] += update(P[node], x)
                other = S[DSLOTS[j]].copy()
                update(other, x)
                merge(P[node], other)
            if REPLY[j] >= 0:
                S[REPLY[j]], sages[REPLY[j]] = P[node], ages[node]
    return (P.reshape(N_NODES, -1), ages, S.reshape(N_SLOTS, -1), sages,
            *margins)


def deviation(ref, state, pool):
    """Largest absolute difference of params and reply slots from the replay,
    ages equal. (The torch loop trains delivered slots in place.)"""
    r = [s for s in REPLY if s >= 0]
    assert np.array_equal(ref[1], state.ages.cpu().numpy())
    assert np.array_equal(ref[3][r], pool.slot_ages.cpu().numpy()[r])
    return max(np.abs(ref[0] - state.params.cpu().double().numpy()).max(),
               np.abs(ref[2][r] - pool.slots.cpu().double().numpy()[r]).max())
