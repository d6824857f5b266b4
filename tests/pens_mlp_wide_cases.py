"""Cases of the MLP PENS step-1 event on the wide route for
``test_pens_mlp_wide_cases.py`` (CPU) and ``test_gpu_pens_mlp_wide.py``
(MI355X), with the float64 replay of ``pens_mlp_cases`` written so that it
takes an empty shard. Not a test module. ``PensCase`` and ``build`` are those
of ``pens_logreg_wide_cases``; every case runs under the knob. Seeds were
picked on the CPU so that the float64 forward alone meets ``check_inputs``.
Measured on the CPU: smallest top-2 logit gap 3.8e-3 (mnist) to 6.8e-2 (cg);
fp32 ``TorchBackend.deliver_pens`` within 7.9e-8 (fullbatch) to 1.8e-7
(mnist) of the replay, under TOL / 8 = 1.25e-5.
"""

import functools

import numpy as np

import ref64
from gossipy_amd.engine import MLPSpec
from pens_logreg_wide_cases import PensCase, build  # noqa: F401
from pens_mlp_cases import (  # noqa: F401
    MARGIN, TOL, _forward64, _stable_top, events, run_backend)


def _case(name, d, hidden, k, bs, shards, nodes, ptr, seed, dups, counts,
          picks):
    spec = MLPSpec(d_in=d, n_classes=k, hidden=hidden, lr=0.1, batch_size=bs)
    return PensCase(name, spec, shards, nodes, ptr, seed, dups, "1", counts,
                    picks)


CASES = [
    # d_in % 4 != 0: scalar loads, K panels 32 + 32 + 6; 3 of 16 head columns
    _case("ragged", 70, (40,), 3, 16, (37,) * 6, (1, 4), (0, 5, 12), 6000, (),
          ((12, 10, 9, 16, 14), (14, 12, 10, 11, 13, 16, 14)),
          ((3, 4), (5, 0))),
    # 16-byte loads; 136 hidden outputs: two column-group passes, and the
    # head's K = 136 is four panels and a ragged fifth; a full head tile
    _case("cg", 72, (136,), 16, 32, (40,) * 3, (0, 2), (0, 4, 7), 6100,
          ((2, 3),), ((1, 5, 4, 4), (2, 2, 0)), ((1, 2), (0, 1))),
    # ping-pong over three layers; an event with fewer candidates than
    # m_top, one on the empty shard
    _case("deep", 64, (48, 32), 5, 16, (37, 20, 0, 33), (0, 1, 2),
          (0, 4, 5, 8), 6200, (),
          ((4, 7, 4, 7), (3,), (0, 0, 0)), ((1, 3), (0,), (0, 1))),
    # 318 KB model row, past the LDS plan; a shard smaller than a batch
    _case("mnist", 784, (100,), 10, 32, (40, 33, 7), (0, 1, 2), (0, 3, 6, 9),
          6300, (),
          ((5, 3, 5), (5, 3, 4), (0, 2, 0)), ((0, 2), (0, 2), (1, 0))),
    # a 200-row batch: act / grad in the workspace, four row blocks
    _case("fullbatch", 784, (100,), 10, 0, (200,), (0,), (0, 4), 6404, (),
          ((20, 19, 25, 20),), ((2, 0),)),
]
BY_NAME = {c.name: c for c in CASES}


def replay64(case):
    """``pens_mlp_cases.replay64`` on the case's CPU inputs."""
    spec, (state, data, pool, wins) = case.spec, build(case)
    rs, wins = ref64.RefState(state, data, pool), wins.long().numpy()
    nodes, ptr, slots, owners = (t.tolist() for t in events(case))
    out = {"correct": [], "picks": [], "gap": []}
    for i, node in enumerate(nodes):
        x, y = rs.shard(node)
        cand, own = slots[ptr[i]:ptr[i + 1]], owners[ptr[i]:ptr[i + 1]]
        correct, gap = [], np.inf
        for s in cand:
            z = _forward64(spec, rs.slots[s], x)
            top = np.sort(z, axis=1)
            gap = min([gap, *(top[:, -1] - top[:, -2])])
            correct.append(int((z.argmax(axis=1) == y).sum()))
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
    # computed once and only read
    return replay64(BY_NAME[name])


def check_inputs(name):
    """As ``pens_logreg_wide_cases.check_inputs``."""
    case, ref = BY_NAME[name], reference(name)
    assert tuple(ref["correct"]) == case.want_counts, ref["correct"]
    assert tuple(ref["picks"]) == case.want_picks, ref["picks"]
    assert min(ref["gap"]) >= MARGIN, ref["gap"]
    first = tuple(range(case.m_top))
    assert any(tuple(sorted(p)) != first for p in ref["picks"])
    assert any(c[j] == c[p[-1]] for c, p in zip(ref["correct"], ref["picks"])
               for j in range(len(c)) if j not in p)


def compare(name, state, counts):
    """Params at TOL, ages and winner counts exactly; the deviation."""
    ref = reference(name)
    dev = float(np.abs(state.params.cpu().double().numpy()
                       - ref["params"]).max())
    print(f"dev {name} {dev:.3e} tol {TOL:.1e}")
    assert dev <= TOL, (name, dev)
    assert np.array_equal(state.ages.cpu().numpy().ravel(), ref["ages"].ravel())
    assert np.array_equal(counts.cpu().numpy(), ref["counts"])
    return dev
