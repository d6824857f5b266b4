"""The two PENS step-1 cases of the MLP family that ``test_pens_mlp.py`` (CPU)
and ``test_gpu_pens_mlp.py`` (GPU) share, with a plain float64 numpy replay
of one ``deliver_pens`` call: forward, argmax counts, stable top-m, mean,
then ``ref64``'s MLP update. Not a test module (no ``test_`` prefix).

Case A: ragged MFMA tiles (d_in 20, hidden 24, 3 classes), shards of 37 rows
(16 + 16 + 5 at batch_size 16, or one 37-row chunk at batch_size 0), a
three-way tie at the cut. Case B: shards of 530 rows at batch_size 0, more
rows than the block has threads; a scorer that sees the first 512 rows alone
picks another candidate.

Top-m selection is discrete, so a test that compares two fp32 backends first
asserts two conditions on its inputs, both from the float64 forward:
``min_gap`` (the smallest top-2 head-logit gap over all candidate/sample
pairs) is at least ``MARGIN`` — the fp32 forward error at these shapes is
about K * eps * |v| ~ 5e-6 — and ``cut_conditions`` (some event's top-m set is
not the first m in arrival order, some event has a tie at the cut).
"""

from dataclasses import dataclass, replace

import numpy as np
import torch

import ref64
from gossipy_amd.data import make_synthetic_classification
from gossipy_amd.engine import DataArena, MLPSpec, NodeStateArena, SlotPool
from gossipy_amd.engine.backend import TorchBackend
from gossipy_amd.engine.rng import RandomTape

CPU = torch.device("cpu")
MARGIN = 1e-4
TOL = 1e-4  # the project's fp32-vs-reference bound on parameters


@dataclass
class PensCase:
    name: str
    spec: MLPSpec
    n_nodes: int
    data_shape: tuple
    n_slots: int
    noise: float
    noise_seed: int
    nodes: tuple
    ptr: tuple
    m_top: int
    want_counts: tuple   # float64 correct counts per event
    want_picks: tuple    # picked candidate positions per event, pick order
    # a scorer limited to the first trunc_rows samples counts trunc_counts
    # in event 0 (0 = the case has no such variant)
    trunc_rows: int = 0
    trunc_counts: tuple = ()


CASE_A = PensCase(
    name="A",
    spec=MLPSpec(d_in=20, n_classes=3, hidden=(24,), lr=0.1, batch_size=16),
    n_nodes=6, data_shape=(222, 20, 3), n_slots=12, noise=0.2, noise_seed=6,
    nodes=(1, 4), ptr=(0, 5, 12), m_top=2,
    want_counts=((10, 18, 10, 8, 12), (14, 14, 18, 14, 4, 9, 10)),
    want_picks=((1, 4), (2, 0)),
)
# the same inputs as one 37-row chunk
CASE_A_FULL = replace(CASE_A, name="A_bs0",
                      spec=replace(CASE_A.spec, batch_size=0))
CASE_B = PensCase(
    name="B",
    spec=MLPSpec(d_in=4, n_classes=3, hidden=(8,), lr=0.1, batch_size=0),
    n_nodes=2, data_shape=(1060, 4, 3), n_slots=6, noise=0.5, noise_seed=3,
    nodes=(0, 1), ptr=(0, 3, 6), m_top=2,
    want_counts=((139, 191, 139), (331, 173, 173)),
    want_picks=((1, 0), (0, 1)),
    trunc_rows=512, trunc_counts=(134, 185, 136),
)
CASES = {c.name: c for c in (CASE_A, CASE_A_FULL, CASE_B)}


def build(case, device=CPU):
    """``(state, data, pool, counts)`` of the case on ``device``."""
    spec = case.spec
    be = TorchBackend()
    X, y = make_synthetic_classification(case.data_shape, seed=3)
    idx = np.array_split(np.arange(case.data_shape[0]), case.n_nodes)
    cd = DataArena.from_shards([(X[s], y[s]) for s in idx], CPU)
    data = DataArena(cd.x.to(device), cd.y.to(device), cd.counts.to(device))

    st = NodeStateArena(case.n_nodes, spec.D, CPU)
    be.init_params(st, spec, RandomTape(3))
    state = NodeStateArena(case.n_nodes, spec.D, device)
    state.params.copy_(st.params)
    state.ages.copy_(
        (torch.arange(case.n_nodes) % 5).to(torch.int32).view_as(st.ages))

    cand = NodeStateArena(case.n_slots, spec.D, CPU)
    be.init_params(cand, spec, RandomTape(103))
    g = torch.Generator().manual_seed(case.noise_seed)
    rows = cand.params + case.noise * torch.randn(
        case.n_slots, spec.D, generator=g)
    pool = SlotPool(spec.D, device, case.n_slots)
    pool.slots[: case.n_slots].copy_(rows)
    pool.slot_ages[: case.n_slots].copy_(
        (2 * torch.arange(case.n_slots)).to(torch.int32).view_as(
            pool.slot_ages[: case.n_slots]))

    counts = torch.zeros(case.n_nodes, case.n_slots, dtype=torch.int32,
                         device=device)
    return state, data, pool, counts


def events(case):
    """Host tensors ``(nodes, ptr, slots, owners)``: slots 0..n-1 in arrival
    order, every candidate from a distinct owner."""
    n = case.ptr[-1]
    return (torch.tensor(case.nodes), torch.tensor(case.ptr),
            torch.arange(n), torch.arange(n))


def run_backend(backend, case, state, data, pool, counts):
    backend.deliver_pens(state, pool, data, case.spec, *events(case), counts,
                         case.m_top)


def _forward64(spec, row, x):
    h = x
    offs = spec.layer_offsets()
    for li, (w_off, b_off, fin, fout) in enumerate(offs):
        h = h @ row[w_off:b_off].reshape(fout, fin).T + row[b_off:b_off + fout]
        if li < len(offs) - 1:
            h = np.maximum(h, 0.0)
    return h


def _stable_top(correct, m):
    """Positions of the top-m counts, the first of equal counts first."""
    picks, left = [], list(range(len(correct)))
    for _ in range(min(m, len(correct))):
        best = left[0]
        for c in left:
            if correct[c] > correct[best]:
                best = c
        picks.append(best)
        left.remove(best)
    return picks


def replay64(case, state, data, pool, rows=None):
    """The float64 replay of the case on CPU inputs. Returns a dict with the
    final ``params`` / ``ages`` (all nodes), the ``counts`` matrix, and per
    event the ``correct`` counts, the ``picks`` and the smallest top-2 logit
    ``gap``. ``rows`` limits the scorer to the first ``rows`` samples of a
    shard (the defect of a per-sample stage that does not stride)."""
    spec = case.spec
    rs = ref64.RefState(state, data, pool)
    nodes, ptr, slots, owners = (t.tolist() for t in events(case))
    wins = np.zeros((case.n_nodes, case.n_slots), dtype=np.int64)
    out = {"correct": [], "picks": [], "gap": []}
    for i, node in enumerate(nodes):
        x, y = rs.shard(node)
        cand = slots[ptr[i]:ptr[i + 1]]
        own = owners[ptr[i]:ptr[i + 1]]
        correct, gap = [], np.inf
        for s in cand:
            h = _forward64(spec, rs.slots[s], x)
            top = np.sort(h, axis=1)
            gap = min(gap, float((top[:, -1] - top[:, -2]).min()))
            hit = h.argmax(axis=1) == y
            correct.append(int(hit[:rows].sum()))
        picks = _stable_top(correct, case.m_top)
        row, age = rs.params[node].copy(), int(rs.ages[node])
        for c in picks:
            row += rs.slots[cand[c]]
            age = max(age, int(rs.slot_ages[cand[c]]))
            wins[node, own[c]] += 1
        row /= len(picks) + 1
        rs.params[node] = row
        rs.ages[node] = age
        out["correct"].append(tuple(correct))
        out["picks"].append(tuple(picks))
        out["gap"].append(gap)
    ref64.update(spec, rs, nodes)
    out.update(params=rs.params, ages=rs.ages, counts=wins)
    return out


_REF = {}


def reference(name):
    """The case's float64 result on its CPU inputs, computed once and only
    read."""
    if name not in _REF:
        case = CASES[name]
        state, data, pool, _ = build(case)
        _REF[name] = replay64(case, state, data, pool)
    return _REF[name]


def check_inputs(name):
    """The two conditions that make the discrete selection comparable
    between fp32 backends, and the recorded float64 counts and picks."""
    case, ref = CASES[name], reference(name)
    assert tuple(ref["correct"]) == case.want_counts, ref["correct"]
    assert tuple(ref["picks"]) == case.want_picks, ref["picks"]
    # (i) margin
    assert min(ref["gap"]) >= MARGIN, ref["gap"]
    # (ii) cut: a top-m that is not the first m arrivals, and a tie between
    # the last pick and a candidate left out. In case A the picked SET
    # differs from the first m; in case B both events pick positions {0, 1},
    # so what differs is the ranking (event 0 picks 1 before 0), and the
    # selection is pinned by the truncated scorer instead: one that sees
    # only the first 512 rows of a 530-row shard picks {1, 2}.
    m = case.m_top
    first = tuple(range(m))
    if case.trunc_rows:
        assert any(p != first for p in ref["picks"])
        state, data, pool, _ = build(case)
        cut = replay64(case, state, data, pool, rows=case.trunc_rows)
        assert tuple(cut["correct"][0]) == case.trunc_counts, cut["correct"]
        assert set(cut["picks"][0]) != set(ref["picks"][0])
    else:
        assert any(tuple(sorted(p)) != first for p in ref["picks"])
    assert any(
        any(c[j] == c[p[-1]] for j in range(len(c)) if j not in p)
        for c, p in zip(ref["correct"], ref["picks"])
    )


def compare(name, state, counts):
    """Deviation checks of a backend's result against the float64 replay:
    params at TOL, ages and counts exactly."""
    ref = reference(name)
    dev = float(np.abs(state.params.detach().cpu().double().numpy()
                       - ref["params"]).max())
    print(f"dev {name} {dev:.3e} tol {TOL:.1e}")
    assert dev <= TOL, (name, dev)
    assert np.array_equal(state.ages.cpu().long().numpy().reshape(-1),
                          ref["ages"].reshape(-1))
    assert np.array_equal(counts.cpu().long().numpy(), ref["counts"])
