"""The case table shared by ``test_ref64.py`` (CPU: fp32 oracle against the
float64 reference) and ``test_gpu_ref64.py`` (MI355X: HIP kernels against the
same reference). Not a test module.

A case is a spec, one shard size per node (at most 6 nodes), an optional
update of every node and an optional deliver launch, all built from the
case's position in the table as the seed. ``tol`` is the absolute bound the
HIP result must meet against the float64 reference. It is a literal, floored
at the suite's 1e-4, and the CPU file asserts that the fp32 oracle's own
deviation ``e32`` from the reference is at most ``tol / 8``: the factor 8
leaves room for the kernels' different summation order (FMA chains, two MFMA
accumulators) and ``__expf``. The measured ``e32`` stands next to each
``tol``.

``block`` marks the cases whose batches have more rows than the kernel's
block has threads (128 for logreg, 512 for the MLP); the CPU file checks
that a per-sample stage covering only the first ``block`` rows would move
the result by at least ``10 * tol``.
"""

from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import torch

import ref64
from gossipy_amd.core import CreateModelMode
from gossipy_amd.engine import (
    DataArena,
    LogRegSpec,
    MLPSpec,
    NodeStateArena,
    SlotPool,
)

CPU = torch.device("cpu")
MU = CreateModelMode.MERGE_UPDATE
UP = CreateModelMode.UPDATE
UM = CreateModelMode.UPDATE_MERGE
PA = CreateModelMode.PASS
MODES = {"merge_update": MU, "update": UP, "update_merge": UM, "pass": PA}


@dataclass
class Case:
    name: str
    spec: object
    shards: List[int]
    tol: float
    #: receiver rows of the deliver launch: (node, deliveries, positions of
    #: the deliveries that ask for a reply snapshot); None = no deliver
    rows: Optional[List[Tuple[int, int, Tuple[int, ...]]]] = None
    update: bool = True  #: update every node before the deliver
    ages: Optional[List[int]] = None       #: default arange % 5
    slot_ages: Optional[List[int]] = None  #: default arange * 2 % 7
    flags: Optional[List[int]] = None      #: pass-through coin per delivery
    block: Optional[int] = None
    seed: int = field(default=0)


def _rows5():
    # receiver rows of 1, 2, 1, 1 and 3 deliveries over five nodes, replies
    # after the only delivery of node 2 and between those of node 4
    return [(0, 1, ()), (1, 2, ()), (2, 1, (0,)), (3, 1, ()), (4, 3, (0, 1))]


ROWS3 = [(0, 2, (0,)), (1, 1, ()), (2, 1, (0,))]
ROWS4 = [(0, 2, (0,)), (1, 1, ()), (2, 1, (0,)), (3, 1, ())]
# one receiver row of 4 deliveries, replies after the 1st and the 3rd
ROW_LONG = [(0, 4, (0, 2)), (1, 1, ()), (2, 2, ())]

CASES: List[Case] = []


def _add(name, spec, shards, tol=1e-4, **kw):
    assert len(shards) <= 6
    CASES.append(Case(name, spec, shards, tol, seed=len(CASES) + 1, **kw))


# tol and the measured e32 (fp32 TorchBackend against the reference, CPU)
# of every case below; e32 is mostly the rounding of the result to fp32:
#   case                               tol     e32
#   rows_logreg_k2_merge_update        1e-4    3.247e-08
#   rows_logreg_k2_update_merge        1e-4    3.660e-08
#   rows_logreg_k16_merge_update       1e-4    5.443e-08
#   rows_logreg_k16_update_merge       1e-4    4.253e-08
#   rows_logreg_bs200                  1e-4    4.648e-08
#   rows_logreg_limited                1e-4    4.027e-08
#   rows_part_d9_merge_update          1e-4    3.416e-08
#   rows_part_d9_update                1e-4    2.940e-08
#   rows_part_d80                      1e-4    5.561e-08
#   rows_mlp_merge_update              1e-4    5.759e-08
#   rows_mlp_update_merge              1e-4    1.302e-07
#   rows_mlp_bs600                     1e-4    8.042e-08
#   mfma_fwd_k31                       1e-4    6.957e-08
#   mfma_fwd_k32                       1e-4    5.535e-08
#   mfma_fwd_k33                       1e-4    5.124e-08
#   mfma_fwd_k63                       1e-4    5.014e-08
#   mfma_fwd_k64                       1e-4    7.930e-08
#   mfma_fwd_k65                       1e-4    6.263e-08
#   mfma_fwd_k127                      1e-4    7.223e-08
#   mfma_fwd_k128                      1e-4    5.813e-08
#   mfma_fwd_k129                      1e-4    6.102e-08
#   mfma_fwd_k132                      1e-4    6.245e-08
#   mfma_fwd_k133                      1e-4    7.616e-08
#   mfma_fwd_k136                      1e-4    6.463e-08
#   mfma_fwd_k141                      1e-4    6.135e-08
#   mfma_dx_k33                        1e-4    4.734e-08
#   mfma_dx_k65                        1e-4    6.801e-08
#   mfma_dx_k129                       1e-4    5.902e-08
#   mfma_dx_k133                       1e-4    8.265e-08
#   mfma_dw_rows                       1e-4    4.378e-08
#   mfma_ragged_1_15_16                1e-4    5.877e-08
#   mfma_ragged_15_16_17               1e-4    6.358e-08
#   mfma_ragged_16_17_2                1e-4    5.514e-08
#   mfma_ragged_17_1_15                1e-4    4.870e-08
#   mlp_one_layer                      1e-4    4.063e-08
#   mlp_three_layers                   1e-4    7.457e-08
#   mlp_256_threads                    1e-4    5.095e-08
#   mlp_512_threads                    1e-4    8.225e-08
#   mlp_wd_epochs_merge_update         1e-4    7.420e-08
#   mlp_wd_epochs_pass                 1e-4    0.000e+00
#   mlp_wd_epochs_update               1e-4    1.301e-07
#   mlp_wd_epochs_update_merge         1e-4    5.973e-08
#   mlp_limited_merge_update           1e-4    6.350e-08
#   mlp_limited_update_merge           1e-4    6.725e-08
#   wide_logreg_d64_plain              1e-4    7.296e-08
#   wide_logreg_d64_limited            1e-4    9.561e-08
#   wide_logreg_d64_pass_through       1e-4    8.112e-08
#   wide_logreg_d129_plain             1e-4    7.830e-08
#   wide_logreg_d129_limited           1e-4    7.513e-08
#   wide_logreg_d129_pass_through      1e-4    6.175e-08
# evaluation cases: tol 1e-6 (EVAL_TOL), e32 at most 5.1e-08


# ---- rows per batch against the block size: logreg (128 threads) -------------
# lr = 4: one row of 129 carries 1/129 of the batch gradient, and the step
# it contributes must stand out by 10 * tol (see the sensitivity test)
ROWS_LR = 4.0
SH_ROWS = [127, 128, 129, 130, 257]
for _k in (2, 16):
    for _mn in ("merge_update", "update_merge"):
        _add(
            f"rows_logreg_k{_k}_{_mn}",
            LogRegSpec(d_in=9, n_classes=_k, lr=ROWS_LR, batch_size=0,
                       mode=MODES[_mn]),
            SH_ROWS, rows=_rows5(), block=128,
        )
_add(
    "rows_logreg_bs200",  # batches of 200 and 130; 129 rows in one batch
    LogRegSpec(d_in=9, n_classes=2, lr=ROWS_LR, batch_size=200),
    [330, 129, 5], rows=ROWS3, block=128,
)
_add(
    "rows_logreg_limited",
    LogRegSpec(d_in=9, n_classes=3, lr=ROWS_LR, batch_size=0,
               age_diff_threshold=2),
    [129, 130, 64], rows=ROWS3, block=128,
)
for _mn in ("merge_update", "update"):
    _add(  # the whole shard fits the 64 KB staging budget
        f"rows_part_d9_{_mn}",
        LogRegSpec(d_in=9, n_classes=2, lr=ROWS_LR, batch_size=0, n_parts=3,
                   mode=MODES[_mn]),
        [129, 257, 40], rows=ROWS3, block=128,
    )
_add(  # 257 * 80 floats = 82 KB: batches are staged one at a time
    "rows_part_d80",
    LogRegSpec(d_in=80, n_classes=2, lr=ROWS_LR, batch_size=0, n_parts=3),
    [129, 257, 40], rows=ROWS3, block=128,
)

# ---- rows per batch against the block size: MLP (512 threads) ----------------
# 520 rows * (4 + 8 + 3 + 2 * 8) floats = 64 KB of LDS
MLP_ROWS_LR = 4.0
for _mn in ("merge_update", "update_merge"):
    _add(
        f"rows_mlp_{_mn}",
        MLPSpec(d_in=4, n_classes=3, hidden=(8,), lr=MLP_ROWS_LR,
                batch_size=0, mode=MODES[_mn]),
        [511, 512, 513, 520], rows=ROWS4, block=512,
    )
_add(  # batches of 600 and 100: 600 * 31 floats = 74 KB, inside 160 KB
    "rows_mlp_bs600",
    MLPSpec(d_in=4, n_classes=3, hidden=(8,), lr=MLP_ROWS_LR,
            batch_size=600),
    [700, 513, 9], rows=ROWS3, block=512,
)

# ---- MFMA K-loop: forward K = d_in -------------------------------------------
for _d in (31, 32, 33, 63, 64, 65, 127, 128, 129, 132, 133, 136, 141):
    _add(
        f"mfma_fwd_k{_d}",
        MLPSpec(d_in=_d, n_classes=3, hidden=(8,), lr=0.1, batch_size=32),
        [20, 33, 7], rows=ROWS3,
    )
# ---- dX K = fout of the second layer -----------------------------------------
for _h in (33, 65, 129, 133):
    _add(
        f"mfma_dx_k{_h}",
        MLPSpec(d_in=6, n_classes=3, hidden=(8, _h), lr=0.1, batch_size=32),
        [20, 33, 7], rows=ROWS3,
    )
# ---- dW K = rows of a full batch, narrow model -------------------------------
_add(
    "mfma_dw_rows",
    MLPSpec(d_in=5, n_classes=3, hidden=(6,), lr=0.1, batch_size=0),
    [33, 65, 129, 133], rows=ROWS4,
)
# ---- ragged output tiles: widths and rows around 16 ---------------------------
for _fin, _h, _k in ((1, 15, 16), (15, 16, 17), (16, 17, 2), (17, 1, 15)):
    _add(  # 4 tiles at the most: the 256-thread launch
        f"mfma_ragged_{_fin}_{_h}_{_k}",
        MLPSpec(d_in=_fin, n_classes=_k, hidden=(_h,), lr=0.1, batch_size=0),
        [1, 15, 16, 17, 20], rows=_rows5(),
    )
_add(
    "mlp_one_layer",
    MLPSpec(d_in=17, n_classes=5, hidden=(), lr=0.1, batch_size=16),
    [20, 33, 7], rows=ROWS3,
)
_add(
    "mlp_three_layers",
    MLPSpec(d_in=12, n_classes=4, hidden=(9, 7), lr=0.1, batch_size=16),
    [20, 33, 7], rows=ROWS3,
)
_add(  # 1 tile per stage: 256 threads
    "mlp_256_threads",
    MLPSpec(d_in=10, n_classes=3, hidden=(12,), lr=0.1, batch_size=16),
    [16, 9, 3], rows=ROWS3,
)
_add(  # forward has 2 * 5 tiles: 512 threads
    "mlp_512_threads",
    MLPSpec(d_in=20, n_classes=3, hidden=(70,), lr=0.1, batch_size=32),
    [32, 40, 3], rows=ROWS3,
)
# weight decay, two epochs, a last batch of 6 and of 1, a 0-row shard
for _mn in sorted(MODES):
    _add(
        f"mlp_wd_epochs_{_mn}",
        MLPSpec(d_in=11, n_classes=3, hidden=(13,), lr=0.1, batch_size=32,
                weight_decay=0.05, local_epochs=2, mode=MODES[_mn]),
        [70, 65, 0, 32], rows=[(0, 4, (0, 2)), (1, 1, ()), (2, 2, (1,)),
                               (3, 1, ())],
    )
# limited merge, L = 2, single deliveries: node 0 keeps (9 > 3 + 2), node 1
# adopts (8 > 1 + 2), node 2 mixes 3:4, node 3 has a + b == 0; node 4's row
# of 4 deliveries walks through the rule with its growing age
for _mn in ("merge_update", "update_merge"):
    _add(
        f"mlp_limited_{_mn}",
        MLPSpec(d_in=11, n_classes=3, hidden=(13,), lr=0.1, batch_size=32,
                mode=MODES[_mn], age_diff_threshold=2),
        [20, 33, 7, 12, 40],
        rows=[(0, 1, ()), (1, 1, (0,)), (2, 1, ()), (3, 1, ()),
              (4, 4, (0, 2))],
        update=False, ages=[9, 1, 3, 0, 2],
        slot_ages=[3, 8, 4, 0, 2, 12, 14, 1],
    )

# ---- logreg rows wider than the 1024 prefetched floats (D = 1040) --------------
# node 0 (40 rows, 2 batches per update) starts at age 2 with L = 1: slot
# ages 2, 9, 11, 3 give MIX (fused first delivery), ADOPT (9 > 4 + 1), MIX
# (11 against 11) and KEEP (3 against 13) on the prefetched path
for _d, _k in ((64, 16), (129, 8)):
    _wide = dict(
        shards=[40, 33, 7, 12], rows=ROW_LONG + [(3, 1, (0,))], update=False,
        ages=[2, 0, 3, 1], slot_ages=[2, 9, 11, 3, 1, 6, 0, 5],
    )
    _add(f"wide_logreg_d{_d}_plain",
         LogRegSpec(d_in=_d, n_classes=_k, lr=0.1, batch_size=32), **_wide)
    _add(f"wide_logreg_d{_d}_limited",
         LogRegSpec(d_in=_d, n_classes=_k, lr=0.1, batch_size=32,
                    age_diff_threshold=1), **_wide)
    # pass-through: the 2nd delivery of the long row (on the prefetched
    # path) and the first of node 2's row (which leaves that path)
    _add(f"wide_logreg_d{_d}_pass_through",
         LogRegSpec(d_in=_d, n_classes=_k, lr=0.1, batch_size=32,
                    pass_through=True),
         flags=[0, 1, 0, 0, 0, 1, 0, 0], **_wide)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- building and running a case ----------------------------------------------

def events(case):
    """(recv, ptr, slots, reply, pids, n_slots) of the case's deliver."""
    recv, ptr, reply = [], [0], []
    for node, nd, rep in case.rows:
        recv.append(node)
        ptr.append(ptr[-1] + nd)
        reply += [1 if p in rep else 0 for p in range(nd)]
    nd = ptr[-1]
    nxt = nd
    for j, r in enumerate(reply):
        if r:
            reply[j], nxt = nxt, nxt + 1
        else:
            reply[j] = -1
    pids = None
    P = getattr(case.spec, "n_parts", 0)
    if P > 0:
        pids = torch.tensor([(2 * j + 1) % P for j in range(nd)])
    elif case.flags is not None:
        assert len(case.flags) == nd
        pids = torch.tensor(case.flags, dtype=torch.int64)
    def t(v):
        return torch.tensor(v, dtype=torch.int64)

    return t(recv), t(ptr), torch.arange(nd), t(reply), pids, nxt


def build(case, device=CPU):
    """Fresh (state, data, pool) of the case on ``device``; the values are
    generated on the CPU from the case's seed, so every device sees the
    same ones."""
    spec = case.spec
    g = torch.Generator().manual_seed(case.seed)
    n, aw = len(case.shards), spec.age_width if hasattr(spec, "age_width") else 1
    params = torch.randn(n, spec.D, generator=g) * 0.3
    ages = (torch.tensor(case.ages, dtype=torch.int32) if case.ages
            else torch.arange(n, dtype=torch.int32) % 5)
    shards = [
        (torch.randn(c, spec.d_in, generator=g),
         torch.randint(0, spec.n_classes, (c,), generator=g).float())
        for c in case.shards
    ]
    state = NodeStateArena(n, spec.D, device, age_width=aw)
    state.params.copy_(params)
    if aw > 1:  # partition p of node i starts at age (i + p) % 5
        ages = (ages[:, None] + torch.arange(aw, dtype=torch.int32)) % 5
    state.ages.copy_(ages)
    cd = DataArena.from_shards(shards, CPU)
    data = DataArena(cd.x.to(device), cd.y.to(device), cd.counts.to(device))
    pool = None
    if case.rows is not None:
        cap = events(case)[5]
        pool = SlotPool(spec.D, device, cap, age_width=aw)
        pool.slots.copy_(torch.randn(cap, spec.D, generator=g) * 0.3)
        sa = torch.arange(cap, dtype=torch.int32) * 2 % 7
        if case.slot_ages:
            sa[: len(case.slot_ages)] = torch.tensor(
                case.slot_ages, dtype=torch.int32)[:cap]
        if aw > 1:
            sa = (sa[:, None] + 2 * torch.arange(aw, dtype=torch.int32)) % 7
        pool.slot_ages.copy_(sa)
    return state, data, pool


def run_backend(backend, case, state, data, pool):
    nodes = torch.arange(len(case.shards))
    if case.update:
        backend.update(state, data, case.spec, nodes)
    if case.rows is not None:
        recv, ptr, slots, reply, pids, _ = events(case)
        backend.deliver(state, pool, data, case.spec, recv, ptr, slots, reply,
                        pids)


def run_ref(case, broken=None):
    """The float64 reference's final :class:`ref64.RefState` of the case."""
    state, data, pool = build(case)
    rs = ref64.RefState(state, data, pool)
    if case.update:
        ref64.update(case.spec, rs, range(len(case.shards)), broken)
    if case.rows is not None:
        recv, ptr, slots, reply, pids, _ = events(case)
        ref64.deliver(case.spec, rs, recv, ptr, slots, reply, pids, broken)
    return rs


def n_deliveries(case):
    return 0 if case.rows is None else sum(nd for _, nd, _ in case.rows)


def deviation(case, rs, state, pool):
    """Largest absolute deviation of a backend's (state, pool) from the
    reference over the params and the reply slots, after checking that the
    node ages and the reply slots' ages agree exactly. (The delivered slots
    are left out: the fp32 oracle trains a received model in place.)"""
    err = float((state.params.cpu().double() -
                 torch.from_numpy(rs.params)).abs().max())
    assert torch.equal(state.ages.cpu().long(), torch.from_numpy(rs.ages)), (
        case.name, state.ages.cpu().tolist(), rs.ages.tolist())
    if pool is not None:
        nd = n_deliveries(case)
        assert torch.equal(pool.slot_ages[nd:].cpu().long(),
                           torch.from_numpy(rs.slot_ages[nd:])), case.name
        if pool.slots.shape[0] > nd:
            err = max(err, float((pool.slots[nd:].cpu().double() -
                                  torch.from_numpy(rs.slots[nd:])).abs().max()))
    return err


# ---- evaluation cases -----------------------------------------------------------
# X and the models hold small integers, so every score is exact in fp32 and
# no argmax or rank can differ between fp32 and float64: the metrics must
# agree with the reference to EVAL_TOL in every entry.
EVAL_TOL = 1e-6
EVAL_SIZES = (1, 63, 64, 65, 255, 256, 257, 700)


@dataclass
class EvalCase:
    name: str
    spec: object
    params: torch.Tensor  # [R, D]
    X: torch.Tensor       # [n, d]
    y: torch.Tensor       # [n] class index, or -1 / +1 for a margin family


def _ints(g, shape, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def _logreg_eval(name, n, d, k, seed, R=3, zero=False, labels=None,
                 never=None, absent=None):
    g = torch.Generator().manual_seed(seed)
    spec = LogRegSpec(d_in=d, n_classes=k)
    params = _ints(g, (R, spec.D), -2, 2)
    if zero:
        params.zero_()
    if never is not None:  # class `never` loses every argmax
        params.view(R, -1)[:, never * d:(never + 1) * d] = 0.0
        params[:, k * d + never] = -1000.0
    X = _ints(g, (n, d), -2, 2)
    y = torch.randint(0, k, (n,), generator=g).float()
    if absent is not None:  # class `absent` has no sample
        y[y == absent] = float((absent + 1) % k)
    if labels is not None:
        y.fill_(labels)
    return EvalCase(name, spec, params, X, y)


def _margin_eval(name, n, d, seed, R=3):
    from gossipy_amd.engine import PegasosSpec

    g = torch.Generator().manual_seed(seed)
    spec = PegasosSpec(d_in=d)
    params = _ints(g, (R, spec.D), -1, 1)
    X = _ints(g, (n, d), -1, 1)  # d = 3: about a quarter of the scores is 0
    y = _ints(g, (n,), 0, 1) * 2 - 1
    return EvalCase(name, spec, params, X, y)


def _big_eval(name, distinct):
    # the n_eval limit: 1024 positives x 1024 negatives = 2^20 pairs
    spec = LogRegSpec(d_in=4, n_classes=2)
    g = torch.Generator().manual_seed(77)
    X = _ints(g, (2048, 4), -2, 2)
    params = torch.zeros(2, spec.D)
    if distinct:  # class-1 score = a permutation of 0..2047
        X[:, 0] = torch.randperm(2048, generator=g).float()
        params[:, 4] = 1.0          # class 1 reads feature 0
        params[1, 4] = -1.0         # the second model ranks them backwards
        params[:, 8] = 1000.0       # class 0 bias: argmax is not a tie
    y = (torch.randperm(2048, generator=g) < 1024).float()
    return EvalCase(name, spec, params, X, y)


def eval_cases():
    out = []
    for n in EVAL_SIZES:
        out.append(_logreg_eval(f"eval_zero_model_n{n}", n, 5, 2, 100 + n,
                                zero=True))
        out.append(_logreg_eval(f"eval_repeats_n{n}", n, 3, 2, 200 + n))
        out.append(_margin_eval(f"eval_margin_n{n}", n, 3, 300 + n))
    for lab in (0, 1):
        out.append(_logreg_eval(f"eval_all_label{lab}", 257, 3, 2, 400 + lab,
                                labels=float(lab)))
    for k in (3, 16):
        out.append(_logreg_eval(f"eval_k{k}_missing_classes", 257, 4, k,
                                500 + k, never=1, absent=k - 1))
    out.append(_big_eval("eval_2048_all_ties", False))
    out.append(_big_eval("eval_2048_all_distinct", True))
    # d = 512: the LDS budget leaves a tile of about 77 samples for n = 100
    out.append(_logreg_eval("eval_tile_smaller_than_n", 100, 512, 2, 600))
    return out


def eval_reference(case, row, X=None, y=None):
    """Reference metric dict of one model row on the case's eval set."""
    X = case.X if X is None else X
    y = case.y if y is None else y
    spec = case.spec
    if spec.family == "logreg":
        sc = ref64.logreg_scores(row.numpy(), X.numpy(), spec.d_in,
                                 spec.n_classes)
        return ref64.class_metrics(sc, y.numpy())
    return ref64.margin_metrics(
        X.double().numpy() @ row.double().numpy(), y.numpy())
