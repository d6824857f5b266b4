"""Cases of the plain MLP tick past the LDS budget, shared by
``test_mlp_wide_cases.py`` (CPU: fp32 oracle against the float64 reference)
and ``test_gpu_mlp_wide.py`` (MI355X: the global-resident wide kernel
against the same reference). Not a test module.

The cases are ``tick_cases.Case`` objects and are built, run and compared
with that module's helpers; ``tol`` and ``e32`` mean what they mean there.
Every shape misses ``tick_mlp_kernel``'s budget of 160 KB of LDS:

* 784-100-10 (D = 79,510 floats, 318 KB), the MNIST-shaped classifier: every
  mode with weight decay, two epochs, last batches of 6 and of 1 and a 0-row
  shard; limited merge; pass-through coins; one full batch of 200 rows,
  whose activations and gradients miss the LDS budget too (248 KB) and move
  to the kernel's workspace;
* 300-140-3 (D = 42,563 floats, 170 KB): the model row alone overflows, the
  staging of a batch of 16 would fit many times over;
* 784-64-33-10: three layers, a hidden dX with K = 33.
"""

from typing import List

import tick_cases as tc
from gossipy_amd.engine import MLPSpec

# tol and the measured e32 (fp32 TorchBackend against the reference, CPU):
#   case                               tol     e32
#   wide_mlp_784_merge_update          1e-4    3.800e-07
#   wide_mlp_784_update                1e-4    9.636e-07
#   wide_mlp_784_update_merge          1e-4    1.117e-06
#   wide_mlp_784_pass                  1e-4    0.000e+00
#   wide_mlp_D_only                    1e-4    4.339e-07
#   wide_mlp_three_layers              1e-4    1.765e-06
#   wide_mlp_limited                   1e-4    7.586e-07
#   wide_mlp_full_batch                1e-4    1.750e-06
#   wide_mlp_pass_through              1e-4    (below)
# e32 is larger here than in the standing table: a row of 784 standard
# normal inputs makes a step's Jacobian about 0.1 * 784, so the rounding of
# one step is amplified by the next ones. All stay under tol / 8 = 1.25e-5.
#
# wide_mlp_full_batch does not take its seed from its position. With that
# seed (1008) one hidden unit's pre-activation of one of the 200 rows is
# zero to within fp32 rounding: the fp32 oracle and the float64 reference
# take different sides of the ReLU, and e32 is 6.8e-4 in that unit's 785
# parameters alone (median over the row 4e-9). Such a case measures a coin
# toss, not a kernel, whatever the bound. Seed 2008, the next one tried,
# has no such row.

CASES: List[tc.Case] = []


def _add(name, spec, shards, tol=1e-4, seed=None, **kw):
    assert len(shards) <= 6
    # seeds past the standing table's, which uses the case's position
    seed = 1001 + len(CASES) if seed is None else seed
    CASES.append(tc.Case(name, spec, shards, tol, seed=seed, **kw))


def mnist_mlp(**kw):
    kw.setdefault("hidden", (100,))
    kw.setdefault("batch_size", 32)
    return MLPSpec(d_in=784, n_classes=10, lr=0.1, **kw)


for _mn in ("merge_update", "update", "update_merge", "pass"):
    _add(
        f"wide_mlp_784_{_mn}",
        mnist_mlp(weight_decay=0.05, local_epochs=2, mode=tc.MODES[_mn]),
        [70, 65, 0, 32],
        rows=[(0, 4, (0, 2)), (1, 1, ()), (2, 2, (1,)), (3, 1, ())],
    )
_add(
    "wide_mlp_D_only",
    MLPSpec(d_in=300, n_classes=3, hidden=(140,), lr=0.1, batch_size=16),
    [20, 33, 7], rows=tc.ROWS3,
)
_add(
    "wide_mlp_three_layers",
    mnist_mlp(hidden=(64, 33)),
    [40, 33, 7], rows=tc.ROWS3,
)
_add(  # ages, slot ages and rows of the standing mlp_limited_* cases
    "wide_mlp_limited",
    mnist_mlp(mode=tc.UM, age_diff_threshold=2),
    [20, 33, 7, 12, 40],
    rows=[(0, 1, ()), (1, 1, (0,)), (2, 1, ()), (3, 1, ()), (4, 4, (0, 2))],
    update=False, ages=[9, 1, 3, 0, 2],
    slot_ages=[3, 8, 4, 0, 2, 12, 14, 1],
)
_add(  # one batch of 200 rows: 200 * (110 + 2 * 100) floats = 248 KB
    "wide_mlp_full_batch",
    mnist_mlp(batch_size=0),
    [200, 33, 7], rows=tc.ROWS3, seed=2008,
)
_add(  # coins on the 2nd delivery of the long row and the 1st of node 2's
    "wide_mlp_pass_through",
    mnist_mlp(pass_through=True),
    [40, 33, 7, 12], rows=tc.ROW_LONG + [(3, 1, (0,))],
    flags=[0, 1, 0, 0, 0, 1, 0, 0],
)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

_REF = {}


def reference(name):
    """The case's reference result, computed once and only read."""
    if name not in _REF:
        _REF[name] = tc.run_ref(BY_NAME[name])
    return _REF[name]
