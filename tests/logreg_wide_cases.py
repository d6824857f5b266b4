"""Cases of the plain logreg tick past the LDS budget, for
``test_logreg_wide_cases.py`` (CPU: fp32 oracle against the float64
reference) and ``test_gpu_logreg_wide.py`` (MI355X: the wide kernel against
it). Not a test module. ``tick_cases.Case`` objects, built, run and compared
with that module's helpers. Every shape needs more than 160 KB for the
``tick_logreg_*`` kernels' ``4 * (2 * D + rows * d + rows * k)`` bytes:
784x10 with batches of 32 by 592 bytes, 561x6 by its batch of 200 rows,
3072x10 by its two model slabs alone, 700x2 by 257 rows (17 row tiles)."""

import functools

import tick_cases as tc
from gossipy_amd.engine import LogRegSpec

# every case: tol 1e-4, measured e32 (fp32 TorchBackend against the
# reference, CPU) between 0 (784_pass) and 3.0e-7, under tol / 8 = 1.25e-5

CASES = []


def _add(name, spec, shards, tol=1e-4, **kw):
    # seeds past the standing table's and the wide-MLP table's
    CASES.append(tc.Case(name, spec, shards, tol, seed=4001 + len(CASES), **kw))


def logreg(d, k, **kw):
    kw.setdefault("batch_size", 32)
    return LogRegSpec(d_in=d, n_classes=k, lr=0.1, **kw)


for _mn in ("merge_update", "update", "update_merge", "pass"):
    _add(  # last batches of 6 and of 1, an empty shard
        f"784_{_mn}",
        logreg(784, 10, weight_decay=0.05, local_epochs=2, mode=tc.MODES[_mn]),
        [70, 65, 0, 32],
        rows=[(0, 4, (0, 2)), (1, 1, ()), (2, 2, (1,)), (3, 1, ())],
    )
_add("har_full_batch", logreg(561, 6, batch_size=0), [200, 33, 7],
     rows=tc.ROWS3)
_add("cifar_D_only", logreg(3072, 10, batch_size=16), [20, 33, 7],
     rows=tc.ROWS3)
_add("k16", logreg(640, 16), [40, 33, 7], rows=tc.ROWS3)
_add("k2_rows", logreg(700, 2, batch_size=0), [129, 257, 17], rows=tc.ROWS3)
_add(  # ages, slot ages and rows of the standing mlp_limited_* cases
    "limited",
    logreg(784, 10, mode=tc.UM, age_diff_threshold=2),
    [20, 33, 7, 12, 40],
    rows=[(0, 1, ()), (1, 1, (0,)), (2, 1, ()), (3, 1, ()), (4, 4, (0, 2))],
    update=False, ages=[9, 1, 3, 0, 2], slot_ages=[3, 8, 4, 0, 2, 12, 14, 1],
)
_add(  # coins on the 2nd delivery of the long row and the 1st of node 2's
    "pass_through",
    logreg(784, 10, pass_through=True),
    [40, 33, 7, 12], rows=tc.ROW_LONG + [(3, 1, (0,))],
    flags=[0, 1, 0, 0, 0, 1, 0, 0],
)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


@functools.lru_cache(maxsize=None)
def reference(name):
    """The case's reference result, computed once and only read."""
    return tc.run_ref(BY_NAME[name])


def lds_plan_bytes(case):
    """Bytes of LDS the ``tick_logreg_*`` kernels need for the case."""
    spec = case.spec
    rows = min(spec.batch_size or max(case.shards), max(case.shards))
    return 4 * (2 * spec.D + rows * spec.d_in + rows * spec.n_classes)
