"""Cases of the compressed MLP tick on ``tick_mlp_comp_wide_kernel`` for
``test_mlp_comp_wide_cases.py`` (CPU) and ``test_gpu_mlp_comp_wide.py``; not a
test module. ``tick_cases.Case`` objects, ``tol`` and ``e32`` as there.
Partitioned cases go against ``ref64``, sampled ones against
``_run_samp_ref`` with the sample seeds in ``Case.flags``.

11-20-3 (D = 303): ``tc.events`` draws odd partition ids only, so besides four
partitions (1: ragged first and last column; 3: layer 0's biases through all
of layer 1) there are three (0: from 0 to mid-column; 2: weights into biases
into the next layer), 40 (inside one column) and 1. 303 draws from 303 repeat
indices, and the bitmap's last word is partial. 784-100-10 misses the LDS
kernel's budget: ``W2`` in the workspace, a 0-row shard, a batch of 200 rows
whose activations move there too."""

import functools

import ref64
import tick_cases as tc
from gossipy_amd.engine import MLPSpec
from gossipy_amd.engine.rng import sample_indices

# tol is 1e-4 throughout; the measured e32 (fp32 TorchBackend against the
# reference, CPU), all under tol / 8 = 1.25e-5, no 784 case on a ReLU coin toss:
#   part4_merge_update 2.161e-07   samp03_merge_update 1.564e-07
#   samp10_merge_update 2.164e-07   part4_update 8.173e-08
#   samp03_update 9.926e-08   samp10_update 7.271e-08
#   part4_update_merge 1.676e-07   samp03_update_merge 1.841e-07
#   samp10_update_merge 1.096e-07   part3 1.589e-07
#   part40 2.748e-07   part1 1.095e-07
#   part4_three_layers 2.506e-07   wide_784_part4 2.585e-07
#   wide_784_samp01 7.025e-07   wide_784_part4_full_batch 1.272e-07

CASES = []

ROWS = [(0, 4, (0, 2)), (1, 1, ()), (2, 2, (1,)), (3, 1, ())]
SEEDS = [11, 2 ** 31 - 5, 7, 123456789, 42, 99991, 3, 2 ** 30 + 1]


def _add(name, spec, shards, rows, tol=1e-4):
    flags = SEEDS[: sum(nd for _, nd, _ in rows)] if spec.sample_size else None
    CASES.append(tc.Case(name, spec, shards, tol, rows=rows, flags=flags,
                         seed=4001 + len(CASES)))


def small(hidden=(20,), **kw):
    return MLPSpec(d_in=11, n_classes=3, hidden=hidden, lr=0.1, batch_size=8,
                   local_epochs=2, weight_decay=0.01, **kw)


def mnist(batch_size=32, **kw):
    return MLPSpec(d_in=784, n_classes=10, hidden=(100,), lr=0.1,
                   batch_size=batch_size, **kw)


SH = [20, 9, 0, 13]
for _mn in ("merge_update", "update", "update_merge"):
    _add(f"part4_{_mn}", small(n_parts=4, mode=tc.MODES[_mn]), SH, ROWS)
    _add(f"samp03_{_mn}", small(sample_size=0.3, mode=tc.MODES[_mn]), SH, ROWS)
    _add(f"samp10_{_mn}", small(sample_size=1.0, mode=tc.MODES[_mn]), SH, ROWS)
for _p in (3, 40, 1):
    _add(f"part{_p}", small(n_parts=_p, mode=tc.UM), SH, ROWS)
_add("part4_three_layers", small(hidden=(20, 12), n_parts=4, mode=tc.UM), SH,
     ROWS)
_add("wide_784_part4", mnist(n_parts=4, mode=tc.UM), [40, 33, 0, 7], ROWS)
_add("wide_784_samp01", mnist(sample_size=0.1), [40, 33, 0, 7], ROWS)
_add("wide_784_part4_full_batch", mnist(n_parts=4, batch_size=0),
     [200, 33, 7], tc.ROWS3)

BY_NAME = {c.name: c for c in CASES}


def _run_samp_ref(case):
    """float64 replay: a sampled index gets the mean of the pre-merge values,
    UPDATE modes train a copy of the received model, ages are never merged."""
    spec, rs = case.spec, ref64.RefState(*tc.build(case))
    if case.update:
        ref64.update(spec, rs, range(len(case.shards)))
    recv, ptr, slots, reply, seeds, _ = tc.events(case)
    for i, node in enumerate(recv.tolist()):
        (x, y), row, age = rs.shard(node), rs.params[node], rs.ages[node]
        for j in range(int(ptr[i]), int(ptr[i + 1])):
            src = rs.slots[int(slots[j])].copy()
            if spec.mode != tc.MU:
                if spec.mode == tc.UM:
                    age = ref64._train(spec, row, age, x, y)
                ref64._train(spec, src, 0, x, y)
            idx = sample_indices(int(seeds[j]), spec.samp_count(), spec.D)
            row[idx] = 0.5 * (row[idx] + src[idx])
            if spec.mode == tc.MU:
                age = ref64._train(spec, row, age, x, y)
            if int(reply[j]) >= 0:
                rs.slots[int(reply[j])] = row
                rs.slot_ages[int(reply[j])] = age
        rs.ages[node] = age
    return rs


def _run_part_ref(case):
    """``tc.run_ref``, with the flat ages of a single partition as the
    ``[*, 1]`` columns ``ref64`` indexes by partition."""
    rs = ref64.RefState(*tc.build(case))
    shapes = rs.ages.shape, rs.slot_ages.shape
    rs.ages = rs.ages.reshape(shapes[0][0], -1)
    rs.slot_ages = rs.slot_ages.reshape(shapes[1][0], -1)
    if case.update:
        ref64.update(case.spec, rs, range(len(case.shards)))
    recv, ptr, slots, reply, pids, _ = tc.events(case)
    ref64.deliver(case.spec, rs, recv, ptr, slots, reply, pids)
    rs.ages = rs.ages.reshape(shapes[0])
    rs.slot_ages = rs.slot_ages.reshape(shapes[1])
    return rs


@functools.lru_cache(None)
def reference(name):
    """The case's reference result, computed once and only read."""
    run = _run_samp_ref if BY_NAME[name].spec.sample_size else _run_part_ref
    return run(BY_NAME[name])
