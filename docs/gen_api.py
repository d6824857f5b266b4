"""Generate the API reference (docs/api/*.md) from the package's
docstrings — stdlib-only (the image has no sphinx/pdoc).

Usage: python docs/gen_api.py
"""

import importlib
import inspect
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODULES = [
    "gossipy_amd",
    "gossipy_amd.core",
    "gossipy_amd.simul",
    "gossipy_amd.node",
    "gossipy_amd.flow_control",
    "gossipy_amd.utils",
    "gossipy_amd.model",
    "gossipy_amd.model.nn",
    "gossipy_amd.model.handler",
    "gossipy_amd.model.sampling",
    "gossipy_amd.data",
    "gossipy_amd.data.handler",
    "gossipy_amd.engine",
    "gossipy_amd.engine.arena",
    "gossipy_amd.engine.models",
    "gossipy_amd.engine.schedule",
    "gossipy_amd.engine.runner",
    "gossipy_amd.engine.backend",
    "gossipy_amd.engine.metrics",
    "gossipy_amd.engine.rng",
    "gossipy_amd.ops",
    "gossipy_amd.ops.build",
]


def _sig(obj):
    try:
        return str(inspect.signature(obj))
    except (ValueError, TypeError):
        return "(...)"


def _doc(obj, indent=""):
    d = inspect.getdoc(obj)
    if not d:
        return ""
    return "\n".join(indent + line for line in d.splitlines()) + "\n"


def render_module(name: str) -> str:
    mod = importlib.import_module(name)
    out = [f"# `{name}`\n"]
    md = inspect.getdoc(mod)
    if md:
        out.append(md + "\n")
    public = getattr(mod, "__all__", None)
    members = inspect.getmembers(mod)
    for mname, obj in members:
        if public is not None and mname not in public:
            continue
        if public is None and mname.startswith("_"):
            continue
        if inspect.ismodule(obj):
            continue
        owner = getattr(obj, "__module__", None)
        if owner is not None and not str(owner).startswith("gossipy_amd"):
            continue
        if inspect.isclass(obj):
            out.append(f"## class `{mname}{_sig(obj)}`\n")
            out.append(_doc(obj))
            for aname, attr in inspect.getmembers(obj):
                if aname.startswith("_") or not (
                    inspect.isfunction(attr) or isinstance(
                        attr, (classmethod, staticmethod, property)
                    )
                ):
                    continue
                if isinstance(attr, property):
                    out.append(f"### property `{mname}.{aname}`\n")
                    out.append(_doc(attr.fget) if attr.fget else "")
                    continue
                fn = attr.__func__ if isinstance(
                    attr, (classmethod, staticmethod)
                ) else attr
                if not _doc(fn):
                    continue
                out.append(f"### `{mname}.{aname}{_sig(fn)}`\n")
                out.append(_doc(fn))
        elif inspect.isfunction(obj):
            out.append(f"## `{mname}{_sig(obj)}`\n")
            out.append(_doc(obj))
    return "\n".join(out)


def main():
    api_dir = os.path.join(ROOT, "docs", "api")
    os.makedirs(api_dir, exist_ok=True)
    index = ["# gossipy_amd API reference\n",
             "Generated from docstrings by `docs/gen_api.py`.\n"]
    for name in MODULES:
        fname = name.replace(".", "_") + ".md"
        with open(os.path.join(api_dir, fname), "w") as f:
            f.write(render_module(name))
        index.append(f"- [`{name}`](api/{fname})")
        print("wrote", fname)
    with open(os.path.join(ROOT, "docs", "API.md"), "w") as f:
        f.write("\n".join(index) + "\n" + COMPRESSION_NOTE)


#: hand-written section of the index: which compression scheme runs on which
#: engine model family (kept here so regenerating API.md preserves it)
COMPRESSION_NOTE = """
## Compressed gossip by model family

Hegedus 2021's two compression schemes are spec fields plus a matching
`EngineConfig` switch; both run on the torch oracle and, on one GPU, on the
HIP kernels (per-tick path and whole-round executor), with the plain and the
tokenized simulators. The multi-rank route is the model-agnostic one: for
the MLP variants it is tested on the CPU oracle (two gloo ranks, bit-equal
to one rank) and has not been run on more than one GPU.

| scheme | spec | config | `LogRegSpec` | `MLPSpec` | other families |
|---|---|---|---|---|---|
| partitioned (`PartitionedTMH`) | `n_parts=P` | `EngineConfig(n_parts=P)` | yes | yes | `ValueError` |
| sampled (`SamplingTMH`) | `sample_size=f` | `EngineConfig(sampled=True)` | yes | yes | `ValueError` |
| limited merge (`LimitedMergeTMH`) | `age_diff_threshold=L` | none | yes | yes | `TorchModuleSpec`: torch only; others `ValueError` on HIP |

Limited merge (Danner 2023) is no compression scheme but lives in the same
place, the merge: with `a` the receiver's age and `b` the received model's,
the receiver keeps its model when `a > b + L`, adopts the received one when
`b > a + L`, and otherwise averages with weights `a/(a+b)` and `b/(a+b)`
(`(1/2, 1/2)` when both ages are 0, where the reference divides by zero).
`None` is the plain mean. It needs no config switch, combines with
`pass_through` (a PASS delivery still adopts) and not with `n_parts` or
`sample_size`; the PENS and all2all simulators refuse it. On HIP it runs in
second instantiations of the logreg and MLP tick kernels, per tick and
through the stream whole-round executor; the opt-in cooperative and
single-workgroup rounds are not extended and are bypassed. The extension's
`tick_logreg`, `tick_mlp`, `run_round_logreg` and `run_round_mlp` take the
threshold as `merge_limit` directly after `mode`, always: `-1` is the plain
mean.

`n_parts` and `sample_size` are mutually exclusive, and `MLPSpec` rejects
either together with `pass_through=True` (`ValueError`): PASS is an error
for both handlers. Modes `MERGE_UPDATE`, `UPDATE` and `UPDATE_MERGE` are
supported. Partitioned runs keep `[n_nodes, P]` ages. The MLP kernels hold
the model row (two rows outside `MERGE_UPDATE`), one batch of activations
and two gradient buffers in LDS and refuse shapes over 160 KiB per block;
shrink `batch_size` or `hidden` when that check fires.

## The extension's whole-round ops

Every `run_round_<family>` op of the HIP extension starts with the same
block: `params, ages, slots, slot_ages`, then the round as one upload
(`round_buf`, a 1-D int32 device tensor holding the round's event arrays back
to back, and `lens`, their lengths), then `snap_tptr, recv_tptr, pull_tptr,
rep_tptr` (int32, on the host; on the device for `run_round_coop_logreg`),
then `X, Y, counts`; the family's own arguments follow. Which arrays, and in
which order, is the extension's `ROUND_ARRAY_NAMES` (14 names) and
`ROUND_TPTR_NAMES`, exported by `_gossip_sched` as well and defined once in
`csrc/round_source.h`. A call whose `round_buf` is not a contiguous int32
device tensor, whose `lens` has another count, a negative entry or a sum past
the buffer, or whose tick pointers are empty or differ in length raises
`RuntimeError` and launches nothing.

## Launch order within a round

The native scheduler hands a round over as launch groups. Its default packer
merges ticks greedily, so a launch lasts as long as its longest receiver row.
`NativeSchedulerAdapter.set_pack_levels(cap)` orders the rounds generated
after the call by dependency level instead (`csrc/round_levels.h`): a
delivery runs in the first launch after the previous delivery to its
receiver and after the delivery that produced the state its slot holds, at
most `cap` deliveries per row, so the launches of a round add up to its
critical path. Every delivery computes what it computed before; results are
bit-equal. Rounds with pull or reply events (PULL, PUSH_PULL) keep the
default packer; `pack_level_stats()` counts both kinds. `start()` turns it
on, with `cap = 1`, on the single-rank HIP fast path for logreg (plain,
partitioned, limited merge) and pegasos/adaline, and leaves it off for the
other families; `GOSSIPY_PACK_LEVELS=0` turns it off and
`GOSSIPY_PACK_LEVELS=<cap>` sets the cap for every family of that path.
Multi-rank runs, the tokenized, PENS and all2all simulators and the torchmod
group replay never use it. Measurements: `profiles/level_packing.md`.
"""


if __name__ == "__main__":
    main()
