"""CPU test of ``kmeans_match_cases.py``: the replay's discrete choices clear
``MARGIN``, and the fp32 ``TorchBackend`` loop agrees with it to 1e-5 (some
hundred roundings of values in [0, 1); another permutation shows as 1e-2)."""

import pytest

import kmeans_match_cases as kc
from gossipy_amd.engine.backend import TorchBackend


@pytest.mark.parametrize("case", kc.CASES, ids=kc.IDS)
def test_margins_and_oracle(case):
    ref = kc.replay(case)
    assert ref[4] >= kc.MARGIN and ref[5] >= kc.MARGIN
    state, pool, data = kc.build(case)
    kc.deliver(TorchBackend(), case, state, pool, data)
    assert kc.deviation(ref, state, pool) <= 1e-5
