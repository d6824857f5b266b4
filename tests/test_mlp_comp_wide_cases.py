"""CPU test of ``mlp_comp_wide_cases.py``: the fp32 ``TorchBackend`` oracle
is within ``tol / 8`` of the float64 reference on every case, ages equal."""

import pytest

import mlp_comp_wide_cases as cw
import tick_cases as tc
from gossipy_amd.engine.backend import TorchBackend


@pytest.mark.parametrize("name", [c.name for c in cw.CASES])
def test_oracle_within_an_eighth_of_tol(name):
    case = cw.BY_NAME[name]
    assert case.tol >= 1e-4 and case.seed >= 4001
    state, data, pool = tc.build(case)
    tc.run_backend(TorchBackend(), case, state, data, pool)
    e32 = tc.deviation(case, cw.reference(name), state, pool)
    print(f"e32 {name} {e32:.3e} tol {case.tol:.1e}")
    assert e32 <= case.tol / 8, (name, e32)
