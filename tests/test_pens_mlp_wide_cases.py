"""CPU test of ``pens_mlp_wide_cases.py``: every case meets its input
conditions on the float64 forward, and fp32 ``TorchBackend.deliver_pens`` is
within ``TOL / 8`` of the replay with equal ages and winner counts."""

import pytest

import pens_mlp_wide_cases as pc
from gossipy_amd.engine.backend import TorchBackend


@pytest.mark.parametrize("name", [c.name for c in pc.CASES])
def test_inputs_and_oracle_within_an_eighth_of_tol(name):
    pc.check_inputs(name)
    case = pc.BY_NAME[name]
    state, data, pool, counts = pc.build(case)
    pc.run_backend(TorchBackend(), case, state, data, pool, counts)
    assert pc.compare(name, state, counts) <= pc.TOL / 8
