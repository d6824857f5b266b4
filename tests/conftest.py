"""Shared pytest configuration.

Registers the ``gpu`` marker: tests that need a real MI355X are marked
``@pytest.mark.gpu`` and are skipped on CPU-only machines; everything else
must pass without a GPU.
"""

import atexit
import os
import shutil
import tempfile

# The multi-rank tests assert that a gloo run is BIT-identical to the
# single-rank run. Each rank holds its block of the data arena, so the same
# node's rows sit at a different address alignment in the two runs. MKL's
# default sgemm picks its code path by operand alignment on some hosts
# (observed on AMD EPYC: 1-ulp differences between 4-byte-shifted copies of
# the same matrix), which breaks bit-identity for reasons unrelated to the
# engine. MKL's conditional-numerical-reproducibility mode makes the result
# independent of alignment; it must be in the environment before MKL starts
# (i.e. before torch is imported) and is inherited by the spawned ranks.
os.environ.setdefault("MKL_CBWR", "AUTO")

# MIOpen appends what it finds to its user DB. The engine points MIOpen at
# the pre-tuned DB shipped in the package, so a test run would rewrite
# tracked files: give the tests (and the example scripts they spawn) a
# scratch copy instead — same tuned entries, writes land outside the tree.
if "MIOPEN_USER_DB_PATH" not in os.environ:
    _udb_src = os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
        "gossipy_amd", "ops", "miopen_udb",
    )
    if os.path.isdir(_udb_src):
        _udb_tmp = tempfile.mkdtemp(prefix="gossipy_miopen_udb_")
        atexit.register(shutil.rmtree, _udb_tmp, ignore_errors=True)
        shutil.copytree(_udb_src, _udb_tmp, dirs_exist_ok=True)
        os.environ["MIOPEN_USER_DB_PATH"] = _udb_tmp

import pytest  # noqa: E402
import torch  # noqa: E402


def pytest_configure(config):
    config.addinivalue_line(
        "markers", "gpu: test requires a GPU (run on the MI355X box)"
    )


def pytest_collection_modifyitems(config, items):
    if torch.cuda.is_available():
        return
    skip_gpu = pytest.mark.skip(reason="no GPU on this machine")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip_gpu)


@pytest.fixture(autouse=True)
def _clear_global_cache():
    """Each test starts with an empty model cache."""
    from gossipy_amd import CACHE

    CACHE.clear()
    yield
    CACHE.clear()
