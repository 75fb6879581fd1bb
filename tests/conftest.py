import functools
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    if has_gpu():
        # torch's HIP runtime and the product's share the process: start torch's before anything loads the product's library, the order
        # bench.py has.  Loaded the other way round with the CPU tests in between, one of the two runtimes is left without a device.
        import torch
        torch.cuda.init()


@pytest.fixture(scope="session", autouse=True)
def _built():
    """Native libraries are built in-tree by __graft_entry__.build(); build them if this checkout has none yet."""
    from rfw_rs_amd import HIP_LIB, HOST_LIB
    from oracle.bindings import ORACLE_LIB
    if not (os.path.exists(HIP_LIB) and os.path.exists(HOST_LIB) and os.path.exists(ORACLE_LIB)):
        import __graft_entry__
        __graft_entry__.build()


@functools.lru_cache(maxsize=None)
def has_gpu():
    """Asked in a child process, so that the test process starts torch's HIP runtime only where pytest_configure does."""
    import subprocess
    r = subprocess.run([sys.executable, "-c", "import torch, sys; sys.exit(0 if torch.cuda.is_available() else 1)"],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return r.returncode == 0


def rel_l2(a, b):
    import numpy as np
    return float(np.linalg.norm(a.astype(np.float64) - b.astype(np.float64)) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))
