import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(REPO, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (HIP) device; runs the HIP kernels")


@pytest.fixture(scope="session")
def golden():
    def load(name):
        return np.load(os.path.join(GOLDEN, name))
    return load


@pytest.fixture(scope="session")
def sort_backend(golden):
    """The reference's sort-backend vectors (make_golden.save_sort_backend stores them in three
    files) as one dict with the keys they were captured under."""
    g = dict(golden("sort_backend.npz"))
    a, b = golden("sort_backend_100k_a.npz"), golden("sort_backend_100k_b.npz")
    g["100k_front__index"] = a["100k_front__index"]
    g["xyz_100k"] = np.concatenate([a["xyz_100k__rows0"], b["xyz_100k__rows1"]])
    return g


@pytest.fixture(scope="session")
def oracle_mod():
    import oracle
    oracle.lib()
    return oracle


@pytest.fixture(scope="session")
def gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("GPU test collected but no HIP device is visible")
    return torch.device("cuda", 0)
