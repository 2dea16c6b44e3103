"""CPU: the host side of gsr_knn_workspace / gsr_knn_mean_dist2 / gsr_knn_stages (include/gsr.h).
The loaded library refuses bad arguments before any HIP call, so no device is needed."""
import re
import os

import pytest

from gaussiansplattingviewer_amd import _lib

FAKE = 0x1000  # a non-NULL pointer nothing dereferences: every call below is refused first
INVALID = -1   # GSR_E_INVALID
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include",
                      "gsr.h")


def _fns():
    return _lib.knn_fns(_lib.load_library())


def test_the_entries_are_declared_exported_and_bound():
    lib = _lib.load_library()
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    for name in _lib.KNN_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(lib, name), name
    assert _lib.KNN_SYMBOLS == ("gsr_knn_workspace", "gsr_knn_mean_dist2", "gsr_knn_stages")
    ws, knn, stages = _fns()
    assert ws is lib.gsr_knn_workspace and knn is lib.gsr_knn_mean_dist2
    assert len(knn.argtypes) == 5 and len(stages.argtypes) == 6 and len(ws.argtypes) == 1
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4  # additive

    class Older:
        gsr_densify_plan = object()

    with pytest.raises(RuntimeError, match="no gsr_knn_workspace"):
        _lib.knn_fns(Older())


REFUSALS = {
    "xyz": (None, 10, FAKE, FAKE),
    "dist2": (FAKE, 10, None, FAKE),
    "workspace": (FAKE, 10, FAKE, None),
    "N_negative": (FAKE, -1, FAKE, FAKE),
    "N_2_30": (FAKE, 2 ** 30, FAKE, FAKE),
    "N_huge": (FAKE, 2 ** 40, FAKE, FAKE),
}


@pytest.mark.parametrize("case", sorted(REFUSALS))
def test_refusals(case):
    lib = _lib.load_library()
    _, knn, stages = _fns()
    assert lib.gsr_forward(None, None, None, None, None) < 0  # another entry's message
    assert knn(*REFUSALS[case], None) == INVALID
    assert b"gsr_knn_mean_dist2" in lib.gsr_last_error()
    assert lib.gsr_forward(None, None, None, None, None) < 0
    assert stages(*REFUSALS[case], 2, None) == INVALID
    assert b"gsr_knn_stages" in lib.gsr_last_error()


@pytest.mark.parametrize("n_stages", [0, 5, -1])
def test_stage_count_refusals(n_stages):
    _, _, stages = _fns()
    assert stages(FAKE, 10, FAKE, FAKE, n_stages, None) == INVALID
    assert b"gsr_knn_stages" in _lib.load_library().gsr_last_error()


def test_empty_cloud_is_ok_without_a_launch():
    _, knn, stages = _fns()
    assert knn(None, 0, None, None, None) == 0
    assert stages(None, 0, None, None, 3, None) == 0
    assert stages(None, 0, None, None, 0, None) == INVALID  # refusals come first


def test_workspace_size():
    lib = _lib.load_library()
    ws = _fns()[0]
    for bad in (-1, 2 ** 30, 2 ** 62):
        assert lib.gsr_forward(None, None, None, None, None) < 0
        assert ws(bad) == INVALID
        assert b"gsr_knn_workspace" in lib.gsr_last_error()
    sizes = [ws(N) for N in (0, 1, 2, 255, 256, 257, 1000, 4096, 4097, 10 ** 6, 2 ** 30 - 1)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[-1] < 40 * 2 ** 30  # about 32 bytes per point
    assert 32 * 10 ** 6 <= ws(10 ** 6) < 34 * 10 ** 6
