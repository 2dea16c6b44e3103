"""GPU: the tile ranges taken from the row pass (radix_sort.hip tile_starts_block and k_tile_runs) against the
oracle's literal 64-bit sort, on the smallest frames where they can go wrong: 16 x 12 tiles, lists
of 4-7 sort tiles of 4096 entries with the tile columns' boundaries inside them
(tests/tile_start_scenes.py; test_tile_start_scenes.py checks the scenes with the oracle alone).

Covered: trailing, leading and consecutive empty tile columns, empty tiles inside full columns,
a partly filled last sort tile, an image size that is no multiple of 16, strips of one tile row
(no row pass: the ranges are the column runs) and of two, a frame without a visible Gaussian,
tight binning on and off, GSR_OPT_FRAME_GRAPHS 0, 1 and 2 with and without the second stream,
and a capacity overflow that is rendered again.

A column boundary exactly on a sort-tile boundary: none of the sweep's 20 seeds hits one
(test_tile_start_scenes.py::test_seed_sweep_boundaries asserts that count), so
test_aligned_column_boundary renders a scene built to have one.
"""
import numpy as np
import pytest

from gaussiansplattingviewer_amd import _lib

import tile_start_scenes as ts
from gpu_helpers import (assert_image_close, assert_parity, run_hip, run_oracle, set_option,
                         tight_binning)
from test_gpu_tight_pin import pin_tight_lists

pytestmark = pytest.mark.gpu

_orc = {}


def _oracle(oracle_mod, key, build):
    """(scene, oracle result) of a named scene, computed once."""
    if key not in _orc:
        s = build()
        _orc[key] = (s, run_oracle(oracle_mod, s))
    return _orc[key]


def _kind(oracle_mod, kind):
    return _oracle(oracle_mod, kind, lambda: ts.scene(kind))


LEAN = ("final_T", "n_contrib")  # upstream's full lists, and a frame the graphs may take (no rgb)


def _check_lists(hip, orc, rows=None):
    """assert_parity's integer outputs, lists and image for a forward with the LEAN extras."""
    y = slice(None) if rows is None else slice(rows[0] * 16, rows[1] * 16)
    if rows is None:
        assert hip["num_rendered"] == orc["num_rendered"]
        np.testing.assert_array_equal(hip["point_list"], orc["point_list"])
        np.testing.assert_array_equal(hip["point_tiles"],
                                      (orc["point_keys"] >> np.uint64(32)).astype(np.uint32))
        np.testing.assert_array_equal(hip["ranges"], orc["ranges"])
    np.testing.assert_array_equal(hip["radii"], orc["radii"])
    assert_image_close(hip["color"], orc["color"][:, y])
    assert_image_close(hip["final_T"], orc["final_T"][y], "final_T")
    mism = float((hip["n_contrib"] != orc["n_contrib"][y]).mean())
    assert mism <= 1e-4, f"n_contrib differs at {mism:.2e} of pixels"


def _check_tight(gpu, oracle_mod, s, orc, slot=0):
    """A forward without n_contrib (tight lists): subsequences of the oracle's lists that drop
    only pairs no pixel sees, ranges and tile ids consistent, and the image."""
    hip = run_hip(s, gpu, extras=(), slot=slot)
    pin_tight_lists(oracle_mod, orc, hip, s["W"], s["H"])
    assert_image_close(hip["color"], orc["color"])
    return hip


@pytest.mark.parametrize("kind", sorted(ts.KINDS))
def test_scene_ranges_and_lists(gpu, oracle_mod, kind):
    s, orc = _kind(oracle_mod, kind)
    assert_parity(run_hip(s, gpu), orc)  # n_contrib requested: upstream's full lists
    tight = _check_tight(gpu, oracle_mod, s, orc)
    with tight_binning(gpu, 0):  # the full lists again, through the forward without n_contrib
        off = run_hip(s, gpu, extras=())
    for k in ("point_list", "point_tiles", "ranges"):
        np.testing.assert_array_equal(off[k], orc[k] if k != "point_tiles" else
                                      (orc["point_keys"] >> np.uint64(32)).astype(np.uint32))
    assert_image_close(off["color"], orc["color"])
    if kind != "none":
        assert len(tight["point_list"]) < len(off["point_list"])


def test_image_size_not_a_multiple_of_16(gpu, oracle_mod):
    s, orc = _oracle(oracle_mod, "odd", lambda: ts.scene("full", w=250, h=187))
    assert_parity(run_hip(s, gpu), orc)
    _check_tight(gpu, oracle_mod, s, orc)


def test_aligned_column_boundary(gpu, oracle_mod):
    s, orc = _oracle(oracle_mod, "aligned", lambda: ts.aligned_boundary_scene(oracle_mod)[0])
    assert_parity(run_hip(s, gpu), orc)


@pytest.mark.parametrize("seed", range(20))
def test_seed_sweep(gpu, oracle_mod, seed):
    s = ts.scene("full", seed=seed)
    assert_parity(run_hip(s, gpu), run_oracle(oracle_mod, s))


def _check_strip(gpu, s, orc, rows, slot=0):
    """A strip's ranges, lists and image rows against the full-frame oracle result."""
    part = run_hip(s, gpu, tile_rows=rows, extras=LEAN, slot=slot)
    tiles = (orc["point_keys"] >> np.uint64(32)).astype(np.uint32)
    t0, t1 = rows[0] * ts.GX, rows[1] * ts.GX
    before = int((tiles < t0).sum())
    want = orc["ranges"].reshape(-1, 2).astype(np.int64).copy()
    nonempty = want[:, 1] > want[:, 0]
    want[nonempty] -= before
    want[:t0] = 0
    want[t1:] = 0
    np.testing.assert_array_equal(part["ranges"].reshape(-1, 2), want)
    sel = (tiles >= t0) & (tiles < t1)
    np.testing.assert_array_equal(part["point_list"], orc["point_list"][sel])
    np.testing.assert_array_equal(part["point_tiles"], tiles[sel])
    _check_lists(part, orc, rows)


def _big(oracle_mod):
    return _oracle(oracle_mod, "big", lambda: ts.scene("full", P=12000, seed=3))


@pytest.mark.parametrize("rows", [(5, 6), (5, 7), (0, 1), (11, 12)])
@pytest.mark.parametrize("kind", ["big", "band"])
def test_strips_of_one_and_two_tile_rows(gpu, oracle_mod, kind, rows):
    """One tile row: no row pass, the ranges are the column runs.  Two: a row pass over one bit,
    its list of several sort tiles (rows 5-7; test_tile_start_scenes.py).  The band scene leaves
    the top and bottom strips without an entry."""
    s, orc = _big(oracle_mod) if kind == "big" else _kind(oracle_mod, kind)
    _check_strip(gpu, s, orc, rows)


# context slots of this file's own (test_gpu_frame_graphs.py hands out 20 upwards, others use
# single slots up to 150)
_next_slot = [200]


def _slot(gpu, graphs, second_stream):
    """A context slot no forward has run on yet (no list capacity, no deferred-K frame)."""
    while True:
        slot = _next_slot[0]
        _next_slot[0] += 1
        st = _lib.frame_graph_stats(0, slot)
        if st["list_cap"] == 0 and st["graph_frames"] == 0:
            break
    set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, graphs, slot)
    set_option(gpu, _lib.GSR_OPT_SECOND_STREAM, second_stream, slot)
    return slot


@pytest.mark.parametrize("second_stream", [1, 0])
@pytest.mark.parametrize("graphs", [0, 1, 2])
def test_frame_graph_modes_and_streams(gpu, oracle_mod, graphs, second_stream):
    """Every scene, a one-row strip and the tight lists on a context of its own in each mode:
    the first frame sets the list capacity the direct way, the later ones run the deferred-K
    chains (modes 1 and 2), the empty frame's length reaching the row pass on the device."""
    slot = _slot(gpu, graphs, second_stream)
    st0 = _lib.frame_graph_stats(0, slot)
    for kind in ("left", "band", "none", "full", "left"):
        s, orc = _kind(oracle_mod, kind)
        _check_lists(run_hip(s, gpu, extras=LEAN, slot=slot), orc)
    s, orc = _kind(oracle_mod, "band")
    _check_tight(gpu, oracle_mod, s, orc, slot)
    for rows in ((5, 6), (5, 7)):
        _check_strip(gpu, s, orc, rows, slot)
    st = _lib.frame_graph_stats(0, slot)
    assert st["overflows"] == st0["overflows"]
    assert st["graph_frames"] - st0["graph_frames"] == (7 if graphs else 0), (st0, st)


@pytest.mark.parametrize("graphs,second_stream", [(2, 1), (2, 0), (1, 1)])
def test_capacity_overflow_is_rendered_again(gpu, oracle_mod, graphs, second_stream):
    """A short list sets the smallest capacity; a list beyond it overflows on its first frame
    (the tile-range blocks then see a count above the capacity), is rendered again the direct
    way and equals the oracle; the next frame runs deferred again."""
    slot = _slot(gpu, graphs, second_stream)
    st0 = _lib.frame_graph_stats(0, slot)
    assert st0["list_cap"] == 0, st0  # a context of this test's own
    s, orc = _kind(oracle_mod, "left")
    for _ in range(2):
        _check_lists(run_hip(s, gpu, extras=LEAN, slot=slot), orc)
    cap0 = _lib.frame_graph_stats(0, slot)["list_cap"]
    s, orc = _big(oracle_mod)
    assert orc["num_rendered"] > cap0 > 0
    for _ in range(2):
        _check_lists(run_hip(s, gpu, extras=LEAN, slot=slot), orc)
    st = _lib.frame_graph_stats(0, slot)
    assert st["overflows"] == 1 and st["list_cap"] > cap0 and st["graph_frames"] >= 3, st
