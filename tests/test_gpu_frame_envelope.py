"""GPU: the binning and the blend at the edges of the frame-shape envelope (api.hip setup_frame),
against the C oracle's literal 64-bit sort, on the scenes of envelope_scenes.py
(test_envelope_scenes.py checks the scenes with the oracle alone; DESIGN.md section 4, "The
frame-shape envelope", lists what each frame reaches).

Every case asserts which binning form ran: a context under GSR_OPT_FRAME_GRAPHS 1 that has a list
capacity takes a frame through the recorded chains if and only if the frame is column-first
(api.hip graph_eligible), and counts it in gsr_frame_graph_stats' graph_frames.

  1 every frame of envelope_scenes.CASES: the form, the lists through the lean forward, then one
    forward with all extras held to assert_parity; the boundary frames again with tight lists and
    with tight binning off
  2 frames of 65,536 tiles a side are refused and leave the context usable
  3 P = 2^24 (column-first, id 2^24 - 1 under the 24-bit id mask) and 2^24 + 1 (per pair, the
    fused pass the entire sort)
  4 the 256 x 2 and 2 x 256 frames through the deferred-K chains, recorded and direct, with and
    without the second stream
  5 strips of a 2 x 300 frame: 256 and 257 rows, strips that start past, straddle and end at
    tile row 255 and beyond, and the full frame's pairs per tile row
  6 the other blend kernels at pixel y up to 4,111: the per-pixel float64 bound, the depth planes,
    the median planes, one GL shading
"""
import time

import numpy as np
import pytest

from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import tile_row_pairs

import depth_scenes as ds
import envelope_scenes as es
import median_reference as mr
import shading_reference as sr
import tile_start_scenes as ts
from gpu_helpers import (ALL_EXTRAS, assert_blend_exact, assert_image_close, assert_parity,
                         run_hip, run_oracle, set_option, tight_binning)
from test_gpu_shading import _check_against_reference
from test_gpu_shading import _render as _render_shaded
from test_gpu_tile_starts import LEAN, _check_lists, _check_tight

pytestmark = pytest.mark.gpu

# context slots of this file's own (the other files hand out 20, 200, 300 and 400 upwards)
_next_slot = [600]
_orc = {}
PLANES = ds.PLANES
SURF = ("median_depth", "median_id")


def _oracle(oracle_mod, name):
    """The oracle's forward of a named scene, once; kept in the scene as blend_scenes.run does."""
    sc = es.get(name)
    if "orc" not in sc:
        sc["orc"] = run_oracle(oracle_mod, sc["s"])
    return sc, sc["orc"]


def _slot(gpu, graphs=1, second_stream=1):
    """A context slot no forward has run on yet, under the given options."""
    while True:
        slot = _next_slot[0]
        _next_slot[0] += 1
        st = _lib.frame_graph_stats(0, slot)
        if st["list_cap"] == 0 and st["graph_frames"] == 0:
            break
    set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, graphs, slot)
    set_option(gpu, _lib.GSR_OPT_SECOND_STREAM, second_stream, slot)
    return slot


def _form_slot(gpu, oracle_mod):
    """A fresh slot under GSR_OPT_FRAME_GRAPHS 1 whose list capacity a small column-first frame
    has set (the direct way: graph_frames stays 0)."""
    slot = _slot(gpu)
    if "small" not in _orc:
        s = ts.scene("left")
        _orc["small"] = (s, run_oracle(oracle_mod, s))
    s, orc = _orc["small"]
    _check_lists(run_hip(s, gpu, extras=LEAN, slot=slot), orc)
    st = _lib.frame_graph_stats(0, slot)
    assert st["list_cap"] > 0 and st["graph_frames"] == 0, st
    return slot


def _lean(gpu, s, slot, tile_rows=None):
    """(the form that ran, the result) of a forward with the LEAN extras on a _form_slot."""
    before = _lib.frame_graph_stats(0, slot)["graph_frames"]
    hip = run_hip(s, gpu, tile_rows=tile_rows, extras=LEAN, slot=slot)
    taken = _lib.frame_graph_stats(0, slot)["graph_frames"] - before
    assert taken in (0, 1), taken
    return (es.COL if taken else es.PAIR), hip


def _same_lists(hip, orc):
    assert hip["num_rendered"] == orc["num_rendered"]
    np.testing.assert_array_equal(hip["point_list"], orc["point_list"])
    np.testing.assert_array_equal(hip["point_tiles"], es.tiles_of(orc).astype(np.uint32))
    np.testing.assert_array_equal(hip["ranges"], orc["ranges"])
    np.testing.assert_array_equal(hip["radii"], orc["radii"])


# ---- 1 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(es.CASES))
def test_frame(gpu, oracle_mod, name):
    sc, orc = _oracle(oracle_mod, name)
    s = sc["s"]
    slot = _form_slot(gpu, oracle_mod)
    form, lean = _lean(gpu, s, slot)
    assert form == es.CASES[name]["form"], f"{name} was binned {form}"
    _same_lists(lean, orc)
    assert_parity(run_hip(s, gpu, slot=slot), orc)  # n_contrib requested: upstream's full lists
    if name in es.BOUNDARY:
        tight = _check_tight(gpu, oracle_mod, s, orc, slot)
        with tight_binning(gpu, 0, slot):  # the full lists through the forward without n_contrib
            off = run_hip(s, gpu, extras=(), slot=slot)
        _same_lists(off, orc)
        assert_image_close(off["color"], orc["color"])
        if es.CASES[name]["form"] == es.COL:  # (tight binning is the column-first form's)
            assert len(tight["point_list"]) < len(off["point_list"])
    if sc["W"] * sc["H"] > 1 << 22:  # (the largest images are not kept for the session)
        del sc["orc"]


# ---- 2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", es.TOO_LARGE)
def test_65536_tiles_a_side_are_refused(gpu, oracle_mod, W, H):
    """GSR_E_INVALID, and the next ordinary frame on the same context equals the oracle."""
    slot = _slot(gpu, graphs=0)
    sc = es.scene_of(W, H, 64)
    with pytest.raises(RuntimeError, match="larger than 65535 tiles"):
        run_hip(sc["s"], gpu, extras=LEAN, slot=slot)
    s = ts.scene("full")
    assert_parity(run_hip(s, gpu, slot=slot), run_oracle(oracle_mod, s))


# ---- 3 --------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def p_edge():
    return es.p_edge_arrays()


@pytest.mark.parametrize("P,form", [(es.P_EDGE, es.COL), (es.P_EDGE + 1, es.PAIR)])
def test_p_edge(gpu, oracle_mod, p_edge, P, form):
    """P = 2^col_shift and one more on the 1 x 129 frame (col_shift 24): column-first with ids
    2^24 - 2 and 2^24 - 1 under the 24-bit id mask, then per pair with tbits = 8, the fused
    pass being the entire sort.  The reference is the oracle on the full scene."""
    g, ids = p_edge
    sc = es.p_edge_scene(g, P)
    s = sc["s"]
    t0 = time.perf_counter()
    orc = run_oracle(oracle_mod, s)
    t1 = time.perf_counter()
    for i in ids[ids < P][-2:]:
        assert (orc["point_list"] == i).any()
    slot = _form_slot(gpu, oracle_mod)
    ran, lean = _lean(gpu, s, slot)
    assert ran == form == es.expected_form(sc["W"], sc["H"], P)
    _same_lists(lean, orc)
    assert_parity(run_hip(s, gpu, slot=slot), orc)
    print(f"P = {P}: oracle {t1 - t0:.1f} s, two GPU forwards with their uploads and checks "
          f"{time.perf_counter() - t1:.1f} s")


# ---- 4 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second_stream", [1, 0])
@pytest.mark.parametrize("graphs", [1, 2])
def test_deferred_k_on_256_columns_and_256_rows(gpu, oracle_mod, graphs, second_stream):
    """The 256 x 2 and 2 x 256 frames through the deferred-K chains on a context of their own:
    the first frame sets the list capacity the direct way, the others are binned into the
    capacity with the list length read on the device, the padded tail of the row pass's last
    sort tile now a whole capacity long."""
    slot = _slot(gpu, graphs, second_stream)
    st0 = _lib.frame_graph_stats(0, slot)
    for name in ("4096x32", "32x4096", "4096x32", "32x4096"):
        sc, orc = _oracle(oracle_mod, name)
        _check_lists(run_hip(sc["s"], gpu, extras=LEAN, slot=slot), orc)
    for name in ("4096x32", "32x4096"):
        sc, orc = _oracle(oracle_mod, name)
        _check_tight(gpu, oracle_mod, sc["s"], orc, slot)
    st = _lib.frame_graph_stats(0, slot)
    assert st["overflows"] == st0["overflows"]
    assert st["graph_frames"] - st0["graph_frames"] == 5, (st0, st)


# ---- 5 --------------------------------------------------------------------------------------------
def _check_strip(gpu, s, orc, rows, gx, slot):
    """A strip's ranges, lists, tile ids and image rows against the full-frame oracle result
    (test_gpu_tile_starts._check_strip for a grid of gx columns); returns the form that ran."""
    form, part = _lean(gpu, s, slot, tile_rows=rows)
    tiles = es.tiles_of(orc)
    t0, t1 = rows[0] * gx, rows[1] * gx
    before = int((tiles < t0).sum())
    want = orc["ranges"].reshape(-1, 2).astype(np.int64).copy()
    nonempty = want[:, 1] > want[:, 0]
    want[nonempty] -= before
    want[:t0] = 0
    want[t1:] = 0
    np.testing.assert_array_equal(part["ranges"].reshape(-1, 2), want)
    sel = (tiles >= t0) & (tiles < t1)
    assert sel.sum() > 0
    np.testing.assert_array_equal(part["point_list"], orc["point_list"][sel])
    np.testing.assert_array_equal(part["point_tiles"], tiles[sel].astype(np.uint32))
    _check_lists(part, orc, rows)
    return form


@pytest.mark.parametrize("rows", sorted(es.STRIPS))
def test_strip_of_a_tall_frame(gpu, oracle_mod, rows):
    sc, orc = _oracle(oracle_mod, es.STRIP_FRAME)
    slot = _form_slot(gpu, oracle_mod)
    form = _check_strip(gpu, sc["s"], orc, rows, es.grid(sc["W"], sc["H"])[0], slot)
    assert form == es.STRIPS[rows][0], f"strip {rows} was binned {form}"


def test_tile_row_pairs_of_300_rows(gpu, oracle_mod):
    """gsr_tile_row_pairs of the full 2 x 300 frame (per pair) and of its 256-row strip
    (column-first) against the oracle's sums per tile row."""
    sc, orc = _oracle(oracle_mod, es.STRIP_FRAME)
    want, _ = es.per_row_and_column(orc, sc["W"], sc["H"])
    slot = _slot(gpu, graphs=0)
    run_hip(sc["s"], gpu, extras=LEAN, slot=slot, binning=False)
    got = tile_row_pairs(300, gpu.index or 0, slot).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, want)
    run_hip(sc["s"], gpu, extras=LEAN, slot=slot, binning=False, tile_rows=(44, 300))
    got = tile_row_pairs(256, gpu.index or 0, slot).cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(got, want[44:])


# ---- 6 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", es.BLEND_FRAMES)
def test_blend_exact_at_large_y(gpu, oracle_mod, name):
    sc, orc = _oracle(oracle_mod, name)
    try:
        for fast in (1, 0):
            set_option(gpu, _lib.GSR_OPT_BLEND_FAST, fast)
            assert_blend_exact(oracle_mod, run_hip(sc["s"], gpu), orc, sc["s"]["bg"],
                               what=f"{name} {'fast' if fast else 'exact'}")
    finally:
        set_option(gpu, _lib.GSR_OPT_BLEND_FAST, 1)


@pytest.mark.parametrize("name", es.BLEND_FRAMES)
def test_depth_planes_at_large_y(gpu, oracle_mod, name):
    """The planes bit for bit channels 0 and 1 of a forward with (z, 1 / z, 0) as the colour,
    and within the float64 bound."""
    sc, orc = _oracle(oracle_mod, name)
    ref = ds.reference(oracle_mod, sc, orc)
    hip = run_hip(sc["s"], gpu, extras=ALL_EXTRAS + PLANES)
    assert_parity(hip, orc, image=False)
    z, iz = ds.features(hip["depths"], hip["radii"])
    twin = run_hip(ds.zero_bg(sc), gpu, binning=False,
                   colors_precomp=np.stack([z, iz, np.zeros_like(z)], axis=1))
    for c, k in enumerate(PLANES):
        np.testing.assert_array_equal(hip[k].view(np.uint32), twin["color"][c].view(np.uint32),
                                      err_msg=f"{name}: {k} is not its twin channel")
        ds.assert_plane_exact(hip[k], hip["n_contrib"], ref[k], f"{name} {k}")
    for k in ("final_T", "n_contrib"):
        np.testing.assert_array_equal(twin[k].view(np.uint32), hip[k].view(np.uint32), err_msg=k)


@pytest.mark.parametrize("name", es.BLEND_FRAMES)
def test_median_planes_at_large_y(gpu, oracle_mod, name):
    sc, orc = _oracle(oracle_mod, name)
    ref = mr.reference(oracle_mod, sc, orc)
    mr.assert_scene_decides(ref, name)
    hip = run_hip(sc["s"], gpu, extras=ALL_EXTRAS + PLANES + SURF)
    assert_parity(hip, orc, image=False)
    mr.assert_median_accepted(ref, sc, hip["median_id"], hip["median_depth"], hip["depths"], name)
    few = run_hip(sc["s"], gpu, extras=SURF, binning=False)  # no n_contrib: tight lists
    mr.assert_median_accepted(ref, sc, few["median_id"], few["median_depth"], hip["depths"],
                              name + " (planes only)")
    assert (hip["median_id"][-16:] >= 0).any() and (hip["median_id"][:16] >= 0).any()


@pytest.mark.parametrize("name", es.BLEND_FRAMES)
def test_gauss_ball_shading_at_large_y(gpu, oracle_mod, name):
    sc, orc = _oracle(oracle_mod, name)
    ref = sr.reference(sc, orc, sr.GAUSS_BALL)
    hip = _render_shaded(sc, gpu, sr.GAUSS_BALL, binning=True)
    np.testing.assert_array_equal(hip["point_list"], orc["point_list"])
    np.testing.assert_array_equal(hip["ranges"], orc["ranges"])
    _check_against_reference(hip, sc, orc, ref, sr.GAUSS_BALL, f"{name} shading {sr.GAUSS_BALL}")
