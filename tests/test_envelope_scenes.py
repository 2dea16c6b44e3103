"""CPU: the scenes of test_gpu_frame_envelope.py are what that test needs, by the oracle alone
(envelope_scenes.py): each case's binning form and pass count are the ones DESIGN.md section 4
lists, every tile row and tile column of every frame holds pairs, the lists span at least three
sort tiles of the row pass, the 2 x 256 frame's last sort tile is padded and holds entries of the
last tile row, the blend frames meet the float64 references' conditions on the scene, and the
2^24-Gaussian scene's lists are the index-mapped lists of its visible subset."""
import numpy as np
import pytest

import depth_scenes as ds
import envelope_scenes as es
import median_reference as mr
from gaussiansplattingviewer_amd.gaussian_data import GaussianData
from gpu_helpers import UNSTABLE_CAP, blend_reference, run_oracle

_bins = {}


def _bin(oracle_mod, name):
    if name not in _bins:
        _bins[name] = run_oracle(oracle_mod, es.get(name)["s"], stages="bin")
    return _bins[name]


def test_form_rule_at_its_edges():
    """expected_form is setup_frame's rule: each limit from both sides."""
    f = es.expected_form
    assert [f(16 * gx, 32, 3000) for gx in (255, 256, 257)] == [es.COL, es.COL, es.PAIR]
    assert [f(32, 16 * gy, 3000) for gy in (255, 256, 257)] == [es.COL, es.COL, es.PAIR]
    assert f(32, 4081, 3000) == es.COL and es.grid(32, 4081) == (2, 256)
    # the packed word: rows 129 .. 256 leave 24 id bits, 2 rows leave 31, one row all 32
    W, H = es.P_EDGE_FRAME
    assert es.grid(W, H) == (1, 129) and es.row_bits(W, H) == 8
    assert es.row_bits(16, 2048) == 7  # (128 rows: the limit would be 2^25)
    assert f(W, H, 1 << 24) == es.COL and f(W, H, (1 << 24) + 1) == es.PAIR
    assert es.tile_sort_passes(W, H) == (8, 1)  # the fused pass is the whole sort
    assert f(16, 32, 1 << 31) == es.COL and f(16, 32, (1 << 31) + 1) == es.PAIR
    assert f(16, 16, (1 << 32) - 1) == es.COL
    # tbits counts T - 1: 256 tiles are 8 bits and one pass, 257 are 9 and two
    assert es.tile_sort_passes(16, 16 * 256) == (8, 1)
    assert es.tile_sort_passes(16, 16 * 257) == (9, 2)
    assert es.tile_sort_passes(4096, 4096) == (16, 2) and es.tile_sort_passes(4112, 4096) == (17, 3)
    for W, H in es.TOO_LARGE:
        assert max(es.grid(W, H)) == 65536
    assert max(es.grid(16, 1048560)) == 65535


@pytest.mark.parametrize("name", sorted(es.CASES))
def test_case_has_the_listed_form_and_pass_count(name):
    c = es.CASES[name]
    assert es.expected_form(c["W"], c["H"], c["P"]) == c["form"]
    if c["form"] == es.COL:
        assert es.row_bits(c["W"], c["H"]) == c["what"]
    else:
        assert es.tile_sort_passes(c["W"], c["H"]) == c["what"]


def test_row_counts_reach_every_width_at_both_ends():
    """1 x r tiles: every row-pass width 1 .. 8 at its smallest and its largest r but 256
    (which the 2 x 256 frames hold), col_shift 31 .. 24."""
    seen = {}
    for r in es.ROW_COUNTS:
        seen.setdefault(es.row_bits(16, 16 * r), []).append(r)
    assert sorted(seen) == list(range(1, 9))
    for b, rs in seen.items():
        assert min(rs) == (1 << (b - 1)) + 1 and (b == 8 or max(rs) == 1 << b), (b, rs)


def test_strips_have_the_listed_forms():
    c = es.CASES[es.STRIP_FRAME]
    assert es.grid(c["W"], c["H"]) == (2, 300)
    for rows, (form, what) in es.STRIPS.items():
        assert es.expected_form(c["W"], c["H"], c["P"], rows) == form, rows
        if form == es.COL:
            assert es.row_bits(c["W"], c["H"], rows) == what, rows
        else:
            assert es.tile_sort_passes(c["W"], c["H"], rows) == what, rows
    assert {r[1] - r[0] for r in es.STRIPS} >= {256, 257, 1}
    assert any(r[0] > 255 for r in es.STRIPS) and any(r[0] <= 255 < r[1] - 1 for r in es.STRIPS)


@pytest.mark.parametrize("name", sorted(es.CASES))
def test_scene_fills_its_frame(oracle_mod, name):
    """Every tile row and every tile column holds pairs, the first and the last included (all
    65,535 of the longest frames too); at least three sort tiles, the last partly filled."""
    c = es.CASES[name]
    orc = _bin(oracle_mod, name)
    rows, cols = es.per_row_and_column(orc, c["W"], c["H"])
    gx, gy = es.grid(c["W"], c["H"])
    assert len(rows) == gy and len(cols) == gx
    assert (rows > 0).all() and (cols > 0).all()
    K = orc["num_rendered"]
    assert K >= 3 * es.SORT_TILE and K % es.SORT_TILE != 0
    if name not in es.LONG:  # small Gaussians: many of them, and none reaches far
        assert (orc["radii"] > 0).mean() > 0.95 and orc["radii"].max() <= 32
    if c["form"] == es.COL and gx > 1:  # column boundaries inside sort tiles
        starts = np.cumsum(cols)[:-1]
        assert np.all(starts % es.SORT_TILE != 0)
        assert len(np.unique(starts // es.SORT_TILE)) >= min(3, gx - 1)


def test_last_sort_tile_of_2x256_is_padded_and_holds_the_last_row(oracle_mod):
    """The row pass of 256 rows uses digit 255 for the last tile row and for the padded keys of
    the last sort tile: that tile is partly filled and holds entries of row 255."""
    for name in ("32x4096", "32x4081"):
        orc = _bin(oracle_mod, name)
        c = es.CASES[name]
        rows = es.row_pass_input_rows(orc, c["W"], c["H"])
        K = len(rows)
        tail = rows[K - K % es.SORT_TILE:]
        assert 0 < len(tail) < es.SORT_TILE
        assert (tail == 255).sum() > 0 and (rows[:K - len(tail)] == 255).sum() > 0, name


def test_column_boundaries_in_the_padded_sort_tile_of_256x256(oracle_mod):
    """256 x 256 tiles: column boundaries fall inside the partly filled last sort tile, whose
    padded keys share digit 255 with the last tile row -- the boundary count (radix_sort.hip
    rows_before) must stop at the boundary -- and that tile holds entries of row 255."""
    name = "4096x4096"
    c = es.CASES[name]
    orc = _bin(oracle_mod, name)
    rows = es.row_pass_input_rows(orc, c["W"], c["H"])
    K = len(rows)
    last = K - K % es.SORT_TILE
    starts = np.cumsum(es.per_row_and_column(orc, c["W"], c["H"])[1])[:-1]
    assert ((starts > last) & (starts < K)).sum() >= 8
    assert (rows[last:] == 255).sum() > 0


@pytest.mark.parametrize("name", es.BLEND_FRAMES)
def test_blend_frames_meet_the_references_conditions(oracle_mod, name):
    """UNSTABLE_CAP is a condition on the scene: the oracle's own float64 blend, the depth
    planes' and the median's meet it on these seeds."""
    sc = es.get(name)
    orc = run_oracle(oracle_mod, sc["s"])
    sc["orc"] = orc
    ref = blend_reference(oracle_mod, orc, sc["s"]["bg"])
    share = 1.0 - float(ref["stable"].mean())
    print(f"{name}: unstable {share:.5f}")
    assert share <= UNSTABLE_CAP
    for k, r in ds.reference(oracle_mod, sc, orc).items():
        assert 1.0 - float(r["stable"].mean()) <= UNSTABLE_CAP, k
    mr.assert_scene_decides(mr.reference(oracle_mod, sc, orc), name)


def test_strip_frame_rows(oracle_mod):
    """Every one of the 300 tile rows of the strip frame holds pairs, so every strip of
    es.STRIPS has a list, the one-row strip at row 299 included."""
    c = es.CASES[es.STRIP_FRAME]
    rows, _ = es.per_row_and_column(_bin(oracle_mod, es.STRIP_FRAME), c["W"], c["H"])
    assert len(rows) == 300 and (rows > 0).all()


def test_p_edge_scene(oracle_mod):
    """P = 2^24 and 2^24 + 1: the lists of the full scene are the lists of its visible subset
    with the ids mapped, ids 2^24 - 2, 2^24 - 1 (and 2^24) among them."""
    g, ids = es.p_edge_arrays()
    assert len(g.xyz) == es.P_EDGE + 1 and sum(a.nbytes for a in es.fields(g)) < 1 << 30
    assert list(ids[-3:]) == [es.P_EDGE - 2, es.P_EDGE - 1, es.P_EDGE]
    W, H = es.P_EDGE_FRAME
    for P in (es.P_EDGE, es.P_EDGE + 1):
        sc = es.p_edge_scene(g, P)
        assert len(sc["s"]["g"].xyz) == P and sc["s"]["g"].xyz.base is not None  # a view
        orc = run_oracle(oracle_mod, sc["s"], stages="bin")
        vis = ids[ids < P]
        seen = np.flatnonzero(orc["radii"] > 0)
        assert set(seen) <= set(vis) and len(seen) > 0.95 * len(vis)
        for i in vis[-2:]:
            assert orc["radii"][i] > 0 and (orc["point_list"] == i).any(), i
        sub = GaussianData(*(a[vis] for a in es.fields(g)))
        small = run_oracle(oracle_mod, dict(sc["s"], g=sub), stages="bin")
        assert small["num_rendered"] == orc["num_rendered"] >= 3 * es.SORT_TILE
        np.testing.assert_array_equal(vis[small["point_list"]], orc["point_list"])
        np.testing.assert_array_equal(small["point_keys"], orc["point_keys"])
        np.testing.assert_array_equal(small["ranges"], orc["ranges"])
        rows, _ = es.per_row_and_column(orc, W, H)
        assert (rows > 0).all()
