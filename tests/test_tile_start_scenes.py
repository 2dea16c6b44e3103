"""CPU: the scenes of test_gpu_tile_starts.py really are what that test needs, by the oracle
alone: lists of several 4096-entry sort tiles whose tile-column boundaries fall inside sort
tiles, the empty tile columns each scene is built for, a partly filled last sort tile, and one
scene with a column boundary exactly on a sort-tile boundary."""
import numpy as np
import pytest

import tile_start_scenes as ts
from gpu_helpers import run_oracle


def _starts(oracle_mod, s, gx=ts.GX):
    orc = run_oracle(oracle_mod, s, stages="bin")
    return orc, ts.column_starts(orc, gx)


@pytest.mark.parametrize("kind", ["full", "left", "band"])
def test_lists_span_sort_tiles_with_inner_boundaries(oracle_mod, kind):
    orc, cs = _starts(oracle_mod, ts.scene(kind))
    n = int(cs[-1])
    assert n == orc["num_rendered"] and n >= 4 * ts.SORT_TILE
    assert n % ts.SORT_TILE != 0  # the last sort tile is partly filled
    inner = cs[(cs > 0) & (cs < n)]
    assert len(inner) >= 4 and np.all(inner % ts.SORT_TILE != 0)
    assert len(np.unique(inner // ts.SORT_TILE)) >= 3  # boundaries in several sort tiles


def test_empty_columns(oracle_mod):
    per_col = {k: np.diff(_starts(oracle_mod, ts.scene(k))[1]) for k in ts.KINDS}
    assert np.all(per_col["full"] > 0)
    left = per_col["left"]
    assert left[0] > 0 and np.all(left[ts.GX // 2:] == 0)  # trailing empty columns
    band = per_col["band"]
    assert np.all(band[:2] == 0) and np.all(band[-3:] == 0) and band[ts.GX // 2] > 0
    assert per_col["none"].sum() == 0  # no visible Gaussian
    # tile rows that are empty inside non-empty columns too: (0, 0) ranges between full ones
    orc = run_oracle(oracle_mod, ts.scene("band"), stages="bin")
    rg = orc["ranges"].reshape(ts.GY, ts.GX, 2)
    empty = rg[..., 1] == rg[..., 0]
    assert empty[:, band > 0].any() and not empty[:, band > 0].all()


def test_odd_image_size_keeps_the_grid(oracle_mod):
    orc, cs = _starts(oracle_mod, ts.scene("full", w=250, h=187))
    assert (250 + 15) // 16 == ts.GX and (187 + 15) // 16 == ts.GY
    assert cs[-1] >= 4 * ts.SORT_TILE and np.all(np.diff(cs) > 0)


def test_overflow_scene_outgrows_the_smallest_capacity(oracle_mod):
    small = run_oracle(oracle_mod, ts.scene("left"), stages="bin")["num_rendered"]
    big = run_oracle(oracle_mod, ts.scene("full", P=12000, seed=3), stages="bin")["num_rendered"]
    assert small + small // 4 < 1 << 16 < big  # (api.hip kMinListCap = 65536 entries)


@pytest.mark.parametrize("kind", ["big", "band"])
def test_strip_lists(oracle_mod, kind):
    """The two-row strip (tile rows 5-7) has a list of several sort tiles; the band scene has no
    entry in the top and bottom strips."""
    s = ts.scene("full", P=12000, seed=3) if kind == "big" else ts.scene("band")
    orc = run_oracle(oracle_mod, s, stages="bin")
    rows = (orc["point_keys"] >> np.uint64(32)).astype(np.int64) // ts.GX
    assert ((rows >= 5) & (rows < 7)).sum() >= 2 * ts.SORT_TILE
    assert ((rows == 5).sum() > 0)
    if kind == "band":
        assert (rows == 0).sum() == 0 and (rows == 11).sum() == 0


def test_aligned_boundary_scene(oracle_mod):
    s, c = ts.aligned_boundary_scene(oracle_mod)
    _, cs = _starts(oracle_mod, s)
    assert 0 < cs[c] < cs[-1] and cs[c] % ts.SORT_TILE == 0 and cs[c + 1] > cs[c]


def test_seed_sweep_boundaries(oracle_mod):
    """How many of the GPU sweep's seeds put a column boundary on a sort-tile boundary by
    chance: none of the 20 (each boundary has a 1 in 4096 chance), which is why
    aligned_boundary_scene constructs one."""
    hits = 0
    for seed in range(20):
        _, cs = _starts(oracle_mod, ts.scene("full", seed=seed))
        inner = cs[(cs > 0) & (cs < cs[-1])]
        hits += int((inner % ts.SORT_TILE == 0).sum())
    assert hits == 0
