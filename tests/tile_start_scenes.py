"""Small scenes for the tile-range tests (test_gpu_tile_starts.py, test_tile_start_scenes.py):
a few thousand Gaussians, large enough on a 256 x 192 image (16 x 12 tiles) that the pair list
spans several 4096-entry sort tiles, so the tile columns' boundaries in the column-sorted list
fall inside sort tiles; confined in x so that whole tile columns stay empty."""
from __future__ import annotations

import numpy as np

from gaussiansplattingviewer_amd.camera import static_camera
from gaussiansplattingviewer_amd.gaussian_data import activate

from gpu_helpers import scene_inputs

W, H = 256, 192
GX, GY = W // 16, H // 16
SORT_TILE = 4096  # entries per tile of the row pass (radix_sort.hip)

# kind: world x, y and z ranges of the centres (the camera at (0, 0, 4) sees about x in
# [-2.2, 2.2] at z = 0; image x grows with world x; positive z is toward the camera)
KINDS = {
    "full": ((-2.0, 2.0), (-1.6, 1.6), (-2.0, 2.0)),
    # the left third: trailing empty columns
    "left": ((-2.0, -0.9), (-1.6, 1.6), (-1.0, 1.0)),
    # a middle band, short of the top and bottom: leading and trailing empty columns, and empty
    # tiles above and below the full ones of a column
    "band": ((-0.45, 0.45), (-0.4, 0.4), (-1.0, 1.0)),
    "none": ((-2.0, 2.0), (-1.6, 1.6), (6.0, 9.0)),  # every Gaussian behind the camera
}


def gaussians(kind, P=3000, seed=0):
    (x0, x1), (y0, y1), (z0, z1) = KINDS[kind]
    rng = np.random.default_rng(1000 + seed)
    xyz = np.stack([rng.uniform(x0, x1, P), rng.uniform(y0, y1, P), rng.uniform(z0, z1, P)], 1)
    log_scale = rng.uniform(-3.2, -2.2, (P, 3))
    quat = rng.standard_normal((P, 4))
    opacity = rng.normal(0.0, 1.5, (P, 1))
    f_dc = rng.normal(0.0, 0.6, (P, 3))
    f_rest = rng.normal(0.0, 0.05, (P, 45))
    return activate(xyz, quat, log_scale, opacity, f_dc, f_rest)


def scene(kind, P=3000, seed=0, w=W, h=H):
    return scene_inputs(gaussians(kind, P, seed), static_camera(w, h), 3)


def column_starts(orc, gx):
    """Start of every tile column's run in the column-sorted list (gx + 1 values, the last the
    list length), from an oracle result's tile keys."""
    tiles = (orc["point_keys"] >> np.uint64(32)).astype(np.int64)
    per_col = np.bincount(tiles % gx, minlength=gx)
    return np.concatenate([[0], np.cumsum(per_col)])


def _subset(weights, target):
    """Indices of a subset of the positive integer weights that sums to target, or None."""
    reach = [1]
    for w in weights:
        reach.append(reach[-1] | (reach[-1] << int(w)))
    if not (reach[-1] >> target) & 1:
        return None
    out = []
    for i in range(len(weights) - 1, -1, -1):
        if not (reach[i] >> target) & 1:
            out.append(i)
            target -= int(weights[i])
    return out if target == 0 else None


def aligned_boundary_scene(oracle, seed=0):
    """The "full" scene with a few Gaussians removed so that one tile column's run starts exactly
    on a sort-tile boundary inside the list (with upstream's full lists): Gaussians whose tiles
    all lie left of column c are dropped until the pairs left of c are a multiple of SORT_TILE.
    Returns (scene, c).  Every other Gaussian keeps its pairs: the preprocess is per Gaussian."""
    from gpu_helpers import run_oracle
    g = gaussians("full", 3000, seed)
    orc = run_oracle(oracle, scene("full", seed=seed), stages="bin")
    tiles = (orc["point_keys"] >> np.uint64(32)).astype(np.int64)
    ids = orc["point_list"].astype(np.int64)
    P = len(g.xyz)
    max_col = np.full(P, -1)
    np.maximum.at(max_col, ids, tiles % GX)
    touched = np.bincount(ids, minlength=P)
    starts = column_starts(orc, GX)
    for c in range(GX - 1, 0, -1):
        excess = int(starts[c] % SORT_TILE)
        if starts[c] < SORT_TILE or excess == 0:
            continue
        cand = np.flatnonzero((max_col >= 0) & (max_col < c))
        pick = _subset(touched[cand], excess)
        if pick is None:
            continue
        keep = np.ones(P, bool)
        keep[cand[pick]] = False
        from gaussiansplattingviewer_amd.gaussian_data import GaussianData
        g2 = GaussianData(g.xyz[keep], g.rot[keep], g.scale[keep], g.opacity[keep], g.sh[keep])
        return scene_inputs(g2, static_camera(W, H), 3), c
    raise AssertionError("no column could be aligned")
