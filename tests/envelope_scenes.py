"""Scenes at the edges of the frame-shape envelope of the binning (api.hip setup_frame), for
test_envelope_scenes.py (CPU, the oracle alone) and test_gpu_frame_envelope.py.

setup_frame bins a frame column-first when its tile grid has at most 256 columns and its strip at
most 256 rows and the packed word (strip row << col_shift | id) holds every id, and per (Gaussian,
tile) pair otherwise; expected_form restates that rule and tile_sort_passes the per-pair form's
pass count.  CASES lists one frame on every side of every limit.

A scene is a few thousand small Gaussians placed in pixel space: static_camera keeps the vertical
field of view whatever the aspect ratio, so at 32 x 4096 px the visible world is 2.4 units high and
0.019 wide, and a Gaussian of a fixed world size covers either nothing or the whole width.  The
centres are therefore chosen as pixel positions and view depths and mapped back to the world, the
sizes likewise as a standard deviation in pixels; along the frame's long axis they are stratified
(one per equal slice, jittered), so that every tile row and column holds pairs with few Gaussians.
"""
from __future__ import annotations

import numpy as np

from gaussiansplattingviewer_amd.camera import cuda_camera_inputs, static_camera
from gaussiansplattingviewer_amd.gaussian_data import GaussianData

from gpu_helpers import scene_inputs

F32 = np.float32
SORT_TILE = 4096   # entries per tile of the row pass (radix_sort.hip)
EYE_DEPTH = 4.0    # static_camera looks at the origin from (0, 0, 4)
COL, PAIR = "col", "pair"


def bits_for(v):
    """api.hip bits_for: bits needed to represent every value <= v (32 at the most)."""
    return min(int(v).bit_length(), 32)


def grid(W, H):
    return (W + 15) // 16, (H + 15) // 16


def expected_form(W, H, P, tile_rows=None):
    """The binning form setup_frame chooses: COL (column-first) or PAIR (per pair)."""
    gx, gy = grid(W, H)
    rows = gy if tile_rows is None else tile_rows[1] - tile_rows[0]
    ybits = bits_for(rows - 1) if rows > 1 else 0
    col_shift = 32 - ybits
    ok = gx <= 256 and rows <= 256 and (col_shift == 32 or P <= 1 << col_shift)
    return COL if ok else PAIR


def row_bits(W, H, tile_rows=None):
    """The row pass's digit width (column-first frames): 0 means no row pass."""
    rows = grid(W, H)[1] if tile_rows is None else tile_rows[1] - tile_rows[0]
    return bits_for(rows - 1) if rows > 1 else 0


def tile_sort_passes(W, H, tile_rows=None):
    """(tbits, passes) of a per-pair frame: the tile-id bits and the 8-bit passes that sort them,
    the first fused with the duplication (radix_sort.hip gsr_radix_plan)."""
    gx, gy = grid(W, H)
    rows = gy if tile_rows is None else tile_rows[1] - tile_rows[0]
    T = gx * rows
    tbits = bits_for(T - 1) if T > 1 else 0
    return tbits, (tbits + 7) // 8


# name: (W, H, P, sigma range in px, form, row bits (col) or (tbits, passes) (pair))
def _case(W, H, P, sigma, form, what):
    return dict(W=W, H=H, P=P, sigma=sigma, form=form, what=what)


MID = (3.0, 8.0)
CASES = {
    # 255, 256, 257 tile columns: all 256 column digits, the gx edge from both sides
    "4080x32": _case(4080, 32, 3000, MID, COL, 1),
    "4096x32": _case(4096, 32, 3000, MID, COL, 1),
    "4112x32": _case(4112, 32, 3000, MID, PAIR, (10, 2)),
    # 255, 256, 256 (the last 1 px high), 257 tile rows
    "32x4080": _case(32, 4080, 3000, MID, COL, 8),
    "32x4096": _case(32, 4096, 3000, MID, COL, 8),
    "32x4081": _case(32, 4081, 3000, MID, COL, 8),
    "32x4112": _case(32, 4112, 3000, MID, PAIR, (10, 2)),
    # the column-first form at its largest, and one column more: three tile-sort passes
    "4096x4096": _case(4096, 4096, 3000, MID, COL, 8),
    "4112x4096": _case(4112, 4096, 3000, MID, PAIR, (17, 3)),
    # 65,535 tiles a side: 16-bit rects at 0xFFFF
    "16x1048560": _case(16, 1048560, 3000, MID, PAIR, (16, 2)),
    "1048560x16": _case(1048560, 16, 3000, MID, PAIR, (16, 2)),
    # strips of a tall frame (2 x 300 tiles)
    "32x4800": _case(32, 4800, 3000, MID, PAIR, (10, 2)),
}
# 1 x r tiles: every row-pass width 1 .. 8 at both ends, col_shift 31 .. 24
ROW_COUNTS = (2, 3, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129)
for _r in ROW_COUNTS:
    # K >= 3 sort tiles needs more Gaussians the fewer tiles each can reach
    CASES[f"16x{16 * _r}"] = _case(16, 16 * _r, 7000 if _r < 8 else 5000, MID, COL,
                                    bits_for(_r - 1))
BOUNDARY = ("4080x32", "4096x32", "4112x32", "32x4080", "32x4096", "32x4081", "32x4112")
LONG = ("16x1048560", "1048560x16")       # filled by stretched Gaussians (get)
TOO_LARGE = ((16, 1048576), (1048576, 16))  # 65,536 tiles a side: refused
BLEND_FRAMES = ("32x4112", "32x4096")     # the other blend kernels at large y
STRIP_FRAME = "32x4800"
# (tile_row_begin, tile_row_end): form, row bits or (tbits, passes)
STRIPS = {(0, 256): (COL, 8), (44, 300): (COL, 8), (43, 300): (PAIR, (10, 2)),
          (256, 300): (COL, 6), (255, 257): (COL, 1), (299, 300): (COL, 0)}

# seeds other than 0: the 256 x 256 frame's puts entries of tile row 255 into the padded last
# sort tile (seed 0 has none there); the blend frames' seed 0 meets UNSTABLE_CAP
# (test_envelope_scenes.py asserts both)
SEEDS = {"4096x4096": 1}


def pixel_gaussians(W, H, P, seed=0, sigma=MID, depth=(3.4, 4.6), stretch=None, M=16):
    """P Gaussians whose centres project to pixel positions spread over the W x H frame:
    stratified along the long axis, uniform along the short one, from 4 px outside the frame
    on either side; view depth uniform in `depth`; a random rotation about the view axis and
    per-axis standard deviations that appear as `sigma` px (log-uniform).  stretch: the
    standard deviation in px along the frame's long axis instead (no rotation), for frames too
    long to fill otherwise."""
    rng = np.random.default_rng(7000 + seed)
    ty = float(cuda_camera_inputs(static_camera(W, H))[4])
    u = 2.0 * ty / H  # world units per pixel at view depth 1
    t = rng.permutation((np.arange(P) + rng.uniform(0.0, 1.0, P)) / P)
    s = rng.uniform(0.0, 1.0, P)
    px, py = (t, s) if W >= H else (s, t)
    px = px * (W + 8.0) - 4.0
    py = py * (H + 8.0) - 4.0
    z = rng.uniform(depth[0], depth[1], P)
    xyz = np.stack([(px - 0.5 * W) * u * z, (py - 0.5 * H) * u * z, EYE_DEPTH - z], 1)
    sig = np.exp(rng.uniform(np.log(sigma[0]), np.log(sigma[1]), (P, 3)))
    # rotated about the view axis only, and thin along it where the frame is wider than high:
    # at tan(half fov x) = 38 (4080 x 32) a Gaussian's extent in depth projects onto x 50-fold
    half = 0.5 * rng.uniform(0.0, 2.0 * np.pi, P)
    rot = np.stack([np.cos(half), np.zeros(P), np.zeros(P), np.sin(half)], 1)
    sig[:, 2] *= min(1.0, H / W)
    if stretch is not None:
        rot = np.tile([1.0, 0.0, 0.0, 0.0], (P, 1))
        sig[:, 0 if W >= H else 1] = stretch
    scale = sig * (u * z)[:, None]
    opacity = rng.uniform(0.1, 0.9, (P, 1))
    sh = np.concatenate([rng.normal(0.0, 0.6, (P, 3)), rng.normal(0.0, 0.1, (P, 3 * (M - 1)))], 1)
    a = lambda v: np.ascontiguousarray(v, F32)  # noqa: E731
    return GaussianData(a(xyz), a(rot), a(scale), a(opacity), a(sh))


def scene_of(W, H, P, seed=0, sigma=MID, stretch=None, bg=(0.1, 0.2, 0.3)):
    """The scene in the layout of blend_scenes (s, colors, cov6, W, H): SH colours, degree 3."""
    g = pixel_gaussians(W, H, P, seed, sigma, stretch=stretch)
    return dict(s=scene_inputs(g, static_camera(W, H), 3, bg=bg), colors=None, cov6=None, W=W, H=H)


_cache = {}


def get(name):
    """The scene of CASES[name], built once."""
    if name not in _cache:
        c = CASES[name]
        long = max(c["W"], c["H"])
        # a frame of 65,535 tiles: a standard deviation of one slice of the long axis, so that
        # 3 sigma reaches the neighbours' slices wherever the jitter puts the centres
        stretch = long / c["P"] if name in LONG else None
        _cache[name] = dict(scene_of(c["W"], c["H"], c["P"], SEEDS.get(name, 0), c["sigma"],
                                     stretch), name=name)
    return _cache[name]


def tiles_of(orc):
    return (orc["point_keys"] >> np.uint64(32)).astype(np.int64)


def per_row_and_column(orc, W, H):
    """(pairs per tile row, pairs per tile column) of an oracle result's lists."""
    gx, gy = grid(W, H)
    t = tiles_of(orc)
    return np.bincount(t // gx, minlength=gy), np.bincount(t % gx, minlength=gx)


def row_pass_input_rows(orc, W, H):
    """The tile row of every entry of the list the row pass sorts (column-first form): the pairs
    by tile column, inside a column by the Gaussians' depth order (ties by id, as the stable
    depth sort leaves them) and inside a Gaussian by row."""
    gx, _ = grid(W, H)
    t = tiles_of(orc)
    depth = (orc["point_keys"] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ids = orc["point_list"].astype(np.int64)
    order = np.lexsort((t // gx, ids, depth, t % gx))
    return (t // gx)[order]


# ---- the P edge: col_shift = 24 and P = 2^24, 2^24 + 1 ------------------------------------------
P_EDGE = 1 << 24
P_EDGE_FRAME = (16, 2064)  # 1 x 129 tiles: ybits 8, the smallest frame whose limit is 2^24
P_EDGE_VISIBLE = 5000  # (K >= 3 sort tiles takes 5,000 on 129 tiles)


def p_edge_arrays():
    """The arrays of the P = 2^24 + 1 scene, SH degree 0 with M = 1 (0.94 GB): 5,000 visible
    Gaussians of a 16 x 2064 scene at ids spread over [0, 2^24), two of them at 2^24 - 2 and
    2^24 - 1, one more at 2^24, and everything else behind the camera with constant fields.
    Returns (GaussianData of 2^24 + 1, ids of the visible ones, ascending).  The scene of
    P = 2^24 is its first 2^24 rows."""
    W, H = P_EDGE_FRAME
    n = P_EDGE_VISIBLE + 1
    vis = pixel_gaussians(W, H, n, seed=24, sigma=MID, M=1)
    rng = np.random.default_rng(24)
    ids = np.sort(rng.choice(P_EDGE - 2, n - 3, replace=False))
    ids = np.concatenate([ids, [P_EDGE - 2, P_EDGE - 1, P_EDGE]]).astype(np.int64)
    P = P_EDGE + 1
    xyz = np.empty((P, 3), F32)
    xyz[:] = (0.0, 0.0, 8.0)  # behind the camera at (0, 0, 4), which looks down -z
    rot = np.zeros((P, 4), F32)
    rot[:, 0] = 1.0
    scale = np.full((P, 3), 0.01, F32)
    opacity = np.full((P, 1), 0.5, F32)
    sh = np.zeros((P, 3), F32)
    for dst, src in ((xyz, vis.xyz), (rot, vis.rot), (scale, vis.scale), (opacity, vis.opacity),
                     (sh, vis.sh)):
        dst[ids] = src
    return GaussianData(xyz, rot, scale, opacity, sh), ids


def fields(g):
    return g.xyz, g.rot, g.scale, g.opacity, g.sh


def p_edge_scene(g, P):
    """The first P Gaussians of p_edge_arrays' as a scene (views, no copies)."""
    W, H = P_EDGE_FRAME
    part = GaussianData(*(a[:P] for a in fields(g)))
    return dict(s=scene_inputs(part, static_camera(W, H), 0), colors=None, cov6=None, W=W, H=H)
