"""The strips of the strip-backward tests (test_strip_grad_reference.py on the CPU,
test_gpu_strip_backward.py on the GPU; gsr_backward_strip): partitions of the tile
rows of three scenes of frame_grad_scenes, the smallest that reach each path.

  scene  shape                      strips (a partition)      reaches
  wall   32 x 32, 2 x 2 tiles       (0,1) (1,2)               waves that stop early; Gaussians
                                                              straddling the cut
  frame  200 x 136, 13 x 9 tiles,   (0,3) (3,8) (8,9)         a strip whose rows = 8 (not 16 (e -
         the last row 8 px                                    b)); the four big Gaussians clipped
                                                              by every cut
  tall   24 x 4112, 2 x 257 tiles   (0,1) (1,257)             the second strip has 256 rows, so its
                                                              rebuild bins column-first with packed
                                                              words and id_mask, while the whole
                                                              frame takes the per-pair form

Every strip holds the conditions test_strip_grad_reference.py asserts -- at most fs.MASK_CAP of its
pixels masked, fs.QUADRANT_KEEP per quadrant, a Gaussian wholly inside it, one clipped by it, one
without a tile in it -- with the cuts above (none had to be moved), but for wall: its two tile rows
allow one cut only, and 418 of its 420 Gaussians straddle it (which is what the scene is here
for).  (0,1) has 2 Gaussians wholly inside and none without a tile, (1,2) has 2 without a tile and
none wholly inside, so on wall the three classes are asserted over the partition, not per strip;
frame's and tall's strips hold all three each.

The backward on the strip [b, e) is the whole frame's with the image gradients zero outside the
strip's pixel rows, so the strip reference is frame_grad_scenes.reference's machinery under
fs.masked further zeroed outside those rows.  It walks only the strip's tiles of the oracle's
lists: a pixel with zero image gradients adds exactly nothing (test_strip_grad_reference.py checks
that against the walk over every tile on wall).
"""
from __future__ import annotations

import numpy as np
import torch

import aa_reference as ar
import camera_grad_reference as cgr
import frame_grad_scenes as fs
import grad_reference as gr

F32 = np.float32
STRIPS = {"wall": ((0, 1), (1, 2)),
          "frame": ((0, 3), (3, 8), (8, 9)),
          "tall": ((0, 1), (1, 257))}
# the losses a test runs per scene: fs.reference's kinds
KINDS = {"wall": ("colour",), "frame": ("colour", "all", "all_aa"), "tall": ("colour",)}
CASES = [(n, s) for n in STRIPS for s in STRIPS[n]]


def grid(sc):
    return (sc["W"] + 15) // 16, (sc["H"] + 15) // 16


def pixel_rows(sc, strip):
    """(y0, y1): the strip's pixel rows [y0, y1) of the frame."""
    return 16 * strip[0], min(sc["H"], 16 * strip[1])


def full_dL(sc, strip, planes=True):
    """(dL, dLp): fs.masked, zero outside the strip's rows; whole-frame shapes."""
    y0, y1 = pixel_rows(sc, strip)
    out = []
    for a in fs.masked(sc, planes):
        if a is not None:
            z = np.zeros_like(a)
            z[:, y0:y1] = a[:, y0:y1]
            a = z
        out.append(a)
    assert np.abs(out[0]).max() > 0
    return tuple(out)


def local_dL(sc, strip, planes=True):
    """(dL, dLp) as gsr_backward_strip takes them: the strip's rows alone, [3, rows, W] each (dLp:
    the three planes' [rows, W] stacked)."""
    y0, y1 = pixel_rows(sc, strip)
    return tuple(None if a is None else np.ascontiguousarray(a[:, y0:y1])
                 for a in fs.masked(sc, planes))


def strip_lists(sc, strip):
    """The oracle's lists with the ranges of the tiles outside the strip emptied."""
    ranges, plist = fs.lists_of(sc)
    ranges = np.asarray(ranges).reshape(-1, 2)
    gx, _ = grid(sc)
    only = np.zeros_like(ranges)
    only[strip[0] * gx:strip[1] * gx] = ranges[strip[0] * gx:strip[1] * gx]
    return only, plist


def reference(sc, strip, kind, dtype=torch.float64, gates=None, every_tile=False):
    """fs.reference under full_dL: the strip's reference gradients.  every_tile: walk the whole
    frame's lists instead of the strip's tiles (the same numbers; slower).  The float64 results
    are kept per scene."""
    key = ("strip_ref", tuple(strip), kind)
    if dtype == torch.float64 and not every_tile and key in sc:
        return sc[key]
    lists = fs.lists_of(sc) if every_tile else strip_lists(sc, strip)
    radii = fs.oracle_of(sc)["radii"]
    dL, dLp = full_dL(sc, strip)
    if kind == "colour":
        out = gr.scene_gradients(sc, lists, radii, dL, dtype, gates)
    elif kind == "all":
        out = cgr.scene_gradients(sc, lists, radii, dL, dLp, dtype, gates)
    else:
        out = ar.scene_gradients(sc, lists, radii, dL, dLp, dtype, gates)
    if dtype == torch.float64 and not every_tile:
        sc[key] = out
    return out


def tile_rows_of(sc):
    """(lo, hi) [P] each: the first and one past the last tile row a Gaussian is listed in by the
    oracle's (untight) lists -- the rows of its rect; lo == hi == 0 without a tile."""
    if "tile_rows" not in sc:
        ranges, plist = fs.lists_of(sc)
        ranges = np.asarray(ranges).reshape(-1, 2).astype(np.int64)
        plist = np.asarray(plist).astype(np.int64)
        gx, gy = grid(sc)
        P = len(sc["s"]["g"].xyz)
        lo, hi = np.full(P, gy, np.int64), np.zeros(P, np.int64)
        for tile, (r0, r1) in enumerate(ranges):
            ids = plist[r0:r1]
            lo[ids] = np.minimum(lo[ids], tile // gx)
            hi[ids] = np.maximum(hi[ids], tile // gx + 1)
        lo[hi == 0] = 0
        sc["tile_rows"] = (lo, hi)
    return sc["tile_rows"]


def classes(sc, strip):
    """(inside, clipped, none) [P] bool each: the Gaussian's rect lies wholly inside the strip's
    rows; it has tiles inside and outside; it has no tile in the strip (culled Gaussians and
    Gaussians without any tile included)."""
    lo, hi = tile_rows_of(sc)
    b, e = strip
    has = (np.minimum(hi, e) > np.maximum(lo, b)) & (hi > lo)
    inside = has & (lo >= b) & (hi <= e)
    return inside, has & ~inside, ~has


# ---- the tolerance of the GPU tests: measured, not chosen ------------------------------------------
# frame_grad_scenes.F32_SPREAD's rule per strip: fs.err of `reference` evaluated in float32 against
# float64 (lists and gates of the float64 run), relative to the strip's own largest gradient,
# measured on the CPU (test_strip_grad_reference.py re-measures it and holds each constant to within
# a factor 2).  The GPU tests allow gr.BOUND_FACTOR x f of the strip they run.
F32_SPREAD = {
    ("wall", (0, 1), "colour"): {"means3D": 3.5e-7, "means2D": 3.5e-7, "means2D_px": 3.5e-7,
        "conic": 3.9e-7, "opacity": 4.4e-7, "rgb": 2.5e-7, "shs": 3.2e-7, "scales": 5.6e-7,
        "rotations": 4.3e-7},
    ("wall", (1, 2), "colour"): {"means3D": 2.2e-7, "means2D": 1.9e-7, "means2D_px": 1.9e-7,
        "conic": 6.8e-7, "opacity": 6.3e-7, "rgb": 3.1e-7, "shs": 3.2e-7, "scales": 6.8e-7,
        "rotations": 6.8e-7},
    ("frame", (0, 3), "colour"): {"means3D": 2.5e-6, "means2D": 2.3e-6, "means2D_px": 2.3e-6,
        "conic": 9.7e-7, "opacity": 7.5e-7, "rgb": 8.5e-7, "shs": 7.9e-7, "scales": 3.0e-6,
        "rotations": 1.0e-6},
    ("frame", (0, 3), "all"): {"means3D": 2.2e-6, "means2D": 1.5e-6, "opacity": 1.0e-6,
        "shs": 7.9e-7, "scales": 2.1e-6, "rotations": 1.0e-6, "viewmatrix": 7.8e-8,
        "projmatrix": 5.9e-8, "campos": 1.0e-7},
    ("frame", (0, 3), "all_aa"): {"means3D": 1.9e-6, "means2D": 1.8e-6, "opacity": 8.6e-7,
        "shs": 7.9e-7, "scales": 2.3e-6, "rotations": 1.1e-6, "viewmatrix": 7.3e-8,
        "projmatrix": 1.1e-7, "campos": 4.3e-8},  # (campos: see below)
    ("frame", (3, 8), "colour"): {"means3D": 2.5e-6, "means2D": 1.9e-6, "means2D_px": 2.8e-6,
        "conic": 1.1e-6, "opacity": 2.8e-7, "rgb": 7.1e-7, "shs": 8.3e-7, "scales": 1.0e-6,
        "rotations": 2.7e-6},
    ("frame", (3, 8), "all"): {"means3D": 2.1e-6, "means2D": 1.7e-6, "opacity": 6.2e-7,
        "shs": 8.3e-7, "scales": 1.0e-6, "rotations": 4.0e-6, "viewmatrix": 1.1e-7,
        "projmatrix": 1.5e-7, "campos": 9.9e-8},
    ("frame", (3, 8), "all_aa"): {"means3D": 2.4e-6, "means2D": 2.0e-6, "opacity": 6.4e-7,
        "shs": 7.9e-7, "scales": 9.5e-7, "rotations": 3.1e-6, "viewmatrix": 7.0e-8,
        "projmatrix": 1.4e-7, "campos": 6.9e-8},
    ("frame", (8, 9), "colour"): {"means3D": 2.0e-6, "means2D": 2.1e-6, "means2D_px": 2.1e-6,
        "conic": 4.8e-7, "opacity": 1.3e-6, "rgb": 5.6e-7, "shs": 4.8e-7, "scales": 1.7e-6,
        "rotations": 1.4e-6},
    ("frame", (8, 9), "all"): {"means3D": 2.1e-6, "means2D": 2.1e-6, "opacity": 1.3e-6,
        "shs": 4.8e-7, "scales": 2.0e-6, "rotations": 1.5e-6, "viewmatrix": 2.2e-7,
        "projmatrix": 6.1e-7, "campos": 1.5e-7},
    ("frame", (8, 9), "all_aa"): {"means3D": 2.4e-6, "means2D": 2.6e-6, "opacity": 1.1e-6,
        "shs": 4.7e-7, "scales": 2.3e-6, "rotations": 1.7e-6, "viewmatrix": 2.6e-7,
        "projmatrix": 6.0e-7, "campos": 2.7e-7},
    ("tall", (0, 1), "colour"): {"means3D": 3.9e-5, "means2D": 3.9e-5, "means2D_px": 3.9e-5,
        "conic": 6.3e-5, "opacity": 7.7e-5, "rgb": 2.1e-5, "shs": 2.1e-5, "scales": 1.2e-5,
        "rotations": 2.4e-5},
    ("tall", (1, 257), "colour"): {"means3D": 9.7e-5, "means2D": 1.1e-4, "means2D_px": 1.1e-4,
        "conic": 7.0e-5, "opacity": 7.1e-5, "rgb": 4.1e-5, "shs": 3.9e-5, "scales": 5.5e-5,
        "rotations": 4.9e-5},
}
# (frame (0, 3), all_aa, campos: a sum over every Gaussian that sits below one float32 ulp, as
# camera_grad_reference notes; two machines' CPUs measure 2.3e-8 and 7.9e-8 for it, whatever the
# thread count, while every other constant moves by a factor 1.6 at the most.  The constant is
# their geometric mean, which holds the factor 2 on both.)
for _t in F32_SPREAD.values():
    if "rgb" in _t:
        _t["colors"] = _t["rgb"]


def bound(name, strip, kind, key):
    return gr.BOUND_FACTOR * F32_SPREAD[(name, tuple(strip), kind)][key]


def spread(sc, strip, kind, keys):
    """The measurement behind F32_SPREAD for one (scene, strip, loss)."""
    r64 = reference(sc, strip, kind)
    assert r64["near"][0] == 0
    r32 = reference(sc, strip, kind, torch.float32, r64["gates"])
    return {k: fs.err(r32[k], r64, k) for k in keys if k in r64 and np.abs(r64[k]).max() > 0}
