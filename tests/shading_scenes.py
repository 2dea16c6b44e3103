"""Scenes for the GL shadings (csrc/blend.hip k_shade_q, gsr_forward_shaded): the edge scenes of
blend_scenes.py that matter to a first-hit scan, and new ones built with its helpers; shared by
the CPU check of the float64 reference (test_shading_reference.py) and the GPU check
(test_gpu_shading.py).

  first_hit_N      24x20, N in 1, 64, 65, 129: N - 1 frame-wide splats of opacity 0.2 (never a
                   ball hit: 0.2 < 0.22), then one of opacity 0.9 as the deepest; every tile lists
                   all N.  The ball hit is the last entry of a chunk of 64, the first of the next,
                   or in the third chunk; the billboard hits at position 1
  sparse           64x48, 40 isotropic splats, sigma 1-4 px, opacity U(0.05, 0.99), centres in
                   the left 5/8 of the frame: hits and misses in every shading
  mixed            64x48, 400 anisotropic splats, sigma 1-6 px, opacity U(0.05, 0.99)
  threshold_edges  64x32; centres exactly on pixel centres, opacity float32(0.22), its two
                   neighbours, 0.2199, 0.2201 and 0.5, twice; covariance 0.01 + 0.3 px^2, so only
                   the centre pixel can reach alpha > 0.22 (the next one has alpha <= 0.11)
  quad_edges       64x32; isotropic splats with 3 sqrt(sigma^2 + 0.3) = 3 or 6, centred on a pixel
                   and 1e-3 px beside one (both axes): the billboard quad's edges fall on pixel
                   centres, and 1e-3 px inside and outside them
  front_transparent 32x16; an opacity-0 frame-wide splat nearest, three opaque ones behind it:
                   the billboard paints the transparent one, the ball modes see through it
"""
from __future__ import annotations

import numpy as np

import blend_scenes as bs

F32 = np.float32
O_MIN = F32(0.22)  # the ball modes' alpha threshold (gau_frag.glsl), as the float32 constant
FIRST_HIT_NS = (1, 64, 65, 129)
REUSED = ("chunk_survivors", "pads_0", "indefinite", "on_centre", "opacity_edges",
          "opaque_stack") + tuple(f"ragged_{w}x{h}" for w, h in bs.RAGGED) + ("synthetic",)
NEW = tuple(f"first_hit_{n}" for n in FIRST_HIT_NS) + (
    "sparse", "mixed", "threshold_edges", "quad_edges", "front_transparent")
NAMES = REUSED + NEW
SHADINGS = (1, 2, 3)  # _lib.GSR_SHADE_BILLBOARD, FLAT_BALL, GAUSS_BALL

THRESHOLD_OPACITIES = np.array([O_MIN, np.nextafter(O_MIN, F32(0)), np.nextafter(O_MIN, F32(1)),
                                0.2199, 0.2201, 0.5], F32)
THRESHOLD_TARGETS = [(5 + 10 * i, 6 + 3 * (i % 2)) for i in range(6)] + \
                    [(8 + 10 * i, 22 + 3 * (i % 2)) for i in range(6)]
# (x, y, quad half-width E, offset of the centre from the pixel in both axes)
QUAD_SPLATS = [(6, 8, 3, 0.0), (16, 8, 3, 1e-3), (26, 8, 3, -1e-3), (42, 9, 6, 0.0),
               (10, 23, 6, 1e-3), (27, 23, 6, -1e-3), (44, 25, 3, 0.0)]


def _on_pixels(oracle, W, H, targets, cov_px, opacity, colors, exact):
    """Splats at one depth (list order = index order) with the 2D covariance cov_px (px^2, before
    the 0.3 I); the rows of `exact` get a float32 centre exactly on their target."""
    targets = np.asarray(targets, np.float64)
    n = len(targets)
    sc = bs._splats(W, H, targets[:, 0], targets[:, 1], np.full(n, 4.0), cov_px, opacity, colors)
    xyz = sc["s"]["g"].xyz.copy()
    exact = np.flatnonzero(exact)
    xyz[exact] = bs.solve_centres(oracle, W, H, targets[exact])
    out = bs._scene(W, H, xyz, opacity, np.asarray(colors, F32), sc["cov6"])
    out["targets"] = targets
    return out


def build(oracle, name):
    if name in REUSED:
        return bs.build(oracle, name)
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("first_hit_"):
        n = int(name.rsplit("_", 1)[1])
        W, H = 24, 20
        # centres 40..80 px off the frame's left or right edge, as blend_scenes chunk_edges_N:
        # power stays clear of 0 in the frame, and >= -0.16 (sigma >= 200, <= 112 px away), so
        # the opacity-0.9 splat has alpha >= 0.76 at every pixel
        side = rng.random(n) < 0.5
        px = np.where(side, -rng.uniform(40, 80, n), W + rng.uniform(40, 80, n))
        op = np.full(n, 0.2)
        op[-1] = 0.9
        return bs._splats(W, H, px, rng.uniform(-20, H + 20, n), bs._depths(n),
                          bs._iso(rng.uniform(200, 300, n)), op, rng.uniform(0, 1, (n, 3)))
    if name == "sparse":
        W, H, n = 64, 48, 40
        return bs._splats(W, H, rng.uniform(0, 40, n), rng.uniform(0, H, n), bs._depths(n, rng),
                          bs._iso(rng.uniform(1.0, 4.0, n)), rng.uniform(0.05, 0.99, n),
                          rng.uniform(0, 1, (n, 3)))
    if name == "mixed":
        W, H, n = 64, 48, 400
        return bs._splats(W, H, rng.uniform(0, W, n), rng.uniform(0, H, n), bs._depths(n, rng),
                          bs._aniso(rng, n, 1.0, 6.0), rng.uniform(0.05, 0.99, n),
                          rng.uniform(0, 1, (n, 3)))
    if name == "threshold_edges":
        W, H = 64, 32
        n = len(THRESHOLD_TARGETS)
        return _on_pixels(oracle, W, H, THRESHOLD_TARGETS, bs._iso(np.full(n, 0.1)),
                          np.tile(THRESHOLD_OPACITIES, 2), rng.uniform(0.1, 1, (n, 3)),
                          np.ones(n, bool))
    if name == "quad_edges":
        W, H = 64, 32
        q = np.asarray(QUAD_SPLATS, np.float64)
        n = len(q)
        cov = bs._iso(np.sqrt((q[:, 2] / 3.0) ** 2 - 0.3))
        sc = _on_pixels(oracle, W, H, q[:, :2] + q[:, 3:4], cov, np.full(n, 0.9),
                        rng.uniform(0.1, 1, (n, 3)), q[:, 3] == 0.0)
        sc["quads"] = q
        return sc
    if name == "front_transparent":
        W, H = 32, 16
        px, py = [16.3, 6.4, 16.6, 25.7], [7.6, 7.3, 8.4, 7.8]
        return bs._splats(W, H, px, py, bs._depths(4), bs._iso([300.0, 3.0, 3.0, 3.0]),
                          [0.0, 1.0, 1.0, 1.0], rng.uniform(0.1, 1, (4, 3)))
    raise KeyError(name)


def run(oracle, sc):
    return bs.run(oracle, sc)
