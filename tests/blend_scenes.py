"""Small scenes that drive the blend (csrc/blend.hip k_blend_q) through the paths the large
synthetic scenes reach only by accident; shared by the CPU check of the float64 reference
(test_blend_reference.py) and the GPU check (test_gpu_blend_exact.py).

Every scene goes through the normal forward with colors_precomp and cov3D_precomp, so a splat
is placed by its pixel centre, its view depth (the list order) and its 2D covariance in px^2
(upstream adds 0.3 I to it).  Camera: the static view at (0, 0, 4); a point at view depth d
projects to  px = (W - 1) / 2 + f x / d,  py = (H - 1) / 2 - f y / d,  f = H / (2 tan(fovy / 2)).

  chunk_edges_N   24x20 (one tile and three ragged ones); N splats far wider than the frame, alpha
                  0.02..0.05 at every pixel: no cull, no termination, lists of exactly N
  chunk_survivors 24x20; small splats so that, per quadrant of tile 0, one chunk of 64 list
                  entries leaves 64, 63, 1 and 0 survivors of the cull and the next an odd count
  pads_K          64x32 (8 tiles); tile t's list is one chunk of 64 whose survivors number
                  k = 63 - 2 (8 K + t) in its quadrant A and 64 - k in D (none in B, C), so over
                  K = 0, 1 the pad slot of an odd count is written at every position 1 .. 63
  indefinite      32x16; every splat in both tiles' lists: list positions 0..63 positive definite,
                  64..127 with det(cov2D + 0.3 I) < 0, 128..255 mixed
  on_centre       64x32; centres exactly on pixel centres and on quadrant centres (x.5)
  opacity_edges   64x48; opacity 0, 1e-40, float32(1/255) and its neighbours, 0.5, 0.99, 1, 1.5
  opaque_stack    64x48; ten coincident wide splats of opacity 1 over a coloured background
  term_window     16x16; T = 1 -> 0.01 -> 1.05e-4 (inside [1e-4, 1.1e-4)) -> terminated
  ragged_WxH      1x1, 7x5, 9x23, 17x9: quadrants cut by the frame or wholly outside it
  synthetic       160x120, 3k synthetic_gaussians through SH colours: the ordinary case
"""
from __future__ import annotations

import numpy as np

from gaussiansplattingviewer_amd.camera import Camera, static_camera
from gaussiansplattingviewer_amd.gaussian_data import GaussianData, synthetic_gaussians

from gpu_helpers import run_oracle, scene_inputs

F32 = np.float32
A_MIN = F32(1.0) / F32(255.0)
BG = (0.2, 0.4, 0.6)
CHUNK_NS = (1, 2, 63, 64, 65, 127, 128, 129, 193)
RAGGED = ((1, 1), (7, 5), (9, 23), (17, 9))
NAMES = (tuple(f"chunk_edges_{n}" for n in CHUNK_NS) +
         ("chunk_survivors", "indefinite", "on_centre", "opacity_edges", "opaque_stack",
          "term_window", "pads_0", "pads_1") +
         tuple(f"ragged_{w}x{h}" for w, h in RAGGED) + ("synthetic",))


def _focal(H):
    return H / (2.0 * Camera(H, H).get_htanfovxy_focal()[1])


def _splats(W, H, px, py, depth, cov, opacity, colors, bg=BG):
    """Scene dict of splats given by pixel centre, view depth, 2D covariance (cxx, cxy, cyy in
    px^2, before the 0.3 I) and opacity.  The 3D covariance is the 2D one scaled back to the
    world at the splat's depth, in the x-y plane (zz ~ 0)."""
    px, py, depth, opacity = (np.asarray(v, np.float64).reshape(-1) for v in (px, py, depth, opacity))
    n = len(px)
    f = _focal(H)
    xyz = np.stack([(px - (W - 1) / 2.0) * depth / f, -(py - (H - 1) / 2.0) * depth / f,
                    4.0 - depth], axis=1).astype(F32)
    cov = np.asarray(cov, np.float64).reshape(n, 3) * ((depth / f) ** 2)[:, None]
    cov6 = np.zeros((n, 6), F32)
    cov6[:, 0], cov6[:, 1], cov6[:, 3], cov6[:, 5] = cov[:, 0], cov[:, 1], cov[:, 2], 1e-8
    return _scene(W, H, xyz, opacity, np.asarray(colors, F32).reshape(n, 3), cov6, bg)


def _scene(W, H, xyz, opacity, colors, cov6, bg=BG):
    n = len(xyz)
    g = GaussianData(np.ascontiguousarray(xyz, F32), np.tile(F32([1, 0, 0, 0]), (n, 1)),
                     np.full((n, 3), 0.01, F32), np.asarray(opacity, F32).reshape(n, 1),
                     np.zeros((n, 3), F32))
    return dict(s=scene_inputs(g, static_camera(W, H), 0, bg=bg), colors=colors, cov6=cov6,
                W=W, H=H)


def _iso(sigma):
    sigma = np.asarray(sigma, np.float64)
    return np.stack([sigma ** 2, np.zeros_like(sigma), sigma ** 2], axis=-1)


def _aniso(rng, n, s_lo, s_hi):
    """n positive-definite 2D covariances with axes logU(s_lo, s_hi) px at random angles."""
    s1 = np.exp(rng.uniform(np.log(s_lo), np.log(s_hi), n)) ** 2
    s2 = np.exp(rng.uniform(np.log(s_lo), np.log(s_hi), n)) ** 2
    th = rng.uniform(0, np.pi, n)
    c, s = np.cos(th), np.sin(th)
    return np.stack([c * c * s1 + s * s * s2, c * s * (s1 - s2), s * s * s1 + c * c * s2], axis=-1)


def _depths(n, rng=None):
    """Distinct view depths 3.5 .. 4.5 in list order (shuffled over the splats with rng)."""
    d = np.linspace(3.5, 4.5, n) if n > 1 else np.array([4.0])
    return d if rng is None else rng.permutation(d)


def run(oracle, sc):
    """The oracle's forward of a scene (rgb zeroed: neither side computes it with precomputed
    colours) -- computed once per scene and kept in it."""
    if "orc" not in sc:
        orc = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"])
        if sc["colors"] is not None:
            orc["rgb"] = np.zeros_like(orc["rgb"])
        sc["orc"] = orc
    return sc["orc"]


def features(sc, orc):
    return orc["rgb"] if sc["colors"] is None else sc["colors"]


def solve_centres(oracle, W, H, targets, depth=4.0):
    """xyz (float32) whose projected float32 centre is exactly each (px, py) of targets: the
    linear guess, then a search over the neighbouring float32 values of x and of y (the two
    are independent for this camera)."""
    targets = np.asarray(targets, np.float64).reshape(-1, 2)
    base = _splats(W, H, targets[:, 0], targets[:, 1], np.full(len(targets), depth),
                   _iso(np.ones(len(targets))), np.ones(len(targets)),
                   np.ones((len(targets), 3)))["s"]["g"].xyz
    out = base.copy()
    steps = np.arange(-400, 401)
    for axis in (0, 1):
        for i, t in enumerate(targets):
            cand = np.repeat(out[i][None], len(steps), axis=0)
            v = base[i, axis]
            cand[:, axis] = (v.view(np.int32) + steps * (1 if v >= 0 else -1)).astype(
                np.int32).view(F32) if v != 0 else F32(0)
            sc = _scene(W, H, cand, np.ones(len(cand)), np.ones((len(cand), 3), F32),
                        np.tile(F32([1e-3, 0, 0, 1e-3, 0, 1e-8]), (len(cand), 1)))
            m = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"],
                           stages="preprocess")["means2D"]
            hit = np.flatnonzero(m[:, axis] == F32(t[axis]))
            assert len(hit), f"no float32 coordinate projects to {t[axis]} (axis {axis})"
            out[i, axis] = cand[hit[len(hit) // 2], axis]
    return out


def build(oracle, name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name.startswith("chunk_edges_"):
        n = int(name.rsplit("_", 1)[1])
        W, H = 24, 20
        # centres 40..80 px off the frame's left or right edge: power stays clear of 0 in the
        # frame (a pixel at a centre is undecidable by definition, |power| <= its rounding)
        side = rng.random(n) < 0.5
        px = np.where(side, -rng.uniform(40, 80, n), W + rng.uniform(40, 80, n))
        return _splats(W, H, px, rng.uniform(-20, H + 20, n), _depths(n, rng),
                       _iso(rng.uniform(200, 300, n)), rng.uniform(0.025, 0.05, n),
                       rng.uniform(0, 1, (n, 3)))
    if name == "chunk_survivors":
        # tile 0's quadrants: A (0..7, 0..7), B (8..15, 0..7), C (0..7, 8..15), D (8..15, 8..15).
        # Opacity 0.05, sigma^2 = 1.2^2 + 0.3: alpha >= 1/255 within 2.26 sigma = 2.9 px.
        # Nearest 64 (one chunk): 63 on the A|B border (both), 1 on the A|C border (both);
        # then 5 in D, 3 in C, 2 in B.
        W, H = 24, 20
        px = np.concatenate([rng.uniform(7.2, 7.8, 63), [3.5], rng.uniform(11, 13, 5),
                             rng.uniform(3, 5, 3), rng.uniform(11, 13, 2)])
        py = np.concatenate([rng.uniform(2.5, 4.5, 63), [7.5], rng.uniform(11.5, 12.5, 5),
                             rng.uniform(11.5, 12.5, 3), rng.uniform(3, 4, 2)])
        n = len(px)
        return _splats(W, H, px, py, _depths(n), _iso(np.full(n, 1.2)), np.full(n, 0.05),
                       rng.uniform(0, 1, (n, 3)))
    if name.startswith("pads_"):
        # opacity 0.06, sigma^2 = 0.6^2 + 0.3 (radius ceil(3 sqrt(0.66 + sqrt(0.1))) = 3: the rect
        # stays in the tile): alpha >= 1/255 within 1.9 px of a centre that lies within 0.4 px of its quadrant's centre (4.5 px
        # from the next quadrant); A's and D's splats interleaved in depth, so the compaction
        # has gaps to close
        W, H, K = 64, 32, int(name[-1])
        px, py = [], []
        for t in range(8):
            k = 63 - 2 * (8 * K + t)
            in_a = rng.permutation(np.arange(64) < k)
            c = np.where(in_a, 3.5, 11.5)
            px.append(16 * (t % 4) + c + rng.uniform(-0.4, 0.4, 64))
            py.append(16 * (t // 4) + c + rng.uniform(-0.4, 0.4, 64))
        n = 8 * 64
        return _splats(W, H, np.concatenate(px), np.concatenate(py), _depths(n, rng),
                       _iso(np.full(n, 0.6)), np.full(n, 0.06), rng.uniform(0, 1, (n, 3)))
    if name == "indefinite":
        W, H, n = 32, 16, 256
        kind = np.concatenate([np.zeros(64, bool), np.ones(64, bool), rng.random(128) < 0.5])
        cov = _aniso(rng, n, 12.0, 30.0)  # radius >= 36 px: every splat in both tiles
        # indefinite: one axis sigma 12..30 px, the other eigenvalue -(1.5 .. 40) px^2
        s1 = rng.uniform(12.0, 30.0, n) ** 2
        s2 = -rng.uniform(1.5, 40.0, n)
        th = rng.uniform(0, np.pi, n)
        c, s = np.cos(th), np.sin(th)
        ind = np.stack([c * c * s1 + s * s * s2, c * s * (s1 - s2), s * s * s1 + c * c * s2], -1)
        cov[kind] = ind[kind]
        sc = _splats(W, H, rng.uniform(0, W, n), rng.uniform(0, H, n), _depths(n), cov,
                     rng.uniform(0.02, 0.06, n), rng.uniform(0, 1, (n, 3)))
        sc["indefinite"] = kind
        return sc
    if name == "on_centre":
        W, H = 64, 32
        tg = [(x, y) for y in (3.5, 11.5, 19.5, 27.5) for x in (3.5, 27.5, 35.5, 59.5)]
        tg += [(x, y) for y in (4.0, 15.0, 16.0, 24.0) for x in (7.0, 8.0, 31.0, 48.0)]
        n = len(tg)
        xyz = solve_centres(oracle, W, H, tg)  # one depth: list order = index order
        f = _focal(H)
        cov = np.where((np.arange(n) % 2 == 0)[:, None], _iso(rng.uniform(1.0, 3.0, n)),
                       _aniso(rng, n, 0.7, 5.0)) * (4.0 / f) ** 2
        cov6 = np.zeros((n, 6), F32)
        cov6[:, 0], cov6[:, 1], cov6[:, 3], cov6[:, 5] = cov[:, 0], cov[:, 1], cov[:, 2], 1e-8
        op = rng.uniform(0.3, 0.95, n).astype(F32)
        op[::4] = A_MIN  # alpha = opacity = float32(1/255) exactly at a centre on a pixel
        sc = _scene(W, H, xyz, op, rng.uniform(0, 1, (n, 3)).astype(F32), cov6)
        sc["targets"] = np.asarray(tg, F32)
        return sc
    if name == "opacity_edges":
        W, H = 64, 48
        vals = np.array([0.0, 1e-40, np.nextafter(A_MIN, F32(0)), A_MIN, np.nextafter(A_MIN, F32(1)),
                         0.5, 0.99, 1.0, 1.5], F32)
        n = 12 * len(vals)
        op = np.tile(vals, 12)
        return _splats(W, H, rng.uniform(0, W, n), rng.uniform(0, H, n), _depths(n, rng),
                       _aniso(rng, n, 1.0, 5.0), op, rng.uniform(0, 1, (n, 3)))
    if name == "opaque_stack":
        W, H, n = 64, 48, 10
        return _splats(W, H, np.full(n, 30.0), np.full(n, 22.0), _depths(n), _iso(np.full(n, 40.0)),
                       np.ones(n), rng.uniform(0.1, 1, (n, 3)))
    if name == "term_window":
        W, H = 16, 16
        return _splats(W, H, [7.5] * 4, [7.5] * 4, _depths(4), _iso(np.full(4, 800.0)),
                       [1.0, 0.9895, 0.5, 0.5], rng.uniform(0.1, 1, (4, 3)))
    if name.startswith("ragged_"):
        W, H = (int(v) for v in name.split("_")[1].split("x"))
        n = 300
        return _splats(W, H, rng.uniform(-3, W + 3, n), rng.uniform(-3, H + 3, n), _depths(n, rng),
                       _aniso(rng, n, 0.8, 5.0), rng.uniform(0.05, 0.95, n),
                       rng.uniform(0, 1, (n, 3)))
    if name == "synthetic":
        W, H = 160, 120
        return dict(s=scene_inputs(synthetic_gaussians(3000, 3, 3), static_camera(W, H), 3, bg=BG),
                    colors=None, cov6=None, W=W, H=H)
    raise KeyError(name)


def quadrant_survivors(orc, tile, W):
    """Per quadrant (4) and chunk of 64 list entries of a tile: how many entries can reach
    alpha >= 1/255 inside the quadrant's pixel-centre box (the blend's cull keeps exactly
    these, up to its rounding margins), from the oracle's float32 records, with q minimised
    over the box on a 1/8-px grid.  Also returns the smallest distance of any entry's
    ln(255 alpha_max) from 0, so that a scene can assert it is clear of those margins."""
    gx = (W + 15) // 16
    s, e = (int(v) for v in orc["ranges"][tile])
    ids = orc["point_list"][s:e]
    m2 = orc["means2D"][ids].astype(np.float64)
    co = orc["conic_opacity"][ids].astype(np.float64)
    tx, ty = tile % gx, tile // gx
    grid = np.arange(0, 7.0001, 0.125)
    counts = np.zeros((4, (len(ids) + 63) // 64), np.int64)
    margin = np.inf
    for q in range(4):
        X = 16 * tx + 8 * (q & 1) + grid[None, :, None]
        Y = 16 * ty + 8 * (q >> 1) + grid[None, None, :]
        dx, dy = m2[:, 0, None, None] - X, m2[:, 1, None, None] - Y
        power = (-0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy)
                 - co[:, 1, None, None] * dx * dy)
        lg = np.log(255.0 * co[:, 3]) + power.reshape(len(ids), -1).max(axis=1)
        margin = min(margin, float(np.abs(lg).min()))
        np.add.at(counts[q], np.arange(len(ids)) // 64, lg >= 0)
    return counts, margin
