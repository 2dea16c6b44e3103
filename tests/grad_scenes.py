"""The scenes of the backward-pass tests (test_grad_reference.py on the CPU, test_gpu_backward.py
on the GPU): the smallest shapes at which the backward kernels can still go wrong.  Each is a
dict in the layout of preprocess_scenes (s = gpu_helpers.scene_inputs, colors, cov6) plus dL, the
image gradient the tests feed.  The seeds are chosen so that the float64 reference
(grad_reference) finds no decision within rounding of its gate (test_grad_reference.py asserts
it: zero near-gate pairs in every scene).

  S1 chain        P = 96, 40 x 24 px: 3 x 2 tiles with a partial right column and bottom row; SH
                  degree 3 (M = 16), scales and rotations, bg (0.3, 0.6, 0.1), scale_modifier 1.3
  S2 long_lists   P = 200 over 32 x 16 px (2 tiles), each list > 128 entries (3 chunks, odd
                  counts); opacities up to 1.0: pixels terminate and o G caps at 0.99
  S3 precomputed  P = 64 with cov3D_precomp and colors_precomp
  S4 edges        M = 16 with D = 1, about a third of the colour channels clamped at 0, Gaussians
                  beyond the 1.3 tan clamp that still reach the frame, Gaussians with z <= 0.2, and
                  one whose 2D covariance has det == 0 exactly
"""
from __future__ import annotations

import numpy as np

from gaussiansplattingviewer_amd.camera import static_camera
from gaussiansplattingviewer_amd.gaussian_data import GaussianData
from gpu_helpers import scene_inputs

F32 = np.float32
NAMES = ("chain", "long_lists", "precomputed", "edges")
SEEDS = {"chain": 1, "long_lists": 43, "precomputed": 3, "edges": 4}


def _gaussians(rng, P, half_x, half_y, s_lo, s_hi, o_lo, o_hi, M=16, dc=(0.0, 0.6), rest=0.1):
    xyz = np.stack([rng.uniform(-half_x, half_x, P), rng.uniform(-half_y, half_y, P),
                    rng.uniform(-1.0, 1.0, P)], 1)
    scale = np.exp(rng.uniform(np.log(s_lo), np.log(s_hi), (P, 3)))
    rot = rng.standard_normal((P, 4))
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    opacity = rng.uniform(o_lo, o_hi, (P, 1))
    sh = np.concatenate([rng.normal(dc[0], dc[1], (P, 3)), rng.normal(0, rest, (P, 3 * (M - 1)))], 1)
    a = lambda v: np.ascontiguousarray(v, F32)  # noqa: E731
    return GaussianData(a(xyz), a(rot), a(scale), a(opacity), a(sh))


def _cov6(g, mod=1.0):
    """R diag((mod s)^2) R^T of every Gaussian, upper triangle, in float64 then float32."""
    r, x, y, z = (g.rot[:, k].astype(np.float64) for k in range(4))
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                  2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                  2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    N = R * (mod * g.scale.astype(np.float64))[:, None, :]
    S = N @ N.transpose(0, 2, 1)
    return np.ascontiguousarray(np.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2],
                                          S[:, 2, 2]], 1), F32)


def build(name):
    rng = np.random.default_rng(SEEDS[name])
    colors = cov6 = None
    special = {}
    if name == "chain":
        W, H, D, mod, bg = 40, 24, 3, 1.3, (0.3, 0.6, 0.1)
        g = _gaussians(rng, 96, 2.2, 1.4, 0.05, 0.35, 0.1, 0.9)
    elif name == "long_lists":
        W, H, D, mod, bg = 32, 16, 3, 1.0, (0.2, 0.4, 0.6)
        g = _gaussians(rng, 200, 2.4, 0.9, 0.25, 0.8, 0.02, 0.3)
        g.opacity[::9] = 1.0
    elif name == "precomputed":
        W, H, D, mod, bg = 40, 24, 0, 1.0, (0.2, 0.4, 0.6)
        g = _gaussians(rng, 64, 2.2, 1.4, 0.05, 0.35, 0.1, 0.9)
        cov6 = _cov6(g)
        colors = np.ascontiguousarray(rng.uniform(0, 1, (64, 3)), F32)
    elif name == "edges":
        W, H, D, mod, bg = 24, 24, 1, 1.0, (0.2, 0.4, 0.6)
        g = _gaussians(rng, 80, 1.4, 1.4, 0.05, 0.35, 0.1, 0.9, dc=(-1.0, 1.8), rest=0.3)
        # beyond the 1.3 tan clamp (|t.x / t.z| or |t.y / t.z| > 0.39 at this camera), near and
        # large enough to reach the frame
        n = 8
        side = rng.choice([-1.0, 1.0], n)
        g.xyz[:n, 0] = side * rng.uniform(0.55, 0.9, n)
        g.xyz[:n, 1] = rng.uniform(-0.2, 0.2, n)
        g.xyz[2:4, :2] = g.xyz[2:4, 1::-1]  # two of them beyond the y clamp
        g.xyz[:n, 2] = 3.0
        g.scale[:n] = rng.uniform(0.15, 0.3, (n, 3))
        special["clamp"] = np.arange(n)
        # z <= 0.2: at and behind the camera plane (the eye is at z = 4, looking down -z)
        g.xyz[n:n + 4, 2] = (3.8, 3.9, 4.0, 5.0)
        special["behind"] = np.arange(n, n + 4)
        # det == 0: on the axis, the unnormalised quaternion (0.5, 0, 0, 0.5) is exactly
        # 0.5 [[1, -1, 0], [1, 1, 0], [0, 0, 1]], so scale (1024, 0, 0) gives cov2 = h [[1, 1], [1, 1]]
        # with one float h > 2^24 that absorbs the 0.3: a c - b b == 0
        k = n + 4
        g.xyz[k] = (0.0, 0.0, 0.0)
        g.rot[k] = (0.5, 0.0, 0.0, 0.5)
        g.scale[k] = (1024.0, 0.0, 0.0)
        special["det0"] = np.array([k])
    else:
        raise KeyError(name)
    s = scene_inputs(g, static_camera(W, H), D, bg=bg, scale_modifier=mod)
    dL = np.ascontiguousarray(rng.standard_normal((3, H, W)), F32)
    return dict(name=name, s=s, colors=colors, cov6=cov6, W=W, H=H, dL=dL, special=special)


_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = build(name)
    return _cache[name]
