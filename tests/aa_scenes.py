"""The scenes of the antialiasing tests (test_aa_reference.py on the CPU, test_gpu_antialiasing.py
on the GPU): the four grad_scenes as they are, plus two of the same size in the same layout
(s = gpu_helpers.scene_inputs, colors, cov6, dL, special) that put the opacity compensation
rho = det(cov2D) / det(cov2D + 0.3 I), s = sqrt(max(0.000025, rho)) where it can go wrong.

  subpixel  P = 160, 40 x 24 px (3 x 2 tiles, partial right column and bottom row), SH degree 3,
            scales and rotations.  The screen-space sigma runs log-uniformly over about 0.18 ..
            2.4 px (10 px per world unit at the scene's depth), so rho spans about 0.01 .. 0.9;
            every fifth Gaussian has an opacity of 0.01 .. 0.03, whose effective opacity falls
            below 1/255; the first 6 are needles (axis ratio 100:1, about 3 px long), where
            D0 = a' c' - b b cancels to ~1e-4 of its terms but stays far above the floor.
  floor     P = 120, 40 x 24 px, cov3D_precomp and colors_precomp.  The first 10 rows of the
            covariance are all zero (rho exactly 0: a point, drawn as the bare 0.3 px dilation),
            with opacity 0.99 so that some still reach 1/255 at a pixel centre; the next 6 are
            discs seen edge-on (spanned by the Gaussian's own view ray and a direction across it:
            the ray projects to nothing, so D0 is 0 up to rounding), opacity 0.99 as well; the
            rest is ordinary.

The seeds are chosen so that aa_reference finds no Gaussian within rounding of the floor gate that
is not flagged as such, and at most 10 % flagged (test_aa_reference.py asserts both)."""
from __future__ import annotations

import numpy as np

import grad_scenes
from gaussiansplattingviewer_amd.camera import static_camera
from gpu_helpers import scene_inputs

F32 = np.float32
NEW = ("subpixel", "floor")
NAMES = grad_scenes.NAMES + NEW
SEEDS = {"subpixel": 7, "floor": 12}
EYE_Z = 4.0  # static_camera: the eye at (0, 0, 4), looking down -z


def build(name):
    rng = np.random.default_rng(SEEDS[name])
    W, H, bg = 40, 24, (0.2, 0.4, 0.6)
    colors = cov6 = None
    special = {}
    if name == "subpixel":
        P, D, mod = 160, 3, 1.0
        g = grad_scenes._gaussians(rng, P, 1.8, 1.0, 0.018, 0.24, 0.3, 0.95)
        g.opacity[4::5] = rng.uniform(0.01, 0.03, (len(g.opacity[4::5]), 1))
        special["faint"] = np.arange(P)[4::5]
        n = 6  # needles: about 3 px long, 100:1
        g.scale[:n] = np.array([0.3, 0.003, 0.003], F32)
        g.opacity[:n] = rng.uniform(0.5, 0.9, (n, 1))
        special["needles"] = np.arange(n)
    elif name == "floor":
        P, D, mod = 120, 0, 1.0
        g = grad_scenes._gaussians(rng, P, 1.8, 1.0, 0.05, 0.3, 0.2, 0.9)
        cov6 = grad_scenes._cov6(g)
        nz, nd = 10, 6
        cov6[:nz] = 0.0
        g.opacity[:nz] = 0.99
        special["zero"] = np.arange(nz)
        # discs: sigma^2 (d d^T + u u^T), d the unit ray from the eye, u across it
        for k in range(nz, nz + nd):
            p = g.xyz[k].astype(np.float64)
            d = p - np.array([0.0, 0.0, EYE_Z])
            d /= np.linalg.norm(d)
            u = np.cross(d, rng.standard_normal(3))
            u /= np.linalg.norm(u)
            S = 0.2 ** 2 * (np.outer(d, d) + np.outer(u, u))
            cov6[k] = (S[0, 0], S[0, 1], S[0, 2], S[1, 1], S[1, 2], S[2, 2])
        g.opacity[nz:nz + nd] = 0.99
        special["discs"] = np.arange(nz, nz + nd)
        colors = np.ascontiguousarray(rng.uniform(0, 1, (P, 3)), F32)
    else:
        raise KeyError(name)
    s = scene_inputs(g, static_camera(W, H), D, bg=bg, scale_modifier=mod)
    dL = np.ascontiguousarray(rng.standard_normal((3, H, W)), F32)
    return dict(name=name, s=s, colors=colors, cov6=cov6, W=W, H=H, dL=dL, special=special)


_cache = {}


def get(name):
    if name in grad_scenes.NAMES:
        return grad_scenes.get(name)
    if name not in _cache:
        _cache[name] = build(name)
    return _cache[name]
