"""The scenes of the camera-gradient tests (test_camera_grad_reference.py on the CPU,
test_gpu_camera_gradients.py on the GPU): the four of grad_scenes, reused as they are, and two
whose only purpose is the reduction over the Gaussians (gsr_backward_camera sums 27 values over
blocks of 256 Gaussians, then over the blocks):

  blocks  P = 600 over 40 x 24 px: three blocks, the last with 88 threads (one full wave and 24
          lanes of the next); scales and rotations, SH degree 3
  sparse  P = 66,000: the 96 Gaussians of `chain` at scattered indices, every other Gaussian behind
          the eye (world z in [4.5, 9], the eye at z = 4 looking down -z) and small, so the forward
          culls it (radii == 0; the tests assert it).  258 blocks: more than one pass of the
          finishing kernel's strided loop (256 threads), and most blocks bring exact zeros.  The
          image, the lists' order and the image gradient are chain's; the reference sees 96
          Gaussians

Same layout as grad_scenes (s, colors, cov6, W, H, dL, special); the seeds are chosen so that the
float64 reference finds no decision within rounding of a gate (test_camera_grad_reference.py).
"""
from __future__ import annotations

import numpy as np

import grad_scenes
from gaussiansplattingviewer_amd.camera import static_camera
from gpu_helpers import scene_inputs

F32 = np.float32
NAMES = grad_scenes.NAMES + ("blocks", "sparse")
SEEDS = dict(grad_scenes.SEEDS, blocks=7, sparse=11)
SPARSE_P = 66000


def build(name):
    rng = np.random.default_rng(SEEDS[name])
    special = {}
    if name == "blocks":
        W, H, D, mod, bg = 40, 24, 3, 1.0, (0.3, 0.6, 0.1)
        g = grad_scenes._gaussians(rng, 600, 2.2, 1.4, 0.04, 0.2, 0.05, 0.5)
        dL = np.ascontiguousarray(rng.standard_normal((3, H, W)), F32)
    elif name == "sparse":
        chain = grad_scenes.get("chain")
        c, s0 = chain["s"]["g"], chain["s"]
        W, H, D, mod, bg = chain["W"], chain["H"], s0["sh_degree"], s0["scale_modifier"], s0["bg"]
        P, n = SPARSE_P, len(c.xyz)
        at = np.sort(rng.choice(P, n, replace=False))  # ascending: chain's order among themselves
        g = grad_scenes._gaussians(rng, P, 2.2, 1.4, 0.005, 0.01, 0.1, 0.9)
        g.xyz[:, 2] = rng.uniform(4.5, 9.0, P).astype(F32)
        for dst, src in ((g.xyz, c.xyz), (g.rot, c.rot), (g.scale, c.scale),
                         (g.opacity, c.opacity), (g.sh, c.sh)):
            dst[at] = src
        dL = chain["dL"]
        special["kept"] = at
    else:
        raise KeyError(name)
    s = scene_inputs(g, static_camera(W, H), D, bg=bg, scale_modifier=mod)
    return dict(name=name, s=s, colors=None, cov6=None, W=W, H=H, dL=dL, special=special)


_cache = {}


def get(name):
    if name in grad_scenes.NAMES:
        return grad_scenes.get(name)
    if name not in _cache:
        _cache[name] = build(name)
    return _cache[name]


def plane_dL(name):
    """The planes' gradients of a scene, [3, H, W] float32 (depth, inverse depth, final_T):
    plane_grad_reference.plane_dL's for its scenes, made the same way for the two new ones."""
    sc = get(name)
    rng = np.random.default_rng(100 + SEEDS["chain" if name == "sparse" else name])
    return np.ascontiguousarray(rng.standard_normal((3, sc["H"], sc["W"])), F32)
