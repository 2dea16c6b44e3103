"""Scenes of the median planes (gsr_forward_surface), shared by test_median_reference.py and
test_gpu_median.py: every scene of depth_scenes.py, blend_scenes' `synthetic`, and

  layers   64x48; three surfaces behind one another: 12 wall splats (sigma 40 px, opacity 0.9,
           view depth 8 .. 8.5) that close the frame, 16 veil splats (sigma 6 .. 10 px, opacity 0.3,
           depth 4 .. 4.4) and 40 foreground splats (sigma 1.5 .. 4 px, opacity 0.6 .. 0.95, depth
           1 .. 2, centres at least 4 px inside the frame).  Between the layers no Gaussian lies:
           the expected depth of gsr_forward_depth falls into the gaps (2.2, 3.8) and (4.6, 7.8)
           at most pixels, a median depth never can.
"""
from __future__ import annotations

import numpy as np

import blend_scenes as bs
import depth_scenes as ds

NAMES = ds.NAMES + ("synthetic", "layers")
GAPS = ((2.2, 3.8), (4.6, 7.8))  # view depths at which `layers` has no surface
LAYER_EDGES = (3.0, 6.0)         # foreground | veil | wall


def build(oracle, name):
    if name == "synthetic":
        return bs.build(oracle, name)
    if name != "layers":
        return ds.build(oracle, name)
    rng = np.random.default_rng(sum(map(ord, name)))
    W, H = 64, 48
    nw, nv, nf = 12, 16, 40
    px = np.concatenate([rng.uniform(0, W, nw), rng.uniform(0, W, nv), rng.uniform(4, W - 4, nf)])
    py = np.concatenate([rng.uniform(0, H, nw), rng.uniform(0, H, nv), rng.uniform(4, H - 4, nf)])
    depth = np.concatenate([rng.uniform(8.0, 8.5, nw), rng.uniform(4.0, 4.4, nv),
                            rng.uniform(1.0, 2.0, nf)])
    sigma = np.concatenate([np.full(nw, 40.0), rng.uniform(6.0, 10.0, nv),
                            rng.uniform(1.5, 4.0, nf)])
    opacity = np.concatenate([np.full(nw, 0.9), np.full(nv, 0.3), rng.uniform(0.6, 0.95, nf)])
    n = nw + nv + nf
    return bs._splats(W, H, px, py, depth, bs._iso(sigma), opacity, rng.uniform(0, 1, (n, 3)))


def in_gaps(z):
    z = np.asarray(z, np.float64)
    return ((z > GAPS[0][0]) & (z < GAPS[0][1])) | ((z > GAPS[1][0]) & (z < GAPS[1][1]))


def scene_cache(oracle):
    """get(name) -> the scene with its oracle forward (`orc`), built once."""
    cache = {}

    def get(name):
        if name not in cache:
            sc = build(oracle, name)
            bs.run(oracle, sc)
            cache[name] = sc
        return cache[name]
    return get
