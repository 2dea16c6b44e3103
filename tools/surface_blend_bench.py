"""Blend stage of the forward's forms -- plain, with n_contrib, depth planes (gsr_forward_depth),
median planes (gsr_forward_surface), both -- serial, one context.

Blocks of each kind alternate in one process on one context; each block is timed with
gsr_set_timing(2) (HIP events around the blend on every 8th forward, the mean of the block read
back with gsr_stage_times).  Reports (one JSON line) the mean blend time of each kind over all its
blocks, the spread of the per-block means and every kind's ratio to `plain`.  With GSR_LIB naming
a library from before gsr_forward_surface, pass --kinds plain,contrib (,depth): the same loop on
that build, for the ratio to the parent's blend.

Usage: python tools/surface_blend_bench.py [--config c3] [--blocks 30] [--block-frames 48]
                                           [--kinds plain,contrib,depth,surface,surface_depth]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from bench import CONFIGS, Scene  # noqa: E402
from gaussiansplattingviewer_amd import _lib  # noqa: E402
from gaussiansplattingviewer_amd.rasterizer import rasterize_gaussians_native  # noqa: E402

EXTRAS = {"plain": (), "contrib": ("n_contrib",), "depth": ("depth_map", "inv_depth_map"),
          "surface": ("median_depth", "median_id"),
          "surface_depth": ("depth_map", "inv_depth_map", "median_depth", "median_id")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--blocks", type=int, default=30, help="blocks of each kind")
    ap.add_argument("--block-frames", type=int, default=48, help="forwards per block (8 per sample)")
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--kinds", default=",".join(EXTRAS))
    a = ap.parse_args()
    kinds = a.kinds.split(",")
    dev = torch.device("cuda", 0)
    scene = Scene(a.config, dev)
    lib = _lib.load_library()
    ctx = _lib.context(0)
    names = _lib.stage_names()
    blend = names.index("blend")
    buf = (ctypes.c_float * len(names))()
    view, proj, campos, tx, ty, _ = scene.cams[0]
    # outputs allocated once would be better still; the extras are small beside the frame
    color = torch.empty((3, scene.H, scene.W), device=dev)

    def frame(kind):
        return rasterize_gaussians_native(scene.bg, scene.xyz, None, scene.opacity, scene.scale,
                                          scene.rot, 1.0, None, view, proj, tx, ty, scene.H,
                                          scene.W, scene.sh, scene.deg, campos, False, False,
                                          out_color=color, extras=EXTRAS[kind])

    for i in range(a.warmup):
        frame(kinds[i % len(kinds)])
    torch.cuda.synchronize()
    means = {k: [] for k in kinds}
    for b in range(len(kinds) * a.blocks):
        kind = kinds[b % len(kinds)]
        _lib.check(lib.gsr_set_timing(ctx, 2), "gsr_set_timing")
        for _ in range(a.block_frames):
            frame(kind)
        _lib.check(lib.gsr_stage_times(ctx, buf, len(names)), "gsr_stage_times")
        _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
        means[kind].append(float(buf[blend]))
    out = {"config": a.config, "library": os.path.relpath(_lib.LIB_PATH, REPO),
           "frames_each": a.blocks * a.block_frames,
           "timed_samples_each": a.blocks * ((a.block_frames + 7) // 8)}
    for kind, v in means.items():
        out[f"blend_ms_{kind}"] = round(statistics.fmean(v), 5)
        out[f"blend_ms_{kind}_block_min_max"] = [round(min(v), 5), round(max(v), 5)]
    for kind in kinds[1:]:
        out[f"{kind}_over_{kinds[0]}"] = round(out[f"blend_ms_{kind}"] / out[f"blend_ms_{kinds[0]}"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
