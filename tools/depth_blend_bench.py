"""Blend stage of a plain forward against a depth forward (gsr_forward_depth), serial, one context.

Blocks of plain and of depth forwards alternate in one process on one context; each block is
timed with gsr_set_timing(2) (HIP events around the blend on every 8th forward, the mean of the
block read back with gsr_stage_times).  Reports (one JSON line) the mean blend time of each kind
over all its blocks, their ratio, and the spread of the per-block means.

Usage: python tools/depth_blend_bench.py [--config c3] [--blocks 50] [--block-frames 48]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3", choices=sorted(CONFIGS))
    ap.add_argument("--blocks", type=int, default=50, help="blocks of each kind")
    ap.add_argument("--block-frames", type=int, default=48, help="forwards per block (8 per sample)")
    ap.add_argument("--warmup", type=int, default=200)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    scene = Scene(a.config, dev)
    lib = _lib.load_library()
    ctx = _lib.context(0)
    names = _lib.stage_names()
    blend = names.index("blend")
    buf = (ctypes.c_float * len(names))()
    view, proj, campos, tx, ty, _ = scene.cams[0]
    # outputs allocated once: the loop times kernels, not the allocator
    color = torch.empty((3, scene.H, scene.W), device=dev)
    extras = {"plain": (), "depth": ("depth_map", "inv_depth_map")}

    def frame(kind):
        return rasterize_gaussians_native(scene.bg, scene.xyz, None, scene.opacity, scene.scale,
                                          scene.rot, 1.0, None, view, proj, tx, ty, scene.H,
                                          scene.W, scene.sh, scene.deg, campos, False, False,
                                          out_color=color, extras=extras[kind])

    for i in range(a.warmup):
        frame("depth" if i % 2 else "plain")
    torch.cuda.synchronize()
    means = {"plain": [], "depth": []}
    for b in range(2 * a.blocks):
        kind = "depth" if b % 2 else "plain"
        _lib.check(lib.gsr_set_timing(ctx, 2), "gsr_set_timing")
        for _ in range(a.block_frames):
            frame(kind)
        _lib.check(lib.gsr_stage_times(ctx, buf, len(names)), "gsr_stage_times")
        _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
        means[kind].append(float(buf[blend]))
    out = {"config": a.config, "frames_each": a.blocks * a.block_frames,
           "timed_samples_each": a.blocks * ((a.block_frames + 7) // 8)}
    for kind, v in means.items():
        out[f"blend_ms_{kind}"] = round(statistics.fmean(v), 5)
        out[f"blend_ms_{kind}_block_min_max"] = [round(min(v), 5), round(max(v), 5)]
    out["depth_over_plain"] = round(out["blend_ms_depth"] / out["blend_ms_plain"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
