"""C feature channels per Gaussian (gsr_forward_features / gsr_backward_features) against what a
caller had to do without them: ceil(C / 3) colors_precomp forwards, and as many backwards, each
repeating the preprocess, the depth sort and the binning (the backward: the rebuild and the whole
blend backward).

Steps, each in a child process under its own time limit (--limit seconds), serial, one context,
timed with HIP events around the calls of one frame:

  forward            one gsr_forward_features call: the colour and the C planes
  forward_plain      one gsr_forward call (the colour alone), for the feature launches' share
  forward_workaround ceil(C / 3) gsr_forward calls with colors_precomp = three feature columns, bg 0
  backward           one gsr_backward_features call under a gradient of the C planes (dL_dcolor NULL)
  backward_workaround ceil(C / 3) gsr_backward calls of those colors_precomp frames
  blend              the "blend" stage (gsr_stage_times) with and without features, and their
                     difference per chunk launch beside the colour blend's own time; and ms[1] of
                     gsr_backward_times with features alone, per chunk launch

One JSON line: the means, min / max, and the two ratios workaround / features.

Usage: python tools/bench_features.py [--config c3] [--features 16] [--steps 30] [--warmup 5]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STEPS = ("forward", "forward_plain", "forward_workaround", "backward", "backward_workaround",
         "blend")


def worker(a):
    import torch

    from bench import Scene
    from gaussiansplattingviewer_amd import _lib
    from gaussiansplattingviewer_amd.rasterizer import (rasterize_gaussians_backward_native,
                                                        rasterize_gaussians_native)
    dev = torch.device("cuda", 0)
    scene = Scene(a.config, dev)
    lib = _lib.load_library()
    ctx = _lib.context(0)
    view, proj, campos, tx, ty, _ = scene.cams[0]
    C, P, H, W = a.features, scene.xyz.shape[0], scene.H, scene.W
    triples = (C + 2) // 3
    feat = torch.randn((P, C), device=dev)
    cols = torch.zeros((P, 3 * triples), device=dev)
    cols[:, :C] = feat
    cols = [cols[:, 3 * j:3 * j + 3].contiguous() for j in range(triples)]
    color = torch.empty((3, H, W), device=dev)
    dLf = torch.randn((C, H, W), device=dev)
    dLc = [torch.randn((3, H, W), device=dev) for _ in range(triples)]
    zero_bg = torch.zeros(3, device=dev)

    def forward(features=None, colors=None):
        return rasterize_gaussians_native(
            zero_bg if colors is not None else scene.bg, scene.xyz, colors, scene.opacity,
            scene.scale, scene.rot, 1.0, None, view, proj, tx, ty, H, W,
            None if colors is not None else scene.sh, scene.deg, campos, False, False,
            out_color=color, features=features)

    def backward(dL=None, colors=None, **kw):
        return rasterize_gaussians_backward_native(
            zero_bg if colors is not None else scene.bg, scene.xyz, colors, scene.opacity,
            scene.scale, scene.rot, 1.0, None, view, proj, tx, ty, dL,
            None if colors is not None else scene.sh, scene.deg, campos, **kw)

    frames = {
        "forward": lambda: forward(features=feat),
        "forward_plain": lambda: forward(),
        "forward_workaround": lambda: [forward(colors=c) for c in cols],
        "backward": lambda: backward(features=feat, dL_dfeature_map=dLf),
        "backward_workaround": lambda: [backward(dL, c) for dL, c in zip(dLc, cols)],
    }
    out = {}
    if a.step != "blend":
        frame = frames[a.step]
        for _ in range(a.warmup):
            frame()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            frame()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[a.step + "_ms"] = round(statistics.fmean(ms), 5)
        out[a.step + "_ms_min_max"] = [round(min(ms), 5), round(max(ms), 5)]
    else:
        names = _lib.stage_names()
        blend = names.index("blend")
        stage = (ctypes.c_float * 16)()
        for key, frame in (("blend_ms_plain", frames["forward_plain"]),
                           ("blend_ms_features", frames["forward"])):
            for _ in range(a.warmup):
                frame()
            _lib.check(lib.gsr_set_timing(ctx, 1), "gsr_set_timing")
            for _ in range(a.steps):
                frame()
            _lib.check(lib.gsr_stage_times(ctx, stage, 16), "gsr_stage_times")
            _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
            out[key] = round(float(stage[blend]), 5)
        fwd_chunks = C // 16 + (1 if C % 16 else 0)
        out["forward_chunk_launches"] = fwd_chunks
        out["blend_ms_per_feature_chunk"] = round(
            (out["blend_ms_features"] - out["blend_ms_plain"]) / fwd_chunks, 5)
        for _ in range(a.warmup):
            frames["backward"]()
        _lib.check(lib.gsr_set_timing(ctx, 1), "gsr_set_timing")
        buf, rows = (ctypes.c_float * 3)(), []
        for _ in range(a.steps):
            frames["backward"]()
            _lib.check(lib.gsr_backward_times(ctx, buf, 3), "gsr_backward_times")
            rows.append([float(buf[i]) for i in range(3)])
        _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
        for i, name in enumerate(("rebuild_ms", "blend_bwd_ms_features_alone",
                                  "preprocess_bwd_ms")):
            out[name] = round(statistics.fmean(r[i] for r in rows), 5)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--features", type=int, default=16, metavar="C")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--limit", type=int, default=120, help="seconds per GPU step")
    ap.add_argument("--step", default=None, choices=STEPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.step:
        return worker(a)
    out = {"config": a.config, "features": a.features, "steps": a.steps,
           "workaround_calls": (a.features + 2) // 3}
    for step in STEPS:  # a fresh process each, under its own time limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", a.config,
                            "--features", str(a.features), "--steps", str(a.steps), "--warmup",
                            str(a.warmup), "--step", step],
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"bench_features: the {step} step failed ({r.returncode}); nothing more is run")
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    out["forward_ratio"] = round(out["forward_workaround_ms"] / out["forward_ms"], 3)
    out["backward_ratio"] = round(out["backward_workaround_ms"] / out["backward_ms"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
