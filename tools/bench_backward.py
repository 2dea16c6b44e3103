"""The backward pass (gsr_backward) of a benchmark config beside its forward, serial, one context.

Times with HIP events: the forward of the frame (torch events around gsr_forward), and the three
stages of gsr_backward as the library records them under gsr_set_timing (gsr_backward_times): the
rebuild of the per-Gaussian stage, the depth sort and upstream's lists; the blend's backward
(k_blend_bwd_q, with the zeroing of its sums); the per-Gaussian backward (k_preprocess_bwd).
Reports (one JSON line) their means and spreads, and the blend backward's atomic traffic against
the chip-wide float atomic rate: 36 B per (splat, quadrant wave) contribution, the contributions
per frame taken from --contributions (they are not counted on the device; the default is C3's,
from the forward's ~118 composited splats per quadrant wave, blend.hip), so the byte figure is an
upper estimate: a staged splat no pixel of the quadrant composites adds nothing.

--planes: the backward is gsr_backward_planes with the gradients of depth_map, inv_depth_map and
final_T beside the image's (k_blend_bwd_planes_q, k_preprocess_bwd_planes: ten sums, 40 B per
contribution); the forward timed is then gsr_forward_depth with final_T, the frame that backward
belongs to.

--camera: the backward is gsr_backward_camera, which also returns the gradients of viewmatrix,
projmatrix and campos (k_preprocess_bwd_camera / k_preprocess_bwd_planes_camera and
k_camera_finish, inside the third stage); with or without --planes.

--antialiasing: forward and backward with the antialiasing option (gsr_forward_filtered,
gsr_backward_filtered: k_preprocess_aa and the k_preprocess_bwd*_aa kernels); with or without
--planes and --camera.  The forward step also reports preprocess_ms, the per-Gaussian stage of
the forward as gsr_stage_times gives it, with and without the option.

--deterministic: the backward is gsr_backward_ordered in its deterministic mode
(k_blend_bwd_det_q / k_blend_bwd_planes_det_q store to slots, k_grad_rows_gather fills the rows;
the slab scan, the zeroing of the marks and the gather are inside blend_bwd_ms); with or without
--planes, --camera and --antialiasing.  The atomic figures are then not reported: the mode has no
float atomics.

--strip r/N: forward and backward on strip r of the equal split of the tile rows into N
(strips.strip_rows): the strip forward, and gsr_backward_strip under strip-local gradients; with
any of the options above.  Also reports the strip's tile rows and, with --deterministic, the
slots' and marks' workspace for the strip's num_rendered (det_workspace_MB).  The atomic figures
are not reported for a strip (--contributions is the whole frame's).

--features C: forward and backward with C feature channels per Gaussian beside the colour
(gsr_forward_features, gsr_backward_features: the k_blend_features_q launches inside the forward,
the k_blend_bwd_features_q launches inside blend_bwd_ms); with --planes, --camera, --antialiasing
and --strip, not with --deterministic.  The atomic figures are not reported (--contributions counts
the colour pass's).  tools/bench_features.py compares the pair with what a caller had to do before.

--absgrad: the backward is gsr_backward_abs, which also returns dL_dmeans2D_abs (the
k_blend_bwd*_abs_q instantiations: two more sums per (splat, quadrant), 8 B more per contribution,
inside blend_bwd_ms; k_means2d_abs inside preprocess_bwd_ms); with --planes, --camera,
--antialiasing, --deterministic and --strip, not with --features (the library refuses the pair).
With --deterministic the slots hold two more words (det_workspace_MB).

Each GPU step runs in a child process under its own time limit (--limit seconds).

Usage: python tools/bench_backward.py [--config c3] [--steps 50] [--warmup 10] [--planes]
                                      [--camera] [--antialiasing] [--deterministic]
                                      [--strip r/N] [--features C] [--absgrad]
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

ATOMIC_RATE_GBS = 1300.0  # chip-wide float atomic adds, bytes added per second (MI355X)
BYTES_PER_CONTRIBUTION = 36  # nine float sums per (splat, quadrant wave)


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
    n_rows, fwd_strip, bwd_strip = scene.H, {}, {}
    if a.strip:
        from gaussiansplattingviewer_amd.strips import strip_pixel_rows, strip_rows
        r, n = (int(v) for v in a.strip.split("/"))
        tile_rows = strip_rows((scene.H + 15) // 16, n, r)
        n_rows = strip_pixel_rows(tile_rows, scene.H)[1]
        fwd_strip = {"tile_rows": tile_rows}
        bwd_strip = {"tile_rows": tile_rows, "image_height": scene.H}
    color = torch.empty((3, n_rows, scene.W), device=dev)
    dL = torch.randn((3, n_rows, scene.W), device=dev)
    extras, plane_grads = (), {}
    aa = {"antialiasing": True} if a.antialiasing else {}
    if a.planes:
        extras = ("depth_map", "inv_depth_map", "final_T")
        plane_grads = {f"dL_d{n}": torch.randn((n_rows, scene.W), device=dev) for n in extras}

    feat = {}
    if a.features:
        feat = {"features": torch.randn((scene.xyz.shape[0], a.features), device=dev)}
        bwd_strip = dict(bwd_strip, **feat, dL_dfeature_map=torch.randn(
            (a.features, n_rows, scene.W), device=dev))

    def forward():
        return rasterize_gaussians_native(scene.bg, scene.xyz, None, scene.opacity, scene.scale,
                                          scene.rot, 1.0, None, view, proj, tx, ty, scene.H,
                                          scene.W, scene.sh, scene.deg, campos, False, False,
                                          out_color=color, extras=extras, **aa, **fwd_strip,
                                          **feat)

    def backward():
        return rasterize_gaussians_backward_native(scene.bg, scene.xyz, None, scene.opacity,
                                                   scene.scale, scene.rot, 1.0, None, view, proj,
                                                   tx, ty, dL, scene.sh, scene.deg, campos,
                                                   camera=bool(a.camera),
                                                   deterministic=bool(a.deterministic),
                                                   absgrad=bool(a.absgrad),
                                                   **plane_grads, **aa, **bwd_strip)

    out = {"config": a.config, "steps": a.steps, "planes": bool(a.planes),
           "camera": bool(a.camera), "antialiasing": bool(a.antialiasing),
           "deterministic": bool(a.deterministic), "features": a.features,
           "absgrad": bool(a.absgrad)}
    if a.strip:
        out.update(strip=a.strip, tile_rows=list(fwd_strip["tile_rows"]), rows=n_rows)
    if a.step == "forward":
        for _ in range(a.warmup):
            forward()
        ms = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            res = forward()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out.update(forward_ms=round(statistics.fmean(ms), 5),
                   forward_ms_min_max=[round(min(ms), 5), round(max(ms), 5)],
                   num_rendered=res.num_rendered)
        if a.deterministic:  # 4 slots of 9 (10; --absgrad: 2 more) floats, 4 marks per list entry
            sums = (10 if a.planes else 9) + (2 if a.absgrad else 0)
            out.update(det_workspace_MB=round(res.num_rendered * (4 * 4 * sums + 4) / 1e6, 2))
        # the per-Gaussian stage of the forward: the library's own stage events, the mean over
        # these frames
        _lib.check(lib.gsr_set_timing(ctx, 1), "gsr_set_timing")
        for _ in range(a.steps):
            forward()
        stage = (ctypes.c_float * 8)()
        _lib.check(lib.gsr_stage_times(ctx, stage, 8), "gsr_stage_times")
        _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
        out.update(preprocess_ms=round(float(stage[0]), 5))
    else:
        for _ in range(a.warmup):
            backward()
        _lib.check(lib.gsr_set_timing(ctx, 1), "gsr_set_timing")
        buf = (ctypes.c_float * 3)()
        rows = []
        for _ in range(a.steps):
            backward()
            _lib.check(lib.gsr_backward_times(ctx, buf, 3), "gsr_backward_times")
            rows.append([float(buf[i]) for i in range(3)])
        _lib.check(lib.gsr_set_timing(ctx, 0), "gsr_set_timing")
        for i, name in enumerate(("rebuild_ms", "blend_bwd_ms", "preprocess_bwd_ms")):
            v = [r[i] for r in rows]
            out[name] = round(statistics.fmean(v), 5)
            out[name + "_min_max"] = [round(min(v), 5), round(max(v), 5)]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--limit", type=int, default=240, help="seconds per GPU step")
    ap.add_argument("--contributions", type=float, default=3.9e6,
                    help="(splat, quadrant) contributions per frame (C3: ~118 composited splats "
                         "per quadrant wave, blend.hip)")
    ap.add_argument("--planes", action="store_true",
                    help="gsr_backward_planes: colour plus the three planes' gradients")
    ap.add_argument("--camera", action="store_true",
                    help="gsr_backward_camera: also the gradients of the camera")
    ap.add_argument("--antialiasing", action="store_true",
                    help="gsr_forward_filtered / gsr_backward_filtered with antialiasing = 1")
    ap.add_argument("--deterministic", action="store_true",
                    help="gsr_backward_ordered with deterministic = 1: bit-reproducible gradients")
    ap.add_argument("--strip", default=None, metavar="r/N",
                    help="strip r of the equal split of the tile rows into N: the strip forward "
                         "and gsr_backward_strip")
    ap.add_argument("--features", type=int, default=0, metavar="C",
                    help="C feature channels per Gaussian beside the colour, forward and backward")
    ap.add_argument("--absgrad", action="store_true",
                    help="gsr_backward_abs: also dL_dmeans2D_abs, the absolute means2D gradient")
    ap.add_argument("--step", default=None, choices=["forward", "backward"], help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.absgrad and a.features:
        sys.exit("bench_backward: --absgrad and --features exclude each other (gsr_backward_abs)")
    if a.step:
        return worker(a)
    out = {}
    for step in ("forward", "backward"):  # a fresh process each, under its own time limit
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--config", a.config,
                            "--steps", str(a.steps), "--warmup", str(a.warmup), "--step", step] +
                           (["--planes"] if a.planes else []) +
                           (["--camera"] if a.camera else []) +
                           (["--antialiasing"] if a.antialiasing else []) +
                           (["--deterministic"] if a.deterministic else []) +
                           (["--strip", a.strip] if a.strip else []) +
                           (["--features", str(a.features)] if a.features else []) +
                           (["--absgrad"] if a.absgrad else []),
                           capture_output=True, text=True, timeout=a.limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit(f"bench_backward: the {step} step failed ({r.returncode}); nothing more is run")
        out.update(json.loads(r.stdout.strip().splitlines()[-1]))
    if a.deterministic or a.strip or a.features:  # no colour-pass atomic traffic to report
        print(json.dumps(out))
        return
    atomic_bytes = a.contributions * (BYTES_PER_CONTRIBUTION + (4 if a.planes else 0) +
                                      (8 if a.absgrad else 0))
    out["atomic_MB_per_frame_upper"] = round(atomic_bytes / 1e6, 1)
    out["atomic_GBs_if_all_added"] = round(atomic_bytes / (out["blend_bwd_ms"] * 1e-3) / 1e9, 1)
    out["atomic_rate_share"] = round(out["atomic_GBs_if_all_added"] / ATOMIC_RATE_GBS, 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
