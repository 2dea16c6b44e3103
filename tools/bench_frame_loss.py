"""The frame's loss on a strip (gsr_image_loss_window + its backward) against the two things it
stands between: the strip-alone loss on the same rows (gsr_image_loss on the strip image, what a
rank had before; it pads every seam) and the whole-frame call (what one GPU pays).

One 3 x 1080 x 1920 frame, its 1/8 strip (rank 3 of the equal split of 68 tile rows: 144 rows, a
neighbour on both sides) and its 1/2 strip (rank 0 of 2: 544 rows, a neighbour below).  Serial, on
one stream; after a warm-up the paths alternate, each timed per iteration with HIP events around
`--inner` forward + backward pairs of the C ABI enqueued back to back into buffers allocated
beforehand (kernels and launches; no allocator, no autograd):

  frame_ms          gsr_image_loss + gsr_image_loss_backward on the frame
  alone_ms[strip]   the same pair on the strip image alone
  window_ms[strip]  gsr_image_loss_window + gsr_image_loss_window_backward on the strip's band
  expected[strip]   the ratio of block work, window over alone: the forward's tiles cover the apron
                    (rows + 5 per neighbour), the backward's the own rows
  assemble_ms       the band buffers as frame_loss_on_strip builds them: one concatenation of
                    (above, strip, below) and one contiguous slice of the target
  public_ms         frame_loss_on_strip(...).backward() end to end, with photometric_loss on the
                    strip alone beside it (autograd and the allocator included)

`--baseline-lib PATH` takes frame_ms and alone_ms from another build of libgsr.so (the parent
commit's), loaded beside the tree's; without it they are the tree's own entries, whose kernels
are the parent's.  One JSON line.
Usage: python tools/bench_frame_loss.py [--steps 30] [--warmup 5] [--inner 10] [--baseline-lib P]
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

TILE_H = 16


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--shape", type=int, nargs=3, default=(3, 1080, 1920), metavar=("C", "H", "W"))
    ap.add_argument("--baseline-lib", default=None)
    a = ap.parse_args()

    import torch

    from gaussiansplattingviewer_amd import _lib, frame_loss_on_strip, losses, photometric_loss
    from gaussiansplattingviewer_amd.strips import strip_layout, strip_pixel_rows

    C, H, W = a.shape
    lam = 0.2
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand((C, H, W), device=dev, generator=gen)
    image = (target + 0.05 * torch.randn((C, H, W), device=dev, generator=gen)).clamp(0, 1)
    lib = _lib.load_library()
    base = lib
    if a.baseline_lib:
        base = ctypes.CDLL(a.baseline_lib)
        _lib._declare(base)
    stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)  # noqa: E731

    def frame_pair(x, y):
        """gsr_image_loss + backward of `base` on one image pair, buffers allocated here."""
        c, h, w = x.shape
        inp = _lib.GsrImageLossInputs(c, h, w, lam, x.data_ptr(), y.data_ptr())
        values, saved, grad = f32(3), f32(3, c, h, w), f32(c, h, w)
        ws = torch.empty(base.gsr_image_loss_workspace(c, h, w), dtype=torch.uint8, device=dev)

        def run():
            for _ in range(a.inner):
                assert base.gsr_image_loss(ctypes.byref(inp), values.data_ptr(), saved.data_ptr(),
                                           ws.data_ptr(), stream) == 0
                assert base.gsr_image_loss_backward(ctypes.byref(inp), saved.data_ptr(), None,
                                                    grad.data_ptr(), stream) == 0
        run.keep = (x, y, inp, values, saved, grad, ws)
        return run

    def window_pair(bx, by, row0, own):
        workspace, forward, backward = _lib.image_loss_window_fns(lib)
        c, h, w = bx.shape
        inp = _lib.GsrImageLossInputs(c, h, w, lam, bx.data_ptr(), by.data_ptr())
        win = _lib.GsrLossWindow(H, row0, own[0], own[1])
        a0, a1 = losses.apron_rows(H, own)
        values, saved, grad = f32(3), f32(3, c, a1 - a0, w), f32(c, own[1] - own[0], w)
        ws = torch.empty(workspace(ctypes.byref(inp), ctypes.byref(win)), dtype=torch.uint8,
                         device=dev)

        def run():
            for _ in range(a.inner):
                assert forward(ctypes.byref(inp), ctypes.byref(win), values.data_ptr(),
                               saved.data_ptr(), ws.data_ptr(), stream) == 0
                assert backward(ctypes.byref(inp), ctypes.byref(win), saved.data_ptr(), None,
                                grad.data_ptr(), stream) == 0
        run.keep = (bx, by, inp, win, values, saved, grad, ws)
        return run

    gy = (H + TILE_H - 1) // TILE_H
    strips = {"1/8": strip_layout(gy, 8)[3], "1/2": strip_layout(gy, 2)[0]}
    paths, info, public = {"frame": frame_pair(image, target)}, {}, {}
    for name, tiles in strips.items():
        y0, r = strip_pixel_rows(tiles, H)
        own = (y0, y0 + r)
        up, down = losses.halo_counts(own, H)
        strip = image[:, y0:y0 + r].contiguous()
        tstrip = target[:, y0:y0 + r].contiguous()
        above = image[:, y0 - up:y0].contiguous() if up else None
        below = image[:, y0 + r:y0 + r + down].contiguous() if down else None

        def assemble(strip=strip, above=above, below=below, lo=y0 - up, hi=y0 + r + down):
            for _ in range(a.inner):
                band = torch.cat([t for t in (above, strip, below) if t is not None], dim=1)
                tband = target[:, lo:hi].contiguous()
            return band, tband
        band, tband = assemble()
        paths[f"alone {name}"] = frame_pair(strip, tstrip)
        paths[f"window {name}"] = window_pair(band, tband, y0 - up, own)
        paths[f"assemble {name}"] = assemble
        a0, a1 = losses.apron_rows(H, own)
        tiles_of = lambda rows: (rows + TILE_H - 1) // TILE_H  # noqa: E731
        info[name] = {"rows": r, "halo_rows": [up, down], "band_rows": r + up + down,
                      "expected": round((tiles_of(a1 - a0) + tiles_of(r)) / (2 * tiles_of(r)), 4)}
        leaf = strip.clone().requires_grad_(True)

        def public_window(leaf=leaf, own=own, above=above, below=below):
            for _ in range(a.inner):
                leaf.grad = None
                frame_loss_on_strip(leaf, target, own, above=above, below=below).backward()

        def public_alone(leaf=leaf, tstrip=tstrip):
            for _ in range(a.inner):
                leaf.grad = None
                photometric_loss(leaf, tstrip).backward()
        public[f"public window {name}"] = public_window
        public[f"public alone {name}"] = public_alone
    paths.update(public)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / a.inner

    for _ in range(a.warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize(dev)
    ms = {k: [] for k in paths}
    for _ in range(a.steps):  # alternating
        for k, fn in paths.items():
            ms[k].append(timed(fn))
    stat = {k: {"mean": round(statistics.fmean(v), 5), "min": round(min(v), 5),
                "max": round(max(v), 5)} for k, v in ms.items()}
    out = {"shape": [C, H, W], "steps": a.steps, "warmup": a.warmup, "inner": a.inner,
           "baseline_lib": a.baseline_lib, "ms": stat, "strips": info}
    for name in strips:
        w, al = stat[f"window {name}"]["mean"], stat[f"alone {name}"]["mean"]
        info[name]["window_over_alone"] = round(w / al, 4)
        info[name]["window_over_frame"] = round(w / stat["frame"]["mean"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
