"""The fused L1 + D-SSIM loss (photometric_loss: gsr_image_loss + gsr_image_loss_backward) against
what a user had to write without it: the torch restatement of tests/loss_reference.py (conv2d,
groups = C, float32, autograd's backward), on the same GPU in the same process.

One 3 x 1080 x 1920 image, serial.  After a warm-up the two paths alternate, one forward +
backward each per iteration, each timed with HIP events around its own calls:

  fused_ms     photometric_loss(image, target).backward()
  torch_ms     loss_values(image, target, 0.2)[0].backward() of the restatement
  kernels_ms   the fused pair's kernels alone: the C ABI's forward + backward enqueued `steps`
               times back to back between two events (no Python between the launches' work)

and the byte floor: per element the forward reads 8 B and writes 12 B, the backward reads 20 B
and writes 4 B, 44 N bytes at the HBM rate DESIGN.md's rooflines use (8 TB/s).

One JSON line.  Usage: python tools/bench_loss.py [--steps 30] [--warmup 5] [--shape 3 1080 1920]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "tests")):
    sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shape", type=int, nargs=3, default=(3, 1080, 1920), metavar=("C", "H", "W"))
    a = ap.parse_args()

    import torch

    import loss_reference as L
    from gaussiansplattingviewer_amd import losses, photometric_loss

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    target = torch.rand(tuple(a.shape), device=dev, generator=gen)
    image = (target + 0.05 * torch.randn(tuple(a.shape), device=dev, generator=gen)).clamp(0, 1)
    image.requires_grad_(True)

    def fused():
        image.grad = None
        loss = photometric_loss(image, target)
        loss.backward()
        return loss

    def restated():
        image.grad = None
        loss = L.loss_values(image, target, 0.2)[0]
        loss.backward()
        return loss

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        fused()
        restated()
    torch.cuda.synchronize(dev)
    ms = {"fused": [], "torch": []}
    for _ in range(a.steps):  # alternating
        ms["fused"].append(timed(fused))
        ms["torch"].append(timed(restated))
    lf, gf = fused().item(), image.grad.clone()
    lt, gt = restated().item(), image.grad.clone()

    # the kernels alone: the C ABI's pair, back to back
    x = image.detach()
    values, saved = losses.image_loss_native(x, target, 0.2, True)

    def pairs():
        for _ in range(a.steps):
            losses.image_loss_native(x, target, 0.2, True)
            losses.image_loss_backward_native(x, target, 0.2, saved)
    pairs()
    torch.cuda.synchronize(dev)
    kernels_ms = timed(pairs) / a.steps

    n = x.numel()
    floor_ms = 44.0 * n / HBM_BYTES_PER_S * 1e3
    mean = {k: statistics.fmean(v) for k, v in ms.items()}
    out = {
        "shape": list(a.shape), "steps": a.steps, "warmup": a.warmup,
        "fused_ms": round(mean["fused"], 5),
        "fused_ms_min_max": [round(min(ms["fused"]), 5), round(max(ms["fused"]), 5)],
        "torch_ms": round(mean["torch"], 5),
        "torch_ms_min_max": [round(min(ms["torch"]), 5), round(max(ms["torch"]), 5)],
        "torch_over_fused": round(mean["torch"] / mean["fused"], 3),
        "kernels_ms": round(kernels_ms, 5),
        "byte_floor_mb": round(44.0 * n / 1e6, 1), "byte_floor_ms": round(floor_ms, 5),
        "floor_fraction_fused": round(floor_ms / mean["fused"], 4),
        "floor_fraction_kernels": round(floor_ms / kernels_ms, 4),
        "loss_fused": lf, "loss_torch": lt,
        "grad_max_abs_diff": float((gf - gt).abs().max()),
        "grad_max_abs": float(gt.abs().max()),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
