"""The nearest-neighbour search in HIP (gsr_knn_mean_dist2) against what a caller had
to write without it -- a chunked torch.cdist + topk(4, largest=False) -- on the same GPU in the same
process.

For every N (default 100k and 1M) and scene (uniform: U(0, 1)^3; clustered: 64 Gaussian clusters of
sigma 0.02 in [0, 4]^3), serial, after a warm-up, the paths alternating in one process:

  knn     device events around gsr_knn_stages(n) for n = 1..4, each `--steps` times; stage k is the
          mean of prefix k minus the mean of prefix k - 1 (1 bounds + codes, 2 sort, 3 gather +
          boxes, 4 search); total = prefix 4, which is gsr_knn_mean_dist2 itself.
          boxes_scanned: the mean and the largest number of boxes a block of the search scanned,
          out of ceil(N / 256), from the words the call leaves at the head of its workspace.
  torch   device events around the loop over chunks of rows: cdist(chunk, all), topk(4,
          largest=False), the mean of the squares of columns 1..3.  `--torch-steps` iterations
          (default: `--steps` up to N = 200k, 2 above: a call at 1M takes seconds).
          rel_diff_median: the median relative difference of its result from the search's (cdist
          takes the matrix-product route, which is not exact; the search is).

One JSON line per (N, scene, path).  Usage: python tools/bench_knn.py [--N 100000 1000000]
[--steps 30] [--warmup 3] [--torch-steps K]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

STAGES = ("bounds_codes", "sort", "gather_boxes", "search")


def make_scene(torch, kind, N, dev):
    gen = torch.Generator(device=dev).manual_seed(7)
    if kind == "uniform":
        return torch.rand((N, 3), device=dev, generator=gen)
    centres = torch.rand((64, 3), device=dev, generator=gen) * 4.0
    which = torch.randint(0, 64, (N,), device=dev, generator=gen)
    return (centres[which] + 0.02 * torch.randn((N, 3), device=dev, generator=gen)).contiguous()


def torch_route(torch, xyz, chunk):
    out = torch.empty(xyz.shape[0], device=xyz.device)
    for s in range(0, xyz.shape[0], chunk):
        d = torch.cdist(xyz[s:s + chunk], xyz)
        near = d.topk(4, dim=1, largest=False).values[:, 1:]
        out[s:s + chunk] = (near * near).mean(1)
    return out


def summary(xs):
    return dict(mean=round(statistics.mean(xs), 5), median=round(statistics.median(xs), 5),
                min_max=[round(min(xs), 5), round(max(xs), 5)])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[100_000, 1_000_000])
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-steps", type=int, default=None)
    a = ap.parse_args()

    import torch

    from gaussiansplattingviewer_amd import pointcloud

    dev = torch.device("cuda", 0)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn):
        ev[0].record()
        out = fn()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1]), out

    for N in a.N:
        nb = (N + 255) // 256
        chunk = 4096 if N <= 200_000 else 1024
        torch_steps = a.torch_steps if a.torch_steps is not None else \
            (a.steps if N <= 200_000 else 2)
        for kind in ("uniform", "clustered"):
            xyz = make_scene(torch, kind, N, dev)
            dist2 = torch.empty(N, device=dev)
            ws = torch.empty(pointcloud.workspace_bytes(N), dtype=torch.uint8, device=dev)
            prefix = {n: [] for n in range(1, 5)}
            plain, ref = [], None
            for it in range(a.warmup + a.steps):
                for n in range(1, 5):
                    ms, _ = timed(lambda: pointcloud.knn_stages(xyz, dist2, ws, n))
                    if it >= a.warmup:
                        prefix[n].append(ms)
                # the torch route: once untimed, then in the last torch_steps iterations
                first = max(a.warmup + a.steps - torch_steps, 1)
                if it == 0 or it >= first:
                    ms, ref = timed(lambda: torch_route(torch, xyz, chunk))
                    if it >= first:
                        plain.append(ms)
            scanned = ws[:4 * nb].view(torch.int32).float()
            means = [statistics.mean(prefix[n]) for n in range(1, 5)]
            line = dict(path="knn", N=N, scene=kind, steps=a.steps, total_ms=summary(prefix[4]),
                        stage_ms={k: round(means[i] - (means[i - 1] if i else 0.0), 5)
                                  for i, k in enumerate(STAGES)},
                        boxes=nb, boxes_scanned_mean=round(float(scanned.mean()), 2),
                        boxes_scanned_max=int(scanned.max()),
                        workspace_mb=round(ws.numel() / 1e6, 2))
            print(json.dumps(line), flush=True)
            rel = ((ref - dist2).abs() / dist2.clamp_min(1e-30)).median()
            line = dict(path="torch", N=N, scene=kind, steps=len(plain), chunk_rows=chunk,
                        total_ms=summary(plain), rel_diff_median=float(f"{float(rel):.3g}"),
                        ratio_to_knn=round(statistics.mean(plain) / means[3], 1))
            print(json.dumps(line), flush=True)
            del xyz, dist2, ws, ref


if __name__ == "__main__":
    main()
