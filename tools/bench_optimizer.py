"""The fused sparse Adam step (gsr_adam_step: one launch for all parameter tensors) against what a
user has without it, on the same GPU in the same process.

P Gaussians (default 1M, config C3's) with the six 3DGS tensors: xyz 3, f_dc 3, f_rest 45,
opacity 1, scaling 3, rotation 4 floats per Gaussian.  Serial; after a warm-up the paths
alternate, one step each per iteration, each timed with HIP events around its own calls:

  dense     fused           gsr_adam_step without a mask (the float4 path)
            torch_adam      torch.optim.Adam, default (foreach)
            torch_fused     torch.optim.Adam(fused=True)
  masked    fused           gsr_adam_step with a bool mask, for visible fractions 1.0, 0.5, 0.1,
                            each as a random mask and as one contiguous run of rows
            fused_radii     the same with the int32 radii as the mask
            torch_masked    the masked step written in torch ops (index the visible rows, update
                            them, index_copy_ them back), which is what the sparse rule costs today

and per path the byte floor from shapes, visible rows x 59 floats x 28 B (param, grad, m, v read;
param, m, v written) + P mask bytes, and `floor_share`: the floor's time at 6.3 TB/s (the rate a
float4 copy reaches on this GPU) over the measured time.

One JSON line per path.  Usage: python tools/bench_optimizer.py [--P 1000000] [--steps 30]
[--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COPY_BYTES_PER_S = 6.3e12
MS = (3, 3, 45, 1, 3, 4)
LRS = (1.6e-4, 2.5e-3, 1.25e-4, 0.05, 5e-3, 1e-3)
BETAS = (0.9, 0.999)
EPS = 1e-15


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--P", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()

    import torch

    from gaussiansplattingviewer_amd import optim

    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev).manual_seed(0)
    P = a.P

    def state():
        return dict(p=[torch.randn((P, M), device=dev, generator=gen) for M in MS],
                    g=[1e-3 * torch.randn((P, M), device=dev, generator=gen) for M in MS],
                    m=[torch.zeros((P, M), device=dev) for M in MS],
                    v=[torch.zeros((P, M), device=dev) for M in MS])

    ours = state()

    def fused(mask):
        optim.adam_step_native(ours["p"], ours["g"], ours["m"], ours["v"], LRS, [EPS] * 6, mask,
                               *BETAS)

    def torch_opt(**kw):
        s = state()
        params = [torch.nn.Parameter(p) for p in s["p"]]
        for p, g in zip(params, s["g"]):
            p.grad = g
        opt = torch.optim.Adam([{"params": [p], "lr": lr} for p, lr in zip(params, LRS)],
                               eps=EPS, betas=BETAS, **kw)
        return opt.step

    theirs = state()

    def torch_masked(mask):
        idx = mask.nonzero(as_tuple=True)[0]
        for p, g, m, v, lr in zip(theirs["p"], theirs["g"], theirs["m"], theirs["v"], LRS):
            gi = g[idx]
            mi = m[idx].mul_(BETAS[0]).add_(gi, alpha=1.0 - BETAS[0])
            vi = v[idx].mul_(BETAS[1]).addcmul_(gi, gi, value=1.0 - BETAS[1])
            m.index_copy_(0, idx, mi)
            v.index_copy_(0, idx, vi)
            p.index_add_(0, idx, mi / vi.sqrt().add_(EPS), alpha=-lr)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def run(title, paths, visible_rows, mask_bytes):
        """paths: name -> callable; alternating, `steps` timed iterations after the warm-up."""
        for _ in range(a.warmup):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize(dev)
        ms = {k: [] for k in paths}
        for _ in range(a.steps):
            for k, fn in paths.items():
                ms[k].append(timed(fn))
        floor = visible_rows * sum(MS) * 28 + mask_bytes
        floor_ms = floor / COPY_BYTES_PER_S * 1e3
        for k, v in ms.items():
            mean = statistics.fmean(v)
            print(json.dumps({"case": title, "path": k, "P": P, "steps": a.steps,
                              "ms": round(mean, 5), "ms_median": round(statistics.median(v), 5),
                              "ms_min_max": [round(min(v), 5), round(max(v), 5)],
                              "byte_floor_mb": round(floor / 1e6, 2),
                              "byte_floor_ms": round(floor_ms, 5),
                              "floor_share_of_6.3TBps": round(floor_ms / mean, 4)}), flush=True)

    run("dense", {"fused": lambda: fused(None), "torch_adam": torch_opt(),
                  "torch_fused": torch_opt(fused=True)}, P, 0)
    for frac in (1.0, 0.5, 0.1):
        n = int(round(frac * P))
        masks = {"random": torch.rand(P, device=dev, generator=gen) < frac if frac < 1.0
                 else torch.ones(P, dtype=torch.bool, device=dev),
                 "contiguous": torch.arange(P, device=dev) < n}
        for kind, mask in masks.items():
            radii = mask.to(torch.int32) * 7
            rows = int(mask.sum())
            run(f"masked {frac} {kind}",
                {"fused": lambda: fused(mask), "fused_radii": lambda: fused(radii),
                 "torch_masked": lambda: torch_masked(mask)}, rows, P)


if __name__ == "__main__":
    main()
