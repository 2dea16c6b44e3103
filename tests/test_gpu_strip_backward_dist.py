"""GPU, two ranks on one device (gloo carries the GPU tensors; RCCL refuses two ranks on one
GPU): multi-GPU fitting end to end on frame_grad_scenes' `frame` with the balanced two-strip
layout.  Each rank renders its strip through GaussianRasterizer(tile_rows=, deterministic=True),
runs backward() on its strip's loss, then strips.reduce_gradients.  Rank 0 also computes both strips
alone and adds them with torch: the reduced gradients equal that sum bit for bit (a two-term float
sum is commutative, so no tolerance is needed)."""
import os
import socket
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_path):
    import numpy as np
    import torch
    import torch.distributed as dist
    for p in (REPO, os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import frame_grad_scenes as fs
    from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                        GaussianRasterizer, tile_row_pairs)
    from gaussiansplattingviewer_amd.strips import (balanced_layout, reduce_gradients,
                                                    strip_pixel_rows)
    from gpu_helpers import run_hip, to_dev
    from test_gpu_backward import _inputs
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sc = fs.get("frame")
        s, H, W = sc["s"], sc["H"], sc["W"]
        gy, gx = (H + 15) // 16, (W + 15) // 16
        # the balanced layout: the whole frame's pair counts per tile row plus StripBalancer's
        # per-tile constant (every rank computes the same split)
        run_hip(s, dev, binning=False)
        costs = tile_row_pairs(gy).cpu().numpy().view(np.uint32).astype(np.int64) + 64 * gx
        layout = balanced_layout(costs, world)

        def strip_grads(strip):
            d = _inputs(sc, dev)
            for v in d.values():
                if v is not None:
                    v.requires_grad_(True)
            leaves = dict(d, means2D=torch.zeros_like(d["means3D"], requires_grad=True),
                          view=to_dev(s["view"], dev).requires_grad_(True))
            rs = GaussianRasterizationSettings(
                H, W, s["tx"], s["ty"], to_dev(s["bg"], dev), s["scale_modifier"], leaves["view"],
                to_dev(s["proj"], dev), s["sh_degree"], to_dev(s["campos"], dev), False, False,
                tile_rows=strip, deterministic=True)
            color, _ = GaussianRasterizer(rs)(means2D=leaves["means2D"], **d)
            y0, rows = strip_pixel_rows(strip, H)
            assert color.shape == (3, rows, W)
            (color * to_dev(np.ascontiguousarray(sc["dL"][:, y0:y0 + rows]), dev)).sum().backward()
            return {k: t.grad for k, t in leaves.items() if t is not None}

        mine = strip_grads(layout[rank])
        reduce_gradients(mine.values())
        torch.cuda.synchronize()
        if rank == 0:
            a, b = strip_grads(layout[0]), strip_grads(layout[1])
            ok = [bool(torch.equal((a[k] + b[k]).view(torch.int32), mine[k].view(torch.int32)))
                  for k in sorted(mine)]
            moved = [bool((a[k] != 0).any() and (b[k] != 0).any()) for k in sorted(mine)]
            np.save(out_path, np.array([len(mine), layout[0][1]] + ok + moved, dtype=np.int64))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_rank_strip_gradients_reduce_to_the_sum(tmp_path, gpu):
    import numpy as np
    import torch.multiprocessing as mp
    out = str(tmp_path / "ok.npy")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True,
                       start_method="spawn")
    res = np.load(out)
    n, cut = int(res[0]), int(res[1])
    assert n == 7 and 0 < cut < 9 and len(res) == 2 + 2 * n
    assert res[2:].all(), res
