"""GPU, two ranks on one device (gloo carries the GPU tensors; RCCL refuses two ranks on one
GPU): the frame's loss fitted on strips, end to end, on frame_grad_scenes' `frame` with the
balanced two-strip layout.  Each rank renders its strip through
GaussianRasterizer(tile_rows=, deterministic=True), calls strips.exchange_halo and
losses.frame_loss_on_strip, runs backward(), then strips.reduce_gradients.  Rank 0 also computes
both strips alone, with halos sliced from its own renders:

   - the halos a rank receives are, bit for bit, the neighbour's rows as rank 0 renders them;
   - the reduced gradients are, bit for bit, the sum rank 0 forms of the two strips' (a two-term
     float sum is commutative, so no tolerance is needed);
   - the two shares add up to the one-process frame loss within the shares' bound of
     test_gpu_frame_loss_strips.py: (8 x loss_reference.F32_SPREAD + R 2^-24) |value|, R = 2.
"""
import os
import socket
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAM = 0.2


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
    from gaussiansplattingviewer_amd import frame_loss_on_strip, photometric_loss
    from gaussiansplattingviewer_amd.losses import halo_counts
    from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                        GaussianRasterizer, tile_row_pairs)
    from gaussiansplattingviewer_amd.strips import (balanced_layout, exchange_halo,
                                                    reduce_gradients, strip_pixel_rows)
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
        run_hip(s, dev, binning=False)
        costs = tile_row_pairs(gy).cpu().numpy().view(np.uint32).astype(np.int64) + 64 * gx
        layout = balanced_layout(costs, world)
        target = to_dev(np.random.default_rng(11).uniform(0, 1, (3, H, W)).astype(np.float32),
                        dev)

        def render(strip):
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
            return leaves, color

        def fit(strip, halos):
            """-> (share, gradients, the strip's render, the halos used)."""
            leaves, color = render(strip)
            y0, rows = strip_pixel_rows(strip, H)
            assert color.shape == (3, rows, W)
            above, below = halos(color.detach(), (y0, y0 + rows))
            share = frame_loss_on_strip(color, target, (y0, y0 + rows), above=above, below=below,
                                        lambda_dssim=LAM)
            share.backward()
            return (share.detach(), {k: t.grad for k, t in leaves.items() if t is not None},
                    color.detach(), (above, below))

        share, mine, _, got = fit(layout[rank],
                                  lambda strip, rows: exchange_halo(strip, layout, H, rank))
        reduce_gradients(mine.values())
        shares = torch.stack([share, share])
        shares[1 - rank] = 0.0
        reduce_gradients([shares])
        torch.cuda.synchronize()
        # the other rank's halos, for rank 0 to compare: (above, below) of rank 1
        if rank == 1:
            for t in got:
                if t is not None:
                    dist.send(t.cpu(), 0)
        if rank == 0:
            renders = [render(layout[r])[1].detach() for r in range(world)]
            whole = torch.cat(renders, dim=1)

            def sliced(strip, rows):
                a, b = halo_counts(rows, H)
                return (whole[:, rows[0] - a:rows[0]] if a else None,
                        whole[:, rows[1]:rows[1] + b] if b else None)

            alone = [fit(layout[r], sliced) for r in range(world)]
            halos1 = []
            for want in alone[1][3]:  # halo_plan gives rank 1 a halo exactly where one exists
                t = None if want is None else torch.zeros(tuple(want.shape))
                if t is not None:
                    dist.recv(t, 1)
                halos1.append(None if t is None else t.to(dev))
            same = lambda a, b: bool(a.shape == b.shape and  # noqa: E731
                                     torch.equal(a.view(torch.int32), b.view(torch.int32)))
            empty = torch.zeros((3, 0, W), device=dev)
            halo_ok = [same(g if g is not None else empty, w if w is not None else empty)
                       for g, w in list(zip(got, alone[0][3])) + list(zip(halos1, alone[1][3]))]
            halo_rows = [0 if w is None else w.shape[1] for r in range(world) for w in alone[r][3]]
            ok = [same(alone[0][1][k] + alone[1][1][k], mine[k]) for k in sorted(mine)]
            moved = [bool((alone[0][1][k] != 0).any() and (alone[1][1][k] != 0).any())
                     for k in sorted(mine)]
            frame_loss = photometric_loss(whole, target, LAM)
            np.save(out_path, np.array(
                [len(mine), layout[0][1]] + halo_rows + halo_ok + ok + moved, dtype=np.int64))
            np.save(out_path + ".loss.npy", np.array(
                [float(shares[0]), float(shares[1]), float(frame_loss),
                 float(alone[0][0]), float(alone[1][0])], dtype=np.float64))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_fit_the_frames_loss(tmp_path, gpu):
    import numpy as np
    import torch.multiprocessing as mp

    import loss_reference as L
    out = str(tmp_path / "ok.npy")
    mp.start_processes(_worker, args=(2, _free_port(), out), nprocs=2, join=True,
                       start_method="spawn")
    res = np.load(out)
    n, cut = int(res[0]), int(res[1])
    assert n == 7 and 0 < cut < 9 and len(res) == 2 + 4 + 4 + 2 * n
    # rank 0 has no rows above, rank 1 none below, and the seam's halos are whole
    assert list(res[2:6]) == [0, min(10, 136 - 16 * cut), 10, 0]
    assert res[6:].all(), res
    s0, s1, frame, a0, a1 = np.load(out + ".loss.npy")
    assert (s0, s1) == (a0, a1)  # a share has the bits of the strip computed alone
    e = abs((s0 + s1) - frame)
    bound = (L.BOUND_FACTOR * L.F32_SPREAD["loss"][LAM] + 2 * 2.0 ** -24) * abs(frame)
    print(f"shares {s0!r} + {s1!r} against the frame's {frame!r}: {e:.3g} = {e / bound:.3g} of "
          f"{bound:.3g}")
    assert s0 > 0 and s1 > 0 and e <= bound
