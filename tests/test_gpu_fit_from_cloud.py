"""GPU: a fit that starts where a real one starts -- scene_from_point_cloud on a point cloud --
and runs the README's loop on raw tensors: GaussianRasterizer(deterministic=True) ->
photometric_loss -> backward -> densification_stats -> SparseGaussianAdam.step, twenty times, then
one densify_and_prune with the extent of colmap.scene_extent.

The cloud: 300 points in [-1, 1]^3 in front of static_camera(64, 48).  The target is the render of
the scene with the cloud's true colours, the start the same cloud in grey, so the fit has the
colours to find (and everything else may move).  Asserted: the loss falls, two runs from one start
have the same bits in every parameter and in the loss sequence, and the densify succeeds.

Measured on an MI355X: loss 0.04260 -> 0.00787 in 20 steps.
"""
import numpy as np
import pytest
import torch

from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer,
                                         SparseGaussianAdam, colmap, densification_stats,
                                         densify_and_prune, photometric_loss,
                                         scene_from_point_cloud, static_camera)
from gpu_helpers import scene_inputs, to_dev

pytestmark = pytest.mark.gpu

N, W, H, SH_DEGREE, STEPS, LAMBDA = 300, 64, 48, 3, 20, 0.2
NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
LRS = dict(xyz=4e-3, f_dc=1e-2, f_rest=1e-2, opacity=5e-2, scaling=5e-3, rotation=1e-3)


def _cloud():
    rng = np.random.default_rng(11)
    xyz = rng.uniform(-1.0, 1.0, (N, 3)).astype(np.float32)
    rgb = rng.integers(0, 256, (N, 3)).astype(np.uint8)
    return xyz, rgb


def _activate(p):
    return dict(means3D=p["xyz"], shs=torch.cat([p["f_dc"], p["f_rest"]], dim=1),
                opacities=torch.sigmoid(p["opacity"]), scales=torch.exp(p["scaling"]),
                rotations=torch.nn.functional.normalize(p["rotation"]))


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _fit(gpu):
    xyz, rgb = _cloud()
    s = scene_inputs(None, static_camera(W, H), SH_DEGREE)
    rs = GaussianRasterizationSettings(
        H, W, s["tx"], s["ty"], to_dev(s["bg"], gpu), 1.0, to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), SH_DEGREE, to_dev(s["campos"], gpu), False, False,
        deterministic=True)
    raster = GaussianRasterizer(rs)
    truth = scene_from_point_cloud(xyz, rgb, sh_degree=SH_DEGREE, device=gpu)
    with torch.no_grad():
        target, radii = raster(means2D=None, colors_precomp=None, cov3D_precomp=None,
                               **_activate(truth))
    assert int((radii > 0).sum()) > N // 2 and float(target.max()) > 0.05
    start = scene_from_point_cloud(xyz, np.full((N, 3), 0.5, np.float32), sh_degree=SH_DEGREE,
                                   device=gpu)
    for k in NAMES:
        same = torch.equal(start[k], truth[k])
        assert same == (k != "f_dc"), k  # the colours alone differ
    params = {k: torch.nn.Parameter(start[k]) for k in NAMES}
    opt = SparseGaussianAdam([{"params": [params[k]], "lr": LRS[k], "name": k} for k in NAMES],
                             lr=0.0, eps=1e-15)
    accum = torch.zeros((N, 1), device=gpu)
    denom = torch.zeros((N, 1), device=gpu)
    max_radii = torch.zeros(N, dtype=torch.int32, device=gpu)
    losses = []
    for _ in range(STEPS):
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((N, 3), device=gpu, requires_grad=True)
        color, radii = raster(means2D=means2D, colors_precomp=None, cov3D_precomp=None,
                              **_activate(params))
        loss = photometric_loss(color, target, LAMBDA)
        loss.backward()
        densification_stats(radii, means2D.grad, accum, denom, max_radii)
        opt.step(radii, N)
        losses.append(loss.detach())
    with torch.no_grad():
        color, _ = raster(means2D=None, colors_precomp=None, cov3D_precomp=None,
                          **_activate(params))
        losses.append(photometric_loss(color, target, LAMBDA))
    out = {k: _bits(params[k]) for k in NAMES}
    out["losses"] = _bits(torch.stack(losses))
    return out, (opt, accum, denom, max_radii)


def test_a_fit_from_a_point_cloud_falls_repeats_and_densifies(gpu):
    first, state = _fit(gpu)
    second, _ = _fit(gpu)
    assert set(first) == set(second)
    for k in first:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)
    losses = first["losses"].view(np.float32)
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f} in {STEPS} steps")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

    # one densify on the result, with the extent of a ring of cameras round the cloud
    ring = np.array([[4.0 * np.cos(a), 0.5, 4.0 * np.sin(a)] for a in np.linspace(0, 6.0, 8)])
    _, extent = colmap.scene_extent(ring)
    opt, accum, denom, max_radii = state
    r = densify_and_prune(opt, accum, denom, max_radii, max_grad=2e-4, min_opacity=0.005,
                          extent=extent, max_screen_size=20, seed=1)
    assert sum(r.counts) >= N and r.counts.total == r.params["xyz"].shape[0] > 0
    assert r.counts.n_kept + r.counts.n_split + r.counts.n_removed == N
    for k in NAMES:
        p = r.params[k]
        assert p.shape[0] == r.counts.total and bool(torch.isfinite(p).all()), k
        assert opt.state[p]["exp_avg"].shape == p.shape
    assert r.source_index.shape == (r.counts.total,) and int(r.source_index.max()) < N
