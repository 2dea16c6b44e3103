"""GPU: a whole fit iteration is bit-reproducible -- GaussianRasterizer(deterministic=True) ->
photometric_loss -> backward -> densification_stats -> SparseGaussianAdam.step(radii, P), twenty
times from one start, run twice (tests/fit_step_reference.py has the scene, the start and the
float64 restatement the learning rates were chosen with).

The float64 CPU restatement: loss 0.07461 -> 0.01102 in 20 steps, ratio 0.148.  Measured on an
MI355X: 0.07461 -> 0.01102, ratio 0.148.  This test asserts the bits of two runs, final < initial,
and that the statistics are consistent with the GPU's own radii; that the numbers are the right
ones is asserted in tests/test_gpu_fit_chain.py: the loss of every one of the twenty iterations
against the float64 sequence (fit_step_reference.LOSSES) within 8 x the float32 restatement's own
spread, and single iterations of this fit, started from the GPU's own state, against the float64
restatement of the iteration (image, loss, every gradient, the Adam step and the statistics).
"""
import numpy as np
import pytest
import torch

import fit_step_reference as fr
from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer,
                                         SparseGaussianAdam, densification_stats,
                                         photometric_loss)
from gpu_helpers import to_dev

pytestmark = pytest.mark.gpu


def _bits(t):
    a = t.detach().cpu().numpy()
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _fit(gpu):
    sc = fr.scene()
    s = sc["s"]
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, deterministic=True)
    raster = GaussianRasterizer(rs)
    with torch.no_grad():
        target, _ = raster(means2D=None, colors_precomp=None, cov3D_precomp=None,
                           **{k: to_dev(v, gpu) for k, v in fr.parameters(sc, False).items()})
    start = fr.parameters(sc, True)
    params = {k: torch.nn.Parameter(to_dev(start[k], gpu)) for k in fr.NAMES}
    P = len(start["means3D"])
    opt = SparseGaussianAdam([{"params": [params[k]], "lr": fr.LRS[k], "name": k}
                              for k in fr.NAMES], lr=0.0, eps=fr.EPS, betas=fr.BETAS)
    accum = torch.zeros((P, 1), device=gpu)
    denom = torch.zeros((P, 1), device=gpu)
    max_radii = torch.zeros(P, dtype=torch.int32, device=gpu)
    losses, radii_log = [], []
    for _ in range(fr.STEPS):
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color, radii = raster(means2D=means2D, colors_precomp=None, cov3D_precomp=None, **params)
        loss = photometric_loss(color, target, fr.LAMBDA)
        loss.backward()
        densification_stats(radii, means2D.grad, accum, denom, max_radii)
        opt.step(radii, P)
        losses.append(loss.detach())
        radii_log.append(radii)
    with torch.no_grad():
        color, _ = raster(means2D=None, colors_precomp=None, cov3D_precomp=None, **params)
        losses.append(photometric_loss(color, target, fr.LAMBDA))
    out = {f"param {k}": params[k] for k in fr.NAMES}
    for k in fr.NAMES:
        st = opt.state[params[k]]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == fr.STEPS
        out[f"exp_avg {k}"], out[f"exp_avg_sq {k}"] = st["exp_avg"], st["exp_avg_sq"]
    out.update(grad_accum=accum, denom=denom, max_radii=max_radii, losses=torch.stack(losses),
               radii=torch.stack(radii_log))
    return {k: _bits(v) for k, v in out.items()}, start


def test_two_fits_from_one_start_have_the_same_bits(gpu):
    first, start = _fit(gpu)
    second, _ = _fit(gpu)
    assert set(first) == set(second)
    for k in first:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)

    losses = first["losses"].view(np.float32)
    radii = first["radii"]
    print(f"loss {losses[0]:.5f} -> {losses[-1]:.5f} in {fr.STEPS} steps, "
          f"ratio {losses[-1] / losses[0]:.3f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]

    # the Gaussian no frame saw: parameters and moments untouched, no statistics
    assert (radii[:, fr.BEHIND] == 0).all()
    for k in fr.NAMES:
        np.testing.assert_array_equal(first[f"param {k}"][fr.BEHIND],
                                      start[k][fr.BEHIND].view(np.uint32), err_msg=k)
        assert not first[f"exp_avg {k}"][fr.BEHIND].any()
        assert not first[f"exp_avg_sq {k}"][fr.BEHIND].any()
    denom = first["denom"].view(np.float32).reshape(-1)
    accum = first["grad_accum"].view(np.float32).reshape(-1)
    assert denom[fr.BEHIND] == 0.0 and accum[fr.BEHIND] == 0.0
    # the others moved, and the statistics count what the frames saw
    np.testing.assert_array_equal(denom, (radii > 0).sum(0).astype(np.float32))
    np.testing.assert_array_equal(first["max_radii"], radii.max(0).clip(min=0))
    assert first["max_radii"][fr.LARGE] > fr.MIN_LARGE_RADIUS
    assert (accum >= 0.0).all() and not accum[denom == 0].any() and accum[fr.LARGE] > 0.0
    seen = (radii > 0).any(0)
    for k in fr.NAMES:
        moved = (first[f"param {k}"] != start[k].view(np.uint32)).reshape(len(seen), -1).any(1)
        assert moved[seen].any() and not moved[~seen].any(), k
