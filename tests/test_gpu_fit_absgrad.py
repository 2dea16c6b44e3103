"""GPU: a fit that densifies on absolute gradients is bit-reproducible -- the fit of
tests/test_gpu_fit_step.py (the scene, start and learning rates of tests/fit_step_reference.py:
GaussianRasterizer(deterministic=True) -> photometric_loss -> backward -> densification_stats ->
SparseGaussianAdam.step) for twenty iterations, with densification_stats fed from
means2D_abs.grad (gsr_backward_abs) and one densify_and_prune after the tenth, run twice from one
start: every parameter, both moments, the statistics, source_index, the counts and the loss
sequence have the same bits.

The signed run: means2D_abs reaches no parameter, so up to the densify the fit is the signed fit
step for step, and the same loop accumulates the signed statistic from means2D.grad beside the
absolute one.  Before the densify grad_accum of the absolute run is at least the signed run's, row
by row: in the deterministic order fl(sum |v|) >= |fl(sum v)| word by word (one tree of monotone
roundings), and the norm and the accumulation are monotone too.

max_grad is twice test_gpu_fit_densify.py's: the absolute statistic is the larger one, and AbsGS
and gsplat raise the threshold with it (by 2 and by 4).  The counts are printed, not pinned: of
them the test asserts that they add up to the new P.
"""
import numpy as np
import pytest
import torch

import fit_step_reference as fr
from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer,
                                         SparseGaussianAdam, densification_stats,
                                         densify_and_prune, photometric_loss)
from gpu_helpers import to_dev

pytestmark = pytest.mark.gpu

ITERATIONS, DENSIFY_AFTER, SEED = 20, 10, 20
ROLES = dict(xyz="means3D", scaling="scales", rotation="rotations", opacity="opacities")
CONTROL = dict(max_grad=4.8e-4, min_opacity=0.005, extent=8.3, max_screen_size=24,
               percent_dense=0.01)


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
    # the signed run's statistics, up to the densify (module docstring)
    signed = [torch.zeros((P, 1), device=gpu), torch.zeros((P, 1), device=gpu),
              torch.zeros(P, dtype=torch.int32, device=gpu)]
    losses, out, before = [], {}, {}
    for it in range(1, ITERATIONS + 1):
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((P, 3), device=gpu, requires_grad=True)
        means2D_abs = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color, radii = raster(means2D=means2D, means2D_abs=means2D_abs, colors_precomp=None,
                              cov3D_precomp=None, **params)
        loss = photometric_loss(color, target, fr.LAMBDA)
        loss.backward()
        densification_stats(radii, means2D_abs.grad, accum, denom, max_radii)
        if it <= DENSIFY_AFTER:
            densification_stats(radii, means2D.grad, *signed)
        opt.step(radii, P)
        losses.append(loss.detach())
        if it == DENSIFY_AFTER:
            before = dict(accum=accum.cpu().numpy(), denom=denom.cpu().numpy(),
                          signed_accum=signed[0].cpu().numpy(),
                          signed_denom=signed[1].cpu().numpy(),
                          abs_grad=means2D_abs.grad.cpu().numpy(),
                          grad=means2D.grad.cpu().numpy())
            r = densify_and_prune(opt, accum, denom, max_radii, seed=SEED, roles=ROLES,
                                  activated=True, **CONTROL)
            params = dict(r.params)
            accum, denom, max_radii = r.grad_accum, r.denom, r.max_radii2D
            P = r.counts.total
            out.update(counts=torch.tensor(tuple(r.counts)), source_index=r.source_index)
    for k in fr.NAMES:
        st = opt.state[params[k]]
        assert float(st["step"]) == ITERATIONS and params[k].shape[0] == P
        out[f"param {k}"], out[f"exp_avg {k}"], out[f"exp_avg_sq {k}"] = \
            params[k], st["exp_avg"], st["exp_avg_sq"]
    out.update(grad_accum=accum, denom=denom, max_radii=max_radii, losses=torch.stack(losses))
    return {k: _bits(v) for k, v in out.items()}, before


def test_two_fits_on_absolute_gradients_have_the_same_bits(gpu):
    first, before = _fit(gpu)
    second, again = _fit(gpu)
    assert set(first) == set(second)
    for k in first:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)
    for k in before:
        np.testing.assert_array_equal(before[k].view(np.uint32), again[k].view(np.uint32),
                                      err_msg=k)

    losses = first["losses"].view(np.float32)
    counts = tuple(int(v) for v in first["counts"])
    print(f"counts (kept, cloned, split, removed) {counts}; loss {losses[0]:.5f} -> "
          f"{losses[DENSIFY_AFTER - 1]:.5f} -> {losses[-1]:.5f}")
    assert np.isfinite(losses).all() and len(losses) == ITERATIONS
    assert losses[DENSIFY_AFTER - 1] < losses[0]
    n_kept, n_clone, n_split, _ = counts
    assert first["param means3D"].shape[0] == n_kept + n_clone + 2 * n_split

    # the absolute statistic dominates the signed one, row by row
    np.testing.assert_array_equal(before["denom"], before["signed_denom"])
    assert (before["abs_grad"] >= np.abs(before["grad"])).all()
    assert (before["accum"] >= before["signed_accum"]).all()
    seen = before["denom"].reshape(-1) > 0
    assert seen.any() and before["accum"].max() > 0
    ratio = before["accum"].sum() / before["signed_accum"].sum()
    print(f"sum of grad_accum: absolute / signed = {ratio:.2f}")
    assert ratio > 1.0
    assert not before["accum"][~seen].any() and not before["accum"][fr.BEHIND].any()
