"""GPU: a whole fit, density control included, is bit-reproducible -- the fit of
tests/test_gpu_fit_step.py (the scene, start and learning rates of tests/fit_step_reference.py) for
forty iterations with densify_and_prune after the twentieth, run twice from one start: every
parameter, both moments, the statistics, source_index, the counts and the loss sequence have the
same bits, and the counts are the restatement's (tests/densify_reference.py) classification of the
GPU's own accumulators.

The thresholds were chosen on the CPU, before any GPU run, from the float64 restatement of the
first twenty iterations (reference_fit's loop with the gradient of the means2D offset accumulated
as gsr_densify_stats does), so that every Gaussian's statistic lies at least 10 % from its
threshold -- more than the float32 drift of the fit can move it:
    max_grad 2.4e-4        the nearest averages 2.044e-4 and 2.795e-4: 14.8 % and 16.5 % away
    percent_dense * extent = 0.01 * 8.3 = 0.083
                           the nearest largest scales 0.0726 and 0.0958: 12.5 % and 15.4 %
    min_opacity 0.005      the nearest opacities -0.056 and +0.031 (a factor 6)
    max_screen_size 24     the nearest radii 18 and 31: 25 % and 29 %; the world-size bound
                           0.1 * 8.3 is 60 % above the largest scale it tests
The float64 counts there: 9 kept, 4 cloned, 79 split, 10 removed (the 9 transparent ones and the
large near Gaussian, by its screen radius), so P goes from 98 to 171.  Measured on an MI355X: the
same counts; of the counts this test asserts that they are the restatement's classification of
the GPU's own accumulators and that each of n_clone, n_split and n_removed is >= 1.

Bit-reproducibility says nothing about the values: tests/test_gpu_fit_chain.py runs this same fit
(and the one upstream's parametrisation gives) and holds single iterations of it, before the
densify and on the first frames at the new P, to the float64 restatement of the iteration.
"""
import numpy as np
import pytest
import torch

import densify_reference as D
import fit_step_reference as fr
from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer,
                                         SparseGaussianAdam, densification_stats, densify,
                                         densify_and_prune, photometric_loss)
from gpu_helpers import to_dev

pytestmark = pytest.mark.gpu

ITERATIONS, DENSIFY_AFTER, SEED = 40, 20, 20
ROLES = dict(xyz="means3D", scaling="scales", rotation="rotations", opacity="opacities")
CONTROL = dict(max_grad=2.4e-4, min_opacity=0.005, extent=8.3, max_screen_size=24,
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
    losses, out = [], {}
    for it in range(1, ITERATIONS + 1):
        opt.zero_grad(set_to_none=True)
        means2D = torch.zeros((P, 3), device=gpu, requires_grad=True)
        color, radii = raster(means2D=means2D, colors_precomp=None, cov3D_precomp=None, **params)
        loss = photometric_loss(color, target, fr.LAMBDA)
        loss.backward()
        densification_stats(radii, means2D.grad, accum, denom, max_radii)
        opt.step(radii, P)
        losses.append(loss.detach())
        if it == DENSIFY_AFTER:
            before = {k: params[k].detach().cpu().numpy() for k in fr.NAMES}
            before.update(accum=accum.cpu().numpy(), denom=denom.cpu().numpy(),
                          max_radii=max_radii.cpu().numpy())
            r = densify_and_prune(opt, accum, denom, max_radii, seed=SEED, roles=ROLES,
                                  activated=True, **CONTROL)
            params = dict(r.params)
            accum, denom, max_radii = r.grad_accum, r.denom, r.max_radii2D
            P = r.counts.total
            out.update(counts=torch.tensor(tuple(r.counts)), source_index=r.source_index)
            assert [g["params"][0] for g in opt.param_groups] == [params[k] for k in fr.NAMES]
    for k in fr.NAMES:
        st = opt.state[params[k]]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == ITERATIONS
        assert st["exp_avg"].shape == params[k].shape and params[k].shape[0] == P
        out[f"param {k}"], out[f"exp_avg {k}"], out[f"exp_avg_sq {k}"] = \
            params[k], st["exp_avg"], st["exp_avg_sq"]
    assert len(opt.state) == len(fr.NAMES)
    out.update(grad_accum=accum, denom=denom, max_radii=max_radii, losses=torch.stack(losses))
    return {k: _bits(v) for k, v in out.items()}, before


def test_two_fits_with_density_control_have_the_same_bits(gpu):
    first, before = _fit(gpu)
    second, _ = _fit(gpu)
    assert set(first) == set(second)
    for k in first:
        np.testing.assert_array_equal(first[k], second[k], err_msg=k)

    losses = first["losses"].view(np.float32)
    counts = tuple(int(v) for v in first["counts"])
    print(f"counts {counts}; loss {losses[0]:.5f} -> {losses[DENSIFY_AFTER - 1]:.5f} -> "
          f"{losses[DENSIFY_AFTER]:.5f} (after densify) -> {losses[-1]:.5f}")
    assert np.isfinite(losses).all() and len(losses) == ITERATIONS

    # the counts and the order are the restatement's classification of the GPU's accumulators
    thresholds, radius = densify.stored_thresholds(activated=True, **CONTROL)
    keep, clone, split = D.classify(before["accum"], before["denom"], before["scales"],
                                    before["opacities"], before["max_radii"], thresholds, radius,
                                    log_space=False)
    P = len(keep)
    rows = np.arange(P, dtype=np.int32)
    assert counts == (keep.sum(), clone.sum(), split.sum(), P - keep.sum() - split.sum())
    np.testing.assert_array_equal(first["source_index"], np.concatenate(
        [rows[keep], rows[clone], rows[split], rows[split]]))
    n_kept, n_clone, n_split, n_removed = counts
    assert n_clone >= 1 and n_split >= 1 and n_removed >= 1
    assert first["param means3D"].shape[0] == n_kept + n_clone + 2 * n_split
    # the margins the thresholds were chosen for, on the GPU's own statistics
    with np.errstate(divide="ignore", invalid="ignore"):
        avg = np.nan_to_num(before["accum"].reshape(-1) / before["denom"].reshape(-1))
    print("margins: grad %.3f, split %.3f" % (
        np.abs(avg / thresholds[0] - 1).min(),
        np.abs(before["scales"].max(1) / thresholds[1] - 1).min()))
    # after the call the statistics start again from zero, for the new rows
    assert first["denom"].view(np.float32).max() <= ITERATIONS - DENSIFY_AFTER
    assert first["denom"].shape == (n_kept + n_clone + 2 * n_split, 1)
