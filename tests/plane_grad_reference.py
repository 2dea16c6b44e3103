"""The reference of the plane-gradient tests (gsr_backward_planes, include/gsr.h):
grad_reference's restatement with three more channels.  CPU only, torch.

No new composite: depth_map, inv_depth_map and final_T are the three channels of
gr.composite(lists, m2, conic, opacity, feat, bg=(0, 0, 1)) with feat = (z, 1 / z, 0) -- the
channel identity gsr_forward_depth states.  z is restated from means3D and the view matrix (zero
rows for radii == 0, as gr.project's), and the planes' composite takes the gates of the colour run.

The loss is sum(color * dL) + sum(planes * dLp), dL the scene's own (grad_scenes) and dLp =
plane_dL(name): three planes in the order depth, inverse depth, transmittance.  Either may be None.
"""
from __future__ import annotations

import numpy as np
import torch

import grad_reference as gr
import grad_scenes

F32 = np.float32
PLANES = ("depth_map", "inv_depth_map", "final_T")
PLANE_BG = (0.0, 0.0, 1.0)


def plane_dL(name):
    """The planes' gradients of a grad scene: [3, H, W] float32, depth, inverse depth, final_T."""
    sc = grad_scenes.get(name)
    rng = np.random.default_rng(100 + grad_scenes.SEEDS[name])
    return np.ascontiguousarray(rng.standard_normal((3, sc["H"], sc["W"])), F32)


def view_depth(cam, radii, means3D):
    """View-space z of the Gaussians the forward kept (zero rows for the others)."""
    vis = torch.as_tensor(np.flatnonzero(np.asarray(radii) > 0))
    vm = cam["view"]
    p = means3D[vis]
    z = vm[2] * p[:, 0] + vm[6] * p[:, 1] + vm[10] * p[:, 2] + vm[14]
    return torch.zeros(means3D.shape[0], dtype=means3D.dtype).index_put((vis,), z)


def features(z, radii):
    """feat [P,3] = (z, 1 / z, 0), two functions of one z; zero rows for radii == 0."""
    keep = torch.as_tensor(np.asarray(radii) > 0)
    safe = torch.where(keep, z, torch.ones_like(z))
    zero = torch.zeros_like(z)
    return torch.stack([torch.where(keep, z, zero), torch.where(keep, 1.0 / safe, zero), zero], 1)


def planes_of(lists, m2, conic, opacity, feat, W, H, gates=None):
    """(planes [3,H,W], gates, near_gate): depth_map, inv_depth_map, final_T of given records."""
    return gr.composite(lists, m2, conic, opacity, feat, PLANE_BG, W, H, gates)


def disparity_loss(sc, dLd):
    """loss_fn of scene_gradients: sum(d * dLd) with d stereo.metric_disparity(inv_depth_map,
    final_T, tanfovx, W, normalise=True) restated in the planes' dtype."""
    from gaussiansplattingviewer_amd.stereo import BASELINE
    scale = float(sc["W"]) / (2.0 * float(sc["s"]["tx"])) * abs(float(BASELINE))

    def loss(color, planes):
        cover = 1.0 - planes[2]
        d = torch.where(cover > 0, planes[1] * scale / cover, torch.zeros_like(cover))
        return (d * torch.as_tensor(np.asarray(dLd, np.float64)).to(planes.dtype)).sum()
    return loss


def disparity_dL(name, final_T):
    """The disparity's gradient of a grad scene, [H, W] float32: zero where the covered share
    1 - final_T (of the float64 reference) is below 1e-3, so that the quotient's conditioning
    stays out of the test."""
    rng = np.random.default_rng(200 + grad_scenes.SEEDS[name])
    dLd = rng.standard_normal(np.shape(final_T))
    return np.ascontiguousarray(np.where(1.0 - np.asarray(final_T) < 1e-3, 0.0, dLd), F32)


def scene_gradients(sc, lists, radii, dL, dLp, dtype=torch.float64, gates=None, loss_fn=None):
    """gr.scene_gradients for the loss sum(color * dL) + sum(planes * dLp) (either None = absent)
    + loss_fn(color, planes) (if given): d loss / d(every input), the 2D gradients in between, and
    `depths`: the gradient of z through the features only (gsr_plane_gradients.dL_ddepths).  gates:
    (project, composite) gates of a float64 run.  Returns dict(grads..., gates=, near=, color=,
    planes=)."""
    s = sc["s"]
    cam = gr.camera_constants(s)
    lv = gr.leaves(sc, dtype)
    gp, gc = gates if gates is not None else (None, None)
    m2, conic, rgb, gates_p, near_p = gr.project(
        cam, radii, lv["means3D"], lv["means2D"], lv.get("scales"), lv.get("rotations"),
        lv.get("cov3D"), lv.get("shs"), lv.get("colors"), gp)
    z = view_depth(cam, radii, lv["means3D"])
    for v in (m2, conic, rgb, z):
        v.retain_grad()
    color, gates_c, near_c = gr.composite(lists, m2, conic, lv["opacity"], rgb, s["bg"], cam["W"],
                                          cam["H"], gc)
    planes, _, _ = planes_of(lists, m2, conic, lv["opacity"], features(z, radii), cam["W"],
                             cam["H"], gates_c)
    as_t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    loss = torch.zeros((), dtype=dtype)
    if dL is not None:
        loss = loss + (color * as_t(dL)).sum()
    if dLp is not None:
        loss = loss + (planes * as_t(dLp)).sum()
    if loss_fn is not None:
        loss = loss + loss_fn(color, planes)
    loss.backward()
    g = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    out = {k: g(v).detach().double().numpy() for k, v in lv.items()}
    out.update(means2D_px=g(m2).double().numpy(), conic=g(conic).double().numpy(),
               rgb=g(rgb).double().numpy(), depths=g(z).double().numpy(),
               gates=(gates_p, gates_c), near=(near_p, near_c),
               color=color.detach().double().numpy(), planes=planes.detach().double().numpy())
    return out


# ---- the tolerance of the GPU tests: measured, not chosen ----------------------------------------
# f: gr.rel_err of scene_gradients in float32 (gates and lists of the float64 run) against float64,
# the largest over the losses the GPU tests feed -- colour plus the three planes and the three
# planes alone on the four grad_scenes (the columns below), and each plane alone on S1 (which sets
# opacity, 1.5e-6, and scales, 1.3e-6, both under final_T alone) -- measured on the CPU with the
# oracle's lists (test_plane_grad_reference.py re-measures it and holds each constant to within a
# factor 2).
# The GPU tests allow gr.BOUND_FACTOR x f, for grad_reference's reasons: lane trees, atomics in
# arrival order, T rebuilt by division.  grad_reference.F32_SPREAD cannot stand in: the planes' loss
# weighs other pixels and splats (z is O(4), 1 / z O(0.3)).
#                                                   S1        S2        S3        S4
F32_SPREAD = {
    "means3D": 2.5e-6,      # 1.1e-6   1.3e-6   2.5e-6   2.4e-7
    "means2D": 3.1e-6,      # 1.1e-6   1.8e-6   3.1e-6   2.1e-7   (upstream's units)
    "means2D_px": 2.9e-6,   # 1.1e-6   1.4e-6   2.9e-6   2.1e-7   (pixels: the blend's own)
    "conic": 1.8e-6,        # 1.8e-6   1.7e-6   1.1e-6   6.3e-7
    "opacity": 1.5e-6,      # 5.8e-7   1.3e-6   1.1e-6   4.9e-7
    "depths": 1.3e-6,       # 5.0e-7   4.6e-7   1.3e-6   3.9e-7   (dL_ddepths: the tenth sum)
    "rgb": 1.2e-6,          # 4.8e-7   6.2e-7   1.2e-6   3.3e-7   (dL_dcolors; combined loss only)
    "shs": 6.5e-7,          # 5.0e-7   6.5e-7   -        2.7e-7   (combined loss only)
    "scales": 1.3e-6,       # 5.7e-7   8.3e-7   -        4.5e-7
    "rotations": 1.3e-6,    # 5.4e-7   1.3e-6   -        4.8e-7
    "cov3D": 2.7e-6,        # -        -        2.7e-6   -
}
F32_SPREAD["colors"] = F32_SPREAD["rgb"]
LOSSES = ("combined", "planes")  # the losses f is measured under on every scene
ONE_PLANE_SCENE = "chain"        # ... and each of PLANES alone on this one


def loss_gradients(sc, loss):
    """(dL, dLp) of a loss by name: "combined", "planes", or one of PLANES (the others zero, which
    is what a NULL plane reads as)."""
    dLp = plane_dL(sc["name"])
    if loss in PLANES:
        keep = np.array([n == loss for n in PLANES], F32)
        dLp = dLp * keep[:, None, None]
    return (sc["dL"] if loss == "combined" else None), dLp


# The same measurement for the disparity loss (disparity_loss with disparity_dL) on S1, the scene
# of the metric_disparity test: every pixel of S1 is covered (max final_T 0.91), as torch's quotient
# needs (where 1 - final_T == 0 its backward is 0 x nan).
F32_SPREAD_DISPARITY = {"means3D": 2.1e-6, "means2D": 3.4e-6, "opacity": 1.6e-6, "scales": 1.8e-6,
                        "rotations": 2.1e-6}


def bound(key, table=None):
    return gr.BOUND_FACTOR * (F32_SPREAD if table is None else table)[key]
