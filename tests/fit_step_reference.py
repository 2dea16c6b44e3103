"""The small fit of tests/test_gpu_fit_step.py, and its float64 restatement on the CPU.

The scene is grad_scenes "chain" (P = 96, 40 x 24 px) plus two Gaussians: one behind the camera,
which no frame ever sees, and one made large and near enough for a screen radius above 20 px.
The target is the scene's own render; the start is a seeded perturbation of the means, the
opacities and the SH coefficients.  An iteration is render -> L1 + D-SSIM loss -> backward ->
densification statistics -> sparse Adam step over the five parameter tensors, the rows chosen by
the frame's radii.

reference_fit() runs that in float64 with the torch restatements of tests/grad_reference.py (the
lists and radii of every iteration from the CPU oracle on the current parameters) and
tests/loss_reference.py, and a float64 sparse Adam in upstream's uncorrected form.  The
perturbation, the learning rates and the step count below were chosen with it, before any GPU
run, so that the reference's loss at least halves (test_fit_step_reference.py holds that); the
GPU test asserts only final < initial.
"""
from __future__ import annotations

import copy

import numpy as np
import torch

import grad_reference as gr
import grad_scenes
import loss_reference as L

F32 = np.float32
STEPS = 20
SEED = 2024
LAMBDA = 0.2
EPS = 1e-15
BETAS = (0.9, 0.999)
# the rasterizer's argument names, in the optimizer's group order
NAMES = ("means3D", "shs", "opacities", "scales", "rotations")
LRS = dict(means3D=4e-3, shs=1e-2, opacities=1e-2, scales=1e-3, rotations=1e-3)
PERTURB = dict(means3D=0.04, shs=0.15, opacities=0.08)
BEHIND, LARGE = 96, 97  # the two added rows
MIN_LARGE_RADIUS = 20


def scene():
    """"chain" with the two added Gaussians: a grad_scenes-layout dict (the target's scene)."""
    sc = copy.deepcopy(grad_scenes.get("chain"))
    sc.pop("orc", None)
    sc.pop("ref64", None)
    g = sc["s"]["g"]
    add = lambda a, rows: np.ascontiguousarray(np.concatenate([a, np.asarray(rows, F32)]), F32)  # noqa: E731
    sh = np.zeros((2, g.sh.shape[1]), F32)
    sh[:, :3] = ((0.5, -0.2, 0.1), (-0.3, 0.4, 0.6))
    # the eye is at z = 4 and looks down -z: z = 6 is behind it; z = 2 is near
    g.xyz = add(g.xyz, [(0.3, -0.2, 6.0), (0.4, 0.1, 2.0)])
    g.rot = add(g.rot, [(1.0, 0.0, 0.0, 0.0), (0.8, 0.0, 0.6, 0.0)])
    g.scale = add(g.scale, [(0.2, 0.2, 0.2), (0.45, 0.3, 0.2)])
    g.opacity = add(g.opacity, [(0.7,), (0.35,)])
    g.sh = add(g.sh, sh)
    sc["name"] = "chain_fit"
    return sc


def parameters(sc, perturbed):
    """name -> float32 array by the rasterizer's argument names; with `perturbed` the fit's
    start (the two added rows keep their places)."""
    g = sc["s"]["g"]
    P = len(g.xyz)
    out = dict(means3D=g.xyz.copy(), shs=g.sh.reshape(P, -1, 3).copy(), opacities=g.opacity.copy(),
               scales=g.scale.copy(), rotations=g.rot.copy())
    if perturbed:
        rng = np.random.default_rng(SEED)
        for k, amp in PERTURB.items():
            d = (amp * rng.standard_normal(out[k].shape)).astype(F32)
            d[BEHIND:] = 0.0
            out[k] = out[k] + d
        out["opacities"] = np.clip(out["opacities"], 0.05, 0.95).astype(F32)
    return {k: np.ascontiguousarray(v, F32) for k, v in out.items()}


def _oracle_lists(sc, params):
    import oracle
    s = sc["s"]
    f = {k: np.ascontiguousarray(v, F32) for k, v in params.items()}
    P = len(f["means3D"])
    return oracle.forward(f["means3D"], f["opacities"], s["view"], s["proj"], s["campos"], s["tx"],
                          s["ty"], s["W"], s["H"], shs=f["shs"].reshape(P, -1), sh_degree=s["sh_degree"],
                          scales=f["scales"], rotations=f["rotations"],
                          scale_modifier=s["scale_modifier"], bg=s["bg"])


def render64(sc, params, orc=None):
    """The float64 restatement's image of `params` (tensors or arrays) -> (color, radii)."""
    s = sc["s"]
    cam = gr.camera_constants(s)
    t = {k: v if torch.is_tensor(v) else torch.tensor(np.asarray(v, np.float64)) for k, v in params.items()}
    if orc is None:
        orc = _oracle_lists(sc, {k: v.detach().numpy() for k, v in t.items()})
    zero = torch.zeros((len(t["means3D"]), 3), dtype=torch.float64)
    m2, conic, rgb, _, _ = gr.project(cam, orc["radii"], t["means3D"], zero, t["scales"],
                                      t["rotations"], None, t["shs"], None)
    color, _, _ = gr.composite((orc["ranges"], orc["point_list"]), m2, conic, t["opacities"], rgb,
                               s["bg"], cam["W"], cam["H"])
    return color, np.asarray(orc["radii"])


def reference_fit(steps=STEPS):
    """The float64 fit -> dict(losses [steps + 1] (the last after the final step), radii per
    iteration)."""
    sc = scene()
    target = render64(sc, parameters(sc, False))[0].detach()
    p = {k: torch.tensor(v.astype(np.float64), requires_grad=True)
         for k, v in parameters(sc, True).items()}
    m = {k: torch.zeros_like(v) for k, v in p.items()}
    v2 = {k: torch.zeros_like(v) for k, v in p.items()}
    losses, radii_log = [], []
    for it in range(steps + 1):
        color, radii = render64(sc, p)
        loss = L.loss_values(color, target, LAMBDA)[0]
        losses.append(float(loss.detach()))
        radii_log.append(radii)
        if it == steps:
            break
        for t in p.values():
            t.grad = None
        loss.backward()
        rows = torch.as_tensor(radii > 0)
        with torch.no_grad():
            for k in NAMES:
                g = p[k].grad
                sel = rows.reshape((-1,) + (1,) * (g.dim() - 1))
                m1 = BETAS[0] * m[k] + (1.0 - BETAS[0]) * g
                v1 = BETAS[1] * v2[k] + (1.0 - BETAS[1]) * g * g
                p1 = p[k] - LRS[k] * (m1 / (v1.sqrt() + EPS))
                m[k], v2[k] = torch.where(sel, m1, m[k]), torch.where(sel, v1, v2[k])
                p[k].copy_(torch.where(sel, p1, p[k]))
    return dict(losses=losses, radii=radii_log)
