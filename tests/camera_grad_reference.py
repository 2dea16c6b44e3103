"""The reference of the camera-gradient tests (gsr_backward_camera, include/gsr.h):
the per-Gaussian stage of grad_reference.project restated with the camera as tensors.  CPU only,
torch.  gr.project takes the camera as Python floats and rebuilds the view rotation and campos with
torch.tensor, which cuts the graph; here viewmatrix [16], projmatrix [16] (column-major, as the
kernels read them) and campos [3] are tensors, possibly functions of a pose
(camera.camera_tensors), and everything downstream is grad_reference's and plane_grad_reference's:
gr.composite for the colour, the planes' composite with z = t_2 differentiable in the view matrix.
Lists and radii come from the forward under test, float gates from the float64 run, as everywhere
in this suite.  tanfov and the focal lengths are constants: the intrinsics get no gradient.

The error scale.  The camera enters as per-Gaussian copies: vm.expand(P, 16), pm.expand(P, 16),
c.expand(P, 3), with their gradients retained, so the gradient of copy i is G_i, Gaussian i's
contribution.  The reference gradient is sum_i G_i; the scale of a tensor is
S = max over its entries of sum_i |G_i|, the size at which these sums round, and every camera
comparison is e = max|got - ref| / S (cam_err).  A gradient that happens to cancel over the
Gaussians does not inflate the error of a correct kernel.
"""
from __future__ import annotations

import numpy as np
import torch

import grad_reference as gr
import plane_grad_reference as pg
from grad_reference import LOW_PASS, W_EPS, sh_basis

F32 = np.float32
CAMERA = ("viewmatrix", "projmatrix", "campos")


def camera_of(s, dtype=torch.float64, requires_grad=True):
    """(vm [16], pm [16], c [3]) of a scene_inputs dict as leaves: the float32 values the kernels
    read, in `dtype`."""
    t = lambda a, n: torch.tensor(np.asarray(a, F32).reshape(-1)[:n].astype(np.float64),  # noqa: E731
                                  dtype=dtype, requires_grad=requires_grad)
    return t(s["view"], 16), t(s["proj"], 16), t(s["campos"], 3)


def project(cam, radii, vmP, pmP, cP, means3D, means2D, scales=None, rotations=None, cov3D=None,
            shs=None, colors=None, gates=None):
    """gr.project with the camera per Gaussian: vmP [P,16], pmP [P,16], cP [P,3] (cam gives the
    constants only: W, H, fx, fy, limx, limy, mod, D).  Same operations in the same order.  Returns
    (means2D_px, conic, rgb, z [P], gates, near_gate); z = t_2, zero rows for radii == 0."""
    vis = torch.as_tensor(np.flatnonzero(np.asarray(radii) > 0))
    P, dt = means3D.shape[0], means3D.dtype
    vm, pm = vmP[vis], pmP[vis]
    p = means3D[vis]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    t = [vm[:, k] * x + vm[:, 4 + k] * y + vm[:, 8 + k] * z + vm[:, 12 + k] for k in range(3)]
    h = [pm[:, k] * x + pm[:, 4 + k] * y + pm[:, 8 + k] * z + pm[:, 12 + k] for k in range(4)]
    pw = 1.0 / (h[3] + W_EPS)
    ndc = torch.stack([h[0] * pw, h[1] * pw], 1) + means2D[vis][:, :2]
    size = torch.tensor([cam["W"], cam["H"]], dtype=dt)
    px = ((ndc + 1.0) * size - 1.0) * 0.5

    if cov3D is not None:
        c = cov3D[vis]
        V = torch.stack([c[:, 0], c[:, 1], c[:, 2], c[:, 1], c[:, 3], c[:, 4], c[:, 2], c[:, 4],
                         c[:, 5]], 1).reshape(-1, 3, 3)
    else:
        q = rotations[vis]
        r, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
        R = torch.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - r * qz), 2 * (qx * qz + r * qy),
                         2 * (qx * qy + r * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - r * qx),
                         2 * (qx * qz - r * qy), 2 * (qy * qz + r * qx), 1 - 2 * (qx * qx + qy * qy)],
                        1).reshape(-1, 3, 3)
        N = R * (cam["mod"] * scales[vis])[:, None, :]
        V = N @ N.transpose(1, 2)

    near = 0
    new_gates = {}
    tc = []
    for k, lim in ((0, cam["limx"]), (1, cam["limy"])):
        ratio = t[k] / t[2]
        if gates is None:
            lo, hi = ratio.detach() < -lim, ratio.detach() > lim
            near += int(((ratio.detach().abs() - lim).abs() <= 1e-5 * lim).sum())
        else:
            lo, hi = gates[f"lo{k}"], gates[f"hi{k}"]
        new_gates[f"lo{k}"], new_gates[f"hi{k}"] = lo, hi
        cl = torch.where(lo, torch.full_like(ratio, -lim),
                         torch.where(hi, torch.full_like(ratio, lim), ratio))
        tc.append(cl * t[2])
    tz = t[2]
    zero = torch.zeros_like(tz)
    J = torch.stack([cam["fx"] / tz, zero, -(cam["fx"] * tc[0]) / (tz * tz),
                     zero, cam["fy"] / tz, -(cam["fy"] * tc[1]) / (tz * tz)], 1).reshape(-1, 2, 3)
    # R[r][c] = vm[4 c + r], per Gaussian
    Rv = torch.stack([vm[:, 4 * c_ + r_] for r_ in range(3) for c_ in range(3)], 1).reshape(-1, 3, 3)
    A = J @ Rv
    cov = A @ V @ A.transpose(1, 2)
    a, b, cc = cov[:, 0, 0] + LOW_PASS, cov[:, 0, 1], cov[:, 1, 1] + LOW_PASS
    det = a * cc - b * b
    conic = torch.stack([cc / det, -b / det, a / det], 1)

    if colors is not None:
        rgb = colors[vis]
    else:
        d = p - cP[vis]
        d = d / d.norm(dim=1, keepdim=True)
        n = (cam["D"] + 1) ** 2
        val = (sh_basis(d)[:, :n, None] * shs[vis][:, :n, :]).sum(1) + 0.5
        if gates is None:
            clamped = val.detach() < 0
            near += int((val.detach().abs() <= 1e-5).any(dim=1).sum())
        else:
            clamped = gates["clamped"]
        new_gates["clamped"] = clamped
        rgb = torch.where(clamped, torch.zeros_like(val), val)

    def full(v):
        out = torch.zeros((P,) + v.shape[1:], dtype=dt)
        return out.index_put((vis,), v)
    return full(px), full(conic), full(rgb), full(tz), new_gates, near


def scene_loss(sc, lists, radii, dL, dLp, camera, lv, gates=None):
    """The loss sum(color * dL) + sum(planes * dLp) (either None = absent) of a scene under the
    camera (vm, pm, c) (tensors of lv's dtype, any graph).  Returns (loss, parts): parts holds the
    per-Gaussian copies vmP, pmP, cP (gradients retained), gates, near, color, planes."""
    s = sc["s"]
    cam = gr.camera_constants(s)
    P = lv["means3D"].shape[0]
    dtype = lv["means3D"].dtype
    vmP, pmP, cP = (t.reshape(1, -1).expand(P, -1) for t in camera)
    for t in (vmP, pmP, cP):
        if t.requires_grad:
            t.retain_grad()
    gp, gc = gates if gates is not None else (None, None)
    m2, conic, rgb, z, gates_p, near_p = project(
        cam, radii, vmP, pmP, cP, lv["means3D"], lv["means2D"], lv.get("scales"),
        lv.get("rotations"), lv.get("cov3D"), lv.get("shs"), lv.get("colors"), gp)
    color, gates_c, near_c = gr.composite(lists, m2, conic, lv["opacity"], rgb, s["bg"], cam["W"],
                                          cam["H"], gc)
    as_t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    loss = torch.zeros((), dtype=dtype)
    planes = None
    if dL is not None:
        loss = loss + (color * as_t(dL)).sum()
    if dLp is not None:
        planes, _, _ = pg.planes_of(lists, m2, conic, lv["opacity"], pg.features(z, radii),
                                    cam["W"], cam["H"], gates_c)
        loss = loss + (planes * as_t(dLp)).sum()
    return loss, dict(vmP=vmP, pmP=pmP, cP=cP, gates=(gates_p, gates_c), near=(near_p, near_c),
                      color=color, planes=planes, m2=m2, conic=conic, rgb=rgb, z=z)


def scene_gradients(sc, lists, radii, dL, dLp=None, dtype=torch.float64, gates=None, camera=None):
    """d loss / d(viewmatrix, projmatrix, campos) of scene_loss, each the partial with the other
    two fixed, as flat float64 arrays [16], [16], [3]; `S`: the error scale per tensor (module
    docstring); and the gradients of the Gaussians' own inputs by gr.LEAVES names.  camera: (vm,
    pm, c) to differentiate through (e.g. camera_tensors of a pose leaf; the caller reads the
    pose's .grad afterwards), default the scene's as leaves.  gates: a float64 run's."""
    lv = gr.leaves(sc, dtype)
    if camera is None:
        camera = camera_of(sc["s"], dtype)
    loss, parts = scene_loss(sc, lists, radii, dL, dLp, camera, lv, gates)
    loss.backward()
    out = {k: (torch.zeros_like(v) if v.grad is None else v.grad).detach().double().numpy()
           for k, v in lv.items()}
    out["S"] = {}
    for name, key in zip(CAMERA, ("vmP", "pmP", "cP")):
        t = parts[key]
        G = (torch.zeros_like(t) if t.grad is None else t.grad).detach().double().numpy()
        out[name] = G.sum(0)
        out["S"][name] = float(np.abs(G).sum(0).max())
    out.update(gates=parts["gates"], near=parts["near"], loss=float(loss.detach()))
    return out


def cam_err(got, ref, name):
    """e = max|got - ref[name]| / S[name] (0 where S is 0 and the two agree exactly)."""
    d = float(np.abs(np.asarray(got, np.float64).reshape(-1) - ref[name]).max())
    S = ref["S"][name]
    return d / S if S > 0 else d


# ---- the tolerance of the GPU tests: measured, not chosen ----------------------------------------
# f: cam_err of scene_gradients evaluated in float32 (gates and lists of the float64 run, so only
# rounding differs) against float64, the largest over the six camera_grad_scenes and over the
# colour-only and the combined (colour + three planes) losses, measured on the CPU with the oracle's
# lists (test_camera_grad_reference.py re-measures it and holds each constant to within a factor 2).
# The GPU tests allow gr.BOUND_FACTOR x f, for grad_reference's reasons: the kernels group the sums
# differently (lane trees and atomics for the 2D gradients, then rows of 16 lanes, the block's 16
# rows, the blocks in double), roundings of the same class as f.  A wrong term shows at order 1.
# (the larger of the two losses per scene; campos sits below one float32 ulp because S adds the
# Gaussians' magnitudes while their independent roundings add in quadrature)
#                            chain     long_lists precomputed edges    blocks    sparse
F32_SPREAD = {
    "viewmatrix": 6.8e-7,  # 1.8e-7   1.2e-7     3.5e-7      6.8e-7   2.4e-7    1.8e-7
    "projmatrix": 8.2e-7,  # 3.0e-7   3.1e-7     8.2e-7      4.0e-7   1.5e-7    3.0e-7
    "campos": 9.8e-8,      # 2.7e-8   3.6e-8     -           9.8e-8   2.0e-8    2.7e-8
}
LOSSES = ("colour", "combined")


def bound(name):
    return gr.BOUND_FACTOR * F32_SPREAD[name]
