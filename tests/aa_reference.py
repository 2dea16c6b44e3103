"""The reference of the antialiasing tests (gsr_forward_filtered / gsr_backward_filtered,
include/gsr.h).  CPU only.

The option replaces the opacity by
    o_eff = opacity * s,  s = sqrtf(fmaxf(0.000025f, rho)),  rho = D0 / D,
    D0 = a' c' - b b  (the 2D covariance before the 0.3 dilation),  D = a c - b b  (after it).

  forward_value(sc)    o_eff per Gaussian in float64 with a running bound for the float32 chain
                       (preprocess_reference's E arithmetic, the kernel's operations in the
                       kernel's order), the floor decision, and `judged`: no decision (the floor,
                       det != 0, the z cull) changes within the bound;
  scene_gradients(..)  the float64 torch restatement: camera_grad_reference's per-Gaussian stage
                       (restated here because it must hand out a', c' and D; (a' + 0.3) - 0.3 is not
                       a'), o_eff in between, then gr.composite and the planes' composite.
                       Autograd is the oracle of the backward; its gates are float64's and are
                       handed to a float32 run, so only rounding differs between the two;
  closed_form(..)      the terms include/gsr.h states, for the test that holds autograd to them.

The floor is a gate: on its flat side (rho <= 0.000025f, NaN included) s is the constant
sqrtf(0.000025f) and nothing flows to the covariance."""
from __future__ import annotations

import numpy as np
import torch

import camera_grad_reference as cgr
import grad_reference as gr
import plane_grad_reference as pg
from grad_reference import LOW_PASS, W_EPS, sh_basis
from preprocess_reference import CLAMP, E, NEAR, _cols, _mat_mul, _tp, _transpose

F32 = np.float32
FLOOR = float(F32(0.000025))
S_FLOOR = float(np.sqrt(F32(0.000025), dtype=F32))  # sqrtf(0.000025f), correctly rounded


# ---- the forward value with its float32 bound ---------------------------------------------------
def forward_value(sc) -> dict:
    """Per Gaussian of a scene dict: o_eff (float64), o_eff_bound, rho, rho_bound, floor (rho on
    the floor's flat side), in_frustum, det_ok, and judged (every decision that o_eff depends on
    is stable under the bound and nothing left float32's range)."""
    s = sc["s"]
    g = s["g"]
    W, H = int(s["W"]), int(s["H"])
    with np.errstate(all="ignore"):
        E.over = ~np.isfinite(g.xyz.astype(np.float64)).all(axis=1)
        vm = [float(v) for v in np.asarray(s["view"], F32).reshape(-1)]
        p = [E(g.xyz[:, k]) for k in range(3)]
        pv = [_tp(p, vm, k) for k in range(3)]
        unstable = np.abs(pv[2].v - NEAR) <= pv[2].e
        in_frustum = pv[2].v > NEAR
        if sc.get("cov6") is not None:
            c6 = np.asarray(sc["cov6"], F32)
            c = [E(c6[:, k]) for k in range(6)]
        else:
            mod = float(F32(s["scale_modifier"]))
            S = _cols(1, 0, 0, 0, 1, 0, 0, 0, 1)
            for k in range(3):
                S[k][k] = mod * E(g.scale[:, k])
            r, x, y, z = (E(g.rot[:, k]) for k in range(4))
            R = _cols(1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - r * z), 2.0 * (x * z + r * y),
                      2.0 * (x * y + r * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - r * x),
                      2.0 * (x * z - r * y), 2.0 * (y * z + r * x), 1.0 - 2.0 * (x * x + y * y))
            Mm = _mat_mul(S, R)
            Sig = _mat_mul(_transpose(Mm), Mm)
            c = [Sig[0][0], Sig[0][1], Sig[0][2], Sig[1][1], Sig[1][2], Sig[2][2]]
        tanx, tany = E(float(F32(s["tx"]))), E(float(F32(s["ty"])))
        fy = float(H) / (2.0 * tany)
        fx = float(W) / (2.0 * tanx)
        limx, limy = CLAMP * tanx, CLAMP * tany
        t = list(pv)
        t[0] = (t[0] / t[2]).fmax(-limx).fmin(limx) * t[2]
        t[1] = (t[1] / t[2]).fmax(-limy).fmin(limy) * t[2]
        tz2 = t[2] * t[2]
        J = _cols(fx / t[2], 0, -(fx * t[0]) / tz2, 0, fy / t[2], -(fy * t[1]) / tz2, 0, 0, 0)
        Wm = _cols(vm[0], vm[4], vm[8], vm[1], vm[5], vm[9], vm[2], vm[6], vm[10])
        T = _mat_mul(Wm, J)
        Vrk = _cols(c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5])
        cov = _mat_mul(_mat_mul(_transpose(T), _transpose(Vrk)), T)
        a0, b, c0 = cov[0][0], cov[0][1], cov[1][1]
        a, cc = a0 + LOW_PASS, c0 + LOW_PASS
        det = a * cc - b * b
        unstable |= np.abs(det.v) <= det.e
        det_ok = det.v != 0
        det0 = a0 * c0 - b * b
        rho = det0 / det
        floor = ~(rho.v > FLOOR)
        unstable |= np.abs(rho.v - FLOOR) <= rho.e
        sq = E(np.where(floor, FLOOR, rho.v), np.where(floor, 0.0, rho.e)).sqrt()
        o_eff = E(np.asarray(g.opacity, F32).reshape(-1)) * sq
        over = E.over.copy()
        E.over = None
    judged = ~unstable & ~over & np.isfinite(o_eff.e) & in_frustum & det_ok
    return dict(o_eff=o_eff.v, o_eff_bound=o_eff.e, rho=rho.v, rho_bound=rho.e, floor=floor,
                in_frustum=in_frustum, det_ok=det_ok, judged=judged)


def floor_value(opacity):
    """o_eff of a floor Gaussian, the bits the kernel gives: opacity * sqrtf(0.000025f)."""
    return (np.asarray(opacity, F32).reshape(-1) * F32(S_FLOOR)).astype(F32)


# ---- the differentiable restatement -------------------------------------------------------------
def project(cam, radii, vmP, pmP, cP, means3D, means2D, scales=None, rotations=None, cov3D=None,
            shs=None, colors=None, gates=None):
    """camera_grad_reference.project, operation for operation, that also returns the 2D covariance
    before the dilation and the determinant after it: (means2D_px, conic, rgb, z, (a0, b, c0,
    det) [P each, ones / zeros for radii == 0], gates, near_gate)."""
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
    Rv = torch.stack([vm[:, 4 * c_ + r_] for r_ in range(3) for c_ in range(3)], 1).reshape(-1, 3, 3)
    A = J @ Rv
    cov = A @ V @ A.transpose(1, 2)
    a0, b, c0 = cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]
    a, cc = a0 + LOW_PASS, c0 + LOW_PASS
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

    def full(v, fill=0.0):
        out = torch.full((P,) + v.shape[1:], fill, dtype=dt)
        return out.index_put((vis,), v)
    return (full(px), full(conic), full(rgb), full(tz), (full(a0), full(b), full(c0), full(det, 1.0)),
            new_gates, near)


def rho_of(a0, b, c0, det):
    return (a0 * c0 - b * b) / det


def factor(a0, b, c0, det, floor=None):
    """(s, floor, near_gate): s = sqrt(max(FLOOR, rho)) with the floor as a gate.  floor: a float64
    run's mask, else decided here.  near_gate counts the Gaussians whose rho lies within a
    float32 evaluation's reach of the floor: 1e-4 relative plus the cancellation of D0, 4 float32
    ulp of its terms."""
    rho = rho_of(a0, b, c0, det)
    near = 0
    if floor is None:
        r = rho.detach()
        floor = ~(r > FLOOR)
        reach = 1e-4 * FLOOR + 4 * 6e-8 * ((a0 * c0).abs() + b * b).detach() / det.detach().abs()
        near = int(((r - FLOOR).abs() <= reach).sum())
    safe = torch.where(floor, torch.ones_like(rho), rho)
    s = torch.where(floor, torch.full_like(rho, S_FLOOR), torch.sqrt(safe))
    return s, floor, near


def closed_form(a0, b, c0, opacity, G):
    """include/gsr.h's terms in numpy float64: (s, dL_dopacity, dL/da', dL/db, dL/dc') for
    G = dL/do_eff; zeros beyond dL_dopacity on the floor's flat side."""
    a0, b, c0, opacity, G = (np.asarray(v, np.float64) for v in (a0, b, c0, opacity, G))
    a, c = a0 + LOW_PASS, c0 + LOW_PASS
    D0, D = a0 * c0 - b * b, a * c - b * b
    rho = D0 / D
    on = rho > FLOOR
    s = np.where(on, np.sqrt(np.where(on, rho, 1.0)), S_FLOOR)
    grho = np.where(on, G * opacity / (2.0 * s), 0.0)
    return (s, G * s, grho * (c0 * D - D0 * c) / D ** 2, grho * (-2.0 * b * (D - D0)) / D ** 2,
            grho * (a0 * D - D0 * a) / D ** 2)


def scene_gradients(sc, lists, radii, dL, dLp=None, dtype=torch.float64, gates=None,
                    antialiasing=True):
    """camera_grad_reference.scene_gradients for the antialiased forward: d loss / d(every input
    of the Gaussians, by gr.LEAVES names) and d(viewmatrix, projmatrix, campos) with their error
    scales `S`, for loss = sum(color * dL) + sum(planes * dLp) (either None = absent).  Also
    o_eff, s, floor (bool [P]) and G = dL/do_eff [P].  gates: (project, composite, floor) of a
    float64 run.  near: (project, composite, floor) counts."""
    s_in = sc["s"]
    cam = gr.camera_constants(s_in)
    lv = gr.leaves(sc, dtype)
    camera = cgr.camera_of(s_in, dtype)
    P = lv["means3D"].shape[0]
    vmP, pmP, cP = (t.reshape(1, -1).expand(P, -1) for t in camera)
    for t in (vmP, pmP, cP):
        t.retain_grad()
    gp, gc, gf = gates if gates is not None else (None, None, None)
    m2, conic, rgb, z, (a0, b, c0, det), gates_p, near_p = project(
        cam, radii, vmP, pmP, cP, lv["means3D"], lv["means2D"], lv.get("scales"),
        lv.get("rotations"), lv.get("cov3D"), lv.get("shs"), lv.get("colors"), gp)
    fac, floor, near_f = factor(a0, b, c0, det, gf)
    if not antialiasing:
        fac = torch.ones_like(fac)
    o_eff = lv["opacity"].reshape(-1) * fac
    o_eff.retain_grad()
    color, gates_c, near_c = gr.composite(lists, m2, conic, o_eff, rgb, s_in["bg"], cam["W"],
                                          cam["H"], gc)
    as_t = lambda v: torch.as_tensor(np.asarray(v, np.float64)).to(dtype)  # noqa: E731
    loss = torch.zeros((), dtype=dtype)
    planes = None
    if dL is not None:
        loss = loss + (color * as_t(dL)).sum()
    if dLp is not None:
        planes, _, _ = pg.planes_of(lists, m2, conic, o_eff, pg.features(z, radii), cam["W"],
                                    cam["H"], gates_c)
        loss = loss + (planes * as_t(dLp)).sum()
    loss.backward()
    zg = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    out = {k: zg(v).detach().double().numpy() for k, v in lv.items()}
    out["S"] = {}
    for name, t in zip(cgr.CAMERA, (vmP, pmP, cP)):
        G = zg(t).detach().double().numpy()
        out[name] = G.sum(0)
        out["S"][name] = float(np.abs(G).sum(0).max())
    out.update(gates=(gates_p, gates_c, floor), near=(near_p, near_c, near_f),
               o_eff=o_eff.detach().double().numpy(), s=fac.detach().double().numpy(),
               floor=floor.numpy(), G=zg(o_eff).detach().double().numpy(),
               color=color.detach().double().numpy(),
               planes=None if planes is None else planes.detach().double().numpy(),
               cov2=tuple(v.detach().double().numpy() for v in (a0, b, c0, det)))
    return out


# ---- the tolerance of the GPU tests: measured, not chosen ----------------------------------------
# f: the reference's own float32 spread per gradient tensor under the antialiased forward --
# gr.rel_err (the camera's three: cgr.cam_err) of scene_gradients evaluated in float32 against
# float64 with the float64 run's gates, the largest over the six aa_scenes and over the two losses
# of LOSSES (colour alone; colour and the three planes), measured on the CPU with the oracle's
# lists.  test_aa_reference.py re-measures it and holds each constant to within a factor 2.  The GPU
# tests allow gr.BOUND_FACTOR x f, for grad_reference's reasons.
LOSSES = ("colour", "combined")
# (the larger of the two losses per scene; subpixel's needles, whose D0 cancels to ~1e-4 of its
# terms, set scales and rotations: a float32 rho there carries ~1e-3 of relative error)
#                           chain    long_l.  precomp. edges    subpixel floor
F32_SPREAD = {
    "means3D": 4.3e-6,     # 1.5e-6   8.0e-7   4.0e-6   7.1e-7   4.3e-6   1.4e-6
    "means2D": 5.9e-6,     # 1.5e-6   9.0e-7   5.9e-6   6.4e-7   3.3e-6   1.1e-6
    "opacity": 1.1e-5,     # 6.9e-7   6.4e-7   1.3e-6   4.4e-7   1.1e-5   4.0e-7
    "scales": 2.6e-4,      # 1.3e-6   4.2e-7   -        9.6e-7   2.6e-4   -
    "rotations": 1.5e-5,   # 1.1e-6   5.1e-7   -        5.1e-7   1.5e-5   -
    "cov3D": 2.4e-6,       # -        -        2.4e-6   -        -        1.6e-6
    "shs": 3.0e-6,         # 4.8e-7   1.8e-7   -        2.4e-7   3.0e-6   -
    "colors": 1.1e-6,      # -        -        1.1e-6   -        -        6.5e-7
    "viewmatrix": 1.3e-6,  # 3.2e-7   1.5e-7   3.0e-7   2.0e-7   1.3e-6   1.4e-7
    "projmatrix": 7.2e-7,  # 2.4e-7   3.7e-7   7.2e-7   3.4e-7   4.9e-7   2.0e-7
    "campos": 1.4e-7,      # 2.6e-8   1.4e-7   -        9.3e-8   1.4e-7   -
}


def err(got, ref, key):
    """The error of one gradient tensor against a scene_gradients result, on its scale."""
    if key in cgr.CAMERA:
        return cgr.cam_err(got, ref, key)
    return gr.rel_err(np.asarray(got, np.float64).reshape(ref[key].shape), ref[key])


def bound(key):
    return gr.BOUND_FACTOR * F32_SPREAD[key]


def plane_dL(sc):
    """The planes' gradients of a scene, [3, H, W] float32 (depth, inverse depth, final_T), from
    the scene's own generator state: fixed per scene."""
    rng = np.random.default_rng(1000 + sum(map(ord, sc["name"])))
    return np.ascontiguousarray(rng.standard_normal((3, sc["H"], sc["W"])), F32)


def loss_gradients(sc, loss):
    """(dL, dLp) of a loss of LOSSES."""
    return (sc["dL"], None) if loss == "colour" else (sc["dL"], plane_dL(sc))
