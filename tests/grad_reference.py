"""A differentiable restatement of the forward in torch, with autograd as the oracle of the
backward pass (gsr_backward, include/gsr.h).  CPU only; float64 is the reference, float32 the
yardstick of a correct float32 backward's rounding.

  project(...)    the per-Gaussian stage: view transform, the 1e-7 divide, cov3D from scale and
                  rotation, the EWA cov2D with the 1.3 tan clamp and + 0.3, the conic, ndc2Pix with
                  a (zero) means2D offset added in NDC, SH -> rgb with its clamp;
  composite(...)  per tile over given (ranges, point_list): alpha, the two skips, the exclusive
                  cumprod for T, the termination mask, the colour with final_T bg.

Integer decisions (the lists, and with them depth order, rect membership and culls) are given:
`lists` and `radii` come from the forward under test (bit-exact-pinned integers), never from
here.  Float gates are evaluated in float64 and returned as masks (`gates`); a float32 evaluation
takes the float64 run's masks, so only rounding differs between the two.  Gates select: every mask
is applied with torch.where on constants, so nothing flows through a flat side.

near_gate counts, per call, the decisions that rounding could flip -- the condition on a test scene
is that both counts are 0 (test_grad_reference.py):
  composite: (pixel, splat) pairs, up to the pixel's termination, with alpha within 1e-5 relative
             of 1/255, o G within 1e-5 relative of 0.99, power in (-1e-6, 0], or T (1 - alpha)
             within 1e-3 relative of 1e-4;
  project:   Gaussians with |t.x / t.z| or |t.y / t.z| within 1e-5 relative of 1.3 tan, or an
             SH sum + 0.5 within 1e-5 (absolute: the knee is 0, colours are O(1)) of 0.
Scenes too large for that condition (frame_grad_scenes) ask composite for the pixels near a gate
instead (its `band` argument) and zero their image gradients there.
"""
from __future__ import annotations

import numpy as np
import torch

F32 = np.float32
# the forward's constants, as the float32 values its kernels hold
A_MIN = float(F32(1.0) / F32(255.0))
A_CAP = float(F32(0.99))
T_MIN = float(F32(0.0001))
LOW_PASS = float(F32(0.3))
W_EPS = float(F32(0.0000001))
SH_C0 = float(F32(0.28209479177387814))
SH_C1 = float(F32(0.4886025119029199))
SH_C2 = [float(F32(v)) for v in (1.0925484305920792, -1.0925484305920792, 0.31539156525252005,
                                 -1.0925484305920792, 0.5462742152960396)]
SH_C3 = [float(F32(v)) for v in (-0.5900435899266435, 2.890611442640554, -0.4570457994644658,
                                 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
                                 -0.5900435899266435)]


def sh_basis(d):
    """The 16 SH basis values at unit directions d [n,3], signed as upstream adds them."""
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    return torch.stack([
        torch.full_like(x, SH_C0), -SH_C1 * y, SH_C1 * z, -SH_C1 * x,
        SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz,
        SH_C2[4] * (xx - yy),
        SH_C3[0] * y * (3.0 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4.0 * zz - xx - yy),
        SH_C3[3] * z * (2.0 * zz - 3.0 * xx - 3.0 * yy), SH_C3[4] * x * (4.0 * zz - xx - yy),
        SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3.0 * yy)], dim=1)


def camera_constants(s):
    """The scalars the kernels derive from a scene_inputs dict, in their float32 arithmetic."""
    W, H = int(s["W"]), int(s["H"])
    tx, ty = F32(s["tx"]), F32(s["ty"])
    return dict(W=W, H=H, fx=float(F32(W) / (F32(2.0) * tx)), fy=float(F32(H) / (F32(2.0) * ty)),
                limx=float(F32(1.3) * tx), limy=float(F32(1.3) * ty),
                view=[float(v) for v in np.asarray(s["view"], F32).reshape(-1)],
                proj=[float(v) for v in np.asarray(s["proj"], F32).reshape(-1)],
                campos=[float(v) for v in np.asarray(s["campos"], F32).reshape(-1)[:3]],
                mod=float(F32(s["scale_modifier"])), D=int(s["sh_degree"]))


def project(cam, radii, means3D, means2D, scales=None, rotations=None, cov3D=None, shs=None,
            colors=None, gates=None):
    """The per-Gaussian stage of the Gaussians the forward kept (radii > 0); the others get zero
    rows (they are in no list).  Tensors of one dtype; means2D [P,3] is the offset added to the
    NDC centre (x, y).  Returns (means2D_px [P,2], conic [P,3], rgb [P,3], gates, near_gate):
    gates holds this run's clamp masks (pass a float64 run's to a float32 run)."""
    vis = torch.as_tensor(np.flatnonzero(np.asarray(radii) > 0))
    P, dt = means3D.shape[0], means3D.dtype
    vm, pm = cam["view"], cam["proj"]
    p = means3D[vis]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    t = [vm[k] * x + vm[4 + k] * y + vm[8 + k] * z + vm[12 + k] for k in range(3)]
    h = [pm[k] * x + pm[4 + k] * y + pm[8 + k] * z + pm[12 + k] for k in range(4)]
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

    # the clamp: the clamped ratio times t.z, differentiated as written
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
        cl = torch.where(lo, torch.full_like(ratio, -lim), torch.where(hi, torch.full_like(ratio, lim), ratio))
        tc.append(cl * t[2])
    tz = t[2]
    zero = torch.zeros_like(tz)
    J = torch.stack([cam["fx"] / tz, zero, -(cam["fx"] * tc[0]) / (tz * tz),
                     zero, cam["fy"] / tz, -(cam["fy"] * tc[1]) / (tz * tz)], 1).reshape(-1, 2, 3)
    Rv = torch.tensor([[vm[4 * c_ + r_] for c_ in range(3)] for r_ in range(3)], dtype=dt)
    A = J @ Rv
    cov = A @ V @ A.transpose(1, 2)
    a, b, cc = cov[:, 0, 0] + LOW_PASS, cov[:, 0, 1], cov[:, 1, 1] + LOW_PASS
    det = a * cc - b * b
    conic = torch.stack([cc / det, -b / det, a / det], 1)

    if colors is not None:
        rgb = colors[vis]
    else:
        d = p - torch.tensor(cam["campos"], dtype=dt)
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
    return full(px), full(conic), full(rgb), new_gates, near


def composite(lists, means2D_px, conic, opacity, rgb, bg, W, H, gates=None, band=None):
    """The blend over given lists: lists = (ranges [T,2], point_list [K]) as integer arrays.
    Returns (color [3,H,W], gates, near_gate); gates holds, per tile, the float decisions
    (contributing pairs, capped pairs) of this run.

    band (a run that decides its own gates only): a fourth result, near_px [H,W] bool -- the pixel
    has, up to its termination, a pair with alpha within `band` relative of 1/255, o G within
    `band` relative of 0.99, power in (-0.1 band, 0] or T (1 - alpha) within 100 band relative of
    1e-4: near_gate's four bands in their ratios (1 : 1 : 0.1 : 100), scaled.  near_gate itself
    keeps its bands.  A caller zeroes its image gradients there (frame_grad_scenes)."""
    if band is not None and gates is not None:
        raise ValueError("band: only with this run's own gates")
    near_px = np.zeros((H, W), bool)
    ranges = np.asarray(lists[0]).reshape(-1, 2).astype(np.int64)
    plist = np.asarray(lists[1]).astype(np.int64)
    dt = means2D_px.dtype
    gx = (W + 15) // 16
    bgt = torch.as_tensor(np.asarray(bg, np.float64)).to(dt)
    color = bgt[:, None, None].expand(3, H, W).clone()
    op = opacity.reshape(-1)
    new_gates, near = {}, 0
    for tile, (r0, r1) in enumerate(ranges):
        if r1 <= r0:
            continue
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        xs = torch.arange(x0, min(x0 + 16, W), dtype=dt)
        ys = torch.arange(y0, min(y0 + 16, H), dtype=dt)
        pxx = xs[None, :].expand(len(ys), len(xs)).reshape(-1, 1)
        pyy = ys[:, None].expand(len(ys), len(xs)).reshape(-1, 1)
        ids = torch.as_tensor(plist[r0:r1])
        dx = means2D_px[ids, 0][None, :] - pxx
        dy = means2D_px[ids, 1][None, :] - pyy
        ca, cb, cc = conic[ids, 0][None, :], conic[ids, 1][None, :], conic[ids, 2][None, :]
        power = -0.5 * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
        G = torch.exp(power)
        oG = op[ids][None, :] * G
        if gates is None:
            with torch.no_grad():
                cap = oG > A_CAP
                alpha = torch.where(cap, torch.full_like(oG, A_CAP), oG)
                skip = (power > 0) | (alpha < A_MIN)
                a_eff = torch.where(skip, torch.zeros_like(alpha), alpha)
                T = torch.cumprod(1 - a_eff, 1)
                T = torch.cat([torch.ones_like(T[:, :1]), T[:, :-1]], 1)
                test_T = T * (1 - a_eff)
                term = ~skip & (test_T < T_MIN)
                before = (torch.cumsum(term, 1) - term.long()) == 0  # up to the terminating splat
                contrib = ~skip & (torch.cumsum(term, 1) == 0)
                rel = lambda v, k, e: (v - k).abs() <= e * k  # noqa: E731
                near += int((before & (rel(alpha, A_MIN, 1e-5) | rel(oG, A_CAP, 1e-5) |
                                       ((power > -1e-6) & (power <= 0)) |
                                       (~skip & rel(test_T, T_MIN, 1e-3)))).sum())
                if band is not None:
                    hit = before & (rel(alpha, A_MIN, band) | rel(oG, A_CAP, band) |
                                    ((power > -0.1 * band) & (power <= 0)) |
                                    (~skip & rel(test_T, T_MIN, 100.0 * band)))
                    near_px[y0:y0 + len(ys), x0:x0 + len(xs)] = \
                        hit.any(1).reshape(len(ys), len(xs)).numpy()
        else:
            cap, contrib = gates[tile]
        new_gates[tile] = (cap, contrib)
        alpha = torch.where(cap, torch.full_like(oG, A_CAP), oG)
        a_c = torch.where(contrib, alpha, torch.zeros_like(alpha))
        Tn = torch.cumprod(1 - a_c, 1)
        T = torch.cat([torch.ones_like(Tn[:, :1]), Tn[:, :-1]], 1)
        w = a_c * T
        C = w @ rgb[ids] + Tn[:, -1:] * bgt[None, :]
        color[:, y0:y0 + len(ys), x0:x0 + len(xs)] = C.t().reshape(3, len(ys), len(xs))
    if band is not None:
        return color, new_gates, near, near_px
    return color, new_gates, near


# ---- one scene, both stages, through autograd ---------------------------------------------------
LEAVES = ("means3D", "means2D", "opacity", "scales", "rotations", "cov3D", "shs", "colors")


def leaves(sc, dtype):
    """The differentiable inputs of a grad scene (grad_scenes layout) as leaf tensors."""
    g = sc["s"]["g"]
    P = len(g.xyz)
    src = dict(means3D=g.xyz, means2D=np.zeros((P, 3)), opacity=g.opacity.reshape(P, 1))
    if sc["cov6"] is None:
        src.update(scales=g.scale, rotations=g.rot)
    else:
        src["cov3D"] = sc["cov6"]
    if sc["colors"] is None:
        src["shs"] = g.sh.reshape(P, -1, 3)
    else:
        src["colors"] = sc["colors"]
    return {k: torch.tensor(np.asarray(v, F32).astype(np.float64), dtype=dtype, requires_grad=True)
            for k, v in src.items()}


def scene_gradients(sc, lists, radii, dL, dtype=torch.float64, gates=None):
    """d(sum(color * dL)) / d(every input) of composite(project(...)) for a grad scene, and the
    2D gradients in between (the blend backward's outputs).  gates: (project gates, composite
    gates) of a float64 run.  Returns dict(grads..., gates=, near=(project, composite), color=)."""
    s = sc["s"]
    cam = camera_constants(s)
    lv = leaves(sc, dtype)
    gp, gc = gates if gates is not None else (None, None)
    m2, conic, rgb, gates_p, near_p = project(
        cam, radii, lv["means3D"], lv["means2D"], lv.get("scales"), lv.get("rotations"),
        lv.get("cov3D"), lv.get("shs"), lv.get("colors"), gp)
    for v in (m2, conic, rgb):
        v.retain_grad()
    color, gates_c, near_c = composite(lists, m2, conic, lv["opacity"], rgb, s["bg"], cam["W"],
                                       cam["H"], gc)
    (color * torch.as_tensor(np.asarray(dL, np.float64)).to(dtype)).sum().backward()
    z = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    out = {k: z(v).detach().double().numpy() for k, v in lv.items()}
    out.update(means2D_px=z(m2).double().numpy(), conic=z(conic).double().numpy(),
               rgb=z(rgb).double().numpy(), gates=(gates_p, gates_c), near=(near_p, near_c),
               color=color.detach().double().numpy())
    return out


def rel_err(got, ref):
    """e = max|got - ref| / max|ref| (0 for two all-zero tensors)."""
    ref = np.asarray(ref, np.float64)
    m = float(np.abs(ref).max()) if ref.size else 0.0
    d = float(np.abs(np.asarray(got, np.float64) - ref).max()) if ref.size else 0.0
    return d / m if m > 0 else d


# ---- the tolerance of the GPU tests: measured, not chosen ----------------------------------------
# f: the reference's own float32 spread per gradient tensor -- rel_err of scene_gradients evaluated
# in float32 (gates and lists from the float64 run, so only rounding differs) against float64, the
# largest over the four grad_scenes, measured on the CPU (test_grad_reference.py re-measures it and
# holds these constants to within a factor 2 of what it finds).  The GPU tests allow
# BOUND_FACTOR x f: the margin covers the kernel's different grouping of the pixel sums (lane
# trees, then atomics in arrival order) and its backward reconstruction of T, roundings of the
# same class as f.  A wrong term shows as an error of order 1.
#                                                   S1        S2        S3        S4
F32_SPREAD = {
    "means3D": 4.7e-6,      # 9.1e-7   3.8e-7   4.7e-6   6.8e-7
    "means2D": 7.1e-6,      # 8.9e-7   1.0e-6   7.0e-6   8.2e-7   (upstream's units)
    "means2D_px": 5.3e-6,   # 8.9e-7   5.0e-7   5.3e-6   8.3e-7   (pixels: the blend's own)
    "conic": 1.8e-6,        # 1.7e-6   2.8e-7   5.4e-7   5.1e-7
    "opacity": 6.1e-7,      # 3.6e-7   3.9e-7   6.1e-7   5.6e-7
    "rgb": 1.2e-6,          # 4.8e-7   6.2e-7   1.2e-6   3.4e-7   (dL_dcolors)
    "shs": 6.5e-7,          # 5.0e-7   6.5e-7   -        2.7e-7
    "scales": 1.2e-6,       # 1.2e-6   1.9e-7   -        5.7e-7
    "rotations": 1.3e-6,    # 1.2e-6   1.8e-7   -        1.7e-7
    "cov3D": 2.8e-6,        # -        -        2.8e-6   -
}
F32_SPREAD["colors"] = F32_SPREAD["rgb"]
BOUND_FACTOR = 8.0


def bound(key):
    return BOUND_FACTOR * F32_SPREAD[key]
