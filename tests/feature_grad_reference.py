"""The reference of the feature-channel tests (gsr_forward_features / gsr_backward_features,
include/gsr.h): grad_reference's restatement with C more channels.  CPU only, torch.

No new composite: feature_map[3 j .. 3 j + 2] is gr.composite(lists, m2, conic, opacity,
features[:, 3 j .. 3 j + 2], bg = 0) with the colour run's gates, as plane_grad_reference.planes_of
takes them -- the twin property gsr_forward_features states, three channels at a time (the last
triple padded with zero columns).  The features are a leaf of their own, [P, C].

The loss is sum(color * dL) + sum(planes * dLp) + sum(feature_map * dLf); any of the three may be
None.  The per-Gaussian stage is aa_reference.project (camera_grad_reference's, operation for
operation), so the same function also gives the camera's gradients and the antialiased forward's
for the one case that asks for everything at once.
"""
from __future__ import annotations

import numpy as np
import torch

import aa_reference as ar
import camera_grad_reference as cgr
import grad_reference as gr
import grad_scenes
import plane_grad_reference as pg

F32 = np.float32
CHANNELS = (1, 5, 17)            # the C of the gradient tests: below a triple, odd, several chunks
LOSSES = ("features", "combined")  # features alone (dL_dcolor NULL); colour plus features
ALL_SCENE = "chain"              # ... and on this one everything at once (ALL_C channels)
ALL_C = 5
ZERO_BG = (0.0, 0.0, 0.0)


def feature_rows(name, C):
    """The features of a grad scene: [P, C] float32, standard normal (negatives included)."""
    sc = grad_scenes.get(name)
    rng = np.random.default_rng(300 + 17 * C + grad_scenes.SEEDS[name])
    return np.ascontiguousarray(rng.standard_normal((len(sc["s"]["g"].xyz), C)), F32)


def feature_dL(name, C):
    """The feature planes' gradient of a grad scene: [C, H, W] float32."""
    sc = grad_scenes.get(name)
    rng = np.random.default_rng(400 + 17 * C + grad_scenes.SEEDS[name])
    return np.ascontiguousarray(rng.standard_normal((C, sc["H"], sc["W"])), F32)


def feature_map_of(lists, m2, conic, opacity, feat, W, H, gates):
    """feature_map [C,H,W] of given records and features [P,C]: gr.composite per triple of
    channels with bg = 0 and the given (the colour run's) gates."""
    C = feat.shape[1]
    pad = (-C) % 3
    if pad:
        feat = torch.cat([feat, torch.zeros((feat.shape[0], pad), dtype=feat.dtype)], 1)
    maps = [gr.composite(lists, m2, conic, opacity, feat[:, j:j + 3], ZERO_BG, W, H, gates)[0]
            for j in range(0, C + pad, 3)]
    return torch.cat(maps, 0)[:C]


def scene_gradients(sc, lists, radii, dL, feat, dLf, dLp=None, dtype=torch.float64, gates=None,
                    antialiasing=False):
    """d loss / d(every input of the Gaussians, by gr.LEAVES names), d loss / d features
    (`features`), the 2D gradients in between (means2D_px, conic, rgb) and d(viewmatrix,
    projmatrix, campos) with their error scales `S` (cgr.cam_err), for loss = sum(color * dL) +
    sum(planes * dLp) + sum(feature_map * dLf) (each None = absent).  feat: [P, C] float32 values.
    gates: (project, composite, floor) of a float64 run.  near: (project, composite, floor)."""
    s_in = sc["s"]
    cam = gr.camera_constants(s_in)
    lv = gr.leaves(sc, dtype)
    f = torch.tensor(np.asarray(feat, F32).astype(np.float64), dtype=dtype, requires_grad=True)
    camera = cgr.camera_of(s_in, dtype)
    P = lv["means3D"].shape[0]
    vmP, pmP, cP = (t.reshape(1, -1).expand(P, -1) for t in camera)
    for t in (vmP, pmP, cP):
        t.retain_grad()
    gp, gc, gf = gates if gates is not None else (None, None, None)
    m2, conic, rgb, z, (a0, b, c0, det), gates_p, near_p = ar.project(
        cam, radii, vmP, pmP, cP, lv["means3D"], lv["means2D"], lv.get("scales"),
        lv.get("rotations"), lv.get("cov3D"), lv.get("shs"), lv.get("colors"), gp)
    fac, floor, near_f = ar.factor(a0, b, c0, det, gf)
    if not antialiasing:
        fac, near_f = torch.ones_like(fac), 0
    o_eff = lv["opacity"].reshape(-1) * fac
    for v in (m2, conic, rgb, o_eff):
        v.retain_grad()
    color, gates_c, near_c = gr.composite(lists, m2, conic, o_eff, rgb, s_in["bg"], cam["W"],
                                          cam["H"], gc)
    as_t = lambda v: torch.as_tensor(np.asarray(v, np.float64)).to(dtype)  # noqa: E731
    loss = torch.zeros((), dtype=dtype)
    if dL is not None:
        loss = loss + (color * as_t(dL)).sum()
    if dLp is not None:
        planes, _, _ = pg.planes_of(lists, m2, conic, o_eff, pg.features(z, radii), cam["W"],
                                    cam["H"], gates_c)
        loss = loss + (planes * as_t(dLp)).sum()
    fmap = None
    if dLf is not None:
        fmap = feature_map_of(lists, m2, conic, o_eff, f, cam["W"], cam["H"], gates_c)
        loss = loss + (fmap * as_t(dLf)).sum()
    loss.backward()
    zg = lambda t: torch.zeros_like(t) if t.grad is None else t.grad  # noqa: E731
    out = {k: zg(v).detach().double().numpy() for k, v in lv.items()}
    out["S"] = {}
    for name, t in zip(cgr.CAMERA, (vmP, pmP, cP)):
        G = zg(t).detach().double().numpy()
        out[name] = G.sum(0)
        out["S"][name] = float(np.abs(G).sum(0).max())
    out.update(features=zg(f).detach().double().numpy(), means2D_px=zg(m2).double().numpy(),
               conic=zg(conic).double().numpy(), rgb=zg(rgb).double().numpy(),
               o_eff=zg(o_eff).double().numpy(), gates=(gates_p, gates_c, floor),
               near=(near_p, near_c, near_f), color=color.detach().double().numpy(),
               feature_map=None if fmap is None else fmap.detach().double().numpy())
    return out


def loss_gradients(sc, loss, C):
    """(dL, feat, dLf) of a loss of LOSSES on a grad scene with C channels."""
    return (sc["dL"] if loss == "combined" else None, feature_rows(sc["name"], C),
            feature_dL(sc["name"], C))


# ---- the tolerance of the GPU tests: measured, not chosen ----------------------------------------
# f: gr.rel_err of scene_gradients in float32 (gates and lists of the float64 run) against float64
# per gradient tensor, `features` included, the largest over the two losses of LOSSES (features
# alone; colour plus features), over the C of CHANNELS and over the four grad_scenes (the columns
# below: the largest over losses and C per scene), measured on the CPU with the oracle's lists.
# test_feature_grad_reference.py re-measures it and holds each constant to within a factor 2.  The
# GPU tests allow gr.BOUND_FACTOR x f, for grad_reference's reasons: lane trees, atomics in arrival
# order, T rebuilt by division -- and here the geometry's sums arriving from several launches.
# grad_reference.F32_SPREAD cannot stand in: a standard-normal feature loss weighs other splats
# than the colours in [0, 1] do, and cancels more.
#                                                   S1        S2        S3        S4
F32_SPREAD = {
    "features": 8.7e-7,     # 6.9e-7   3.6e-7   8.7e-7   4.5e-7   (dL_dfeatures)
    "means3D": 3.4e-6,      # 9.0e-7   5.1e-7   3.4e-6   1.4e-6
    "means2D": 3.3e-6,      # 2.1e-6   7.7e-7   3.3e-6   1.0e-6   (upstream's units)
    "means2D_px": 3.0e-6,   # 1.4e-6   5.0e-7   3.0e-6   1.0e-6   (pixels: the blend's own)
    "conic": 1.4e-6,        # 1.4e-6   3.9e-7   7.2e-7   8.3e-7
    "opacity": 1.2e-6,      # 1.2e-6   4.0e-7   6.1e-7   5.8e-7
    "rgb": 1.2e-6,          # 4.8e-7   6.2e-7   1.2e-6   3.3e-7   (dL_dcolors; combined loss only)
    "shs": 6.5e-7,          # 5.0e-7   6.5e-7   -        2.7e-7   (combined loss only)
    "scales": 1.3e-6,       # 1.3e-6   5.7e-7   -        9.7e-7
    "rotations": 1.1e-6,    # 1.1e-6   7.9e-7   -        9.3e-7
    "cov3D": 4.0e-6,        # -        -        4.0e-6   -
}
F32_SPREAD["colors"] = F32_SPREAD["rgb"]

# The same measurement for the one case with everything at once on S1 (ALL_SCENE): colour, the three
# planes (pg.plane_dL), ALL_C feature channels, the antialiased forward, and the camera's three
# gradients on their own scale (cgr.cam_err).
F32_SPREAD_ALL = {
    "features": 5.5e-7, "means3D": 7.6e-7, "means2D": 6.2e-7, "opacity": 4.4e-7, "scales": 7.0e-7,
    "rotations": 7.9e-7, "shs": 4.8e-7, "viewmatrix": 2.2e-7, "projmatrix": 1.4e-7,
    "campos": 2.6e-8,
}


def all_gradients(sc, lists, radii, dtype=torch.float64, gates=None):
    """scene_gradients of the everything-at-once case on ALL_SCENE."""
    return scene_gradients(sc, lists, radii, sc["dL"], feature_rows(sc["name"], ALL_C),
                           feature_dL(sc["name"], ALL_C), pg.plane_dL(sc["name"]), dtype, gates,
                           antialiasing=True)


def err(got, ref, key):
    """The error of one gradient tensor against a scene_gradients result, on its scale."""
    if key in cgr.CAMERA:
        return cgr.cam_err(got, ref, key)
    return gr.rel_err(np.asarray(got, np.float64).reshape(ref[key].shape), ref[key])


def bound(key, table=None):
    return gr.BOUND_FACTOR * (F32_SPREAD if table is None else table)[key]
