"""The reference of the absolute means2D gradient (gsr_backward_abs, include/gsr.h):
grad_reference's restatement differentiated pixel by pixel.  CPU only, torch; no tests here
(test_absgrad_reference.py pins this file, test_gpu_absgrad.py holds the kernels to it).

dL_dmeans2D is the gradient of the loss sum_p l(p), l(p) = sum_c color[c, p] dL[c, p] (+ the planes'
terms sum_k planes[k, p] dLp[k, p], plane_grad_reference's channels), with respect to the pixel
centre means2D_px, times (0.5 W, 0.5 H).  The absolute gradient takes each pixel's share by its
absolute value before the sum over pixels:

    means2D_abs[i] = (0.5 W sum_p |d l(p) / d means2D_px[i, 0]|, 0.5 H sum_p |... [i, 1]|, 0)

l(p) is the pixel's total over every channel of the call, so one backward pass per pixel (batched
here) through grad_reference.composite gives the addends; the integer decisions (lists, radii) are
given and the float gates are the float64 run's, as everywhere.
"""
from __future__ import annotations

import numpy as np
import torch

import grad_reference as gr
import plane_grad_reference as pg

BATCH = 128  # pixels per batched backward pass


def pixel_gradients(sc, lists, radii, dL, dLp=None, dtype=torch.float64, gates=None):
    """d l(p) / d means2D_px for every pixel p of a grad scene: [H * W, P, 2] in `dtype` (row-major
    pixels), with the run's gates.  dL [3,H,W] or None, dLp [3,H,W] (depth, inverse depth, final_T)
    or None; gates: (project gates, composite gates) of a float64 run.
    Returns dict(per_pixel=, gates=, near=(project, composite))."""
    s = sc["s"]
    cam = gr.camera_constants(s)
    W, H = cam["W"], cam["H"]
    gp, gc = gates if gates is not None else (None, None)
    with torch.no_grad():
        lv = gr.leaves(sc, dtype)
        m2, conic, rgb, gates_p, near_p = gr.project(
            cam, radii, lv["means3D"], lv["means2D"], lv.get("scales"), lv.get("rotations"),
            lv.get("cov3D"), lv.get("shs"), lv.get("colors"), gp)
        z = pg.view_depth(cam, radii, lv["means3D"])
        opacity = lv["opacity"].detach()
    m2 = m2.clone().requires_grad_(True)
    color, gates_c, near_c = gr.composite(lists, m2, conic, opacity, rgb, s["bg"], W, H, gc)
    as_t = lambda a: torch.as_tensor(np.asarray(a, np.float64)).to(dtype)  # noqa: E731
    loss = torch.zeros((H, W), dtype=dtype)
    if dL is not None:
        loss = loss + (color * as_t(dL)).sum(0)
    if dLp is not None:
        planes, _, _ = pg.planes_of(lists, m2, conic, opacity, pg.features(z, radii), W, H,
                                    gates_c)
        loss = loss + (planes * as_t(dLp)).sum(0)
    flat = loss.reshape(-1)
    N = flat.numel()
    out = np.zeros((N,) + tuple(m2.shape), np.float32 if dtype == torch.float32 else np.float64)
    for b0 in range(0, N, BATCH):
        n = min(BATCH, N - b0)
        hot = torch.zeros((n, N), dtype=dtype)
        hot[torch.arange(n), b0 + torch.arange(n)] = 1.0
        (g,) = torch.autograd.grad(flat, m2, hot, retain_graph=True, is_grads_batched=True)
        out[b0:b0 + n] = g.numpy()
    return dict(per_pixel=out, gates=(gates_p, gates_c), near=(near_p, near_c))


def units(sc):
    """k_preprocess_bwd's factors from pixels to upstream's units: (0.5 W, 0.5 H)."""
    return np.array([0.5 * sc["W"], 0.5 * sc["H"]])


def scene_abs_gradients(sc, lists, radii, dL, dLp=None, dtype=torch.float64, gates=None):
    """The reference of one call: dict(means2D_abs [P,3] (the output: upstream's units, z = 0),
    means2D_signed [P,3] (the same sums with their signs: dL_dmeans2D), means2D_px_signed [P,2]
    (pixels: scene_gradients' means2D_px), gates=, near=), float64 arrays.  The addends, their
    absolute values and the sums over pixels are all formed in `dtype`."""
    r = pixel_gradients(sc, lists, radii, dL, dLp, dtype, gates)
    pp = r["per_pixel"]
    P = pp.shape[1]
    u = units(sc)
    out_abs, out_signed = np.zeros((P, 3)), np.zeros((P, 3))
    out_abs[:, :2] = (np.abs(pp).sum(0) * u.astype(pp.dtype)).astype(np.float64)
    out_signed[:, :2] = (pp.sum(0) * u.astype(pp.dtype)).astype(np.float64)
    return dict(means2D_abs=out_abs, means2D_signed=out_signed,
                means2D_px_signed=pp.sum(0).astype(np.float64),
                gates=r["gates"], near=r["near"])


def row_err(got, ref):
    """(e, row): e = max over the words with ref > 0 of |got - ref| / ref -- every word against its
    own value, which is already the sum of its addends' magnitudes (row_grad_reference's unit) --
    and the row of the worst word; inf if got != 0.0 anywhere ref == 0."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    on = ref > 0
    r = np.where(on, np.abs(got - ref) / np.where(on, ref, 1.0), 0.0)
    r = np.where(~on & (got != 0.0), np.inf, r)
    i = np.unravel_index(int(np.argmax(r)), r.shape)
    return float(r[i]), int(i[0])


# ---- the losses and the tolerance of the GPU tests: measured, not chosen ---------------------------
# the (scene, loss) pairs the GPU tests feed: the colour loss on the four grad_scenes, and on S1 the
# colour with the three planes ("combined") and the planes alone (plane_grad_reference's losses)
CASES = (("chain", "colour"), ("long_lists", "colour"), ("precomputed", "colour"),
         ("edges", "colour"), ("chain", "combined"), ("chain", "planes"))


def loss_gradients(sc, loss):
    """(dL, dLp) of one of CASES' losses."""
    if loss == "colour":
        return sc["dL"], None
    return pg.loss_gradients(sc, loss)


# f: the reference's own float32 spread for means2D_abs -- scene_abs_gradients with the addends
# evaluated in float32 (lists and gates of the float64 run, so only rounding differs) against
# float64, the largest over CASES, measured on the CPU with the oracle's lists
# (test_absgrad_reference.py re-measures both and holds each constant to within a factor 2):
#   F32_SPREAD  per tensor, gr.rel_err: max|got - ref| / max|ref|
#   ROW_SPREAD  per row, row_err: every word against its own value
# The GPU tests allow gr.BOUND_FACTOR x f, for grad_reference's reasons.
#                         chain   long_lists  precomputed  edges  chain/combined  chain/planes
F32_SPREAD = 6.2e-7     # 6.2e-7  3.4e-7      4.5e-7      3.3e-7  5.1e-7          3.6e-7
ROW_SPREAD = 4.0e-6     # 4.0e-6  1.5e-6      1.9e-6      2.4e-6  3.3e-6          3.4e-6


def bound():
    return gr.BOUND_FACTOR * F32_SPREAD


def row_bound():
    return gr.BOUND_FACTOR * ROW_SPREAD


def spread(sc, lists, radii, loss, ref64=None):
    """(per tensor, per row): the measurement behind F32_SPREAD and ROW_SPREAD for one case."""
    dL, dLp = loss_gradients(sc, loss)
    if ref64 is None:
        ref64 = scene_abs_gradients(sc, lists, radii, dL, dLp)
    r32 = scene_abs_gradients(sc, lists, radii, dL, dLp, torch.float32, ref64["gates"])
    return (gr.rel_err(r32["means2D_abs"], ref64["means2D_abs"]),
            row_err(r32["means2D_abs"], ref64["means2D_abs"])[0])


# ---- the cancellation the output exists for -------------------------------------------------------
def cancellation_scene():
    """One isotropic Gaussian (equal scales, identity rotation, SH degree 0) at the world origin of
    a 16 x 16 frame -- one tile, whose centre (7.5, 7.5) it projects to -- under an image gradient
    that is even in x and y about that centre: pixel (x, y)'s term of dL_dmeans2D is the negative
    of pixel (15 - x, y)'s in x and of (x, 15 - y)'s in y, so the signed sums cancel while the
    absolute ones add up.  A grad scene (grad_scenes' layout)."""
    from gaussiansplattingviewer_amd.camera import static_camera
    from gaussiansplattingviewer_amd.gaussian_data import GaussianData
    from gpu_helpers import scene_inputs
    a = lambda v: np.ascontiguousarray(v, np.float32)  # noqa: E731
    sh = np.zeros((1, 48))
    sh[0, :3] = (0.4, -0.2, 0.9)
    g = GaussianData(a(np.zeros((1, 3))), a([[1.0, 0.0, 0.0, 0.0]]), a(np.full((1, 3), 0.5)),
                     a([[0.6]]), a(sh))
    s = scene_inputs(g, static_camera(16, 16), 0, bg=(0.3, 0.6, 0.1))
    rng = np.random.default_rng(11)
    q = rng.standard_normal((3, 8, 8))
    top = np.concatenate([q, q[:, :, ::-1]], 2)
    dL = np.ascontiguousarray(np.concatenate([top, top[:, ::-1, :]], 1), np.float32)
    return dict(name="cancellation", s=s, colors=None, cov6=None, W=16, H=16, dL=dL, special={})


CANCEL_RATIO = 1e-3  # |dL_dmeans2D| <= CANCEL_RATIO x dL_dmeans2D_abs in x and y on that scene
