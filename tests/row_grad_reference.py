"""A per-row yardstick for the backward pass: every word of every gradient row is held to a scale of
its own, not to the largest entry of its tensor.  CPU only, float64; no tests here
(test_row_grad_reference.py pins this file, test_gpu_row_gradients.py holds the kernels to it).

grad_reference.rel_err = max|got - ref| / max|ref| is a norm-wise bound: a row five decades below
the tensor's maximum may be zero, doubled or sign-flipped within it, and the rows of a 3DGS
gradient span seven to eight decades ("Every gradient row against its own bound").
The unit of a word here is the sum of the absolute values of what is added to it:

  blend_sums(...)    the blend's backward restated in closed form, per tile over (pixels x list
                     positions) in numpy: per Gaussian and per word of the 2D gradients (means2D_px
                     2, conic 3, opacity 1, rgb 3, and with planes depths 1) the signed sum over
                     pixels of the pixel's contribution and A, the sum of the absolute values of
                     those contributions, on the decisions (gates) grad_reference.composite returned
  pixel_terms(...)   the same contributions from batched autograd of the per-pixel loss (toy scenes)
  scales(...)        A pushed through the per-Gaussian stage: each row of project depends on its own
                     inputs only, so one backward pass per output word with a one-hot grad_outputs
                     over all rows gives every row's Jacobian J_i, and S3d = |J_i|^T A2d_i
  row_err(...)       max |got - ref| / S over the words with S > 0, and whether got == 0.0 exactly
                     wherever S == 0

The unit.  A pixel's contribution to the geometry and the opacity goes through d loss / d alpha =
T s - (sum of the later positions' w s + final_T bg . dL) / (1 - alpha), s = dL . feature: itself a
difference of sums over channels and list positions, which a float32 evaluation rounds one by one.
A row that one or two pixels composite and whose pixel term cancels is therefore not within an
epsilon of A (frame has such a row at 1.1e-4 of A, a hundred times the others), so S takes the
pixel term's own addends by their absolute values too: blend_sums returns it beside A as `S`, equal
to A for rgb and depths (single products) and >= A elsewhere.  A stays what the sums are checked
against autograd in; S is what scales() pushes through the per-Gaussian stage and what row_err
divides by.

With planes the loss is plane_grad_reference's: depth_map, inv_depth_map and final_T are three more
channels of the composite with features (z, 1 / z, 0) and background (0, 0, 1); the depth word adds
the two feature channels' sums at z, and its A adds their absolute sums (the two channels are summed
over pixels apart before they meet, as autograd and the kernels do).
"""
from __future__ import annotations

import numpy as np
import torch

import grad_reference as gr
import plane_grad_reference as pg

WORDS = {"means2D_px": 2, "conic": 3, "opacity": 1, "rgb": 3, "depths": 1}
FLOOR = float(np.finfo(np.float32).tiny)  # the one absolute floor: a device may flush subnormals


def _np(v):
    return v.detach().double().numpy() if isinstance(v, torch.Tensor) else np.asarray(v, np.float64)


def _tiles(lists, W, H):
    ranges = np.asarray(lists[0]).reshape(-1, 2).astype(np.int64)
    plist = np.asarray(lists[1]).astype(np.int64)
    gx = (W + 15) // 16
    for tile, (r0, r1) in enumerate(ranges):
        if r1 <= r0:
            continue
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        w, h = min(16, W - x0), min(16, H - y0)
        yield tile, plist[r0:r1], x0, y0, w, h


def _channels(rec, bg, dL, dLp, z, x0, y0, w, h, ids):
    """(F [n,C], B [C], D [N,C], colour channels): the composite's features, background and image
    gradients of one tile; C = 3 (colour), 3 (planes) or 6."""
    F, B, D = [], [], []
    nc = 0
    if dL is not None:
        F.append(rec[3][ids])
        B.append(np.asarray(bg, np.float64))
        D.append(dL[:, y0:y0 + h, x0:x0 + w].reshape(3, -1).T)
        nc = 3
    if dLp is not None:
        zi = z[ids]
        safe = np.where(zi != 0, zi, 1.0)
        F.append(np.stack([zi, np.where(zi != 0, 1.0 / safe, 0.0), np.zeros_like(zi)], 1))
        B.append(np.asarray(pg.PLANE_BG, np.float64))
        D.append(dLp[:, y0:y0 + h, x0:x0 + w].reshape(3, -1).T)
    return np.concatenate(F, 1), np.concatenate(B), np.concatenate(D, 1), nc


def _tile_terms(rec, ids, cap, con, x0, y0, w, h, F, B, D):
    """The per-(pixel, position) contributions of one tile: dict word -> [N,n] (conic: three,
    means2D_px: two), and `w` = alpha T of the contributing pairs."""
    m2, conic, op = rec[0], rec[1], rec[2]
    xs, ys = np.arange(x0, x0 + w, dtype=np.float64), np.arange(y0, y0 + h, dtype=np.float64)
    pxx = np.broadcast_to(xs[None, :], (h, w)).reshape(-1, 1)
    pyy = np.broadcast_to(ys[:, None], (h, w)).reshape(-1, 1)
    dx, dy = m2[ids, 0][None, :] - pxx, m2[ids, 1][None, :] - pyy
    ca, cb, cc = conic[ids, 0][None, :], conic[ids, 1][None, :], conic[ids, 2][None, :]
    power = -0.5 * (ca * dx * dx + cc * dy * dy) - cb * dx * dy
    live = con & ~cap  # alpha = o G: the geometry and the opacity receive a gradient
    with np.errstate(over="ignore", invalid="ignore"):
        G = np.where(live, np.exp(np.where(live, power, 0.0)), 0.0)
    a = np.where(con, np.where(cap, gr.A_CAP, op[ids][None, :] * G), 0.0)
    Tn = np.cumprod(1.0 - a, 1)
    T = np.concatenate([np.ones_like(Tn[:, :1]), Tn[:, :-1]], 1)
    wgt = a * T
    s = D @ F.T
    ws = wgt * s
    after = np.cumsum(ws[:, ::-1], 1)[:, ::-1] - ws + Tn[:, -1:] * (D @ B)[:, None]
    g = np.where(live, T * s - after / (1.0 - a), 0.0)  # d loss / d alpha of the pair
    hh = a * g                                           # d loss / d power
    # the same with every addend of g taken by its absolute value: channel by channel, position by
    # position (module docstring, "the unit")
    sa = np.abs(D) @ np.abs(F).T
    wsa = wgt * sa
    after_a = np.cumsum(wsa[:, ::-1], 1)[:, ::-1] - wsa + Tn[:, -1:] * (np.abs(D) @ np.abs(B))[:, None]
    ga = np.where(live, T * sa + after_a / (1.0 - a), 0.0)
    ha = a * ga
    fine = dict(opacity=[G * ga],
                means2D_px=[ha * (np.abs(ca * dx) + np.abs(cb * dy)),
                            ha * (np.abs(cc * dy) + np.abs(cb * dx))],
                conic=[0.5 * ha * dx * dx, ha * np.abs(dx * dy), 0.5 * ha * dy * dy])
    return dict(opacity=[G * g],
                means2D_px=[-hh * (ca * dx + cb * dy), -hh * (cc * dy + cb * dx)],
                conic=[-0.5 * hh * dx * dx, -hh * dx * dy, -0.5 * hh * dy * dy],
                w=wgt, fine=fine)


def blend_sums(lists, rec, gates, W, H, bg, dL, dLp=None, z=None, drop_last=False, keep=False):
    """The blend's backward per Gaussian and word.  rec = (means2D_px, conic, opacity, rgb) as
    frame_grad_scenes.records hands them; gates = grad_reference.composite's of that run (per tile:
    capped pairs, contributing pairs); dL [3,H,W] or None, dLp [3,H,W] or None (then z [P], the
    view depths, is needed).
    Returns dict(sum={word: [P,k]}, A={word: [P,k]}, S={word: [P,k]}, tile=[P], pos=[P]): S is
    the unit (module docstring); tile and pos are the tile, and the list position in it, whose
    pixels add the largest share of the row's colour and plane sums (-1: the row gets nothing).
    drop_last: every pixel's last contributing list position adds nothing (a mutation of
    test_row_grad_reference.py).  keep: also `terms`, per tile (ids, {word: [k,N,n]})."""
    rec = tuple(_np(v).reshape(len(_np(rec[0])), -1) if i != 2 else _np(v).reshape(-1)
                for i, v in enumerate(rec))
    P = len(rec[0])
    dL = None if dL is None else np.asarray(dL, np.float64)
    dLp = None if dLp is None else np.asarray(dLp, np.float64)
    z = None if z is None else _np(z).reshape(-1)
    words = [k for k in WORDS if k != "depths" or dLp is not None]
    out_s = {k: np.zeros((P, WORDS[k])) for k in words}
    out_a = {k: np.zeros((P, WORDS[k])) for k in words}
    out_f = {k: np.zeros((P, WORDS[k])) for k in words}
    best = np.zeros(P)
    best_tile, best_pos = np.full(P, -1), np.full(P, -1)
    terms = {}
    for tile, ids, x0, y0, w, h in _tiles(lists, W, H):
        cap, con = (_g.numpy() for _g in gates[tile])
        F, B, D, nc = _channels(rec, bg, dL, dLp, z, x0, y0, w, h, ids)
        t = _tile_terms(rec, ids, cap, con, x0, y0, w, h, F, B, D)
        feat = [t["w"] * D[:, c][:, None] for c in range(D.shape[1])]
        if nc:
            t["rgb"] = feat[:3]
        else:
            t["rgb"] = [np.zeros_like(t["w"])] * 3
        use = np.ones_like(con)
        if drop_last:
            n = con.shape[1]
            last = np.where(con, np.arange(n)[None, :], -1).max(1)
            use = np.arange(n)[None, :] != last[:, None]
        for k in ("means2D_px", "conic", "opacity", "rgb"):
            for c, v in enumerate(t[k]):
                out_s[k][ids, c] += (v * use).sum(0)
                out_a[k][ids, c] += (np.abs(v) * use).sum(0)
                out_f[k][ids, c] += (t["fine"].get(k, [np.abs(x) for x in t[k]])[c] * use).sum(0)
        if dLp is not None:
            zi = z[ids]
            dz, dinv = feat[nc], feat[nc + 1]
            out_s["depths"][ids, 0] += (dz * use).sum(0) - (dinv * use).sum(0) / (zi * zi)
            out_a["depths"][ids, 0] += (np.abs(dz) * use).sum(0) + (np.abs(dinv) * use).sum(0) / (zi * zi)
            t["depths"] = [dz - dinv / (zi * zi)[None, :]]
        share = sum(np.abs(v).sum(0) for v in feat)
        better = share > best[ids]
        best[ids] = np.where(better, share, best[ids])
        best_tile[ids] = np.where(better, tile, best_tile[ids])
        best_pos[ids] = np.where(better, np.arange(len(ids)), best_pos[ids])
        if keep:
            terms[tile] = (ids, {k: np.stack(t[k]) for k in words})
    if dLp is not None:
        out_f["depths"] = out_a["depths"].copy()
    out = dict(sum=out_s, A=out_a, S=out_f, tile=best_tile, pos=best_pos)
    if keep:
        out["terms"] = terms
    return out


def pixel_terms(lists, rec, gates, W, H, bg, dL, dLp=None, z=None):
    """blend_sums' `terms` from autograd: every (pixel, position) pair of a tile gets leaves of its
    own, the tile's loss is composited from them by grad_reference.composite's formulas, and one
    backward pass leaves each pair's contribution in its leaf's gradient.  Toy scenes only."""
    t64 = lambda v: torch.as_tensor(_np(v))  # noqa: E731
    m2, conic, op, rgb = (t64(v) for v in rec)
    op = op.reshape(-1)
    out = {}
    for tile, ids, x0, y0, w, h in _tiles(lists, W, H):
        cap, con = gates[tile]
        N, n = con.shape
        F, B, D, nc = _channels((None, None, None, _np(rgb)), bg,
                                None if dL is None else np.asarray(dL, np.float64),
                                None if dLp is None else np.asarray(dLp, np.float64),
                                None if z is None else _np(z).reshape(-1), x0, y0, w, h, ids)
        per = lambda v: v[None, :].expand(N, n).clone().requires_grad_(True)  # noqa: E731
        lv = dict(mx=per(m2[ids, 0]), my=per(m2[ids, 1]), ca=per(conic[ids, 0]),
                  cb=per(conic[ids, 1]), cc=per(conic[ids, 2]), op=per(op[ids]))
        feat = [per(torch.as_tensor(F[:, c])) for c in range(F.shape[1])]
        xs = torch.arange(x0, x0 + w, dtype=torch.float64)
        ys = torch.arange(y0, y0 + h, dtype=torch.float64)
        dx = lv["mx"] - xs[None, :].expand(h, w).reshape(-1, 1)
        dy = lv["my"] - ys[:, None].expand(h, w).reshape(-1, 1)
        power = -0.5 * (lv["ca"] * dx * dx + lv["cc"] * dy * dy) - lv["cb"] * dx * dy
        oG = lv["op"] * torch.exp(power)
        alpha = torch.where(cap, torch.full_like(oG, gr.A_CAP), oG)
        a_c = torch.where(con, alpha, torch.zeros_like(alpha))
        Tn = torch.cumprod(1 - a_c, 1)
        T = torch.cat([torch.ones_like(Tn[:, :1]), Tn[:, :-1]], 1)
        wgt = a_c * T
        Dt, Bt = torch.as_tensor(D), torch.as_tensor(B)
        loss = sum((Dt[:, c] * ((wgt * feat[c]).sum(1) + Tn[:, -1] * Bt[c])).sum()
                   for c in range(F.shape[1]))
        loss.backward()
        g = lambda v: torch.zeros(N, n, dtype=torch.float64) if v.grad is None else v.grad  # noqa: E731
        t = dict(means2D_px=torch.stack([g(lv["mx"]), g(lv["my"])]).numpy(),
                 conic=torch.stack([g(lv["ca"]), g(lv["cb"]), g(lv["cc"])]).numpy(),
                 opacity=g(lv["op"])[None].numpy(),
                 rgb=(torch.stack([g(f) for f in feat[:3]]).numpy() if nc
                      else np.zeros((3, N, n))))
        if dLp is not None:
            # the planes' features are functions of z: d z = 1, d (1 / z) = -1 / z^2
            zi = torch.as_tensor(_np(z).reshape(-1)[ids])
            t["depths"] = (g(feat[nc]) - g(feat[nc + 1]) / (zi * zi)[None, :])[None].numpy()
        out[tile] = (ids, t)
    return out


# ---- the per-Gaussian stage -----------------------------------------------------------------------
STAGE_KEYS = ("means3D", "means2D", "opacity", "scales", "rotations", "shs", "cov3D", "colors")


def scales(sc, radii, A2d):
    """S per word of every gradient the backward returns, from the blend's A2d (blend_sums' A):
    the 2D words keep A2d; a 3D word gets sum over the 2D words of |d word2D / d word3D| A2d, the
    Jacobian of grad_reference.project (and, with `depths` in A2d, of the view depth) row by row.
    Keys: the 2D words, and means3D, means2D (upstream's units), opacity [P,1], scales, rotations,
    shs, cov3D, colors as the scene has them."""
    cam = gr.camera_constants(sc["s"])
    lv = gr.leaves(sc, torch.float64)
    m2, conic, rgb, _, _ = gr.project(cam, radii, lv["means3D"], lv["means2D"], lv.get("scales"),
                                      lv.get("rotations"), lv.get("cov3D"), lv.get("shs"),
                                      lv.get("colors"))
    outs = [(m2, "means2D_px"), (conic, "conic"), (rgb, "rgb")]
    if "depths" in A2d:
        outs.append((pg.view_depth(cam, radii, lv["means3D"])[:, None], "depths"))
    keys = [k for k in STAGE_KEYS if k in lv and k != "opacity"]
    S = {k: np.zeros(tuple(lv[k].shape)) for k in keys}
    for out, word in outs:
        for c in range(out.shape[1]):
            hot = torch.zeros_like(out)
            hot[:, c] = 1.0
            grads = torch.autograd.grad(out, [lv[k] for k in keys], hot, retain_graph=True,
                                        allow_unused=True)
            for k, g in zip(keys, grads):
                if g is not None:
                    a = A2d[word][:, c].reshape((-1,) + (1,) * (g.dim() - 1))
                    S[k] += np.abs(g.numpy()) * a
    S["opacity"] = A2d["opacity"].reshape(-1, 1).copy()
    for k, v in A2d.items():
        S[k] = v
    return S


def reference(sc, lists, radii, dL, dLp=None, dtype=torch.float64, gates=None):
    """The scene's gradients through autograd: grad_reference.scene_gradients for the colour loss,
    plane_grad_reference.scene_gradients with the planes."""
    if dLp is None:
        return gr.scene_gradients(sc, lists, radii, dL, dtype, gates)
    return pg.scene_gradients(sc, lists, radii, dL, dLp, dtype, gates)


def scene_scales(sc, lists, radii, dL, dLp=None, ref=None, drop_last=False):
    """(ref, sums, S) of a scene end to end: the float64 reference (computed unless given), the
    blend's closed-form sums on float64 project's records under the reference's own gates, and S per
    key.  S["tile"], S["pos"]: blend_sums' report of where a row's largest addends come from."""
    if ref is None:
        ref = reference(sc, lists, radii, dL, dLp)
    cam = gr.camera_constants(sc["s"])
    with torch.no_grad():
        lv = gr.leaves(sc, torch.float64)
        m2, conic, rgb, _, _ = gr.project(cam, radii, lv["means3D"], lv["means2D"],
                                          lv.get("scales"), lv.get("rotations"), lv.get("cov3D"),
                                          lv.get("shs"), lv.get("colors"))
        z = pg.view_depth(cam, radii, lv["means3D"])
    sums = blend_sums(lists, (m2, conic, lv["opacity"], rgb), ref["gates"][1], cam["W"], cam["H"],
                      sc["s"]["bg"], dL, dLp, z, drop_last=drop_last)
    S = scales(sc, radii, sums["S"])
    S["tile"], S["pos"] = sums["tile"], sums["pos"]
    return ref, sums, S


def row_err(got, ref, S):
    """(e, index, zeros): e = max |got - ref| / S over the words with S > 0 (differences below the
    smallest normal float32 count as none), the index of the worst word in the tensor's shape, and
    whether got == 0.0 exactly wherever S == 0.  No word is left out."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64).reshape(ref.shape)
    S = np.asarray(S, np.float64).reshape(ref.shape)
    on = S > 0
    d = np.maximum(np.abs(got - ref) - FLOOR, 0.0)
    r = np.where(on, d / np.where(on, S, 1.0), 0.0)
    if not np.isfinite(got).all():
        r = np.where(np.isfinite(got), r, np.inf)
    i = np.unravel_index(int(np.argmax(r)), r.shape) if r.size else ()
    return (float(r[i]) if r.size else 0.0), i, bool((got[~on] == 0.0).all())


# ---- the scenes ------------------------------------------------------------------------------------
# The smallest that reach the tails: grad_scenes' four, frame_grad_scenes' wall and frame (under
# their masks) and long_lists through pose_scenes' dense rotation.
SCENES = ("chain", "long_lists", "precomputed", "edges", "wall", "frame", "long_lists@oblique")


def case(name):
    """(sc, dL, dLp) of one of SCENES: the scene and the image gradients the row tests feed (the
    frame scenes': masked)."""
    import frame_grad_scenes as fs
    import grad_scenes
    import pose_scenes as ps
    if name in fs.NAMES:
        sc = fs.get(name)
        return (sc,) + fs.masked(sc)
    if "@" in name:
        sc = ps.get(*name.split("@"))
        return sc, sc["dL"], ps.plane_dL(sc)
    sc = grad_scenes.get(name)
    return sc, sc["dL"], pg.plane_dL(name)


# ---- the tolerance of the GPU tests: measured, not chosen ------------------------------------------
# ROW_SPREAD[key]: the reference's own float32 spread in units of S -- row_err of `reference`
# evaluated in float32 (lists and gates of the float64 run, so only rounding differs) against
# float64, the largest over SPREAD_SCENES and over the colour loss and colour + planes, measured on
# the CPU with the oracle's lists (test_row_grad_reference.py re-measures it and holds every
# constant to within a factor 2).  The GPU tests allow grad_reference.BOUND_FACTOR x it, per word.
# `frame` sets every constant but two: its lists are the deepest (T is a product of up to 258 rounded
# factors) and its pixel coordinates the largest, and a row that one pixel composites has no other
# addends to average over.
# (columns: chain, long_lists, precomputed, edges, wall, frame, long_lists@oblique; the larger of
# the two losses)
ROW_SPREAD = {
    "means3D": 4.5e-6,      # 3.4e-7  2.4e-7  6.1e-7  2.9e-7  4.7e-7  4.5e-6  1.9e-7
    "means2D": 4.9e-6,      # 3.4e-7  2.4e-7  6.1e-7  3.0e-7  4.8e-7  4.9e-6  2.4e-7   (upstream's units)
    "means2D_px": 4.9e-6,   # 3.4e-7  2.4e-7  6.1e-7  3.0e-7  4.8e-7  4.9e-6  2.4e-7   (pixels)
    "conic": 8.9e-6,        # 4.3e-7  3.3e-7  7.6e-7  6.1e-7  8.6e-7  8.9e-6  7.5e-7
    "opacity": 7.3e-6,      # 5.3e-7  2.4e-7  7.5e-7  5.7e-7  5.7e-7  7.3e-6  3.8e-7
    "rgb": 2.2e-5,          # 1.3e-6  6.3e-7  9.2e-7  1.4e-6  1.5e-6  2.2e-5  1.1e-6   (dL_dcolors)
    "depths": 1.7e-5,       # 1.6e-6  4.4e-7  1.4e-6  8.0e-7  1.2e-6  1.7e-5  6.4e-7   (planes only)
    "shs": 3.7e-5,          # 1.8e-6  9.2e-7  -       1.1e-6  9.3e-6  3.7e-5  3.5e-6
    "scales": 7.1e-6,       # 2.3e-7  4.0e-7  -       4.0e-7  7.1e-6  5.5e-6  1.9e-6
    "rotations": 5.0e-6,    # 2.3e-7  2.6e-7  -       4.1e-7  6.9e-7  5.0e-6  2.3e-7
    "cov3D": 3.8e-7,        # -       -       3.8e-7  -       -       -       -
    "colors": 9.2e-7,       # -       -       9.2e-7  -       -       -       -
}


def bound(key):
    return gr.BOUND_FACTOR * ROW_SPREAD[key]
