"""The frame-scale scenes of the backward-pass tests (test_frame_grad_reference.py on the CPU,
test_gpu_backward_frames.py on the GPU): the smallest frames that reach the paths of the backward
the toy scenes of grad_scenes cannot -- not the workload's sizes.  Layout of grad_scenes (s,
colors, cov6, W, H, dL, special).

  frame  200 x 136 px = 13 x 9 tiles, the last column 8 px wide and the last row 8 px high, so
         their outer quadrants lie wholly outside the image; P = 6,000, SH degree 3, bg (0.3, 0.6,
         0.1); more than 2,048 Gaussians kept, lists beyond 256 entries (five chunks); the first
         four Gaussians are large and faint and sit in every one of the 117 lists: hundreds of
         waves add to their gradient rows
  wall   32 x 32 px (4 tiles), P = 420: a near layer of 120 (the first 120 of every list) in front
         of 300 faint ones, with a gap on the right.  Behind the layer pixels terminate in chunk 0
         or 1 of lists of seven chunks, so waves stop early, at differing chunks; in the gap
         pixels run to the end of their list, and at its edge both kinds share a quadrant
  wide   4112 x 24 px = 257 x 2 tiles (more than 256 tile columns: the per-pair binning form, whose
         point list holds plain ids in row-major tile order), the lower row 8 px high; P = 3,000
         small Gaussians over the width
  tall   24 x 4112 px = 2 x 257 tiles, the transpose of wide (more than 256 tile rows: the per-pair
         form again, now for its rows), the right column 8 px wide; pixel y up to 4111 in the
         blend and its backward; P = 3,000 small Gaussians over the height.  The camera keeps its
         vertical field of view, so a pixel is 1 / 1696 world units here: the centres' spread and
         the sizes are wide's in pixels (14 px either side of the short axis' centre), the sizes
         1 .. 4 px

The seeds are chosen so that grad_reference.project finds no Gaussian within rounding of a gate
(asserted).  The composite's gates cannot be kept clear at this size -- `frame` has about 7 M
(pixel, splat) pairs and, whichever seed, some tens within grad_reference's bands -- so the scenes
mask instead: the image gradients are zeroed at every pixel with a pair inside BAND of a gate up
to the pixel's termination (grad_reference.composite's near_px).  Every term a pixel adds to any
sum is proportional to its own image gradient, so a masked pixel adds exactly nothing, whichever
way the device decides its gate, and the check stays strict everywhere else.  The mask is the
union over the records a test may composite: float64 project's, the C oracle's float32 ones (what
the device's forward holds, bit for bit), both again with the antialiased opacity (`frame`), and
every pixel where the float64 decisions on those two sets of records differ.
"""
from __future__ import annotations

import numpy as np
import torch

import aa_reference as ar
import camera_grad_reference as cgr
import grad_reference as gr
import grad_scenes
import oracle
from gaussiansplattingviewer_amd.camera import cuda_camera_inputs, static_camera
from gpu_helpers import run_oracle, scene_inputs

F32 = np.float32
NAMES = ("frame", "wall", "wide", "tall")
SEEDS = {"frame": 1, "wall": 2, "wide": 3, "tall": 0}
AA_SCENES = ("frame",)  # the scenes a test runs antialiased
BIG = 4                 # frame: the large, faint Gaussians
FRONT = 120             # wall: the near layer

# ---- the mask band: measured, not chosen ----------------------------------------------------------
# ALPHA_F32_SPREAD: the largest relative difference in alpha = o G between a float32 and a float64
# evaluation of grad_reference.composite's formula on the oracle's float32 records, over all (pixel,
# splat) pairs of the four scenes with alpha within a factor 2 of 1/255, measured on the CPU
# (alpha_spread; test_frame_grad_reference.py re-measures it and holds the constant to within a
# factor 2).  BAND = 8 x that, the project's margin for the kernel's rounding, which is of this
# class; the power and T gates keep grad_reference's ratios to it (0.1 x and 100 x).
#                                  frame     wall      wide      tall
ALPHA_F32_SPREAD = 1.3e-5        # 1.3e-5    1.2e-6    1.2e-6    2.6e-6
BAND = gr.BOUND_FACTOR * ALPHA_F32_SPREAD
MASK_CAP = 0.10           # at most this share of a scene's pixels masked ...
QUADRANT_KEEP = 0.5       # ... and every quadrant keeps at least this share of its pixels inside


def build(name):
    rng = np.random.default_rng(SEEDS[name])
    special = {}
    if name == "frame":
        W, H, D, bg = 200, 136, 3, (0.3, 0.6, 0.1)
        g = grad_scenes._gaussians(rng, 6000, 3.2, 2.2, 0.03, 0.2, 0.05, 0.9)
        g.scale[:BIG] = rng.uniform(1.0, 2.0, (BIG, 3))
        g.opacity[:BIG] = rng.uniform(0.02, 0.08, (BIG, 1))
        g.xyz[:BIG] = rng.uniform(-0.5, 0.5, (BIG, 3))
        special["big"] = np.arange(BIG)
    elif name == "wall":
        W, H, D, bg = 32, 32, 3, (0.2, 0.4, 0.6)
        g = grad_scenes._gaussians(rng, 420, 1.3, 1.3, 0.35, 0.7, 0.004, 0.02)
        g.xyz[:, 2] = rng.uniform(-1.0, 0.3, 420)
        # the near layer: in front of everything, left of x = 0.35 (the gap is to its right)
        # and in two sheets: the nearer 84 over one half of the height, so that they fill chunk 0 of
        # every list and end their own half's pixels there; the other 36 behind them over the
        # other half, which end theirs in chunk 1
        n, na = FRONT, 84
        g.xyz[:n, 0] = rng.uniform(-1.4, 0.35, n)
        g.xyz[:na, 1] = rng.uniform(-1.3, 0.1, na)
        g.xyz[na:n, 1] = rng.uniform(0.0, 1.3, n - na)
        g.xyz[:na, 2] = rng.uniform(0.9, 1.0, na)
        g.xyz[na:n, 2] = rng.uniform(0.8, 0.88, n - na)
        g.scale[:n] = rng.uniform(0.3, 0.5, (n, 3))
        g.opacity[:n] = rng.uniform(0.6, 0.95, (n, 1))
        special["front"] = np.arange(n)
    elif name == "wide":
        W, H, D, bg = 4112, 24, 3, (0.2, 0.4, 0.6)
        tx = float(cuda_camera_inputs(static_camera(W, H))[3])  # tan of half the horizontal fov
        g = grad_scenes._gaussians(rng, 3000, 4.0 * tx, 1.4, 0.01, 0.04, 0.1, 0.9)
    elif name == "tall":
        W, H, D, bg = 24, 4112, 3, (0.2, 0.4, 0.6)
        ty = float(cuda_camera_inputs(static_camera(W, H))[4])  # tan of half the vertical fov
        u = 8.0 * ty / H  # world units per pixel at the origin's depth
        g = grad_scenes._gaussians(rng, 3000, 14.0 * u, 4.0 * ty, 1.0 * u, 4.0 * u, 0.1, 0.9)
    else:
        raise KeyError(name)
    s = scene_inputs(g, static_camera(W, H), D, bg=bg, scale_modifier=1.0)
    dL = np.ascontiguousarray(rng.standard_normal((3, H, W)), F32)
    dLp = np.ascontiguousarray(rng.standard_normal((3, H, W)), F32)
    return dict(name=name, s=s, colors=None, cov6=None, W=W, H=H, dL=dL, dLp=dLp, special=special)


_cache = {}


def get(name):
    if name not in _cache:
        _cache[name] = build(name)
    return _cache[name]


# ---- the oracle's integers and float32 records, and the float64 records ---------------------------
def oracle_of(sc):
    """The C oracle's forward of a scene (lists, radii, float32 records), once per scene."""
    if "orc" not in sc:
        sc["orc"] = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"],
                               cov3D_precomp=sc["cov6"])
    return sc["orc"]


def lists_of(sc):
    orc = oracle_of(sc)
    return orc["ranges"], orc["point_list"]


def records(sc):
    """Per set of records a test composites, (means2D_px, conic, opacity, rgb) as float64 tensors:
    "f64" project's, "f32" the oracle's, and for AA_SCENES "f64aa" / "f32aa", the same with the
    antialiased opacity (float64's, and float64's rounded to float32 beside the float32 records).
    Also asserts project's near-gate count of 0."""
    if "records" in sc:
        return sc["records"]
    orc = oracle_of(sc)
    t = lambda a: torch.tensor(np.asarray(a, F32).astype(np.float64))  # noqa: E731
    with torch.no_grad():
        lv = gr.leaves(sc, torch.float64)
        cam = gr.camera_constants(sc["s"])
        P = lv["means3D"].shape[0]
        vmP, pmP, cP = (v.reshape(1, -1).expand(P, -1) for v in cgr.camera_of(sc["s"]))
        m2, conic, rgb, _, (a0, b, c0, det), _, near = ar.project(
            cam, orc["radii"], vmP, pmP, cP, lv["means3D"], lv["means2D"], lv["scales"],
            lv["rotations"], None, lv["shs"])
        assert near == 0, near
        op = lv["opacity"].reshape(-1)
        out = {"f64": (m2, conic, op, rgb),
               "f32": (t(orc["means2D"]), t(orc["conic_opacity"][:, :3]),
                       t(orc["conic_opacity"][:, 3]), t(orc["rgb"]))}
        if sc["name"] in AA_SCENES:
            fac, _, near_f = ar.factor(a0, b, c0, det)
            assert near_f == 0, near_f
            o_eff = op * fac
            out["f64aa"] = (m2, conic, o_eff, rgb)
            out["f32aa"] = out["f32"][:2] + (o_eff.float().double(), out["f32"][3])
    sc["records"] = out
    return out


def decisions(sc):
    """Per set of records: grad_reference.composite's float64 gates (per tile: capped pairs,
    contributing pairs), and near_px at BAND."""
    if "decisions" not in sc:
        out = {}
        with torch.no_grad():
            for key, rec in records(sc).items():
                _, gates, _, near_px = gr.composite(lists_of(sc), *rec, sc["s"]["bg"], sc["W"],
                                                    sc["H"], band=BAND)
                out[key] = (gates, near_px)
        sc["decisions"] = out
    return sc["decisions"]


def _differ(sc, gates_a, gates_b):
    """[H,W] bool: a contributing pair, or the cap of one, differs between two runs' gates."""
    W, H = sc["W"], sc["H"]
    gx = (W + 15) // 16
    out = np.zeros((H, W), bool)
    for tile, (cap_a, con_a) in gates_a.items():
        cap_b, con_b = gates_b[tile]
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        w, h = min(16, W - x0), min(16, H - y0)
        d = ((con_a != con_b) | ((cap_a != cap_b) & con_a)).any(1)
        out[y0:y0 + h, x0:x0 + w] = d.reshape(h, w).numpy()
    return out


def mask(sc):
    """[H,W] bool, the pixels whose image gradients the tests zero (module docstring)."""
    if "mask" not in sc:
        dec = decisions(sc)
        m = np.zeros((sc["H"], sc["W"]), bool)
        for _, near_px in dec.values():
            m |= near_px
        m |= _differ(sc, dec["f64"][0], dec["f32"][0])
        if "f64aa" in dec:
            m |= _differ(sc, dec["f64aa"][0], dec["f32aa"][0])
        sc["mask"] = m
    return sc["mask"]


def masked(sc, planes=True):
    """(dL, dLp) of the scene with the masked pixels zeroed (dLp None without planes)."""
    keep = (~mask(sc)).astype(F32)[None]
    return sc["dL"] * keep, (sc["dLp"] * keep if planes else None)


def localized(sc, tile_x, tile_y, quad):
    """The masked dL, zero outside one 8 x 8 quadrant (quad = 2 qy + qx of the tile)."""
    dL, _ = masked(sc, planes=False)
    x0, y0 = 16 * tile_x + 8 * (quad & 1), 16 * tile_y + 8 * (quad >> 1)
    out = np.zeros_like(dL)
    out[:, y0:y0 + 8, x0:x0 + 8] = dL[:, y0:y0 + 8, x0:x0 + 8]
    assert np.abs(out).max() > 0
    return out


def quadrants(sc):
    """(ids [H,W] int, n): the 8 x 8 quadrant of every pixel, numbered over the grid of quadrants
    with a pixel inside the image."""
    ys, xs = np.mgrid[0:sc["H"], 0:sc["W"]]
    qx = (sc["W"] + 7) // 8
    ids = (ys // 8) * qx + xs // 8
    return ids, qx * ((sc["H"] + 7) // 8)


def outside_quadrants(sc):
    """The (tile, quadrant) pairs of the tile grid that lie wholly outside the image."""
    gx, gy = (sc["W"] + 15) // 16, (sc["H"] + 15) // 16
    return [(t, q) for t in range(gx * gy) for q in range(4)
            if (t % gx) * 16 + (q & 1) * 8 >= sc["W"] or (t // gx) * 16 + (q >> 1) * 8 >= sc["H"]]


def alpha_spread(sc):
    """The measurement behind ALPHA_F32_SPREAD on one scene: max |alpha32 - alpha64| / alpha64
    over the pairs of the lists with alpha64 in [1/510, 2/255], alpha = o G evaluated by composite's
    formula in each dtype on the oracle's float32 records."""
    ranges, plist = lists_of(sc)
    ranges = np.asarray(ranges).reshape(-1, 2).astype(np.int64)
    plist = np.asarray(plist).astype(np.int64)
    W, H = sc["W"], sc["H"]
    gx = (W + 15) // 16
    worst = 0.0
    rec = {dt: tuple(v.to(dt) for v in records(sc)["f32"][:3]) for dt in (torch.float32, torch.float64)}
    for tile, (r0, r1) in enumerate(ranges):
        if r1 <= r0:
            continue
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        ids = torch.as_tensor(plist[r0:r1])
        oG = {}
        for dt, (m2, conic, op) in rec.items():
            xs = torch.arange(x0, min(x0 + 16, W), dtype=dt)
            ys = torch.arange(y0, min(y0 + 16, H), dtype=dt)
            pxx = xs[None, :].expand(len(ys), len(xs)).reshape(-1, 1)
            pyy = ys[:, None].expand(len(ys), len(xs)).reshape(-1, 1)
            dx, dy = m2[ids, 0][None, :] - pxx, m2[ids, 1][None, :] - pyy
            power = -0.5 * (conic[ids, 0][None, :] * dx * dx + conic[ids, 2][None, :] * dy * dy) \
                - conic[ids, 1][None, :] * dx * dy
            oG[dt] = (op[ids][None, :] * torch.exp(power)).double()
        a64 = oG[torch.float64]
        sel = (a64 >= 0.5 * gr.A_MIN) & (a64 <= 2.0 * gr.A_MIN)
        if sel.any():
            worst = max(worst, float(((oG[torch.float32] - a64).abs() / a64)[sel].max()))
    return worst


def stops(sc):
    """Per (tile, quadrant) with pixels inside the image, from the float64 decisions on project's
    records: dict(chunks = chunks of the tile's list, last = the chunk of the last contributing
    list position over the quadrant's pixels (-1: none), walked = the chunks a wave walks before all
    its pixels have terminated (chunks if one never does), terminated / running = pixels that
    terminate / that run to the end of the list)."""
    ranges = np.asarray(lists_of(sc)[0]).reshape(-1, 2).astype(np.int64)
    rec = records(sc)["f64"]
    plist = np.asarray(lists_of(sc)[1]).astype(np.int64)
    W, H = sc["W"], sc["H"]
    gx = (W + 15) // 16
    gates = decisions(sc)["f64"][0]
    out = {}
    for tile, (cap, con) in gates.items():
        r0, r1 = ranges[tile]
        n = int(r1 - r0)
        x0, y0 = (tile % gx) * 16, (tile // gx) * 16
        w, h = min(16, W - x0), min(16, H - y0)
        # the terminating splat, restated: the first non-skipped pair after the last contributing
        # one whose T (1 - alpha) < 1e-4 -- composite's own rule, from its formula
        ids = torch.as_tensor(plist[r0:r1])
        xs = torch.arange(x0, x0 + w, dtype=torch.float64)
        ys = torch.arange(y0, y0 + h, dtype=torch.float64)
        pxx = xs[None, :].expand(h, w).reshape(-1, 1)
        pyy = ys[:, None].expand(h, w).reshape(-1, 1)
        m2, conic, op, _ = rec
        dx, dy = m2[ids, 0][None, :] - pxx, m2[ids, 1][None, :] - pyy
        power = -0.5 * (conic[ids, 0][None, :] * dx * dx + conic[ids, 2][None, :] * dy * dy) \
            - conic[ids, 1][None, :] * dx * dy
        alpha = torch.clamp(op[ids][None, :] * torch.exp(power), max=gr.A_CAP)
        skip = (power > 0) | (alpha < gr.A_MIN)
        a_c = torch.where(con, alpha, torch.zeros_like(alpha))
        T = torch.cumprod(1 - a_c, 1)
        T = torch.cat([torch.ones_like(T[:, :1]), T[:, :-1]], 1)
        term = ~skip & ~con & (T * (1 - alpha) < gr.T_MIN)
        pos = torch.arange(n)[None, :]
        term_pos = torch.where(term, pos, torch.full_like(pos, n)).min(1).values.reshape(h, w).numpy()
        last_pos = torch.where(con, pos, torch.full_like(pos, -1)).max(1).values.reshape(h, w).numpy()
        chunks = (n + 63) // 64
        for q in range(4):
            qx0, qy0 = 8 * (q & 1), 8 * (q >> 1)
            if qx0 >= w or qy0 >= h:
                continue
            tp = term_pos[qy0:qy0 + 8, qx0:qx0 + 8]
            lp = last_pos[qy0:qy0 + 8, qx0:qx0 + 8]
            done = tp < n
            out[(tile, q)] = dict(chunks=chunks, last=int(lp.max()) // 64 if lp.max() >= 0 else -1,
                                  walked=int(tp.max()) // 64 + 1 if done.all() else chunks,
                                  terminated=int(done.sum()), running=int((~done).sum()))
    return out


def composited(sc):
    """[P] bool: some pixel composites the Gaussian, by the float64 decisions on any set of
    records."""
    ranges = np.asarray(lists_of(sc)[0]).reshape(-1, 2).astype(np.int64)
    plist = np.asarray(lists_of(sc)[1]).astype(np.int64)
    out = np.zeros(len(sc["s"]["g"].xyz), bool)
    for gates, _ in decisions(sc).values():
        for tile, (_, con) in gates.items():
            out[plist[ranges[tile][0]:ranges[tile][1]][con.any(0).numpy()]] = True
    return out


# ---- the references --------------------------------------------------------------------------------
def reference(sc, kind, dtype=torch.float64, gates=None):
    """The reference gradients of a scene on the oracle's lists and radii under the masked image
    gradients: "colour" -- grad_reference.scene_gradients; "all" -- colour + the three planes + the
    camera, camera_grad_reference.scene_gradients; "all_aa" -- the same antialiased,
    aa_reference.scene_gradients.  The float64 results are kept per scene."""
    key = "ref_" + kind
    if dtype == torch.float64 and key in sc:
        return sc[key]
    lists, radii = lists_of(sc), oracle_of(sc)["radii"]
    dL, dLp = masked(sc)
    if kind == "colour":
        out = gr.scene_gradients(sc, lists, radii, dL, dtype, gates)
    elif kind == "all":
        out = cgr.scene_gradients(sc, lists, radii, dL, dLp, dtype, gates)
    else:
        out = ar.scene_gradients(sc, lists, radii, dL, dLp, dtype, gates)
    if dtype == torch.float64:
        sc[key] = out
    return out


# (scene, tile column, tile row, quadrant) of the localised image gradients: the single inside
# quadrant of frame's bottom-right tile, a quadrant of a middle tile, one in tile column 256
# of wide, and of tall one in the first tile row, one in a middle row of the 8 px wide right
# column and one in the last, tile row 256
PLACEMENTS = (("frame", 12, 8, 0), ("frame", 6, 4, 3), ("wide", 256, 0, 3),
              ("tall", 0, 0, 1), ("tall", 1, 128, 2), ("tall", 0, 256, 3))


def localized_reference(sc, tile_x, tile_y, quad, dtype=torch.float64, gates=None):
    """grad_reference.scene_gradients under localized(...): the colour loss of one quadrant.  Only
    that tile's list is composited (the other pixels' image gradients are zero)."""
    ranges, plist = lists_of(sc)
    tile = tile_y * ((sc["W"] + 15) // 16) + tile_x
    only = np.zeros_like(np.asarray(ranges).reshape(-1, 2))
    only[tile] = np.asarray(ranges).reshape(-1, 2)[tile]
    return gr.scene_gradients(sc, (only, plist), oracle_of(sc)["radii"],
                              localized(sc, tile_x, tile_y, quad), dtype, gates)


def err(got, ref, key):
    """The error of one gradient tensor against a reference: cgr.cam_err for the camera's three,
    gr.rel_err for the others."""
    return ar.err(got, ref, key)


# ---- the tolerance of the GPU tests: measured, not chosen ------------------------------------------
# f: the reference's own float32 spread per gradient tensor and scene -- gr.rel_err (the camera's
# three: cgr.cam_err) of `reference` evaluated in float32 against float64, lists and gates of the
# float64 run, masked image gradients -- measured on the CPU with the oracle's lists
# (test_frame_grad_reference.py re-measures it and holds each constant to within a factor 2).  The
# GPU tests allow gr.BOUND_FACTOR x f of the scene they run, for grad_reference's reasons.  The toy
# scenes' constants cannot stand in: `wide` computes pixel distances at coordinates up to 4112,
# where a float32 holds 2.4e-4 px, and its spread is that much larger.
F32_SPREAD = {
    # the colour loss, grad_reference.scene_gradients
    ("frame", "colour"): {"means3D": 2.5e-6, "means2D": 1.9e-6, "means2D_px": 2.7e-6,
                          "conic": 5.6e-7, "opacity": 6.2e-7, "rgb": 6.8e-7, "shs": 7.8e-7,
                          "scales": 1.7e-6, "rotations": 2.5e-6},
    ("wall", "colour"): {"means3D": 4.5e-7, "means2D": 3.3e-7, "means2D_px": 3.3e-7,
                         "conic": 3.9e-7, "opacity": 3.1e-7, "rgb": 4.4e-7, "shs": 4.6e-7,
                         "scales": 6.7e-7, "rotations": 6.9e-7},
    ("wide", "colour"): {"means3D": 8.4e-5, "means2D": 4.6e-4, "means2D_px": 6.7e-5,
                         "conic": 7.5e-6, "opacity": 3.1e-5, "rgb": 3.5e-5, "shs": 3.2e-5,
                         "scales": 2.8e-5, "rotations": 2.0e-5},
    # (pixel distances at y up to 4111, as wide's at x)
    ("tall", "colour"): {"means3D": 9.7e-5, "means2D": 1.1e-4, "means2D_px": 1.1e-4,
                         "conic": 7.0e-5, "opacity": 7.1e-5, "rgb": 4.1e-5, "shs": 3.9e-5,
                         "scales": 5.5e-5, "rotations": 4.9e-5},
    # colour + the three planes + the camera, camera_grad_reference.scene_gradients
    ("frame", "all"): {"means3D": 2.1e-6, "means2D": 1.7e-6, "opacity": 7.5e-7, "shs": 7.8e-7,
                       "scales": 1.0e-6, "rotations": 4.3e-6, "viewmatrix": 9.5e-8,
                       "projmatrix": 8.2e-8, "campos": 1.1e-7},
    # ... antialiased, aa_reference.scene_gradients
    ("frame", "all_aa"): {"means3D": 2.4e-6, "means2D": 2.0e-6, "opacity": 7.7e-7, "shs": 7.5e-7,
                          "scales": 1.1e-6, "rotations": 3.0e-6, "viewmatrix": 7.2e-8,
                          "projmatrix": 1.0e-7, "campos": 7.4e-8},
    # the colour loss of one quadrant (localized_reference), the larger over the scene's PLACEMENTS
    ("frame", "local"): {"means3D": 3.2e-6, "means2D": 3.2e-6, "means2D_px": 3.2e-6,
                         "conic": 9.3e-7, "opacity": 1.7e-6, "rgb": 1.0e-6, "shs": 1.1e-6,
                         "scales": 2.0e-6, "rotations": 2.5e-6},
    ("wide", "local"): {"means3D": 3.2e-5, "means2D": 3.3e-5, "means2D_px": 1.3e-5,
                        "conic": 2.3e-5, "opacity": 5.4e-6, "rgb": 8.7e-6, "shs": 8.7e-6,
                        "scales": 2.3e-5, "rotations": 2.4e-5},
    ("tall", "local"): {"means3D": 1.6e-4, "means2D": 2.7e-4, "means2D_px": 1.8e-4,
                        "conic": 1.5e-4, "opacity": 3.7e-5, "rgb": 5.1e-5, "shs": 5.1e-5,
                        "scales": 1.5e-4, "rotations": 7.7e-5},
}
for _t in F32_SPREAD.values():
    if "rgb" in _t:
        _t["colors"] = _t["rgb"]


def bound(name, kind, key):
    return gr.BOUND_FACTOR * F32_SPREAD[(name, kind)][key]
