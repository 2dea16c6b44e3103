"""Small scenes that put the per-Gaussian stage (csrc/preprocess.hip: k_preprocess<false/true>,
k_color, k_color_generic, k_color_ids) on its decisions, where the synthetic clouds of the other
tests never are; shared by the CPU checks (test_preprocess_reference.py) and the GPU checks
(test_gpu_preprocess_edges.py).

Frames are at most 160x120 and scenes at most 600 Gaussians.  Every scene but `boundaries_*`
(ordinary throughout) also holds N_ORD ordinary synthetic_gaussians interleaved by index with
the special ones (sc["special"] marks those), so a wave and a tile list always mix both: a
culled or poisoned neighbour must not disturb them.

  near_plane        160x120, rotated and translated view from an eye 0.1 off the origin: view
                    depth (float32 transform_point_4x3) is exactly float32(0.2), its two float
                    neighbours on either side, float32(0.2000001), 0.25 and 1; small scales
  clamp             160x120: t.x / t.z and t.y / t.z at 0.99, 1 (and x, y one and two floats
                    either side of it), 1.01, 2 and 10 times 1.3 tanfov, both signs; scales so
                    large that every rect still reaches the frame
  rect_edges_WxH    1x1, 16x16, 17x9, 33x31, cov3D_precomp + colors_precomp, radius 9: px - r,
                    px + r + 15 (and the same in y) at a multiple of 16 -- 0, 16, 16 grid (a rect
                    that starts at the grid's end, from outside), and a rect that ends exactly at
                    column / row 0 from outside (negative px) -- on the nearest float32 centre
                    below, at (where one exists) and above it
  radius_ceil       160x120, isotropic 2D covariances at the jump of ceil(3 sqrt(lambda)) from k
                    to k + 1, k = 3..40 (lambda = sigma^2 + 0.3 + sqrt(0.1): upstream's 0.1 floor
                    under the root adds sqrt(0.1) for an isotropic splat): the two float32
                    covariances below the jump and the two above it
  det_cancel        160x120, elongated covariances a c ~ b^2 at 1e6..1e8 px^2 whose float32 det
                    is 0, a rounding granule either side of it, or small and positive
  scale_range_mS    scale_modifier 0, 0.7, 100: scales 0, 1e-30, 1e-20, 1e-3, 1, 1e3, 1e8, 1e15,
                    negative scales, the zero quaternion, quaternions of norm 0.3 and 2
  nonfinite         NaN, +inf, -inf in exactly one of xyz, scale, rot, opacity, SH
  nonfinite_precomp the same in one entry of cov3D_precomp (colors_precomp)
  sh_edges_D_M      every (D, M) with (D + 1)^2 <= M, M in 1, 4, 9, 16: directions along each
                    axis from campos, a mean equal to campos (len = 0), a channel exactly -0.5
                    before the + 0.5 (and one float either side), coefficients of 1e30 (opacity
                    below 1/255: the colour is compared, the image never sees it)
  boundaries_P      P in 1, 63, 64, 65, 255, 256, 257, 513 ordinary Gaussians, a third culled
"""
from __future__ import annotations

import numpy as np

from gaussiansplattingviewer_amd.camera import cuda_camera_inputs, static_camera
from gaussiansplattingviewer_amd.gaussian_data import GaussianData, synthetic_gaussians

import blend_scenes as bs
from gpu_helpers import run_oracle, scene_inputs

F32 = np.float32
BG = (0.2, 0.4, 0.6)
N_ORD = 50
INT_MAX = 2**31 - 1
RECT_FRAMES = ((1, 1), (16, 16), (17, 9), (33, 31))
RECT_R = 9
SCALE_MODS = {"m0": 0.0, "m07": 0.7, "m100": 100.0}
SH_PAIRS = tuple((d, m) for m in (1, 4, 9, 16) for d in range(4) if (d + 1) ** 2 <= m)
BOUNDARY_PS = (1, 63, 64, 65, 255, 256, 257, 513)
NAMES = (("near_plane", "clamp") + tuple(f"rect_edges_{w}x{h}" for w, h in RECT_FRAMES) +
         ("radius_ceil", "det_cancel") + tuple(f"scale_range_{k}" for k in SCALE_MODS) +
         ("nonfinite", "nonfinite_precomp") + tuple(f"sh_edges_{d}_{m}" for d, m in SH_PAIRS) +
         tuple(f"boundaries_{p}" for p in BOUNDARY_PS))
# The scenes whose threshold is the point: held to the order-exact check only (their decisions
# sit on their thresholds by construction, so a float64 evaluation cannot decide them).
THRESHOLD_BUILT = ("near_plane", "rect_edges", "radius_ceil", "det_cancel")


# Scenes whose blend is held to the oracle's image only, not to its float64 reference too
# (gpu_helpers.assert_blend_exact needs finite records, and pixels whose decisions float32 can
# make: test_preprocess_reference.py shows the list is exactly the scenes that lack either).
BLEND_NOT_EXACT = {
    "scale_range_m07": "NaN conics (det = inf - inf)",
    "scale_range_m100": "NaN conics (det = inf - inf)",
    "nonfinite": "NaN and infinite opacities",
    "nonfinite_precomp": "NaN conics",
}


def assert_bits_or_nan(got, want, what=""):
    """Float arrays equal bit for bit where `want` is not NaN, and NaN where it is (x86 and the
    GPU produce different NaN sign and payload bits)."""
    got = np.ascontiguousarray(got, F32)
    want = np.ascontiguousarray(want, F32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    bad = np.where(nan, ~np.isnan(got), got.view(np.uint32) != want.view(np.uint32))
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} values differ, first at {i}: "
                             f"got {got[i]!r} ({got.view(np.uint32)[i]:#010x}), want {want[i]!r} "
                             f"({want.view(np.uint32)[i]:#010x})")


def ulp_steps(v, steps):
    """float32 v moved by each of `steps` (ints) places along the float32 number line."""
    i = np.asarray(v, F32).reshape(()).view(np.int32).astype(np.int64)
    key = (-(i & 0x7FFFFFFF) if i < 0 else i) + np.asarray(steps, np.int64)
    bits = np.where(key < 0, (-key) | 0x80000000, key)
    return bits.astype(np.uint32).view(F32)


def _ordinary(n, seed, M=16):
    g = synthetic_gaussians(n, 3, seed)
    g.sh = np.ascontiguousarray(g.sh[:, :3 * M])
    return g


def _interleave(ns, no):
    """Order that spreads `no` ordinary entries evenly among `ns` special ones (specials first in
    the concatenation); returns (order, special mask in the new order)."""
    pos = np.concatenate([(np.arange(ns) + 0.25) / max(ns, 1), (np.arange(no) + 0.5) / max(no, 1)])
    order = np.argsort(pos, kind="stable")
    return order, order < ns


def _mixed(name, cam, D, sp: GaussianData, seed, scale_modifier=1.0, colors=None, cov6=None,
           oracle=None, campos=None):
    """Scene of the special Gaussians `sp` (with their colours / cov6 where the scene uses the
    precomputed inputs) interleaved with N_ORD ordinary ones."""
    M = sp.sh.shape[1] // 3
    od = _ordinary(N_ORD, seed, M)
    order, special = _interleave(len(sp), N_ORD)
    cat = lambda a, b: np.ascontiguousarray(np.concatenate([a, b])[order], F32)  # noqa: E731
    g = GaussianData(cat(sp.xyz, od.xyz), cat(sp.rot, od.rot), cat(sp.scale, od.scale),
                     cat(sp.opacity, od.opacity), cat(sp.sh, od.sh))
    rng = np.random.default_rng(seed + 1)
    if colors is not None:
        colors = cat(colors, rng.uniform(0, 1, (N_ORD, 3)))
    if cov6 is not None:
        cov6 = cat(cov6, oracle.cov3d(od.scale, od.rot))
    s = scene_inputs(g, cam, D, bg=BG, scale_modifier=scale_modifier)
    if campos is not None:
        s["campos"] = np.asarray(campos, F32)
    return dict(name=name, s=s, colors=colors, cov6=cov6, W=cam.w, H=cam.h, special=special)


def _plain(n, rng, M=16, scale=0.02, opacity=0.6):
    """n Gaussians with identity rotation, one scale, one opacity and ordinary SH rows."""
    sh = np.concatenate([rng.normal(0, 0.6, (n, 3)), rng.normal(0, 0.05, (n, 3 * (M - 1)))], 1)
    return GaussianData(np.zeros((n, 3), F32), np.tile(F32([1, 0, 0, 0]), (n, 1)),
                        np.full((n, 3), scale, F32), np.full((n, 1), opacity, F32),
                        np.ascontiguousarray(sh, F32))


def run(oracle, sc):
    """The oracle's forward of a scene, computed once per scene and kept in it (rgb zeroed with
    precomputed colours: neither side computes it then)."""
    if "orc" not in sc:
        orc = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"], cov3D_precomp=sc["cov6"])
        if sc["colors"] is not None:
            orc["rgb"] = np.zeros_like(orc["rgb"])
        sc["orc"] = orc
    return sc["orc"]


def features(sc, orc):
    return orc["rgb"] if sc["colors"] is None else sc["colors"]


def view_z32(xyz, vm):
    """upstream transformPoint4x3's z in float32, in its order, for rows of xyz (float32)."""
    x, y, z = (np.ascontiguousarray(xyz[:, k], F32) for k in range(3))
    vm = np.asarray(vm, F32).reshape(-1)
    return ((vm[2] * x + vm[6] * y) + vm[10] * z) + vm[14]


NEAR_T0 = F32(0.2)
NEAR_TARGETS = tuple(ulp_steps(NEAR_T0, [-2, -1, 0, 1, 2])) + (F32(0.2000001), F32(0.25), F32(1.0))
NEAR_LATERAL = ((0.0, 0.0), (0.25, 0.15), (-0.25, 0.15), (0.25, -0.15), (-0.25, -0.15), (0.1, -0.2))


def _near_plane():
    W, H = 160, 120
    cam = static_camera(W, H, eye=(0.06, -0.04, 0.07))
    view = cuda_camera_inputs(cam)[0]
    V = view.T.astype(np.float64)  # math layout: p_view = V [p, 1]
    Rm, tr = V[:3, :3], V[:3, 3]
    ax = np.argsort(-np.abs(V[2, :3]))  # the world axes by their weight in view z
    s0 = np.arange(-4000, 4001)
    s1 = np.arange(-8, 9)
    xyz, want = [], []
    for d in NEAR_TARGETS:
        for lx, ly in NEAR_LATERAL:
            # the mean in float64, then nudged by ulps until the float32 view depth lands on d
            p = (Rm.T @ (np.array([lx * d, ly * d, float(d)]) - tr)).astype(F32)
            cand = np.repeat(p[None], len(s0) * len(s1), axis=0)
            cand[:, ax[0]] = np.repeat(ulp_steps(p[ax[0]], s0), len(s1))
            cand[:, ax[1]] = np.tile(ulp_steps(p[ax[1]], s1), len(s0))
            hit = np.flatnonzero(view_z32(cand, view) == d)
            assert len(hit), f"near_plane: no float32 mean at view depth {d!r}"
            best = hit[np.argmin(np.abs(s0[hit // len(s1)]) + np.abs(s1[hit % len(s1)]))]
            xyz.append(cand[best])
            want.append(d)
    n = len(xyz)
    rng = np.random.default_rng(7)
    sp = _plain(n, rng)
    sp.xyz = np.asarray(xyz, F32)
    q = rng.standard_normal((n, 4))
    sp.rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    sp.scale = rng.uniform(0.0005, 0.002, (n, 3)).astype(F32)  # <= 6 px radius at depth 0.2
    sc = _mixed("near_plane", cam, 3, sp, 101)
    sc["depth_targets"] = np.asarray(want, F32)
    return sc


CLAMP_RATIOS = (0.99, 1.0, 1.01, 2.0, 10.0)


def _clamp():
    W, H = 160, 120
    cam = static_camera(W, H)
    _, _, _, tx, ty = cuda_camera_inputs(cam)
    lim = (float(F32(1.3) * F32(tx)), float(F32(1.3) * F32(ty)))
    xyz, scale = [], []
    d = 4.0  # view depth of world z = 0; view x = -world x, view y = world y
    for axis in (0, 1):
        for sign in (-1.0, 1.0):
            for r in CLAMP_RATIOS:
                p = np.zeros(3, F32)
                p[axis] = sign * r * lim[axis] * d
                # ratio 1: also one and two floats either side of the solved coordinate
                for st in ((-2, -1, 0, 1, 2) if r == 1.0 else (0,)):
                    q = p.copy()
                    q[axis] = ulp_steps(p[axis], [st])[0]
                    s = np.full(3, 0.05)
                    s[axis] = 0.4 * r * lim[axis] * d + 0.05  # 3 sigma = 1.2 x the centre's offset
                    s[2] = s[axis]  # and as deep: the clamped t enters through J's third column
                    xyz.append(q)
                    scale.append(s)
    n = len(xyz)
    rng = np.random.default_rng(8)
    sp = _plain(n, rng, opacity=0.1)
    sp.xyz, sp.scale = np.asarray(xyz, F32), np.asarray(scale, F32)
    sp.opacity = rng.uniform(0.05, 0.3, (n, 1)).astype(F32)
    return _mixed("clamp", cam, 3, sp, 102)


def _cov6_px(cov_px, depth, H):
    """cov3D rows (x-y plane, zz ~ 0) of 2D covariances in px^2 at a view depth, as
    blend_scenes._splats scales them."""
    cov = np.asarray(cov_px, np.float64).reshape(-1, 3) * (depth / bs._focal(H)) ** 2
    c6 = np.zeros((len(cov), 6), F32)
    c6[:, 0], c6[:, 1], c6[:, 3], c6[:, 5] = cov[:, 0], cov[:, 1], cov[:, 2], 1e-8
    return c6


def _world_xy(W, H, px, py, depth=4.0):
    f = bs._focal(H)
    return np.stack([(np.asarray(px, np.float64) - (W - 1) / 2.0) * depth / f,
                     -(np.asarray(py, np.float64) - (H - 1) / 2.0) * depth / f,
                     np.full(np.shape(px), 4.0 - depth)], axis=-1).astype(F32)


def rect_targets(W, H):
    """(axis, target centre, what) of rect_edges: where px - r or px + r + 15 is a multiple of 16."""
    r = RECT_R
    out = []
    for axis, g in ((0, (W + 15) // 16), (1, (H + 15) // 16)):
        for m in sorted({0, 1, g}):
            out.append((axis, 16.0 * m + r, f"lo=16*{m}"))       # px - r = 16 m
            out.append((axis, 16.0 * m - 15 - r, f"hi=16*{m}"))  # px + r + 15 = 16 m
    return out


def _rect_edges(oracle, W, H):
    name = f"rect_edges_{W}x{H}"
    sigma2 = 2.7 ** 2  # ceil(3 sqrt(7.29 + 0.3 + sqrt(0.1))) = 9
    steps = np.arange(-300, 301)
    tg = rect_targets(W, H)
    mid = ((W - 1) / 2.0, (H - 1) / 2.0)
    cand, owner = [], []
    for k, (axis, t, _) in enumerate(tg):
        c = [mid[0], mid[1]]
        c[axis] = t
        p = _world_xy(W, H, c[0], c[1])
        q = np.repeat(p[None], len(steps), axis=0)
        # world steps of a quarter of the centre's float32 spacing (not ulps of the world
        # coordinate, which is 0 for a centre on the optical axis)
        h = 0.25 * float(np.spacing(F32(max(abs(t), 1.0)))) * 4.0 / bs._focal(H)
        q[:, axis] = (float(p[axis]) + steps * h).astype(F32)
        cand.append(q)
        owner += [k] * len(steps)
    cand, owner = np.concatenate(cand), np.asarray(owner)
    # the float32 centres of all candidates: one oracle preprocess with a radius that keeps every
    # candidate's rect in the frame
    big = bs._scene(W, H, cand, np.ones(len(cand)), np.ones((len(cand), 3), F32),
                    np.repeat(_cov6_px([[60.0 ** 2, 0, 60.0 ** 2]], 4.0, H), len(cand), axis=0))
    pre = run_oracle(oracle, big["s"], colors_precomp=big["colors"], cov3D_precomp=big["cov6"],
                     stages="preprocess")
    assert (pre["radii"] > 0).all()
    xyz, kinds = [], []
    for k, (axis, t, what) in enumerate(tg):
        sel = np.flatnonzero(owner == k)
        v = pre["means2D"][sel, axis]
        t32 = F32(t)
        below, at, above = sel[v < t32], sel[v == t32], sel[v > t32]
        assert len(below) and len(above), (name, what)
        picks = [below[np.argmax(pre["means2D"][below, axis])],
                 above[np.argmin(pre["means2D"][above, axis])]]
        if len(at):
            picks.append(at[len(at) // 2])
        for i in picks:
            xyz.append(cand[i])
            kinds.append((axis, what, float(pre["means2D"][i, axis]) - t))
    n = len(xyz)
    rng = np.random.default_rng(9)
    sp = _plain(n, rng, M=1, opacity=0.5)
    sp.xyz = np.asarray(xyz, F32)
    sc = _mixed(name, static_camera(W, H), 0, sp, 103, colors=rng.uniform(0, 1, (n, 3)),
                cov6=np.repeat(_cov6_px([[sigma2, 0, sigma2]], 4.0, H), n, axis=0), oracle=oracle)
    sc["kinds"] = kinds
    return sc


RADIUS_KS = tuple(range(3, 41))


def _radius_ceil(oracle):
    W, H = 160, 120
    rng = np.random.default_rng(10)
    steps = np.arange(-400, 401)
    nk = len(RADIUS_KS)
    px, py = rng.uniform(10, W - 10, nk), rng.uniform(10, H - 10, nk)
    xyz = _world_xy(W, H, px, py)
    lam = (np.asarray(RADIUS_KS, np.float64) / 3.0) ** 2
    base = _cov6_px(np.stack([lam - 0.3 - np.sqrt(0.1)] * 2, -1)[:, [0, 0, 1]] * [1, 0, 1], 4.0, H)
    cand_xyz = np.repeat(xyz, len(steps), axis=0)
    cand_cov = np.repeat(base, len(steps), axis=0)
    for i in range(nk):
        v = ulp_steps(base[i, 0], steps)
        cand_cov[i * len(steps):(i + 1) * len(steps), 0] = v
        cand_cov[i * len(steps):(i + 1) * len(steps), 3] = v
    big = bs._scene(W, H, cand_xyz, np.ones(len(cand_xyz)), np.ones((len(cand_xyz), 3), F32), cand_cov)
    rad = run_oracle(oracle, big["s"], colors_precomp=big["colors"], cov3D_precomp=big["cov6"],
                     stages="preprocess")["radii"].reshape(nk, len(steps))
    sel_xyz, sel_cov, ks = [], [], []
    for i, k in enumerate(RADIUS_KS):
        r = rad[i]
        assert r[0] == k and r[-1] == k + 1 and (np.diff(r) >= 0).all(), ("radius_ceil", k, r[0], r[-1])
        j = int(np.argmax(r == k + 1))  # the first covariance past the jump
        for jj in (j - 2, j - 1, j, j + 1):
            sel_xyz.append(xyz[i])
            sel_cov.append(cand_cov[i * len(steps) + jj])
            ks.append(k + (jj >= j))
    n = len(sel_xyz)
    sp = _plain(n, rng, M=1, opacity=0.3)
    sp.xyz = np.asarray(sel_xyz, F32)
    sc = _mixed("radius_ceil", static_camera(W, H), 0, sp, 104, colors=rng.uniform(0, 1, (n, 3)),
                cov6=np.asarray(sel_cov, F32), oracle=oracle)
    sc["radius_want"] = np.asarray(ks)
    return sc


def _det_cancel(oracle):
    W, H = 160, 120
    rng = np.random.default_rng(11)
    n = 120
    L = np.exp(rng.uniform(np.log(1e6), np.log(1e8), n))
    th = rng.uniform(0.3, 1.2, n) * rng.choice([-1.0, 1.0], n)
    c, s = np.cos(th), np.sin(th)
    granule = 2.0 ** -24 * (L * c * s) ** 2  # about one rounding of a c (and of b b)
    # the small eigenvalue (before upstream's + 0.3) so that det(cov + 0.3 I) ~ L (l + 0.3) is
    # within a few granules of 0 -- the last quarter clearly positive (4 .. 60 granules)
    k = np.where(np.arange(n) % 4 == 3, rng.uniform(4, 60, n), rng.uniform(-3, 3, n))
    l = -0.3 + k * granule / L
    cov = np.stack([c * c * L + s * s * l, c * s * (L - l), s * s * L + c * c * l], -1)
    sp = _plain(n, rng, M=1)
    sp.xyz = _world_xy(W, H, rng.uniform(20, W - 20, n), rng.uniform(20, H - 20, n))
    # opacity under 2^-10: conics of 1e3 and of either sign put power's sign and size within the
    # rounding of any float32 quadratic, so these splats are compared as records, never blended
    sp.opacity = rng.uniform(0.0002, 0.0009, (n, 1)).astype(F32)
    return _mixed("det_cancel", static_camera(W, H), 0, sp, 105, colors=rng.uniform(0, 1, (n, 3)),
                  cov6=_cov6_px(cov, 4.0, H), oracle=oracle)


SCALE_VALUES = (0.0, 1e-30, 1e-20, 1e-3, 1.0, 1e3, 1e8, 1e15)


def _scale_range(key):
    W, H = 160, 120
    rng = np.random.default_rng(12)
    scale, rot = [], []
    q_id = [1.0, 0, 0, 0]
    q_r = rng.standard_normal((64, 4))
    q_r /= np.linalg.norm(q_r, axis=1, keepdims=True)
    for i, v in enumerate(SCALE_VALUES):
        # (from 1 up only the first two: an isotropic splat of thousands of px is undecidable
        # in float32 -- mid^2 - det cancels -- and the scene must keep enough decidable members)
        scale += [(v, v, v), (0.01, v, 0.02), (v, 0.01, 0.01), (v, 0.01, 0.01)][:4 if v < 1 else 2]
        rot += [q_id, q_r[2 * i], q_id, q_r[2 * i + 1]][:4 if v < 1 else 2]
    scale += [(-0.01, -0.01, -0.01), (-0.02, 0.01, 0.01), (-10.0, 1.0, 1.0)]
    rot += [q_id, q_r[40], q_r[41]]
    for q in ([0.0, 0, 0, 0], 0.3 * q_r[50], 0.3 * q_r[51], 2.0 * q_r[52], 2.0 * q_r[53]):
        scale.append((0.03, 0.02, 0.01))
        rot.append(q)
    n = len(scale)
    sp = _plain(n, rng)
    sp.xyz = rng.uniform(-1.0, 1.0, (n, 3)).astype(F32)
    sp.scale, sp.rot = np.asarray(scale, F32), np.asarray(rot, F32)
    # scales 1 .. 1e3 sit at view depth 400: a radius of 1e7 px is undecidable in float32 (its
    # rounding exceeds 1); 1e8 and 1e15 stay near, where they saturate the radius or overflow
    far = (np.abs(sp.scale).max(axis=1) >= 1) & (np.abs(sp.scale).max(axis=1) <= 1e3)
    sp.xyz[far] *= F32([30.0, 20.0, 0.0])
    sp.xyz[far, 2] = F32(-396.0)
    sp.opacity = rng.uniform(0.1, 0.9, (n, 1)).astype(F32)
    # from 1e8 up the finite conics are rounding residue around 0 (1e-11, of either sign): power's
    # sign is undecidable over the whole frame, so these stay under 1/255 and only a NaN conic
    # (alpha = min(0.99, NaN) = 0.99 whatever the opacity) reaches the image
    sp.opacity[np.abs(sp.scale).max(axis=1) >= 1e8] = F32(0.003)
    return _mixed(f"scale_range_{key}", static_camera(W, H), 3, sp, 106,
                  scale_modifier=SCALE_MODS[key])


POISONS = (np.nan, np.inf, -np.inf)
NONFINITE_EYE = (0.5, 0.3, 4.0)


def _nonfinite():
    W, H = 160, 120
    rng = np.random.default_rng(13)
    fields = [("xyz", 0), ("xyz", 1), ("xyz", 2), ("scale", 0), ("scale", 2), ("rot", 0),
              ("rot", 2), ("opacity", 0), ("sh", 1), ("sh", 3 * 1 + 0)]
    n = len(fields) * len(POISONS)
    sp = _plain(n, rng)
    sp.xyz = rng.uniform(-0.8, 0.8, (n, 3)).astype(F32)
    # above the camera position, so the direction's y is positive: the degree-1 y term enters as
    # -C1 y sh[1], and a +inf there gives -inf, clamped to 0 (colours stay finite)
    sp.xyz[:, 1] = rng.uniform(0.5, 0.9, n).astype(F32)
    q = rng.standard_normal((n, 4))
    sp.rot = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    what = []
    for i, (f, j) in enumerate((f, j) for f, j in fields for _ in POISONS):
        v = POISONS[i % len(POISONS)]
        # colours stay finite: an infinite coefficient only where its term is -inf (clamped to
        # 0) -- the DC term is +C0 sh[0], the y term -C1 y sh[1] with y > 0; the excluded sign
        # goes to the next channel with the other sign
        if f == "sh" and j == 1 and v == np.inf:
            j, v = 2, -np.inf
        if f == "sh" and j == 3 and v == -np.inf:
            j, v = 4, np.inf
        getattr(sp, f)[i, j] = v
        what.append((f, j, v))
    sc = _mixed("nonfinite", static_camera(W, H, eye=NONFINITE_EYE), 3, sp, 107)
    sc["poisons"] = what
    return sc


def _nonfinite_precomp(oracle):
    W, H = 160, 120
    rng = np.random.default_rng(14)
    n = 6 * len(POISONS)
    sp = _plain(n, rng, M=1)
    sp.xyz = rng.uniform(-0.8, 0.8, (n, 3)).astype(F32)
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    cov6 = oracle.cov3d(rng.uniform(0.01, 0.05, (n, 3)).astype(F32), q.astype(F32))
    what = []
    for i in range(n):
        cov6[i, i // len(POISONS)] = POISONS[i % len(POISONS)]
        what.append(("cov3D_precomp", i // len(POISONS), POISONS[i % len(POISONS)]))
    sc = _mixed("nonfinite_precomp", static_camera(W, H, eye=NONFINITE_EYE), 0, sp, 108,
                colors=rng.uniform(0, 1, (n, 3)), cov6=cov6, oracle=oracle)
    sc["poisons"] = what
    return sc


SH_CAMPOS = (0.5, 0.25, 0.0)
SH_C0 = F32(0.28209479177387814)


def sh_half_coefficient():
    """The float32 DC coefficient whose float32 product with SH_C0 is exactly -0.5."""
    c = ulp_steps(F32(-0.5 / float(SH_C0)), np.arange(-16, 17))
    hit = c[(SH_C0 * c) == F32(-0.5)]
    assert len(hit)
    return hit[len(hit) // 2]


def _sh_edges(D, M):
    W, H = 160, 120
    rng = np.random.default_rng(15)
    cp = np.asarray(SH_CAMPOS, F32)
    xyz, sh, op = [], [], []
    row = lambda: np.concatenate([rng.normal(0, 0.6, 3), rng.normal(0, 0.3, 3 * (M - 1))])  # noqa: E731
    # directions along each axis from campos (both signs, two distances), and campos itself
    for axis in range(3):
        for dist in (-1.0, -0.25, 0.25, 1.0):
            p = cp.copy()
            p[axis] += F32(dist)
            xyz.append(p)
            sh.append(row())
            op.append(0.6)
    xyz.append(cp.copy())  # len = 0: the direction is 0 / 0
    sh.append(row())
    op.append(0.6)
    # a channel exactly -0.5 before the + 0.5, and one float either side: the DC term alone
    # (higher coefficients 0, so they add +-0 and the sum stays exact)
    half = sh_half_coefficient()
    for ch in range(3):
        for st in (-1, 0, 1):
            r = np.zeros(3 * M)
            r[:3] = rng.normal(0, 0.6, 3)
            r[ch] = ulp_steps(half, [st])[0]
            xyz.append(rng.uniform(-1, 1, 3))
            sh.append(r)
            op.append(0.6)
    # coefficients of 1e30 (opacity under 1/255: compared as colours, never blended)
    for _ in range(6):
        xyz.append(rng.uniform(-1, 1, 3))
        sh.append(1e30 * rng.choice([-1.0, 1.0], 3 * M))
        op.append(0.003)
    n = len(xyz)
    sp = _plain(n, rng, M=M)
    sp.xyz, sp.sh = np.asarray(xyz, F32), np.ascontiguousarray(sh, F32)
    sp.opacity = np.asarray(op, F32).reshape(n, 1)
    return _mixed(f"sh_edges_{D}_{M}", static_camera(W, H), D, sp, 109, campos=cp)


def _boundaries(P):
    W, H = 160, 120
    g = synthetic_gaussians(P, 3, 200 + P)
    g.xyz = (g.xyz * F32(0.6)).astype(F32)  # inside the frustum of the eye at (0, 0, 4)
    g.xyz[1::3, 2] += F32(6.0)              # a third behind the camera
    s = scene_inputs(g, static_camera(W, H), 3, bg=BG)
    return dict(name=f"boundaries_{P}", s=s, colors=None, cov6=None, W=W, H=H,
                special=np.zeros(P, bool))


def build(oracle, name):
    if name == "near_plane":
        return _near_plane()
    if name == "clamp":
        return _clamp()
    if name.startswith("rect_edges_"):
        return _rect_edges(oracle, *(int(v) for v in name.rsplit("_", 1)[1].split("x")))
    if name == "radius_ceil":
        return _radius_ceil(oracle)
    if name == "det_cancel":
        return _det_cancel(oracle)
    if name.startswith("scale_range_"):
        return _scale_range(name.rsplit("_", 1)[1])
    if name == "nonfinite":
        return _nonfinite()
    if name == "nonfinite_precomp":
        return _nonfinite_precomp(oracle)
    if name.startswith("sh_edges_"):
        return _sh_edges(*(int(v) for v in name.split("_")[2:]))
    if name.startswith("boundaries_"):
        return _boundaries(int(name.rsplit("_", 1)[1]))
    raise KeyError(name)


_cache: dict = {}


def get(oracle, name):
    """build(), once per process: the scene and the oracle result kept in it are shared by the
    tests that use it and left unchanged."""
    if name not in _cache:
        _cache[name] = build(oracle, name)
    return _cache[name]


def finite_records(sc, orc):
    """Whether every colour and every conic the blend reads is finite (then the blend is held to
    the float64 reference too)."""
    vis = orc["radii"] > 0
    return bool(np.isfinite(orc["conic_opacity"][vis]).all() and
                np.isfinite(features(sc, orc)[vis]).all())
