"""The scenes of the general-pose backward tests (test_pose_grad_reference.py on the CPU,
test_gpu_pose_gradients.py on the GPU): scenes of grad_scenes and camera_grad_scenes under cameras
whose view rotation is not diagonal, and one scene of edges built per pose.

Every other gradient test of the suite looks through static_camera: the view matrix the kernels
read is diag(-1, 1, -1) with a translation along z, so R and R^T are the same numbers and six
entries of projmatrix are exact zeros.  A backward that swaps a row index for a column index of
either matrix is bit-identical there ("The backward under a general pose").

  POSES    yaw      eye (2.6, 0.5, 3.0) -> 0, up +y: a rotation about (nearly) one axis
           oblique  eye (1.9, 1.1, 3.2) -> (0.3, -0.2, 0.1), up (0.35, 0.9, -0.25): a dense rotation
                    with roll, all three translations nonzero, and all twelve entries of the first
                    three columns of projmatrix nonzero
           close    eye (0.89, -0.7, 1.6) -> (-0.2, 0.1, 0), up (-0.3, 0.8, 0.5): near and strongly
                    off axis; a third to a half of the Gaussians sit beyond the 1.3 tan clamp
                    (at x = 0.9 chain has one decision within rounding of its gate)
           static   static_camera itself (the scene as it is), for the tests that show what that
                    pose cannot see
           (four scene x pose pairs look from an eye up to 0.1 beside their pose's: EYES)
  SCENES   chain, long_lists, precomputed (grad_scenes), blocks (camera_grad_scenes), re-posed by
           repose(); and pose_edges, built in view space and mapped to the world through the
           float64 inverse of the pose, rounded once:
             P = 80 over 24 x 24 px, M = 16 with D = 1, about a third of the colour channels
             clamped at 0; eight Gaussians beyond the clamp that still reach the frame (three on x,
             two on y, three on both); four with view z at 0.2 (2e-5 under it: nearer than that the
             float32 rounding of the world mean decides the cull), at 0.19, in the eye's plane and
             behind the eye
           grad_scenes' `edges` is not re-posed: its det == 0 Gaussian is built for the axis, and
           under another pose it becomes visible with a scale of 1024.

Same layout as grad_scenes (s, colors, cov6, W, H, dL, special) plus `base` (the scene's name
without the pose) and `pose`; `name` is "<base>@<pose>", which keeps the GPU modules' caches apart.
"""
from __future__ import annotations

import numpy as np
import torch

import aa_reference as ar
import camera_grad_reference as cg
import camera_grad_scenes
import feature_grad_reference as fg
import grad_reference as gr
import grad_scenes
import plane_grad_reference as pg
from gaussiansplattingviewer_amd.camera import Camera, cuda_camera_inputs, look_at

F32 = np.float32
POSES = {
    "yaw": ((2.6, 0.5, 3.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0)),
    "oblique": ((1.9, 1.1, 3.2), (0.3, -0.2, 0.1), (0.35, 0.9, -0.25)),
    "close": ((0.89, -0.7, 1.6), (-0.2, 0.1, 0.0), (-0.3, 0.8, 0.5)),
}
# The float64 reference may hold no decision within rounding of its gate (grad_reference's
# near_gate; test_pose_grad_reference.py asserts zero for every scene under every pose).  Where a
# scene has such a pair at a pose's eye, that scene looks from the nearest eye on a 0.01 grid that
# has none (searched outwards from the pose's own); target and up stay.
EYES = {
    ("long_lists", "yaw"): (2.58, 0.5, 3.0),
    ("blocks", "yaw"): (2.59, 0.49, 3.0),
    ("long_lists", "oblique"): (1.92, 1.1, 3.2),
    ("long_lists", "close"): (0.94, -0.68, 1.7),
}
NAMES = tuple(POSES)                      # the non-static poses
STATIC = ((0.0, 0.0, 4.0), (0.0, 0.0, 0.0), (0.0, 1.0, 0.0))
REPOSED = ("chain", "long_lists", "precomputed", "blocks")
SCENES = REPOSED + ("pose_edges",)
EDGES_SEED = 21
NEAR_Z = (0.2 - 2e-5, 0.19, 0.0, -1.0)    # the view z of pose_edges' four culled Gaussians


def look(pose, base=None):
    """(eye, target, up) of a pose for the scene `base` (EYES)."""
    eye, target, up = STATIC if pose == "static" else POSES[pose]
    return EYES.get((base, pose), eye), target, up


def camera_inputs(W, H, pose, base=None):
    """(view, proj, campos, tx, ty) of a pose as the viewer builds them."""
    eye, target, up = look(pose, base)
    cam = Camera(H, W)
    cam.position = np.asarray(eye, F32)
    return cuda_camera_inputs(cam, look_at(eye, target, up))


def gl_camera(W, H, pose, base=None):
    """(view [4,4] float32 in GL math layout, the GL projection) of a pose: camera_tensors' inputs."""
    eye, target, up = look(pose, base)
    return look_at(eye, target, up), Camera(H, W).get_project_matrix()


def repose(scene, pose):
    """A copy of a scene (grad_scenes layout) whose s has view, proj, campos, tx and ty of the
    pose.  Nothing a test cached in the scene travels."""
    base = scene.get("base", scene["name"])
    view, proj, campos, tx, ty = camera_inputs(scene["W"], scene["H"], pose, base)
    s = dict(scene["s"], view=view, proj=proj, campos=campos, tx=tx, ty=ty)
    return dict(name=f"{base}@{pose}", base=base, pose=pose, s=s, colors=scene["colors"],
                cov6=scene["cov6"], W=scene["W"], H=scene["H"], dL=scene["dL"],
                special=dict(scene["special"]))


def _to_world(view, t):
    """World points of view-space points t [n,3] under the kernels' view matrix (column-major:
    t = R p + T, R[r][c] = view[c][r]), in float64."""
    m = np.asarray(view, np.float64)
    R, T = m[:3, :3].T, m[3, :3]
    return (t - T) @ R  # R^T (t - T), row-wise


def build_edges(pose):
    rng = np.random.default_rng(EDGES_SEED)
    W, H, D, mod, bg = 24, 24, 1, 1.0, (0.2, 0.4, 0.6)
    g = grad_scenes._gaussians(rng, 80, 1.4, 1.4, 0.05, 0.35, 0.1, 0.9, dc=(-1.0, 1.8), rest=0.3)
    # view space: x, y as drawn, z in [3, 5] in front of the eye
    t = np.stack([g.xyz[:, 0], g.xyz[:, 1], 4.0 - g.xyz[:, 2]], 1).astype(np.float64)
    special = {}
    # beyond the 1.3 tan clamp (|t.x / t.z| or |t.y / t.z| > 0.39 on this frame) at view z = 1,
    # large enough to reach the frame: 0..2 on x, 3..4 on y, 5..7 on both
    n = 8
    far = rng.choice([-1.0, 1.0], (n, 2)) * rng.uniform(0.5, 0.75, (n, 2))
    inside = rng.uniform(-0.2, 0.2, (n, 2))
    on_x = np.array([1, 1, 1, 0, 0, 1, 1, 1], bool)
    on_y = np.array([0, 0, 0, 1, 1, 1, 1, 1], bool)
    t[:n, 0] = np.where(on_x, far[:, 0], inside[:, 0])
    t[:n, 1] = np.where(on_y, far[:, 1], inside[:, 1])
    t[:n, 2] = 1.0
    g.scale[:n] = rng.uniform(0.15, 0.3, (n, 3))
    special.update(clamp=np.arange(n), clamp_x=np.flatnonzero(on_x), clamp_y=np.flatnonzero(on_y))
    # view z <= 0.2: at the near plane, just under it, in the eye's plane, behind the eye
    t[n:n + 4, 2] = NEAR_Z
    special["behind"] = np.arange(n, n + 4)
    view, proj, campos, tx, ty = camera_inputs(W, H, pose)
    g.xyz[:] = _to_world(view, t).astype(F32)
    s = dict(g=g, view=view, proj=proj, campos=campos, tx=tx, ty=ty, W=W, H=H, sh_degree=D,
             bg=np.asarray(bg, F32), scale_modifier=mod)
    dL = np.ascontiguousarray(rng.standard_normal((3, H, W)), F32)
    return dict(name=f"pose_edges@{pose}", base="pose_edges", pose=pose, s=s, colors=None,
                cov6=None, W=W, H=H, dL=dL, special=special)


_cache = {}


def get(name, pose):
    """Scene `name` of SCENES under `pose` of POSES, or "static": the scene as its module has it
    (pose_edges: built for that camera)."""
    key = (name, pose)
    if key not in _cache:
        if name == "pose_edges":
            _cache[key] = build_edges(pose)
        elif pose == "static":
            _cache[key] = camera_grad_scenes.get(name)
        else:
            _cache[key] = repose(camera_grad_scenes.get(name), pose)
    return _cache[key]


CASES = [(n, p) for p in NAMES for n in SCENES]


def plane_dL(sc):
    """The planes' gradients of a scene, [3, H, W] float32 (depth, inverse depth, final_T): the
    base scene's (camera_grad_scenes.plane_dL), made the same way for pose_edges."""
    base = sc.get("base", sc["name"])
    if base != "pose_edges":
        return camera_grad_scenes.plane_dL(base)
    rng = np.random.default_rng(100 + EDGES_SEED)
    return np.ascontiguousarray(rng.standard_normal((3, sc["H"], sc["W"])), F32)


# ---- the references, per kind of backward ----------------------------------------------------------
# kind      loss                                               reference                 scenes
# colour    sum(color dL)                                      grad_reference            all
# planes    + the three planes                                 plane_grad_reference      PLANE_SCENES
# camera    colour, and colour + planes: the camera's three    camera_grad_reference     all
# aa        colour + planes, antialiased, camera included      aa_reference              chain
# features  the same + fg.ALL_C feature channels               feature_grad_reference    chain
KINDS = ("colour", "planes", "camera", "aa", "features")
PLANE_SCENES = ("chain", "pose_edges")
ALL_SCENE = "chain"
CAMERA_LOSSES = cg.LOSSES


def kind_scenes(kind):
    return {"colour": SCENES, "camera": SCENES, "planes": PLANE_SCENES}.get(kind, (ALL_SCENE,))


def reference(kind, sc, lists, radii, dtype=torch.float64, gates=None, loss="combined"):
    """The reference gradients of a kind on a scene of this module (loss: of CAMERA_LOSSES, read by
    kind "camera" alone).  gates: the float64 run's, for a float32 run."""
    dL, dLp = sc["dL"], plane_dL(sc)
    if kind == "colour":
        return gr.scene_gradients(sc, lists, radii, dL, dtype, gates)
    if kind == "planes":
        return pg.scene_gradients(sc, lists, radii, dL, dLp, dtype, gates)
    if kind == "camera":
        return cg.scene_gradients(sc, lists, radii, dL, dLp if loss == "combined" else None, dtype,
                                  gates)
    if kind == "aa":
        return ar.scene_gradients(sc, lists, radii, dL, dLp, dtype, gates)
    if kind == "features":
        return fg.scene_gradients(sc, lists, radii, dL, fg.feature_rows(sc["base"], fg.ALL_C),
                                  fg.feature_dL(sc["base"], fg.ALL_C), dLp, dtype, gates,
                                  antialiasing=True)
    raise KeyError(kind)


def err(got, ref, key):
    """The error of one gradient tensor against a reference() result on its scale: gr.rel_err, the
    camera's three by cg.cam_err."""
    return ar.err(got, ref, key)


# ---- the tolerance of the GPU tests: measured, not chosen ------------------------------------------
# POSE_F32_SPREAD: the references' own float32 spread under the three poses -- err of reference()
# evaluated in float32 (lists and gates of the float64 run, so only rounding differs) against
# float64, the largest over the poses and over kind_scenes(kind) (camera: over both losses too),
# measured on the CPU with the oracle's lists.  test_pose_grad_reference.py re-measures every value
# and holds it to within a factor 2.  The GPU tests allow, per tensor,
#     gr.BOUND_FACTOR x max(the kind's existing F32_SPREAD, POSE_F32_SPREAD):
# the project's margin of 8 over the reference's own rounding, never below the bound the static
# scenes already use.
# (columns: the largest per pose -- yaw, oblique, close; then the constant over the kind's existing
# one, and the scene that sets it)
POSE_F32_SPREAD = {
    "colour": {
        "means3D": 4.3e-6,     # 4.3e-6  2.4e-6  9.0e-7   0.9 x  (precomputed@yaw)
        "means2D": 4.6e-6,     # 4.6e-6  3.2e-6  1.9e-6   0.7 x  (precomputed@yaw)
        "means2D_px": 4.6e-6,  # 4.6e-6  2.6e-6  1.4e-6   0.9 x  (precomputed@yaw)
        "conic": 1.8e-6,       # 1.8e-6  1.3e-6  1.1e-6   1.0 x  (precomputed@yaw)
        "opacity": 1.6e-6,     # 9.7e-7  1.6e-6  4.7e-7   2.6 x  (blocks@oblique)
        "rgb": 1.5e-6,         # 1.0e-6  1.5e-6  6.3e-7   1.2 x  (precomputed@oblique)
        "shs": 1.2e-6,         # 1.0e-6  1.2e-6  4.8e-7   1.8 x  (blocks@oblique)
        "scales": 4.7e-6,      # 3.2e-6  4.7e-6  1.3e-6   4.0 x  (chain@oblique)
        "rotations": 1.4e-6,   # 1.4e-6  1.2e-6  1.0e-6   1.0 x  (blocks@yaw)
        "cov3D": 1.8e-6,       # 1.8e-6  1.0e-6  2.1e-7   0.6 x  (precomputed@yaw)
        "colors": 1.5e-6,      # 1.0e-6  1.5e-6  6.3e-7   1.2 x  (precomputed@oblique)
    },
    "planes": {
        "means3D": 3.0e-6,     # 6.1e-7  3.0e-6  1.4e-6   1.2 x  (pose_edges@oblique)
        "means2D": 3.2e-6,     # 8.8e-7  3.2e-6  2.6e-6   1.0 x  (pose_edges@oblique)
        "means2D_px": 3.2e-6,  # 9.1e-7  3.2e-6  1.9e-6   1.1 x  (pose_edges@oblique)
        "conic": 3.1e-6,       # 5.5e-7  3.1e-6  2.0e-6   1.7 x  (chain@oblique)
        "opacity": 1.1e-6,     # 1.1e-6  6.9e-7  6.6e-7   0.7 x  (chain@yaw)
        "depths": 1.0e-6,      # 6.0e-7  1.0e-6  1.0e-6   0.8 x  (chain@oblique)
        "rgb": 7.5e-7,         # 5.7e-7  7.5e-7  4.9e-7   0.6 x  (chain@oblique)
        "shs": 9.2e-7,         # 5.0e-7  9.2e-7  4.4e-7   1.4 x  (chain@oblique)
        "scales": 2.2e-6,      # 7.7e-7  2.2e-6  1.2e-6   1.7 x  (chain@oblique)
        "rotations": 1.9e-6,   # 1.2e-6  1.9e-6  6.7e-7   1.5 x  (chain@oblique)
    },
    "camera": {
        "viewmatrix": 5.6e-7,  # 3.8e-7  5.6e-7  3.8e-7   0.8 x  (precomputed@oblique)
        "projmatrix": 7.6e-7,  # 7.6e-7  7.4e-7  3.2e-7   0.9 x  (precomputed@yaw)
        "campos": 2.5e-7,      # 1.6e-7  2.5e-7  2.3e-7   2.6 x  (chain@oblique)
    },
    "aa": {
        "means3D": 8.1e-7,     # 8.1e-7  5.0e-7  7.8e-7   0.2 x  (chain@yaw)
        "means2D": 1.7e-6,     # 5.7e-7  5.2e-7  1.7e-6   0.3 x  (chain@close)
        "opacity": 1.1e-6,     # 1.1e-6  6.7e-7  3.8e-7   0.1 x  (chain@yaw)
        "scales": 1.7e-6,      # 1.1e-6  1.4e-6  1.7e-6   0.0 x  (chain@close)
        "rotations": 1.6e-6,   # 1.4e-6  1.6e-6  9.2e-7   0.1 x  (chain@oblique)
        "shs": 7.9e-7,         # 6.4e-7  7.9e-7  3.1e-7   0.3 x  (chain@oblique)
        "viewmatrix": 2.4e-7,  # 2.4e-7  1.7e-7  2.2e-7   0.2 x  (chain@yaw)
        "projmatrix": 2.0e-7,  # 9.5e-8  1.9e-7  2.0e-7   0.3 x  (chain@close)
        "campos": 2.6e-7,      # 1.5e-7  2.6e-7  6.3e-8   1.9 x  (chain@oblique)
    },
    "features": {
        "features": 1.0e-6,    # 1.0e-6  9.2e-7  6.4e-7   1.8 x  (chain@yaw)
        "means3D": 8.5e-7,     # 6.9e-7  8.5e-7  5.6e-7   1.1 x  (chain@oblique)
        "means2D": 1.0e-6,     # 2.7e-7  1.0e-6  8.6e-7   1.6 x  (chain@oblique)
        "opacity": 6.7e-7,     # 5.7e-7  6.7e-7  3.0e-7   1.5 x  (chain@oblique)
        "scales": 1.3e-6,      # 7.6e-7  1.3e-6  5.3e-7   1.9 x  (chain@oblique)
        "rotations": 1.2e-6,   # 1.2e-6  7.1e-7  7.4e-7   1.6 x  (chain@yaw)
        "shs": 7.9e-7,         # 6.4e-7  7.9e-7  3.1e-7   1.6 x  (chain@oblique)
        "viewmatrix": 3.3e-7,  # 2.4e-7  3.3e-7  2.3e-7   1.5 x  (chain@oblique)
        "projmatrix": 2.7e-7,  # 9.0e-8  1.6e-7  2.7e-7   1.9 x  (chain@close)
        "campos": 2.6e-7,      # 1.5e-7  2.6e-7  6.3e-8   10.0 x  (chain@oblique)
    },
}
EXISTING = {"colour": gr.F32_SPREAD, "planes": pg.F32_SPREAD, "camera": cg.F32_SPREAD,
            "aa": ar.F32_SPREAD, "features": fg.F32_SPREAD_ALL}


def bound(kind, key):
    return gr.BOUND_FACTOR * max(EXISTING[kind][key], POSE_F32_SPREAD[kind][key])
