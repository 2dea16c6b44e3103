"""CPU: the scenes and the yardsticks of the general-pose backward tests (pose_scenes;
test_gpu_pose_gradients.py runs them on the device).

  1 the poses are what they claim: the static view rotation is diagonal and six entries of its
    projmatrix are exact zeros (the gap); yaw, oblique and close are not symmetric, oblique and
    close dense in the rotation, the translation and the twelve entries of projmatrix the backward
    reads
  2 every scene under every pose: no decision within rounding of its gate in any reference that
    runs on it, at least 60 % of the Gaussians kept, every tile of chain non-empty, pose_edges'
    clamp and behind sets what they claim
  3 POSE_F32_SPREAD is what a float32 evaluation of the references gives here, within a factor 2
  4 teeth: mutants of the references, each with one index pattern wrong in the reference's own text.
    Those that read a rotation's transpose are exactly the reference at the static pose -- the gap
    this module closes -- and every mutant exceeds the GPU tests' bound at every other pose.
"""
import contextlib
import inspect

import numpy as np
import pytest
import torch

import grad_reference as gr
import plane_grad_reference as pg
import pose_scenes as ps
from test_grad_reference import _oracle

_ref_cache = {}


def _lists(sc):
    orc = _oracle(sc)
    return (orc["ranges"], orc["point_list"]), orc["radii"]


def _ref64(kind, sc, loss="combined"):
    key = (kind, sc["name"], loss)
    if key not in _ref_cache:
        _ref_cache[key] = ps.reference(kind, sc, *_lists(sc), loss=loss)
    return _ref_cache[key]


# ---- 1 --------------------------------------------------------------------------------------------
def _camera(pose, W=40, H=24):
    view, proj, campos, _, _ = ps.camera_inputs(W, H, pose)
    vm, pm = np.asarray(view, np.float64).reshape(-1), np.asarray(proj, np.float64).reshape(-1)
    R = np.array([[vm[4 * c + r] for c in range(3)] for r in range(3)])
    return R, vm[12:15], pm, np.asarray(campos, np.float64)


def test_the_static_pose_is_the_gap():
    R, T, pm, campos = _camera("static")
    assert (R == np.diag([-1.0, 1.0, -1.0])).all() and (T[:2] == 0).all()
    assert (pm[[1, 3, 4, 7, 8, 9]] == 0).all() and (campos[:2] == 0).all()


@pytest.mark.parametrize("pose", ps.NAMES)
def test_pose_matrices(pose):
    R, T, pm, campos = _camera(pose)
    assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and np.linalg.det(R) > 0
    assert np.abs(R - R.T).max() >= 0.5
    # the entries the backward reads: pm[4 c + r], r = 0, 1, 3
    read = pm[[4 * c + r for c in range(3) for r in (0, 1, 3)]]
    if pose == "yaw":  # about one axis, but for the eye's height
        assert np.abs(R[0, 1]) <= 1e-6 and np.abs(T[:2]).max() <= 1e-6
    if pose == "oblique":
        assert 0.24 <= np.abs(R).min() <= 0.25 and 0.14 <= np.abs(T).min() <= 0.143
        assert np.abs(pm[:12]).min() >= 0.3
    if pose == "close":
        assert np.abs(R).min() >= 0.25 and np.abs(T).min() >= 0.1 and np.abs(pm[:12]).min() >= 0.2
        assert np.abs(T[2]) <= 2.0
    if pose != "yaw":
        assert np.abs(read).min() >= 0.2 and np.abs(campos).min() >= 0.5
    for (base, p), eye in ps.EYES.items():  # a moved eye stays on the pose
        if p == pose:
            assert np.abs(np.subtract(eye, ps.POSES[p][0])).max() <= 0.1 + 1e-9


# ---- 2 --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,pose", ps.CASES)
def test_scene_conditions(name, pose):
    sc = ps.get(name, pose)
    orc = _oracle(sc)
    assert sc["W"] <= 40 and sc["H"] <= 24 and len(orc["radii"]) <= 600
    ref = _ref64("colour", sc)
    assert ref["near"] == (0, 0)
    for loss in ps.CAMERA_LOSSES:
        assert _ref64("camera", sc, loss)["near"] == (0, 0)
    if name in ps.PLANE_SCENES:
        assert _ref64("planes", sc)["near"] == (0, 0)
    if name == ps.ALL_SCENE:
        assert _ref64("aa", sc)["near"] == (0, 0, 0) and _ref64("features", sc)["near"] == (0, 0, 0)
    kept = orc["radii"] > 0
    assert kept.mean() >= 0.6
    gates = ref["gates"][0]
    beyond = (gates["lo0"] | gates["hi0"] | gates["lo1"] | gates["hi1"]).numpy()
    if pose == "close" and name != "pose_edges":
        assert beyond.mean() >= 0.3
    counts = orc["ranges"][:, 1].astype(int) - orc["ranges"][:, 0].astype(int)
    if name == "chain":
        assert len(counts) == 6 and (counts > 0).all()
    if name == "long_lists":
        assert len(counts) == 2 and (counts > 128).all()
    if name == "pose_edges":
        sp = sc["special"]
        assert (orc["radii"][sp["clamp"]] > 0).all() and (orc["radii"][sp["behind"]] == 0).all()
        assert set(sp["clamp"]) <= set(orc["point_list"].tolist())
        vis = np.flatnonzero(kept)
        on_x, on_y = (gates["lo0"] | gates["hi0"]).numpy(), (gates["lo1"] | gates["hi1"]).numpy()
        at = np.searchsorted(vis, sp["clamp"])
        np.testing.assert_array_equal(np.flatnonzero(on_x[at]), sp["clamp_x"])
        np.testing.assert_array_equal(np.flatnonzero(on_y[at]), sp["clamp_y"])
        assert (on_x[at] & on_y[at]).sum() == 3 and (on_x[at] ^ on_y[at]).sum() == 5
        assert 0.25 <= gates["clamped"].numpy().mean() <= 0.45
        # view space as built: the four culled ones at their z under this very view matrix
        vm = np.asarray(sc["s"]["view"], np.float64).reshape(-1)
        p = sc["s"]["g"].xyz.astype(np.float64)[sp["behind"]]
        z = vm[2] * p[:, 0] + vm[6] * p[:, 1] + vm[10] * p[:, 2] + vm[14]
        assert np.abs(z - np.array(ps.NEAR_Z)).max() <= 2e-6 and (z < 0.2 - 1e-5).all()


# ---- 3 --------------------------------------------------------------------------------------------
def _measure(kind):
    """{key: (the largest float32 spread, {(scene, pose[, loss]): spread})} of a kind."""
    seen, table = {}, {}
    for pose in ps.NAMES:
        for name in ps.kind_scenes(kind):
            sc = ps.get(name, pose)
            for loss in (ps.CAMERA_LOSSES if kind == "camera" else ("combined",)):
                r64 = _ref64(kind, sc, loss)
                r32 = ps.reference(kind, sc, *_lists(sc), torch.float32, r64["gates"], loss)
                for k in ps.EXISTING[kind]:
                    scale = r64["S"][k] if k in r64.get("S", {}) else \
                        (np.abs(r64[k]).max() if k in r64 else 0.0)
                    if scale > 0:
                        e = ps.err(r32[k], r64, k)
                        table[(k, name, pose, loss)] = e
                        seen[k] = max(seen.get(k, 0.0), e)
    return seen, table


@pytest.mark.parametrize("kind", ps.KINDS)
def test_pose_float32_spread_constants(kind):
    seen, table = _measure(kind)
    for k, e in sorted(table.items()):
        print(kind, k, f"{e:.2e}")
    print(kind, {k: f"{v:.2e}" for k, v in seen.items()})
    print(kind, "pose / existing:", {k: f"{v / ps.EXISTING[kind][k]:.2f}" for k, v in seen.items()})
    assert set(seen) == set(ps.POSE_F32_SPREAD[kind])
    for k, f in seen.items():
        assert 0.5 * f <= ps.POSE_F32_SPREAD[kind][k] <= 2.0 * f, (k, f, ps.POSE_F32_SPREAD[kind][k])


# ---- 4 --------------------------------------------------------------------------------------------
def _mutant(module, fn, old, new):
    """module.fn with one piece of its text replaced (it must occur exactly once)."""
    src = inspect.getsource(getattr(module, fn))
    assert src.count(old) == 1, (fn, old)
    ns = dict(vars(module))
    exec(compile(src.replace(old, new), f"<mutant of {fn}>", "exec"), ns)
    return ns[fn]


# name -> (module, function, the reference's text, the mutant's, kind, blind at the static pose)
MUTANTS = {
    # A = J R^T
    "A_transposed": (gr, "project", "vm[4 * c_ + r_] for c_ in range(3)",
                     "vm[4 * r_ + c_] for c_ in range(3)", "colour", True),
    # t = R^T p + T: the gradient of the mean goes through the wrong rotation
    "t_transposed": (gr, "project", "vm[k] * x + vm[4 + k] * y + vm[8 + k] * z + vm[12 + k]",
                     "vm[4 * k] * x + vm[4 * k + 1] * y + vm[4 * k + 2] * z + vm[12 + k]",
                     "colour", True),
    # hom = P^T p: rows and columns of the whole projection swapped (the translation moves into
    # the w row, which the static pose sees too)
    "h_transposed": (gr, "project", "pm[k] * x + pm[4 + k] * y + pm[8 + k] * z + pm[12 + k]",
                     "pm[4 * k] * x + pm[4 * k + 1] * y + pm[4 * k + 2] * z + pm[4 * k + 3]",
                     "colour", False),
    # ... and of its 3 x 3 block alone, which is what a swapped index in the backward's dp lines is
    "h_block_transposed": (gr, "project",
                           "pm[k] * x + pm[4 + k] * y + pm[8 + k] * z + pm[12 + k] for k in range(4)",
                           "(pm[4 * k] * x + pm[4 * k + 1] * y + pm[4 * k + 2] * z if k < 3 else "
                           "pm[k] * x + pm[4 + k] * y + pm[8 + k] * z) + pm[12 + k] for k in range(4)",
                           "colour", True),
    # the planes' depth from the view's z column
    "z_column": (pg, "view_depth", "vm[2] * p[:, 0] + vm[6] * p[:, 1] + vm[10] * p[:, 2]",
                 "vm[8] * p[:, 0] + vm[9] * p[:, 1] + vm[10] * p[:, 2]", "planes", True),
    # dir = p + campos
    "campos_negated": (gr, "project", 'd = p - torch.tensor(cam["campos"], dtype=dt)',
                       'd = p + torch.tensor(cam["campos"], dtype=dt)', "colour", False),
}
MUTANT_SCENES = ("chain", "precomputed")


@contextlib.contextmanager
def _patched(module, fn, value):
    old = getattr(module, fn)
    setattr(module, fn, value)
    try:
        yield
    finally:
        setattr(module, fn, old)


def _mutant_errors(mutant, name, pose):
    """{key: (err of the mutant's gradient against the reference's, the GPU tests' bound)} on one
    scene; the mutant runs with the reference's float64 gates."""
    module, fn, old, new, kind, _ = MUTANTS[mutant]
    sc = ps.get(name, pose)
    if (kind == "planes" and name not in ps.PLANE_SCENES) or \
            (mutant == "campos_negated" and sc["colors"] is not None):
        return {}
    ref = _ref64(kind, sc)
    with _patched(module, fn, _mutant(module, fn, old, new)):
        got = ps.reference(kind, sc, *_lists(sc), gates=ref["gates"])
    return {k: (ps.err(got[k], ref, k), ps.bound(kind, k)) for k in ps.POSE_F32_SPREAD[kind]
            if k in ref and np.abs(ref[k]).max() > 0}


@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_at_the_static_pose(mutant):
    """The gap: a mutant that reads a rotation's transpose (or the z column for the z row) is the
    reference itself at the static pose, error exactly 0 on every tensor.  The other two are seen
    there."""
    blind = MUTANTS[mutant][5]
    seen = 0
    for name in MUTANT_SCENES:
        errs = _mutant_errors(mutant, name, "static")
        seen += len(errs)
        print(mutant, name, {k: f"{e:.2e}" for k, (e, _) in errs.items()})
        if blind:
            assert all(e == 0.0 for e, _ in errs.values()), (mutant, name, errs)
        elif errs:
            assert any(e > b for e, b in errs.values()), (mutant, name, errs)
    assert seen >= 4


@pytest.mark.parametrize("pose", ps.NAMES)
@pytest.mark.parametrize("mutant", MUTANTS)
def test_mutants_are_rejected(mutant, pose):
    """At every other pose every mutant exceeds the GPU tests' bound on at least one tensor of
    every scene it runs on."""
    seen = 0
    for name in MUTANT_SCENES:
        errs = _mutant_errors(mutant, name, pose)
        if not errs:
            continue
        seen += 1
        print(mutant, f"{name}@{pose}", {k: f"{e:.2e}" for k, (e, _) in errs.items()})
        assert any(e > b for e, b in errs.values()), (mutant, name, pose, errs)
        assert max(e for e, _ in errs.values()) >= 1e-2  # order 1, not a rounding question
    assert seen >= 1
