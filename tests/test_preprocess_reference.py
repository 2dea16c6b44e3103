"""CPU: the per-Gaussian stage of the oracle on the edge scenes of preprocess_scenes.py.

1. Order-exact: the C oracle equals the pure-Python float32 restatement (py_preprocess of
   test_oracle_restatement.py, which covers cov3D_precomp, colors_precomp, scale_modifier, M in
   1, 4, 9, 16 and the non-positive-radius rule) on every Gaussian of every scene, bit for bit
   where finite and NaN where NaN.
2. Float64: on the scenes that are not built on a threshold, the oracle's decisions equal the
   float64 reference's (preprocess_reference.py) on stable Gaussians and its floats lie within
   their bounds; the unstable share stays under the project's cap; a wrong constant is caught.
3. A non-positive saturated radius (NaN radius) is culled, and oracle.forward renders it.
Each scene is also shown to reach the edge it was built for, on the oracle alone.
"""
import numpy as np
import pytest

from gaussiansplattingviewer_amd.camera import cuda_camera_inputs, static_camera

import blend_scenes as bs
import preprocess_reference as pr
import preprocess_scenes as ps
from gpu_helpers import UNSTABLE_CAP, blend_reference
from test_oracle_restatement import py_preprocess

F32 = np.float32


@pytest.mark.parametrize("name", ps.NAMES)
def test_oracle_equals_python_restatement(oracle_mod, name):
    sc = ps.get(oracle_mod, name)
    orc = ps.run(oracle_mod, sc)
    s = sc["s"]
    g = s["g"]
    view, proj = s["view"].reshape(-1), s["proj"].reshape(-1)
    nvis = 0
    for i in range(len(g)):
        e = py_preprocess(i, g, view, proj, s["campos"], s["tx"], s["ty"], s["W"], s["H"],
                          s["sh_degree"], scale_modifier=s["scale_modifier"],
                          cov3D_precomp=sc["cov6"], colors_precomp=sc["colors"])
        if e is None:
            assert orc["radii"][i] == 0 and orc["tiles_touched"][i] == 0, (name, i)
            continue
        nvis += 1
        assert orc["radii"][i] == e["radius"], (name, i)
        assert orc["tiles_touched"][i] == e["tiles"], (name, i)
        ps.assert_bits_or_nan(orc["depths"][i], e["depth"], f"{name} depth {i}")
        ps.assert_bits_or_nan(orc["means2D"][i], F32(e["xy"]), f"{name} means2D {i}")
        ps.assert_bits_or_nan(orc["conic_opacity"][i, :3], F32(e["conic"]), f"{name} conic {i}")
        if e["rgb"] is not None:
            ps.assert_bits_or_nan(orc["rgb"][i], F32(e["rgb"]), f"{name} rgb {i}")
    assert nvis == int((orc["radii"] > 0).sum()) and nvis > 0
    # the invariant of test_oracle_properties.py holds on hostile input too
    np.testing.assert_array_equal(orc["radii"] > 0, orc["tiles_touched"] > 0)
    assert orc["num_rendered"] == int(orc["tiles_touched"].sum())


def test_scenes_are_small_and_interleaved(oracle_mod):
    for name in ps.NAMES:
        sc = ps.get(oracle_mod, name)
        sp = sc["special"]
        assert sc["W"] <= 160 and sc["H"] <= 120 and len(sp) <= 600, name
        if not name.startswith("boundaries_"):
            assert (~sp).sum() == ps.N_ORD, name
            # no run of 64 (a wave) without an ordinary Gaussian, where there are that many
            runs = np.diff(np.flatnonzero(np.concatenate([[True], ~sp, [True]])))
            assert runs.max() <= 64, name


def test_near_plane_lands_on_its_depths(oracle_mod):
    sc = ps.get(oracle_mod, "near_plane")
    orc = ps.run(oracle_mod, sc)
    sp = np.flatnonzero(sc["special"])
    want = sc["depth_targets"]
    assert set(want.tolist()) == set(F32(ps.NEAR_TARGETS).tolist())
    np.testing.assert_array_equal(ps.view_z32(sc["s"]["g"].xyz[sp], sc["s"]["view"]), want)
    near = want <= F32(0.2)
    assert near.sum() == 3 * len(ps.NEAR_LATERAL)
    assert (orc["radii"][sp[near]] == 0).all()            # z = 0.2 itself is culled
    assert (orc["radii"][sp[~near]] > 0).all()
    np.testing.assert_array_equal(orc["depths"][sp[~near]], want[~near])
    assert orc["radii"][sp].max() <= 16                    # modest radii at depth 0.2


def test_clamp_straddles_the_limit(oracle_mod):
    sc = ps.get(oracle_mod, "clamp")
    orc = ps.run(oracle_mod, sc)
    s = sc["s"]
    sp = np.flatnonzero(sc["special"])
    assert (orc["radii"][sp] > 0).all()  # every rect still reaches the frame
    xyz = s["g"].xyz[sp]
    for axis, tan in ((0, s["tx"]), (1, s["ty"])):
        lim = F32(1.3) * F32(tan)
        on = xyz[:, 1 - axis] == 0
        ratio = np.abs(xyz[on, axis] / F32(4.0)) / lim  # |t / t.z| in float32, over the limit
        for r in ps.CLAMP_RATIOS:
            assert (np.abs(ratio - r) < 1e-5 * r).sum() >= 2, (axis, r)
        assert (ratio < 1).any() and (ratio > 1).any() and (xyz[on, axis] > 0).any() \
            and (xyz[on, axis] < 0).any()


@pytest.mark.parametrize("frame", ps.RECT_FRAMES)
def test_rect_edges_straddle_tile_boundaries(oracle_mod, frame):
    W, H = frame
    sc = ps.get(oracle_mod, f"rect_edges_{W}x{H}")
    orc = ps.run(oracle_mod, sc)
    sp = np.flatnonzero(sc["special"])
    assert (orc["radii"][sp][orc["radii"][sp] > 0] == ps.RECT_R).all()
    kinds = sc["kinds"]
    exact = 0
    for axis, what in sorted({(a, w) for a, w, _ in kinds}):
        d = [dd for a, w, dd in kinds if (a, w) == (axis, what)]
        assert min(d) < 0 < max(d), (axis, what)  # a centre below and one above the boundary
        # ... no further off than two float32 steps at the centre's magnitude
        assert max(abs(v) for v in d) <= 2.5 * float(np.spacing(F32(64.0))), (axis, what, d)
        exact += 0.0 in d
    assert exact >= 1 or (W, H) == (1, 1)
    # rects that end at column / row 0 or start at the grid's end from outside are empty, their
    # neighbours one float inside are not; negative centres occur
    m2 = orc["means2D"][sp]
    assert (orc["tiles_touched"][sp] == 0).any() and (orc["tiles_touched"][sp] > 0).any()
    assert (sc["s"]["g"].xyz[sp][:, 0] < -1).any()


def test_radius_ceil_sits_on_the_jump(oracle_mod):
    sc = ps.get(oracle_mod, "radius_ceil")
    orc = ps.run(oracle_mod, sc)
    sp = np.flatnonzero(sc["special"])
    np.testing.assert_array_equal(orc["radii"][sp], sc["radius_want"])
    assert set(sc["radius_want"].tolist()) == set(range(3, 42))


def test_det_cancel_reaches_all_three_classes(oracle_mod):
    sc = ps.get(oracle_mod, "det_cancel")
    orc = ps.run(oracle_mod, sc)
    sp = np.flatnonzero(sc["special"])
    # specials sit inside the frame at depth 4 with a radius of thousands of px: the only cull
    # left is det == 0; otherwise conic.x = cov.z / det has det's sign (cov.z > 0)
    zero = orc["radii"][sp] == 0
    neg = ~zero & (orc["conic_opacity"][sp, 0] < 0)
    pos = ~zero & (orc["conic_opacity"][sp, 0] > 0)
    print(f"det_cancel: det == 0: {zero.sum()}, det < 0: {neg.sum()}, det > 0: {pos.sum()}")
    assert zero.sum() >= 5 and neg.sum() >= 5 and pos.sum() >= 5
    assert zero.sum() + neg.sum() + pos.sum() == len(sp)


@pytest.mark.parametrize("key", ps.SCALE_MODS)
def test_scale_range_reaches_saturation_and_nan_conics(oracle_mod, key):
    sc = ps.get(oracle_mod, f"scale_range_{key}")
    orc = ps.run(oracle_mod, sc)
    assert np.isfinite(orc["color"]).all()
    if ps.SCALE_MODS[key] > 0:
        assert (orc["radii"] == ps.INT_MAX).any()
        nan_conic = np.isnan(orc["conic_opacity"][:, :3]).any(axis=1)
        assert (nan_conic & (orc["radii"] > 0)).any()
    else:  # every covariance is 0: the low-pass alone, radius ceil(3 sqrt(0.3 + sqrt(0.1))) = 3
        assert set(orc["radii"][sc["special"]].tolist()) <= {0, 3}


@pytest.mark.parametrize("name", ["nonfinite", "nonfinite_precomp"])
def test_nonfinite_inputs_render_finite_pixels(oracle_mod, name):
    sc = ps.get(oracle_mod, name)
    orc = ps.run(oracle_mod, sc)
    assert len(sc["poisons"]) == int(sc["special"].sum())
    assert {repr(v) for _, _, v in sc["poisons"]} == {"nan", "inf", "-inf"}
    assert np.isfinite(ps.features(sc, orc)).all()
    assert np.isfinite(orc["color"]).all() and np.isfinite(orc["final_T"]).all()
    # the ordinary Gaussians are those of the same scene without the poisoned ones
    sp = sc["special"]
    assert (orc["radii"][~sp] > 0).sum() >= 20


def test_sh_edges_reach_their_edges(oracle_mod):
    half = ps.sh_half_coefficient()
    assert F32(ps.SH_C0 * half) == F32(-0.5)
    for D, M in ps.SH_PAIRS:
        sc = ps.get(oracle_mod, f"sh_edges_{D}_{M}")
        orc = ps.run(oracle_mod, sc)
        g = sc["s"]["g"]
        assert g.sh.shape[1] == 3 * M and sc["s"]["sh_degree"] == D
        sp = np.flatnonzero(sc["special"])
        assert (orc["radii"][sp] > 0).all()
        d = g.xyz[sp] - sc["s"]["campos"]
        assert ((d != 0).sum(axis=1) == 0).sum() == 1          # a mean equal to campos
        for axis in range(3):                                  # both signs along each axis
            on = ((d != 0).sum(axis=1) == 1) & (d[:, axis] != 0)
            assert (d[on, axis] > 0).any() and (d[on, axis] < 0).any()
        rgb = orc["rgb"][sp]
        assert (rgb == 0).any() and (rgb >= 1e29).any() and np.isfinite(rgb).all()
        assert (orc["clamped"][sp].any(axis=1)).any()
        # exactly -0.5 + 0.5: a zero that the clamp did not make
        assert ((rgb == 0) & (orc["clamped"][sp] == 0)).any()


@pytest.mark.parametrize("P", ps.BOUNDARY_PS)
def test_boundaries_cull_about_a_third(oracle_mod, P):
    sc = ps.get(oracle_mod, f"boundaries_{P}")
    orc = ps.run(oracle_mod, sc)
    culled = float((orc["radii"] == 0).mean())
    assert len(orc["radii"]) == P and (P == 1 or 0.25 <= culled <= 0.45), culled


# ---- 2. the float64 reference --------------------------------------------------------------
F64_SCENES = tuple(n for n in ps.NAMES if not n.startswith(ps.THRESHOLD_BUILT)
                   and not n.startswith("nonfinite")) + ("synthetic",)


def _f64_scene(oracle_mod, name):
    if name == "synthetic":
        sc = bs.build(oracle_mod, "synthetic")  # 3k synthetic_gaussians at 160x120
        return sc, bs.run(oracle_mod, sc)
    sc = ps.get(oracle_mod, name)
    return sc, ps.run(oracle_mod, sc)


@pytest.mark.parametrize("name", F64_SCENES)
def test_oracle_within_float64_bounds(oracle_mod, name):
    sc, orc = _f64_scene(oracle_mod, name)
    ref = pr.evaluate(sc)
    ratios = pr.check(ref, orc, name)
    print(f"{name}: judged {int((ref['stable'] & ref['finite']).sum())} of {len(ref['stable'])}, " +
          ", ".join(f"{k} {v:.3g}" for k, v in ratios.items()))
    assert ratios["unstable"] <= UNSTABLE_CAP, f"{name}: {ratios['unstable']:.4f} unstable"
    assert (ref["stable"] & ref["finite"] & ref["visible"]).sum() >= 1
    if name.startswith("scale_range") and ps.SCALE_MODS[name.rsplit("_", 1)[1]] > 0:
        assert (~ref["finite"]).any()  # the 1e15 scales leave float32's range


def test_conic_bound_carries_its_conditioning(oracle_mod):
    sc, _ = _f64_scene(oracle_mod, "synthetic")
    ref = pr.evaluate(sc)
    v = ref["visible"] & ref["finite"]
    rel = (ref["conic_bound"][v] / np.abs(ref["conic"][v]))[:, 0]
    cond = ref["conditioning"][v]
    assert (rel >= pr.U * cond).all()
    assert np.corrcoef(np.log(rel), np.log(cond))[0, 1] > 0.5


@pytest.mark.parametrize("const", ["SH_C3", "LOW_PASS", "CLAMP"])
def test_reference_catches_a_wrong_constant(oracle_mod, monkeypatch, const):
    """The check has teeth: with one of upstream's constants 1e-4 (relative) off in the
    reference, the oracle no longer agrees with it."""
    if const == "SH_C3":
        monkeypatch.setattr(pr, "SH_C3", [pr.SH_C3[0] * (1 + 1e-4)] + pr.SH_C3[1:])
        name = "synthetic"
    else:
        monkeypatch.setattr(pr, const, getattr(pr, const) * (1 + 1e-4))
        name = "clamp"
    sc, orc = _f64_scene(oracle_mod, name)
    with pytest.raises(AssertionError):
        pr.check(pr.evaluate(sc), orc, name)


def test_blend_is_decidable_where_it_is_held_exact(oracle_mod):
    """The scenes on which the GPU test also holds the blend to its float64 reference
    (assert_blend_exact) are those with finite colours and conics on which the oracle alone meets
    the unstable-pixel cap; the others are named, with the reason."""
    for name in ps.NAMES:
        sc = ps.get(oracle_mod, name)
        orc = ps.run(oracle_mod, sc)
        if not ps.finite_records(sc, orc):
            assert name in ps.BLEND_NOT_EXACT, name
            continue
        st = blend_reference(oracle_mod, orc, sc["s"]["bg"], ps.features(sc, orc))["stable"]
        share = 1.0 - float(st.mean())
        print(f"{name}: blend unstable share {share:.4f}")
        assert (share <= UNSTABLE_CAP) == (name not in ps.BLEND_NOT_EXACT), (name, share)


# ---- 3. the non-positive radius --------------------------------------------------------------
def _one_gaussian(oracle_mod, scale=(0.01, 0.01, 0.01), rot=(1, 0, 0, 0), cov6=None):
    W, H = 40, 24
    view, proj, campos, tx, ty = cuda_camera_inputs(static_camera(W, H))
    kw = dict(cov3D_precomp=F32([cov6])) if cov6 is not None else \
        dict(scales=F32([scale]), rotations=F32([rot]))
    return oracle_mod.forward(F32([[0, 0, 0]]), F32([0.5]), view, proj, campos, tx, ty, W, H,
                              colors_precomp=F32([[1, 0.5, 0.25]]), bg=(0.1, 0.2, 0.3), **kw)


NAN = float("nan")
POISONED = {
    "scale_inf": dict(scale=(np.inf, 0.01, 0.01)),
    "scale_1e25": dict(scale=(1e25, 1e25, 1e25)),
    "scale_3e19": dict(scale=(3e19, 3e19, 3e19)),
    "scale_nan": dict(scale=(NAN, NAN, NAN)),
    "quat_nan": dict(rot=(1, NAN, 0, 0)),
    # indefinite, negative trace: lambda1 < 0 under the square root
    "cov_negative_trace": dict(cov6=(-1.0, 0.0, 0.0, -2.0, 0.0, 1e-8)),
}


@pytest.mark.parametrize("case", sorted(POISONED))
def test_nonpositive_radius_is_culled(oracle_mod, case):
    r = _one_gaussian(oracle_mod, **POISONED[case])  # oracle_bin no longer fails with -3
    assert r["radii"][0] == 0 and r["tiles_touched"][0] == 0 and r["num_rendered"] == 0
    assert len(r["point_list"]) == 0
    np.testing.assert_array_equal(r["color"], np.broadcast_to(F32([0.1, 0.2, 0.3])[:, None, None],
                                                              r["color"].shape))


def test_ordinary_single_gaussian_is_kept(oracle_mod):
    r = _one_gaussian(oracle_mod)
    assert r["radii"][0] > 0 and r["num_rendered"] == r["tiles_touched"][0] > 0
