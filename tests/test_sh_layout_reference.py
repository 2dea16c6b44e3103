"""CPU: the conditions on the scenes of the SH-layout tests (sh_layout_scenes), met by the oracle and
grad_reference alone, and the measured numbers the GPU tests (test_gpu_sh_layouts.py) are held to.

  - no decision within rounding of its gate in any base scene;
  - 15 % to 45 % of the colour channels on the clamp's flat side at every degree;
  - the culled Gaussians are culled, the last one is visible and has a gradient;
  - every layout variant holds the base's active coefficients bit for bit, and the oracle renders
    it to the base's bits: the oracle is layout-invariant, so the GPU's identities are claims
    about the kernels alone;
  - the float32 spread per SH band (BAND_SPREAD) is what a float32 evaluation gives here, and the
    whole-tensor spreads stay within grad_reference.F32_SPREAD, whose bounds then apply unchanged.
"""
import numpy as np
import pytest
import torch

import grad_reference as gr
import oracle
import sh_layout_scenes as L
from gpu_helpers import run_oracle

_orc, _ref = {}, {}


def _oracle(sc):
    if sc["name"] not in _orc:
        _orc[sc["name"]] = run_oracle(oracle, sc["s"])
    return _orc[sc["name"]]


def _ref64(sc):
    if sc["name"] not in _ref:
        orc = _oracle(sc)
        _ref[sc["name"]] = gr.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                              sc["dL"])
    return _ref[sc["name"]]


@pytest.mark.parametrize("base", L.BASES)
def test_scene_shapes(base):
    sc = L.get(base)
    g, orc = sc["s"]["g"], _oracle(sc)
    assert (len(g.xyz), sc["W"], sc["H"], sc["M"], sc["D"]) == (96, 40, 24, 16, L.degree(base))
    assert g.sh.shape == (96, 48) and sc["s"]["sh_degree"] == sc["D"]
    counts = orc["ranges"][:, 1].astype(int) - orc["ranges"][:, 0].astype(int)
    assert len(counts) == 6 and (counts > 0).all()
    assert (orc["radii"][L.CULLED] == 0).all() and orc["radii"][-1] > 0
    ref = _ref64(sc)
    assert np.abs(ref["shs"][-1]).max() > 0 and np.abs(ref["means3D"][-1]).max() > 0
    n = (sc["D"] + 1) ** 2
    assert (ref["shs"][:, n:] == 0).all() and (ref["shs"][L.CULLED] == 0).all()
    for l in range(sc["D"] + 1):
        assert np.abs(ref["shs"][:, L.band(l)]).max() > 0
    # the coefficients above the active degree are there, and not 0: they must be ignored
    assert (g.sh[:, 3 * n:] != 0).all()
    # one geometry under the four degrees
    for k in ("xyz", "rot", "scale", "opacity", "sh"):
        np.testing.assert_array_equal(getattr(g, k), getattr(L.get("deg3")["s"]["g"], k))


@pytest.mark.parametrize("base", L.BASES)
def test_no_decision_near_its_gate(base):
    assert _ref64(L.get(base))["near"] == (0, 0)


@pytest.mark.parametrize("base", L.BASES)
def test_clamped_share(base):
    """The G[ch] = 0 gate is taken and not taken, at every degree."""
    clamped = _ref64(L.get(base))["gates"][0]["clamped"].numpy()
    share = float(clamped.mean())
    print(f"{base}: {share:.3f} of the colour channels clamped")
    assert 0.15 <= share <= 0.45
    assert clamped.any(axis=1).sum() >= 10 and (~clamped).all(axis=1).sum() >= 10


@pytest.mark.parametrize("base", L.BASES)
def test_variants_hold_the_base_and_the_oracle_is_layout_invariant(base):
    b = L.get(base)
    D, n = b["D"], (b["D"] + 1) ** 2
    want_M = {"tight": n, "mid": (D + 2) ** 2, "off4": 16, "wide": 25, "poison": 16}
    names = L.variants(base)
    assert set(names) == {"tight", "off4", "wide"} | ({"mid"} if D < 2 else set()) | \
        ({"poison"} if D < 3 else set())
    ob = _oracle(b)
    for v in names:
        sc = L.get(base, v)
        sh, M = sc["s"]["g"].sh, sc["M"]
        assert M == want_M[v] and sh.shape == (96, 3 * M) and M >= n
        assert sc["unaligned"] == (v == "off4")
        np.testing.assert_array_equal(sh[:, :3 * n].view(np.uint32),
                                      b["s"]["g"].sh[:, :3 * n].view(np.uint32))
        if v == "poison":
            assert np.isnan(sh[:, 3 * n:]).all()
        else:
            assert np.isfinite(sh).all()
            m = min(M, 16)
            np.testing.assert_array_equal(sh[:, :3 * m], b["s"]["g"].sh[:, :3 * m])
        if v == "wide":
            assert (sh[:, 48:] != 0).all()
        for k in ("xyz", "rot", "scale", "opacity"):
            assert getattr(sc["s"]["g"], k) is getattr(b["s"]["g"], k)
        assert sc["dL"] is b["dL"]
        ov = _oracle(sc)
        assert ov["num_rendered"] == ob["num_rendered"]
        for k in ("rgb", "color", "final_T", "n_contrib", "radii", "point_list", "ranges"):
            x, y = np.ascontiguousarray(ov[k]), np.ascontiguousarray(ob[k])
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32), err_msg=f"{v}: {k}")
        assert np.isfinite(ov["color"]).all() and np.isfinite(ov["rgb"]).all()


def test_reference_is_layout_invariant():
    """grad_reference gives a variant the base's gradients, and zeros above the degree."""
    for base, v in (("deg1", "tight"), ("deg2", "wide"), ("deg0", "poison")):
        b, sc = L.get(base), L.get(base, v)
        rb, ob = _ref64(b), _oracle(b)
        rv = gr.scene_gradients(sc, (ob["ranges"], ob["point_list"]), ob["radii"], sc["dL"])
        n, m = (b["D"] + 1) ** 2, min(sc["M"], 16)
        for k in ("means3D", "means2D", "opacity", "scales", "rotations"):
            np.testing.assert_array_equal(rv[k], rb[k], err_msg=k)
        np.testing.assert_array_equal(rv["shs"][:, :m], rb["shs"][:, :m])
        assert rv["shs"].shape == (96, sc["M"], 3) and (rv["shs"][:, n:] == 0).all()


def test_image_gradient_parts():
    """dL_masks: every pixel in exactly one part, a part inside at most two of the blend
    backward's 8 x 8 quadrants (its waves); the gradients of the parts add up to the whole
    image's, and no part puts a decision within rounding of its gate."""
    masks = L.dL_masks()
    assert len(masks) == 8 and all(m.shape == (L.H, L.W) and m.dtype == np.float32 for m in masks)
    assert (np.sum(masks, axis=0) == 1).all() and all(set(np.unique(m)) <= {0.0, 1.0} for m in masks)
    for m in masks:
        quads = {(y // 8, x // 8) for y, x in np.argwhere(m > 0)}
        assert 1 <= len(quads) <= 2
        assert m.sum() == sum(min(8, L.H - 8 * qy) * min(8, L.W - 8 * qx) for qy, qx in quads)
    sc = L.get("deg3")
    orc, whole = _oracle(sc), _ref64(sc)
    parts = [gr.scene_gradients(dict(sc), (orc["ranges"], orc["point_list"]), orc["radii"],
                                sc["dL"] * m) for m in masks]
    for k in ("shs", "means3D", "rgb"):
        total = sum(p[k] for p in parts)
        assert np.abs(total - whole[k]).max() <= 1e-12 * np.abs(whole[k]).max()
    assert all(p["near"] == (0, 0) for p in parts)


def test_float32_spread_per_band():
    """BAND_SPREAD is what a float32 evaluation of the reference gives here, to within a factor 2
    either way; and no base scene's whole-tensor spread exceeds grad_reference.F32_SPREAD."""
    bad = []
    for base in L.BASES:
        sc = L.get(base)
        orc, r64 = _oracle(sc), _ref64(sc)
        r32 = gr.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"], sc["dL"],
                                 torch.float32, r64["gates"])
        whole = {k: gr.rel_err(r32[k], r64[k]) for k in gr.F32_SPREAD
                 if k in r64 and np.abs(r64[k]).max() > 0}
        assert set(whole) == set(gr.F32_SPREAD) - {"cov3D", "colors"}
        bands = [gr.rel_err(r32["shs"][:, L.band(l)], r64["shs"][:, L.band(l)])
                 for l in range(sc["D"] + 1)]
        print(base, "bands", [f"{f:.2e}" for f in bands],
              "whole / F32_SPREAD", {k: f"{f / gr.F32_SPREAD[k]:.2f}" for k, f in whole.items()})
        assert len(L.BAND_SPREAD[base]) == sc["D"] + 1
        for l, f in enumerate(bands):
            if not 0.5 * f <= L.BAND_SPREAD[base][l] <= 2.0 * f:
                bad.append((base, l, f, L.BAND_SPREAD[base][l]))
        bad += [(base, k, f, gr.F32_SPREAD[k]) for k, f in whole.items() if f > gr.F32_SPREAD[k]]
    assert not bad, bad
