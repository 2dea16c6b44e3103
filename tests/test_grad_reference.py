"""CPU: pins the reference of the backward-pass tests (grad_reference) against the oracles the
forward is pinned by, checks it with torch.autograd.gradcheck, asserts the condition on the test
scenes (no decision within rounding of its gate) and re-measures the float32 spread the GPU
tolerance is built from.  Also the host side of gsr_backward: exported, validating without a
device, ABI version unchanged."""
import ctypes

import numpy as np
import pytest
import torch

import grad_reference as gr
import grad_scenes
import oracle
import preprocess_reference as pref
from gaussiansplattingviewer_amd import _lib
from gpu_helpers import run_oracle


def _oracle(sc):
    if "orc" not in sc:
        sc["orc"] = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"],
                               cov3D_precomp=sc["cov6"])
    return sc["orc"]


def _ref64(sc):
    if "ref64" not in sc:
        orc = _oracle(sc)
        sc["ref64"] = gr.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"],
                                         sc["dL"])
    return sc["ref64"]


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_scene_shapes(name):
    """Each scene holds what its description says (grad_scenes docstring)."""
    sc = grad_scenes.get(name)
    orc = _oracle(sc)
    counts = orc["ranges"][:, 1].astype(int) - orc["ranges"][:, 0].astype(int)
    if name == "chain":
        assert (sc["W"], sc["H"], len(counts)) == (40, 24, 6) and (counts > 0).all()
    if name == "long_lists":
        assert len(counts) == 2 and all(128 < c <= 192 and c % 2 == 1 for c in counts)
        f64 = oracle.render_f64(orc["ranges"], orc["point_list"], orc["means2D"],
                                orc["conic_opacity"], orc["rgb"], sc["s"]["bg"], sc["W"], sc["H"])
        assert (f64["flags"] & oracle.F64_CAP).any() and (f64["flags"] & oracle.F64_TERM).any()
    if name == "edges":
        sp = sc["special"]
        assert (orc["radii"][sp["clamp"]] > 0).all()
        assert (orc["radii"][sp["behind"]] == 0).all() and (orc["radii"][sp["det0"]] == 0).all()
        gates = _ref64(sc)["gates"][0]
        vis = np.flatnonzero(orc["radii"] > 0)
        beyond = (gates["lo0"] | gates["hi0"] | gates["lo1"] | gates["hi1"]).numpy()
        assert set(sp["clamp"]) <= set(vis[beyond])
        assert 0.25 <= gates["clamped"].numpy().mean() <= 0.45


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_project_matches_the_oracle(name):
    """project (float64) against oracle.forward's per-Gaussian outputs (float32), within the
    bounds preprocess_reference derives for a float32 evaluation."""
    sc = grad_scenes.get(name)
    orc, ref = _oracle(sc), pref.evaluate(sc)
    lv = gr.leaves(sc, torch.float64)
    with torch.no_grad():
        m2, conic, rgb, _, _ = gr.project(gr.camera_constants(sc["s"]), orc["radii"], lv["means3D"],
                                          lv["means2D"], lv.get("scales"), lv.get("rotations"),
                                          lv.get("cov3D"), lv.get("shs"), lv.get("colors"))
    sel = ref["stable"] & ref["finite"] & ref["visible"] & (orc["radii"] > 0)
    assert sel.sum() >= 0.9 * (orc["radii"] > 0).sum()
    pairs = [(m2.numpy(), orc["means2D"], ref["means2D_bound"]),
             (conic.numpy(), orc["conic_opacity"][:, :3], ref["conic_bound"])]
    if sc["colors"] is None:
        pairs.append((rgb.numpy(), orc["rgb"], ref["rgb_bound"]))
    for mine, theirs, bnd in pairs:
        assert (np.abs(mine - theirs.astype(np.float64))[sel] <= bnd[sel]).all()


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_composite_matches_render_f64(name):
    sc = grad_scenes.get(name)
    orc = _oracle(sc)
    feat = orc["rgb"] if sc["colors"] is None else sc["colors"]
    f64 = oracle.render_f64(orc["ranges"], orc["point_list"], orc["means2D"], orc["conic_opacity"],
                            feat, sc["s"]["bg"], sc["W"], sc["H"])
    t = lambda a: torch.tensor(np.asarray(a, np.float32).astype(np.float64))  # noqa: E731
    with torch.no_grad():
        color, _, near = gr.composite((orc["ranges"], orc["point_list"]), t(orc["means2D"]),
                                      t(orc["conic_opacity"][:, :3]), t(orc["conic_opacity"][:, 3]),
                                      t(feat), sc["s"]["bg"], sc["W"], sc["H"])
    assert near == 0
    assert np.abs(color.numpy() - f64["color"]).max() <= 1e-12


@pytest.mark.parametrize("name", grad_scenes.NAMES)
def test_no_decision_near_its_gate(name):
    assert _ref64(grad_scenes.get(name))["near"] == (0, 0)


def _tiny():
    """4 Gaussians on an 8 x 8 frame, kept away from every gate."""
    from gaussiansplattingviewer_amd.camera import static_camera
    from gaussiansplattingviewer_amd.gaussian_data import GaussianData
    from gpu_helpers import scene_inputs
    rng = np.random.default_rng(5)
    a = lambda v: np.ascontiguousarray(v, np.float32)  # noqa: E731
    rot = rng.standard_normal((4, 4))
    g = GaussianData(a(rng.uniform(-0.25, 0.25, (4, 3))), a(rot / np.linalg.norm(rot, axis=1)[:, None]),
                     a(rng.uniform(0.15, 0.3, (4, 3))), a(rng.uniform(0.3, 0.6, (4, 1))),
                     a(np.concatenate([rng.normal(0.5, 0.3, (4, 3)), rng.normal(0, 0.1, (4, 45))], 1)))
    s = scene_inputs(g, static_camera(8, 8), 3, bg=(0.3, 0.6, 0.1), scale_modifier=1.3)
    return dict(name="tiny", s=s, colors=None, cov6=None, W=8, H=8)


def test_gradcheck():
    sc = _tiny()
    orc = _oracle(sc)
    assert (orc["radii"] > 0).all()
    lists = (orc["ranges"], orc["point_list"])
    cam = gr.camera_constants(sc["s"])
    lv = gr.leaves(sc, torch.float64)
    keys = ("means3D", "means2D", "scales", "rotations", "shs")
    _, _, _, gates_p, near_p = gr.project(cam, orc["radii"], *(lv[k] for k in keys[:4]), None,
                                          lv["shs"])

    def proj(*x):
        return gr.project(cam, orc["radii"], x[0], x[1], x[2], x[3], None, x[4], None, gates_p)[:3]
    assert torch.autograd.gradcheck(proj, tuple(lv[k] for k in keys), eps=1e-6, atol=1e-7)
    with torch.no_grad():
        m2, conic, rgb = proj(*(lv[k] for k in keys))
    leaves = [v.clone().requires_grad_(True) for v in (m2, conic, lv["opacity"].detach(), rgb)]
    _, gates_c, near_c = gr.composite(lists, *leaves, sc["s"]["bg"], 8, 8)
    assert (near_p, near_c) == (0, 0)

    def comp(*x):
        return gr.composite(lists, *x, sc["s"]["bg"], 8, 8, gates_c)[0]
    assert torch.autograd.gradcheck(comp, tuple(leaves), eps=1e-6, atol=1e-7)


def test_float32_spread_constants():
    """F32_SPREAD (the GPU tests' yardstick) is what a float32 evaluation of the reference gives
    here, to within a factor 2 either way."""
    seen = {}
    for name in grad_scenes.NAMES:
        sc = grad_scenes.get(name)
        orc, r64 = _oracle(sc), _ref64(sc)
        r32 = gr.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"], sc["dL"],
                                 torch.float32, r64["gates"])
        for k in gr.F32_SPREAD:
            if k in r64 and np.abs(r64[k]).max() > 0:
                seen[k] = max(seen.get(k, 0.0), gr.rel_err(r32[k], r64[k]))
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(gr.F32_SPREAD)
    for k, f in seen.items():
        assert 0.5 * f <= gr.F32_SPREAD[k] <= 2.0 * f, (k, f, gr.F32_SPREAD[k])


def test_backward_host_abi():
    """gsr_backward is exported and validates before any device call; the ABI version stays 4."""
    lib = _lib.load_library()
    assert "gsr_backward" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "gsr_backward")
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4
    fn = _lib.backward_fn(lib)
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    g, st = _lib.GsrGaussians(P=4), _lib.GsrRasterSettings(image_width=8, image_height=8)
    inp, out = _lib.GsrBackwardInputs(), _lib.GsrGradients()
    ref = ctypes.byref
    for args in ((None, ref(g), ref(st), ref(inp), ref(out)), (ctx, None, ref(st), ref(inp), ref(out)),
                 (ctx, ref(g), None, ref(inp), ref(out)), (ctx, ref(g), ref(st), None, ref(out)),
                 (ctx, ref(g), ref(st), ref(inp), None)):
        assert fn(*args, None) == -1  # GSR_E_INVALID
    st.tile_row_begin, st.tile_row_end = 0, 1
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(out), None) == -1
    assert b"whole frames only" in lib.gsr_last_error()
    st.tile_row_end = 0
    g.P = -1
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(out), None) == -1
    g.P = 4  # dL_dcolor missing, then neither colour form, then both covariance forms
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(out), None) == -1
    inp.dL_dcolor = 64
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(out), None) == -1
    assert b"SHs or precomputed colors" in lib.gsr_last_error()
    g.shs = g.scales = g.rotations = g.cov3D_precomp = 64
    assert fn(ctx, ref(g), ref(st), ref(inp), ref(out), None) == -1
    assert b"precomputed 3D covariance" in lib.gsr_last_error()
