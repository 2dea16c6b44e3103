"""CPU: pins the reference of the antialiasing tests (aa_reference) -- its autograd against the
closed-form terms include/gsr.h states and against central differences, the conditions on the six
scenes (aa_scenes), the float32 spread the GPU tolerance is built from -- and the Python and host
side of the option: the settings tuple, the exported entry points and their validation without
a device."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import aa_reference as ar
import aa_scenes
import grad_reference as gr
import oracle
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    rasterize_gaussians_backward_native,
                                                    rasterize_gaussians_native)
from gaussiansplattingviewer_amd.renderer import HIPRenderer
from gpu_helpers import run_oracle

# long_lists, as grad_scenes builds it, has one (pixel, splat) pair whose termination product
# T (1 - alpha) lies 1.9e-6 relative above 1e-4 under the effective opacities -- inside
# grad_reference's 1e-3 net for that gate, about 20 float32 ulp from it.  The scene is taken as
# it is; every other count is 0.
NEAR_COMPOSITE = {"long_lists": 1}


def _oracle(sc):
    if "orc" not in sc:
        sc["orc"] = run_oracle(oracle, sc["s"], colors_precomp=sc["colors"],
                               cov3D_precomp=sc["cov6"])
    return sc["orc"]


def _ref64(sc, loss="colour"):
    key = "aa64_" + loss
    if key not in sc:
        orc = _oracle(sc)
        dL, dLp = ar.loss_gradients(sc, loss)
        sc[key] = ar.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"], dL, dLp)
    return sc[key]


@pytest.mark.parametrize("name", aa_scenes.NEW)
def test_scene_shapes(name):
    """The two new scenes hold what aa_scenes says."""
    sc = aa_scenes.get(name)
    orc, fv = _oracle(sc), ar.forward_value(sc)
    kept = orc["radii"] > 0
    P = len(kept)
    assert P <= 200 and (sc["W"], sc["H"]) == (40, 24) and kept.all()
    counts = orc["ranges"][:, 1].astype(int) - orc["ranges"][:, 0].astype(int)
    assert len(counts) == 6 and (counts > 0).all()
    sp = sc["special"]
    if name == "subpixel":
        rho = fv["rho"]
        assert rho.min() < 0.01 and rho.max() > 0.85 and not fv["floor"].any()
        assert (rho[sp["needles"]] < 0.01).all() and (rho[sp["needles"]] > 40 * ar.FLOOR).all()
        assert (np.median(rho) > 0.05) and ((rho > 0.01) & (rho < 0.9)).mean() > 0.9
        faint = fv["o_eff"] < gr.A_MIN
        assert faint[sp["faint"]].sum() >= 5
        # the needles' D0 cancels: its bound is >= 1e-3 of the value, the others' ~1e-5
        rel = fv["rho_bound"] / fv["rho"]
        assert (rel[sp["needles"]] > 1e-3).all() and np.median(rel) < 1e-4
    else:
        assert (fv["rho"][sp["zero"]] == 0).all() and fv["floor"][sp["zero"]].all()
        assert fv["floor"][sp["discs"]].all() and (np.abs(fv["rho"][sp["discs"]]) < 0.1 * ar.FLOOR).all()
        rest = np.setdiff1d(np.arange(P), np.concatenate([sp["zero"], sp["discs"]]))
        assert not fv["floor"][rest].any()
        # some floor Gaussians still reach a pixel: their dL/do_eff is not zero
        r = _ref64(sc)
        assert (np.abs(r["G"][sp["zero"]]) > 0).sum() >= 2 and (np.abs(r["G"][sp["discs"]]) > 0).any()


@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_no_gaussian_near_the_floor_unflagged(name):
    """forward_value flags every Gaussian whose floor decision (or det != 0, or the z cull) could
    change within the float32 bound and judges the others: at most 10 % of the kept are left out,
    by the reference alone.  The float64 restatement takes the same floor decisions and finds
    none within a float32 evaluation's reach of the gate."""
    sc = aa_scenes.get(name)
    orc, fv = _oracle(sc), ar.forward_value(sc)
    kept = orc["radii"] > 0
    assert kept.sum() > 0 and (fv["judged"] & kept).sum() >= 0.9 * kept.sum()
    near_gate = np.abs(fv["rho"] - ar.FLOOR) <= fv["rho_bound"]
    assert not (near_gate & fv["judged"]).any()
    for loss in ar.LOSSES:
        r = _ref64(sc, loss)
        assert r["near"] == (0, NEAR_COMPOSITE.get(name, 0), 0), r["near"]
        np.testing.assert_array_equal(r["floor"][kept & fv["judged"]],
                                      fv["floor"][kept & fv["judged"]])


@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_forward_value_matches_the_restatement(name):
    """o_eff of the float64 torch restatement lies within forward_value's float32 bound of it on
    the judged Gaussians (two statements of one formula), and on the floor both give
    opacity * sqrtf(0.000025f)."""
    sc = aa_scenes.get(name)
    orc, fv, r = _oracle(sc), ar.forward_value(sc), _ref64(sc)
    sel = (orc["radii"] > 0) & fv["judged"]
    assert (np.abs(r["o_eff"] - fv["o_eff"])[sel] <= fv["o_eff_bound"][sel]).all()
    fl = sel & fv["floor"]
    op = np.asarray(sc["s"]["g"].opacity, np.float32).reshape(-1)
    assert np.abs(r["o_eff"][fl] - ar.floor_value(op)[fl]).max(initial=0) <= 1e-9


@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_autograd_agrees_with_the_closed_form(name):
    """d o_eff / d(opacity, a', b, c') by autograd (b the one stored off-diagonal entry), by the
    closed-form terms of include/gsr.h and by central differences, in float64 on the scene's own
    2D covariances; zeros on the floor's flat side."""
    sc = aa_scenes.get(name)
    orc, r = _oracle(sc), _ref64(sc)
    kept = np.flatnonzero(orc["radii"] > 0)
    a0, b, c0, _ = (v[kept] for v in r["cov2"])
    op = np.asarray(sc["s"]["g"].opacity, np.float64).reshape(-1)[kept]
    G = np.random.default_rng(3).standard_normal(len(kept))

    def o_eff(x):
        a0_, b_, c0_, op_ = x
        det = (a0_ + gr.LOW_PASS) * (c0_ + gr.LOW_PASS) - b_ * b_
        s, floor, _ = ar.factor(a0_, b_, c0_, det, torch.as_tensor(r["floor"][kept]))
        return op_ * s
    x = [torch.tensor(v, requires_grad=True) for v in (a0, b, c0, op)]
    (o_eff(x) * torch.tensor(G)).sum().backward()
    s, d_op, d_a, d_b, d_c = ar.closed_form(a0, b, c0, op, G)
    np.testing.assert_array_equal(s == ar.S_FLOOR, r["floor"][kept])
    for got, want in ((x[3].grad, d_op), (x[0].grad, d_a), (x[1].grad, d_b), (x[2].grad, d_c)):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-10, atol=1e-12 * np.abs(want).max())
    fl = r["floor"][kept]
    for g in (x[0].grad, x[1].grad, x[2].grad):
        assert (g.numpy()[fl] == 0).all()
    # central differences, per variable, with a step relative to the 2D covariance's size
    with torch.no_grad():
        for k, want in ((0, d_a), (1, d_b), (2, d_c)):
            h = 1e-6 * (np.abs(a0) + np.abs(c0) + 0.3)
            xp = [v.detach().clone() for v in x]
            xm = [v.detach().clone() for v in x]
            xp[k] += torch.tensor(h)
            xm[k] -= torch.tensor(h)
            num = ((o_eff(xp) - o_eff(xm)).numpy() * G) / (2 * h)
            scale = np.abs(want).max() if np.abs(want).max() > 0 else 1.0
            # (a needle's rho curves sharply in b: second order in h, still ~1e-5 of the largest)
            assert np.abs(num - want).max() <= 1e-4 * scale, (k, np.abs(num - want).max() / scale)


def test_gradcheck_through_the_scene():
    """torch.autograd.gradcheck of o_eff through the per-Gaussian stage, on the needles and a
    few ordinary Gaussians of `subpixel`."""
    sc = aa_scenes.get("subpixel")
    cam = gr.camera_constants(sc["s"])
    g = sc["s"]["g"]
    ids = np.array([0, 1, 2, 10, 11, 12])
    t = lambda a: torch.tensor(np.asarray(a, np.float32)[ids].astype(np.float64), requires_grad=True)  # noqa: E731
    means3D, scales, rot, op = t(g.xyz), t(g.scale), t(g.rot), t(g.opacity.reshape(-1))
    camera = ar.cgr.camera_of(sc["s"])
    P = len(ids)
    radii = np.ones(P, np.int32)
    zeros = torch.zeros((P, 3), dtype=torch.float64)
    colors = torch.zeros((P, 3), dtype=torch.float64)

    def fn(means3D, scales, rot, op, vm):
        vmP, pmP, cP = (v.reshape(1, -1).expand(P, -1) for v in (vm, camera[1], camera[2]))
        _, _, _, _, (a0, b, c0, det), gates, near = ar.project(
            cam, radii, vmP, pmP, cP, means3D, zeros, scales, rot, None, None, colors)
        assert near == 0
        s, floor, near_f = ar.factor(a0, b, c0, det)
        assert near_f == 0 and not floor.any()
        return op * s
    assert torch.autograd.gradcheck(fn, (means3D, scales, rot, op, camera[0]), eps=1e-6,
                                    atol=1e-6, rtol=1e-4)


def test_float32_spread_constants():
    """F32_SPREAD (the GPU tests' yardstick) is what a float32 evaluation of the reference gives
    here, over the six scenes and the two losses, to within a factor 2 either way."""
    seen = {}
    for name in aa_scenes.NAMES:
        sc = aa_scenes.get(name)
        orc = _oracle(sc)
        for loss in ar.LOSSES:
            r64 = _ref64(sc, loss)
            dL, dLp = ar.loss_gradients(sc, loss)
            r32 = ar.scene_gradients(sc, (orc["ranges"], orc["point_list"]), orc["radii"], dL, dLp,
                                     torch.float32, r64["gates"])
            for k in ar.F32_SPREAD:
                if k in r64 and np.abs(r64[k]).max() > 0:
                    seen[k] = max(seen.get(k, 0.0), ar.err(r32[k], r64, k))
    print({k: f"{v:.3e}" for k, v in seen.items()})
    assert set(seen) == set(ar.F32_SPREAD)
    for k, f in seen.items():
        assert 0.5 * f <= ar.F32_SPREAD[k] <= 2.0 * f, (k, f, ar.F32_SPREAD[k])


def test_plain_restatement_is_grad_reference():
    """With antialiasing off the restatement is grad_reference's, gradient for gradient."""
    sc = aa_scenes.get("chain")
    orc = _oracle(sc)
    lists = (orc["ranges"], orc["point_list"])
    mine = ar.scene_gradients(sc, lists, orc["radii"], sc["dL"], antialiasing=False)
    theirs = gr.scene_gradients(sc, lists, orc["radii"], sc["dL"])
    for k in gr.LEAVES:
        if k in theirs:
            assert gr.rel_err(mine[k], theirs[k]) <= 1e-12, k


# ---- the Python API -----------------------------------------------------------------------------
def _settings_args():
    bg = torch.zeros(3)
    return (24, 40, 0.5, 0.3, bg, 1.0, torch.eye(4), torch.eye(4), 3, torch.zeros(3), False, False)


def test_settings_tuple():
    """antialiasing is keyword only and an attribute like depth_maps: `_fields`, positional
    construction, unpacking and comparison stay those of the 13-field tuple; `_replace` carries
    it; `_make` gives False."""
    a = _settings_args()
    S = GaussianRasterizationSettings
    plain = S(*a)
    assert plain.antialiasing is False and plain.depth_maps is False and plain.shading == 0
    assert S._fields[-1] == "shading" and len(S._fields) == 13
    assert "antialiasing" not in S._fields and "antialiasing" not in S._field_defaults
    aa = S(*a, antialiasing=True)
    assert aa.antialiasing is True and aa.depth_maps is False
    assert len(aa) == 13 and tuple(aa)[:4] == tuple(plain)[:4]
    assert all(x is y for x, y in zip(aa, plain))  # equality and unpacking: the tuple's
    # positional: 13 arguments end at shading, the 14th is depth_maps, a 15th is an error
    s13 = S(*a, 2)
    assert s13.shading == 2 and not s13.depth_maps and not s13.antialiasing
    s14 = S(*a, 0, True)
    assert s14.shading == 0 and s14.depth_maps is True and s14.antialiasing is False
    with pytest.raises(TypeError):
        S(*a, 0, True, True)
    both = S(*a, 0, True, antialiasing=1)
    assert both.depth_maps is True and both.antialiasing is True
    # upstream's keyword construction
    kw = dict(zip(S._fields, a))
    assert S(**kw, antialiasing=True).antialiasing is True
    # _replace carries it and can set it; _make gives False
    assert aa._replace(sh_degree=1).antialiasing is True
    assert aa._replace(sh_degree=1).sh_degree == 1
    assert plain._replace(antialiasing=True).antialiasing is True
    assert aa._replace(antialiasing=False).antialiasing is False
    assert both._replace(shading=1).depth_maps is True and both._replace(shading=1).antialiasing
    made = S._make(tuple(aa))
    assert made.antialiasing is False and made.depth_maps is False


def test_keywords_of_the_native_entries_and_the_renderer():
    for fn in (rasterize_gaussians_native, rasterize_gaussians_backward_native):
        p = inspect.signature(fn).parameters["antialiasing"]
        assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    r = HIPRenderer(40, 24, device="cpu", antialiasing=True)
    assert r.antialiasing is True and HIPRenderer(40, 24, device="cpu").antialiasing is False
    with pytest.raises(RuntimeError, match="antialiasing belongs to the splat composite"):
        rasterize_gaussians_native(None, torch.zeros(4, 3), None, None, None, None, 1.0, None,
                                   None, None, 1.0, 1.0, 8, 8, None, 0, None, False, False,
                                   shading=_lib.GSR_SHADE_FLAT_BALL, antialiasing=True)


def test_filtered_host_abi():
    """gsr_forward_filtered and gsr_backward_filtered are exported and validate before any device
    call: a value other than 0 or 1 is GSR_E_INVALID whatever else is passed; a NULL filter and
    antialiasing = 0 take gsr_forward_surface's / gsr_backward_camera's checks; a strip backward is
    GSR_E_INVALID with the option too.  The ABI version stays 4."""
    lib = _lib.load_library()
    assert lib.gsr_abi_version() == _lib.ABI_VERSION == 4
    for n in ("gsr_forward_filtered", "gsr_backward_filtered"):
        assert n in _lib.EXPORTED_SYMBOLS and hasattr(lib, n)
    fw, bw = _lib.filtered_fns(lib)
    assert ctypes.sizeof(_lib.GsrFilterSettings) == 4
    ctx = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)  # never dereferenced
    g, st = _lib.GsrGaussians(P=4), _lib.GsrRasterSettings(image_width=8, image_height=8)
    out, inp, gr_ = _lib.GsrOutputs(), _lib.GsrBackwardInputs(), _lib.GsrGradients()
    ref = ctypes.byref
    for v in (2, -1, 255):
        f = _lib.GsrFilterSettings(antialiasing=v)
        assert fw(ctx, ref(g), ref(st), ref(out), None, None, ref(f), None) == -1
        assert b"antialiasing must be 0 or 1" in lib.gsr_last_error()
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, ref(f), ref(gr_), None) == -1
        assert b"antialiasing must be 0 or 1" in lib.gsr_last_error()
    for f in (None, ref(_lib.GsrFilterSettings(antialiasing=0)),
              ref(_lib.GsrFilterSettings(antialiasing=1))):
        assert fw(None, ref(g), ref(st), ref(out), None, None, f, None) == -1
        assert fw(ctx, None, ref(st), ref(out), None, None, f, None) == -1
        assert bw(ctx, ref(g), ref(st), None, None, None, f, ref(gr_), None) == -1
        st.tile_row_begin, st.tile_row_end = 0, 1
        assert bw(ctx, ref(g), ref(st), ref(inp), None, None, f, ref(gr_), None) == -1
        assert b"whole frames only" in lib.gsr_last_error()
        st.tile_row_end = 0
