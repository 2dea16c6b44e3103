"""GPU: the antialiasing option (gsr_forward_filtered / gsr_backward_filtered) on the
six scenes of aa_scenes, against aa_reference.

  1 the effective opacity: conic_opacity[:, 3] within the float32 bound of the float64 value on
    the judged Gaussians, exactly opacity * sqrtf(0.000025f) on the floor, and every other
    per-Gaussian output and num_rendered bit-equal to the plain forward's
  2 the identity: an antialiased forward is, bit for bit, the plain forward fed o_eff -- image,
    final_T, n_contrib, depth and median planes, the tight lists -- with tight binning and the
    blend cull on and off, both blend arithmetics, a strip, frame graphs mode 1 and 2
  3 per call, not sticky: plain, antialiased, plain on one context and interleaved over two slots
  4 the backward against float64 autograd on the GPU forward's lists, per tensor within 8 x the
    reference's float32 spread (aa_reference.F32_SPREAD), by `_C` and by ctypes, with the planes
    and the camera; exact zeros for culled Gaussians; the floor's gradients
  5 dL_dopacity = s x the plain backward's dL_dopacity at opacities = o_eff
  6 errors   7 antialiasing=False is the call without the argument
"""
import ctypes

import numpy as np
import pytest
import torch

import aa_reference as ar
import aa_scenes
import grad_reference as gr
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer, binning_state,
                                                    rasterize_gaussians_backward_native,
                                                    rasterize_gaussians_native)
from gpu_helpers import ALL_EXTRAS, set_option, to_dev

pytestmark = pytest.mark.gpu

PLANES = ("depth_map", "inv_depth_map", "median_depth", "median_id")
PER_GAUSSIAN = ("depths", "means2D", "rgb", "tiles_touched")
_cache = {}
# (context slots of this file alone: test_gpu_frame_graphs.py hands out slots from 20 upwards,
# test_gpu_tile_starts.py from 200; 147, 149 and 150 are the depth maps' and the median's)
_next_slot = [300]


def _new_slot():
    _next_slot[0] += 1
    return _next_slot[0]


def _args(sc, gpu, opacity=None):
    s, g = sc["s"], sc["s"]["g"]
    P = len(g.xyz)
    sr = sc["cov6"] is None
    sh = None if sc["colors"] is not None else to_dev(g.sh.reshape(P, -1, 3), gpu)
    op = g.opacity if opacity is None else np.asarray(opacity, np.float32).reshape(P, 1)
    return dict(bg=to_dev(s["bg"], gpu), means3D=to_dev(g.xyz, gpu), colors=to_dev(sc["colors"], gpu),
                opacities=to_dev(op, gpu), scales=to_dev(g.scale, gpu) if sr else None,
                rotations=to_dev(g.rot, gpu) if sr else None, mod=s["scale_modifier"],
                cov6=to_dev(sc["cov6"], gpu), view=to_dev(s["view"], gpu),
                proj=to_dev(s["proj"], gpu), tx=s["tx"], ty=s["ty"], sh=sh, deg=s["sh_degree"],
                campos=to_dev(s["campos"], gpu))


def _forward(sc, gpu, aa=None, opacity=None, extras=ALL_EXTRAS, tile_rows=None, slot=0,
             binning=False):
    """One forward as numpy arrays.  aa None: the call without the argument."""
    a = _args(sc, gpu, opacity)
    kw = {} if aa is None else {"antialiasing": aa}
    res = rasterize_gaussians_native(
        a["bg"], a["means3D"], a["colors"], a["opacities"], a["scales"], a["rotations"], a["mod"],
        a["cov6"], a["view"], a["proj"], a["tx"], a["ty"], sc["H"], sc["W"], a["sh"], a["deg"],
        a["campos"], False, False, extras=extras, tile_rows=tile_rows, slot=slot, **kw)
    out = {"num_rendered": res.num_rendered, "color": res.color.cpu().numpy(),
           "radii": res.radii.cpu().numpy()}
    out.update({k: v.cpu().numpy() for k, v in res.extras.items()})
    if binning:
        pl, pt, rg = binning_state(gpu.index or 0, slot)
        out.update(point_list=pl.cpu().numpy(), point_tiles=pt.cpu().numpy(), ranges=rg.cpu().numpy())
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _same(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: {k}")


def _aa_forward(sc, gpu):
    """The antialiased forward with every extra (n_contrib among them: upstream's lists)."""
    key = ("aa", sc["name"])
    if key not in _cache:
        _cache[key] = _forward(sc, gpu, True, binning=True)
    return _cache[key]


def _plain_forward(sc, gpu):
    key = ("plain", sc["name"])
    if key not in _cache:
        _cache[key] = _forward(sc, gpu, None, binning=True)
    return _cache[key]


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_effective_opacity(name, gpu):
    sc = aa_scenes.get(name)
    plain, aa, fv = _plain_forward(sc, gpu), _aa_forward(sc, gpu), ar.forward_value(sc)
    kept = plain["radii"] > 0
    _same(aa, plain, ("radii",) + PER_GAUSSIAN + ("point_list", "point_tiles", "ranges"), name)
    assert aa["num_rendered"] == plain["num_rendered"]
    np.testing.assert_array_equal(_bits(aa["conic_opacity"][:, :3]), _bits(plain["conic_opacity"][:, :3]))
    op = np.asarray(sc["s"]["g"].opacity, np.float32).reshape(-1)
    np.testing.assert_array_equal(_bits(plain["conic_opacity"][kept, 3]), _bits(op[kept]))
    got = aa["conic_opacity"][:, 3]
    assert (got[~kept] == 0).all()
    sel = kept & fv["judged"]
    assert sel.sum() >= 0.9 * kept.sum()
    e = np.abs(got.astype(np.float64) - fv["o_eff"])
    ratio = float((e[sel] / fv["o_eff_bound"][sel]).max())
    print(f"{name}: judged {sel.sum()} of {kept.sum()}, floor {int((sel & fv['floor']).sum())}, "
          f"max err / bound = {ratio:.3f}, max rel err = {(e[sel] / fv['o_eff'][sel]).max():.2e}")
    assert (e[sel] <= fv["o_eff_bound"][sel]).all()
    fl = sel & fv["floor"]
    np.testing.assert_array_equal(_bits(got[fl]), _bits(ar.floor_value(op)[fl]))
    if name in aa_scenes.NEW:
        assert not np.array_equal(aa["color"], plain["color"])


# ---- 2 ------------------------------------------------------------------------------------------
def _identity(sc, gpu, what, slot=0, tile_rows=None, lists=True):
    o_eff = _aa_forward(sc, gpu)["conic_opacity"][:, 3]
    # with n_contrib (upstream's lists) and the planes ...
    ex = ALL_EXTRAS + PLANES
    a = _forward(sc, gpu, True, extras=ex, tile_rows=tile_rows, slot=slot)
    p = _forward(sc, gpu, None, o_eff, extras=ex, tile_rows=tile_rows, slot=slot)
    keys = ("color", "radii", "final_T", "n_contrib", "depths", "means2D", "rgb", "tiles_touched") + PLANES
    _same(a, p, keys, what)
    assert a["num_rendered"] == p["num_rendered"]
    np.testing.assert_array_equal(_bits(a["conic_opacity"]), _bits(p["conic_opacity"]))
    # ... and without it: tight binning (where on), the lists the blend read
    ex = ("final_T",) + PLANES
    a = _forward(sc, gpu, True, extras=ex, tile_rows=tile_rows, slot=slot, binning=lists)
    p = _forward(sc, gpu, None, o_eff, extras=ex, tile_rows=tile_rows, slot=slot, binning=lists)
    _same(a, p, ("color", "radii") + ex + (("point_list", "point_tiles", "ranges") if lists else ()),
          what + " (no n_contrib)")
    assert a["num_rendered"] == p["num_rendered"]
    return a


@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_identity(name, gpu):
    sc = aa_scenes.get(name)
    tight = _identity(sc, gpu, name)
    # the tight lists are in-order subsequences of the plain frame's tight lists
    plain = _forward(sc, gpu, None, extras=(), binning=True)
    assert tight["num_rendered"] == plain["num_rendered"]
    for t, (r0, r1) in enumerate(tight["ranges"].view(np.uint32).astype(int)):
        q0, q1 = plain["ranges"].view(np.uint32).astype(int)[t]
        sub, full = list(tight["point_list"][r0:r1]), iter(plain["point_list"][q0:q1])
        assert all(any(x == y for y in full) for x in sub), f"{name}: tile {t}"
    print(f"{name}: tight list {len(tight['point_list'])} antialiased, {len(plain['point_list'])} "
          f"plain, of {plain['num_rendered']} pairs")
    assert len(tight["point_list"]) <= len(plain["point_list"]) <= plain["num_rendered"]


@pytest.mark.parametrize("opt,value", ((_lib.GSR_OPT_TIGHT_BINNING, 0), (_lib.GSR_OPT_BLEND_CULL, 0),
                                       (_lib.GSR_OPT_BLEND_FAST, 0), (_lib.GSR_OPT_BLEND_FAST, 1)))
def test_identity_under_options(opt, value, gpu):
    slot = _new_slot()
    set_option(gpu, opt, value, slot)
    for name in aa_scenes.NEW:
        _identity(aa_scenes.get(name), gpu, f"{name} option {opt} = {value}", slot=slot)
    assert _lib.get_option(_lib.context(gpu.index or 0, slot), opt) == value


def test_identity_on_a_strip(gpu):
    for name in aa_scenes.NEW:
        for rows in ((0, 1), (1, 2)):
            _identity(aa_scenes.get(name), gpu, f"{name} strip {rows}", tile_rows=rows)


@pytest.mark.parametrize("mode", (1, 2))
def test_identity_with_frame_graphs(mode, gpu):
    slot = _new_slot()
    set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, mode, slot)
    sc = aa_scenes.get("subpixel")
    direct = _identity(sc, gpu, "direct")
    before = _lib.frame_graph_stats(gpu.index or 0, slot)["graph_frames"]
    for _ in range(2):  # (the first frames of a context size its capacity the direct way)
        got = _identity(sc, gpu, f"graphs {mode}", slot=slot)
    _same(got, direct, ("color", "final_T") + PLANES, f"graphs {mode} against direct")
    assert _lib.frame_graph_stats(gpu.index or 0, slot)["graph_frames"] > before


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("graphs", (0, 1))
def test_per_call_not_sticky(graphs, gpu):
    sc = aa_scenes.get("subpixel")
    s1, s2 = _new_slot(), _new_slot()
    for s in (s1, s2):
        set_option(gpu, _lib.GSR_OPT_FRAME_GRAPHS, graphs, s)
    ex = ("final_T", "conic_opacity")
    keys = ("color", "radii") + ex
    want_p = _forward(sc, gpu, None, extras=ex)
    want_a = _forward(sc, gpu, True, extras=ex)
    assert not np.array_equal(want_p["color"], want_a["color"])
    for _ in range(2):  # (graphs: past the sizing frames)
        _forward(sc, gpu, None, extras=ex, slot=s1)
    for i, aa in enumerate((False, True, False, True, True, False)):
        _same(_forward(sc, gpu, aa, extras=ex, slot=s1), want_a if aa else want_p, keys,
              f"slot {s1} frame {i} aa={aa}")
    for i in range(4):  # interleaved over two slots, each alternating the other way
        for s, aa in ((s1, i % 2 == 0), (s2, i % 2 == 1)):
            _same(_forward(sc, gpu, aa, extras=ex, slot=s), want_a if aa else want_p, keys,
                  f"slot {s} round {i} aa={aa}")
    if graphs:
        assert _lib.frame_graph_stats(gpu.index or 0, s1)["graph_frames"] >= 4


# ---- 4 ------------------------------------------------------------------------------------------
def _backward(sc, gpu, loss="colour", camera=False, aa=True, opacity=None, conic=False):
    a = _args(sc, gpu, opacity)
    dL, dLp = ar.loss_gradients(sc, loss)
    kw = {}
    if dLp is not None:
        kw = dict(dL_ddepth_map=to_dev(dLp[0], gpu), dL_dinv_depth_map=to_dev(dLp[1], gpu),
                  dL_dfinal_T=to_dev(dLp[2], gpu))
    if aa is not None:
        kw["antialiasing"] = aa
    g = rasterize_gaussians_backward_native(
        a["bg"], a["means3D"], a["colors"], a["opacities"], a["scales"], a["rotations"], a["mod"],
        a["cov6"], a["view"], a["proj"], a["tx"], a["ty"], to_dev(dL, gpu), a["sh"], a["deg"],
        a["campos"], conic=conic, camera=camera, **kw)
    return {k: v.cpu().numpy().astype(np.float64) for k, v in g.items()}


def _reference(sc, gpu, loss):
    key = ("ref", sc["name"], loss)
    if key not in _cache:
        fwd = _aa_forward(sc, gpu)
        dL, dLp = ar.loss_gradients(sc, loss)
        _cache[key] = ar.scene_gradients(sc, (fwd["ranges"].view(np.uint32), fwd["point_list"].view(np.uint32)),
                                         fwd["radii"], dL, dLp)
        assert _cache[key]["near"][0] == 0 and _cache[key]["near"][2] == 0
    return _cache[key]


NAMES = (("dL_dmeans3D", "means3D"), ("dL_dmeans2D", "means2D"), ("dL_dopacity", "opacity"),
         ("dL_dscales", "scales"), ("dL_drotations", "rotations"), ("dL_dsh", "shs"),
         ("dL_dcov3D", "cov3D"), ("dL_dcolors", "colors"), ("dL_dviewmatrix", "viewmatrix"),
         ("dL_dprojmatrix", "projmatrix"), ("dL_dcampos", "campos"))


def _assert_close(got, ref, what):
    bad = []
    for name, key in NAMES:
        if name not in got or key not in ref or got[name] is None:
            continue
        e = ar.err(got[name].reshape(-1)[:3] if key == "campos" else got[name], ref, key)
        print(f"{what}: e[{key}] = {e:.3e} = {e / ar.F32_SPREAD[key]:.2f} f  (f = "
              f"{ar.F32_SPREAD[key]:.1e}, bound {ar.bound(key):.1e})")
        if not e <= ar.bound(key):
            bad.append(f"{what}: e[{key}] = {e:.3e} > {ar.bound(key):.1e}")
    assert not bad, bad


@pytest.mark.parametrize("loss,camera", (("colour", False), ("combined", False), ("colour", True),
                                         ("combined", True)))
@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_backward_ctypes(name, loss, camera, gpu):
    sc = aa_scenes.get(name)
    ref = _reference(sc, gpu, loss)
    got = _backward(sc, gpu, loss, camera)
    _assert_close(got, ref, f"{name}/{loss}/camera={camera}")
    culled = _aa_forward(sc, gpu)["radii"] == 0
    for k, v in got.items():
        if k not in ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos"):
            assert (v[culled] == 0).all(), k


@pytest.mark.parametrize("mode", ("colour", "planes", "camera"))
@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_backward_autograd(name, mode, gpu):
    """Through GaussianRasterizer (`_C`): the three autograd Functions."""
    sc = aa_scenes.get(name)
    s, a = sc["s"], _args(sc, gpu)
    loss = "colour" if mode == "colour" else "combined"
    ref = _reference(sc, gpu, loss)
    leaves = dict(means3D=a["means3D"], opacities=a["opacities"], shs=a["sh"],
                  colors_precomp=a["colors"], scales=a["scales"], rotations=a["rotations"],
                  cov3D_precomp=a["cov6"])
    for v in leaves.values():
        if v is not None:
            v.requires_grad_(True)
    means2D = torch.zeros_like(a["means3D"], requires_grad=True)
    cam = [a["view"], a["proj"], a["campos"]]
    if mode == "camera":
        for t in cam:
            t.requires_grad_(True)
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], a["bg"], s["scale_modifier"], cam[0], cam[1],
        s["sh_degree"], cam[2], False, False, depth_maps=mode != "colour", antialiasing=True)
    out = GaussianRasterizer(rs)(means2D=means2D, **leaves)
    dL, dLp = ar.loss_gradients(sc, loss)
    total = (out[0] * to_dev(dL, gpu)).sum()
    if dLp is not None:
        total = total + sum((out[2 + i] * to_dev(dLp[i], gpu)).sum() for i in range(3))
    total.backward()
    fwd = _aa_forward(sc, gpu)
    np.testing.assert_array_equal(_bits(out[0].detach().cpu().numpy()), _bits(fwd["color"]))
    grad = lambda t: None if t is None or t.grad is None else t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
    got = dict(dL_dmeans3D=grad(leaves["means3D"]), dL_dmeans2D=grad(means2D),
               dL_dopacity=grad(leaves["opacities"]), dL_dscales=grad(leaves["scales"]),
               dL_drotations=grad(leaves["rotations"]), dL_dsh=grad(leaves["shs"]),
               dL_dcov3D=grad(leaves["cov3D_precomp"]), dL_dcolors=grad(leaves["colors_precomp"]))
    if mode == "camera":
        got.update(dL_dviewmatrix=grad(cam[0]), dL_dprojmatrix=grad(cam[1]), dL_dcampos=grad(cam[2]))
        if sc["colors"] is not None:
            got.pop("dL_dcampos")
    _assert_close({k: v for k, v in got.items() if v is not None}, ref, f"{name}/_C/{mode}")


def test_floor_gradients(gpu):
    """On floor Gaussians dL_dopacity == G * sqrtf(0.000025f) with G the blend's sum, and the
    covariance gets the conic's term alone: dL_dcov3D there is the plain backward's at o_eff."""
    sc = aa_scenes.get("floor")
    fwd, fv = _aa_forward(sc, gpu), ar.forward_value(sc)
    fl = np.flatnonzero(fv["floor"] & fv["judged"] & (fwd["radii"] > 0))
    assert len(fl) >= 10
    ref = _reference(sc, gpu, "colour")
    got = _backward(sc, gpu, conic=True)
    plain = _backward(sc, gpu, aa=None, opacity=fwd["conic_opacity"][:, 3], conic=True)
    G = plain["dL_dopacity"].reshape(-1)
    assert (np.abs(G[fl]) > 0).sum() >= 4
    # one float32 product, on sums whose last bits vary from run to run (atomics)
    want = G[fl] * ar.S_FLOOR
    tol = gr.bound("opacity") * np.abs(ref["G"]).max() * ar.S_FLOOR
    assert np.abs(got["dL_dopacity"].reshape(-1)[fl] - want).max() <= tol
    exact = np.float32(G[fl]) * np.float32(ar.S_FLOOR)
    again = _backward(sc, gpu)["dL_dopacity"].reshape(-1)[fl]
    print("floor: dL_dopacity bit-equal to float32(G) * sqrtf(0.000025f) on",
          int((np.float32(again) == exact).sum()), "of", len(fl))
    scale = np.abs(ref["cov3D"]).max()
    assert np.abs(got["dL_dcov3D"][fl] - plain["dL_dcov3D"][fl]).max() <= gr.bound("cov3D") * scale
    assert np.abs(got["dL_dcov3D"][fl] - ref["cov3D"][fl]).max() <= ar.bound("cov3D") * scale
    # ... while off the floor the new term is there
    off = np.flatnonzero(~fv["floor"] & (fwd["radii"] > 0))
    assert np.abs(got["dL_dcov3D"][off] - plain["dL_dcov3D"][off]).max() > 10 * ar.bound("cov3D") * scale


# ---- 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", aa_scenes.NAMES)
def test_opacity_gradient_is_s_times_the_plain_one(name, gpu):
    sc = aa_scenes.get(name)
    fwd = _aa_forward(sc, gpu)
    ref = _reference(sc, gpu, "colour")
    got = _backward(sc, gpu)["dL_dopacity"].reshape(-1)
    G = _backward(sc, gpu, aa=None, opacity=fwd["conic_opacity"][:, 3])["dL_dopacity"].reshape(-1)
    want = ref["s"] * G
    # bound: the opacity spread (one rounding and the atomics' run-to-run spread lie inside it)
    e = np.abs(got - want).max() / np.abs(ref["opacity"]).max()
    print(f"{name}: max|dL_dopacity - s G| / max|ref| = {e:.3e} (bound {ar.bound('opacity'):.1e})")
    assert e <= ar.bound("opacity")


# ---- 6 ------------------------------------------------------------------------------------------
def test_errors(gpu):
    sc = aa_scenes.get("chain")
    a = _args(sc, gpu)
    P = len(sc["s"]["g"].xyz)
    # antialiasing = 2 at the C ABI: GSR_E_INVALID, outputs untouched
    lib = _lib.load_library()
    fw, bw = _lib.filtered_fns(lib)
    color = torch.full((3, sc["H"], sc["W"]), 7.0, device=gpu)
    radii = torch.full((P,), 7, dtype=torch.int32, device=gpu)
    g = _lib.GsrGaussians(P=P, D=3, M=16, scale_modifier=1.0, means3D=a["means3D"].data_ptr(),
                          scales=a["scales"].data_ptr(), rotations=a["rotations"].data_ptr(),
                          opacities=a["opacities"].data_ptr(), shs=a["sh"].data_ptr())
    st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=a["tx"],
                                tanfovy=a["ty"], viewmatrix=a["view"].data_ptr(),
                                projmatrix=a["proj"].data_ptr(), campos=a["campos"].data_ptr(),
                                bg=a["bg"].data_ptr())
    out = _lib.GsrOutputs(color=color.data_ptr(), radii=radii.data_ptr())
    two = _lib.GsrFilterSettings(antialiasing=2)
    ctx = _lib.context(gpu.index or 0)
    assert fw(ctx, ctypes.byref(g), ctypes.byref(st), ctypes.byref(out), None, None,
              ctypes.byref(two), None) == -1
    d_op = torch.full((P, 1), 7.0, device=gpu)
    dL = to_dev(sc["dL"], gpu)
    assert bw(ctx, ctypes.byref(g), ctypes.byref(st),
              ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=dL.data_ptr())), None, None,
              ctypes.byref(two), ctypes.byref(_lib.GsrGradients(dL_dopacity=d_op.data_ptr())),
              None) == -1
    torch.cuda.synchronize()
    assert (color == 7).all() and (radii == 7).all() and (d_op == 7).all()
    with pytest.raises(RuntimeError, match="antialiasing must be 0 or 1"):
        _forward(sc, gpu, 2)
    # a strip backward is GSR_E_INVALID with the option too
    st.tile_row_begin, st.tile_row_end = 0, 1
    one = _lib.GsrFilterSettings(antialiasing=1)
    with pytest.raises(RuntimeError, match="whole frames only"):
        _lib.check(bw(ctx, ctypes.byref(g), ctypes.byref(st),
                      ctypes.byref(_lib.GsrBackwardInputs(dL_dcolor=dL.data_ptr())), None, None,
                      ctypes.byref(one), ctypes.byref(_lib.GsrGradients(dL_dopacity=d_op.data_ptr())),
                      None), "gsr_backward_filtered")
    assert (d_op == 7).all()
    # antialiasing with a shading: RuntimeError, natively and through the rasterizer
    s = sc["s"]
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], a["bg"], s["scale_modifier"], a["view"], a["proj"],
        s["sh_degree"], a["campos"], False, False, _lib.GSR_SHADE_FLAT_BALL, antialiasing=True)
    with pytest.raises(RuntimeError, match="antialiasing belongs to the splat composite"):
        GaussianRasterizer(rs)(means3D=a["means3D"], means2D=None, opacities=a["opacities"],
                               shs=a["sh"], scales=a["scales"], rotations=a["rotations"])


# ---- 7 ------------------------------------------------------------------------------------------
def test_false_is_the_call_without_the_argument(gpu):
    sc = aa_scenes.get("subpixel")
    ex = ALL_EXTRAS + PLANES
    _same(_forward(sc, gpu, False, extras=ex, binning=True), _forward(sc, gpu, None, extras=ex, binning=True),
          ("color", "radii", "point_list", "point_tiles", "ranges") + ex, "forward")
    # ... and at the C ABI: a NULL filter and antialiasing = 0 are gsr_forward_surface itself
    want = _forward(sc, gpu, None, extras=("final_T",))
    a = _args(sc, gpu)
    P = len(sc["s"]["g"].xyz)
    g = _lib.GsrGaussians(P=P, D=3, M=16, scale_modifier=1.0, means3D=a["means3D"].data_ptr(),
                          scales=a["scales"].data_ptr(), rotations=a["rotations"].data_ptr(),
                          opacities=a["opacities"].data_ptr(), shs=a["sh"].data_ptr())
    st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=a["tx"],
                                tanfovy=a["ty"], viewmatrix=a["view"].data_ptr(),
                                projmatrix=a["proj"].data_ptr(), campos=a["campos"].data_ptr(),
                                bg=a["bg"].data_ptr())
    fw = _lib.filtered_fns(_lib.load_library())[0]
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    for f in (None, ctypes.byref(_lib.GsrFilterSettings(antialiasing=0))):
        color = torch.empty((3, sc["H"], sc["W"]), device=gpu)
        radii = torch.empty((P,), dtype=torch.int32, device=gpu)
        final_T = torch.empty((sc["H"], sc["W"]), device=gpu)
        out = _lib.GsrOutputs(color=color.data_ptr(), radii=radii.data_ptr(), final_T=final_T.data_ptr())
        _lib.check(fw(_lib.context(gpu.index or 0), ctypes.byref(g), ctypes.byref(st),
                      ctypes.byref(out), None, None, f, stream), "gsr_forward_filtered")
        _same(dict(color=color.cpu().numpy(), radii=radii.cpu().numpy(), final_T=final_T.cpu().numpy()),
              want, ("color", "radii", "final_T"), "C ABI, filter off")
        assert out.num_rendered == want["num_rendered"]
    # the backward: antialiasing=False is the very call without the argument; its sums over
    # pixels are float atomics, whose last bits vary from run to run, so two runs are held to
    # the float32 spread of each tensor (a term of the option would show at order 1)
    x, y = (_backward(sc, gpu, "combined", True, aa=v) for v in (False, None))
    ref = _reference(sc, gpu, "combined")
    for name, key in NAMES:
        if name in x:
            scale = ref["S"][key] if key in ref["S"] else np.abs(y[name]).max()
            assert np.abs(x[name] - y[name]).max() <= ar.bound(key) * scale, name
    # and through the rasterizer: antialiasing=False settings render the plain bits
    s, ar_ = sc["s"], _args(sc, gpu)
    base = (sc["H"], sc["W"], s["tx"], s["ty"], ar_["bg"], s["scale_modifier"], ar_["view"],
            ar_["proj"], s["sh_degree"], ar_["campos"], False, False)
    kw = dict(means3D=ar_["means3D"], means2D=None, opacities=ar_["opacities"], shs=ar_["sh"],
              scales=ar_["scales"], rotations=ar_["rotations"])
    c0, _ = GaussianRasterizer(GaussianRasterizationSettings(*base))(**kw)
    c1, _ = GaussianRasterizer(GaussianRasterizationSettings(*base, antialiasing=False))(**kw)
    c2, _ = GaussianRasterizer(GaussianRasterizationSettings(*base, antialiasing=True))(**kw)
    assert torch.equal(c0, c1) and not torch.equal(c0, c2)
    np.testing.assert_array_equal(_bits(c2.cpu().numpy()), _bits(_aa_forward(sc, gpu)["color"]))
