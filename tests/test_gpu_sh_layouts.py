"""GPU: every SH layout a caller can pass, through both forms of the per-Gaussian kernels' row
access (12 float4 for M == 16 at 16-byte aligned pointers, float by float otherwise), forward and
backward, on the scenes of sh_layout_scenes.  The conditions on the scenes and the oracle's own
layout invariance are test_sh_layout_reference.py's (CPU).

  1 forward: every layout variant renders the base scene's bits (the base is held to the oracle by
    assert_parity), with all extras and with none; no NaN from the poisoned rows
  2 forward: compacted strip frames of layouts the compacted-id colour pass refuses (k_color_generic)
    against the rows of the uncompacted full frame, bit for bit
  3 backward: every layout variant gives the base scene's gradients bit for bit, exact zeros above
    the active degree (columns 16 .. 24 of M = 25 among them) and for culled Gaussians, no NaN
  4 the same through the planes', the camera's and the antialiased kernels, and all three at once
  5 backward through the C ABI: dL_dsh at an unaligned pointer, and short and long rows at aligned
    ones, inside a buffer of sentinel words that must stay untouched
  6 backward against float64 autograd, per tensor (grad_reference.bound) and per SH band
    (BOUND_FACTOR x sh_layout_scenes.BAND_SPREAD), by ctypes and through `_C`

Every SH tensor lives inside a larger device buffer whose words before and after the rows are NaN
(_sh_dev): a read past the rows that reaches an output shows.

Bit identity between two backward calls (3, 4, 5).  The per-Gaussian kernel is a function of the
Gaussian's inputs and of its row of 2D gradients, the blend kernel's sums over pixels.  Those sums
are float atomics in the order the waves arrive: with a gradient on every pixel two calls on the
same inputs, the base scene's own among them, differ in the last bits of many rows (include/gsr.h
says so of gsr_backward; measured here: of the 96 rows of deg0, eight were found in none of four
further calls).  The comparisons therefore hand the image gradient to the kernels in the eight
parts of sh_layout_scenes.dL_masks, two of the blend's waves to a part, one call per part: a row
then has at most two non-zero addends, the calls are reproducible bit for bit (asserted: the base
scene is compared with a second call of itself like any variant), and the identity is asserted
on every tensor of every part, the camera's sums included.
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_reference as gr
import sh_layout_scenes as L
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.camera import static_camera
from gaussiansplattingviewer_amd.gaussian_data import GaussianData, synthetic_gaussians
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer, binning_state,
                                                    rasterize_gaussians_backward_native,
                                                    rasterize_gaussians_native)
from gpu_helpers import (ALL_EXTRAS, assert_parity, run_hip, run_oracle, scene_inputs, set_option,
                         to_dev, to_dev_unaligned)

pytestmark = pytest.mark.gpu

GUARD = 64          # NaN (inputs) or sentinel (outputs) words either side of the rows
SENTINEL = -559038737  # 0xDEADBEEF as int32
MODES = ("plain", "planes", "camera", "aa", "all")
CAMERA = ("dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos")

_dev, _fwd, _bwd, _ref = {}, {}, {}, {}
worst = {}  # (check, key) -> the largest e / bound seen (test_report_worst_ratio prints it)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def _guarded(rows, gpu, unaligned=False):
    """rows on the device between GUARD NaN words, 16-byte aligned or 4 bytes past that."""
    rows = np.ascontiguousarray(rows, np.float32)
    pad = np.full(GUARD, np.nan, np.float32)
    flat = np.concatenate([pad, rows.reshape(-1), pad])
    buf = to_dev_unaligned(flat, gpu) if unaligned else to_dev(flat, gpu)
    view = buf[GUARD:GUARD + rows.size].view(rows.shape)
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 if unaligned else 0)
    assert torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + rows.size:]).all()
    return view


def _sh_dev(sc, gpu):
    """The scene's (P, M, 3) SH tensor on the device, guarded (once per scene)."""
    if sc["name"] not in _dev:
        g = sc["s"]["g"]
        _dev[sc["name"]] = _guarded(g.sh.reshape(len(g.xyz), sc["M"], 3), gpu, sc["unaligned"])
    return _dev[sc["name"]]


def _render(s, sh, gpu, extras=ALL_EXTRAS, tile_rows=None, radii=True):
    """gpu_helpers.run_hip with the SH tensor given (its pointer is the point)."""
    g = s["g"]
    res = rasterize_gaussians_native(
        to_dev(s["bg"], gpu), to_dev(g.xyz, gpu), None, to_dev(g.opacity, gpu),
        to_dev(g.scale, gpu), to_dev(g.rot, gpu), s["scale_modifier"], None, to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], s["H"], s["W"], sh, s["sh_degree"],
        to_dev(s["campos"], gpu), False, False, tile_rows=tile_rows, extras=extras, radii=radii)
    out = {"num_rendered": res.num_rendered, "color": res.color.cpu().numpy()}
    if res.radii is not None:
        out["radii"] = res.radii.cpu().numpy()
    out.update({k: v.cpu().numpy() for k, v in res.extras.items()})
    pl, _, rg = binning_state(gpu.index or 0)
    out.update(point_list=pl.cpu().numpy(), ranges=rg.cpu().numpy())
    return out


def _same(a, b, keys, what):
    for k in keys:
        np.testing.assert_array_equal(_bits(a[k]), _bits(b[k]), err_msg=f"{what}: {k}")


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", L.BASES)
def test_forward_layout_invariance(base, gpu, oracle_mod):
    b = L.get(base)
    hip = run_hip(b["s"], gpu)
    assert_parity(hip, run_oracle(oracle_mod, b["s"]))
    culled = b["special"]["culled"]
    assert (hip["radii"][culled] == 0).all() and hip["radii"][-1] > 0
    full = _render(b["s"], _sh_dev(b, gpu), gpu)
    _same(full, hip, ("rgb", "color", "final_T", "n_contrib", "radii", "point_list", "ranges"), base)
    lean = _render(b["s"], _sh_dev(b, gpu), gpu, extras=())  # the viewer's call
    for v in L.variants(base):
        sc = L.get(base, v)
        sh = _sh_dev(sc, gpu)
        assert tuple(sh.shape) == (L.P, sc["M"], 3)
        got = _render(sc["s"], sh, gpu)
        _same(got, full, ("rgb", "color", "final_T", "n_contrib", "radii", "point_list", "ranges"),
              sc["name"])
        assert got["num_rendered"] == full["num_rendered"]
        got0 = _render(sc["s"], sh, gpu, extras=())
        _same(got0, lean, ("color", "radii", "point_list", "ranges"), sc["name"] + " (no extras)")
        for k in ("rgb", "color", "final_T", "conic_opacity", "means2D", "depths"):
            assert np.isfinite(got[k]).all(), (sc["name"], k)
        assert np.isfinite(got0["color"]).all()


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", (1, 3))
@pytest.mark.parametrize("D,M,unaligned", ((2, 9, False), (1, 16, False), (3, 16, True)))
def test_compacted_strip_generic_colour(D, M, unaligned, form, gpu):
    """Compacted strip frames (GSR_OPT_DEPTH_SORT 1 or 3, forced) colour through k_color_ids only
    at degree 3 with vector rows; these three layouts take k_color_generic instead.  Every strip
    is the same rows of the full, uncompacted frame, with and without the radii output."""
    W, H = 160, 96
    g = synthetic_gaussians(2000, 3, 7)
    g = GaussianData(g.xyz, g.rot, g.scale, g.opacity, np.ascontiguousarray(g.sh[:, :3 * M]))
    s = scene_inputs(g, static_camera(W, H), D)
    sh = _guarded(g.sh.reshape(len(g.xyz), M, 3), gpu, unaligned)
    pix = ("final_T", "n_contrib")  # no "rgb"
    full = _render(s, sh, gpu, extras=pix)
    assert full["num_rendered"] > 1000 and (full["n_contrib"] > 0).mean() > 0.2
    assert np.isfinite(full["color"]).all()
    set_option(gpu, _lib.GSR_OPT_DEPTH_SORT, form)
    try:
        for rows in ((0, 2), (2, 4), (4, 6)):
            y0, y1 = 16 * rows[0], 16 * rows[1]
            part = _render(s, sh, gpu, extras=pix, tile_rows=rows)
            want = dict(color=full["color"][:, y0:y1], final_T=full["final_T"][y0:y1],
                        n_contrib=full["n_contrib"][y0:y1], radii=full["radii"])
            _same(part, want, ("color", "final_T", "n_contrib", "radii"), f"strip {rows}")
            lean = _render(s, sh, gpu, extras=pix, tile_rows=rows, radii=False)
            _same(lean, part, ("color", "final_T", "n_contrib", "point_list"), f"strip {rows}, no radii")
    finally:
        set_option(gpu, _lib.GSR_OPT_DEPTH_SORT, -1)


# ---- 3, 4 -----------------------------------------------------------------------------------------
def _plane_gradients():
    rng = np.random.default_rng(77)
    return [np.ascontiguousarray(rng.standard_normal((L.H, L.W)), np.float32) for _ in range(3)]


def _backward(sc, gpu, mode="plain", conic=True, part=None):
    """One backward call as numpy arrays.  part: the image gradient (and the planes') on that part
    of dL_masks only (default: everywhere)."""
    s, g = sc["s"], sc["s"]["g"]
    mask = 1.0 if part is None else L.dL_masks()[part]
    kw = {}
    if mode in ("planes", "all"):
        d, i, t = (to_dev(p * mask, gpu) for p in _plane_gradients())
        kw.update(dL_ddepth_map=d, dL_dinv_depth_map=i, dL_dfinal_T=t, depths=True)
    if mode in ("camera", "all"):
        kw["camera"] = True
    if mode in ("aa", "all"):
        kw["antialiasing"] = True
    out = rasterize_gaussians_backward_native(
        to_dev(s["bg"], gpu), to_dev(g.xyz, gpu), None, to_dev(g.opacity, gpu),
        to_dev(g.scale, gpu), to_dev(g.rot, gpu), s["scale_modifier"], None, to_dev(s["view"], gpu),
        to_dev(s["proj"], gpu), s["tx"], s["ty"], to_dev(sc["dL"] * mask, gpu), _sh_dev(sc, gpu),
        s["sh_degree"], to_dev(s["campos"], gpu), conic=conic, **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


def _base_call(base, gpu, mode, part):
    """The base scene's call in a mode on a part (kept: every variant is compared with the same)."""
    key = (base, mode, part)
    if key not in _bwd:
        _bwd[key] = _backward(L.get(base), gpu, mode, part=part)
    return _bwd[key]


def _same_bits(got, ref, cols, what):
    """Every tensor of a call bit for bit another call's; dL_dsh over its first `cols` columns."""
    assert set(got) == set(ref), what
    for k, v in got.items():
        w = ref[k]
        if k == "dL_dsh":
            v, w = v[:, :cols], w[:, :cols]
        bad = _bits(v) != _bits(w)
        rows = np.flatnonzero(bad.reshape(len(bad), -1).any(axis=1))
        assert not bad.any(), f"{what}: {k} differs from the base scene's bits in rows {rows[:8]}"


def _layout_identity(base, variant, mode, gpu):
    """Checks 3 and 4 for one layout in one mode, over the parts; returns the parts' dL_dsh and
    dL_dcolors added up (what the whole image gradient reaches)."""
    b, sc = L.get(base), L.get(base, variant)
    n = (sc["D"] + 1) ** 2
    total = {"dL_dsh": 0.0, "dL_dcolors": 0.0, "dL_dmeans3D": 0.0}
    for part in range(len(L.dL_masks())):
        what = f"{sc['name']}/{mode}/part {part}"
        got = _backward(sc, gpu, mode, part=part)
        assert got["dL_dsh"].shape == (L.P, sc["M"], 3)
        for k, v in got.items():
            assert np.isfinite(v).all(), (what, k)
            if k not in CAMERA:
                assert (v[b["special"]["culled"]] == 0).all(), (what, k)
        assert (got["dL_dsh"][:, n:] == 0).all(), what
        assert ("dL_ddepths" in got) == (mode in ("planes", "all"))
        assert all((k in got) == (mode in ("camera", "all")) for k in CAMERA)
        _same_bits(got, _base_call(base, gpu, mode, part), min(sc["M"], 16), what)
        for k in total:
            total[k] = total[k] + np.abs(got[k].astype(np.float64))
        if mode in ("camera", "all"):
            assert np.abs(got["dL_dcampos"]).max() > 0 and np.abs(got["dL_dviewmatrix"]).max() > 0
    # the parts together reach every band, the last Gaussian, and every Gaussian on a list
    for l in range(sc["D"] + 1):
        assert total["dL_dsh"][:, L.band(l)].max() > 0
    assert total["dL_dsh"][-1].max() > 0 and total["dL_dmeans3D"][-1].max() > 0
    return total


@pytest.mark.parametrize("base", L.BASES)
def test_backward_layout_invariance(base, gpu):
    """Check 3.  The base scene goes through the same comparison: a second call of it has the
    first one's bits, part by part (the premise of comparing calls at all)."""
    listed = np.zeros(L.P, bool)
    listed[np.unique(run_hip(L.get(base)["s"], gpu)["point_list"])] = True
    for v in ("base",) + L.variants(base):
        total = _layout_identity(base, v, "plain", gpu)
        reached = total["dL_dcolors"].max(axis=1) > 0
        # ... the Gaussians the float64 reference gives a colour gradient (no decision of its
        # composite is within rounding of a gate: the same pairs contribute here)
        assert (reached <= listed).all()
        assert (reached == (np.abs(_reference(base, gpu)["rgb"]).max(axis=1) > 0)).all()
    # the clamp's gate was taken and not taken: channels of dL_dsh at 0 beside non-zero ones
    dc = total["dL_dsh"][:, 0, :][reached]
    assert (dc == 0).sum() >= 10 and (dc != 0).sum() >= 10


@pytest.mark.parametrize("mode", MODES[1:])
@pytest.mark.parametrize("base", ("deg2", "deg3"))
def test_backward_layout_invariance_all_kernels(base, mode, gpu):
    """Check 4: k_preprocess_bwd_planes, _camera, _aa and _planes_camera_aa (check 3 runs the plain
    kernel; the other three combinations are compiled from the same text)."""
    for v in ("base", "tight", "off4"):
        _layout_identity(base, v, mode, gpu)


# ---- 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,variant,offset,mode", (
    ("deg3", "base", 1, "plain"), ("deg1", "tight", 1, "plain"), ("deg1", "tight", 0, "plain"),
    ("deg2", "tight", 0, "plain"), ("deg3", "wide", 0, "plain"), ("deg0", "tight", 1, "plain"),
    ("deg1", "tight", 1, "all"), ("deg2", "wide", 0, "all")))
def test_backward_output_rows_and_guard_words(base, variant, offset, mode, gpu):
    """gsr_backward (mode "all": gsr_backward_filtered with the planes, the camera and antialiasing,
    k_preprocess_bwd_planes_camera_aa) with a gsr_gradients filled here: dL_dsh `offset` floats
    past a 16-byte boundary inside a buffer of sentinel words.  The rows have the bits of the call
    through torch's aligned tensors (every tensor, every column); no word outside the P M 3 floats
    is written, and none inside keeps the sentinel."""
    sc = L.get(base, variant)
    s, g, M = sc["s"], sc["s"]["g"], sc["M"]
    n = L.P * M * 3
    buf = torch.full((GUARD + offset + n + GUARD,), SENTINEL, dtype=torch.int32, device=gpu)
    assert buf.data_ptr() % 16 == 0
    t = dict(means3D=to_dev(g.xyz, gpu), scales=to_dev(g.scale, gpu), rotations=to_dev(g.rot, gpu),
             opacities=to_dev(g.opacity, gpu), view=to_dev(s["view"], gpu), proj=to_dev(s["proj"], gpu),
             campos=to_dev(s["campos"], gpu), bg=to_dev(s["bg"], gpu))
    sh = _sh_dev(sc, gpu)
    assert sh.data_ptr() % 16 == 0
    f32 = dict(dtype=torch.float32, device=gpu)
    grads = {"dL_dmeans3D": torch.zeros((L.P, 3), **f32), "dL_dmeans2D": torch.zeros((L.P, 3), **f32),
             "dL_dopacity": torch.zeros((L.P, 1), **f32), "dL_dcolors": torch.zeros((L.P, 3), **f32),
             "dL_dconic": torch.zeros((L.P, 3), **f32), "dL_dscales": torch.zeros((L.P, 3), **f32),
             "dL_drotations": torch.zeros((L.P, 4), **f32), "dL_dcov3D": torch.zeros((L.P, 6), **f32)}
    gg = _lib.GsrGaussians(P=L.P, D=sc["D"], M=M, scale_modifier=s["scale_modifier"],
                           means3D=t["means3D"].data_ptr(), scales=t["scales"].data_ptr(),
                           rotations=t["rotations"].data_ptr(), opacities=t["opacities"].data_ptr(),
                           shs=sh.data_ptr())
    st = _lib.GsrRasterSettings(image_width=sc["W"], image_height=sc["H"], tanfovx=s["tx"],
                                tanfovy=s["ty"], viewmatrix=t["view"].data_ptr(),
                                projmatrix=t["proj"].data_ptr(), campos=t["campos"].data_ptr(),
                                bg=t["bg"].data_ptr())
    out = _lib.GsrGradients(**{k: v.data_ptr() for k, v in grads.items()},
                            dL_dsh=buf.data_ptr() + 4 * (GUARD + offset))
    assert out.dL_dsh % 16 == 4 * offset
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    lib, ctx = _lib.load_library(), _lib.context(gpu.index or 0)
    more = {}
    if mode == "all":
        more = {"dL_ddepths": torch.zeros((L.P,), **f32), "dL_dviewmatrix": torch.zeros((4, 4), **f32),
                "dL_dprojmatrix": torch.zeros((4, 4), **f32), "dL_dcampos": torch.zeros((3,), **f32)}
    seen = 0.0
    for part, mask in enumerate(L.dL_masks()):
        what = f"{sc['name']} at +{offset}, {mode}, part {part}"
        dL = to_dev(sc["dL"] * mask, gpu)
        inp = _lib.GsrBackwardInputs(dL_dcolor=dL.data_ptr())
        buf.fill_(SENTINEL)
        with torch.cuda.device(gpu):
            if mode == "all":
                d, i, tt = (to_dev(p * mask, gpu) for p in _plane_gradients())
                planes = _lib.GsrPlaneGradients(dL_ddepth_map=d.data_ptr(), dL_dinv_depth_map=i.data_ptr(),
                                                dL_dfinal_T=tt.data_ptr(),
                                                dL_ddepths=more["dL_ddepths"].data_ptr())
                cam = _lib.GsrCameraGradients(**{k: more[k].data_ptr() for k in CAMERA})
                _lib.check(_lib.filtered_fns(lib)[1](
                    ctx, ctypes.byref(gg), ctypes.byref(st), ctypes.byref(inp), ctypes.byref(planes),
                    ctypes.byref(cam), ctypes.byref(_lib.GsrFilterSettings(antialiasing=1)),
                    ctypes.byref(out), stream), "gsr_backward_filtered")
            else:
                _lib.check(_lib.backward_fn(lib)(ctx, ctypes.byref(gg), ctypes.byref(st),
                                                 ctypes.byref(inp), ctypes.byref(out), stream),
                           "gsr_backward")
        words = buf.cpu().numpy()
        lo, hi = words[:GUARD + offset], words[GUARD + offset + n:]
        assert len(hi) == GUARD and (lo == SENTINEL).all() and (hi == SENTINEL).all(), \
            (what, np.flatnonzero(lo != SENTINEL), np.flatnonzero(hi != SENTINEL))
        got = {k: v.cpu().numpy() for k, v in {**grads, **more}.items()}
        got["dL_dsh"] = words[GUARD + offset:GUARD + offset + n].view(np.float32).reshape(L.P, M, 3)
        assert np.isfinite(got["dL_dsh"]).all(), what
        assert (got["dL_dsh"][:, (sc["D"] + 1) ** 2:] == 0).all(), what
        assert (got["dL_dsh"][sc["special"]["culled"]] == 0).all(), what
        # the aligned call of this very scene, through torch's tensors: every column (M = 25 too)
        _same_bits(got, _backward(sc, gpu, mode, part=part), M, what)
        seen = seen + np.abs(got["dL_dsh"].astype(np.float64))
    assert seen[-1].max() > 0 and all(seen[:, L.band(l)].max() > 0 for l in range(sc["D"] + 1))


# ---- 6 ------------------------------------------------------------------------------------------
def _reference(base, gpu):
    """Autograd of composite(project(...)) in float64 on the GPU forward's lists and radii."""
    if base not in _ref:
        b = L.get(base)
        if base not in _fwd:
            _fwd[base] = run_hip(b["s"], gpu, extras=ALL_EXTRAS, binning=True)
        fwd = _fwd[base]
        ref = gr.scene_gradients(b, (fwd["ranges"], fwd["point_list"]), fwd["radii"], b["dL"])
        assert ref["near"] == (0, 0)
        _ref[base] = ref
    return _ref[base]


END_TO_END = (("dL_dmeans3D", "means3D"), ("dL_dmeans2D", "means2D"), ("dL_dopacity", "opacity"),
              ("dL_dscales", "scales"), ("dL_drotations", "rotations"), ("dL_dsh", "shs"))


@pytest.mark.parametrize("path", ("ctypes", "C"))
@pytest.mark.parametrize("variant", ("base", "tight"))
@pytest.mark.parametrize("base", L.BASES)
def test_against_float64_per_band(base, variant, path, gpu):
    sc = L.get(base, variant)
    s, g, M, D = sc["s"], sc["s"]["g"], sc["M"], sc["D"]
    ref = _reference(base, gpu)
    if path == "ctypes":
        got = {k: v.astype(np.float64) for k, v in _backward(sc, gpu, conic=False).items()}
    else:
        d = dict(means3D=to_dev(g.xyz, gpu), opacities=to_dev(g.opacity, gpu),
                 shs=_sh_dev(sc, gpu).detach(), scales=to_dev(g.scale, gpu),
                 rotations=to_dev(g.rot, gpu))
        for v in d.values():
            v.requires_grad_(True)
        means2D = torch.zeros_like(d["means3D"], requires_grad=True)
        rs = GaussianRasterizationSettings(
            sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
            to_dev(s["view"], gpu), to_dev(s["proj"], gpu), D, to_dev(s["campos"], gpu), False, False)
        color, radii = GaussianRasterizer(rs)(means2D=means2D, **d)
        np.testing.assert_array_equal(radii.cpu().numpy(), _fwd[base]["radii"])
        (color * to_dev(sc["dL"], gpu)).sum().backward()
        grad = lambda t: t.grad.cpu().numpy().astype(np.float64)  # noqa: E731
        got = dict(dL_dmeans3D=grad(d["means3D"]), dL_dmeans2D=grad(means2D),
                   dL_dopacity=grad(d["opacities"]), dL_dscales=grad(d["scales"]),
                   dL_drotations=grad(d["rotations"]), dL_dsh=grad(d["shs"]))
    what, bad = f"{sc['name']}/{path}", []
    assert got["dL_dsh"].shape == (L.P, M, 3) and (got["dL_dmeans2D"][:, 2] == 0).all()
    for name, key in END_TO_END:
        want = ref[key][:, :M] if key == "shs" else ref[key]
        e = gr.rel_err(got[name].reshape(want.shape), want)
        print(f"{what}: e[{key}] = {e:.3e}  (bound {gr.bound(key):.1e})")
        worst[("tensor", key)] = max(worst.get(("tensor", key), 0.0), e / gr.bound(key))
        if not e <= gr.bound(key):
            bad.append(f"{what}: e[{key}] = {e:.3e} > {gr.bound(key):.1e}")
    for l in range(D + 1):
        bnd = gr.BOUND_FACTOR * L.BAND_SPREAD[base][l]
        e = gr.rel_err(got["dL_dsh"][:, L.band(l)], ref["shs"][:, L.band(l)])
        print(f"{what}: band {l}: e = {e:.3e}  (f = {L.BAND_SPREAD[base][l]:.1e}, bound {bnd:.1e}, "
              f"max|ref| = {np.abs(ref['shs'][:, L.band(l)]).max():.3e})")
        worst[("band", l)] = max(worst.get(("band", l), 0.0), e / bnd)
        if not e <= bnd:
            bad.append(f"{what}: band {l}: e = {e:.3e} > {bnd:.1e}")
    assert not bad, bad
    assert (got["dL_dsh"][:, (D + 1) ** 2:] == 0).all()


# ---- 7 ------------------------------------------------------------------------------------------
def test_report_worst_ratio():
    """Not a check of its own: prints the largest e / bound check 6 saw per tensor and per SH band
    (README and DESIGN.md 3e quote it)."""
    for (kind, key), v in sorted(worst.items(), key=str):
        print(f"{kind:7s} {str(key):10s} {v:.3f}")
    if worst:
        print(f"worst e / bound: {max(worst.values()):.3f}")
