"""GPU: per-Gaussian feature channels in the forward (gsr_forward_features).

The oracle is the twin property: plane c of feature_map is, bit for bit, a colour channel of a
plain forward of the same scene with colors_precomp[:, j] = features[:, c] and bg = 0.  The twins
are rendered once per (scene, arithmetic mode, antialiasing) for the 35 columns of one feature
matrix, three at a time, on the default context; a call with C channels takes the matrix's first C
columns, so every C, option and output combination below is held to the same twin planes.

Scenes (grad_scenes): S1 `chain`, 40 x 24 -- a partial right column and bottom row, two tile rows
(strips); S2 `long_lists`, 32 x 16 -- lists of more than 128 entries: three chunks, odd counts,
termination and the 0.99 cap; S4 `edges` for the culled Gaussians.  Features are standard normal.
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_scenes
from gaussiansplattingviewer_amd import _lib
from gaussiansplattingviewer_amd.rasterizer import (GaussianRasterizationSettings,
                                                    GaussianRasterizer, binning_state,
                                                    rasterize_gaussians_native)
from gpu_helpers import set_option, to_dev, to_dev_unaligned
from test_gpu_backward import _inputs

pytestmark = pytest.mark.gpu

SCENES = ("chain", "long_lists")
CHANNELS = (1, 3, 5, 16, 17, 35)  # below a chunk, a chunk of 4, 4 + 1, 16, 16 + 1, 16 + 16 + 3
C_MAX = max(CHANNELS)
ALL_PIXEL_EXTRAS = ("final_T", "n_contrib", "depth_map", "inv_depth_map", "median_depth",
                    "median_id")
_slots = {}
_twins = {}
_feat = {}


def _slot(gpu, **options):
    """A context slot of this file's own with the given options (the others at their defaults)."""
    key = tuple(sorted(options.items()))
    if key not in _slots:
        _slots[key] = 70 + len(_slots)
        for name, value in options.items():
            set_option(gpu, getattr(_lib, f"GSR_OPT_{name}"), value, _slots[key])
    return _slots[key]


def _features(name, gpu):
    """The scene's [P, 35] standard-normal feature matrix (host, device)."""
    if name not in _feat:
        P = len(grad_scenes.get(name)["s"]["g"].xyz)
        f = np.random.default_rng(500 + grad_scenes.SEEDS[name]).standard_normal((P, C_MAX))
        f = np.ascontiguousarray(f, np.float32)
        assert (f < 0).any()
        _feat[name] = (f, to_dev(f, gpu))
    return _feat[name]


def _render(sc, gpu, features=None, colors=None, bg=None, **kw):
    """One native forward of a grad scene; colors: colors_precomp in the SH's place."""
    s, d = sc["s"], _inputs(sc, gpu)
    if colors is not None:
        d["shs"], d["colors_precomp"] = None, colors
    return rasterize_gaussians_native(
        to_dev(s["bg"] if bg is None else bg, gpu), d["means3D"], d["colors_precomp"],
        d["opacities"], d["scales"], d["rotations"], s["scale_modifier"], d["cov3D_precomp"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"], s["ty"], sc["H"], sc["W"],
        d["shs"], s["sh_degree"], to_dev(s["campos"], gpu), False, False, features=features, **kw)


def _twin(name, gpu, fast, aa=False):
    """[35, H, W]: channel c from the colors_precomp forward of columns 3 (c // 3) .. + 2, bg = 0,
    in the arithmetic mode `fast`."""
    key = (name, fast, aa)
    if key not in _twins:
        sc = grad_scenes.get(name)
        f = _features(name, gpu)[0]
        slot = _slot(gpu, BLEND_FAST=fast)
        planes = []
        for j in range(0, C_MAX, 3):
            cols = np.zeros((len(f), 3), np.float32)
            cols[:, :min(3, C_MAX - j)] = f[:, j:j + 3]
            res = _render(sc, gpu, colors=to_dev(cols, gpu), bg=np.zeros(3, np.float32), slot=slot,
                          antialiasing=aa)
            planes.append(res.color.cpu().numpy())
        _twins[key] = np.concatenate(planes)[:C_MAX]
    return _twins[key]


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype.itemsize == 4 else a.dtype)


def _assert_twin(res, twin, C, what):
    assert tuple(res.feature_map.shape) == (C,) + twin.shape[1:], what
    np.testing.assert_array_equal(_bits(res.feature_map), _bits(twin[:C]), err_msg=what)


@pytest.mark.parametrize("fast", (1, 0))
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("name", SCENES)
def test_twin_property(name, C, fast, gpu):
    """Every plane is the matching colour channel's bits, in both arithmetic modes; every other
    output is the same call's without features."""
    sc = grad_scenes.get(name)
    f = _features(name, gpu)[1][:, :C].contiguous()
    slot = _slot(gpu, BLEND_FAST=fast)
    res = _render(sc, gpu, features=f, slot=slot)
    _assert_twin(res, _twin(name, gpu, fast), C, f"{name} C={C} fast={fast}")
    lists = [_bits(t) for t in binning_state(gpu.index or 0, slot)]
    plain = _render(sc, gpu, slot=slot)
    assert plain.feature_map is None and res.num_rendered == plain.num_rendered
    np.testing.assert_array_equal(_bits(res.color), _bits(plain.color))
    np.testing.assert_array_equal(_bits(res.radii), _bits(plain.radii))
    for a, b in zip(lists, binning_state(gpu.index or 0, slot)):
        np.testing.assert_array_equal(a, _bits(b))
    assert np.abs(res.feature_map.cpu().numpy()).max() > 0.1


@pytest.mark.parametrize("name", SCENES)
def test_same_bits_under_every_option(name, gpu):
    """Tight binning on and off, the blend cull on and off, frame graphs 1 and 2: the twin's bits
    (C = 17: a chunk of 16 and a padded chunk of 4)."""
    sc = grad_scenes.get(name)
    C = 17
    f = _features(name, gpu)[1][:, :C].contiguous()
    twin = _twin(name, gpu, 1)
    for options in (dict(TIGHT_BINNING=0), dict(TIGHT_BINNING=1), dict(BLEND_CULL=0),
                    dict(BLEND_CULL=1), dict(BLEND_CULL=0, BLEND_FAST=0)):
        res = _render(sc, gpu, features=f, slot=_slot(gpu, **options))
        mode = options.get("BLEND_FAST", 1)
        _assert_twin(res, _twin(name, gpu, mode), C, f"{name} {options}")
    for mode in (1, 2):
        slot = _slot(gpu, FRAME_GRAPHS=mode)
        for i in range(3):  # the first frame sizes the capacity; the next ones take the chains
            res = _render(sc, gpu, features=f, slot=slot)
            _assert_twin(res, twin, C, f"{name} frame graphs {mode}, frame {i}")
        assert _lib.frame_graph_stats(gpu.index or 0, slot)["graph_frames"] >= 1


@pytest.mark.parametrize("fast", (1, 0))
@pytest.mark.parametrize("name", SCENES)
def test_with_every_other_output(name, fast, gpu):
    """With and without n_contrib, the depth planes and the median planes: the feature planes keep
    the twin's bits, and each of those outputs its bits from the call without features."""
    sc = grad_scenes.get(name)
    C = 5
    f = _features(name, gpu)[1][:, :C].contiguous()
    slot = _slot(gpu, BLEND_FAST=fast)
    twin = _twin(name, gpu, fast)
    for extras in (("n_contrib",), ("final_T",), ("depth_map", "inv_depth_map"),
                   ("median_depth", "median_id"), ALL_PIXEL_EXTRAS,
                   ("depths", "means2D", "conic_opacity", "rgb", "tiles_touched")):
        res = _render(sc, gpu, features=f, slot=slot, extras=extras)
        _assert_twin(res, twin, C, f"{name} fast={fast} {extras}")
        plain = _render(sc, gpu, slot=slot, extras=extras)
        assert res.num_rendered == plain.num_rendered
        np.testing.assert_array_equal(_bits(res.color), _bits(plain.color))
        for n in extras:
            np.testing.assert_array_equal(_bits(res.extras[n]), _bits(plain.extras[n]), err_msg=n)


@pytest.mark.parametrize("name", SCENES)
def test_antialiasing_against_an_antialiased_twin(name, gpu):
    sc = grad_scenes.get(name)
    C = 17
    f = _features(name, gpu)[1][:, :C].contiguous()
    for fast in (1, 0):
        res = _render(sc, gpu, features=f, slot=_slot(gpu, BLEND_FAST=fast), antialiasing=True)
        twin = _twin(name, gpu, fast, aa=True)
        _assert_twin(res, twin, C, f"{name} antialiased fast={fast}")
        assert not np.array_equal(_bits(twin), _bits(_twin(name, gpu, fast)))


@pytest.mark.parametrize("C", (4, 16, 17))
@pytest.mark.parametrize("name", SCENES)
def test_unaligned_feature_rows(name, C, gpu):
    """Rows that start one float into a buffer (4-byte aligned only) take the scalar gather: the
    same bits.  C = 4 and 16 would take the vector gather at an aligned pointer."""
    sc = grad_scenes.get(name)
    f = to_dev_unaligned(_features(name, gpu)[0][:, :C], gpu)
    assert f.data_ptr() % 16 == 4
    res = _render(sc, gpu, features=f)
    _assert_twin(res, _twin(name, gpu, 1), C, f"{name} unaligned C={C}")


@pytest.mark.parametrize("fast", (1, 0))
def test_strips_stack_to_the_frame(fast, gpu):
    """S1's two tile rows rendered as strips (0, 1) and (1, 2): stacked, the frame's bits."""
    sc = grad_scenes.get("chain")
    C = 17
    f = _features("chain", gpu)[1][:, :C].contiguous()
    slot = _slot(gpu, BLEND_FAST=fast)
    parts = [_render(sc, gpu, features=f, slot=slot, tile_rows=rows) for rows in ((0, 1), (1, 2))]
    assert [tuple(p.feature_map.shape) for p in parts] == [(C, 16, 40), (C, 8, 40)]
    stacked = torch.cat([p.feature_map for p in parts], 1)
    np.testing.assert_array_equal(_bits(stacked), _bits(_twin("chain", gpu, fast)[:C]))
    # radii=False (a strip rank that needs its image only) leaves the planes as they are
    lean = _render(sc, gpu, features=f, slot=slot, tile_rows=(1, 2), radii=False)
    np.testing.assert_array_equal(_bits(lean.feature_map), _bits(parts[1].feature_map))


def test_nan_rows_of_culled_gaussians_reach_nothing(gpu):
    """S4: NaN feature rows for the Gaussians with radii == 0 leave every output finite and
    bit-identical to the call with zeros there."""
    sc = grad_scenes.get("edges")
    P = len(sc["s"]["g"].xyz)
    f = np.ascontiguousarray(np.random.default_rng(9).standard_normal((P, 5)), np.float32)
    radii = _render(sc, gpu).radii.cpu().numpy()
    culled = radii == 0
    assert culled.sum() >= 5
    zeros, nans = f.copy(), f.copy()
    zeros[culled], nans[culled] = 0.0, np.nan
    for fast in (1, 0):
        slot = _slot(gpu, BLEND_FAST=fast)
        a = _render(sc, gpu, features=to_dev(zeros, gpu), slot=slot, extras=ALL_PIXEL_EXTRAS)
        b = _render(sc, gpu, features=to_dev(nans, gpu), slot=slot, extras=ALL_PIXEL_EXTRAS)
        assert torch.isfinite(b.feature_map).all() and torch.isfinite(b.color).all()
        np.testing.assert_array_equal(_bits(a.feature_map), _bits(b.feature_map))
        np.testing.assert_array_equal(_bits(a.color), _bits(b.color))
        for n in ALL_PIXEL_EXTRAS:
            np.testing.assert_array_equal(_bits(a.extras[n]), _bits(b.extras[n]), err_msg=n)


def test_empty_scenes_give_zero_planes(gpu):
    """P = 0, and a frame whose lists are empty (every Gaussian behind the camera)."""
    sc = grad_scenes.get("chain")
    s = sc["s"]
    e = torch.zeros((0, 3), device=gpu)
    res = rasterize_gaussians_native(
        to_dev(s["bg"], gpu), e, None, torch.zeros((0, 1), device=gpu), e,
        torch.zeros((0, 4), device=gpu), 1.0, None, to_dev(s["view"], gpu), to_dev(s["proj"], gpu),
        s["tx"], s["ty"], sc["H"], sc["W"], torch.zeros((0, 16, 3), device=gpu), 3,
        to_dev(s["campos"], gpu), False, False, features=torch.zeros((0, 5), device=gpu))
    assert tuple(res.feature_map.shape) == (5, 24, 40) and not res.feature_map.any()
    d = _inputs(sc, gpu)
    behind = d["means3D"].clone()
    behind[:, 2] = 9.0  # the eye is at z = 4, looking down -z
    f = _features("chain", gpu)[1][:, :17].contiguous()
    res = rasterize_gaussians_native(
        to_dev(s["bg"], gpu), behind, None, d["opacities"], d["scales"], d["rotations"],
        s["scale_modifier"], None, to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"], s["ty"],
        sc["H"], sc["W"], d["shs"], s["sh_degree"], to_dev(s["campos"], gpu), False, False,
        features=f)
    assert res.num_rendered == 0 and not res.radii.any()
    assert tuple(res.feature_map.shape) == (17, 24, 40)
    assert not _bits(res.feature_map).any()


def test_refusals_leave_the_output_untouched(gpu):
    """C < 1, C > GSR_MAX_FEATURES and a NULL features with a map given: GSR_E_INVALID by ctypes, a
    poisoned map untouched; Python: RuntimeError, also for a shading."""
    sc = grad_scenes.get("chain")
    s, d = sc["s"], _inputs(sc, gpu)
    f = _features("chain", gpu)[1][:, :4].contiguous()
    lib = _lib.load_library()
    ctx = _lib.context(gpu.index or 0, 0)
    from gaussiansplattingviewer_amd.rasterizer import _scene_structs
    _, _, P, g, st, held = _scene_structs(
        to_dev(s["bg"], gpu), d["means3D"], None, d["opacities"], d["scales"], d["rotations"],
        s["scale_modifier"], None, to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["tx"], s["ty"],
        sc["H"], sc["W"], d["shs"], s["sh_degree"], to_dev(s["campos"], gpu), False, False)
    color = torch.full((3, sc["H"], sc["W"]), 7.0, device=gpu)
    radii = torch.full((P,), -5, dtype=torch.int32, device=gpu)
    fmap = torch.full((4, sc["H"], sc["W"]), 7.0, device=gpu)
    out = _lib.GsrOutputs(color=color.data_ptr(), radii=radii.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    fn = _lib.features_fns(lib)[0]
    for C, ptr in ((0, f.data_ptr()), (-3, f.data_ptr()), (_lib.MAX_FEATURES + 1, f.data_ptr()),
                   (4, None)):
        feat = _lib.GsrFeatureOutputs(C=C, features=ptr, feature_map=fmap.data_ptr())
        rc = fn(ctx, ctypes.byref(g), ctypes.byref(st), ctypes.byref(out), None, None, None,
                ctypes.byref(feat), stream)
        assert rc == -1 and b"gsr_forward_features" in lib.gsr_last_error()
        torch.cuda.synchronize(gpu)
        assert (fmap == 7.0).all() and (color == 7.0).all() and (radii == -5).all()
    # the same call with good arguments writes all three
    feat = _lib.GsrFeatureOutputs(C=4, features=f.data_ptr(), feature_map=fmap.data_ptr())
    assert fn(ctx, ctypes.byref(g), ctypes.byref(st), ctypes.byref(out), None, None, None,
              ctypes.byref(feat), stream) == 0
    np.testing.assert_array_equal(_bits(fmap), _bits(_twin("chain", gpu, 1)[:4]))
    assert not (color == 7.0).any() and (radii >= 0).all()
    # Python
    for bad in (torch.zeros((P, 0), device=gpu), torch.zeros((P, 257), device=gpu),
                torch.zeros((P + 1, 4), device=gpu), torch.zeros((P,), device=gpu)):
        with pytest.raises(RuntimeError, match="features"):
            _render(sc, gpu, features=bad)
    for shading in (1, 2, 3):
        with pytest.raises(RuntimeError, match="shading"):
            _render(sc, gpu, features=f, shading=shading)
    rs = GaussianRasterizationSettings(
        sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
        to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"], to_dev(s["campos"], gpu),
        False, False, 2)
    with pytest.raises(RuntimeError, match="shading"):
        GaussianRasterizer(rs)(means2D=None, features=f, **d)


@pytest.mark.parametrize("name", SCENES)
def test_rasterizer_module_returns_the_same_planes(name, gpu):
    """GaussianRasterizer(..., features=f): the usual outputs followed by feature_map, through the
    `_C` extension, with the native call's bits; with depth_maps the 5 + 1; without features
    today's tuple."""
    sc = grad_scenes.get(name)
    s, d = sc["s"], _inputs(sc, gpu)
    C = 17
    f = _features(name, gpu)[1][:, :C].contiguous()
    upstream = (sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
                to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"],
                to_dev(s["campos"], gpu), False, False)
    twin = _twin(name, gpu, 1)
    with torch.no_grad():
        plain = GaussianRasterizer(GaussianRasterizationSettings(*upstream))(means2D=None, **d)
        out = GaussianRasterizer(GaussianRasterizationSettings(*upstream))(
            means2D=None, features=f, **d)
        deep = GaussianRasterizer(GaussianRasterizationSettings(*upstream, depth_maps=True))(
            means2D=None, features=f, **d)
        deep0 = GaussianRasterizer(GaussianRasterizationSettings(*upstream, depth_maps=True))(
            means2D=None, **d)
    assert len(plain) == 2 and len(out) == 3 and len(deep) == 6 and len(deep0) == 5
    np.testing.assert_array_equal(_bits(out[2]), _bits(twin[:C]))
    np.testing.assert_array_equal(_bits(deep[5]), _bits(twin[:C]))
    for a, b in zip(out[:2] + deep[:5], plain + deep0):
        np.testing.assert_array_equal(_bits(a), _bits(b))
