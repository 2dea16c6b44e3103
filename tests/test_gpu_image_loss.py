"""GPU: the fused L1 + D-SSIM loss (gsr_image_loss / gsr_image_loss_backward, csrc/loss.hip;
gaussiansplattingviewer_amd.losses) against the float64 restatement of tests/loss_reference.py.

   1 values and dL_dimage within 8 x f (the reference's own float32 spread, F32_SPREAD) on every
     image of loss_images() -- 1x1x1, smaller than the window, random, smooth, dark, near the
     target, and the tile's edges (15..17 x 63..65) -- for lambda 0, 0.2, 1, dL_dloss NULL and given
   2 lambda = 0 is exactly the L1 gradient: +-(1/N), and 0 where image == target
   3 ssim alone and the three saved planes against the float64 partials
   4 the same bits on every call, on a second stream, and dL_dloss = 2 exactly doubles
   5 identical images: l1 == 0.0, ssim within its bound of 1
   6 no stray writes around 4-byte-aligned outputs; saved = NULL writes only values
   7 ctypes and `_C` give the same bits; no_grad keeps nothing for a backward
   8 end to end: the rasterizer's gradients through photometric_loss(color, target).backward()
     are bit for bit those of color.backward(gradient = the loss's own dL_dimage)
   9 the Python refusals; NaN propagates
"""
import ctypes

import numpy as np
import pytest
import torch

import grad_scenes
import loss_reference as L
from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer, _C,
                                         _lib, losses, photometric_loss, ssim)
from gpu_helpers import to_dev, to_dev_unaligned
from grad_reference import rel_err
from test_gpu_backward import _inputs

pytestmark = pytest.mark.gpu

IMAGES = L.loss_images()
F, K = L.F32_SPREAD, L.BOUND_FACTOR


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a,
                                np.float32).view(np.uint32)


def _run(name, lam, gpu, gl=None, saved=True, pair=None):
    """Forward and backward by ctypes -> (values [3], saved, dL_dimage) as numpy."""
    x, y = (to_dev(a, gpu) for a in (pair or IMAGES[name]))
    values, planes = losses.image_loss_native(x, y, lam, saved)
    grad = None
    if saved:
        g = None if gl is None else torch.tensor([gl], dtype=torch.float32, device=gpu)
        grad = losses.image_loss_backward_native(x, y, lam, planes, g).cpu().numpy()
        planes = planes.cpu().numpy()
    return values.cpu().numpy(), planes, grad


def _within(what, got, ref, f):
    e = rel_err(got, ref)
    print(f"{what}: rel_err {e:.3g}, bound {K:g} x {f:.3g}")
    assert e <= K * f, (what, e, K * f)


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_values_and_gradient(name, gpu):
    for lam in L.LAMBDAS:
        ref = L.reference(name, lam)
        values, _, grad = _run(name, lam, gpu)
        _within(f"{name} lambda {lam} loss", values[0], ref["loss"], F["loss"][lam])
        _within(f"{name} lambda {lam} l1", values[1], ref["l1"], F["l1"])
        _within(f"{name} lambda {lam} ssim", values[2], ref["ssim"], F["ssim"])
        _within(f"{name} lambda {lam} dL_dimage", grad, ref["dL_dimage"], F["dL_dimage"][lam])
        _, _, scaled = _run(name, lam, gpu, gl=-2.5)
        _within(f"{name} lambda {lam} dL_dimage, dL_dloss -2.5", scaled, -2.5 * ref["dL_dimage"],
                F["dL_dimage"][lam])


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "tile_17x65"])
def test_lambda_zero_is_the_l1_gradient(name, gpu):
    image, target = IMAGES[name]
    _, _, grad = _run(name, 0.0, gpu)
    step = np.float32(1.0) / np.float32(image.size)
    want = (np.sign(image - target) * step).astype(np.float32)
    assert (grad == want).all()
    ties = image == target
    assert ties.sum() == (4 if name == "random" else 0) and (grad[ties] == 0.0).all()
    assert set(np.unique(np.abs(grad[~ties]))) == {step}


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(IMAGES))
def test_map_and_saved_planes(name, gpu):
    ref = L.reference(name, 0.2)
    x, y = (to_dev(a, gpu) for a in IMAGES[name])
    _within(f"{name} ssim()", float(ssim(x, y)), ref["ssim"], F["ssim"])
    _, planes, _ = _run(name, 0.2, gpu)
    assert planes.shape == (3, *x.shape)
    for i, k in enumerate(L.SAVED_NAMES):
        _within(f"{name} {k}", planes[i], ref["saved"][i], F[k])


# ---- 4 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["smooth", "tile_17x65"])
def test_reproducible_bits(name, gpu):
    first = _run(name, 0.2, gpu, gl=1.0)
    again = _run(name, 0.2, gpu, gl=1.0)
    side = torch.cuda.Stream(gpu)
    with torch.cuda.stream(side):
        other = _run(name, 0.2, gpu, gl=1.0)
    null = _run(name, 0.2, gpu)  # dL_dloss NULL is 1.0
    for run in (again, other, null):
        for a, b in zip(run, first):
            np.testing.assert_array_equal(_bits(a), _bits(b))
    twice = _run(name, 0.2, gpu, gl=2.0)[2]
    np.testing.assert_array_equal(_bits(twice), _bits(2.0 * first[2]))


# ---- 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "dark", "small"])
def test_identical_images(name, gpu):
    image = IMAGES[name][0]
    values, _, grad = _run(name, 0.2, gpu, pair=(image, image.copy()))
    assert values[1] == 0.0
    _within(f"{name} identical ssim", values[2], 1.0, F["ssim"])
    assert np.isfinite(grad).all()


# ---- 6 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["small", "tile_17x65", "random"])
def test_no_stray_writes(name, gpu):
    image, target = IMAGES[name]
    N = image.size
    x, y = to_dev_unaligned(image, gpu), to_dev_unaligned(target, gpu)
    assert x.data_ptr() % 8 == 4
    lib = _lib.load_library()
    workspace, forward, backward = _lib.image_loss_fns(lib)
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=gpu)  # noqa: E731
    pad = 64
    vbuf, sbuf, gbuf, v2 = nan(1 + 3 + pad), nan(1 + 3 * N + pad), nan(1 + N + pad), nan(4 + pad)
    ws = torch.empty(workspace(*image.shape), dtype=torch.uint8, device=gpu)
    inp = _lib.GsrImageLossInputs(*image.shape, 0.2, x.data_ptr(), y.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    at = lambda t: t.data_ptr() + 4  # noqa: E731
    assert forward(ctypes.byref(inp), at(vbuf), at(sbuf), ws.data_ptr(), stream) == 0
    assert backward(ctypes.byref(inp), at(sbuf), None, at(gbuf), stream) == 0
    assert forward(ctypes.byref(inp), at(v2), None, ws.data_ptr(), stream) == 0
    torch.cuda.synchronize(gpu)
    for buf, n in ((vbuf, 3), (sbuf, 3 * N), (gbuf, N), (v2, 3)):
        host = buf.cpu().numpy()
        assert np.isnan(host[0]) and np.isnan(host[1 + n:]).all()
        assert np.isfinite(host[1:1 + n]).all()
    want = _run(name, 0.2, gpu)
    np.testing.assert_array_equal(_bits(vbuf[1:4]), _bits(want[0]))
    np.testing.assert_array_equal(_bits(v2[1:4]), _bits(want[0]))
    np.testing.assert_array_equal(_bits(sbuf[1:1 + 3 * N]), _bits(want[1]).reshape(-1))
    np.testing.assert_array_equal(_bits(gbuf[1:1 + N]), _bits(want[2]).reshape(-1))


# ---- 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["one", "smooth", "tile_17x65"])
def test_routes_give_the_same_bits(name, gpu, monkeypatch):
    x, y = (to_dev(a, gpu) for a in IMAGES[name])
    values, planes, grad = _run(name, 0.2, gpu, gl=0.75)
    v, s = _C.fused_image_loss(x, y, 0.2, True)
    g = _C.fused_image_loss_backward(x, y, 0.2, s, torch.tensor([0.75], device=gpu))
    for a, b in ((v, values), (s, planes), (g, grad)):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    v0, s0 = _C.fused_image_loss(x, y, 0.2, False)
    assert s0.numel() == 0 and torch.equal(v0, v)
    # the public entry: the same bits again, and what it keeps for a backward
    kept = []
    inner = losses._forward

    def spy(image, target, lam, need_saved):
        out = inner(image, target, lam, need_saved)
        kept.append((need_saved, out[1]))
        return out
    monkeypatch.setattr(losses, "_forward", spy)
    xg = x.clone().requires_grad_(True)
    loss, l1, ss = photometric_loss(xg, y, return_parts=True)
    assert loss.dim() == 0 and loss.device == x.device and loss.requires_grad
    assert not l1.requires_grad and not ss.requires_grad
    (0.75 * loss).backward()
    np.testing.assert_array_equal(_bits(torch.stack([loss, l1, ss])), _bits(values))
    np.testing.assert_array_equal(_bits(xg.grad), _bits(grad))
    assert kept[-1][0] is True and tuple(kept[-1][1].shape) == (3, *x.shape)
    with torch.no_grad():
        quiet = photometric_loss(xg, y)
    assert kept[-1] == (False, None) and not quiet.requires_grad
    plain = photometric_loss(x, y)  # no gradient asked for
    assert kept[-1] == (False, None) and not plain.requires_grad
    np.testing.assert_array_equal(_bits(quiet), _bits(values[0]))
    np.testing.assert_array_equal(_bits(plain), _bits(values[0]))
    # inputs are made contiguous float32
    wide = torch.zeros((*x.shape[:2], 2 * x.shape[2]), dtype=torch.float64, device=gpu)
    wide[:, :, ::2] = x.double()
    np.testing.assert_array_equal(_bits(photometric_loss(wide[:, :, ::2], y)), _bits(values[0]))


# ---- 8 ------------------------------------------------------------------------------------------
def test_end_to_end_through_the_rasterizer(gpu):
    sc = grad_scenes.get("chain")
    s = sc["s"]
    target = to_dev(np.random.default_rng(5).uniform(0, 1, (3, sc["H"], sc["W"])).astype(np.float32),
                    gpu)

    def render():
        d = _inputs(sc, gpu)
        for k in ("means3D", "opacities", "shs"):
            d[k].requires_grad_(True)
        rs = GaussianRasterizationSettings(
            sc["H"], sc["W"], s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
            to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"],
            to_dev(s["campos"], gpu), False, False, deterministic=True)
        color, _ = GaussianRasterizer(rs)(means2D=None, **d)
        return d, color

    d1, color1 = render()
    loss = photometric_loss(color1, target)
    loss.backward()
    d2, color2 = render()
    assert torch.equal(color1, color2)
    c = color2.detach().clone().requires_grad_(True)
    photometric_loss(c, target).backward()
    color2.backward(gradient=c.grad)
    for k in ("means3D", "opacities", "shs"):
        assert d1[k].grad is not None and float(d1[k].grad.abs().max()) > 0.0, k
        np.testing.assert_array_equal(_bits(d1[k].grad), _bits(d2[k].grad), err_msg=k)


# ---- 9 ------------------------------------------------------------------------------------------
def test_python_refusals(gpu):
    x = torch.rand(3, 8, 9, device=gpu)
    with pytest.raises(ValueError, match="one shape"):
        photometric_loss(x, torch.rand(3, 9, 8, device=gpu))
    with pytest.raises(ValueError, match="one shape"):
        photometric_loss(x[0], x[0])
    with pytest.raises(ValueError, match="target on cpu"):
        photometric_loss(x, x.cpu())
    with pytest.raises(ValueError, match="HIP device"):
        photometric_loss(x.cpu(), x.cpu())
    with pytest.raises(ValueError, match="must not require a gradient"):
        photometric_loss(x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="HIP device"):
        ssim(x.cpu(), x.cpu())


def test_nan_propagates(gpu):
    image, target = (a.copy() for a in IMAGES["random"])
    image[1, 20, 20] = np.nan
    values, _, grad = _run("random", 0.2, gpu, pair=(image, target))
    assert np.isnan(values).all()
    assert np.isnan(grad[1, 20, 20]) and np.isnan(grad[1, 15:26, 15:26]).all()
    assert np.isfinite(grad[0]).all() and np.isfinite(grad[1, :9, :9]).all()
