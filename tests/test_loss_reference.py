"""CPU: the torch restatement of the fused image loss (tests/loss_reference.py) is right -- its
manual backward against float64 autograd, the separable form against the 2-D window -- the
committed float32 spread is what a fresh measurement finds, and the loaded library refuses bad
arguments before any HIP call (include/gsr.h).  At the end, the helpers of the seam tests
(test_gpu_image_loss_seams.py): their cases, their measured spread, and the locality of the
float64 restatement that the translation test rests on."""
import ctypes

import numpy as np
import pytest
import torch

import loss_reference as L
from gaussiansplattingviewer_amd import _lib
from grad_reference import rel_err

IMAGES = L.loss_images()


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_manual_gradient_is_float64_autograd(name):
    """Within 1e-12 relative.  `near` at lambda = 1 is left out: there the gradient is the small
    remainder of cancelling terms and float64 autograd itself moves by 1.6e-12 between the 2-D
    and the separable evaluation of the same definition (the formula's distance to it was
    1.4e-12), so the reference's own noise is above the bound; `near` is held at 0 and 0.2."""
    image, target = IMAGES[name]
    x, y = (torch.tensor(a, dtype=torch.float64) for a in (image, target))
    for lam in L.LAMBDAS[:2] if name == "near" else L.LAMBDAS:
        ref = L.reference(name, lam)["dL_dimage"]
        assert rel_err(L.manual_gradient(x, y, lam).numpy(), ref) <= 1e-12
        assert rel_err(L.manual_gradient(x, y, lam, gl=-2.5).numpy(), -2.5 * ref) <= 1e-12


@pytest.mark.parametrize("name", sorted(IMAGES))
def test_separable_form_is_the_2d_window(name):
    image, target = IMAGES[name]
    x, y = (torch.tensor(a, dtype=torch.float64) for a in (image, target))
    for p in (x, y, x * x, x * y):
        assert float((L.conv_separable(p) - L.conv(p)).abs().max()) <= 1e-13
    a = torch.stack(L.loss_values(x, y, 0.2, L.conv_separable))
    b = torch.stack(L.loss_values(x, y, 0.2))
    assert float((a - b).abs().max()) <= 1e-13


def test_window_and_definition():
    g = L.window_1d()
    assert g.shape == (11,) and abs(float(g.sum()) - 1.0) < 1e-15 and torch.equal(g, g.flip(0))
    assert float(g[5]) == pytest.approx(0.2660117, abs=1e-7)
    # zero padding: a constant image's mean falls off at the border, its centre does not
    c = L.conv(torch.ones(1, 21, 21, dtype=torch.float64))[0]
    assert float(c[10, 10]) == pytest.approx(1.0, abs=1e-14) and float(c[0, 0]) < 0.5
    # identical images: map == 1, l1 == 0
    x = torch.tensor(IMAGES["random"][0], dtype=torch.float64)
    loss, l1, ssim = L.loss_values(x, x, 0.2)
    assert float(l1) == 0.0 and abs(float(ssim) - 1.0) < 1e-14 and abs(float(loss)) < 1e-14


def test_images_are_the_issue_s_cases():
    shapes = {k: v[0].shape for k, v in IMAGES.items()}
    assert shapes["one"] == (1, 1, 1) and shapes["small"] == (1, 7, 9)
    assert shapes["random"] == shapes["smooth"] == (3, 37, 53)
    assert shapes["dark"] == (4, 16, 200) and shapes["near"] == (3, 64, 80)
    assert {shapes[f"tile_{h}x{w}"][1:] for h in (15, 16, 17) for w in (63, 64, 65)} == \
        {(h, w) for h in (15, 16, 17) for w in (63, 64, 65)}
    assert all(int(np.prod(s)) <= 4 * 67 * 200 for s in shapes.values())
    for image, target in IMAGES.values():
        assert image.dtype == target.dtype == np.float32
    assert max(float(a.max()) for a in IMAGES["dark"]) < 0.02
    assert float(np.abs(IMAGES["near"][0] - IMAGES["near"][1]).max()) <= 1.001e-3
    assert int((IMAGES["random"][0] == IMAGES["random"][1]).sum()) == 4  # the ties of sign(0)


def test_committed_spread_is_the_measured_one():
    """F32_SPREAD is measured, not chosen: within a factor 2 of a fresh measurement."""
    got = L.measure_spread(IMAGES)
    print("measured float32 spread:", got)

    def pairs(a, b):
        for k in a:
            if isinstance(a[k], dict):
                yield from ((f"{k}[{lam}]", a[k][lam], b[k][lam]) for lam in a[k])
            else:
                yield k, a[k], b[k]
    assert set(got) == set(L.F32_SPREAD)
    for name, have, want in pairs(L.F32_SPREAD, got):
        assert want / 2.0 <= have <= want * 2.0, (name, have, want)


# ---- the library's refusals: checked before the first HIP call, so no device is needed ---------

FAKE = 0x1000  # a non-NULL pointer nothing dereferences: every call below is refused first


def _inputs(C=3, H=8, W=8, lam=0.2, image=FAKE, target=FAKE):
    return _lib.GsrImageLossInputs(C, H, W, lam, image, target)


def test_struct_layout_matches_header(tmp_path):
    import os
    import subprocess
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = [f for f, _ in _lib.GsrImageLossInputs._fields_]
    c_names = ["lambda" if f == "lambda_" else f for f in names]
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "gsr.h"', "int main(void){",
             'printf("%zu\\n", sizeof(gsr_image_loss_inputs));']
    lines += [f'printf("%zu\\n", offsetof(gsr_image_loss_inputs, {f}));' for f in c_names]
    (tmp_path / "probe.c").write_text("\n".join(lines + ["return 0;}"]))
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(repo, "include"),
                    str(tmp_path / "probe.c"), "-o", str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], capture_output=True, text=True, check=True)
    got = [int(v) for v in out.stdout.split()]
    assert got[0] == ctypes.sizeof(_lib.GsrImageLossInputs)
    assert got[1:] == [getattr(_lib.GsrImageLossInputs, f).offset for f in names]


def test_workspace_query():
    workspace, _, _ = _lib.image_loss_fns(_lib.load_library())
    assert workspace(1, 1, 1) == 8  # one block's (l1, map) pair
    th, tw = L.TILE_H, L.TILE_W
    assert workspace(3, th, tw) == 3 * 8 and workspace(3, th + 1, tw + 1) == 3 * 4 * 8
    assert workspace(3, 1080, 1920) == 3 * 68 * 30 * 8
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (-1, 4, 4), (1, 1 << 16, 1 << 15),
                (2, 1 << 15, 1 << 15), (3, 46341, 46341)):
        assert workspace(*bad) == -1, bad  # GSR_E_INVALID
    assert workspace(1, 1 << 15, (1 << 16) - 1) > 0  # C*H*W = 2^31 - 2^15


@pytest.mark.parametrize("case", ["in", "image", "target", "values", "workspace", "C", "H", "W",
                                  "too_large", "lambda_low", "lambda_high", "lambda_nan"])
def test_forward_refusals(case):
    _, forward, _ = _lib.image_loss_fns(_lib.load_library())
    args = dict(values=FAKE, saved=FAKE, workspace=FAKE)
    kw = {}
    if case in ("image", "target"):
        kw[case] = None
    elif case in ("values", "workspace"):
        args[case] = None
    elif case in ("C", "H", "W"):
        kw[case] = 0
    elif case == "too_large":
        kw.update(C=2, H=1 << 15, W=1 << 15)
    elif case.startswith("lambda"):
        kw["lam"] = {"lambda_low": -1e-6, "lambda_high": 1.0 + 1e-6,
                     "lambda_nan": float("nan")}[case]
    inp = None if case == "in" else ctypes.byref(_inputs(**kw))
    assert forward(inp, args["values"], args["saved"], args["workspace"], None) == -1
    assert b"gsr_image_loss" in _lib.load_library().gsr_last_error()


@pytest.mark.parametrize("case", ["in", "image", "target", "saved", "dL_dimage", "H",
                                  "too_large", "lambda_nan"])
def test_backward_refusals(case):
    backward = _lib.image_loss_fns(_lib.load_library())[2]
    args = dict(saved=FAKE, dL_dimage=FAKE)
    kw = {}
    if case in ("image", "target"):
        kw[case] = None
    elif case in ("saved", "dL_dimage"):
        args[case] = None
    elif case == "H":
        kw["H"] = -3
    elif case == "too_large":
        kw.update(C=1, H=1 << 16, W=1 << 15)
    elif case == "lambda_nan":
        kw["lam"] = float("nan")
    inp = None if case == "in" else ctypes.byref(_inputs(**kw))
    assert backward(inp, args["saved"], None, args["dL_dimage"], None) == -1
    assert b"gsr_image_loss_backward" in _lib.load_library().gsr_last_error()


def test_python_refusals_need_no_device():
    from gaussiansplattingviewer_amd import photometric_loss, ssim
    x = torch.zeros(3, 8, 8)
    with pytest.raises(ValueError, match="HIP device"):
        photometric_loss(x, x.clone())
    with pytest.raises(ValueError, match="one shape"):
        photometric_loss(x, torch.zeros(3, 8, 9))
    with pytest.raises(ValueError, match="one shape"):
        ssim(torch.zeros(8, 8), torch.zeros(8, 8))
    with pytest.raises(ValueError, match="must not require a gradient"):
        photometric_loss(x, x.clone().requires_grad_(True))
    with pytest.raises(ValueError, match="lambda_dssim"):
        photometric_loss(x, x.clone(), lambda_dssim=1.5)


# ---- the helpers of the seam tests (test_gpu_image_loss_seams.py) -------------------------------

def test_seam_cases_are_the_issue_s():
    images = L.seam_images()
    assert [v[0].shape for v in images.values()] == [
        (3, 33, 129), (2, 48, 192), (5, 100, 1000), (1, 1, 130), (1, 70, 1), (2, 5, 5),
        (1, 11, 11), (1, 12, 12)]
    assert list(images) == [L.shape_name(s) for s in L.SEAM_SHAPES]
    for image, target in images.values():
        assert image.dtype == target.dtype == np.float32 and image.shape == target.shape
        assert 0.0 <= min(image.min(), target.min()) and max(image.max(), target.max()) <= 1.0
        assert not (image == target).all()
    # a tile with neighbours on all four sides: 3 x 3 tiles at least, with C > 1
    th, tw = L.TILE_H, L.TILE_W
    assert (33 - 1) // th == 2 and (129 - 1) // tw == 2 and L.blocks_of((3, 33, 129)) == 27
    assert L.blocks_of(L.LOCALITY_SHAPE) == 2 * 3 * 3 and L.LOCALITY_SHAPE in L.SEAM_SHAPES
    assert L.LOCALITY_PIXELS == ((0, 0), (47, 191), (15, 63), (16, 64), (16, 63), (24, 96))
    # the translation pair: 4 x 4 tiles, crops of a quarter of its elements that fit
    assert L.TRANSLATION_SHAPE == (2, 64, 256) and (L.CROP_H, L.CROP_W) == (32, 128)
    assert L.TRANSLATION_OFFSETS == ((0, 0), (1, 1), (15, 63), (16, 64), (17, 65), (7, 100),
                                     (32, 128))
    pair = L.translation_pair()
    for dy, dx in L.TRANSLATION_OFFSETS:
        x, y = L.crop(pair, dy, dx)
        assert x.shape == y.shape == (2, 32, 128) and x.flags.c_contiguous
        assert 4 * x.size == pair[0].size and x[1, 3, 4] == pair[0][1, dy + 3, dx + 4]
    # the integer images: block counts around the finish loop's trips, sums that stay exact
    assert L.INTEGER_SHAPES == {(5, 100, 1000): 560, (1, 16, 16384): 256, (1, 16, 16385): 257,
                                (2, 16, 16384): 512, (3, 17, 65): 12}
    workspace = _lib.image_loss_fns(_lib.load_library())[0]
    for shape, blocks in L.INTEGER_SHAPES.items():
        assert L.blocks_of(shape) == blocks and workspace(*shape) == 8 * blocks
        x, y = L.integer_images(shape)
        assert x.dtype == y.dtype == np.float32 and x.shape == y.shape == shape
        for a in (x, y):
            assert (a == np.round(a)).all() and a.min() == 0.0 and a.max() == 8.0
        S = int(np.abs(x.astype(np.int64) - y.astype(np.int64)).sum())
        N = np.float64(x.size)
        assert 0 < S < 1 << 22
        q = [np.float32(np.float64(s) / N) for s in (S - 1, S, S + 1)]
        assert q[0] < q[1] < q[2]  # a dropped or doubled unit of |x - y| changes the bits
    assert L.outside_window(48, 192, 0, 0, 5).sum() == 48 * 192 - 36
    assert L.outside_window(48, 192, 24, 96, 10).sum() == 48 * 192 - 441
    assert L.pixel_err(np.array([1.0, 2.0, 4.0]), np.array([1.0, 2.0, 3.0])) == 1.0 / 5.0


def test_committed_seam_spread_is_the_measured_one():
    """SEAM_SPREAD is measured, not chosen: within a factor 2 of a fresh measurement."""
    got = L.measure_seam_spread()
    print("measured float32 seam spread:", got)
    assert set(got) == set(L.SEAM_SPREAD) == {"max", "pixel"}
    for kind in got:
        assert set(got[kind]) == set(L.SEAM_SPREAD[kind]) == set(L.SAVED_NAMES) | {"dL_dimage"}
        for k in L.SAVED_NAMES:
            have, want = L.SEAM_SPREAD[kind][k], got[kind][k]
            assert want / 2.0 <= have <= want * 2.0, (kind, k, have, want)
        assert set(got[kind]["dL_dimage"]) == set(L.SEAM_LAMBDAS)
        for lam in L.SEAM_LAMBDAS:
            have, want = L.SEAM_SPREAD[kind]["dL_dimage"][lam], got[kind]["dL_dimage"][lam]
            assert want / 2.0 <= have <= want * 2.0, (kind, "dL_dimage", lam, have, want)
    # well conditioned: orders of magnitude below the spread that `near` and `dark` set
    assert L.SEAM_SPREAD["max"]["dm_dmu1"] < 1e-3 * L.F32_SPREAD["dm_dmu1"]
    assert L.SEAM_SPREAD["max"]["dL_dimage"][1.0] < 1e-2 * L.F32_SPREAD["dL_dimage"][1.0]


def test_float64_restatement_is_local():
    """The design of the GPU translation test, on the reference: a 32 x 128 crop of the 64 x 256
    pair has the full pair's saved planes 5 pixels inside its border and 4 x its gradient (N is a
    quarter) 10 pixels inside.  Bound 1e-13 of each entry's scale (pixel_err): measured 0.0 here
    (conv2d adds the 121 taps in one order wherever the window sits); 1e-13 leaves room for a
    backend that groups them differently -- a few hundred float64 roundings of 1.1e-16 -- and is
    six orders below the float32 ulp that the GPU test turns on."""
    pair = L.translation_pair()
    worst = 0.0
    for lam in L.SEAM_LAMBDAS:
        full = L.evaluate(*pair, lam)
        for dy, dx in L.TRANSLATION_OFFSETS:
            part = L.evaluate(*L.crop(pair, dy, dx), lam)
            a = part["saved"][:, :, 5:-5, 5:-5]
            b = full["saved"][:, :, dy + 5:dy + L.CROP_H - 5, dx + 5:dx + L.CROP_W - 5]
            assert a.shape == b.shape == (3, 2, 22, 118)
            g = part["dL_dimage"][:, 10:-10, 10:-10]
            h = 4.0 * full["dL_dimage"][:, dy + 10:dy + L.CROP_H - 10, dx + 10:dx + L.CROP_W - 10]
            assert g.shape == h.shape == (2, 12, 108)
            worst = max([worst, L.pixel_err(g, h)] + [L.pixel_err(a[i], b[i]) for i in range(3)])
            # and it is the border that differs: the crop's edge rows see zero padding
            if (dy, dx) != (0, 0):
                assert rel_err(part["saved"][0][:, :5], full["saved"][0][:, dy:dy + 5,
                                                                        dx:dx + L.CROP_W]) > 1e-3
    print(f"float64 locality: worst per-pixel difference {worst:.3g}")
    assert worst <= 1e-13
