"""CPU: the torch restatement of the fused image loss (tests/loss_reference.py) is right -- its
manual backward against float64 autograd, the separable form against the 2-D window -- the
committed float32 spread is what a fresh measurement finds, and the loaded library refuses bad
arguments before any HIP call (include/gsr.h)."""
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
