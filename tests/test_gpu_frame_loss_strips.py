"""GPU: the frame's loss on a window of its rows (gsr_image_loss_window and its backward,
csrc/loss.hip; losses.frame_loss_on_strip) against the whole-frame call's bits and the float64
restatement.  Windows: frame_loss_reference.WINDOW_CASES -- (3, 40, 70) in tile-row strips of 16,
16 and 8 rows, (1, 11, 5) as one strip, (2, 48, 130) in arbitrary pixel windows off the frame's
tile grid, (3, 33, 129) in windows of 1 and 32 rows; lambda 0, 0.2, 1; dL_dloss NULL and 0.75.

   1 bits per pixel: every window's `saved` (apron rows) and dL_dimage (own rows) are the
     whole-frame call's bits at those rows
   2 the shares, added in float64 on the host, against the float64 reference within
     (8 x the float32 spread + R 2^-24) |value|, R = the number of shares
   3 the whole-frame window has gsr_image_loss's bits in values, saved and the gradient
   4 zero at seams is wrong: the strip-alone photometric_loss gradient, weighted by the strip's
     share of the elements, is the frame's away from a seam and not next to one; the windowed
     gradient is the frame's everywhere
   5 halo contents: NaN in every band row the call need not read changes nothing; a NaN in row
     own_begin - 10 reaches dL_dimage on exactly its 21 x 21 footprint
   6 guard words around values, saved, dL_dimage and the workspace; a dirty workspace and a second
     stream give the same bits
   7 ctypes, `_C` and frame_loss_on_strip give the same bits; no_grad keeps nothing
   8 end to end through GaussianRasterizer(tile_rows=, deterministic=True) on frame_grad_scenes'
     `frame`: every band's color.grad is the frame's dL_dimage rows bit for bit, and the Gaussians'
     gradients summed over the bands lie within the strip bound of the frame fit's
"""
import ctypes

import numpy as np
import pytest
import torch

import frame_grad_scenes as fs
import frame_loss_reference as R
import loss_reference as L
import strip_grad_scenes as ss
from gaussiansplattingviewer_amd import (GaussianRasterizationSettings, GaussianRasterizer, _C,
                                         _lib, frame_loss_on_strip, losses, photometric_loss)
from gpu_helpers import to_dev, to_dev_unaligned
from test_gpu_backward import _inputs

pytestmark = pytest.mark.gpu

SHAPES = list(R.WINDOW_CASES)
IDS = [L.shape_name(s) for s in SHAPES]
F = L.F32_SPREAD


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a,
                                np.float32).view(np.uint32)


def _same(a, b, what):
    np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=what)


def _gl(gl, gpu):
    return None if gl is None else torch.tensor([gl], dtype=torch.float32, device=gpu)


_FRAMES: dict = {}


def _frame(shape, lam, gl, gpu):
    """The whole-frame call on a shape's pair, once: (x, y on the device; values, saved, grad)."""
    key = (shape, lam, gl)
    if key not in _FRAMES:
        if ("dev", shape) not in _FRAMES:
            _FRAMES[("dev", shape)] = tuple(to_dev(a, gpu) for a in R.window_pair(shape))
        x, y = _FRAMES[("dev", shape)]
        values, saved = losses.image_loss_native(x, y, lam, True)
        grad = losses.image_loss_backward_native(x, y, lam, saved, _gl(gl, gpu))
        _FRAMES[key] = (x, y, values.cpu().numpy(), saved.cpu().numpy(), grad.cpu().numpy())
    return _FRAMES[key]


def _band(t, row0, rows):
    return t[:, row0:row0 + rows].contiguous()


def _window(x, y, H, win, lam, gl, gpu, saved=True):
    """gsr_image_loss_window and its backward by ctypes on a window of the device frame (x, y)
    -> (values, saved, dL_dimage) as numpy (the last two None without `saved`)."""
    row0, rows, own = win
    bx, by = _band(x, row0, rows), _band(y, row0, rows)
    values, planes = losses.image_loss_window_native(bx, by, H, row0, own, lam, saved)
    if not saved:
        return values.cpu().numpy(), None, None
    grad = losses.image_loss_window_backward_native(bx, by, H, row0, own, lam, planes,
                                                    _gl(gl, gpu))
    return values.cpu().numpy(), planes.cpu().numpy(), grad.cpu().numpy()


# ---- 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_bits_per_pixel(shape, gpu):
    H = shape[1]
    for lam in L.LAMBDAS:
        for gl in R.GLS:
            x, y, _, saved, grad = _frame(shape, lam, gl, gpu)
            for win in R.WINDOW_CASES[shape]:
                own = win[2]
                a0, a1 = R.apron_of(own, H)
                _, s, g = _window(x, y, H, win, lam, gl, gpu)
                assert s.shape == (3, shape[0], a1 - a0, shape[2])
                assert g.shape == (shape[0], own[1] - own[0], shape[2])
                what = f"{shape} window {win} lambda {lam} dL_dloss {gl}"
                _same(s, saved[:, :, a0:a1], what + ": saved")
                _same(g, grad[:, own[0]:own[1]], what + ": dL_dimage")


# ---- 2 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_shares_add_up_to_the_frame(shape, gpu):
    H, worst = shape[1], 0.0
    windows = R.WINDOW_CASES[shape]
    for lam in L.LAMBDAS:
        ref = R.window_reference(shape, lam)
        x, y = _frame(shape, lam, None, gpu)[:2]
        for with_saved in (True, False):
            shares = np.array([_window(x, y, H, win, lam, None, gpu, with_saved)[0]
                               for win in windows], np.float64)
            for i, (k, f) in enumerate((("loss", F["loss"][lam]), ("l1", F["l1"]),
                                        ("ssim", F["ssim"]))):
                e = abs(float(shares[:, i].sum()) - ref[k])
                b = R.share_sum_bound(ref[k], f, len(windows))
                print(f"{shape} lambda {lam} saved {with_saved} {k}: |sum - ref| {e:.3g} = "
                      f"{e / b if b else 0.0:.3g} of {b:.3g}")
                assert e <= b, (k, lam, e, b)
                worst = max(worst, e / b if b else 0.0)
    print(f"{shape}: largest e / bound {worst:.3g}")


# ---- 3 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_whole_frame_window(shape, gpu):
    H = shape[1]
    for lam in L.LAMBDAS:
        for gl in R.GLS:
            x, y, values, saved, grad = _frame(shape, lam, gl, gpu)
            v, s, g = _window(x, y, H, (0, H, (0, H)), lam, gl, gpu)
            for a, b, what in ((v, values, "values"), (s, saved, "saved"), (g, grad, "dL_dimage")):
                _same(a, b, f"{shape} lambda {lam} dL_dloss {gl}: {what}")
            _same(_window(x, y, H, (0, H, (0, H)), lam, gl, gpu, saved=False)[0], values,
                  f"{shape} lambda {lam}: values without saved")


# ---- 4 ------------------------------------------------------------------------------------------
def test_zero_padding_at_a_seam_is_not_the_frames_loss(gpu):
    shape, lam = (3, 40, 70), 1.0
    C, H, W = shape
    x, y, _, _, grad = _frame(shape, lam, None, gpu)
    scale = float(np.abs(grad).max())
    for row0, rows, own in R.WINDOW_CASES[shape]:
        r = own[1] - own[0]
        strip = x[:, own[0]:own[1]].clone().requires_grad_(True)
        # the strip alone, weighted by its share of the frame's elements
        (photometric_loss(strip, y[:, own[0]:own[1]], lam) * (r / H)).backward()
        alone = np.abs(strip.grad.cpu().numpy() - grad[:, own[0]:own[1]]).max(axis=(0, 2)) / scale
        seams = [s for s in (own[0], own[1]) if 0 < s < H]
        dist = np.array([min(min(abs(q - s), abs(q + 1 - s)) for s in seams)
                         for q in range(own[0], own[1])])
        print(f"strip {own}: strip-alone error per row / max|grad| {np.round(alone, 6)}")
        # a row whose 21-row footprint crosses no seam: only roundings differ (the weight r / H
        # and 1 / N_strip against 1 / N: a few float32 ulps of the gradient)
        assert (alone[dist >= 10] <= 16 * 2.0 ** -24).all()
        # the row at the seam loses nearly half of its window to the padding: an error of the
        # gradient's own order
        assert (alone[dist == 0] > 1e-2).all()
        windowed = _window(x, y, H, (row0, rows, own), lam, None, gpu)[2]
        _same(windowed, grad[:, own[0]:own[1]], f"strip {own}: windowed gradient")


# ---- 5 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,own", [((2, 48, 130), (20, 28)), ((3, 40, 70), (16, 32)),
                                       ((3, 40, 70), (32, 40))])
def test_rows_beyond_the_halo_are_not_read(shape, own, gpu):
    C, H, W = shape
    lam = 0.2
    x, y = _frame(shape, lam, None, gpu)[:2]
    win = (0, H, own)  # the whole frame as the band: rows the call need not read on both sides
    for with_saved, reach in ((True, 10), (False, 5)):
        clean = _window(x, y, H, win, lam, 0.75, gpu, with_saved)
        px, py = x.clone(), y.clone()
        for t in (px, py):
            t[:, :max(0, own[0] - reach)] = float("nan")
            t[:, min(H, own[1] + reach):] = float("nan")
        assert bool(torch.isnan(px).any()) or (own[0] < reach and own[1] + reach > H)
        dirty = _window(px, py, H, win, lam, 0.75, gpu, with_saved)
        for a, b, what in zip(dirty, clean, ("values", "saved", "dL_dimage")):
            if a is not None:
                assert np.isfinite(a).all(), what
                _same(a, b, f"{shape} own {own} saved {with_saved}: {what}")


def test_a_nan_in_the_outermost_halo_row_reaches_its_footprint(gpu):
    shape, own, lam = (2, 48, 130), (20, 28), 0.2
    C, H, W = shape
    x, y = _frame(shape, lam, None, gpu)[:2]
    clean = _window(x, y, H, (10, 28, own), lam, None, gpu)
    px = x.clone()
    c, row, col = 1, own[0] - 10, 64
    px[c, row, col] = float("nan")
    values, saved, grad = _window(px, y, H, (10, 28, own), lam, None, gpu)
    _same(values, clean[0], "the shares read +- 5 rows only")
    hit = np.isnan(grad)
    want = np.zeros_like(hit)
    want[c, 0, col - 10:col + 11] = True  # the own row 10 rows below, 21 columns
    np.testing.assert_array_equal(hit, want)
    _same(grad[~want], clean[2][~want], "outside the footprint")
    # and through the saved planes: the apron's first row, 11 columns
    shit = np.isnan(saved)
    swant = np.zeros_like(shit)
    swant[:, c, 0, col - 5:col + 6] = True
    np.testing.assert_array_equal(shit, swant)


# ---- 6 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,win", [((3, 40, 70), (6, 34, (16, 32))),
                                       ((2, 48, 130), (13, 35, (23, 48))),
                                       ((1, 11, 5), (0, 11, (0, 11)))])
def test_guards_dirty_workspace_and_streams(shape, win, gpu):
    C, H, W = shape
    row0, rows, own = win
    lam = 0.2
    pair = R.window_pair(shape)
    bx, by = (to_dev_unaligned(a[:, row0:row0 + rows], gpu) for a in pair)
    x, y = _frame(shape, lam, None, gpu)[:2]
    want = _window(x, y, H, win, lam, None, gpu)
    workspace, forward, backward = _lib.image_loss_window_fns(_lib.load_library())
    inp = _lib.GsrImageLossInputs(C, rows, W, lam, bx.data_ptr(), by.data_ptr())
    w = _lib.GsrLossWindow(H, row0, own[0], own[1])
    a0, a1 = R.apron_of(own, H)
    nS, nG = 3 * C * (a1 - a0) * W, C * (own[1] - own[0]) * W
    nW = workspace(ctypes.byref(inp), ctypes.byref(w)) // 4
    assert nW > 0
    nan = lambda n: torch.full((n,), float("nan"), dtype=torch.float32, device=gpu)  # noqa: E731
    pad = 64
    at = lambda t: t.data_ptr() + 4  # noqa: E731

    def run(stream):
        vbuf, sbuf, gbuf, wbuf, v2 = (nan(1 + n + pad) for n in (3, nS, nG, nW, 3))
        handle = ctypes.c_void_p(stream.cuda_stream)
        torch.cuda.synchronize(gpu)  # the buffers were filled on the current stream
        with torch.cuda.stream(stream):
            assert forward(ctypes.byref(inp), ctypes.byref(w), at(vbuf), at(sbuf), at(wbuf),
                           handle) == 0
            assert backward(ctypes.byref(inp), ctypes.byref(w), at(sbuf), None, at(gbuf),
                            handle) == 0
            # the same (now dirty) workspace again, without saved
            assert forward(ctypes.byref(inp), ctypes.byref(w), at(v2), None, at(wbuf),
                           handle) == 0
        stream.synchronize()
        out = []
        for buf, n in ((vbuf, 3), (sbuf, nS), (gbuf, nG), (wbuf, nW), (v2, 3)):
            host = buf.cpu().numpy()
            assert np.isnan(host[0]) and np.isnan(host[1 + n:]).all()
            out.append(host[1:1 + n])
        assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all() and np.isfinite(out[2]).all()
        return out

    first = run(torch.cuda.current_stream(gpu))
    _same(first[0], want[0], "values")
    _same(first[1], want[1].reshape(-1), "saved")
    _same(first[2], want[2].reshape(-1), "dL_dimage")
    again = run(torch.cuda.current_stream(gpu))
    other = run(torch.cuda.Stream(gpu))
    for r in (again, other):
        for a, b, what in zip(r, first, ("values", "saved", "dL_dimage", "workspace", "values2")):
            _same(a, b, what)


# ---- 7 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 40, 70), (1, 11, 5)], ids=["3x40x70", "1x11x5"])
def test_routes_give_the_same_bits(shape, gpu, monkeypatch):
    C, H, W = shape
    lam = 0.2
    x, y = _frame(shape, lam, None, gpu)[:2]
    kept = []
    inner = losses._window_forward

    def spy(*args):
        out = inner(*args)
        kept.append((args[-1], out[1]))
        return out
    monkeypatch.setattr(losses, "_window_forward", spy)
    for row0, rows, own in R.WINDOW_CASES[shape]:
        values, saved, grad = _window(x, y, H, (row0, rows, own), lam, 0.75, gpu)
        bx, by = _band(x, row0, rows), _band(y, row0, rows)
        v, s = _C.fused_image_loss_window(bx, by, H, row0, own[0], own[1], lam, True)
        g = _C.fused_image_loss_window_backward(bx, by, H, row0, own[0], own[1], lam, s,
                                                torch.tensor([0.75], device=gpu))
        for a, b, what in ((v, values, "values"), (s, saved, "saved"), (g, grad, "dL_dimage")):
            _same(a, b, f"_C {own}: {what}")
        v0, s0 = _C.fused_image_loss_window(bx, by, H, row0, own[0], own[1], lam, False)
        assert s0.numel() == 0
        # the public entry, halos sliced from the frame
        a, b = losses.halo_counts(own, H)
        above = x[:, own[0] - a:own[0]] if a else None
        below = x[:, own[1]:own[1] + b] if b else None
        strip = x[:, own[0]:own[1]].clone().requires_grad_(True)
        loss, l1, ssim = frame_loss_on_strip(strip, y, own, above=above, below=below,
                                             lambda_dssim=lam, return_parts=True)
        assert loss.dim() == 0 and loss.requires_grad and not l1.requires_grad
        (0.75 * loss).backward()
        _same(torch.stack([loss, l1, ssim]), values, f"frame_loss_on_strip {own}: shares")
        _same(strip.grad, grad, f"frame_loss_on_strip {own}: gradient")
        assert kept[-1][0] is True
        with torch.no_grad():
            quiet = frame_loss_on_strip(strip, y, own, above=above, below=below, lambda_dssim=lam)
        assert kept[-1] == (False, None) and not quiet.requires_grad
        _same(quiet, v0[0], "no_grad: the share without saved")
        plain = frame_loss_on_strip(strip.detach(), y, own, above=above, below=below,
                                    lambda_dssim=lam)
        assert kept[-1] == (False, None) and not plain.requires_grad
    # an empty strip: a zero share that reads nothing
    empty = x[:, H:H].clone().requires_grad_(True)
    zero = frame_loss_on_strip(empty, y, (H, H))
    assert float(zero.detach()) == 0.0
    zero.backward()
    assert empty.grad.shape == (C, 0, W)


# ---- 8 ------------------------------------------------------------------------------------------
LEAVES = (("means3D", "means3D"), ("means2D", "means2D"), ("opacities", "opacity"),
          ("shs", "shs"), ("scales", "scales"), ("rotations", "rotations"))


def test_bands_through_the_rasterizer_fit_the_frames_loss(gpu):
    sc = fs.get("frame")
    s, H, W = sc["s"], sc["H"], sc["W"]
    target = to_dev(np.random.default_rng(11).uniform(0, 1, (3, H, W)).astype(np.float32), gpu)

    def render(strip):
        d = _inputs(sc, gpu)
        for v in d.values():
            if v is not None:
                v.requires_grad_(True)
        leaves = dict(d, means2D=torch.zeros_like(d["means3D"], requires_grad=True))
        rs = GaussianRasterizationSettings(
            H, W, s["tx"], s["ty"], to_dev(s["bg"], gpu), s["scale_modifier"],
            to_dev(s["view"], gpu), to_dev(s["proj"], gpu), s["sh_degree"],
            to_dev(s["campos"], gpu), False, False, tile_rows=strip, deterministic=True)
        color, _ = GaussianRasterizer(rs)(means2D=leaves["means2D"], **d)
        color.retain_grad()
        return leaves, color

    leaves, frame = render(None)
    loss = photometric_loss(frame, target)
    loss.backward()
    whole = {k: t.grad.cpu().numpy().astype(np.float64) for k, t in leaves.items()
             if t is not None and t.grad is not None}
    frame_grad, whole_render = frame.grad, frame.detach()
    shares, parts = [], []
    for strip in ss.STRIPS["frame"]:
        y0, y1 = ss.pixel_rows(sc, strip)
        a, b = losses.halo_counts((y0, y1), H)
        bl, color = render(strip)
        _same(color, whole_render[:, y0:y1], f"strip {strip}: the render")
        share = frame_loss_on_strip(color, target, (y0, y1),
                                    above=whole_render[:, y0 - a:y0] if a else None,
                                    below=whole_render[:, y1:y1 + b] if b else None)
        share.backward()
        _same(color.grad, frame_grad[:, y0:y1], f"strip {strip}: color.grad")
        shares.append(float(share))
        parts.append({k: t.grad.cpu().numpy().astype(np.float64) for k, t in bl.items()
                      if t is not None and t.grad is not None})
    # the shares' bound of check 2, here against the frame's own float32 loss
    e = abs(sum(shares) - float(loss))
    print(f"shares {shares} sum {sum(shares)!r}, frame loss {float(loss)!r}")
    assert e <= R.share_sum_bound(float(loss), F["loss"][0.2], len(shares))
    seen = 0
    for leaf, key in LEAVES:
        if leaf not in whole:
            continue
        allow = fs.bound("frame", "colour", key) * float(np.abs(whole[leaf]).max())
        for strip, p in zip(ss.STRIPS["frame"], parts):
            allow += ss.bound("frame", strip, "colour", key) * float(np.abs(p[leaf]).max())
        d = float(np.abs(sum(p[leaf] for p in parts) - whole[leaf]).max())
        print(f"{leaf}: |sum of bands - frame| {d:.3e} = {d / allow:.3f} of {allow:.3e}")
        assert d <= allow and np.abs(whole[leaf]).max() > 0, leaf
        seen += 1
    assert seen >= 5
