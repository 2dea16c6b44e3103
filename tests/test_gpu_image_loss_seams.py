"""GPU: the fused L1 + D-SSIM loss (csrc/loss.hip) per pixel, across tile seams and over many
blocks.  test_gpu_image_loss.py holds it to max-norm bounds that the ill-conditioned `near` and
`dark` images set, on grids of at most 2 x 4 tiles and 24 blocks; a few wrong pixels at a seam
pass there.  Here the images are well conditioned (uniform random, or small integers) and most
checks are exact, from properties the code guarantees beyond "close to float64":

   A translation: a pixel's saved planes and gradient do not depend on where it sits in its
     tile or in the image (bitwise)
   B locality: a one-pixel change moves only its 11 x 11 / 21 x 21 footprint (bitwise)
   C the two sums over up to 560 blocks: exact on integer images, whatever k_loss_finish's trips
   D dL_dimage and the saved planes per pixel within 8 x SEAM_SPREAD of float64, from 1 x 1 x 130
     to 5 x 100 x 1000
   E a poisoned or reused workspace, and image and target in one buffer, change no bit
   F reversing the channels reverses the outputs (bitwise)

The float64 references come from loss_reference.seam_reference, computed once and shared.
"""
import ctypes

import numpy as np
import pytest
import torch

import loss_reference as L
from gaussiansplattingviewer_amd import _lib, losses, photometric_loss, ssim
from gpu_helpers import to_dev, to_dev_unaligned
from grad_reference import rel_err

pytestmark = pytest.mark.gpu

IMAGES = L.seam_images()
F, K = L.F32_SPREAD, L.BOUND_FACTOR


def _bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a,
                                np.float32).view(np.uint32)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


def _forward(pair, lam, gpu):
    """-> (values [3] numpy, saved [3, C, H, W] device, x, y device)."""
    x, y = (to_dev(a, gpu) for a in pair)
    values, planes = losses.image_loss_native(x, y, lam, True)
    return values.cpu().numpy(), planes, x, y


def _backward(x, y, lam, planes, gl, gpu):
    g = None if gl is None else torch.tensor([gl], dtype=torch.float32, device=gpu)
    return losses.image_loss_backward_native(x, y, lam, planes, g).cpu().numpy()


def _run(pair, lam, gpu, gl=None):
    """Forward and backward by ctypes -> (values [3], saved, dL_dimage) as numpy."""
    values, planes, x, y = _forward(pair, lam, gpu)
    return values, planes.cpu().numpy(), _backward(x, y, lam, planes, gl, gpu)


def _values_with(pair, lam, gpu, ws, saved=None):
    """gsr_image_loss by ctypes on the caller's workspace tensor -> values [3] as numpy."""
    x, y = (to_dev(a, gpu) for a in pair)
    workspace, forward, _ = _lib.image_loss_fns(_lib.load_library())
    assert ws.numel() * ws.element_size() >= workspace(*x.shape) > 0
    values = torch.full((3,), float("nan"), dtype=torch.float32, device=gpu)
    inp = _lib.GsrImageLossInputs(*x.shape, lam, x.data_ptr(), y.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream(gpu).cuda_stream)
    assert forward(ctypes.byref(inp), values.data_ptr(),
                   None if saved is None else saved.data_ptr(), ws.data_ptr(), stream) == 0
    torch.cuda.synchronize(gpu)
    return values.cpu().numpy()


# ---- A ------------------------------------------------------------------------------------------
_FULL: dict = {}
GLS = (None, 0.75)


def _full(gpu):
    """The 2 x 64 x 256 pair's saved planes and its gradients per (lambda, dL_dloss), once."""
    if not _FULL:
        pair = L.translation_pair()
        _, planes, x, y = _forward(pair, 0.2, gpu)
        _FULL["saved"] = planes.cpu().numpy()
        for lam in L.SEAM_LAMBDAS:
            for gl in GLS:
                _FULL[lam, gl] = _backward(x, y, lam, planes, gl, gpu)
    return _FULL


@pytest.mark.parametrize("dy,dx", L.TRANSLATION_OFFSETS)
def test_translation(dy, dx, gpu):
    """A 32 x 128 crop at (dy, dx) of the 64 x 256 pair (4 x 4 tiles), run as an image of its own.
    A pixel 5 inside the crop's border has its whole window inside the crop and goes through the
    same window4 / vertical4 sequence on the same numbers in both calls: the three saved planes
    have the same bits there.  10 inside, the backward sees the same saved values, image and
    target; N is a quarter and both N are powers of two, so gm and cl are exactly 4 x and so is
    every term: dL_dimage(crop) == 4 dL_dimage(full) bit for bit.

    The offsets put the full image's tile seams at every place relative to the crop's own: on
    them (0, 0; 16, 64; 32, 128), one off either way, and far off (7, 100).  What would fail, in
    loss.hip: `gr = k.r0 - kR + r` / `gc = k.c0 - kR + cc` and the `in` predicate of stage (a
    halo row or column from the wrong place, or zeroed inside the image: a pixel within 5 of a
    seam in one call and not in the other differs); kSin / kSh and the `4 * cg + t`, `4 * rg + t`
    offsets of the two passes (a tap that depends on the position in the tile); tile_of's r0 and
    c0 (the full image has tiles_x = tiles_y = 4, the crop 2 x 2, with C = 2)."""
    full = _full(gpu)
    pair = L.crop(L.translation_pair(), dy, dx)
    values, planes, x, y = _forward(pair, 0.2, gpu)
    assert np.isfinite(values).all()
    H, W = L.CROP_H, L.CROP_W
    got = planes.cpu().numpy()[:, :, 5:H - 5, 5:W - 5]
    want = full["saved"][:, :, dy + 5:dy + H - 5, dx + 5:dx + W - 5]
    assert got.shape == want.shape == (3, 2, 22, 118)
    for i, k in enumerate(L.SAVED_NAMES):
        _same(got[i], want[i], f"{k} of the crop at {(dy, dx)}")
    assert len(np.unique(_bits(got[0]))) > got[0].size // 2  # values, not a constant plane
    for lam in L.SEAM_LAMBDAS:
        for gl in GLS:
            g = _backward(x, y, lam, planes, gl, gpu)[:, 10:H - 10, 10:W - 10]
            h = full[lam, gl][:, dy + 10:dy + H - 10, dx + 10:dx + W - 10]
            assert g.shape == h.shape == (2, 12, 108) and np.isfinite(g).all()
            assert np.abs(h).min() > 1e-30  # 4 x is exact: nothing near the subnormals
            _same(g, np.float32(4.0) * h, f"dL_dimage of the crop at {(dy, dx)}, lambda {lam}, "
                                          f"dL_dloss {gl}")


# ---- B ------------------------------------------------------------------------------------------
_BASE: dict = {}


def _base(gpu):
    if not _BASE:
        for lam in L.SEAM_LAMBDAS:
            _BASE[lam] = _run(IMAGES[L.shape_name(L.LOCALITY_SHAPE)], lam, gpu)
    return _BASE


@pytest.mark.parametrize("r,c", L.LOCALITY_PIXELS)
def test_one_pixel_moves_only_its_footprint(r, c, gpu):
    """image[1, r, c] of the 2 x 48 x 192 pair (3 x 3 tiles) changes by 0.5.  Outside the 11 x 11
    window around (r, c) the saved planes of channel 1 keep their bits, outside the 21 x 21 window
    its gradient does (the changed x also enters 2 x (gm cb) and the sign at its own pixel,
    inside the window); channel 0 keeps every bit.  Inside, something changes.

    The pixels are the image's corners, both sides of a tile corner, (16, 63) and the middle of
    the interior tile.  What would fail, in loss.hip: a window wider than 11 taps or a kSpan /
    `4 * cg + t` offset that reaches a 12th value; LDS rows that overlap (kSin, kSh shorter than
    the rows they hold), through which a value leaks to a row it does not belong to; `plane` or
    tile_of's `k.c` (channel 0 would see channel 1's pixel); a store outside the thread's own
    pixel (`at`), or one that the `gr >= H || gc >= W` skip should have stopped."""
    base = _base(gpu)
    image, target = (a.copy() for a in IMAGES[L.shape_name(L.LOCALITY_SHAPE)])
    image[1, r, c] = np.float32((image[1, r, c] + 0.5) % 1.0)
    _, H, W = image.shape
    far5, far10 = L.outside_window(H, W, r, c, 5), L.outside_window(H, W, r, c, 10)
    assert 0 < (~far5).sum() <= 121 and 0 < (~far10).sum() <= 441
    for lam in L.SEAM_LAMBDAS:
        values, planes, grad = _run((image, target), lam, gpu)
        v0, p0, g0 = base[lam]
        assert values[1] != v0[1]  # the input did change
        for i, k in enumerate(L.SAVED_NAMES):
            _same(planes[i, 0], p0[i, 0], f"{k} channel 0")
            _same(planes[i, 1][far5], p0[i, 1][far5], f"{k} channel 1 outside the window")
            assert (_bits(planes[i, 1][~far5]) != _bits(p0[i, 1][~far5])).any(), k
        _same(grad[0], g0[0], "dL_dimage channel 0")
        _same(grad[1][far10], g0[1][far10], "dL_dimage channel 1 outside the window")
        assert (_bits(grad[1][~far10]) != _bits(g0[1][~far10])).any()
        assert _bits(grad[1, r, c]) != _bits(g0[1, r, c])


# ---- C ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(L.INTEGER_SHAPES), ids=L.shape_name)
def test_integer_images_sum_exactly(shape, gpu):
    """Image and target hold integers 0..8, so every |x - y|, thread sum, shuffle-tree sum and
    block pair of the L1 term is an integer below 2^24, exact in float32, and k_loss_finish's
    double sum S is exact whatever its order: l1 is float32(S / N) bit for bit, and with lambda
    0 so is the loss (0 (1 - ssim) adds nothing while ssim is finite).  S < 2^22, so S - 1 and
    S + 1 give other bits (test_loss_reference.py asserts it too): one unit of one pixel shows.

    Blocks: 12; 256 | 257 and 512 (the finish loop `for (i = threadIdx.x; i < blocks; i +=
    kThreads)` ends its first and second trip there); 560 with a ragged last row and column of
    tiles.  What would fail, in loss.hip: that loop's bound or stride (pairs dropped or added
    twice from 257 blocks on); `partial[2 * blockIdx.x]`; the shuffle tree and the `red[0][..]`
    sum of the four waves; tile_of (a tile visited twice and another never); in stage, an `in`
    predicate that zeroes or repeats a pixel of the image; lambda = 0 is also exactly the L1
    gradient, sign(x - y) / N and 0 at the (many) ties, which `gr >= H || gc >= W` and `at` of
    k_loss_backward must get right in every ragged tile."""
    image, target = L.integer_images(shape)
    N = image.size
    S = int(np.abs(image.astype(np.int64) - target.astype(np.int64)).sum())
    assert S < 1 << 22 and L.blocks_of(shape) == L.INTEGER_SHAPES[shape]
    want = np.float32(np.float64(S) / np.float64(N))
    assert np.float32(np.float64(S - 1) / np.float64(N)) < want < \
        np.float32(np.float64(S + 1) / np.float64(N))
    values, _, grad = _run((image, target), 0.0, gpu)
    print(f"{L.shape_name(shape)}: {L.INTEGER_SHAPES[shape]} blocks, S {S}, l1 {values[1]!r}, "
          f"want {want!r}, ssim {values[2]!r}")
    assert np.isfinite(values).all()
    _same(values[1], want, "l1")
    _same(values[0], values[1], "loss at lambda 0")
    step = np.float32(1.0) / np.float32(N)
    assert (grad == (np.sign(image - target) * step).astype(np.float32)).all()
    ties = image == target
    assert ties.sum() > N // 20 and (grad[ties] == 0.0).all()
    assert set(np.unique(np.abs(grad[~ties]))) == {step}
    # without the saved planes (k_loss_forward<false>) the sums are the same
    x, y = (to_dev(a, gpu) for a in (image, target))
    _same(losses.image_loss_native(x, y, 0.0, False)[0], values, "values, saved = NULL")


def test_many_blocks_values(gpu):
    """The uniform random 5 x 100 x 1000 pair (560 blocks, three trips of the finish loop): loss,
    l1 and ssim within the standing 8 x F32_SPREAD of float64 at lambda 0.2, twice the same
    bits.  A block's share of either sum is about 1 / 560 = 1.8e-3 and l1's bound is 7.3e-7: a
    dropped or doubled block pair is far outside it (a single pixel is not: the integer images'
    part).  The 16 x 7 tiles end in 4 rows and 40 columns: without k_loss_forward's `gr >= H ||
    gc >= W` skip the out-of-image pixels of those tiles would add their map (1 where the
    window sees only padding) to the ssim sum."""
    name = L.shape_name((5, 100, 1000))
    ref = L.seam_reference(name, 0.2)
    first = _run(IMAGES[name], 0.2, gpu)
    for k, got, f in (("loss", first[0][0], F["loss"][0.2]), ("l1", first[0][1], F["l1"]),
                      ("ssim", first[0][2], F["ssim"])):
        e = rel_err(got, ref[k])
        print(f"{name} {k}: rel_err {e:.3g}, bound {K:g} x {f:.3g}, ratio {e / (K * f):.3f}")
        assert e <= K * f, (k, e, K * f)
    again = _run(IMAGES[name], 0.2, gpu)
    for a, b, what in zip(again, first, ("values", "saved", "dL_dimage")):
        _same(a, b, what)


# ---- D ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(IMAGES))
def test_per_pixel_bounds(name, gpu):
    """dL_dimage (lambda 0.2 and 1) and the three saved planes against float64, in two norms:
    rel_err (max-norm) and pixel_err, max |got - ref| / (|ref| + median|ref|), each within 8 x
    SEAM_SPREAD -- the float32 restatement's own distance to float64 on these images, the larger
    of its 2-D and separable forms (loss_reference.py; re-measured by test_loss_reference.py).
    The max-norm bounds are 8.8e-6 .. 1.0e-4 where test_gpu_image_loss.py allows 3.5e-4 .. 0.5."""
    image, target = IMAGES[name]
    for lam in L.SEAM_LAMBDAS:
        ref = L.seam_reference(name, lam)
        _, planes, grad = _run((image, target), lam, gpu)
        assert planes.shape == (3, *image.shape) and grad.shape == image.shape
        checks = [("dL_dimage", grad, ref["dL_dimage"],
                   {kind: L.SEAM_SPREAD[kind]["dL_dimage"][lam] for kind in L.SEAM_ERRORS})]
        if lam == L.SEAM_LAMBDAS[0]:
            checks += [(k, planes[i], ref["saved"][i],
                        {kind: L.SEAM_SPREAD[kind][k] for kind in L.SEAM_ERRORS})
                       for i, k in enumerate(L.SAVED_NAMES)]
        failed = []
        for k, got, want, f in checks:
            for kind, err in L.SEAM_ERRORS.items():
                e = err(got, want)
                print(f"{name} lambda {lam} {k} {kind}: err {e:.3g}, bound {K:g} x {f[kind]:.3g}, "
                      f"ratio {e / (K * f[kind]):.3f}")
                if not e <= K * f[kind]:
                    failed.append((k, kind, lam, e, K * f[kind]))
        assert not failed, failed


# ---- E ------------------------------------------------------------------------------------------
def test_workspace_leftovers_do_not_leak(gpu):
    """The workspace is scratch: every pair a call reads, it wrote in that call (k_loss_finish
    reads `blocks` pairs, k_loss_forward writes one per block).  NaN bytes before the call, or
    the pairs of an earlier, larger call behind this call's own, change no bit of the values."""
    workspace = _lib.image_loss_fns(_lib.load_library())[0]
    fresh = {}
    for shape in ((3, 33, 129), (5, 100, 1000), (2, 5, 5)):
        pair = IMAGES[L.shape_name(shape)]
        ws = torch.zeros(workspace(*shape), dtype=torch.uint8, device=gpu)
        fresh[shape] = _values_with(pair, 0.2, gpu, ws)
        assert np.isfinite(fresh[shape]).all()
        _same(fresh[shape], _run(pair, 0.2, gpu)[0], f"{shape}: own workspace")
    poisoned = torch.full((workspace(3, 33, 129),), 0xFF, dtype=torch.uint8, device=gpu)
    assert torch.isnan(poisoned.view(torch.float32)).all()
    _same(_values_with(IMAGES["3x33x129"], 0.2, gpu, poisoned), fresh[3, 33, 129], "poisoned")
    assert not torch.isnan(poisoned.view(torch.float32)).any()  # all 27 pairs were written
    shared = torch.full((workspace(5, 100, 1000),), 0xFF, dtype=torch.uint8, device=gpu)
    for shape in ((5, 100, 1000), (2, 5, 5), (3, 33, 129)):
        got = _values_with(IMAGES[L.shape_name(shape)], 0.2, gpu, shared)
        _same(got, fresh[shape], f"{shape} on the shared workspace")


def test_image_and_target_in_one_buffer(gpu):
    """Both arguments may be the same storage (the kernels only read them), and may be views of
    one buffer at pointers that are 4-byte aligned only."""
    image, target = IMAGES["3x33x129"]
    x = to_dev(image, gpu).requires_grad_(True)
    loss, l1, ss = photometric_loss(x, x.detach(), return_parts=True)
    loss.backward()
    assert float(l1) == 0.0 and abs(float(ss) - 1.0) <= K * F["ssim"]
    assert torch.isfinite(x.grad).all() and torch.isfinite(loss)
    assert abs(float(ssim(x.detach(), x.detach())) - 1.0) <= K * F["ssim"]
    # one buffer, image one float in, target behind it at the next address that is 4 mod 8
    N = image.size
    gap = 1 + N + (N % 2)
    buf = torch.full((gap + N + 1,), float("nan"), dtype=torch.float32, device=gpu)
    xv, yv = buf[1:1 + N].view(image.shape), buf[gap:gap + N].view(image.shape)
    xv.copy_(torch.as_tensor(image))
    yv.copy_(torch.as_tensor(target))
    assert xv.data_ptr() % 8 == 4 and yv.data_ptr() % 8 == 4 and xv.is_contiguous()
    want = _run((image, target), 0.2, gpu, gl=0.75)
    values, planes = losses.image_loss_native(xv, yv, 0.2, True)
    grad = losses.image_loss_backward_native(
        xv, yv, 0.2, planes, torch.tensor([0.75], dtype=torch.float32, device=gpu))
    for a, b, what in zip((values, planes, grad), want, ("values", "saved", "dL_dimage")):
        _same(a, b, what)
    host = buf.cpu().numpy()
    assert np.isnan(host[0]) and np.isnan(host[1 + N:gap]).all() and np.isnan(host[gap + N:]).all()
    # and through the public entry, which keeps such views as they are
    xu = to_dev_unaligned(image, gpu).requires_grad_(True)
    (0.75 * photometric_loss(xu, to_dev_unaligned(target, gpu))).backward()
    _same(xu.grad, want[2], "dL_dimage through photometric_loss")


# ---- F ------------------------------------------------------------------------------------------
def test_channels_are_independent(gpu):
    """The 3 x 33 x 129 pair (3 x 3 tiles per channel) with its channels reversed: the saved
    planes and dL_dimage come out reversed with the same bits.  A block's channel and its
    plane's offset come from tile_of (`k.c = t / tiles_y`, `k.r0 = (t - k.c tiles_y) kTh`) and
    `plane = k.c H W`: a mix-up there with C = 3, tiles_x = tiles_y = 3 reads or writes another
    channel's tile and cannot commute with the reversal.  The three values keep their bits too:
    the block pairs reach k_loss_finish in another order, but its double sum of 27 floats is far
    inside double's 53 bits, and it is rounded to float32 once."""
    image, target = IMAGES["3x33x129"]
    values, planes, grad = _run((image, target), 0.2, gpu, gl=0.75)
    flipped = tuple(np.ascontiguousarray(a[::-1]) for a in (image, target))
    assert not (flipped[0][0] == image[0]).all()
    v, p, g = _run(flipped, 0.2, gpu, gl=0.75)
    _same(p[:, ::-1], planes, "saved")
    _same(g[::-1], grad, "dL_dimage")
    _same(v, values, "values")
    assert not (_bits(grad[0]) == _bits(grad[2])).all()  # the channels do differ
