"""The photometric loss (gsr_image_loss, include/gsr.h) restated in torch: the definition with
`conv2d`, groups = C, evaluated in float64 (the reference) and in float32 (the yardstick of a
correct float32 implementation's rounding, and the path a user without the fused kernels runs).
CPU for the tests; `tools/bench_loss.py` times the same float32 restatement on the GPU.

  loss = (1 - lam) * mean|image - target| + lam * (1 - mean(map)),  map = Cc D / (A B)

`evaluate` gives every output the kernels produce: the three values, dL_dimage by autograd of the
definition, and the three saved partial derivatives by their formulas.  `manual_gradient` is the
backward the kernels implement (the window is symmetric: conv is its own adjoint under zero
padding); test_loss_reference.py holds it to float64 autograd.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from grad_reference import rel_err

RADIUS, SIGMA = 5, 1.5
C1, C2 = 0.01 ** 2, 0.03 ** 2
LAMBDAS = (0.0, 0.2, 1.0)
TILE_H, TILE_W = 16, 64  # csrc/loss.hip's tile: the sizes at which a halo or an edge tile goes wrong


def window_1d(dtype=torch.float64) -> torch.Tensor:
    """g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), normalised in float64 (float32: its roundings)."""
    i = np.arange(2 * RADIUS + 1, dtype=np.float64)
    g = np.exp(-((i - RADIUS) ** 2) / (2.0 * SIGMA ** 2))
    return torch.tensor(g / g.sum(), dtype=torch.float64).to(dtype)


def conv(x: torch.Tensor) -> torch.Tensor:
    """The "same" correlation of [C, H, W] with the 2-D window g (x) g, zero padding of 5."""
    g = window_1d(x.dtype).to(x.device)
    w = torch.outer(g, g).expand(x.shape[0], 1, -1, -1).contiguous()
    return F.conv2d(x[None], w, padding=RADIUS, groups=x.shape[0])[0]


def conv_separable(x: torch.Tensor) -> torch.Tensor:
    """`conv` as a horizontal then a vertical 11-tap pass (what the kernels do)."""
    C = x.shape[0]
    g = window_1d(x.dtype).to(x.device)
    h = F.conv2d(x[None], g.view(1, 1, 1, -1).expand(C, 1, 1, -1).contiguous(),
                 padding=(0, RADIUS), groups=C)
    return F.conv2d(h, g.view(1, 1, -1, 1).expand(C, 1, -1, 1).contiguous(),
                    padding=(RADIUS, 0), groups=C)[0]


def statistics(image, target, conv_fn=conv):
    mu1, mu2 = conv_fn(image), conv_fn(target)
    s1 = conv_fn(image * image) - mu1 * mu1
    s2 = conv_fn(target * target) - mu2 * mu2
    s12 = conv_fn(image * target) - mu1 * mu2
    A, B = mu1 * mu1 + mu2 * mu2 + C1, s1 + s2 + C2
    Cc, D = 2.0 * mu1 * mu2 + C1, 2.0 * s12 + C2
    return mu1, mu2, A, B, Cc, D


def loss_values(image, target, lam, conv_fn=conv):
    """(loss, l1, ssim) as 0-dim tensors of the images' dtype."""
    _, _, A, B, Cc, D = statistics(image, target, conv_fn)
    ssim = (Cc * D / (A * B)).mean()
    l1 = (image - target).abs().mean()
    return (1.0 - lam) * l1 + lam * (1.0 - ssim), l1, ssim


def saved_partials(image, target, conv_fn=conv):
    """[3, C, H, W]: dm_dmu1, dm_ds1, dm_ds12 of map = Cc D / (A B)."""
    mu1, mu2, A, B, Cc, D = statistics(image, target, conv_fn)
    dm_dmu1 = (2.0 * mu2 * D / (A * B) - 2.0 * mu2 * Cc / (A * B)
               - 2.0 * mu1 * Cc * D / (A * A * B) + 2.0 * mu1 * Cc * D / (A * B * B))
    return torch.stack([dm_dmu1, -Cc * D / (A * B * B), 2.0 * Cc / (A * B)])


def manual_gradient(image, target, lam, gl=1.0, conv_fn=conv):
    """dL_dimage by the formula of include/gsr.h."""
    N = image.numel()
    s = saved_partials(image, target)
    gm = -gl * lam / N
    return (conv_fn(gm * s[0]) + 2.0 * image * conv_fn(gm * s[1]) + target * conv_fn(gm * s[2])
            + gl * (1.0 - lam) / N * torch.sign(image - target))


def evaluate(image, target, lam, dtype=torch.float64, conv_fn=conv) -> dict:
    """Every output of the fused loss for numpy float32 images, evaluated in `dtype`:
    loss, l1, ssim (floats), dL_dimage (autograd of the definition) and saved [3, C, H, W]."""
    x = torch.tensor(np.asarray(image), dtype=dtype).requires_grad_(True)
    y = torch.tensor(np.asarray(target), dtype=dtype)
    loss, l1, ssim = loss_values(x, y, lam, conv_fn)
    (grad,) = torch.autograd.grad(loss, x)
    with torch.no_grad():
        saved = saved_partials(x, y, conv_fn)
    return dict(loss=float(loss.detach()), l1=float(l1.detach()), ssim=float(ssim.detach()),
                dL_dimage=grad.numpy(),
                saved=saved.numpy())


# ---- the test images: (image, target) pairs of float32 [C, H, W] -------------------------------

def _smooth(rng, C, H, W):
    yy, xx = np.meshgrid(np.arange(H) / max(H - 1, 1), np.arange(W) / max(W - 1, 1), indexing="ij")
    ph = rng.uniform(0.0, 2.0 * np.pi, size=(C, 2))
    return np.stack([0.5 + 0.35 * np.sin(2.0 * np.pi * xx + ph[c, 0]) *
                     np.cos(1.5 * np.pi * yy + ph[c, 1]) for c in range(C)])


def loss_images() -> dict:
    """name -> (image, target): the shapes and contents the GPU tests run (test_gpu_image_loss.py)
    and the float32 spread is measured on.  `random` has a few elements equal to the target's."""
    rng = np.random.default_rng(20240611)
    f32 = np.float32
    u = lambda *s: rng.uniform(0.0, 1.0, size=s).astype(f32)
    out = {"one": (u(1, 1, 1), u(1, 1, 1)), "small": (u(1, 7, 9), u(1, 7, 9))}
    img, tgt = u(3, 37, 53), u(3, 37, 53)
    for c, r, col in ((0, 0, 0), (1, 17, 30), (2, 36, 52), (2, 5, 5)):
        img[c, r, col] = tgt[c, r, col]
    out["random"] = (img, tgt)
    tgt = _smooth(rng, 3, 37, 53).astype(f32)
    out["smooth"] = (np.clip(tgt + 0.02 * rng.standard_normal(tgt.shape), 0, 1).astype(f32), tgt)
    out["dark"] = ((0.02 * u(4, 16, 200)).astype(f32), (0.02 * u(4, 16, 200)).astype(f32))
    tgt = (0.6 * _smooth(rng, 3, 64, 80) + 0.4 * u(3, 64, 80)).astype(f32)
    out["near"] = ((tgt + rng.uniform(-1e-3, 1e-3, size=tgt.shape)).astype(f32), tgt)
    for h in (TILE_H - 1, TILE_H, TILE_H + 1):
        for w in (TILE_W - 1, TILE_W, TILE_W + 1):
            out[f"tile_{h}x{w}"] = (u(2, h, w), u(2, h, w))
    return out


# ---- the tolerance of the GPU tests: measured, not chosen --------------------------------------
# f: the reference's own float32 spread per output -- rel_err (grad_reference.py) of `evaluate` in
# float32 against float64, the largest over loss_images(), per lambda for the two outputs that
# depend on it.  test_loss_reference.py re-measures them and holds these constants to within a
# factor 2 of what it finds; the GPU tests allow BOUND_FACTOR x f.  (lambda = 1 on `near` leaves
# loss = 1 - ssim ~ 1e-3 of a float32 mean near 1, hence its larger spread.)
BOUND_FACTOR = 8.0
F32_SPREAD = {
    "l1": 9.1e-8, "ssim": 3.5e-7, "dm_dmu1": 6.3e-2, "dm_ds1": 4.5e-4, "dm_ds12": 2.9e-4,
    "loss": {0.0: 9.1e-8, 0.2: 4.0e-5, 1.0: 7.5e-3},
    "dL_dimage": {0.0: 5.8e-8, 0.2: 4.4e-5, 1.0: 1.0e-3},
}
SAVED_NAMES = ("dm_dmu1", "dm_ds1", "dm_ds12")


def measure_spread(images=None) -> dict:
    """F32_SPREAD as measured now."""
    images = images or loss_images()
    f = {k: 0.0 for k in ("l1", "ssim") + SAVED_NAMES}
    f["loss"] = {lam: 0.0 for lam in LAMBDAS}
    f["dL_dimage"] = {lam: 0.0 for lam in LAMBDAS}
    for image, target in images.values():
        for lam in LAMBDAS:
            ref, got = evaluate(image, target, lam), evaluate(image, target, lam, torch.float32)
            for k in ("loss", "dL_dimage"):
                f[k][lam] = max(f[k][lam], rel_err(got[k], ref[k]))
            if lam == LAMBDAS[0]:
                for k in ("l1", "ssim"):
                    f[k] = max(f[k], rel_err(got[k], ref[k]))
                for i, k in enumerate(SAVED_NAMES):
                    f[k] = max(f[k], rel_err(got["saved"][i], ref["saved"][i]))
    return f


_REFERENCES: dict = {}


def reference(name: str, lam: float) -> dict:
    """`evaluate` in float64 of a loss_images() pair, computed once and shared (read-only)."""
    key = (name, float(lam))
    if key not in _REFERENCES:
        if "images" not in _REFERENCES:
            _REFERENCES["images"] = loss_images()
        _REFERENCES[key] = evaluate(*_REFERENCES["images"][name], lam)
    return _REFERENCES[key]


# ---- the seam tests (test_gpu_image_loss_seams.py): well-conditioned images, exact properties ---
# Uniform random [0, 1] pairs: no cancellation in 1 - ssim or in the partials, so the float32
# spread is near the format's own precision and a wrong tap, halo column or corner pixel shows.

SEAM_SHAPES = ((3, 33, 129),    # the smallest shape with a tile that is interior in both directions
               (2, 48, 192),    # 3 x 3 tiles: the locality pair
               (5, 100, 1000),  # 560 blocks, ragged last row (4 rows) and column (40) of tiles
               (1, 1, 130), (1, 70, 1),             # one pixel thick
               (2, 5, 5), (1, 11, 11), (1, 12, 12))  # at and around the window's width
SEAM_LAMBDAS = (0.2, 1.0)
LOCALITY_SHAPE = (2, 48, 192)
LOCALITY_PIXELS = ((0, 0), (47, 191), (15, 63), (16, 64), (16, 63), (24, 96))
TRANSLATION_SHAPE, CROP_H, CROP_W = (2, 64, 256), 32, 128
TRANSLATION_OFFSETS = ((0, 0), (1, 1), (15, 63), (16, 64), (17, 65), (7, 100), (32, 128))
# shape -> blocks (C x tiles_y x tiles_x): k_loss_finish's loop boundaries at 256 and 512 pairs
INTEGER_SHAPES = {(5, 100, 1000): 560, (1, 16, 16384): 256, (1, 16, 16385): 257,
                  (2, 16, 16384): 512, (3, 17, 65): 12}


def shape_name(shape) -> str:
    return "x".join(str(int(n)) for n in shape)


def blocks_of(shape) -> int:
    """The grid of both kernels: one block per 16 x 64 tile and channel."""
    C, H, W = shape
    return C * ((H + TILE_H - 1) // TILE_H) * ((W + TILE_W - 1) // TILE_W)


def random_pair(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.0, 1.0, size=shape).astype(np.float32),
            rng.uniform(0.0, 1.0, size=shape).astype(np.float32))


def seam_images() -> dict:
    """"CxHxW" -> (image, target), uniform random in [0, 1], one pair per SEAM_SHAPES."""
    return {shape_name(s): random_pair(s, 7100 + i) for i, s in enumerate(SEAM_SHAPES)}


def translation_pair():
    """The 4 x 4-tile pair whose 32 x 128 crops are compared with it."""
    return random_pair(TRANSLATION_SHAPE, 7200)


def crop(pair, dy, dx):
    return tuple(np.ascontiguousarray(a[:, dy:dy + CROP_H, dx:dx + CROP_W]) for a in pair)


def integer_images(shape):
    """(image, target) of float32 integers 0..8: every |x - y| and every partial sum of them is an
    integer below 2^24, so the kernels' float sums are exact whatever their order."""
    rng = np.random.default_rng(2)
    return (rng.integers(0, 9, size=shape).astype(np.float32),
            rng.integers(0, 9, size=shape).astype(np.float32))


def outside_window(H, W, r, c, radius) -> np.ndarray:
    """[H, W] bool: True where (r, c) is not within `radius` rows and columns."""
    rr, cc = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (np.abs(rr - r) > radius) | (np.abs(cc - c) > radius)


def pixel_err(got, ref) -> float:
    """max |got - ref| / (|ref| + median|ref|): every entry on its own scale, small ones on the
    tensor's typical scale (not on its maximum, as rel_err)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    a = np.abs(ref)
    return float((np.abs(got - ref) / (a + np.median(a))).max())


# Measured as F32_SPREAD is: `evaluate` in float32 against float64, the largest over seam_images()
# and over the 2-D and the separable form of the window (the kernels are separable); "max" is
# rel_err, "pixel" is pixel_err.  test_loss_reference.py holds the table within a factor 2 of a
# fresh measurement; the GPU tests allow BOUND_FACTOR x it.
SEAM_SPREAD = {
    "max": {"dm_dmu1": 9.7e-6, "dm_ds1": 1.3e-5, "dm_ds12": 4.4e-6,
            "dL_dimage": {0.2: 1.1e-6, 1.0: 1.5e-6}},
    "pixel": {"dm_dmu1": 8.8e-6, "dm_ds1": 5.6e-5, "dm_ds12": 3.8e-6,
              "dL_dimage": {0.2: 1.9e-6, 1.0: 3.3e-6}},
}
SEAM_ERRORS = {"max": rel_err, "pixel": pixel_err}


def seam_reference(name: str, lam: float) -> dict:
    """`evaluate` in float64 of a seam_images() pair, computed once and shared (read-only)."""
    key = ("seam", name, float(lam))
    if key not in _REFERENCES:
        if "seam_images" not in _REFERENCES:
            _REFERENCES["seam_images"] = seam_images()
        _REFERENCES[key] = evaluate(*_REFERENCES["seam_images"][name], lam)
    return _REFERENCES[key]


def measure_seam_spread(images=None, per_image=None) -> dict:
    """SEAM_SPREAD as measured now (`per_image`: a dict that receives each image's own table)."""
    shared = images is None  # the module's own images: their float64 references are cached
    images = images or seam_images()
    blank =lambda: {kind: {**{k: 0.0 for k in SAVED_NAMES},  # noqa: E731
                            "dL_dimage": {lam: 0.0 for lam in SEAM_LAMBDAS}}
                     for kind in SEAM_ERRORS}
    f = blank()
    for name, (image, target) in images.items():
        own = blank()
        for lam in SEAM_LAMBDAS:
            ref = seam_reference(name, lam) if shared else evaluate(image, target, lam)
            for conv_fn in (conv, conv_separable):
                got = evaluate(image, target, lam, torch.float32, conv_fn)
                for kind, err in SEAM_ERRORS.items():
                    own[kind]["dL_dimage"][lam] = max(own[kind]["dL_dimage"][lam],
                                                      err(got["dL_dimage"], ref["dL_dimage"]))
                    if lam == SEAM_LAMBDAS[0]:
                        for i, k in enumerate(SAVED_NAMES):
                            own[kind][k] = max(own[kind][k], err(got["saved"][i], ref["saved"][i]))
        for kind in SEAM_ERRORS:
            for k in SAVED_NAMES:
                f[kind][k] = max(f[kind][k], own[kind][k])
            for lam in SEAM_LAMBDAS:
                f[kind]["dL_dimage"][lam] = max(f[kind]["dL_dimage"][lam],
                                                own[kind]["dL_dimage"][lam])
        if per_image is not None:
            per_image[name] = own
    return f
