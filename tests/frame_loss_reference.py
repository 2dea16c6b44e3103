"""The frame's loss on a window of its rows (gsr_image_loss_window, include/gsr.h)
restated in float64 on top of loss_reference: what ONE rank computes from ITS band alone -- its
own rows and `halo` rendered rows of each neighbour -- with zero padding wherever the band ends.

At a frame edge that padding is the definition's.  At a seam it is wrong, but only within 5 rows
of the band's end for the map and its partials, and within 5 more for the gradient: with
halo = 10 nothing an own row reads is touched, with 9 (or 5) the partials at the apron's outer
row are, and the gradient of the first and last own rows with them.  test_frame_loss_reference.py
holds the construction to the frame's own values and keeps the two short halos as mutants.
"""
from __future__ import annotations

import numpy as np
import torch

import loss_reference as L

HALO_ROWS, APRON_ROWS = 10, 5


def band_of(own, H, halo=HALO_ROWS):
    """The frame rows [lo, hi) a rank holds: its own rows and `halo` more, inside the frame."""
    return max(0, own[0] - halo), min(H, own[1] + halo)


def apron_of(own, H):
    return band_of(own, H, APRON_ROWS)


def partition(H, cuts):
    """Own ranges [(0, c1), (c1, c2), ..., (ck, H)] of a frame."""
    edges = [0, *cuts, H]
    return [(edges[i], edges[i + 1]) for i in range(len(edges) - 1)]


def rank_outputs(image, target, own, lam, gl=1.0, halo=HALO_ROWS) -> dict:
    """What a rank forms from its band of two float64 [C, H, W] tensors: the shares l1, ssim and
    loss of the own rows, the saved partials on the apron and the gradient on the own rows.  Only
    rows [lo, hi) of `image` and `target` are read; H enters through N alone."""
    C, H, W = image.shape
    N = C * H * W
    lo, hi = band_of(own, H, halo)
    x, y = image[:, lo:hi], target[:, lo:hi]
    o0, o1 = own[0] - lo, own[1] - lo
    _, _, A, B, Cc, D = L.statistics(x, y)
    smap = Cc * D / (A * B)
    l1 = (x - y).abs()[:, o0:o1].sum() / N
    ssim = smap[:, o0:o1].sum() / N
    n_own = C * (own[1] - own[0]) * W
    loss = (1.0 - lam) * l1 + lam * (n_own / N - ssim)
    s = L.saved_partials(x, y)
    gm = -gl * lam / N
    grad = (L.conv(gm * s[0]) + 2.0 * x * L.conv(gm * s[1]) + y * L.conv(gm * s[2])
            + gl * (1.0 - lam) / N * torch.sign(x - y))
    a0, a1 = apron_of(own, H)
    return dict(loss=float(loss), l1=float(l1), ssim=float(ssim),
                saved=s[:, :, a0 - lo:a1 - lo].numpy(), dL_dimage=grad[:, o0:o1].numpy())


def frame_outputs(image, target, lam, gl=1.0) -> dict:
    """The whole frame's values and `manual_gradient`, float64."""
    loss, l1, ssim = L.loss_values(image, target, lam)
    return dict(loss=float(loss), l1=float(l1), ssim=float(ssim),
                saved=L.saved_partials(image, target).numpy(),
                dL_dimage=L.manual_gradient(image, target, lam, gl).numpy())


def as_f64(pair):
    return tuple(torch.tensor(np.asarray(a), dtype=torch.float64) for a in pair)


# ---- the GPU tests' windows (test_gpu_frame_loss_strips.py) -------------------------------------
# shape -> [(row0, band rows, own)]: the band buffer's first frame row and rows, and the own rows.
# None for the band: exactly the rows the call needs (own +- 10, inside the frame).


def strip_windows(H, tile_rows):
    """Tile-row strips as windows with minimal bands."""
    out = []
    for tb, te in tile_rows:
        own = (min(H, 16 * tb), min(H, 16 * te))
        lo, hi = band_of(own, H)
        out.append((lo, hi - lo, own))
    return out


WINDOW_CASES = {
    # 16, 16 and 8 rows: the last strip shorter than the halo, the last column tile partial
    (3, 40, 70): strip_windows(40, ((0, 1), (1, 2), (2, 3))),
    # a frame smaller than the window, one strip
    (1, 11, 5): strip_windows(11, ((0, 1),)),
    # arbitrary pixel windows, bands from rows 0 and 13: the tile grid is off the frame's in rows
    (2, 48, 130): [(0, 33, (0, 7)), (0, 33, (7, 23)), (13, 35, (23, 48))],
    # windows of 1 row and of 32 rows
    (3, 33, 129): [(0, 11, (0, 1)), (0, 33, (1, 33))],
}
WINDOW_SEEDS = {shape: 7300 + i for i, shape in enumerate(WINDOW_CASES)}
GLS = (None, 0.75)

_CACHE: dict = {}


def window_pair(shape):
    """The float32 (image, target) of a WINDOW_CASES shape (loss_reference.random_pair)."""
    if ("pair", shape) not in _CACHE:
        _CACHE[("pair", shape)] = L.random_pair(shape, WINDOW_SEEDS[shape])
    return _CACHE[("pair", shape)]


def window_reference(shape, lam) -> dict:
    """`loss_reference.evaluate` in float64 of a shape's pair, computed once and shared."""
    key = ("ref", shape, float(lam))
    if key not in _CACHE:
        _CACHE[key] = L.evaluate(*window_pair(shape), lam)
    return _CACHE[key]


def share_sum_bound(ref_value, spread, roundings):
    """|sum of the shares - float64 reference| allowed: the whole-frame values' bound
    (BOUND_FACTOR x the measured float32 spread, relative) plus 2^-24 |value| for each of the
    `roundings` of the shares to float32."""
    return (L.BOUND_FACTOR * spread + roundings * 2.0 ** -24) * abs(ref_value)
