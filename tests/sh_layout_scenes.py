"""The scenes of the SH-layout tests (test_sh_layout_reference.py on the CPU, test_gpu_sh_layouts.py
on the GPU): one small geometry at every active degree, and every way a caller stores the rows.

The per-Gaussian kernels move a Gaussian's SH row as 12 float4 when M == 16 and the pointers are
16-byte aligned, and float by float otherwise (preprocess.hip color_from_sh,
backward_gaussian.inc).  The scenes here take both forms, at every degree, over the same numbers.

Geometry: that of grad_scenes "chain" -- P = 96, 40 x 24 px (3 x 2 tiles with a partial right
column and bottom row), scales and rotations, bg (0.3, 0.6, 0.1), scale_modifier 1.3, dL drawn as
grad_scenes draws it.  Four Gaussians (CULLED) sit at z <= 0.2 and are culled; the last one
(P - 1) is put in the middle of the frame, so the last row of every layout carries a gradient.

Base scenes deg0 .. deg3: M = 16 rows, active degree D = 0 .. 3, dc ~ N(-1.0, 1.8) and rest ~
N(0, 0.3) as grad_scenes "edges", so that a fifth to a third of the colour channels sit on the
clamp's flat side at every degree.  All 16 coefficients are drawn whatever D is: the ones above
the active degree must be ignored.  The seeds are chosen so that the float64 reference finds no
decision within rounding of its gate (test_sh_layout_reference.py asserts it).

Layout variants of a base scene (get(base, variant)); each holds the base's first (D + 1)^2
coefficients bit for bit:

  tight   M = (D + 1)^2: 1, 4, 9, 16
  mid     the next larger square below 16: D = 0 -> M = 4, D = 1 -> M = 9 (storage beyond the
          degree, but not 16)
  off4    M = 16, rows at a pointer 4 bytes past a 16-byte boundary (unaligned=True: the GPU test
          places them)
  wide    M = 25: nine more coefficients per Gaussian
  poison  M = 16 with every coefficient above the active degree NaN (D < 3)

BAND_SPREAD: the reference's own float32 spread of dL_dsh per SH band l = 0 .. D of each base
scene: max|g32 - g64| over the band's coefficients / max|g64| over the band, scene_gradients in
float32 with the float64 run's gates against float64 (as grad_reference.F32_SPREAD is measured).
Measured on the CPU; test_sh_layout_reference.py re-measures it and holds the table to within a
factor 2.  The GPU test allows grad_reference.BOUND_FACTOR x these.
"""
from __future__ import annotations

import numpy as np

from gaussiansplattingviewer_amd.camera import static_camera
from gaussiansplattingviewer_amd.gaussian_data import GaussianData
from gpu_helpers import scene_inputs
from grad_scenes import _gaussians

F32 = np.float32
P, W, H = 96, 40, 24
BASES = ("deg0", "deg1", "deg2", "deg3")
SEEDS = {"deg0": 14, "deg1": 14, "deg2": 14, "deg3": 14}  # one geometry, one set of numbers
CULLED = np.arange(40, 44)
WIDE_M = 25

#                    l = 0     l = 1     l = 2     l = 3
BAND_SPREAD = {
    "deg0": (3.6e-7,),
    "deg1": (3.6e-7, 3.4e-7),
    "deg2": (3.6e-7, 3.4e-7, 3.7e-7),
    "deg3": (3.6e-7, 3.4e-7, 3.7e-7, 4.1e-7),
}


def degree(base):
    return BASES.index(base)


def variants(base):
    """The layout variants of a base scene, by name."""
    D = degree(base)
    return ("tight",) + (("mid",) if D < 2 else ()) + ("off4", "wide") + (("poison",) if D < 3 else ())


def band(l):
    """The coefficient columns of SH band l."""
    return slice(l * l, (l + 1) * (l + 1))


def _base(name):
    rng = np.random.default_rng(SEEDS[name])
    D = degree(name)
    g = _gaussians(rng, P, 2.2, 1.4, 0.05, 0.35, 0.1, 0.9, dc=(-1.0, 1.8), rest=0.3)
    # z <= 0.2: at and behind the camera plane (the eye is at z = 4, looking down -z)
    g.xyz[CULLED, 2] = (3.81, 3.9, 4.0, 5.0)
    # the last Gaussian: mid-frame, in front of most, so that its gradients are not 0
    g.xyz[P - 1] = (0.1, -0.05, 0.6)
    g.opacity[P - 1] = 0.6
    g.scale[P - 1] = (0.2, 0.15, 0.25)
    s = scene_inputs(g, static_camera(W, H), D, bg=(0.3, 0.6, 0.1), scale_modifier=1.3)
    dL = np.ascontiguousarray(rng.standard_normal((3, H, W)), F32)
    extra = np.ascontiguousarray(rng.normal(0, 0.3, (P, 3 * (WIDE_M - 16))), F32)  # wide's columns
    return dict(name=name, base=name, variant="base", s=s, colors=None, cov6=None, W=W, H=H, dL=dL,
                D=D, M=16, unaligned=False, special={"culled": CULLED}, _extra=extra)


def _variant(base, variant):
    b = get(base)
    D, g = b["D"], b["s"]["g"]
    n = (D + 1) ** 2
    sh16 = g.sh
    unaligned = False
    if variant == "tight":
        M, sh = n, sh16[:, :3 * n]
    elif variant == "mid" and D < 2:
        M = (D + 2) ** 2
        sh = sh16[:, :3 * M]
    elif variant == "off4":
        M, sh, unaligned = 16, sh16, True
    elif variant == "wide":
        M, sh = WIDE_M, np.concatenate([sh16, b["_extra"]], 1)
    elif variant == "poison" and D < 3:
        M, sh = 16, sh16.copy()
        sh[:, 3 * n:] = np.nan
    else:
        raise KeyError((base, variant))
    g2 = GaussianData(g.xyz, g.rot, g.scale, g.opacity, np.ascontiguousarray(sh, F32))
    s = dict(b["s"], g=g2)
    return dict(b, name=f"{base}/{variant}", variant=variant, s=s, M=M, unaligned=unaligned)


def dL_masks():
    """The frame's pixels split into 8 parts, (H, W) arrays of 0.0 / 1.0 that add up to 1: the 15
    8 x 8 quadrants of the 16 x 16 tiles (5 across, 3 down), two to a part.

    Why: the backward's blend kernel adds each wave's sums -- one wave per quadrant -- to a
    Gaussian's row of 2D gradients with float atomics, in the order the waves arrive, so with a
    gradient on every pixel two calls on the same inputs differ in the last bits of many rows
    (include/gsr.h says so of gsr_backward).  With the image gradient (and the planes') confined
    to one part, a row gets at most two non-zero addends -- every other wave adds an exact 0 --
    and a + b == b + a: the rows, and with them everything the per-Gaussian kernel derives from
    them, are reproducible bit for bit, which is what the layout comparisons need.  The parts
    together hand every pixel's gradient to the kernels once."""
    parts = []
    quads = [(qy, qx) for qy in range((H + 7) // 8) for qx in range((W + 7) // 8)]
    for i in range(0, len(quads), 2):
        m = np.zeros((H, W), F32)
        for qy, qx in quads[i:i + 2]:
            m[8 * qy:8 * qy + 8, 8 * qx:8 * qx + 8] = 1.0
        parts.append(m)
    return parts


_cache = {}


def get(base, variant="base"):
    key = (base, variant)
    if key not in _cache:
        _cache[key] = _base(base) if variant == "base" else _variant(base, variant)
    return _cache[key]
