"""Drop-in replacement for the `diff_gaussian_rasterization` Python API the viewer imports.

renderer_cuda.py:13 does `from diff_gaussian_rasterization import GaussianRasterizationSettings,
GaussianRasterizer` and renderer_cuda.py:211-224 calls

    GaussianRasterizer(raster_settings=GaussianRasterizationSettings(**settings))(
        means3D=..., means2D=None, shs=..., colors_precomp=None, opacities=...,
        scales=..., rotations=..., cov3D_precomp=None)  ->  (color [3,H,W], radii [P])

The names, field order, argument checks and return values below follow that third-party API
(upstream `diff_gaussian_rasterization/__init__.py` and `_C.rasterize_gaussians` in
rasterize_points.cu); the work is done by libgsr.so (HIP, gfx950) through `_lib`.
The viewer renders under `torch.no_grad()` (renderer_cuda.py:214) and pays nothing for it, but the
image is differentiable: `_RasterizeGaussians.backward` returns the gradients of the splat
composite (`gsr_backward`, include/gsr.h), as upstream's does for training code.  With
`GaussianRasterizationSettings.depth_maps` the rasterizer also returns depth_map, inv_depth_map and
final_T, differentiable too (`_RasterizeGaussiansPlanes`, `gsr_backward_planes`).  When
`viewmatrix`, `projmatrix` or `campos` of the settings requires a gradient, the camera gets one as
well (`_RasterizeGaussiansCamera`, `gsr_backward_camera`).  `GaussianRasterizationSettings(...,
antialiasing=True)` (upstream's keyword) switches all three Functions to the compensated opacity
(`gsr_forward_filtered` / `gsr_backward_filtered`).  `GaussianRasterizationSettings(...,
deterministic=True)`, or `torch.use_deterministic_algorithms(True)` with the setting left at None,
makes every backward bit-reproducible (`gsr_backward_ordered`).
`GaussianRasterizationSettings(..., tile_rows=(b, e))` renders and differentiates one strip of
16-px tile rows (`gsr_backward_strip`): the image-like outputs are strip-local, the gradients
whole-scene, and over a partition of the rows they add up to the whole frame's
(`strips.reduce_gradients` sums them over the ranks).
`GaussianRasterizer(...)(..., means2D_abs=leaf)` also leaves the absolute gradient of the 2D means
in `leaf.grad` (`_RasterizeGaussiansAbs`, `gsr_backward_abs`): means2D's gradient with every
pixel's term taken by its absolute value, the number AbsGS-style densification thresholds.
"""
from __future__ import annotations

import ctypes
from typing import NamedTuple

import torch

from . import _lib


class _SettingsTuple(NamedTuple):
    image_height: int
    image_width: int
    tanfovx: float
    tanfovy: float
    bg: torch.Tensor
    scale_modifier: float
    viewmatrix: torch.Tensor
    projmatrix: torch.Tensor
    sh_degree: int
    campos: torch.Tensor
    prefiltered: bool
    debug: bool
    # not upstream's: one of _lib.GSR_SHADE_* (the GL backend's billboard / ball shadings,
    # include/gsr.h gsr_forward_shaded); last and defaulted, so upstream's constructions hold
    shading: int = 0


def _tile_rows(tile_rows):
    """None, or (begin, end) as a tuple of two ints."""
    if tile_rows is None:
        return None
    b, e = tile_rows
    return int(b), int(e)


def _strip_rows(tile_rows, H):
    """(begin, end, y0, rows) of a strip of a frame H pixels high; RuntimeError outside the grid."""
    gy = (H + 15) // 16
    rb, re = int(tile_rows[0]), int(tile_rows[1])
    if not (0 <= rb < re <= gy):
        raise RuntimeError(f"tile_rows {tuple(tile_rows)} outside [0, {gy}]")
    return rb, re, rb * 16, min(H, re * 16) - rb * 16


class GaussianRasterizationSettings(_SettingsTuple):
    """upstream's settings tuple (its 12 fields, then `shading`) and one more setting beside it:
    depth_maps (not upstream's; the last argument, after shading, default False).  With it
    GaussianRasterizer returns (color, radii, depth_map, inv_depth_map, final_T), the three (H, W)
    planes of gsr_forward_depth / gsr_outputs, differentiable like the image
    (gsr_backward_planes); the splat composite only.  It is an attribute of the instance, not an
    element of the tuple: `_fields`, `_field_defaults`, unpacking and comparison stay those of the
    13-field tuple that callers and tests of the shading rely on; `_replace` carries it.

    antialiasing (upstream's name; keyword only here, default False, an attribute like
    depth_maps): the Mip-Splatting compensation of the 0.3-pixel dilation -- every Gaussian is
    drawn with opacity * sqrt(max(0.000025, det(cov2D) / det(cov2D + 0.3 I))), forward and
    backward (gsr_forward_filtered / gsr_backward_filtered in include/gsr.h).  The splat composite
    only: RuntimeError with a shading.  Upstream's positional place for it is `shading` here.

    deterministic (not upstream's; keyword only, default None, an attribute like antialiasing): the
    backward whose gradients, the camera's included, have the same bits on every call with the
    same inputs (gsr_backward_ordered in include/gsr.h: no float atomics; it costs workspace, 144
    to 160 B per (Gaussian, tile) pair).  True and False force the mode; None follows
    torch.are_deterministic_algorithms_enabled() when the backward runs.  The forward is
    reproducible either way.

    tile_rows (not upstream's; keyword only, default None, an attribute like antialiasing): (b, e),
    the 16-px tile rows [b, e) of the frame to render and to differentiate (gsr_backward_strip in
    include/gsr.h).  image_height and image_width stay the frame's.  GaussianRasterizer then returns
    the strip-local colour (3, rows, W), rows = min(H, 16 e) - 16 b, and with depth_maps the
    strip-local planes (rows, W); radii stays (P,).  backward() gives the whole-scene gradients of
    the strip's loss -- the whole frame's backward with the image gradients zero outside the strip
    -- through all three Functions (planes, camera, antialiasing, deterministic).  The splat
    composite only, like every backward."""
    depth_maps = False  # (instances made by _make)
    antialiasing = False
    deterministic = None
    tile_rows = None

    def __new__(cls, *args, depth_maps=False, **kwargs):
        # (antialiasing and deterministic travel in kwargs: the parameter list ends at depth_maps,
        # as tests/test_plane_grad_reference.py pins it)
        antialiasing = kwargs.pop("antialiasing", False)
        deterministic = kwargs.pop("deterministic", None)
        tile_rows = kwargs.pop("tile_rows", None)
        if len(args) == len(cls._fields) + 1:  # given by position, after shading
            *args, depth_maps = args
        self = super().__new__(cls, *args, **kwargs)
        self.depth_maps = bool(depth_maps)
        self.antialiasing = bool(antialiasing)
        self.deterministic = None if deterministic is None else bool(deterministic)
        self.tile_rows = _tile_rows(tile_rows)
        return self

    def _replace(self, **kwargs):
        depth_maps = kwargs.pop("depth_maps", self.depth_maps)
        antialiasing = kwargs.pop("antialiasing", self.antialiasing)
        deterministic = kwargs.pop("deterministic", self.deterministic)
        tile_rows = kwargs.pop("tile_rows", self.tile_rows)
        new = super()._replace(**kwargs)
        new.depth_maps = bool(depth_maps)
        new.antialiasing = bool(antialiasing)
        new.deterministic = None if deterministic is None else bool(deterministic)
        new.tile_rows = _tile_rows(tile_rows)
        return new


def _device_of(t: torch.Tensor) -> torch.device:
    if not t.is_cuda:
        raise RuntimeError("means3D must be a device (HIP) tensor")
    return t.device


def _as_dev(t, device, shape_hint: str):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.numel() == 0:
        return None
    if t.device != device:
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous()


def _scene_structs(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier,
                   cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, H, W, sh, degree,
                   campos, prefiltered, debug):
    """The inputs both directions share, as the library takes them: (device, device index, P,
    gsr_gaussians, gsr_raster_settings of a whole frame, the device tensors the two point into:
    hold them while the structs are in use)."""
    device = _device_of(means3D)
    dev_index = device.index if device.index is not None else torch.cuda.current_device()
    P = int(means3D.size(0))
    means3D = _as_dev(means3D, device, "P,3")
    opacities = _as_dev(opacities, device, "P,1")
    scales = _as_dev(scales, device, "P,3")
    rotations = _as_dev(rotations, device, "P,4")
    cov3D_precomp = _as_dev(cov3D_precomp, device, "P,6")
    colors_precomp = _as_dev(colors_precomp, device, "P,3")
    sh = _as_dev(sh, device, "P,M,3")
    bg = _as_dev(bg, device, "3")
    viewmatrix = _as_dev(viewmatrix, device, "4,4")
    projmatrix = _as_dev(projmatrix, device, "4,4")
    campos = _as_dev(campos, device, "3")
    M = 0
    if sh is not None:
        M = int(sh.size(1)) if sh.ndimension() == 3 else int(sh.numel() // max(P, 1) // 3)
    g = _lib.GsrGaussians(P=P, D=int(degree), M=M, scale_modifier=float(scale_modifier),
                          means3D=_lib.ptr(means3D), scales=_lib.ptr(scales),
                          rotations=_lib.ptr(rotations), opacities=_lib.ptr(opacities),
                          shs=_lib.ptr(sh), colors_precomp=_lib.ptr(colors_precomp),
                          cov3D_precomp=_lib.ptr(cov3D_precomp))
    st = _lib.GsrRasterSettings(image_width=W, image_height=H, tanfovx=float(tanfovx),
                                tanfovy=float(tanfovy), viewmatrix=_lib.ptr(viewmatrix),
                                projmatrix=_lib.ptr(projmatrix), campos=_lib.ptr(campos),
                                bg=_lib.ptr(bg), tile_row_begin=0, tile_row_end=0,
                                prefiltered=int(bool(prefiltered)), debug=int(bool(debug)))
    return device, dev_index, P, g, st, (means3D, opacities, scales, rotations, cov3D_precomp,
                                         colors_precomp, sh, bg, viewmatrix, projmatrix, campos)


def _feature_rows(features, P, device):
    """`features` as the library reads it: float32 (P, C) on `device` with contiguous rows of C --
    the tensor itself when it already is (a view at an odd offset included), else a copy.
    RuntimeError for another shape or a C outside 1..256."""
    if not isinstance(features, torch.Tensor) or features.ndimension() != 2 or \
            int(features.size(0)) != P:
        raise RuntimeError(f"features must have dimensions (num_points, C) = ({P}, C)")
    C = int(features.size(1))
    if not 1 <= C <= _lib.MAX_FEATURES:
        raise RuntimeError(f"features: C = {C} outside 1..{_lib.MAX_FEATURES}")
    if features.device != device:
        features = features.to(device)
    if features.dtype != torch.float32:
        features = features.float()
    return features.detach().contiguous()


class ForwardResult(NamedTuple):
    """Everything one native forward produced (color/radii plus optional intermediates)."""
    num_rendered: int
    color: torch.Tensor
    radii: torch.Tensor
    extras: dict
    feature_map: torch.Tensor | None = None  # (C, rows, W) with `features`, else None


def rasterize_gaussians_native(bg, means3D, colors_precomp, opacities, scales, rotations,
                               scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tanfovx,
                               tanfovy, image_height, image_width, sh, degree, campos, prefiltered,
                               debug, *, tile_rows=None, extras=(), stream=None, slot=0,
                               out_color=None, radii=True, shading=0,
                               antialiasing=False, features=None) -> ForwardResult:
    """Same arguments, order and validation as upstream `_C.rasterize_gaussians`.

    Extensions (keyword-only, for the strip partition and the parity tests):
      tile_rows -- (begin, end) 16-px tile rows to render; the image is then strip-local;
      extras    -- names of intermediates to return: depths, means2D, conic_opacity, rgb,
                   tiles_touched, final_T, n_contrib; and the per-pixel planes depth_map,
                   inv_depth_map, (rows, W) float32: the sums of z and 1 / z under the colour's
                   weights, premultiplied (gsr_forward_depth in include/gsr.h; `depths` stays the
                   per-Gaussian view-space z).  Splat composite only: RuntimeError with a shading;
                   and the median planes median_depth (rows, W) float32 and median_id (rows, W)
                   int32: the view-space z and the global Gaussian id of the splat at which the
                   pixel's transmittance crosses 0.5, 0.0 / -1 where it never does
                   (gsr_forward_surface; any combination with the other extras).  Splat composite
                   only, like the depth planes;
      stream    -- HIP stream handle (default: torch's current stream);
      slot      -- context slot (`_lib.context`): forwards in different slots may overlap;
      out_color -- preallocated contiguous f32 (3, rows, W) output (e.g. a gather buffer);
      radii     -- False (strips only, no per-Gaussian extras): no radii output
                   (ForwardResult.radii is None); Gaussians whose footprint bound misses the
                   strip skip the per-Gaussian work (a multi-GPU strip rank needs its image only);
      shading   -- _lib.GSR_SHADE_*: 0 the splat composite, 1 billboard, 2 flat ball, 3 gaussian
                   ball (the GL backend's shadings, gsr_forward_shaded in include/gsr.h);
      antialiasing -- True: the effective opacity of the 0.3-pixel dilation's compensation in
                   place of the opacity (gsr_forward_filtered in include/gsr.h; the extra
                   conic_opacity[:, 3] is then that opacity).  Splat composite only: RuntimeError
                   with a shading.  False is the call without the argument.
      features  -- (P, C) float32, 1 <= C <= 256: C channels of the caller's own per Gaussian.
                   ForwardResult.feature_map is then (C, rows, W): each plane the sum of the
                   channel under the colour's weights, no background term (gsr_forward_features in
                   include/gsr.h: bit for bit a colour channel of a colors_precomp forward with
                   bg = 0).  A view whose rows are contiguous and whose storage is a (P, C) block
                   is read in place, whatever its alignment.  Splat composite only: RuntimeError
                   with a shading.  None is the call without the argument.
    """
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if features is not None:
        if shading != _lib.GSR_SHADE_SPLAT:
            raise RuntimeError("features are composited by the splat composite: not available "
                               f"with shading {shading}")
        features = _feature_rows(features, int(means3D.size(0)), means3D.device)
    if not radii and (tile_rows is None or any(
            n in extras for n in ("depths", "means2D", "conic_opacity", "rgb", "tiles_touched"))):
        raise RuntimeError("radii=False needs tile_rows and no per-Gaussian extras")
    depth_planes = [n for n in ("depth_map", "inv_depth_map") if n in extras]
    if depth_planes and shading != _lib.GSR_SHADE_SPLAT:
        raise RuntimeError("depth_map / inv_depth_map come from the splat composite: not "
                           f"available with shading {shading}")
    surface_planes = [n for n in ("median_depth", "median_id") if n in extras] if extras else ()
    if surface_planes and shading != _lib.GSR_SHADE_SPLAT:
        raise RuntimeError("median_depth / median_id come from the splat composite: not "
                           f"available with shading {shading}")
    if antialiasing and shading != _lib.GSR_SHADE_SPLAT:
        raise RuntimeError("antialiasing belongs to the splat composite: not available with "
                           f"shading {shading}")
    H, W = int(image_height), int(image_width)
    device, dev_index, P, g, st, held = _scene_structs(
        bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp,
        viewmatrix, projmatrix, tanfovx, tanfovy, H, W, sh, degree, campos, prefiltered, debug)

    if tile_rows is None:
        rb, re = 0, 0
        y0, rows = 0, H
    else:
        rb, re, y0, rows = _strip_rows(tile_rows, H)

    f32 = dict(dtype=torch.float32, device=device)
    if out_color is None:
        color = torch.empty((3, rows, W), **f32)
    else:
        if (out_color.dtype != torch.float32 or not out_color.is_contiguous() or
                tuple(out_color.shape) != (3, rows, W) or out_color.device != device):
            raise RuntimeError(f"out_color must be a contiguous float32 (3, {rows}, {W}) tensor "
                               f"on {device}")
        color = out_color
    radii = torch.empty((P,), dtype=torch.int32, device=device) if radii else None
    ext = {}
    for name in extras:
        if name == "depths":
            ext[name] = torch.zeros((P,), **f32)
        elif name == "means2D":
            ext[name] = torch.zeros((P, 2), **f32)
        elif name == "conic_opacity":
            ext[name] = torch.zeros((P, 4), **f32)
        elif name == "rgb":
            ext[name] = torch.zeros((P, 3), **f32)
        elif name == "tiles_touched":
            ext[name] = torch.zeros((P,), dtype=torch.int32, device=device)
        elif name in ("final_T", "depth_map", "inv_depth_map", "median_depth"):
            ext[name] = torch.zeros((rows, W), **f32)
        elif name == "median_id":
            ext[name] = torch.full((rows, W), -1, dtype=torch.int32, device=device)
        elif name == "n_contrib":
            ext[name] = torch.zeros((rows, W), dtype=torch.int32, device=device)
        else:
            raise ValueError(f"unknown extra output {name!r}")

    feature_map = None
    if features is not None:
        feature_map = torch.zeros((features.size(1), rows, W), **f32)
    st.tile_row_begin, st.tile_row_end = rb, re
    out = _lib.GsrOutputs(color=color.data_ptr(),
                          radii=radii.data_ptr() if P and radii is not None else None)
    for name, t in ext.items():
        if name not in depth_planes and name not in surface_planes:
            setattr(out, name, t.data_ptr())
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    lib = _lib.load_library()
    ctx = _lib.context(dev_index, slot)
    head = (ctx, ctypes.byref(g), ctypes.byref(st), ctypes.byref(out))
    # the optional structs, NULL for each the call does without
    structs = _refs(
        depth_planes and _lib.GsrDepthOutputs(**{n: ext[n].data_ptr() for n in depth_planes}),
        surface_planes and _lib.GsrSurfaceOutputs(**{n: ext[n].data_ptr()
                                                     for n in surface_planes}),
        antialiasing and _lib.GsrFilterSettings(antialiasing=int(antialiasing)),
        features is not None and _lib.GsrFeatureOutputs(
            C=int(features.size(1)), features=_lib.ptr(features),
            feature_map=feature_map.data_ptr()))
    with torch.cuda.device(dev_index):
        if shading != _lib.GSR_SHADE_SPLAT:
            _lib.check(lib.gsr_forward_shaded(*head, int(shading), ctypes.c_void_p(stream)),
                       "gsr_forward_shaded")
        else:
            name, fn, n = _lowest_entry(_FORWARD_ENTRIES, lib, structs)
            _lib.check(fn(*head, *structs[:n], ctypes.c_void_p(stream)), name)
    return ForwardResult(int(out.num_rendered), color, radii, ext, feature_map)


def _refs(*structs):
    """ctypes.byref of each struct; None for anything else (a struct the call does without)."""
    return tuple(ctypes.byref(s) if isinstance(s, ctypes.Structure) else None for s in structs)


# The entries the ctypes path calls, lowest first: (name, its accessor, how many of the top entry's
# optional structs it takes, whether a backward honours a tile row strip).  The lowest entry that
# can express a request is called, so an older build of ABI 4 loaded through GSR_LIB serves every
# request it has an entry for.
_FORWARD_ENTRIES = (
    ("gsr_forward", lambda lib: lib.gsr_forward, 0, True),
    ("gsr_forward_filtered", lambda lib: _lib.filtered_fns(lib)[0], 3, True),
    ("gsr_forward_features", lambda lib: _lib.features_fns(lib)[0], 4, True))
_BACKWARD_ENTRIES = (
    ("gsr_backward", _lib.backward_fn, 0, False),
    ("gsr_backward_filtered", lambda lib: _lib.filtered_fns(lib)[1], 3, False),
    ("gsr_backward_ordered", _lib.backward_ordered_fn, 4, False),
    ("gsr_backward_strip", _lib.backward_strip_fn, 4, True),
    ("gsr_backward_features", lambda lib: _lib.features_fns(lib)[1], 5, True),
    ("gsr_backward_abs", _lib.backward_abs_fn, 6, True))


def _lowest_entry(entries, lib, structs, strip=False):
    """(name, function, number of optional structs it takes) of the lowest of `entries` that takes
    the last struct of `structs` that is not None, and a strip if there is one."""
    used = max((i + 1 for i, s in enumerate(structs) if s is not None), default=0)
    return next((name, accessor(lib), n) for name, accessor, n, strips in entries
                if n >= used and (strips or not strip))


def rasterize_gaussians_backward_native(bg, means3D, colors_precomp, opacities, scales, rotations,
                                        scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                        tanfovx, tanfovy, dL_dout_color, sh, degree, campos,
                                        debug=False, *, conic=False, stream=None, slot=0,
                                        dL_ddepth_map=None, dL_dinv_depth_map=None,
                                        dL_dfinal_T=None, depths=False, camera=False,
                                        antialiasing=False, deterministic=False,
                                        tile_rows=None, image_height=None, features=None,
                                        dL_dfeature_map=None, absgrad=False) -> dict:
    """`gsr_backward` over ctypes (the GSR_LIB A/B path and the tests): the forward's inputs in
    `rasterize_gaussians_native`'s order with dL_dout_color (3, H, W) in place of the image size.
    Returns a dict of the gradients by their gsr_gradients names: dL_dmeans3D, dL_dmeans2D (P, 3:
    upstream's units, z = 0), dL_dopacity (P, 1), dL_dcolors, dL_dcov3D, dL_dsh (with SHs),
    dL_dscales and dL_drotations (with scales and rotations); conic=True adds dL_dconic (P, 3).

    With anything below the call is `gsr_backward_filtered`, with NULL for what is not asked for
    (which makes it `gsr_backward_planes` or `gsr_backward_camera`, include/gsr.h).

    dL_ddepth_map, dL_dinv_depth_map or dL_dfinal_T ((H, W) each, None = unused), or depths=True:
    the planes' gradients join the image's (dL_dout_color may then be None; H, W come from the
    first plane given), and depths=True adds dL_ddepths (P,), dL/dz through the features z and
    1 / z only.

    camera=True adds dL_dviewmatrix (4, 4), dL_dprojmatrix (4, 4), both in the inputs'
    (column-major) layout, and dL_dcampos (3,).

    antialiasing=True: the backward of the forward with the same argument, with whatever of the
    planes and the camera is asked for.

    deterministic=True: the call is `gsr_backward_ordered` in its deterministic mode -- the same
    gradients up to the rounding of the sums over pixels, with the same bits on every call.

    tile_rows=(b, e), with image_height (required then: the strip does not tell the frame's
    height): the call is `gsr_backward_strip` -- the backward of the strip's loss.  dL_dout_color is
    strip-local, (3, rows, W) with rows = min(H, 16 e) - 16 b, the plane gradients (rows, W); the
    gradients are whole-scene, exact zeros for Gaussians without a tile in the strip.

    features (P, C) with dL_dfeature_map (C, rows, W): the call is `gsr_backward_features` -- the
    feature planes' gradient joins the others (dL_dout_color may then be None) and the result also
    holds dL_dfeatures (P, C), exact zeros for culled Gaussians.  With deterministic=True the
    library refuses the call (RuntimeError): the deterministic slots have no room for C more sums.

    absgrad=True: the call is `gsr_backward_abs` and the result also holds dL_dmeans2D_abs (P, 3),
    dL_dmeans2D's sums over pixels with each pixel's term taken by its absolute value (AbsGS; exact
    zeros for culled Gaussians).  With a feature gradient the library refuses the call."""
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    if (features is None) != (dL_dfeature_map is None):
        raise RuntimeError("features and dL_dfeature_map belong together")
    if features is not None:
        features = _feature_rows(features, int(means3D.size(0)), means3D.device)
        if dL_dfeature_map.ndimension() != 3 or int(dL_dfeature_map.size(0)) != features.size(1):
            raise RuntimeError("dL_dfeature_map must have dimensions (C, H, W) = "
                               f"({features.size(1)}, H, W)")
    if tile_rows is not None and image_height is None:
        raise RuntimeError("tile_rows needs image_height: the frame's height, not the strip's")
    if tile_rows is None and image_height is not None:
        raise RuntimeError("image_height belongs to tile_rows: a whole frame's comes from "
                           "dL_dout_color")
    plane_grads = {"dL_ddepth_map": dL_ddepth_map, "dL_dinv_depth_map": dL_dinv_depth_map,
                   "dL_dfinal_T": dL_dfinal_T}
    plane_grads = {n: t for n, t in plane_grads.items() if t is not None}
    if dL_dout_color is None and not plane_grads and features is None:
        raise RuntimeError("dL_dout_color or a plane gradient is required")
    if dL_dout_color is not None and (dL_dout_color.ndimension() != 3 or
                                      dL_dout_color.size(0) != 3):
        raise RuntimeError("dL_dout_color must have dimensions (3, H, W)")
    if dL_dout_color is not None:
        H, W = int(dL_dout_color.size(1)), int(dL_dout_color.size(2))
    else:
        first = next(iter(plane_grads.values())) if plane_grads else dL_dfeature_map
        H, W = int(first.size(-2)), int(first.size(-1))
    rb = re = 0
    if tile_rows is not None:  # H so far: the strip's rows
        rb, re, _, rows = _strip_rows(tile_rows, int(image_height))
        if H != rows:
            raise RuntimeError(f"tile_rows {tuple(tile_rows)} of a frame {int(image_height)} px "
                               f"high: the image and plane gradients must have {rows} rows, got {H}")
        H = int(image_height)
    else:
        rows = H
    for n, t in plane_grads.items():
        if t.ndimension() != 2 or tuple(t.shape) != (rows, W):
            raise RuntimeError(f"{n} must have dimensions (H, W) = ({rows}, {W})")
    if features is not None and tuple(dL_dfeature_map.shape[1:]) != (rows, W):
        raise RuntimeError(f"dL_dfeature_map must have dimensions (C, H, W) = "
                           f"({features.size(1)}, {rows}, {W})")
    device, dev_index, P, g, st, held = _scene_structs(
        bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp,
        viewmatrix, projmatrix, tanfovx, tanfovy, H, W, sh, degree, campos, False, debug)
    st.tile_row_begin, st.tile_row_end = rb, re
    dL = _as_dev(dL_dout_color, device, "3,H,W")
    f32 = dict(dtype=torch.float32, device=device)
    grads = {"dL_dmeans3D": torch.zeros((P, 3), **f32), "dL_dmeans2D": torch.zeros((P, 3), **f32),
             "dL_dopacity": torch.zeros((P, 1), **f32), "dL_dcolors": torch.zeros((P, 3), **f32),
             "dL_dcov3D": torch.zeros((P, 6), **f32)}
    if conic:
        grads["dL_dconic"] = torch.zeros((P, 3), **f32)
    if g.shs:
        grads["dL_dsh"] = torch.zeros((P, g.M, 3), **f32)
    if g.scales:
        grads["dL_dscales"] = torch.zeros((P, 3), **f32)
        grads["dL_drotations"] = torch.zeros((P, 4), **f32)
    inp = _lib.GsrBackwardInputs(dL_dcolor=_lib.ptr(dL))
    out = _lib.GsrGradients(**{n: _lib.ptr(t) for n, t in grads.items()})
    plane_grads = {n: _as_dev(t, device, "H,W") for n, t in plane_grads.items()}
    if depths:
        grads["dL_ddepths"] = torch.zeros((P,), **f32)
    if stream is None:
        stream = torch.cuda.current_stream(device).cuda_stream
    lib = _lib.load_library()
    ctx = _lib.context(dev_index, slot)
    cam = {}
    if camera:
        cam = {"dL_dviewmatrix": torch.zeros((4, 4), **f32),
               "dL_dprojmatrix": torch.zeros((4, 4), **f32), "dL_dcampos": torch.zeros((3,), **f32)}
    head = (ctx, ctypes.byref(g), ctypes.byref(st), ctypes.byref(inp))
    if absgrad:
        d_abs = grads["dL_dmeans2D_abs"] = torch.zeros((P, 3), **f32)
    if features is not None:
        d_feat = grads["dL_dfeatures"] = torch.zeros((P, features.size(1)), **f32)
        d_map = _as_dev(dL_dfeature_map, device, "C,H,W")
    # the optional structs, NULL for each the call does without
    structs = _refs(
        (plane_grads or depths) and _lib.GsrPlaneGradients(
            **{n: _lib.ptr(t) for n, t in plane_grads.items()},
            dL_ddepths=_lib.ptr(grads.get("dL_ddepths"))),
        camera and _lib.GsrCameraGradients(**{n: _lib.ptr(t) for n, t in cam.items()}),
        antialiasing and _lib.GsrFilterSettings(antialiasing=int(antialiasing)),
        deterministic and _lib.GsrBackwardOrder(deterministic=int(deterministic)),
        features is not None and _lib.GsrFeatureGradients(
            C=int(features.size(1)), features=_lib.ptr(features),
            dL_dfeature_map=_lib.ptr(d_map), dL_dfeatures=_lib.ptr(d_feat)),
        absgrad and _lib.GsrAbsGradients(dL_dmeans2D_abs=_lib.ptr(d_abs)))
    with torch.cuda.device(dev_index):
        name, fn, n = _lowest_entry(_BACKWARD_ENTRIES, lib, structs, strip=bool(re))
        _lib.check(fn(*head, *structs[:n], ctypes.byref(out), ctypes.c_void_p(stream)), name)
    grads.update(cam)
    return grads


def rasterize_gaussians(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                        cov3Ds_precomp, raster_settings: GaussianRasterizationSettings,
                        features=None):
    """upstream rasterize_gaussians(...) -> (color, radii), through _RasterizeGaussians; with
    raster_settings.depth_maps -> (color, radii, depth_map, inv_depth_map, final_T), through
    _RasterizeGaussiansPlanes.  When viewmatrix, projmatrix or campos of the settings requires a
    gradient (and gradients are recorded), through _RasterizeGaussiansCamera, which returns the
    same outputs and also differentiates with respect to the three.  With `features` (P, C), through
    _RasterizeGaussiansFeatures: the same outputs followed by feature_map (C, rows, W)."""
    rs = raster_settings
    if features is not None:
        return _RasterizeGaussiansFeatures.apply(means3D, means2D, sh, colors_precomp, opacities,
                                                 scales, rotations, cov3Ds_precomp, rs, features,
                                                 rs.viewmatrix, rs.projmatrix, rs.campos)
    if torch.is_grad_enabled() and any(
            isinstance(t, torch.Tensor) and t.requires_grad
            for t in (rs.viewmatrix, rs.projmatrix, rs.campos)):
        return _RasterizeGaussiansCamera.apply(means3D, means2D, sh, colors_precomp, opacities,
                                               scales, rotations, cov3Ds_precomp, rs,
                                               rs.viewmatrix, rs.projmatrix, rs.campos)
    if raster_settings.depth_maps:
        return _RasterizeGaussiansPlanes.apply(means3D, means2D, sh, colors_precomp, opacities,
                                               scales, rotations, cov3Ds_precomp, raster_settings)
    return _RasterizeGaussians.apply(means3D, means2D, sh, colors_precomp, opacities, scales,
                                     rotations, cov3Ds_precomp, raster_settings)


# upstream's debug dump (diff-gaussian-rasterization __init__.py; the reference ignores the file
# in /root/reference/.gitignore:7)
SNAPSHOT_FILE = "snapshot_fw.dump"


def _cpu_copy(args):
    """The `_C.rasterize_gaussians` argument tuple with every tensor copied to the host."""
    return tuple(a.detach().cpu().clone() if isinstance(a, torch.Tensor) else a for a in args)


def replay_snapshot(path: str = SNAPSHOT_FILE, device=None):
    """Re-run a forward from a debug snapshot (the 19 `_C.rasterize_gaussians` arguments, tensors
    on the host) on `device` (default: the current HIP device); returns upstream's 6-tuple.
    Loaded with weights_only=True: the file holds tensors and plain numbers only."""
    from . import _C
    args = torch.load(path, weights_only=True)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    args = tuple(a.to(dev) if isinstance(a, torch.Tensor) and a.numel() else a for a in args)
    return _C.rasterize_gaussians(*args)


PLANE_NAMES = ("depth_map", "inv_depth_map", "final_T")


def _pack(rs, means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp):
    """`_C.rasterize_gaussians`'s 19 arguments; absent inputs travel as empty tensors, as
    upstream's __init__.py passes them."""
    none = lambda t: torch.empty(0) if t is None else t  # noqa: E731
    return (rs.bg, means3D, none(colors_precomp), opacities, none(scales), none(rotations),
            rs.scale_modifier, none(cov3Ds_precomp), rs.viewmatrix, rs.projmatrix, rs.tanfovx,
            rs.tanfovy, rs.image_height, rs.image_width, none(sh), rs.sh_degree, rs.campos,
            rs.prefiltered, rs.debug)


def _saved(args):
    """The tensors of `_pack`'s tuple a backward needs: means3D, sh, colors_precomp, opacities,
    scales, rotations, cov3Ds_precomp."""
    return args[1], args[14], args[2], args[3], args[4], args[5], args[7]


def _forward(args, rs, planes: bool, features=None):
    """One frame of `_pack`'s arguments -> (num_rendered, color, radii, planes, feature_map):
    PLANE_NAMES' tensors, or () without `planes`; feature_map (C, rows, W) of `features` (P, C),
    or None without.  Through `_C`: upstream's entry for the plain frame, its shaded twin, the
    features' entry, the general entry for the rest; under GSR_LIB (an A/B build: `_C` links the
    in-tree library) by ctypes."""
    strip = getattr(rs, "tile_rows", None)
    if not _lib._native_shares_library():
        res = rasterize_gaussians_native(*args, extras=PLANE_NAMES if planes else (),
                                         shading=rs.shading, antialiasing=rs.antialiasing,
                                         tile_rows=strip, features=features)
        return (res.num_rendered, res.color, res.radii,
                tuple(res.extras[n] for n in PLANE_NAMES) if planes else (), res.feature_map)
    from . import _C
    if strip:  # (checked here for the message; the entry checks it again)
        _strip_rows(strip, int(rs.image_height))
    feature_map = None
    if features is not None:
        num_rendered, color, radii, *maps, feature_map = _C.rasterize_gaussians_features(
            *args, planes, bool(rs.antialiasing), *(strip or (0, 0)), features)
    elif planes or rs.antialiasing or strip:
        num_rendered, color, radii, *maps = _C.rasterize_gaussians_ext(
            *args, int(rs.shading), planes, bool(rs.antialiasing), *(strip or ()))
    elif rs.shading:  # upstream's 19 arguments and the shading
        num_rendered, color, radii, *maps = _C.rasterize_gaussians_shaded(*args, int(rs.shading))
    else:
        num_rendered, color, radii, *maps = _C.rasterize_gaussians(*args)
    return num_rendered, color, radii, tuple(maps) if planes else (), feature_map


_GRADIENT_ORDER = ("dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D",
                   "dL_dsh", "dL_dscales", "dL_drotations") + _lib.CAMERA_GRADIENT_NAMES


def _deterministic(rs) -> bool:
    """The backward's mode: the setting, or with None torch's global switch, read when the
    backward runs."""
    det = getattr(rs, "deterministic", None)
    return torch.are_deterministic_algorithms_enabled() if det is None else bool(det)


def _refuse_deterministic_features(rs):
    """The deterministic mode has no feature sums (gsr_backward_features refuses it): the setting
    raises; torch's global switch raises too, or with warn_only warns and runs the atomic sums."""
    what = ("the deterministic backward has no feature channels: its slots hold 9 or 10 sums per "
            "(Gaussian, tile, quadrant) and have no room for C more")
    if getattr(rs, "deterministic", None):
        raise RuntimeError(f"GaussianRasterizationSettings(deterministic=True) with features: {what}")
    if getattr(rs, "deterministic", None) is None and torch.are_deterministic_algorithms_enabled():
        if not torch.is_deterministic_algorithms_warn_only_enabled():
            raise RuntimeError(f"torch.use_deterministic_algorithms(True) with features: {what} "
                               "(deterministic=False in the settings runs the atomic sums)")
        import warnings
        warnings.warn(f"gaussiansplattingviewer_amd: {what}; the sums over pixels are float "
                      "atomics in this backward", UserWarning, stacklevel=3)


def _backward(rs, saved, grads, camera=None, features=None, grad_feature_map=None,
              absgrad=False):
    """The gradients of one frame.  saved: `_saved`'s seven; grads: those of (color, depth_map,
    inv_depth_map, final_T), None = unused; camera: None, or the (viewmatrix, projmatrix, campos)
    to differentiate by, which the frame was rendered with.  Returns `_GRADIENT_ORDER`'s eleven,
    the camera's three None without `camera`.  Through `_C`: upstream's entry when only the
    image's gradient is asked for, else the general one; under GSR_LIB by ctypes.  In the
    deterministic mode (`_deterministic`) the general entry with a 23rd argument, True; on a
    strip (rs.tile_rows) the strip's entry, whose three more are the strip's rows and the frame's
    height.  With `features` (the frame's feature rows) and grad_feature_map, its planes' gradient
    or None, a twelfth follows: dL_dfeatures, through the features' entry, which has no
    deterministic mode (`_refuse_deterministic_features`).  With `absgrad` (never with features)
    a twelfth follows instead: dL_dmeans2D_abs, through the absolute gradient's entry, on whole
    frames and strips and in both modes."""
    means3D, sh, colors_precomp, opacities, scales, rotations, cov3Ds = saved
    det = _deterministic(rs)
    if features is not None:
        _refuse_deterministic_features(rs)
        if grad_feature_map is None:  # the loss does not read the feature planes
            g = _backward(rs._replace(deterministic=False), saved, grads, camera)
            return (*g, torch.zeros_like(features))
        det = False
    strip = getattr(rs, "tile_rows", None)
    viewmatrix, projmatrix, campos = camera or (rs.viewmatrix, rs.projmatrix, rs.campos)
    if not _lib._native_shares_library():
        g = rasterize_gaussians_backward_native(
            rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier,
            cov3Ds, viewmatrix, projmatrix, rs.tanfovx, rs.tanfovy, grads[0], sh, rs.sh_degree,
            campos, rs.debug, dL_ddepth_map=grads[1], dL_dinv_depth_map=grads[2],
            dL_dfinal_T=grads[3], camera=camera is not None, antialiasing=rs.antialiasing,
            deterministic=det, tile_rows=strip,
            image_height=None if strip is None else rs.image_height,
            features=features, dL_dfeature_map=grad_feature_map, absgrad=absgrad)
        return tuple(g.get(n) for n in _GRADIENT_ORDER) + \
            (() if features is None else (g["dL_dfeatures"],)) + \
            ((g["dL_dmeans2D_abs"],) if absgrad else ())
    from . import _C
    e = torch.empty(0)
    if (camera is None and not rs.antialiasing and not det and strip is None and
            features is None and not absgrad and all(t is None for t in grads[1:])):
        # (radii, num_rendered and the three buffers: accepted and ignored)
        return _C.rasterize_gaussians_backward(
            rs.bg, means3D, e, colors_precomp, scales, rotations, rs.scale_modifier, cov3Ds,
            viewmatrix, projmatrix, rs.tanfovx, rs.tanfovy, grads[0], sh, rs.sh_degree, campos, e,
            0, e, e, rs.debug, opacities) + (None,) * 3
    if camera is not None:
        viewmatrix, projmatrix, campos = (_as_dev(t.detach(), means3D.device, "")
                                          for t in camera)
    if features is not None:
        entry = _C.rasterize_gaussians_backward_features
        tail = (False, *(strip or (0, 0)), int(rs.image_height), features, grad_feature_map)
    elif absgrad:
        entry = _C.rasterize_gaussians_backward_abs
        tail = (det, *(strip or (0, 0)), int(rs.image_height))
    elif strip:
        entry = _C.rasterize_gaussians_backward_strip_ext
        tail = (det, *strip, int(rs.image_height))
    else:
        entry = _C.rasterize_gaussians_backward_ext
        tail = (True,) if det else ()
    g = entry(
        rs.bg, means3D, colors_precomp, opacities, scales, rotations, rs.scale_modifier, cov3Ds,
        viewmatrix, projmatrix, rs.tanfovx, rs.tanfovy, sh, rs.sh_degree, campos, rs.debug,
        *(e if t is None else t for t in grads), camera is not None, bool(rs.antialiasing), *tail)
    return g if camera is not None else g[:8] + (None,) * 3 + g[11:]


def _input_grads(has_means2D, saved, g):
    """`_backward`'s result as a Function's nine: the gradients in input order (means3D, means2D,
    sh, colors_precomp, opacities, scales, rotations, cov3Ds_precomp, None); None for absent
    inputs.  means2D's is upstream's screen-space gradient, (P, 3) with z = 0 (densification
    reads it)."""
    _, sh, colors_precomp, opacities, scales, rotations, cov3Ds = saved
    d_means2D, d_colors, d_opacity, d_means3D, d_cov3D, d_sh, d_scales, d_rot = g[:8]
    has = lambda t: t.numel() != 0  # noqa: E731
    return (d_means3D, d_means2D if has_means2D else None,
            d_sh.reshape(sh.shape) if has(sh) else None,
            d_colors if has(colors_precomp) else None, d_opacity.view_as(opacities),
            d_scales if has(scales) else None, d_rot if has(rotations) else None,
            d_cov3D if has(cov3Ds) else None, None)


def _contiguous(grads):
    return [None if t is None else t.contiguous() for t in grads]


class _RasterizeGaussians(torch.autograd.Function):
    """upstream `_RasterizeGaussians`: packs the settings into `_C.rasterize_gaussians`'s
    argument tuple and keeps (color, radii) of its 6-tuple; `backward` hands the saved inputs and
    the image's gradient to `_C.rasterize_gaussians_backward`.  Under `torch.no_grad()` (the
    viewer, renderer_cuda.py:214) nothing is saved and the forward is the same call."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                cov3Ds_precomp, raster_settings):
        # means2D only carries screen-space gradients, as upstream
        ctx.has_means2D = isinstance(means2D, torch.Tensor)
        rs = raster_settings
        args = _pack(rs, means3D, sh, colors_precomp, opacities, scales, rotations,
                     cov3Ds_precomp)
        # debug (upstream __init__.py): the arguments are copied to the host first, and a
        # forward that raises leaves them in SNAPSHOT_FILE for replay_snapshot()
        cpu_args = _cpu_copy(args) if rs.debug else None
        if rs.antialiasing and rs.shading:
            raise RuntimeError("antialiasing belongs to the splat composite: not available with "
                               f"shading {rs.shading}")
        try:
            num_rendered, color, radii, _, _ = _forward(args, rs, False)
        except Exception:
            if cpu_args is not None:
                torch.save(cpu_args, SNAPSHOT_FILE)
                print(f"\nThe forward raised; its arguments are in {SNAPSHOT_FILE} "
                      "(gaussiansplattingviewer_amd.rasterizer.replay_snapshot re-runs them).")
            raise
        ctx.num_rendered = num_rendered
        ctx.raster_settings = rs
        ctx.save_for_backward(*_saved(args))
        ctx.mark_non_differentiable(radii)
        return color, radii

    @staticmethod
    def backward(ctx, grad_color, grad_radii):
        """Gradients in input order (`_input_grads`)."""
        del grad_radii
        rs = ctx.raster_settings
        if rs.shading:
            raise RuntimeError("gaussiansplattingviewer_amd differentiates the splat composite "
                               f"only: no backward under shading {rs.shading}")
        g = _backward(rs, ctx.saved_tensors, (grad_color.contiguous(), None, None, None))
        return _input_grads(ctx.has_means2D, ctx.saved_tensors, g)


class _RasterizeGaussiansPlanes(torch.autograd.Function):
    """`_RasterizeGaussians` with the per-pixel planes (GaussianRasterizationSettings.depth_maps):
    returns (color, radii, depth_map, inv_depth_map, final_T).  The planes are those of
    `rasterize_gaussians_native(extras=PLANE_NAMES)` bit for bit, color and radii those of the
    plain call.  All four image-like outputs are differentiable through one `gsr_backward_planes`
    call; an output the loss does not use (its incoming gradient is None) travels as NULL.  Under
    `torch.no_grad()` nothing is saved."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                cov3Ds_precomp, raster_settings):
        rs = raster_settings
        if rs.shading != _lib.GSR_SHADE_SPLAT:
            raise RuntimeError("depth_map / inv_depth_map come from the splat composite: not "
                               f"available with shading {rs.shading}")
        ctx.has_means2D = isinstance(means2D, torch.Tensor)
        args = _pack(rs, means3D, sh, colors_precomp, opacities, scales, rotations,
                     cov3Ds_precomp)
        _, color, radii, planes, _ = _forward(args, rs, True)
        ctx.raster_settings = rs
        ctx.save_for_backward(*_saved(args))
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)  # an unused output's gradient arrives as None, not zeros
        return (color, radii, *planes)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth, grad_inv_depth, grad_final_T):
        """Gradients in input order (`_input_grads`)."""
        del grad_radii
        g = _backward(ctx.raster_settings, ctx.saved_tensors,
                      _contiguous((grad_color, grad_depth, grad_inv_depth, grad_final_T)))
        return _input_grads(ctx.has_means2D, ctx.saved_tensors, g)


class _RasterizeGaussiansCamera(torch.autograd.Function):
    """The two Functions above with the camera as tensor arguments: viewmatrix, projmatrix and
    campos (those of the settings, which the forward reads) follow raster_settings, and backward
    returns their gradients in the inputs' shape, dtype and device (`gsr_backward_camera`; each
    the partial with the other two held fixed).  The forward is the very call of the Function it
    stands in for -- (color, radii), or with depth_maps the 5-tuple -- so its outputs have those
    bits.  An unused output's gradient travels as NULL; a shading raises in backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                cov3Ds_precomp, raster_settings, viewmatrix, projmatrix, campos):
        rs = raster_settings
        ctx.has_means2D = isinstance(means2D, torch.Tensor)
        ctx.raster_settings = rs
        ctx.set_materialize_grads(False)
        args = _pack(rs, means3D, sh, colors_precomp, opacities, scales, rotations,
                     cov3Ds_precomp)
        ctx.save_for_backward(*_saved(args), viewmatrix, projmatrix, campos)
        # (inside a Function's forward no graph is recorded: the inner Function saves nothing)
        inner = _RasterizeGaussiansPlanes if rs.depth_maps else _RasterizeGaussians
        out = inner.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                          cov3Ds_precomp, rs)
        ctx.mark_non_differentiable(out[1])
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth=None, grad_inv_depth=None,
                 grad_final_T=None):
        """Gradients in input order: the nine of `_input_grads`, then viewmatrix's, projmatrix's
        and campos's."""
        del grad_radii
        rs = ctx.raster_settings
        if rs.shading:
            raise RuntimeError("gaussiansplattingviewer_amd differentiates the splat composite "
                               f"only: no backward under shading {rs.shading}")
        *saved, viewmatrix, projmatrix, campos = ctx.saved_tensors
        grads = _contiguous((grad_color, grad_depth, grad_inv_depth, grad_final_T))
        if all(t is None for t in grads):  # nothing reaches the outputs
            return (None,) * 12
        g = _backward(rs, saved, grads, camera=(viewmatrix, projmatrix, campos))
        need = ctx.needs_input_grad
        like = lambda d, t: d.reshape(t.shape).to(device=t.device, dtype=t.dtype)  # noqa: E731
        return (*_input_grads(ctx.has_means2D, saved, g),
                like(g[8], viewmatrix) if need[9] else None,
                like(g[9], projmatrix) if need[10] else None,
                like(g[10], campos) if need[11] else None)


class _RasterizeGaussiansFeatures(torch.autograd.Function):
    """The three Functions above in one, with `features` (P, C) composited beside the colour
    (`gsr_forward_features`): returns the outputs of the call without features -- (color, radii),
    with depth_maps (color, radii, depth_map, inv_depth_map, final_T) -- followed by feature_map
    (C, rows, W).  Everything but radii is differentiable through one `gsr_backward_features` call,
    with respect to features and everything the colour reaches; viewmatrix, projmatrix and campos
    travel as tensor arguments and get their gradients when they require them.  An unused output's
    gradient travels as NULL."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                cov3Ds_precomp, raster_settings, features, viewmatrix, projmatrix, campos):
        rs = raster_settings
        if rs.shading != _lib.GSR_SHADE_SPLAT:
            raise RuntimeError("features are composited by the splat composite: not available "
                               f"with shading {rs.shading}")
        ctx.has_means2D = isinstance(means2D, torch.Tensor)
        ctx.raster_settings = rs
        ctx.set_materialize_grads(False)
        args = _pack(rs, means3D, sh, colors_precomp, opacities, scales, rotations,
                     cov3Ds_precomp)
        rows = _feature_rows(features, int(means3D.size(0)), means3D.device)
        _, color, radii, planes, feature_map = _forward(args, rs, bool(rs.depth_maps), rows)
        # (a camera given as plain numbers has no gradient and is read from the settings)
        ctx.save_for_backward(*_saved(args), rows, *(
            t if isinstance(t, torch.Tensor) else None for t in (viewmatrix, projmatrix, campos)))
        ctx.features_like = (features.dtype, features.device)
        ctx.mark_non_differentiable(radii)
        return (color, radii, *planes, feature_map)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, *more):
        """Gradients in input order: the nine of `_input_grads`, features', then viewmatrix's,
        projmatrix's and campos's."""
        del grad_radii
        rs = ctx.raster_settings
        *saved, rows, viewmatrix, projmatrix, campos = ctx.saved_tensors
        grad_planes = more[:-1] if rs.depth_maps else (None, None, None)
        grads = _contiguous((grad_color, *grad_planes))
        grad_map = None if more[-1] is None else more[-1].contiguous()
        if all(t is None for t in grads) and grad_map is None:
            return (None,) * 13
        need = ctx.needs_input_grad
        with_camera = any(need[10:13])
        if viewmatrix is None or projmatrix is None or campos is None:
            viewmatrix, projmatrix, campos = rs.viewmatrix, rs.projmatrix, rs.campos
        g = _backward(rs, saved, grads, (viewmatrix, projmatrix, campos) if with_camera else None,
                      features=rows, grad_feature_map=grad_map)
        like = lambda d, t: d.reshape(t.shape).to(device=t.device, dtype=t.dtype)  # noqa: E731
        features = ctx.features_like
        return (*_input_grads(ctx.has_means2D, saved, g)[:8], None,
                g[11].to(dtype=features[0], device=features[1]) if need[9] else None,
                like(g[8], viewmatrix) if need[10] else None,
                like(g[9], projmatrix) if need[11] else None,
                like(g[10], campos) if need[12] else None)


def _check_means2D_abs(means2D_abs, means3D):
    """`means2D_abs` as GaussianRasterizer.forward takes it; ValueError otherwise."""
    P = int(means3D.size(0))
    t = means2D_abs
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != (P, 3):
        raise ValueError(f"means2D_abs must be a tensor of shape (num_points, 3) = ({P}, 3)")
    if t.dtype != torch.float32:
        raise ValueError(f"means2D_abs must be float32, got {t.dtype}")
    if t.device != means3D.device:
        raise ValueError(f"means2D_abs must be on the scene's device {means3D.device}, got "
                         f"{t.device}")
    if not t.requires_grad:
        raise ValueError("means2D_abs must require a gradient: its .grad is the output")


class _RasterizeGaussiansAbs(torch.autograd.Function):
    """The first three Functions in one, with `means2D_abs`, a second (P, 3) leaf beside means2D
    whose value is never read: returns the outputs of the call without it -- (color, radii), with
    depth_maps (color, radii, depth_map, inv_depth_map, final_T) -- with those bits, and backward
    returns dL_dmeans2D_abs (`gsr_backward_abs`, include/gsr.h) as means2D_abs's gradient beside
    every gradient of the call without it.  viewmatrix, projmatrix and campos travel as tensor
    arguments and get their gradients when they require them.  An unused output's gradient travels
    as NULL; a shading raises in backward."""

    @staticmethod
    def forward(ctx, means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                cov3Ds_precomp, raster_settings, means2D_abs, viewmatrix, projmatrix, campos):
        rs = raster_settings
        ctx.has_means2D = isinstance(means2D, torch.Tensor)
        ctx.raster_settings = rs
        ctx.set_materialize_grads(False)
        args = _pack(rs, means3D, sh, colors_precomp, opacities, scales, rotations,
                     cov3Ds_precomp)
        ctx.save_for_backward(*_saved(args), *(
            t if isinstance(t, torch.Tensor) else None for t in (viewmatrix, projmatrix, campos)))
        # (inside a Function's forward no graph is recorded: the inner Function saves nothing)
        inner = _RasterizeGaussiansPlanes if rs.depth_maps else _RasterizeGaussians
        out = inner.apply(means3D, means2D, sh, colors_precomp, opacities, scales, rotations,
                          cov3Ds_precomp, rs)
        ctx.mark_non_differentiable(out[1])
        return tuple(out)

    @staticmethod
    def backward(ctx, grad_color, grad_radii, grad_depth=None, grad_inv_depth=None,
                 grad_final_T=None):
        """Gradients in input order: the nine of `_input_grads`, means2D_abs's, then
        viewmatrix's, projmatrix's and campos's."""
        del grad_radii
        rs = ctx.raster_settings
        if rs.shading:
            raise RuntimeError("gaussiansplattingviewer_amd differentiates the splat composite "
                               f"only: no backward under shading {rs.shading}")
        *saved, viewmatrix, projmatrix, campos = ctx.saved_tensors
        grads = _contiguous((grad_color, grad_depth, grad_inv_depth, grad_final_T))
        if all(t is None for t in grads):  # nothing reaches the outputs
            return (None,) * 13
        need = ctx.needs_input_grad
        with_camera = any(need[10:13])
        if viewmatrix is None or projmatrix is None or campos is None:
            viewmatrix, projmatrix, campos = rs.viewmatrix, rs.projmatrix, rs.campos
        g = _backward(rs, saved, grads, (viewmatrix, projmatrix, campos) if with_camera else None,
                      absgrad=True)
        like = lambda d, t: d.reshape(t.shape).to(device=t.device, dtype=t.dtype)  # noqa: E731
        return (*_input_grads(ctx.has_means2D, saved, g), g[11] if need[9] else None,
                like(g[8], viewmatrix) if need[10] else None,
                like(g[9], projmatrix) if need[11] else None,
                like(g[10], campos) if need[12] else None)


class GaussianRasterizer(torch.nn.Module):
    def __init__(self, raster_settings: GaussianRasterizationSettings):
        super().__init__()
        self.raster_settings = raster_settings

    def markVisible(self, positions: torch.Tensor) -> torch.Tensor:
        """Frustum-cull test per point: view-space z > 0.2 (upstream markVisible, through
        `_C.mark_visible`)."""
        from . import _C
        with torch.no_grad():
            rs = self.raster_settings
            return _C.mark_visible(positions, rs.viewmatrix, rs.projmatrix)

    def forward(self, means3D, means2D, opacities, shs=None, colors_precomp=None, scales=None,
                rotations=None, cov3D_precomp=None, means2D_abs=None, features=None):
        """upstream's forward; features (not upstream's; (P, C) float32, 1 <= C <= 256): the call
        returns its usual outputs followed by feature_map (C, rows, W), the channels composited
        under the colour's weights without a background term (gsr_forward_features in
        include/gsr.h), differentiable with respect to features and everything the colour
        reaches.  Composes with depth_maps, camera gradients, antialiasing and tile_rows; not
        with a shading, nor with the deterministic backward (RuntimeError at backward).

        means2D_abs (not upstream's; pass it by keyword: it stands before features, which stays
        the last parameter; a (P, 3) float32 leaf on the scene's device that requires a
        gradient, used the way means2D is: its value is never read): after backward() its .grad
        is dL_dmeans2D_abs, means2D's gradient with every pixel's term taken by its absolute
        value before the sum over pixels (AbsGS; gsr_backward_abs in include/gsr.h), the number
        to feed `optim.densification_stats` in place of means2D.grad.  It accumulates over
        backward() calls like any .grad.  The outputs are those of the call without it.  Composes
        with depth_maps, camera gradients, antialiasing, tile_rows and deterministic; ValueError
        for a tensor of another shape, dtype or device or one that requires no gradient;
        RuntimeError together with features (the absolute value of a pixel's total cannot be
        split over the feature channels' passes), and at backward with a shading."""
        rs = self.raster_settings
        if (shs is None and colors_precomp is None) or (shs is not None and colors_precomp is not None):
            raise Exception('Please provide excatly one of either SHs or precomputed colors!')
        if ((scales is None or rotations is None) and cov3D_precomp is None) or \
                ((scales is not None or rotations is not None) and cov3D_precomp is not None):
            raise Exception('Please provide exactly one of either scale/rotation pair or '
                            'precomputed 3D covariance!')
        if means2D_abs is not None:
            if features is not None:
                raise RuntimeError(
                    "means2D_abs with features: the feature channels add their share of "
                    "dL/dalpha in passes of their own, and the absolute value of a pixel's total "
                    "cannot be split over passes")
            _check_means2D_abs(means2D_abs, means3D)
            return _RasterizeGaussiansAbs.apply(means3D, means2D, shs, colors_precomp, opacities,
                                                scales, rotations, cov3D_precomp, rs, means2D_abs,
                                                rs.viewmatrix, rs.projmatrix, rs.campos)
        if features is not None:
            return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales,
                                       rotations, cov3D_precomp, rs, features=features)
        return rasterize_gaussians(means3D, means2D, shs, colors_precomp, opacities, scales,
                                   rotations, cov3D_precomp, rs)


def binning_state(device_index: int = 0, slot: int = 0):
    """(point_list, point_tiles, ranges [T,2]) of the last forward on a device's context slot,
    as device int32 tensors holding the uint32 values (test / debug helper)."""
    lib = _lib.load_library()
    ctx = _lib.context(device_index, slot)
    K = ctypes.c_int64()
    T = ctypes.c_int32()
    stream = ctypes.c_void_p(torch.cuda.current_stream(device_index).cuda_stream)
    _lib.check(lib.gsr_get_binning(ctx, None, None, None, ctypes.byref(K), ctypes.byref(T),
                                   stream), "gsr_get_binning")
    dev = torch.device("cuda", device_index)
    pl = torch.empty((K.value,), dtype=torch.int32, device=dev)
    pt = torch.empty((K.value,), dtype=torch.int32, device=dev)
    rg = torch.empty((T.value, 2), dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_get_binning(ctx, _lib.ptr(pl), _lib.ptr(pt), _lib.ptr(rg), None, None,
                                   stream), "gsr_get_binning")
    return pl, pt, rg


def tile_row_pairs(n_rows: int, device_index: int = 0, slot: int = 0, out=None,
                   stream=None) -> torch.Tensor:
    """Pair count of every tile row of the last forward's strip on a device's context slot
    (gsr_tile_row_pairs), as a device int32 tensor of n_rows uint32 values, written on `stream`
    (default: the current stream) without synchronising.  strips.StripBalancer weights the
    next frame's strip boundaries by these counts."""
    lib = _lib.load_library()
    ctx = _lib.context(device_index, slot)
    if out is None:
        out = torch.empty((n_rows,), dtype=torch.int32, device=torch.device("cuda", device_index))
    s = stream if stream is not None else torch.cuda.current_stream(device_index)
    _lib.check(lib.gsr_tile_row_pairs(ctx, _lib.ptr(out), int(n_rows),
                                      ctypes.c_void_p(s.cuda_stream)), "gsr_tile_row_pairs")
    return out
