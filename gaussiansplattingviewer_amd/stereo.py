"""Stereo dataset capture on the device.

The fork's product is a stereo dataset: for every COLMAP pose the viewer renders the left
view, a disparity image and the right view, and saves them as left/{i}.png, depth/{i}.png and
right/{i}.png (main.py:839-923).  Upstream that only works in the GL backend (render mode -1,
FBO readbacks).  Here the same three images come from the HIP rasterizer:

* `disparity_colors` -- the per-Gaussian disparity grey of gau_vert.glsl:182-207 (HIP kernel
  `gsr_disparity_colors`), composited like any colour with the Gaussians scaled by 1.2
  (gau_vert.glsl:152-156) -- see `HIPRenderer.set_render_mod(-1)`;
* `pack_image` -- the device packer (`gsr_pack_image`): RGB8 as glReadPixels(GL_RGB,
  GL_UNSIGNED_BYTE) converts, uint16 = disparity * 65535 truncated (main.py:873-874), or the
  HWC RGBA float of renderer_cuda.py:226-228;
* `metric_disparity` -- the left view's disparity in pixels, fx |B| / z, from the inverse-depth
  plane of the left image's own blend pass (`gsr_forward_depth`): metric, pixel-aligned with
  the left image, and no third forward (`StereoCapture(disparity="metric")`);
* `median_disparity` -- fx |B| / z of the pixel's median splat (`gsr_forward_surface`): the
  disparity of one Gaussian of the pixel's list, never a mix of foreground and background at a
  silhouette (`StereoCapture(disparity="median")`);
* `StereoCapture` -- the capture sequence of main.py:843-917 (left pose, disparity with the
  left pose still bound, right pose) on a `HIPRenderer`, returning device tensors; `save`
  writes the PNGs (PIL) the way the viewer names them.

Orientation: the viewer's CUDA path negates view rows 0 and 2 (renderer_cuda.py:189-191),
which puts NDC +y (the top of the GL framebuffer) at raster row 0.  The GL capture reads rows
bottom-up and then flips them (main.py:875-879, 911-912), so its PNG row 0 is the top as well:
the rasterizer's rows are saved as they are (flip_rows=False).
"""
from __future__ import annotations

import ctypes
import os

import numpy as np
import torch

from . import _lib
from .colmap import BASELINE, load_camera_positions

DISPARITY_SCALE = 1.2  # gau_vert.glsl:152-153: scale * scale_modifier * 1.2 in mode -1

_FORMATS = {
    "rgba_f32": (_lib.GSR_PACK_RGBA_F32, torch.float32, 4),
    "rgb8": (_lib.GSR_PACK_RGB8, torch.uint8, 3),
    "r16": (_lib.GSR_PACK_R16, torch.uint16, 0),
}


def _stream(dev: torch.device) -> int:
    return torch.cuda.current_stream(dev).cuda_stream


def _mat16(m) -> ctypes.Array:
    a = np.ascontiguousarray(np.asarray(m, dtype=np.float32).reshape(16))
    return (ctypes.c_float * 16)(*a.tolist())


def disparity_colors(xyz: torch.Tensor, view_gl, proj_gl, baseline: float = BASELINE,
                     out: torch.Tensor | None = None) -> torch.Tensor:
    """(P, 3) float32 device colours (d, d, d), d = |x_l - x_r| of gau_vert.glsl:182-207.
    view_gl / proj_gl: host 4x4 math-layout GL view and projection (util.py:58-105)."""
    if not (isinstance(xyz, torch.Tensor) and xyz.is_cuda):
        raise RuntimeError("disparity_colors needs a device xyz tensor (no CPU path)")
    if xyz.ndim != 2 or xyz.shape[1] != 3:
        raise RuntimeError("xyz must have dimensions (num_points, 3)")
    xyz = xyz.float().contiguous()
    P = int(xyz.shape[0])
    if out is None:
        out = torch.empty((P, 3), dtype=torch.float32, device=xyz.device)
    elif out.shape != (P, 3) or out.dtype != torch.float32 or not out.is_contiguous():
        raise RuntimeError("out must be a contiguous float32 (P, 3) tensor")
    lib = _lib.load_library()
    _lib.check(lib.gsr_disparity_colors(_lib.ptr(xyz), P, _mat16(view_gl), _mat16(proj_gl),
                                        float(baseline), _lib.ptr(out), _stream(xyz.device)),
               "gsr_disparity_colors")
    return out


def pack_image(image: torch.Tensor, fmt: str, flip_rows: bool = False,
               out: torch.Tensor | None = None) -> torch.Tensor:
    """Pack a (3, H, W) float32 device image: "rgb8" -> uint8 (H, W, 3), "r16" -> uint16 (H, W)
    from channel 0, "rgba_f32" -> float32 (H, W, 4) with alpha 1."""
    if fmt not in _FORMATS:
        raise ValueError(f"unknown format {fmt!r}; expected one of {sorted(_FORMATS)}")
    if not (isinstance(image, torch.Tensor) and image.is_cuda):
        raise RuntimeError("pack_image needs a device image (no CPU path)")
    if image.ndim != 3 or image.shape[0] != 3 or image.dtype != torch.float32:
        raise RuntimeError("image must be a float32 (3, H, W) tensor")
    image = image.contiguous()
    code, dtype, ch = _FORMATS[fmt]
    H, W = int(image.shape[1]), int(image.shape[2])
    shape = (H, W, ch) if ch else (H, W)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=image.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous {dtype} {shape} tensor")
    lib = _lib.load_library()
    _lib.check(lib.gsr_pack_image(_lib.ptr(image), H, W, code, int(bool(flip_rows)),
                                  _lib.ptr(out), _stream(image.device)), "gsr_pack_image")
    return out


def metric_disparity(inv_depth_map: torch.Tensor, final_T: torch.Tensor, tanfovx: float,
                     width: int, baseline: float = BASELINE, normalise: bool = True) -> torch.Tensor:
    """Disparity in pixels, float32 (H, W), of a rectified pair whose right view is the left one
    translated by `baseline` along view-space x (colmap.py load_camera_positions):
    fx |baseline| / z with fx = width / (2 tanfovx), linear in inverse depth.  inv_depth_map and
    final_T are the left frame's planes (premultiplied sum of w / z; transmittance).  normalise:
    divided by the covered share 1 - final_T where that is > 0, else 0 (no surface); False
    returns the premultiplied map.  Plain torch ops: device or host tensors."""
    inv = inv_depth_map.to(torch.float32)
    scale = float(width) / (2.0 * float(tanfovx)) * abs(float(baseline))
    d = inv * scale
    if not normalise:
        return d
    cover = 1.0 - final_T.to(torch.float32)
    # (the quotient where cover <= 0 is discarded: five element-wise kernels in all)
    return torch.where(cover > 0, d / cover, torch.zeros((), dtype=d.dtype, device=d.device))


def median_disparity(median_depth: torch.Tensor, tanfovx: float, width: int,
                     baseline: float = BASELINE) -> torch.Tensor:
    """Disparity in pixels, float32 (H, W), of the pixel's median splat: fx |baseline| / z with
    fx = width / (2 tanfovx) where median_depth > 0, else 0 (no surface: the transmittance never
    reaches 0.5).  median_depth is the left frame's plane (gsr_forward_surface), the view-space z
    of one Gaussian per pixel, so every value is the disparity of a Gaussian of the scene: no
    pixel lies between a foreground and a background surface, as the expected inverse depth
    (metric_disparity) does along a silhouette.  One float32 division of the float32 product
    fx |baseline|.  Plain torch ops: device or host tensors."""
    z = median_depth.to(torch.float32)
    scale = torch.tensor(float(width) / (2.0 * float(tanfovx)) * abs(float(baseline)),
                         dtype=torch.float32, device=z.device)
    return torch.where(z > 0, scale / z, torch.zeros((), dtype=z.dtype, device=z.device))


def disparity_u16(disparity: torch.Tensor) -> torch.Tensor:
    """The KITTI disparity PNG's values: uint16 = min(65535, round(256 d)), 0 = no surface;
    returned as int32 (H, W) (torch's uint16 has no rounding ops), cast at the save."""
    return torch.clamp(torch.round(disparity.to(torch.float32) * 256.0), 0, 65535).to(torch.int32)


class StereoCapture:
    """main.py:839-923 on a HIPRenderer: left RGB, disparity, right RGB for one pose.

    `render_mode` is the viewer's g_render_mode - 3 (default 3: full SH, main.py:99).
    `disparity`: "gl" (default) the GL backend's mode -1 image as "depth", a third forward;
    "metric" the left frame's own inverse-depth plane as "disparity" (metric_disparity, float32
    pixels), two forwards -- the renderer must be a HIPRenderer(depth_maps=True); "both" all
    four from three forwards; "median" the left frame's median-depth plane as "disparity"
    (median_disparity, float32 pixels), two forwards -- the renderer must be a
    HIPRenderer(surface_maps=True)."""

    DISPARITIES = ("gl", "metric", "both", "median")

    def __init__(self, renderer, camera, render_mode: int = 3, disparity: str = "gl"):
        if disparity not in self.DISPARITIES:
            raise ValueError(f"disparity must be one of {self.DISPARITIES}, not {disparity!r}")
        if disparity == "median":
            if not getattr(renderer, "surface_maps", False):
                raise RuntimeError('disparity="median" needs HIPRenderer(..., surface_maps=True)')
        elif disparity != "gl" and not getattr(renderer, "depth_maps", False):
            raise RuntimeError(f'disparity="{disparity}" needs HIPRenderer(..., depth_maps=True)')
        self.renderer = renderer
        self.camera = camera
        self.render_mode = int(render_mode)
        self.disparity = disparity

    def render(self, camera_pose) -> dict:
        """One images.txt entry -> {"left": u8 (H,W,3), "depth": u16 (H,W), "right": u8
        (H,W,3)} device tensors, in the viewer's draw order (main.py:845-900); with
        disparity="metric" or "median" {"left", "right", "disparity": f32 (H,W) pixels}, "both"
        all four."""
        r, cam = self.renderer, self.camera
        pose_left, pose_right = load_camera_positions(camera_pose)
        r.update_camera_intrin(cam)                       # main.py:826-827
        r.set_render_mod(self.render_mode)                 # main.py:845
        r.sort_and_update(cam, True, pose_left)
        r.update_camera_pose(cam, True, pose_left)
        out = {"left": pack_image(r.draw(), "rgb8")}
        if self.disparity == "median":
            if r.median_depth is None:
                raise RuntimeError("the median disparity needs the splat composite (render_mode "
                                   f"{self.render_mode} is a GL shading)")
            rs = r.raster_settings
            out["disparity"] = median_disparity(r.median_depth, rs["tanfovx"], rs["image_width"])
        elif self.disparity != "gl":
            if r.inv_depth_map is None:
                raise RuntimeError("the metric disparity needs the splat composite (render_mode "
                                   f"{self.render_mode} is a GL shading)")
            rs = r.raster_settings
            out["disparity"] = metric_disparity(r.inv_depth_map, r.final_T, rs["tanfovx"],
                                                rs["image_width"])
        # only the left frame needs its planes (they stay in the renderer, the left view's)
        planes, r.depth_maps = r.depth_maps, r.depth_maps and self.disparity == "gl"
        surface = getattr(r, "surface_maps", False)
        if self.disparity == "median":
            r.surface_maps = False
        try:
            if self.disparity not in ("metric", "median"):
                r.set_render_mod(-1)                       # main.py:867-868: left pose bound
                out["depth"] = pack_image(r.draw(), "r16")
            r.set_render_mod(self.render_mode)             # main.py:885-889
            r.sort_and_update(cam, True, pose_right)
            r.update_camera_pose(cam, True, pose_right)
            out["right"] = pack_image(r.draw(), "rgb8")
        finally:
            r.depth_maps = planes
            if self.disparity == "median":
                r.surface_maps = surface
        return out

    @staticmethod
    def save(frames: dict, out_dir: str, scene: str, pose_index: int) -> list[str]:
        """Write left/right RGB PNGs and the 16-bit disparity PNG under
        out_dir/scene/{left,right,depth}/{pose_index}.png (main.py:701-712, 879, 916-917); a
        metric "disparity" as disparity/{pose_index}.png, uint16 = min(65535, round(256 d)) with
        0 = no surface (the KITTI convention)."""
        from PIL import Image
        paths = []
        for kind in ("left", "depth", "disparity", "right"):
            if kind not in frames:
                continue
            d = os.path.join(out_dir, scene, kind)
            os.makedirs(d, exist_ok=True)
            if kind == "disparity":
                a = disparity_u16(frames[kind]).cpu().numpy().astype(np.uint16)
            else:
                a = frames[kind].cpu().numpy()
            path = os.path.join(d, f"{pose_index}.png")
            Image.fromarray(a).save(path)
            paths.append(path)
        return paths
