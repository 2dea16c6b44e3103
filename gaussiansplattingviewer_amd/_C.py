"""upstream `diff_gaussian_rasterization._C`: the native entry points, from the PyTorch-ROCm
extension `_native.so` (csrc/torch_ext.cpp) over libgsr.so.

Upstream's Python package calls one C++ entry per forward (rasterize_points.cu
`RasterizeGaussiansCUDA`, bound as `_C.rasterize_gaussians`; its caller is
`_RasterizeGaussians.forward` in `diff_gaussian_rasterization/__init__.py`, which the viewer
reaches through renderer_cuda.py:211-224):

    num_rendered, color, radii, geomBuffer, binningBuffer, imgBuffer = \\
        _C.rasterize_gaussians(bg, means3D, colors_precomp, opacities, scales, rotations,
                               scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tanfovx,
                               tanfovy, image_height, image_width, sh, sh_degree, campos,
                               prefiltered, debug)

    visible = _C.mark_visible(means3D, viewmatrix, projmatrix)

`_C.rasterize_gaussians_shaded(<the same 19 arguments>, shading)` is this package's own: the
same forward under one of the GL backend's shadings (`gsr_forward_shaded`, include/gsr.h).

Same arguments, order and return arity; absent optional inputs are empty tensors, as upstream
passes them.  The work is `gsr_forward` / `gsr_mark_visible` in libgsr.so, on torch's current
HIP stream, with one `gsr_context` per device held by the extension.  The three buffers are
upstream's scratch (geometry, binning and image state, kept for the backward pass); this
rasterizer keeps its state inside its context (reused across frames) and its backward rebuilds
what it needs from the inputs, so they are returned as empty uint8 device tensors.

The backward (rasterize_points.cu `RasterizeGaussiansBackwardCUDA`, called by
`_RasterizeGaussians.backward`):

    dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, \\
        dL_drotations = _C.rasterize_gaussians_backward(
            bg, means3D, radii, colors_precomp, scales, rotations, scale_modifier, cov3D_precomp,
            viewmatrix, projmatrix, tanfovx, tanfovy, dL_dout_color, sh, sh_degree, campos,
            geomBuffer, num_rendered, binningBuffer, imgBuffer, debug, opacities)

Upstream's 21 arguments in upstream's order and upstream's 8-tuple, plus ONE MORE trailing
argument, `opacities`: upstream reads them out of geomBuffer, here nothing of the forward is kept
and `gsr_backward` (include/gsr.h, which states the semantics) rebuilds the state from the
inputs.  `radii`, `num_rendered` and the three buffers are accepted and ignored.

`_C.rasterize_gaussians_ext(<the 19 arguments>, shading, planes, antialiasing)` ->
(num_rendered, color, radii, depth_map, inv_depth_map, final_T) and
`_C.rasterize_gaussians_backward_ext(bg, means3D, colors_precomp, opacities, scales, rotations,
scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, sh, sh_degree, campos,
debug, dL_dout_color, dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T, camera, antialiasing)` -> the
same 8-tuple, then dL_dviewmatrix (4, 4), dL_dprojmatrix (4, 4) and dL_dcampos (3,) are this
package's own, one general entry per direction behind `GaussianRasterizationSettings(depth_maps=
True)`, `(antialiasing=True)` and a `viewmatrix`, `projmatrix` or `campos` that requires a
gradient.  The forward is `gsr_forward_filtered` with the per-pixel planes only if `planes`
(without, the three tensors are empty) and the filter only if `antialiasing`; a shading, or
neither, is `gsr_forward_shaded`.  The backward is `gsr_backward_filtered` with NULL for what is
not asked for: an empty tensor is an unused gradient, and without `camera` its three are empty.
A strip of tile rows (`GaussianRasterizationSettings(tile_rows=)`): the forward takes
`tile_row_begin, tile_row_end` after `antialiasing` (they may be left out), and
`_C.rasterize_gaussians_backward_strip_ext(<the backward's arguments>, deterministic,
tile_row_begin, tile_row_end, image_height)` is `gsr_backward_strip` -- the image-like tensors are
then strip-local, and image_height is the frame's.
Feature channels (`GaussianRasterizer(...)(..., features=)`):
`_C.rasterize_gaussians_features(<the 19 arguments>, planes, antialiasing, tile_row_begin,
tile_row_end, features)` is `gsr_forward_features` -> the 6-tuple of `rasterize_gaussians_ext`,
then feature_map (C, rows, W); `_C.rasterize_gaussians_backward_features(<the backward's
arguments>, deterministic, tile_row_begin, tile_row_end, image_height, features,
dL_dfeature_map)` is `gsr_backward_features` -> the 11-tuple, then dL_dfeatures (P, C).
The absolute gradient of the 2D means (`GaussianRasterizer(...)(..., means2D_abs=)`):
`_C.rasterize_gaussians_backward_abs(<the backward's arguments>, deterministic, tile_row_begin,
tile_row_end, image_height)`, tile rows (0, 0) for a whole frame, is `gsr_backward_abs` -> the
11-tuple, then dL_dmeans2D_abs (P, 3).
The photometric loss (`losses.photometric_loss`): `_C.fused_image_loss(image, target,
lambda_dssim, need_saved)` is `gsr_image_loss` -> (values (3,) = loss, l1, ssim; saved
(3, C, H, W), empty without `need_saved`), and `_C.fused_image_loss_backward(image, target,
lambda_dssim, saved, dL_dloss)` is `gsr_image_loss_backward` -> dL_dimage; the images are contiguous
float32 (C, H, W) device tensors and dL_dloss one device value (empty = 1.0).  No context is used.
The frame's loss on a strip (`losses.frame_loss_on_strip`): `_C.fused_image_loss_window(image,
target, frame_H, row0, own_begin, own_end, lambda_dssim, need_saved)` is `gsr_image_loss_window`
on band buffers (C, rows, W) whose row 0 is frame row row0 -> (the window's three shares; saved
(3, C, A, W) over the apron), and `_C.fused_image_loss_window_backward(image, target, frame_H,
row0, own_begin, own_end, lambda_dssim, saved, dL_dloss)` is `gsr_image_loss_window_backward` ->
dL_dimage (C, own_end - own_begin, W).
The optimizer (`optim.SparseGaussianAdam`, `optim.densification_stats`): `_C.adamUpdate(param,
grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M)` has upstream's signature (one group,
in place, no bias correction); `_C.fused_adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs,
epss, mask, b1, b2, bc1, bc2_sqrt)` is `gsr_adam_step` on up to 8 groups in one launch (mask: bool
or uint8 (P), int32 radii (P), or empty); `_C.densification_stats(radii, means2D_grad, grad_accum,
denom, max_radii)` is `gsr_densify_stats`.  All three work in place on torch's current stream.
Density control (`densify.densify_and_prune`): `_C.densify_plan(grad_accum, denom, max_radii,
scaling, opacity, thresholds, radius_threshold, scale_space, workspace, counts)` is
`gsr_densify_plan` and `_C.densify_apply(<the same first eight>, seed, roles, has_moments,
src_params, src_exp_avgs, src_exp_avg_sqs, dst_params, dst_exp_avgs, dst_exp_avg_sqs, workspace,
source_index)` is `gsr_densify_apply`; the caller allocates every tensor, P_out is source_index's
length, and a group with has_moments 0 passes any tensors in the moments' places.
The start of a fit (`pointcloud.knn_mean_dist2`): `_C.distCUDA2(points)` has the signature of
upstream's `simple_knn._C.distCUDA2` -- points (N, 3) -> (N,) the mean squared distance to the
three nearest neighbours -- and is `gsr_knn_mean_dist2` on torch's current stream.

No fallback: importing this module fails when `_native.so` is not built
(`python -c "import __graft_entry__ as g; g.build()"`).
"""
from __future__ import annotations

try:
    from ._native import (abi_version, adamUpdate, densification_stats,  # noqa: F401
                          densify_apply, densify_plan, distCUDA2, fused_adam_step, fused_image_loss, fused_image_loss_backward,
                          fused_image_loss_window, fused_image_loss_window_backward,
                          mark_visible, rasterize_gaussians,
                          rasterize_gaussians_backward, rasterize_gaussians_backward_abs,
                          rasterize_gaussians_backward_ext,
                          rasterize_gaussians_backward_features,
                          rasterize_gaussians_backward_strip_ext, rasterize_gaussians_ext,
                          rasterize_gaussians_features, rasterize_gaussians_shaded)
except ImportError as e:  # pragma: no cover - a build problem, reported loudly
    raise ImportError(f"gaussiansplattingviewer_amd._native is not built or does not load ({e}); "
                      "run __graft_entry__.build()") from e
