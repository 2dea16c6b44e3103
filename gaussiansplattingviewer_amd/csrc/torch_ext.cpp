// torch_ext.cpp -- the thin PyTorch-ROCm C++ extension `gaussiansplattingviewer_amd._C`: the
// native entry points the upstream Python package calls, with upstream's signatures, over the C
// ABI of libgsr.so (include/gsr.h).  No kernels here: every launch happens in libgsr.so, on the
// caller's current HIP stream.
//
//   _C.rasterize_gaussians(bg, means3D, colors_precomp, opacities, scales, rotations,
//                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tanfovx,
//                          tanfovy, image_height, image_width, sh, sh_degree, campos,
//                          prefiltered, debug)
//       -> (num_rendered, color [3,H,W], radii [P], geomBuffer, binningBuffer, imgBuffer)
//     upstream rasterize_points.cu RasterizeGaussiansCUDA, reached from GaussianRasterizer
//     (renderer_cuda.py:211-224) through _RasterizeGaussians.  The three buffers hold upstream's
//     backward state; here they are empty: the backward rebuilds its state from the inputs.
//   _C.rasterize_gaussians_shaded(<the same 19 arguments>, shading) -> the same 6-tuple
//     this package's own: the forward under a GL shading (gsr_forward_shaded, GSR_SHADE_*).
//   _C.rasterize_gaussians_backward(bg, means3D, radii, colors_precomp, scales, rotations,
//                                   scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
//                                   tanfovx, tanfovy, dL_dout_color, sh, sh_degree, campos,
//                                   geomBuffer, R, binningBuffer, imgBuffer, debug, opacities)
//       -> (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales,
//           dL_drotations)
//     upstream RasterizeGaussiansBackwardCUDA's arguments and 8-tuple over gsr_backward, plus one
//     trailing argument: upstream reads the opacities out of geomBuffer, here the state is
//     rebuilt from the inputs.  radii, R and the three buffers are accepted and ignored.
//   _C.rasterize_gaussians_planes(<rasterize_gaussians' 19 arguments>)
//       -> (num_rendered, color, radii, depth_map [H,W], inv_depth_map [H,W], final_T [H,W])
//   _C.rasterize_gaussians_backward_planes(bg, means3D, colors_precomp, opacities, scales,
//                                          rotations, scale_modifier, cov3D_precomp, viewmatrix,
//                                          projmatrix, tanfovx, tanfovy, sh, sh_degree, campos,
//                                          debug, dL_dout_color, dL_ddepth_map,
//                                          dL_dinv_depth_map, dL_dfinal_T) -> the same 8-tuple
//     this package's own (GaussianRasterizationSettings.depth_maps): gsr_forward_depth with
//     final_T, and gsr_backward_planes; an empty gradient tensor is an unused one.
//   _C.rasterize_gaussians_backward_camera(<rasterize_gaussians_backward_planes' 20 arguments>)
//       -> its 8-tuple, then dL_dviewmatrix [4,4], dL_dprojmatrix [4,4], dL_dcampos [3]
//     this package's own: gsr_backward_camera.  The two matrices' gradients are in the inputs'
//     layout (the 16 floats of the input, viewed (4, 4)).
//   _C.rasterize_gaussians_filtered(<rasterize_gaussians' 19 arguments>, antialiasing)
//       -> rasterize_gaussians_planes' 6-tuple
//   _C.rasterize_gaussians_backward_filtered(<rasterize_gaussians_backward_camera's 20
//                                            arguments>, antialiasing) -> its 11-tuple
//     this package's own (GaussianRasterizationSettings.antialiasing): gsr_forward_filtered and
//     gsr_backward_filtered, the effective opacity of the 0.3-pixel dilation's compensation.
//   _C.mark_visible(means3D, viewmatrix, projmatrix) -> bool [P]
//     upstream markVisible (GaussianRasterizer.markVisible).
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <mutex>
#include <tuple>
#include <vector>

#include "gsr.h"

namespace {

// One context per device, created on first use; _lib.context(device, 0) renders with the same
// one (context_handle), so both entry paths share a workspace.
std::mutex g_lock;
std::vector<gsr_context *> g_ctx;

gsr_context *context_for(int device) {
    std::lock_guard<std::mutex> lk(g_lock);
    if ((int)g_ctx.size() <= device) g_ctx.resize(device + 1, nullptr);
    if (!g_ctx[device]) {
        c10::hip::HIPGuard guard(device);
        gsr_context *c = nullptr;
        TORCH_CHECK(gsr_create(&c) == GSR_OK, "gsr_create: ", gsr_last_error());
        g_ctx[device] = c;
    }
    return g_ctx[device];
}

// An input as contiguous float32 on means3D's device (copied there if needed, as the Python
// entry does), or nullptr for an absent (empty) optional input (upstream passes
// torch.Tensor([]) for them).  A present input must hold at least `count` values: the kernels
// read the first `count` (upstream reads campos as a vec3 of whatever it is given, and the
// stereo viewer hands a homogeneous 4-vector).
const float *opt_ptr(const torch::Tensor &t, const torch::Device &dev, const char *name,
                     std::vector<torch::Tensor> &keep, int64_t count) {
    if (!t.defined() || t.numel() == 0) return nullptr;
    TORCH_CHECK(t.numel() >= count, name, " holds ", t.numel(), " values, expected ", count);
    torch::Tensor c = t.to(dev, torch::kFloat32).contiguous();
    keep.push_back(c);
    return c.data_ptr<float>();
}

using Forward6 =
    std::tuple<int64_t, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;

// The per-pixel planes of rasterize_gaussians_planes: depth_map, inv_depth_map, final_T, [H,W] each.
struct Planes {
    torch::Tensor depth_map, inv_depth_map, final_T;
};

// upstream's 19 arguments and the shading (GSR_SHADE_*, gsr_forward_shaded); planes: the splat
// composite through gsr_forward_depth, which also fills them
Forward6 forward_impl(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height,
    int64_t image_width, const torch::Tensor &sh, int64_t degree, const torch::Tensor &campos,
    bool prefiltered, bool debug, int64_t shading, Planes *planes, bool antialiasing = false) {
    if (means3D.ndimension() != 2 || means3D.size(1) != 3)
        AT_ERROR("means3D must have dimensions (num_points, 3)");
    TORCH_CHECK(means3D.is_cuda(), "means3D must be a device (HIP) tensor");
    const torch::Device dev = means3D.device();
    const int64_t P = means3D.size(0);
    const int64_t H = image_height, W = image_width;
    auto f32 = means3D.options().dtype(torch::kFloat32);
    // upstream zero-fills both; the forward writes every pixel and every radius (P > 0), so
    // only an empty scene needs the fill (two fill kernels fewer per frame)
    torch::Tensor color = P ? torch::empty({3, H, W}, f32) : torch::zeros({3, H, W}, f32);
    torch::Tensor radii = P ? torch::empty({P}, means3D.options().dtype(torch::kInt32))
                            : torch::zeros({P}, means3D.options().dtype(torch::kInt32));
    auto bytes = means3D.options().dtype(torch::kUInt8);
    torch::Tensor geom = torch::empty({0}, bytes), binning = torch::empty({0}, bytes),
                  img = torch::empty({0}, bytes);
    int64_t num_rendered = 0;
    if (planes) {  // a pixel that composites nothing: depth 0, inverse depth 0, transmittance 1
        planes->depth_map = P ? torch::empty({H, W}, f32) : torch::zeros({H, W}, f32);
        planes->inv_depth_map = P ? torch::empty({H, W}, f32) : torch::zeros({H, W}, f32);
        planes->final_T = P ? torch::empty({H, W}, f32) : torch::ones({H, W}, f32);
    }
    if (P != 0) {
        std::vector<torch::Tensor> keep;
        gsr_gaussians g{};
        g.P = P;
        g.D = (int32_t)degree;
        g.M = !(sh.defined() && sh.numel() != 0) ? 0
              : sh.dim() == 3                ? (int32_t)sh.size(1)
                                             : (int32_t)(sh.numel() / P / 3);
        g.scale_modifier = (float)scale_modifier;
        g.means3D = opt_ptr(means3D, dev, "means3D", keep, 3 * P);
        g.scales = opt_ptr(scales, dev, "scales", keep, 3 * P);
        g.rotations = opt_ptr(rotations, dev, "rotations", keep, 4 * P);
        g.opacities = opt_ptr(opacity, dev, "opacities", keep, P);
        g.shs = opt_ptr(sh, dev, "sh", keep, 3 * (int64_t)g.M * P);
        g.colors_precomp = opt_ptr(colors, dev, "colors_precomp", keep, 3 * P);
        g.cov3D_precomp = opt_ptr(cov3D_precomp, dev, "cov3D_precomp", keep, 6 * P);
        gsr_raster_settings st{};
        st.image_width = (int32_t)W;
        st.image_height = (int32_t)H;
        st.tanfovx = (float)tan_fovx;
        st.tanfovy = (float)tan_fovy;
        st.viewmatrix = opt_ptr(viewmatrix, dev, "viewmatrix", keep, 16);
        st.projmatrix = opt_ptr(projmatrix, dev, "projmatrix", keep, 16);
        st.campos = opt_ptr(campos, dev, "campos", keep, 3);
        st.bg = opt_ptr(background, dev, "bg", keep, 3);
        st.prefiltered = prefiltered ? 1 : 0;
        st.debug = debug ? 1 : 0;
        gsr_outputs out{};
        out.color = color.data_ptr<float>();
        out.radii = radii.data_ptr<int32_t>();
        c10::hip::HIPGuard guard(dev.index());
        gsr_context *ctx = context_for(dev.index());
        hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
        int rc;
        {  // the forward waits for K (pinned memory): other Python threads may run meanwhile
            pybind11::gil_scoped_release no_gil;
            if (planes) {
                out.final_T = planes->final_T.data_ptr<float>();
                gsr_depth_outputs d{planes->depth_map.data_ptr<float>(),
                                    planes->inv_depth_map.data_ptr<float>()};
                const gsr_filter_settings fs{antialiasing ? 1 : 0};
                rc = antialiasing ? gsr_forward_filtered(ctx, &g, &st, &out, &d, nullptr, &fs, s)
                                  : gsr_forward_depth(ctx, &g, &st, &out, &d, s);
            } else {
                rc = gsr_forward_shaded(ctx, &g, &st, &out, (int32_t)shading, s);
            }
        }
        TORCH_CHECK(rc == GSR_OK, "gsr_forward failed (", rc, "): ", gsr_last_error());
        num_rendered = out.num_rendered;
    }
    return std::make_tuple(num_rendered, color, radii, geom, binning, img);
}

Forward6 rasterize_gaussians_shaded(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height,
    int64_t image_width, const torch::Tensor &sh, int64_t degree, const torch::Tensor &campos,
    bool prefiltered, bool debug, int64_t shading) {
    return forward_impl(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                        cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height,
                        image_width, sh, degree, campos, prefiltered, debug, shading, nullptr);
}

// upstream's 19 arguments -> (num_rendered, color, radii, depth_map, inv_depth_map, final_T)
Forward6 rasterize_gaussians_planes(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height,
    int64_t image_width, const torch::Tensor &sh, int64_t degree, const torch::Tensor &campos,
    bool prefiltered, bool debug) {
    Planes pl;
    Forward6 r = forward_impl(background, means3D, colors, opacity, scales, rotations,
                              scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                              tan_fovy, image_height, image_width, sh, degree, campos, prefiltered,
                              debug, GSR_SHADE_SPLAT, &pl);
    return std::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r), pl.depth_map,
                           pl.inv_depth_map, pl.final_T);
}

Forward6 rasterize_gaussians(const torch::Tensor &background, const torch::Tensor &means3D,
                             const torch::Tensor &colors, const torch::Tensor &opacity,
                             const torch::Tensor &scales, const torch::Tensor &rotations,
                             double scale_modifier, const torch::Tensor &cov3D_precomp,
                             const torch::Tensor &viewmatrix, const torch::Tensor &projmatrix,
                             double tan_fovx, double tan_fovy, int64_t image_height,
                             int64_t image_width, const torch::Tensor &sh, int64_t degree,
                             const torch::Tensor &campos, bool prefiltered, bool debug) {
    return rasterize_gaussians_shaded(background, means3D, colors, opacity, scales, rotations,
                                      scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                      tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                                      campos, prefiltered, debug, GSR_SHADE_SPLAT);
}

using Backward8 = std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                             torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;

// The backward of both entries.  planes (3 tensors: dL_ddepth_map, dL_dinv_depth_map,
// dL_dfinal_T, each [H,W] or empty = unused), or nullptr: gsr_backward.  With a plane gradient
// dL_dout_color may be empty.  camera (3 tensors, written: dL_dviewmatrix [4,4], dL_dprojmatrix
// [4,4], dL_dcampos [3]), or nullptr: with it the call is gsr_backward_camera.
Backward8 backward_impl(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &scales, const torch::Tensor &rotations, double scale_modifier,
    const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy,
    const torch::Tensor &dL_dout_color, const torch::Tensor &sh, int64_t degree,
    const torch::Tensor &campos, bool debug, const torch::Tensor &opacities,
    const torch::Tensor *planes, torch::Tensor *camera = nullptr, bool antialiasing = false) {
    if (means3D.ndimension() != 2 || means3D.size(1) != 3)
        AT_ERROR("means3D must have dimensions (num_points, 3)");
    TORCH_CHECK(means3D.is_cuda(), "means3D must be a device (HIP) tensor");
    const bool has_color = dL_dout_color.defined() && dL_dout_color.numel() != 0;
    int64_t H = 0, W = 0;
    if (has_color || !planes) {
        TORCH_CHECK(dL_dout_color.dim() == 3 && dL_dout_color.size(0) == 3,
                    "dL_dout_color must have dimensions (3, H, W)");
        H = dL_dout_color.size(1), W = dL_dout_color.size(2);
    }
    if (planes) {
        bool any = false;
        for (int i = 0; i < 3; ++i) {
            const torch::Tensor &t = planes[i];
            if (!t.defined() || t.numel() == 0) continue;
            TORCH_CHECK(t.dim() == 2, "a plane gradient must have dimensions (H, W)");
            if (!has_color && !any) H = t.size(0), W = t.size(1);
            TORCH_CHECK(t.size(0) == H && t.size(1) == W,
                        "the image and plane gradients must share (H, W)");
            any = true;
        }
        TORCH_CHECK(any || has_color, "dL_dout_color or a plane gradient is required");
    }
    const torch::Device dev = means3D.device();
    const int64_t P = means3D.size(0);
    const int64_t M = !(sh.defined() && sh.numel() != 0) ? 0
                      : sh.dim() == 3                    ? sh.size(1)
                                                         : (P ? sh.numel() / P / 3 : 0);
    auto f32 = means3D.options().dtype(torch::kFloat32);
    torch::Tensor d_means3D = torch::zeros({P, 3}, f32), d_means2D = torch::zeros({P, 3}, f32);
    torch::Tensor d_colors = torch::zeros({P, 3}, f32), d_opacity = torch::zeros({P, 1}, f32);
    torch::Tensor d_cov3D = torch::zeros({P, 6}, f32), d_sh = torch::zeros({P, M, 3}, f32);
    torch::Tensor d_scales = torch::zeros({P, 3}, f32), d_rot = torch::zeros({P, 4}, f32);
    if (camera) {  // (no Gaussian: zeros)
        camera[0] = torch::zeros({4, 4}, f32), camera[1] = torch::zeros({4, 4}, f32);
        camera[2] = torch::zeros({3}, f32);
    }
    if (P != 0) {
        std::vector<torch::Tensor> keep;
        gsr_gaussians g{};
        g.P = P;
        g.D = (int32_t)degree;
        g.M = (int32_t)M;
        g.scale_modifier = (float)scale_modifier;
        g.means3D = opt_ptr(means3D, dev, "means3D", keep, 3 * P);
        g.scales = opt_ptr(scales, dev, "scales", keep, 3 * P);
        g.rotations = opt_ptr(rotations, dev, "rotations", keep, 4 * P);
        g.opacities = opt_ptr(opacities, dev, "opacities", keep, P);
        g.shs = opt_ptr(sh, dev, "sh", keep, 3 * M * P);
        g.colors_precomp = opt_ptr(colors, dev, "colors_precomp", keep, 3 * P);
        g.cov3D_precomp = opt_ptr(cov3D_precomp, dev, "cov3D_precomp", keep, 6 * P);
        gsr_raster_settings st{};
        st.image_width = (int32_t)W;
        st.image_height = (int32_t)H;
        st.tanfovx = (float)tan_fovx;
        st.tanfovy = (float)tan_fovy;
        st.viewmatrix = opt_ptr(viewmatrix, dev, "viewmatrix", keep, 16);
        st.projmatrix = opt_ptr(projmatrix, dev, "projmatrix", keep, 16);
        st.campos = opt_ptr(campos, dev, "campos", keep, 3);
        st.bg = opt_ptr(background, dev, "bg", keep, 3);
        st.debug = debug ? 1 : 0;
        gsr_backward_inputs in{};
        in.dL_dcolor = opt_ptr(dL_dout_color, dev, "dL_dout_color", keep, 3 * H * W);
        gsr_plane_gradients pg{};
        if (planes) {
            pg.dL_ddepth_map = opt_ptr(planes[0], dev, "dL_ddepth_map", keep, H * W);
            pg.dL_dinv_depth_map = opt_ptr(planes[1], dev, "dL_dinv_depth_map", keep, H * W);
            pg.dL_dfinal_T = opt_ptr(planes[2], dev, "dL_dfinal_T", keep, H * W);
        }
        gsr_gradients gr{};
        gr.dL_dmeans3D = d_means3D.data_ptr<float>();
        gr.dL_dmeans2D = d_means2D.data_ptr<float>();
        gr.dL_dopacity = d_opacity.data_ptr<float>();
        gr.dL_dcolors = d_colors.data_ptr<float>();
        gr.dL_dcov3D = d_cov3D.data_ptr<float>();
        if (g.shs) gr.dL_dsh = d_sh.data_ptr<float>();
        if (g.scales) {
            gr.dL_dscales = d_scales.data_ptr<float>();
            gr.dL_drotations = d_rot.data_ptr<float>();
        }
        c10::hip::HIPGuard guard(dev.index());
        gsr_context *ctx = context_for(dev.index());
        hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
        int rc;
        {  // the rebuild waits for K (pinned memory), as the forward does
            pybind11::gil_scoped_release no_gil;
            if (camera) {
                const gsr_camera_gradients cg{camera[0].data_ptr<float>(),
                                              camera[1].data_ptr<float>(),
                                              camera[2].data_ptr<float>()};
                const gsr_filter_settings fs{antialiasing ? 1 : 0};
                rc = antialiasing
                         ? gsr_backward_filtered(ctx, &g, &st, &in, planes ? &pg : nullptr, &cg,
                                                 &fs, &gr, s)
                         : gsr_backward_camera(ctx, &g, &st, &in, planes ? &pg : nullptr, &cg, &gr,
                                               s);
            } else {
                rc = planes ? gsr_backward_planes(ctx, &g, &st, &in, &pg, &gr, s)
                            : gsr_backward(ctx, &g, &st, &in, &gr, s);
            }
        }
        TORCH_CHECK(rc == GSR_OK, "gsr_backward failed (", rc, "): ", gsr_last_error());
    }
    return std::make_tuple(d_means2D, d_colors, d_opacity, d_means3D, d_cov3D, d_sh, d_scales,
                           d_rot);
}

Backward8 rasterize_gaussians_backward(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &radii,
    const torch::Tensor &colors, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy,
    const torch::Tensor &dL_dout_color, const torch::Tensor &sh, int64_t degree,
    const torch::Tensor &campos, const torch::Tensor &geomBuffer, int64_t R,
    const torch::Tensor &binningBuffer, const torch::Tensor &imageBuffer, bool debug,
    const torch::Tensor &opacities) {
    (void)radii, (void)geomBuffer, (void)R, (void)binningBuffer, (void)imageBuffer;
    return backward_impl(background, means3D, colors, scales, rotations, scale_modifier,
                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                         sh, degree, campos, debug, opacities, nullptr);
}

// This package's own: the forward's inputs in rasterize_gaussians' order (opacities in place),
// then the four gradients of rasterize_gaussians_planes' image-like outputs (empty = unused).
Backward8 rasterize_gaussians_backward_planes(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacities, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, const torch::Tensor &sh,
    int64_t degree, const torch::Tensor &campos, bool debug, const torch::Tensor &dL_dout_color,
    const torch::Tensor &dL_ddepth_map, const torch::Tensor &dL_dinv_depth_map,
    const torch::Tensor &dL_dfinal_T) {
    const torch::Tensor planes[3] = {dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T};
    return backward_impl(background, means3D, colors, scales, rotations, scale_modifier,
                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                         sh, degree, campos, debug, opacities, planes);
}

// rasterize_gaussians_backward_planes with the camera's gradients after its 8-tuple.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor>
rasterize_gaussians_backward_camera(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacities, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, const torch::Tensor &sh,
    int64_t degree, const torch::Tensor &campos, bool debug, const torch::Tensor &dL_dout_color,
    const torch::Tensor &dL_ddepth_map, const torch::Tensor &dL_dinv_depth_map,
    const torch::Tensor &dL_dfinal_T) {
    const torch::Tensor planes[3] = {dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T};
    torch::Tensor camera[3];
    const Backward8 g = backward_impl(background, means3D, colors, scales, rotations,
                                      scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                      tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, debug,
                                      opacities, planes, camera);
    return std::tuple_cat(g, std::make_tuple(camera[0], camera[1], camera[2]));
}

// rasterize_gaussians_planes with the antialiasing option (gsr_forward_filtered).
Forward6 rasterize_gaussians_filtered(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height,
    int64_t image_width, const torch::Tensor &sh, int64_t degree, const torch::Tensor &campos,
    bool prefiltered, bool debug, bool antialiasing) {
    Planes pl;
    Forward6 r = forward_impl(background, means3D, colors, opacity, scales, rotations,
                              scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                              tan_fovy, image_height, image_width, sh, degree, campos, prefiltered,
                              debug, GSR_SHADE_SPLAT, &pl, antialiasing);
    return std::make_tuple(std::get<0>(r), std::get<1>(r), std::get<2>(r), pl.depth_map,
                           pl.inv_depth_map, pl.final_T);
}

// rasterize_gaussians_backward_camera with the antialiasing option (gsr_backward_filtered).
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
           torch::Tensor>
rasterize_gaussians_backward_filtered(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacities, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, const torch::Tensor &sh,
    int64_t degree, const torch::Tensor &campos, bool debug, const torch::Tensor &dL_dout_color,
    const torch::Tensor &dL_ddepth_map, const torch::Tensor &dL_dinv_depth_map,
    const torch::Tensor &dL_dfinal_T, bool antialiasing) {
    const torch::Tensor planes[3] = {dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T};
    torch::Tensor camera[3];
    const Backward8 g = backward_impl(background, means3D, colors, scales, rotations,
                                      scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
                                      tan_fovx, tan_fovy, dL_dout_color, sh, degree, campos, debug,
                                      opacities, planes, camera, antialiasing);
    return std::tuple_cat(g, std::make_tuple(camera[0], camera[1], camera[2]));
}

torch::Tensor mark_visible(const torch::Tensor &means3D, const torch::Tensor &viewmatrix,
                           const torch::Tensor &projmatrix) {
    TORCH_CHECK(means3D.is_cuda(), "means3D must be a device (HIP) tensor");
    const torch::Device dev = means3D.device();
    const int64_t P = means3D.size(0);
    torch::Tensor present = torch::full({P}, false, means3D.options().dtype(torch::kBool));
    if (P != 0) {
        std::vector<torch::Tensor> keep;
        const float *xyz = opt_ptr(means3D, dev, "means3D", keep, 3 * P);
        const float *view = opt_ptr(viewmatrix, dev, "viewmatrix", keep, 16);
        const float *proj = opt_ptr(projmatrix, dev, "projmatrix", keep, 16);
        c10::hip::HIPGuard guard(dev.index());
        gsr_context *ctx = context_for(dev.index());
        hipStream_t s = c10::hip::getCurrentHIPStream(dev.index()).stream();
        const int rc = gsr_mark_visible(ctx, xyz, P, view, proj,
                                        reinterpret_cast<uint8_t *>(present.data_ptr<bool>()), s);
        TORCH_CHECK(rc == GSR_OK, "gsr_mark_visible failed (", rc, "): ", gsr_last_error());
    }
    return present;
}

void release_contexts() {
    std::lock_guard<std::mutex> lk(g_lock);
    for (gsr_context *&c : g_ctx) {
        if (c) gsr_destroy(c);
        c = nullptr;
    }
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
    m.doc() = "gaussiansplattingviewer_amd native entry points (upstream _C signatures) over libgsr.so";
    m.def("rasterize_gaussians", &rasterize_gaussians,
          "upstream RasterizeGaussiansCUDA: (num_rendered, color, radii, geomBuffer, "
          "binningBuffer, imgBuffer)");
    m.def("rasterize_gaussians_shaded", &rasterize_gaussians_shaded,
          "rasterize_gaussians under a GL shading: its 19 arguments, then GSR_SHADE_* (0 splat, "
          "1 billboard, 2 flat ball, 3 gaussian ball)");
    m.def("rasterize_gaussians_backward", &rasterize_gaussians_backward,
          "upstream RasterizeGaussiansBackwardCUDA: its 21 arguments, then opacities -> "
          "(dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_dsh, dL_dscales, "
          "dL_drotations)");
    m.def("rasterize_gaussians_planes", &rasterize_gaussians_planes,
          "rasterize_gaussians' 19 arguments -> (num_rendered, color, radii, depth_map, "
          "inv_depth_map, final_T): the splat composite with its per-pixel planes");
    m.def("rasterize_gaussians_backward_planes", &rasterize_gaussians_backward_planes,
          "bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, "
          "cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, sh, sh_degree, campos, debug, "
          "dL_dout_color, dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T (empty = unused) -> "
          "rasterize_gaussians_backward's 8-tuple");
    m.def("rasterize_gaussians_backward_camera", &rasterize_gaussians_backward_camera,
          "rasterize_gaussians_backward_planes' 20 arguments -> its 8-tuple, then dL_dviewmatrix "
          "(4, 4), dL_dprojmatrix (4, 4), dL_dcampos (3)");
    m.def("rasterize_gaussians_filtered", &rasterize_gaussians_filtered,
          "rasterize_gaussians' 19 arguments, then antialiasing -> rasterize_gaussians_planes' "
          "6-tuple (gsr_forward_filtered)");
    m.def("rasterize_gaussians_backward_filtered", &rasterize_gaussians_backward_filtered,
          "rasterize_gaussians_backward_camera's 20 arguments, then antialiasing -> its 11-tuple "
          "(gsr_backward_filtered)");
    m.def("mark_visible", &mark_visible, "upstream markVisible: bool[P]");
    m.def("abi_version", []() { return gsr_abi_version(); });
    m.def(
        "context_handle",
        [](int64_t device) { return (uintptr_t)context_for((int)device); },
        "the device's gsr_context (as an address), created on first use");
    m.def("release_contexts", &release_contexts, "destroy every context (process exit)");
}
