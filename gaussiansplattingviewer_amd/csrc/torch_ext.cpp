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
//   _C.rasterize_gaussians_ext(<rasterize_gaussians' 19 arguments>, shading, planes, antialiasing,
//                              tile_row_begin = 0, tile_row_end = 0)
//       -> (num_rendered, color, radii, depth_map [H,W], inv_depth_map [H,W], final_T [H,W])
//     this package's own, every forward in one entry (GaussianRasterizationSettings.shading,
//     .depth_maps, .antialiasing).  A shading: gsr_forward_shaded.  The splat composite:
//     gsr_forward_features without features, with the depth planes and final_T only if `planes`
//     (without, the three tensors are empty and nothing of them is rendered) and a filter only if
//     `antialiasing` (the effective opacity of the 0.3-pixel dilation's compensation).  With a
//     strip of tile rows (the two trailing arguments, not both 0; they may be left out) the image
//     and the planes are strip-local, [3, rows, W] and [rows, W], rows = min(H, 16 end) - 16 begin.
//   _C.rasterize_gaussians_backward_ext(bg, means3D, colors_precomp, opacities, scales, rotations,
//                                       scale_modifier, cov3D_precomp, viewmatrix, projmatrix,
//                                       tanfovx, tanfovy, sh, sh_degree, campos, debug,
//                                       dL_dout_color, dL_ddepth_map, dL_dinv_depth_map,
//                                       dL_dfinal_T, camera, antialiasing,
//                                       deterministic = False)
//       -> rasterize_gaussians_backward's 8-tuple, then dL_dviewmatrix [4,4], dL_dprojmatrix
//          [4,4], dL_dcampos [3] (empty without `camera`)
//     this package's own, every backward in one entry: gsr_backward_features without features
//     (which is every entry below it), with the plane gradients only if one of the three is not
//     empty (an empty gradient tensor is an unused one), the camera's only if `camera`, a filter
//     only if `antialiasing`; with `deterministic` the gradients have the same bits on every call
//     (the trailing argument may be left out: the 22-argument call is unchanged).  The two matrices'
//     gradients are in the inputs' layout (the 16 floats of the input, viewed (4, 4)).
//   _C.rasterize_gaussians_backward_strip_ext(<rasterize_gaussians_backward_ext's 23 arguments>,
//                                             tile_row_begin, tile_row_end, image_height)
//       -> the same 11-tuple
//     this package's own: the same call on a strip of tile rows (not both 0; gsr_backward_strip's
//     request) in either mode.  The image and plane gradients are strip-local, [3, rows, W] and [rows, W], and
//     image_height gives the frame's height, which they no longer tell; the gradients stay
//     whole-scene.  (An entry of its own: rasterize_gaussians_backward_ext keeps its signature.)
//   _C.rasterize_gaussians_features(<rasterize_gaussians' 19 arguments>, planes, antialiasing,
//                                   tile_row_begin, tile_row_end, features)
//       -> rasterize_gaussians_ext's 6-tuple, then feature_map [C, rows, W]
//     this package's own: gsr_forward_features, the splat composite with C channels of the
//     caller's own per Gaussian (features [P, C], 1 <= C <= GSR_MAX_FEATURES) composited under the
//     colour's weights.  (An entry of its own: the entries above keep their signatures.)
//   _C.rasterize_gaussians_backward_features(<rasterize_gaussians_backward_ext's 23 arguments>,
//                                            tile_row_begin, tile_row_end, image_height, features,
//                                            dL_dfeature_map)
//       -> the 11-tuple, then dL_dfeatures [P, C]
//     this package's own: gsr_backward_features; tile rows (0, 0) for a whole frame (image_height
//     is then not read); dL_dout_color may be empty.  `deterministic` is refused by the library.
//   _C.mark_visible(means3D, viewmatrix, projmatrix) -> bool [P]
//     upstream markVisible (GaussianRasterizer.markVisible).
//   _C.fused_image_loss(image, target, lambda_dssim, need_saved) -> (values [3], saved)
//     this package's own: gsr_image_loss, the fused L1 + D-SSIM loss of two contiguous float32
//     [C, H, W] device images; values = (loss, l1, ssim), saved = [3, C, H, W] for the backward,
//     empty (and not computed) without `need_saved`.  No context is involved.
//   _C.fused_image_loss_backward(image, target, lambda_dssim, saved, dL_dloss) -> dL_dimage
//     gsr_image_loss_backward; dL_dloss is a one-element device tensor (read on the device, no
//     host wait) or empty for 1.0.
//   _C.fused_image_loss_window(image, target, frame_H, row0, own_begin, own_end, lambda_dssim,
//                              need_saved) -> (values [3], saved)
//     gsr_image_loss_window: the frame's loss on the rows [own_begin, own_end) of a frame of
//     frame_H rows, from the band buffers image / target [C, rows, W] whose row 0 is frame row
//     row0; values = the window's shares, saved = [3, C, A, W] over the apron (own rows +- 5,
//     clipped to the frame), empty without `need_saved`.
//   _C.fused_image_loss_window_backward(image, target, frame_H, row0, own_begin, own_end,
//                                       lambda_dssim, saved, dL_dloss) -> dL_dimage
//     gsr_image_loss_window_backward: the frame loss's gradient on the own rows,
//     [C, own_end - own_begin, W].
//   _C.adamUpdate(param, grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M)
//     upstream's fused sparse Adam (SparseGaussianAdam): gsr_adam_step on one [N, M] group, in
//     place, for the rows whose `visible` (bool or uint8 [N]) is set; no bias correction.
//   _C.fused_adam_step(params, grads, exp_avgs, exp_avg_sqs, lrs, epss, mask, b1, b2, bc1,
//                      bc2_sqrt)
//     this package's own: gsr_adam_step on 1..GSR_MAX_PARAM_GROUPS groups [P, M_i] in ONE launch,
//     in place.  mask: bool / uint8 [P] (visible), int32 [P] (radii, > 0 = update) or empty
//     (every row).  bc1, bc2_sqrt: 1 - b1^t and sqrt(1 - b2^t), or 1.0 for upstream's form.
//   _C.densification_stats(radii, means2D_grad, grad_accum, denom, max_radii)
//     gsr_densify_stats, upstream's add_densification_stats in place; max_radii int32 [P] or
//     empty.  None of the three uses a context.
//   _C.densify_plan(grad_accum, denom, max_radii, scaling, opacity, thresholds, radius_threshold,
//                   scale_space, workspace, counts)
//     gsr_densify_plan into the caller's int32 workspace and counts [4]; thresholds = (grad, scale
//     split, opacity prune, scale prune) in the tensors' stored space, max_radii int32 [P] or empty.
//   _C.densify_apply(<the same first eight>, seed, roles, has_moments, src_params, src_exp_avgs,
//                    src_exp_avg_sqs, dst_params, dst_exp_avgs, dst_exp_avg_sqs, workspace,
//                    source_index)
//     gsr_densify_apply into the caller's dst tensors [P_out, M_i] and source_index [P_out]
//     (int32; its length is P_out).  No context, no allocation, no synchronisation.
//   _C.distCUDA2(points) -> float32 [N]
//     upstream's simple_knn entry (scene/gaussian_model.py create_from_pcd): the mean squared
//     distance of every point of points [N, 3] to its three nearest neighbours,
//     gsr_knn_mean_dist2 on torch's current stream; torch allocates the result and the workspace.
#include <torch/extension.h>

#include <c10/hip/HIPGuard.h>
#include <c10/hip/HIPStream.h>

#include <algorithm>
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
using Backward8 = std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor,
                             torch::Tensor, torch::Tensor, torch::Tensor, torch::Tensor>;
using Backward11 = decltype(std::tuple_cat(
    Backward8(), std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>()));

// The inputs the forward and the backward share, in rasterize_gaussians' order.
struct Inputs {
    const torch::Tensor &background, &means3D, &colors, &opacities, &scales, &rotations;
    double scale_modifier;
    const torch::Tensor &cov3D_precomp, &viewmatrix, &projmatrix;
    double tan_fovx, tan_fovy;
    const torch::Tensor &sh;
    int64_t degree;
    const torch::Tensor &campos;
    bool prefiltered, debug;
};

// ... parsed: means3D's checks, P and the SH coefficients stored per Gaussian (M); fill() makes
// the two structs of a call on P > 0 Gaussians, whose pointers `keep` keeps alive.
struct Scene {
    const Inputs &in;
    torch::Device dev;
    int64_t P, M;
    gsr_gaussians g{};
    gsr_raster_settings st{};
    std::vector<torch::Tensor> keep;

    explicit Scene(const Inputs &i) : in(i), dev(i.means3D.device()) {
        if (in.means3D.ndimension() != 2 || in.means3D.size(1) != 3)
            AT_ERROR("means3D must have dimensions (num_points, 3)");
        TORCH_CHECK(in.means3D.is_cuda(), "means3D must be a device (HIP) tensor");
        P = in.means3D.size(0);
        M = !(in.sh.defined() && in.sh.numel() != 0) ? 0
            : in.sh.dim() == 3                       ? in.sh.size(1)
                                                     : (P ? in.sh.numel() / P / 3 : 0);
    }

    void fill(int64_t H, int64_t W) {
        g.P = P;
        g.D = (int32_t)in.degree;
        g.M = (int32_t)M;
        g.scale_modifier = (float)in.scale_modifier;
        g.means3D = opt_ptr(in.means3D, dev, "means3D", keep, 3 * P);
        g.scales = opt_ptr(in.scales, dev, "scales", keep, 3 * P);
        g.rotations = opt_ptr(in.rotations, dev, "rotations", keep, 4 * P);
        g.opacities = opt_ptr(in.opacities, dev, "opacities", keep, P);
        g.shs = opt_ptr(in.sh, dev, "sh", keep, 3 * M * P);
        g.colors_precomp = opt_ptr(in.colors, dev, "colors_precomp", keep, 3 * P);
        g.cov3D_precomp = opt_ptr(in.cov3D_precomp, dev, "cov3D_precomp", keep, 6 * P);
        st.image_width = (int32_t)W;
        st.image_height = (int32_t)H;
        st.tanfovx = (float)in.tan_fovx;
        st.tanfovy = (float)in.tan_fovy;
        st.viewmatrix = opt_ptr(in.viewmatrix, dev, "viewmatrix", keep, 16);
        st.projmatrix = opt_ptr(in.projmatrix, dev, "projmatrix", keep, 16);
        st.campos = opt_ptr(in.campos, dev, "campos", keep, 3);
        st.bg = opt_ptr(in.background, dev, "bg", keep, 3);
        st.prefiltered = in.prefiltered ? 1 : 0;
        st.debug = in.debug ? 1 : 0;
    }
};

// Every forward: (num_rendered, color, radii, depth_map, inv_depth_map, final_T), the three
// planes empty without `planes`.
// rows of the strip [rb, re) of a frame H pixels high (0, 0: the frame); checks the strip
int64_t strip_rows(int64_t H, int64_t rb, int64_t re) {
    if (rb == 0 && re == 0) return H;
    TORCH_CHECK(H > 0 && 0 <= rb && rb < re && re <= (H + 15) / 16, "tile rows (", rb, ", ", re,
                ") outside [0, ", (H + 15) / 16, "]");
    return std::min(H, 16 * re) - 16 * rb;
}

// features [P, C] as the library reads it (contiguous float32 on the scene's device); checks the
// shape and C
torch::Tensor feature_rows(const torch::Tensor &features, const Scene &sc) {
    TORCH_CHECK(features.defined() && features.dim() == 2 && features.size(0) == sc.P,
                "features must have dimensions (num_points, C) = (", sc.P, ", C)");
    TORCH_CHECK(features.size(1) >= 1 && features.size(1) <= GSR_MAX_FEATURES, "features: C = ",
                features.size(1), " outside 1..", GSR_MAX_FEATURES);
    return features.to(sc.dev, torch::kFloat32).contiguous();
}

// features / feature_map: gsr_forward_features' (both NULL: none); feature_map is allocated here.
Forward6 forward_impl(const Inputs &in, int64_t frame_H, int64_t W, int64_t shading, bool planes,
                      bool antialiasing, int64_t tile_row_begin = 0, int64_t tile_row_end = 0,
                      const torch::Tensor *features = nullptr,
                      torch::Tensor *feature_map = nullptr) {
    Scene sc(in);
    // (the outputs are strip-local: H rows from here on)
    const int64_t H = strip_rows(frame_H, tile_row_begin, tile_row_end);
    TORCH_CHECK(shading == GSR_SHADE_SPLAT || (!planes && !antialiasing),
                "the planes and antialiasing belong to the splat composite: not available with "
                "shading ", shading);
    const int64_t P = sc.P;
    auto f32 = in.means3D.options().dtype(torch::kFloat32);
    auto i32 = in.means3D.options().dtype(torch::kInt32);
    // upstream zero-fills both; the forward writes every pixel and every radius (P > 0), so
    // only an empty scene needs the fill (two fill kernels fewer per frame)
    torch::Tensor color = P ? torch::empty({3, H, W}, f32) : torch::zeros({3, H, W}, f32);
    torch::Tensor radii = P ? torch::empty({P}, i32) : torch::zeros({P}, i32);
    torch::Tensor depth_map = torch::empty({0}, f32), inv_depth_map = depth_map,
                  final_T = depth_map;
    if (planes) {  // a pixel that composites nothing: depth 0, inverse depth 0, transmittance 1
        depth_map = P ? torch::empty({H, W}, f32) : torch::zeros({H, W}, f32);
        inv_depth_map = P ? torch::empty({H, W}, f32) : torch::zeros({H, W}, f32);
        final_T = P ? torch::empty({H, W}, f32) : torch::ones({H, W}, f32);
    }
    torch::Tensor rows_f;
    if (features) {  // (a pixel that composites nothing: 0)
        rows_f = feature_rows(*features, sc);
        *feature_map = P ? torch::empty({rows_f.size(1), H, W}, f32)
                         : torch::zeros({rows_f.size(1), H, W}, f32);
    }
    int64_t num_rendered = 0;
    if (P != 0) {
        sc.fill(frame_H, W);
        sc.st.tile_row_begin = (int32_t)tile_row_begin;
        sc.st.tile_row_end = (int32_t)tile_row_end;
        gsr_feature_outputs fo{};
        if (features)
            fo = {(int32_t)rows_f.size(1), rows_f.data_ptr<float>(),
                  feature_map->data_ptr<float>()};
        gsr_outputs out{};
        out.color = color.data_ptr<float>();
        out.radii = radii.data_ptr<int32_t>();
        gsr_depth_outputs d{};
        if (planes) {
            out.final_T = final_T.data_ptr<float>();
            d = {depth_map.data_ptr<float>(), inv_depth_map.data_ptr<float>()};
        }
        const gsr_filter_settings fs{1};
        c10::hip::HIPGuard guard(sc.dev.index());
        gsr_context *ctx = context_for(sc.dev.index());
        hipStream_t s = c10::hip::getCurrentHIPStream(sc.dev.index()).stream();
        int rc;
        {  // the forward waits for K (pinned memory): other Python threads may run meanwhile
            pybind11::gil_scoped_release no_gil;
            // (gsr_forward_features with NULLs is every splat forward below it)
            rc = shading != GSR_SHADE_SPLAT
                     ? gsr_forward_shaded(ctx, &sc.g, &sc.st, &out, (int32_t)shading, s)
                     : gsr_forward_features(ctx, &sc.g, &sc.st, &out, planes ? &d : nullptr,
                                            nullptr, antialiasing ? &fs : nullptr,
                                            features ? &fo : nullptr, s);
        }
        TORCH_CHECK(rc == GSR_OK, "gsr_forward failed (", rc, "): ", gsr_last_error());
        num_rendered = out.num_rendered;
    }
    return std::make_tuple(num_rendered, color, radii, depth_map, inv_depth_map, final_T);
}

Forward6 rasterize_gaussians_ext(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height,
    int64_t image_width, const torch::Tensor &sh, int64_t degree, const torch::Tensor &campos,
    bool prefiltered, bool debug, int64_t shading, bool planes, bool antialiasing,
    int64_t tile_row_begin, int64_t tile_row_end) {
    return forward_impl({background, means3D, colors, opacity, scales, rotations, scale_modifier,
                         cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, sh, degree,
                         campos, prefiltered, debug},
                        image_height, image_width, shading, planes, antialiasing, tile_row_begin,
                        tile_row_end);
}

using Forward7 = decltype(std::tuple_cat(Forward6(), std::tuple<torch::Tensor>()));
Forward7 rasterize_gaussians_features(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height,
    int64_t image_width, const torch::Tensor &sh, int64_t degree, const torch::Tensor &campos,
    bool prefiltered, bool debug, bool planes, bool antialiasing, int64_t tile_row_begin,
    int64_t tile_row_end, const torch::Tensor &features) {
    torch::Tensor feature_map;
    Forward6 r = forward_impl({background, means3D, colors, opacity, scales, rotations,
                               scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                               tan_fovy, sh, degree, campos, prefiltered, debug},
                              image_height, image_width, GSR_SHADE_SPLAT, planes, antialiasing,
                              tile_row_begin, tile_row_end, &features, &feature_map);
    return std::tuple_cat(r, std::make_tuple(feature_map));
}

// ... with upstream's three buffers in the planes' place.  They hold upstream's backward state;
// here they are empty: the backward rebuilds its state from the inputs.
Forward6 rasterize_gaussians_shaded(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacity, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, int64_t image_height,
    int64_t image_width, const torch::Tensor &sh, int64_t degree, const torch::Tensor &campos,
    bool prefiltered, bool debug, int64_t shading) {
    Forward6 r = forward_impl({background, means3D, colors, opacity, scales, rotations,
                               scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                               tan_fovy, sh, degree, campos, prefiltered, debug},
                              image_height, image_width, shading, false, false);
    auto bytes = means3D.options().dtype(torch::kUInt8);
    std::get<3>(r) = torch::empty({0}, bytes);
    std::get<4>(r) = torch::empty({0}, bytes);
    std::get<5>(r) = torch::empty({0}, bytes);
    return r;
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

// Every backward.  planes: dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T, each [H,W] or empty =
// unused; with one of them dL_dout_color may be empty.  upstream: rasterize_gaussians_backward,
// which takes no plane gradient and is gsr_backward itself.
Backward11 backward_impl(const Inputs &in, const torch::Tensor &dL_dout_color,
                         const torch::Tensor (&planes)[3], bool camera, bool antialiasing,
                         bool upstream = false, bool deterministic = false,
                         int64_t tile_row_begin = 0, int64_t tile_row_end = 0,
                         int64_t image_height = 0, const torch::Tensor *features = nullptr,
                         const torch::Tensor *dL_dfeature_map = nullptr,
                         torch::Tensor *dL_dfeatures = nullptr,
                         torch::Tensor *dL_dmeans2D_abs = nullptr) {
    Scene sc(in);
    const bool strip = tile_row_begin != 0 || tile_row_end != 0;
    const bool has_color = dL_dout_color.defined() && dL_dout_color.numel() != 0;
    int64_t H = 0, W = 0;
    if (has_color || upstream) {
        TORCH_CHECK(dL_dout_color.dim() == 3 && dL_dout_color.size(0) == 3,
                    "dL_dout_color must have dimensions (3, H, W)");
        H = dL_dout_color.size(1), W = dL_dout_color.size(2);
    }
    bool any = false;
    for (const torch::Tensor &t : planes) {
        if (!t.defined() || t.numel() == 0) continue;
        TORCH_CHECK(t.dim() == 2, "a plane gradient must have dimensions (H, W)");
        if (!has_color && !any) H = t.size(0), W = t.size(1);
        TORCH_CHECK(t.size(0) == H && t.size(1) == W,
                    "the image and plane gradients must share (H, W)");
        any = true;
    }
    torch::Tensor rows_f;
    if (features) {  // gsr_backward_features: the feature planes' gradient, [C, H, W]
        rows_f = feature_rows(*features, sc);
        const torch::Tensor &t = *dL_dfeature_map;
        TORCH_CHECK(t.defined() && t.dim() == 3 && t.size(0) == rows_f.size(1),
                    "dL_dfeature_map must have dimensions (C, H, W) = (", rows_f.size(1),
                    ", H, W)");
        if (!has_color && !any) H = t.size(1), W = t.size(2);
        TORCH_CHECK(t.size(1) == H && t.size(2) == W,
                    "the image, plane and feature gradients must share (H, W)");
    }
    TORCH_CHECK(any || has_color || upstream || features,
                "dL_dout_color or a plane gradient is required");
    // a strip: H so far is the strip's rows, which must be those of the frame's strip
    const int64_t frame_H = strip ? image_height : H;
    TORCH_CHECK(strip_rows(frame_H, tile_row_begin, tile_row_end) == H,
                "the image and plane gradients of tile rows (", tile_row_begin, ", ", tile_row_end,
                ") of a frame ", frame_H, " px high must have ",
                strip_rows(frame_H, tile_row_begin, tile_row_end), " rows, got ", H);
    const int64_t P = sc.P, M = sc.M;
    auto f32 = in.means3D.options().dtype(torch::kFloat32);
    torch::Tensor d_means3D = torch::zeros({P, 3}, f32), d_means2D = torch::zeros({P, 3}, f32);
    torch::Tensor d_colors = torch::zeros({P, 3}, f32), d_opacity = torch::zeros({P, 1}, f32);
    torch::Tensor d_cov3D = torch::zeros({P, 6}, f32), d_sh = torch::zeros({P, M, 3}, f32);
    torch::Tensor d_scales = torch::zeros({P, 3}, f32), d_rot = torch::zeros({P, 4}, f32);
    torch::Tensor d_view = torch::empty({0}, f32), d_proj = d_view, d_campos = d_view;
    if (camera) {  // (no Gaussian: zeros)
        d_view = torch::zeros({4, 4}, f32), d_proj = torch::zeros({4, 4}, f32);
        d_campos = torch::zeros({3}, f32);
    }
    if (features) *dL_dfeatures = torch::zeros({P, rows_f.size(1)}, f32);
    if (dL_dmeans2D_abs) *dL_dmeans2D_abs = torch::zeros({P, 3}, f32);
    if (P != 0) {
        sc.fill(frame_H, W);
        sc.st.tile_row_begin = (int32_t)tile_row_begin;
        sc.st.tile_row_end = (int32_t)tile_row_end;
        std::vector<torch::Tensor> &keep = sc.keep;
        gsr_feature_gradients fg{};
        if (features)
            fg = {(int32_t)rows_f.size(1), rows_f.data_ptr<float>(),
                  opt_ptr(*dL_dfeature_map, sc.dev, "dL_dfeature_map", keep,
                          rows_f.size(1) * H * W),
                  dL_dfeatures->data_ptr<float>()};
        gsr_backward_inputs bi{};
        bi.dL_dcolor = opt_ptr(dL_dout_color, sc.dev, "dL_dout_color", keep, 3 * H * W);
        gsr_plane_gradients pg{};
        pg.dL_ddepth_map = opt_ptr(planes[0], sc.dev, "dL_ddepth_map", keep, H * W);
        pg.dL_dinv_depth_map = opt_ptr(planes[1], sc.dev, "dL_dinv_depth_map", keep, H * W);
        pg.dL_dfinal_T = opt_ptr(planes[2], sc.dev, "dL_dfinal_T", keep, H * W);
        gsr_camera_gradients cg{};
        if (camera)
            cg = {d_view.data_ptr<float>(), d_proj.data_ptr<float>(), d_campos.data_ptr<float>()};
        const gsr_filter_settings fs{1};
        const gsr_backward_order order{deterministic ? 1 : 0};
        gsr_gradients gr{};
        gr.dL_dmeans3D = d_means3D.data_ptr<float>();
        gr.dL_dmeans2D = d_means2D.data_ptr<float>();
        gr.dL_dopacity = d_opacity.data_ptr<float>();
        gr.dL_dcolors = d_colors.data_ptr<float>();
        gr.dL_dcov3D = d_cov3D.data_ptr<float>();
        if (sc.g.shs) gr.dL_dsh = d_sh.data_ptr<float>();
        if (sc.g.scales) {
            gr.dL_dscales = d_scales.data_ptr<float>();
            gr.dL_drotations = d_rot.data_ptr<float>();
        }
        c10::hip::HIPGuard guard(sc.dev.index());
        gsr_context *ctx = context_for(sc.dev.index());
        hipStream_t s = c10::hip::getCurrentHIPStream(sc.dev.index()).stream();
        int rc;
        {  // the rebuild waits for K (pinned memory), as the forward does
            pybind11::gil_scoped_release no_gil;
            if (upstream && !features)
                rc = gsr_backward(ctx, &sc.g, &sc.st, &bi, &gr, s);
            else if (dL_dmeans2D_abs) {  // gsr_backward_abs: the entry below and one more output
                const gsr_abs_gradients ag{dL_dmeans2D_abs->data_ptr<float>()};
                rc = gsr_backward_abs(ctx, &sc.g, &sc.st, &bi, any ? &pg : nullptr,
                                      camera ? &cg : nullptr, antialiasing ? &fs : nullptr, &order,
                                      features ? &fg : nullptr, &ag, &gr, s);
            } else  // with NULLs and a 0 every entry below it; refuses deterministic with features
                rc = gsr_backward_features(ctx, &sc.g, &sc.st, &bi, any ? &pg : nullptr,
                                           camera ? &cg : nullptr, antialiasing ? &fs : nullptr,
                                           &order, features ? &fg : nullptr, &gr, s);
        }
        TORCH_CHECK(rc == GSR_OK, "gsr_backward failed (", rc, "): ", gsr_last_error());
    }
    return std::make_tuple(d_means2D, d_colors, d_opacity, d_means3D, d_cov3D, d_sh, d_scales,
                           d_rot, d_view, d_proj, d_campos);
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
    const torch::Tensor none[3];
    auto [d_means2D, d_colors, d_opacity, d_means3D, d_cov3D, d_sh, d_scales, d_rot, d_view,
          d_proj, d_campos] =
        backward_impl({background, means3D, colors, opacities, scales, rotations, scale_modifier,
                       cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, sh, degree,
                       campos, false, debug},
                      dL_dout_color, none, false, false, true);
    return std::make_tuple(d_means2D, d_colors, d_opacity, d_means3D, d_cov3D, d_sh, d_scales,
                           d_rot);
}

// The forward's inputs in rasterize_gaussians' order (opacities in place), then the four
// gradients of rasterize_gaussians_ext's image-like outputs (empty = unused).
Backward11 rasterize_gaussians_backward_ext(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacities, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, const torch::Tensor &sh,
    int64_t degree, const torch::Tensor &campos, bool debug, const torch::Tensor &dL_dout_color,
    const torch::Tensor &dL_ddepth_map, const torch::Tensor &dL_dinv_depth_map,
    const torch::Tensor &dL_dfinal_T, bool camera, bool antialiasing, bool deterministic) {
    const torch::Tensor planes[3] = {dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T};
    return backward_impl({background, means3D, colors, opacities, scales, rotations,
                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                          sh, degree, campos, false, debug},
                         dL_dout_color, planes, camera, antialiasing, false, deterministic);
}

// ... on a strip of tile rows of a frame image_height pixels high.
Backward11 rasterize_gaussians_backward_strip_ext(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacities, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, const torch::Tensor &sh,
    int64_t degree, const torch::Tensor &campos, bool debug, const torch::Tensor &dL_dout_color,
    const torch::Tensor &dL_ddepth_map, const torch::Tensor &dL_dinv_depth_map,
    const torch::Tensor &dL_dfinal_T, bool camera, bool antialiasing, bool deterministic,
    int64_t tile_row_begin, int64_t tile_row_end, int64_t image_height) {
    TORCH_CHECK(tile_row_begin != 0 || tile_row_end != 0,
                "rasterize_gaussians_backward_strip_ext needs a strip: tile rows (0, 0) given");
    const torch::Tensor planes[3] = {dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T};
    return backward_impl({background, means3D, colors, opacities, scales, rotations,
                          scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy,
                          sh, degree, campos, false, debug},
                         dL_dout_color, planes, camera, antialiasing, false, deterministic,
                         tile_row_begin, tile_row_end, image_height);
}

// ... with feature channels: tile rows (0, 0) for a whole frame.
using Backward12 = decltype(std::tuple_cat(Backward11(), std::tuple<torch::Tensor>()));
Backward12 rasterize_gaussians_backward_features(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacities, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, const torch::Tensor &sh,
    int64_t degree, const torch::Tensor &campos, bool debug, const torch::Tensor &dL_dout_color,
    const torch::Tensor &dL_ddepth_map, const torch::Tensor &dL_dinv_depth_map,
    const torch::Tensor &dL_dfinal_T, bool camera, bool antialiasing, bool deterministic,
    int64_t tile_row_begin, int64_t tile_row_end, int64_t image_height,
    const torch::Tensor &features, const torch::Tensor &dL_dfeature_map) {
    const torch::Tensor planes[3] = {dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T};
    torch::Tensor dL_dfeatures;
    Backward11 g = backward_impl({background, means3D, colors, opacities, scales, rotations,
                                  scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                  tan_fovy, sh, degree, campos, false, debug},
                                 dL_dout_color, planes, camera, antialiasing, false, deterministic,
                                 tile_row_begin, tile_row_end, image_height, &features,
                                 &dL_dfeature_map, &dL_dfeatures);
    return std::tuple_cat(g, std::make_tuple(dL_dfeatures));
}

// The strip-capable general backward with the absolute gradient of the 2D means
// (gsr_backward_abs): its arguments, tile rows (0, 0) for a whole frame; its tuple with
// dL_dmeans2D_abs [P, 3] appended.
Backward12 rasterize_gaussians_backward_abs(
    const torch::Tensor &background, const torch::Tensor &means3D, const torch::Tensor &colors,
    const torch::Tensor &opacities, const torch::Tensor &scales, const torch::Tensor &rotations,
    double scale_modifier, const torch::Tensor &cov3D_precomp, const torch::Tensor &viewmatrix,
    const torch::Tensor &projmatrix, double tan_fovx, double tan_fovy, const torch::Tensor &sh,
    int64_t degree, const torch::Tensor &campos, bool debug, const torch::Tensor &dL_dout_color,
    const torch::Tensor &dL_ddepth_map, const torch::Tensor &dL_dinv_depth_map,
    const torch::Tensor &dL_dfinal_T, bool camera, bool antialiasing, bool deterministic,
    int64_t tile_row_begin, int64_t tile_row_end, int64_t image_height) {
    const torch::Tensor planes[3] = {dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T};
    torch::Tensor dL_dmeans2D_abs;
    Backward11 g = backward_impl({background, means3D, colors, opacities, scales, rotations,
                                  scale_modifier, cov3D_precomp, viewmatrix, projmatrix, tan_fovx,
                                  tan_fovy, sh, degree, campos, false, debug},
                                 dL_dout_color, planes, camera, antialiasing, false, deterministic,
                                 tile_row_begin, tile_row_end, image_height, nullptr, nullptr,
                                 nullptr, &dL_dmeans2D_abs);
    return std::tuple_cat(g, std::make_tuple(dL_dmeans2D_abs));
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

// The loss's two images: contiguous float32 [C, H, W] on one HIP device (the Python entry makes
// them so); fills the C ABI's struct.
gsr_image_loss_inputs loss_inputs(const torch::Tensor &image, const torch::Tensor &target,
                                  double lambda) {
    TORCH_CHECK(image.is_cuda() && target.is_cuda(), "image and target must be device (HIP) tensors");
    TORCH_CHECK(image.device() == target.device(), "image and target must be on one device");
    TORCH_CHECK(image.dim() == 3 && image.sizes() == target.sizes(),
                "image and target must have one shape (C, H, W)");
    TORCH_CHECK(image.scalar_type() == torch::kFloat32 && target.scalar_type() == torch::kFloat32 &&
                    image.is_contiguous() && target.is_contiguous(),
                "image and target must be contiguous float32");
    TORCH_CHECK(image.numel() < ((int64_t)1 << 31), "image too large: C*H*W must be < 2^31");
    gsr_image_loss_inputs in{};
    in.C = (int32_t)image.size(0);
    in.H = (int32_t)image.size(1);
    in.W = (int32_t)image.size(2);
    in.lambda = (float)lambda;
    in.image = image.data_ptr<float>();
    in.target = target.data_ptr<float>();
    return in;
}

std::tuple<torch::Tensor, torch::Tensor> fused_image_loss(const torch::Tensor &image,
                                                          const torch::Tensor &target,
                                                          double lambda, bool need_saved) {
    const gsr_image_loss_inputs in = loss_inputs(image, target, lambda);
    const int64_t bytes = gsr_image_loss_workspace(in.C, in.H, in.W);
    TORCH_CHECK(bytes >= 0, "gsr_image_loss_workspace failed (", bytes, "): ", gsr_last_error());
    c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor values = torch::empty({3}, image.options());
    torch::Tensor saved = need_saved ? torch::empty({3, in.C, in.H, in.W}, image.options())
                                     : torch::empty({0}, image.options());
    torch::Tensor ws = torch::empty({bytes}, image.options().dtype(torch::kUInt8));
    hipStream_t s = c10::hip::getCurrentHIPStream(image.device().index()).stream();
    const int rc = gsr_image_loss(&in, values.data_ptr<float>(),
                                  need_saved ? saved.data_ptr<float>() : nullptr, ws.data_ptr(), s);
    TORCH_CHECK(rc == GSR_OK, "gsr_image_loss failed (", rc, "): ", gsr_last_error());
    return std::make_tuple(values, saved);
}

torch::Tensor fused_image_loss_backward(const torch::Tensor &image, const torch::Tensor &target,
                                        double lambda, const torch::Tensor &saved,
                                        const torch::Tensor &dL_dloss) {
    const gsr_image_loss_inputs in = loss_inputs(image, target, lambda);
    TORCH_CHECK(saved.is_cuda() && saved.device() == image.device() &&
                    saved.scalar_type() == torch::kFloat32 && saved.is_contiguous() &&
                    saved.numel() == 3 * image.numel(),
                "saved must be the forward's contiguous float32 (3, C, H, W) tensor");
    const float *gl = nullptr;
    torch::Tensor g;
    if (dL_dloss.defined() && dL_dloss.numel() != 0) {
        TORCH_CHECK(dL_dloss.numel() == 1, "dL_dloss must hold one value");
        g = dL_dloss.to(image.device(), torch::kFloat32).contiguous();
        gl = g.data_ptr<float>();
    }
    c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor grad = torch::empty_like(image);
    hipStream_t s = c10::hip::getCurrentHIPStream(image.device().index()).stream();
    const int rc = gsr_image_loss_backward(&in, saved.data_ptr<float>(), gl,
                                           grad.data_ptr<float>(), s);
    TORCH_CHECK(rc == GSR_OK, "gsr_image_loss_backward failed (", rc, "): ", gsr_last_error());
    return grad;
}

// A window of a frame for the two entries below: the band's struct is loss_inputs' (the frame's
// size limit is the C ABI's to check).
gsr_loss_window loss_window(int64_t frame_H, int64_t row0, int64_t own_begin, int64_t own_end) {
    const int64_t lim = (int64_t)1 << 31;
    TORCH_CHECK(frame_H >= 0 && frame_H < lim && row0 >= 0 && row0 < lim && own_begin >= 0 &&
                    own_begin < lim && own_end >= 0 && own_end < lim,
                "frame_H, row0, own_begin and own_end must be in [0, 2^31)");
    gsr_loss_window w{};
    w.frame_H = (int32_t)frame_H;
    w.row0 = (int32_t)row0;
    w.own_begin = (int32_t)own_begin;
    w.own_end = (int32_t)own_end;
    return w;
}

int64_t apron_rows(const gsr_loss_window &w) {
    const int64_t a0 = std::max<int64_t>(0, (int64_t)w.own_begin - 5);
    const int64_t a1 = std::min<int64_t>(w.frame_H, (int64_t)w.own_end + 5);
    return std::max<int64_t>(0, a1 - a0);
}

std::tuple<torch::Tensor, torch::Tensor> fused_image_loss_window(
    const torch::Tensor &image, const torch::Tensor &target, int64_t frame_H, int64_t row0,
    int64_t own_begin, int64_t own_end, double lambda, bool need_saved) {
    const gsr_image_loss_inputs in = loss_inputs(image, target, lambda);
    const gsr_loss_window w = loss_window(frame_H, row0, own_begin, own_end);
    const int64_t bytes = gsr_image_loss_window_workspace(&in, &w);
    TORCH_CHECK(bytes >= 0, "gsr_image_loss_window_workspace failed (", bytes, "): ",
                gsr_last_error());
    c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor values = torch::empty({3}, image.options());
    torch::Tensor saved = need_saved ? torch::empty({3, in.C, apron_rows(w), in.W}, image.options())
                                     : torch::empty({0}, image.options());
    torch::Tensor ws = torch::empty({bytes}, image.options().dtype(torch::kUInt8));
    hipStream_t s = c10::hip::getCurrentHIPStream(image.device().index()).stream();
    const int rc = gsr_image_loss_window(&in, &w, values.data_ptr<float>(),
                                         need_saved ? saved.data_ptr<float>() : nullptr,
                                         ws.data_ptr(), s);
    TORCH_CHECK(rc == GSR_OK, "gsr_image_loss_window failed (", rc, "): ", gsr_last_error());
    return std::make_tuple(values, saved);
}

torch::Tensor fused_image_loss_window_backward(const torch::Tensor &image,
                                               const torch::Tensor &target, int64_t frame_H,
                                               int64_t row0, int64_t own_begin, int64_t own_end,
                                               double lambda, const torch::Tensor &saved,
                                               const torch::Tensor &dL_dloss) {
    const gsr_image_loss_inputs in = loss_inputs(image, target, lambda);
    const gsr_loss_window w = loss_window(frame_H, row0, own_begin, own_end);
    TORCH_CHECK(own_begin < own_end && own_end <= frame_H, "own rows must lie in the frame");
    TORCH_CHECK(saved.is_cuda() && saved.device() == image.device() &&
                    saved.scalar_type() == torch::kFloat32 && saved.is_contiguous() &&
                    saved.numel() == 3 * (int64_t)in.C * apron_rows(w) * in.W,
                "saved must be the window forward's contiguous float32 (3, C, A, W) tensor");
    const float *gl = nullptr;
    torch::Tensor g;
    if (dL_dloss.defined() && dL_dloss.numel() != 0) {
        TORCH_CHECK(dL_dloss.numel() == 1, "dL_dloss must hold one value");
        g = dL_dloss.to(image.device(), torch::kFloat32).contiguous();
        gl = g.data_ptr<float>();
    }
    c10::hip::HIPGuard guard(image.device().index());
    torch::Tensor grad = torch::empty({in.C, own_end - own_begin, in.W}, image.options());
    hipStream_t s = c10::hip::getCurrentHIPStream(image.device().index()).stream();
    const int rc = gsr_image_loss_window_backward(&in, &w, saved.data_ptr<float>(), gl,
                                                  grad.data_ptr<float>(), s);
    TORCH_CHECK(rc == GSR_OK, "gsr_image_loss_window_backward failed (", rc, "): ",
                gsr_last_error());
    return grad;
}

// A float32 [P, M] tensor of the optimizer entries: on `dev`, contiguous, `numel` elements.
float *adam_buffer(const torch::Tensor &t, const torch::Device &dev, int64_t numel,
                   const char *name) {
    TORCH_CHECK(t.defined() && t.is_cuda() && t.device() == dev, name,
                " must be a device (HIP) tensor on the parameters' device");
    TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.is_contiguous(), name,
                " must be contiguous float32");
    TORCH_CHECK(t.numel() == numel, name, " holds ", t.numel(), " values, expected ", numel);
    return t.data_ptr<float>();
}

// mask -> the settings' visible (bool / uint8) or radii (int32), or neither for an empty one
void adam_mask(const torch::Tensor &mask, const torch::Device &dev, int64_t P,
               gsr_adam_settings *s) {
    if (!mask.defined() || mask.numel() == 0) return;
    TORCH_CHECK(mask.is_cuda() && mask.device() == dev && mask.is_contiguous(),
                "mask must be a contiguous device (HIP) tensor on the parameters' device");
    TORCH_CHECK(mask.numel() == P, "mask holds ", mask.numel(), " values, expected ", P);
    if (mask.scalar_type() == torch::kBool || mask.scalar_type() == torch::kUInt8)
        s->visible = static_cast<const uint8_t *>(mask.data_ptr());
    else if (mask.scalar_type() == torch::kInt32)
        s->radii = mask.data_ptr<int32_t>();
    else
        TORCH_CHECK(false, "mask must be bool, uint8 (visible) or int32 (radii)");
}

void fused_adam_step(const std::vector<torch::Tensor> &params,
                     const std::vector<torch::Tensor> &grads,
                     const std::vector<torch::Tensor> &exp_avgs,
                     const std::vector<torch::Tensor> &exp_avg_sqs, const std::vector<double> &lrs,
                     const std::vector<double> &epss, const torch::Tensor &mask, double b1,
                     double b2, double bc1, double bc2_sqrt) {
    const size_t n = params.size();
    TORCH_CHECK(n >= 1 && n <= GSR_MAX_PARAM_GROUPS, "1..", GSR_MAX_PARAM_GROUPS,
                " parameter groups per call, got ", n);
    TORCH_CHECK(grads.size() == n && exp_avgs.size() == n && exp_avg_sqs.size() == n &&
                    lrs.size() == n && epss.size() == n,
                "params, grads, exp_avgs, exp_avg_sqs, lrs and epss must have one length");
    TORCH_CHECK(params[0].defined() && params[0].is_cuda(),
                "params must be device (HIP) tensors");
    const torch::Device dev = params[0].device();
    TORCH_CHECK(params[0].dim() >= 1, "a parameter must be at least 1-D: [P, ...]");
    const int64_t P = params[0].size(0);
    gsr_adam_settings s{};
    s.P = P;
    s.n_groups = (int32_t)n;
    s.beta1 = (float)b1;
    s.beta2 = (float)b2;
    s.bias_correction1 = (float)bc1;
    s.bias_correction2_sqrt = (float)bc2_sqrt;
    adam_mask(mask, dev, P, &s);
    gsr_param_group g[GSR_MAX_PARAM_GROUPS] = {};
    for (size_t i = 0; i < n; ++i) {
        const torch::Tensor &p = params[i];
        TORCH_CHECK(p.defined() && p.dim() >= 1 && p.size(0) == P,
                    "every parameter's first dimension must be ", P);
        const int64_t numel = p.numel(), M = P > 0 ? numel / P : 1;
        TORCH_CHECK(M >= 1 && M < ((int64_t)1 << 31), "a parameter row of ", M, " floats");
        g[i].M = (int32_t)M;
        g[i].lr = (float)lrs[i];
        g[i].eps = (float)epss[i];
        g[i].param = adam_buffer(p, dev, numel, "param");
        g[i].grad = adam_buffer(grads[i], dev, numel, "grad");
        g[i].exp_avg = adam_buffer(exp_avgs[i], dev, numel, "exp_avg");
        g[i].exp_avg_sq = adam_buffer(exp_avg_sqs[i], dev, numel, "exp_avg_sq");
    }
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t st = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int rc = gsr_adam_step(&s, g, st);
    TORCH_CHECK(rc == GSR_OK, "gsr_adam_step failed (", rc, "): ", gsr_last_error());
}

void adam_update(torch::Tensor &param, const torch::Tensor &grad, torch::Tensor &exp_avg,
                 torch::Tensor &exp_avg_sq, const torch::Tensor &visible, double lr, double b1,
                 double b2, double eps, int64_t N, int64_t M) {
    TORCH_CHECK(param.defined() && param.is_cuda(), "param must be a device (HIP) tensor");
    TORCH_CHECK(N >= 0 && M >= 1 && M < ((int64_t)1 << 31), "bad N, M: ", N, ", ", M);
    TORCH_CHECK(visible.defined() && visible.numel() == N &&
                    (visible.scalar_type() == torch::kBool ||
                     visible.scalar_type() == torch::kUInt8),
                "visible must be a bool or uint8 tensor of N values");
    const torch::Device dev = param.device();
    gsr_adam_settings s{};
    s.P = N;
    s.n_groups = 1;
    s.beta1 = (float)b1;
    s.beta2 = (float)b2;
    s.bias_correction1 = 1.0f;
    s.bias_correction2_sqrt = 1.0f;
    adam_mask(visible, dev, N, &s);
    gsr_param_group g{};
    g.M = (int32_t)M;
    g.lr = (float)lr;
    g.eps = (float)eps;
    g.param = adam_buffer(param, dev, N * M, "param");
    g.grad = adam_buffer(grad, dev, N * M, "grad");
    g.exp_avg = adam_buffer(exp_avg, dev, N * M, "exp_avg");
    g.exp_avg_sq = adam_buffer(exp_avg_sq, dev, N * M, "exp_avg_sq");
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t st = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int rc = gsr_adam_step(&s, &g, st);
    TORCH_CHECK(rc == GSR_OK, "gsr_adam_step failed (", rc, "): ", gsr_last_error());
}

void densification_stats(const torch::Tensor &radii, const torch::Tensor &means2D_grad,
                         torch::Tensor &grad_accum, torch::Tensor &denom,
                         const torch::Tensor &max_radii) {
    TORCH_CHECK(radii.defined() && radii.is_cuda() && radii.scalar_type() == torch::kInt32 &&
                    radii.is_contiguous(),
                "radii must be a contiguous int32 device (HIP) tensor");
    const torch::Device dev = radii.device();
    const int64_t P = radii.numel();
    gsr_densify_inputs in{};
    in.P = P;
    in.radii = radii.data_ptr<int32_t>();
    in.dL_dmeans2D = adam_buffer(means2D_grad, dev, 3 * P, "means2D_grad");
    in.grad_accum = adam_buffer(grad_accum, dev, P, "grad_accum");
    in.denom = adam_buffer(denom, dev, P, "denom");
    if (max_radii.defined() && max_radii.numel() != 0) {
        TORCH_CHECK(max_radii.is_cuda() && max_radii.device() == dev &&
                        max_radii.scalar_type() == torch::kInt32 && max_radii.is_contiguous() &&
                        max_radii.numel() == P,
                    "max_radii must be a contiguous int32 tensor of ", P, " values on radii's device");
        in.max_radii = max_radii.data_ptr<int32_t>();
    }
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t st = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int rc = gsr_densify_stats(&in, st);
    TORCH_CHECK(rc == GSR_OK, "gsr_densify_stats failed (", rc, "): ", gsr_last_error());
}

// gsr_densify_plan_inputs of both densify entries: the statistics and the two tensors the
// classification reads (checked), thresholds = (grad, scale split, opacity prune, scale prune) as
// float32 values held in doubles.
gsr_densify_plan_inputs densify_inputs(const torch::Tensor &grad_accum, const torch::Tensor &denom,
                                       const torch::Tensor &max_radii,
                                       const torch::Tensor &scaling, const torch::Tensor &opacity,
                                       const std::vector<double> &thresholds,
                                       int64_t radius_threshold, int64_t scale_space,
                                       uint64_t seed) {
    TORCH_CHECK(scaling.defined() && scaling.is_cuda(), "scaling must be a device (HIP) tensor");
    TORCH_CHECK(scaling.dim() >= 1, "scaling must be [P, 3]");
    TORCH_CHECK(thresholds.size() == 4, "thresholds: grad, scale split, opacity prune, scale prune");
    const torch::Device dev = scaling.device();
    const int64_t P = scaling.size(0);
    gsr_densify_plan_inputs in{};
    in.P = P;
    in.seed = seed;
    in.scale_space = (int32_t)scale_space;
    in.grad_threshold = (float)thresholds[0];
    in.scale_split_threshold = (float)thresholds[1];
    in.opacity_prune_threshold = (float)thresholds[2];
    in.scale_prune_threshold = (float)thresholds[3];
    in.radius_prune_threshold = (int32_t)std::min<int64_t>(radius_threshold, INT32_MAX);
    in.grad_accum = adam_buffer(grad_accum, dev, P, "grad_accum");
    in.denom = adam_buffer(denom, dev, P, "denom");
    in.scaling = adam_buffer(scaling, dev, 3 * P, "scaling");
    in.opacity = adam_buffer(opacity, dev, P, "opacity");
    if (max_radii.defined() && max_radii.numel() != 0) {
        TORCH_CHECK(max_radii.is_cuda() && max_radii.device() == dev &&
                        max_radii.scalar_type() == torch::kInt32 && max_radii.is_contiguous() &&
                        max_radii.numel() == P,
                    "max_radii must be a contiguous int32 tensor of ", P, " values on scaling's device");
        in.max_radii = max_radii.data_ptr<int32_t>();
    }
    return in;
}

void *densify_workspace(const torch::Tensor &workspace, const torch::Device &dev, int64_t P) {
    const int64_t bytes = gsr_densify_workspace(P);
    TORCH_CHECK(bytes >= 0, "gsr_densify_workspace failed (", bytes, "): ", gsr_last_error());
    TORCH_CHECK(workspace.defined() && workspace.is_cuda() && workspace.device() == dev &&
                    workspace.is_contiguous() && workspace.scalar_type() == torch::kInt32 &&
                    workspace.numel() * 4 >= bytes,
                "workspace must be a contiguous int32 device tensor of at least ", bytes, " bytes");
    return workspace.data_ptr();
}

void densify_plan(const torch::Tensor &grad_accum, const torch::Tensor &denom,
                  const torch::Tensor &max_radii, const torch::Tensor &scaling,
                  const torch::Tensor &opacity, const std::vector<double> &thresholds,
                  int64_t radius_threshold, int64_t scale_space, torch::Tensor &workspace,
                  torch::Tensor &counts) {
    const gsr_densify_plan_inputs in = densify_inputs(grad_accum, denom, max_radii, scaling, opacity,
                                                      thresholds, radius_threshold, scale_space, 0);
    const torch::Device dev = scaling.device();
    void *ws = densify_workspace(workspace, dev, in.P);
    TORCH_CHECK(counts.defined() && counts.is_cuda() && counts.device() == dev &&
                    counts.scalar_type() == torch::kInt32 && counts.is_contiguous() &&
                    counts.numel() == 4,
                "counts must be a contiguous int32 device tensor of 4 values");
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t st = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int rc = gsr_densify_plan(&in, ws, counts.data_ptr<int32_t>(), st);
    TORCH_CHECK(rc == GSR_OK, "gsr_densify_plan failed (", rc, "): ", gsr_last_error());
}

void densify_apply(const torch::Tensor &grad_accum, const torch::Tensor &denom,
                   const torch::Tensor &max_radii, const torch::Tensor &scaling,
                   const torch::Tensor &opacity, const std::vector<double> &thresholds,
                   int64_t radius_threshold, int64_t scale_space, uint64_t seed,
                   const std::vector<int64_t> &roles, const std::vector<int64_t> &has_moments,
                   const std::vector<torch::Tensor> &src_params,
                   const std::vector<torch::Tensor> &src_exp_avgs,
                   const std::vector<torch::Tensor> &src_exp_avg_sqs,
                   const std::vector<torch::Tensor> &dst_params,
                   const std::vector<torch::Tensor> &dst_exp_avgs,
                   const std::vector<torch::Tensor> &dst_exp_avg_sqs,
                   const torch::Tensor &workspace, torch::Tensor &source_index) {
    gsr_densify_plan_inputs in = densify_inputs(grad_accum, denom, max_radii, scaling, opacity,
                                                thresholds, radius_threshold, scale_space, seed);
    const torch::Device dev = scaling.device();
    const size_t n = src_params.size();
    TORCH_CHECK(n >= 1 && n <= GSR_MAX_PARAM_GROUPS, "1..", GSR_MAX_PARAM_GROUPS,
                " parameter groups per call, got ", n);
    TORCH_CHECK(roles.size() == n && has_moments.size() == n && src_exp_avgs.size() == n && src_exp_avg_sqs.size() == n &&
                    dst_params.size() == n && dst_exp_avgs.size() == n &&
                    dst_exp_avg_sqs.size() == n,
                "roles, has_moments and the six tensor lists must have one length");
    TORCH_CHECK(source_index.defined() && source_index.is_cuda() && source_index.device() == dev &&
                    source_index.scalar_type() == torch::kInt32 && source_index.is_contiguous(),
                "source_index must be a contiguous int32 device tensor");
    const int64_t P = in.P, Pout = source_index.numel();
    in.P_out = Pout;
    in.n_groups = (int32_t)n;
    gsr_densify_group src[GSR_MAX_PARAM_GROUPS] = {}, dst[GSR_MAX_PARAM_GROUPS] = {};
    // a group without moments (has_moments 0) passes any tensors in their places: NULL
    auto moment = [&](size_t i, const torch::Tensor &t, int64_t numel, const char *name) {
        return has_moments[i] ? adam_buffer(t, dev, numel, name) : nullptr;
    };
    for (size_t i = 0; i < n; ++i) {
        const torch::Tensor &p = src_params[i], &q = dst_params[i];
        TORCH_CHECK(p.defined() && p.dim() >= 1 && p.size(0) == P && q.defined() && q.dim() >= 1 &&
                        q.size(0) == Pout,
                    "a source's first dimension must be ", P, ", a destination's ", Pout);
        const int64_t M = P > 0 ? p.numel() / P : (Pout > 0 ? q.numel() / Pout : 1);
        TORCH_CHECK(M >= 1 && M < ((int64_t)1 << 31), "a parameter row of ", M, " floats");
        src[i].M = dst[i].M = (int32_t)M;
        src[i].role = dst[i].role = (int32_t)roles[i];
        src[i].param = adam_buffer(p, dev, P * M, "a source parameter");
        dst[i].param = adam_buffer(q, dev, Pout * M, "a destination parameter");
        src[i].exp_avg = moment(i, src_exp_avgs[i], P * M, "a source exp_avg");
        src[i].exp_avg_sq = moment(i, src_exp_avg_sqs[i], P * M, "a source exp_avg_sq");
        dst[i].exp_avg = moment(i, dst_exp_avgs[i], Pout * M, "a destination exp_avg");
        dst[i].exp_avg_sq = moment(i, dst_exp_avg_sqs[i], Pout * M, "a destination exp_avg_sq");
    }
    const void *ws = densify_workspace(workspace, dev, P);
    c10::hip::HIPGuard guard(dev.index());
    hipStream_t st = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int rc = gsr_densify_apply(&in, src, dst, ws, source_index.data_ptr<int32_t>(), st);
    TORCH_CHECK(rc == GSR_OK, "gsr_densify_apply failed (", rc, "): ", gsr_last_error());
}

// upstream's simple_knn distCUDA2: the mean squared distance of every point to its three nearest
// neighbours, gsr_knn_mean_dist2 on torch's current stream in a workspace torch allocates.
torch::Tensor dist_cuda2(const torch::Tensor &points) {
    TORCH_CHECK(points.defined() && points.is_cuda(), "points must be a device (HIP) tensor");
    TORCH_CHECK(points.scalar_type() == torch::kFloat32 && points.dim() == 2 &&
                    points.size(1) == 3 && points.is_contiguous(),
                "points must be a contiguous float32 tensor of dimensions (num_points, 3)");
    const torch::Device dev = points.device();
    const int64_t N = points.size(0);
    const int64_t bytes = gsr_knn_workspace(N);
    TORCH_CHECK(bytes >= 0, "gsr_knn_workspace failed (", bytes, "): ", gsr_last_error());
    c10::hip::HIPGuard guard(dev.index());
    torch::Tensor dist2 = torch::empty({N}, points.options());
    torch::Tensor workspace = torch::empty({bytes}, points.options().dtype(torch::kUInt8));
    hipStream_t st = c10::hip::getCurrentHIPStream(dev.index()).stream();
    const int rc = gsr_knn_mean_dist2(points.data_ptr<float>(), N, dist2.data_ptr<float>(),
                                      workspace.data_ptr(), st);
    TORCH_CHECK(rc == GSR_OK, "gsr_knn_mean_dist2 failed (", rc, "): ", gsr_last_error());
    return dist2;
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
    m.def("rasterize_gaussians_ext", &rasterize_gaussians_ext,
          "rasterize_gaussians' 19 arguments, then shading (GSR_SHADE_*), planes, antialiasing, "
          "tile_row_begin = 0, tile_row_end = 0 (a strip: strip-local image and planes) -> "
          "(num_rendered, color, radii, depth_map, inv_depth_map, final_T), the three planes "
          "empty without `planes`",
          pybind11::arg("bg"), pybind11::arg("means3D"), pybind11::arg("colors_precomp"),
          pybind11::arg("opacities"), pybind11::arg("scales"), pybind11::arg("rotations"),
          pybind11::arg("scale_modifier"), pybind11::arg("cov3D_precomp"),
          pybind11::arg("viewmatrix"), pybind11::arg("projmatrix"), pybind11::arg("tanfovx"),
          pybind11::arg("tanfovy"), pybind11::arg("image_height"), pybind11::arg("image_width"),
          pybind11::arg("sh"), pybind11::arg("sh_degree"), pybind11::arg("campos"),
          pybind11::arg("prefiltered"), pybind11::arg("debug"), pybind11::arg("shading"),
          pybind11::arg("planes"), pybind11::arg("antialiasing"),
          pybind11::arg("tile_row_begin") = 0, pybind11::arg("tile_row_end") = 0);
    m.def("rasterize_gaussians_backward_ext", &rasterize_gaussians_backward_ext,
          "bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, "
          "cov3D_precomp, viewmatrix, projmatrix, tanfovx, tanfovy, sh, sh_degree, campos, debug, "
          "dL_dout_color, dL_ddepth_map, dL_dinv_depth_map, dL_dfinal_T (empty = unused), camera, "
          "antialiasing, deterministic = False (gsr_backward_ordered: the same bits on every "
          "call) -> rasterize_gaussians_backward's 8-tuple, then dL_dviewmatrix (4, 4), "
          "dL_dprojmatrix (4, 4), dL_dcampos (3), empty without `camera`",
          pybind11::arg("bg"), pybind11::arg("means3D"), pybind11::arg("colors_precomp"),
          pybind11::arg("opacities"), pybind11::arg("scales"), pybind11::arg("rotations"),
          pybind11::arg("scale_modifier"), pybind11::arg("cov3D_precomp"),
          pybind11::arg("viewmatrix"), pybind11::arg("projmatrix"), pybind11::arg("tanfovx"),
          pybind11::arg("tanfovy"), pybind11::arg("sh"), pybind11::arg("sh_degree"),
          pybind11::arg("campos"), pybind11::arg("debug"), pybind11::arg("dL_dout_color"),
          pybind11::arg("dL_ddepth_map"), pybind11::arg("dL_dinv_depth_map"),
          pybind11::arg("dL_dfinal_T"), pybind11::arg("camera"), pybind11::arg("antialiasing"),
          pybind11::arg("deterministic") = false);
    m.def("rasterize_gaussians_backward_strip_ext", &rasterize_gaussians_backward_strip_ext,
          "rasterize_gaussians_backward_ext's 23 arguments, then tile_row_begin, tile_row_end, "
          "image_height: gsr_backward_strip, the backward on a strip of tile rows of a frame "
          "image_height px high (strip-local image and plane gradients) -> the same 11-tuple");
    m.def("rasterize_gaussians_features", &rasterize_gaussians_features,
          "rasterize_gaussians' 19 arguments, then planes, antialiasing, tile_row_begin, "
          "tile_row_end, features (P, C): gsr_forward_features -> rasterize_gaussians_ext's "
          "6-tuple, then feature_map (C, rows, W)");
    m.def("rasterize_gaussians_backward_features", &rasterize_gaussians_backward_features,
          "rasterize_gaussians_backward_ext's 23 arguments, then tile_row_begin, tile_row_end, "
          "image_height, features (P, C), dL_dfeature_map (C, rows, W): gsr_backward_features -> "
          "the 11-tuple, then dL_dfeatures (P, C)");
    m.def("rasterize_gaussians_backward_abs", &rasterize_gaussians_backward_abs,
          "rasterize_gaussians_backward_strip_ext's 26 arguments, tile rows (0, 0) for a whole "
          "frame: gsr_backward_abs -> the 11-tuple, then dL_dmeans2D_abs (P, 3), the sums over "
          "pixels of the absolute values of the pixels' terms of dL_dmeans2D");
    m.def("mark_visible", &mark_visible, "upstream markVisible: bool[P]");
    m.def("fused_image_loss", &fused_image_loss,
          "image, target (contiguous float32 (C, H, W)), lambda_dssim, need_saved: gsr_image_loss "
          "-> (values (3,) = loss, l1, ssim; saved (3, C, H, W), empty without need_saved)");
    m.def("fused_image_loss_backward", &fused_image_loss_backward,
          "image, target, lambda_dssim, saved, dL_dloss (one device value, or empty for 1.0): "
          "gsr_image_loss_backward -> dL_dimage (C, H, W)");
    m.def("fused_image_loss_window", &fused_image_loss_window,
          "band image, band target (contiguous float32 (C, rows, W)), frame_H, row0, own_begin, "
          "own_end, lambda_dssim, need_saved: gsr_image_loss_window -> (values (3,), saved "
          "(3, C, A, W) or empty)");
    m.def("fused_image_loss_window_backward", &fused_image_loss_window_backward,
          "band image, band target, frame_H, row0, own_begin, own_end, lambda_dssim, saved, "
          "dL_dloss: gsr_image_loss_window_backward -> dL_dimage (C, own_end - own_begin, W)");
    m.def("adamUpdate", &adam_update,
          "upstream's adamUpdate: param, grad, exp_avg, exp_avg_sq (N, M), visible (bool or uint8 "
          "N), lr, b1, b2, eps, N, M: gsr_adam_step on one group, in place, no bias correction");
    m.def("fused_adam_step", &fused_adam_step,
          "params, grads, exp_avgs, exp_avg_sqs (lists of (P, M_i) tensors), lrs, epss, mask "
          "(bool / uint8 (P), int32 radii (P), or empty), b1, b2, bc1, bc2_sqrt: gsr_adam_step on "
          "all groups in one launch, in place");
    m.def("densification_stats", &densification_stats,
          "radii (P) int32, means2D_grad (P, 3), grad_accum (P), denom (P), max_radii (P) int32 "
          "or empty: gsr_densify_stats, in place");
    m.def("densify_plan", &densify_plan,
          "grad_accum, denom, max_radii (int32 (P) or empty), scaling, opacity, thresholds (grad, "
          "scale split, opacity prune, scale prune), radius_threshold, scale_space, workspace "
          "(int32), counts (int32 (4)): gsr_densify_plan, into workspace and counts");
    m.def("densify_apply", &densify_apply,
          "the plan's first eight arguments, seed, roles, has_moments, src params / exp_avgs / "
          "exp_avg_sqs, dst params / exp_avgs / exp_avg_sqs, workspace, source_index (int32 "
          "(P_out)): gsr_densify_apply, into the dst tensors and source_index");
    m.def("distCUDA2", &dist_cuda2,
          "upstream's simple_knn distCUDA2: points (N, 3) -> (N) the mean squared distance to the "
          "three nearest neighbours (gsr_knn_mean_dist2)");
    m.def("abi_version", []() { return gsr_abi_version(); });
    m.def(
        "context_handle",
        [](int64_t device) { return (uintptr_t)context_for((int)device); },
        "the device's gsr_context (as an address), created on first use");
    m.def("release_contexts", &release_contexts, "destroy every context (process exit)");
}
