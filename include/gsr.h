/*
 * gsr.h -- C ABI of the MI355X-native forward Gaussian-splat rasterizer (libgsr.so).
 *
 * This is the drop-in boundary under the viewer's CUDA backend.  Every entry point names
 * the reference interface it replaces (paths relative to /root/reference):
 *
 *   gsr_forward        <- diff_gaussian_rasterization `_C.rasterize_gaussians(...)` as called
 *                         by GaussianRasterizer.forward, which renderer_cuda.py:211-224
 *                         (CUDARenderer.draw) invokes every frame.  [third-party, un-vendored]
 *   gsr_mark_visible   <- `_C.mark_visible(positions, viewmatrix, projmatrix)` behind
 *                         GaussianRasterizer.markVisible.  [third-party, un-vendored]
 *   gsr_depth_argsort  <- the per-frame depth sort backend `_sort_gaussian(gaus, view_mat)`
 *                         (renderer_ogl.py:10-19 cpu, :22-38 cupy, :41-53 torch), consumed by
 *                         OpenGLRenderer.sort_and_update (renderer_ogl.py:139-146).
 *   gsr_ply_probe/load <- util_gau.load_ply (util_gau.py:63-125).
 *   gsr_disparity_colors <- the disparity render mode (render_mod == -1) of the GL vertex
 *                         shader, gau_vert.glsl:182-207, driven by main.py:862-868.
 *   gsr_pack_image     <- the frame hand-offs: CHW -> HWC+alpha (renderer_cuda.py:226-228) and
 *                         the capture readbacks glReadPixels RGB8 / R32F->uint16 with their
 *                         row flips (main.py:855-879, 895-917).
 *
 * Conventions (plain pointers and sizes only; no torch or HIP types):
 *   - every array pointer is DEVICE memory unless the comment says host;
 *   - matrices passed as device pointers are 16 floats, column-major (upstream's layout,
 *     i.e. the row-major bytes of `view.T` that renderer_cuda.py:192-194 uploads);
 *   - `stream` is a hipStream_t (NULL = the default stream); all work is enqueued on it.
 *     gsr_forward waits once per call for the number of (Gaussian, tile) pairs, as upstream
 *     does for num_rendered -- not for the stream: the GPU stores it into pinned memory as
 *     soon as the preprocess has counted it, while the depth sort runs.  With frame graphs
 *     (GSR_OPT_FRAME_GRAPHS) that wait comes after the whole frame is queued;
 *   - every function returns GSR_OK (0) or a negative GSR_E* code; gsr_last_error()
 *     returns the calling thread's last message.  The Python layer raises RuntimeError;
 *   - a context serves one call at a time: every entry point taking a gsr_context holds the
 *     context's mutex for the call (two host threads rendering on one context are serialised,
 *     not interleaved).  Its workspace is ordered on the stream of the call that used it last: a
 *     call on another stream first waits for the device (hipDeviceSynchronize), so a context
 *     used from two streams stays correct but serial.  Frames meant to overlap on the GPU use
 *     one context (and one stream) each.
 */
#ifndef GSR_H
#define GSR_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2 (round 4): option ids renumbered (GSR_OPT_COLUMN_PAIRS retired, tight binning moved to 13,
 * ids 10 and 12 reserved), GSR_OPT_DEPTH_SORT (id 11, was COMPACT_SORT) gains the MSD form,
 * gsr_get_binning exports tight lists.
 * 3 (round 6): gsr_get_option; contexts are serialised by a mutex and ordered across streams.
 * 4: gsr_forward_shaded and the GSR_SHADE_* ids (additive). */
#define GSR_ABI_VERSION 4

enum {
    GSR_OK = 0,
    GSR_E_INVALID = -1, /* bad argument / shape */
    GSR_E_HIP = -2,     /* a HIP runtime call or kernel failed */
    GSR_E_NOMEM = -3,   /* device allocation failed */
    GSR_E_STATE = -4    /* call order (e.g. no forward yet) */
};

typedef struct gsr_context gsr_context; /* device workspace + stage events; one per device */

/* Gaussians: the five tensors of GaussianDataCUDA (renderer_cuda.py:55-68, built by
 * gaus_cuda_from_cpu :87-98), contiguous float32.  Exactly one of {shs, colors_precomp} and
 * exactly one of {(scales, rotations), cov3D_precomp} must be non-NULL. */
typedef struct {
    int64_t P;            /* number of Gaussians */
    int32_t D;            /* active SH degree (raster_settings["sh_degree"], :137) */
    int32_t M;            /* SH coefficients stored per Gaussian = shs.size(1) (16 or 1) */
    float scale_modifier; /* raster_settings["scale_modifier"] */
    const float *means3D;        /* [P,3]  */
    const float *scales;         /* [P,3]  (already exp-activated, util_gau.py:118-119) */
    const float *rotations;      /* [P,4]  quaternion (r,x,y,z), normalised by the loader */
    const float *opacities;      /* [P,1]  (sigmoid-activated) */
    const float *shs;            /* [P,M,3] */
    const float *colors_precomp; /* [P,3]  */
    const float *cov3D_precomp;  /* [P,6]  upper triangle xx,xy,xz,yy,yz,zz */
} gsr_gaussians;

/* GaussianRasterizationSettings (renderer_cuda.py:104-117). */
typedef struct {
    int32_t image_width, image_height;
    float tanfovx, tanfovy;
    const float *viewmatrix;    /* device [16], column-major */
    const float *projmatrix;     /* device [16], column-major (full projection * view) */
    const float *campos;         /* device [3] */
    const float *bg;             /* device [3] */
    /* Image-space strip (multi-GPU partition): render only 16-px tile rows
     * [tile_row_begin, tile_row_end).  0/0 = the whole frame.  Output images are then
     * strip-local: [3, rows, W] with rows = min(H, 16*end) - 16*begin. */
    int32_t tile_row_begin, tile_row_end;
    int32_t prefiltered; /* upstream: points are known to be in the frustum */
    int32_t debug;       /* synchronise + check after every stage */
} gsr_raster_settings;

typedef struct {
    float *color;    /* required: [3, rows, W] float32 (CHW, as upstream out_color) */
    /* [P] int32 (0 = culled).  Required for whole frames.  On a strip (tile_row_begin/end)
     * it may be NULL when no per-Gaussian intermediate below is requested either: Gaussians
     * whose conservative footprint bound misses the strip then skip the covariance, radius and
     * record work (a multi-GPU strip rank needs only its image).
     * A Gaussian whose saturated radius is <= 0 (a NaN radius: a non-finite covariance, or a
     * negative eigenvalue under the square root) is culled like one outside the frame: radius
     * 0, no tiles, no pairs, not in num_rendered, no per-Gaussian output written.  A radius
     * is > 0 exactly where the Gaussian touches a tile. */
    int32_t *radii;
    /* optional per-Gaussian intermediates (NULL = not written) */
    float *depths;        /* [P]   view-space z */
    float *means2D;       /* [P,2] pixel-space centre */
    float *conic_opacity; /* [P,4] inverse 2D covariance (a,b,c) + opacity */
    float *rgb;           /* [P,3] SH-evaluated colour, clamped >= 0 */
    uint32_t *tiles_touched; /* [P] tiles overlapped inside the rendered strip */
    /* optional per-pixel outputs, strip-local like color */
    float *final_T;     /* [rows, W] */
    uint32_t *n_contrib; /* [rows, W] */
    /* written by gsr_forward */
    int64_t num_rendered; /* K: number of (Gaussian, tile) pairs in the strip */
} gsr_outputs;

int gsr_abi_version(void);
const char *gsr_last_error(void);

int gsr_create(gsr_context **out); /* binds to the calling thread's current HIP device */
void gsr_destroy(gsr_context *ctx);

/* Pre-size the workspace so that a timed loop never allocates (sizes are grown on demand
 * otherwise).  P Gaussians, K pairs. */
int gsr_reserve(gsr_context *ctx, int64_t P, int64_t K);

/* Forward rasterization: preprocess (EWA projection + SH) -> device radix depth sort ->
 * tile binning (scan + duplicate + radix tile sort + ranges) -> per-tile blend. */
int gsr_forward(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                gsr_outputs *out, void *stream);

/* gsr_forward with one of the GL backend's shadings (the viewer's "shading" combo, main.py:98;
 * the fragment rule of shaders/gau_frag.glsl:15-38) on the rasterizer's geometry: preprocess,
 * culls, rects, lists and the pixel-centre convention are gsr_forward's, only the per-tile stage
 * differs.  GSR_SHADE_SPLAT is gsr_forward itself.  Under the others a pixel takes the colour of
 * the FIRST entry of its tile's list (depth order) that hits it, nothing is composited; with
 * dx = mx - x, dy = my - y, power = -(a dx^2 + c dy^2) / 2 - b dx dy and
 * alpha = min(0.99, o exp(power)) an entry hits when
 *   GSR_SHADE_BILLBOARD  (GL render_mod -2): |dx| <= 3 sqrt(cxx) and |dy| <= 3 sqrt(cyy), with
 *     cxx = c / (a c - b^2), cyy = a / (a c - b^2) -- the axis-aligned +-3 sigma quad
 *     (quadwh_scr, gau_vert.glsl:174) of the 2D covariance with its 0.3.  The opacity is not
 *     read (gau_frag.glsl:15-19 returns before any discard); a NaN extent never hits;
 *   GSR_SHADE_FLAT_BALL  (GL -3, the combo's "Gaussian Ball"): power <= 0 and alpha > 0.22;
 *   GSR_SHADE_GAUSS_BALL (GL -4): as FLAT_BALL,
 * and the pixel is the entry's rgb (BILLBOARD, FLAT_BALL: the record's bits, no arithmetic) or
 * rgb * exp(power) (GAUSS_BALL).  At a hit at list position k: final_T = 0, n_contrib = k + 1;
 * without one: the pixel is bg (its bits), final_T = 1, n_contrib = 0.  GL draws back to front
 * with alpha in {0, 1}, which is the same image.
 * Lists: the billboard quad reaches beyond the alpha >= 1/255 ellipse but stays inside upstream's
 * rect, so a BILLBOARD frame always bins upstream's lists (GSR_OPT_TIGHT_BINNING is ignored for
 * it); the ball shadings keep tight lists under gsr_forward's conditions.  GSR_OPT_BLEND_CULL
 * gives identical bits either way; GSR_OPT_BLEND_FAST does not apply (one arithmetic).  The
 * shading kernel is timed as the "blend" stage.  `shading` is an argument of the call, not a
 * context option: a shared context carries no renderer's mode into another's frame.  Any other
 * value: GSR_E_INVALID. */
enum { GSR_SHADE_SPLAT = 0, GSR_SHADE_BILLBOARD = 1, GSR_SHADE_FLAT_BALL = 2,
       GSR_SHADE_GAUSS_BALL = 3 };
int gsr_forward_shaded(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                       gsr_outputs *out, int32_t shading, void *stream);

/* gsr_forward (the splat composite) that also fills two optional per-pixel planes, strip-local
 * like final_T ([rows, W] float32), from the same blend pass as the image:
 *   depth_map[y,x]     = sum_k z_k       w_k      (expected view-space depth, premultiplied)
 *   inv_depth_map[y,x] = sum_k (1 / z_k) w_k      (expected inverse depth, premultiplied)
 * over exactly the splats the colour composites at that pixel (the list order, the power > 0 and
 * alpha < 1/255 skips, the 0.99 cap and the T < 1e-4 termination are the colour's), with w_k the
 * very weight of the colour channels in the context's arithmetic (GSR_OPT_BLEND_FAST 0: alpha T in
 * upstream's order; 1: |T| - |T_next|, accumulated with one FMA).  z_k is the Gaussian's
 * view-space z -- the bits of the `depths` output and of its depth-sort key -- and 1 / z_k the
 * correctly rounded float32 quotient, computed once per staged splat.  A listed Gaussian has a
 * finite z > 0.2.  So each plane is, bit for bit, a colour channel of a gsr_forward of the same
 * scene with colors_precomp = (z, 1 / z, 0) and bg = 0 (tests/test_gpu_depth_maps.py).  There is
 * no background term: a pixel that composites nothing is 0, and the expected depth of the covered
 * part is depth_map / (1 - final_T), a division left to the caller.  A rectified stereo pair of
 * baseline B has the disparity fx |B| / z in pixels, linear in inverse depth: inv_depth_map is the
 * left image's pixel-aligned ground-truth disparity (stereo.metric_disparity).
 * Everything else is the same gsr_forward call's, bit for bit: every gsr_outputs member,
 * num_rendered and the lists gsr_get_binning exports.  A NULL struct or two NULL planes is
 * gsr_forward itself (today's kernels, today's arguments); one plane gives the bits it has when
 * both are asked for.  Strips (radii NULL included), debug, every option and every context work
 * as in gsr_forward; GSR_OPT_BLEND_CULL and GSR_OPT_TIGHT_BINNING leave the planes bit-identical
 * (a dropped splat has weight exactly 0).  Frame graphs: the blend is launched directly after the
 * recorded chains with this call's pointers, so depth and plain frames share their graphs and
 * nothing of a plane is recorded; a frame whose list outgrew the capacity writes no plane before
 * it is rendered again.  The kernel is timed as the "blend" stage.  (Additive to ABI 4.) */
typedef struct {
    float *depth_map;     /* [rows, W] or NULL */
    float *inv_depth_map; /* [rows, W] or NULL */
} gsr_depth_outputs;
int gsr_forward_depth(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                      gsr_outputs *out, const gsr_depth_outputs *depth, void *stream);

/* gsr_forward_depth that also fills two optional per-pixel planes of the pixel's MEDIAN splat,
 * strip-local like final_T ([rows, W]), from the same blend pass as the image and the depth planes.
 * For a pixel, walk the splats the colour composites, in list order (the power > 0 and
 * alpha < 1/255 skips, the 0.99 cap and the T < 1e-4 termination are the colour's, in the context's
 * arithmetic: GSR_OPT_BLEND_FAST 0 or 1, with that mode's own float32 T).  With T_k the
 * transmittance in front of composited splat k and T_{k+1} = T_k (1 - alpha_k) the one behind it,
 * the median splat is the first -- the only -- composited splat with T_k > 0.5 and T_{k+1} <= 0.5:
 * the splat at which half of the light is absorbed.  The terminating splat can never be it
 * (alpha <= 0.99 and T_{k+1} < 1e-4 force T_k < 0.01).
 *   median_id[y,x]    = int32, that splat's Gaussian id: the global index into the input tensors,
 *                       on strips too;
 *   median_depth[y,x] = float32, that Gaussian's view-space z -- the bits of the `depths` output
 *                       and of its depth-sort key, as in gsr_forward_depth; no arithmetic.
 * A pixel whose transmittance never reaches 0.5 (final_T > 0.5, an empty list, everything culled,
 * P = 0) gets median_id = -1 and median_depth = 0.0f: "no surface", the 0 of a KITTI-style
 * disparity PNG.  No background term.  Unlike the expected depth of gsr_forward_depth, which at a
 * silhouette mixes foreground and background into a depth where no surface is, median_depth is
 * always the depth of one Gaussian of the pixel's list.
 * Everything else is the same gsr_forward_depth call's, bit for bit: every gsr_outputs member, the
 * depth planes (`depth` may be NULL), num_rendered and the lists gsr_get_binning exports.  A NULL
 * `surface`, or one with two NULL members, is gsr_forward_depth itself (the same kernels, the same
 * arguments); one plane gives the bits it has when both are asked for, and the planes are the same
 * bits with and without n_contrib and with and without the depth planes.  Strips (radii NULL
 * included), debug, every option and every context work as in gsr_forward_depth;
 * GSR_OPT_BLEND_CULL and GSR_OPT_TIGHT_BINNING leave the planes bit-identical (a dropped splat has
 * alpha_eff = 0: T does not move across it, so it cannot be the median; tight binning stays on for
 * surface frames).  Frame graphs: the blend is launched directly after the recorded chains with
 * this call's pointers, so surface, depth and plain frames share their graphs and nothing of a
 * plane is recorded; a frame whose list outgrew the capacity writes no plane before it is rendered
 * again.  The kernel is timed as the "blend" stage.  The GL shadings (gsr_forward_shaded) have no
 * median.  The planes have no gradient.  (Additive to ABI 4.) */
typedef struct {
    float *median_depth; /* [rows, W] or NULL */
    int32_t *median_id;  /* [rows, W] or NULL */
} gsr_surface_outputs;
int gsr_forward_surface(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                        gsr_outputs *out, const gsr_depth_outputs *depth,
                        const gsr_surface_outputs *surface, void *stream);

/* The backward pass of gsr_forward (the splat composite): the gradients of a scalar loss L with
 * respect to the Gaussians, from dL/dcolor.  (Additive to ABI 4.)
 * The function differentiated is the forward exactly as stated above: upstream's preprocess and
 * upstream's compositing in upstream's operation order (GSR_OPT_BLEND_FAST 0's arithmetic; the
 * backward has this one arithmetic whatever the option says).  The derivative is derived from
 * that forward, not copied from upstream's backward:
 *   - gates select and are constants: z <= 0.2, det == 0, an empty rect and rect / tile
 *     membership, the power > 0 and alpha < 1/255 skips, the T (1 - alpha) < 1e-4 termination
 *     (the terminating splat contributes nothing);
 *   - min, max and clamps pass nothing on their flat side: alpha = min(0.99, o G) gives 0 to o and
 *     G where it caps, max(rgb + 0.5, 0) gives 0 to the SH of a clamped channel, and the 1.3 tan
 *     clamp of t.x / t.z is differentiated as written, the clamped value times t.z (upstream's
 *     hand-written backward lets the cap through and treats the clamped t.x as independent of
 *     t.z);
 *   - the background term final_T bg is part of the colour and is differentiated; bg gets none.
 * dL_dmeans2D keeps upstream's shape and units: [P,3], x and y the pixel-space gradient times
 * (0.5 W, 0.5 H) -- the gradient with respect to an offset added to the NDC centre before ndc2Pix
 * -- and z = 0.  A Gaussian the forward culls (radius 0) gets exactly 0.0 in every gradient, and so
 * do SH coefficients above the active degree D.  With cov3D_precomp the chain ends at dL_dcov3D
 * (dL_dscales and dL_drotations, if asked for, are 0); with colors_precomp at dL_dcolors (dL_dsh 0).
 * Whole frames only (a strip: GSR_E_INVALID); prefiltered, debug and scale_modifier as in the
 * forward.  The gradients of the depth planes come from gsr_backward_planes (below); bg gets none.
 * Inputs only: the call is a function of its arguments.  It rebuilds the per-Gaussian stage, the
 * depth sort and upstream's (untight) lists from them, launched directly (no frame graph is
 * replayed; recorded graphs stay usable), and recomputes each pixel's transmittance inside its
 * blend kernel, so it is correct whatever ran on the context since the matching forward.
 * Afterwards gsr_get_binning exports the backward's lists (upstream's, K = num_rendered), as after
 * a forward.  Every member of gsr_gradients is optional (NULL = not wanted); the call zeroes, then
 * fills, each one given (it does not accumulate).  The sums over pixels are float atomics: the
 * last bits of a gradient may differ from run to run (gsr_backward_ordered, below, has a mode in
 * which they do not). */
typedef struct {
    const float *dL_dcolor; /* [3,H,W] */
} gsr_backward_inputs;
typedef struct {
    float *dL_dmeans3D;   /* [P,3] */
    float *dL_dmeans2D;   /* [P,3], units above */
    float *dL_dopacity;   /* [P,1] */
    float *dL_dcolors;    /* [P,3] w.r.t. the per-Gaussian rgb after the clamp */
    float *dL_dconic;     /* [P,3] a,b,c of the conic (b once, as stored) */
    float *dL_dsh;        /* [P,M,3] */
    float *dL_dscales;    /* [P,3] */
    float *dL_drotations; /* [P,4] */
    float *dL_dcov3D;     /* [P,6] */
} gsr_gradients;
int gsr_backward(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                 const gsr_backward_inputs *in, gsr_gradients *grads, void *stream);
/* gsr_backward that also takes the gradients of the per-pixel planes of the same composite:
 * depth_map and inv_depth_map (gsr_forward_depth) and final_T (gsr_outputs).  (Additive to ABI 4:
 * gsr_backward, gsr_backward_inputs and gsr_gradients keep their layout.)
 * With alpha_i, T_i and w_i = alpha_i T_i of the splats i = 1..n a pixel composites,
 *   depth_map     = sum_i z_i w_i        a colour channel with feature z_i,     background 0
 *   inv_depth_map = sum_i (1 / z_i) w_i  a colour channel with feature 1 / z_i, background 0
 *   final_T       = prod_i (1 - alpha_i) a colour channel with feature 0,       background 1
 * -- the channel identity gsr_forward_depth states bit for bit -- so their gradients run through
 * gsr_backward's recursion as three more channels.  With g = dL/dcolor, gd = dL/ddepth_map,
 * gi = dL/dinv_depth_map and gT = dL/dfinal_T at the pixel, and every gate, skip and cap held
 * constant exactly as in gsr_backward:
 *   - the value carried back to front starts at g . bg + gT (gsr_backward: g . bg);
 *   - the per-splat term is gc_i = g . c_i + gd z_i + gi (1 / z_i), and dL/dalpha_i =
 *     T_i (gc_i - r_i) with r_i the carried value behind splat i; from it dL_dmeans2D, dL_dconic
 *     and dL_dopacity follow as in gsr_backward (the 0.99 cap passes nothing);
 *   - one more sum per splat, the direct path through the features:
 *     dL/dz_i += w_i (gd - gi (1 / z_i)^2), with 1 / z_i the rounded float32 quotient the forward
 *     uses and its derivative taken as -(1 / z_i)^2.
 * z is the view-space depth, z = vm[2] x + vm[6] y + vm[10] z_world + vm[14] (column-major), so the
 * per-Gaussian stage adds (vm[2], vm[6], vm[10]) dL/dz to dL_dmeans3D.  The z <= 0.2 cull is a
 * gate: a listed Gaussian has a finite z > 0.2, a culled one gets exact zeros.
 * final_T is here because every consumer of the two depth planes divides by 1 - final_T: the
 * expected depth of the covered part, and stereo.metric_disparity(normalise=True).
 * dL_ddepths (optional output, [P]) is dL/dz through the features z and 1 / z only -- the new sum
 * by itself, not the gradient through the projection (depths is not an input).  The plane features
 * are not colours: dL_dcolors gets nothing from them; every member of gsr_gradients means what it
 * means in gsr_backward.
 * A NULL struct, or one whose three inputs are NULL, is gsr_backward itself: the same kernels, the
 * same arguments, dL_dcolor required; dL_ddepths, if given, is then zero-filled.  With at least one
 * plane gradient in->dL_dcolor may be NULL and reads as zero.  Everything else is gsr_backward's:
 * whole frames only, a function of its inputs (it rebuilds the lists), zeroes then fills each
 * gradient given, exact zeros for culled Gaussians, timing through gsr_backward_times, and
 * gsr_get_binning exports the backward's lists afterwards. */
typedef struct {
    const float *dL_ddepth_map;     /* [H,W] or NULL */
    const float *dL_dinv_depth_map; /* [H,W] or NULL */
    const float *dL_dfinal_T;       /* [H,W] or NULL */
    float *dL_ddepths;              /* optional output [P]: dL/dz through the features only */
} gsr_plane_gradients;
int gsr_backward_planes(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                        const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                        gsr_gradients *grads, void *stream);
/* gsr_backward_planes that also returns the gradients of the camera: the view matrix, the
 * projection matrix and the camera position of gsr_raster_settings.  (Additive to ABI 4.)
 * The three are independent arguments of the forward, so each gradient is the partial with the
 * other two held fixed; a caller whose projmatrix and campos are functions of a pose chains them.
 * With q = (x, y, z, 1) the world mean of a Gaussian the forward kept (radii > 0), vm and pm the
 * column-major matrices and c = campos, the forward reads the camera in four places, and each
 * gradient is the sum over the kept Gaussians of:
 *   1. the projective divide, hom_r = sum_c pm[4c+r] q_c, of which hom.x, hom.y and hom.w are
 *      used:  dL/dpm[4c+r] += dhom_r q_c for r = 0, 1, 3.  Nothing reads hom.z (the depth is the
 *      view matrix's), so row 2 of dL_dprojmatrix is exactly 0;
 *   2. the view transform, t_r = sum_c vm[4c+r] q_c, r < 3:  dL/dvm[4c+r] += dt_r q_c, with dt
 *      through the Jacobian J of the EWA covariance, the 1.3 tan clamp as gsr_backward
 *      differentiates it (on its flat side dt.x or dt.y is 0 and dt.z takes the clamped ratio
 *      times it) and, with plane gradients, dL/dz through the features, because z = t_2;
 *   3. the view rotation in A = J R, R[r][c] = vm[4c+r], c < 3:  dL/dR = J^T dL/dA, that is
 *      dL/dvm[4c+0] += J00 dA0[c], dL/dvm[4c+1] += J11 dA1[c],
 *      dL/dvm[4c+2] += J02 dA0[c] + J12 dA1[c];
 *   4. the SH direction (p - c) / |p - c|:  dL/dc -= (dd - dir (dir . dd)) / len, minus the term
 *      dL_dmeans3D gets; exactly 0 with colors_precomp.
 * Entries the forward never reads get exactly 0: row 3 of the view matrix (vm[3], vm[7], vm[11],
 * vm[15]) and row 2 of the projection.  Everything gsr_backward holds constant stays constant
 * (the z <= 0.2 cull, det == 0, rect and tile membership, the depth order, the skips, the cap, the
 * termination), and so do tanfovx, tanfovy and the focal lengths derived from them: the
 * intrinsics get no gradient.
 * The 27 sums are reduced without atomics (per block, then over the blocks in double, rounded
 * once): given the same per-Gaussian 2D gradients they are bit-reproducible; those come from
 * gsr_backward's float atomics, so the last bits may still differ from run to run.
 * A NULL camera, or one with three NULL members, is gsr_backward_planes itself: the same kernels,
 * the same arguments.  planes may be NULL as there.  Each buffer given is written, not accumulated
 * into; with P == 0, or nothing on any list, it is zero-filled.  Everything else is
 * gsr_backward_planes': whole frames only (a strip: GSR_E_INVALID, nothing written), a function
 * of its inputs, exact zeros for culled Gaussians' own gradients, the debug stage checks, and
 * timing through gsr_backward_times with the new work inside ms[2]. */
typedef struct {
    float *dL_dviewmatrix; /* device [16], the input's column-major layout, or NULL */
    float *dL_dprojmatrix; /* device [16] or NULL */
    float *dL_dcampos;     /* device [3]  or NULL */
} gsr_camera_gradients;
int gsr_backward_camera(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                        const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                        const gsr_camera_gradients *camera, gsr_gradients *grads, void *stream);

/* gsr_forward_surface and gsr_backward_camera with the antialiasing option of upstream's
 * GaussianRasterizationSettings(antialiasing=...): the Mip-Splatting compensation of the 0.3-pixel
 * screen-space dilation.  (Additive to ABI 4; no existing struct changes layout.)
 * Every Gaussian's 2D covariance gets + 0.3 I (computeCov2D); without the option the opacity stays
 * what it was, so a splat much smaller than a pixel is drawn with far more energy than it has.
 * With (a', b, c') the 2D covariance before the dilation, h = 0.3f, a = a' + h, c = c' + h (the
 * values the conic is built from), all in float32 and in this order:
 *     D0  = a' * c' - b * b          (before the dilation)
 *     D   = a  * c  - b * b          (the det the conic divides by)
 *     rho = D0 / D
 *     s   = sqrtf(fmaxf(0.000025f, rho))
 *     o_eff = opacity * s
 * With antialiasing == 1, o_eff takes the place of opacity everywhere downstream of the
 * preprocess: the blend's record, the conic_opacity output (its fourth component, as upstream),
 * the cull data and the span words (tight binning cuts to the alpha >= 1/255 ellipse of the
 * effective opacity) and the blend cull.  Nothing else moves: radii, rects, tiles_touched,
 * num_rendered, the depth keys, means2D, the conic's three components and rgb are the plain
 * forward's bits.  Consequences:
 *   - identity: an antialiased forward is, bit for bit in every output (image, final_T, n_contrib,
 *     the depth and the median planes), the plain forward of the same scene whose opacities are
 *     the antialiased run's conic_opacity[:, 3] -- except conic_opacity[:, 3] itself, which the
 *     plain run passes through;
 *   - the tight lists of an antialiased frame are in-order subsequences of the plain frame's;
 *     num_rendered is equal;
 *   - the floor is a gate: rho <= 0.000025f (which covers D0 <= 0 by rounding, a zero
 *     cov3D_precomp and NaN) gives s = sqrtf(0.000025f);
 *   - the option belongs to the call, not to the context: a plain frame after an antialiased one
 *     on the same context has the plain bits, and the other way round.  The preprocess runs
 *     outside the recorded frame graphs, so both kinds of frame share their graphs;
 *   - the splat composite only: the GL shadings have no such option;
 *   - strips, radii == NULL, debug, prefiltered and every option work as in the plain forward.
 * The backward differentiates that forward as written; gates are constants.  With G = dL/do_eff
 * (what the blend's backward accumulates, gsr_backward's dL_dopacity):
 *     dL_dopacity = G s;
 *   on the floor's flat side nothing more; otherwise dL/drho = G opacity / (2 s) and
 *     drho/da' = (c' D - D0 c) / D^2,  drho/dc' = (a' D - D0 a) / D^2,
 *     drho/db  = -2 b (D - D0) / D^2   (b the one stored off-diagonal entry)
 * are added to the gradient of the 2D covariance where the conic's gradient becomes it, so
 * dL_dcov3D, dL_dscales, dL_drotations, dL_dmeans3D (through J) and the camera's dL_dviewmatrix
 * (through J and R) receive the term.  dL_dconic keeps its meaning (the gradient of the conic's
 * three components); the planes' and the camera's gradients compose with the option; culled
 * Gaussians still get exact zeros; the backward's rebuild runs the antialiased preprocess.
 * A NULL filter, or antialiasing == 0, is gsr_forward_surface / gsr_backward_camera itself: the
 * same kernels, the same arguments.  Any other value than 0 or 1: GSR_E_INVALID, nothing
 * written.  (The struct leaves room for the dilation's size; 0.3 is a constant for now.) */
typedef struct {
    int32_t antialiasing; /* 0 or 1 */
} gsr_filter_settings;
int gsr_forward_filtered(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                         gsr_outputs *out, const gsr_depth_outputs *depth,
                         const gsr_surface_outputs *surface, const gsr_filter_settings *filter,
                         void *stream);
int gsr_backward_filtered(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                          const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                          const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                          gsr_gradients *grads, void *stream);
/* gsr_backward_filtered with a choice of how the sums over pixels are formed.  (Additive to ABI 4;
 * no existing struct changes layout.)
 * deterministic == 1: every gradient of the call -- each member of gsr_gradients, dL_ddepths and
 * the camera's three -- has the same bits on every call with the same inputs, whichever context,
 * stream or option set (GSR_OPT_DEPTH_SORT, GSR_OPT_BLEND_CULL, GSR_OPT_SECOND_STREAM, ...) runs
 * it and whatever ran before it.  No float atomics, no sort:
 *   - in upstream's (untight) lists, which the backward rebuilds, a Gaussian is listed in exactly
 *     the tiles of its rect, so every (Gaussian, tile, 8x8 quadrant) owns a slot: the blend's
 *     backward stores that quadrant's 9 sums (10 with plane gradients) there with plain stores and
 *     sets the slot's mark, one byte per slot (the four quadrant waves of a tile write different
 *     bytes); only the marks are zeroed per call, an unmarked slot is never read;
 *   - a gather then fills each Gaussian's 2D gradient row: it adds the marked slots of the rect in
 *     a fixed order (lane j of 16 takes slots j, j + 16, ... in tile row-major, then quadrant
 *     order; the 16 lanes by a fixed tree), from +0.0, in double, rounded once.  The order depends
 *     on the Gaussian's rect and marks only;
 *   - the per-Gaussian stage and the camera's 27 sums follow unchanged (they have no atomics).
 * The values differ from gsr_backward_filtered's by the rounding of those sums only (a row with
 * at most two addends has the same bits in both modes); culled Gaussians and Gaussians no pixel
 * composites still get exact zeros.
 * Workspace of the context, grown on demand and freed with it, with K = num_rendered: slots 144 B
 * per list entry (160 B with plane gradients), marks 4 B per list entry, 8 B per Gaussian; at
 * K = 9,594,635 that is 1.38 GB (1.54 GB), 38 MB.  A failed allocation: GSR_E_NOMEM, nothing
 * written.  Slots are indexed with 32 bits: a frame with K >= 2^30 is refused with GSR_E_INVALID,
 * nothing written.
 * A NULL order, or deterministic == 0, is gsr_backward_filtered itself: the same kernels, the same
 * arguments.  Any other value than 0 or 1: GSR_E_INVALID, nothing written.  Everything else is
 * gsr_backward_filtered's: whole frames only (a strip: GSR_E_INVALID), planes, camera and filter
 * as there, gsr_get_binning afterwards, and gsr_backward_times with the scan, the zeroing of the
 * marks and the gather inside ms[1]. */
typedef struct {
    int32_t deterministic; /* 0 or 1 */
} gsr_backward_order;
int gsr_backward_ordered(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                         const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                         const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                         const gsr_backward_order *order, gsr_gradients *grads, void *stream);
/* gsr_backward_ordered on a strip of tile rows: the one backward entry that honours
 * s->tile_row_begin / tile_row_end (every entry above keeps refusing a strip).  (Additive to ABI 4;
 * no existing struct changes layout.)
 * Every term a pixel adds to any gradient is proportional to that pixel's own image gradient, so
 * the backward on the strip [begin, end) is the whole-frame backward with the image gradients zero
 * outside the strip's pixel rows y0 = 16 begin .. min(H, 16 end), rows = min(H, 16 end) - y0:
 *   - the inputs are strip-local, like the forward's outputs: in->dL_dcolor is [3, rows, W], the
 *     three plane gradients [rows, W];
 *   - the outputs are whole-scene: every gsr_gradients member [P, ...], dL_ddepths [P], the
 *     camera's three buffers of their fixed sizes;
 *   - on a strip that is a proper subset of the tile rows, a Gaussian without a tile in it (the
 *     rebuild's strip rect is empty; culled Gaussians included) leaves the per-Gaussian stage before
 *     any arithmetic: +0.0 in every gradient, and exactly 0 added to the camera's sums.  A Gaussian
 *     with a tile that no pixel composites gets zeros of either sign, as on a whole frame;
 *   - over a partition of the tile rows into strips the strips' gradients, the camera's included,
 *     add up to the whole frame's up to float32 rounding.
 * deterministic == 1: the same bits on every call, as gsr_backward_ordered.  The slots exist for
 * the strip's (Gaussian, tile) pairs only: with K the strip's num_rendered the workspace is 144 B
 * (160 B with plane gradients) plus 4 B of marks per list entry of the strip, and K < 2^30 is asked
 * of the strip's K.  The gather's order is a function of a Gaussian's strip rect and marks alone, so
 * a Gaussian whose rect lies wholly inside the strip's rows has the bits of the whole-frame
 * deterministic backward under the image gradient zeroed outside the strip, and the strip
 * (0, grid_y) has those bits for every Gaussian and for the camera.
 * tile_row_begin == tile_row_end == 0 is gsr_backward_ordered itself: the same kernels, the same
 * arguments.  A bad strip (begin < 0, end > grid_y, begin >= end): GSR_E_INVALID, nothing written.
 * Everything else is gsr_backward_ordered's: a function of its inputs, zeroes then fills each
 * gradient, debug, gsr_backward_times, planes, camera, filter and order as there; gsr_get_binning
 * afterwards exports the strip's lists, as after a strip forward. */
int gsr_backward_strip(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                       const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                       const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                       const gsr_backward_order *order, gsr_gradients *grads, void *stream);
/* gsr_forward_filtered and gsr_backward_strip with C channels of the caller's own per Gaussian: a
 * semantic or language embedding, normals, a soft label field, any learned C-vector.  (Additive to
 * ABI 4; no existing struct, entry point or kernel changes.)
 * Forward.  features is [P, C] float32, row-major; feature_map is [C, rows, W] float32, strip-local
 * like color:
 *   feature_map[c, y, x] = sum_k features[id_k, c] * w_k
 * over exactly the splats the colour composites at that pixel (the list order, the power > 0 and
 * alpha < 1/255 skips, the 0.99 cap and the T < 1e-4 termination are the colour's), with w_k the
 * very weight of the colour channels in the context's arithmetic (GSR_OPT_BLEND_FAST 0 or 1), as
 * gsr_forward_depth defines it.  There is no background term, as for the depth planes: a pixel that
 * composites nothing is 0, and normalising by 1 - final_T is the caller's business.
 * Twin property (tests/test_gpu_feature_maps.py): plane c is, bit for bit, a colour channel of a
 * gsr_forward of the same scene with colors_precomp[:, j] = features[:, c] and bg = 0 -- in both
 * arithmetic modes, on strips, with tight or upstream lists, with and without n_contrib, with frame
 * graphs, with the blend cull on or off, and under antialiasing against the antialiased twin.
 * colors_precomp is copied unclamped by the preprocess, so negative features obey the twin too.
 * Everything else the call returns is the bits of the same call without features: the image, radii,
 * every gsr_outputs member, the depth and median planes, num_rendered and the lists gsr_get_binning
 * exports.  Rows of Gaussians that are on no list (culled, or outside the strip) are never read:
 * NaN in such rows reaches no output.  P == 0 and empty lists give all-zero planes.
 * The feature channels run as launches of their own over the lists the call has built, after the
 * colour blend, in chunks of 16, 8 or 4 channels (the last one padded inside the kernel: no word at
 * or beyond C is read or written); they are timed inside the "blend" stage.  Frame graphs: the
 * launches come directly after the recorded chains with the call's pointers, nothing of a feature
 * is recorded, and a frame whose list outgrew the capacity writes no plane before it is rendered
 * again.  features rows may sit at any 4-byte-aligned address and C need not be a multiple of 4:
 * the rows are gathered as float4 where they are 16-byte aligned (the pointer, and C % 4 == 0) and
 * word by word otherwise, with the same bits.
 * A NULL feat, or one with feature_map NULL, is gsr_forward_filtered itself: the same kernels, the
 * same arguments.  Refused with GSR_E_INVALID and nothing written: C < 1 or C > GSR_MAX_FEATURES,
 * features NULL with a map given (P > 0).  The splat composite only: the GL shadings have no
 * features (the entry takes no shading).
 *
 * Backward.  dL_dfeature_map is [C, rows, W], strip-local.  With gF the pixel's C feature
 * gradients, f_i splat i's feature row, and every gate held constant as in gsr_backward:
 *   - dL_dfeatures[id_i, c] += gF_c w_i: final, there is no per-Gaussian stage behind it;
 *   - the per-splat term of the recursion gains gF . f_i:
 *     gc_i = g . c_i + gd z_i + gi / z_i + gF . f_i;
 *   - the carried value's start gains nothing: the features' background is 0;
 *   - dL/dalpha_i = T_i (gc_i - r_i) then feeds dL_dmeans2D, dL_dconic, dL_dopacity and everything
 *     behind them, the camera's sums and the antialiasing term included, unchanged;
 *   - dL_dcolors gets nothing from features;
 *   - culled Gaussians (and, on a strip, Gaussians without a tile in it) get exact zeros in
 *     dL_dfeatures: the buffer is zeroed and then filled, never accumulated into.
 * dL/dalpha and the six geometry sums are linear in the channel set, so the feature channels run
 * as launches of their own beside the colour / planes blend-backward, each carrying r for its own
 * channels and adding into the same zeroed 2D gradient rows: the same gradient up to the float32
 * rounding of the sums.  They are timed inside ms[1] of gsr_backward_times.
 * A NULL feat, or one with dL_dfeature_map NULL, is gsr_backward_strip itself: the same kernels,
 * the same arguments.  tile_row_begin / tile_row_end are honoured exactly as there.  With a feature
 * gradient present in->dL_dcolor may be NULL and reads as zero; then no colour blend-backward
 * runs.  dL_dfeatures may be NULL when only the geometry's gradients are wanted.  Refused with
 * GSR_E_INVALID and nothing written: C < 1 or C > GSR_MAX_FEATURES, features NULL with a gradient
 * given, and order->deterministic == 1 together with a feature gradient (the deterministic slots
 * hold 9 or 10 sums per (Gaussian, tile, quadrant) and have no room for C more). */
#define GSR_MAX_FEATURES 256
typedef struct {
    int32_t C;             /* channels per Gaussian, 1..GSR_MAX_FEATURES */
    const float *features; /* [P, C] */
    float *feature_map;    /* [C, rows, W] or NULL */
} gsr_feature_outputs;
int gsr_forward_features(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                         gsr_outputs *out, const gsr_depth_outputs *depth,
                         const gsr_surface_outputs *surface, const gsr_filter_settings *filter,
                         const gsr_feature_outputs *feat, void *stream);
typedef struct {
    int32_t C;
    const float *features;        /* [P, C] */
    const float *dL_dfeature_map; /* [C, rows, W] or NULL */
    float *dL_dfeatures;          /* [P, C] or NULL */
} gsr_feature_gradients;
int gsr_backward_features(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                          const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                          const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                          const gsr_backward_order *order, const gsr_feature_gradients *feat,
                          gsr_gradients *grads, void *stream);
/* gsr_backward_features that also returns the absolute gradient of the 2D means (AbsGS'
 * "homodirectional" gradient, gsplat's absgrad), for densification: dL_dmeans2D is a signed sum
 * over the pixels a Gaussian covers, and over a blurry region the pixels' terms point in opposite
 * directions and cancel; this output adds their magnitudes.  (Additive to ABI 4; no existing
 * struct, entry point or kernel changes.)
 * With v0_i(p), v1_i(p) pixel p's addends to the x and y word of Gaussian i's 2D gradient row in
 * the blend's backward -- dL/dalpha_i(p) = T_i (gc_i - r_i) times d alpha_i / d mean2D_i, in
 * pixels, where the per-splat term gc_i = g . c_i + gd z_i + gi / z_i holds every image-like
 * gradient of the call (colour and planes), so "per pixel" is the pixel's total over all channels,
 * not per channel; the gates and the 0.99 cap are gsr_backward's, and a capped or
 * non-contributing (pixel, splat) pair adds 0:
 *   dL_dmeans2D_abs[i] = (0.5 W sum_p |v0_i(p)|, 0.5 H sum_p |v1_i(p)|, 0)      [P, 3] float32
 * in dL_dmeans2D's shape and units (its factors 0.5 W, 0.5 H), so that dL_dmeans2D[i] is the same
 * sums without the bars.  The absolute value is taken per pixel, in float32, before any sum across
 * pixels; the sums then go the way of the row's other words (float atomics, or with
 * deterministic == 1 the slots and the gather in double: the same bits on every call).  Exact 0.0
 * in all three words for a Gaussian the forward culls, on a strip for a Gaussian without a tile in
 * the strip, and for a Gaussian no pixel composites.  The call zeroes, then fills, as for every
 * other gradient; over a partition of the tile rows into strips the strips' outputs add up to the
 * frame's.  Every other gradient of the call is what it is without the option: the same bits with
 * deterministic == 1, the same up to the order of the atomics without.
 * With deterministic == 1 a slot holds two more sums: 176 B per list entry (192 B with plane
 * gradients) where gsr_backward_ordered has 144 B (160 B); at K = 9,594,635 that is 1.69 GB
 * (1.84 GB).  The marks and the K < 2^30 rule are unchanged.  Timed inside ms[1] (the sums) and
 * ms[2] (the scaling) of gsr_backward_times.
 * A NULL abs, or one with dL_dmeans2D_abs NULL, is gsr_backward_features itself: the same kernels,
 * the same arguments.  Refused with GSR_E_INVALID and nothing written: dL_dmeans2D_abs together
 * with a feature gradient (the feature channels add their share of dL/dalpha in passes of their
 * own, and the absolute value of a pixel's total cannot be split over passes).  P == 0 writes
 * nothing. */
typedef struct {
    float *dL_dmeans2D_abs; /* [P, 3] or NULL */
} gsr_abs_gradients;
int gsr_backward_abs(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *s,
                     const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                     const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                     const gsr_backward_order *order, const gsr_feature_gradients *feat,
                     const gsr_abs_gradients *abs, gsr_gradients *grads, void *stream);
/* The stage times (ms, HIP events on the backward's stream) of the last gsr_backward run while
 * gsr_set_timing was not 0: ms[0] the rebuild (per-Gaussian stage, depth sort, lists), ms[1] the
 * blend's backward (with the zeroing of its sums), ms[2] the per-Gaussian backward.  Waits for
 * that backward; writes min(n, 3); returns 3.  The rebuild records no forward stage times. */
int gsr_backward_times(gsr_context *ctx, float *ms, int n);

/* Binning state of the last gsr_forward (or gsr_backward) on this context: the pair lists its
 * blend read.  Writes
 * the sizes (list_entries = K, the entries of the lists; num_tiles = T, tiles of the whole
 * frame) and, for each non-NULL caller-owned
 * DEVICE buffer, copies: point_list[K] Gaussian ids sorted by (tile, depth); point_tiles[K]
 * their global tile ids; ranges[2*T] = [start,end) per tile (tiles outside the strip stay 0,0,
 * as upstream's memset leaves unused tiles).  With upstream's lists (GSR_OPT_TIGHT_BINNING 0, a
 * strip, or a forward that asked for n_contrib) K is the forward's num_rendered; after a tight
 * forward the lists are the tight ones and K <= num_rendered (each tile's list is an in-order
 * subsequence of upstream's: tests/test_gpu_tight_pin.py checks that against the oracle).  Call
 * once with NULL buffers to size them.  Synchronises `stream`. */
int gsr_get_binning(gsr_context *ctx, uint32_t *point_list, uint32_t *point_tiles,
                    uint32_t *ranges, int64_t *list_entries, int32_t *num_tiles, void *stream);

/* Per tile row of the last gsr_forward's strip, its (Gaussian, tile) pair count:
 * row_pairs[r] for r < n_rows = tile_row_end - tile_row_begin (DEVICE buffer, written on
 * `stream`, no synchronisation).  The multi-GPU strip split (strips.StripBalancer) weights its
 * next boundaries by these counts.  No reference counterpart: the reference renders each frame
 * on one device (renderer_cuda.py:205-224). */
int gsr_tile_row_pairs(gsr_context *ctx, uint32_t *row_pairs, int32_t n_rows, void *stream);

/* GaussianRasterizer.markVisible: visible[i] = view-space z > 0.2. */
int gsr_mark_visible(gsr_context *ctx, const float *means3D, int64_t P, const float *viewmatrix,
                     const float *projmatrix, uint8_t *visible, void *stream);

/* Depth-sort backend (renderer_ogl.py:10-19): depth = (view @ [xyz,1]).z with `view` the HOST
 * 4x4 row-major (math-layout) matrix the viewer passes; out_index[P] int32 = stable ascending
 * argsort of depth (== np.argsort(depth, kind='stable')).  out_depth[P] optional. */
int gsr_depth_argsort(gsr_context *ctx, const float *xyz, int64_t P, const float *view_host16,
                      int32_t *out_index, float *out_depth, void *stream);

/* ---- PLY loader (replaces util_gau.load_ply, util_gau.py:63-125) ----
 * Reads a 3D Gaussian Splatting PLY (binary little / big endian or ascii) whose vertex
 * element has x y z, f_dc_0..2, 45 f_rest_* (SH degree 3), opacity, scale_0..2, rot_0..3, and
 * returns the reference's activated data as SoA float32 arrays: xyz[P*3], rot[P*4]
 * (normalised quaternion), scale[P*3] (exp), opacity[P] (sigmoid), sh[P*48] (DC, then the 15
 * rest coefficients channel-interleaved), plus the bounding box and mean of the positions.
 * gsr_ply_probe reads the header only (P, sh_coeffs = 16).  gsr_ply_load fills the caller's
 * arrays: host memory when device == 0, device memory (uploaded on `stream`, synchronised
 * before return) otherwise.  info->P must be 0 or the probed count.  Errors: GSR_E_INVALID with
 * gsr_last_error() naming the problem (missing property, wrong f_rest count, short file). */
typedef struct gsr_ply_info {
    int64_t P;          /* vertices */
    int32_t sh_coeffs;  /* 16 (degree 3, the only layout the reference loader accepts) */
    int32_t binary;     /* 1 binary, 0 ascii */
    float bbox_min[3];  /* util_gau.py:80-85: min / max / mean of xyz (gsr_ply_load) */
    float bbox_max[3];
    float center[3];
} gsr_ply_info;

int gsr_ply_probe(const char *path, gsr_ply_info *info);
int gsr_ply_load(const char *path, gsr_ply_info *info, float *xyz, float *rot, float *scale,
                 float *opacity, float *sh, int device, void *stream);

/* ---- Scene files: a fit's raw tensors as upstream's save_ply writes them, and back ----------
 * The scene is the fit's own tensors, not activated: xyz[P*3], f_dc[P*1*3], f_rest[P*(M-1)*3],
 * opacity[P], scaling[P*3], rotation[P*4], M = (d + 1)^2 coefficients for a degree d = 0..4.
 *
 * The file: the header plyfile writes for upstream's save_ply ("ply", "format
 * binary_little_endian 1.0", "element vertex <P>", one "property float <name>" line for each of
 * x y z nx ny nz f_dc_0..2 f_rest_0..3(Mo-1)-1 opacity scale_0..2 rot_0..3, "end_header"; '\n'
 * line ends, no comment), then P rows of R = 17 + 3 (Mo - 1) little-endian float32 words:
 *   columns 0..2               xyz[p][:]
 *   columns 3..5               +0.0 (the normals)
 *   column  6 + c              f_dc[p][0][c]
 *   column  9 + c (Mo-1) + j   f_rest[p][j][c] for j < M - 1, else +0.0
 *                              (upstream's transpose(1, 2).flatten(1): c the channel, j the
 *                              coefficient)
 *   column  9 + 3 (Mo-1)       opacity[p], then scaling[p][:], then rotation[p][:]
 * Every word is a bit copy of a word of the scene or the bits of +0.0f: NaN payloads, infinities
 * and -0.0 survive.  Mo = file_sh_coeffs is the file's coefficient count: 0 means M; a larger
 * square pads the f_rest columns with +0.0 (Mo = 16 makes a degree-0..2 scene a file that
 * gsr_ply_load accepts); Mo < M is refused.
 *
 * gsr_ply_save: device == 0: the pointers are host memory and the rows are packed in plain C++.
 * Otherwise they are device memory of the calling thread's current device: k_ply_pack writes
 * chunk_rows packed rows into one of two device slots, hipMemcpyAsync copies the slot into one
 * of two pinned host slots, and the host write()s one slot while the next chunk packs and
 * copies -- 2 x chunk_rows x 4R bytes on either side whatever P is, no full-size host copy.  The
 * stream is synchronised before return.  The scene is only read; pointers need 4-byte alignment
 * only.  chunk_rows == 0 is the library's default (GSR_PLY_CHUNK_ROWS); values above
 * GSR_PLY_MAX_CHUNK_ROWS are taken as that.  The bytes go to "<path>.tmp.<pid>", renamed over
 * `path` after the last one; any failure removes the temporary file and leaves a file already
 * at `path` as it was.  P == 0 writes the header alone.
 *
 * gsr_ply_probe_scene fills info->P and info->sh_coeffs from the header alone.
 * gsr_ply_load_scene fills the six tensors (f_rest may be NULL when M == 1) with the raw
 * values: the inverse of the column table, no activation, no bounding box.  scene->P and
 * scene->sh_coeffs must be what the probe reported.  It reads what gsr_ply_load reads, by the
 * same rules (either endianness or ascii, any scalar type per property converted like numpy's
 * astype(float32) -- float properties are bit copies --, any property order, f_rest_* / scale_* /
 * rot* sorted by integer suffix, other properties ignored), with 3 (M - 1) f_rest properties for
 * any M above.  device != 0: a little-endian file whose vertex properties are all float goes in
 * row chunks through pinned staging to the device, where k_ply_unpack scatters them into the
 * tensors; every other file is converted on the host and uploaded.  Both give the same bits;
 * the stream is synchronised before return.
 *
 * Refused with GSR_E_INVALID before any HIP call and before the file is touched: a NULL path,
 * scene / info or required pointer (P == 0 needs none); P < 0 or P >= 2^30; sh_coeffs or
 * file_sh_coeffs that is no square of 1..5; file_sh_coeffs < sh_coeffs; chunk_rows < 0.
 * GSR_E_INVALID too: a file that cannot be created or opened, a short write or a short file, an
 * f_rest count that is not 3 (M - 1) for such an M, a P or sh_coeffs that is not the file's. */
#define GSR_PLY_CHUNK_ROWS 65536
#define GSR_PLY_MAX_CHUNK_ROWS 1048576
typedef struct gsr_ply_scene {
    int64_t P;
    int32_t sh_coeffs;      /* M of the tensors */
    int32_t file_sh_coeffs; /* Mo of the file written; 0 = M (gsr_ply_save only) */
    int64_t chunk_rows;     /* rows per staging slot; 0 = the library's default */
    float *xyz, *f_dc, *f_rest, *opacity, *scaling, *rotation;
} gsr_ply_scene;

int gsr_ply_save(const char *path, const gsr_ply_scene *scene, int device, void *stream);
int gsr_ply_probe_scene(const char *path, gsr_ply_scene *info);
int gsr_ply_load_scene(const char *path, gsr_ply_scene *scene, int device, void *stream);

/* ---- Stereo dataset outputs ----
 * gsr_disparity_colors: colors[3*i..3*i+2] = d_i for every Gaussian, with
 *   d = |(ndc_x(p) + 1)/2 - (ndc_x(p + (baseline, 0, 0)) + 1)/2|, ndc_x(q) = (P V [q;1]).x /
 *   (P V [q;1]).w -- gau_vert.glsl:182-207.  view_host16 / proj_host16 are HOST row-major
 *   (math-layout) 4x4 matrices: the GL view and projection (util.py:58-105), NOT the negated /
 *   transposed upstream pair.  Render these colours as colors_precomp with scale_modifier x 1.2
 *   (gau_vert.glsl:152-156) to get the viewer's disparity image.
 * gsr_pack_image: chw = the rasterizer's (3,H,W) float image (format R16 reads channel 0 only);
 *   output row r comes from input row (flip_rows ? H-1-r : r).
 *     GSR_PACK_RGBA_F32: float[H][W][4], alpha 1 (renderer_cuda.py:226-228, no flip);
 *     GSR_PACK_RGB8:     uint8[H][W][3] = round(clamp(v,0,1)*255) (GL unorm conversion);
 *     GSR_PACK_R16:      uint16[H][W] = uint16(v*65535) (numpy astype: truncate, wrap). */
enum {
    GSR_PACK_RGBA_F32 = 0,
    GSR_PACK_RGB8 = 1,
    GSR_PACK_R16 = 2
};
int gsr_disparity_colors(const float *means3D, int64_t P, const float *view_host16,
                         const float *proj_host16, float baseline, float *colors, void *stream);
int gsr_pack_image(const float *chw, int32_t H, int32_t W, int32_t format, int32_t flip_rows,
                   void *out, void *stream);

/* ---- The photometric loss of a fit: fused L1 + D-SSIM of one image against a target ----
 * (additive to ABI 4)
 *
 *   loss = (1 - lambda) * l1 + lambda * (1 - ssim),  l1 = mean|image - target|, ssim = mean(map)
 *
 * over all N = C*H*W elements of two contiguous float32 [C, H, W] images whose channels are
 * independent.  The window is g (x) g with g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10,
 * normalised to sum 1 (the kernels hold the float32 roundings of the float64 values); conv(x) is
 * the "same" correlation with zero padding of 5 per channel, so images smaller than the window
 * are valid.  With mu1 = conv(image), mu2 = conv(target), s1 = conv(image^2) - mu1^2,
 * s2 = conv(target^2) - mu2^2, s12 = conv(image target) - mu1 mu2, C1 = 0.01^2, C2 = 0.03^2:
 *   A = mu1^2 + mu2^2 + C1, B = s1 + s2 + C2, Cc = 2 mu1 mu2 + C1, D = 2 s12 + C2,
 *   map = Cc D / (A B).
 * NaN and infinities propagate; nothing is clamped.  A strip image is an image like any other:
 * its loss is that of the strip alone, zero padded at the strip's edges.  The frame's loss on a
 * strip, seams unpadded, is gsr_image_loss_window's (below).
 *
 * Neither call takes a context (no mutex, no ordering against frames in flight), allocates or
 * synchronises: all memory is the caller's and all work is enqueued on `stream`.  No atomics:
 * every block writes its two partial sums to `workspace` and one finishing block adds them in
 * a fixed order in double and rounds once, so `values` and `dL_dimage` have the same bits on
 * every call with the same inputs, on any stream.
 *
 * gsr_image_loss_workspace: the bytes of device scratch gsr_image_loss needs for C, H, W
 *   (GSR_E_INVALID for a size < 1 or C*H*W >= 2^31).
 * gsr_image_loss: values = device float[3] (loss, l1, ssim).  saved = device [3, C, H, W], the
 *   partial derivatives of map the backward reads,
 *     dm_dmu1 = 2 mu2 D/(A B) - 2 mu2 Cc/(A B) - 2 mu1 Cc D/(A^2 B) + 2 mu1 Cc D/(A B^2),
 *     dm_ds1  = -Cc D/(A B^2),   dm_ds12 = 2 Cc/(A B),
 *   or NULL when no gradient is wanted: then nothing of them is computed or written.
 * gsr_image_loss_backward: the gradient with respect to `image` (target is a constant).  With
 *   gl = *dL_dloss (a device float[1], so that no host wait is needed; NULL = 1.0) and
 *   gm = -gl lambda / N,
 *     dL_dimage = gm conv(dm_dmu1) + 2 image gm conv(dm_ds1) + target gm conv(dm_ds12)
 *                 + gl (1 - lambda)/N sign(image - target),   sign(0) = 0
 *   (the window is symmetric, so conv is its own adjoint).  dL_dimage [C, H, W] is written, not
 *   accumulated into.
 * Refused with GSR_E_INVALID before any HIP call, nothing written: a NULL in, image, target or
 * values; a size < 1 or C*H*W >= 2^31; lambda outside [0, 1] or NaN; a NULL workspace; the
 * backward's NULL saved or dL_dimage. */
typedef struct gsr_image_loss_inputs {
    int32_t C, H, W;
    float lambda;        /* the weight of the D-SSIM term (3D Gaussian Splatting: 0.2) */
    const float *image;  /* device [C, H, W] */
    const float *target; /* device [C, H, W] */
} gsr_image_loss_inputs;
int64_t gsr_image_loss_workspace(int32_t C, int32_t H, int32_t W);
int gsr_image_loss(const gsr_image_loss_inputs *in, float *values, float *saved, void *workspace,
                   void *stream);
int gsr_image_loss_backward(const gsr_image_loss_inputs *in, const float *saved,
                            const float *dL_dloss, float *dL_dimage, void *stream);

/* ---- The frame's loss on a window of its rows: a strip's share, with halo rows ----
 * (additive to ABI 4; no existing struct, entry point or kernel changes)
 *
 * The loss above, of a frame [C, frame_H, W], computed from a band of its rows: what a rank that
 * rendered a strip, or a fit that walks a large frame band by band, needs to minimise the
 * frame's loss and not the strip's.  The map at a pixel reads the images within 5 rows of it and
 * the gradient at a pixel reads the map's partial derivatives within 5 rows of it, so the own
 * rows and 10 rows of each neighbour are all a window needs.
 *
 * `in` describes the band: in->image and in->target are contiguous [C, in->H, W] buffers whose
 * row 0 is frame row w->row0, and the band lies inside the frame (row0 >= 0, row0 + in->H <=
 * frame_H).  The own rows [own_begin, own_end) are the rows summed and differentiated; the apron
 * is [max(0, own_begin - 5), min(frame_H, own_end + 5)), A rows.  N = C * frame_H * W, the
 * frame's, normalises everything, and n_own = C (own_end - own_begin) W.
 *
 * Padding: frame rows < 0 or >= frame_H are the zero padding, as are columns outside [0, W).
 *   Every other row a call needs must lie inside the band.  A seam is never padded.
 * Rows needed: with `saved`, [max(0, own_begin - 10), min(frame_H, own_end + 10)); without, the
 *   apron; the backward reads of the band only the own rows.  Band rows beyond these are not read.
 * values[3] = (loss, l1, ssim), the window's shares:
 *     l1 = sum_own |image - target| / N,   ssim = sum_own map / N,
 *     loss = (1 - lambda) l1 + lambda (n_own / N - ssim),
 *   each formed in double from the blocks' partial sums in a fixed order and rounded once.  Over
 *   a partition of the frame's rows into own ranges the shares add up to the frame's three
 *   values (up to the roundings of the shares and of their sum).
 * saved: device [3, C, A, W] over the apron rows, or NULL when no gradient is wanted.  The
 *   forward computes the map and its partial derivatives on the apron and sums only the own rows;
 *   without `saved` it computes the own rows alone, so the partial sums, and with them the last
 *   bits of `values`, may differ between the two.
 * dL_dimage: device [C, own_end - own_begin, W], written, not accumulated into.  It is the FRAME
 *   loss's gradient on the own rows: it includes the terms from map pixels in the apron that a
 *   neighbour sums into ITS share.  So it is the gradient of the sum of all windows' shares,
 *   under the same dL_dloss on every window; it is NOT the gradient of this window's share alone.
 * Per-pixel bits: the arithmetic is gsr_image_loss's own code (the same device functions, tap
 *   order and constants, gm and cl from the frame's N).  Every element of `saved` on the apron
 *   and of dL_dimage on the own rows has the bits gsr_image_loss / gsr_image_loss_backward on the
 *   whole frame give that pixel, wherever the window and its tile grid fall.  The window row0 = 0,
 *   own = [0, frame_H) has gsr_image_loss's bits in `values` too.
 * Like the pair above: no context, no allocation, no synchronisation, no atomics; the same bits on
 *   every call with the same inputs, on any stream.  gsr_image_loss_window_workspace gives the
 *   bytes of device scratch gsr_image_loss_window needs (it reads the sizes and the own range
 *   only, not the band's pointers or coverage).
 * Refused with GSR_E_INVALID before any HIP call, nothing written: a NULL in, w, image, target,
 *   values or workspace; the backward's NULL saved or dL_dimage; a size < 1;
 *   C*frame_H*W >= 2^31; own_begin < 0, own_begin >= own_end or own_end > frame_H; a band outside
 *   the frame or one that does not cover the rows the call needs; lambda outside [0, 1] or NaN. */
typedef struct gsr_loss_window {
    int32_t frame_H;   /* rows of the whole frame */
    int32_t row0;      /* the frame row of row 0 of in->image / in->target */
    int32_t own_begin; /* frame rows [own_begin, own_end): summed and differentiated */
    int32_t own_end;
} gsr_loss_window;
int64_t gsr_image_loss_window_workspace(const gsr_image_loss_inputs *in, const gsr_loss_window *w);
int gsr_image_loss_window(const gsr_image_loss_inputs *in, const gsr_loss_window *w, float *values,
                          float *saved, void *workspace, void *stream);
int gsr_image_loss_window_backward(const gsr_image_loss_inputs *in, const gsr_loss_window *w,
                                   const float *saved, const float *dL_dloss, float *dL_dimage,
                                   void *stream);

/* ---- The parameter update of a fit: a fused, visibility-masked ("sparse") Adam step, and the
 * densification statistics ---- (additive to ABI 4)
 *
 * gsr_adam_step updates up to GSR_MAX_PARAM_GROUPS parameter tensors of one scene, [P, M] each
 * with its own M, lr and eps, in ONE kernel launch.  Every element of an updated row runs, in
 * float32, in exactly this order, without FMA contraction and with a correctly rounded divide
 * and square root:
 *
 *   m = beta1 * m + (1.0f - beta1) * g
 *   v = beta2 * v + ((1.0f - beta2) * g) * g
 *   p = p - (lr / bias_correction1) * (m / (sqrtf(v) / bias_correction2_sqrt + eps))
 *
 * (1.0f - beta and lr / bias_correction1 are computed once, in float32.)  With both corrections
 * 1.0f the divisions by them are exact and this is upstream's adamUpdate (SparseGaussianAdam);
 * with 1 - beta1^t and sqrt(1 - beta2^t) it is torch.optim.Adam's step without weight decay,
 * amsgrad or maximize.  NaN and infinities propagate; nothing is clamped; g = 0, v = 0, eps > 0
 * leaves p unchanged.
 *
 * The rows that are updated: with `visible`, those whose byte is nonzero; with `radii` (the
 * rasterizer's output), those with radii[i] > 0; with neither, all.  A row that is not updated is
 * never read or written, in any of its four buffers: it keeps its bits, moments included (they
 * do not decay: the sparse rule), and a NaN in its grad reaches nothing.
 *
 * gsr_densify_stats is upstream's add_densification_stats: for every row with radii[i] > 0, in
 * place, grad_accum[i] += sqrtf(x * x + y * y) (float32, in that order) with x, y =
 * dL_dmeans2D[i][0], [1]; denom[i] += 1.0f; and, with max_radii, max_radii[i] =
 * max(max_radii[i], radii[i]).  No other row is touched.
 *
 * Neither call takes a context, allocates or synchronises: all memory is the caller's (device
 * memory, except the host array `groups`, which is read before the call returns) and all work is
 * enqueued on `stream`.  The update is elementwise, so the results have the same bits on every
 * call with the same inputs.  Buffers of one call that alias each other: undefined.
 *
 * Refused with GSR_E_INVALID before any HIP call, nothing written: gsr_adam_step for a NULL s or
 * groups; P < 0; n_groups outside 1..GSR_MAX_PARAM_GROUPS; an M < 1; a NULL buffer with P > 0; a
 * beta outside [0, 1) or NaN; a correction <= 0 or NaN; an lr or eps NaN; both masks given; sizes
 * beyond 2^31 - 1 blocks (P M of the order of 2^41).  gsr_densify_stats for a NULL in, P < 0, or
 * a NULL radii, dL_dmeans2D, grad_accum or denom with P > 0.  P == 0 is GSR_OK, with no launch. */
#define GSR_MAX_PARAM_GROUPS 8
typedef struct gsr_param_group {
    int32_t M;            /* floats per Gaussian row, >= 1 */
    float lr, eps;
    float *param;         /* [P, M] contiguous float32; 4-byte alignment is enough */
    const float *grad;    /* [P, M] */
    float *exp_avg;       /* [P, M] */
    float *exp_avg_sq;    /* [P, M] */
} gsr_param_group;
typedef struct gsr_adam_settings {
    int64_t P;
    int32_t n_groups;         /* 1..GSR_MAX_PARAM_GROUPS */
    float beta1, beta2;
    float bias_correction1;   /* 1 - beta1^t, or 1.0f for upstream's uncorrected form */
    float bias_correction2_sqrt; /* sqrt(1 - beta2^t), or 1.0f */
    const uint8_t *visible;   /* [P], nonzero = update the row; or NULL */
    const int32_t *radii;     /* [P], > 0 = update the row (the rasterizer's output); or NULL */
} gsr_adam_settings;
int gsr_adam_step(const gsr_adam_settings *s, const gsr_param_group *groups /* host */,
                  void *stream);

typedef struct gsr_densify_inputs {
    int64_t P;
    const int32_t *radii;      /* [P] */
    const float *dL_dmeans2D;  /* [P, 3], upstream's units; x and y are read */
    float *grad_accum;         /* [P]  += sqrtf(x*x + y*y) */
    float *denom;              /* [P]  += 1.0f */
    int32_t *max_radii;        /* [P]  = max(old, radii), or NULL */
} gsr_densify_inputs;
int gsr_densify_stats(const gsr_densify_inputs *in, void *stream);

/* ---- Adaptive density control: clone, split and prune a fitted scene ---- (additive to ABI 4;
 * DESIGN.md §3p)
 *
 * Upstream's densify_and_prune (densify_and_clone, densify_and_split with N = 2, prune_points) on
 * up to GSR_MAX_PARAM_GROUPS parameter tensors [P, M_i] and their Adam moments, as a plan (classify
 * every row, scan, four counts) and an apply (write the P' output rows into the caller's new
 * buffers).  The caller reads the counts between the two: it must size the outputs.
 *
 * Four groups carry a role: xyz (M = 3), scaling (M = 3), rotation (M = 4, (r, x, y, z), not
 * normalised) and opacity (M = 1); all others are only copied.  Every threshold is in the space
 * the tensors are STORED in (scale_space says whether the scaling words are sigma or log sigma;
 * the opacity threshold is compared with the stored opacity word), so a row is classified by
 * comparisons of stored words alone.
 *
 * Per source row i, from row i alone, in float32, with a correctly rounded divide:
 *   avg   = grad_accum[i] / denom[i], NaN -> 0.0f        hot = avg >= grad_threshold
 *   smax  = fmaxf(fmaxf(s0, s1), s2) of the stored scaling words
 *   clone = hot && smax <= scale_split_threshold
 *   split = hot && smax >  scale_split_threshold
 *   pruned(o, s, r) = o < opacity_prune_threshold || s > scale_prune_threshold ||
 *                     r > radius_prune_threshold      (the last only with max_radii and a
 *                                                      threshold > 0; +inf switches the second off)
 * A row that is not split survives iff !pruned(opacity, smax, max_radii[i]); its clone survives
 * with it (same words, same decision).  A split row's source always goes; its GSR_SPLIT_CHILDREN
 * children survive iff !pruned(opacity, child(smax), max_radii[i]) -- the child's scaling, the
 * source's opacity and radius; both children share the decision.
 * Deviation from upstream: upstream zeroes max_radii2D (densification_postfix) before its
 * screen-size test reads it, so that test never fires there.  Here the test reads the caller's
 * values as they are; radius_prune_threshold <= 0 or a NULL max_radii gives upstream's behaviour.
 *
 * Output order, upstream's: the surviving unsplit sources in source order, then the surviving
 * clones in source order, then child 0 of every surviving split source in source order, then
 * child 1 likewise.  counts = (n_kept, n_clone, n_split, n_removed): n_split counts the split
 * sources whose children survive, n_removed the source rows of which nothing is left, so
 * P = n_kept + n_split + n_removed and P' = n_kept + n_clone + 2 n_split <= 2 P.
 *
 * Rows: a kept row copies every parameter and both moments bit for bit.  A clone and a child copy
 * every parameter of the source and get zero moments; two tensors of a child differ:
 *   scaling  s - c in log space with c = (float)log(1.6) = 0x3EF0A451, s / 1.6f in linear
 *            space: one float operation per word
 *   xyz      with q = rotation / sqrtf(((r r + x x) + y y) + z z), R = upstream's build_rotation
 *              R00 = 1 - 2 (y y + z z)  R01 = 2 (x y - r z)      R02 = 2 (x z + r y)
 *              R10 = 2 (x y + r z)      R11 = 1 - 2 (x x + z z)  R12 = 2 (y z - r x)
 *              R20 = 2 (x z - r y)      R21 = 2 (y z + r x)      R22 = 1 - 2 (x x + y y)
 *            sigma = the SOURCE's stored scaling (expf of it in log space), v = sigma * z,
 *            xyz_k = ((Rk0 v0 + Rk1 v1) + Rk2 v2) + xyz_k(source), without FMA contraction
 *   z        from Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl 0x9E3779B9,
 *            0xBB67AE85), key (seed low word, seed high word), counter (i, child, 0, 0), output
 *            words x0..x3:  u_k = ((float)(x_k >> 8) + 0.5f) * 2^-24  (one rounded add: in (0, 1])
 *              z0 = sqrtf(-2.0f * logf(u0)) * cosf(6.2831855f * u1)
 *              z1 = sqrtf(-2.0f * logf(u0)) * sinf(6.2831855f * u1)
 *              z2 = sqrtf(-2.0f * logf(u2)) * cosf(6.2831855f * u3)
 * A sample is a function of (seed, source row, child) alone, never of the launch geometry, the
 * stream or what ran before.  source_index[P'] gets the source row of every output row (for state
 * that is not in these tensors).  Of a row of which nothing survives only the scaling, the opacity
 * and the statistics are read; of a split source, no moment: a NaN elsewhere reaches nothing.
 *
 * Stateless like gsr_adam_step: no context, no allocation, no atomics, no synchronisation; all
 * memory is the caller's, all work is enqueued on `stream`.  The scan is over integers, so every
 * output has the same bits on every call with the same inputs.  `workspace` holds
 * gsr_densify_workspace(P) bytes (4-byte aligned), written by the plan and read by the apply of the
 * same `in`; counts_dev is four int32 on the device.  gsr_densify_apply takes in->P_out = P' (the
 * plan ignores it); its kernels bound every write by P_out and every read by P, whatever the
 * workspace holds.  src_groups and dst_groups are host arrays of in->n_groups entries, [P, M] and
 * [P_out, M]; a group has both moments or neither, the same in both arrays.
 *
 * Refused with GSR_E_INVALID before any HIP call, nothing written: a NULL in, workspace,
 * counts_dev, src_groups or dst_groups; P < 0 or P >= 2^30 (gsr_densify_workspace returns
 * GSR_E_INVALID for those); n_groups outside 1..GSR_MAX_PARAM_GROUPS; an M < 1, or a role with the
 * wrong M, an unknown role, a missing or duplicated role; one moment NULL and the other not, or
 * moments in one of src / dst only (a destination of P_out == 0 rows may be all NULL); a NULL grad_accum, denom, scaling or opacity, or a NULL
 * source buffer, with P > 0; the scaling or opacity role at another address than in->scaling /
 * in->opacity; a NULL destination buffer or source_index with P_out > 0; a NaN threshold; a
 * scale_space that is neither; P_out < 0, P_out > 2 P; sizes beyond 2^31 - 1 blocks.
 * P_out == 0 (so also P == 0) is GSR_OK without a launch of the apply step; the plan of P == 0
 * writes four zeros. */
#define GSR_SPLIT_CHILDREN 2
enum { GSR_ROLE_NONE = 0, GSR_ROLE_XYZ = 1, GSR_ROLE_SCALING = 2, GSR_ROLE_ROTATION = 3,
       GSR_ROLE_OPACITY = 4 };
enum { GSR_SCALE_LINEAR = 0, GSR_SCALE_LOG = 1 };
typedef struct gsr_densify_group {
    int32_t M;            /* floats per row, >= 1 */
    int32_t role;         /* GSR_ROLE_* */
    float *param;         /* [rows, M] contiguous float32; 4-byte alignment is enough */
    float *exp_avg;       /* [rows, M], or NULL with exp_avg_sq for a tensor without moments */
    float *exp_avg_sq;
} gsr_densify_group;
typedef struct gsr_densify_plan_inputs {
    int64_t P;                     /* source rows, 0 <= P < 2^30 */
    int64_t P_out;                 /* P', gsr_densify_apply only */
    uint64_t seed;
    int32_t n_groups;              /* 1..GSR_MAX_PARAM_GROUPS, gsr_densify_apply only */
    int32_t scale_space;           /* GSR_SCALE_LINEAR or GSR_SCALE_LOG */
    float grad_threshold;
    float scale_split_threshold;
    float opacity_prune_threshold;
    float scale_prune_threshold;   /* +inf = off */
    int32_t radius_prune_threshold; /* <= 0 = off */
    const float *grad_accum;       /* [P] */
    const float *denom;            /* [P] */
    const int32_t *max_radii;      /* [P], or NULL = the radius test off */
    const float *scaling;          /* [P, 3], the scaling role's source buffer */
    const float *opacity;          /* [P], the opacity role's source buffer */
} gsr_densify_plan_inputs;
int64_t gsr_densify_workspace(int64_t P);
int gsr_densify_plan(const gsr_densify_plan_inputs *in, void *workspace,
                     int32_t *counts_dev /* [4] device */, void *stream);
int gsr_densify_apply(const gsr_densify_plan_inputs *in,
                      const gsr_densify_group *src_groups /* host */,
                      const gsr_densify_group *dst_groups /* host */, const void *workspace,
                      int32_t *source_index /* [P_out] device */, void *stream);

/* ---- The start of a fit from a point cloud: nearest-neighbour distances ---- (additive to
 * ABI 4)
 *
 * gsr_knn_mean_dist2 is upstream's simple_knn distCUDA2: dist2[i], float32, is the mean squared
 * distance of point i of xyz [N, 3] (contiguous float32; 4-byte alignment is enough) to its three
 * nearest neighbours, from which create_from_pcd derives the initial scales.  In float32, in
 * exactly this order, without FMA contraction and with a correctly rounded divide:
 *   for every j != i:  dx = x_i - x_j, dy = y_i - y_j, dz = z_i - z_j,
 *                      d_ij = ((dx * dx + dy * dy) + dz * dz)
 *   b0 <= b1 <= b2 the three smallest d_ij:  dist2[i] = ((b0 + b1) + b2) / 3.0f
 * Only the index is excluded: duplicate points are neighbours at distance 0, as upstream.
 * Deviation from upstream: with fewer than four points upstream leaves FLT_MAX in the sums; here
 * k = min(3, N - 1) neighbours are averaged, (b0 + b1) / 2.0f or b0 / 1.0f, and N == 1 gives 0.0f.
 * The three smallest values are a multiset that depends on neither the search order nor on how
 * ties are broken, so the result is one bit pattern per point: that of a brute-force search over
 * all pairs (tests/knn_reference.py), on every call, stream and device.  No tolerance applies.
 *
 * The search (csrc/knn.hip): the cloud's bounding box, a 30-bit Morton code per point, the
 * library's radix sort, boxes of 256 consecutive sorted points with their bounds, and one block per
 * box that visits the other boxes outward and skips a box no lane can gain from.  The distance to
 * a box is computed with d_ij's operations in d_ij's order; float32 subtraction, multiplication
 * and addition are monotone under rounding, so it never exceeds the computed d_ij of a point in
 * the box, and the prune is exact.
 *
 * Stateless like gsr_adam_step: no context, no allocation, no synchronisation, no atomics in the
 * knn kernels; all memory is the caller's (device memory) and all work is enqueued on `stream`.
 * `workspace` holds gsr_knn_workspace(N) bytes at any address (about 32 N bytes; the segments
 * start at its first 256-byte-aligned address); it is scratch, with one readable part: after the
 * call the first ceil(N / 256) uint32 words at that aligned address hold, per block of the search,
 * the number of boxes it scanned (tools/bench_knn.py reports their mean).  xyz, dist2 and
 * workspace must not overlap.
 *
 * Coordinates must be finite.  For non-finite input the values of dist2 are unspecified, but
 * every access stays in bounds and every loop ends: cell coordinates are clamped, every loop's
 * trip count is a function of N, and no word outside dist2[0, N) and the workspace is written.
 *
 * gsr_knn_stages is gsr_knn_mean_dist2 cut short, for timing: it runs the first n_stages of
 * (1 bounds + codes, 2 sort, 3 gather + boxes, 4 search); 4 is gsr_knn_mean_dist2 itself, and only
 * then is dist2 written.
 *
 * Refused with GSR_E_INVALID before any HIP call, nothing written: N < 0 or N >= 2^30
 * (gsr_knn_workspace returns GSR_E_INVALID for those); a NULL xyz, dist2 or workspace with N > 0;
 * n_stages outside 1..4.  N == 0 is GSR_OK without a launch. */
int64_t gsr_knn_workspace(int64_t N);
int gsr_knn_mean_dist2(const float *xyz, int64_t N, float *dist2, void *workspace, void *stream);
int gsr_knn_stages(const float *xyz, int64_t N, float *dist2, void *workspace, int32_t n_stages,
                   void *stream);

/* Stage timing (HIP events on the forward's stream, no extra synchronisation).
 * gsr_set_timing(1) starts recording one event set per forward (a ring of the last 256);
 * gsr_stage_times waits for the last timed forward and writes the MEAN per-stage time (ms)
 * over the recorded forwards into ms[i] for i < n; it returns the number of stages.
 * Stage names via gsr_stage_name(i).  Each event costs the stream a few microseconds, so
 * gsr_set_timing(2) records only the two events around the blend (the other stages read 0).
 * gsr_set_timing(0) stops recording. */
int gsr_set_timing(gsr_context *ctx, int enable);
int gsr_stage_times(gsr_context *ctx, float *ms, int n);
const char *gsr_stage_name(int i);

/* Options (per context; every setting renders the same image bits except the blend arithmetic,
 * which changes pixels by float rounding at most -- tests/test_gpu_parity.py checks each):
 *   GSR_OPT_BLEND_CULL (default 1): conservative ellipse-vs-quadrant cull in the blend;
 *     outputs are bit-identical either way.
 *   GSR_OPT_BLEND_FAST (default 1): blend arithmetic with log2(e) folded into the conic, FMA
 *     contraction and the hardware exp2 (tolerance in tests/gpu_helpers.py); 0 keeps upstream's
 *     per-pixel operation order (IEEE, no FMA, ocml expf).
 *   GSR_OPT_DEPTH_SORT (default -1 = auto): the form of the per-frame depth sort.  0 = LSD passes
 *     of 12 key bits, the first dropping the keys of Gaussians without pairs in the strip;
 *     1 = the same after a compaction of the kept keys; 2 = one MSD pass over the top 12 bits
 *     of the kept keys' range (key - smallest kept key), then every bucket sorted by the rest in
 *     LDS; 3 = 2 after the compaction.  auto = the compaction on strips (a proper subset of the
 *     tile rows) of >= 4M Gaussians, the MSD form when the previous frame's kept keys spanned a
 *     range of <= 25 bits (3 or 2), else the LSD passes (1 or 0).  Every form gives the same
 *     permutation.
 *   GSR_OPT_FRAME_GRAPHS (default 0): deferred-K frames.  1: the chains of the frame after the
 *     preprocess (the frame stream's K publish + depth sort and its binning with the
 *     tile ranges and blend order; the second stream's colour) are recorded once per context and key
 *     (input pointers, sizes, strip, workspace) as three linear HIP graphs and replayed; 2: the
 *     same chains launched directly.  Either way the binning is sized by a capacity (the list
 *     lengths seen so far + 25 %) instead of a mid-frame wait for K, the host reads K after
 *     queueing the whole frame, and a frame whose list outgrew the capacity is rendered again
 *     the direct way after the capacity grows.  Used for column-first frames without debug,
 *     per-stage timing (gsr_set_timing 1), the compacting depth sort or the rgb output; the
 *     image and every output are the same as with 0 (DESIGN.md decision 12 has the timings).
 *   GSR_OPT_TIGHT_BINNING (default 1): with the column-first form and no n_contrib output, each
 *     Gaussian of a rect up to 8 tile columns x 15 rows is paired only with the tiles its
 *     alpha >= 1/255 ellipse reaches (upstream's blend skips it on the others), so the lists are
 *     subsequences of upstream's and every pixel composites the same splats in the same order.
 *     Full frames only (a strip's replicated preprocess would write a record per Gaussian for
 *     one strip's lists).  num_rendered stays upstream's count; gsr_get_binning exports the
 *     tight lists (0 binds upstream's lists).
 *   GSR_OPT_SECOND_STREAM (default 1): the frame's K publish (LSD frames) and colour run on
 *     the context's second stream (created on first use), beside the same frame's depth sort and
 *     binning.  0: they run in order on the frame's own stream and the second stream is
 *     destroyed, so the context holds one hardware queue instead of two -- with the process's
 *     GPU_MAX_HW_QUEUES = 4, four frames in flight on four contexts then each have a queue of
 *     their own (FramePipeline with depth >= 3; DESIGN.md decision 13).  With 0, frame graphs
 *     (GSR_OPT_FRAME_GRAPHS) run the second stream's chain in order on the frame's stream (mode
 *     1 records it on a stream made for the recording; ABI 3).  The image is the same either way.
 * The binning form is chosen per frame: column-first (the first tile-sort pass on (Gaussian,
 * tile column) segments, the second on packed (tile row, Gaussian id) words) up to 256 tile
 * columns and strip rows, else the per-pair form; both produce the same lists.  Ids 10 and 12
 * are retired (ABI 1's column-pairs and tight-binning options) and rejected. */
enum { GSR_OPT_BLEND_CULL = 1, GSR_OPT_BLEND_FAST = 2, GSR_OPT_DEPTH_SORT = 11,
       GSR_OPT_TIGHT_BINNING = 13, GSR_OPT_FRAME_GRAPHS = 14, GSR_OPT_SECOND_STREAM = 15 };
int gsr_set_option(gsr_context *ctx, int option, int64_t value);
/* The current value of an option (so a caller that changes one can restore it). */
int gsr_get_option(gsr_context *ctx, int option, int64_t *value);

/* Frame-graph counters of a context: stats[0] forwards rendered by replaying graphs,
 * stats[1] graph pairs recorded, stats[2] forwards re-rendered after the list outgrew the
 * capacity, stats[3] the current list capacity.  Writes min(n, 4); returns 4. */
int gsr_frame_graph_stats(gsr_context *ctx, int64_t *stats, int n);

#ifdef __cplusplus
}
#endif
#endif /* GSR_H */
