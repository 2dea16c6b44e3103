// backward.hip -- the gradients of the splat composite (gsr_backward, include/gsr.h) for gfx950.
//
// The function differentiated is the forward as this project states it: upstream's preprocess
// (preprocess.hip, gsr_internal.h) and upstream's compositing in upstream's operation order
// (blend.hip, kFast == false).  The derivative is derived from that forward, not
// restated from upstream's backward.cu: gates select and are constants; min, max and clamps pass
// nothing on their flat side; the background term final_T bg is part of the colour.
//
//  * k_blend_bwd_q -- the forward's layout: one wave per (16x16 tile, 8x8 quadrant), one pixel per
//    lane, the tile's list in 64-entry chunks through the may_touch cull (a dropped splat has
//    weight exactly 0).  A front-to-back pass gives each lane its final T and its last contributing
//    list position; then the chunks are staged again back to front and every splat's nine sums
//    over the wave's pixels (d/dmean2D x2, d/dconic x3, d/dopacity, d/drgb x3) are reduced across
//    each row of 16 lanes with DPP and kept in the row's lane of the splat's slot.  After 16 slots
//    the wave adds the four rows through LDS and then its <= 16 x 9 sums to the Gaussians' 64-B
//    gradient rows with <= 3 atomic wave-instructions, consecutive lanes on consecutive words of
//    a row (~7 rows of 36 B per instruction) -- never one atomic per lane and splat.
//  * k_preprocess_bwd -- one thread per Gaussian: the 2D gradients through the conic, the EWA
//    covariance, the projection, the SH colour and the 3D covariance to the inputs.
//  * k_blend_bwd_planes_q, k_preprocess_bwd_planes -- the same two bodies with kPlanes set
//    (gsr_backward_planes): depth_map, inv_depth_map and final_T are colour channels
//    of the same composite with the features z, 1 / z, 0 and the backgrounds 0, 0, 1, so their
//    gradients enter the recursion's start value and per-splat term, and a tenth sum per splat
//    (dL/dz through the two features) goes to word 9 of the Gaussian's row and from there to
//    dL_dmeans3D along the view matrix's z row.  Without the flag the bodies compile as before.
//  * k_preprocess_bwd_camera, k_preprocess_bwd_planes_camera, k_camera_finish -- the per-Gaussian
//    body with kCamera set (gsr_backward_camera): the factors of the camera's
//    gradient the body computes on its way to dL_dmeans3D (dhom, dt, dA, J, the SH direction
//    term) are kept, multiplied out to 27 products after the body and summed over the block
//    (rows of 16 lanes by DPP, the 16 rows through LDS), one word per sum and block; the finish
//    adds the blocks in double.  No atomics.  Without the flag the two kernels above compile as
//    before (profiles/backward_camera_resources.txt).
//  * k_preprocess_bwd_aa, ..._planes_aa, ..._camera_aa, ..._planes_camera_aa -- the per-Gaussian
//    body with kAA set (gsr_backward_filtered): the antialiased forward's opacity
//    factor and its gradient through the 2D covariance.  The four kernels above compile as
//    before (profiles/antialias_resources.txt).
//  * k_blend_bwd_det_q, k_blend_bwd_planes_det_q, k_slab_*, k_grad_rows_gather -- the deterministic
//    mode (gsr_backward_ordered): the blend's body with kDet set stores each (splat,
//    quadrant)'s sums to a slot of its own, addressed from the Gaussian's tile rect and the scan of
//    the rects' sizes, and marks it; the gather adds a Gaussian's marked slots in a fixed order, in
//    double, into its row.  No atomics, no zeroing but the marks'.  The kernels above compile as
//    before (profiles/backward_deterministic_resources.txt).
//  * k_blend_bwd_strip_q, ..._planes_strip_q, ..._det_strip_q, ..._planes_det_strip_q, k_strip_gate
//    -- the backward on a strip of tile rows (gsr_backward_strip): the blend's body
//    with kStrip set takes its tile rows from the strip's first and reads the strip-local image
//    gradients; the gate zeroes the rebuilt radius of every Gaussian without a tile in the strip,
//    so the eight per-Gaussian kernels leave it as they leave a culled one.  The kernels above
//    compile as before (profiles/backward_strips_resources.txt).
//  * k_blend_bwd_features_q -- the blend's backward for 16, 8 or 4 feature channels of the caller's
//    own (gsr_backward_features): a body of its own beside blend_bwd, launched per
//    chunk of channels over the same lists; it adds its share of the six geometry sums to the same
//    rows and the channels' sums straight to dL_dfeatures.  The kernels above compile as before
//    (profiles/features_resources.txt).
//  * k_blend_bwd_abs_q, ..._planes_abs_q, ... (eight), k_means2d_abs -- the absolute gradient of the
//    2D mean (gsr_backward_abs): the blend's body with kAbs set keeps two more sums
//    per (splat, quadrant), |v0| and |v1| taken per pixel before any cross-lane sum, through the
//    same row_sum, flush and atomics (or slots) into words 10 and 11 of the Gaussian's row; the
//    elementwise kernel scales them to dL_dmeans2D_abs.  The kernels above compile as before
//    (profiles/backward_absgrad_resources.txt).
#include "gsr_internal.h"

#include <algorithm>
#include <type_traits>

using namespace gsr;

namespace {

// ---- cross-lane sums -----------------------------------------------------------------------
// v from another lane of the row of 16 (DPP; every lane of the wave must be active).
template <int kCtrl>
__device__ __forceinline__ float dpp_f(float v) {
    return __int_as_float(
        __builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, 0xF, 0xF, true));
}
// The sum of v over the lane's row of 16 lanes, in every lane of the row: within quads (quad_perm
// 1,0,3,2 and 2,3,0,1), across the halves of 8 (row_half_mirror) and of 16 (row_mirror).  The
// wave's four rows are added when the sums leave the wave (the flush below).
__device__ __forceinline__ float row_sum(float v) {
    v += dpp_f<0xB1>(v);
    v += dpp_f<0x4E>(v);
    v += dpp_f<0x141>(v);
    v += dpp_f<0x140>(v);
    return v;
}

// One staged splat: g = x, y, conic a, conic b; q = conic c, opacity, r, g; e = b, list position
// + 1 (uint bits: upstream's `contributor`).
template <bool kPlanes>
struct BwdSplatT {
    float4 g, q;
    float2 e;
};
// kPlanes: zf = z, 1 / z (the forward's features, blend.hip k_blend_depth_q), in the 8 B the
// record's 16-B alignment pads anyway
template <>
struct BwdSplatT<true> {
    float4 g, q;
    float2 e, zf;
};

// The body of both blend backward kernels.  kPlanes: p holds the planes' gradients and the depth
// keys; a.dL_dcolor may be NULL.  Without it p is not read.
// kDet (gsr_backward_ordered): the flush stores the sums to the (Gaussian, tile,
// quadrant)'s own slot of d and marks it, instead of adding them to a.grad2d; without it d is not
// read.
// kStrip (gsr_backward_strip): the grid is the strip's tiles; r gives the strip's
// first tile row (the pixels' coordinates stay the frame's) and the offset and height of the
// strip-local image and plane gradients; without it r is not read.
// kAbs (gsr_backward_abs): two more sums per (splat, quadrant), the pixels' |v0| and
// |v1|, for words 10 and 11 of the Gaussian's row (with and without the planes; in a slot they
// follow the kBase words directly).
template <bool kPlanes, bool kDet = false, bool kStrip = false, bool kAbs = false>
__device__ __forceinline__ void blend_bwd(const GsrBlendBwdArgs &a, const GsrPlaneBwdArgs &p,
                                          const GsrDetBwdArgs &d = GsrDetBwdArgs{},
                                          const GsrStripBwdArgs &r = GsrStripBwdArgs{}) {
    using BwdSplat = BwdSplatT<kPlanes>;
    // per (splat, quadrant): the words 0..8 of a gradient row, and word 9 (dL/dz) with the planes
    constexpr int kBase = kPlanes ? 10 : 9;
    // kAbs: the sums kBase and kBase + 1 are sum |v0| and sum |v1|, the row's words kAbsWord, + 1
    constexpr int kSums = kBase + (kAbs ? 2 : 0);
    constexpr int kAbsWord = 10;
    static_assert(kAbsWord >= kBase && kAbsWord + 2 <= kGradRow, "words 10, 11 are free");
    __shared__ BwdSplat s_spl_q[4][64];
    __shared__ uint32_t s_id_q[4][64];
    __shared__ float s_red_q[4][64 * kSums];
    // kDet: the staged splat's slot (pair * 4 + quad), kNoSlot for one that must not be stored
    constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
    __shared__ uint32_t s_slot_q[kDet ? 4 : 1][kDet ? 64 : 1];

    const uint32_t tile = blockIdx.x;
    if (tile >= a.n_tiles) return;
    const uint32_t quad = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    BwdSplat *const s_spl = s_spl_q[quad];
    uint32_t *const s_id = s_id_q[quad];
    float *const s_red = s_red_q[quad];
    [[maybe_unused]] uint32_t *const s_slot = s_slot_q[kDet ? quad : 0];
    // ty: the tile row within the launch's grid (the strip's, which the slots are addressed by)
    const uint32_t tx = tile % a.grid_x, ty = tile / a.grid_x;
    const int qx0 = (int)tx * GSR_TILE_X + (int)(quad & 1u) * 8;
    int qy0 = (int)ty * GSR_TILE_Y + (int)(quad >> 1) * 8;
    if constexpr (kStrip) qy0 = (int)(r.row_begin + ty) * GSR_TILE_Y + (int)(quad >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pfx = (float)px, pfy = (float)py;
    const float X0 = (float)qx0, Y0 = (float)qy0;
    const uint2 range = a.ranges[tile];
    if (__ballot(inside) == 0ull || range.x >= range.y) return;

    // Stages chunk `start` (the forward's gather, cull and in-order compaction); returns the
    // number of staged splats.  with_z (kPlanes, the back-to-front pass): also z by Gaussian id
    // from the depth keys and 1 / z, once per staged splat; kDet: also the splat's slot.
    auto stage = [&](uint32_t start, auto with_z) {
        const uint32_t idx = start + (uint32_t)lane;
        const bool valid = idx < range.y;
        SplatRecord r;
        uint32_t id = 0u;
        if (valid) {
            id = a.point_list[idx] & a.id_mask;
            r = a.records[id];
        }
        bool keep = valid;
        if (valid && a.cull)
            keep = may_touch(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.z, r.b.w, 2.0f * r.c.x, X0,
                             X0 + 7, Y0, Y0 + 7);
        const uint64_t bal = __ballot(keep);
        if (keep) {
            const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
            const int slot = __popcll(bal & lt);
            s_spl[slot].g = r.a;
            s_spl[slot].q = make_float4(r.b.x, r.b.y, r.c.y, r.c.z);
            s_spl[slot].e = make_float2(r.c.w, __uint_as_float(idx - range.x + 1u));
            s_id[slot] = id;
            if constexpr (kPlanes) {
                if constexpr (decltype(with_z)::value) {
                    const float z = __uint_as_float(p.z_bits[id]);
                    s_spl[slot].zf = make_float2(z, 1.0f / z);
                }
            }
            if constexpr (kDet) {
                if constexpr (decltype(with_z)::value) {
                    const uint2 rc = d.strip_rect[id];
                    const uint32_t cx = tx - (rc.x & 0xFFFFu), w = rc.x >> 16;
                    const uint32_t cy = ty - (rc.y & 0xFFFFu), rows = rc.y >> 16;
                    const uint64_t pair = d.slab[id] + (uint64_t)cy * w + cx;
                    const bool ok = cx < w && cy < rows && pair < (uint64_t)d.K;
                    s_slot[slot] = ok ? (uint32_t)pair * 4u + quad : kNoSlot;
                }
            }
        }
        return __popcll(bal);
    };

    // ---- front to back: the forward's decisions (blend.hip, the exact form) -------------------
    float T = inside ? 1.0f : -1.0f;  // done carried in the sign, as the forward
    uint32_t last = 0u;               // list position + 1 of the last splat the pixel composited
    uint32_t chunks = 0u;             // chunks the forward walked
    for (uint32_t start = range.x; start < range.y; start += 64) {
        ++chunks;
        const int count = stage(start, std::false_type{});
        for (int k = 0; k < count; ++k) {
            const BwdSplat sp = s_spl[k];
            const float dx = sp.g.x - pfx, dy = sp.g.y - pfy;
            const float power = -0.5f * (sp.g.z * dx * dx + sp.q.x * dy * dy) - sp.g.w * dx * dy;
            const float alpha = fminf(0.99f, sp.q.y * exp_core(power));
            const bool vis = !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
            const float test_T = T * (1 - alpha);
            const bool acc = vis && !(test_T < 0.0001f);
            const bool term = vis && (test_T < 0.0001f);
            T = acc ? test_T : (term ? -fabsf(T) : T);
            last = acc ? __float_as_uint(sp.e.y) : last;
        }
        if (__ballot(!(T <= 0.0f)) == 0ull) break;
    }

    // ---- back to front -------------------------------------------------------------------------
    // With R_i the colour behind splat i at unit transmittance (R_n = bg, R_{i-1} = c_i alpha_i +
    // (1 - alpha_i) R_i) the pixel is R_0 and dC/dalpha_i = T_i (c_i - R_i); only r = g . R is
    // carried (g = dL/dC of the pixel).  T_i is rebuilt as T_{i+1} / (1 - alpha_i), alpha <= 0.99.
    size_t plane = (size_t)a.H * a.W, pid = (size_t)(inside ? py : 0) * a.W + (inside ? px : 0);
    if constexpr (kStrip) {  // strip-local gradients (an inside pixel of a strip tile: py >= y0)
        plane = (size_t)r.rows_out * a.W;
        pid = (size_t)(inside ? py - r.y0 : 0) * a.W + (inside ? px : 0);
    }
    // (kPlanes: a NULL dL_dcolor, a NULL plane and a pixel outside the image all read 0)
    const bool has_g = inside && (!kPlanes || a.dL_dcolor);
    const float g0 = has_g ? a.dL_dcolor[pid] : 0.0f;
    const float g1 = has_g ? a.dL_dcolor[plane + pid] : 0.0f;
    const float g2 = has_g ? a.dL_dcolor[2 * plane + pid] : 0.0f;
    // dL/ddepth_map, dL/dinv_depth_map, dL/dfinal_T
    [[maybe_unused]] float gd = 0.0f, gi = 0.0f, gT = 0.0f;
    if constexpr (kPlanes) {
        gd = inside && p.dL_ddepth_map ? p.dL_ddepth_map[pid] : 0.0f;
        gi = inside && p.dL_dinv_depth_map ? p.dL_dinv_depth_map[pid] : 0.0f;
        gT = inside && p.dL_dfinal_T ? p.dL_dfinal_T[pid] : 0.0f;
    }
    float Tc = fabsf(T);
    // the planes' backgrounds are 0, 0, 1: final_T is the channel with feature 0
    float rr = g0 * a.bg[0] + g1 * a.bg[1] + g2 * a.bg[2];
    if constexpr (kPlanes) rr += gT;
    for (uint32_t c = chunks; c-- > 0u;) {
        const int count = stage(range.x + 64u * c, std::bool_constant<kPlanes || kDet>{});
        // groups of 16 slots, back to front: lane 16 r + j keeps row r's share of the nine sums
        // of the splat in slot 16 kg + j
        for (int kg = (count - 1) >> 4; kg >= 0; --kg) {
            const int k_lo = 16 * kg, k_hi = min(count, k_lo + 16);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f,
                  s8 = 0.f;
            [[maybe_unused]] float s9 = 0.f, sa0 = 0.f, sa1 = 0.f;
            uint32_t touched = 0u;  // slots of the group with a contributing pixel
            for (int k = k_hi; k-- > k_lo;) {
                const BwdSplat sp = s_spl[k];
                const float dx = sp.g.x - pfx, dy = sp.g.y - pfy;
                const float power =
                    -0.5f * (sp.g.z * dx * dx + sp.q.x * dy * dy) - sp.g.w * dx * dy;
                const float G = exp_core(power);
                const float oG = sp.q.y * G;
                const float alpha = fminf(0.99f, oG);
                const bool con = inside && __float_as_uint(sp.e.y) <= last && !(power > 0.0f) &&
                                 !(alpha < 1.0f / 255.0f);
                if (__ballot(con) == 0ull) continue;
                touched |= 1u << (k & 15);
                const float Ti = Tc / (1.0f - alpha);
                const float w = alpha * Ti;
                float gc = g0 * sp.q.z + g1 * sp.q.w + g2 * sp.e.x;
                if constexpr (kPlanes) gc += gd * sp.zf.x + gi * sp.zf.y;
                const float dLa = Ti * (gc - rr);
                // alpha = min(0.99, o G): nothing passes where it caps
                const bool open = con && !(oG > 0.99f);
                const float dLp = open ? dLa * oG : 0.0f;  // d/dpower (dG/dpower = G)
                const float v0 = dLp * (-sp.g.z * dx - sp.g.w * dy);
                const float v1 = dLp * (-sp.q.x * dy - sp.g.w * dx);
                const float v2 = dLp * (-0.5f * dx * dx);
                const float v3 = dLp * (-dx * dy);
                const float v4 = dLp * (-0.5f * dy * dy);
                const float v5 = open ? dLa * G : 0.0f;
                const float v6 = con ? g0 * w : 0.0f;
                const float v7 = con ? g1 * w : 0.0f;
                const float v8 = con ? g2 * w : 0.0f;
                rr = con ? alpha * gc + (1.0f - alpha) * rr : rr;
                Tc = con ? Ti : Tc;
                const bool mine = (lane & 15) == (k & 15);
                const float t0 = row_sum(v0), t1 = row_sum(v1), t2 = row_sum(v2);
                s0 = mine ? t0 : s0, s1 = mine ? t1 : s1, s2 = mine ? t2 : s2;
                const float t3 = row_sum(v3), t4 = row_sum(v4), t5 = row_sum(v5);
                s3 = mine ? t3 : s3, s4 = mine ? t4 : s4, s5 = mine ? t5 : s5;
                const float t6 = row_sum(v6), t7 = row_sum(v7), t8 = row_sum(v8);
                s6 = mine ? t6 : s6, s7 = mine ? t7 : s7, s8 = mine ? t8 : s8;
                if constexpr (kPlanes) {
                    // the direct path through the features: d(z w)/dz = w, d((1/z) w)/dz =
                    // -(1/z)^2 w with the forward's rounded quotient
                    const float v9 = con ? w * (gd - gi * (sp.zf.y * sp.zf.y)) : 0.0f;
                    const float t9 = row_sum(v9);
                    s9 = mine ? t9 : s9;
                }
                if constexpr (kAbs) {
                    // per pixel, before any cross-lane sum: what cancels in s0, s1 adds up here
                    const float ta0 = row_sum(fabsf(v0)), ta1 = row_sum(fabsf(v1));
                    sa0 = mine ? ta0 : sa0, sa1 = mine ? ta1 : sa1;
                }
            }
            if (touched == 0u) continue;
            // slot-major in LDS, the four rows of a slot side by side; then word t of the group's
            // slots x 9 goes to word t % 9 of the row of slot t / 9: consecutive lanes add to
            // consecutive words (kPlanes: slots x 10 <= 160 words, still <= 3 instructions)
            float *mine9 = s_red + ((lane & 15) * 4 + (lane >> 4)) * kSums;
            mine9[0] = s0, mine9[1] = s1, mine9[2] = s2, mine9[3] = s3, mine9[4] = s4;
            mine9[5] = s5, mine9[6] = s6, mine9[7] = s7, mine9[8] = s8;
            if constexpr (kPlanes) mine9[9] = s9;
            if constexpr (kAbs) mine9[kBase] = sa0, mine9[kBase + 1] = sa1;
            const int n = (k_hi - k_lo) * kSums;
            for (int t = lane; t < n; t += 64) {
                const int slot = t / kSums, word = t - slot * kSums;
                if ((touched >> slot) & 1u) {
                    const float *q4 = s_red + slot * 4 * kSums + word;
                    const float sum = (q4[0] + q4[kSums]) + (q4[2 * kSums] + q4[3 * kSums]);
                    if constexpr (kDet) {
                        // a plain store: the slot is this wave's alone, and written once
                        const uint32_t to = s_slot[k_lo + slot];
                        if (to != kNoSlot) {
                            d.sums[(size_t)to * kSums + word] = sum;
                            if (word == 0) d.marks[to] = 1;
                        }
                    } else {
                        // (kAbs: the last two sums go to the words 10, 11 whatever kBase is)
                        const int to = kAbs && word >= kBase ? word - kBase + kAbsWord : word;
                        atomicAdd(&a.grad2d[(size_t)s_id[k_lo + slot] * kGradRow + to], sum);
                    }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_blend_bwd_q(const GsrBlendBwdArgs a) {
    blend_bwd<false>(a, GsrPlaneBwdArgs{});
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_q(const GsrBlendBwdArgs a,
                                                            const GsrPlaneBwdArgs p) {
    blend_bwd<true>(a, p);
}
__global__ __launch_bounds__(256) void k_blend_bwd_det_q(const GsrBlendBwdArgs a,
                                                         const GsrDetBwdArgs d) {
    blend_bwd<false, true>(a, GsrPlaneBwdArgs{}, d);
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_det_q(const GsrBlendBwdArgs a,
                                                                const GsrPlaneBwdArgs p,
                                                                const GsrDetBwdArgs d) {
    blend_bwd<true, true>(a, p, d);
}
// The same four on a strip of tile rows (gsr_backward_strip): instantiations of their own, so the
// four above keep their code and registers (profiles/backward_strips_resources.txt).
__global__ __launch_bounds__(256) void k_blend_bwd_strip_q(const GsrBlendBwdArgs a,
                                                           const GsrStripBwdArgs r) {
    blend_bwd<false, false, true>(a, GsrPlaneBwdArgs{}, GsrDetBwdArgs{}, r);
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_strip_q(const GsrBlendBwdArgs a,
                                                                  const GsrPlaneBwdArgs p,
                                                                  const GsrStripBwdArgs r) {
    blend_bwd<true, false, true>(a, p, GsrDetBwdArgs{}, r);
}
__global__ __launch_bounds__(256) void k_blend_bwd_det_strip_q(const GsrBlendBwdArgs a,
                                                               const GsrDetBwdArgs d,
                                                               const GsrStripBwdArgs r) {
    blend_bwd<false, true, true>(a, GsrPlaneBwdArgs{}, d, r);
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_det_strip_q(const GsrBlendBwdArgs a,
                                                                      const GsrPlaneBwdArgs p,
                                                                      const GsrDetBwdArgs d,
                                                                      const GsrStripBwdArgs r) {
    blend_bwd<true, true, true>(a, p, d, r);
}
// The same eight with kAbs set (gsr_backward_abs): instantiations of their own again, so the eight
// above keep their code, registers and LDS (profiles/backward_absgrad_resources.txt).
__global__ __launch_bounds__(256) void k_blend_bwd_abs_q(const GsrBlendBwdArgs a) {
    blend_bwd<false, false, false, true>(a, GsrPlaneBwdArgs{});
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_abs_q(const GsrBlendBwdArgs a,
                                                                const GsrPlaneBwdArgs p) {
    blend_bwd<true, false, false, true>(a, p);
}
__global__ __launch_bounds__(256) void k_blend_bwd_det_abs_q(const GsrBlendBwdArgs a,
                                                             const GsrDetBwdArgs d) {
    blend_bwd<false, true, false, true>(a, GsrPlaneBwdArgs{}, d);
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_det_abs_q(const GsrBlendBwdArgs a,
                                                                    const GsrPlaneBwdArgs p,
                                                                    const GsrDetBwdArgs d) {
    blend_bwd<true, true, false, true>(a, p, d);
}
__global__ __launch_bounds__(256) void k_blend_bwd_strip_abs_q(const GsrBlendBwdArgs a,
                                                               const GsrStripBwdArgs r) {
    blend_bwd<false, false, true, true>(a, GsrPlaneBwdArgs{}, GsrDetBwdArgs{}, r);
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_strip_abs_q(const GsrBlendBwdArgs a,
                                                                      const GsrPlaneBwdArgs p,
                                                                      const GsrStripBwdArgs r) {
    blend_bwd<true, false, true, true>(a, p, GsrDetBwdArgs{}, r);
}
__global__ __launch_bounds__(256) void k_blend_bwd_det_strip_abs_q(const GsrBlendBwdArgs a,
                                                                   const GsrDetBwdArgs d,
                                                                   const GsrStripBwdArgs r) {
    blend_bwd<false, true, true, true>(a, GsrPlaneBwdArgs{}, d, r);
}
__global__ __launch_bounds__(256) void k_blend_bwd_planes_det_strip_abs_q(
    const GsrBlendBwdArgs a, const GsrPlaneBwdArgs p, const GsrDetBwdArgs d,
    const GsrStripBwdArgs r) {
    blend_bwd<true, true, true, true>(a, p, d, r);
}

// ---- the feature channels' blend backward (gsr_backward_features) ----------------
// What one launch differentiates: channels [c0, c0 + kC) of the Gaussians' feature rows.
struct FeatBwdArgs {
    const float *features;         // [P, C]
    const float *dL_dfeature_map;  // [C, rows, W]
    float *dL_dfeatures;           // [P, C], zeroed by the caller, or NULL
    int C, c0;
    int vec4;  // 16-B aligned feature rows
};

// blend_bwd's two passes for kC channels of the caller's own in place of the colours: the pixel
// keeps kC gradients gF, the per-splat term is gF . f_i (f_i the splat's feature words, staged into
// LDS by the lane that stages the splat and read by broadcast), the carried value starts at 0 (no
// background), and a splat has 6 + kC sums per quadrant: words 0..5 (d/dmean2D, d/dconic,
// d/dopacity) are added to the Gaussian's row of a.grad2d beside the colour pass's, the kC sums
// gF_c w straight to dL_dfeatures[id * C + c0 + c].  Channels at or beyond C read as zero and are
// neither read from memory nor written.
template <int kC, bool kStrip>
__device__ __forceinline__ void blend_bwd_features(const GsrBlendBwdArgs &a, const FeatBwdArgs &ft,
                                                   const GsrStripBwdArgs &r) {
    static_assert(kC % 4 == 0, "feature chunks are whole float4s");
    using BwdSplat = BwdSplatT<false>;
    constexpr int kSums = 6 + kC;
    __shared__ BwdSplat s_spl_q[4][64];
    __shared__ uint32_t s_id_q[4][64];
    __shared__ float s_red_q[4][64 * kSums];
    __shared__ alignas(16) float s_ft_q[4][64 * kC];

    const uint32_t tile = blockIdx.x;
    if (tile >= a.n_tiles) return;
    const uint32_t quad = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    BwdSplat *const s_spl = s_spl_q[quad];
    uint32_t *const s_id = s_id_q[quad];
    float *const s_red = s_red_q[quad];
    float *const s_ft = s_ft_q[quad];
    const uint32_t tx = tile % a.grid_x, ty = tile / a.grid_x;
    const int qx0 = (int)tx * GSR_TILE_X + (int)(quad & 1u) * 8;
    int qy0 = (int)ty * GSR_TILE_Y + (int)(quad >> 1) * 8;
    if constexpr (kStrip) qy0 = (int)(r.row_begin + ty) * GSR_TILE_Y + (int)(quad >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pfx = (float)px, pfy = (float)py;
    const float X0 = (float)qx0, Y0 = (float)qy0;
    const uint2 range = a.ranges[tile];
    if (__ballot(inside) == 0ull || range.x >= range.y) return;
    const int n_ch = ft.C - ft.c0;  // channels of this launch that exist (the rest: zeros)

    // blend_bwd's stage; with_f (the back-to-front pass): also the splat's feature words
    auto stage = [&](uint32_t start, auto with_f) {
        const uint32_t idx = start + (uint32_t)lane;
        const bool valid = idx < range.y;
        SplatRecord rec;
        uint32_t id = 0u;
        if (valid) {
            id = a.point_list[idx] & a.id_mask;
            rec = a.records[id];
        }
        bool keep = valid;
        if (valid && a.cull)
            keep = may_touch(rec.a.x, rec.a.y, rec.a.z, rec.a.w, rec.b.x, rec.b.z, rec.b.w,
                             2.0f * rec.c.x, X0, X0 + 7, Y0, Y0 + 7);
        const uint64_t bal = __ballot(keep);
        if (keep) {
            const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
            const int slot = __popcll(bal & lt);
            s_spl[slot].g = rec.a;
            s_spl[slot].q = make_float4(rec.b.x, rec.b.y, rec.c.y, rec.c.z);
            s_spl[slot].e = make_float2(rec.c.w, __uint_as_float(idx - range.x + 1u));
            s_id[slot] = id;
            if constexpr (decltype(with_f)::value) {
                const float *src = ft.features + (size_t)id * ft.C + ft.c0;
                float *dst = s_ft + slot * kC;
                if (ft.vec4) {
#pragma unroll
                    for (int c = 0; c < kC; c += 4)
                        *reinterpret_cast<float4 *>(dst + c) =
                            c < n_ch ? *reinterpret_cast<const float4 *>(src + c)
                                     : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                } else {
#pragma unroll
                    for (int c = 0; c < kC; ++c) dst[c] = c < n_ch ? src[c] : 0.0f;
                }
            }
        }
        return __popcll(bal);
    };

    // ---- front to back: the forward's decisions, as blend_bwd ---------------------------------
    float T = inside ? 1.0f : -1.0f;
    uint32_t last = 0u, chunks = 0u;
    for (uint32_t start = range.x; start < range.y; start += 64) {
        ++chunks;
        const int count = stage(start, std::false_type{});
        for (int k = 0; k < count; ++k) {
            const BwdSplat sp = s_spl[k];
            const float dx = sp.g.x - pfx, dy = sp.g.y - pfy;
            const float power = -0.5f * (sp.g.z * dx * dx + sp.q.x * dy * dy) - sp.g.w * dx * dy;
            const float alpha = fminf(0.99f, sp.q.y * exp_core(power));
            const bool vis = !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
            const float test_T = T * (1 - alpha);
            const bool acc = vis && !(test_T < 0.0001f);
            const bool term = vis && (test_T < 0.0001f);
            T = acc ? test_T : (term ? -fabsf(T) : T);
            last = acc ? __float_as_uint(sp.e.y) : last;
        }
        if (__ballot(!(T <= 0.0f)) == 0ull) break;
    }

    // ---- back to front -------------------------------------------------------------------------
    size_t plane = (size_t)a.H * a.W, pid = (size_t)(inside ? py : 0) * a.W + (inside ? px : 0);
    if constexpr (kStrip) {
        plane = (size_t)r.rows_out * a.W;
        pid = (size_t)(inside ? py - r.y0 : 0) * a.W + (inside ? px : 0);
    }
    float gF[kC];
#pragma unroll
    for (int c = 0; c < kC; ++c)
        gF[c] = inside && c < n_ch ? ft.dL_dfeature_map[(size_t)(ft.c0 + c) * plane + pid] : 0.0f;
    float Tc = fabsf(T);
    float rr = 0.0f;  // the features' background is 0
    for (uint32_t ch = chunks; ch-- > 0u;) {
        const int count = stage(range.x + 64u * ch, std::true_type{});
        for (int kg = (count - 1) >> 4; kg >= 0; --kg) {
            const int k_lo = 16 * kg, k_hi = min(count, k_lo + 16);
            float s[kSums];
#pragma unroll
            for (int w = 0; w < kSums; ++w) s[w] = 0.f;
            uint32_t touched = 0u;
            for (int k = k_hi; k-- > k_lo;) {
                const BwdSplat sp = s_spl[k];
                const float dx = sp.g.x - pfx, dy = sp.g.y - pfy;
                const float power =
                    -0.5f * (sp.g.z * dx * dx + sp.q.x * dy * dy) - sp.g.w * dx * dy;
                const float G = exp_core(power);
                const float oG = sp.q.y * G;
                const float alpha = fminf(0.99f, oG);
                const bool con = inside && __float_as_uint(sp.e.y) <= last && !(power > 0.0f) &&
                                 !(alpha < 1.0f / 255.0f);
                if (__ballot(con) == 0ull) continue;
                touched |= 1u << (k & 15);
                const float Ti = Tc / (1.0f - alpha);
                const float w = alpha * Ti;
                float gc = 0.0f;
                float v[kSums];
#pragma unroll
                for (int c = 0; c < kC; c += 4) {
                    const float4 f = *reinterpret_cast<const float4 *>(s_ft + k * kC + c);
                    gc += gF[c] * f.x;
                    gc += gF[c + 1] * f.y;
                    gc += gF[c + 2] * f.z;
                    gc += gF[c + 3] * f.w;
                }
                const float dLa = Ti * (gc - rr);
                const bool open = con && !(oG > 0.99f);
                const float dLp = open ? dLa * oG : 0.0f;
                v[0] = dLp * (-sp.g.z * dx - sp.g.w * dy);
                v[1] = dLp * (-sp.q.x * dy - sp.g.w * dx);
                v[2] = dLp * (-0.5f * dx * dx);
                v[3] = dLp * (-dx * dy);
                v[4] = dLp * (-0.5f * dy * dy);
                v[5] = open ? dLa * G : 0.0f;
#pragma unroll
                for (int c = 0; c < kC; ++c) v[6 + c] = con ? gF[c] * w : 0.0f;
                rr = con ? alpha * gc + (1.0f - alpha) * rr : rr;
                Tc = con ? Ti : Tc;
                const bool mine = (lane & 15) == (k & 15);
#pragma unroll
                for (int i = 0; i < kSums; ++i) {
                    const float t = row_sum(v[i]);
                    s[i] = mine ? t : s[i];
                }
            }
            if (touched == 0u) continue;
            // slot-major in LDS, the four rows of a slot side by side, as blend_bwd; word t of
            // the group's slots x kSums: the first six to the 2D gradient row, the rest to the
            // Gaussian's feature gradient row -- consecutive lanes on consecutive words of both
            float *mine_s = s_red + ((lane & 15) * 4 + (lane >> 4)) * kSums;
#pragma unroll
            for (int i = 0; i < kSums; ++i) mine_s[i] = s[i];
            const int n = (k_hi - k_lo) * kSums;
            for (int t = lane; t < n; t += 64) {
                const int slot = t / kSums, word = t - slot * kSums;
                if (!((touched >> slot) & 1u)) continue;
                const float *q4 = s_red + slot * 4 * kSums + word;
                const float sum = (q4[0] + q4[kSums]) + (q4[2 * kSums] + q4[3 * kSums]);
                const size_t id = s_id[k_lo + slot];
                if (word < 6)
                    atomicAdd(&a.grad2d[id * kGradRow + word], sum);
                else if (ft.dL_dfeatures && word - 6 < n_ch)
                    atomicAdd(&ft.dL_dfeatures[id * ft.C + ft.c0 + (word - 6)], sum);
            }
        }
    }
}

template <int kC, bool kStrip>
__global__ __launch_bounds__(256) void k_blend_bwd_features_q(const GsrBlendBwdArgs a,
                                                              const FeatBwdArgs ft,
                                                              const GsrStripBwdArgs r) {
    blend_bwd_features<kC, kStrip>(a, ft, r);
}

// gsr_launch_strip_gate: a Gaussian without a tile in the strip reads as culled from here on.
__global__ __launch_bounds__(256) void k_strip_gate(const uint2 *__restrict__ strip_rect,
                                                    int64_t P, int32_t *radii) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < P && strip_rect[i].x == 0u) radii[i] = 0;
}

// gsr_launch_means2d_abs: dL_dmeans2D_abs from the rows' words 10 and 11, in dL_dmeans2D's units
// (k_preprocess_bwd's factors); exact zeros for a culled (or, after the gate, strip-less) Gaussian.
__global__ __launch_bounds__(256) void k_means2d_abs(const int32_t *__restrict__ radii,
                                                     const float *__restrict__ grad2d, int64_t P,
                                                     int W, int H, float *out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= P) return;
    float ax = 0.f, ay = 0.f;
    if (radii[i] > 0) {
        ax = grad2d[i * kGradRow + 10] * (0.5f * (float)W);
        ay = grad2d[i * kGradRow + 11] * (0.5f * (float)H);
    }
    out[3 * i] = ax, out[3 * i + 1] = ay, out[3 * i + 2] = 0.f;
}

// ---- the deterministic mode's slab scan and gather ------------------------------
constexpr int kSlabPer = 4;                    // Gaussians per thread
constexpr int kSlabBlock = 256 * kSlabPer;     // ... per block
__device__ __forceinline__ uint32_t rect_tiles(uint2 rc) { return (rc.x >> 16) * (rc.y >> 16); }

// The inclusive scan of v over the block's 256 threads (s_scan: 256 words), then a barrier.
__device__ __forceinline__ uint64_t block_scan_incl(uint64_t v, uint64_t *s_scan) {
    s_scan[threadIdx.x] = v;
    __syncthreads();
    for (uint32_t n = 1; n < 256; n <<= 1) {
        const uint64_t add = threadIdx.x >= n ? s_scan[threadIdx.x - n] : 0ull;
        __syncthreads();
        s_scan[threadIdx.x] += add;
        __syncthreads();
    }
    return s_scan[threadIdx.x];
}

// partials[b] = the rect tiles of block b's kSlabBlock Gaussians
__global__ __launch_bounds__(256) void k_slab_reduce(const uint2 *__restrict__ strip_rect,
                                                     int64_t P, uint64_t *partials) {
    __shared__ uint64_t s_scan[256];
    const int64_t i0 = (int64_t)blockIdx.x * kSlabBlock + (int64_t)threadIdx.x * kSlabPer;
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < kSlabPer; ++j)
        if (i0 + j < P) v += rect_tiles(strip_rect[i0 + j]);
    const uint64_t incl = block_scan_incl(v, s_scan);
    if (threadIdx.x == 255) partials[blockIdx.x] = incl;
}
// partials -> their exclusive scan, in place: one block, 256 entries at a time
__global__ __launch_bounds__(256) void k_slab_scan_partials(uint64_t *partials, uint32_t blocks) {
    __shared__ uint64_t s_scan[256];
    uint64_t base = 0;
    for (uint32_t b0 = 0; b0 < blocks; b0 += 256) {
        const uint32_t b = b0 + threadIdx.x;
        const uint64_t v = b < blocks ? partials[b] : 0ull;
        const uint64_t incl = block_scan_incl(v, s_scan);
        if (b < blocks) partials[b] = base + incl - v;
        base += s_scan[255];
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void k_slab_apply(const uint2 *__restrict__ strip_rect,
                                                    int64_t P, const uint64_t *partials,
                                                    uint64_t *slab) {
    __shared__ uint64_t s_scan[256];
    const int64_t i0 = (int64_t)blockIdx.x * kSlabBlock + (int64_t)threadIdx.x * kSlabPer;
    uint32_t n[kSlabPer];
    uint64_t v = 0;
#pragma unroll
    for (int j = 0; j < kSlabPer; ++j) {
        n[j] = i0 + j < P ? rect_tiles(strip_rect[i0 + j]) : 0u;
        v += n[j];
    }
    uint64_t at = partials[blockIdx.x] + block_scan_incl(v, s_scan) - v;
#pragma unroll
    for (int j = 0; j < kSlabPer; ++j) {
        if (i0 + j < P) slab[i0 + j] = at;
        at += n[j];
    }
}

// v of lane (lane ^ kMask), for the gather's tree (every lane of the wave active)
template <int kMask>
__device__ __forceinline__ double xor_d(double v) {
    const int lo = __shfl_xor(__double2loint(v), kMask, 64);
    const int hi = __shfl_xor(__double2hiint(v), kMask, 64);
    return __hiloint2double(hi, lo);
}

// One row of 16 lanes per Gaussian (gsr_internal.h, gsr_launch_grad_rows_gather).  kAbs: the
// slot's last two sums are the absolute ones, for the row's words 10 and 11.
template <int kSums, bool kAbs>
__device__ __forceinline__ void grad_rows_gather(const GsrDetBwdArgs &d, int64_t P,
                                                 float *grad2d) {
    const int64_t id = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    const uint32_t j = threadIdx.x & 15u;
    uint64_t first = 0, slots = 0;
    if (id < P) {
        slots = 4ull * rect_tiles(d.strip_rect[id]);
        first = 4ull * d.slab[id];
        // (the rebuild's rects end at K; anything else is not read)
        if (first + slots > 4ull * d.K) slots = 0;
    }
    double acc[kSums];
#pragma unroll
    for (int w = 0; w < kSums; ++w) acc[w] = 0.0;
    for (uint64_t t = j; t < slots; t += 16) {
        const uint64_t slot = first + t;
        if (d.marks[slot] == 0) continue;
        const float *src = d.sums + slot * kSums;
#pragma unroll
        for (int w = 0; w < kSums; ++w) acc[w] += (double)src[w];
    }
    float out = 0.0f;
#pragma unroll
    for (int w = 0; w < kSums; ++w) {
        double v = acc[w];
        v += xor_d<1>(v);
        v += xor_d<2>(v);
        v += xor_d<4>(v);
        v += xor_d<8>(v);
        const int to = kAbs && w >= kSums - 2 ? w - (kSums - 2) + 10 : w;
        out = j == (uint32_t)to ? (float)v : out;
    }
    if (id < P) grad2d[id * kGradRow + j] = out;
}
template <int kSums>
__global__ __launch_bounds__(256) void k_grad_rows_gather(const GsrDetBwdArgs d, int64_t P,
                                                          float *grad2d) {
    grad_rows_gather<kSums, false>(d, P, grad2d);
}
// kSums: 11, or 12 with the planes (gsr_backward_abs)
template <int kSums>
__global__ __launch_bounds__(256) void k_grad_rows_gather_abs(const GsrDetBwdArgs d, int64_t P,
                                                              float *grad2d) {
    grad_rows_gather<kSums, true>(d, P, grad2d);
}

// ---- per Gaussian ------------------------------------------------------------------------------
constexpr float kC0 = 0.28209479177387814f, kC1 = 0.4886025119029199f;
constexpr float kC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                          -1.0925484305920792f, 0.5462742152960396f};
constexpr float kC3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                          0.3731763325901154f, -0.4570457994644658f, 1.445305721320277f,
                          -0.5900435899266435f};

// The 16 SH basis values at the unit direction (x, y, z), signed as eval_sh (preprocess.hip) adds
// them, and their partial derivatives.
__device__ __forceinline__ void sh_basis(float x, float y, float z, float (&b)[16],
                                         float (&bx)[16], float (&by)[16], float (&bz)[16]) {
    const float xx = x * x, yy = y * y, zz = z * z;
    b[0] = kC0, bx[0] = by[0] = bz[0] = 0.f;
    b[1] = -kC1 * y, bx[1] = 0.f, by[1] = -kC1, bz[1] = 0.f;
    b[2] = kC1 * z, bx[2] = 0.f, by[2] = 0.f, bz[2] = kC1;
    b[3] = -kC1 * x, bx[3] = -kC1, by[3] = 0.f, bz[3] = 0.f;
    b[4] = kC2[0] * x * y, bx[4] = kC2[0] * y, by[4] = kC2[0] * x, bz[4] = 0.f;
    b[5] = kC2[1] * y * z, bx[5] = 0.f, by[5] = kC2[1] * z, bz[5] = kC2[1] * y;
    b[6] = kC2[2] * (2.0f * zz - xx - yy), bx[6] = kC2[2] * -2.0f * x, by[6] = kC2[2] * -2.0f * y,
    bz[6] = kC2[2] * 4.0f * z;
    b[7] = kC2[3] * x * z, bx[7] = kC2[3] * z, by[7] = 0.f, bz[7] = kC2[3] * x;
    b[8] = kC2[4] * (xx - yy), bx[8] = kC2[4] * 2.0f * x, by[8] = kC2[4] * -2.0f * y, bz[8] = 0.f;
    b[9] = kC3[0] * y * (3.0f * xx - yy), bx[9] = kC3[0] * 6.0f * x * y,
    by[9] = kC3[0] * (3.0f * xx - 3.0f * yy), bz[9] = 0.f;
    b[10] = kC3[1] * x * y * z, bx[10] = kC3[1] * y * z, by[10] = kC3[1] * x * z,
    bz[10] = kC3[1] * x * y;
    b[11] = kC3[2] * y * (4.0f * zz - xx - yy), bx[11] = kC3[2] * -2.0f * x * y,
    by[11] = kC3[2] * (4.0f * zz - xx - 3.0f * yy), bz[11] = kC3[2] * 8.0f * y * z;
    b[12] = kC3[3] * z * (2.0f * zz - 3.0f * xx - 3.0f * yy), bx[12] = kC3[3] * -6.0f * x * z,
    by[12] = kC3[3] * -6.0f * y * z, bz[12] = kC3[3] * (6.0f * zz - 3.0f * xx - 3.0f * yy);
    b[13] = kC3[4] * x * (4.0f * zz - xx - yy), bx[13] = kC3[4] * (4.0f * zz - 3.0f * xx - yy),
    by[13] = kC3[4] * -2.0f * x * y, bz[13] = kC3[4] * 8.0f * x * z;
    b[14] = kC3[5] * z * (xx - yy), bx[14] = kC3[5] * 2.0f * x * z, by[14] = kC3[5] * -2.0f * y * z,
    bz[14] = kC3[5] * (xx - yy);
    b[15] = kC3[6] * x * (xx - 3.0f * yy), bx[15] = kC3[6] * (3.0f * xx - 3.0f * yy),
    by[15] = kC3[6] * -6.0f * x * y, bz[15] = 0.f;
}

__device__ __forceinline__ void store3(float *p, int64_t i, float x, float y, float z) {
    if (p) p[3 * i] = x, p[3 * i + 1] = y, p[3 * i + 2] = z;
}


// ---- the camera's gradient (gsr_backward_camera) ---------------------------------
// What one Gaussian leaves of backward_gaussian.inc for the 27 sums: the factors, not the
// products, so that only dh and dc live through the body's SH section.
struct CameraTerms {
    float dh[3];          // dL/d(hom.x, hom.y, hom.w)
    float dc[3];          // dL/dcampos through the SH direction
    float dt[3];          // dL/dt, t the view-space mean (the clamp's and the planes' terms in dt[2])
    float dA0[3], dA1[3]; // dL/dA, A = J R
    float J[4];           // J00, J02, J11, J12
    float q[4];           // the world mean, 1
};
constexpr int kCamSums = kCameraSums;  // view matrix rows 0..2 (12), projection rows 0, 1, 3 (12), campos (3)

// Sum k of the block's Gaussians, in the order the finish (k_camera_finish) maps back:
//   k = 3 c + r      (k < 12)  dL/dvm[4 c + r], r < 3: dt_r q_c + (J^T dA)[r][c] for c < 3
//   k = 12 + 3 c + j           dL/dpm[4 c + r], r = 0, 1, 3 for j = 0, 1, 2: dh_j q_c
//   k = 24 + i                 dL/dcampos[i]
// Called by every thread of the block (a thread without a kept Gaussian brings zeros): a row of 16
// lanes by DPP, the block's 16 rows through LDS in a fixed order, then one word per sum to
// partials[k * gridDim.x + blockIdx.x].
__device__ __forceinline__ void camera_block_sums(const CameraTerms &t, float *partials) {
    __shared__ float s_cam[16][kCamSums];
    float v[kCamSums];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        v[3 * c] = t.dt[0] * t.q[c];
        v[3 * c + 1] = t.dt[1] * t.q[c];
        v[3 * c + 2] = t.dt[2] * t.q[c];
        if (c < 3) {
            v[3 * c] += t.J[0] * t.dA0[c];
            v[3 * c + 1] += t.J[2] * t.dA1[c];
            v[3 * c + 2] += t.J[1] * t.dA0[c] + t.J[3] * t.dA1[c];
        }
#pragma unroll
        for (int j = 0; j < 3; ++j) v[12 + 3 * c + j] = t.dh[j] * t.q[c];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) v[24 + i] = t.dc[i];
    const int row = threadIdx.x >> 4;
#pragma unroll
    for (int k = 0; k < kCamSums; ++k) {
        const float sum = row_sum(v[k]);
        if ((threadIdx.x & 15) == 0) s_cam[row][k] = sum;
    }
    __syncthreads();
    if (threadIdx.x < kCamSums) {
        float sum = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += s_cam[r][threadIdx.x];
        partials[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = sum;
    }
}

// One block per sum: the column of the blocks' partials in double, a thread's share in index
// order, the block's 256 shares by a fixed tree; rounded once.  The same partials give the same
// bits.  The entries the forward never reads (the view matrix's row 3, the projection's row 2:
// nothing reads hom.z) are written as 0.
__global__ __launch_bounds__(256) void k_camera_finish(const float *partials, uint32_t blocks,
                                                       float *dL_dviewmatrix,
                                                       float *dL_dprojmatrix, float *dL_dcampos) {
    __shared__ double s_sum[256];
    const uint32_t k = blockIdx.x;
    const float *col = partials + (size_t)k * blocks;
    double acc = 0.0;
    for (uint32_t i = threadIdx.x; i < blocks; i += 256) acc += (double)col[i];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (uint32_t n = 128; n > 0; n >>= 1) {
        if (threadIdx.x < n) s_sum[threadIdx.x] += s_sum[threadIdx.x + n];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const float out = (float)s_sum[0];
    if (k < 12) {
        const uint32_t c = k / 3, r = k % 3;
        if (dL_dviewmatrix) {
            dL_dviewmatrix[4 * c + r] = out;
            if (r == 0) dL_dviewmatrix[4 * c + 3] = 0.f;
        }
    } else if (k < 24) {
        const uint32_t c = (k - 12) / 3, j = (k - 12) % 3;
        if (dL_dprojmatrix) {
            dL_dprojmatrix[4 * c + (j == 2 ? 3 : j)] = out;
            if (j == 0) dL_dprojmatrix[4 * c + 2] = 0.f;
        }
    } else if (dL_dcampos) {
        dL_dcampos[k - 24] = out;
    }
}

// The four kernels are the statements of backward_gaussian.inc; the second adds the planes' term,
// the camera pair keeps the camera's factors (the text as a lambda's body: its early returns leave
// the lambda, not the kernel) and sums them over the block.
__global__ __launch_bounds__(256) void k_preprocess_bwd(const GsrPreprocessBwdArgs a) {
    constexpr bool kPlanes = false, kCamera = false, kAA = false;
    [[maybe_unused]] float *const dL_ddepths = nullptr;
    [[maybe_unused]] const float *const opacities = nullptr;
    [[maybe_unused]] CameraTerms cam;
#include "backward_gaussian.inc"
}
__global__ __launch_bounds__(256) void k_preprocess_bwd_planes(const GsrPreprocessBwdArgs a,
                                                               float *dL_ddepths) {
    constexpr bool kPlanes = true, kCamera = false, kAA = false;
    [[maybe_unused]] const float *const opacities = nullptr;
    [[maybe_unused]] CameraTerms cam;
#include "backward_gaussian.inc"
}
__global__ __launch_bounds__(256) void k_preprocess_bwd_camera(const GsrPreprocessBwdArgs a,
                                                               float *partials) {
    constexpr bool kPlanes = false, kCamera = true, kAA = false;
    [[maybe_unused]] float *const dL_ddepths = nullptr;
    [[maybe_unused]] const float *const opacities = nullptr;
    CameraTerms cam{};
    [&] {
#include "backward_gaussian.inc"
    }();
    camera_block_sums(cam, partials);
}
__global__ __launch_bounds__(256) void k_preprocess_bwd_planes_camera(const GsrPreprocessBwdArgs a,
                                                                      float *dL_ddepths,
                                                                      float *partials) {
    constexpr bool kPlanes = true, kCamera = true, kAA = false;
    [[maybe_unused]] const float *const opacities = nullptr;
    CameraTerms cam{};
    [&] {
#include "backward_gaussian.inc"
    }();
    camera_block_sums(cam, partials);
}

// The same four with kAA set (gsr_backward_filtered, antialiasing): the effective opacity's
// factor s and its gradient through the 2D covariance; `opacities` is the forward's input.
__global__ __launch_bounds__(256) void k_preprocess_bwd_aa(const GsrPreprocessBwdArgs a,
                                                           const float *opacities) {
    constexpr bool kPlanes = false, kCamera = false, kAA = true;
    [[maybe_unused]] float *const dL_ddepths = nullptr;
    [[maybe_unused]] CameraTerms cam;
#include "backward_gaussian.inc"
}
__global__ __launch_bounds__(256) void k_preprocess_bwd_planes_aa(const GsrPreprocessBwdArgs a,
                                                                  float *dL_ddepths,
                                                                  const float *opacities) {
    constexpr bool kPlanes = true, kCamera = false, kAA = true;
    [[maybe_unused]] CameraTerms cam;
#include "backward_gaussian.inc"
}
__global__ __launch_bounds__(256) void k_preprocess_bwd_camera_aa(const GsrPreprocessBwdArgs a,
                                                                  float *partials,
                                                                  const float *opacities) {
    constexpr bool kPlanes = false, kCamera = true, kAA = true;
    [[maybe_unused]] float *const dL_ddepths = nullptr;
    CameraTerms cam{};
    [&] {
#include "backward_gaussian.inc"
    }();
    camera_block_sums(cam, partials);
}
__global__ __launch_bounds__(256) void k_preprocess_bwd_planes_camera_aa(
    const GsrPreprocessBwdArgs a, float *dL_ddepths, float *partials, const float *opacities) {
    constexpr bool kPlanes = true, kCamera = true, kAA = true;
    CameraTerms cam{};
    [&] {
#include "backward_gaussian.inc"
    }();
    camera_block_sums(cam, partials);
}

}  // namespace

// A strip's arguments must describe rows of the frame: the kernels index with them unchecked.
static bool strip_ok(const GsrBlendBwdArgs &a, const GsrStripBwdArgs *r) {
    if (!r) return true;
    if (a.grid_x == 0 || a.n_tiles % a.grid_x != 0 || r->y0 != (int)r->row_begin * GSR_TILE_Y)
        return false;
    const int64_t end = ((int64_t)r->row_begin + a.n_tiles / a.grid_x) * GSR_TILE_Y;
    return r->y0 < a.H && r->rows_out == (int)std::min<int64_t>(a.H, end) - r->y0;
}

hipError_t gsr_launch_blend_bwd(const GsrBlendBwdArgs &a, const GsrPlaneBwdArgs *p,
                                const GsrDetBwdArgs *d, const GsrStripBwdArgs *strip,
                                hipStream_t s, bool abs) {
    if (p && (!p->z_bits || (!p->dL_ddepth_map && !p->dL_dinv_depth_map && !p->dL_dfinal_T)))
        return hipErrorInvalidValue;
    const bool no_gradient = !p && !a.dL_dcolor;
    if (d && (no_gradient || !d->strip_rect || !d->slab || !d->sums || !d->marks ||
              d->K >= (1u << 30)))
        return hipErrorInvalidValue;
    if (a.n_tiles == 0) return hipSuccess;
    if (no_gradient || !strip_ok(a, strip)) return hipErrorInvalidValue;
    auto launch = [&](auto kernel, auto... more) {
        hipLaunchKernelGGL(kernel, dim3(a.n_tiles), dim3(256), 0, s, a, more...);
    };
    switch ((p ? 1 : 0) | (d ? 2 : 0) | (strip ? 4 : 0) | (abs ? 8 : 0)) {
        case 0: launch(k_blend_bwd_q); break;
        case 1: launch(k_blend_bwd_planes_q, *p); break;
        case 2: launch(k_blend_bwd_det_q, *d); break;
        case 3: launch(k_blend_bwd_planes_det_q, *p, *d); break;
        case 4: launch(k_blend_bwd_strip_q, *strip); break;
        case 5: launch(k_blend_bwd_planes_strip_q, *p, *strip); break;
        case 6: launch(k_blend_bwd_det_strip_q, *d, *strip); break;
        case 7: launch(k_blend_bwd_planes_det_strip_q, *p, *d, *strip); break;
        case 8: launch(k_blend_bwd_abs_q); break;
        case 9: launch(k_blend_bwd_planes_abs_q, *p); break;
        case 10: launch(k_blend_bwd_det_abs_q, *d); break;
        case 11: launch(k_blend_bwd_planes_det_abs_q, *p, *d); break;
        case 12: launch(k_blend_bwd_strip_abs_q, *strip); break;
        case 13: launch(k_blend_bwd_planes_strip_abs_q, *p, *strip); break;
        case 14: launch(k_blend_bwd_det_strip_abs_q, *d, *strip); break;
        case 15: launch(k_blend_bwd_planes_det_strip_abs_q, *p, *d, *strip); break;
    }
    return hipGetLastError();
}

hipError_t gsr_launch_blend_bwd_features(const GsrBlendBwdArgs &a, const float *features, int C,
                                         const float *dL_dfeature_map, float *dL_dfeatures,
                                         hipStream_t s, const GsrStripBwdArgs *strip) {
    if (!features || !dL_dfeature_map || C < 1) return hipErrorInvalidValue;
    if (a.n_tiles == 0) return hipSuccess;
    if (!strip_ok(a, strip)) return hipErrorInvalidValue;
    FeatBwdArgs ft{features, dL_dfeature_map, dL_dfeatures, C, 0,
                   (reinterpret_cast<uintptr_t>(features) & 15) == 0 && C % 4 == 0};
    const GsrStripBwdArgs r = strip ? *strip : GsrStripBwdArgs{};
    while (ft.c0 < C) {
        // the rest of the channels in the narrowest of 4, 8, 16 that holds it, else 16: at C3 one
        // launch of 16 (22 row sums per splat, 3 waves per SIMD) takes 1.66 ms where two of 8
        // (14 row sums, 4 waves) take 2.19 ms -- the two passes over the list, the exp and the six
        // geometry sums are paid per launch
        const int rest = C - ft.c0, w = rest > 8 ? 16 : rest > 4 ? 8 : 4;
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(a.n_tiles), dim3(256), 0, s, a, ft, r);
        };
        if (w == 4) {
            if (strip) launch(k_blend_bwd_features_q<4, true>);
            else launch(k_blend_bwd_features_q<4, false>);
        } else if (w == 8) {
            if (strip) launch(k_blend_bwd_features_q<8, true>);
            else launch(k_blend_bwd_features_q<8, false>);
        } else {
            if (strip) launch(k_blend_bwd_features_q<16, true>);
            else launch(k_blend_bwd_features_q<16, false>);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ft.c0 += w;
    }
    return hipSuccess;
}

hipError_t gsr_launch_strip_gate(const uint2 *strip_rect, int64_t P, int32_t *radii,
                                 hipStream_t s) {
    if (P <= 0) return hipSuccess;
    if (!strip_rect || !radii) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_strip_gate, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s,
                       strip_rect, P, radii);
    return hipGetLastError();
}

int64_t gsr_slab_blocks(int64_t P) { return (P + kSlabBlock - 1) / kSlabBlock; }

hipError_t gsr_launch_slab_scan(const uint2 *strip_rect, int64_t P, uint64_t *partials,
                                uint64_t *slab, hipStream_t s) {
    if (P <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)gsr_slab_blocks(P);
    hipLaunchKernelGGL(k_slab_reduce, dim3(blocks), dim3(256), 0, s, strip_rect, P, partials);
    hipLaunchKernelGGL(k_slab_scan_partials, dim3(1), dim3(256), 0, s, partials, blocks);
    hipLaunchKernelGGL(k_slab_apply, dim3(blocks), dim3(256), 0, s, strip_rect, P, partials, slab);
    return hipGetLastError();
}

hipError_t gsr_launch_means2d_abs(const int32_t *radii, const float *grad2d, int64_t P, int W,
                                  int H, float *dL_dmeans2D_abs, hipStream_t s) {
    if (P <= 0) return hipSuccess;
    if (!radii || !grad2d || !dL_dmeans2D_abs) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_means2d_abs, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, s, radii,
                       grad2d, P, W, H, dL_dmeans2D_abs);
    return hipGetLastError();
}

hipError_t gsr_launch_grad_rows_gather(const GsrDetBwdArgs &d, int64_t P, bool planes,
                                       float *grad2d, hipStream_t s, bool abs) {
    if (P <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((P + 15) / 16);
    if (abs && planes)
        hipLaunchKernelGGL(k_grad_rows_gather_abs<12>, dim3(blocks), dim3(256), 0, s, d, P,
                           grad2d);
    else if (abs)
        hipLaunchKernelGGL(k_grad_rows_gather_abs<11>, dim3(blocks), dim3(256), 0, s, d, P,
                           grad2d);
    else if (planes)
        hipLaunchKernelGGL(k_grad_rows_gather<10>, dim3(blocks), dim3(256), 0, s, d, P, grad2d);
    else
        hipLaunchKernelGGL(k_grad_rows_gather<9>, dim3(blocks), dim3(256), 0, s, d, P, grad2d);
    return hipGetLastError();
}

hipError_t gsr_launch_preprocess_bwd(const GsrPreprocessBwdArgs &args,
                                     const GsrPreprocessBwdExtras &x, hipStream_t s) {
    const GsrCameraBwdArgs *const c = x.camera;
    if (c && (!c->partials || (!c->dL_dviewmatrix && !c->dL_dprojmatrix && !c->dL_dcampos)))
        return hipErrorInvalidValue;
    if (args.P == 0) return hipSuccess;
    GsrPreprocessBwdArgs a = args;
    a.sh_vec4 = a.shs && a.M == 16 && (reinterpret_cast<uintptr_t>(a.shs) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(a.dL_dsh) & 15) == 0;
    const unsigned blocks = (unsigned)gsr_preprocess_blocks(a.P);
    const float *const op = x.aa_opacities;
    float *const part = c ? c->partials : nullptr;
    auto launch = [&](auto kernel, auto... more) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, s, a, more...);
    };
    switch ((x.planes ? 1 : 0) | (c ? 2 : 0) | (op ? 4 : 0)) {
        case 0: launch(k_preprocess_bwd); break;
        case 1: launch(k_preprocess_bwd_planes, x.dL_ddepths); break;
        case 2: launch(k_preprocess_bwd_camera, part); break;
        case 3: launch(k_preprocess_bwd_planes_camera, x.dL_ddepths, part); break;
        case 4: launch(k_preprocess_bwd_aa, op); break;
        case 5: launch(k_preprocess_bwd_planes_aa, x.dL_ddepths, op); break;
        case 6: launch(k_preprocess_bwd_camera_aa, part, op); break;
        case 7: launch(k_preprocess_bwd_planes_camera_aa, x.dL_ddepths, part, op); break;
    }
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !c) return e;
    hipLaunchKernelGGL(k_camera_finish, dim3(kCamSums), dim3(256), 0, s, part, blocks,
                       c->dL_dviewmatrix, c->dL_dprojmatrix, c->dL_dcampos);
    return hipGetLastError();
}
