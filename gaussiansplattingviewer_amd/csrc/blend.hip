// blend.hip -- per-tile front-to-back alpha compositing for gfx950.
//
// Replaces upstream diff-gaussian-rasterization forward.cu renderCUDA (GLSL twin of the
// per-pixel alpha: shaders/gau_frag.glsl:21-27).  k_blend_q: one wave per (16x16 tile, 8x8
// quadrant), one pixel per lane, a tile's four quadrant waves in one 256-thread block that never
// synchronises (each wave is independent; one block per tile instead of one per quadrant:
// blend -2 %, C3 +2 % in flight, profiles/r06p_ab_blend_tile_blocks.txt).  Each wave streams its
// tile's depth-sorted list 64 splats at a time, culls them against its own quadrant (the
// splat's conservative alpha >= 1/255 ellipse from preprocess.hip cull_data: bounding box,
// then the exact ellipse-vs-box minimum with a rounding bound), compacts the survivors into
// LDS with a ballot, composites them two at a time, and stops at the pair after which its 64
// pixels are done (kStopPairs below: the rest of the chunk's survivors would be composited at
// weight 0 in every lane).  At C3, on tight lists, a quadrant wave examines 2.99 chunks (~190
// list entries), stages 127.3 splats and composites 104.4 of them (a per-wave timeline,
// tools/lab/blend_trace.py; profiles/r07b_blend_trace.txt); by the ISA about two thirds of its
// VALU is the compositing loop (33 VALU + 5 LDS reads per composited pair, and the exit's one
// compare) and one third the per-chunk gather, cull and staging.
//
// Skipping splats that provably cannot reach alpha >= 1/255 changes nothing: upstream skips
// them too (`if (alpha < 1/255) continue`), and n_contrib -- upstream's running `contributor`
// at the last contributing splat -- is that splat's list position + 1 either way.
// Arithmetic (GSR_OPT_BLEND_FAST): 1 (default) stages each splat as the exponent's quadratic in
// the lane's offset from the quadrant centre, with log2(e), -1/2 and log2(opacity) folded in
// (5 FMA per pixel, then the raw v_exp_f32); 0 keeps upstream's per-pixel operation order (the
// core of ocml's expf).  Both are within the
// image tolerance of tests/gpu_helpers.py.
#include <type_traits>

#include "blend_order.h"

using namespace gsr;

namespace {

// Block -> tile, XCD-aware: the hardware deals block b to XCD b % 8 (speed only, never
// correctness); groups of kGroupTiles consecutive tiles (four row-adjacent tiles, 16 quadrant
// waves) go round-robin over the XCDs, so each group shares one L2 while the image's heavy and
// light regions are spread evenly over the 8 XCDs.  With `order` (blend_order.h) the groups are
// dealt heaviest first: every wave of the last round is then a short one, and the kernel's
// tail -- the last waves finishing on an emptying chip -- shrinks.
__device__ __forceinline__ uint32_t xcd_tile(uint32_t b, const uint32_t *order,
                                             uint32_t n_groups) {
    const uint32_t x = b & 7u, l = b >> 3;
    uint32_t g = (l / kGroupTiles) * 8u + x;
    if (order && g < n_groups) g = order[g];
    return g * kGroupTiles + l % kGroupTiles;
}

// One staged splat as the inner loop reads it: three 16-B LDS reads from one address (fast
// arithmetic without n_contrib: a pair shares the even slot's e = {b0, b1, bound0, bound1}).
// exact: g = x, y, conic a, conic b; q = conic c, opacity, r, g; e = b, position + 1 (uint bits:
// upstream's `contributor`), -, -.
// fast: the exponent as a quadratic in the lane's offset (u, v) from the quadrant centre,
// log2(opacity) folded in: p = k0 + k1 u + k2 v + k3 u^2 + k4 uv + k5 v^2 (g = k0..k3,
// q = k4, k5, r, g); e = b, position + 1, the bound p must not exceed (log2(opacity): p > it <=>
// upstream's power > 0; +inf for a positive-definite conic), -.
struct StagedSplat {
    float4 g;
    float4 q;
    float4 e;
};

// Blocks are mapped XCD-aware (xcd_tile).  Only the next chunk's point-list ids are
// prefetched (no record prefetch): the kernel fits 64 VGPRs and 8 waves per SIMD, and the
// record gathers' latency is left to the other waves (a record prefetch spilled at 8 waves
// and lost at fewer).  A block per tile with shared staging lost to independent
// quadrant waves (its batch barriers cost ~40 % of wave time), and so did a separate kernel
// culling each splat once per tile into per-quadrant lists (the in-wave cull is ~5 % of the
// blend's VALU; the extra pass over the lists cost more than it saved).
// kContrib: track the last contributor (the n_contrib output); off (no n_contrib requested),
// the composite step loses one v_cndmask.
//
// kDepth (k_blend_depth_q, gsr_forward_depth): two more accumulators per pixel, the expected
// view-space depth and inverse depth sum z w and sum (1/z) w over the very splats and with the very
// weight w of the colour channels (a colour channel with the feature in place of the colour: the
// twin property).  z is gathered by Gaussian id from the depth keys (its bits,
// preprocess.hip back_one), 1/z is one IEEE division per staged splat, and the pair {z0, 1/z0,
// z1, 1/z1} lies in 16 B of LDS of its own (the paired-slot layout has no spare word in e): one
// more LDS read per composited pair.  The pad slot of an odd count holds 0, 0 (weight 0 times a
// finite feature).  Without kDepth none of it is compiled: k_blend_q is the kernel it was.
//
// kMedian (k_blend_surface_q, gsr_forward_surface): the median splat of a pixel is the composited
// splat in front of which T > 0.5 and behind which T <= 0.5.  T only falls, so at most one splat
// of a list qualifies: the pixel keeps that splat's list position + 1 (the word the kContrib
// staging carries, so these kernels stage unpaired whatever kContrib is) -- two compares and a
// select per composited splat -- and the epilogue gathers the Gaussian id from the list and z from
// the depth keys once per pixel.  The terminating splat cannot qualify (alpha <= 0.99 and
// T' < 1e-4 need T < 0.01), nor can a skipped one (T' = T), nor anything after the pixel is done
// (T <= 0).  Without kMedian none of it is compiled.
//
// kStopPairs: after every kStopPairs composited pairs the wave asks whether any of its pixels
// is still live and, if none is, leaves the pair loop and with it the chunk loop (no further
// gather, cull or staging).  A done pixel has T <= 0: its weight is 0, -|T| is idempotent, and
// neither last_contributor nor median_pos can change, so for finite inputs the composites
// skipped change no bit of the colour, final_T, n_contrib, the depth planes or the median outputs.
// 1 of 1, 2, 4, 8 by measurement (profiles/r07b_ab_blend_stop.txt): the test after every pair is
// the loop's own back edge (one v_cmp, the scalar branch it already had) and the serial C3 blend
// goes 113.5 -> 101-103 us; a test every 2, 4 or 8 pairs compiles to a second branch and a
// recomputed LDS address per pair and gains less (108-110 us).
//
// kFeat (k_blend_features_q, gsr_forward_features): the composite with kFeat channels of the
// caller's own in place of the three colours: channels [ft.c0, ft.c0 + kFeat) of the Gaussians'
// feature rows ([P, C] floats), each accumulated under the colour's weight as a colour channel is
// (the twin property).  The lane that stages a splat gathers its kFeat words into LDS,
// slot for slot (words at or beyond C are zeros and never read from memory); the composite reads
// the row by broadcast.  No colour, final_T, n_contrib, depth or median work: the epilogue writes
// the planes below C only.  Without kFeat none of it is compiled.
constexpr int kStopPairs = 1;
template <bool kFast, bool kContrib, bool kDepth, bool kMedian = false, int kFeat = 0>
__device__ __forceinline__ void blend_q(const GsrBlendArgs &a, uint32_t n_tiles,
                                        const GsrDepthArgs &d,
                                        const GsrSurfaceArgs &m = GsrSurfaceArgs{},
                                        const GsrFeatureArgs &ft = GsrFeatureArgs{}) {
    static_assert(kFeat % 4 == 0 && kFeat <= 64, "feature chunks are whole float4s, a lane a word");
    __shared__ StagedSplat s_spl_q[4][64];  // per quadrant wave
    // paired colour / bound words (see staging)
    constexpr bool kPair = kFast && !kContrib && !kMedian;

    const uint32_t tile = xcd_tile(blockIdx.x, a.order, (n_tiles + kGroupTiles - 1) / kGroupTiles);
    if (tile >= n_tiles) return;
    if (a.list_n && *a.list_n > a.list_cap) return;  // not binned (frame graphs: re-rendered)
    const uint32_t quad = threadIdx.x >> 6;  // this wave's quadrant
    const int lane = threadIdx.x & 63;
    StagedSplat *const s_spl = s_spl_q[quad];
    float2 *s_zf = nullptr;  // kDepth: {z, 1 / z} of the staged splats, slot for slot
    if constexpr (kDepth) {
        __shared__ alignas(16) float2 s_zf_q[4][64];  // (a pair: one 16-B read)
        s_zf = s_zf_q[quad];
    }
    float *s_ft = nullptr;  // kFeat: the staged splats' feature words, slot for slot
    if constexpr (kFeat > 0) {
        __shared__ alignas(16) float s_ft_q[4][64 * kFeat];
        s_ft = s_ft_q[quad];
    }
    const uint32_t tx = tile % a.grid_x, ty_local = tile / a.grid_x, ty = a.row_begin + ty_local;
    const int qx0 = (int)tx * GSR_TILE_X + (int)(quad & 1u) * 8;
    const int qy0 = (int)ty * GSR_TILE_Y + (int)(quad >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pfx = (float)px, pfy = (float)py;
    // fast: the lane's offset from the quadrant centre and its products (exact small values)
    const float pu = (float)(lane & 7) - 3.5f, pv = (float)(lane >> 3) - 3.5f;
    const float puu = pu * pu, puv = pu * pv, pvv = pv * pv;

    const uint2 range = a.ranges[tile];
    // done carried in the sign of T (T <= 0: the lane composites no more)
    float T = inside ? 1.0f : -1.0f, C0 = 0.0f, C1 = 0.0f, C2 = 0.0f;
    float D0 = 0.0f, D1 = 0.0f;  // kDepth: sum z w, sum (1 / z) w
    [[maybe_unused]] float F[kFeat > 0 ? kFeat : 1] = {};  // kFeat: sum f_c w
    uint32_t last_contributor = 0;
    uint32_t median_pos = 0;  // kMedian: list position + 1 of the median splat, 0 = none (yet)
    auto live_any = [&]() { return __ballot(!(T <= 0.0f)) != 0ull; };
    if (!live_any()) return;

    // kBound (fast form): test upstream's power > 0 skip as p > bound -- only chunks holding a
    // conic that is not positive definite need it (staging below)
    // frow (kFeat): the splat's feature words in LDS
    auto composite = [&](const StagedSplat &sp, float fz, float fiz, auto bound_tag,
                         [[maybe_unused]] const float *frow = nullptr) {
        constexpr bool kBound = decltype(bound_tag)::value;
        [[maybe_unused]] float f[kFeat > 0 ? kFeat : 1];
        if constexpr (kFeat > 0) {
#pragma unroll
            for (int c = 0; c < kFeat; c += 4) {
                const float4 v = *reinterpret_cast<const float4 *>(frow + c);
                f[c] = v.x, f[c + 1] = v.y, f[c + 2] = v.z, f[c + 3] = v.w;
            }
        }
        bool vis, acc, term;
        float test_T;
        if (kFast) {
            // The loop-carried chain is only T -> T (1 - alpha_eff) -> compare -> select:
            // alpha_eff = 0 for an invisible splat (then test_T = T), and a pixel that
            // terminates keeps -|T| (idempotent once done).  The weight is |T| - |T'|: T - test_T
            // while the pixel composites, 0 for the terminating splat and after it.
            float p2 = __builtin_fmaf(sp.g.y, pu, sp.g.x);
            p2 = __builtin_fmaf(sp.g.z, pv, p2);
            p2 = __builtin_fmaf(sp.g.w, puu, p2);
            p2 = __builtin_fmaf(sp.q.x, puv, p2);
            p2 = __builtin_fmaf(sp.q.y, pvv, p2);
            const float alpha = fminf(0.99f, __builtin_amdgcn_exp2f(p2));
            vis = !(alpha < 1.0f / 255.0f);
            if (kBound) vis = vis && !(p2 > sp.e.z);
            // T (1 - alpha) as one fma, T - alpha T; alpha_eff = 0 leaves T exactly
            const float alpha_eff = vis ? alpha : 0.0f;
            test_T = __builtin_fmaf(-T, alpha_eff, T);
            const bool lo = test_T < 0.0001f;
            const float T_next = lo ? -fabsf(T) : test_T;
            const float wgt = fabsf(T) - fabsf(T_next);
            if constexpr (kFeat == 0) {
                C0 = __builtin_fmaf(sp.q.z, wgt, C0);
                C1 = __builtin_fmaf(sp.q.w, wgt, C1);
                C2 = __builtin_fmaf(sp.e.x, wgt, C2);
            } else {
#pragma unroll
                for (int c = 0; c < kFeat; ++c) F[c] = __builtin_fmaf(f[c], wgt, F[c]);
            }
            if constexpr (kDepth) {
                D0 = __builtin_fmaf(fz, wgt, D0);
                D1 = __builtin_fmaf(fiz, wgt, D1);
            }
            if (kContrib)
                last_contributor = (vis && !lo) ? __float_as_uint(sp.e.y) : last_contributor;
            if constexpr (kMedian)  // (a done pixel has T <= 0; a skipped splat test_T = T)
                median_pos = (T > 0.5f && test_T <= 0.5f) ? __float_as_uint(sp.e.y) : median_pos;
            T = T_next;
            return;
        } else {
            const float dx = sp.g.x - pfx, dy = sp.g.y - pfy;
            const float power =
                -0.5f * (sp.g.z * dx * dx + sp.q.x * dy * dy) - sp.g.w * dx * dy;
            const float alpha = fminf(0.99f, sp.q.y * exp_core(power));
            vis = !(power > 0.0f) && !(alpha < 1.0f / 255.0f);
            test_T = T * (1 - alpha);
            acc = vis && !(test_T < 0.0001f);
            term = vis && (test_T < 0.0001f);
            if constexpr (kFeat == 0) {
                C0 = acc ? C0 + sp.q.z * alpha * T : C0;
                C1 = acc ? C1 + sp.q.w * alpha * T : C1;
                C2 = acc ? C2 + sp.e.x * alpha * T : C2;
            } else {
#pragma unroll
                for (int c = 0; c < kFeat; ++c) F[c] = acc ? F[c] + f[c] * alpha * T : F[c];
            }
            if constexpr (kDepth) {
                D0 = acc ? D0 + fz * alpha * T : D0;
                D1 = acc ? D1 + fiz * alpha * T : D1;
            }
            if constexpr (kMedian)
                median_pos =
                    (acc && T > 0.5f && test_T <= 0.5f) ? __float_as_uint(sp.e.y) : median_pos;
        }
        T = acc ? test_T : (term ? -fabsf(T) : T);
        if (kContrib) last_contributor = acc ? __float_as_uint(sp.e.y) : last_contributor;
    };
    const float X0 = (float)qx0, Y0 = (float)qy0;

    // the next chunk's ids are in flight while this chunk's records are gathered
    const uint32_t i0 = range.x + (uint32_t)lane;
    uint32_t id_next = i0 < range.y ? (a.point_list[i0] & a.id_mask) : 0u;
    for (uint32_t start = range.x; start < range.y; start += 64) {
        const uint32_t idx = start + (uint32_t)lane;
        const bool valid = idx < range.y;
        SplatRecord r;
        if (valid) r = a.records[id_next];
        float z = 1.0f;  // kDepth: by Gaussian id, as the record
        if constexpr (kDepth)
            if (valid) z = __uint_as_float(d.z_bits[id_next]);
        [[maybe_unused]] const uint32_t id_cur = id_next;  // kFeat: the feature row's
        if (idx + 64u < range.y) id_next = (a.point_list[idx + 64u] & a.id_mask);

        bool keep = valid;
        if (valid && a.cull)
            keep = may_touch(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.z, r.b.w, 2.0f * r.c.x, X0,
                             X0 + 7, Y0, Y0 + 7);
        const uint64_t bal = __ballot(keep);
        bool npd = false;  // a staged conic that is not positive definite (fast form)
        if (keep) {
            StagedSplat st;
            if (kFast) {
                // exponent log2(e) * (-q/2) = a dx^2 + b dx dy + c dy^2 with dx = ex - u,
                // dy = ey - v, expanded in (u, v)
                const float kL2e = 1.4426950408889634f;
                float ca = r.a.z * (-0.5f * kL2e), cb = r.a.w * (-kL2e),
                      cc = r.b.x * (-0.5f * kL2e);
                const float ex = r.a.x - (X0 + 3.5f), ey = r.a.y - (Y0 + 3.5f);
                float lo = __builtin_amdgcn_logf(r.b.y);  // log2(opacity)
                // the conic as upstream reads it (before the rescaling below)
                const bool pd = ca < 0.0f && cc < 0.0f && 4.0f * ca * cc > cb * cb;
                bool neg_inf = false;
                if (r.b.y < 0.0f) {
                    // a negative opacity has no logarithm.  Upstream's alpha = o exp(power) is
                    // negative (skipped): exponent -inf.  Except for o = -inf where exp(power)
                    // underflows to 0 (power log2(e) < -150): -inf * 0 = NaN and min(0.99, NaN) =
                    // 0.99.  There the exponent becomes -2^20 (power log2(e) + 150), by exact
                    // scaling of the conic: >= 0 (alpha 0.99) where upstream's exp is 0, and
                    // below -8 (alpha < 1/255) within 8e-6 above that threshold, power > 0 included
                    neg_inf = r.b.y == -__builtin_huge_valf();
                    lo = -__builtin_huge_valf();
                    if (neg_inf) {
                        ca *= -0x1p20f, cb *= -0x1p20f, cc *= -0x1p20f;
                        lo = -150.0f * 0x1p20f;
                    }
                }
                const float k0 = __builtin_fmaf(ex, __builtin_fmaf(ca, ex, cb * ey), cc * ey * ey);
                st.g = make_float4(k0 + lo, __builtin_fmaf(-2.0f * ca, ex, -cb * ey),
                                   __builtin_fmaf(-cb, ex, -2.0f * cc * ey), ca);
                st.q = make_float4(cb, cc, r.c.y, r.c.z);
                // upstream skips power > 0, which a positive-definite conic reaches only through
                // rounding; the expanded form rounds differently (at a centre that falls on a
                // pixel it can land just above 0), so the test is kept for the other conics only
                npd = !pd && !neg_inf;
                st.e = make_float4(r.c.w, __uint_as_float(idx - range.x + 1u),
                                   (pd || neg_inf) ? __builtin_huge_valf() : lo, 0.0f);
            } else {
                st.g = r.a;
                st.q = make_float4(r.b.x, r.b.y, r.c.y, r.c.z);
                st.e = make_float4(r.c.w, __uint_as_float(idx - range.x + 1u), 0.0f, 0.0f);
            }
            const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
            const int slot = __popcll(bal & lt);  // compacted in list order
            if (kPair) {
                // a pair's blues and power bounds share the even slot's e: {b0, b1, bound0,
                // bound1} (5 LDS reads per composited pair instead of 6)
                s_spl[slot].g = st.g;
                s_spl[slot].q = st.q;
                float *pe = &s_spl[slot & ~1].e.x;
                pe[slot & 1] = st.e.x;
                pe[2 + (slot & 1)] = st.e.z;
            } else {
                s_spl[slot] = st;
            }
            if constexpr (kDepth) s_zf[slot] = make_float2(z, 1.0f / z);
            if constexpr (kFeat > 0) {
                // words [c0, c0 + n) of the Gaussian's row; n <= kFeat, the rest of the chunk 0
                const float *src = ft.features + (size_t)id_cur * ft.C + ft.c0;
                const int n = ft.C - ft.c0;
                float *dst = s_ft + slot * kFeat;
                if (ft.vec4) {  // 16-B aligned rows (C, c0 and so n multiples of 4)
#pragma unroll
                    for (int c = 0; c < kFeat; c += 4)
                        *reinterpret_cast<float4 *>(dst + c) =
                            c < n ? *reinterpret_cast<const float4 *>(src + c)
                                  : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                } else {
#pragma unroll
                    for (int c = 0; c < kFeat; ++c) dst[c] = c < n ? src[c] : 0.0f;
                }
            }
        }
        int count = __popcll(bal);
        if (count == 0) continue;
        // the compacted slots are the list (no index indirection); an odd count is padded with
        // an opacity-0 splat in slot `count` (< 64 for an odd count): exact: opacity 0; fast:
        // exponent -inf (alpha 0, the bound-free loop included) and a power bound of -inf
        if (count & 1) {
            if (kPair) {
                if (lane < 8)
                    reinterpret_cast<float *>(&s_spl[count])[lane] =
                        lane == 0 ? -__builtin_huge_valf() : 0.0f;
                if (lane == 8) s_spl[count - 1].e.y = 0.0f;
                if (lane == 9) s_spl[count - 1].e.w = -__builtin_huge_valf();
            } else if (lane < 12) {
                reinterpret_cast<float *>(&s_spl[count])[lane] =
                    (kFast && (lane == 0 || lane == 10)) ? -__builtin_huge_valf() : 0.0f;
            }
            if constexpr (kDepth)
                if (lane == 12) s_zf[count] = make_float2(0.0f, 0.0f);
            if constexpr (kFeat > 0)  // (weight 0 times a finite feature)
                if (lane < kFeat) s_ft[count * kFeat + lane] = 0.0f;
            ++count;
        }
        // one wave: its LDS writes above complete before the reads below are served

        // single-buffered: a software-pipelined form (the next pair's LDS reads in flight
        // during this pair) spilled past 64 VGPRs and was slower
        auto composite_all = [&](auto bound_tag) {
            int k = 0;  // (count >= 2 and even here)
            do {
                float4 zf = make_float4(0.0f, 0.0f, 0.0f, 0.0f);  // the pair's {z, 1 / z}
                if constexpr (kDepth) zf = *reinterpret_cast<const float4 *>(&s_zf[k]);
                // (kFeat: the pair's feature rows; without it the argument is not read)
                const float *const f0 = s_ft + k * kFeat, *const f1 = f0 + kFeat;
                if (kPair) {
                    const float4 e = s_spl[k].e;
                    composite(StagedSplat{s_spl[k].g, s_spl[k].q, make_float4(e.x, 0.0f, e.z, 0.0f)},
                              zf.x, zf.y, bound_tag, f0);
                    composite(StagedSplat{s_spl[k + 1].g, s_spl[k + 1].q,
                                          make_float4(e.y, 0.0f, e.w, 0.0f)},
                              zf.z, zf.w, bound_tag, f1);
                } else {
                    const StagedSplat a0 = s_spl[k], a1 = s_spl[k + 1];
                    composite(a0, zf.x, zf.y, bound_tag, f0);
                    composite(a1, zf.z, zf.w, bound_tag, f1);
                }
                k += 2;
                // the early exit (kStopPairs above): k and count are wave-uniform, the test is
                // a compare of T into an SGPR pair and a scalar branch
            } while (k < count && ((k / 2) % kStopPairs != 0 || live_any()));
        };
        // (the exact form always tests power > 0, as upstream writes it)
        if (!kFast || __ballot(npd) != 0ull)
            composite_all(std::integral_constant<bool, true>{});
        else
            composite_all(std::integral_constant<bool, false>{});
        if (!live_any()) break;
    }

    if constexpr (kFeat > 0) {  // the planes below C, no background term; nothing else
        if (inside) {
            const size_t pid = (size_t)(py - a.y0) * a.W + px;
            const size_t plane = (size_t)a.rows_out * a.W;
            const int n = ft.C - ft.c0;
#pragma unroll
            for (int c = 0; c < kFeat; ++c)
                if (c < n) ft.feature_map[(size_t)(ft.c0 + c) * plane + pid] = F[c];
        }
        return;
    }
    if (inside) {
        const int row = py - a.y0;
        const size_t pid = (size_t)row * a.W + px;
        const size_t plane = (size_t)a.rows_out * a.W;
        const float Tf = fabsf(T);
        if (a.final_T) a.final_T[pid] = Tf;
        if (kContrib && a.n_contrib) a.n_contrib[pid] = last_contributor;
        a.out_color[pid] = C0 + Tf * a.bg[0];
        a.out_color[plane + pid] = C1 + Tf * a.bg[1];
        a.out_color[2 * plane + pid] = C2 + Tf * a.bg[2];
        if constexpr (kDepth) {  // premultiplied, no background term
            if (d.depth_map) d.depth_map[pid] = D0;
            if (d.inv_depth_map) d.inv_depth_map[pid] = D1;
        }
        if constexpr (kMedian) {  // no surface: id -1, depth 0
            // (median_pos is a staged position + 1 of this list: range.x + median_pos - 1 < range.y)
            int32_t id = -1;
            float z = 0.0f;
            if (median_pos) {
                id = (int32_t)(a.point_list[range.x + median_pos - 1u] & a.id_mask);
                if (m.median_depth) z = __uint_as_float(d.z_bits[id]);
            }
            if (m.median_depth) m.median_depth[pid] = z;
            if (m.median_id) m.median_id[pid] = id;
        }
    }
}

template <bool kFast, bool kContrib>
__global__ __launch_bounds__(256, 8) void k_blend_q(const GsrBlendArgs a, uint32_t n_tiles) {
    blend_q<kFast, kContrib, false>(a, n_tiles, GsrDepthArgs{});
}

// The depth-accumulating form: 14 KiB of LDS per block; kDepthWaves waves per SIMD leave it the
// registers for the two accumulators and the pair's features without scratch.
// Without n_contrib the kernel has always fitted 72 VGPRs, 7 waves; its bound says so, since
// under a bound of 6 some forms of the early exit's loop took a 73rd
// (profiles/blend_stop_resources.txt).
constexpr int kDepthWaves = 6;
template <bool kFast, bool kContrib>
__global__ __launch_bounds__(256, kContrib ? kDepthWaves : kDepthWaves + 1) void k_blend_depth_q(
    const GsrBlendArgs a, uint32_t n_tiles, const GsrDepthArgs d) {
    blend_q<kFast, kContrib, true>(a, n_tiles, d);
}

// The median-noting forms: the plain composite's 12 KiB of LDS or the depth form's 14 (kDepth).
// The median position is one more live register per pixel: at the plain composite's 8 waves per
// SIMD (64 VGPRs) the fast forms spilled 8 and 16 B per lane, at kSurfaceWaves none do
// (profiles/median_resources.txt); with kDepth the depth form's budget holds it.
constexpr int kSurfaceWaves = 7;
template <bool kFast, bool kContrib, bool kDepth>
__global__ __launch_bounds__(256, kDepth ? kDepthWaves : kSurfaceWaves) void k_blend_surface_q(
    const GsrBlendArgs a, uint32_t n_tiles, const GsrDepthArgs d, const GsrSurfaceArgs m) {
    blend_q<kFast, kContrib, kDepth, true>(a, n_tiles, d, m);
}

// The feature-compositing form (gsr_forward_features): kFeat channels per launch, 12 KiB of staged
// splats and 1 KiB per channel of their feature words.  At kFeat = 16 that is 28 KiB, 5 blocks per
// CU, so the bound is 5 waves per SIMD -- 4 for the fast form, whose pair of splats in flight with
// their two feature rows spilled 56 B per lane at 5 waves' 96 VGPRs; the narrower chunks keep their
// LDS's share of the registers (profiles/features_resources.txt: no scratch in any).
template <bool kFast, int kFeat>
__global__ __launch_bounds__(256, kFeat >= 16 ? (kFast ? 4 : 5)
                                  : kFeat >= 8 ? 6 : 7) void k_blend_features_q(
    const GsrBlendArgs a, uint32_t n_tiles, const GsrFeatureArgs ft) {
    blend_q<kFast, false, false, false, kFeat>(a, n_tiles, GsrDepthArgs{}, GsrSurfaceArgs{}, ft);
}

// Grid of whole XCD groups: one block per tile, kGroupTiles per XCD round; blocks past the
// last tile exit.
inline uint32_t xcd_grid(uint32_t n_tiles) {
    const uint32_t g = kGroupTiles * 8u;
    return (n_tiles + g - 1) / g * g;
}

// ---- the GL backend's geometry shadings (gsr_forward_shaded, include/gsr.h) -------------------
// shaders/gau_frag.glsl:15-38 on the rasterizer's lists: a pixel takes the colour of the first
// entry of its tile's list that hits it -- nothing is composited.  An entry hits
//   billboard (1):        |dx| <= 3 sqrt(cxx) and |dy| <= 3 sqrt(cyy), the axis-aligned quad of
//                         gau_vert.glsl:174 (cxx = c / det, cyy = a / det, det = a c - b^2: the 2D
//                         covariance with its 0.3); the opacity plays no part;
//   the ball modes (2, 3): power <= 0 and alpha = min(0.99, o exp(power)) > 0.22, tested without
//                         a transcendental per pixel as power > ln(0.22 / o) (0.99 > 0.22),
// with upstream's dx = mx - x, dy = my - y, power = -1/2 (a dx^2 + c dy^2) - b dx dy in upstream's
// operation order.  One arithmetic (GSR_OPT_BLEND_FAST does not apply).  The colour is the
// record's rgb, bit for bit (1, 2), or rgb exp(power) (3: the one exp of a pixel, at its hit).
//
// The staged splat, 40 B of LDS: g = {mx, my, ex, ey} (billboard) or {mx, my, a, b} (ball);
// q = {c, threshold, r, g} (billboard: -, -, r, g); e = {b, list position + 1 (uint bits)}.
//
// What is dropped before the scan can never hit, so the cull changes no bit (tested):
//   ball: an opacity not above 0.22f -- the threshold ln(0.22f / o) is then >= 0 while a hit
//     needs power <= 0 -- and, with GSR_OPT_BLEND_CULL, may_touch: alpha > 0.22 lies inside the
//     alpha >= 1/255 region it bounds;
//   billboard: a NaN extent, and with the cull a quad whose box misses the quadrant's pixel-centre
//     box.  The box test is the per-pixel test itself at the nearest column / row: fl(mx - x) is
//     monotone in x, so if the quadrant's nearest pixel fails, all fail.
constexpr int kShadeBillboard = 1, kShadeFlatBall = 2, kShadeGaussBall = 3;

template <int kMode>
__global__ __launch_bounds__(256, 8) void k_shade_q(const GsrBlendArgs a, uint32_t n_tiles) {
    constexpr bool kBill = kMode == kShadeBillboard;
    __shared__ float4 s_g_q[4][64], s_q_q[4][64];  // per quadrant wave
    __shared__ float2 s_e_q[4][64];

    const uint32_t tile = xcd_tile(blockIdx.x, a.order, (n_tiles + kGroupTiles - 1) / kGroupTiles);
    if (tile >= n_tiles) return;
    if (a.list_n && *a.list_n > a.list_cap) return;  // not binned (frame graphs: re-rendered)
    const uint32_t quad = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    float4 *const s_g = s_g_q[quad], *const s_q = s_q_q[quad];
    float2 *const s_e = s_e_q[quad];
    const uint32_t tx = tile % a.grid_x, ty = a.row_begin + tile / a.grid_x;
    const int qx0 = (int)tx * GSR_TILE_X + (int)(quad & 1u) * 8;
    const int qy0 = (int)ty * GSR_TILE_Y + (int)(quad >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pfx = (float)px, pfy = (float)py;
    const float X0 = (float)qx0, Y0 = (float)qy0;

    const uint2 range = a.ranges[tile];
    bool done = !inside;  // hit, or outside the frame
    float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, hit_power = 0.0f;
    uint32_t hit_pos = 0;  // list position + 1 of the hit
    if (__ballot(!done) == 0ull) return;

    const uint32_t i0 = range.x + (uint32_t)lane;
    uint32_t id_next = i0 < range.y ? (a.point_list[i0] & a.id_mask) : 0u;
    for (uint32_t start = range.x; start < range.y; start += 64) {
        const uint32_t idx = start + (uint32_t)lane;
        const bool valid = idx < range.y;
        SplatRecord r;
        if (valid) r = a.records[id_next];
        if (idx + 64u < range.y) id_next = (a.point_list[idx + 64u] & a.id_mask);

        bool keep = valid;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f), q = g;
        if (valid) {
            if (kBill) {
                // the determinant in double: a c ~ b^2 for elongated splats would cancel in float
                const float det = (float)((double)r.a.z * (double)r.b.x - (double)r.a.w * (double)r.a.w);
                const float ex = 3.0f * sqrtf(r.b.x / det), ey = 3.0f * sqrtf(r.a.z / det);
                keep = ex == ex && ey == ey;
                if (keep && a.cull) {
                    const float ulo = X0 - r.a.x, uhi = r.a.x - (X0 + 7.0f);
                    const float vlo = Y0 - r.a.y, vhi = r.a.y - (Y0 + 7.0f);
                    keep = !(ulo > 0.0f && ulo > ex) && !(uhi > 0.0f && uhi > ex) &&
                           !(vlo > 0.0f && vlo > ey) && !(vhi > 0.0f && vhi > ey);
                }
                g = make_float4(r.a.x, r.a.y, ex, ey);
                q = make_float4(0.0f, 0.0f, r.c.y, r.c.z);
            } else {
                keep = r.b.y > 0.22f;
                if (keep && a.cull)
                    keep = may_touch(r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.z, r.b.w, 2.0f * r.c.x,
                                     X0, X0 + 7, Y0, Y0 + 7);
                g = r.a;
                q = make_float4(r.b.x, logf(0.22f / r.b.y), r.c.y, r.c.z);
            }
        }
        const uint64_t bal = __ballot(keep);
        if (keep) {
            const uint64_t lt = lane == 0 ? 0ull : (~0ull >> (64 - lane));
            const int slot = __popcll(bal & lt);  // compacted in list order
            s_g[slot] = g;
            s_q[slot] = q;
            s_e[slot] = make_float2(r.c.w, __uint_as_float(idx - range.x + 1u));
        }
        const int count = __popcll(bal);
        // one wave: its LDS writes above complete before the reads below are served
        for (int k = 0; k < count; ++k) {
            const float4 sg = s_g[k], sq = s_q[k];
            const float2 se = s_e[k];
            const float dx = sg.x - pfx, dy = sg.y - pfy;
            bool hit;
            float power = 0.0f;
            if (kBill) {
                hit = fabsf(dx) <= sg.z && fabsf(dy) <= sg.w;
            } else {
                power = -0.5f * (sg.z * dx * dx + sq.x * dy * dy) - sg.w * dx * dy;
                hit = !(power > 0.0f) && power > sq.y;
            }
            hit = hit && !done;
            C0 = hit ? sq.z : C0;
            C1 = hit ? sq.w : C1;
            C2 = hit ? se.x : C2;
            hit_pos = hit ? __float_as_uint(se.y) : hit_pos;
            if (kMode == kShadeGaussBall) hit_power = hit ? power : hit_power;
            done = done || hit;
            if ((k & 3) == 3 && __ballot(!done) == 0ull) break;
        }
        if (__ballot(!done) == 0ull) break;
    }

    if (inside) {
        const size_t pid = (size_t)(py - a.y0) * a.W + px;
        const size_t plane = (size_t)a.rows_out * a.W;
        const bool hit = hit_pos != 0u;
        if (kMode == kShadeGaussBall) {
            const float e = exp_core(hit_power);
            C0 *= e, C1 *= e, C2 *= e;
        }
        if (a.final_T) a.final_T[pid] = hit ? 0.0f : 1.0f;
        if (a.n_contrib) a.n_contrib[pid] = hit_pos;
        a.out_color[pid] = hit ? C0 : a.bg[0];
        a.out_color[plane + pid] = hit ? C1 : a.bg[1];
        a.out_color[2 * plane + pid] = hit ? C2 : a.bg[2];
    }
}

}  // namespace

hipError_t gsr_launch_shade(const GsrBlendArgs &a, int shading, hipStream_t s) {
    if (a.rows_tiles == 0 || a.grid_x == 0) return hipSuccess;
    const uint32_t n_tiles = a.grid_x * a.rows_tiles;
    const dim3 grid(xcd_grid(n_tiles));
    if (shading == kShadeBillboard)
        hipLaunchKernelGGL((k_shade_q<kShadeBillboard>), grid, dim3(256), 0, s, a, n_tiles);
    else if (shading == kShadeFlatBall)
        hipLaunchKernelGGL((k_shade_q<kShadeFlatBall>), grid, dim3(256), 0, s, a, n_tiles);
    else if (shading == kShadeGaussBall)
        hipLaunchKernelGGL((k_shade_q<kShadeGaussBall>), grid, dim3(256), 0, s, a, n_tiles);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

uint32_t gsr_blend_order_groups(uint32_t n_tiles) {
    return (n_tiles + kGroupTiles - 1) / kGroupTiles;
}

hipError_t gsr_launch_blend(const GsrBlendArgs &a, hipStream_t s) {
    if (a.rows_tiles == 0 || a.grid_x == 0) return hipSuccess;
    const uint32_t n_tiles = a.grid_x * a.rows_tiles;
    const dim3 grid(xcd_grid(n_tiles));
    if (a.fast && !a.n_contrib)
        hipLaunchKernelGGL((k_blend_q<true, false>), grid, dim3(256), 0, s, a, n_tiles);
    else if (a.fast)
        hipLaunchKernelGGL((k_blend_q<true, true>), grid, dim3(256), 0, s, a, n_tiles);
    else
        hipLaunchKernelGGL((k_blend_q<false, true>), grid, dim3(256), 0, s, a, n_tiles);
    return hipGetLastError();
}

hipError_t gsr_launch_blend_depth(const GsrBlendArgs &a, const GsrDepthArgs &d, hipStream_t s) {
    if (!d.z_bits || (!d.depth_map && !d.inv_depth_map)) return hipErrorInvalidValue;
    if (a.rows_tiles == 0 || a.grid_x == 0) return hipSuccess;
    const uint32_t n_tiles = a.grid_x * a.rows_tiles;
    const dim3 grid(xcd_grid(n_tiles));
    if (a.fast && !a.n_contrib)
        hipLaunchKernelGGL((k_blend_depth_q<true, false>), grid, dim3(256), 0, s, a, n_tiles, d);
    else if (a.fast)
        hipLaunchKernelGGL((k_blend_depth_q<true, true>), grid, dim3(256), 0, s, a, n_tiles, d);
    else
        hipLaunchKernelGGL((k_blend_depth_q<false, true>), grid, dim3(256), 0, s, a, n_tiles, d);
    return hipGetLastError();
}

template <bool kDepth>
static hipError_t launch_surface(const GsrBlendArgs &a, const GsrDepthArgs &d,
                                 const GsrSurfaceArgs &m, uint32_t n_tiles, hipStream_t s) {
    const dim3 grid(xcd_grid(n_tiles));
    if (a.fast && !a.n_contrib)
        hipLaunchKernelGGL((k_blend_surface_q<true, false, kDepth>), grid, dim3(256), 0, s, a,
                           n_tiles, d, m);
    else if (a.fast)
        hipLaunchKernelGGL((k_blend_surface_q<true, true, kDepth>), grid, dim3(256), 0, s, a,
                           n_tiles, d, m);
    else
        hipLaunchKernelGGL((k_blend_surface_q<false, true, kDepth>), grid, dim3(256), 0, s, a,
                           n_tiles, d, m);
    return hipGetLastError();
}

hipError_t gsr_launch_blend_surface(const GsrBlendArgs &a, const GsrDepthArgs &d,
                                    const GsrSurfaceArgs &m, hipStream_t s) {
    if (!d.z_bits || (!m.median_depth && !m.median_id)) return hipErrorInvalidValue;
    if (a.rows_tiles == 0 || a.grid_x == 0) return hipSuccess;
    const uint32_t n_tiles = a.grid_x * a.rows_tiles;
    if (d.depth_map || d.inv_depth_map) return launch_surface<true>(a, d, m, n_tiles, s);
    return launch_surface<false>(a, d, m, n_tiles, s);
}

// The chunk widths of a feature launch: the rest of the channels in the narrowest of 4, 8, 16 that
// holds it, else 16.
static int feature_chunk(int rest) { return rest > 8 ? 16 : rest > 4 ? 8 : 4; }

hipError_t gsr_launch_blend_features(const GsrBlendArgs &a, const float *features, int C,
                                     float *feature_map, hipStream_t s) {
    if (!features || !feature_map || C < 1) return hipErrorInvalidValue;
    if (a.rows_tiles == 0 || a.grid_x == 0) return hipSuccess;
    const uint32_t n_tiles = a.grid_x * a.rows_tiles;
    const dim3 grid(xcd_grid(n_tiles));
    GsrFeatureArgs ft{features, feature_map, C, 0,
                      (reinterpret_cast<uintptr_t>(features) & 15) == 0 && C % 4 == 0};
    for (; ft.c0 < C;) {
        const int w = feature_chunk(C - ft.c0);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(256), 0, s, a, n_tiles, ft);
        };
        if (a.fast) {
            if (w == 16) launch(k_blend_features_q<true, 16>);
            else if (w == 8) launch(k_blend_features_q<true, 8>);
            else launch(k_blend_features_q<true, 4>);
        } else {
            if (w == 16) launch(k_blend_features_q<false, 16>);
            else if (w == 8) launch(k_blend_features_q<false, 8>);
            else launch(k_blend_features_q<false, 4>);
        }
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        ft.c0 += w;
    }
    return hipSuccess;
}
