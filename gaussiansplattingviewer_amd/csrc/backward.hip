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
#include "gsr_internal.h"

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
struct BwdSplat {
    float4 g, q;
    float2 e;
};

constexpr int kSums = 9;  // per (splat, quadrant): the words 0..8 of a gradient row

__global__ __launch_bounds__(256) void k_blend_bwd_q(const GsrBlendBwdArgs a) {
    __shared__ BwdSplat s_spl_q[4][64];
    __shared__ uint32_t s_id_q[4][64];
    __shared__ float s_red_q[4][64 * kSums];

    const uint32_t tile = blockIdx.x;
    if (tile >= a.n_tiles) return;
    const uint32_t quad = threadIdx.x >> 6;
    const int lane = threadIdx.x & 63;
    BwdSplat *const s_spl = s_spl_q[quad];
    uint32_t *const s_id = s_id_q[quad];
    float *const s_red = s_red_q[quad];
    const uint32_t tx = tile % a.grid_x, ty = tile / a.grid_x;
    const int qx0 = (int)tx * GSR_TILE_X + (int)(quad & 1u) * 8;
    const int qy0 = (int)ty * GSR_TILE_Y + (int)(quad >> 1) * 8;
    const int px = qx0 + (lane & 7), py = qy0 + (lane >> 3);
    const bool inside = px < a.W && py < a.H;
    const float pfx = (float)px, pfy = (float)py;
    const float X0 = (float)qx0, Y0 = (float)qy0;
    const uint2 range = a.ranges[tile];
    if (__ballot(inside) == 0ull || range.x >= range.y) return;

    // Stages chunk `start` (the forward's gather, cull and in-order compaction); returns the
    // number of staged splats.
    auto stage = [&](uint32_t start) {
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
        }
        return __popcll(bal);
    };

    // ---- front to back: the forward's decisions (blend.hip, the exact form) -------------------
    float T = inside ? 1.0f : -1.0f;  // done carried in the sign, as the forward
    uint32_t last = 0u;               // list position + 1 of the last splat the pixel composited
    uint32_t chunks = 0u;             // chunks the forward walked
    for (uint32_t start = range.x; start < range.y; start += 64) {
        ++chunks;
        const int count = stage(start);
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
    const size_t plane = (size_t)a.H * a.W, pid = (size_t)(inside ? py : 0) * a.W + (inside ? px : 0);
    const float g0 = inside ? a.dL_dcolor[pid] : 0.0f;
    const float g1 = inside ? a.dL_dcolor[plane + pid] : 0.0f;
    const float g2 = inside ? a.dL_dcolor[2 * plane + pid] : 0.0f;
    float Tc = fabsf(T);
    float rr = g0 * a.bg[0] + g1 * a.bg[1] + g2 * a.bg[2];
    for (uint32_t c = chunks; c-- > 0u;) {
        const int count = stage(range.x + 64u * c);
        // groups of 16 slots, back to front: lane 16 r + j keeps row r's share of the nine sums
        // of the splat in slot 16 kg + j
        for (int kg = (count - 1) >> 4; kg >= 0; --kg) {
            const int k_lo = 16 * kg, k_hi = min(count, k_lo + 16);
            float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f, s4 = 0.f, s5 = 0.f, s6 = 0.f, s7 = 0.f,
                  s8 = 0.f;
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
                const float gc = g0 * sp.q.z + g1 * sp.q.w + g2 * sp.e.x;
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
            }
            if (touched == 0u) continue;
            // slot-major in LDS, the four rows of a slot side by side; then word t of the group's
            // slots x 9 goes to word t % 9 of the row of slot t / 9: consecutive lanes add to
            // consecutive words
            float *mine9 = s_red + ((lane & 15) * 4 + (lane >> 4)) * kSums;
            mine9[0] = s0, mine9[1] = s1, mine9[2] = s2, mine9[3] = s3, mine9[4] = s4;
            mine9[5] = s5, mine9[6] = s6, mine9[7] = s7, mine9[8] = s8;
            const int n = (k_hi - k_lo) * kSums;
            for (int t = lane; t < n; t += 64) {
                const int slot = t / kSums, word = t - slot * kSums;
                if ((touched >> slot) & 1u) {
                    const float *q4 = s_red + slot * 4 * kSums + word;
                    const float sum = (q4[0] + q4[kSums]) + (q4[2 * kSums] + q4[3 * kSums]);
                    atomicAdd(&a.grad2d[(size_t)s_id[k_lo + slot] * kGradRow + word], sum);
                }
            }
        }
    }
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

__global__ __launch_bounds__(256) void k_preprocess_bwd(const GsrPreprocessBwdArgs a) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= a.P) return;
    float *const sh_out = a.dL_dsh ? a.dL_dsh + idx * (int64_t)a.M * 3 : nullptr;
    if (a.radii[idx] <= 0) {  // culled by the forward: exact zeros
        store3(a.dL_dmeans3D, idx, 0.f, 0.f, 0.f);
        store3(a.dL_dmeans2D, idx, 0.f, 0.f, 0.f);
        if (a.dL_dopacity) a.dL_dopacity[idx] = 0.f;
        store3(a.dL_dcolors, idx, 0.f, 0.f, 0.f);
        store3(a.dL_dconic, idx, 0.f, 0.f, 0.f);
        store3(a.dL_dscales, idx, 0.f, 0.f, 0.f);
        if (a.dL_drotations)
            for (int i = 0; i < 4; ++i) a.dL_drotations[4 * idx + i] = 0.f;
        if (a.dL_dcov3D)
            for (int i = 0; i < 6; ++i) a.dL_dcov3D[6 * idx + i] = 0.f;
        if (sh_out && a.sh_vec4) {
            for (int i = 0; i < 12; ++i)
                reinterpret_cast<float4 *>(sh_out)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        } else if (sh_out) {
            for (int i = 0; i < 3 * a.M; ++i) sh_out[i] = 0.f;
        }
        return;
    }
    const float *gr = a.grad2d + idx * kGradRow;
    const float gmx = gr[0], gmy = gr[1], gca = gr[2], gcb = gr[3], gcc = gr[4], gop = gr[5];
    const float grgb[3] = {gr[6], gr[7], gr[8]};
    // upstream's units: the gradient with respect to an offset added to the NDC centre
    const float gnx = gmx * (0.5f * (float)a.W), gny = gmy * (0.5f * (float)a.H);
    store3(a.dL_dmeans2D, idx, gnx, gny, 0.f);
    if (a.dL_dopacity) a.dL_dopacity[idx] = gop;
    store3(a.dL_dcolors, idx, grgb[0], grgb[1], grgb[2]);
    store3(a.dL_dconic, idx, gca, gcb, gcc);

    const float *vm = a.viewmatrix, *pm = a.projmatrix;
    const float3 p = make_float3(a.means3D[3 * idx], a.means3D[3 * idx + 1], a.means3D[3 * idx + 2]);
    float dpx = 0.f, dpy = 0.f, dpz = 0.f;  // dL/dmeans3D

    // ---- the projective divide: ndc = hom.xy / (hom.w + 1e-7) --------------------------------
    {
        const float4 h = transform_point_4x4(p, pm);
        const float pw = 1.0f / (h.w + 0.0000001f);
        const float dhx = gnx * pw, dhy = gny * pw;
        const float dhw = -(gnx * h.x + gny * h.y) * pw * pw;
        dpx += pm[0] * dhx + pm[1] * dhy + pm[3] * dhw;
        dpy += pm[4] * dhx + pm[5] * dhy + pm[7] * dhw;
        dpz += pm[8] * dhx + pm[9] * dhy + pm[11] * dhw;
    }

    // ---- the colour: rgb = max(sum_b basis_b(dir) sh_b + 0.5, 0), dir = (p - campos) / len -----
    if (a.shs) {
        const float *sh = a.shs + idx * (int64_t)a.M * 3;
        const int ncoef = (a.D + 1) * (a.D + 1);
        float dx = p.x - a.campos[0], dy = p.y - a.campos[1], dz = p.z - a.campos[2];
        const float len = sqrtf(dx * dx + dy * dy + dz * dz);
        dx = dx / len, dy = dy / len, dz = dz / len;
        float b[16], bx[16], by[16], bz[16];
        sh_basis(dx, dy, dz, b, bx, by, bz);
        // the coefficients of the active degree (the others read as 0), kept in registers; rows
        // of 16 coefficients at 16-B aligned pointers move as 12 float4 (a.sh_vec4), in and out
        float c[48];
        const int nflt = 3 * ncoef;
        if (a.sh_vec4) {
            const float4 *v = reinterpret_cast<const float4 *>(sh);
            float4 rowv[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) rowv[i] = v[i];
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                c[4 * i] = 4 * i < nflt ? rowv[i].x : 0.f;
                c[4 * i + 1] = 4 * i + 1 < nflt ? rowv[i].y : 0.f;
                c[4 * i + 2] = 4 * i + 2 < nflt ? rowv[i].z : 0.f;
                c[4 * i + 3] = 4 * i + 3 < nflt ? rowv[i].w : 0.f;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 48; ++i) c[i] = i < nflt ? sh[i] : 0.f;
        }
        float val[3] = {0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 16; ++k)
            if (k < ncoef)
                for (int ch = 0; ch < 3; ++ch) val[ch] += b[k] * c[3 * k + ch];
        float G[3];  // max(v + 0.5, 0) passes nothing on its flat side
        for (int ch = 0; ch < 3; ++ch) G[ch] = (val[ch] + 0.5f < 0.0f) ? 0.0f : grgb[ch];
        float ddx = 0.f, ddy = 0.f, ddz = 0.f;  // dL/ddir
        float o[48];                            // dL/dsh: 0 above the active degree
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const bool on = k < ncoef;
            if (on) {
                const float m = G[0] * c[3 * k] + G[1] * c[3 * k + 1] + G[2] * c[3 * k + 2];
                ddx += bx[k] * m, ddy += by[k] * m, ddz += bz[k] * m;
            }
            for (int ch = 0; ch < 3; ++ch) o[3 * k + ch] = on ? b[k] * G[ch] : 0.f;
        }
        if (sh_out) {
            if (a.sh_vec4) {
                float4 *w = reinterpret_cast<float4 *>(sh_out);
#pragma unroll
                for (int i = 0; i < 12; ++i)
                    w[i] = make_float4(o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]);
            } else {
#pragma unroll
                for (int i = 0; i < 48; ++i)
                    if (i < 3 * a.M) sh_out[i] = o[i];
                for (int i = 48; i < 3 * a.M; ++i) sh_out[i] = 0.f;
            }
        }
        // dir = d / |d|: (I - dir dir^T) / len
        const float dot = dx * ddx + dy * ddy + dz * ddz;
        dpx += (ddx - dx * dot) / len;
        dpy += (ddy - dy * dot) / len;
        dpz += (ddz - dz * dot) / len;
    } else if (sh_out) {
        for (int i = 0; i < 3 * a.M; ++i) sh_out[i] = 0.f;
    }

    // ---- the 3D covariance --------------------------------------------------------------------
    float c6[6];
    float3 sc = make_float3(0.f, 0.f, 0.f);
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (a.cov3D_precomp) {
        for (int i = 0; i < 6; ++i) c6[i] = a.cov3D_precomp[6 * idx + i];
    } else {
        sc = make_float3(a.scales[3 * idx], a.scales[3 * idx + 1], a.scales[3 * idx + 2]);
        q = make_float4(a.rotations[4 * idx], a.rotations[4 * idx + 1], a.rotations[4 * idx + 2],
                        a.rotations[4 * idx + 3]);
        compute_cov3d(sc, a.scale_modifier, q, c6);
    }

    // ---- the conic: (c, -b, a) / det of cov2 = A V A^T + 0.3 I, A = J R (2 x 3) ----------------
    const float3 t = transform_point_4x3(p, vm);
    const float limx = 1.3f * a.tanfovx, limy = 1.3f * a.tanfovy;
    const float txtz = t.x / t.z, tytz = t.y / t.z;
    const float cx = fminf(limx, fmaxf(-limx, txtz)), cy = fminf(limy, fmaxf(-limy, tytz));
    const bool clx = cx != txtz, cly = cy != tytz;  // on the clamp's flat side
    const float tx = cx * t.z, ty = cy * t.z, tz = t.z;
    const float fx = a.focal_x, fy = a.focal_y;
    const float tz2 = tz * tz;
    const float J00 = fx / tz, J02 = -(fx * tx) / tz2, J11 = fy / tz, J12 = -(fy * ty) / tz2;
    // R[r][c] = vm[4 c + r] (the view rotation); A = J R
    float A0[3], A1[3];
    for (int c = 0; c < 3; ++c) {
        A0[c] = J00 * vm[4 * c] + J02 * vm[4 * c + 2];
        A1[c] = J11 * vm[4 * c + 1] + J12 * vm[4 * c + 2];
    }
    const float V[3][3] = {{c6[0], c6[1], c6[2]}, {c6[1], c6[3], c6[4]}, {c6[2], c6[4], c6[5]}};
    float VA0[3], VA1[3];  // V A^T
    for (int i = 0; i < 3; ++i) {
        VA0[i] = V[i][0] * A0[0] + V[i][1] * A0[1] + V[i][2] * A0[2];
        VA1[i] = V[i][0] * A1[0] + V[i][1] * A1[1] + V[i][2] * A1[2];
    }
    const float ca = A0[0] * VA0[0] + A0[1] * VA0[1] + A0[2] * VA0[2] + 0.3f;
    const float cb = A0[0] * VA1[0] + A0[1] * VA1[1] + A0[2] * VA1[2];
    const float cc = A1[0] * VA1[0] + A1[1] * VA1[1] + A1[2] * VA1[2] + 0.3f;
    const float det = ca * cc - cb * cb;
    const float id2 = 1.0f / (det * det);
    // conic = (cc, -cb, ca) / det, det - ca cc = -cb^2
    const float dca = (-cc * cc * gca + cb * cc * gcb - cb * cb * gcc) * id2;
    const float dcc = (-cb * cb * gca + ca * cb * gcb - ca * ca * gcc) * id2;
    const float dcb = (2.0f * cb * cc * gca - (ca * cc + cb * cb) * gcb + 2.0f * ca * cb * gcc) * id2;
    const float hb = 0.5f * dcb;  // each off-diagonal of the symmetric dL/dcov2
    // dL/dV = A^T G2 A (an off-diagonal of V stands for two entries: twice in dL/dcov3D)
    float GA0[3], GA1[3];  // G2 A
    for (int c = 0; c < 3; ++c) {
        GA0[c] = dca * A0[c] + hb * A1[c];
        GA1[c] = hb * A0[c] + dcc * A1[c];
    }
    float dV[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) dV[i][j] = A0[i] * GA0[j] + A1[i] * GA1[j];
    const float d6[6] = {dV[0][0], 2.0f * dV[0][1], 2.0f * dV[0][2], dV[1][1], 2.0f * dV[1][2],
                         dV[2][2]};
    if (a.dL_dcov3D)
        for (int i = 0; i < 6; ++i) a.dL_dcov3D[6 * idx + i] = d6[i];
    // dL/dA = 2 G2 A V, dL/dJ = dL/dA R^T
    float dA0[3], dA1[3];
    for (int c = 0; c < 3; ++c) {
        dA0[c] = 2.0f * (dca * VA0[c] + hb * VA1[c]);
        dA1[c] = 2.0f * (hb * VA0[c] + dcc * VA1[c]);
    }
    const float dJ00 = dA0[0] * vm[0] + dA0[1] * vm[4] + dA0[2] * vm[8];
    const float dJ02 = dA0[0] * vm[2] + dA0[1] * vm[6] + dA0[2] * vm[10];
    const float dJ11 = dA1[0] * vm[1] + dA1[1] * vm[5] + dA1[2] * vm[9];
    const float dJ12 = dA1[0] * vm[2] + dA1[1] * vm[6] + dA1[2] * vm[10];
    const float tz3 = tz2 * tz;
    float dtz = -fx / tz2 * dJ00 - fy / tz2 * dJ11 + 2.0f * fx * tx / tz3 * dJ02 +
                2.0f * fy * ty / tz3 * dJ12;
    const float dtxc = -fx / tz2 * dJ02, dtyc = -fy / tz2 * dJ12;  // d/d(clamped t.x, t.y)
    // t.x' = clamp(t.x / t.z) t.z, as written: (t.x / t.z) t.z inside (d/dt.x = 1, d/dt.z = 0),
    // +-lim t.z on the flat side (d/dt.x = 0, d/dt.z = +-lim)
    const float dtx = clx ? 0.0f : dtxc, dty = cly ? 0.0f : dtyc;
    dtz += (clx ? cx * dtxc : 0.0f) + (cly ? cy * dtyc : 0.0f);
    dpx += vm[0] * dtx + vm[1] * dty + vm[2] * dtz;
    dpy += vm[4] * dtx + vm[5] * dty + vm[6] * dtz;
    dpz += vm[8] * dtx + vm[9] * dty + vm[10] * dtz;
    store3(a.dL_dmeans3D, idx, dpx, dpy, dpz);

    // ---- Sigma = N N^T, N = Rq diag(mod s) (the rotation as given, not renormalised) ------------
    if (a.cov3D_precomp) {
        store3(a.dL_dscales, idx, 0.f, 0.f, 0.f);
        if (a.dL_drotations)
            for (int i = 0; i < 4; ++i) a.dL_drotations[4 * idx + i] = 0.f;
        return;
    }
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    const float Rq[3][3] = {
        {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y)},
        {2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x)},
        {2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)}};
    const float sm[3] = {a.scale_modifier * sc.x, a.scale_modifier * sc.y, a.scale_modifier * sc.z};
    float ds[3], D[3][3];  // dL/ds, dL/dRq
    for (int j = 0; j < 3; ++j) {
        ds[j] = 0.f;
        for (int i = 0; i < 3; ++i) {
            // dL/dN[i][j] = 2 (dV N)[i][j], N[k][j] = Rq[k][j] sm[j]
            const float dN = 2.0f * sm[j] *
                             (dV[i][0] * Rq[0][j] + dV[i][1] * Rq[1][j] + dV[i][2] * Rq[2][j]);
            ds[j] += dN * Rq[i][j];
            D[i][j] = dN * sm[j];
        }
        ds[j] *= a.scale_modifier;
    }
    store3(a.dL_dscales, idx, ds[0], ds[1], ds[2]);
    if (a.dL_drotations) {
        float *o = a.dL_drotations + 4 * idx;
        o[0] = 2.f * (-z * D[0][1] + y * D[0][2] + z * D[1][0] - x * D[1][2] - y * D[2][0] +
                      x * D[2][1]);
        o[1] = 2.f * (y * D[0][1] + z * D[0][2] + y * D[1][0] - 2.f * x * D[1][1] - r * D[1][2] +
                      z * D[2][0] + r * D[2][1] - 2.f * x * D[2][2]);
        o[2] = 2.f * (-2.f * y * D[0][0] + x * D[0][1] + r * D[0][2] + x * D[1][0] + z * D[1][2] -
                      r * D[2][0] + z * D[2][1] - 2.f * y * D[2][2]);
        o[3] = 2.f * (-2.f * z * D[0][0] - r * D[0][1] + x * D[0][2] + r * D[1][0] -
                      2.f * z * D[1][1] + y * D[1][2] + x * D[2][0] + y * D[2][1]);
    }
}

}  // namespace

hipError_t gsr_launch_blend_bwd(const GsrBlendBwdArgs &a, hipStream_t s) {
    if (a.n_tiles == 0) return hipSuccess;
    hipLaunchKernelGGL(k_blend_bwd_q, dim3(a.n_tiles), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t gsr_launch_preprocess_bwd(const GsrPreprocessBwdArgs &args, hipStream_t s) {
    if (args.P == 0) return hipSuccess;
    GsrPreprocessBwdArgs a = args;
    a.sh_vec4 = a.shs && a.M == 16 && (reinterpret_cast<uintptr_t>(a.shs) & 15) == 0 &&
                (reinterpret_cast<uintptr_t>(a.dL_dsh) & 15) == 0;
    hipLaunchKernelGGL(k_preprocess_bwd, dim3((unsigned)gsr_preprocess_blocks(a.P)), dim3(256), 0,
                       s, a);
    return hipGetLastError();
}
