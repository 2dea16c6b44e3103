// gsr_internal.h -- device-side building blocks shared by the gsr kernels (gfx950 only).
//
// Arithmetic contract: every float expression below is evaluated in exactly the order the
// upstream diff-gaussian-rasterization C++ writes it (left-to-right sums, glm column-major
// mat3 products), with FMA contraction OFF and correctly rounded div/sqrt (HIP defaults).
// That is what makes radii / tiles_touched / sort keys / point lists / ranges bit-identical
// to the CPU oracle (oracle/gsr_oracle.c), which restates the same upstream functions.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>
#include <string>
#include <vector>

#pragma clang fp contract(off)

#define GSR_TILE_X 16
#define GSR_TILE_Y 16

namespace gsr {

// One visible Gaussian as the blend consumes it: 48 B, three 16-B loads, gathered by tile
// lists.  a = {x, y, conic.a, conic.b}; b = {conic.c, opacity, cull_ex, cull_ey}; c = {cull_Lm,
// r, g, b} (cull_*: conservative alpha >= 1/255 region, see preprocess.hip cull_data).
// k_preprocess writes a, b and c.x; k_color writes the colour c.yzw (on the second stream).
struct alignas(16) SplatRecord {
    float4 a, b, c;
};

__device__ __forceinline__ int f2i_sat(float v) {
    // float -> int with CUDA cvt.rzi.s32.f32 semantics: truncate, saturate, NaN -> 0.
    if (!(v == v)) return 0;
    if (v >= 2147483648.0f) return 2147483647;
    if (v <= -2147483648.0f) return (-2147483647 - 1);
    return (int)v;
}

// --- upstream auxiliary.h --------------------------------------------------------------
__device__ __forceinline__ float3 transform_point_4x3(float3 p, const float *M) {
    float3 r;
    r.x = M[0] * p.x + M[4] * p.y + M[8] * p.z + M[12];
    r.y = M[1] * p.x + M[5] * p.y + M[9] * p.z + M[13];
    r.z = M[2] * p.x + M[6] * p.y + M[10] * p.z + M[14];
    return r;
}

__device__ __forceinline__ float4 transform_point_4x4(float3 p, const float *M) {
    float4 r;
    r.x = M[0] * p.x + M[4] * p.y + M[8] * p.z + M[12];
    r.y = M[1] * p.x + M[5] * p.y + M[9] * p.z + M[13];
    r.z = M[2] * p.x + M[6] * p.y + M[10] * p.z + M[14];
    r.w = M[3] * p.x + M[7] * p.y + M[11] * p.z + M[15];
    return r;
}

// upstream ndc2Pix: `((v + 1.0) * S - 1.0) * 0.5` -- the literals are double.
__device__ __forceinline__ float ndc2pix(float v, int S) {
    return (float)((((double)v + 1.0) * (double)S - 1.0) * 0.5);
}

struct Rect {
    uint32_t x0, y0, x1, y1;
};

__device__ __forceinline__ Rect get_rect(float px, float py, int r, uint32_t gx, uint32_t gy) {
    Rect q;
    q.x0 = min(gx, (uint32_t)max(0, f2i_sat((px - r) / GSR_TILE_X)));
    q.y0 = min(gy, (uint32_t)max(0, f2i_sat((py - r) / GSR_TILE_Y)));
    q.x1 = min(gx, (uint32_t)max(0, f2i_sat((px + r + GSR_TILE_X - 1) / GSR_TILE_X)));
    q.y1 = min(gy, (uint32_t)max(0, f2i_sat((py + r + GSR_TILE_Y - 1) / GSR_TILE_Y)));
    return q;
}

// --- glm-style 3x3, column-major m[col][row] -------------------------------------------
struct Mat3 {
    float m[3][3];
};

__device__ __forceinline__ Mat3 mat3_cols(float a0, float a1, float a2, float a3, float a4,
                                          float a5, float a6, float a7, float a8) {
    Mat3 r;
    r.m[0][0] = a0; r.m[0][1] = a1; r.m[0][2] = a2;
    r.m[1][0] = a3; r.m[1][1] = a4; r.m[1][2] = a5;
    r.m[2][0] = a6; r.m[2][1] = a7; r.m[2][2] = a8;
    return r;
}

__device__ __forceinline__ Mat3 mat3_mul(const Mat3 &a, const Mat3 &b) {
    Mat3 r;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            float s = a.m[0][i] * b.m[j][0];
            s = s + a.m[1][i] * b.m[j][1];
            s = s + a.m[2][i] * b.m[j][2];
            r.m[j][i] = s;
        }
    return r;
}

__device__ __forceinline__ Mat3 mat3_transpose(const Mat3 &a) {
    Mat3 r;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int i = 0; i < 3; ++i) r.m[i][j] = a.m[j][i];
    return r;
}

// upstream forward.cu computeCov3D (twin: shaders/gau_vert.glsl:73-93)
__device__ __forceinline__ void compute_cov3d(float3 s, float mod, float4 q, float c[6]) {
    Mat3 S = mat3_cols(1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f);
    S.m[0][0] = mod * s.x;
    S.m[1][1] = mod * s.y;
    S.m[2][2] = mod * s.z;
    const float r = q.x, x = q.y, y = q.z, z = q.w;
    Mat3 R = mat3_cols(1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                       2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                       2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y));
    Mat3 M = mat3_mul(S, R);
    Mat3 Mt = mat3_transpose(M);
    Mat3 Sig = mat3_mul(Mt, M);
    c[0] = Sig.m[0][0];
    c[1] = Sig.m[0][1];
    c[2] = Sig.m[0][2];
    c[3] = Sig.m[1][1];
    c[4] = Sig.m[1][2];
    c[5] = Sig.m[2][2];
}

// upstream forward.cu computeCov2D (twin: shaders/gau_vert.glsl:95-120).  `t` is the
// view-space mean (transformPoint4x3(mean, viewmatrix), already computed by the caller).
// pre (the antialiased preprocess, else NULL): the diagonal before the 0.3 dilation, a' and c'
// ((a' + 0.3f) - 0.3f is not a'); the plain callers' code is what it was.
__device__ __forceinline__ float3 compute_cov2d(float3 t, float fx, float fy, float tanfovx,
                                                float tanfovy, const float c[6], const float *vm,
                                                float *pre = nullptr) {
    const float limx = 1.3f * tanfovx;
    const float limy = 1.3f * tanfovy;
    const float txtz = t.x / t.z;
    const float tytz = t.y / t.z;
    t.x = fminf(limx, fmaxf(-limx, txtz)) * t.z;
    t.y = fminf(limy, fmaxf(-limy, tytz)) * t.z;
    Mat3 J = mat3_cols(fx / t.z, 0.0f, -(fx * t.x) / (t.z * t.z), 0.0f, fy / t.z,
                       -(fy * t.y) / (t.z * t.z), 0.f, 0.f, 0.f);
    Mat3 W = mat3_cols(vm[0], vm[4], vm[8], vm[1], vm[5], vm[9], vm[2], vm[6], vm[10]);
    Mat3 T = mat3_mul(W, J);
    Mat3 Vrk = mat3_cols(c[0], c[1], c[2], c[1], c[3], c[4], c[2], c[4], c[5]);
    Mat3 Tt = mat3_transpose(T);
    Mat3 Vt = mat3_transpose(Vrk);
    Mat3 A = mat3_mul(Tt, Vt);
    Mat3 cov = mat3_mul(A, T);
    if (pre) pre[0] = cov.m[0][0], pre[1] = cov.m[1][1];
    cov.m[0][0] += 0.3f;
    cov.m[1][1] += 0.3f;
    return make_float3(cov.m[0][0], cov.m[0][1], cov.m[1][1]);
}

// Order-preserving float -> uint32 key for a general float sort (negatives, -0 == +0,
// every NaN last): stable radix on these keys == np.argsort(kind='stable').
__device__ __forceinline__ uint32_t float_sort_key(float f) {
    uint32_t u = __float_as_uint(f);
    if (f == 0.0f) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    if (f != f) u = 0xFFFFFFFFu;
    return u;
}

// --- tight binning: the tile rows each column of a splat's rect really reaches ------------
// Upstream pairs a Gaussian with every tile of its 3-sigma square (getRect); at C3 ~43 % of those
// tiles lie outside the ellipse where the splat can reach alpha >= 1/255, and the blend skips them
// there (upstream `alpha < 1/255: continue`).  A Gaussian whose strip rect has w <= kSpanCols
// columns and h <= kSpanRows rows carries a span word: byte c = lo | cnt << 4, the strip rect's
// rows [lo, lo + cnt) that column c of the rect keeps (preprocess.hip col_spans).  Tight binning
// (GSR_OPT_TIGHT_BINNING) emits only those pairs; every tile list keeps its order, so each
// pixel composites exactly the same splats in the same order.  Larger rects keep every tile.
constexpr uint32_t kSpanCols = 8, kSpanRows = 15;
__device__ __forceinline__ bool span_coded(uint2 rect) {
    return (rect.x >> 16) <= kSpanCols && (rect.y >> 16) <= kSpanRows;
}
// Rows [lo, lo + cnt) of column c (< width) of the rect; cols is ignored unless span_coded.
__device__ __forceinline__ void col_span(uint2 rect, uint2 cols, uint32_t c, uint32_t &lo,
                                         uint32_t &cnt) {
    if (span_coded(rect)) {
        const uint32_t b = ((c < 4 ? cols.x : cols.y) >> (8 * (c & 3))) & 0xFFu;
        lo = b & 15u;
        cnt = b >> 4;
    } else {
        lo = 0u;
        cnt = rect.y >> 16;
    }
}

// --- the depth keys' spread (the preprocess blocks' largest / smallest kept key) -------------
// D: the bits in which the kept keys differ (the highest bit where the largest and the smallest
// differ: every key in between shares the bits above it); Dr: the bits of their range
// max - min, which the MSD depth sort buckets (key - min) by.  No kept key: max < min.
struct KeyBits {
    uint32_t D, Dr, min;
};
__device__ __forceinline__ KeyBits key_bits(uint32_t mx, uint32_t mn) {
    KeyBits k{0u, 0u, 0u};
    if (mx >= mn) {
        k.D = mx != mn ? 32u - (uint32_t)__clz(mx ^ mn) : 0u;
        k.Dr = mx != mn ? 32u - (uint32_t)__clz(mx - mn) : 0u;
        k.min = mn;
    }
    return k;
}
// The MSD depth sort's control words (depth_sort.hip): ctl[1] = D, ctl[2] = the MSD pass's
// shift (Dr - 12, or 0: (key - min) >> shift is the 12-bit bucket), ctl[3] = min.
__device__ __forceinline__ void gsr_msd_ctl(const KeyBits &k, uint32_t *ctl) {
    ctl[1] = k.D;
    ctl[2] = k.Dr > 12u ? k.Dr - 12u : 0u;
    ctl[3] = k.min;
}

// --- the blend's exp and its quadrant cull (blend.hip, backward.hip: one arithmetic for the
// composite and its derivative, so both take the same skip decisions) -----------------------
// ocml __ocml_exp_f32 (non-DAZ path) without the final range selects: identical results for
// every finite argument (below about -104 both give 0, above 88.7 both give +inf).
__device__ __forceinline__ float exp_core(float x) {
    const float kLog2eHi = 0x1.715476p+0f;   // 1.44269502
    const float kLog2eLo = 0x1.4ae0bep-26f;  // 1.92596299e-08
    const float ph = x * kLog2eHi;
    const float n = __builtin_rintf(ph);
    const float hi = ph - n;
    float lo = __builtin_fmaf(x, kLog2eHi, -ph);
    lo = __builtin_fmaf(x, kLog2eLo, lo);
    const float e = __builtin_amdgcn_exp2f(hi + lo);
    return __builtin_ldexpf(e, (int)n);
}

// Lower bound of q(u, v) = A u^2 + 2B uv + C v^2 evaluated in float: q minus a bound on its
// rounding error.
__device__ __forceinline__ float q_lower(float A, float B, float C, float u, float v) {
    const float uu = A * u * u, uv = 2.0f * B * u * v, vv = C * v * v;
    return (uu + uv + vv) - 16.0f * 5.96e-8f * (uu + fabsf(uv) + vv);
}

// May the splat reach alpha >= 1/255 at some pixel centre of the box [bx0,bx1] x [by0,by1]?
// False only when provably not (NaN / inf data always answer true).
__device__ __forceinline__ bool may_touch(float x, float y, float A, float B, float C, float ex,
                                          float ey, float twoL, float bx0, float bx1, float by0,
                                          float by1) {
    const float ulo = bx0 - x, uhi = bx1 - x, vlo = by0 - y, vhi = by1 - y;
    if (fmaxf(fmaxf(ulo, -uhi), 0.0f) > ex || fmaxf(fmaxf(vlo, -vhi), 0.0f) > ey) return false;
    if (ulo <= 0.0f && uhi >= 0.0f && vlo <= 0.0f && vhi >= 0.0f) return true;
    // centre outside the box: q is convex, so its minimum over the box lies on an edge whose
    // constraint the centre violates (at the minimiser, the direction to the centre leaves the
    // box through an active face), where it is the 1-D minimum clamped to the edge: at most one
    // vertical and one horizontal edge.  The minimiser's slope -B/C (-B/A) comes from
    // v_rcp_f32 (1 ulp) instead of an IEEE division (~10 VALU): a minimiser a few ulp off
    // raises q there by C * dv^2 ~ 1e-13 * q, far inside q_lower's 16-ulp rounding margin.
    const float su = -B * __builtin_amdgcn_rcpf(C), sv = -B * __builtin_amdgcn_rcpf(A);
    const float ue = ulo > 0.0f ? ulo : uhi, ve = vlo > 0.0f ? vlo : vhi;
    const float lu = q_lower(A, B, C, ue, fminf(fmaxf(su * ue, vlo), vhi));
    const float lv = q_lower(A, B, C, fminf(fmaxf(sv * ve, ulo), uhi), ve);
    const float inf = __builtin_huge_valf();
    const float lb = fminf((ulo > 0.0f || uhi < 0.0f) ? lu : inf,
                           (vlo > 0.0f || vhi < 0.0f) ? lv : inf);
    return !(lb > twoL);
}

// --- wave / block scans (256-thread blocks, wave64) ------------------------------------
__device__ __forceinline__ uint32_t wave_inclusive_scan(uint32_t x) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    return x;
}

// Exclusive scan over a 256-thread block.  s_tmp: 4 words of LDS.  Returns the exclusive
// prefix of `v` and the block total in `total`.  Contains two barriers.
__device__ __forceinline__ uint32_t block256_exclusive_scan(uint32_t v, uint32_t *s_tmp,
                                                            uint32_t &total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const uint32_t inc = wave_inclusive_scan(v);
    if (lane == 63) s_tmp[w] = inc;
    __syncthreads();
    uint32_t pre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = s_tmp[i];
        pre += (i < w) ? t : 0u;
        tot += t;
    }
    __syncthreads();
    total = tot;
    return pre + inc - v;
}

// --- XCD-aware block order for the scattering passes ---------------------------------------
// The hardware deals workgroup b to XCD b % 8.  Here chunks of kXcdChunk consecutive logical
// blocks go to one XCD, the chunks round-robin over the XCDs, so the partial lines that
// neighbouring blocks write into one digit's run meet in one L2 and leave it merged, while the
// XCDs stay balanced (the column pass's depth-ordered blocks shrink with depth) and the live
// blocks of a grid sized for capacity (a device-side count) still come first on every XCD.
// The grid is a multiple of 8 kXcdChunk blocks (xcd_run_grid); speed only, every logical block
// does the same work.  One contiguous run per XCD lost on both counts
// (profiles/r06k_ab_xcd_runs.txt, r06n_ab_xcd_sort_chunk.txt); chunks of 16 gain C3 +2 %, the
// C4 full frame +7 %.
constexpr uint32_t kXcdChunk = 16;
__device__ __forceinline__ uint32_t xcd_run_block(uint32_t b) {
    const uint32_t x = b & 7u, l = b >> 3;
    return ((l / kXcdChunk) * 8u + x) * kXcdChunk + l % kXcdChunk;
}
inline uint32_t xcd_run_grid(int64_t nb) {
    const int64_t m = 8 * (int64_t)kXcdChunk;
    return (uint32_t)((nb + m - 1) / m * m);
}

}  // namespace gsr

// The words a context's kernels store for its host: pinned host memory, device-mapped, eight
// 64-bit words, zero at first (tag 0 never matches a frame; a frame's tag is nonzero).  The
// stores are system-scope atomics and the host reads with acquire loads.  k_publish_K
// (preprocess.hip) stores D, Dr, K_spans and K, then K_tag with release order, which the host
// spins on; the depth sort's pass 0 stores sort_D for the host to count the LSD passes, and the
// MSD local sort stores crowd (depth_sort.hip: both take the address of their one word).
struct GsrHostWords {
    unsigned long long unused;
    unsigned long long crowd;    // the tag of the last frame whose MSD buckets crowded the LDS
    unsigned long long K;        // (Gaussian, strip tile) pairs: upstream's num_rendered
    unsigned long long D;        // the bits in which the kept depth keys differ
    unsigned long long sort_D;   // (frame tag << 32) | D, from the depth sort's pass 0
    unsigned long long K_spans;  // the pair count over the spans (tight binning's list length)
    unsigned long long Dr;       // the bits of the kept depth keys' range (gsr::key_bits)
    unsigned long long K_tag;    // the tag of the frame whose K, D, Dr and K_spans are above
};
static_assert(sizeof(GsrHostWords) == 8 * sizeof(unsigned long long), "eight pinned words");

// ---- host-side launchers (defined in the .hip files, called by api.hip) ------------------
struct GsrPreprocessArgs {
    int64_t P;
    int D, M;
    float scale_modifier;
    const float *means3D, *scales, *rotations, *opacities, *shs, *colors_precomp, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *campos;
    float tanfovx, tanfovy, focal_x, focal_y;
    int W, H;
    uint32_t grid_x, grid_y, row_begin, row_end;
    int prefiltered;
    int sh_vec4, rot_vec4;  // 16-B aligned rows: vector loads allowed
    // workspace outputs
    int32_t *radii;  // nullptr on a strip without radii: strip_skip
    int strip_skip;  // skip Gaussians whose footprint bound misses the strip (preprocess.hip)
    gsr::SplatRecord *records;
    uint32_t *sort_keys;  // depth keys (0xFFFFFFFF: no pair in the strip); values are indices
    uint32_t *block_kept; // optional: per 256-Gaussian block, its count of kept keys
    // per Gaussian: strip-clipped tile rect {x0 | width << 16, strip-local row0 | rows << 16},
    // {0, 0} when it has no pair in the strip (grid dimensions < 2^16, checked by the host)
    uint2 *strip_rect;
    // tight binning (else NULL): per Gaussian {strip rect, span word} (gsr::col_span; the span
    // word only for span-coded rects), {0, 0, 0, 0} without pairs in the strip
    uint4 *strip_rc;
    // per k_preprocess block (ceil(P / 256)): its (Gaussian, strip tile) pair count (low 32
    // bits) and its pair count over the spans (high 32 bits: the same without tight binning),
    // then as many uint2 of the OR / AND of its kept depth keys
    uint64_t *block_pairs;
    GsrHostWords *host_words;    // (the device view)
    uint32_t k_tag;              // nonzero: stored to host_words->K_tag after K
    // frame graphs (api.hip): device words of the context -- [0] the frame's tag, [4..6] the
    // camera position -- which k_preprocess's block 0 stores (k_tag, *campos) for the kernels of
    // a recorded graph, whose arguments cannot change per frame; NULL otherwise
    uint32_t *frame_words;
    // optional debug outputs
    float *depths, *means2D, *conic_opacity, *rgb;
    uint32_t *tiles_touched;
    // gsr_forward_filtered: 1 = the antialiased preprocess (k_preprocess_aa), whose record,
    // cull data, spans and conic_opacity carry the effective opacity; the call's, not the context's
    int antialiasing;
};

// k_preprocess blocks of 256 Gaussians: the count of GsrPreprocessArgs.block_pairs entries and
// of the kept-key OR / AND words after them (the one definition every reader of them uses).
inline int64_t gsr_preprocess_blocks(int64_t P) { return (P + 255) / 256; }
hipError_t gsr_launch_preprocess(const GsrPreprocessArgs &a, hipStream_t s);
// SH -> RGB (or colors_precomp) of every Gaussian with radii > 0 into SplatRecord.c.yzw (+ rgb).
// waves_per_simd (1..7): cap on the colour waves a CU holds at once (0 = no cap).
hipError_t gsr_launch_color(const GsrPreprocessArgs &a, int waves_per_simd, hipStream_t s);
// Once per device (gsr_create): k_color's dynamic LDS limit for those reservations.
hipError_t gsr_color_setup();
// Colour of the Gaussians listed in ids[0 .. *d_n) (the depth sort's compacted kept ids of a
// strip frame), degree-3 16-B-aligned SH and no rgb output only (gsr_color_ids_ok).
bool gsr_color_ids_ok(const GsrPreprocessArgs &a);
hipError_t gsr_launch_color_ids(const GsrPreprocessArgs &a, const uint32_t *ids,
                                const uint32_t *d_n, int waves_per_simd, hipStream_t s);
// K of the frame (sum of the preprocess blocks' pair counts), the pair count over the spans and
// D -> a.host_words (pinned host memory), after the preprocess.  ds_ctl (optional): also the MSD
// depth sort's control words, ctl[1] = D and ctl[2] = its pass's shift (gsr_depth_sort_msd
// with keybits NULL), so the publish runs on the main stream in place of the sort's own
// key-bit reduction.
// d_tag (frame graphs): the tag is read from this device word (k_preprocess's frame_words[0])
// instead of a.k_tag.
hipError_t gsr_launch_count_pairs(const GsrPreprocessArgs &a, hipStream_t s,
                                  uint32_t *ds_ctl = nullptr, const uint32_t *d_tag = nullptr);
hipError_t gsr_launch_mark_visible(const float *means3D, int64_t P, const float *viewmatrix,
                                   uint8_t *visible, hipStream_t s);
hipError_t gsr_launch_view_depth_keys(const float *xyz, int64_t P, float v20, float v21, float v22,
                                      float v23, uint32_t *keys, float *depth_out, hipStream_t s);

// Radix sort of (uint32 key, uint32 value) pairs, stable, LSD over key bits [begin, end) in
// passes of <= 8 bits, starting at pass first_pass of that plan (the per-pair binning's first
// pass runs fused with the duplication).  On return *keys / *vals point at the buffers holding
// the sorted data (either the input pair or the alt pair).  hist needs gsr_radix_hist_words(n)
// words, digit_total 256.
int64_t gsr_radix_hist_words(int64_t n);
hipError_t gsr_radix_sort_pairs(uint32_t **keys, uint32_t **vals, uint32_t **keys_alt,
                                uint32_t **vals_alt, int64_t n, int begin_bit, int end_bit,
                                uint32_t *hist, uint32_t *digit_total, hipStream_t s,
                                int first_pass = 0);
// The same for keys alone (the column-first binning's row pass over packed pair words).
// d_n (frame graphs): the element count is *d_n, read on the device; n is then the capacity
// the grids, the buffers and hist are sized for, and a count above it sorts nothing (the host
// re-renders such a frame, api.hip).
// tile_starts (optional; single-pass sorts only, the column-first binning's row pass): the
// downsweep also writes the strip's tile ranges, from the scanned histogram it ranks by, and a
// one-block kernel behind it the blend's tile-group order (radix_sort.hip).
// ranges[r * gx + c] = {start, end} of strip tile (r, c) in the sorted list, (0, 0) for a tile
// without entries; order: gsr_blend_order_groups(gx * rows) words.  col_starts: the columns'
// starts in the column-sorted input and its length (257 words,
// gsr_launch_col_pairs_scatter).  gx = 0: none.
struct GsrTileStarts {
    const uint32_t *col_starts;
    uint32_t gx, rows;
    uint2 *ranges;
    uint32_t *order;
};
hipError_t gsr_radix_sort_keys(uint32_t **keys, uint32_t **keys_alt, int64_t n, int begin_bit,
                               int end_bit, uint32_t *hist, uint32_t *digit_total, hipStream_t s,
                               const uint32_t *d_n = nullptr,
                               const GsrTileStarts *tile_starts = nullptr);
// k_rs_scan alone: per digit, exclusive scan of hist[d][0..nb) across tiles -> digit_total[d].
hipError_t gsr_launch_digit_scan(uint32_t *hist, int64_t nb, uint32_t *digit_total,
                                 hipStream_t s);

// Radix pass plan: the key bits [begin, end) split into n <= 4 passes of <= 8 bits.
#define GSR_RADIX_MAX_PASSES 4
struct GsrRadixPlan {
    int n;
    int shift[GSR_RADIX_MAX_PASSES];
    int nbits[GSR_RADIX_MAX_PASSES];
    uint32_t mask[GSR_RADIX_MAX_PASSES];
};
GsrRadixPlan gsr_radix_plan(int begin_bit, int end_bit);

// Depth sort (depth_sort.hip): stable sort of n 32-bit keys, values = indices, in passes of
// 12 key bits (pass p: bits [12p, 12p + 12)).  drop: keys 0xFFFFFFFF are dropped; the kept
// count lands in ctl[0] and the bits in which the kept keys differ (D) in ctl[1], both on the
// device after pass 0.  Passes [pass_begin, pass_end) are launched; a pass with 12p >= D exits
// at once and the last needed pass writes the permutation (ids of the kept keys in key order)
// to perm.  A caller that knows D launches gsr_depth_sort_passes(D) passes in total, else all
// three.  pairs_a / pairs_b: n (key, id) pairs each (ping-pong scratch); hist:
// gsr_depth_sort_hist_words(n), digit_total: gsr_depth_sort_digit_words(), ctl:
// gsr_depth_sort_ctl_words(n) words.
int64_t gsr_depth_sort_hist_words(int64_t n);
int64_t gsr_depth_sort_ctl_words(int64_t n);
int gsr_depth_sort_digit_words();
int gsr_depth_sort_passes(uint32_t key_bits);
// host_D (optional, device view of pinned host memory): pass 0 stores (tag << 32) | D there.
hipError_t gsr_depth_sort(const uint32_t *keys, int64_t n, int drop, uint2 *pairs_a,
                          uint2 *pairs_b, uint32_t *perm, uint32_t *hist, uint32_t *digit_total,
                          uint32_t *ctl, int pass_begin, int pass_end, hipStream_t s,
                          unsigned long long *host_D = nullptr, uint32_t tag = 0);
// The frame's sort (no compaction): D from the preprocess blocks' OR / AND of their kept keys
// (keybits: n_keybits uint2, GsrPreprocessArgs.block_pairs after the counts), one global pass
// over the top 12 of the D varying bits (dropping the 0xFFFFFFFF keys), then every bucket sorted
// by the remaining bits in LDS.  Same result, ctl and perm contract as gsr_depth_sort with drop;
// pairs_a holds the bucketed pairs, pairs_b is scratch.  host_D as in gsr_depth_sort.  keybits
// NULL: ctl[1] and ctl[2] are already set (gsr_launch_count_pairs with ds_ctl).  host_crowd
// (optional, device view of pinned host memory): the local sort stores the tag there when its
// buckets of 513-1024 keys crowd the 4096 LDS slots of a group; wide: the 8192-slot local sort.
hipError_t gsr_depth_sort_msd(const uint32_t *keys, int64_t n, const uint2 *keybits,
                              int64_t n_keybits, uint2 *pairs_a, uint2 *pairs_b, uint32_t *perm,
                              uint32_t *hist, uint32_t *digit_total, uint32_t *ctl, hipStream_t s,
                              unsigned long long *host_D = nullptr, uint32_t tag = 0,
                              unsigned long long *host_crowd = nullptr, int wide = 0);
// Compacting front end for sparse key sets (strips): the kept keys of each 256-key block
// (block_kept[b] of them, from the preprocess) are written in order to keys_c, their indices
// to ids_c, and their count to ctl[0]; then the sort runs on those (gsr_depth_sort_compacted,
// same contract as gsr_depth_sort with drop, n the uncompacted upper bound).  block_kept is
// scanned in place.  keys_c / ids_c may be the two halves of pairs_b.  msd: the MSD form on the
// compacted keys instead of the LSD passes (the whole sort in one call, pass_begin 0; keybits as
// in gsr_depth_sort_msd).
hipError_t gsr_depth_sort_compacted(const uint32_t *keys, int64_t n, uint32_t *block_kept,
                                    uint32_t *keys_c, uint32_t *ids_c, uint2 *pairs_a,
                                    uint2 *pairs_b, uint32_t *perm, uint32_t *hist,
                                    uint32_t *digit_total, uint32_t *ctl, int pass_begin,
                                    int pass_end, hipStream_t s,
                                    unsigned long long *host_D = nullptr, uint32_t tag = 0,
                                    uint32_t *ids_copy = nullptr, hipEvent_t compacted = nullptr,
                                    int msd = 0, const uint2 *keybits = nullptr,
                                    int64_t n_keybits = 0);

// Binning: offsets scan over depth-sorted strip tile counts, duplicate into (tile, id)
// pairs, and tile ranges.
int64_t gsr_scan_blocks(int64_t n);
// also writes rect_sorted[e] = strip_rect[perm[e]].  d_n (optional): entries of perm to scan
// (the compacting depth sort's count; n is then only the grid bound).
hipError_t gsr_launch_scan_reduce(const uint32_t *perm, const uint2 *strip_rect, int64_t n,
                                  const uint32_t *d_n, uint32_t *partials, uint2 *rect_sorted,
                                  hipStream_t s);
hipError_t gsr_launch_scan_partials(uint32_t *partials, int64_t nb, uint64_t *total,
                                    hipStream_t s);
// bin[e] (e = depth rank, only for Gaussians with pairs) = {exclusive pair offset, Gaussian
// id, x0 | width << 16, strip-local row0}
hipError_t gsr_launch_scan_down(const uint32_t *perm, const uint2 *rect_sorted,
                                const uint32_t *partials, int64_t n, const uint32_t *d_n,
                                const uint64_t *total, uint4 *bin, uint32_t *chunk_first,
                                hipStream_t s);
int64_t gsr_duplicate_chunks(int64_t K);
// Fused duplicate + first tile-sort radix pass (digit (key >> shift) & (2^nbits - 1)):
// writes the K pairs, stably ordered by that digit, to keys_out / vals_out.  Uses
// chunk_first as written by gsr_launch_scan_down; hist needs gsr_radix_hist_words(K) words.
hipError_t gsr_launch_dup_sort_pass(const uint4 *bin, const uint32_t *chunk_first, int64_t K,
                                    uint32_t gx, int shift, int nbits, uint32_t *hist,
                                    uint32_t *digit_total, uint32_t *keys_out, uint32_t *vals_out,
                                    uint2 *ranges_zero, uint32_t n_ranges, hipStream_t s);
// Column-first pair generation (binning.hip): pass 1 of the tile sort on (Gaussian, column)
// segments of the depth-sorted Gaussians.  hist: gsr_col_blocks(n_max) * 256 words (per group of
// 4 blocks its column totals, per sub-block of every group its offsets within the group).
int64_t gsr_col_blocks(int64_t n);
// Tight binning: strip_rc (GsrPreprocessArgs) instead of strip_rect, and the depth-ordered copy
// goes to rc_sorted instead of rect_sorted (NULL: full rects).
hipError_t gsr_launch_col_pairs_count(const uint32_t *perm, const uint2 *strip_rect,
                                      const uint4 *strip_rc, int64_t n_max, const uint32_t *d_n,
                                      uint2 *rect_sorted, uint4 *rc_sorted, uint32_t *hist,
                                      uint32_t *digit_total, hipStream_t s);
// list_n (frame graphs, else NULL): the list length (the column totals' sum) is stored there
// for the row pass; a list longer than cap is not written (the host re-renders the frame).
// col_starts (257 words): the columns' starts in the list and its length, kept for the tile
// ranges (GsrTileStarts; the row pass overwrites digit_total).
hipError_t gsr_launch_col_pairs_scatter(const uint32_t *perm, const uint2 *rect_sorted,
                                        const uint4 *rc_sorted, int64_t n_max,
                                        const uint32_t *d_n, const uint32_t *hist,
                                        const uint32_t *digit_total, int pack_shift, uint32_t *out,
                                        uint32_t *col_starts, hipStream_t s,
                                        uint32_t cap = 0xFFFFFFFFu,
                                        uint32_t *list_n = nullptr);
hipError_t gsr_launch_digit_scan_n(uint32_t *hist, int64_t nb, uint32_t *digit_total,
                                   const uint32_t *d_n, int64_t tile, hipStream_t s);
// Packed pair lists (column-first binning): ids = packed & mask; tile ids (offset + strip-local
// tile) from the tile ranges.
hipError_t gsr_launch_unpack_ids(const uint32_t *packed, int64_t K, uint32_t mask, uint32_t *out,
                                 hipStream_t s);
hipError_t gsr_launch_fill_tiles(const uint2 *ranges, uint32_t n_tiles, uint32_t offset,
                                 uint32_t *out, hipStream_t s);
hipError_t gsr_launch_ranges(const uint32_t *tile_keys, int64_t K, uint32_t *ranges,
                             hipStream_t s);
// A list without a row pass -- a strip of one tile row (its tiles are the column runs), or an
// empty list (n = 0, d_n NULL: every range (0, 0)) -- gets its ranges and the order from one
// small kernel instead.  n / d_n as in gsr_radix_sort_keys.
hipError_t gsr_launch_tile_runs(int64_t n, const uint32_t *d_n, const GsrTileStarts &ts,
                                hipStream_t s);
// Pair count per tile row of a strip's ranges (gsr_tile_row_pairs).
hipError_t gsr_launch_row_pairs(const uint2 *ranges, uint32_t gx, uint32_t rows, uint32_t *out,
                                hipStream_t s);
hipError_t gsr_launch_globalize_tiles(const uint32_t *local, int64_t K, uint32_t offset,
                                      uint32_t *global, hipStream_t s);

struct GsrBlendArgs {
    const uint2 *ranges;  // strip-local tile ranges
    const uint32_t *point_list;
    const gsr::SplatRecord *records;
    int W, H;
    uint32_t grid_x, row_begin, rows_tiles;
    int y0, rows_out;
    const float *bg;
    float *out_color, *final_T;
    uint32_t *n_contrib;
    int cull;            // 0: no quadrant cull (identical output, tested)
    int fast;            // 1: folded-constant FMA arithmetic + raw v_exp_f32; 0: upstream order
    uint32_t id_mask;    // point_list word -> Gaussian id (packed pair lists; else ~0u)
    const uint32_t *order;  // tile groups heaviest first (GsrTileStarts.order), or nullptr
    // frame graphs: the list length on the device (k_col_scatter) and the capacity the list was
    // binned into; a longer list was not binned, so the blend writes nothing (the host
    // re-renders the frame).  NULL: the host sized the list.
    const uint32_t *list_n;
    uint32_t list_cap;
};
hipError_t gsr_launch_blend(const GsrBlendArgs &a, hipStream_t s);
// gsr_forward_depth's planes (blend.hip k_blend_depth_q): the composite of gsr_launch_blend, which
// also accumulates z and 1 / z under the colour's weights.  z_bits: per Gaussian, the bits of its
// view-space z -- the depth keys (GsrPreprocessArgs.sort_keys), read by the ids of the list; either
// plane may be NULL (not both), [rows_out, W] strip-local like final_T.
struct GsrDepthArgs {
    const uint32_t *z_bits;
    float *depth_map, *inv_depth_map;
};
hipError_t gsr_launch_blend_depth(const GsrBlendArgs &a, const GsrDepthArgs &d, hipStream_t s);
// gsr_forward_surface's planes (blend.hip k_blend_surface_q): the composite of gsr_launch_blend
// (d's planes both NULL) or of gsr_launch_blend_depth, which also notes the splat at which the
// pixel's transmittance crosses 0.5 and writes its Gaussian id and that Gaussian's z (d.z_bits,
// required).  Either plane may be NULL (not both), [rows_out, W] strip-local like final_T.
struct GsrSurfaceArgs {
    float *median_depth;
    int32_t *median_id;
};
hipError_t gsr_launch_blend_surface(const GsrBlendArgs &a, const GsrDepthArgs &d,
                                    const GsrSurfaceArgs &m, hipStream_t s);
// gsr_forward_features' planes (blend.hip k_blend_features_q): launches of their own over the
// lists of `a`, after its blend: per chunk of 16, 8 or 4 channels (the last one padded inside the
// kernel) the composite of gsr_launch_blend with the Gaussians' feature words in the colours'
// place, under the colour's weights in a.fast's arithmetic.  features: [P, C] floats at any 4-byte
// aligned address (float4 gathers where the rows are 16-B aligned, scalar ones otherwise);
// feature_map: [C, rows_out, W], strip-local like out_color.  Of `a` the colour, final_T,
// n_contrib and bg members are not read.  No word beyond C is read or written.
struct GsrFeatureArgs {
    const float *features;
    float *feature_map;
    int C, c0;  // the row length; the launch's first channel
    int vec4;   // set by the launcher: 16-B aligned rows
};
hipError_t gsr_launch_blend_features(const GsrBlendArgs &a, const float *features, int C,
                                     float *feature_map, hipStream_t s);
// The GL backend's geometry shadings in place of the composite (blend.hip k_shade_q): shading =
// GSR_SHADE_BILLBOARD / FLAT_BALL / GAUSS_BALL.  Same arguments; a.fast is not read.
hipError_t gsr_launch_shade(const GsrBlendArgs &a, int shading, hipStream_t s);
// The blend's dispatch order: the groups of 4 row-adjacent tiles (16 quadrant waves, one XCD)
// by descending pair count, so the last waves to start are the short ones.
// (computed with the tile ranges: GsrTileStarts, blend_order.h)
uint32_t gsr_blend_order_groups(uint32_t n_tiles);

// ---- the backward pass (backward.hip; gsr_backward in api.hip) ---------------------------------
// The per-Gaussian 2D gradients the blend's backward sums and the per-Gaussian backward reads: one
// 64-B row per Gaussian, {d/dmean2D x, y (pixels), d/dconic a, b, c, d/dopacity, d/drgb r, g, b,
// 7 pad}, so one splat's nine sums are one contiguous segment of one 64-B atomic request.  With the
// planes (gsr_backward_planes) word 9 is d/dz through the features z and 1 / z, 6 pad.  With the
// absolute gradient (gsr_backward_abs) words 10 and 11 are the sums over pixels of |the pixel's
// addend to word 0| and |... to word 1|, with and without the planes; 4 pad.
constexpr int kGradRow = 16;
struct GsrBlendBwdArgs {
    const uint2 *ranges;  // whole-frame tile ranges
    const uint32_t *point_list;
    const gsr::SplatRecord *records;
    int W, H;
    uint32_t grid_x, n_tiles;
    const float *bg;
    const float *dL_dcolor;  // [3, H, W]
    uint32_t id_mask;
    int cull;
    float *grad2d;  // [P, kGradRow], zeroed by the caller
};
// gsr_backward_strip: the backward on the tile rows [row_begin, row_begin +
// a.n_tiles / a.grid_x) of the frame.  a.ranges are then the strip's (strip-local tiles, the grid
// of the launch), a.H stays the frame's; pixel coordinates stay the frame's (a tile's rows from
// its global tile row) while a.dL_dcolor ([3, rows_out, W]) and the plane gradients ([rows_out, W])
// are strip-local, read at (py - y0) * W + px, as blend.hip writes the forward's strip.  The
// deterministic slot takes the strip-local tile row against the strip-local strip_rect.  Passed to
// the two launchers below it selects the k_blend_bwd*_strip_q instantiations; NULL launches the
// whole-frame kernels, which have no such argument (profiles/backward_strips_resources.txt).
struct GsrStripBwdArgs {
    uint32_t row_begin;
    int y0, rows_out;
};
// gsr_backward_planes (k_blend_bwd_planes_q): the gradients of depth_map, inv_depth_map and
// final_T ([H, W] each, any NULL but not all) beside a.dL_dcolor, which may then be NULL.  z_bits:
// per Gaussian, the bits of its view-space z (the rebuild's depth keys, as GsrDepthArgs).  The
// tenth sum, dL/dz through the features z and 1 / z, goes to word 9 of the Gaussian's row.
struct GsrPlaneBwdArgs {
    const uint32_t *z_bits;
    const float *dL_ddepth_map, *dL_dinv_depth_map, *dL_dfinal_T;
};
// gsr_backward_features (k_blend_bwd_features_q): launches of their own beside the colour / planes
// blend-backward, per chunk of 16, 8 or 4 channels (the forward's rule), over the same lists.
// A launch carries the recursion for its own channels (the start value is 0: no background), adds
// its share of the words 0..5 of a.grad2d (dL/dalpha is linear in the channel set) and the chunk's
// sums gF_c w_i straight into dL_dfeatures[id * C + c] (zeroed by the caller; NULL: not wanted).
// Of `a`, dL_dcolor and bg are not read.  dL_dfeature_map: [C, rows, W], strip-local under `strip`
// like a.dL_dcolor.  No word beyond C is read or written.
hipError_t gsr_launch_blend_bwd_features(const GsrBlendBwdArgs &a, const float *features, int C,
                                         const float *dL_dfeature_map, float *dL_dfeatures,
                                         hipStream_t s, const GsrStripBwdArgs *strip = nullptr);
// gsr_backward_ordered, deterministic (k_blend_bwd_det_q, k_blend_bwd_planes_det_q; DESIGN.md
// 3k): no sum is added to a.grad2d.  In upstream's (untight) lists a Gaussian is listed in exactly
// the tiles of its rect, so every (Gaussian, tile, quadrant) owns a slot,
//   pair = slab[id] + (ty - row0) * w + (tx - x0),   slot = pair * 4 + quad,
// with {x0 | w << 16, row0 | rows << 16} = strip_rect[id] of the whole frame and slab the exclusive
// scan of w * rows in id order (its total is K, the list's length).  The wave stores its kSums
// words (9, or 10 with the planes; two more with the absolute sums of gsr_backward_abs, which come
// last) to sums[slot * kSums ...] and sets marks[slot] = 1; marks
// ([4 K] bytes) is zeroed by the caller, sums ([4 K * kSums] floats) needs no zeroing: a slot
// without its mark is never read.  A staged splat whose tile lies outside its rect, or whose pair
// is not below K, is not stored (it cannot happen with the rebuild's lists).  K < 2^30.
struct GsrDetBwdArgs {
    const uint2 *strip_rect;  // [P], the rebuild's
    const uint64_t *slab;     // [P]
    float *sums;
    uint8_t *marks;
    uint32_t K;
};
// The blend's backward, one of the eight k_blend_bwd*_q: with the planes (p), the deterministic
// slots (d) and a strip, each NULL for without.  hipErrorInvalidValue without a gradient to read
// (a.dL_dcolor NULL and no p), for a p without z_bits or without any of its three gradients, a d
// with a NULL buffer or K >= 2^30, or a strip that does not describe rows of the frame.  An empty
// grid (a.n_tiles == 0) launches nothing and is hipSuccess, whatever the strip; without d it also
// comes before the missing a.dL_dcolor.
// abs (gsr_backward_abs): the eight k_blend_bwd*_abs_q instantiations, which also sum
// the pixels' |v0| and |v1| into words 10 and 11 of the row; a slot of d then holds kSums + 2 words
// (11, or 12 with the planes), the two absolute sums last.
hipError_t gsr_launch_blend_bwd(const GsrBlendBwdArgs &a, const GsrPlaneBwdArgs *p,
                                const GsrDetBwdArgs *d, const GsrStripBwdArgs *strip,
                                hipStream_t s, bool abs = false);
// slab[i] = sum over j < i of w_j * rows_j (strip_rect, 0 for a Gaussian without a rect), 64-bit;
// partials: workspace of gsr_slab_blocks(P) uint64.  P == 0 launches nothing.
int64_t gsr_slab_blocks(int64_t P);
hipError_t gsr_launch_slab_scan(const uint2 *strip_rect, int64_t P, uint64_t *partials,
                                uint64_t *slab, hipStream_t s);
// k_grad_rows_gather: every word of grad2d's P rows from the slots.  A row of 16 lanes per
// Gaussian: lane j adds the marked slots j, j + 16, ... of the Gaussian's 4 w rows slots in that
// order (tile row-major within the rect, then quadrant), each sum from +0.0 in double; the 16 lanes
// are combined by the fixed tree (xor 1, 2, 4, 8) and rounded once.  Words kSums..15 and the rows
// of Gaussians without a rect or a mark are zeros: no memset of grad2d.  The order is a function
// of the rect and the marks alone.  abs: slots of kSums + 2 words, whose last two go to the words
// 10 and 11 by the same sums in the same order.
hipError_t gsr_launch_grad_rows_gather(const GsrDetBwdArgs &d, int64_t P, bool planes,
                                       float *grad2d, hipStream_t s, bool abs = false);
// gsr_backward_abs's output (k_means2d_abs), after the gate on a strip: dL_dmeans2D_abs[i] =
// (0.5 W row[10], 0.5 H row[11], 0) where radii[i] > 0, else (0, 0, 0).  [P, 3], any 4-byte
// alignment.  P == 0 launches nothing.
hipError_t gsr_launch_means2d_abs(const int32_t *radii, const float *grad2d, int64_t P, int W,
                                  int H, float *dL_dmeans2D_abs, hipStream_t s);
// gsr_backward_strip's gate (k_strip_gate): radii[i] = 0 for every Gaussian without a tile in the
// strip (strip_rect[i].x == 0), in place, so that each of the eight k_preprocess_bwd* kernels
// leaves it where it leaves a culled Gaussian: before any arithmetic, +0.0 in every gradient, zeros
// to the camera's sums.  The kernels themselves are the whole frame's.
hipError_t gsr_launch_strip_gate(const uint2 *strip_rect, int64_t P, int32_t *radii,
                                 hipStream_t s);
struct GsrPreprocessBwdArgs {
    int64_t P;
    int D, M;
    float scale_modifier;
    const float *means3D, *scales, *rotations, *shs, *colors_precomp, *cov3D_precomp;
    const float *viewmatrix, *projmatrix, *campos;
    float tanfovx, tanfovy, focal_x, focal_y;
    int W, H;
    int sh_vec4;  // set by the launcher: SH rows (and dL_dsh rows) of 16 coefficients, 16-B aligned
    // of the rebuilt per-Gaussian stage: 0 = culled, every gradient 0 (on a strip also a Gaussian
    // without a tile in it: gsr_launch_strip_gate)
    const int32_t *radii;
    const float *grad2d;   // [P, kGradRow]
    // outputs, each optional (gsr_gradients)
    float *dL_dmeans3D, *dL_dmeans2D, *dL_dopacity, *dL_dcolors, *dL_dconic, *dL_dsh, *dL_dscales,
        *dL_drotations, *dL_dcov3D;
};
// gsr_backward_camera: the sums of the camera's 27 gradient entries over the Gaussians.  partials:
// workspace of kCameraSums x gsr_preprocess_blocks(P) floats, [sum][block], every word written
// before it is read.  The three outputs (device, 16 / 16 / 3 floats, at least one given) are
// written, the entries the forward never reads as 0.  No atomics: the same 2D gradient rows give
// the same bits.
constexpr int kCameraSums = 27;
struct GsrCameraBwdArgs {
    float *partials;
    float *dL_dviewmatrix, *dL_dprojmatrix, *dL_dcampos;
};
// What a per-Gaussian backward adds to the plain one; the three flags pick one of the eight
// k_preprocess_bwd* kernels.
struct GsrPreprocessBwdExtras {
    // the planes' term: also reads word 9 of the rows, adds (vm[2], vm[6], vm[10]) times it to
    // dL_dmeans3D and writes it to dL_ddepths ([P], optional; not read without `planes`)
    bool planes = false;
    float *dL_ddepths = nullptr;
    // NULL, or the camera instantiation, which k_camera_finish follows
    const GsrCameraBwdArgs *camera = nullptr;
    // NULL, or the forward's opacities [P]: the antialiased twin (k_preprocess_bwd*_aa) -- the
    // rows' word 5 is then dL/do_eff of gsr_forward_filtered's effective opacity
    const float *aa_opacities = nullptr;
};
// hipErrorInvalidValue for a camera without partials or without an output; P == 0 launches nothing.
hipError_t gsr_launch_preprocess_bwd(const GsrPreprocessBwdArgs &a,
                                     const GsrPreprocessBwdExtras &x, hipStream_t s);

// ---- the PLY reader's header parser and value conversion (host code, defined in ply_loader.hip;
// shared with the scene reader in ply_writer.hip) ---------------------------------------------
#define GSR_TRY_PLY(expr)             \
    do {                              \
        const int rc_ = (expr);       \
        if (rc_ != GSR_OK) return rc_; \
    } while (0)

namespace gsr_ply {

enum class PType { I8, U8, I16, U16, I32, U32, F32, F64 };

struct Prop {
    std::string name;
    PType type;
    int size;
    int offset;  // within the binary vertex record
};

struct Header {
    enum Format { ASCII, BLE, BBE } format = BLE;
    int64_t count = 0;
    std::vector<Prop> props;
    int stride = 0;
    size_t data_offset = 0;  // first byte of the vertex element
};

// A read-only mapping of the whole file, unmapped by the destructor.
struct Mapped {
    const unsigned char *p = nullptr;
    size_t size = 0;
    ~Mapped();
};

// gsr_set_error(code, "PLY: " + msg).
int fail(int code, const std::string &msg);
int map_file(const char *path, Mapped &m);
// The vertex element's properties, count, stride and first byte; every count and stride of the
// (untrusted) header is bounded by the file size.
int parse_header(const Mapped &m, Header &h);
int find_prop(const Header &h, const std::string &name);
// Properties whose name starts with `prefix`, sorted by their integer suffix.
std::vector<int> prefixed(const Header &h, const std::string &prefix);
// The next whitespace-separated number of an ascii body, parsed as float64 and then taken to the
// property's type as plyfile's text path does; s moves past it.
int ascii_value(const char *&s, const char *end, PType type, double &out);

// A value of a property as double (exact for every PLY scalar type).
inline double read_value(const unsigned char *p, PType t, bool swap) {
    unsigned char b[8];
    int n = 0;
    switch (t) {
        case PType::I8: case PType::U8: n = 1; break;
        case PType::I16: case PType::U16: n = 2; break;
        case PType::I32: case PType::U32: case PType::F32: n = 4; break;
        case PType::F64: n = 8; break;
    }
    for (int i = 0; i < n; ++i) b[i] = swap ? p[n - 1 - i] : p[i];
    switch (t) {
        case PType::I8: { int8_t v; std::memcpy(&v, b, 1); return v; }
        case PType::U8: { uint8_t v; std::memcpy(&v, b, 1); return v; }
        case PType::I16: { int16_t v; std::memcpy(&v, b, 2); return v; }
        case PType::U16: { uint16_t v; std::memcpy(&v, b, 2); return v; }
        case PType::I32: { int32_t v; std::memcpy(&v, b, 4); return v; }
        case PType::U32: { uint32_t v; std::memcpy(&v, b, 4); return v; }
        case PType::F32: { float v; std::memcpy(&v, b, 4); return v; }
        case PType::F64: { double v; std::memcpy(&v, b, 8); return v; }
    }
    return 0.0;
}

// The reference builds xyz / opacity from the property arrays as read (float32 for float
// properties) and the other fields in float64: value as float32 = numpy astype(float32).
inline float as_f32(double v) { return (float)v; }

}  // namespace gsr_ply
