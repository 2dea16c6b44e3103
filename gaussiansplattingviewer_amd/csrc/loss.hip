// loss.hip -- the photometric loss of a fit, fused: L1 + D-SSIM of one [C, H, W] image against a
// target, forward and backward (gsr_image_loss, gsr_image_loss_backward; include/gsr.h states
// the semantics, DESIGN.md §3n the design).  Stateless: no context, no allocation, no atomics.
//
// Both directions are one block of 256 threads per 16 x 64 tile and channel:
//   1. the tile's planes with their 5-pixel halo (26 x 74, out-of-image taps 0.0) go to LDS;
//   2. a horizontal 11-tap pass over the 26 halo rows goes to LDS (forward: the five products
//      x, y, x^2, y^2, xy; backward: the three saved planes).  A thread owns 4 adjacent columns
//      of one row and slides the window over 14 loaded values;
//   3. a vertical pass: a thread owns one column and 4 adjacent rows (14 loaded values per
//      plane), then the per-pixel arithmetic.
// LDS rows are an odd number of words long (75, 65): in pass 2 the lanes of a wave run down the
// rows and in pass 3 along the columns, and either way 32 consecutive lanes then touch 32 banks.
// The forward's two sums leave a block as one float pair (a fixed shuffle tree, then the four
// waves in order); k_loss_finish adds the pairs in a fixed order in double and rounds once.
//
// A window of a frame (gsr_image_loss_window and its backward) runs the same
// bodies: loss_forward, loss_backward and loss_finish below are the kernels' code, and the
// template argument kWin only moves the tile grid to the window's first row, addresses the band
// buffers from their first frame row and keeps rows outside the window out of the sums.  A frame
// kernel passes kWin = false and an unused Rows: what it compiles to does not change.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "gsr.h"

#pragma clang fp contract(off)

int gsr_set_error(int code, const std::string &msg);  // api.hip

namespace {

constexpr int kThreads = 256;
constexpr int kTh = 16, kTw = 64;  // the tile (tests/test_gpu_image_loss.py walks its edges)
constexpr int kR = 5;              // the window's radius: 11 taps
constexpr int kHh = kTh + 2 * kR, kHw = kTw + 2 * kR;  // the tile with its halo, 26 x 74
constexpr int kSin = kHw + 1;                          // 75 words per staged row
constexpr int kSh = kTw + 1;                           // 65 words per row of the horizontal pass
constexpr int kGroups = kTw / 4;                       // column groups of a row in pass 2
constexpr int kSpan = 4 + 2 * kR;                      // values under a 4-wide sliding window

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum: the float32 roundings of the float64 values
__device__ constexpr float kG[11] = {
    0x1.0d956cp-10f, 0x1.f1fe02p-8f, 0x1.26eb18p-5f, 0x1.bff0fep-4f, 0x1.b43c4p-3f, 0x1.10656p-2f,
    0x1.b43c4p-3f,   0x1.bff0fep-4f, 0x1.26eb18p-5f, 0x1.f1fe02p-8f, 0x1.0d956cp-10f};
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct Tile {
    int c, r0, c0;  // channel, first row, first column
};

__device__ __forceinline__ Tile tile_of(uint32_t block, int tiles_x, int tiles_y) {
    const uint32_t t = block / (uint32_t)tiles_x;
    Tile k;
    k.c0 = (int)(block - t * (uint32_t)tiles_x) * kTw;
    k.c = (int)(t / (uint32_t)tiles_y);
    k.r0 = (int)(t - (uint32_t)k.c * (uint32_t)tiles_y) * kTh;
    return k;
}

// What a window adds to a frame call (frame rows throughout; a frame call reads none of it).
struct Rows {
    int row0, Hb;   // the band buffers: their first frame row and their rows
    int lo, hi;     // the rows the call may read: inside the frame AND inside the buffer it stages
    int g0, g1;     // the rows computed; the tile grid starts at g0
    int own0, own1; // the rows summed (forward) / differentiated (backward)
    int64_t NS;     // the plane stride of `saved`: C * (apron rows) * W
};

// kP planes' 26 x 74 halo tiles -> LDS, out-of-image elements 0.0 (rows outside [lo, hi), columns
// outside [0, W); row `row0` is the planes' first).  Every load of a thread (8 per
// plane) is issued before the first LDS store, from an address that is always valid (an
// out-of-image element reads the plane's first word and is replaced by 0.0), so the loads are
// straight-line code and their latencies overlap instead of adding up.
template <int kP>
__device__ __forceinline__ void stage(const float *const (&src)[kP], int lo, int hi, int W, Tile k,
                                      float *const (&dst)[kP], int row0) {
    constexpr int kIter = (kHh * kHw + kThreads - 1) / kThreads;
    float v[kP][kIter];
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int i = threadIdx.x + it * kThreads;
        const int r = i / kHw, cc = i - r * kHw;
        const int gr = k.r0 - kR + r, gc = k.c0 - kR + cc;
        const bool in = i < kHh * kHw && gr >= lo && gr < hi && gc >= 0 && gc < W;
        const int64_t off = in ? (int64_t)(gr - row0) * W + gc : 0;
#pragma unroll
        for (int p = 0; p < kP; ++p) {
            const float t = src[p][off];
            v[p][it] = in ? t : 0.0f;
        }
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int i = threadIdx.x + it * kThreads;
        const int r = i / kHw, cc = i - r * kHw;
        if (i < kHh * kHw) {
#pragma unroll
            for (int p = 0; p < kP; ++p) dst[p][r * kSin + cc] = v[p][it];
        }
    }
}

// The 4 window sums over v[j .. j+10], j = 0..3.
__device__ __forceinline__ void window4(const float (&v)[kSpan], float (&o)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float s = v[j] * kG[0];
#pragma unroll
        for (int t = 1; t < 11; ++t) s = fmaf(v[j + t], kG[t], s);
        o[j] = s;
    }
}

// Pass 3 of one plane: the 4 vertical window sums of column `col`, rows 4 rg .. 4 rg + 3.
__device__ __forceinline__ void vertical4(const float *__restrict__ h, int rg, int col,
                                          float (&o)[4]) {
    float v[kSpan];
#pragma unroll
    for (int t = 0; t < kSpan; ++t) v[t] = h[(4 * rg + t) * kSh + col];
    window4(v, o);
}

// The forward's block.  H: the frame's rows; N = C H W of the frame.  kWin: `image` and `target`
// are band buffers [C, w.Hb, W], the tiles cover rows [w.g0, w.g1), `saved` is [3, C, g1 - g0, W]
// and only rows [w.own0, w.own1) enter the two sums.
template <bool kSave, bool kWin>
__device__ __forceinline__ void loss_forward(const float *__restrict__ image,
                                             const float *__restrict__ target, int H, int W,
                                             int tiles_x, int tiles_y, int64_t N,
                                             float *__restrict__ saved,
                                             float *__restrict__ partial, const Rows &w) {
    __shared__ float sx[kHh * kSin], sy[kHh * kSin];
    __shared__ float sh[5][kHh * kSh];
    __shared__ float red[2][kThreads / 64];
    Tile k = tile_of(blockIdx.x, tiles_x, tiles_y);
    if (kWin) k.r0 += w.g0;
    const int64_t plane = (int64_t)k.c * (kWin ? w.Hb : H) * W;
    const float *const src[2] = {image + plane, target + plane};
    float *const dst[2] = {sx, sy};
    stage<2>(src, kWin ? w.lo : 0, kWin ? w.hi : H, W, k, dst, kWin ? w.row0 : 0);
    __syncthreads();

    for (int item = threadIdx.x; item < kHh * kGroups; item += kThreads) {
        const int cg = item / kHh, r = item - cg * kHh;
        float x[kSpan], y[kSpan], p[kSpan], o[4];
#pragma unroll
        for (int t = 0; t < kSpan; ++t) {
            x[t] = sx[r * kSin + 4 * cg + t];
            y[t] = sy[r * kSin + 4 * cg + t];
        }
        float *out = &sh[0][r * kSh + 4 * cg];
        window4(x, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = o[j];
        window4(y, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[kHh * kSh + j] = o[j];
#pragma unroll
        for (int t = 0; t < kSpan; ++t) p[t] = x[t] * x[t];
        window4(p, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[2 * kHh * kSh + j] = o[j];
#pragma unroll
        for (int t = 0; t < kSpan; ++t) p[t] = y[t] * y[t];
        window4(p, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[3 * kHh * kSh + j] = o[j];
#pragma unroll
        for (int t = 0; t < kSpan; ++t) p[t] = x[t] * y[t];
        window4(p, o);
#pragma unroll
        for (int j = 0; j < 4; ++j) out[4 * kHh * kSh + j] = o[j];
    }
    __syncthreads();

    const int col = threadIdx.x & (kTw - 1), rg = threadIdx.x / kTw;
    float mu1[4], mu2[4], e11[4], e22[4], e12[4];
    vertical4(sh[0], rg, col, mu1);
    vertical4(sh[1], rg, col, mu2);
    vertical4(sh[2], rg, col, e11);
    vertical4(sh[3], rg, col, e22);
    vertical4(sh[4], rg, col, e12);
    float sum_l1 = 0.0f, sum_map = 0.0f;
    const int gc = k.c0 + col;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gr = k.r0 + 4 * rg + j;
        if (gr >= (kWin ? w.g1 : H) || gc >= W) continue;
        const float x = sx[(4 * rg + j + kR) * kSin + col + kR];
        const float y = sy[(4 * rg + j + kR) * kSin + col + kR];
        const float m1 = mu1[j], m2 = mu2[j];
        const float m11 = m1 * m1, m22 = m2 * m2, m12 = m1 * m2;
        const float s1 = e11[j] - m11, s2 = e22[j] - m22, s12 = e12[j] - m12;
        const float A = m11 + m22 + kC1, B = s1 + s2 + kC2;
        const float Cc = 2.0f * m12 + kC1, D = 2.0f * s12 + kC2;
        const float iA = 1.0f / A, iB = 1.0f / B;
        const float iAB = iA * iB;
        const float map = Cc * D * iAB;
        if (!kWin || (gr >= w.own0 && gr < w.own1)) {
            sum_l1 += fabsf(x - y);
            sum_map += map;
        }
        if (kSave) {
            const int64_t NS = kWin ? w.NS : N;
            const int64_t at = kWin ? ((int64_t)k.c * (w.g1 - w.g0) + (gr - w.g0)) * W + gc
                                    : plane + (int64_t)gr * W + gc;
            // 2 mu2 (D - Cc)/(A B) + 2 mu1 map (1/B - 1/A)
            saved[at] = 2.0f * m2 * (D - Cc) * iAB + 2.0f * m1 * map * (iB - iA);
            saved[NS + at] = -(map * iB);
            saved[2 * NS + at] = 2.0f * Cc * iAB;
        }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        sum_l1 += __shfl_down(sum_l1, d, 64);
        sum_map += __shfl_down(sum_map, d, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        red[0][threadIdx.x >> 6] = sum_l1;
        red[1][threadIdx.x >> 6] = sum_map;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[2 * (int64_t)blockIdx.x] = ((red[0][0] + red[0][1]) + red[0][2]) + red[0][3];
        partial[2 * (int64_t)blockIdx.x + 1] = ((red[1][0] + red[1][1]) + red[1][2]) + red[1][3];
    }
}

template <bool kSave>
__global__ void __launch_bounds__(kThreads)
k_loss_forward(const float *__restrict__ image, const float *__restrict__ target, int H, int W,
               int tiles_x, int tiles_y, int64_t N, float *__restrict__ saved,
               float *__restrict__ partial) {
    loss_forward<kSave, false>(image, target, H, W, tiles_x, tiles_y, N, saved, partial, Rows{});
}

template <bool kSave>
__global__ void __launch_bounds__(kThreads)
k_loss_window_forward(const float *__restrict__ image, const float *__restrict__ target, int H,
                      int W, int tiles_x, int tiles_y, int64_t N, float *__restrict__ saved,
                      float *__restrict__ partial, Rows w) {
    loss_forward<kSave, true>(image, target, H, W, tiles_x, tiles_y, N, saved, partial, w);
}

// The blocks' pairs, added in a fixed order in double: thread t takes pairs t, t + 256, ..., then
// a tree over the 256 threads.  values = (loss, l1, ssim), each rounded once.  `whole` is the
// share of the frame's elements the pairs were summed over, n_own / N: 1.0 for a frame.
__device__ __forceinline__ void loss_finish(const float *__restrict__ partial, int blocks, double N,
                                            float lambda, double whole,
                                            float *__restrict__ values) {
    __shared__ double s[2][kThreads];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < blocks; i += kThreads) {
        a += (double)partial[2 * (int64_t)i];
        b += (double)partial[2 * (int64_t)i + 1];
    }
    s[0][threadIdx.x] = a;
    s[1][threadIdx.x] = b;
    __syncthreads();
    for (int d = kThreads / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            s[0][threadIdx.x] += s[0][threadIdx.x + d];
            s[1][threadIdx.x] += s[1][threadIdx.x + d];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double l1 = s[0][0] / N, ssim = s[1][0] / N, w = (double)lambda;
        values[0] = (float)((1.0 - w) * l1 + w * (whole - ssim));
        values[1] = (float)l1;
        values[2] = (float)ssim;
    }
}

__global__ void __launch_bounds__(kThreads)
k_loss_finish(const float *__restrict__ partial, int blocks, double N, float lambda,
              float *__restrict__ values) {
    loss_finish(partial, blocks, N, lambda, 1.0, values);
}

__global__ void __launch_bounds__(kThreads)
k_loss_window_finish(const float *__restrict__ partial, int blocks, double N, float lambda,
                     double whole, float *__restrict__ values) {
    loss_finish(partial, blocks, N, lambda, whole, values);
}

// The backward's block.  kWin: the tiles cover the own rows [w.own0, w.own1); `saved` is the
// window forward's [3, C, w.hi - w.lo, W] over the apron rows [w.lo, w.hi) and is staged from
// there (rows outside it are outside the frame: 0.0); `image` and `target` are the band buffers;
// dL_dimage is [C, own1 - own0, W].  gm and cl are the frame's.
template <bool kWin>
__device__ __forceinline__ void loss_backward(const float *__restrict__ image,
                                              const float *__restrict__ target, int H, int W,
                                              int tiles_x, int tiles_y, int64_t N, float lambda,
                                              const float *__restrict__ saved,
                                              const float *__restrict__ dL_dloss,
                                              float *__restrict__ dL_dimage, const Rows &w) {
    __shared__ float sa[3][kHh * kSin];
    __shared__ float sh[3][kHh * kSh];
    Tile k = tile_of(blockIdx.x, tiles_x, tiles_y);
    if (kWin) k.r0 += w.own0;
    const int64_t plane = (int64_t)k.c * (kWin ? w.Hb : H) * W;
    const int64_t NS = kWin ? w.NS : N;
    const int64_t splane = kWin ? (int64_t)k.c * (w.hi - w.lo) * W : plane;
    const float *const src[3] = {saved + splane, saved + NS + splane, saved + 2 * NS + splane};
    float *const dst[3] = {sa[0], sa[1], sa[2]};
    stage<3>(src, kWin ? w.lo : 0, kWin ? w.hi : H, W, k, dst, kWin ? w.lo : 0);
    // this thread's 4 pixels of image and target, asked for before the passes that hide them
    const int col = threadIdx.x & (kTw - 1), rg = threadIdx.x / kTw;
    const int gc = k.c0 + col;
    float px[4], py[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gr = k.r0 + 4 * rg + j;
        const int64_t at = gr < (kWin ? w.own1 : H) && gc < W
                               ? plane + (int64_t)(kWin ? gr - w.row0 : gr) * W + gc
                               : plane;
        px[j] = image[at];
        py[j] = target[at];
    }
    __syncthreads();

    for (int item = threadIdx.x; item < kHh * kGroups; item += kThreads) {
        const int cg = item / kHh, r = item - cg * kHh;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
            float v[kSpan], o[4];
#pragma unroll
            for (int t = 0; t < kSpan; ++t) v[t] = sa[p][r * kSin + 4 * cg + t];
            window4(v, o);
#pragma unroll
            for (int j = 0; j < 4; ++j) sh[p][r * kSh + 4 * cg + j] = o[j];
        }
    }
    __syncthreads();

    float ca[4], cb[4], cc[4];
    vertical4(sh[0], rg, col, ca);
    vertical4(sh[1], rg, col, cb);
    vertical4(sh[2], rg, col, cc);
    const float gl = dL_dloss ? dL_dloss[0] : 1.0f;
    const float Nf = (float)N;
    const float gm = -(gl * lambda) / Nf;           // the weight of d map
    const float cl = gl * (1.0f - lambda) / Nf;     // the weight of sign(image - target)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int gr = k.r0 + 4 * rg + j;
        if (gr >= (kWin ? w.own1 : H) || gc >= W) continue;
        const int64_t at = kWin ? ((int64_t)k.c * (w.own1 - w.own0) + (gr - w.own0)) * W + gc
                                : plane + (int64_t)gr * W + gc;
        const float x = px[j], y = py[j];
        const float d = x - y;
        const float sg = d > 0.0f ? 1.0f : d < 0.0f ? -1.0f : d == 0.0f ? 0.0f : d;  // NaN stays
        dL_dimage[at] = (gm * ca[j] + 2.0f * x * (gm * cb[j]) + y * (gm * cc[j])) + cl * sg;
    }
}

__global__ void __launch_bounds__(kThreads)
k_loss_backward(const float *__restrict__ image, const float *__restrict__ target, int H, int W,
                int tiles_x, int tiles_y, int64_t N, float lambda,
                const float *__restrict__ saved, const float *__restrict__ dL_dloss,
                float *__restrict__ dL_dimage) {
    loss_backward<false>(image, target, H, W, tiles_x, tiles_y, N, lambda, saved, dL_dloss,
                         dL_dimage, Rows{});
}

__global__ void __launch_bounds__(kThreads)
k_loss_window_backward(const float *__restrict__ image, const float *__restrict__ target, int H,
                       int W, int tiles_x, int tiles_y, int64_t N, float lambda,
                       const float *__restrict__ saved, const float *__restrict__ dL_dloss,
                       float *__restrict__ dL_dimage, Rows w) {
    loss_backward<true>(image, target, H, W, tiles_x, tiles_y, N, lambda, saved, dL_dloss,
                        dL_dimage, w);
}

struct Shape {
    int tiles_x, tiles_y;
    int64_t N, blocks;
};

// The sizes of a call, or false for C, H, W the ABI refuses.
bool shape_of(int32_t C, int32_t H, int32_t W, Shape *s) {
    if (C < 1 || H < 1 || W < 1) return false;
    const int64_t lim = (int64_t)1 << 31, hw = (int64_t)H * W;
    if (hw >= lim || hw * C >= lim) return false;  // (hw < 2^31 first: hw * C then fits)
    s->N = hw * C;
    s->tiles_x = (W + kTw - 1) / kTw;
    s->tiles_y = (H + kTh - 1) / kTh;
    s->blocks = (int64_t)C * s->tiles_x * s->tiles_y;  // <= N
    return true;
}

bool check_inputs(const gsr_image_loss_inputs *in, Shape *s) {
    return in && in->image && in->target && shape_of(in->C, in->H, in->W, s) &&
           in->lambda >= 0.0f && in->lambda <= 1.0f;  // false for NaN
}

constexpr int kHalo = 2 * kR;  // rows of a neighbour a window with `saved` reads: 5 + 5

// A checked window: the forward's and the backward's Rows and grids.
struct Window {
    Rows fwd, bwd;
    int tiles_x, fwd_tiles_y, bwd_tiles_y;
    int64_t N, n_own, fwd_blocks, bwd_blocks, apron_blocks;
};

int tile_rows_of(int rows) { return (rows + kTh - 1) / kTh; }

// False for what the window entries refuse.  `halo`: the rows beyond the own rows the band must
// hold, inside the frame (10 with `saved`, 5 without, 0 for the backward); -1 skips the band's
// pointers and coverage (the workspace size depends on neither).
bool window_of(const gsr_image_loss_inputs *in, const gsr_loss_window *w, int halo, bool save,
               Window *o) {
    if (!in || !w) return false;
    Shape frame;
    if (in->H < 1 || !shape_of(in->C, w->frame_H, in->W, &frame)) return false;
    if (!(in->lambda >= 0.0f && in->lambda <= 1.0f)) return false;
    const int64_t H = w->frame_H;
    if (w->own_begin < 0 || w->own_begin >= w->own_end || w->own_end > H) return false;
    if (w->row0 < 0 || (int64_t)w->row0 + in->H > H) return false;  // the band lies in the frame
    const int own0 = w->own_begin, own1 = w->own_end;
    const auto below = [](int r, int d) { return r > d ? r - d : 0; };
    const auto above = [H](int r, int d) { return (int)(r + (int64_t)d < H ? r + d : H); };
    if (halo >= 0) {
        if (!in->image || !in->target) return false;
        if (w->row0 > below(own0, halo) || w->row0 + in->H < above(own1, halo)) return false;
    }
    const int a0 = below(own0, kR), a1 = above(own1, kR);  // the apron
    o->tiles_x = frame.tiles_x;
    o->N = frame.N;
    o->n_own = (int64_t)in->C * (own1 - own0) * in->W;
    const int64_t NS = (int64_t)in->C * (a1 - a0) * in->W;
    const int g0 = save ? a0 : own0, g1 = save ? a1 : own1;
    o->fwd = Rows{w->row0, in->H, below(g0, kR), above(g1, kR), g0, g1, own0, own1, NS};
    o->bwd = Rows{w->row0, in->H, a0, a1, own0, own1, own0, own1, NS};
    o->fwd_tiles_y = tile_rows_of(g1 - g0);
    o->bwd_tiles_y = tile_rows_of(own1 - own0);
    o->fwd_blocks = (int64_t)in->C * o->tiles_x * o->fwd_tiles_y;
    o->bwd_blocks = (int64_t)in->C * o->tiles_x * o->bwd_tiles_y;
    o->apron_blocks = (int64_t)in->C * o->tiles_x * tile_rows_of(a1 - a0);
    return true;
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return gsr_set_error(GSR_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return GSR_OK;
}

}  // namespace

extern "C" {

int64_t gsr_image_loss_workspace(int32_t C, int32_t H, int32_t W) {
    Shape s;
    if (!shape_of(C, H, W, &s))
        return gsr_set_error(GSR_E_INVALID, "gsr_image_loss_workspace: bad sizes");
    return s.blocks * 2 * (int64_t)sizeof(float);
}

int gsr_image_loss(const gsr_image_loss_inputs *in, float *values, float *saved, void *workspace,
                   void *stream) {
    Shape s;
    if (!check_inputs(in, &s) || !values || !workspace)
        return gsr_set_error(GSR_E_INVALID, "gsr_image_loss: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *partial = static_cast<float *>(workspace);
    if (saved)
        hipLaunchKernelGGL(k_loss_forward<true>, dim3((uint32_t)s.blocks), dim3(kThreads), 0, st,
                           in->image, in->target, in->H, in->W, s.tiles_x, s.tiles_y, s.N, saved,
                           partial);
    else
        hipLaunchKernelGGL(k_loss_forward<false>, dim3((uint32_t)s.blocks), dim3(kThreads), 0, st,
                           in->image, in->target, in->H, in->W, s.tiles_x, s.tiles_y, s.N, saved,
                           partial);
    int rc = launched("image loss forward");
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(kThreads), 0, st, partial, (int)s.blocks,
                       (double)s.N, in->lambda, values);
    return launched("image loss finish");
}

int gsr_image_loss_backward(const gsr_image_loss_inputs *in, const float *saved,
                            const float *dL_dloss, float *dL_dimage, void *stream) {
    Shape s;
    if (!check_inputs(in, &s) || !saved || !dL_dimage)
        return gsr_set_error(GSR_E_INVALID, "gsr_image_loss_backward: bad arguments");
    hipLaunchKernelGGL(k_loss_backward, dim3((uint32_t)s.blocks), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), in->image, in->target, in->H, in->W,
                       s.tiles_x, s.tiles_y, s.N, in->lambda, saved, dL_dloss, dL_dimage);
    return launched("image loss backward");
}

int64_t gsr_image_loss_window_workspace(const gsr_image_loss_inputs *in,
                                        const gsr_loss_window *w) {
    Window win;
    if (!window_of(in, w, -1, true, &win))
        return gsr_set_error(GSR_E_INVALID, "gsr_image_loss_window_workspace: bad arguments");
    return win.apron_blocks * 2 * (int64_t)sizeof(float);  // the grid with `saved`, the larger
}

int gsr_image_loss_window(const gsr_image_loss_inputs *in, const gsr_loss_window *w,
                          float *values, float *saved, void *workspace, void *stream) {
    Window win;
    if (!values || !workspace || !window_of(in, w, saved ? kHalo : kR, saved != nullptr, &win))
        return gsr_set_error(GSR_E_INVALID, "gsr_image_loss_window: bad arguments");
    hipStream_t st = static_cast<hipStream_t>(stream);
    float *partial = static_cast<float *>(workspace);
    if (saved)
        hipLaunchKernelGGL(k_loss_window_forward<true>, dim3((uint32_t)win.fwd_blocks),
                           dim3(kThreads), 0, st, in->image, in->target, w->frame_H, in->W,
                           win.tiles_x, win.fwd_tiles_y, win.N, saved, partial, win.fwd);
    else
        hipLaunchKernelGGL(k_loss_window_forward<false>, dim3((uint32_t)win.fwd_blocks),
                           dim3(kThreads), 0, st, in->image, in->target, w->frame_H, in->W,
                           win.tiles_x, win.fwd_tiles_y, win.N, saved, partial, win.fwd);
    int rc = launched("image loss window forward");
    if (rc != GSR_OK) return rc;
    hipLaunchKernelGGL(k_loss_window_finish, dim3(1), dim3(kThreads), 0, st, partial,
                       (int)win.fwd_blocks, (double)win.N, in->lambda,
                       (double)win.n_own / (double)win.N, values);
    return launched("image loss window finish");
}

int gsr_image_loss_window_backward(const gsr_image_loss_inputs *in, const gsr_loss_window *w,
                                   const float *saved, const float *dL_dloss, float *dL_dimage,
                                   void *stream) {
    Window win;
    if (!saved || !dL_dimage || !window_of(in, w, 0, true, &win))
        return gsr_set_error(GSR_E_INVALID, "gsr_image_loss_window_backward: bad arguments");
    hipLaunchKernelGGL(k_loss_window_backward, dim3((uint32_t)win.bwd_blocks), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), in->image, in->target, w->frame_H, in->W,
                       win.tiles_x, win.bwd_tiles_y, win.N, in->lambda, saved, dL_dloss,
                       dL_dimage, win.bwd);
    return launched("image loss window backward");
}

}  // extern "C"
