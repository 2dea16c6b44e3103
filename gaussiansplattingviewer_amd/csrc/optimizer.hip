// optimizer.hip -- the last two device steps of a fit iteration: the visibility-masked ("sparse")
// Adam update of up to GSR_MAX_PARAM_GROUPS parameter tensors in ONE launch (gsr_adam_step), and
// the densification statistics (gsr_densify_stats).  include/gsr.h states the semantics,
// DESIGN.md §3o the design.  Stateless: no context, no allocation, no atomics, no LDS.
//
// k_adam: the group table travels by value in the kernel arguments.  Every group owns a run of
// blocks (first_block, computed on the host), and a block finds its group by walking the table
// with its block index -- uniform, scalar code.  Within a group a block owns either
//   * kRowElems / M whole rows (M <= kRowElems), whose elements are contiguous in memory, so
//     element l of the block is word base + l, its row is l / M by a multiply-high with the
//     host's ceil(2^32 / M) (exact for l M < 2^32; l <= kRowElems), or
//   * one chunk of kRowElems columns of one row (M > kRowElems),
// and a thread takes elements tid, tid + 256, ...: a wave's loads are consecutive words, and the
// words of rows the mask leaves out are never asked for.  A thread's kIter mask words are loaded
// together; a wave whose lanes all have all their elements runs straight-line code (4 kIter
// loads in flight before the first store), any other predicates element by element.  The kernel
// is instantiated per kind of mask (none, uint8, int32).  A call without a mask is flat: the host
// passes the group as P M rows of one float, and where the four pointers are 16-byte aligned and
// P M divides by 4 the block moves float4 (kVec per thread).  One inline function does the
// arithmetic of both paths, without contraction, so they give the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "gsr.h"

#pragma clang fp contract(off)

int gsr_set_error(int code, const std::string &msg);  // api.hip

namespace {

constexpr int kThreads = 256;
constexpr int kIter = 4;                         // elements of a thread on the word path
constexpr uint32_t kRowElems = kThreads * kIter; // the most words of a block on the word path
constexpr int kVec = 2;                          // float4 of a thread on the dense path
constexpr uint32_t kVecElems = kThreads * kVec * 4;

struct Group {
    float *param;
    const float *grad;
    float *m, *v;
    int64_t rows;         // P, or P M on a flat (unmasked) call
    float step, eps;      // lr / bias_correction1
    uint32_t M;           // words per row (1 on a flat call)
    uint32_t mul;         // ceil(2^32 / M), M >= 2
    uint32_t R;           // rows of a block
    uint32_t col_chunks;  // blocks along a row: 1 for M <= kRowElems
    uint32_t first_block;
    uint32_t vec;         // the float4 path
};

struct Args {
    Group g[GSR_MAX_PARAM_GROUPS];
    const uint8_t *visible;
    const int32_t *radii;
    float beta1, beta2, omb1, omb2;  // omb = 1.0f - beta
    float bc2s;
    int32_t n_groups;
};

struct Coef {
    float beta1, beta2, omb1, omb2, bc2s, step, eps;
};

// include/gsr.h's three lines, in its order
__device__ __forceinline__ void adam_one(float &p, float g, float &m, float &v, const Coef &c) {
    m = c.beta1 * m + c.omb1 * g;
    v = c.beta2 * v + (c.omb2 * g) * g;
    p = p - c.step * (m / (sqrtf(v) / c.bc2s + c.eps));
}

enum { kDense = 0, kVisible = 1, kRadii = 2 };

template <int kMask>
__global__ void __launch_bounds__(kThreads) k_adam(const Args a) {
    int gi = 0;
    for (int i = 1; i < a.n_groups; ++i)
        if (blockIdx.x >= a.g[i].first_block) gi = i;
    const Group &G = a.g[gi];
    const uint32_t b = blockIdx.x - G.first_block;
    const Coef c{a.beta1, a.beta2, a.omb1, a.omb2, a.bc2s, G.step, G.eps};
    float *const P = G.param;
    const float *const Gr = G.grad;
    float *const Mo = G.m;
    float *const Vo = G.v;

    if (kMask == kDense && G.vec) {
        const int64_t nvec = G.rows >> 2;
        float4 p[kVec], g[kVec], m[kVec], v[kVec];
        int64_t q[kVec];
#pragma unroll
        for (int it = 0; it < kVec; ++it) {
            q[it] = (int64_t)b * (kThreads * kVec) + it * kThreads + threadIdx.x;
            if (q[it] < nvec) {
                p[it] = reinterpret_cast<const float4 *>(P)[q[it]];
                g[it] = reinterpret_cast<const float4 *>(Gr)[q[it]];
                m[it] = reinterpret_cast<const float4 *>(Mo)[q[it]];
                v[it] = reinterpret_cast<const float4 *>(Vo)[q[it]];
            }
        }
#pragma unroll
        for (int it = 0; it < kVec; ++it) {
            if (q[it] < nvec) {
                adam_one(p[it].x, g[it].x, m[it].x, v[it].x, c);
                adam_one(p[it].y, g[it].y, m[it].y, v[it].y, c);
                adam_one(p[it].z, g[it].z, m[it].z, v[it].z, c);
                adam_one(p[it].w, g[it].w, m[it].w, v[it].w, c);
                reinterpret_cast<float4 *>(P)[q[it]] = p[it];
                reinterpret_cast<float4 *>(Mo)[q[it]] = m[it];
                reinterpret_cast<float4 *>(Vo)[q[it]] = v[it];
            }
        }
        return;
    }

    const uint32_t rb = b / G.col_chunks, cc = b - rb * G.col_chunks;
    const int64_t row0 = (int64_t)rb * G.R;
    const int64_t at0 = row0 * G.M + (int64_t)cc * kRowElems + threadIdx.x;
    // the words of this block: R whole rows, or what is left of the row from column cc kRowElems
    const uint32_t nloc = G.col_chunks == 1 ? G.R * G.M : min(kRowElems, G.M - cc * kRowElems);
    // the mask words of the thread's kIter elements, all asked for before the first is looked at
    // (an element past the end reads the last row's, which is always there)
    bool on[kIter];
    int32_t mask[kIter];
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const uint32_t l = it * kThreads + threadIdx.x;
        const int64_t row = row0 + (G.M == 1 ? l : __umulhi(l, G.mul));
        on[it] = l < nloc && row < G.rows;
        const int64_t r = min(row, G.rows - 1);
        mask[it] = kMask == kVisible ? (int32_t)a.visible[r] : kMask == kRadii ? a.radii[r] : 1;
    }
    bool all = true;
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        on[it] = on[it] && (kMask == kRadii ? mask[it] > 0 : mask[it] != 0);
        all = all && on[it];
    }
    if (__all(all)) {
        // every lane of the wave has all its elements: straight-line code, 4 kIter loads in flight
        float p[kIter], g[kIter], m[kIter], v[kIter];
#pragma unroll
        for (int it = 0; it < kIter; ++it) {
            const int64_t at = at0 + it * kThreads;
            p[it] = P[at];
            g[it] = Gr[at];
            m[it] = Mo[at];
            v[it] = Vo[at];
        }
#pragma unroll
        for (int it = 0; it < kIter; ++it) {
            const int64_t at = at0 + it * kThreads;
            adam_one(p[it], g[it], m[it], v[it], c);
            P[at] = p[it];
            Mo[at] = m[it];
            Vo[at] = v[it];
        }
        return;
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const int64_t at = at0 + it * kThreads;
        if (on[it]) {
            float p = P[at], m = Mo[at], v = Vo[at];
            adam_one(p, Gr[at], m, v, c);
            P[at] = p;
            Mo[at] = m;
            Vo[at] = v;
        }
    }
}

__global__ void __launch_bounds__(kThreads)
k_densify_stats(int64_t P, const int32_t *__restrict__ radii, const float *__restrict__ grad,
                float *__restrict__ accum, float *__restrict__ denom,
                int32_t *__restrict__ max_radii) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= P) return;
    const int32_t r = radii[i];
    if (r <= 0) return;
    const float x = grad[3 * i], y = grad[3 * i + 1];
    accum[i] += sqrtf(x * x + y * y);
    denom[i] += 1.0f;
    if (max_radii) max_radii[i] = max(max_radii[i], r);
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return gsr_set_error(GSR_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return GSR_OK;
}

int refuse(const char *why) {
    return gsr_set_error(GSR_E_INVALID, std::string("gsr_adam_step: ") + why);
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

extern "C" {

int gsr_adam_step(const gsr_adam_settings *s, const gsr_param_group *groups, void *stream) {
    if (!s || !groups) return refuse("NULL settings or groups");
    if (s->P < 0) return refuse("P < 0");
    if (s->n_groups < 1 || s->n_groups > GSR_MAX_PARAM_GROUPS)
        return refuse("n_groups outside 1..GSR_MAX_PARAM_GROUPS");
    if (!(s->beta1 >= 0.0f && s->beta1 < 1.0f) || !(s->beta2 >= 0.0f && s->beta2 < 1.0f))
        return refuse("beta outside [0, 1)");
    if (!(s->bias_correction1 > 0.0f) || !(s->bias_correction2_sqrt > 0.0f))
        return refuse("a bias correction <= 0 or NaN");
    if (s->visible && s->radii) return refuse("both visible and radii given");
    for (int i = 0; i < s->n_groups; ++i) {
        const gsr_param_group &g = groups[i];
        if (g.M < 1) return refuse("a group's M < 1");
        if (std::isnan(g.lr) || std::isnan(g.eps)) return refuse("a group's lr or eps is NaN");
        if (s->P > 0 && (!g.param || !g.grad || !g.exp_avg || !g.exp_avg_sq))
            return refuse("a NULL buffer");
    }
    if (s->P == 0) return GSR_OK;

    const bool masked = s->visible || s->radii;
    Args a{};
    a.visible = s->visible;
    a.radii = s->radii;
    a.beta1 = s->beta1;
    a.beta2 = s->beta2;
    a.omb1 = 1.0f - s->beta1;
    a.omb2 = 1.0f - s->beta2;
    a.bc2s = s->bias_correction2_sqrt;
    a.n_groups = s->n_groups;
    int64_t blocks = 0;
    for (int i = 0; i < s->n_groups; ++i) {
        const gsr_param_group &g = groups[i];
        Group &d = a.g[i];
        if (s->P > INT64_MAX / g.M) return refuse("P * M overflows");
        d.param = g.param;
        d.grad = g.grad;
        d.m = g.exp_avg;
        d.v = g.exp_avg_sq;
        d.step = g.lr / s->bias_correction1;
        d.eps = g.eps;
        // without a mask the rows do not matter: P M rows of one word
        d.rows = masked ? s->P : s->P * g.M;
        d.M = masked ? (uint32_t)g.M : 1u;
        d.mul = d.M >= 2 ? 0xFFFFFFFFu / d.M + 1u : 0u;
        d.R = d.M <= kRowElems ? kRowElems / d.M : 1u;
        d.col_chunks = d.M <= kRowElems ? 1u : (d.M + kRowElems - 1) / kRowElems;
        d.vec = !masked && (d.rows & 3) == 0 && aligned16(g.param) && aligned16(g.grad) &&
                aligned16(g.exp_avg) && aligned16(g.exp_avg_sq);
        d.first_block = (uint32_t)blocks;
        int64_t n;
        if (d.vec)
            n = (d.rows + kVecElems - 1) / kVecElems;
        else {
            const int64_t row_blocks = (d.rows + d.R - 1) / d.R;
            if (row_blocks > INT32_MAX / (int64_t)d.col_chunks) return refuse("too many blocks");
            n = row_blocks * d.col_chunks;
        }
        blocks += n;
        if (blocks > INT32_MAX) return refuse("too many blocks");
    }
    const dim3 grid((uint32_t)blocks), block(kThreads);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (s->visible)
        hipLaunchKernelGGL(k_adam<kVisible>, grid, block, 0, st, a);
    else if (s->radii)
        hipLaunchKernelGGL(k_adam<kRadii>, grid, block, 0, st, a);
    else
        hipLaunchKernelGGL(k_adam<kDense>, grid, block, 0, st, a);
    return launched("adam step");
}

int gsr_densify_stats(const gsr_densify_inputs *in, void *stream) {
    if (!in || in->P < 0 ||
        (in->P > 0 && (!in->radii || !in->dL_dmeans2D || !in->grad_accum || !in->denom)))
        return gsr_set_error(GSR_E_INVALID, "gsr_densify_stats: bad arguments");
    if (in->P == 0) return GSR_OK;
    const int64_t blocks = (in->P + kThreads - 1) / kThreads;
    if (blocks > INT32_MAX) return gsr_set_error(GSR_E_INVALID, "gsr_densify_stats: P too large");
    hipLaunchKernelGGL(k_densify_stats, dim3((uint32_t)blocks), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), in->P, in->radii, in->dL_dmeans2D,
                       in->grad_accum, in->denom, in->max_radii);
    return launched("densify stats");
}

}  // extern "C"
