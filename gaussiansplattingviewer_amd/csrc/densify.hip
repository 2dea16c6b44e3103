// densify.hip -- adaptive density control of a fit: upstream's densify_and_prune (clone, split in
// two, prune) as a plan and an apply (gsr_densify_plan / gsr_densify_apply).  include/gsr.h states
// the semantics, DESIGN.md §3p the design.  Stateless: no context, no allocation, no atomics.
//
// The plan: k_classify gives every source row one word -- three flags (the row survives unsplit, its
// clone survives, its two children survive) and the row's three exclusive offsets within its block
// of kThreads rows (one scan of the three counts packed into one word) -- and every block its three
// sums; k_finish, one block, loops over the block sums in chunks of kThreads, turns them into
// exclusive offsets in place and writes the four counts (to the caller and into the workspace).
// The apply: k_index turns the plan into source_index (output row -> source row; -1 past the plan's
// total); k_gather, ONE launch for all groups with k_adam's by-value group table and its "block
// owns kRowElems / M whole rows, row by one multiply-high" mapping, is output-driven: it writes
// consecutive words of the new tensors (the moments of rows past n_kept as zeros) from the rows
// source_index names; k_children then overwrites the xyz and the scaling of the 2 n_split children.
// Every read is bounded by P and every write by P_out, whatever the workspace holds.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cmath>
#include <string>

#include "gsr.h"

#pragma clang fp contract(off)

int gsr_set_error(int code, const std::string &msg);  // api.hip

namespace {

constexpr int kThreads = 256;                     // rows of a scan block
constexpr int kIter = 4;                          // words of a thread in the gather
constexpr uint32_t kRowElems = kThreads * kIter;  // the most words of a gather block
constexpr int kHeader = 8;                        // workspace words before the row words
constexpr int64_t kMaxP = (int64_t)1 << 30;
constexpr uint32_t kKeep = 1u << 24, kClone = 1u << 25, kSplit = 1u << 26;
constexpr float kLog16 = (float)0.47000362924573555;  // (float)log(1.6)

struct Plan {
    const float *grad_accum, *denom, *scaling, *opacity;
    const int32_t *max_radii;
    float grad_thr, split_thr, opacity_thr, scale_thr;
    int32_t radius_thr;
    int32_t log_space;
    int32_t P;
};

__device__ __forceinline__ float child_scale(float s, bool log_space) {
    return log_space ? s - kLog16 : s / 1.6f;
}

// inclusive scan of one word per thread over the block; `total` is the block's sum
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *lds, uint32_t &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= d) incl += t;
    }
    __syncthreads();  // the previous use of lds is over
    if (lane == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) {
        const uint32_t s = lds[w];
        if (w < wave) before += s;
        total += s;
    }
    return before + incl;
}

__global__ void __launch_bounds__(kThreads)
k_classify(const Plan p, uint32_t *__restrict__ rows, int32_t *__restrict__ bsum) {
    __shared__ uint32_t lds[kThreads / 64];
    const int32_t i = (int32_t)(blockIdx.x * kThreads + threadIdx.x);
    uint32_t flags = 0;
    if (i < p.P) {
        float avg = p.grad_accum[i] / p.denom[i];
        if (avg != avg) avg = 0.0f;
        const bool hot = avg >= p.grad_thr;
        const float smax = fmaxf(fmaxf(p.scaling[3 * (int64_t)i], p.scaling[3 * (int64_t)i + 1]),
                                 p.scaling[3 * (int64_t)i + 2]);
        const bool split = hot && smax > p.split_thr;
        const bool clone = hot && smax <= p.split_thr;
        const float s = split ? child_scale(smax, p.log_space != 0) : smax;
        bool pruned = p.opacity[i] < p.opacity_thr || s > p.scale_thr;
        if (p.max_radii && p.radius_thr > 0) pruned = pruned || p.max_radii[i] > p.radius_thr;
        if (!pruned) flags = split ? kSplit : clone ? (kKeep | kClone) : kKeep;
    }
    const uint32_t packed = (flags & kKeep ? 1u : 0u) | (flags & kClone ? 1u << 10 : 0u) |
                            (flags & kSplit ? 1u << 20 : 0u);
    uint32_t total;
    const uint32_t excl = block_scan(packed, lds, total) - packed;
    if (i < p.P)
        rows[i] = flags | (excl & 0x3FFu) | ((excl >> 10) & 0x3FFu) << 8 |
                  ((excl >> 20) & 0x3FFu) << 16;
    if (threadIdx.x == 0) {
        bsum[3 * blockIdx.x] = (int32_t)(total & 0x3FFu);
        bsum[3 * blockIdx.x + 1] = (int32_t)((total >> 10) & 0x3FFu);
        bsum[3 * blockIdx.x + 2] = (int32_t)((total >> 20) & 0x3FFu);
    }
}

// one block: the block sums -> exclusive offsets, in place; the counts
__global__ void __launch_bounds__(kThreads)
k_finish(int32_t P, int32_t nb, int32_t *__restrict__ bsum, int32_t *__restrict__ header,
         int32_t *__restrict__ counts) {
    __shared__ uint32_t lds[kThreads / 64];
    uint32_t carry[3] = {0, 0, 0};
    for (int32_t c = 0; c < nb; c += kThreads) {
        const int32_t b = c + (int32_t)threadIdx.x;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const uint32_t v = b < nb ? (uint32_t)bsum[3 * (int64_t)b + k] : 0u;
            uint32_t total;
            const uint32_t incl = block_scan(v, lds, total);
            if (b < nb) bsum[3 * (int64_t)b + k] = (int32_t)(carry[k] + incl - v);
            carry[k] += total;
        }
    }
    if (threadIdx.x == 0) {
        const int32_t c[4] = {(int32_t)carry[0], (int32_t)carry[1], (int32_t)carry[2],
                              P - (int32_t)carry[0] - (int32_t)carry[2]};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            header[k] = c[k];
            counts[k] = c[k];
        }
    }
}

__global__ void __launch_bounds__(kThreads)
k_index(int32_t P, int32_t Pout, const int32_t *__restrict__ header,
        const uint32_t *__restrict__ rows, const int32_t *__restrict__ bofs,
        int32_t *__restrict__ source_index) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t nk = header[0], nc = header[1], ns = header[2];
    if (t < Pout && (t >= nk + nc + 2 * ns || nk < 0 || nc < 0 || ns < 0)) source_index[t] = -1;
    if (t >= P) return;
    const uint32_t w = rows[t];
    const int64_t b = t >> 8;
    static_assert(kThreads == 256, "the row's block is t >> 8");
    if (w & kKeep) {
        const int64_t d = (int64_t)bofs[3 * b] + (w & 255u);
        if (d >= 0 && d < Pout) source_index[d] = (int32_t)t;
    }
    if (w & kClone) {
        const int64_t d = nk + bofs[3 * b + 1] + ((w >> 8) & 255u);
        if (d >= 0 && d < Pout) source_index[d] = (int32_t)t;
    }
    if (w & kSplit) {
        const int64_t d = nk + nc + bofs[3 * b + 2] + ((w >> 16) & 255u);
        if (d >= 0 && d < Pout) source_index[d] = (int32_t)t;
        if (d + ns >= 0 && d + ns < Pout) source_index[d + ns] = (int32_t)t;
    }
}

struct Group {
    const float *sp, *sm, *sv;
    float *dp, *dm, *dv;  // dm, dv NULL: a tensor without moments
    uint32_t M;
    uint32_t mul;         // ceil(2^32 / M), M >= 2
    uint32_t R;           // output rows of a block
    uint32_t col_chunks;  // blocks along a row: 1 for M <= kRowElems
    uint32_t first_block;
};

struct Args {
    Group g[GSR_MAX_PARAM_GROUPS];
    const int32_t *header;
    const int32_t *source_index;
    int32_t n_groups;
    int32_t P, Pout;
};

__global__ void __launch_bounds__(kThreads) k_gather(const Args a) {
    int gi = 0;
    for (int i = 1; i < a.n_groups; ++i)
        if (blockIdx.x >= a.g[i].first_block) gi = i;
    const Group &G = a.g[gi];
    const uint32_t b = blockIdx.x - G.first_block;
    const uint32_t rb = b / G.col_chunks, cc = b - rb * G.col_chunks;
    const int64_t row0 = (int64_t)rb * G.R;
    // the words of this block: R whole rows, or what is left of the row from column cc kRowElems
    const uint32_t nloc = G.col_chunks == 1 ? G.R * G.M : min(kRowElems, G.M - cc * kRowElems);
    const int64_t n_kept = a.header[0];
    int64_t row[kIter], from[kIter];
    uint32_t col[kIter];
    bool on[kIter];
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        const uint32_t l = it * kThreads + threadIdx.x;
        // the word's row within the block: exact for l M < 2^32 (l < kRowElems, M <= kRowElems)
        const uint32_t rl = G.col_chunks > 1 ? 0u : G.M == 1 ? l : __umulhi(l, G.mul);
        row[it] = row0 + rl;
        col[it] = G.col_chunks > 1 ? cc * kRowElems + l : l - rl * G.M;
        on[it] = l < nloc && row[it] < a.Pout;
        from[it] = on[it] ? a.source_index[row[it]] : -1;
        on[it] = on[it] && from[it] >= 0 && from[it] < a.P;
    }
    // every load of the thread before its first store: up to 3 kIter loads in flight
    const bool moments = G.dm != nullptr;
    float p[kIter], m[kIter], v[kIter];
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        m[it] = v[it] = 0.0f;
        if (!on[it]) continue;
        const int64_t src = from[it] * G.M + col[it];
        p[it] = G.sp[src];
        if (moments && row[it] < n_kept) {
            m[it] = G.sm[src];
            v[it] = G.sv[src];
        }
    }
#pragma unroll
    for (int it = 0; it < kIter; ++it) {
        if (!on[it]) continue;
        const int64_t at = row[it] * G.M + col[it];
        G.dp[at] = p[it];
        if (moments) {
            G.dm[at] = m[it];
            G.dv[at] = v[it];
        }
    }
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t x[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    x[0] = c0;
    x[1] = c1;
    x[2] = c2;
    x[3] = c3;
}

__device__ __forceinline__ float unit(uint32_t x) {
    return ((float)(x >> 8) + 0.5f) * 5.9604644775390625e-8f;  // 2^-24
}

struct Children {
    const float *xyz, *scaling, *rotation;  // source
    float *out_xyz, *out_scaling;
    const int32_t *header, *source_index;
    uint32_t seed_lo, seed_hi;
    int32_t log_space;
    int32_t P, Pout;
};

__global__ void __launch_bounds__(kThreads) k_children(const Children c) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    const int64_t first = (int64_t)c.header[0] + c.header[1], ns = c.header[2];
    if (r >= c.Pout || r < first || first < 0 || ns < 0 || r >= first + 2 * ns) return;
    const int64_t i = c.source_index[r];
    if (i < 0 || i >= c.P) return;
    const uint32_t child = r - first >= ns ? 1u : 0u;
    const bool log_space = c.log_space != 0;
    float s[3], sigma[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k] = c.scaling[3 * i + k];
        sigma[k] = log_space ? expf(s[k]) : s[k];
        c.out_scaling[3 * r + k] = child_scale(s[k], log_space);
    }
    uint32_t x[4];
    philox4x32_10((uint32_t)i, child, 0u, 0u, c.seed_lo, c.seed_hi, x);
    const float rad0 = sqrtf(-2.0f * logf(unit(x[0]))), ang0 = 6.2831855f * unit(x[1]);
    const float rad2 = sqrtf(-2.0f * logf(unit(x[2]))), ang2 = 6.2831855f * unit(x[3]);
    const float v0 = sigma[0] * (rad0 * cosf(ang0));
    const float v1 = sigma[1] * (rad0 * sinf(ang0));
    const float v2 = sigma[2] * (rad2 * cosf(ang2));
    float qr = c.rotation[4 * i], qx = c.rotation[4 * i + 1], qy = c.rotation[4 * i + 2],
          qz = c.rotation[4 * i + 3];
    const float n = sqrtf(((qr * qr + qx * qx) + qy * qy) + qz * qz);
    qr = qr / n;
    qx = qx / n;
    qy = qy / n;
    qz = qz / n;
    const float R00 = 1.0f - 2.0f * (qy * qy + qz * qz), R01 = 2.0f * (qx * qy - qr * qz),
                R02 = 2.0f * (qx * qz + qr * qy);
    const float R10 = 2.0f * (qx * qy + qr * qz), R11 = 1.0f - 2.0f * (qx * qx + qz * qz),
                R12 = 2.0f * (qy * qz - qr * qx);
    const float R20 = 2.0f * (qx * qz - qr * qy), R21 = 2.0f * (qy * qz + qr * qx),
                R22 = 1.0f - 2.0f * (qx * qx + qy * qy);
    c.out_xyz[3 * r] = ((R00 * v0 + R01 * v1) + R02 * v2) + c.xyz[3 * i];
    c.out_xyz[3 * r + 1] = ((R10 * v0 + R11 * v1) + R12 * v2) + c.xyz[3 * i + 1];
    c.out_xyz[3 * r + 2] = ((R20 * v0 + R21 * v1) + R22 * v2) + c.xyz[3 * i + 2];
}

int launched(const char *what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return gsr_set_error(GSR_E_HIP, std::string(what) + " launch: " + hipGetErrorString(e));
    return GSR_OK;
}

int refuse(const char *who, const char *why) {
    return gsr_set_error(GSR_E_INVALID, std::string(who) + ": " + why);
}

// what both entries ask of `in`; nullptr = fine
const char *bad_inputs(const gsr_densify_plan_inputs *in) {
    if (!in) return "NULL in";
    if (in->P < 0 || in->P >= kMaxP) return "P outside 0..2^30 - 1";
    if (in->scale_space != GSR_SCALE_LINEAR && in->scale_space != GSR_SCALE_LOG)
        return "scale_space is neither GSR_SCALE_LINEAR nor GSR_SCALE_LOG";
    if (std::isnan(in->grad_threshold) || std::isnan(in->scale_split_threshold) ||
        std::isnan(in->opacity_prune_threshold) || std::isnan(in->scale_prune_threshold))
        return "a NaN threshold";
    if (in->P > 0 && (!in->grad_accum || !in->denom || !in->scaling || !in->opacity))
        return "a NULL grad_accum, denom, scaling or opacity";
    return nullptr;
}

int64_t scan_blocks(int64_t P) { return (P + kThreads - 1) / kThreads; }

}  // namespace

extern "C" {

int64_t gsr_densify_workspace(int64_t P) {
    if (P < 0 || P >= kMaxP)
        return refuse("gsr_densify_workspace", "P outside 0..2^30 - 1");
    return 4 * (kHeader + P + 3 * scan_blocks(P));
}

int gsr_densify_plan(const gsr_densify_plan_inputs *in, void *workspace, int32_t *counts_dev,
                     void *stream) {
    const char *who = "gsr_densify_plan";
    if (const char *why = bad_inputs(in)) return refuse(who, why);
    if (!workspace || !counts_dev) return refuse(who, "NULL workspace or counts_dev");
    const int32_t P = (int32_t)in->P, nb = (int32_t)scan_blocks(in->P);
    int32_t *header = static_cast<int32_t *>(workspace);
    uint32_t *rows = reinterpret_cast<uint32_t *>(header + kHeader);
    int32_t *bsum = header + kHeader + P;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (P > 0) {
        Plan p{};
        p.grad_accum = in->grad_accum;
        p.denom = in->denom;
        p.scaling = in->scaling;
        p.opacity = in->opacity;
        p.max_radii = in->max_radii;
        p.grad_thr = in->grad_threshold;
        p.split_thr = in->scale_split_threshold;
        p.opacity_thr = in->opacity_prune_threshold;
        p.scale_thr = in->scale_prune_threshold;
        p.radius_thr = in->radius_prune_threshold;
        p.log_space = in->scale_space == GSR_SCALE_LOG;
        p.P = P;
        hipLaunchKernelGGL(k_classify, dim3((uint32_t)nb), dim3(kThreads), 0, st, p, rows, bsum);
        if (const int rc = launched("densify classify")) return rc;
    }
    hipLaunchKernelGGL(k_finish, dim3(1), dim3(kThreads), 0, st, P, nb, bsum, header, counts_dev);
    return launched("densify scan");
}

int gsr_densify_apply(const gsr_densify_plan_inputs *in, const gsr_densify_group *src_groups,
                      const gsr_densify_group *dst_groups, const void *workspace,
                      int32_t *source_index, void *stream) {
    const char *who = "gsr_densify_apply";
    if (const char *why = bad_inputs(in)) return refuse(who, why);
    if (!src_groups || !dst_groups || !workspace)
        return refuse(who, "NULL src_groups, dst_groups or workspace");
    if (in->n_groups < 1 || in->n_groups > GSR_MAX_PARAM_GROUPS)
        return refuse(who, "n_groups outside 1..GSR_MAX_PARAM_GROUPS");
    const int64_t P = in->P, Pout = in->P_out;
    if (Pout < 0 || Pout > GSR_SPLIT_CHILDREN * P) return refuse(who, "P_out outside 0..2 P");
    int role_at[5] = {-1, -1, -1, -1, -1};
    static const int32_t role_M[5] = {0, 3, 3, 4, 1};
    for (int i = 0; i < in->n_groups; ++i) {
        const gsr_densify_group &s = src_groups[i], &d = dst_groups[i];
        if (s.M < 1 || d.M != s.M) return refuse(who, "a group's M < 1, or not the same in src and dst");
        if (s.role != d.role || s.role < GSR_ROLE_NONE || s.role > GSR_ROLE_OPACITY)
            return refuse(who, "an unknown role, or not the same in src and dst");
        if (s.role != GSR_ROLE_NONE) {
            if (s.M != role_M[s.role]) return refuse(who, "a role with the wrong M");
            if (role_at[s.role] >= 0) return refuse(who, "a duplicated role");
            role_at[s.role] = i;
        }
        // (a destination of no rows may be all NULL)
        if (!s.exp_avg != !s.exp_avg_sq || (Pout > 0 && !d.exp_avg != !d.exp_avg_sq))
            return refuse(who, "one moment NULL and the other not");
        if (Pout > 0 && !s.exp_avg != !d.exp_avg)
            return refuse(who, "moments in one of src and dst only");
        if (P > 0 && !s.param) return refuse(who, "a NULL source buffer");
        if (Pout > 0 && !d.param) return refuse(who, "a NULL destination buffer");
    }
    for (int r = GSR_ROLE_XYZ; r <= GSR_ROLE_OPACITY; ++r)
        if (role_at[r] < 0) return refuse(who, "a missing role (xyz, scaling, rotation, opacity)");
    if (P > 0 && (src_groups[role_at[GSR_ROLE_SCALING]].param != in->scaling ||
                  src_groups[role_at[GSR_ROLE_OPACITY]].param != in->opacity))
        return refuse(who, "the scaling or opacity role is not the plan's buffer");
    if (Pout > 0 && !source_index) return refuse(who, "NULL source_index");

    Args a{};
    const int32_t *header = static_cast<const int32_t *>(workspace);
    a.header = header;
    a.source_index = source_index;
    a.n_groups = in->n_groups;
    a.P = (int32_t)P;
    a.Pout = (int32_t)Pout;
    int64_t blocks = 0;
    for (int i = 0; i < in->n_groups; ++i) {
        const gsr_densify_group &s = src_groups[i], &d = dst_groups[i];
        Group &g = a.g[i];
        g.sp = s.param;
        g.sm = s.exp_avg;
        g.sv = s.exp_avg_sq;
        g.dp = d.param;
        g.dm = d.exp_avg;
        g.dv = d.exp_avg_sq;
        g.M = (uint32_t)s.M;
        g.mul = g.M >= 2 ? 0xFFFFFFFFu / g.M + 1u : 0u;
        g.R = g.M <= kRowElems ? kRowElems / g.M : 1u;
        g.col_chunks = g.M <= kRowElems ? 1u : (g.M + kRowElems - 1) / kRowElems;
        g.first_block = (uint32_t)blocks;
        blocks += (Pout + g.R - 1) / g.R * g.col_chunks;
        if (blocks > INT32_MAX) return refuse(who, "too many blocks");
    }
    if (Pout == 0) return GSR_OK;

    hipStream_t st = static_cast<hipStream_t>(stream);
    const uint32_t *rows = reinterpret_cast<const uint32_t *>(header + kHeader);
    const int32_t *bofs = header + kHeader + P;
    const int64_t most = P > Pout ? P : Pout;
    hipLaunchKernelGGL(k_index, dim3((uint32_t)scan_blocks(most)), dim3(kThreads), 0, st,
                       (int32_t)P, (int32_t)Pout, header, rows, bofs, source_index);
    if (const int rc = launched("densify index")) return rc;
    hipLaunchKernelGGL(k_gather, dim3((uint32_t)blocks), dim3(kThreads), 0, st, a);
    if (const int rc = launched("densify gather")) return rc;
    Children c{};
    c.xyz = src_groups[role_at[GSR_ROLE_XYZ]].param;
    c.scaling = src_groups[role_at[GSR_ROLE_SCALING]].param;
    c.rotation = src_groups[role_at[GSR_ROLE_ROTATION]].param;
    c.out_xyz = dst_groups[role_at[GSR_ROLE_XYZ]].param;
    c.out_scaling = dst_groups[role_at[GSR_ROLE_SCALING]].param;
    c.header = header;
    c.source_index = source_index;
    c.seed_lo = (uint32_t)in->seed;
    c.seed_hi = (uint32_t)(in->seed >> 32);
    c.log_space = in->scale_space == GSR_SCALE_LOG;
    c.P = (int32_t)P;
    c.Pout = (int32_t)Pout;
    hipLaunchKernelGGL(k_children, dim3((uint32_t)scan_blocks(Pout)), dim3(kThreads), 0, st, c);
    return launched("densify children");
}

}  // extern "C"
