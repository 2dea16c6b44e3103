// knn.hip -- the start of a fit from a point cloud: for every point the mean squared distance to
// its three nearest neighbours (gsr_knn_mean_dist2; upstream's simple_knn distCUDA2).
// include/gsr.h states the semantics, DESIGN.md §3t the design.  Stateless: no context, no
// allocation, no atomics of its own, no synchronisation.
//
// Four stages, all on the caller's stream and in the caller's workspace:
//   0  k_knn_bounds (block partials) and k_knn_bounds_finish (one block): the cloud's bounding
//      box; k_knn_codes: a 30-bit Morton code per point (10 bits per axis), value = index;
//   1  gsr_radix_sort_pairs over bits [0, 30) (radix_sort.hip, untouched);
//   2  k_knn_boxes: one block per box of kBox consecutive sorted points gathers their float4
//      records (x, y, z, original index as bits) and reduces the box's axis-aligned bounds;
//   3  k_knn_search: one block per box, one lane per point, three running best values in
//      registers.  The block scans its own box, then visits the others outward (b + 1, b - 1,
//      b + 2, ...), kBox candidates per round: each lane pre-tests one candidate box against the
//      block's own bounds and the block's largest third-best value; for each survivor, in outward
//      order, every lane computes its own distance to the box and the block skips the box when no
//      lane can gain from it; otherwise the box's records are staged in LDS (4 KB) and the lanes
//      that can gain scan them.
// Every distance to a box is computed with the operations of d_ij in d_ij's order, and float32
// subtraction, multiplication and addition are monotone under rounding, so it is <= the computed
// d_ij of every point in the box: a skipped box holds no value below the lane's third best, and
// the three smallest values -- a multiset -- are those of the brute-force search, bit for bit.
// Every barrier sits in block-uniform control flow: the decisions that guard one are read from
// LDS words (or reduced over the block) that every lane sees alike; lanes past N stay in every
// loop, never vote for a scan and write nothing.  Every loop's trip count is a function of N and
// the block's index; every index into a buffer is clamped or compared with N first.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>

#include "gsr.h"
#include "gsr_internal.h"

#pragma clang fp contract(off)

int gsr_set_error(int code, const std::string &msg);  // api.hip

namespace {

constexpr int kBox = 256;            // points of a box = threads of a block
constexpr int kWaves = kBox / 64;
constexpr int kBoundsBlocks = 1024;  // the most blocks of the bounds pass
constexpr int64_t kMaxN = (int64_t)1 << 30;
constexpr int64_t kAlign = 256;      // every workspace segment starts on a multiple of it
constexpr int kStages = 4;

__device__ __forceinline__ float pos_inf() { return __int_as_float(0x7F800000); }

struct Bounds {
    float lo[3], hi[3];
};

// min / max of the six words over the block, in every thread (lds: kWaves * 6 floats)
__device__ __forceinline__ Bounds block_bounds(Bounds v, float *lds) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            v.lo[a] = fminf(v.lo[a], __shfl_xor(v.lo[a], d, 64));
            v.hi[a] = fmaxf(v.hi[a], __shfl_xor(v.hi[a], d, 64));
        }
    }
    __syncthreads();  // the previous use of lds is over
    if (lane == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            lds[wave * 6 + a] = v.lo[a];
            lds[wave * 6 + 3 + a] = v.hi[a];
        }
    }
    __syncthreads();
    Bounds r;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        r.lo[a] = lds[a];
        r.hi[a] = lds[3 + a];
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            r.lo[a] = fminf(r.lo[a], lds[w * 6 + a]);
            r.hi[a] = fmaxf(r.hi[a], lds[w * 6 + 3 + a]);
        }
    }
    return r;
}

__device__ __forceinline__ Bounds empty_bounds() {
    Bounds b;
#pragma unroll
    for (int a = 0; a < 3; ++a) b.lo[a] = pos_inf(), b.hi[a] = -pos_inf();
    return b;
}

__device__ __forceinline__ void add_point(Bounds &b, float x, float y, float z) {
    b.lo[0] = fminf(b.lo[0], x), b.hi[0] = fmaxf(b.hi[0], x);
    b.lo[1] = fminf(b.lo[1], y), b.hi[1] = fmaxf(b.hi[1], y);
    b.lo[2] = fminf(b.lo[2], z), b.hi[2] = fmaxf(b.hi[2], z);
}

// stage 0: `grid` blocks, block g takes points g * kBox + t, + grid * kBox, ...; partial[6 g ..]
__global__ void __launch_bounds__(kBox)
k_knn_bounds(const float *__restrict__ xyz, int32_t N, float *__restrict__ partial) {
    __shared__ float lds[kWaves * 6];
    Bounds b = empty_bounds();
    const int64_t stride = (int64_t)gridDim.x * kBox;
    for (int64_t i = (int64_t)blockIdx.x * kBox + threadIdx.x; i < N; i += stride)
        add_point(b, xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]);
    b = block_bounds(b, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            partial[6 * blockIdx.x + a] = b.lo[a];
            partial[6 * blockIdx.x + 3 + a] = b.hi[a];
        }
    }
}

// one block: the partials of n_partial blocks -> bbox[0..2] = lo, bbox[4..6] = hi
__global__ void __launch_bounds__(kBox)
k_knn_bounds_finish(const float *__restrict__ partial, int32_t n_partial,
                    float *__restrict__ bbox) {
    __shared__ float lds[kWaves * 6];
    Bounds b = empty_bounds();
    for (int32_t g = threadIdx.x; g < n_partial; g += kBox) {
        add_point(b, partial[6 * g], partial[6 * g + 1], partial[6 * g + 2]);
        add_point(b, partial[6 * g + 3], partial[6 * g + 4], partial[6 * g + 5]);
    }
    b = block_bounds(b, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            bbox[a] = b.lo[a];
            bbox[4 + a] = b.hi[a];
        }
    }
}

// 10 bits -> every third bit of 30
__device__ __forceinline__ uint32_t spread3(uint32_t v) {
    v &= 0x3FFu;
    v = (v | (v << 16)) & 0x030000FFu;
    v = (v | (v << 8)) & 0x0300F00Fu;
    v = (v | (v << 4)) & 0x030C30C3u;
    v = (v | (v << 2)) & 0x09249249u;
    return v;
}

// cell 0..1023 of p on an axis [lo, hi]; an axis of zero (or non-finite) extent maps to cell 0.
// The cell is clamped as a float before and as an integer after the conversion, so that no
// input, finite or not, leaves [0, 1023].
__device__ __forceinline__ uint32_t cell(float p, float lo, float hi) {
    const float ext = hi - lo;
    if (!(ext > 0.0f)) return 0u;
    float t = ((p - lo) / ext) * 1023.0f;
    t = fminf(fmaxf(t, 0.0f), 1023.0f);  // (fmaxf(NaN, 0) = 0)
    const int c = (int)t;
    return (uint32_t)min(max(c, 0), 1023);
}

__global__ void __launch_bounds__(kBox)
k_knn_codes(const float *__restrict__ xyz, int32_t N, const float *__restrict__ bbox,
            uint32_t *__restrict__ keys, uint32_t *__restrict__ vals) {
    const int64_t i = (int64_t)blockIdx.x * kBox + threadIdx.x;
    if (i >= N) return;
    const uint32_t cx = cell(xyz[3 * i], bbox[0], bbox[4]);
    const uint32_t cy = cell(xyz[3 * i + 1], bbox[1], bbox[5]);
    const uint32_t cz = cell(xyz[3 * i + 2], bbox[2], bbox[6]);
    keys[i] = spread3(cx) | (spread3(cy) << 1) | (spread3(cz) << 2);
    vals[i] = (uint32_t)i;
}

// stage 2: block b = box b = sorted positions [b kBox, min(N, (b + 1) kBox)).  rec[s] = the
// point at sorted position s and its index; boxes[2 b] = the box's lo, boxes[2 b + 1] its hi.
__global__ void __launch_bounds__(kBox)
k_knn_boxes(const float *__restrict__ xyz, int32_t N, const uint32_t *__restrict__ order,
            float4 *__restrict__ rec, float4 *__restrict__ boxes) {
    __shared__ float lds[kWaves * 6];
    const int64_t s = (int64_t)blockIdx.x * kBox + threadIdx.x;
    Bounds b = empty_bounds();
    if (s < N) {
        // (a sorted permutation holds indices below N; the clamp bounds the read whatever the
        // workspace holds)
        const uint32_t i = min(order[s], (uint32_t)(N - 1));
        const float x = xyz[3 * (int64_t)i], y = xyz[3 * (int64_t)i + 1],
                    z = xyz[3 * (int64_t)i + 2];
        rec[s] = make_float4(x, y, z, __uint_as_float(i));
        add_point(b, x, y, z);
    }
    b = block_bounds(b, lds);
    if (threadIdx.x == 0) {
        boxes[2 * (int64_t)blockIdx.x] = make_float4(b.lo[0], b.lo[1], b.lo[2], 0.0f);
        boxes[2 * (int64_t)blockIdx.x + 1] = make_float4(b.hi[0], b.hi[1], b.hi[2], 0.0f);
    }
}

// max(0, lo - p, p - hi): the distance of p to [lo, hi] on one axis
__device__ __forceinline__ float axis_gap(float p, float lo, float hi) {
    return fmaxf(fmaxf(lo - p, p - hi), 0.0f);
}

// the squared distance of a point to a box, in d_ij's operations and order
__device__ __forceinline__ float box_dist2(float x, float y, float z, const float4 lo,
                                           const float4 hi) {
    const float gx = axis_gap(x, lo.x, hi.x), gy = axis_gap(y, lo.y, hi.y),
                gz = axis_gap(z, lo.z, hi.z);
    return (gx * gx + gy * gy) + gz * gz;
}

// the same between two boxes: on every axis the gap is <= the gap of any point of box a
__device__ __forceinline__ float box_box_dist2(const float4 alo, const float4 ahi,
                                               const float4 lo, const float4 hi) {
    const float gx = fmaxf(fmaxf(lo.x - ahi.x, alo.x - hi.x), 0.0f),
                gy = fmaxf(fmaxf(lo.y - ahi.y, alo.y - hi.y), 0.0f),
                gz = fmaxf(fmaxf(lo.z - ahi.z, alo.z - hi.z), 0.0f);
    return (gx * gx + gy * gy) + gz * gz;
}

// stage 3
__global__ void __launch_bounds__(kBox)
k_knn_search(const float4 *__restrict__ rec, const float4 *__restrict__ boxes, int32_t N,
             int32_t nb, float *__restrict__ dist2, uint32_t *__restrict__ scanned) {
    __shared__ float4 s_rec[kBox];
    __shared__ float s_max[kWaves];
    __shared__ float4 s_box[kBox][2];        // a round's candidate boxes: lo, hi
    __shared__ uint32_t s_cand[kWaves][2];   // a round's surviving candidates, 64 per wave
    __shared__ uint32_t s_vote[2][kWaves];   // two parities: a vote may follow a vote at once
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t b = (int32_t)blockIdx.x;
    const int64_t s = (int64_t)b * kBox + tid;
    const bool valid = s < N;
    const float4 me = valid ? rec[s] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    // a lane past N holds -1: no distance is below it, so it never votes for a scan
    float best0 = valid ? pos_inf() : -1.0f, best1 = best0, best2 = best0;
    const float4 blo = boxes[2 * (int64_t)b], bhi = boxes[2 * (int64_t)b + 1];
    uint32_t n_scanned = 0;
    int parity = 0;

    // stage box c in LDS (the caller's barrier has ended every read of the previous box) and,
    // in the lanes that asked for it, fold its points into the three best
    auto scan = [&](int32_t c, bool mine) {
        const int32_t cnt = min(kBox, N - c * kBox);  // 1..kBox: c < nb
        if (tid < cnt) s_rec[tid] = rec[(int64_t)c * kBox + tid];
        __syncthreads();
        if (mine) {
            const int32_t self = c == b ? tid : -1;  // the index excluded, nothing else
            for (int32_t j = 0; j < cnt; ++j) {
                const float4 q = s_rec[j];
                const float dx = me.x - q.x, dy = me.y - q.y, dz = me.z - q.z;
                float d = (dx * dx + dy * dy) + dz * dz;
                if (j == self) d = pos_inf();
                const float m0 = fmaxf(best0, d);
                best0 = fminf(best0, d);
                const float m1 = fmaxf(best1, m0);
                best1 = fminf(best1, m0);
                best2 = fminf(best2, m1);
            }
        }
        ++n_scanned;
    };

    scan(b, valid);

    // outward position q = 0, 1, 2, ... is box b + 1, b - 1, b + 2, ...; positions beyond either
    // end of the cloud are no boxes.  `total` depends on N and b alone.
    const int32_t total = 2 * max(b, nb - 1 - b);
    for (int32_t base = 0; base < total; base += kBox) {
        // the block's largest third best (lanes past N hold -1)
        float mb = best2;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mb = fmaxf(mb, __shfl_xor(mb, d, 64));
        __syncthreads();  // the previous round's reads of s_max, s_box and s_cand are over
        if (lane == 0) s_max[wave] = mb;
        __syncthreads();
        mb = fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
        // one candidate per lane against the block's own bounds
        const int32_t q = base + tid, step = (q >> 1) + 1;
        const int32_t c = (q & 1) ? b - step : b + step;
        bool need = false;
        if (q < total && c >= 0 && c < nb) {
            const float4 lo = boxes[2 * (int64_t)c], hi = boxes[2 * (int64_t)c + 1];
            need = !(box_box_dist2(blo, bhi, lo, hi) > mb);
            s_box[tid][0] = lo;  // (the votes below read the survivors' bounds from LDS)
            s_box[tid][1] = hi;
        }
        const unsigned long long m = __ballot(need);
        if (lane == 0) {
            s_cand[wave][0] = (uint32_t)m;
            s_cand[wave][1] = (uint32_t)(m >> 32);
        }
        __syncthreads();
        for (int w = 0; w < kWaves; ++w) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                // (a word every lane reads alike, moved to a scalar register: the loop over its
                // bits, and the barriers inside, are uniform for the compiler too)
                uint32_t bits = __builtin_amdgcn_readfirstlane(s_cand[w][h]);
                while (bits) {
                    const int bit = __builtin_ctz(bits);
                    bits &= bits - 1u;
                    const int slot = w * 64 + h * 32 + bit;
                    const int32_t qq = base + slot, st = (qq >> 1) + 1;
                    const int32_t cc = (qq & 1) ? b - st : b + st;  // in [0, nb): it was tested
                    const float4 lo = s_box[slot][0], hi = s_box[slot][1];
                    const bool mine = !(box_dist2(me.x, me.y, me.z, lo, hi) > best2);
                    // the block's vote; it is also the barrier behind the previous scan
                    const unsigned long long v = __ballot(mine);
                    if (lane == 0) s_vote[parity][wave] = v != 0ull;
                    __syncthreads();
                    const uint32_t any = s_vote[parity][0] | s_vote[parity][1] |
                                         s_vote[parity][2] | s_vote[parity][3];
                    parity ^= 1;
                    if (__builtin_amdgcn_readfirstlane(any)) scan(cc, mine);
                }
            }
        }
    }

    if (tid == 0) scanned[b] = n_scanned;
    if (!valid) return;
    const uint32_t i = __float_as_uint(me.w);
    if (i >= (uint32_t)N) return;
    float r = 0.0f;  // N == 1
    if (N >= 4) r = ((best0 + best1) + best2) / 3.0f;
    else if (N == 3) r = (best0 + best1) / 2.0f;
    else if (N == 2) r = best0 / 1.0f;
    dist2[i] = r;
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

int64_t up(int64_t bytes) { return (bytes + kAlign - 1) / kAlign * kAlign; }

// the workspace's segments, as byte offsets from its first kAlign-aligned address
struct Layout {
    int64_t nb, grid;
    int64_t scanned, bbox, partial, keys, keys_alt, vals, vals_alt, hist, digits, rec, boxes, end;
};

Layout layout(int64_t N) {
    Layout l{};
    l.nb = (N + kBox - 1) / kBox;
    l.grid = l.nb < kBoundsBlocks ? l.nb : kBoundsBlocks;
    int64_t at = 0;
    auto take = [&](int64_t bytes) {
        const int64_t here = at;
        at += up(bytes);
        return here;
    };
    l.scanned = take(4 * l.nb);
    l.bbox = take(4 * 8);
    l.partial = take(4 * 6 * l.grid);
    l.keys = take(4 * N);
    l.keys_alt = take(4 * N);
    l.vals = take(4 * N);
    l.vals_alt = take(4 * N);
    l.hist = take(4 * gsr_radix_hist_words(N));
    l.digits = take(4 * 256);
    l.rec = take(16 * N);
    l.boxes = take(32 * l.nb);
    l.end = at;
    return l;
}

}  // namespace

extern "C" {

int64_t gsr_knn_workspace(int64_t N) {
    if (N < 0 || N >= kMaxN) return refuse("gsr_knn_workspace", "N outside 0..2^30 - 1");
    return layout(N).end + kAlign;  // (room to align the caller's pointer)
}

int gsr_knn_stages(const float *xyz, int64_t N, float *dist2, void *workspace, int32_t n_stages,
                   void *stream) {
    const char *who = n_stages == kStages ? "gsr_knn_mean_dist2" : "gsr_knn_stages";
    if (N < 0 || N >= kMaxN) return refuse(who, "N outside 0..2^30 - 1");
    if (n_stages < 1 || n_stages > kStages) return refuse(who, "n_stages outside 1..4");
    if (N > 0 && (!xyz || !dist2 || !workspace)) return refuse(who, "a NULL xyz, dist2 or workspace");
    if (N == 0) return GSR_OK;
    const Layout l = layout(N);
    char *ws = reinterpret_cast<char *>(up((int64_t) reinterpret_cast<uintptr_t>(workspace)));
    auto words = [&](int64_t off) { return reinterpret_cast<uint32_t *>(ws + off); };
    auto floats = [&](int64_t off) { return reinterpret_cast<float *>(ws + off); };
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int32_t n = (int32_t)N, nb = (int32_t)l.nb;
    const dim3 boxes_grid((uint32_t)nb), block(kBox);

    hipLaunchKernelGGL(k_knn_bounds, dim3((uint32_t)l.grid), block, 0, st, xyz, n,
                       floats(l.partial));
    if (const int rc = launched("knn bounds")) return rc;
    hipLaunchKernelGGL(k_knn_bounds_finish, dim3(1), block, 0, st, floats(l.partial),
                       (int32_t)l.grid, floats(l.bbox));
    if (const int rc = launched("knn bounds finish")) return rc;
    hipLaunchKernelGGL(k_knn_codes, boxes_grid, block, 0, st, xyz, n, floats(l.bbox),
                       words(l.keys), words(l.vals));
    if (const int rc = launched("knn codes")) return rc;
    if (n_stages < 2) return GSR_OK;

    uint32_t *keys = words(l.keys), *vals = words(l.vals), *keys_alt = words(l.keys_alt),
             *vals_alt = words(l.vals_alt);
    const hipError_t e = gsr_radix_sort_pairs(&keys, &vals, &keys_alt, &vals_alt, N, 0, 30,
                                              words(l.hist), words(l.digits), st);
    if (e != hipSuccess)
        return gsr_set_error(GSR_E_HIP, std::string("knn sort: ") + hipGetErrorString(e));
    if (n_stages < 3) return GSR_OK;

    float4 *rec = reinterpret_cast<float4 *>(ws + l.rec);
    float4 *boxes = reinterpret_cast<float4 *>(ws + l.boxes);
    hipLaunchKernelGGL(k_knn_boxes, boxes_grid, block, 0, st, xyz, n, vals, rec, boxes);
    if (const int rc = launched("knn boxes")) return rc;
    if (n_stages < 4) return GSR_OK;

    hipLaunchKernelGGL(k_knn_search, boxes_grid, block, 0, st, rec, boxes, n, nb, dist2,
                       words(l.scanned));
    return launched("knn search");
}

int gsr_knn_mean_dist2(const float *xyz, int64_t N, float *dist2, void *workspace, void *stream) {
    return gsr_knn_stages(xyz, N, dist2, workspace, kStages, stream);
}

}  // extern "C"
