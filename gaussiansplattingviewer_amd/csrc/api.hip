// api.hip -- the C ABI of libgsr.so (declared in include/gsr.h): workspace ownership,
// argument validation, stage orchestration on the caller's stream, stage timing.
//
// gsr_forward replaces upstream `_C.rasterize_gaussians` / Rasterizer::forward
// (rasterizer_impl.cu), which the viewer reaches through renderer_cuda.py:211-224.  One frame is
// a fixed sequence of stages, each its own function below:
//
//   main stream                                    second stream (fork after the preprocess)
//   1 preprocess        (preprocess.hip)           pair count K + depth-key bits -> pinned host
//   2 depth sort        (depth_sort.hip)           SH -> RGB colour
//   3 column counts + scan  (binning.hip)
//   4 column scatter    = tile-sort pass 1
//   5 row pass          = tile-sort pass 2 (radix_sort.hip); its downsweep also writes the
//                         tile ranges and the blend's tile-group order
//   6 join                                          <- join
//   7 blend             (blend.hip)               gsr_forward_shaded: a GL shading's first-hit kernel
//                                                  gsr_forward_depth: the depth-accumulating composite
//                                                  gsr_forward_surface: ... that notes the median splat
//
// Binning has two forms with identical results: the column-first form above (default), and the
// per-pair form (offsets scan -> duplicate fused with the first tile-sort pass -> the remaining
// passes -> tile ranges from the sorted keys) for the frames the column form cannot take: more
// than 256 tile columns or strip rows, or more Gaussians than the packed pair word holds (the choice is automatic; tests reach the per-pair form with images
// wider than 256 tiles).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "gsr.h"
#include "gsr_internal.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string &msg) {
    g_err = msg;
    return code;
}

#define GSR_HIP(call, what)                                                                  \
    do {                                                                                     \
        hipError_t e_ = (call);                                                              \
        if (e_ != hipSuccess)                                                                \
            return fail(GSR_E_HIP, std::string(what) + ": " + hipGetErrorString(e_));        \
    } while (0)

#define GSR_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != GSR_OK) return rc_; \
    } while (0)

// A grow-only device buffer (grow) ...
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};
// ... of T, which enters itself in its context's list of buffers (gsr_destroy frees that list).
template <typename T>
struct Buf : DevBuf {
    explicit Buf(std::vector<DevBuf *> &all) { all.push_back(this); }
    T *get() const { return static_cast<T *>(p); }
};

constexpr int kStages = 7;        // the chain on the caller's stream
constexpr int kAllStages = 8;     // + "color", on the second stream (overlaps stages 1..5)
constexpr int kTimingRing = 256;  // frames whose stage events are kept
// The host learns the pair count K and the depth-key bits D by spinning on pinned words the GPU
// stores (k_publish_K, the depth sort's pass 0); after this long without them it falls back to a
// blocking wait (K) or queues every depth pass (D).
constexpr auto kSpinLimit = std::chrono::milliseconds(50);
// Frames with at least this many pairs wait for D before queueing the LSD depth sort's later
// passes (an empty third pass stays off the GPU: C3 3,480 vs 3,340 frames/s); smaller frames are
// bound by the host's submission rate, which the wait would hold to the GPU (DESIGN.md §3
// decision 2).  Only while the previous frame's D left a pass to skip (<= 24 bits): a frame whose
// keys vary in more bits needs all three, and the wait only holds the host (c3r, D = 31).
constexpr int64_t kWaitDPairs = 4 << 20;
// The depth sort compacts the kept keys first on strips of at least this many Gaussians
// (GSR_OPT_DEPTH_SORT auto): a 1/8 strip of C4 keeps ~1/8 of them (DESIGN.md decision 2).
constexpr int64_t kCompactP = 4 << 20;
// The MSD depth sort for frames whose previous frame's kept depth keys spanned a range of <= this
// many bits (setup_frame).
constexpr uint32_t kMsdMaxD = 25;
// ... and of <= this many on one-stream frames (GSR_OPT_SECOND_STREAM 0, frames in flight): there
// the frame's total work counts more than its critical path, and the MSD form's single pass
// outweighs the block sorts of crowded buckets (c3r, Dr = 26, four frames in flight: 4,200 ->
// 4,420 frames/s, while a serial frame loses 0.315 -> 0.342 ms; profiles/r05z5_ab_msd26.txt)
constexpr uint32_t kMsdMaxDOneStream = kMsdMaxD + 1;
// The MSD local sort keeps its wide form (8192 LDS slots) for this many frames after one whose
// buckets crowded the narrow form's 4096 (C5: serial 0.342 -> 0.315 ms; the narrow form's
// smaller LDS keeps C3 even, profiles/r05w_ab_local_slots.txt).
constexpr uint32_t kCrowdFrames = 8;

const char *kStageNames[kAllStages] = {"preprocess", "depth_sort", "scan",  "duplicate",
                                       "tile_sort",  "ranges",     "blend", "color"};

// Frame graphs: recorded pairs of graphs kept per context (least recently used replaced), and
// executable graphs replaced while possibly in flight, kept until a synchronisation point.
constexpr size_t kGraphCache = 4;
constexpr size_t kGraphRetired = 16;
// The binning capacity of frame graphs: the list length seen so far plus a quarter, at least
// kMinListCap entries.
constexpr int64_t kMinListCap = 1 << 16;

// Everything the kernels of a frame's recorded graphs read besides the context's own
// workspace (named by its generation): a forward whose key equals a recorded one replays it.
// The shading (gsr_forward_shaded) reaches the recorded chains only through `tight` -- the
// billboard's full lists -- and selects the blend's kernel, which is launched directly after
// them: frames of different shadings and equal lists share their graphs.  So do depth frames
// (gsr_forward_depth), surface frames (gsr_forward_surface) and plain ones: the planes are
// arguments of that direct launch alone, and the depth keys it reads are written by the
// preprocess, which is a direct launch too.
struct GraphKey {
    uint64_t ws_gen;
    int64_t cap, P;
    const void *means3D, *shs, *colors_precomp;
    int32_t D, M, W, H;
    uint32_t gx, gy, rb, re;
    int32_t col_shift, color_waves;
    uint8_t msd, main_publish, tight, sh_vec4;
};

struct GraphEntry {
    GraphKey key;
    // the frame stream's two halves (K publish + depth sort; column counts + binning) and the
    // second stream's chain: queued in the direct path's order, sort, second stream, binning
    hipGraphExec_t sort = nullptr, bin = nullptr, aux = nullptr;
    uint32_t *point_list = nullptr;                // the list the recorded row pass leaves
    uint64_t used = 0;                             // LRU stamp
};

}  // namespace

struct gsr_context {
    int device = 0;
    // One caller at a time: every entry point that reads or changes the context's workspace,
    // options, pinned words or recorded graphs holds this (the `_C` extension renders with the
    // GIL released, so two host threads may reach one device's context together).
    std::mutex mu;
    // The stream the last call that used the workspace ran on: a call on another stream first
    // waits for the device (the workspace is stream-ordered on one stream at a time).
    hipStream_t ws_stream = nullptr;
    bool ws_stream_set = false;
    // The workspace: every device buffer is declared once, here, with its element type, and
    // enters itself in `bufs`.  Per-Gaussian workspace:
    std::vector<DevBuf *> bufs;
    Buf<gsr::SplatRecord> records{bufs};
    Buf<uint2> strip_rect{bufs}, rect_sorted{bufs};
    Buf<uint32_t> sort_keys{bufs}, partials{bufs}, hist{bufs}, digit_total{bufs};
    Buf<uint64_t> total{bufs}, pair_count{bufs};
    Buf<uint4> bin{bufs};
    Buf<uint32_t> chunk_first{bufs};
    // tight binning: {rect, span word}, by id and in depth order
    Buf<uint4> strip_rc{bufs}, rc_sorted{bufs};
    // depth sort: (key, id) pairs between passes (ping-pong); ds_b also as words, the compacted
    // keys and from word P their ids
    Buf<uint2> ds_a{bufs}, ds_b{bufs};
    uint32_t *ds_b_words() const { return reinterpret_cast<uint32_t *>(ds_b.get()); }
    Buf<uint32_t> block_kept{bufs};  // depth sort compaction (strips): kept keys per 256-key block
    Buf<uint32_t> color_ids{bufs};   // compacted strips: the kept ids the colour pass walks
    Buf<uint32_t> perm{bufs};        // the depth sort's result: kept Gaussian ids in depth order
    Buf<uint32_t> ds_ctl{bufs};      // depth sort control: kept count, key bits, per-tile key stats
    Buf<uint32_t> col_hist{bufs};    // column-first binning: per-(Gaussian block, column) counts
    // per-pair workspace
    Buf<uint32_t> tile_keys{bufs}, tile_vals{bufs}, tile_keys_alt{bufs}, tile_vals_alt{bufs};
    // the strip's tile ranges; also as words (the per-pair form's range kernel)
    Buf<uint2> ranges_local{bufs};
    uint32_t *ranges_words() const { return reinterpret_cast<uint32_t *>(ranges_local.get()); }
    // column-first binning: the columns' starts in the column-sorted list, from the column
    // scatter, for the tile ranges the row pass computes (257 words, GsrTileStarts)
    Buf<uint32_t> col_starts{bufs};
    Buf<uint32_t> blend_order{bufs};  // the blend's tile groups, heaviest first
    // gsr_backward: the per-Gaussian 2D gradient rows (kGradRow floats each) the blend's backward
    // sums into, and the radii of the per-Gaussian stage it rebuilds
    Buf<float> grad2d{bufs};
    Buf<int32_t> bwd_radii{bufs};
    // gsr_backward_camera: the blocks' partial sums of the camera's 27 entries, [27][blocks]
    Buf<float> cam_partials{bufs};
    // gsr_backward_ordered, deterministic (gsr_internal.h GsrDetBwdArgs): the Gaussians' first
    // pairs (and the scan's block totals), the slots' sums (4 K x 9 or 10 floats, 11 or 12 under
    // gsr_backward_abs; never zeroed) and
    // their marks (4 K bytes, zeroed by every call); grown on demand, freed with the context
    Buf<uint64_t> det_slab{bufs}, det_partials{bufs};
    Buf<float> det_sums{bufs};
    Buf<uint8_t> det_marks{bufs};
    // ... and the events around its three stages (rebuild, blend backward, per-Gaussian backward)
    // of the last backward run under gsr_set_timing (created by the first one; gsr_backward_times)
    hipEvent_t ev_bwd[4] = {};
    bool bwd_timed = false;
    // frame graphs (64 B, from gsr_create): [0] tag, [1] list length, [4..6] campos
    Buf<uint32_t> frame_words{bufs};
    uint32_t *list_n() const { return frame_words.get() + 1; }
    // pinned host words the GPU stores into, and their device view
    GsrHostWords *host_words = nullptr, *d_host_words = nullptr;
    uint32_t sort_tag = 0;                  // frames rendered on this context (the pinned tags)
    // the bits of the last frame's kept depth keys' range and the bits in which they differ
    // (read_K); the first frame, with no history, takes the LSD sort, which any spread of depths
    // suits
    uint32_t last_Dr = UINT32_MAX, last_D = UINT32_MAX;
    // state of the last forward (gsr_get_binning, gsr_tile_row_pairs)
    struct LastFrame {
        bool valid = false;  // a forward has completed since the last one began
        int64_t K = 0;       // upstream's num_rendered
        int64_t list = 0;    // pairs in the list (tight binning: fewer than K)
        bool tight = false;
        uint32_t gx = 0, gy = 0, rb = 0, re = 0;
        uint32_t *point_list = nullptr, *tiles_local = nullptr;
        bool packed = false;             // column pairs: packed words, no tile-key array
        uint32_t id_mask = 0xFFFFFFFFu;  // packed word -> Gaussian id
    } last;
    // options (include/gsr.h)
    int cull = 1;
    int fast = 1;
    int depth_sort = -1;  // GSR_OPT_DEPTH_SORT
    int tight = 1;
    // stage timing: a ring of event sets, one per timed forward, read back after the timed region
    int timing = 0;        // 0 off, 1 every stage, 2 the blend only, on every 8th forward
    int64_t forwards = 0;  // forwards since gsr_set_timing (mode 2's sampling)
    int64_t timed_frames = 0;
    hipEvent_t ev[kTimingRing][kStages + 1] = {};
    hipEvent_t ev_color[kTimingRing][2] = {};
    // second stream: pair count and colour, between a fork after the preprocess and
    // a join before the blend.  Created on the first forward that uses it; GSR_OPT_SECOND_STREAM
    // 0 runs that work on the frame's stream and destroys it, freeing its hardware queue for
    // another frame in flight.  Normal priority, as the callers' streams: a stream's hardware
    // queue is picked when it is created among the queues of its priority, and a low-priority
    // second stream held one of the process's 4 queues apart from them, so four one-stream frame
    // streams created after it shared three (C3 depth 4: ~3,300-3,550 against ~4,090 frames/s,
    // profiles/r05y_stream_probe.txt, r05z2_ab_aux_priority.txt)
    int second_stream = 1;
    hipStream_t aux = nullptr;
    hipEvent_t fork = nullptr, join = nullptr;
    hipEvent_t compacted = nullptr;  // the compacted ids are written (main -> second stream)
    // frame graphs (GSR_OPT_FRAME_GRAPHS, DESIGN.md decision 12): the frame stream's chain after
    // the preprocess and the second stream's chain, each recorded once as a linear graph and
    // replayed while the key matches; the binning is sized by a capacity instead of the host
    // waiting for K in mid-frame
    int graphs = 0;
    uint32_t ws_gen = 0;                 // bumped by every (re)allocation of a workspace buffer
    int64_t list_cap = 0;                // pair-list capacity of the graphs (0: none yet)
    std::vector<GraphEntry> graph_cache;
    std::vector<hipGraphExec_t> graph_retired;
    uint64_t graph_clock = 0;
    int64_t graph_frames = 0, graph_records = 0, graph_overflows = 0;  // (gsr_graph_stats)
};

namespace {

// Orders this call after the context's previous workspace user when the caller switched streams
// (rare: a pipeline gives every stream its own context; a synchronisation only then).
int order_stream(gsr_context *ctx, hipStream_t s) {
    if (ctx->ws_stream_set && s != ctx->ws_stream)
        GSR_HIP(hipDeviceSynchronize(), "hipDeviceSynchronize(stream switch)");
    ctx->ws_stream = s;
    ctx->ws_stream_set = true;
    return GSR_OK;
}

// Grow-only device buffer.  Both streams are drained first so no in-flight kernel still reads
// the old allocation.
int grow(gsr_context *ctx, DevBuf &b, size_t bytes, hipStream_t s) {
    if (bytes <= b.cap) return GSR_OK;
    size_t want = std::max(bytes, b.cap + b.cap / 2);
    want = (want + 255) & ~size_t(255);
    if (b.p) {
        GSR_HIP(hipStreamSynchronize(s), "hipStreamSynchronize(grow)");
        if (ctx->aux) GSR_HIP(hipStreamSynchronize(ctx->aux), "hipStreamSynchronize(grow)");
        GSR_HIP(hipFree(b.p), "hipFree");
        b.p = nullptr;
        b.cap = 0;
    }
    ++ctx->ws_gen;  // recorded frame graphs hold the old pointers
    if (hipMalloc(&b.p, want) != hipSuccess) {
        (void)hipGetLastError();
        b.p = nullptr;
        return fail(GSR_E_NOMEM, "hipMalloc of " + std::to_string(want) + " bytes failed");
    }
    b.cap = want;
    return GSR_OK;
}

int reserve_P(gsr_context *ctx, int64_t P, hipStream_t s) {
    const size_t n = (size_t)std::max<int64_t>(P, 1);
    GSR_TRY(grow(ctx, ctx->records, n * sizeof(gsr::SplatRecord), s));
    GSR_TRY(grow(ctx, ctx->strip_rect, n * 8, s));
    GSR_TRY(grow(ctx, ctx->sort_keys, n * 4, s));
    GSR_TRY(grow(ctx, ctx->ds_a, n * 8, s));
    GSR_TRY(grow(ctx, ctx->ds_b, n * 8, s));
    GSR_TRY(grow(ctx, ctx->block_kept, 4 * ((n + 255) / 256), s));
    GSR_TRY(grow(ctx, ctx->partials, (size_t)std::max<int64_t>(gsr_scan_blocks(P), 1) * 4, s));
    GSR_TRY(grow(ctx, ctx->total, 16, s));
    // per preprocess block: its pair count (8 B) and kept-key OR / AND (8 B)
    GSR_TRY(grow(ctx, ctx->pair_count, (size_t)std::max<int64_t>(gsr_preprocess_blocks(P), 1) * 16, s));
    GSR_TRY(grow(ctx, ctx->hist, (size_t)std::max(gsr_radix_hist_words(P),
                                                  gsr_depth_sort_hist_words(P)) * 4, s));
    // column-first binning's per-(block, column) counts: its own buffer, since reserve_K may
    // regrow hist between the count and the scatter
    GSR_TRY(grow(ctx, ctx->col_hist, (size_t)std::max<int64_t>(gsr_col_blocks(P), 1) * 256 * 4, s));
    // 256 words per radix pass; the depth sort's 4096 digits
    GSR_TRY(grow(ctx, ctx->digit_total,
                 (size_t)std::max(256 * GSR_RADIX_MAX_PASSES, gsr_depth_sort_digit_words()) * 4, s));
    GSR_TRY(grow(ctx, ctx->perm, n * 4, s));
    GSR_TRY(grow(ctx, ctx->ds_ctl, (size_t)gsr_depth_sort_ctl_words(P) * 4, s));
    GSR_TRY(grow(ctx, ctx->bin, n * 16, s));
    GSR_TRY(grow(ctx, ctx->rect_sorted, n * 8, s));
    GSR_TRY(grow(ctx, ctx->strip_rc, n * 16, s));
    GSR_TRY(grow(ctx, ctx->rc_sorted, n * 16, s));
    return GSR_OK;
}

int reserve_K(gsr_context *ctx, int64_t K, hipStream_t s) {
    const size_t n = (size_t)std::max<int64_t>(K, 1);
    GSR_TRY(grow(ctx, ctx->tile_keys, n * 4, s));
    GSR_TRY(grow(ctx, ctx->tile_vals, n * 4, s));
    GSR_TRY(grow(ctx, ctx->tile_keys_alt, n * 4, s));
    GSR_TRY(grow(ctx, ctx->tile_vals_alt, n * 4, s));
    GSR_TRY(grow(ctx, ctx->hist, (size_t)gsr_radix_hist_words(K) * 4, s));
    GSR_TRY(grow(ctx, ctx->chunk_first, (size_t)(gsr_duplicate_chunks(K) + 1) * 4, s));
    return GSR_OK;
}

int bits_for(uint64_t max_value) {  // bits needed to represent every value <= max_value
    int b = 0;
    while (b < 32 && (max_value >> b) != 0) ++b;
    return b;
}

// Spin on a pinned word the GPU stores (system scope) until pred(value) holds; false after
// kSpinLimit.  A sleeping event wait adds wake-up jitter to every frame (and its record a host
// call); the spin keeps one host core busy for the frame's first ~20-50 us.
template <typename Pred>
bool spin_on(const unsigned long long *word, Pred pred, uint64_t &value) {
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t spin = 0;; ++spin) {
        value = __atomic_load_n(word, __ATOMIC_ACQUIRE);
        if (pred(value)) return true;
        if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > kSpinLimit)
            return false;
    }
}

uint64_t host_word(const unsigned long long &word) {  // (GsrHostWords, on the host)
    return __atomic_load_n(&word, __ATOMIC_ACQUIRE);
}

// Everything one forward derives from its arguments, shared by the stage functions.
struct Frame {
    hipStream_t s;
    int64_t P;
    int W, H;
    uint32_t gx, gy, rb, re, rows_tiles;  // tile grid; strip tile rows [rb, re)
    int y0, rows_out;                     // strip pixel rows
    uint64_t T_strip;
    bool dbg;
    int tmode;  // this forward's timing: 0 none, 1 every stage, 2 the blend
    hipEvent_t *ev, *evc;
    bool compact_sort;  // the depth sort compacts the kept keys first
    bool msd_sort;      // the depth sort's MSD pass + per-bucket local sort (else LSD passes)
    bool main_publish;  // K is published on the main stream (with the MSD sort's D), not the
                        // second
    bool color_ids;     // the colour pass walks the compacted ids
    bool colpairs;      // column-first binning (else the per-pair form)
    bool graph = false;  // this forward replays recorded frame graphs (forward_graph)
    int col_shift;      // column pairs: packed word = strip row << col_shift | Gaussian id
    uint32_t tag;       // this frame's tag for the pinned words
    bool wide_local;    // the MSD local sort's 8192-slot form (crowded buckets lately)
    GsrPreprocessArgs pa;
    bool tight;  // tight binning: pairs only over the span words (needs the column-first form)
    int shading = GSR_SHADE_SPLAT;  // gsr_forward_shaded: the kernel of stage 7
    // gsr_forward_depth: the planes stage 7 also fills (both NULL: the plain composite)
    float *depth_map = nullptr, *inv_depth_map = nullptr;
    // gsr_forward_surface: the median planes stage 7 also fills (both NULL: none)
    float *median_depth = nullptr;
    int32_t *median_id = nullptr;
    // gsr_forward_features: the planes stage 7's feature launches fill (feature_map NULL: none)
    int feat_C = 0;
    const float *features = nullptr;
    float *feature_map = nullptr;
    bool no_blend = false;  // gsr_backward's rebuild: everything up to the lists, no stage 7
    uint64_t K = 0;   // upstream's num_rendered
    uint64_t KL = 0;  // pairs in the list (K, or fewer with tight binning)
    // the pair list the blend reads and gsr_get_binning exports
    uint32_t *point_list = nullptr, *tiles_local = nullptr;
    uint32_t id_mask = 0xFFFFFFFFu;
};

// What a call asks of its frame beyond the plain composite: every forward entry point, and
// gsr_backward's rebuild, is forward() with one of these.  setup_frame copies it into the Frame,
// so the overflow re-render carries the same state as the first attempt.
struct FrameRequest {
    int shading = GSR_SHADE_SPLAT;
    const gsr_depth_outputs *depth = nullptr;      // NULL: no depth planes
    const gsr_surface_outputs *surface = nullptr;  // NULL: no median planes
    // gsr_forward_filtered: the call's, not the context's; the preprocess runs outside the
    // recorded chains (which read none of its opacity-dependent arguments), so plain and
    // antialiased frames share their graphs
    bool antialiasing = false;
    bool no_blend = false;
    const gsr_feature_outputs *feat = nullptr;  // NULL, or checked by gsr_forward_features
};

int stage_end(gsr_context *ctx, const Frame &f, int i) {
    if (f.tmode == 1 || (f.tmode == 2 && i >= 5))
        GSR_HIP(hipEventRecord(f.ev[i + 1], f.s), "hipEventRecord");
    if (f.dbg) {
        GSR_HIP(hipStreamSynchronize(f.s), std::string("stage ") + kStageNames[i]);
        GSR_HIP(hipGetLastError(), std::string("stage ") + kStageNames[i]);
    }
    (void)ctx;
    return GSR_OK;
}

// Arguments -> Frame (upstream's argument checks and messages, rasterize_points.cu /
// __init__.py), workspace for P.
int setup_frame(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                gsr_outputs *out, hipStream_t s, const FrameRequest &rq, Frame &f) {
    const int64_t P = g->P;
    const int W = st->image_width, H = st->image_height;
    if (P < 0 || P > (int64_t)UINT32_MAX) return fail(GSR_E_INVALID, "gsr_forward: bad P");
    if (W <= 0 || H <= 0) return fail(GSR_E_INVALID, "gsr_forward: image size must be positive");
    const bool strip = st->tile_row_begin != 0 || st->tile_row_end != 0;
    const bool per_gaussian = out->depths || out->means2D || out->conic_opacity || out->rgb ||
                              out->tiles_touched;
    if (!out->color || (P > 0 && !out->radii && (!strip || per_gaussian)))
        return fail(GSR_E_INVALID, "gsr_forward: color and radii outputs are required (radii "
                                   "may be NULL only on a strip without per-Gaussian outputs)");
    if (P > 0) {
        if (!g->means3D || !g->opacities)
            return fail(GSR_E_INVALID, "gsr_forward: means3D and opacities are required");
        if ((g->shs == nullptr) == (g->colors_precomp == nullptr))
            return fail(GSR_E_INVALID,
                        "Please provide excatly one of either SHs or precomputed colors!");
        if (((g->scales == nullptr || g->rotations == nullptr) && g->cov3D_precomp == nullptr) ||
            ((g->scales != nullptr || g->rotations != nullptr) && g->cov3D_precomp != nullptr))
            return fail(GSR_E_INVALID, "Please provide exactly one of either scale/rotation pair "
                                       "or precomputed 3D covariance!");
        if (g->shs && (g->M <= 0 || g->D < 0 || g->D > 3 || (g->D + 1) * (g->D + 1) > g->M))
            return fail(GSR_E_INVALID, "gsr_forward: sh_degree " + std::to_string(g->D) +
                                           " needs (deg+1)^2 <= " + std::to_string(g->M) +
                                           " stored coefficients (deg <= 3)");
        if (!st->viewmatrix || !st->projmatrix || (g->shs && !st->campos))
            return fail(GSR_E_INVALID, "gsr_forward: camera matrices are required");
    }
    if (!st->bg) return fail(GSR_E_INVALID, "gsr_forward: bg is required");
    if (out->conic_opacity && (reinterpret_cast<uintptr_t>(out->conic_opacity) & 15) != 0)
        return fail(GSR_E_INVALID, "gsr_forward: conic_opacity output must be 16-B aligned");

    f.s = s;
    f.shading = rq.shading;
    if (rq.depth) f.depth_map = rq.depth->depth_map, f.inv_depth_map = rq.depth->inv_depth_map;
    if (rq.surface)
        f.median_depth = rq.surface->median_depth, f.median_id = rq.surface->median_id;
    if (rq.feat && rq.feat->feature_map)
        f.feat_C = rq.feat->C, f.features = rq.feat->features, f.feature_map = rq.feat->feature_map;
    f.no_blend = rq.no_blend;
    f.P = P;
    f.W = W;
    f.H = H;
    f.gx = (uint32_t)((W + GSR_TILE_X - 1) / GSR_TILE_X);
    f.gy = (uint32_t)((H + GSR_TILE_Y - 1) / GSR_TILE_Y);
    if (f.gx > 0xFFFFu || f.gy > 0xFFFFu)  // packed 16-bit tile rects (preprocess.hip)
        return fail(GSR_E_INVALID, "gsr_forward: image larger than 65535 tiles per side");
    f.rb = 0;
    f.re = f.gy;
    if (st->tile_row_begin != 0 || st->tile_row_end != 0) {
        if (st->tile_row_begin < 0 || st->tile_row_end > (int)f.gy ||
            st->tile_row_begin >= st->tile_row_end)
            return fail(GSR_E_INVALID, "gsr_forward: bad tile row strip");
        f.rb = (uint32_t)st->tile_row_begin;
        f.re = (uint32_t)st->tile_row_end;
    }
    f.rows_tiles = f.re - f.rb;
    f.y0 = (int)(f.rb * GSR_TILE_Y);
    f.rows_out = std::min(H, (int)(f.re * GSR_TILE_Y)) - f.y0;
    f.T_strip = (uint64_t)f.gx * f.rows_tiles;
    f.dbg = st->debug != 0;
    f.ev = ctx->ev[ctx->timed_frames % kTimingRing];
    f.evc = ctx->ev_color[ctx->timed_frames % kTimingRing];
    f.tmode = ctx->timing == 1 ? 1 : (ctx->timing == 2 && ctx->forwards++ % 8 == 0) ? 2 : 0;

    // column-first binning: the column pass ranks <= 256 columns, the row pass is one 8-bit
    // pass (whose scanned histogram gives the tile ranges) and the packed word holds the strip
    // row and the id
    const int ybits = f.rows_tiles > 1 ? bits_for(f.rows_tiles - 1) : 0;
    f.col_shift = 32 - ybits;
    f.colpairs = f.gx <= 256 && f.rows_tiles <= 256 &&
                 (f.col_shift == 32 || (uint64_t)P <= (1ull << f.col_shift));

    GSR_TRY(reserve_P(ctx, P, s));
    GSR_TRY(grow(ctx, ctx->ranges_local, (size_t)std::max<uint64_t>(f.T_strip, 1) * 8, s));
    if (f.colpairs) {
        GSR_TRY(grow(ctx, ctx->col_starts, 257 * 4, s));
        GSR_TRY(grow(ctx, ctx->blend_order,
                     (size_t)gsr_blend_order_groups((uint32_t)f.T_strip) * 4, s));
    }

    GsrPreprocessArgs &pa = f.pa;
    pa = GsrPreprocessArgs{};
    pa.P = P;
    pa.D = g->D;
    pa.M = g->M;
    pa.scale_modifier = g->scale_modifier;
    pa.means3D = g->means3D;
    pa.scales = g->scales;
    pa.rotations = g->rotations;
    pa.opacities = g->opacities;
    pa.shs = g->shs;
    pa.colors_precomp = g->colors_precomp;
    pa.cov3D_precomp = g->cov3D_precomp;
    pa.viewmatrix = st->viewmatrix;
    pa.projmatrix = st->projmatrix;
    pa.campos = st->campos;
    pa.tanfovx = st->tanfovx;
    pa.tanfovy = st->tanfovy;
    // rasterizer_impl.cu: focal_y = height / (2.0f * tan_fovy); focal_x likewise (float).
    pa.focal_y = (float)H / (2.0f * st->tanfovy);
    pa.focal_x = (float)W / (2.0f * st->tanfovx);
    pa.W = W;
    pa.H = H;
    pa.grid_x = f.gx;
    pa.grid_y = f.gy;
    pa.row_begin = f.rb;
    pa.row_end = f.re;
    pa.prefiltered = st->prefiltered;
    pa.antialiasing = rq.antialiasing ? 1 : 0;
    pa.sh_vec4 = (g->shs && g->M == 16 && (reinterpret_cast<uintptr_t>(g->shs) & 15) == 0) ? 1 : 0;
    pa.rot_vec4 = (g->rotations && (reinterpret_cast<uintptr_t>(g->rotations) & 15) == 0) ? 1 : 0;
    pa.radii = out->radii;
    pa.strip_skip = out->radii == nullptr ? 1 : 0;
    pa.records = ctx->records.get();
    pa.sort_keys = ctx->sort_keys.get();
    f.compact_sort = ctx->depth_sort < 0 ? (f.rows_tiles < f.gy && P >= kCompactP)
                                         : ctx->depth_sort == 1 || ctx->depth_sort == 3;
    pa.block_kept = f.compact_sort ? ctx->block_kept.get() : nullptr;
    // the MSD sort wants buckets of a few thousand keys: its 4096 buckets split the top 12 bits of
    // the kept keys' range (key - min), which balances them while the depths span a few float
    // exponents (Dr <= 25: C2, C3, C5 -- whose near Gaussians cross depth 2.0, D = 31 but Dr =
    // 24-25; C5 in flight +4 %, profiles/r05q_ab_range_msd.txt); wider ranges crowd some buckets
    // past the LDS sort (c3r, Dr = 26: serial 0.313 -> 0.340 ms), so they keep the LSD passes --
    // except on one-stream frames in flight, where the single pass wins (kMsdMaxDOneStream).
    // The choice follows the previous frame's range (the result is the same either way, only the
    // time differs)
    f.msd_sort = ctx->depth_sort < 0
                     ? ctx->last_Dr <= (ctx->second_stream ? kMsdMaxD : kMsdMaxDOneStream)
                     : ctx->depth_sort >= 2;
    // (compacted strips keep the second stream's publish: on the C4 1/8 strip the main-stream
    // publish let the tile counts and colour start earlier, beside the depth sort, 80 -> 134 us)
    f.main_publish = f.msd_sort && !f.compact_sort;
    pa.strip_rect = ctx->strip_rect.get();
    // tight binning: the column-first form, and no n_contrib (upstream's n_contrib counts list
    // positions of the full 3-sigma pairs); span words only then (NULL: every rect full).  Full
    // frames only: on a strip the replicated preprocess writes a 16-B record for every Gaussian
    // to shorten one strip's lists (C4 3/8 strip: preprocess 97 -> 141 us, row pass 52 -> 42 us;
    // C3 3/8 strip 0.150 -> 0.157 ms per frame; DESIGN.md decision 11)
    // Never under the billboard shading: its quads reach beyond the alpha >= 1/255 ellipse the
    // span words are cut to (they stay inside upstream's rect: radius = ceil(3 sqrt(lambda_max))
    // >= 3 sqrt(max(cxx, cyy))), so it reads upstream's lists.  The other prunings hold for it
    // as they are: the blend's quadrant cull has its own box test (blend.hip k_shade_q), and the
    // strip ranks' footprint skip (preprocess.hip strip_reach) bounds upstream's rect, not the
    // ellipse, and reads no opacity.
    f.tight = ctx->tight && f.colpairs && !out->n_contrib && f.rows_tiles == f.gy &&
              rq.shading != GSR_SHADE_BILLBOARD;
    pa.strip_rc = f.tight ? ctx->strip_rc.get() : nullptr;
    pa.block_pairs = ctx->pair_count.get();
    pa.host_words = ctx->d_host_words;
    pa.depths = out->depths;
    pa.means2D = out->means2D;
    pa.conic_opacity = out->conic_opacity;
    pa.rgb = out->rgb;
    pa.tiles_touched = out->tiles_touched;
    // compacted strip frames: the colour pass walks the depth sort's compacted kept ids
    // (k_color_ids) instead of every Gaussian's rect -- at a 1/8 strip of 6M Gaussians a lane
    // in ~8 had a row to read
    f.color_ids = f.compact_sort && gsr_color_ids_ok(pa);
    if (f.color_ids) GSR_TRY(grow(ctx, ctx->color_ids, (size_t)P * 4, s));
    f.tag = ++ctx->sort_tag;
    if (f.tag == 0) f.tag = ++ctx->sort_tag;  // 0 is the pinned words' initial value
    pa.k_tag = f.tag;
    // the local sort's wide form while one of the last kCrowdFrames frames' sorts found buckets
    // of 513-1024 keys crowding a group past 4096 LDS slots (the flag of the frame before this
    // one may not have landed yet: the form is only a speed choice)
    {
        const uint32_t crowd = (uint32_t)host_word(ctx->host_words->crowd);
        f.wide_local = crowd != 0u && f.tag - crowd <= kCrowdFrames;
    }
    return GSR_OK;
}

// ---- 2. the stable depth sort of the Gaussians (depth_sort.hip), passes [p0, p1) ------------
int launch_depth_sort(gsr_context *ctx, const Frame &f, int p0, int p1) {
    uint32_t *hist = ctx->hist.get(), *digit_total = ctx->digit_total.get();
    uint32_t *ctl = ctx->ds_ctl.get(), *perm = ctx->perm.get();
    uint2 *ds_a = ctx->ds_a.get(), *ds_b = ctx->ds_b.get();
    unsigned long long *host_D = &ctx->d_host_words->sort_D;
    hipError_t e;
    const int64_t nb = gsr_preprocess_blocks(f.P);  // (their key OR / AND words)
    const uint2 *keybits = reinterpret_cast<const uint2 *>(f.pa.block_pairs + nb);
    if (f.compact_sort) {
        // the compacted keys / ids live in ds_b until pass 1 (or the MSD pass) has read them
        if (f.msd_sort && p0 != 0) return GSR_OK;  // (no later passes)
        uint32_t *keys_c = ctx->ds_b_words(), *ids_c = keys_c + f.P;
        e = gsr_depth_sort_compacted(f.pa.sort_keys, f.P, f.pa.block_kept, keys_c, ids_c, ds_a,
                                     ds_b, perm, hist, digit_total, ctl, p0, p1, f.s, host_D,
                                     f.tag, f.color_ids ? ctx->color_ids.get() : nullptr,
                                     f.color_ids ? ctx->compacted : nullptr, f.msd_sort ? 1 : 0,
                                     f.msd_sort && !f.main_publish ? keybits : nullptr, nb);
    } else if (f.msd_sort) {
        // MSD pass + per-bucket local sort, the whole sort at once (D from the preprocess blocks)
        if (p0 != 0) return GSR_OK;  // (no later passes)
        e = gsr_depth_sort_msd(f.pa.sort_keys, f.P, f.main_publish ? nullptr : keybits, nb,
                               ds_a, ds_b, perm, hist, digit_total, ctl, f.s,
                               f.graph ? nullptr : host_D, f.tag,
                               f.graph ? nullptr : &ctx->d_host_words->crowd,
                               f.graph ? 0 : f.wide_local);
    } else {  // (frame graphs queue every pass; the host reads no D)
        e = gsr_depth_sort(f.pa.sort_keys, f.P, 1, ds_a, ds_b, perm, hist, digit_total, ctl, p0,
                           p1, f.s, f.graph ? nullptr : host_D, f.tag);
    }
    GSR_HIP(e, "depth sort launch");
    return GSR_OK;
}

// colour waves per SIMD (gsr_launch_color): 2 on a full frame, so the colour leaves the CUs
// to the binning chain it overlaps (C3 two frames in flight 3,890-3,918 -> 3,947-3,954
// frames/s, serial 0.317 -> 0.308 ms; C4 serial 2.09 -> 2.06 ms); 3 on a compacted strip
// (C4 1/8 strip 0.481 -> 0.468 ms).  profiles/r04n_ab_color_waves.txt, DESIGN.md decision 7.
// 4 on a strip that is not compacted: its waves scan every Gaussian and only ~1 lane in 8 has
// a colour to compute, so more of them hide the row loads' latency (C3 strips +2-3 %, colour
// 49 -> 44 us, profiles/r06x_ab_strip_colour_cap.txt).
constexpr int kColorWavesFull = 2, kColorWavesCompacted = 3, kColorWavesStrip = 4;
int color_waves_of(const Frame &f) {
    if (f.color_ids) return kColorWavesCompacted;
    return f.rows_tiles < f.gy ? kColorWavesStrip : kColorWavesFull;
}

// ---- the second stream: K, the colour -----------------------------------------------------
// The second stream's kernels on stream `as` (a frame graph records them on its capture
// stream; d_tag then names the device word holding the frame's tag).
constexpr int kAuxPublish = 1, kAuxColor = 2;  // aux_chain's parts
int aux_chain(gsr_context *ctx, const Frame &f, hipStream_t as, const uint32_t *d_tag,
              int parts = kAuxPublish | kAuxColor) {
    // K first: k_publish_K sums the preprocess blocks' counts into pinned memory; the host
    // waits for it only after the depth sort and the column counts are queued (MSD frames
    // publish on the main stream instead, with the sort's D)
    if (parts & kAuxPublish) {
        if (!f.main_publish)
            GSR_HIP(gsr_launch_count_pairs(f.pa, as, nullptr, d_tag), "pair count launch");
        if (f.tmode == 1) GSR_HIP(hipEventRecord(f.evc[0], as), "hipEventRecord");
    }
    if (!(parts & kAuxColor)) return GSR_OK;
    const int color_waves = color_waves_of(f);
    if (f.color_ids) {
        GSR_HIP(hipStreamWaitEvent(as, ctx->compacted, 0), "hipStreamWaitEvent(compacted)");
        GSR_HIP(gsr_launch_color_ids(f.pa, ctx->color_ids.get(), ctx->ds_ctl.get(), color_waves,
                                     as),
                "color launch");
    } else {
        GSR_HIP(gsr_launch_color(f.pa, color_waves, as), "color launch");
    }
    if (f.tmode == 1) GSR_HIP(hipEventRecord(f.evc[1], as), "hipEventRecord");
    return GSR_OK;
}

// The colour of a column-first frame starts on the second stream once the depth sort is done, so
// that it runs beside the column count, the column scatter and the row pass rather than beside
// the depth sort, which it slows more (C4 serial: depth sort 226 -> 420 us with the colour beside
// it; the tile-count pass that used to precede the colour on this stream delayed it as long).
bool color_after_sort(const gsr_context *ctx, const Frame &f) {
    return ctx->second_stream && f.colpairs;
}

int launch_second_stream(gsr_context *ctx, const Frame &f) {
    if (!ctx->second_stream) return aux_chain(ctx, f, f.s, nullptr);  // in order, same stream
    hipStream_t as = ctx->aux;
    GSR_HIP(hipStreamWaitEvent(as, ctx->fork, 0), "hipStreamWaitEvent(fork)");
    GSR_TRY(aux_chain(ctx, f, as, nullptr,
                      color_after_sort(ctx, f) ? kAuxPublish : kAuxPublish | kAuxColor));
    GSR_HIP(hipEventRecord(ctx->join, as), "hipEventRecord(join)");
    if (f.dbg) GSR_HIP(hipStreamSynchronize(as), "stage color");
    return GSR_OK;
}

// ... and the colour behind the depth sort (color_after_sort frames): the fork event is
// recorded again, after the sort's last pass, for the second stream to wait on.
int launch_color_after_sort(gsr_context *ctx, const Frame &f) {
    if (!color_after_sort(ctx, f)) return GSR_OK;
    hipStream_t as = ctx->aux;
    GSR_HIP(hipEventRecord(ctx->fork, f.s), "hipEventRecord(sorted)");
    GSR_HIP(hipStreamWaitEvent(as, ctx->fork, 0), "hipStreamWaitEvent(sorted)");
    GSR_TRY(aux_chain(ctx, f, as, nullptr, kAuxColor));
    GSR_HIP(hipEventRecord(ctx->join, as), "hipEventRecord(join)");
    if (f.dbg) GSR_HIP(hipStreamSynchronize(as), "stage color");
    return GSR_OK;
}

// ---- 3. the scan: per-column pair counts of the depth-sorted Gaussians (column pairs), or the
// offsets scan over their strip tile counts (per-pair form) --------------------------------------
int launch_scan(gsr_context *ctx, const Frame &f) {
    const uint32_t *perm = ctx->perm.get(), *d_valid = ctx->ds_ctl.get();
    uint2 *rect_sorted = ctx->rect_sorted.get();
    if (f.colpairs) {
        GSR_HIP(gsr_launch_col_pairs_count(perm, f.pa.strip_rect, f.pa.strip_rc, f.P, d_valid,
                                           rect_sorted, f.tight ? ctx->rc_sorted.get() : nullptr,
                                           ctx->col_hist.get(), ctx->digit_total.get(), f.s),
                "column count launch");
    } else {
        uint32_t *partials = ctx->partials.get();
        GSR_HIP(gsr_launch_scan_reduce(perm, f.pa.strip_rect, f.P, d_valid, partials,
                                       rect_sorted, f.s),
                "scan launch");
        GSR_HIP(gsr_launch_scan_partials(partials, gsr_scan_blocks(f.P), ctx->total.get(), f.s),
                "scan launch");
    }
    return GSR_OK;
}

// The frame graphs' list capacity for a list of n entries (capacity cap so far): a quarter more,
// at least kMinListCap, 4096-aligned (the row pass's tiles), and at least 1.5x the old one.
int64_t list_capacity(int64_t n, int64_t cap) {
    int64_t c = std::max({n + n / 4, kMinListCap, cap + cap / 2});
    c = (c + 4095) & ~(int64_t)4095;
    return std::min<int64_t>(c, (int64_t)UINT32_MAX - 4096);
}

// The frame's K, list length, D and Dr from the pinned words k_publish_K stores: the host spins
// on the frame's tag and, past the spin limit, waits for the stream that publishes.
hipStream_t publish_stream(const gsr_context *ctx, const Frame &f) {
    return f.main_publish || !ctx->second_stream ? f.s : ctx->aux;
}
int read_K(gsr_context *ctx, Frame &f, hipStream_t publisher) {
    const GsrHostWords *w = ctx->host_words;
    uint64_t tagv = 0;
    if (!spin_on(&w->K_tag, [&](uint64_t v) { return v == f.tag; }, tagv))
        GSR_HIP(hipStreamSynchronize(publisher), "hipStreamSynchronize(pair count)");
    f.K = host_word(w->K);
    ctx->last_Dr = (uint32_t)host_word(w->Dr);
    ctx->last_D = (uint32_t)host_word(w->D);
    f.KL = f.tight ? host_word(w->K_spans) : f.K;
    if (f.K > (uint64_t)UINT32_MAX - 4096)
        return fail(GSR_E_INVALID, "gsr_forward: more than 2^32-4097 (Gaussian, tile) pairs");
    return GSR_OK;
}

// K (the pair count, which sizes the binning) from k_publish_K on the second stream, published
// in pinned memory ~20 us after the preprocess.  Debug mode also checks it against the depth
// sort's own key bits and, in the per-pair form, against the offsets scan's total.
int wait_K(gsr_context *ctx, Frame &f) {
    GSR_TRY(read_K(ctx, f, publish_stream(ctx, f)));
    if (f.dbg) {
        uint32_t ctl2[2];
        uint64_t scan_K[2] = {0, 0};
        GSR_HIP(hipMemcpyAsync(ctl2, ctx->ds_ctl.get(), 8, hipMemcpyDeviceToHost, f.s),
                "hipMemcpyAsync(ctl)");
        if (!f.colpairs)
            GSR_HIP(hipMemcpyAsync(scan_K, ctx->total.get(), 16, hipMemcpyDeviceToHost, f.s),
                    "hipMemcpyAsync(num_rendered)");
        GSR_HIP(hipStreamSynchronize(f.s), "hipStreamSynchronize(ctl)");
        if (ctl2[1] != ctx->last_D)
            return fail(GSR_E_HIP, "gsr_forward: depth key bits mismatch (pair count " +
                                       std::to_string(ctx->last_D) + ", sort " +
                                       std::to_string(ctl2[1]) + ")");
        if (!f.colpairs && scan_K[0] != f.K)
            return fail(GSR_E_HIP, "gsr_forward: pair count mismatch (preprocess " +
                                       std::to_string(f.K) + ", scan " +
                                       std::to_string(scan_K[0]) + ")");
    }
    // column-first frames also size the frame graphs' list capacity (before the binning, so
    // this frame's list is not reallocated under it)
    int64_t want = (int64_t)f.KL;
    if (ctx->graphs && f.colpairs && want > ctx->list_cap) {
        ctx->list_cap = list_capacity(want, ctx->list_cap);
        want = ctx->list_cap;
    }
    return reserve_K(ctx, want, f.s);
}

// The packed pair word's Gaussian id bits (column-first binning: strip row << col_shift | id).
uint32_t id_mask_of(int col_shift) {
    return col_shift < 32 ? (1u << col_shift) - 1u : 0xFFFFFFFFu;
}

// ---- 4 + 5, column-first form: pass 1 by column on (Gaussian, column) segments, then pass 2 on
// the packed words' row bits, keys only; on f.s, the list it ends in and its id mask into f.
// n: the list's length, known to the host, or with list_n (deferred-K frames) the capacity the
// list is binned into, its length stored to and read from that device word.
//
// The tile ranges and the blend's tile-group order come from the row pass itself: its scanned
// histogram and the column starts the scatter kept give every tile's start, and the leading
// blocks of its downsweep write them (radix_sort.hip, GsrTileStarts); a one-block kernel behind
// it orders the tile groups.  A strip of one tile row has no row pass (its tiles are the column
// runs) and an empty list has all-zero ranges: one small kernel writes those and the order.
int launch_col_binning(gsr_context *ctx, Frame &f, int64_t n, uint32_t *list_n) {
    uint32_t *tv = ctx->tile_vals.get(), *tv_alt = ctx->tile_vals_alt.get();
    uint32_t *col_starts = ctx->col_starts.get();
    if (n > 0)
        GSR_HIP(gsr_launch_col_pairs_scatter(ctx->perm.get(), ctx->rect_sorted.get(),
                                             f.tight ? ctx->rc_sorted.get() : nullptr, f.P,
                                             ctx->ds_ctl.get(), ctx->col_hist.get(),
                                             ctx->digit_total.get(), f.col_shift, tv_alt,
                                             col_starts, f.s,
                                             list_n ? (uint32_t)n : 0xFFFFFFFFu, list_n),
                "column scatter launch");
    std::swap(tv, tv_alt);
    GSR_TRY(stage_end(ctx, f, 3));
    const GsrTileStarts ts{col_starts, f.gx, f.rows_tiles, ctx->ranges_local.get(),
                           ctx->blend_order.get()};
    if (n > 0 && f.col_shift < 32)  // (hist: after reserve_K)
        GSR_HIP(gsr_radix_sort_keys(&tv, &tv_alt, n, f.col_shift, 32, ctx->hist.get(),
                                    ctx->digit_total.get(), f.s, list_n, &ts),
                "tile sort launch");
    else
        GSR_HIP(gsr_launch_tile_runs(n, list_n, ts, f.s), "tile ranges launch");
    GSR_TRY(stage_end(ctx, f, 4));
    f.point_list = tv;
    f.tiles_local = nullptr;
    f.id_mask = id_mask_of(f.col_shift);
    return GSR_OK;
}

// ---- 4 + 5. the pairs, stably sorted by strip tile ------------------------------------------
int launch_binning(gsr_context *ctx, Frame &f) {
    const int64_t K = (int64_t)f.KL;
    if (f.colpairs) return launch_col_binning(ctx, f, K, nullptr);
    const uint32_t *perm = ctx->perm.get(), *d_valid = ctx->ds_ctl.get();
    uint32_t *hist = ctx->hist.get(), *digit_total = ctx->digit_total.get();  // (after reserve_K)
    uint32_t *tk = ctx->tile_keys.get(), *tv = ctx->tile_vals.get();
    uint32_t *tk_alt = ctx->tile_keys_alt.get(), *tv_alt = ctx->tile_vals_alt.get();
    // per-pair form: offsets, then the duplication fused with the first tile-sort pass (which
    // also zeroes the ranges), then the remaining passes and the ranges over the sorted keys
    const int tbits = f.T_strip > 1 ? bits_for(f.T_strip - 1) : 0;
    const GsrRadixPlan plan = gsr_radix_plan(0, tbits);
    if (K > 0) {
        GSR_HIP(gsr_launch_scan_down(perm, ctx->rect_sorted.get(), ctx->partials.get(), f.P,
                                     d_valid, ctx->total.get(), ctx->bin.get(),
                                     ctx->chunk_first.get(), f.s),
                "scan_down launch");
        GSR_HIP(gsr_launch_dup_sort_pass(ctx->bin.get(), ctx->chunk_first.get(), K, f.gx,
                                         plan.n ? plan.shift[0] : 0, plan.n ? plan.nbits[0] : 0,
                                         hist, digit_total, tk_alt, tv_alt,
                                         ctx->ranges_local.get(), (uint32_t)f.T_strip, f.s),
                "duplicate launch");
        std::swap(tk, tk_alt);
        std::swap(tv, tv_alt);
    }
    GSR_TRY(stage_end(ctx, f, 3));
    if (K > 1)
        GSR_HIP(gsr_radix_sort_pairs(&tk, &tv, &tk_alt, &tv_alt, K, 0, tbits, hist, digit_total,
                                     f.s, 1),
                "tile sort launch");
    GSR_TRY(stage_end(ctx, f, 4));
    if (K == 0)
        GSR_HIP(hipMemsetAsync(ctx->ranges_words(), 0, f.T_strip * 8, f.s),
                "hipMemsetAsync(ranges)");
    GSR_HIP(gsr_launch_ranges(tk, K, ctx->ranges_words(), f.s), "ranges launch");
    f.point_list = tv;
    f.tiles_local = tk;
    f.id_mask = 0xFFFFFFFFu;
    return GSR_OK;
}

// ---- 7. blend ----------------------------------------------------------------------------------
int launch_blend(gsr_context *ctx, const Frame &f, const gsr_raster_settings *st,
                 gsr_outputs *out) {
    GsrBlendArgs ba{};
    ba.ranges = ctx->ranges_local.get();
    ba.point_list = f.point_list;
    ba.records = f.pa.records;
    ba.W = f.W;
    ba.H = f.H;
    ba.grid_x = f.gx;
    ba.row_begin = f.rb;
    ba.rows_tiles = f.rows_tiles;
    ba.y0 = f.y0;
    ba.rows_out = f.rows_out;
    ba.bg = st->bg;
    ba.out_color = out->color;
    ba.final_T = out->final_T;
    ba.n_contrib = out->n_contrib;
    ba.cull = ctx->cull;
    ba.fast = ctx->fast;
    ba.id_mask = f.id_mask;
    ba.order = f.colpairs ? ctx->blend_order.get() : nullptr;  // (per-pair form: row-major)
    if (f.graph) {  // the list length is on the device: a list over the capacity is not blended
        ba.list_n = ctx->list_n();
        ba.list_cap = (uint32_t)ctx->list_cap;
    }
    if (f.shading != GSR_SHADE_SPLAT) {  // a GL shading's first-hit kernel instead
        GSR_HIP(gsr_launch_shade(ba, f.shading, f.s), "shade launch");
        return GSR_OK;
    }
    if (f.median_depth || f.median_id) {  // (the depth keys: as below)
        const GsrDepthArgs da{f.pa.sort_keys, f.depth_map, f.inv_depth_map};
        const GsrSurfaceArgs ma{f.median_depth, f.median_id};
        GSR_HIP(gsr_launch_blend_surface(ba, da, ma, f.s), "surface blend launch");
    } else if (f.depth_map || f.inv_depth_map) {
        // z by Gaussian id from the depth keys: written by this frame's preprocess on f.s and only
        // read since (the depth sort takes them const); the next writer is the next call's
        // preprocess or gsr_depth_argsort, queued behind this blend (order_stream)
        const GsrDepthArgs da{f.pa.sort_keys, f.depth_map, f.inv_depth_map};
        GSR_HIP(gsr_launch_blend_depth(ba, da, f.s), "depth blend launch");
    } else {
        GSR_HIP(gsr_launch_blend(ba, f.s), "blend launch");
    }
    // gsr_forward_features: launches of their own over the same lists, behind the colour's (with
    // frame graphs they honour the list_n > list_cap early return through ba, as the colour's)
    if (f.feature_map)
        GSR_HIP(gsr_launch_blend_features(ba, f.features, f.feat_C, f.feature_map, f.s),
                "feature blend launch");
    return GSR_OK;
}

// The second stream must not outlive the caller's view of its inputs: every exit after the
// fork leaves the caller's stream behind the join.
struct JoinGuard {
    hipStream_t s = nullptr;
    hipEvent_t join = nullptr;
    bool armed = false;
    ~JoinGuard() {
        if (armed) (void)hipStreamWaitEvent(s, join, 0);
    }
};

// The state gsr_get_binning / gsr_tile_row_pairs read, after a rendered frame.
void finish_frame(gsr_context *ctx, const Frame &f, gsr_outputs *out) {
    out->num_rendered = (int64_t)f.K;
    gsr_context::LastFrame &l = ctx->last;
    l.K = (int64_t)f.K;
    l.list = (int64_t)f.KL;
    l.tight = f.tight;
    l.gx = f.gx, l.gy = f.gy, l.rb = f.rb, l.re = f.re;
    l.point_list = f.point_list;
    l.tiles_local = f.tiles_local;
    l.id_mask = f.id_mask;
    l.packed = f.colpairs && f.KL > 0;
    l.valid = true;
    if (f.tmode) ++ctx->timed_frames;
}

// The head of a rendered frame: ---- 1. preprocess, and the fork the second stream waits for.
int frame_head(gsr_context *ctx, const Frame &f) {
    if (f.tmode == 1) GSR_HIP(hipEventRecord(f.ev[0], f.s), "hipEventRecord");
    GSR_HIP(gsr_launch_preprocess(f.pa, f.s), "preprocess launch");
    GSR_HIP(hipEventRecord(ctx->fork, f.s), "hipEventRecord(fork)");
    return stage_end(ctx, f, 0);
}

// ... and its tail, once the list is binned: ---- 6. join: the blend reads the second stream's
// colours; ---- 7. blend
int frame_tail(gsr_context *ctx, const Frame &f, const gsr_raster_settings *st,
               gsr_outputs *out) {
    if (ctx->second_stream)
        GSR_HIP(hipStreamWaitEvent(f.s, ctx->join, 0), "hipStreamWaitEvent(join)");
    GSR_TRY(stage_end(ctx, f, 5));
    if (!f.no_blend) GSR_TRY(launch_blend(ctx, f, st, out));
    return stage_end(ctx, f, 6);
}

// ---- frame graphs (DESIGN.md decision 12) -----------------------------------------------------
// A small frame is bound by the host: ~17 kernel launches at ~5 us each.  ROCm launches a linear
// graph as one batch of pre-built packets (a 20-kernel chain in ~6 us), so the frame stream's
// chain after the preprocess (K publish, depth sort, column counts, column scatter, row pass
// with the tile ranges and the blend order) and the second stream's chain (K publish of LSD
// frames, colour) are each recorded once as a linear graph and replayed; the preprocess (the frame's camera and outputs) and the blend (its
// image) stay direct launches, so 2 launches + 2 graph launches + the fork / join remain.  A
// graph cannot take per-frame arguments: the preprocess stores the frame's tag and camera
// position into device words the recorded kernels read, and the binning is sized by a capacity
// (the list lengths seen so far + 25 %) instead of the host waiting for K in mid-frame; the
// column scatter stores the true length on the device and the row pass and the blend do
// nothing when it exceeds the capacity.  The host reads K after queueing the whole frame (for
// num_rendered) and re-renders an overflowed frame the direct way with a larger capacity, so
// every returned image is complete.

// Eligible forwards: column-first binning, a known capacity, no debug, no per-stage timing, no
// compaction (its colour pass waits on a mid-chain event of the frame stream), no rgb output
// (the colour pass's).
// (One-stream frames too: the second stream's chain then runs in order on the frame's stream,
// as the direct path's one-stream frames do -- recorded as its own graph in mode 1.)
bool graph_eligible(const gsr_context *ctx, const Frame &f, const gsr_outputs *out) {
    return ctx->graphs && ctx->list_cap > 0 && f.colpairs && !f.dbg && f.tmode != 1 &&
           !f.compact_sort && !f.color_ids && !out->rgb && f.P > 0;
}

GraphKey graph_key(const gsr_context *ctx, const Frame &f) {
    GraphKey k;
    std::memset(&k, 0, sizeof(k));  // (padding compares equal)
    k.ws_gen = ctx->ws_gen;
    k.cap = ctx->list_cap;
    k.P = f.P;
    k.means3D = f.pa.means3D;
    k.shs = f.pa.shs;
    k.colors_precomp = f.pa.colors_precomp;
    k.D = f.pa.D;
    k.M = f.pa.M;
    k.W = f.W;
    k.H = f.H;
    k.gx = f.gx;
    k.gy = f.gy;
    k.rb = f.rb;
    k.re = f.re;
    k.col_shift = f.col_shift;
    k.color_waves = color_waves_of(f);
    k.msd = f.msd_sort;
    k.main_publish = f.main_publish;
    k.tight = f.tight;
    k.sh_vec4 = (uint8_t)f.pa.sh_vec4;
    return k;
}

// The preprocess arguments the recorded kernels see: the camera position from the frame
// words, and none of the per-frame pointers (camera matrices, outputs), which they do not read.
GsrPreprocessArgs graph_args(const gsr_context *ctx, const GsrPreprocessArgs &a) {
    GsrPreprocessArgs g = a;
    g.campos = a.campos ? reinterpret_cast<const float *>(ctx->frame_words.get() + 4) : nullptr;
    g.viewmatrix = g.projmatrix = nullptr;
    g.scales = g.rotations = g.opacities = g.cov3D_precomp = nullptr;
    g.radii = nullptr;
    g.depths = g.means2D = g.conic_opacity = g.rgb = nullptr;
    g.tiles_touched = nullptr;
    g.k_tag = 0;
    g.frame_words = nullptr;
    return g;
}

void retire_graph(gsr_context *ctx, GraphEntry &e) {
    for (hipGraphExec_t *ge : {&e.sort, &e.bin, &e.aux}) {
        if (*ge) ctx->graph_retired.push_back(*ge);
        *ge = nullptr;
    }
}

// Destroys the retired executable graphs once enough have gathered (they ran only on this
// context's frame stream and second stream, which are drained first).
int drain_retired(gsr_context *ctx, hipStream_t s, bool force) {
    if (ctx->graph_retired.empty() || (!force && ctx->graph_retired.size() < kGraphRetired))
        return GSR_OK;
    GSR_HIP(hipStreamSynchronize(s), "hipStreamSynchronize(graphs)");
    if (ctx->aux) GSR_HIP(hipStreamSynchronize(ctx->aux), "hipStreamSynchronize(graphs)");
    for (hipGraphExec_t ge : ctx->graph_retired) (void)hipGraphExecDestroy(ge);
    ctx->graph_retired.clear();
    return GSR_OK;
}

// Records one chain into an executable graph, captured on the context's second stream (a
// capture executes nothing; a private capture stream would take one of the process's
// GPU_MAX_HW_QUEUES = 4 hardware queues, which the frame streams and second streams of two frames
// in flight already fill: with it, every stream shares a queue and the direct path lost 20 % in
// flight).
// A context without its second stream (one-stream frames) captures on a stream made for the
// recording and destroyed right after it: it holds no hardware queue beyond the recording, which
// happens once per key.
struct CaptureStream {
    hipStream_t s = nullptr;
    bool own = false;
    ~CaptureStream() {
        if (own && s) (void)hipStreamDestroy(s);
    }
};

template <typename Chain>
int record_chain(gsr_context *ctx, Chain chain, hipGraphExec_t *out) {
    CaptureStream capture;
    capture.s = ctx->aux;
    if (!capture.s) {
        GSR_HIP(hipStreamCreateWithFlags(&capture.s, hipStreamNonBlocking),
                "hipStreamCreateWithFlags(capture)");
        capture.own = true;
    }
    hipStream_t cs = capture.s;
    GSR_HIP(hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal), "hipStreamBeginCapture");
    const int rc = chain(cs);
    hipGraph_t graph = nullptr;
    const hipError_t e = hipStreamEndCapture(cs, &graph);  // (ends the capture on every path)
    if (rc != GSR_OK) {
        if (graph) (void)hipGraphDestroy(graph);
        return rc;
    }
    GSR_HIP(e, "hipStreamEndCapture");
    const hipError_t ei = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
    (void)hipGraphDestroy(graph);
    GSR_HIP(ei, "hipGraphInstantiate");
    return GSR_OK;
}

// The deferred-K frame's chains on stream cs (the frame graphs record them; GSR_OPT_FRAME_GRAPHS
// 2 launches them directly): g is graph_frame's copy of the frame.
Frame graph_frame(const gsr_context *ctx, const Frame &f) {
    Frame g = f;
    g.pa = graph_args(ctx, f.pa);
    g.tmode = 0;
    return g;
}

// K publish (main-stream frames) + the depth sort.
int chain_sort(gsr_context *ctx, Frame &g, hipStream_t cs) {
    g.s = cs;
    if (g.main_publish)
        GSR_HIP(gsr_launch_count_pairs(g.pa, cs, ctx->ds_ctl.get(), ctx->frame_words.get()),
                "pair count launch");
    return launch_depth_sort(ctx, g, 0, gsr_depth_sort_passes(32));
}

// The column counts, the column scatter and the row pass over the capacity, the list length
// read on the device; g.point_list: the buffer the sorted list ends in.
int chain_bin(gsr_context *ctx, Frame &g, hipStream_t cs) {
    g.s = cs;
    GSR_TRY(launch_scan(ctx, g));
    return launch_col_binning(ctx, g, ctx->list_cap, ctx->list_n());
}

// Records the frame's three chains (the key's) into e.
int record_frame_graphs(gsr_context *ctx, const Frame &f, GraphEntry &e) {
    Frame g = graph_frame(ctx, f);
    const uint32_t *fw = ctx->frame_words.get();
    GSR_TRY(record_chain(ctx, [&](hipStream_t cs) { return chain_sort(ctx, g, cs); }, &e.sort));
    GSR_TRY(record_chain(ctx, [&](hipStream_t cs) { return chain_bin(ctx, g, cs); }, &e.bin));
    e.point_list = g.point_list;
    GSR_TRY(record_chain(ctx, [&](hipStream_t cs) { return aux_chain(ctx, g, cs, fw); }, &e.aux));
    ++ctx->graph_records;
    return GSR_OK;
}

// The recorded graphs of this frame's key (recording them on a miss), or nullptr on failure.
int find_graphs(gsr_context *ctx, const Frame &f, GraphEntry **out) {
    const GraphKey key = graph_key(ctx, f);
    GraphEntry *hit = nullptr;
    for (auto it = ctx->graph_cache.begin(); it != ctx->graph_cache.end();) {
        if (it->key.ws_gen != ctx->ws_gen || it->key.cap != ctx->list_cap) {  // stale pointers
            retire_graph(ctx, *it);
            it = ctx->graph_cache.erase(it);
            continue;
        }
        if (std::memcmp(&it->key, &key, sizeof(key)) == 0) hit = &*it;
        ++it;
    }
    if (!hit) {
        if (ctx->graph_cache.size() >= kGraphCache) {  // replace the least recently used
            auto lru = std::min_element(ctx->graph_cache.begin(), ctx->graph_cache.end(),
                                        [](const GraphEntry &a, const GraphEntry &b) {
                                            return a.used < b.used;
                                        });
            retire_graph(ctx, *lru);
            ctx->graph_cache.erase(lru);
        }
        GraphEntry e;
        e.key = key;
        const int rc = record_frame_graphs(ctx, f, e);
        if (rc != GSR_OK) {
            retire_graph(ctx, e);
            return rc;
        }
        ctx->graph_cache.push_back(e);
        hit = &ctx->graph_cache.back();
    }
    hit->used = ++ctx->graph_clock;
    *out = hit;
    return GSR_OK;
}

constexpr int kOverflow = 1;  // forward_graph: the list outgrew the capacity (not rendered)
constexpr int kNoGraphs = 2;  // forward_graph: recording failed before anything was queued

int forward_graph(gsr_context *ctx, Frame &f, const gsr_raster_settings *st, gsr_outputs *out) {
    GraphEntry *e = nullptr;
    const bool replay = ctx->graphs == 1;  // 2: the same chains launched directly
    // a chain that cannot be recorded or instantiated leaves the frame to the direct path
    if (replay && find_graphs(ctx, f, &e) != GSR_OK) return kNoGraphs;
    Frame g = graph_frame(ctx, f);
    uint32_t *fw = ctx->frame_words.get();
    hipStream_t s = f.s;
    f.pa.frame_words = fw;
    GSR_TRY(frame_head(ctx, f));
    if (replay) GSR_HIP(hipGraphLaunch(e->sort, s), "hipGraphLaunch(depth sort)");
    else GSR_TRY(chain_sort(ctx, g, s));
    const bool two = ctx->second_stream != 0;  // (else mode 2 on one stream: in order on s)
    // (the second stream's chain behind the depth sort: color_after_sort; K is read last)
    if (two) GSR_HIP(hipEventRecord(ctx->fork, s), "hipEventRecord(sorted)");
    if (two) GSR_HIP(hipStreamWaitEvent(ctx->aux, ctx->fork, 0), "hipStreamWaitEvent(fork)");
    if (replay) GSR_HIP(hipGraphLaunch(e->aux, two ? ctx->aux : s), "hipGraphLaunch(aux chain)");
    else GSR_TRY(aux_chain(ctx, g, two ? ctx->aux : s, fw));
    if (two) GSR_HIP(hipEventRecord(ctx->join, ctx->aux), "hipEventRecord(join)");
    if (replay) GSR_HIP(hipGraphLaunch(e->bin, s), "hipGraphLaunch(binning)");
    else GSR_TRY(chain_bin(ctx, g, s));
    f.point_list = replay ? e->point_list : g.point_list;
    f.tiles_local = nullptr;
    f.id_mask = id_mask_of(f.col_shift);
    GSR_TRY(frame_tail(ctx, f, st, out));
    ++ctx->graph_frames;
    // K for num_rendered: published by the first kernel after the preprocess, long before the
    // host has queued the rest of the frame
    GSR_TRY(read_K(ctx, f, publish_stream(ctx, f)));
    if ((int64_t)f.KL > ctx->list_cap) return kOverflow;
    finish_frame(ctx, f, out);
    return GSR_OK;
}

int forward(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
            gsr_outputs *out, hipStream_t s, const FrameRequest &rq) {
    Frame f;
    ctx->last.valid = false;
    GSR_TRY(setup_frame(ctx, g, st, out, s, rq, f));
    if (ctx->second_stream && !ctx->aux)
        GSR_HIP(hipStreamCreateWithPriority(&ctx->aux, hipStreamNonBlocking, 0),
                "hipStreamCreateWithPriority(second stream)");
    f.graph = graph_eligible(ctx, f, out);
    if (f.graph) {
        GSR_TRY(drain_retired(ctx, s, false));
        int rc = forward_graph(ctx, f, st, out);
        if (rc == kNoGraphs) {
            // recording failed before anything of the frame was queued: this context launches
            // the same deferred-K chains directly from now on (GSR_OPT_FRAME_GRAPHS 2)
            ctx->graphs = 2;
            rc = forward_graph(ctx, f, st, out);
        }
        if (rc != kOverflow) return rc;
        // the list outgrew the capacity: nothing was binned or blended.  Grow the capacity and
        // render the frame again the direct way (the stream orders it after the skipped one)
        ++ctx->graph_overflows;
        ctx->list_cap = list_capacity((int64_t)f.KL, ctx->list_cap);
        GSR_TRY(reserve_K(ctx, ctx->list_cap, s));
        GSR_TRY(setup_frame(ctx, g, st, out, s, rq, f));
        f.graph = false;
    }

    if (f.P == 0) {  // upstream returns the zero-initialised image without rendering
        GSR_HIP(hipMemsetAsync(out->color, 0, (size_t)3 * f.rows_out * f.W * sizeof(float), s),
                "hipMemsetAsync(color)");
        for (float *plane : {f.depth_map, f.inv_depth_map})
            if (plane)
                GSR_HIP(hipMemsetAsync(plane, 0, (size_t)f.rows_out * f.W * sizeof(float), s),
                        "hipMemsetAsync(depth plane)");
        if (f.median_depth)
            GSR_HIP(hipMemsetAsync(f.median_depth, 0, (size_t)f.rows_out * f.W * sizeof(float), s),
                    "hipMemsetAsync(median depth)");
        if (f.median_id)  // -1: no surface
            GSR_HIP(hipMemsetAsync(f.median_id, 0xFF, (size_t)f.rows_out * f.W * sizeof(int32_t), s),
                    "hipMemsetAsync(median id)");
        if (f.feature_map)
            GSR_HIP(hipMemsetAsync(f.feature_map, 0,
                                   (size_t)f.feat_C * f.rows_out * f.W * sizeof(float), s),
                    "hipMemsetAsync(feature map)");
        GSR_HIP(hipMemsetAsync(ctx->ranges_words(), 0, f.T_strip * 8, s), "hipMemsetAsync");
        // an empty list in the per-pair form's buffers; no stage ran, so no timed frame
        f.K = f.KL = 0;
        f.tight = false;
        f.point_list = ctx->tile_vals.get();
        f.tiles_local = ctx->tile_keys.get();
        f.id_mask = 0xFFFFFFFFu;
        f.tmode = 0;
        finish_frame(ctx, f, out);
        return GSR_OK;
    }

    GSR_TRY(frame_head(ctx, f));
    // MSD frames: K for the host and D for the sort from one kernel on the main stream (one
    // launch fewer than the second stream's publish plus the sort's own key-bit reduction)
    if (f.main_publish)
        GSR_HIP(gsr_launch_count_pairs(f.pa, s, ctx->ds_ctl.get()), "pair count launch");

    // ---- 2. depth sort: pass 0 first, then the second stream's work (the host hands the
    // critical chain to the GPU first: queueing the ~10 second-stream commands before it left
    // the main queue idle ~40 us on a strip frame), then the later passes
    GSR_TRY(launch_depth_sort(ctx, f, 0, 1));
    JoinGuard guard{s, ctx->join, false};
    GSR_TRY(launch_second_stream(ctx, f));
    guard.armed = ctx->second_stream != 0;
    // D (the bits in which the kept depth keys differ) arrives in pinned memory from pass 0's
    // scan, tagged with this frame, while pass 0's downsweep runs: the host then queues only the
    // passes D needs.  Without it every pass is queued and the unneeded ones exit at once.
    if (!f.msd_sort) {  // the LSD sort: the passes D needs
        int depth_passes = gsr_depth_sort_passes(32);  // all
        uint64_t dv = 0;
        if (ctx->last.K >= kWaitDPairs && ctx->last_D <= 2u * 12u &&
            spin_on(&ctx->host_words->sort_D,
                    [&](uint64_t v) { return (uint32_t)(v >> 32) == f.tag; }, dv))
            depth_passes = gsr_depth_sort_passes((uint32_t)dv);
        GSR_TRY(launch_depth_sort(ctx, f, 1, depth_passes));
    }
    GSR_TRY(launch_color_after_sort(ctx, f));
    GSR_TRY(stage_end(ctx, f, 1));

    // ---- 3. scan
    GSR_TRY(launch_scan(ctx, f));
    GSR_TRY(stage_end(ctx, f, 2));
    GSR_TRY(wait_K(ctx, f));

    // ---- 4, 5. duplicate + tile sort (+ the per-pair form's ranges)
    GSR_TRY(launch_binning(ctx, f));

    // ---- 6, 7. join + blend
    guard.armed = false;
    GSR_TRY(frame_tail(ctx, f, st, out));
    finish_frame(ctx, f, out);
    return GSR_OK;
}

// Every public forward: the NULL check, the shading's range (gsr_forward_shaded's argument; the
// others pass the splat), the context's lock, the stream's order, the frame.
int forward_entry(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                  gsr_outputs *out, void *stream, const FrameRequest &rq) {
    if (!ctx || !g || !st || !out) return fail(GSR_E_INVALID, "gsr_forward: NULL argument");
    if (rq.shading < GSR_SHADE_SPLAT || rq.shading > GSR_SHADE_GAUSS_BALL)
        return fail(GSR_E_INVALID, "gsr_forward_shaded: unknown shading " +
                                       std::to_string(rq.shading) + " (GSR_SHADE_* 0..3)");
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    GSR_TRY(order_stream(ctx, s));
    return forward(ctx, g, st, out, s, rq);
}

}  // namespace

// The thread's last-error message for the other translation units (ply_loader.hip).
int gsr_set_error(int code, const std::string &msg) { return fail(code, msg); }

extern "C" {

int gsr_abi_version(void) { return GSR_ABI_VERSION; }
const char *gsr_last_error(void) { return g_err.c_str(); }
const char *gsr_stage_name(int i) { return (i >= 0 && i < kAllStages) ? kStageNames[i] : ""; }

int gsr_create(gsr_context **out) {
    if (!out) return fail(GSR_E_INVALID, "gsr_create: out is NULL");
    *out = nullptr;
    gsr_context *ctx = new gsr_context();
    if (hipGetDevice(&ctx->device) != hipSuccess) {
        (void)hipGetLastError();
        delete ctx;
        return fail(GSR_E_HIP, "gsr_create: no HIP device");
    }
    if (hipHostMalloc(reinterpret_cast<void **>(&ctx->host_words), sizeof(GsrHostWords),
                      hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(reinterpret_cast<void **>(&ctx->d_host_words), ctx->host_words,
                                0) != hipSuccess) {
        (void)hipGetLastError();
        delete ctx;
        return fail(GSR_E_HIP, "gsr_create: hipHostMalloc failed");
    }
    std::memset(ctx->host_words, 0, sizeof(GsrHostWords));  // tag 0 never matches a frame
    bool ok = hipMalloc(&ctx->frame_words.p, 64) == hipSuccess &&
              hipMemset(ctx->frame_words.p, 0, 64) == hipSuccess &&
              // stream-to-stream hand-offs on one device: a device-scope release suffices
              hipEventCreateWithFlags(&ctx->fork, hipEventDisableTiming | hipEventReleaseToDevice) ==
                  hipSuccess &&
              hipEventCreateWithFlags(&ctx->join, hipEventDisableTiming | hipEventReleaseToDevice) ==
                  hipSuccess &&
              hipEventCreateWithFlags(&ctx->compacted,
                                      hipEventDisableTiming | hipEventReleaseToDevice) == hipSuccess &&
              gsr_color_setup() == hipSuccess;
    // timing events only time: no system-scope fence (cache writeback) when they complete
    for (auto &set : ctx->ev)
        for (auto &e : set) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableSystemFence) == hipSuccess;
    for (auto &set : ctx->ev_color)
        for (auto &e : set) ok = ok && hipEventCreateWithFlags(&e, hipEventDisableSystemFence) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        gsr_destroy(ctx);
        return fail(GSR_E_HIP, "gsr_create: stream / event creation failed");
    }
    *out = ctx;
    return GSR_OK;
}

void gsr_destroy(gsr_context *ctx) {
    if (!ctx) return;
    (void)hipDeviceSynchronize();
    for (GraphEntry &e : ctx->graph_cache) retire_graph(ctx, e);
    for (hipGraphExec_t ge : ctx->graph_retired) (void)hipGraphExecDestroy(ge);
    for (DevBuf *b : ctx->bufs)
        if (b->p) (void)hipFree(b->p);
    for (auto &set : ctx->ev)
        for (auto &e : set)
            if (e) (void)hipEventDestroy(e);
    for (auto &set : ctx->ev_color)
        for (auto &e : set)
            if (e) (void)hipEventDestroy(e);
    for (auto &e : ctx->ev_bwd)
        if (e) (void)hipEventDestroy(e);
    if (ctx->fork) (void)hipEventDestroy(ctx->fork);
    if (ctx->join) (void)hipEventDestroy(ctx->join);
    if (ctx->compacted) (void)hipEventDestroy(ctx->compacted);
    if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
    if (ctx->host_words) (void)hipHostFree(ctx->host_words);
    delete ctx;
}

int gsr_reserve(gsr_context *ctx, int64_t P, int64_t K) {
    if (!ctx || P < 0 || K < 0) return fail(GSR_E_INVALID, "gsr_reserve: bad arguments");
    std::lock_guard<std::mutex> lock(ctx->mu);
    GSR_TRY(reserve_P(ctx, P, nullptr));
    if (K > ctx->list_cap) ctx->list_cap = std::min<int64_t>((K + 4095) & ~(int64_t)4095,
                                                             (int64_t)UINT32_MAX - 4096);
    GSR_TRY(reserve_K(ctx, std::max<int64_t>(K, ctx->list_cap), nullptr));
    GSR_HIP(hipDeviceSynchronize(), "gsr_reserve");
    return GSR_OK;
}

int gsr_set_option(gsr_context *ctx, int option, int64_t value) {
    if (!ctx) return fail(GSR_E_INVALID, "gsr_set_option: NULL context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    switch (option) {
        case GSR_OPT_BLEND_CULL: ctx->cull = value ? 1 : 0; return GSR_OK;
        case GSR_OPT_BLEND_FAST:
            if (value < 0 || value > 1) return fail(GSR_E_INVALID, "gsr_set_option: fast 0..1");
            ctx->fast = (int)value;
            return GSR_OK;
        case GSR_OPT_TIGHT_BINNING: ctx->tight = value ? 1 : 0; return GSR_OK;
        case GSR_OPT_SECOND_STREAM:
            if (value < 0 || value > 1)
                return fail(GSR_E_INVALID, "gsr_set_option: second stream 0..1");
            ctx->second_stream = (int)value;
            if (!value && ctx->aux) {  // (drained first: its last frame's work may still run)
                GSR_HIP(hipStreamSynchronize(ctx->aux), "hipStreamSynchronize(second stream)");
                GSR_HIP(hipStreamDestroy(ctx->aux), "hipStreamDestroy(second stream)");
                ctx->aux = nullptr;
            }
            return GSR_OK;
        case GSR_OPT_FRAME_GRAPHS:
            if (value < 0 || value > 2) return fail(GSR_E_INVALID, "gsr_set_option: graphs 0..2");
            ctx->graphs = (int)value;
            return GSR_OK;
        case GSR_OPT_DEPTH_SORT:
            if (value < -1 || value > 3)
                return fail(GSR_E_INVALID, "gsr_set_option: depth sort -1..3");
            ctx->depth_sort = (int)value;
            return GSR_OK;
        default:
            return fail(GSR_E_INVALID, "gsr_set_option: unknown option " + std::to_string(option));
    }
}

int gsr_get_option(gsr_context *ctx, int option, int64_t *value) {
    if (!ctx || !value) return fail(GSR_E_INVALID, "gsr_get_option: NULL argument");
    std::lock_guard<std::mutex> lock(ctx->mu);
    switch (option) {
        case GSR_OPT_BLEND_CULL: *value = ctx->cull; return GSR_OK;
        case GSR_OPT_BLEND_FAST: *value = ctx->fast; return GSR_OK;
        case GSR_OPT_TIGHT_BINNING: *value = ctx->tight; return GSR_OK;
        case GSR_OPT_SECOND_STREAM: *value = ctx->second_stream; return GSR_OK;
        case GSR_OPT_FRAME_GRAPHS: *value = ctx->graphs; return GSR_OK;
        case GSR_OPT_DEPTH_SORT: *value = ctx->depth_sort; return GSR_OK;
        default:
            return fail(GSR_E_INVALID, "gsr_get_option: unknown option " + std::to_string(option));
    }
}

int gsr_frame_graph_stats(gsr_context *ctx, int64_t *stats, int n) {
    if (!ctx || (!stats && n > 0)) return fail(GSR_E_INVALID, "gsr_frame_graph_stats: bad arguments");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const int64_t v[4] = {ctx->graph_frames, ctx->graph_records, ctx->graph_overflows,
                          ctx->list_cap};
    for (int i = 0; i < n && i < 4; ++i) stats[i] = v[i];
    return 4;
}

int gsr_set_timing(gsr_context *ctx, int enable) {
    if (!ctx) return fail(GSR_E_INVALID, "gsr_set_timing: NULL context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (enable < 0 || enable > 2) return fail(GSR_E_INVALID, "gsr_set_timing: mode 0..2");
    ctx->timing = enable;
    ctx->forwards = 0;
    ctx->timed_frames = 0;
    return GSR_OK;
}

// Mean per-stage time (ms) over the timed forwards since gsr_set_timing (the most recent
// kTimingRing of them).  Waits for the last one.  Return value: number of stages.
int gsr_stage_times(gsr_context *ctx, float *ms, int n) {
    if (!ctx || (!ms && n > 0)) return fail(GSR_E_INVALID, "gsr_stage_times: bad arguments");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (ctx->timed_frames == 0) return fail(GSR_E_STATE, "gsr_stage_times: no timed forward yet");
    const int64_t frames = std::min<int64_t>(ctx->timed_frames, kTimingRing);
    const int64_t last = (ctx->timed_frames - 1) % kTimingRing;
    GSR_HIP(hipEventSynchronize(ctx->ev[last][kStages]), "hipEventSynchronize");
    const bool all = ctx->timing != 2;  // mode 2 recorded the blend's two events only
    double acc[kAllStages] = {};
    for (int64_t fr = 0; fr < frames; ++fr) {
        const int64_t slot = (ctx->timed_frames - 1 - fr) % kTimingRing;
        for (int i = all ? 0 : kStages - 1; i < kStages; ++i) {
            float t = 0.f;
            GSR_HIP(hipEventElapsedTime(&t, ctx->ev[slot][i], ctx->ev[slot][i + 1]),
                    "hipEventElapsedTime");
            acc[i] += t;
        }
        if (all) {
            float t = 0.f;
            GSR_HIP(hipEventElapsedTime(&t, ctx->ev_color[slot][0], ctx->ev_color[slot][1]),
                    "hipEventElapsedTime");
            acc[kStages] += t;
        }
    }
    for (int i = 0; i < kAllStages && i < n; ++i) ms[i] = (float)(acc[i] / (double)frames);
    return kAllStages;
}

int gsr_forward_shaded(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                       gsr_outputs *out, int32_t shading, void *stream) {
    return forward_entry(ctx, g, st, out, stream, {shading});
}

int gsr_forward(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                gsr_outputs *out, void *stream) {
    return forward_entry(ctx, g, st, out, stream, {});
}

int gsr_forward_depth(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                      gsr_outputs *out, const gsr_depth_outputs *depth, void *stream) {
    return forward_entry(ctx, g, st, out, stream, {GSR_SHADE_SPLAT, depth});
}

int gsr_forward_surface(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                        gsr_outputs *out, const gsr_depth_outputs *depth,
                        const gsr_surface_outputs *surface, void *stream) {
    return forward_entry(ctx, g, st, out, stream, {GSR_SHADE_SPLAT, depth, surface});
}

// 0 or 1 from a gsr_filter_settings (NULL: 0), -1 for anything else.
static int filter_antialiasing(const gsr_filter_settings *filter) {
    if (!filter) return 0;
    return filter->antialiasing == 0 || filter->antialiasing == 1 ? filter->antialiasing : -1;
}

int gsr_forward_filtered(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                         gsr_outputs *out, const gsr_depth_outputs *depth,
                         const gsr_surface_outputs *surface, const gsr_filter_settings *filter,
                         void *stream) {
    const int aa = filter_antialiasing(filter);
    if (aa < 0)
        return fail(GSR_E_INVALID, "gsr_forward_filtered: antialiasing must be 0 or 1, got " +
                                       std::to_string(filter->antialiasing));
    if (!aa) return gsr_forward_surface(ctx, g, st, out, depth, surface, stream);
    return forward_entry(ctx, g, st, out, stream, {GSR_SHADE_SPLAT, depth, surface, true});
}

// NULL if the struct's C and features can be used, else what is wrong with them.
static const char *feature_fault(int32_t C, const float *features, int64_t P) {
    if (C < 1 || C > GSR_MAX_FEATURES) return "C must be in 1..GSR_MAX_FEATURES";
    if (P > 0 && !features) return "features is NULL";
    return nullptr;
}

int gsr_forward_features(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                         gsr_outputs *out, const gsr_depth_outputs *depth,
                         const gsr_surface_outputs *surface, const gsr_filter_settings *filter,
                         const gsr_feature_outputs *feat, void *stream) {
    if (!feat || !feat->feature_map)
        return gsr_forward_filtered(ctx, g, st, out, depth, surface, filter, stream);
    if (!g) return fail(GSR_E_INVALID, "gsr_forward: NULL argument");
    if (const char *why = feature_fault(feat->C, feat->features, g->P))
        return fail(GSR_E_INVALID, std::string("gsr_forward_features: ") + why + " (C = " +
                                       std::to_string(feat->C) + ")");
    const int aa = filter_antialiasing(filter);
    if (aa < 0)
        return fail(GSR_E_INVALID, "gsr_forward_features: antialiasing must be 0 or 1, got " +
                                       std::to_string(filter->antialiasing));
    FrameRequest rq{GSR_SHADE_SPLAT, depth, surface, aa != 0};
    rq.feat = feat;
    return forward_entry(ctx, g, st, out, stream, rq);
}

// ---- the backward: the gradients of the splat composite ----------------------------------------
// Everything is rebuilt from the arguments -- the per-Gaussian stage, the depth sort and upstream's
// (untight) lists, the direct way: no recorded graph is replayed, none is invalidated beyond what a
// forward of the same shape would -- so nothing of an earlier forward on this context is read; then
// backward.hip's two kernels.

// What a public backward was called with, as FrameRequest holds a forward's: NULL for each
// optional struct the entry does not take.
struct BackwardRequest {
    // the entry a message names while none of filter, order, a strip and feat is in use: the entry
    // itself up to gsr_backward_camera, which every later entry is without its own option
    const char *fn;
    const gsr_gaussians *g;
    const gsr_raster_settings *st;
    const gsr_backward_inputs *in;
    gsr_gradients *gr;
    const gsr_plane_gradients *planes = nullptr;
    const gsr_camera_gradients *camera = nullptr;
    const gsr_filter_settings *filter = nullptr;
    const gsr_backward_order *order = nullptr;
    const gsr_feature_gradients *feat = nullptr;
    bool strips = false;  // gsr_backward_strip on: a strip of the settings is honoured, not refused
    const gsr_abs_gradients *abs = nullptr;
};

// What the call does, decided once, before the context is touched.
struct BackwardPlan {
    // the entry the messages name: the last of gsr_backward_filtered, _ordered, _strip,
    // _features and _abs whose option is in use (an option at 0 is the entry below), else rq.fn
    std::string fn;
    hipStream_t s = nullptr;
    bool planes = false;  // a plane gradient is given: the planes instantiations of both kernels
    bool camera = false;  // a camera buffer is given: the camera instantiation and k_camera_finish
    bool aa = false;      // gsr_backward_filtered: the antialiased per-Gaussian twins
    // gsr_backward_ordered: the blend's backward stores every (Gaussian, tile,
    // quadrant)'s sums to a slot of its own and a gather fills the 2D gradient rows in a fixed order
    bool det = false;
    // the settings hold a strip: the rebuild and the blend's backward are the strip's, and on a
    // proper subset of the rows the Gaussians without a tile in it are gated out of the third stage
    bool strip = false;
    const gsr_feature_gradients *ft = nullptr;  // rq.feat when it holds a dL_dfeature_map
    // gsr_backward_abs: rq.abs's dL_dmeans2D_abs, or NULL -- the kAbs instantiations
    // of the blend's backward (and of the gather) and k_means2d_abs in the third stage
    float *abs = nullptr;
};

static bool backward_null(const gsr_context *ctx, const BackwardRequest &rq) {
    return !ctx || !rq.g || !rq.st || !rq.in || !rq.gr;
}

// The optional structs -> p.aa, p.det, p.ft, p.abs and the name the call speaks under.  ctx is compared
// with NULL only.
static int backward_parse(const gsr_context *ctx, const BackwardRequest &rq, BackwardPlan &p) {
    const int aa = rq.filter ? rq.filter->antialiasing : 0;
    const int det = rq.order ? rq.order->deterministic : 0;
    if (rq.feat && rq.feat->dL_dfeature_map) p.ft = rq.feat;
    if (rq.abs) p.abs = rq.abs->dL_dmeans2D_abs;
    p.fn = aa == 0 ? rq.fn : "gsr_backward_filtered";
    if (det != 0) p.fn = "gsr_backward_ordered";
    if (rq.strips) {  // the two entries that read the settings here check their pointers first
        if (backward_null(ctx, rq))
            return fail(GSR_E_INVALID, std::string(p.abs  ? "gsr_backward_abs"
                                                   : p.ft ? "gsr_backward_features"
                                                          : "gsr_backward_strip") + ": NULL argument");
        if (rq.st->tile_row_begin != 0 || rq.st->tile_row_end != 0) p.fn = "gsr_backward_strip";
    }
    if (p.ft) {
        p.fn = "gsr_backward_features";
        if (const char *why = feature_fault(p.ft->C, p.ft->features, rq.g->P))
            return fail(GSR_E_INVALID, p.fn + ": " + why + " (C = " + std::to_string(p.ft->C) + ")");
        if (det == 1)
            return fail(GSR_E_INVALID, p.fn + ": deterministic == 1 with a feature gradient: the "
                                              "deterministic slots hold 9 or 10 sums and have no "
                                              "room for C more");
    }
    if (p.abs) {
        p.fn = "gsr_backward_abs";
        if (p.ft)
            return fail(GSR_E_INVALID, p.fn + ": dL_dmeans2D_abs with a feature gradient: the "
                                              "feature channels add their share of dL/dalpha in "
                                              "passes of their own, and the absolute value of a "
                                              "pixel's total cannot be split over passes");
    }
    if (det != 0 && det != 1)
        return fail(GSR_E_INVALID, p.fn + ": deterministic must be 0 or 1, got " +
                                       std::to_string(det));
    if (aa != 0 && aa != 1)
        return fail(GSR_E_INVALID, p.fn + ": antialiasing must be 0 or 1, got " +
                                       std::to_string(aa));
    p.aa = aa == 1, p.det = det == 1;
    return GSR_OK;
}

// The arguments themselves -> p.strip, p.planes, p.camera.  ctx is compared with NULL only.
static int backward_validate(const gsr_context *ctx, const BackwardRequest &rq, BackwardPlan &p) {
    const std::string &fn = p.fn;
    if (backward_null(ctx, rq)) return fail(GSR_E_INVALID, fn + ": NULL argument");
    const gsr_gaussians *g = rq.g;
    const gsr_raster_settings *st = rq.st;
    p.strip = st->tile_row_begin != 0 || st->tile_row_end != 0;
    if (p.strip && !rq.strips)
        return fail(GSR_E_INVALID, fn + ": whole frames only (a tile row strip is set)");
    if (g->P < 0 || g->P > (int64_t)UINT32_MAX) return fail(GSR_E_INVALID, fn + ": bad P");
    if (st->image_width <= 0 || st->image_height <= 0)
        return fail(GSR_E_INVALID, fn + ": image size must be positive");
    // (before anything is written: the P == 0 path zeroes the camera's buffers)
    if (p.strip && (st->tile_row_begin < 0 || st->tile_row_begin >= st->tile_row_end ||
                    st->tile_row_end > (st->image_height + GSR_TILE_Y - 1) / GSR_TILE_Y))
        return fail(GSR_E_INVALID, fn + ": bad tile row strip");
    const gsr_plane_gradients *pl = rq.planes;
    p.planes = pl && (pl->dL_ddepth_map || pl->dL_dinv_depth_map || pl->dL_dfinal_T);
    const gsr_camera_gradients *cam = rq.camera;
    p.camera = cam && (cam->dL_dviewmatrix || cam->dL_dprojmatrix || cam->dL_dcampos);
    if (g->P > 0) {
        if (!rq.in->dL_dcolor && !p.planes && !p.ft)
            return fail(GSR_E_INVALID, fn + (pl ? ": dL_dcolor or a plane gradient is required"
                                                : ": dL_dcolor is required"));
        if ((g->shs == nullptr) == (g->colors_precomp == nullptr))
            return fail(GSR_E_INVALID,
                        "Please provide excatly one of either SHs or precomputed colors!");
        if (((g->scales == nullptr || g->rotations == nullptr) && g->cov3D_precomp == nullptr) ||
            ((g->scales != nullptr || g->rotations != nullptr) && g->cov3D_precomp != nullptr))
            return fail(GSR_E_INVALID, "Please provide exactly one of either scale/rotation pair "
                                       "or precomputed 3D covariance!");
    }
    return GSR_OK;
}

// The workspace whose size P decides (the deterministic slots' follows the rebuild's K).
static int backward_reserve(gsr_context *ctx, const BackwardRequest &rq, const BackwardPlan &p) {
    const int64_t P = rq.g->P;
    if (p.camera)
        GSR_TRY(grow(ctx, ctx->cam_partials,
                     (size_t)kCameraSums * gsr_preprocess_blocks(P) * sizeof(float), p.s));
    GSR_TRY(grow(ctx, ctx->grad2d, (size_t)P * kGradRow * sizeof(float), p.s));
    GSR_TRY(grow(ctx, ctx->bwd_radii, (size_t)P * sizeof(int32_t), p.s));
    if (p.det) {
        GSR_TRY(grow(ctx, ctx->det_slab, (size_t)P * sizeof(uint64_t), p.s));
        GSR_TRY(grow(ctx, ctx->det_partials, (size_t)gsr_slab_blocks(P) * sizeof(uint64_t), p.s));
    }
    return GSR_OK;
}

// The i-th of the four events around the three timed stages.
static int backward_mark(gsr_context *ctx, const BackwardPlan &p, int i) {
    if (ctx->timing) GSR_HIP(hipEventRecord(ctx->ev_bwd[i], p.s), "hipEventRecord");
    return GSR_OK;
}

static int backward_stage_check(const BackwardRequest &rq, const BackwardPlan &p, const char *what) {
    if (!rq.st->debug) return GSR_OK;
    GSR_HIP(hipStreamSynchronize(p.s), what);
    GSR_HIP(hipGetLastError(), what);
    return GSR_OK;
}

// The caller's options, set aside for the rebuild and put back on every way out of it.
struct RebuildOptions {
    gsr_context *ctx;
    const int tight = ctx->tight, graphs = ctx->graphs, timing = ctx->timing;
    ~RebuildOptions() { ctx->tight = tight, ctx->graphs = graphs, ctx->timing = timing; }
};

// The first timed stage, the rebuild: a forward without its blend, with upstream's lists,
// launched directly and untimed.
static int backward_rebuild(gsr_context *ctx, const BackwardRequest &rq, const BackwardPlan &p) {
    gsr_outputs out{};
    out.color = ctx->grad2d.get();  // (required by the argument check; never written: no_blend)
    out.radii = ctx->bwd_radii.get();
    ctx->bwd_timed = false;
    if (ctx->timing)
        for (auto &e : ctx->ev_bwd)
            if (!e) GSR_HIP(hipEventCreateWithFlags(&e, hipEventDisableSystemFence), "hipEventCreate");
    GSR_TRY(backward_mark(ctx, p, 0));
    RebuildOptions restore{ctx};
    ctx->tight = ctx->graphs = ctx->timing = 0;
    FrameRequest rebuild;
    rebuild.antialiasing = p.aa;
    rebuild.no_blend = true;
    return forward(ctx, rq.g, rq.st, &out, p.s, rebuild);
}

// The second timed stage, the blend's backward: ctx->grad2d's rows from the image-like gradients.
static int backward_blend(gsr_context *ctx, const BackwardRequest &rq, const BackwardPlan &p) {
    const gsr_raster_settings *st = rq.st;
    const gsr_feature_gradients *ft = p.ft;
    const int64_t P = rq.g->P;
    hipStream_t s = p.s;
    const gsr_context::LastFrame &l = ctx->last;
    // the strip the rebuild binned (the whole frame's rows without one), as launch_blend offsets
    // the forward's
    GsrStripBwdArgs sa{};
    sa.row_begin = l.rb;
    sa.y0 = (int)(l.rb * GSR_TILE_Y);
    sa.rows_out = std::min(st->image_height, (int)(l.re * GSR_TILE_Y)) - sa.y0;
    const GsrStripBwdArgs *const sp = p.strip ? &sa : nullptr;
    GsrDetBwdArgs da{};
    if (p.det) {
        // the slots: one per (list entry, quadrant); the lists are upstream's, K = num_rendered
        const uint64_t K = (uint64_t)l.list;
        if (l.tight || l.list != l.K)
            return fail(GSR_E_STATE, p.fn + ": the rebuild left tight lists");
        if (K >= (1ull << 30))
            return fail(GSR_E_INVALID, p.fn + ": deterministic needs num_rendered < 2^30, got " +
                                           std::to_string(K));
        const size_t sums = (p.planes ? 10 : 9) + (p.abs ? 2 : 0);
        GSR_TRY(grow(ctx, ctx->det_marks, std::max<size_t>(4 * K, 1), s));
        GSR_TRY(grow(ctx, ctx->det_sums, std::max<size_t>(4 * K * sums * sizeof(float), 1), s));
        da = {ctx->strip_rect.get(), ctx->det_slab.get(), ctx->det_sums.get(),
              ctx->det_marks.get(), (uint32_t)K};
    }
    GSR_TRY(backward_mark(ctx, p, 1));
    if (p.det) {
        if (da.K > 0)
            GSR_HIP(hipMemsetAsync(da.marks, 0, 4 * (size_t)da.K, s), "hipMemsetAsync(marks)");
        GSR_HIP(gsr_launch_slab_scan(da.strip_rect, P, ctx->det_partials.get(),
                                     ctx->det_slab.get(), s),
                "slab scan launch");
    } else {
        GSR_HIP(hipMemsetAsync(ctx->grad2d.get(), 0, (size_t)P * kGradRow * sizeof(float), s),
                "hipMemsetAsync(grad2d)");
    }
    if (ft && ft->dL_dfeatures)  // zeroed, then filled: culled Gaussians keep exact zeros
        GSR_HIP(hipMemsetAsync(ft->dL_dfeatures, 0, (size_t)P * ft->C * sizeof(float), s),
                "hipMemsetAsync(dL_dfeatures)");
    GsrBlendBwdArgs ba{};
    ba.ranges = ctx->ranges_local.get();
    ba.point_list = l.point_list;
    ba.records = ctx->records.get();
    ba.W = st->image_width;
    ba.H = st->image_height;
    ba.grid_x = l.gx;
    ba.n_tiles = l.gx * (l.re - l.rb);  // (the whole frame: l.gy rows)
    ba.bg = st->bg;
    ba.dL_dcolor = rq.in->dL_dcolor;
    ba.id_mask = l.id_mask;
    ba.cull = ctx->cull;
    ba.grad2d = ctx->grad2d.get();
    if (l.list > 0) {
        // z by Gaussian id from the rebuild's depth keys, as launch_blend hands them to the
        // forward's planes: written by the rebuild's preprocess on s and only read since
        GsrPlaneBwdArgs pa{};
        if (p.planes)
            pa = {ctx->sort_keys.get(), rq.planes->dL_ddepth_map, rq.planes->dL_dinv_depth_map,
                  rq.planes->dL_dfinal_T};
        // (neither: a feature gradient alone, no colour pass)
        if (p.planes || ba.dL_dcolor)
            GSR_HIP(gsr_launch_blend_bwd(ba, p.planes ? &pa : nullptr, p.det ? &da : nullptr, sp,
                                         s, p.abs != nullptr),
                    "blend backward launch");
        // gsr_backward_features: beside the pass above, into the same zeroed rows
        if (ft)
            GSR_HIP(gsr_launch_blend_bwd_features(ba, ft->features, ft->C, ft->dL_dfeature_map,
                                                  ft->dL_dfeatures, s, sp),
                    "feature blend backward launch");
    }
    if (p.det)  // every word of every row, zeros where nothing was stored
        GSR_HIP(gsr_launch_grad_rows_gather(da, P, p.planes, ctx->grad2d.get(), s,
                                            p.abs != nullptr),
                "gradient rows gather launch");
    GSR_TRY(backward_mark(ctx, p, 2));
    return backward_stage_check(rq, p, "stage blend backward");
}

// The third timed stage, the per-Gaussian backward: the caller's gradients from ctx->grad2d's rows.
static int backward_gaussians(gsr_context *ctx, const BackwardRequest &rq, const BackwardPlan &p) {
    const gsr_gaussians *g = rq.g;
    const gsr_raster_settings *st = rq.st;
    const gsr_gradients *gr = rq.gr;
    const int64_t P = g->P;
    hipStream_t s = p.s;
    const gsr_context::LastFrame &l = ctx->last;
    // a proper subset of the rows: the Gaussians without a tile in it read as culled from here on
    // (the strip (0, grid_y) gates nothing: the whole frame's per-Gaussian stage, bit for bit)
    if (p.strip && l.re - l.rb < l.gy)
        GSR_HIP(gsr_launch_strip_gate(ctx->strip_rect.get(), P, ctx->bwd_radii.get(), s),
                "strip gate launch");

    GsrPreprocessBwdArgs pb{};
    pb.P = P;
    pb.D = g->D;
    pb.M = g->M;
    pb.scale_modifier = g->scale_modifier;
    pb.means3D = g->means3D;
    pb.scales = g->scales;
    pb.rotations = g->rotations;
    pb.shs = g->shs;
    pb.colors_precomp = g->colors_precomp;
    pb.cov3D_precomp = g->cov3D_precomp;
    pb.viewmatrix = st->viewmatrix;
    pb.projmatrix = st->projmatrix;
    pb.campos = st->campos;
    pb.tanfovx = st->tanfovx;
    pb.tanfovy = st->tanfovy;
    pb.focal_y = (float)st->image_height / (2.0f * st->tanfovy);
    pb.focal_x = (float)st->image_width / (2.0f * st->tanfovx);
    pb.W = st->image_width;
    pb.H = st->image_height;
    pb.radii = ctx->bwd_radii.get();
    pb.grad2d = ctx->grad2d.get();
    pb.dL_dmeans3D = gr->dL_dmeans3D;
    pb.dL_dmeans2D = gr->dL_dmeans2D;
    pb.dL_dopacity = gr->dL_dopacity;
    pb.dL_dcolors = gr->dL_dcolors;
    pb.dL_dconic = gr->dL_dconic;
    pb.dL_dsh = gr->dL_dsh;
    pb.dL_dscales = gr->dL_dscales;
    pb.dL_drotations = gr->dL_drotations;
    pb.dL_dcov3D = gr->dL_dcov3D;
    float *const dL_ddepths = rq.planes ? rq.planes->dL_ddepths : nullptr;
    GsrPreprocessBwdExtras extras;
    extras.planes = p.planes;
    extras.dL_ddepths = dL_ddepths;
    // (an empty list leaves the rows zero: every product, and so every sum of the camera's, is 0)
    GsrCameraBwdArgs ca{};
    if (p.camera) {
        ca = {ctx->cam_partials.get(), rq.camera->dL_dviewmatrix, rq.camera->dL_dprojmatrix,
              rq.camera->dL_dcampos};
        extras.camera = &ca;
    }
    // gsr_backward_filtered: the antialiased twins, which also read the opacities
    extras.aa_opacities = p.aa ? g->opacities : nullptr;
    GSR_HIP(gsr_launch_preprocess_bwd(pb, extras, s), "per-Gaussian backward launch");
    if (p.abs)  // gsr_backward_abs: the rows' words 10, 11, behind the gate like the kernel above
        GSR_HIP(gsr_launch_means2d_abs(pb.radii, pb.grad2d, P, pb.W, pb.H, p.abs, s),
                "absolute means2D gradient launch");
    if (!p.planes && dL_ddepths)  // no plane gradient: nothing reaches the features
        GSR_HIP(hipMemsetAsync(dL_ddepths, 0, (size_t)P * sizeof(float), s),
                "hipMemsetAsync(dL_ddepths)");
    GSR_TRY(backward_mark(ctx, p, 3));
    ctx->bwd_timed = ctx->timing != 0;
    return backward_stage_check(rq, p, "stage per-Gaussian backward");
}

// Every public backward: the request's parse and checks, the context's lock, the stream's order,
// the three timed stages.
static int backward_entry(gsr_context *ctx, void *stream, const BackwardRequest &rq) {
    BackwardPlan p;
    GSR_TRY(backward_parse(ctx, rq, p));
    GSR_TRY(backward_validate(ctx, rq, p));
    std::lock_guard<std::mutex> lock(ctx->mu);
    p.s = static_cast<hipStream_t>(stream);
    GSR_TRY(order_stream(ctx, p.s));
    if (rq.g->P == 0) {  // no Gaussian, no gradient: the camera's buffers, of a fixed size, are zeros
        if (p.camera) {
            const struct {
                float *p;
                size_t n;
                const char *what;
            } sums[] = {{rq.camera->dL_dviewmatrix, 16, "hipMemsetAsync(dL_dviewmatrix)"},
                        {rq.camera->dL_dprojmatrix, 16, "hipMemsetAsync(dL_dprojmatrix)"},
                        {rq.camera->dL_dcampos, 3, "hipMemsetAsync(dL_dcampos)"}};
            for (const auto &m : sums)
                if (m.p) GSR_HIP(hipMemsetAsync(m.p, 0, m.n * sizeof(float), p.s), m.what);
        }
        return GSR_OK;
    }
    GSR_TRY(backward_reserve(ctx, rq, p));
    GSR_TRY(backward_rebuild(ctx, rq, p));
    GSR_TRY(backward_blend(ctx, rq, p));
    return backward_gaussians(ctx, rq, p);
}

int gsr_backward(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                 const gsr_backward_inputs *in, gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream, {"gsr_backward", g, st, in, gr});
}

int gsr_backward_planes(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                        const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                        gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream, {"gsr_backward_planes", g, st, in, gr, planes});
}

int gsr_backward_camera(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                        const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                        const gsr_camera_gradients *camera, gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream, {"gsr_backward_camera", g, st, in, gr, planes, camera});
}

int gsr_backward_filtered(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                          const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                          const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                          gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream,
                          {"gsr_backward_camera", g, st, in, gr, planes, camera, filter});
}

int gsr_backward_ordered(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                         const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                         const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                         const gsr_backward_order *order, gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream,
                          {"gsr_backward_camera", g, st, in, gr, planes, camera, filter, order});
}

int gsr_backward_strip(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                       const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                       const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                       const gsr_backward_order *order, gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream, {"gsr_backward_camera", g, st, in, gr, planes, camera,
                                        filter, order, nullptr, true});
}

int gsr_backward_features(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                          const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                          const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                          const gsr_backward_order *order, const gsr_feature_gradients *feat,
                          gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream, {"gsr_backward_camera", g, st, in, gr, planes, camera,
                                        filter, order, feat, true});
}

int gsr_backward_abs(gsr_context *ctx, const gsr_gaussians *g, const gsr_raster_settings *st,
                     const gsr_backward_inputs *in, const gsr_plane_gradients *planes,
                     const gsr_camera_gradients *camera, const gsr_filter_settings *filter,
                     const gsr_backward_order *order, const gsr_feature_gradients *feat,
                     const gsr_abs_gradients *abs, gsr_gradients *gr, void *stream) {
    return backward_entry(ctx, stream, {"gsr_backward_camera", g, st, in, gr, planes, camera,
                                        filter, order, feat, true, abs});
}

int gsr_backward_times(gsr_context *ctx, float *ms, int n) {
    if (!ctx || (!ms && n > 0)) return fail(GSR_E_INVALID, "gsr_backward_times: bad arguments");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->bwd_timed) return fail(GSR_E_STATE, "gsr_backward_times: no timed backward yet");
    GSR_HIP(hipEventSynchronize(ctx->ev_bwd[3]), "hipEventSynchronize");
    for (int i = 0; i < 3 && i < n; ++i)
        GSR_HIP(hipEventElapsedTime(&ms[i], ctx->ev_bwd[i], ctx->ev_bwd[i + 1]),
                "hipEventElapsedTime");
    return 3;
}

int gsr_get_binning(gsr_context *ctx, uint32_t *point_list, uint32_t *point_tiles,
                    uint32_t *ranges, int64_t *list_entries, int32_t *num_tiles, void *stream) {
    if (!ctx) return fail(GSR_E_INVALID, "gsr_get_binning: NULL context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    const gsr_context::LastFrame &l = ctx->last;
    if (!l.valid) return fail(GSR_E_STATE, "gsr_get_binning: no forward yet");
    hipStream_t s = static_cast<hipStream_t>(stream);
    GSR_TRY(order_stream(ctx, s));
    const int64_t K = l.list;
    const uint64_t T = (uint64_t)l.gx * l.gy;
    const uint64_t off = (uint64_t)l.rb * l.gx;
    const uint64_t T_strip = (uint64_t)l.gx * (l.re - l.rb);
    if (list_entries) *list_entries = K;  // (tight lists: fewer than the forward's num_rendered)
    if (num_tiles) *num_tiles = (int32_t)T;
    if (point_list && K > 0) {
        if (l.id_mask != 0xFFFFFFFFu)
            GSR_HIP(gsr_launch_unpack_ids(l.point_list, K, l.id_mask, point_list, s),
                    "unpack launch");
        else
            GSR_HIP(hipMemcpyAsync(point_list, l.point_list, (size_t)K * 4,
                                   hipMemcpyDeviceToDevice, s),
                    "hipMemcpyAsync(point_list)");
    }
    if (point_tiles && K > 0) {
        if (!l.packed)
            GSR_HIP(gsr_launch_globalize_tiles(l.tiles_local, K, (uint32_t)off, point_tiles, s),
                    "globalize launch");
        else  // packed list (no key array): the tile of every pair from the ranges
            GSR_HIP(gsr_launch_fill_tiles(ctx->ranges_local.get(), (uint32_t)T_strip,
                                          (uint32_t)off, point_tiles, s),
                    "fill_tiles launch");
    }
    if (ranges) {
        GSR_HIP(hipMemsetAsync(ranges, 0, T * 8, s), "hipMemsetAsync(ranges)");
        GSR_HIP(hipMemcpyAsync(reinterpret_cast<char *>(ranges) + off * 8, ctx->ranges_local.get(),
                               T_strip * 8, hipMemcpyDeviceToDevice, s),
                "hipMemcpyAsync(ranges)");
    }
    GSR_HIP(hipStreamSynchronize(s), "gsr_get_binning");
    return GSR_OK;
}

int gsr_tile_row_pairs(gsr_context *ctx, uint32_t *row_pairs, int32_t n_rows, void *stream) {
    if (!ctx) return fail(GSR_E_INVALID, "gsr_tile_row_pairs: NULL context");
    std::lock_guard<std::mutex> lock(ctx->mu);
    if (!ctx->last.valid) return fail(GSR_E_STATE, "gsr_tile_row_pairs: no forward yet");
    const uint32_t rows = ctx->last.re - ctx->last.rb;
    if (n_rows != (int32_t)rows || (rows > 0 && !row_pairs))
        return fail(GSR_E_INVALID, "gsr_tile_row_pairs: n_rows must be the strip's " +
                                       std::to_string(rows) + " tile rows");
    GSR_TRY(order_stream(ctx, static_cast<hipStream_t>(stream)));
    GSR_HIP(gsr_launch_row_pairs(ctx->ranges_local.get(), ctx->last.gx, rows, row_pairs,
                                 static_cast<hipStream_t>(stream)),
            "row pairs launch");
    return GSR_OK;
}

int gsr_mark_visible(gsr_context *ctx, const float *means3D, int64_t P, const float *viewmatrix,
                     const float *projmatrix, uint8_t *visible, void *stream) {
    (void)projmatrix;  // upstream in_frustum only tests view-space depth
    if (!ctx || P < 0 || (P > 0 && (!means3D || !viewmatrix || !visible)))
        return fail(GSR_E_INVALID, "gsr_mark_visible: bad arguments");
    GSR_HIP(gsr_launch_mark_visible(means3D, P, viewmatrix, visible,
                                    static_cast<hipStream_t>(stream)),
            "mark_visible launch");
    return GSR_OK;
}

int gsr_depth_argsort(gsr_context *ctx, const float *xyz, int64_t P, const float *view_host16,
                      int32_t *out_index, float *out_depth, void *stream) {
    if (!ctx || P < 0 || !view_host16 || (P > 0 && (!xyz || !out_index)))
        return fail(GSR_E_INVALID, "gsr_depth_argsort: bad arguments");
    if (P > (int64_t)INT32_MAX) return fail(GSR_E_INVALID, "gsr_depth_argsort: P too large");
    std::lock_guard<std::mutex> lock(ctx->mu);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (P == 0) return GSR_OK;
    GSR_TRY(order_stream(ctx, s));
    GSR_TRY(reserve_P(ctx, P, s));
    uint32_t *k = ctx->sort_keys.get();
    GSR_HIP(gsr_launch_view_depth_keys(xyz, P, view_host16[8], view_host16[9], view_host16[10],
                                       view_host16[11], k, out_depth, s),
            "view depth launch");
    // every key is kept (no sentinel); the indices land in out_index directly (< 2^31)
    GSR_HIP(gsr_depth_sort(k, P, 0, ctx->ds_a.get(), ctx->ds_b.get(),
                           reinterpret_cast<uint32_t *>(out_index), ctx->hist.get(),
                           ctx->digit_total.get(), ctx->ds_ctl.get(), 0, gsr_depth_sort_passes(32),
                           s),
            "depth argsort launch");
    return GSR_OK;
}

}  // extern "C"
