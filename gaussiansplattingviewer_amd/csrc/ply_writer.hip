// ply_writer.hip -- a fit's raw scene as upstream's save_ply file, and back (include/gsr.h
// "Scene files").
//
// gsr_ply_save writes the 3D Gaussian Splatting PLY that upstream's GaussianModel.save_ply makes
// with plyfile, byte for byte, from the six raw tensors of a fit.  With device tensors the rows
// are packed on the GPU (k_ply_pack) into one of two device slots, copied into one of two pinned
// host slots and written from there while the next chunk packs and copies: no full-size host
// copy exists.  gsr_ply_load_scene is the inverse: the raw tensors with the bits of the file, for
// everything the activated reader (ply_loader.hip) accepts -- its header parser and value
// conversion are used through gsr_internal.h -- and any SH degree 0..4.
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <cerrno>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

#include "gsr.h"
#include "gsr_internal.h"

using namespace gsr_ply;

namespace {

// ---- the column table ----------------------------------------------------------------------
// Words per scene row: xyz 3, f_dc 3, f_rest 3 (M - 1), opacity 1, scaling 3, rotation 4.
constexpr uint32_t kMaxCoeffs = 25;
constexpr uint32_t kMaxSceneWords = 14 + 3 * (kMaxCoeffs - 1);  // 86

// The scene's tensors as words: the writer and the reader copy bits, never floats.
struct Tensors {
    uint32_t *xyz, *dc, *rest, *opacity, *scaling, *rotation;
};

// Shapes of one file: M of the tensors, Mo of the file, R words per file row.
struct Shape {
    uint32_t M, Mo, R, K, Ko;  // K = 3 (M - 1) words of an f_rest row, Ko = Mo - 1
    uint32_t mul;              // ceil(2^32 / R): __umulhi(w, mul) == w / R for w R < 2^32
};

inline uint32_t mul_of(uint32_t d) { return (uint32_t)(((1ull << 32) + d - 1) / d); }

Shape shape_of(uint32_t M, uint32_t Mo) {
    Shape s;
    s.M = M;
    s.Mo = Mo;
    s.R = 17 + 3 * (Mo - 1);
    s.K = 3 * (M - 1);
    s.Ko = Mo - 1;
    s.mul = mul_of(s.R);
    return s;
}

// The word of column `col` of a file row, from the row's words in six arrays: x = xyz + 3 row,
// d = f_dc + 3 row, f = f_rest + K row, o = opacity + row, sc = scaling + 3 row, q = rotation +
// 4 row.  No division: the channel of an f_rest column is two compares.
__host__ __device__ __forceinline__ uint32_t row_word(const Shape &s, uint32_t col,
                                                      const uint32_t *x, const uint32_t *d,
                                                      const uint32_t *f, const uint32_t *o,
                                                      const uint32_t *sc, const uint32_t *q) {
    if (col < 3) return x[col];
    if (col < 6) return 0u;  // nx ny nz: +0.0
    if (col < 9) return d[col - 6];
    const uint32_t t = col - 9;
    if (t < 3 * s.Ko) {
        const uint32_t c = (t >= s.Ko) + (t >= 2 * s.Ko), j = t - c * s.Ko;
        return j + 1 < s.M ? f[3 * j + c] : 0u;
    }
    const uint32_t u = t - 3 * s.Ko;
    if (u == 0) return o[0];
    if (u < 4) return sc[u - 1];
    return q[u - 4];
}

// ---- k_ply_pack ------------------------------------------------------------------------------
// One block owns kPackRows whole rows of the chunk.  Each tensor's words for those rows are one
// contiguous span: the block loads the six spans with consecutive lanes on consecutive words
// (every source word is requested once) into LDS, then writes its kPackRows x R output words,
// which are one contiguous span too, 16 bytes per lane in output order (every output word is
// stored once, whole lines).  Output word w of the block is (row, col) = (w / R, w % R) by a
// 32-bit multiply-high: w < kPackRows x R <= 5504.  The kernel sees the chunk only -- the host
// has added the chunk's first row to every pointer -- so no index in here exceeds
// GSR_PLY_MAX_CHUNK_ROWS x 86 < 2^27 words, and the block's bases are size_t.
constexpr uint32_t kPackRows = 64, kPackThreads = 256;

struct PackArgs {
    Tensors t;      // at the chunk's first row
    uint32_t *out;  // the slot: n x R words, 16-byte aligned
    uint32_t n;     // rows of the chunk
    Shape s;
};

__global__ __launch_bounds__(kPackThreads) void k_ply_pack(const PackArgs a) {
    __shared__ uint32_t lds[kPackRows * kMaxSceneWords];
    const uint32_t r0 = blockIdx.x * kPackRows;
    const uint32_t n = min(kPackRows, a.n - r0);
    const Shape s = a.s;
    uint32_t *const lx = lds, *const ld = lx + 3 * kPackRows, *const lf = ld + 3 * kPackRows,
                    *const lo = lf + s.K * kPackRows, *const ls = lo + kPackRows,
                    *const lq = ls + 3 * kPackRows;
    const struct {
        const uint32_t *src;
        uint32_t *dst, k;
    } spans[6] = {{a.t.xyz, lx, 3u},     {a.t.dc, ld, 3u},      {a.t.rest, lf, s.K},
                  {a.t.opacity, lo, 1u}, {a.t.scaling, ls, 3u}, {a.t.rotation, lq, 4u}};
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const uint32_t words = n * spans[i].k;
        const uint32_t *src = spans[i].src + (size_t)r0 * spans[i].k;
        for (uint32_t w = threadIdx.x; w < words; w += kPackThreads) spans[i].dst[w] = src[w];
    }
    __syncthreads();
    auto word = [&](uint32_t w) {
        const uint32_t row = __umulhi(w, s.mul), col = w - row * s.R;
        return row_word(s, col, lx + 3 * row, ld + 3 * row, lf + s.K * row, lo + row, ls + 3 * row,
                        lq + 4 * row);
    };
    // r0 R is a multiple of 64 words and the slot is 16-byte aligned: uint4 stores
    uint32_t *out = a.out + (size_t)r0 * s.R;
    const uint32_t total = n * s.R;
    for (uint32_t w = 4 * threadIdx.x; w < total; w += 4 * kPackThreads) {
        if (w + 4 <= total) {
            uint4 v;
            v.x = word(w);
            v.y = word(w + 1);
            v.z = word(w + 2);
            v.w = word(w + 3);
            *reinterpret_cast<uint4 *>(out + w) = v;
        } else {
            for (uint32_t i = w; i < total; ++i) out[i] = word(i);
        }
    }
}

// The same rows in plain C++ (device == 0, and the specification the kernel is tested against).
void pack_rows_host(const Tensors &t, const Shape &s, int64_t b, int64_t e, uint32_t *out) {
    for (int64_t r = b; r < e; ++r)
        for (uint32_t col = 0; col < s.R; ++col)
            *out++ = row_word(s, col, t.xyz + 3 * r, t.dc + 3 * r,
                              t.rest ? t.rest + (int64_t)s.K * r : nullptr, t.opacity + r,
                              t.scaling + 3 * r, t.rotation + 4 * r);
}

// ---- k_ply_unpack ----------------------------------------------------------------------------
// One thread per output word of the chunk, in the order [xyz | f_dc | f_rest | opacity | scaling
// | rotation], so a wave stores consecutive words of one tensor.  Word i of a tensor with k words
// per row is (row, e) = (i / k, i % k) by multiply-high (i < kUnpackMaxRows x 72, times k < 2^32),
// and comes from column col[first + e] of file row `row` in the slot (S words per row).
constexpr int64_t kUnpackMaxRows = 1 << 18;
constexpr int64_t kUnpackSlotBytes = 64 << 20;

struct UnpackArgs {
    const uint32_t *in;  // the slot: n rows of S words
    Tensors t;           // at the chunk's first row
    uint32_t n, S, K, mul_K;
    uint16_t col[kMaxSceneWords];  // source column per scene word: xyz, f_dc, f_rest[j][c], ...
};

__global__ __launch_bounds__(256) void k_ply_unpack(const UnpackArgs a) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    const uint32_t n = a.n, K = a.K;
    const uint32_t b1 = 3 * n, b2 = 6 * n, b3 = b2 + K * n, b4 = b3 + n, b5 = b4 + 3 * n,
                   b6 = b5 + 4 * n;
    if (w >= b6) return;
    constexpr uint32_t kMul3 = 0x55555556u;  // ceil(2^32 / 3)
    uint32_t *dst, i, row, k, first;
    if (w < b1) {
        dst = a.t.xyz, i = w, k = 3, first = 0, row = __umulhi(i, kMul3);
    } else if (w < b2) {
        dst = a.t.dc, i = w - b1, k = 3, first = 3, row = __umulhi(i, kMul3);
    } else if (w < b3) {
        dst = a.t.rest, i = w - b2, k = K, first = 6, row = __umulhi(i, a.mul_K);
    } else if (w < b4) {
        dst = a.t.opacity, i = w - b3, k = 1, first = 6 + K, row = i;
    } else if (w < b5) {
        dst = a.t.scaling, i = w - b4, k = 3, first = 7 + K, row = __umulhi(i, kMul3);
    } else {
        dst = a.t.rotation, i = w - b5, k = 4, first = 10 + K, row = i >> 2;
    }
    const uint32_t e = i - row * k;
    dst[i] = a.in[row * a.S + a.col[first + e]];
}

// ---- arguments -------------------------------------------------------------------------------
int refuse(const char *fn, const std::string &msg) {
    return gsr_ply::fail(GSR_E_INVALID, std::string(fn) + ": " + msg);
}

bool is_coeff_count(int32_t m) { return m == 1 || m == 4 || m == 9 || m == 16 || m == 25; }

// What gsr_ply_save and gsr_ply_load_scene refuse before anything else happens.
int check_scene(const char *fn, const char *path, const gsr_ply_scene *sc) {
    if (!path) return refuse(fn, "NULL path");
    if (!sc) return refuse(fn, "NULL scene");
    if (sc->P < 0) return refuse(fn, "P < 0");
    if (sc->P >= ((int64_t)1 << 30)) return refuse(fn, "P >= 2^30");
    if (!is_coeff_count(sc->sh_coeffs))
        return refuse(fn, "sh_coeffs " + std::to_string(sc->sh_coeffs) +
                              " is not (d + 1)^2 for a degree d = 0..4");
    if (sc->chunk_rows < 0) return refuse(fn, "chunk_rows < 0");
    if (sc->P > 0) {
        if (!sc->xyz || !sc->f_dc || !sc->opacity || !sc->scaling || !sc->rotation)
            return refuse(fn, "NULL tensor (xyz, f_dc, opacity, scaling and rotation are required)");
        if (sc->sh_coeffs > 1 && !sc->f_rest)
            return refuse(fn, "NULL f_rest with sh_coeffs > 1");
    }
    return GSR_OK;
}

Tensors tensors_of(const gsr_ply_scene *sc) {
    auto w = [](float *p) { return reinterpret_cast<uint32_t *>(p); };
    return {w(sc->xyz), w(sc->f_dc), w(sc->f_rest), w(sc->opacity), w(sc->scaling), w(sc->rotation)};
}

Tensors at_row(const Tensors &t, int64_t r, uint32_t K) {
    return {t.xyz + 3 * r, t.dc + 3 * r, t.rest ? t.rest + (int64_t)K * r : nullptr, t.opacity + r,
            t.scaling + 3 * r, t.rotation + 4 * r};
}

int64_t chunk_rows_of(const gsr_ply_scene *sc, int64_t cap) {
    const int64_t want = sc->chunk_rows ? sc->chunk_rows : GSR_PLY_CHUNK_ROWS;
    return std::max<int64_t>(1, std::min(std::min(want, cap), std::max<int64_t>(sc->P, 1)));
}

// ---- the file ---------------------------------------------------------------------------------
std::string header_text(int64_t P, uint32_t Mo) {
    std::string h = "ply\nformat binary_little_endian 1.0\nelement vertex " + std::to_string(P) + "\n";
    for (const char *n : {"x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"})
        h += std::string("property float ") + n + "\n";
    for (uint32_t i = 0; i < 3 * (Mo - 1); ++i) h += "property float f_rest_" + std::to_string(i) + "\n";
    for (const char *n : {"opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"})
        h += std::string("property float ") + n + "\n";
    return h + "end_header\n";
}

// The file being written: "<path>.tmp.<pid>", removed by the destructor unless commit() renamed it.
struct TempFile {
    std::string tmp, path;
    int fd = -1;
    ~TempFile() {
        if (fd >= 0) close(fd);
        if (!tmp.empty()) unlink(tmp.c_str());
    }
    int create(const char *p) {
        path = p;
        const std::string name = path + ".tmp." + std::to_string((long long)getpid());
        fd = open(name.c_str(), O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
        if (fd < 0)
            return gsr_ply::fail(GSR_E_INVALID, "cannot create " + name + ": " + std::strerror(errno));
        tmp = name;
        return GSR_OK;
    }
    int write_all(const void *data, size_t n) {
        const char *p = static_cast<const char *>(data);
        while (n > 0) {
            const ssize_t k = ::write(fd, p, n);
            if (k < 0 && errno == EINTR) continue;
            if (k <= 0)
                return gsr_ply::fail(GSR_E_INVALID, "short write to " + tmp + ": " +
                                                        (k < 0 ? std::strerror(errno) : "no progress"));
            p += k;
            n -= (size_t)k;
        }
        return GSR_OK;
    }
    int commit() {
        const int rc = close(fd);
        fd = -1;
        if (rc != 0)
            return gsr_ply::fail(GSR_E_INVALID, "short write to " + tmp + ": " + std::strerror(errno));
        if (rename(tmp.c_str(), path.c_str()) != 0)
            return gsr_ply::fail(GSR_E_INVALID, "cannot rename " + tmp + " to " + path + ": " +
                                                    std::strerror(errno));
        tmp.clear();
        return GSR_OK;
    }
};

// Two device slots, two pinned host slots and their events, freed by the destructor.
struct Staging {
    uint32_t *dev = nullptr, *pin = nullptr;
    hipEvent_t ev[2] = {nullptr, nullptr};
    size_t slot_words = 0;
    ~Staging() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
        if (pin) (void)hipHostFree(pin);
        if (dev) (void)hipFree(dev);
    }
    int alloc(size_t words) {
        slot_words = (words + 63) / 64 * 64;  // the second slot stays 256-byte aligned
        const size_t bytes = 2 * slot_words * sizeof(uint32_t);
        if (hipMalloc(reinterpret_cast<void **>(&dev), bytes) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void **>(&pin), bytes) != hipSuccess) {
            (void)hipGetLastError();
            return gsr_ply::fail(GSR_E_NOMEM, "staging allocation failed");
        }
        for (hipEvent_t &e : ev)
            if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
                (void)hipGetLastError();
                return gsr_ply::fail(GSR_E_HIP, "hipEventCreate failed");
            }
        return GSR_OK;
    }
};

int hip_fail(const char *what) {
    (void)hipGetLastError();
    return gsr_ply::fail(GSR_E_HIP, std::string(what) + " failed");
}

int save_device(TempFile &f, const Tensors &t, const Shape &s, int64_t P, int64_t rows,
                hipStream_t st) {
    Staging g;
    GSR_TRY_PLY(g.alloc((size_t)rows * s.R));
    // chunk c packs and copies on the stream while the host writes chunk c - 1
    int64_t prev_n = 0;
    int c = 0;
    for (int64_t b = 0; b < P; b += rows, ++c) {
        const int64_t n = std::min(rows, P - b);
        const int slot = c & 1;
        PackArgs a{at_row(t, b, s.K), g.dev + slot * g.slot_words, (uint32_t)n, s};
        const uint32_t blocks = (uint32_t)((n + kPackRows - 1) / kPackRows);
        hipLaunchKernelGGL(k_ply_pack, dim3(blocks), dim3(kPackThreads), 0, st, a);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(g.pin + slot * g.slot_words, a.out, (size_t)n * s.R * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipEventRecord(g.ev[slot], st) != hipSuccess) {
            (void)hipStreamSynchronize(st);
            return hip_fail("packing the PLY rows");
        }
        if (c > 0) {
            if (hipEventSynchronize(g.ev[slot ^ 1]) != hipSuccess) return hip_fail("packing the PLY rows");
            const int rc = f.write_all(g.pin + (slot ^ 1) * g.slot_words,
                                       (size_t)prev_n * s.R * sizeof(uint32_t));
            if (rc != GSR_OK) {
                (void)hipStreamSynchronize(st);  // the slots are freed on return
                return rc;
            }
        }
        prev_n = n;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return hip_fail("packing the PLY rows");
    if (c > 0)
        GSR_TRY_PLY(f.write_all(g.pin + ((c - 1) & 1) * g.slot_words,
                                (size_t)prev_n * s.R * sizeof(uint32_t)));
    return GSR_OK;
}

int save_host(TempFile &f, const Tensors &t, const Shape &s, int64_t P, int64_t rows) {
    std::vector<uint32_t> buf((size_t)rows * s.R);
    for (int64_t b = 0; b < P; b += rows) {
        const int64_t e = std::min(P, b + rows);
        pack_rows_host(t, s, b, e, buf.data());
        GSR_TRY_PLY(f.write_all(buf.data(), (size_t)(e - b) * s.R * sizeof(uint32_t)));
    }
    return GSR_OK;
}

// ---- the reader -------------------------------------------------------------------------------
// Indices into Header::props in scene word order: xyz 3, f_dc 3, f_rest[j][c] (3 (M - 1)),
// opacity, scale 3, rot 4.
struct SceneLayout {
    uint32_t M = 0, K = 0;
    std::vector<int> src;
};

int make_scene_layout(const Header &h, SceneLayout &L) {
    auto need = [&](const std::string &n, int &out) {
        if ((out = find_prop(h, n)) < 0)
            return gsr_ply::fail(GSR_E_INVALID, "PLY vertex has no property " + n);
        return (int)GSR_OK;
    };
    int xyz[3], dc[3], opacity;
    const char *names[3] = {"x", "y", "z"};
    for (int i = 0; i < 3; ++i) GSR_TRY_PLY(need(names[i], xyz[i]));
    for (int i = 0; i < 3; ++i) GSR_TRY_PLY(need("f_dc_" + std::to_string(i), dc[i]));
    GSR_TRY_PLY(need("opacity", opacity));
    const std::vector<int> rest = prefixed(h, "f_rest_");
    for (uint32_t m : {1u, 4u, 9u, 16u, 25u})
        if (rest.size() == 3 * (m - 1)) L.M = m;
    if (!L.M)
        return gsr_ply::fail(GSR_E_INVALID,
                             "expected 3 (M - 1) f_rest_* properties for M = 1, 4, 9, 16 or 25, found " +
                                 std::to_string(rest.size()));
    L.K = 3 * (L.M - 1);
    const std::vector<int> sc = prefixed(h, "scale_"), ro = prefixed(h, "rot");
    if (sc.size() != 3) return gsr_ply::fail(GSR_E_INVALID, "expected 3 scale_* properties");
    if (ro.size() != 4) return gsr_ply::fail(GSR_E_INVALID, "expected 4 rot* properties");
    L.src.assign(xyz, xyz + 3);
    L.src.insert(L.src.end(), dc, dc + 3);
    for (uint32_t j = 0; j + 1 < L.M; ++j)
        for (uint32_t c = 0; c < 3; ++c) L.src.push_back(rest[c * (L.M - 1) + j]);
    L.src.push_back(opacity);
    L.src.insert(L.src.end(), sc.begin(), sc.end());
    L.src.insert(L.src.end(), ro.begin(), ro.end());
    return GSR_OK;
}

// Scene word t of row r: where it goes.
inline uint32_t *scene_word(const Tensors &o, uint32_t K, int64_t r, uint32_t t) {
    if (t < 3) return o.xyz + 3 * r + t;
    if (t < 6) return o.dc + 3 * r + (t - 3);
    if (t < 6 + K) return o.rest + (int64_t)K * r + (t - 6);
    if (t == 6 + K) return o.opacity + r;
    if (t < 10 + K) return o.scaling + 3 * r + (t - 7 - K);
    return o.rotation + 4 * r + (t - 10 - K);
}

inline uint32_t f32_bits(float v) {
    uint32_t u;
    std::memcpy(&u, &v, 4);
    return u;
}

// A float property is a bit copy (numpy's astype(float32) of float32 data); every other type goes
// through the activated reader's conversion.
void convert_binary_scene(const Mapped &m, const Header &h, const SceneLayout &L, const Tensors &o) {
    const bool swap = h.format == Header::BBE;
    const unsigned char *data = m.p + h.data_offset;
    const uint32_t words = 14 + L.K;
    for (int64_t r = 0; r < h.count; ++r) {
        const unsigned char *rec = data + (size_t)r * (size_t)h.stride;
        for (uint32_t t = 0; t < words; ++t) {
            const Prop &p = h.props[L.src[t]];
            uint32_t u;
            if (p.type == PType::F32) {
                unsigned char b[4];
                for (int i = 0; i < 4; ++i) b[i] = rec[p.offset + (swap ? 3 - i : i)];
                std::memcpy(&u, b, 4);
            } else {
                u = f32_bits(as_f32(read_value(rec + p.offset, p.type, swap)));
            }
            *scene_word(o, L.K, r, t) = u;
        }
    }
}

int convert_ascii_scene(const Mapped &m, const Header &h, const SceneLayout &L, const Tensors &o) {
    const char *s = reinterpret_cast<const char *>(m.p) + h.data_offset;
    const char *end = reinterpret_cast<const char *>(m.p) + m.size;
    std::vector<double> v(h.props.size());
    const uint32_t words = 14 + L.K;
    for (int64_t r = 0; r < h.count; ++r) {
        for (size_t k = 0; k < h.props.size(); ++k)
            GSR_TRY_PLY(ascii_value(s, end, h.props[k].type, v[k]));
        for (uint32_t t = 0; t < words; ++t)
            *scene_word(o, L.K, r, t) = f32_bits(as_f32(v[L.src[t]]));
    }
    return GSR_OK;
}

// Little-endian rows of float properties only: chunks of file rows through pinned staging to a
// device slot, scattered by k_ply_unpack.
int load_device_fast(const Mapped &m, const Header &h, const SceneLayout &L, const Tensors &o,
                     int64_t rows, hipStream_t st) {
    const uint32_t S = (uint32_t)(h.stride / 4);
    Staging g;
    GSR_TRY_PLY(g.alloc((size_t)rows * S));
    UnpackArgs a{};
    a.S = S;
    a.K = L.K;
    a.mul_K = L.K ? mul_of(L.K) : 0;
    for (size_t t = 0; t < L.src.size(); ++t) a.col[t] = (uint16_t)(h.props[L.src[t]].offset / 4);
    const unsigned char *data = m.p + h.data_offset;
    bool used[2] = {false, false};
    int slot = 0;
    for (int64_t b = 0; b < h.count; b += rows, slot ^= 1) {
        const int64_t n = std::min(rows, h.count - b);
        if (used[slot] && hipEventSynchronize(g.ev[slot]) != hipSuccess)
            return hip_fail("upload of the PLY rows");
        const size_t bytes = (size_t)n * (size_t)h.stride;
        std::memcpy(g.pin + slot * g.slot_words, data + (size_t)b * (size_t)h.stride, bytes);
        a.in = g.dev + slot * g.slot_words;
        a.t = at_row(o, b, L.K);
        a.n = (uint32_t)n;
        const uint32_t blocks = (uint32_t)((n * (14 + L.K) + 255) / 256);
        bool ok = hipMemcpyAsync(g.dev + slot * g.slot_words, g.pin + slot * g.slot_words, bytes,
                                 hipMemcpyHostToDevice, st) == hipSuccess;
        if (ok) {
            hipLaunchKernelGGL(k_ply_unpack, dim3(blocks), dim3(256), 0, st, a);
            ok = hipGetLastError() == hipSuccess && hipEventRecord(g.ev[slot], st) == hipSuccess;
        }
        if (!ok) {
            (void)hipStreamSynchronize(st);
            return hip_fail("upload of the PLY rows");
        }
        used[slot] = true;
    }
    if (hipStreamSynchronize(st) != hipSuccess) return hip_fail("upload of the PLY rows");
    return GSR_OK;
}

int read_header(const char *path, Mapped &m, Header &h, SceneLayout &L) {
    GSR_TRY_PLY(map_file(path, m));
    GSR_TRY_PLY(parse_header(m, h));
    return make_scene_layout(h, L);
}

}  // namespace

extern "C" {

int gsr_ply_save(const char *path, const gsr_ply_scene *scene, int device, void *stream) {
    const char *fn = "gsr_ply_save";
    GSR_TRY_PLY(check_scene(fn, path, scene));
    const int32_t Mo = scene->file_sh_coeffs ? scene->file_sh_coeffs : scene->sh_coeffs;
    if (!is_coeff_count(Mo))
        return refuse(fn, "file_sh_coeffs " + std::to_string(Mo) +
                              " is not (d + 1)^2 for a degree d = 0..4");
    if (Mo < scene->sh_coeffs)
        return refuse(fn, "file_sh_coeffs " + std::to_string(Mo) + " < sh_coeffs " +
                              std::to_string(scene->sh_coeffs) + " (a file cannot drop coefficients)");
    const Shape s = shape_of((uint32_t)scene->sh_coeffs, (uint32_t)Mo);
    const int64_t P = scene->P;
    const int64_t rows = chunk_rows_of(scene, GSR_PLY_MAX_CHUNK_ROWS);
    TempFile f;
    GSR_TRY_PLY(f.create(path));
    const std::string head = header_text(P, s.Mo);
    GSR_TRY_PLY(f.write_all(head.data(), head.size()));
    if (P > 0) {
        const Tensors t = tensors_of(scene);
        GSR_TRY_PLY(device ? save_device(f, t, s, P, rows, static_cast<hipStream_t>(stream))
                           : save_host(f, t, s, P, rows));
    }
    return f.commit();
}

int gsr_ply_probe_scene(const char *path, gsr_ply_scene *info) {
    if (!path || !info) return refuse("gsr_ply_probe_scene", "NULL argument");
    Mapped m;
    Header h;
    SceneLayout L;
    GSR_TRY_PLY(read_header(path, m, h, L));
    if (h.count >= ((int64_t)1 << 30))
        return refuse("gsr_ply_probe_scene", "the file has 2^30 vertices or more");
    info->P = h.count;
    info->sh_coeffs = (int32_t)L.M;
    return GSR_OK;
}

int gsr_ply_load_scene(const char *path, gsr_ply_scene *scene, int device, void *stream) {
    const char *fn = "gsr_ply_load_scene";
    GSR_TRY_PLY(check_scene(fn, path, scene));
    Mapped m;
    Header h;
    SceneLayout L;
    GSR_TRY_PLY(read_header(path, m, h, L));
    if (scene->P != h.count || (uint32_t)scene->sh_coeffs != L.M)
        return refuse(fn, "scene->P / sh_coeffs (" + std::to_string(scene->P) + ", " +
                              std::to_string(scene->sh_coeffs) + ") are not the file's (" +
                              std::to_string(h.count) + ", " + std::to_string(L.M) +
                              "): probe first");
    const int64_t P = h.count;
    if (P == 0) return GSR_OK;
    const Tensors out = tensors_of(scene);
    if (!device) {
        if (h.format == Header::ASCII) return convert_ascii_scene(m, h, L, out);
        convert_binary_scene(m, h, L, out);
        return GSR_OK;
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    bool all_float = h.format == Header::BLE;
    for (const Prop &p : h.props) all_float = all_float && p.type == PType::F32;
    if (all_float && h.stride / 4 <= 65535) {
        const int64_t cap = std::min<int64_t>(kUnpackMaxRows, kUnpackSlotBytes / h.stride);
        return load_device_fast(m, h, L, out, chunk_rows_of(scene, std::max<int64_t>(cap, 1)), st);
    }
    // every other file: the host conversion into one buffer laid out like the six tensors, then
    // one copy each
    const uint32_t k[6] = {3, 3, L.K, 1, 3, 4};
    std::vector<uint32_t> buf((size_t)P * (14 + L.K));
    Tensors hb;
    uint32_t **hp[6] = {&hb.xyz, &hb.dc, &hb.rest, &hb.opacity, &hb.scaling, &hb.rotation};
    uint32_t *const dp[6] = {out.xyz, out.dc, out.rest, out.opacity, out.scaling, out.rotation};
    size_t at = 0;
    for (int i = 0; i < 6; ++i) {
        *hp[i] = buf.data() + at;
        at += (size_t)P * k[i];
    }
    if (h.format == Header::ASCII)
        GSR_TRY_PLY(convert_ascii_scene(m, h, L, hb));
    else
        convert_binary_scene(m, h, L, hb);
    bool ok = true;
    for (int i = 0; i < 6; ++i)
        if (k[i])
            ok = ok && hipMemcpyAsync(dp[i], *hp[i], (size_t)P * k[i] * sizeof(uint32_t),
                                      hipMemcpyHostToDevice, st) == hipSuccess;
    ok = hipStreamSynchronize(st) == hipSuccess && ok;
    if (!ok) return hip_fail("upload of the PLY data");
    return GSR_OK;
}

}  // extern "C"
