// Host-only driver for the sanitizer build of the scene writer and reader (csrc/ply_writer.hip
// with csrc/ply_loader.hip).  Built by tests/test_ply_scene_asan.py with `-Xarch_host
// -fsanitize=address,undefined`: saves a scene of P = 257 rows and M = 16 coefficients from
// exactly-sized heap arrays in chunks of 100 rows (device == 0: no HIP call), probes the file,
// loads it back into exactly-sized arrays and compares the words; then the same padded to 25
// coefficients, a degree-0 scene without f_rest, and an empty scene.  Prints one line per step;
// the exit status is the number of steps that went wrong.  No GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "gsr.h"

static std::string g_msg;
int gsr_set_error(int code, const std::string &msg) {  // api.hip's, for this driver alone
    g_msg = msg;
    return code;
}

struct Scene {
    std::vector<float> xyz, dc, rest, opacity, scaling, rotation;
    gsr_ply_scene c{};
    Scene(int64_t P, int32_t M, bool fill) {
        const size_t n = (size_t)P;
        xyz.resize(3 * n), dc.resize(3 * n), rest.resize(3 * (size_t)(M - 1) * n);
        opacity.resize(n), scaling.resize(3 * n), rotation.resize(4 * n);
        uint32_t x = 12345u;
        for (std::vector<float> *v : {&xyz, &dc, &rest, &opacity, &scaling, &rotation})
            for (float &f : *v) {
                x = x * 1664525u + 1013904223u;  // every bit pattern, NaNs included
                const uint32_t w = fill ? x : 0xdeadbeefu;
                std::memcpy(&f, &w, 4);
            }
        c.P = P;
        c.sh_coeffs = M;
        c.xyz = xyz.data(), c.f_dc = dc.data(), c.f_rest = rest.empty() ? nullptr : rest.data();
        c.opacity = opacity.data(), c.scaling = scaling.data(), c.rotation = rotation.data();
    }
    bool same(const Scene &o) const {
        auto eq = [](const std::vector<float> &a, const std::vector<float> &b) {
            return a.size() == b.size() &&
                   (a.empty() || std::memcmp(a.data(), b.data(), 4 * a.size()) == 0);
        };
        return eq(xyz, o.xyz) && eq(dc, o.dc) && eq(rest, o.rest) && eq(opacity, o.opacity) &&
               eq(scaling, o.scaling) && eq(rotation, o.rotation);
    }
};

static int round_trip(const std::string &path, int64_t P, int32_t M, int32_t Mo, int64_t chunk) {
    Scene a(P, M, true);
    a.c.file_sh_coeffs = Mo;
    a.c.chunk_rows = chunk;
    int rc = gsr_ply_save(path.c_str(), &a.c, 0, nullptr);
    gsr_ply_scene info{};
    if (rc == 0) rc = gsr_ply_probe_scene(path.c_str(), &info);
    const int32_t Mf = Mo ? Mo : M;
    bool ok = rc == 0 && info.P == P && info.sh_coeffs == Mf;
    if (ok) {
        Scene b(P, Mf, false);
        rc = gsr_ply_load_scene(path.c_str(), &b.c, 0, nullptr);
        ok = rc == 0;
        if (ok && Mf == M) ok = a.same(b);
        if (ok && Mf != M) {  // padded: the scene's coefficients, then +0.0
            ok = std::memcmp(b.xyz.data(), a.xyz.data(), 12 * (size_t)P) == 0;
            for (int64_t p = 0; ok && p < P; ++p)
                for (int32_t j = 0; ok && j < Mf - 1; ++j)
                    for (int c = 0; ok && c < 3; ++c) {
                        uint32_t got, want = 0;
                        std::memcpy(&got, &b.rest[(size_t)(p * (Mf - 1) + j) * 3 + c], 4);
                        if (j < M - 1) std::memcpy(&want, &a.rest[(size_t)(p * (M - 1) + j) * 3 + c], 4);
                        ok = got == want;
                    }
        }
    }
    std::printf("%s P=%lld M=%d Mo=%d chunk=%lld rc=%d %s\n", ok ? "ok" : "FAILED", (long long)P, M,
                Mo, (long long)chunk, rc, rc ? g_msg.c_str() : "");
    return ok ? 0 : 1;
}

int main(int argc, char **argv) {
    if (argc != 2) return 100;
    const std::string path = std::string(argv[1]) + "/scene.ply";
    int bad = 0;
    bad += round_trip(path, 257, 16, 0, 100);
    bad += round_trip(path, 257, 16, 25, 100);
    bad += round_trip(path, 257, 1, 0, 256);
    bad += round_trip(path, 3, 4, 16, 0);
    bad += round_trip(path, 0, 9, 0, 0);
    // refusals must not touch the arrays either
    Scene s(4, 4, true);
    s.c.file_sh_coeffs = 1;
    bad += gsr_ply_save(path.c_str(), &s.c, 0, nullptr) == GSR_E_INVALID ? 0 : 1;
    bad += gsr_ply_save((std::string(argv[1]) + "/none/x.ply").c_str(), &s.c, 0, nullptr) ==
                   GSR_E_INVALID ? 0 : 1;
    return bad;
}
