// gs_write_ply (csrc/gs_ply.cpp) under -fsanitize=address,undefined: a small cloud written in both spaces and converted back
// with gs_convert_ply, chunk edges included, and the error paths.  Built and run by tests/test_raw_cpu.py.
//   usage: sanitize_ply_write <scratch directory>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/gsplat.h"

#define CHECK(cond)                                                               \
    do {                                                                          \
        if (!(cond)) {                                                            \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            return 1;                                                             \
        }                                                                         \
    } while (0)

// gs_ply.cpp's gs_load_ply hands its records to the library's upload; this program never loads into a context
extern "C" int gs_upload_gaussians(gs_ctx*, const void*, uint32_t) { return GS_ERR_NO_DEVICE; }

static uint32_t rng_state = 12345u;
static float uniform(float lo, float hi) {
    rng_state = rng_state * 1664525u + 1013904223u;
    return lo + (hi - lo) * (float)(rng_state >> 8) * (1.0f / 16777216.0f);
}

// n raw rows: log-scales, logits, rotations of any length; the 25 floats no call reads hold a NaN
static std::vector<float> raw_cloud(uint32_t n) {
    std::vector<float> rows((size_t)n * 84, std::nanf(""));
    for (uint32_t g = 0; g < n; ++g) {
        float* r = rows.data() + (size_t)g * 84;
        for (int k = 0; k < 3; ++k) { r[k] = uniform(-5.0f, 5.0f); r[4 + k] = uniform(-9.0f, 1.0f); }
        for (int k = 0; k < 4; ++k) r[8 + k] = uniform(-2.0f, 2.0f) + 0.01f;
        r[15] = uniform(-8.0f, 8.0f);
        for (int c = 0; c < 16; ++c)
            for (int ch = 0; ch < 3; ++ch) r[12 + 4 * c + ch] = uniform(-2.0f, 2.0f);
    }
    return rows;
}

static bool finite_fields(const std::vector<float>& rec, uint32_t n) {
    for (uint32_t g = 0; g < n; ++g)
        for (int k = 0; k < 76; ++k)
            if (!std::isfinite(rec[(size_t)g * 84 + k])) return false;
    return true;
}

int main(int argc, char** argv) {
    CHECK(argc == 2);
    const std::string dir = argv[1];
    // 1, a size inside one chunk, and sizes around the writer's chunk of 16384 rows
    const uint32_t sizes[] = {1u, 777u, 16383u, 16384u, 16385u, 40000u};
    for (uint32_t n : sizes) {
        const std::vector<float> raw = raw_cloud(n);
        const std::string a_path = dir + "/raw.ply", b_path = dir + "/records.ply";
        CHECK(gs_write_ply(a_path.c_str(), raw.data(), n, GS_PLY_FROM_RAW) == GS_OK);
        uint32_t count = 0;
        CHECK(gs_convert_ply(a_path.c_str(), nullptr, 0, &count) == GS_OK && count == n);
        std::vector<float> a((size_t)n * 84), b((size_t)n * 84);
        CHECK(gs_convert_ply(a_path.c_str(), a.data(), n, &count) == GS_OK && count == n);
        CHECK(finite_fields(a, n));
        CHECK(gs_write_ply(b_path.c_str(), a.data(), n, GS_PLY_FROM_RECORDS) == GS_OK);
        CHECK(gs_convert_ply(b_path.c_str(), b.data(), n, &count) == GS_OK && count == n);
        CHECK(finite_fields(b, n));
        for (uint32_t g = 0; g < n; ++g)                              // the same order, the positions bit for bit
            CHECK(std::memcmp(a.data() + (size_t)g * 84, b.data() + (size_t)g * 84, 12) == 0);
    }
    // records at the clamps: opacity 0 and 1, scale 0, a NaN scale
    {
        std::vector<float> rec = raw_cloud(4);
        rec[15] = 0.0f; rec[84 + 15] = 1.0f; rec[2 * 84 + 4] = 0.0f; rec[3 * 84 + 5] = std::nanf("");
        for (int g = 0; g < 4; ++g) rec[(size_t)g * 84 + 6] = 0.5f;
        const std::string path = dir + "/clamps.ply";
        CHECK(gs_write_ply(path.c_str(), rec.data(), 4, GS_PLY_FROM_RECORDS) == GS_OK);
        std::vector<float> back(4 * 84);
        uint32_t count = 0;
        CHECK(gs_convert_ply(path.c_str(), back.data(), 4, &count) == GS_OK && count == 4);
    }
    // the error paths
    const std::vector<float> one = raw_cloud(1);
    CHECK(gs_write_ply(nullptr, one.data(), 1, GS_PLY_FROM_RAW) == GS_ERR_INVALID);
    CHECK(gs_write_ply((dir + "/x.ply").c_str(), nullptr, 1, GS_PLY_FROM_RAW) == GS_ERR_INVALID);
    CHECK(gs_write_ply((dir + "/x.ply").c_str(), one.data(), 0, GS_PLY_FROM_RAW) == GS_ERR_INVALID);
    CHECK(gs_write_ply((dir + "/x.ply").c_str(), one.data(), 1, 2u) == GS_ERR_INVALID);
    CHECK(gs_write_ply((dir + "/no_such_dir/x.ply").c_str(), one.data(), 1, GS_PLY_FROM_RAW) == GS_ERR_IO);
    CHECK(std::strlen(gs_ply_last_error()) > 0);
    CHECK(gs_write_ply(dir.c_str(), one.data(), 1, GS_PLY_FROM_RECORDS) == GS_ERR_IO);      // a directory
    std::printf("sanitize_ply_write ok\n");
    return 0;
}
