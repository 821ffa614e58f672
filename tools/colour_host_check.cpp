// Stand-alone CPU program over the host helpers and the arithmetic of the camera front end's crop and colour jitter
// (agplace_amd/csrc/colour.hpp: the text the kernels of csrc/jitter.hip compile).  No GPU, no Python.
//
//   clang++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all tools/colour_host_check.cpp -o colour_host_check
//   ./colour_host_check                self-checks: crop origins against Python's round, hostile parameter records, every op on
//                                      a sweep of colours; exit status 0 and "ok" when all hold
//   ./colour_host_check dump FILE      writes rgb_to_hsv and hsv_to_rgb of all 2^24 inputs (3 bytes each, input order r/H major),
//                                      then blend(deg, x, a) for all byte pairs at the alphas 0, 1/32 .. 2 -- to be compared
//                                      with tests/colour_ref.py (numpy, held to Pillow by tests/test_colour_ref.py)
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../agplace_amd/csrc/colour.hpp"

using namespace agp_colour;

static int fails = 0;
#define CHECK(c)                                                     \
    do {                                                             \
        if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } \
    } while (0)

static int dump(const char* path) {
    FILE* f = std::fopen(path, "wb");
    if (!f) return 2;
    std::vector<uint8_t> buf((size_t)3 << 24);
    for (int pass = 0; pass < 2; ++pass) {
        for (uint32_t v = 0; v < (1u << 24); ++v) {
            const rgb8 p = {(int)(v >> 16), (int)((v >> 8) & 255), (int)(v & 255)};
            const rgb8 o = pass == 0 ? rgb_to_hsv(p) : hsv_to_rgb(p);
            buf[3 * (size_t)v] = (uint8_t)o.r; buf[3 * (size_t)v + 1] = (uint8_t)o.g; buf[3 * (size_t)v + 2] = (uint8_t)o.b;
        }
        std::fwrite(buf.data(), 1, buf.size(), f);
    }
    for (int k = 0; k <= 64; ++k) {
        const float a = (float)k / 32.f;
        for (int d = 0; d < 256; ++d)
            for (int x = 0; x < 256; ++x) buf[(size_t)d * 256 + x] = (uint8_t)blend(d, x, a);
        std::fwrite(buf.data(), 1, 65536, f);
    }
    return std::fclose(f) == 0 ? 0 : 2;
}

int main(int argc, char** argv) {
    if (argc == 3 && !std::strcmp(argv[1], "dump")) return dump(argv[2]);
    // crop origins: Python's round((n - c) / 2.0) is nearbyint in the default rounding mode
    for (int n = 1; n <= 300; ++n)
        for (int c = 1; c <= n; ++c) CHECK(crop_origin(n, c) == (int)std::nearbyint((n - c) / 2.0));
    CHECK(crop_origin(70, 37) == 16 && crop_origin(72, 37) == 18 && crop_origin(16384, 1) == 8192);
    // hostile records read as "no op" / shift 0 and never index outside anything
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float bad[RECORD] = {nan, -1.f, 5.f, inf, nan, inf, -inf, 1e30f};
    const record rb = load_record(bad);
    for (int k = 0; k < 4; ++k) CHECK(rb.op[k] == OP_NONE);
    CHECK(rb.shift == 0 && contrast_pos(rb) == -1);
    const float weird[RECORD] = {1.f, 2.f, 3.f, 4.f, nan, inf, -inf, 255.f};
    const record rw = load_record(weird);
    CHECK(contrast_pos(rw) == 1 && rw.shift == 255);
    // every op over a sweep of colours, with factors that clip both ways and non-finite ones: bytes stay bytes
    const float facs[] = {0.f, 0.3f, 1.f, 1.0000001f, 1.9f, 7.f, -3.f, nan, inf, -inf};
    for (float fa : facs) {
        record c = rw;
        c.fb = c.fc = c.fs = fa;
        for (int r = 0; r < 256; r += 5)
            for (int g = 0; g < 256; g += 7)
                for (int b = 0; b < 256; b += 3) {
                    const rgb8 o = apply_ops(rgb8{r, g, b}, c, 0, 4, 117);
                    CHECK(o.r >= 0 && o.r <= 255 && o.g >= 0 && o.g <= 255 && o.b >= 0 && o.b <= 255);
                }
    }
    // the identity record leaves a pixel alone; hue shift 0 is NOT the identity in general but keeps greys
    const float none[RECORD] = {0, 0, 0, 0, 1, 1, 1, 0};
    const rgb8 o = apply_ops(rgb8{1, 2, 3}, load_record(none), 0, 4, 0);
    CHECK(o.r == 1 && o.g == 2 && o.b == 3);
    const rgb8 grey = hsv_to_rgb(rgb_to_hsv(rgb8{77, 77, 77}));
    CHECK(grey.r == 77 && grey.g == 77 && grey.b == 77);
    CHECK(contrast_mean(0, 1) == 0 && contrast_mean(255ull << 30, 1ull << 30) == 255 && contrast_mean(3, 2) == 2 && contrast_mean(5, 4) == 1);
    std::printf(fails ? "%d checks failed\n" : "ok\n", fails);
    return fails ? 1 : 0;
}
