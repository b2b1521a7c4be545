// gbuffer_variants_host.cpp -- the G-buffer family's selection (csrc/rt_variants.h: gbuffer_variant, its
// kernel names, gbuffer_wave_walk) over its whole input space on the CPU.  Every expectation is written
// out here from the rule as rt_amd.h states it -- none is computed by the header.  Exits non-zero with a
// message on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "rt_variants.h"

using namespace rt;

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("%s:%d: %s: ", __FILE__, __LINE__, #cond);  \
            std::printf(__VA_ARGS__);                               \
            std::printf("\n");                                      \
            std::exit(1);                                           \
        }                                                           \
    } while (0)

enum { LANE = 0, WAVE = 1, AUTO = 2 };

int main() {
    // the build: (list or rectangle) x (sky), four kernels with four names
    static const char *kNames[2][2] = {{"k_gbuffer<const>", "k_gbuffer<tex>"}, {"k_gbuffer_pixels<const>", "k_gbuffer_pixels<tex>"}};
    for (int pixels = 0; pixels < 2; ++pixels)
        for (int tex = 0; tex < 2; ++tex) {
            const GBufferVariant v = gbuffer_variant(pixels != 0, tex != 0);
            CHECK(v.pixels == (pixels != 0) && v.tex == (tex != 0), "pixels %d tex %d", pixels, tex);
            CHECK(std::strcmp(gbuffer_variant_name(v), kNames[pixels][tex]) == 0, "pixels %d tex %d", pixels, tex);
        }
    const GBufferVariant def{};
    CHECK(!def.pixels && !def.tex, "the default variant is the rectangle kernel with the constant sky");

    // the camera walk: every combination of what the rule reads
    unsigned long n = 0, wave = 0;
    for (int pixels = 0; pixels < 2; ++pixels)
        for (int walk = LANE; walk <= AUTO; ++walk)
            for (int settled = -1; settled <= 1; ++settled)
                for (int ext = 0; ext < 2; ++ext)
                    for (int cubes = 0; cubes < 2; ++cubes)
                        for (int nested = 0; nested < 2; ++nested)
                            for (int fits = 0; fits < 2; ++fits) {
                                // the wave walk: a rectangle of a core-build scene that admits the walk, where
                                // the scene forces it or the renderer's frames have settled on it
                                bool want = false;
                                if (!pixels && !ext && !cubes && nested && fits) {
                                    if (walk == WAVE) want = true;
                                    if (walk == AUTO && settled == 1) want = true;
                                }
                                const bool got = gbuffer_wave_walk({pixels != 0, walk, settled, ext != 0, cubes != 0, nested != 0, fits != 0});
                                CHECK(got == want, "pixels %d walk %d settled %d ext %d cubes %d nested %d fits %d", pixels, walk,
                                      settled, ext, cubes, nested, fits);
                                wave += want;
                                ++n;
                            }
    CHECK(n == 2 * 3 * 3 * 16 && wave == 3 + 1, "%lu inputs, %lu wave", n, wave);
    // the rule's edges, one by one
    const GBufferWalkInputs base{false, AUTO, 1, false, false, true, true};
    CHECK(gbuffer_wave_walk(base), "AUTO settled on the wave walk");
    { GBufferWalkInputs in = base; in.settled = -1; CHECK(!gbuffer_wave_walk(in), "AUTO, nothing settled: the lane walk"); }
    { GBufferWalkInputs in = base; in.settled = 0; CHECK(!gbuffer_wave_walk(in), "AUTO settled on the lane walk"); }
    { GBufferWalkInputs in = base; in.walk = LANE; CHECK(!gbuffer_wave_walk(in), "LANE whatever was settled"); }
    { GBufferWalkInputs in = base; in.walk = WAVE; in.settled = -1; CHECK(gbuffer_wave_walk(in), "WAVE needs nothing settled"); }
    { GBufferWalkInputs in = base; in.pixels = true; CHECK(!gbuffer_wave_walk(in), "a pixel list always takes the lane walk"); }
    { GBufferWalkInputs in = base; in.walk = WAVE; in.pixels = true; CHECK(!gbuffer_wave_walk(in), "... under WAVE too"); }
    { GBufferWalkInputs in = base; in.ext = true; CHECK(!gbuffer_wave_walk(in), "the extension build has the lane walk only"); }
    { GBufferWalkInputs in = base; in.has_cubes = true; CHECK(!gbuffer_wave_walk(in), "cubes"); }
    { GBufferWalkInputs in = base; in.nested = false; CHECK(!gbuffer_wave_walk(in), "a tree that is not nested"); }
    { GBufferWalkInputs in = base; in.walk_fits = false; CHECK(!gbuffer_wave_walk(in), "no room for the walk's words"); }
    std::printf("gbuffer_variants_host ok: 4 builds, %lu walk inputs (%lu take the wave walk)\n", n, wave);
    return 0;
}
