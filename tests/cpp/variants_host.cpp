// variants_host.cpp -- the kernel selection (csrc/rt_variants.h) over its whole input space on the
// CPU.  Every expectation is written out here, transcribed from the code the header replaced (the
// launchers' switches, frame_build, the name table of rt_frame_kernel_name) -- none is computed by
// the header.  Exits non-zero with a message on the first mismatch.
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

enum { PATH = 0, WHITTED = 1, PACKET = 2 };
enum { PLAIN = 0, SINGLE = 1, WALKCHECK = 2 };

// MAXD by Trace depth 0..32: PATH frames and rt_trace PATH; PACKET frames (WHITTED: always 1)
static const int kPathMaxd[33] = {1, 1, 4, 4, 4, 10, 10, 10, 10, 10, 10, 32, 32, 32, 32, 32, 32,
                                  32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32};
static const int kPacketMaxd[33] = {1, 1, 10, 10, 10, 10, 10, 10, 10, 10, 10, 32, 32, 32, 32, 32, 32,
                                    32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32, 32};
static int want_maxd(int mode, uint32_t depth) {
    return mode == WHITTED ? 1 : mode == PACKET ? kPacketMaxd[depth] : kPathMaxd[depth];
}

// rt_frame_kernel_name's table as it stood: rows by mode, columns by the depth class 1 / 4 / 10 / 32
static const char *kNames[3][4] = {
    {"k_render<path,1>", "k_render<path,4>", "k_render<path,10>", "k_render<path,32>"},
    {"k_render<whitted,1>", "k_render<whitted,1>", "k_render<whitted,1>", "k_render<whitted,1>"},
    {"k_render<packet,1>", "k_render<packet,10>", "k_render<packet,10>", "k_render<packet,32>"}};
static const char *want_name(int mode, uint32_t depth) {
    return kNames[mode][depth <= 1 ? 0 : depth <= 4 ? 1 : depth <= 10 ? 2 : 3];
}

// the build, as frame_build and the head of launch_frame chose it between them
static int want_build(const FrameInputs &in) {
    const bool class1 = in.depth <= 1;
    if (in.mode != PATH || !class1) return PLAIN;
    if (in.wave_primary && in.walk_check != 0) return WALKCHECK;   // ahead of `waves == 8` in launch_frame
    if (in.frame_waves == 7) return PLAIN;
    if (in.nchunks != (in.spp > 1 ? in.spp : 1)) return PLAIN;
    if (in.overlapped && in.nunits <= 60 * in.num_cus && in.frame_waves != 8) return PLAIN;
    return SINGLE;
}

static void check_frame(const FrameInputs &in) {
    const FrameVariant v = frame_variant(in);
    const int build = v.build == FrameBuild::Plain ? PLAIN : v.build == FrameBuild::SingleSample ? SINGLE : WALKCHECK;
#define WHERE "mode %d depth %u tex %d waves %d nchunks %u spp %u nunits %u cus %u overlapped %d walk %d check %d",             \
              in.mode, in.depth, (int)in.tex, in.frame_waves, in.nchunks, in.spp, in.nunits, in.num_cus, (int)in.overlapped,    \
              in.wave_primary, in.walk_check
    CHECK(v.mode == in.mode && v.tex == in.tex, WHERE);
    CHECK(v.maxd == want_maxd(in.mode, in.depth), WHERE);
    CHECK(build == want_build(in), WHERE);
    const char *name = frame_variant_name(v);
    CHECK(name && std::strcmp(name, want_name(in.mode, in.depth)) == 0, WHERE);
    // rt_frame_kernel_name passes the class alone: the same name, whatever the build
    const FrameVariant c = kernel_class(in.mode, in.depth, in.tex);
    CHECK(c.build == FrameBuild::Plain && c.mode == v.mode && c.maxd == v.maxd && c.tex == v.tex, WHERE);
    CHECK(frame_variant_name(c) == name, WHERE);
#undef WHERE
}

int main() {
    // the classes at their boundaries, spelled out
    const struct { int mode; uint32_t depth; int maxd; } cls[] = {
        {PATH, 0, 1},    {PATH, 1, 1},    {PATH, 2, 4},     {PATH, 4, 4},     {PATH, 5, 10},   {PATH, 10, 10},
        {PATH, 11, 32},  {PATH, 32, 32},  {PACKET, 0, 1},   {PACKET, 1, 1},   {PACKET, 2, 10}, {PACKET, 4, 10},
        {PACKET, 5, 10}, {PACKET, 10, 10}, {PACKET, 11, 32}, {PACKET, 32, 32}, {WHITTED, 0, 1}, {WHITTED, 1, 1},
        {WHITTED, 2, 1}, {WHITTED, 5, 1},  {WHITTED, 11, 1}, {WHITTED, 32, 1}};
    for (const auto &c : cls) {
        CHECK(mode_maxd(c.mode, c.depth) == c.maxd, "mode %d depth %u", c.mode, c.depth);
        for (int tex = 0; tex < 2; ++tex) {
            if (c.mode == PACKET) continue;   // rt_trace: PATH and WHITTED
            const FrameVariant t = trace_variant(c.mode, c.depth, tex != 0);
            CHECK(t.build == FrameBuild::Plain && t.mode == c.mode && t.maxd == c.maxd && t.tex == (tex != 0),
                  "trace mode %d depth %u", c.mode, c.depth);
        }
    }
    const int dclass[] = {1, 1, 4, 4, 4, 10, 10, 10, 10, 10, 10, 32};
    for (uint32_t d = 0; d < 12; ++d) CHECK(depth_class(d) == dclass[d], "depth %u", d);
    CHECK(depth_class(32) == 32, "depth 32");
    // the work frame: class 1, anything else 32
    for (uint32_t d = 0; d <= 32; ++d)
        for (int tex = 0; tex < 2; ++tex) {
            const FrameVariant w = work_variant(d, tex != 0);
            CHECK(w.build == FrameBuild::Plain && w.mode == PATH && w.maxd == (d <= 1 ? 1 : 32) && w.tex == (tex != 0), "work depth %u", d);
        }
    // the primary+shadow frame kernel: PATH frames of class 1
    for (int mode = PATH; mode <= PACKET; ++mode)
        for (uint32_t d = 0; d <= 32; ++d) CHECK(primary_shadow(mode, d) == (mode == PATH && d <= 1), "mode %d depth %u", mode, d);

    // every combination of what frame_variant reads
    const int waves[] = {0, 7, 8};
    const uint32_t spps[] = {0, 1, 2, 4}, chunks[] = {1, 2, 4}, cus[] = {1, 64, 256};
    unsigned long n = 0, builds[3] = {0, 0, 0};
    for (int mode = PATH; mode <= PACKET; ++mode)
        for (uint32_t depth = 0; depth <= 32; ++depth)
            for (int tex = 0; tex < 2; ++tex)
                for (int fw : waves)
                    for (uint32_t spp : spps)
                        for (uint32_t nch : chunks)
                            for (uint32_t nc : cus) {
                                const uint32_t units[] = {0, 1, 60 * nc - 1, 60 * nc, 60 * nc + 1, 1000 * nc};
                                for (uint32_t nu : units)
                                    for (int ov = 0; ov < 2; ++ov)
                                        for (int wp = 0; wp < 2; ++wp)
                                            for (int wc = 0; wc <= 2; ++wc) {
                                                const FrameInputs in{mode, depth, tex != 0, fw, nch, spp, nu, nc, ov != 0, wp, wc};
                                                check_frame(in);
                                                ++builds[want_build(in)];
                                                ++n;
                                            }
                            }
    CHECK(builds[PLAIN] && builds[SINGLE] && builds[WALKCHECK], "a build was never expected");

    // the build rules' boundaries, one by one: a 256-CU device, spp 1 in one chunk
    const FrameInputs base{PATH, 1, false, 0, 1, 1, 60 * 256 + 1, 256, true, 0, 0};
    auto build_of = [](FrameInputs in) { return frame_variant(in).build; };
    CHECK(build_of(base) == FrameBuild::SingleSample, "overlapped, 60 * cus + 1 units");
    { FrameInputs in = base; in.nunits = 60 * 256; CHECK(build_of(in) == FrameBuild::Plain, "overlapped, 60 * cus units"); }
    { FrameInputs in = base; in.nunits = 60 * 256; in.frame_waves = 8; CHECK(build_of(in) == FrameBuild::SingleSample, "small, forced 8"); }
    { FrameInputs in = base; in.nunits = 60 * 256; in.overlapped = false; CHECK(build_of(in) == FrameBuild::SingleSample, "small, serial"); }
    { FrameInputs in = base; in.frame_waves = 7; CHECK(build_of(in) == FrameBuild::Plain, "forced 7"); }
    { FrameInputs in = base; in.spp = 2; CHECK(build_of(in) == FrameBuild::Plain, "spp 2 unsplit"); }
    { FrameInputs in = base; in.spp = 2; in.nchunks = 2; CHECK(build_of(in) == FrameBuild::SingleSample, "spp 2 in 2 chunks"); }
    { FrameInputs in = base; in.spp = 4; in.nchunks = 2; CHECK(build_of(in) == FrameBuild::Plain, "spp 4 in 2 chunks"); }
    { FrameInputs in = base; in.spp = 0; CHECK(build_of(in) == FrameBuild::SingleSample, "spp 0 counts as 1"); }
    { FrameInputs in = base; in.depth = 2; CHECK(build_of(in) == FrameBuild::Plain, "class 4"); }
    { FrameInputs in = base; in.mode = PACKET; CHECK(build_of(in) == FrameBuild::Plain, "PACKET"); }
    { FrameInputs in = base; in.mode = WHITTED; CHECK(build_of(in) == FrameBuild::Plain, "WHITTED"); }
    { FrameInputs in = base; in.wave_primary = 1; CHECK(build_of(in) == FrameBuild::SingleSample, "walk, no check"); }
    { FrameInputs in = base; in.walk_check = 1; CHECK(build_of(in) == FrameBuild::SingleSample, "check without the walk"); }
    for (int wc = 1; wc <= 2; ++wc) {
        FrameInputs in = base;
        in.wave_primary = 1;
        in.walk_check = wc;
        CHECK(build_of(in) == FrameBuild::WalkCheck, "walk check %d", wc);
        in.frame_waves = 8;
        CHECK(build_of(in) == FrameBuild::WalkCheck, "walk check %d wins over waves 8", wc);
        in.frame_waves = 7;
        CHECK(build_of(in) == FrameBuild::WalkCheck, "walk check %d with waves 7", wc);
        in.depth = 2;
        CHECK(build_of(in) == FrameBuild::Plain, "walk check %d, class 4", wc);
    }
    // a variant no build exists for has no name
    CHECK(frame_variant_name(FrameVariant{FrameBuild::Plain, PACKET, 4, false}) == nullptr, "<packet,4>");
    CHECK(frame_variant_name(FrameVariant{FrameBuild::Plain, WHITTED, 32, false}) == nullptr, "<whitted,32>");
    std::printf("variants_host ok: %lu frame inputs (%lu plain, %lu single-sample, %lu walk-check)\n", n, builds[PLAIN],
                builds[SINGLE], builds[WALKCHECK]);
    return 0;
}
