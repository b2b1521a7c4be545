// rt_variants.h -- which compiled build of a kernel a call runs: the whole selection, as pure
// functions of plain values (host-only: no HIP header, no environment; tests/cpp/variants_host.cpp
// walks its input space).  rt_device.hip computes a variant, the kernel builds (rt_kernels.inc)
// map it to a kernel in one table per family, rt_frame_kernel_name names it.
#pragma once
#include <algorithm>
#include <cstdint>

#include "../../include/rt_amd.h"

namespace rt {

// the compiled MAXD class a Trace depth runs in
constexpr int depth_class(uint32_t depth) { return depth <= 1 ? 1 : depth <= 4 ? 4 : depth <= 10 ? 10 : 32; }

// the MAXD of a mode's frame and rt_trace builds: WHITTED has one (its depth is a run-time bound,
// kWHITTED_MAX), PACKET none of class 4 (depths 2-4 run in <packet,10>)
constexpr int mode_maxd(int mode, uint32_t depth) {
    const int c = depth_class(depth);
    return mode == RT_MODE_WHITTED ? 1 : mode == RT_MODE_PACKET && c == 4 ? 10 : c;
}

// the primary+shadow frame kernel: the one frame kernel with more than the plain build
constexpr bool primary_shadow(int mode, uint32_t depth) { return mode == RT_MODE_PATH && depth_class(depth) == 1; }

enum class FrameBuild : int {
    Plain,          // k_render (the primary+shadow frame: 71 VGPRs, 7 waves/SIMD)
    SingleSample,   // k_render_w8: render_tile ONE -- no sample loop, 51 VGPRs, 8 waves/SIMD where the LDS stacks allow
    WalkCheck       // k_render_walkcheck: the camera walk's counters / re-trace compiled in
};

// One build of a kernel family: integrator mode (RT_MODE_*), compiled MAXD, textured sky; for the
// frame kernel also the build (rt_trace and the work frame have the plain one only).
struct FrameVariant {
    FrameBuild build = FrameBuild::Plain;
    int mode = RT_MODE_PATH;
    int maxd = 1;
    bool tex = false;   // non-constant sky texture
};

// The class of a frame or an rt_trace call -- mode, MAXD, sky -- in the plain build: all that a
// kernel's name, rt_trace's kernel and every frame kernel but the primary+shadow one depend on.
constexpr FrameVariant kernel_class(int mode, uint32_t depth, bool tex) {
    return FrameVariant{FrameBuild::Plain, mode, mode_maxd(mode, depth), tex};
}

// what the frame kernel's selection reads
struct FrameInputs {
    int mode;                 // RT_MODE_PATH / _WHITTED / _PACKET
    uint32_t depth;           // Trace depth, at most 32
    bool tex;
    int frame_waves;          // the scene's knob: 0 = chosen here, 7 = the plain build, 8 = the single-sample one
    uint32_t nchunks, spp;    // FrameArgs: sample chunks per tile, samples per pixel
    uint32_t nunits, num_cus; // FrameArgs: work units of the launch; the device's compute units
    bool overlapped;          // the frame runs beside others (frames in flight)
    int wave_primary;         // SceneView: camera rays take the wave walk
    int walk_check;           // SceneView: RT_WALK_CHECK_*
};

// The frame kernel's build.  Frames of one sample per work unit (spp 1, or a sample split into
// single-sample chunks) run the single-sample build, others the plain one; a walk check wins over
// both (only its build holds the checks).
constexpr FrameVariant frame_variant(const FrameInputs &in) {
    FrameVariant v = kernel_class(in.mode, in.depth, in.tex);
    if (!primary_shadow(in.mode, in.depth)) return v;
    if (in.wave_primary && in.walk_check != RT_WALK_CHECK_OFF) {
        v.build = FrameBuild::WalkCheck;
        return v;
    }
    if (in.frame_waves == 7) return v;
    if (in.nchunks != std::max(1u, in.spp)) return v;   // the single-sample build: one sample per unit
    // small overlapped frames (<= 3 rounds of resident waves: TEAPOT-F 720p with 4 in flight
    // 0.059 -> 0.062 ms) keep the plain build; everywhere else the single-sample build won or
    // tied (TEAPOT-F 1080p serial 0.1025 -> 0.096, 2 in flight 0.108 -> 0.099; mig29 x16 1080p 4 in
    // flight 0.223 -> 0.215, serial 0.466 -> 0.471; profiles/r04/frame_build/one_*.log)
    if (in.overlapped && in.nunits <= 3u * 4u * 5u * in.num_cus && in.frame_waves != 8) return v;
    v.build = FrameBuild::SingleSample;
    return v;
}

// rt_trace (RT_MODE_PATH / _WHITTED): the frame kernels' classes, the plain build
constexpr FrameVariant trace_variant(int mode, uint32_t depth, bool tex) { return kernel_class(mode, depth, tex); }

// the dry-run work frame (k_render_work, RT_MODE_PATH): class 1, or 32 for every deeper Trace
constexpr FrameVariant work_variant(uint32_t depth, bool tex) {
    return FrameVariant{FrameBuild::Plain, RT_MODE_PATH, depth_class(depth) == 1 ? 1 : 32, tex};
}

// The first-hit G-buffer family (rt_render_gbuffer / rt_gbuffer_pixels): k_gbuffer, one wave per 8x8 tile
// of the frame's own tile grid, or k_gbuffer_pixels, one lane per listed pixel; each with the constant
// or the textured sky.  A query: no mode, no MAXD, no frame build.
struct GBufferVariant {
    bool pixels = false;   // k_gbuffer_pixels (a pixel list) instead of k_gbuffer (a rectangle of tiles)
    bool tex = false;      // non-constant sky texture
};
constexpr GBufferVariant gbuffer_variant(bool pixels, bool tex) { return GBufferVariant{pixels, tex}; }
constexpr const char *gbuffer_variant_name(const GBufferVariant &v) {
    return v.pixels ? (v.tex ? "k_gbuffer_pixels<tex>" : "k_gbuffer_pixels<const>") : (v.tex ? "k_gbuffer<tex>" : "k_gbuffer<const>");
}

// what the G-buffer's camera walk reads
struct GBufferWalkInputs {
    bool pixels;      // the list form: its lanes are not a tile
    int walk;         // the scene's policy, RT_WALK_*
    int settled;      // the renderer's timed choice for its primary+shadow frames: 1 wave, 0 lane, -1 none yet
    bool ext;         // the scene runs the extension build (its frames never take the wave walk)
    bool has_cubes, nested, walk_fits;   // the scene's conditions of the wave walk (rt_scene_set_camera_walk)
};
// Camera rays of a G-buffer take the wave walk exactly where a primary+shadow frame of the same
// renderer would right now: the scene forces it, or RT_WALK_AUTO has settled on it.  Nothing settled:
// the lane walk -- a query starts and advances no timed choice.
constexpr bool gbuffer_wave_walk(const GBufferWalkInputs &in) {
    if (in.pixels || in.ext || in.has_cubes || !in.nested || !in.walk_fits) return false;
    return in.walk == RT_WALK_WAVE || (in.walk == RT_WALK_AUTO && in.settled > 0);
}

// The public name of a frame variant's kernel (rt_frame_kernel_name; rocprofv3's, abbreviated);
// nullptr: no such build.  It reads the class alone: the single-sample and walk-check builds of
// <path,1> answer k_render<path,1> too -- they are builds of that kernel (same frames, same roofline
// line), and callers compare the name across knobs that switch between them -- so
// rt_frame_kernel_name, which knows no frame's units, passes kernel_class(), the value frame_variant
// starts from.  (k_pt_level and k_render_heat are decided ahead of the variant, there as in
// launch_render.)
constexpr const char *frame_variant_name(const FrameVariant &v) {
    switch (v.mode * 64 + v.maxd) {
    case RT_MODE_PATH * 64 + 1: return "k_render<path,1>";
    case RT_MODE_PATH * 64 + 4: return "k_render<path,4>";
    case RT_MODE_PATH * 64 + 10: return "k_render<path,10>";
    case RT_MODE_PATH * 64 + 32: return "k_render<path,32>";
    case RT_MODE_WHITTED * 64 + 1: return "k_render<whitted,1>";
    case RT_MODE_PACKET * 64 + 1: return "k_render<packet,1>";
    case RT_MODE_PACKET * 64 + 10: return "k_render<packet,10>";
    case RT_MODE_PACKET * 64 + 32: return "k_render<packet,32>";
    }
    return nullptr;
}

}  // namespace rt
