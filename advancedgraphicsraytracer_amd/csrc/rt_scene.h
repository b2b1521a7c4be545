// rt_scene.h -- struct rt_scene, and what the two files that share it need of each other:
// rt_device.hip (scene creation and destruction, the ray calls, renderers and frames) and
// rt_scene_edit.hip (every entry point that changes a live scene).  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_internal.h"
#include "rt_refit.h"

struct rt_scene {
    int device = 0;
    rt::SceneView view{};
    rt::Bvh bvh;
    uint32_t num_prims = 0;
    uint32_t num_materials = 0; // what an inserted triangle's material index is checked against
    uint32_t stack_depth = 0;   // LDS stack entries per lane
    int frame_waves = 0;        // primary+shadow frame kernel build (frame_variant): 0 = chosen, 7 = the
                                // plain build, 8 = the single-sample one wherever it applies (RT_FRAME_WAVES)
    uint32_t num_cus = 256;     // CUs of the device (resident grids, frames-in-flight rules)
    bool has_cubes = false;     // cube acceptance depends on the visiting order: no wave walk
    bool quads = false;         // two-level node records built (RT_PT_QUADS=1, build_quads)
    bool quad_lanes = false;    // ... and the lane kernel walks them
    void *d_quads = nullptr;
    bool walk_fits = true;      // the lane stacks + the wave walk's word stack fit one launch's LDS (kLdsLaunchMax)
    bool nested = true;         // every child box lies inside its parent's (as floats): the wave walk's
                                // exactness needs it (the builders' trees always; a caller's prebuilt one
                                // is checked at rt_scene_create)
    int walk = RT_WALK_LANE;    // camera-ray walk of the global-node primary+shadow kernel
    bool ext = false;           // needs the kext kernels (cubes, quads, textures, non-Light light)
    bool ext_fixed = false;     // ... for reasons no edit of the primitives changes (family_fixed): kept for
                                // the commit of rt_scene_splice_prims, which takes ext anew by creation's rule
    bool pt_lanes = true;           // levels >= 1 run the lane state machine (RT_PT_LANES=0: k_pt_level)
    bool pt_dynamic = true;         // wavefront levels >= 1 fetch chunks dynamically (RT_PT_DYNAMIC=0: static)
    bool pt_wavefront = true;   // depth >= 2 path tracing: wavefront (k_pt_level) vs one kernel (k_render)
    uint32_t pt_drain_level = 64;   // bounce level from which the wavefront always drains (64 = never forced)
    double pt_drain_rounds = 0.25;  // ... and it drains any level holding <= this many rounds of resident lanes
    // small batches (<= pt_small_rounds rounds of resident lanes, e.g. a 1/8 shard's): always drain
    // from level pt_drain_small (0 = off).  Config 5's 1/8 shard (4.1 M paths per batch, ~10 rounds):
    // 1.126 / 1.129 -> 1.055 / 1.059 ms forced from level 4 (1.095 / 1.068 from 3); whole frames
    // (33 M paths, ~84 rounds) lose with it (CFG5-sub 6.70 -> 6.85 ms), so they keep the threshold
    // alone (profiles/r05/c5drain)
    uint32_t pt_drain_small = 4;
    double pt_small_rounds = 16.0;
    // ... and drains any of its levels holding <= this many rounds (the whole frames' 0.25 above):
    // the 1/8 shard 1.084 / 1.077 -> 1.054 / 1.065 ms mean of three interleaved runs (0.0625: 1.058;
    // 0.5: 1.092; profiles/r05/c5drain/c5knobs*.jsonl)
    double pt_small_drain_rounds = 0.125;
    bool tile_order = true;         // measured-cost (longest first) tile order (RT_TILE_ORDER=0: off)
    uint32_t split_units = 40000;   // sample split below this many tiles (1080p = 32,400 tiles)
    bool xcd_order = false;         // measured order grouped by XCD: blocks b, b + 8, ... (one XCD) render
                                    // one compact screen region of 1/8 of the frame's cost (L2 locality)
    uint32_t split_parts = 2;       // ... each as this many waves of 64 / parts lanes (RT_SPLIT_PARTS: 2, 4, 8)
    int32_t heavy_split = -1;       // primary+shadow frames: the costliest tiles run as two half-tile
                                    // waves (RT_SPLIT_HEAVY = count; -1: ntiles / 32)
    uint64_t pt_mem_bytes = 12288ull << 20;   // path-state budget per slot (two when pipelined): 12 GB
                                              // of the 288 GB HBM holds all 16 spp of a 1080p depth-10 frame
    bool pt_pipeline = true;        // sample batches alternate path-state slots and streams
    uint32_t pt_slots = 0;          // path-state slots / streams of pipelined frames (RT_PT_SLOTS, 2-8;
                                    // 0 = 8 for batches of <= 8.4 M paths, else 4)
                                    // (RT_PT_PIPELINE=0: one slot, the caller's stream)
    uint32_t ps_buffers = 0;        // per-sample result buffers of overlapped frames (RT_PS_BUFFERS,
                                    // 2-7; 0 = frames in flight + 1)
    int32_t ps_pipeline = -1;       // primary+shadow frames overlap: -1 timed per renderer (auto),
                                    // 0 never, 1 always (RT_PS_PIPELINE)
    uint32_t ps_depth = 2;          // frames in flight when forced (RT_PS_DEPTH, 2-8)
    float tune_delay_ms = 100.0f;   // GPU time a parameter set runs before its timed choices start
                                    // (RT_TUNE_DELAY_MS): the clocks ramp over ~0.1 s, and choices
                                    // timed on the first frames at low clocks came out wrong
    void *d_nodes = nullptr, *d_prims = nullptr, *d_shade = nullptr, *d_mats = nullptr, *d_sky = nullptr;
    void *d_xprims = nullptr, *d_tex = nullptr;
    void *d_scratch = nullptr;  // staging for the host-pointer batched calls
    void *d_cost = nullptr;     // rt_scene_bvh_cost's partial sums (rt_cost.hip), allocated by its first call
    size_t scratch_bytes = 0;
    hipStream_t stream = nullptr;
    rt::RefitState refit;          // in-place updates (rt_refit.h)
};

namespace rt {

// A stream that is about to read the scene waits for its stream-ordered updates: the
// scene's one event, and only while an async update is pending -- otherwise one branch.
inline int after_updates(const rt_scene *s, hipStream_t st) {
    if (!s->refit.async.issued) return RT_OK;
    HIP_TRY(hipStreamWaitEvent(st, s->refit.async.done, 0));
    return RT_OK;
}

// rt_device.hip: every scene field that follows from the tree, for a created scene and a rebuilt one
void scene_tree_fields(rt_scene *s, uint32_t root_word, bool nested, bool bounds_finite);
// rt_scene_edit.hip: what rt_scene_update_sync does, and every blocking scene entry point first
int fold_updates(rt_scene *s);

}  // namespace rt
