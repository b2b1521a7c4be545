// rt_device.hip -- the device half of the C-ABI: scene upload, renderer state, launches (the entry points
// that change a live scene are rt_scene_edit.hip; struct rt_scene is rt_scene.h).
// The kernels live in rt_kernels.inc (built twice: rt_kern_core.hip / rt_kern_ext.hip).
//
// Hot path: Renderer::Tick -> Camera::GetPrimaryRay -> Renderer::Trace
// -> Scene::IntersectBVH / IsOccluded -> Primitive::Intersect / Hit, plus
// NextEventDirectIllumination, the Diffuse / Mirror / Dielectric / Checkerboard / Light
// materials, the sky lookup, the running-average accumulator and the RGB8 pack -- all in
// ONE kernel launch per frame (k_render).  Launch shape: 256-thread workgroups of four
// wave64s, one wave per 8x8 screen tile (the reference's PACKET_SIZE 64 / SQRT_PACKET_SIZE 8,
// Ray.h:3-5), one lane per pixel.  No MFMA: this is branchy scalar fp32.
//
// Device scene layout in HBM (packed by pack_scene, rt_scene_pack.cpp, with the encoders of
// rt_records.h; uploaded once by rt_scene_create):
//   nodes  : the reference's 32-byte BVHNode array (root 0, node 1 unused, sibling pairs
//            64-byte aligned) with (leftFirst, count) replaced by one packed word
//            (leftFirst << 8 | count) so a 64-byte sibling-pair load carries everything
//            the traversal needs;
//   prims  : leaf order (primitiveIndices applied), 48 B per slot: triangle A, B-A, C-A
//            (host-computed, bit-identical to the reference's per-test subtraction) and
//            the original primitive id -- no index indirection in the leaf loop;
//   shade  : per primitive id, 32 B: geometric normal (triangles, host-computed with the
//            reference's normalize(cross(..))), sphere centre / 1/r, material id;
//   per-lane traversal stack: LDS, [depth][256 lanes] u32, conflict-free.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rt_cost.h"
#include "rt_dev_types.h"
#include "rt_internal.h"
#include "rt_records.h"
#include "rt_refit.h"
#include "rt_scene.h"
#include "rt_sched.h"
#include "rt_tune.h"

// ====================================================================== host side
using namespace rt;

// renderer streams: up to 8 -- frames in flight of overlapped primary+shadow frames (timed
// choice among 2 / 4 / 6, forced up to 8) and the path-state slots of pipelined path-traced
// frames (8 for small batches when the process has >= 8 hardware queues, else 4).  With the
// caller's stream and a communicator's a process may then drive 10 streams; HIP maps them onto
// GPU_MAX_HW_QUEUES hardware queues (default 4, bench.py sets 8 for the workloads that overlap).
constexpr int kPsMaxDepth = 8;   // renderer streams (frames in flight when forced: RT_PS_DEPTH)
constexpr int kPtMaxSlots = 8;    // path-state slots of pipelined path-traced frames (RT_PT_SLOTS; <= kPsMaxDepth streams)
// the process's hardware queues per device as HIP will use them (GPU_MAX_HW_QUEUES, default 4)
inline int hw_queues() {
    const char *e = std::getenv("GPU_MAX_HW_QUEUES");
    const int v = e ? std::atoi(e) : 0;
    return v > 0 ? v : 4;
}

// A ring of N frame-level result buffers ([sample][pixel] radiance), frame n in buffer n % (the
// count in use): each with the event of the finishing pass that last read it, which the next frame
// to write the buffer waits for, and whether that event was recorded since the buffer was made.
// With as many buffers as frames in flight, frame n + 2's kernels waited for frame n's finishing
// pass, which itself follows frame n + 1's kernels on the caller's stream; one buffer more lets a
// frame start behind the finish of the frame `count` back.
template <int N>
struct ResultRing {
    DevBuf buf[N];
    hipEvent_t fin[N] = {};
    bool fin_set[N] = {};

    int event(int b) {   // fin[b], created as first needed
        if (!fin[b]) HIP_TRY(hipEventCreateWithFlags(&fin[b], hipEventDisableTiming | hipEventReleaseToDevice));
        return RT_OK;
    }
    // buffer b grown to `bytes`, after every pending use of the old one
    int ensure(int b, size_t bytes) {
        if (bytes <= buf[b].bytes) return RT_OK;
        fin_set[b] = false;
        return buf[b].grow(bytes, Wait::kDevice);
    }
    // buffers k .. N-1 freed (the caller knows that nothing uses them)
    int drop_from(int k) {
        for (int b = k; b < N; ++b) {
            if (int rc = buf[b].release(); rc != RT_OK) return rc;
            fin_set[b] = false;
        }
        return RT_OK;
    }
    float4 *at(int b) const { return buf[b].template as<float4>(); }
};

struct rt_renderer {
    rt_scene *scene = nullptr;
    int device = 0;             // the scene's device, for rt_renderer_destroy: a caller (Python's
                                // garbage collector) may have destroyed the scene first
    uint32_t W = 0, H = 0;
    float4 *d_acc = nullptr;
    unsigned long long *d_counters = nullptr;
    uint32_t *d_rgb = nullptr;   // staging frame for rt_render_frame_host
    uint64_t primary = 0, frames = 0;
    hipStream_t stream = nullptr;
    // measured-cost tile order (tile_order_step): per-tile cycles of one frame (two cost
    // maps while the camera walk is being timed), longest tile first afterwards
    DevBuf d_order, d_cost;
    std::vector<uint32_t> host_cost;   // the cost map the active order was sorted from (local tiles)
    bool tail_bound = false;    // that map's costliest tile outlasts 2 x the frame's mean time per
                                // resident wave slot: frames in flight beyond 2 become candidates
    uint32_t order_n = 0;
    uint64_t order_key = 0;
    int order_state = 0;        // 0 idle, 1 costs recorded, 2 order active, 3 costs held without an
                                // order (path-traced frames)
    uint32_t order_split = 0;   // leading tiles of the split order that run as order_parts units each
    uint32_t order_parts = 2;
    // The timed choices (rt_tune.h) -- camera walk lane / wave, plain / split order, frames in flight --
    // each with its schedule, the events around its groups, the group times and what they decided
    TimedGroups walk_tg, split_tg, ps_tg;
    hipEvent_t tune_ev[4][16] = {};   // [kWalk / kSplit / kOverlap][2g, 2g + 1 around group g], [kGate][start, probe]
    float walk_ms[4] = {}, split_ms[4] = {}, ps_ms[8] = {};
    int wave = -1;                  // the wave walk measured faster: 1 / 0, -1 not decided yet
    bool use_split = false;         // the split order measured faster
    int ps_use = -1;                // frames in flight (0 = serial), -1 not decided yet
    uint64_t walk_key = 0;          // the parameter set whose frames the walk timing runs on
    hipEvent_t stall_ev = nullptr;  // after the previous frame while a timed group runs (kTuneRestarts)
    bool stall_armed = false;
    int walk_check = RT_WALK_CHECK_OFF;     // rt_renderer_set_walk_check
    // wavefront path tracer (PathArgs): two path-state slots (state, records, queues), grown on
    // demand, each owned by one of the renderer's two path streams.  Sample batches alternate
    // between them, so one batch's (or the next frame's) level 0 fills the CUs that the other
    // batch's thinning bounce levels leave idle.  The per-sample radiance goes to a frame-level
    // buffer (two, by frame parity); one finishing pass per frame on the caller's stream sums
    // it in sample order after every batch's levels (accumulator, RGB8).  d_pt[0] / the
    // caller's stream alone when pipelining is off or the results do not fit.
    DevBuf d_pt[kPtMaxSlots];
    // [sample][pixel] radiance of a frame, frame n in buffer n % (slots + 1): frame n + slots + 1's
    // batches wait for frame n's finishing pass only (see launch_pt_frame)
    ResultRing<kPtMaxSlots + 1> pt_res;
    float4 *d_sum = nullptr;        // the running sample sum across batches (serial path)
    // renderer streams: the path tracer's two path streams are 0 and 1; overlapped primary+
    // shadow frames use the first `depth` of them (frames in flight)
    hipStream_t pt_stream[kPsMaxDepth] = {};
    int nstreams = 0;               // pt_stream[0 .. nstreams) created (ensure_pipe_streams)

    hipEvent_t pt_lv[kPsMaxDepth] = {};   // a renderer stream's work of this frame is done
    int pt_slot = 0, pt_parity = 0;
    uint32_t pt_nslots = 0;         // slots in use, decided for path state of up to pt_need bytes
    size_t pt_need = 0;
    bool pt_serial_last = false;    // the last path-traced frame ran the serial path
    // overlapped primary+shadow frames (overlap_step): with RT_PS_PIPELINE auto, groups of
    // eligible frames back to back at each candidate depth are timed on the caller's stream
    // (ps_tg); the next frame keeps the fastest mode for the parameter set, and the result
    // buffers it does not use are freed
    uint64_t ps_last = 0;           // r->frames at the last timing frame (any other frame restarts)
    uint32_t ps_prev = 0;           // frames in flight of the previous eligible frame (0 serial)
    hipEvent_t ps_join = nullptr;   // caller's stream -> overlap stream, on a switch to overlapped
    hipEvent_t cost_ev = nullptr;   // path-traced frames: the cost map was cleared (caller's stream)
    // the overlapped frames' per-sample results, frame n in buffer n % buffers (kernel on
    // renderer stream n % depth): frame n + buffers waits for the finishing pass of frame n only,
    // so a kernel never waits for the finish of a frame still running beside it
    ResultRing<kPsMaxDepth + 1> ps_res;
    uint32_t ps_count = 0;
    // tuning gate: the timed choices (camera walk, split order, frames in flight) of a parameter
    // set start once its frames have run tune_delay_ms of GPU time -- an event at its first frame
    // and a probe every 8 frames, read without blocking
    uint64_t gate_key = 0;
    int gate_state = 0;             // 0 start, 1 running, 2 probe recorded, 3 open
    uint32_t gate_frames = 0;
    // per-sample values of sample-split frames (FrameArgs::samples)
    DevBuf d_samples;
    // explicit tile deal of rt_render_shard_tiles (FrameArgs::tile_map): local -> global tile,
    // uploaded when it changes; and rank 0's per-global-tile (shard << 24 | local) for assembly
    std::vector<uint32_t> map_host;
    // the tiles whose running averages the accumulator holds: those of the last frame (a frame
    // accumulates exactly its own tiles).  0 none yet, 1 every tile, 2 the interleaved shard
    // held_shard of held_nshards, 3 the explicit list held_list (renderer_held_tiles)
    int held_kind = 0;
    uint32_t held_shard = 0, held_nshards = 1;
    std::vector<uint32_t> held_list;
    uint64_t map_gen = 0, held_gen = 0;   // set_tile_map's changes; the one held_list was copied at
    DevBuf d_work;                  // dry-run work frame: per local tile (work_frame)
    DevBuf d_map;
    uint64_t map_hash = 0;
    DevBuf d_where;
    uint64_t where_hash = 0;
    TileGrid grid() const { return tile_grid(W, H); }
};

// every growable buffer the renderer owns (the accumulator, the counters, d_rgb and d_sum are
// allocated once, at their one size): rt_renderer_destroy frees them, rt_renderer_device_bytes sums them
template <class R, class Fn>
void each_buffer(R &r, Fn f) {
    for (auto &b : r.d_pt) f(b);
    for (auto &b : r.pt_res.buf) f(b);
    for (auto &b : r.ps_res.buf) f(b);
    for (auto *b : {&r.d_samples, &r.d_order, &r.d_cost, &r.d_map, &r.d_work, &r.d_where}) f(*b);
}

namespace {

enum { kWalk, kSplit, kOverlap, kGate };   // rt_renderer::tune_ev rows

void free_scene(rt_scene *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    (void)hipDeviceSynchronize();
    void *ptrs[] = {s->d_nodes, s->d_prims, s->d_shade, s->d_mats, s->d_sky, s->d_xprims, s->d_tex, s->d_scratch, s->d_quads, s->d_cost};
    for (void *p : ptrs)
        if (p) (void)hipFree(p);
    free_refit(s->refit);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

int ensure_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0)
        return fail(RT_ERR_NO_DEVICE, "no HIP device visible: the MI355X path has no CPU fallback");
    if (device < 0 || device >= count) return fail(RT_ERR_INVALID, "device index out of range");
    HIP_TRY(hipSetDevice(device));
    return RT_OK;
}

// RT_PT_QUADS=1: the lane kernel walks two-level node records (build_quads).  Exact (the GPU suite
// passes with it on; test_wavefront_equals_one_kernel_path_tracer runs it), but measured slower,
// so off by default (tools/ab.py serial frames, profiles/r05/quadab): CFG3-sub 2.133 -> 2.385 ms,
// CFG5-sub 8.49 -> 9.41, TEAPOT-F depth 10 1.150 -> 1.253, mig29 x16 spp 4 depth 4 3.78 -> 4.40 --
// a record step costs four slab tests, two box unions and a 128-B load for every lane of the
// wave whichever branch (leaf, odd half, record) each lane is in, and the lanes' chains shrink less
// than the step grows.
#ifndef RT_PT_QUADS_DEFAULT
#define RT_PT_QUADS_DEFAULT 0
#endif
// the environment's part of pack_scene's options
int pack_options_from_env(PackOptions &o) {
    // RT_BVH (plain / sbvh) picks the tree only where the caller left the default
    if (const char *e = std::getenv("RT_BVH")) {
        if (std::strcmp(e, "sbvh") != 0 && std::strcmp(e, "plain") != 0)
            return fail(RT_ERR_INVALID, std::string("RT_BVH must be 'plain' or 'sbvh', not '") + e + "'");
        o.bvh_kind = std::strcmp(e, "sbvh") == 0 ? RT_BVH_SBVH : RT_BVH_PLAIN;
    }
    // the wave walk's cull margin: RT_WALK_MARGIN = its base-2 exponent
    if (const char *e = std::getenv("RT_WALK_MARGIN")) o.walk_margin = std::ldexp(1.0f, std::max(-40, std::min(-1, std::atoi(e))));
    // a sliver's sine limit 2^RT_WALK_STICKY (>= 0: no triangle is one); RT_WALK_STICKY_SPHERES=0: A/B only
    if (const char *e = std::getenv("RT_WALK_STICKY")) o.sliver_lim = std::atoi(e) >= 0 ? 0.0 : std::ldexp(1.0, std::atoi(e));
    if (const char *e = std::getenv("RT_WALK_STICKY_SPHERES")) o.sticky_spheres = std::atoi(e) != 0;
    o.quads = RT_PT_QUADS_DEFAULT != 0;
    if (const char *e = std::getenv("RT_PT_QUADS")) o.quads = std::atoi(e) != 0;
    return RT_OK;
}

}  // namespace

// Every scene field that follows from the tree, set here for a created scene and for a rebuilt one
// (s->bvh's nodes_used, depth and max_leaf and the device node / slot arrays are already the tree's).
// The camera-walk policy is not the tree's: creation derives it afterwards (scene_knobs_from_env), a
// rebuild keeps it unless the new tree no longer admits the wave walk.
void rt::scene_tree_fields(rt_scene *s, uint32_t root_word, bool nested, bool bounds_finite) {
    s->stack_depth = pick_stack(s->bvh.depth);
    s->walk_fits = stack_admits_walk(s->stack_depth);
    s->nested = nested;
    SceneView &v = s->view;
    v.nodes = (const float4 *)s->d_nodes;
    v.prims = (const float4 *)s->d_prims;
    v.root_word = root_word;
    v.stack_entries = s->stack_depth;
    v.bounds_finite = bounds_finite ? 1 : 0;
    // XCD-grouped tile order for scenes whose nodes + primitive slots exceed one XCD's 4 MB L2:
    // mig29 x16 (11.6 MB) 0.449 -> 0.406 ms; a cache-resident TEAPOT-F loses with it (4K
    // 0.377 -> 0.441 ms, 720p neutral) -- profiles/r02/ab_xcd_*.json.  RT_XCD_ORDER=0/1 forces it.
    s->xcd_order = (size_t)s->bvh.nodes_used * 32u + (size_t)s->num_prims * 48u > (4u << 20);
    if (const char *e = std::getenv("RT_XCD_ORDER")) s->xcd_order = std::atoi(e) != 0;
    if (s->walk != RT_WALK_LANE && !(s->nested && s->walk_fits)) s->walk = RT_WALK_LANE;
}

namespace {

// the scene's launch policy: defaults from the tree, overridden by the environment (A/B runs)
void scene_knobs_from_env(rt_scene *s) {
    // Primary+shadow frames read the nodes from global memory (L1/L2-resident, 256-thread
    // workgroups).  The LDS-node kernels of rounds 1-3 (48-B pairs + u16 stacks in two 512-thread
    // workgroups per CU, or 64-B pairs in one 1024-thread group) lost by 12 % once the ray
    // counters were spread over slots (TEAPOT-F 0.169 vs 0.192 ms, profiles/r01/ab_kernel_choice_*;
    // LDS occupancy caps them at 4 waves/SIMD) and were removed in round 4.
    // RT_PT_WAVEFRONT=0 selects the one-kernel path tracer (k_render<path, MAXD>) for A/B runs
    if (const char *e = std::getenv("RT_PT_WAVEFRONT")) s->pt_wavefront = std::atoi(e) != 0;
    if (const char *e = std::getenv("RT_PT_DYNAMIC")) s->pt_dynamic = std::atoi(e) != 0;
    if (const char *e = std::getenv("RT_PT_LANES")) s->pt_lanes = std::atoi(e) != 0;
    // RT_PT_DRAIN_LEVEL / RT_PT_MEM_MB: wavefront drain level and path-state budget (A/B runs)
    if (const char *e = std::getenv("RT_PT_DRAIN_LEVEL")) s->pt_drain_level = (uint32_t)std::max(1, std::atoi(e));
    if (const char *e = std::getenv("RT_PT_DRAIN_ROUNDS")) s->pt_drain_rounds = std::max(0.0, std::atof(e));
    if (const char *e = std::getenv("RT_PT_DRAIN_SMALL")) s->pt_drain_small = (uint32_t)std::max(0, std::atoi(e));
    if (const char *e = std::getenv("RT_PT_SMALL_ROUNDS")) s->pt_small_rounds = std::max(0.0, std::atof(e));
    if (const char *e = std::getenv("RT_PT_SMALL_DRAIN_ROUNDS")) s->pt_small_drain_rounds = std::max(0.0, std::atof(e));
    if (const char *e = std::getenv("RT_TILE_ORDER")) s->tile_order = std::atoi(e) != 0;
    // RT_SPLIT_UNITS: sample-split target units (0 = never split)
    if (const char *e = std::getenv("RT_SPLIT_UNITS")) s->split_units = (uint32_t)std::max(0, std::atoi(e));
    if (const char *e = std::getenv("RT_FRAME_WAVES")) {
        const int w = std::atoi(e);
        s->frame_waves = w == 7 || w == 8 ? w : 0;
    }
    if (const char *e = std::getenv("RT_SPLIT_HEAVY")) s->heavy_split = std::max(-1, std::atoi(e));
    if (const char *e = std::getenv("RT_SPLIT_PARTS")) {
        const int k = std::atoi(e);
        s->split_parts = k >= 8 ? 8u : k >= 4 ? 4u : 2u;
    }
    if (const char *e = std::getenv("RT_PT_PIPELINE")) s->pt_pipeline = std::atoi(e) != 0;
    if (const char *e = std::getenv("RT_PT_SLOTS")) s->pt_slots = (uint32_t)std::max(2, std::min((int)kPtMaxSlots, std::atoi(e)));
    if (const char *e = std::getenv("RT_PS_PIPELINE")) s->ps_pipeline = std::max(-1, std::min(1, std::atoi(e)));
    if (const char *e = std::getenv("RT_PS_BUFFERS")) s->ps_buffers = (uint32_t)std::max(2, std::min(kPsMaxDepth + 1, std::atoi(e)));
    if (const char *e = std::getenv("RT_PS_DEPTH")) s->ps_depth = (uint32_t)std::max(2, std::min(kPsMaxDepth, std::atoi(e)));
    if (const char *e = std::getenv("RT_TUNE_DELAY_MS")) s->tune_delay_ms = (float)std::max(0.0, std::atof(e));
    if (const char *e = std::getenv("RT_PT_MEM_MB"))
        s->pt_mem_bytes = std::max<uint64_t>(1, std::strtoull(e, nullptr, 10)) << 20;
    // camera-ray walk: wave-coherent vs per-lane (RT_WAVE_PRIMARY=0/1 overrides the policy)
    const bool wave_ok = !s->has_cubes && s->nested && s->walk_fits;
    s->walk = wave_ok ? RT_WALK_AUTO : RT_WALK_LANE;
    if (const char *e = std::getenv("RT_WAVE_PRIMARY")) s->walk = std::atoi(e) != 0 && wave_ok ? RT_WALK_WAVE : RT_WALK_LANE;
}

int scene_create(const rt_scene_desc *d, rt_scene **out) {
    if (!d || !out) return fail(RT_ERR_INVALID, "rt_scene_create: empty or null description");
    *out = nullptr;
    PackOptions o;
    int rc = pack_options_from_env(o);
    if (rc != RT_OK) return rc;
    // the description's errors come before the device's: a machine without a GPU reports them too
    ScenePack p;
    if ((rc = pack_scene(d, o, p)) != RT_OK) return rc;
    if ((rc = ensure_device(d->device)) != RT_OK) return rc;

    rt_scene *s = new rt_scene();
    s->device = d->device;
    s->num_prims = d->num_prims;
    s->num_materials = d->num_materials;
    s->ext = p.ext;
    s->ext_fixed = p.ext_fixed;
    s->has_cubes = p.has_cubes;
    s->refit.boxes_finite = p.boxes_finite;
    s->quads = s->quad_lanes = p.has_quads;
    s->refit.sliver_lim = o.sliver_lim;
    s->refit.sticky_spheres = o.sticky_spheres;
    rc = upload(&s->d_nodes, p.nodes);
    if (rc == RT_OK) rc = upload(&s->d_prims, p.prims);
    if (rc == RT_OK) rc = upload(&s->d_shade, p.shade);
    if (rc == RT_OK) rc = upload(&s->d_mats, p.mats);
    if (rc == RT_OK) rc = upload(&s->d_sky, p.sky);
    if (rc == RT_OK) rc = upload(&s->d_xprims, p.xprims);
    if (rc == RT_OK) rc = upload(&s->d_tex, p.texels);
    if (rc == RT_OK && s->quads) rc = upload(&s->d_quads, p.quads);
    if (rc == RT_OK && hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess)
        rc = fail(RT_ERR_HIP, "hipStreamCreate failed");
    if (rc != RT_OK) { free_scene(s); return rc; }
    s->bvh = std::move(p.bvh);
    s->refit.pinfo = std::move(p.pinfo);
    s->refit.pbox = std::move(p.pbox);
    s->refit.pcen = std::move(p.pcen);

    SceneView &v = s->view;
    v = p.view;
    scene_tree_fields(s, p.view.root_word, p.nested, p.view.bounds_finite != 0);
    v.shade = (const float4 *)s->d_shade;
    v.mats = (const DevMaterial *)s->d_mats;
    v.sky = (const uint32_t *)s->d_sky;
    v.xprims = (const float4 *)s->d_xprims;
    v.tex = (const uint32_t *)s->d_tex;
    v.quads = s->quads ? (const float4 *)s->d_quads : nullptr;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, s->device) == hipSuccess && prop.multiProcessorCount > 0)
            s->num_cus = (uint32_t)prop.multiProcessorCount;
    }
    scene_knobs_from_env(s);
    *out = s;
    return RT_OK;
}

size_t stack_bytes(const rt_scene *s) { return (size_t)s->stack_depth * 256u * sizeof(uint32_t); }
// launches whose camera rays may take the wave walk (SceneView::wave_primary) also hold each wave's
// uniform stack of node words past the lane stacks (walk_words in rt_kernels.inc): 4 waves x depth
size_t walk_bytes(const rt_scene *s, const SceneView &v) {
    return v.wave_primary ? (size_t)s->stack_depth * 4u * sizeof(uint32_t) : 0u;
}
// the scene's kernel family: the extension build where the scene holds what only it knows
const Launchers &launchers(const rt_scene *s) { return s->ext ? kext::launchers() : kcore::launchers(); }
// pixels covered by a frame / shard launch (primary rays per sample)
uint64_t frame_pixels(const rt_renderer *r, const FrameArgs &F) {
    return rt::frame_pixels(r->W, r->H, F.ntiles_local, F.shard, F.nshards, F.tile_map ? r->map_host.data() : nullptr);
}

// d_sum: one float4 per pixel of every tile of the frame
size_t sum_bytes(const rt_renderer *r) { return (size_t)r->grid().ntiles * 64u * sizeof(float4); }

uint64_t fnv1a(const void *d, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char *c = static_cast<const unsigned char *>(d);
    for (size_t i = 0; i < n; ++i) h = (h ^ c[i]) * 1099511628211ull;
    return h;
}

// an explicit deal's tile list on the device (FrameArgs::tile_map); a changed list waits for
// every frame still reading the old one.  The list in use is compared element by element (a
// memcmp of at most ntiles words, the same O(n) as hashing it): a caller-supplied identity of
// the list could repeat after its owner was freed and reallocated, and the range /
// duplicate checks below must see every list that differs.
int set_tile_map(rt_renderer *r, const uint32_t *tiles, uint32_t n, uint32_t ntiles) {
    if (r->d_map.p && r->map_host.size() == n && (n == 0 || std::memcmp(r->map_host.data(), tiles, sizeof(uint32_t) * n) == 0))
        return RT_OK;
    const uint64_t h = fnv1a(tiles, sizeof(uint32_t) * n, fnv1a(&n, sizeof(n)));
    std::vector<uint8_t> seen(ntiles, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (tiles[i] >= ntiles || seen[tiles[i]]) return fail(RT_ERR_INVALID, "tile list: index out of range or repeated");
        seen[tiles[i]] = 1;
    }
    HIP_TRY(hipDeviceSynchronize());
    if (int rc = r->d_map.grow(sizeof(uint32_t) * std::max<size_t>(n, 1)); rc != RT_OK) return rc;   // (never empty: null = no deal)
    if (n) HIP_TRY(hipMemcpy(r->d_map.p, tiles, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    r->map_host.assign(tiles, tiles + n);
    r->map_hash = h;
    r->map_gen += 1;
    return RT_OK;
}

// The first n timing events of a row of rt_renderer::tune_ev, created as first needed.
int ensure_events(hipEvent_t *ev, int n) {
    if (!ev[0])
        for (int k = 0; k < n; ++k) HIP_TRY(hipEventCreate(&ev[k]));
    return RT_OK;
}
// The measured time of each timed group, once the last group's end event has completed.
int group_times(const hipEvent_t *ev, int groups, float *ms) {
    HIP_TRY(hipEventSynchronize(ev[2 * groups - 1]));
    for (int g = 0; g < groups; ++g) HIP_TRY(hipEventElapsedTime(&ms[g], ev[2 * g], ev[2 * g + 1]));
    return RT_OK;
}

// The renderer's overlap streams 0 .. n-1 and their ordering events, created as first needed.
// Only as many as a mode uses: each stream becomes a hardware queue of its own (up to
// GPU_MAX_HW_QUEUES), and with 8 queues, creating all 8 streams for a timing that used 2 left
// TEAPOT-F's frames slow for the next ~50 frames -- the first two frames-in-flight groups timed
// 2.5-3.1 / 2.2 ms against 1.5 / 1.6 for the last two (round 5, profiles/r05/hwq).
int ensure_pipe_streams(rt_renderer *r, int n) {
    n = std::min(n, kPsMaxDepth);
    if (!r->pt_res.fin[0])
        for (int k = 0; k <= kPtMaxSlots; ++k)
            if (int rc = r->pt_res.event(k); rc != RT_OK) return rc;
    for (int k = r->nstreams; k < n; ++k) {
        HIP_TRY(hipStreamCreateWithFlags(&r->pt_stream[k], hipStreamNonBlocking));
        // ordering between streams of this device only: a device-scope release
        HIP_TRY(hipEventCreateWithFlags(&r->pt_lv[k], hipEventDisableTiming | hipEventReleaseToDevice));
        r->nstreams = k + 1;
    }
    return RT_OK;
}

// Overlapped primary+shadow frames' result buffer b and its event, grown to `bytes` (overlap_step).
int ensure_ps_res(rt_renderer *r, uint32_t b, uint64_t bytes) {
    if (int rc = r->ps_res.event((int)b); rc != RT_OK) return rc;
    return r->ps_res.ensure((int)b, bytes);
}

// Wavefront path tracing of one frame / shard (PathArgs, rt_dev_types.h): the samples are
// processed in batches that fit RT_PT_MEM_MB (default 12288 MB) of path state; per batch
// one k_pt_level launch per bounce level, then k_pt_finish.
int launch_pt_frame(rt_renderer *r, const FrameArgs &F, SceneView view, bool tex, hipStream_t st,
                    uint32_t *tile_cost = nullptr) {
    rt_scene *s = r->scene;
    // camera rays of level 0 take the wave-coherent walk when the scene forces it, or when
    // the renderer's primary+shadow frames timed it faster (RT_WALK_AUTO)
    view.wave_primary = !s->has_cubes && s->nested && s->walk_fits &&
                        (s->walk == RT_WALK_WAVE || (s->walk == RT_WALK_AUTO && r->wave > 0));
    view.walk_stats = r->d_counters;
    view.walk_check = r->walk_check;
    view.quad_lanes = s->quad_lanes ? 1 : 0;
    const uint64_t npix = (uint64_t)F.ntiles_local * 64u;
    // pipelined: per-sample results of the whole frame in a frame-level buffer (two by frame
    // parity, up to 2 GB each); the serial path keeps them per batch with a running sum
    const uint64_t res_need = (uint64_t)F.spp * npix * 16u;
    const bool pipe = s->pt_pipeline && res_need <= (2ull << 30);
    // per slot: two slots of up to RT_PT_MEM_MB each when pipelined (fewer, larger batches and
    // frame-to-frame overlap beat more batches: CFG5-sub 8.85 ms with half the budget per slot
    // -- two batches a frame -- vs 8.51 ms with one batch a frame, profiles/r02/bench_pipe_*)
    const PathPlan plan = path_plan(F.spp, F.depth, npix, s->pt_mem_bytes, kQueueSegs);
    const uint64_t batch = plan.batch, np = plan.np, seg_cap = plan.seg_cap;
    const size_t qbytes = plan.qbytes, cbytes = plan.cbytes, need = plan.need;
    if (!r->d_sum)   // one float4 per pixel of the whole frame (a shard uses its first npix)
        HIP_TRY(hipMalloc(&r->d_sum, sum_bytes(r)));
    int par = 0;
    // slot 0 was last written on the caller's stream (a serial frame): that work is done before
    // a path stream takes the slot over (a rare switch: frames whose results exceed the buffer)
    if (pipe && r->pt_serial_last) HIP_TRY(hipStreamSynchronize(st));
    r->pt_serial_last = !pipe;
    if (pipe) {
        int rc = RT_OK;
        if (need > r->pt_need) {
            // as many slots as fit beside 8 GB of headroom (at least 2), decided again whenever a
            // frame needs larger slots: every pending frame is done, slots past the count freed
            HIP_TRY(hipDeviceSynchronize());
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            double avail = (double)free_b;
            for (const DevBuf &b : r->d_pt) avail += (double)b.bytes;
            const uint32_t k = path_slots(s->pt_slots, np, hw_queues(), need, avail);
            for (uint32_t j = k; j < (uint32_t)kPtMaxSlots; ++j)
                if ((rc = r->d_pt[j].release()) != RT_OK) return rc;
            if ((rc = r->pt_res.drop_from((int)k + 1)) != RT_OK) return rc;
            r->pt_nslots = k;
            r->pt_need = need;
            r->pt_slot = r->pt_parity = 0;
            for (bool &f : r->pt_res.fin_set) f = false;
        }
        par = r->pt_parity;
        r->pt_parity = (par + 1) % (int)(r->pt_nslots + 1);
        if ((rc = ensure_pipe_streams(r, (int)r->pt_nslots)) != RT_OK) return rc;
        if ((rc = r->pt_res.ensure(par, res_need)) != RT_OK) return rc;
    }
    bool used[kPtMaxSlots] = {};
    const size_t lds = stack_bytes(s);
    const Launchers &K = launchers(s);
    // levels are compacted level by level until one is small enough to drain (k_pt_level)
    const uint32_t drain_level = s->pt_drain_level;
    for (uint32_t s0 = 0; s0 < F.spp; s0 += (uint32_t)batch) {
        const int k = pipe ? r->pt_slot : 0;
        if (pipe) r->pt_slot = (r->pt_slot + 1) % (int)r->pt_nslots;
        hipStream_t X = pipe ? r->pt_stream[k] : st;
        const size_t slot_need = need + (pipe ? 0 : (size_t)np * 16u + 256u);   // serial: + the results
        // (a slot that grows waits for X: the slot's previous batch is done with it)
        if (int rc = r->d_pt[k].grow(slot_need, Wait::kStream, X); rc != RT_OK) return rc;
        // this frame's results buffer was last read by the finish of two frames ago
        if (pipe && !used[k] && r->pt_res.fin_set[par]) HIP_TRY(hipStreamWaitEvent(X, r->pt_res.fin[par], 0));
        if (pipe && !used[k] && tile_cost) HIP_TRY(hipStreamWaitEvent(X, r->cost_ev, 0));   // the cleared cost map
        if (pipe && !used[k])
            if (int rc = after_updates(s, X); rc != RT_OK) return rc;   // (serial: launch_render's wait on st)
        used[k] = true;
        char *b = r->d_pt[k].as<char>();
        auto take = [&](size_t bytes) { char *q = b; b += (bytes + 255u) & ~(size_t)255u; return q; };
        PathArgs P{};
        P.state = reinterpret_cast<float4 *>(take(np * 32u));
        uint32_t *q0 = reinterpret_cast<uint32_t *>(take(qbytes));
        uint32_t *q1 = reinterpret_cast<uint32_t *>(take(qbytes));
        P.qcount = reinterpret_cast<uint32_t *>(take(cbytes));
        P.seg_cap = (uint32_t)seg_cap;
        P.qhead = P.qcount + (size_t)(F.depth + 1) * kQueueSegs * 16u;
        P.dynamic = s->pt_dynamic ? 1 : 0;
        P.rec = reinterpret_cast<float4 *>(take((size_t)(F.depth - 1) * np * 32u));
        // per-path radiance, indexed (sample - s0) * npix + pixel
        P.result = pipe ? r->pt_res.at(par) + (size_t)s0 * npix : reinterpret_cast<float4 *>(take(np * 16u));
        P.sum = r->d_sum;
        P.tile_cost = tile_cost;
        uint32_t dlevel = drain_level;   // this batch's (a small batch drains from pt_drain_small on)
        P.drain_level = dlevel;
        P.drain_below = 0;
        P.s0 = s0;
        P.batch_spp = std::min<uint32_t>((uint32_t)batch, F.spp - s0);
        P.npaths = (uint32_t)(P.batch_spp * npix);
        HIP_TRY(hipMemsetAsync(P.qcount, 0, cbytes, X));
        for (uint32_t level = 0; level < F.depth; ++level) {
            P.level = level;
            P.queue_in = (level & 1u) ? q1 : q0;
            P.queue_out = (level & 1u) ? q0 : q1;
            int resident = 0;
            if (level > 0 && s->pt_lanes) {             // incoherent levels: the lane state machine
                K.pt_lanes(view, F, P, tex, lds, s->num_cus, X);
            } else {
                const size_t lv = level == 0 ? lds + walk_bytes(s, view) : lds;   // camera rays: the walk's words
                resident = K.pt_level(view, F, P, tex, lv, s->num_cus, X);
            }
            if (level >= dlevel) break;                // that launch finished every remaining level
            if (level == 0) {
                const bool small = s->pt_drain_small && (double)P.npaths <= s->pt_small_rounds * resident;
                P.drain_below = (uint32_t)std::min<double>(4e9, (small ? s->pt_small_drain_rounds : s->pt_drain_rounds) * resident);
                if (small) P.drain_level = dlevel = std::min(dlevel, s->pt_drain_small);
            }
        }
        if (!pipe) {   // serial: this batch's samples onto the running sum (the last: accumulate, RGB8)
            const bool last = s0 + P.batch_spp >= F.spp;
            K.pt_finish(F, P, last, st);
        }
    }
    if (pipe) {
        // one finishing pass on the caller's stream: every sample of the frame in sample order
        // (the same float sums as the batched running sum), after every batch's levels
        for (int k = 0; k < (int)r->pt_nslots; ++k)
            if (used[k]) {
                HIP_TRY(hipEventRecord(r->pt_lv[k], r->pt_stream[k]));
                HIP_TRY(hipStreamWaitEvent(st, r->pt_lv[k], 0));
            }
        PathArgs P{};
        P.result = r->pt_res.at(par);
        P.sum = r->d_sum;
        P.s0 = 0;
        P.batch_spp = F.spp;
        K.pt_finish(F, P, true, st);
        HIP_TRY(hipEventRecord(r->pt_res.fin[par], st));
        r->pt_res.fin_set[par] = true;
    }
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// The tile costs and the order of parameter set `key` with n local tiles: a new set drops what the
// last one recorded, a new tile count reallocates d_order / d_cost.
int ensure_order(rt_renderer *r, uint64_t key, uint32_t n) {
    if (key == r->order_key && n == r->order_n) return RT_OK;
    r->order_key = key;
    r->order_state = 0;
    r->host_cost.clear();
    if (n != r->order_n) {   // (a smaller count too: the buffers are exactly the set's)
        HIP_TRY(hipDeviceSynchronize());                             // frames may still read them
        r->order_n = 0;
        int rc = r->d_order.release();
        if (rc == RT_OK) rc = r->d_cost.release();
        if (rc == RT_OK) rc = r->d_order.grow(order_capacity(n) * sizeof(uint32_t));
        if (rc == RT_OK) rc = r->d_cost.grow(2u * (size_t)n * sizeof(uint32_t));   // one cost map per camera walk
        if (rc != RT_OK) return rc;
        r->order_n = n;
    }
    return RT_OK;
}

// What the steps of one primary+shadow / Whitted frame (launch_render) hand to each other.
struct FramePlan {
    uint64_t key = 0;                           // the frame's parameter set (param_key)
    bool gate_open = false, stalled = false;    // tune_gate; the GPU ran dry since the previous frame
    TimedFrame walk, split, ps;                 // tune_ev[kWalk / kSplit / kOverlap] around this launch
    int cost_map = -1;                          // this frame records the tile costs under walk 0 / 1
    bool walk_pending = false;                  // the walk was not decided before this frame
    uint32_t depth = 0, buf = 0, lane = 0;      // frames in flight (0 serial, else 2..6); result buffer, renderer stream
};

// The measured-cost tile order (build_tile_order, rt_sched.h): each tile's wave cycles are recorded on
// one frame, sorted on the host once, and from the next frame on slot i renders the i-th most
// expensive tile -- for as long as camera, size, spp, depth, mode and shard stay the same.
// With the RT_WALK_AUTO camera walk still being timed, the two timed frames record the costs
// under each walk and the frame that picks the walk applies the matching order (active from
// the 4th frame); otherwise frame 1 records and frame 2 applies.  Pixel values do not depend
// on the order.  walk_phase: -1 no walk timing pending, 0 / 1 this frame times the lane /
// wave walk, 2 the walk was picked on this frame, 3 the timing has not started yet.
int tile_order_step(rt_renderer *r, FrameArgs &F, bool split_ok, FramePlan &P) {
    const uint32_t n = F.ntiles_local;
    // the walk: costs recorded on this frame (0 / 1), decided on it (2), still to be timed (3)
    const int walk_phase = P.cost_map >= 0 ? P.cost_map : P.walk.decide ? 2 : P.walk_pending ? 3 : -1;
    if (P.key != r->order_key || n != r->order_n) {
        r->tail_bound = false;
        r->ps_tg.stop();   // the overlap decision belongs to the parameter set too
        r->ps_use = -1;
    }
    if (int rc = ensure_order(r, P.key, n); rc != RT_OK) return rc;
    uint32_t *const d_cost = r->d_cost.as<uint32_t>(), *const d_order = r->d_order.as<uint32_t>();
    int use = -1;                                                      // cost map to sort this frame
    if (walk_phase == 3) {
        // walk timing not started yet: record nothing
    } else if (r->order_state == 0) {
        if (walk_phase == 0 || walk_phase == 1) F.tile_cost = d_cost + (size_t)walk_phase * n;
        else if (walk_phase == 2) use = r->wave;                      // recorded on the timed frames
        else { F.tile_cost = d_cost; r->order_state = 1; }
    } else if (r->order_state == 1) {
        use = 0;
    }
    if (use >= 0) {
        // once per parameter set: a device-wide sync orders the cost read after the recording
        // frame and the order write after every frame still reading the previous order,
        // whatever streams the caller used
        HIP_TRY(hipDeviceSynchronize());
        std::vector<uint32_t> cost(n);
        HIP_TRY(hipMemcpy(cost.data(), d_cost + (size_t)use * n, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
        r->host_cost = cost;
        r->tail_bound = tail_bound(cost, r->scene->num_cus, F.nchunks);
        const uint32_t k = split_count(n, r->scene->heavy_split, split_ok), parts = r->scene->split_parts;
        const TileWhere where{F.tiles_x, F.shard, F.nshards, F.tile_map ? r->map_host.data() : nullptr};
        const std::vector<uint32_t> ent = build_tile_order(cost, k, parts, r->scene->xcd_order && split_ok, where);
        HIP_TRY(hipMemcpy(d_order, ent.data(), ent.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        r->order_split = k;
        r->order_parts = parts;
        r->order_state = 2;
        r->use_split = k > 0 && r->scene->heavy_split > 0;            // a forced count: no timing
        r->split_tg.stop();
        if (k > 0 && r->scene->heavy_split < 0) {                      // groups plain, split, split, plain
            start_two_way(r->split_tg, false);
            if (int rc = ensure_events(r->tune_ev[kSplit], 8); rc != RT_OK) return rc;
        }
    }
    if (r->order_state == 2) {
        P.split = r->split_tg.next(P.gate_open, P.stalled);
        if (P.split.decide) {
            if (int rc = group_times(r->tune_ev[kSplit], 4, r->split_ms); rc != RT_OK) return rc;
            r->use_split = tuned_alternative(r->split_ms);
        }
        const bool split = P.split.group >= 0 ? alternative_group(P.split) : r->use_split;
        F.order = split ? d_order + n : d_order;
        F.nunits = order_units(F.ntiles_local, F.nchunks, split, r->order_split, r->order_parts);
        F.part_shift = part_shift(r->order_parts);
    }
    return RT_OK;
}

// the parameter set a frame belongs to (the tuned choices and the tile order are per set)
uint64_t param_key(const rt_renderer *r, const FrameArgs &F, const rt_camera *cam, const rt_frame_params *p) {
    uint64_t key = fnv1a(cam, sizeof(*cam));
    key = fnv1a(&p->width, sizeof(uint32_t) * 4, key);   // width height spp depth
    key = fnv1a(&p->mode, sizeof(uint32_t), key);
    key = fnv1a(&F.shard, sizeof(uint32_t) * 2, key);    // shard nshards
    if (F.tile_map) key = fnv1a(&r->map_hash, sizeof(r->map_hash), key);   // an explicit deal's tile list
    return key;
}

// true once this parameter set's frames have run tune_delay_ms of GPU time (never blocks)
int tune_gate(rt_renderer *r, uint64_t key, hipStream_t st, bool &open) {
    const float delay = r->scene->tune_delay_ms;
    if (key != r->gate_key) {
        r->gate_key = key;
        r->gate_state = 0;
    }
    if (delay <= 0.0f) r->gate_state = 3;
    if (r->gate_state == 3) { open = true; return RT_OK; }
    open = false;
    if (int rc = ensure_events(r->tune_ev[kGate], 2); rc != RT_OK) return rc;
    if (r->gate_state == 0) {
        HIP_TRY(hipEventRecord(r->tune_ev[kGate][0], st));
        r->gate_state = 1;
        r->gate_frames = 0;
    } else if (r->gate_state == 1) {
        if (++r->gate_frames % 8 == 0) {
            HIP_TRY(hipEventRecord(r->tune_ev[kGate][1], st));
            r->gate_state = 2;
        }
    } else if (hipEventQuery(r->tune_ev[kGate][1]) == hipSuccess) {   // state 2: the probe has run
        float ms = 0.0f;
        HIP_TRY(hipEventElapsedTime(&ms, r->tune_ev[kGate][0], r->tune_ev[kGate][1]));
        r->gate_state = ms >= delay ? 3 : 1;
        open = r->gate_state == 3;
    }
    return RT_OK;
}

// The frame record of one rank's part of a frame (camera, size, the interleaved shard or the
// explicit tile list) -- shared by the frame launch and the dry-run work frame.
int frame_args(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
               const uint32_t *tiles, uint32_t ntiles_map, FrameArgs &F) {
    if (p->width != r->W || p->height != r->H)
        return fail(RT_ERR_INVALID, "frame size differs from the renderer's accumulator");
    if (p->spp == 0) return fail(RT_ERR_INVALID, "spp must be >= 1");
    if (p->mode > RT_MODE_BVH_HEAT) return fail(RT_ERR_INVALID, "unknown integrator mode");
    if (nshards == 0 || shard >= nshards) return fail(RT_ERR_INVALID, "bad shard index");
    HIP_TRY(hipSetDevice(r->scene->device));
    F = FrameArgs{};
    for (int i = 0; i < 3; ++i) {
        F.cam_pos[i] = cam->pos[i]; F.cam_tl[i] = cam->top_left[i];
        F.cam_tr[i] = cam->top_right[i]; F.cam_bl[i] = cam->bottom_left[i];
    }
    F.lens = cam->lens_radius;
    F.rw = 1.0f / (float)r->W;   // Camera::rWidth / rHeight (camera.h:98-99)
    F.rh = 1.0f / (float)r->H;
    F.W = r->W; F.H = r->H; F.spp = p->spp; F.depth = p->depth; F.frame = p->frame; F.reset = p->reset ? 1 : 0;
    const TileGrid g = r->grid();
    F.shard = shard; F.nshards = nshards; F.tiles_x = g.tiles_x;
    F.ntiles_local = local_tiles(g.ntiles, shard, nshards);
    if (tiles) {   // an explicit deal (rt_render_shard_tiles)
        int rc = set_tile_map(r, tiles, ntiles_map, g.ntiles);
        if (rc != RT_OK) return rc;
        F.ntiles_local = ntiles_map;
        F.tile_map = r->d_map.as<uint32_t>();
    }
    F.acc = r->d_acc;
    F.counters = r->d_counters;
    F.nchunks = 1;
    F.nunits = F.ntiles_local;
    return RT_OK;
}

// Dry-run work map (k_render_work) of one rank's part of a frame: per local tile, node visits +
// primitive tests of its rays summed over lanes and samples, read back to the host (blocking on
// `st`).  The camera rays take the reference-order lane walk whatever walk the renderer timed,
// so the map depends on the frame alone.  Path-traced / primary+shadow frames (RT_MODE_PATH) only.
int work_frame(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
               const uint32_t *tiles, uint32_t ntiles_map, std::vector<uint32_t> &work, uint32_t *pixel_work,
               hipStream_t st) {
    if (!r || !cam || !p) return fail(RT_ERR_INVALID, "work frame: null argument");
    if (p->mode != RT_MODE_PATH) return fail(RT_ERR_UNSUPPORTED, "work frame: RT_MODE_PATH frames only");
    if (p->depth > 32) return fail(RT_ERR_UNSUPPORTED, "Trace depth above 32");
    // the counting build keeps 8 per-lane counters past the stacks (launch_work): a tree deeper than
    // 56 leaves no room -- UNSUPPORTED, so rebalance() falls back to the measured cycle costs
    if (stack_bytes(r->scene) + kWorkCounterBytes > kLdsLaunchMax)
        return fail(RT_ERR_UNSUPPORTED, "work frame: this tree's stacks leave no LDS for the counters");
    FrameArgs F;
    int rc = frame_args(r, cam, p, shard, nshards, tiles, ntiles_map, F);
    if (rc != RT_OK) return rc;
    const uint32_t n = F.ntiles_local;
    work.assign(n, 0u);
    if (n == 0) return RT_OK;
    rt_scene *s = r->scene;
    if ((rc = r->d_work.grow(sizeof(uint32_t) * n, Wait::kDevice)) != RT_OK) return rc;
    uint32_t *const d_work = r->d_work.as<uint32_t>();
    if ((rc = after_updates(s, st)) != RT_OK) return rc;
    HIP_TRY(hipMemsetAsync(d_work, 0, sizeof(uint32_t) * n, st));
    SceneView view = s->view;
    view.wave_primary = 0;
    view.walk_check = RT_WALK_CHECK_OFF;
    view.walk_stats = nullptr;
    const FrameLaunch L{work_variant(p->depth, !s->view.sky_const), dim3((n + 3) / 4), stack_bytes(s), st};
    launchers(s).work(view, F, L, d_work, pixel_work);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(work.data(), d_work, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

// Sample split (sample_chunks, rt_sched.h): the frame's (tile, sample chunk) units; their samples go
// to d_samples.
int sample_split(rt_renderer *r, uint32_t spp, bool eligible, FrameArgs &F) {
    F.nchunks = sample_chunks(spp, F.ntiles_local, r->scene->split_units, eligible);
    F.nunits = F.ntiles_local * F.nchunks;
    if (F.nchunks > 1) {
        if (int rc = r->d_samples.grow(sizeof(float4) * (size_t)spp * F.ntiles_local * 64u); rc != RT_OK) return rc;
        F.samples = r->d_samples.as<float4>();
    }
    return RT_OK;
}

// A path-traced (depth >= 2) frame through the wavefront tracer, with the per-tile cost map of a
// path-traced parameter set (rt_renderer_tile_costs, the multi-GPU deal's input): each tile's
// level-0 wave cycles -- its camera rays, their shading and NEE, summed over the samples -- recorded
// on the set's first frame, read on its second (one device synchronisation per set); the bounce levels
// follow the camera level's hits, so a sky tile is cheap at every level.  No tile order is built from it.
int wavefront_frame(rt_renderer *r, const FrameArgs &F, const rt_camera *cam, const rt_frame_params *p, hipStream_t st) {
    rt_scene *s = r->scene;
    uint32_t *rec_cost = nullptr;
    if (s->tile_order) {
        const uint32_t n = F.ntiles_local;
        if (int rc = ensure_order(r, param_key(r, F, cam, p), n); rc != RT_OK) return rc;
        if (r->order_state == 0) {
            if (!r->cost_ev) HIP_TRY(hipEventCreateWithFlags(&r->cost_ev, hipEventDisableTiming | hipEventReleaseToDevice));
            rec_cost = r->d_cost.as<uint32_t>();
            HIP_TRY(hipMemsetAsync(rec_cost, 0, n * sizeof(uint32_t), st));
            HIP_TRY(hipEventRecord(r->cost_ev, st));
            r->order_state = 1;
        } else if (r->order_state == 1) {
            HIP_TRY(hipDeviceSynchronize());                                 // the recording frame is done
            r->host_cost.resize(n);
            HIP_TRY(hipMemcpy(r->host_cost.data(), r->d_cost.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
            r->order_state = 3;                                              // costs held, no order
        }
    }
    return launch_pt_frame(r, F, s->view, !s->view.sky_const, st, rec_cost);
}

// Camera-ray walk of this frame (only the global-node primary+shadow kernel, `walk_kernel`, has both).
// RT_WALK_AUTO times lane against wave (walk_tg: groups lane, wave, wave, lane) and keeps the faster.
int walk_step(rt_renderer *r, bool walk_kernel, SceneView &view, FramePlan &P) {
    const rt_scene *s = r->scene;
    const bool timed = walk_kernel && s->walk == RT_WALK_AUTO;
    // the walk's timed groups must all run on one parameter set's frames: a set change in the
    // middle (a multi-GPU deal switch, a camera move) restarts them from the warm-up
    if (timed && r->walk_tg.running() && P.key != r->walk_key) r->walk_tg.reset();
    if (!r->walk_tg.running()) r->walk_key = P.key;
    P.walk_pending = timed && r->wave < 0;
    if (walk_kernel && s->walk == RT_WALK_WAVE) view.wave_primary = 1;
    if (P.walk_pending) {
        if (int rc = ensure_events(r->tune_ev[kWalk], 8); rc != RT_OK) return rc;
        P.walk = r->walk_tg.next(P.gate_open, P.stalled);
        if (P.walk.decide) {
            if (int rc = group_times(r->tune_ev[kWalk], 4, r->walk_ms); rc != RT_OK) return rc;
            r->wave = tuned_alternative(r->walk_ms) ? 1 : 0;
        } else if (P.walk.group >= 0) {
            view.wave_primary = alternative_group(P.walk) ? 1 : 0;
            P.cost_map = walk_cost_map(P.walk);   // each walk's tile costs, on its first frame
        }
    }
    if (timed && r->wave >= 0) view.wave_primary = r->wave;
    return RT_OK;
}

// Overlapped primary+shadow frames: each pixel's accumulator update has to follow the previous
// frame's, but its traversal does not.  Once the frame is in its steady state (no timing events, no
// cost recording: `ps_ok`) the frame kernel runs on one of the renderer's overlap streams (by frame
// count) and stores its samples in a frame-level result buffer; a finishing pass on the caller's
// stream then does the running average + RGB8 (k_pt_finish, the same float operations as the
// kernel's own epilogue). Frame f+1's waves so fill the CUs that frame f's tail leaves idle.  The
// kernel touches only renderer-private memory; a stream waits only for the finishing pass that last
// read its result buffer.
// Three result buffers (RT_PS_BUFFERS): with two, frame f + 2's kernel waited for frame f's
// finishing pass while frame f + 1's kernel shared the CUs, which put the finishing pass and two
// cross-stream waits on the critical path (TEAPOT-F 1080p 0.119 ms per frame vs 0.1055 with three;
// four measure the same as three; profiles/r02/ps_window*.log).
// It pays where a frame is latency- or tail-bound (mig29 x16 1080p 0.41 -> 0.33 ms, 720p 0.385 ->
// 0.255 ms) and costs where it is issue-bound (TEAPOT-F 1080p 0.1024 -> 0.1055 ms: the finishing
// pass's extra 66 MB of sample traffic is not hidden there), and only when the caller submits
// frames back to back.  A small frame -- a multi-GPU rank's 1/N shard, about one round of resident
// waves -- is one latency chain long, and more frames in flight keep filling its idle issue slots:
// up to 6 renderer streams (round 3).  So by default each renderer times serial, 2, 4 and 6 frames
// in flight on its own frames and keeps the fastest (RT_PS_PIPELINE: -1 auto, 0 off, 1 on with
// RT_PS_DEPTH frames in flight).
// The timing's events go on the caller's stream after a frame: a group is timed from one frame's
// completion to another's, in steady state.  (Events before the first frame timed a deeper group
// short: its first kernels start on their streams while the caller's stream still finishes earlier
// frames; TEAPOT-F shards then picked 4-6 in flight, 0.125-0.144 ms against 0.092 with 2.  Round 4.)
int overlap_step(rt_renderer *r, FrameArgs &F, FrameLaunch &L, bool ps_ok, uint64_t ps_bytes, hipStream_t st, FramePlan &o) {
    const rt_scene *s = r->scene;
    o.depth = (ps_ok && s->ps_pipeline == 1) ? s->ps_depth : 0u;
    if (ps_ok && s->ps_pipeline < 0 && o.gate_open) {   // (gate closed: timing not started, serial)
        // a frame of another kind ran between two timing frames: time it all again
        if (r->ps_tg.running() && r->frames != r->ps_last + 1) r->ps_tg.stop();
        if (!r->ps_tg.active() && r->ps_use < 0) {
            // More than 2 frames in flight are candidates only for frames of a few rounds of resident
            // waves (a multi-GPU rank's small shard, 720p) or whose costliest tile outlasts twice the
            // frame's throughput time (tail_bound, from the tile-order cost map: mig29 x16 1080p and its
            // 1/2 shard, 16,200 tiles, 0.222 -> 0.167 ms with 4 in flight; round 4, depth_exp_*.jsonl);
            // a throughput-bound frame (TEAPOT-F 1080p, 8 rounds) lost with 4 (0.1035 -> 0.114 ms) and
            // the timing only risked picking them.
            const bool deep_ok = F.nunits <= 3u * 4u * 5u * s->num_cus || r->tail_bound;
            // streams, events and every result buffer before the timing
            const uint32_t maxd = deep_ok ? 6u : 2u, nb = s->ps_buffers ? s->ps_buffers : maxd + 1u;
            int rc = ensure_events(r->tune_ev[kOverlap], 16);
            if (rc == RT_OK) rc = ensure_pipe_streams(r, (int)maxd);
            for (uint32_t k = 0; k < nb && rc == RT_OK; ++k) rc = ensure_ps_res(r, k, ps_bytes);
            if (rc != RT_OK) return rc;
            start_overlap(r->ps_tg, deep_ok);
        }
        o.ps = r->ps_tg.next(true, o.stalled);
        if (o.ps.decide) {
            if (int rc = group_times(r->tune_ev[kOverlap], r->ps_tg.groups, r->ps_ms); rc != RT_OK) return rc;
            r->ps_use = (int)tuned_depth(r->ps_ms, r->ps_tg.groups);
            // every timed frame's finishing pass preceded the last event: no buffer is in use, and
            // the ones the chosen depth never touches are released (a 1080p spp-1 buffer is 33 MB)
            const uint32_t keep = r->ps_use == 0 ? 0u : (s->ps_buffers ? s->ps_buffers : r->ps_use + 1u);
            if (int rc = r->ps_res.drop_from((int)keep); rc != RT_OK) return rc;
        }
        o.depth = o.ps.group >= 0 ? overlap_depths(r->ps_tg.groups)[o.ps.group] : (uint32_t)r->ps_use;
        if (o.ps.group >= 0) r->ps_last = r->frames;
    }
    if (o.depth > 0) {
        if (int rc = ensure_pipe_streams(r, (int)o.depth); rc != RT_OK) return rc;
        // frame n's kernel on renderer stream n % depth, its samples in buffer n % buffers: with
        // depth + 1 buffers frame n + depth + 1 waits for frame n's finishing pass only, which
        // follows frame n's kernel alone -- never a kernel still running beside it
        const uint32_t buffers = s->ps_buffers ? s->ps_buffers : o.depth + 1u;
        o.buf = r->ps_count % buffers;
        o.lane = r->ps_count % o.depth;
        ++r->ps_count;
        if (int rc = ensure_ps_res(r, o.buf, ps_bytes); rc != RT_OK) return rc;
        L.stream = r->pt_stream[o.lane];
        if (r->ps_res.fin_set[o.buf]) HIP_TRY(hipStreamWaitEvent(L.stream, r->ps_res.fin[o.buf], 0));
        const bool timed_from = o.ps.group >= 0 && o.ps.index == r->ps_tg.skip;   // records the group's start event
        if (!r->ps_prev || timed_from) {
            // switching from serial frames: start behind the caller's stream; the frame a group is
            // timed from: every renderer stream starts behind everything before it, so that no
            // later frame of the group runs beside the previous group's (whose depth differs)
            if (!r->ps_join) HIP_TRY(hipEventCreateWithFlags(&r->ps_join, hipEventDisableTiming | hipEventReleaseToDevice));
            HIP_TRY(hipEventRecord(r->ps_join, st));
            if (timed_from)
                for (int k = 0; k < r->nstreams; ++k) HIP_TRY(hipStreamWaitEvent(r->pt_stream[k], r->ps_join, 0));
            else
                HIP_TRY(hipStreamWaitEvent(L.stream, r->ps_join, 0));
        }
        F.samples = r->ps_res.at((int)o.buf);
    }
    if (ps_ok) r->ps_prev = o.depth;
    return RT_OK;
}

// The frame on its streams: the timed choices' events around the kernel, the finishing pass of a
// frame that stored its samples, and the completion mark of the next submission's stall check.
int submit_frame(rt_renderer *r, const SceneView &view, const FrameArgs &F, const FrameLaunch &L, const FramePlan &o,
                 hipStream_t st) {
    const rt_scene *s = r->scene;
    if (o.walk.ev_before >= 0) HIP_TRY(hipEventRecord(r->tune_ev[kWalk][o.walk.ev_before], st));
    if (o.split.ev_before >= 0) HIP_TRY(hipEventRecord(r->tune_ev[kSplit][o.split.ev_before], st));
    launchers(s).frame(view, F, L);
    HIP_TRY(hipGetLastError());
    if (o.walk.ev_after >= 0) HIP_TRY(hipEventRecord(r->tune_ev[kWalk][o.walk.ev_after], st));
    if (o.split.ev_after >= 0) HIP_TRY(hipEventRecord(r->tune_ev[kSplit][o.split.ev_after], st));
    if (o.depth > 0) {
        HIP_TRY(hipEventRecord(r->pt_lv[o.lane], L.stream));
        HIP_TRY(hipStreamWaitEvent(st, r->pt_lv[o.lane], 0));
    }
    if (F.samples) {   // the pixels' samples in sample order, running average, RGB8
        PathArgs P{};
        P.batch_spp = F.spp;
        P.result = F.samples;
        launchers(s).pt_finish(F, P, true, st);
        HIP_TRY(hipGetLastError());
        if (o.depth > 0) {
            HIP_TRY(hipEventRecord(r->ps_res.fin[o.buf], st));
            r->ps_res.fin_set[o.buf] = true;
        }
    }
    if (o.ps.ev_after >= 0) HIP_TRY(hipEventRecord(r->tune_ev[kOverlap][o.ps.ev_after], st));
    // a timed group is running: mark this frame's completion for the next submission's stall check
    if (r->walk_tg.running() || r->split_tg.active() || r->ps_tg.active()) {
        if (!r->stall_ev) HIP_TRY(hipEventCreateWithFlags(&r->stall_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(r->stall_ev, st));
        r->stall_armed = true;
    }
    return RT_OK;
}

int launch_render(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
                  uint32_t *out, int packed, void *stream, const uint32_t *tiles = nullptr, uint32_t ntiles_map = 0,
                  const uint32_t *fwd_src = nullptr, uint32_t *fwd_dst = nullptr) {
    if (!r || !cam || !p || !out) return fail(RT_ERR_INVALID, "rt_render: null argument");
    if ((fwd_src || fwd_dst) && (packed || !fwd_src || !fwd_dst)) return fail(RT_ERR_INVALID, "rt_render: bad forward");
    rt_scene *s = r->scene;
    FrameArgs F;
    if (int rc = frame_args(r, cam, p, shard, nshards, tiles, ntiles_map, F); rc != RT_OK) return rc;
    if (tiles) {   // (copied only when the map changed: frames of one deal keep the same list)
        if (r->held_kind != 3 || r->held_gen != r->map_gen) {
            r->held_list = r->map_host;
            r->held_gen = r->map_gen;
        }
        r->held_kind = 3;
    } else {
        r->held_kind = nshards == 1 ? 1 : 2;
        r->held_shard = shard;
        r->held_nshards = nshards;
    }
    F.packed_out = packed;
    F.out = out;
    F.fwd_src = fwd_src;
    F.fwd_dst = fwd_dst;
    if (F.ntiles_local == 0) return RT_OK;
    hipStream_t st = (hipStream_t)stream;
    // the caller's stream (serial frames, the heat map, finishing passes); a renderer stream that
    // takes the frame kernel waits too (below, launch_pt_frame)
    if (int rc = after_updates(s, st); rc != RT_OK) return rc;
    if (p->mode == RT_MODE_BVH_HEAT) {
        // The BVH heat map: the plain serial launch in the tiles' own order.  It reads none of the
        // renderer's timed choices and writes none (no parameter key, gate, walk, order or overlap
        // step), so PATH frames before and after it see the state they left.  p->depth is ignored:
        // the kernel's depth is the tree's (bvhDepth, template/scene.h:282).
        F.depth = s->bvh.depth;
        kcore::launch_heat(s->view, F, stack_bytes(s), st);
        HIP_TRY(hipGetLastError());
        r->primary += frame_pixels(r, F) * p->spp;
        r->frames += 1;
        return RT_OK;
    }
    if (p->depth > 32) return fail(RT_ERR_UNSUPPORTED, "Trace depth above 32");   // = kWHITTED_MAX
    const int mode = (int)p->mode;
    const bool wavefront = mode == RT_MODE_PATH && p->depth >= 2 && s->pt_wavefront;
    if (int rc = sample_split(r, p->spp, mode != RT_MODE_PACKET && !wavefront, F); rc != RT_OK) return rc;
    if (wavefront) {
        if (int rc = wavefront_frame(r, F, cam, p, st); rc != RT_OK) return rc;
        r->primary += frame_pixels(r, F) * p->spp;
        r->frames += 1;
        return RT_OK;
    }
    FrameLaunch L{{}, dim3((F.nunits + 3) / 4), stack_bytes(s), st};
    SceneView view = s->view;
    view.walk_stats = r->d_counters;
    view.walk_check = r->walk_check;
    FramePlan P;
    P.key = param_key(r, F, cam, p);
    if (int rc = tune_gate(r, P.key, st, P.gate_open); rc != RT_OK) return rc;
    // did the GPU run dry since the previous frame?  (a timed group then restarts: kTuneRestarts)
    P.stalled = r->stall_armed && hipEventQuery(r->stall_ev) == hipSuccess;
    r->stall_armed = false;
    const bool ps_kernel = primary_shadow(mode, p->depth);   // the primary+shadow frame kernel
    if (int rc = walk_step(r, ps_kernel && !s->ext, view, P); rc != RT_OK) return rc;
    if (s->tile_order) {
        // half-tile units: primary+shadow frames of the global-node kernel, whole-tile units only
        if (int rc = tile_order_step(r, F, ps_kernel && F.nchunks <= 1, P); rc != RT_OK) return rc;
        L.grid = dim3((F.nunits + 3) / 4);
    }
    const uint64_t ps_bytes = (uint64_t)p->spp * F.ntiles_local * 64u * 16u;
    // (sample-split frames -- a multi-GPU rank's shard at spp N -- store their samples anyway;
    // overlapped, they go to the result buffers instead of d_samples)
    const bool ps_ok = s->ps_pipeline != 0 && ps_kernel && !r->split_tg.active() && !F.tile_cost && !P.walk_pending &&
                       ps_bytes <= (2ull << 30);
    if (int rc = overlap_step(r, F, L, ps_ok, ps_bytes, st, P); rc != RT_OK) return rc;
    if (L.stream != st)
        if (int rc = after_updates(s, L.stream); rc != RT_OK) return rc;
    L.lds_bytes = stack_bytes(s) + walk_bytes(s, view);   // the camera walk's word stack when it runs
    L.v = frame_variant({mode, p->depth, !view.sky_const, s->frame_waves, F.nchunks, F.spp, F.nunits, s->num_cus,
                         P.depth > 0, view.wave_primary, view.walk_check});
    if (int rc = submit_frame(r, view, F, L, P, st); rc != RT_OK) return rc;
    r->primary += frame_pixels(r, F) * p->spp;
    r->frames += 1;
    return RT_OK;
}

// rt_intersect / rt_occluded / rt_intersect_packets / rt_bvh_visualize: one batch of the caller's
// device rays, after the scene's pending updates, on the caller's stream
template <class Launch>
int ray_call(rt_scene *s, const void *rays, void *out, uint32_t n, void *stream, const char *null_text, Launch launch) {
    if (!s || (n && (!rays || !out))) return fail(RT_ERR_INVALID, null_text);
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    if (int rc = after_updates(s, st); rc != RT_OK) return rc;
    launch(st);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

// ---- first-hit G-buffer (rt_render_gbuffer, rt_gbuffer_pixels and their _host forms)
// Refusals come in the order a caller can check them: what the arguments alone decide (here), then the
// device, then what the renderer decides (its frame size) -- so a host without a GPU still hears about
// a bad argument first and never has its handle looked into.
int gbuffer_arguments(const std::string &name, const void *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample,
                      const rt_gbuffer *out) {
    if (!r || !cam || !p || !out) return fail(RT_ERR_INVALID, name + ": null argument");
    if (!out->ray && !out->hit && !out->normal && !out->albedo) return fail(RT_ERR_INVALID, name + ": no plane asked for");
    if (sample >= std::max(1u, p->spp)) return fail(RT_ERR_INVALID, name + ": sample outside the frame's samples per pixel");
    return RT_OK;
}
int gbuffer_rectangle(const std::string &name, const rt_frame_params *p, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h) {
    if (!w || !h) return fail(RT_ERR_INVALID, name + ": empty rectangle");
    if (x0 >= p->width || w > p->width - x0 || y0 >= p->height || h > p->height - y0)
        return fail(RT_ERR_INVALID, name + ": the rectangle leaves the frame");
    return RT_OK;
}
int gbuffer_device() {
    static const bool have = [] {
        int count = 0;
        return hipGetDeviceCount(&count) == hipSuccess && count > 0;
    }();
    return have ? RT_OK : fail(RT_ERR_NO_DEVICE, "no HIP device visible: the MI355X path has no CPU fallback");
}
// The scene's view as a query launches with it right now -- this query's camera walk, no walk counters --
// and the launch's dynamic LDS: the lane stacks, plus the wave walk's word stack when it runs.  The one
// place both are decided: the launch below and rt_renderer_gbuffer_walk read it.
SceneView gbuffer_view(const rt_renderer *r, bool pixels, size_t &lds) {
    const rt_scene *s = r->scene;
    SceneView view = s->view;
    view.wave_primary = gbuffer_wave_walk({pixels, s->walk, r->wave, s->ext, s->has_cubes, s->nested, s->walk_fits}) ? 1 : 0;
    view.walk_check = RT_WALK_CHECK_OFF;
    view.walk_stats = nullptr;
    lds = stack_bytes(s) + walk_bytes(s, view);
    return view;
}
// The launch: the frame's record for the camera, size and seed (nothing of the renderer's frame
// state goes into it or comes out of it), the scene's view with this query's camera walk, on the
// caller's stream behind the scene's pending updates.
int gbuffer_launch(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, GBufferArgs &G, bool pixels, hipStream_t st) {
    if (int rc = gbuffer_device(); rc != RT_OK) return rc;
    rt_frame_params q = *p;
    q.spp = std::max(1u, p->spp);
    q.mode = RT_MODE_PATH;
    FrameArgs F;
    if (int rc = frame_args(r, cam, &q, 0, 1, nullptr, 0, F); rc != RT_OK) return rc;   // (the frame size; the device)
    F.acc = nullptr;
    F.counters = nullptr;
    if (pixels && G.n == 0) return RT_OK;
    rt_scene *s = r->scene;
    if (int rc = after_updates(s, st); rc != RT_OK) return rc;
    size_t lds = 0;
    const SceneView view = gbuffer_view(r, pixels, lds);
    launchers(s).gbuffer(view, F, G, gbuffer_variant(pixels, !view.sky_const), lds, st);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}
GBufferArgs gbuffer_planes(const rt_gbuffer *out, uint32_t sample) {
    GBufferArgs G{};
    G.ray = out->ray; G.hit = out->hit; G.normal = out->normal; G.albedo = out->albedo;
    G.sample = sample;
    return G;
}
// The _host forms' staging in the scene's buffer, on its private stream, as the batched ray calls
// do: [pixel list] | ray | hit | normal | albedo, the asked-for planes only, 256-B aligned pieces of
// `count` records.  `run` launches with the device planes (and the device list).
template <class Run>
int gbuffer_staged(rt_renderer *r, const rt_frame_params *p, const uint32_t *list, size_t count, const rt_gbuffer *out, Run run) {
    if (int rc = gbuffer_device(); rc != RT_OK) return rc;
    if (p->width != r->W || p->height != r->H) return fail(RT_ERR_INVALID, "frame size differs from the renderer's accumulator");
    if (count == 0) return RT_OK;
    rt_scene *s = r->scene;
    HIP_TRY(hipSetDevice(s->device));
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    void *const host[4] = {out->ray, out->hit, out->normal, out->albedo};
    const size_t elem[4] = {sizeof(rt_ray), sizeof(rt_hit), sizeof(rt_gnormal), sizeof(rt_galbedo)};
    size_t off[4], need = list ? up(sizeof(uint32_t) * count) : 0;
    for (int k = 0; k < 4; ++k) {
        off[k] = need;
        if (host[k]) need += up(elem[k] * count);
    }
    if (int rc = grow(&s->d_scratch, &s->scratch_bytes, need); rc != RT_OK) return rc;
    char *b = (char *)s->d_scratch;
    if (list) HIP_TRY(hipMemcpyAsync(b, list, sizeof(uint32_t) * count, hipMemcpyHostToDevice, s->stream));
    rt_gbuffer dev{};
    dev.ray = out->ray ? (rt_ray *)(b + off[0]) : nullptr;
    dev.hit = out->hit ? (rt_hit *)(b + off[1]) : nullptr;
    dev.normal = out->normal ? (rt_gnormal *)(b + off[2]) : nullptr;
    dev.albedo = out->albedo ? (rt_galbedo *)(b + off[3]) : nullptr;
    if (int rc = run((const uint32_t *)b, &dev, s->stream); rc != RT_OK) return rc;
    for (int k = 0; k < 4; ++k)
        if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], b + off[k], elem[k] * count, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return RT_OK;
}

}  // namespace

// accumulator <-> packed [tile][64] float4 of listed tiles: one wave per tile, one lane per pixel
__global__ __launch_bounds__(256) void k_acc_tiles(float4 *__restrict__ acc, float4 *__restrict__ buf,
                                                   const uint32_t *__restrict__ tiles, uint32_t n, uint32_t tiles_x,
                                                   uint32_t W, uint32_t H, int unpack) {
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= n) return;
    const uint32_t t = tiles[i];
    const uint32_t x = (t % tiles_x) * 8u + (lane & 7u), y = (t / tiles_x) * 8u + (lane >> 3);
    const bool on = x < W && y < H;
    if (unpack) {
        if (on) acc[x + (size_t)y * W] = buf[(size_t)i * 64u + lane];
    } else {
        buf[(size_t)i * 64u + lane] = on ? acc[x + (size_t)y * W] : make_float4(0, 0, 0, 0);
    }
}

int rt::renderer_accumulator(rt_renderer *r, void **acc_dev, size_t *bytes) {
    if (!r || !acc_dev || !bytes) return fail(RT_ERR_INVALID, "null argument");
    *acc_dev = r->d_acc;
    *bytes = sizeof(float4) * (size_t)r->W * r->H;
    return RT_OK;
}

static int acc_tiles(rt_renderer *r, const uint32_t *d_tiles, uint32_t n, void *buf, void *stream, int unpack) {
    if (!r || (n && (!d_tiles || !buf))) return fail(RT_ERR_INVALID, "null argument");
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(r->scene->device));
    const uint32_t tiles_x = r->grid().tiles_x;
    hipLaunchKernelGGL(k_acc_tiles, dim3((n + 3) / 4), dim3(256), 0, (hipStream_t)stream, r->d_acc,
                       static_cast<float4 *>(buf), d_tiles, n, tiles_x, r->W, r->H, unpack);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt::accumulator_pack(rt_renderer *r, const uint32_t *tiles_dev, uint32_t n, void *buf_dev, void *stream) {
    return acc_tiles(r, tiles_dev, n, buf_dev, stream, 0);
}

int rt::accumulator_unpack(rt_renderer *r, const uint32_t *tiles_dev, uint32_t n, const void *buf_dev, void *stream) {
    return acc_tiles(r, tiles_dev, n, const_cast<void *>(buf_dev), stream, 1);
}

int rt::render_part(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
                    const uint32_t *tiles, uint32_t n, int packed, uint32_t *out_dev, void *stream,
                    const uint32_t *fwd_src, uint32_t *fwd_dst) {
    if (!r) return fail(RT_ERR_INVALID, "render_part: null renderer");
    if (tiles || n)
        return launch_render(r, cam, p, 0, 1, out_dev, packed, stream, tiles ? tiles : reinterpret_cast<const uint32_t *>(r), n,
                             fwd_src, fwd_dst);
    return launch_render(r, cam, p, shard, nshards, out_dev, packed, stream, nullptr, 0, fwd_src, fwd_dst);
}

int rt::render_work(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
                    const uint32_t *tiles, uint32_t n, std::vector<uint32_t> &work, void *stream) {
    if (!r) return fail(RT_ERR_INVALID, "render_work: null renderer");
    if (tiles || n)
        return work_frame(r, cam, p, 0, 1, tiles ? tiles : reinterpret_cast<const uint32_t *>(r), n, work, nullptr, (hipStream_t)stream);
    return work_frame(r, cam, p, shard, nshards, nullptr, 0, work, nullptr, (hipStream_t)stream);
}

bool rt::renderer_held_tiles(const rt_renderer *r, std::vector<uint32_t> &tiles) {
    return held_tiles(r->held_kind, r->grid().ntiles, r->held_shard, r->held_nshards, r->held_list, tiles);
}

int rt::renderer_geometry(const rt_renderer *r, uint32_t *W, uint32_t *H, int *device) {
    if (!r) return fail(RT_ERR_INVALID, "null renderer");
    *W = r->W;
    *H = r->H;
    *device = r->scene->device;
    return RT_OK;
}

extern "C" {

int rt_device_count(int *count) {
    if (!count) return fail(RT_ERR_INVALID, "null count");
    *count = 0;
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) return fail(RT_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
    *count = c;
    return RT_OK;
}

int rt_scene_create(const rt_scene_desc *desc, rt_scene **out) {
    try {
        return scene_create(desc, out);
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID, std::string("rt_scene_create: ") + e.what());
    }
}

int rt_scene_create_recipe(const char *name, const char *mesh_dir, int32_t device, rt_scene **out) {
    return rt_scene_create_recipe_ex(name, mesh_dir, device, RT_BVH_PLAIN, out);
}

int rt_scene_create_recipe_ex(const char *name, const char *mesh_dir, int32_t device, int32_t bvh_kind, rt_scene **out) {
    if (!name || !mesh_dir || !out) return fail(RT_ERR_INVALID, "rt_scene_create_recipe: null argument");
    try {
        SceneSource src;
        int rc = recipe_source(name, mesh_dir, src);
        if (rc != RT_OK) return rc;
        rt_scene_desc d{};
        d.prims = src.prims.data();
        d.num_prims = (uint32_t)src.prims.size();
        d.materials = src.materials.data();
        d.num_materials = (uint32_t)src.materials.size();
        d.device = device;
        d.bvh_kind = bvh_kind;
        return scene_create(&d, out);
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID, std::string("rt_scene_create_recipe: ") + e.what());
    }
}

int rt_scene_destroy(rt_scene *s) {
    free_scene(s);   // waits for the whole device: nothing of an async update is left to fold
    return RT_OK;
}

int rt_scene_get_info(const rt_scene *s, rt_scene_info *info) {
    if (!s || !info) return fail(RT_ERR_INVALID, "null argument");
    info->num_prims = s->num_prims;
    info->nodes_used = s->bvh.nodes_used;
    info->depth = s->bvh.depth;
    info->max_leaf = s->bvh.max_leaf;
    info->num_refs = (uint32_t)s->bvh.indices.size();
    return RT_OK;
}

int rt_scene_set_camera_walk(rt_scene *s, int walk) {
    if (!s) return fail(RT_ERR_INVALID, "null argument");
    if (walk != RT_WALK_LANE && walk != RT_WALK_WAVE && walk != RT_WALK_AUTO)
        return fail(RT_ERR_INVALID, "unknown camera walk");
    if (walk != RT_WALK_LANE && s->has_cubes)
        return fail(RT_ERR_UNSUPPORTED, "the wave walk needs order-independent hits; cubes accept on tmax (Primitive.h:221-233)");
    if (walk != RT_WALK_LANE && !s->nested)
        return fail(RT_ERR_UNSUPPORTED, "the wave walk needs every child box inside its parent's (this prebuilt BVH has one outside)");
    if (walk != RT_WALK_LANE && !s->walk_fits)
        return fail(RT_ERR_UNSUPPORTED, "the wave walk's word stack does not fit beside this tree's lane stacks (64 KB of LDS)");
    s->walk = walk;
    return RT_OK;
}

int rt_scene_copy_bvh(const rt_scene *cs, void *nodes, uint32_t *indices) {
    if (!cs || !nodes || !indices) return fail(RT_ERR_INVALID, "null argument");
    rt_scene *s = const_cast<rt_scene *>(cs);
    if (int frc = fold_updates(s); frc != RT_OK) return frc;   // the async updates first (rt_scene_update_sync)
    // boxes refitted, or the whole tree rebuilt, on the device since the last copy (both block, so they are settled)
    if (s->refit.bvh_stale || s->refit.topo_stale) {
        HIP_TRY(hipSetDevice(s->device));
        try {
            const int rc = sync_host_tree(s->refit, s->bvh, s->d_nodes);
            if (rc != RT_OK) return rc;
        } catch (const std::exception &e) {
            return fail(RT_ERR_INVALID, std::string("rt_scene_copy_bvh: ") + e.what());
        }
    }
    std::memcpy(nodes, s->bvh.nodes.data(), sizeof(Node) * s->bvh.nodes_used);
    std::memcpy(indices, s->bvh.indices.data(), sizeof(uint32_t) * s->bvh.indices.size());
    return RT_OK;
}

int rt_intersect(rt_scene *s, const rt_ray *rays, rt_hit *hits, uint32_t n, void *stream) {
    return ray_call(s, rays, hits, n, stream, "rt_intersect: null argument",
                    [&](hipStream_t st) { launchers(s).intersect(s->view, rays, hits, n, stack_bytes(s), st); });
}

int rt_occluded(rt_scene *s, const rt_ray *rays, uint8_t *out, uint32_t n, void *stream) {
    return ray_call(s, rays, out, n, stream, "rt_occluded: null argument",
                    [&](hipStream_t st) { launchers(s).occluded(s->view, rays, out, n, stack_bytes(s), st); });
}

int rt_intersect_packets(rt_scene *s, const rt_ray *rays, rt_hit *hits, uint32_t n, void *stream) {
    return ray_call(s, rays, hits, n, stream, "rt_intersect_packets: null argument",
                    [&](hipStream_t st) { launchers(s).intersect_packet(s->view, rays, hits, n, st); });
}
int rt_trace(rt_scene *s, int mode, const rt_ray *rays, uint32_t *seeds, const uint8_t *flags, uint32_t depth,
             float *radiance, rt_hit *hits, uint64_t *ray_counts, uint32_t n, void *stream) {
    if (!s || (n && (!rays || !seeds || !radiance))) return fail(RT_ERR_INVALID, "rt_trace: null argument");
    if (mode != RT_MODE_PATH && mode != RT_MODE_WHITTED) return fail(RT_ERR_INVALID, "rt_trace: mode must be PATH or WHITTED");
    if (depth > 32) return fail(RT_ERR_UNSUPPORTED, "Trace depth above 32");
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    TraceArgs A{};
    A.rays = rays; A.seeds = seeds; A.flags = flags; A.radiance = radiance; A.hits = hits;
    A.counts = reinterpret_cast<unsigned long long *>(ray_counts);
    A.n = n; A.depth = depth;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = after_updates(s, st); rc != RT_OK) return rc;
    launchers(s).trace(s->view, A, trace_variant(mode, depth, !s->view.sky_const), stack_bytes(s), st);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_trace_host(rt_scene *s, int mode, const rt_ray *rays, uint32_t *seeds, const uint8_t *flags, uint32_t depth,
                  float *radiance, rt_hit *hits, uint64_t *ray_counts, uint32_t n) {
    if (!s || (n && (!rays || !seeds || !radiance))) return fail(RT_ERR_INVALID, "rt_trace_host: null argument");
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    // staging: rays | seeds | flags | radiance | hits | counts, 256-B aligned pieces
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_seed = up(sizeof(rt_ray) * (size_t)n), o_flag = o_seed + up(4 * (size_t)n),
                 o_rad = o_flag + up((size_t)n), o_hit = o_rad + up(12 * (size_t)n),
                 o_cnt = o_hit + up(sizeof(rt_hit) * (size_t)n), need = o_cnt + 256;
    if (int rc = grow(&s->d_scratch, &s->scratch_bytes, need)) return rc;
    char *b = (char *)s->d_scratch;
    HIP_TRY(hipMemcpyAsync(b, rays, sizeof(rt_ray) * n, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(b + o_seed, seeds, 4 * (size_t)n, hipMemcpyHostToDevice, s->stream));
    if (flags) HIP_TRY(hipMemcpyAsync(b + o_flag, flags, n, hipMemcpyHostToDevice, s->stream));
    if (ray_counts) HIP_TRY(hipMemcpyAsync(b + o_cnt, ray_counts, 16, hipMemcpyHostToDevice, s->stream));
    int rc = rt_trace(s, mode, (const rt_ray *)b, (uint32_t *)(b + o_seed), flags ? (const uint8_t *)(b + o_flag) : nullptr,
                      depth, (float *)(b + o_rad), hits ? (rt_hit *)(b + o_hit) : nullptr,
                      ray_counts ? (uint64_t *)(b + o_cnt) : nullptr, n, s->stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(radiance, b + o_rad, 12 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(seeds, b + o_seed, 4 * (size_t)n, hipMemcpyDeviceToHost, s->stream));
    if (hits) HIP_TRY(hipMemcpyAsync(hits, b + o_hit, sizeof(rt_hit) * n, hipMemcpyDeviceToHost, s->stream));
    if (ray_counts) HIP_TRY(hipMemcpyAsync(ray_counts, b + o_cnt, 16, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return RT_OK;
}

enum { CALL_INTERSECT, CALL_OCCLUDED, CALL_PACKETS, CALL_VISUALIZE };
static int staged_call(rt_scene *s, const rt_ray *rays, void *out, size_t out_elem, uint32_t n, int kind) {
    if (!s || (n && (!rays || !out))) return fail(RT_ERR_INVALID, "null argument");
    if (n == 0) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    size_t need = (size_t)n * (sizeof(rt_ray) + out_elem) + 256;
    if (int rc = grow(&s->d_scratch, &s->scratch_bytes, need)) return rc;
    rt_ray *d_rays = (rt_ray *)s->d_scratch;
    char *d_out = (char *)s->d_scratch + (((size_t)n * sizeof(rt_ray) + 255) & ~(size_t)255);
    HIP_TRY(hipMemcpyAsync(d_rays, rays, sizeof(rt_ray) * n, hipMemcpyHostToDevice, s->stream));
    int rc = kind == CALL_OCCLUDED ? rt_occluded(s, d_rays, (uint8_t *)d_out, n, s->stream)
             : kind == CALL_PACKETS ? rt_intersect_packets(s, d_rays, (rt_hit *)d_out, n, s->stream)
             : kind == CALL_VISUALIZE ? rt_bvh_visualize(s, d_rays, (uint32_t *)d_out, n, s->stream)
                                    : rt_intersect(s, d_rays, (rt_hit *)d_out, n, s->stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, out_elem * n, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return RT_OK;
}

int rt_intersect_host(rt_scene *s, const rt_ray *rays, rt_hit *hits, uint32_t n) {
    return staged_call(s, rays, hits, sizeof(rt_hit), n, CALL_INTERSECT);
}
int rt_occluded_host(rt_scene *s, const rt_ray *rays, uint8_t *out, uint32_t n) {
    return staged_call(s, rays, out, 1, n, CALL_OCCLUDED);
}
int rt_intersect_packets_host(rt_scene *s, const rt_ray *rays, rt_hit *hits, uint32_t n) {
    return staged_call(s, rays, hits, sizeof(rt_hit), n, CALL_PACKETS);
}

// Batched Scene::BVHVisualization (k_bvh_visualize; the core build serves every scene: nodes only)
int rt_bvh_visualize(rt_scene *s, const rt_ray *rays, uint32_t *counts, uint32_t n, void *stream) {
    return ray_call(s, rays, counts, n, stream, "rt_bvh_visualize: null argument",
                    [&](hipStream_t st) { kcore::launch_visualize(s->view, rays, counts, n, stack_bytes(s), st); });
}
int rt_bvh_visualize_host(rt_scene *s, const rt_ray *rays, uint32_t *counts, uint32_t n) {
    return staged_call(s, rays, counts, 2 * sizeof(uint32_t), n, CALL_VISUALIZE);
}

// Tree cost of the scene's current device nodes (rt_cost.hip)
int rt_scene_bvh_cost(rt_scene *s, rt_bvh_cost *out, void *stream) {
    if (!s || !out) return fail(RT_ERR_INVALID, "rt_scene_bvh_cost: null argument");
    if (int frc = fold_updates(s); frc != RT_OK) return frc;   // the async updates first (rt_scene_update_sync)
    if (!s->view.bounds_finite) return fail(RT_ERR_UNSUPPORTED, "rt_scene_bvh_cost: a node bound is NaN or infinite");
    HIP_TRY(hipSetDevice(s->device));
    rt_bvh_cost c{};
    const int rc = device_bvh_cost(s->d_nodes, s->bvh.nodes_used, &s->d_cost, (hipStream_t)stream, &c);
    if (rc == RT_OK) *out = c;
    return rc;
}

int rt_renderer_create(rt_scene *s, uint32_t W, uint32_t H, rt_renderer **out) {
    if (!s || !out || !W || !H) return fail(RT_ERR_INVALID, "rt_renderer_create: bad argument");
    if ((uint64_t)W * H >= (1ull << 31)) return fail(RT_ERR_UNSUPPORTED, "frame too large");
    HIP_TRY(hipSetDevice(s->device));
    rt_renderer *r = new rt_renderer();
    r->scene = s;
    r->device = s->device;
    r->W = W; r->H = H;
    start_two_way(r->walk_tg, true);
    hipError_t e = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipMalloc(&r->d_acc, sizeof(float4) * (size_t)W * H);   // Renderer::Init, renderer.cpp:6-12
    if (e == hipSuccess) e = hipMemsetAsync(r->d_acc, 0, sizeof(float4) * (size_t)W * H, r->stream);
    if (e == hipSuccess) e = hipMalloc(&r->d_counters, kCounterSlots * 8 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMemsetAsync(r->d_counters, 0, kCounterSlots * 8 * sizeof(unsigned long long), r->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(r->stream);   // ready before any caller stream uses it
    if (e != hipSuccess) {
        if (r->d_acc) (void)hipFree(r->d_acc);
        if (r->d_counters) (void)hipFree(r->d_counters);
        if (r->stream) (void)hipStreamDestroy(r->stream);
        delete r;
        return fail(RT_ERR_HIP, std::string("rt_renderer_create: ") + hipGetErrorString(e));
    }
    *out = r;
    return RT_OK;
}

int rt_renderer_destroy(rt_renderer *r) {
    if (!r) return RT_OK;
    // not r->scene->device: the scene may already be gone, and a freed scene's bytes gave
    // hipSetDevice an invalid ordinal, which the thread's next hipGetLastError() then reported
    (void)hipSetDevice(r->device);
    (void)hipDeviceSynchronize();   // kernels on caller streams may still read the buffers
    (void)hipFree(r->d_acc);
    (void)hipFree(r->d_counters);
    if (r->d_rgb) (void)hipFree(r->d_rgb);
    if (r->d_sum) (void)hipFree(r->d_sum);
    each_buffer(*r, [](DevBuf &b) { (void)b.release(); });
    for (int k = 0; k < kPsMaxDepth; ++k) {
        if (r->pt_stream[k]) (void)hipStreamDestroy(r->pt_stream[k]);
        if (r->pt_lv[k]) (void)hipEventDestroy(r->pt_lv[k]);
    }
    for (auto &row : r->tune_ev)
        for (auto &e : row)
            if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : r->pt_res.fin)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : r->ps_res.fin)
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : {r->ps_join, r->cost_ev, r->stall_ev})
        if (e) (void)hipEventDestroy(e);
    (void)hipStreamDestroy(r->stream);
    delete r;
    return RT_OK;
}

int rt_render_frame(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t *rgb8, void *stream) {
    return launch_render(r, cam, p, 0, 1, rgb8, 0, stream);
}

int rt_render_frame_host(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t *rgb8) {
    if (!r || !rgb8) return fail(RT_ERR_INVALID, "rt_render_frame_host: null argument");
    HIP_TRY(hipSetDevice(r->scene->device));
    if (!r->d_rgb) HIP_TRY(hipMalloc(&r->d_rgb, sizeof(uint32_t) * (size_t)r->W * r->H));
    int rc = launch_render(r, cam, p, 0, 1, r->d_rgb, 0, r->stream);
    if (rc != RT_OK) return rc;
    HIP_TRY(hipMemcpyAsync(rgb8, r->d_rgb, sizeof(uint32_t) * (size_t)r->W * r->H, hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return RT_OK;
}

int rt_render_gbuffer(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample, uint32_t x0, uint32_t y0,
                      uint32_t w, uint32_t h, const rt_gbuffer *out, void *stream) {
    const char *name = "rt_render_gbuffer";
    if (int rc = gbuffer_arguments(name, r, cam, p, sample, out); rc != RT_OK) return rc;
    if (int rc = gbuffer_rectangle(name, p, x0, y0, w, h); rc != RT_OK) return rc;
    GBufferArgs G = gbuffer_planes(out, sample);
    G.x0 = x0; G.y0 = y0; G.w = w; G.h = h;
    G.tx0 = x0 / 8u; G.ty0 = y0 / 8u;
    G.ntx = (x0 + w + 7u) / 8u - G.tx0;
    G.ntiles = G.ntx * ((y0 + h + 7u) / 8u - G.ty0);
    return gbuffer_launch(r, cam, p, G, false, (hipStream_t)stream);
}

int rt_render_gbuffer_host(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample, uint32_t x0,
                           uint32_t y0, uint32_t w, uint32_t h, const rt_gbuffer *out) {
    const char *name = "rt_render_gbuffer_host";
    if (int rc = gbuffer_arguments(name, r, cam, p, sample, out); rc != RT_OK) return rc;
    if (int rc = gbuffer_rectangle(name, p, x0, y0, w, h); rc != RT_OK) return rc;
    return gbuffer_staged(r, p, nullptr, (size_t)w * h, out, [&](const uint32_t *, const rt_gbuffer *dev, hipStream_t st) {
        return rt_render_gbuffer(r, cam, p, sample, x0, y0, w, h, dev, st);
    });
}

int rt_gbuffer_pixels(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample, const uint32_t *pixels,
                      uint32_t n, const rt_gbuffer *out, void *stream) {
    const char *name = "rt_gbuffer_pixels";
    if (int rc = gbuffer_arguments(name, r, cam, p, sample, out); rc != RT_OK) return rc;
    if (n && !pixels) return fail(RT_ERR_INVALID, std::string(name) + ": null pixel list");
    GBufferArgs G = gbuffer_planes(out, sample);
    G.pixels = pixels;
    G.n = n;
    return gbuffer_launch(r, cam, p, G, true, (hipStream_t)stream);
}

int rt_gbuffer_pixels_host(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample,
                           const uint32_t *pixels, uint32_t n, const rt_gbuffer *out) {
    const char *name = "rt_gbuffer_pixels_host";
    if (int rc = gbuffer_arguments(name, r, cam, p, sample, out); rc != RT_OK) return rc;
    if (n && !pixels) return fail(RT_ERR_INVALID, std::string(name) + ": null pixel list");
    for (uint32_t i = 0; i < n; ++i)
        if (pixels[i] >= (uint64_t)p->width * p->height)
            return fail(RT_ERR_INVALID, std::string(name) + ": pixel " + std::to_string(i) + " lies outside the frame");
    return gbuffer_staged(r, p, pixels, n, out, [&](const uint32_t *list, const rt_gbuffer *dev, hipStream_t st) {
        return rt_gbuffer_pixels(r, cam, p, sample, list, n, dev, st);
    });
}

int rt_renderer_gbuffer_walk(const rt_renderer *r, int pixels, int *wave_walk, uint32_t *lds_bytes) {
    if (!r || !wave_walk) return fail(RT_ERR_INVALID, "rt_renderer_gbuffer_walk: null argument");
    size_t lds = 0;
    *wave_walk = gbuffer_view(r, pixels != 0, lds).wave_primary;
    if (lds_bytes) *lds_bytes = (uint32_t)lds;
    return RT_OK;
}

int rt_shard_capacity(uint32_t W, uint32_t H, uint32_t nshards, uint32_t *pixels) {
    if (!pixels || !nshards || !W || !H) return fail(RT_ERR_INVALID, "rt_shard_capacity: bad argument");
    *pixels = local_tiles(tile_grid(W, H).ntiles, 0, nshards) * 64u;   // shard 0's count: no shard has more
    return RT_OK;
}

int rt_render_shard(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
                    uint32_t *tiles, void *stream) {
    return launch_render(r, cam, p, shard, nshards, tiles, 1, stream);
}

int rt_assemble_shards(rt_renderer *r, const uint32_t *gathered, uint32_t nshards, uint32_t *rgb8, void *stream) {
    if (!r || !gathered || !rgb8 || !nshards) return fail(RT_ERR_INVALID, "rt_assemble_shards: bad argument");
    HIP_TRY(hipSetDevice(r->scene->device));
    uint32_t cap = 0;
    rt_shard_capacity(r->W, r->H, nshards, &cap);
    const TileGrid g = r->grid();
    hipStream_t st = (hipStream_t)stream;
    launch_assemble(gathered, cap, nshards, nullptr, g.tiles_x, g.ntiles, r->W, r->H, rgb8, st);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_render_shard_tiles(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, const uint32_t *tiles,
                          uint32_t ntiles, uint32_t *tiles_dev, void *stream) {
    if (!r || (ntiles && !tiles)) return fail(RT_ERR_INVALID, "rt_render_shard_tiles: null argument");
    return launch_render(r, cam, p, 0, 1, tiles_dev, 1, stream, tiles ? tiles : reinterpret_cast<const uint32_t *>(r), ntiles);
}

int rt_assemble_tiles(rt_renderer *r, const uint32_t *gathered, uint32_t stride_px, const uint32_t *deal_tiles,
                      const uint32_t *deal_off, uint32_t nshards, uint32_t *rgb8, void *stream) {
    if (!r || !gathered || !deal_tiles || !deal_off || !rgb8 || !nshards || nshards > 255)
        return fail(RT_ERR_INVALID, "rt_assemble_tiles: bad argument");
    HIP_TRY(hipSetDevice(r->scene->device));
    const uint32_t tiles_x = r->grid().tiles_x, ntiles = r->grid().ntiles;
    if (deal_off[0] != 0 || deal_off[nshards] != ntiles) return fail(RT_ERR_INVALID, "rt_assemble_tiles: the deal must cover every tile once");
    uint64_t h = fnv1a(deal_off, sizeof(uint32_t) * (nshards + 1u), fnv1a(deal_tiles, sizeof(uint32_t) * ntiles));
    if (!r->d_where.p || h != r->where_hash) {
        std::vector<uint32_t> where(ntiles, 0xffffffffu);
        for (uint32_t k = 0; k < nshards; ++k) {
            if (deal_off[k + 1] < deal_off[k] || (size_t)(deal_off[k + 1] - deal_off[k]) * 64u > stride_px)
                return fail(RT_ERR_INVALID, "rt_assemble_tiles: a shard's tiles exceed the stride");
            for (uint32_t i = deal_off[k]; i < deal_off[k + 1]; ++i) {
                const uint32_t t = deal_tiles[i];
                if (t >= ntiles || where[t] != 0xffffffffu) return fail(RT_ERR_INVALID, "rt_assemble_tiles: tile out of range or repeated");
                where[t] = (k << 24) | (i - deal_off[k]);
            }
        }
        HIP_TRY(hipDeviceSynchronize());   // an assembly may still read the previous map
        if (int rc = r->d_where.grow(sizeof(uint32_t) * ntiles); rc != RT_OK) return rc;
        HIP_TRY(hipMemcpy(r->d_where.p, where.data(), sizeof(uint32_t) * ntiles, hipMemcpyHostToDevice));
        r->where_hash = h;
    }
    launch_assemble(gathered, stride_px, nshards, r->d_where.as<uint32_t>(), tiles_x, ntiles, r->W, r->H, rgb8, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return RT_OK;
}

int rt_renderer_counters(rt_renderer *r, rt_counters *out) {
    if (!r || !out) return fail(RT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(r->scene->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> c((size_t)kCounterSlots * 8);
    HIP_TRY(hipMemcpy(c.data(), r->d_counters, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    out->primary = r->primary;
    out->shadow = 0;
    out->bounce = 0;
    for (uint32_t k = 0; k < kCounterSlots; ++k) {
        out->shadow += c[(size_t)k * 8];
        out->bounce += c[(size_t)k * 8 + 1];
    }
    out->frames = r->frames;
    return RT_OK;
}

int rt_renderer_set_walk_check(rt_renderer *r, int level) {
    if (!r || level < RT_WALK_CHECK_OFF || level > RT_WALK_CHECK_VERIFY)
        return fail(RT_ERR_INVALID, "rt_renderer_set_walk_check: bad argument");
    r->walk_check = level;
    return RT_OK;
}

int rt_renderer_walk_stats(rt_renderer *r, uint64_t out[4]) {
    if (!r || !out) return fail(RT_ERR_INVALID, "rt_renderer_walk_stats: null argument");
    HIP_TRY(hipSetDevice(r->scene->device));
    HIP_TRY(hipDeviceSynchronize());
    std::vector<unsigned long long> c((size_t)kCounterSlots * 8);
    HIP_TRY(hipMemcpy(c.data(), r->d_counters, c.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int i = 0; i < 4; ++i) out[i] = 0;
    for (uint32_t k = 0; k < kCounterSlots; ++k) {
        out[0] += c[(size_t)k * 8 + 4];   // camera rays walked
        out[1] += c[(size_t)k * 8 + 2];   // boxes entered through the margin
        out[2] += c[(size_t)k * 8 + 3];   // lanes re-traced (tie / odd)
        out[3] += c[(size_t)k * 8 + 5];   // verify: walk result differed
    }
    return RT_OK;
}

int rt_renderer_overlap(const rt_renderer *r, int *state, float ms[4]) {
    if (!r || !state) return fail(RT_ERR_INVALID, "rt_renderer_overlap: null argument");
    int depth = 0;
    float all[8];
    rt_renderer_overlap_depth(r, &depth, all);
    *state = depth < 0 ? -1 : (depth > 1 ? 1 : 0);
    if (ms) {   // serial, 2 in flight, 2 in flight, serial
        const int n = r->ps_tg.groups == 8 ? 8 : 4;
        const int g[4] = {0, 1, n - 2, n - 1};
        for (int k = 0; k < 4; ++k) ms[k] = all[g[k]];
    }
    return RT_OK;
}

int rt_renderer_choices(const rt_renderer *r, int *walk, int *split, float walk_ms[4], float split_ms[4]) {
    if (!r || !walk || !split) return fail(RT_ERR_INVALID, "rt_renderer_choices: null argument");
    const rt_scene *s = r->scene;
    const bool split_set = r->order_state == 2 && !r->split_tg.active();
    *walk = s->walk == RT_WALK_WAVE ? 1 : s->walk == RT_WALK_LANE ? 0 : r->wave;
    *split = split_set ? (r->use_split ? 1 : 0) : -1;
    for (int g = 0; g < 4; ++g) {
        if (walk_ms) walk_ms[g] = (r->wave >= 0 && s->walk == RT_WALK_AUTO) ? r->walk_ms[g] : 0.0f;
        if (split_ms) split_ms[g] = split_set ? r->split_ms[g] : 0.0f;
    }
    return RT_OK;
}

int rt_renderer_overlap_depth(const rt_renderer *r, int *depth, float ms[8]) {
    if (!r || !depth) return fail(RT_ERR_INVALID, "rt_renderer_overlap_depth: null argument");
    const int32_t mode = r->scene->ps_pipeline;
    const bool decided = mode < 0 && r->ps_use >= 0;
    if (mode == 0) *depth = 1;
    else if (mode == 1) *depth = (int)r->scene->ps_depth;
    else *depth = decided ? (r->ps_use ? r->ps_use : 1) : -1;
    if (ms)
        for (int g = 0; g < 8; ++g) ms[g] = (decided && g < r->ps_tg.groups) ? r->ps_ms[g] : 0.0f;
    return RT_OK;
}

int rt_renderer_device_bytes(const rt_renderer *r, uint64_t *bytes, uint32_t *ps_buffers) {
    if (!r || !bytes) return fail(RT_ERR_INVALID, "rt_renderer_device_bytes: null argument");
    // what is allocated: the fixed blocks (accumulator, counters; the staging frame and the running
    // sample sum once a call needed them) and every growable buffer
    const uint64_t pix = (uint64_t)r->W * r->H;
    uint64_t b = 16u * pix + kCounterSlots * 8u * sizeof(unsigned long long);
    if (r->d_rgb) b += 4u * pix;
    if (r->d_sum) b += sum_bytes(r);
    each_buffer(*r, [&](const DevBuf &x) { b += x.bytes; });
    uint32_t nps = 0;
    for (const DevBuf &x : r->ps_res.buf) nps += x.p != nullptr;
    *bytes = b;
    if (ps_buffers) *ps_buffers = nps;
    return RT_OK;
}

int rt_renderer_tile_work(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t *work, uint32_t n,
                          uint32_t *pixel_work_dev, void *stream) {
    if (!r || !cam || !p || (n && !work)) return fail(RT_ERR_INVALID, "rt_renderer_tile_work: null argument");
    if (n < r->grid().ntiles) return fail(RT_ERR_INVALID, "rt_renderer_tile_work: room for every tile needed");
    std::vector<uint32_t> w;
    int rc = work_frame(r, cam, p, 0, 1, nullptr, 0, w, pixel_work_dev, (hipStream_t)stream);
    if (rc != RT_OK) return rc;
    std::memcpy(work, w.data(), sizeof(uint32_t) * w.size());
    return RT_OK;
}

int rt_renderer_tile_costs(const rt_renderer *r, uint32_t *costs, uint32_t n, uint32_t *n_out) {
    if (!r || !n_out || (n && !costs)) return fail(RT_ERR_INVALID, "rt_renderer_tile_costs: null argument");
    *n_out = (uint32_t)r->host_cost.size();
    if (n && !r->host_cost.empty()) std::memcpy(costs, r->host_cost.data(), sizeof(uint32_t) * std::min<size_t>(n, r->host_cost.size()));
    return RT_OK;
}

int rt_renderer_read_accumulator(rt_renderer *r, float *host) {
    if (!r || !host) return fail(RT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(r->scene->device));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(host, r->d_acc, sizeof(float4) * (size_t)r->W * r->H, hipMemcpyDeviceToHost));
    return RT_OK;
}

const char *rt_frame_kernel_name(const rt_renderer *r, const rt_frame_params *p) {
    if (r && p && p->mode == RT_MODE_BVH_HEAT) return "k_render_heat";   // its depth is the tree's
    if (!r || !p || p->mode > RT_MODE_PACKET || p->depth > 32) {
        fail(RT_ERR_INVALID, "rt_frame_kernel_name: bad argument");
        return nullptr;
    }
    const rt_scene *s = r->scene;
    if (p->mode == RT_MODE_PATH && p->depth >= 2 && s->pt_wavefront) return "k_pt_level";
    // the class launch_render's frame_variant starts from; the name does not depend on the build
    return frame_variant_name(kernel_class((int)p->mode, p->depth, !s->view.sky_const));
}

int rt_renderer_stream(rt_renderer *r, void **stream) {
    if (!r || !stream) return fail(RT_ERR_INVALID, "null argument");
    *stream = (void *)r->stream;
    return RT_OK;
}

int rt_synchronize(rt_renderer *r) {
    if (!r) return fail(RT_ERR_INVALID, "null argument");
    HIP_TRY(hipSetDevice(r->scene->device));
    HIP_TRY(hipDeviceSynchronize());
    return RT_OK;
}

}  // extern "C"
