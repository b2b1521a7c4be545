/*
 * rt_amd.h -- C-ABI of the MI355X-native ray-tracing hot path (librtamd.so).
 *
 * Drop-in boundary for the reference's Renderer::Tick / Renderer::Trace /
 * Scene::IntersectBVH / Scene::IsOccluded path (pmichels19/AdvancedGraphicsRayTracer).
 * The reference has no FFI of its own: its "boundary" is the in-process C++ class
 * surface cited on each entry point below.  A C++ host binds these functions
 * directly (see include/rt_compat.hpp); Python binds them with ctypes
 * (advancedgraphicsraytracer_amd/__init__.py).
 *
 * Conventions
 *   - every entry point is extern "C", returns int status (RT_OK = 0, < 0 error),
 *     and never throws; rt_last_error() returns a thread-local message;
 *   - scene/renderer handles are opaque; the library owns all device buffers it
 *     allocates; pointers named *_dev are caller-owned DEVICE memory, the rest are
 *     caller-owned host memory;
 *   - stream arguments are hipStream_t passed as void*; NULL is HIP's default (null)
 *     stream, as everywhere in HIP.  Handles create and finish their own setup work
 *     before returning; the *_host conveniences run on the handle's private stream
 *     and synchronize it;
 *   - primitive ids follow creation order exactly as the reference's
 *     Primitive::objIdx (Primitive.h:37-38); the light is primitive 0 and must be a
 *     sphere or a quad (Scene::GetRandomLight, template/scene.h:225-227).
 * No CPU fallback exists: without a usable gfx950 device every compute entry
 * point fails with RT_ERR_NO_DEVICE.
 */
#ifndef RT_AMD_H
#define RT_AMD_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 4

enum {
    RT_OK = 0,
    RT_ERR_INVALID = -1,    /* bad argument */
    RT_ERR_NO_DEVICE = -2,  /* no HIP device / kernel image not loadable */
    RT_ERR_HIP = -3,        /* HIP runtime error */
    RT_ERR_IO = -4,         /* file not found / parse error */
    RT_ERR_UNSUPPORTED = -5, /* scene outside the kernels' limits */
    RT_ERR_COMM = -6        /* RCCL missing or a collective failed */
};

/* Primitive kinds, Primitive.h:8-14. */
enum { RT_SPHERE = 0, RT_PLANE = 1, RT_CUBE = 2, RT_QUAD = 3, RT_TRIANGLE = 4 };
/* Materials: Diffuse.h, Mirror.h, Dielectric.h, Checkerboard.h, Light.h, DSMix.h,
 * TextureMaterial.h. */
enum { RT_DIFFUSE = 0, RT_MIRROR = 1, RT_DIELECTRIC = 2, RT_CHECKERBOARD = 3, RT_LIGHT = 4, RT_DSMIX = 5,
       RT_TEXTURE = 6 };
/* Integrators behind Renderer::Tick (renderer.cpp:227-231; the K key toggles them,
 * renderer.h:138): Trace (path tracer, default depth 10, renderer.h:9), WhittedTrace
 * (default depth 20, renderer.h:13), and the PACKET_TRAVERSAL build of Tick
 * (renderer.cpp:247-285): 8x8 tiles as 64-ray packets through IntersectBVHPacket, shaded
 * by TracePacket whose bounces are Trace(.., depth) -- depth 10 in the reference, 0 allowed.
 * depth <= 32 for all three.
 * RT_MODE_BVH_HEAT: the BVH_ANALYSIS build of Tick (renderer.cpp:224-226) -- every sample is
 * Scene::BVHVisualization (template/scene.h:244-283) of its camera ray instead of Trace: red =
 * leaves reached / tree depth, green = 0.25 * nodes visited / tree depth, blue = 0, through the same
 * accumulator and RGB8 pack.  rt_frame_params.depth is ignored; no shadow or bounce ray is counted.
 * Frames only (rt_render_frame, _host, rt_render_shard, rt_render_shard_tiles); rt_render_frame_multi
 * refuses it with RT_ERR_UNSUPPORTED. */
enum { RT_MODE_PATH = 0, RT_MODE_WHITTED = 1, RT_MODE_PACKET = 2, RT_MODE_BVH_HEAT = 3 };

/* One primitive, Primitive::create* factories (Primitive.h:690-747):
 *   RT_SPHERE:   v[0..2] centre, v[3] radius
 *   RT_PLANE:    v[0..2] normal, v[3] distance
 *   RT_CUBE:     v[0..2] position, v[3..5] size; createCube(pos, size, material, T)
 *   RT_QUAD:     v[0] size; createQuad(size, material, T)
 *   RT_TRIANGLE: v[0..8] three world-space vertices (post Scene::LoadModel)
 * T (cube / quad only) comes from rt_scene_desc.transforms. */
typedef struct { int32_t type; int32_t material; float v[9]; } rt_prim;

/* One material.  color = Diffuse/Mirror/Light/DSMix colour or Dielectric absorption;
 * color2 = Checkerboard second colour; ior = Dielectric n; diffuse = the diffuse share
 * of Checkerboard / DSMix / TextureMaterial (clamped to [0, 1]; < 0 selects the short
 * Checkerboard / TextureMaterial constructor: diffuse 1, specular 0); texture = index
 * into rt_scene_desc.textures (RT_TEXTURE only). */
typedef struct {
    int32_t kind; float color[3]; float color2[3]; float ior; float diffuse; int32_t texture;
} rt_material;

/* A Surface (template/template.cpp:1571-1601): 0x00RRGGBB texels, row-major.
 * TextureMaterial indexes it as (u & (width-1)) + (v & (height-1)) * width. */
typedef struct { const uint32_t *pixels; uint32_t width, height; } rt_texture;

/* Scene description, the inputs of Scene::Scene (template/scene.h:40-128). */
typedef struct {
    const rt_prim *prims; uint32_t num_prims;
    const rt_material *materials; uint32_t num_materials;
    /* sky: power-of-two texture of 0x00RRGGBB (renderer.h:15-22); NULL = the
     * synthetic 1024x512 constant 0x406080 sky of SURVEY.md 8(d) */
    const uint32_t *sky_pixels; uint32_t sky_width, sky_height;
    /* optional prebuilt plain BVH: nodes in the 32-byte BVHNode layout
     * (BVHNode.h:5-14, root 0, node 1 unused) + primitiveIndices; NULL = build
     * here with the reference's binned SAH (template/scene.h:845-976) */
    const void *bvh_nodes; uint32_t bvh_num_nodes; const uint32_t *bvh_indices;
    int32_t device;
    /* per-primitive mat4 T (16 floats, row-major as rt_mat4_*), read for RT_CUBE and
     * RT_QUAD only; NULL = identity for all (the factories' default argument) */
    const float *transforms;
    const rt_texture *textures; uint32_t num_textures;
    /* RT_BVH_PLAIN (0): the reference's plain binned-SAH BVH (template/scene.h:845-976), the
     * parity tree; RT_BVH_SBVH: spatial splits (template/scene.h:521-840, built NaN-safe with a
     * growing pool) -- closest hits equal the plain tree's except exact-distance ties.
     * Ignored with a prebuilt BVH. */
    int32_t bvh_kind;
} rt_scene_desc;
enum { RT_BVH_PLAIN = 0, RT_BVH_SBVH = 1 };

/* num_refs = entries of the BVH's primitive-index array (= num_prims for the plain tree;
 * more for an SBVH, whose leaves may share primitives) */
typedef struct { uint32_t num_prims, nodes_used, depth, max_leaf, num_refs; } rt_scene_info;

/* Ray / hit records of the batched entry points (Ray.h:7-32). */
typedef struct { float ox, oy, oz, dx, dy, dz, tmax; } rt_ray;       /* 28 B */
typedef struct { float t; int32_t obj; float u, v; } rt_hit;           /* 16 B */

/* Camera state (camera.h:93-100): origin, virtual screen corners, lens radius. */
typedef struct { float pos[3], top_left[3], top_right[3], bottom_left[3]; float lens_radius; } rt_camera;

/* One frame.  spp samples per pixel per frame; depth = Trace depth (renderer.h:9
 * default 10; depth 1 = primary + NEE shadow ray); frame feeds the per-pixel seed
 * InitSeed(pixel + W*H*(sample + spp*frame)) (template/template.cpp:683-686);
 * reset = clear the accumulator first (renderer.cpp:237). */
typedef struct { uint32_t width, height, spp, depth, frame, mode, reset; } rt_frame_params;

/* Cumulative ray counters of a renderer. */
typedef struct { uint64_t primary, shadow, bounce, frames; } rt_counters;

typedef struct rt_scene rt_scene;
typedef struct rt_renderer rt_renderer;

/* ---- library ---------------------------------------------------------- */
int rt_abi_version(void);
const char *rt_last_error(void);
int rt_device_count(int *count);
void rt_free(void *p);

/* ---- host-side scene preparation (Scene::LoadModel, template/scene.h:156-201) ---- */
/* tinyobj-compatible OBJ read (template/tiny_obj_loader.h, triangulate=true):
 * vertices float[3*nv], faces int32[3*nt] in file order; free with rt_free. */
int rt_obj_load(const char *path, float **verts, uint32_t *nv, int32_t **faces, uint32_t *nt);
/* RTMESH1 container (parsed OBJ vertices + faces) used for the bundled scenes. */
int rt_mesh_load(const char *path, float **verts, uint32_t *nv, int32_t **faces, uint32_t *nt);
int rt_mesh_save(const char *path, const float *verts, uint32_t nv, const int32_t *faces, uint32_t nt);
/* mat4 helpers, template/precomp.h:1007-1039 and template/template.cpp:779-792 */
int rt_mat4_translate(float x, float y, float z, float out[16]);
int rt_mat4_scale(float s, float out[16]);
int rt_mat4_rotate(int axis, float angle, float out[16]);
int rt_mat4_mul(const float a[16], const float b[16], float out[16]);
/* append one triangle per face, vertices = TransformPosition(v, M)
 * (template/scene.h:185-191); out holds nt rt_prim records */
int rt_mesh_to_prims(const float *verts, uint32_t nv, const int32_t *faces, uint32_t nt,
                     const float M[16], int32_t material, rt_prim *out);
/* The SURVEY.md 8(d) scene recipes as descriptions: call once with prims == NULL to get
 * the counts, then with arrays of that size. */
int rt_recipe_describe(const char *name, const char *mesh_dir, rt_prim *prims, uint32_t *num_prims,
                       rt_material *materials, uint32_t *num_materials);
/* plain-BVH build only (no device): nodes (2N+2 x 32 B) and indices (N);
 * transforms as in rt_scene_desc (NULL = identity) */
int rt_bvh_build_host(const rt_prim *prims, const float *transforms, uint32_t n, void *nodes, uint32_t *indices,
                      rt_scene_info *info);
/* The refit of rt_scene_update_triangles on the host, no device: the boxes of nodes (nodes_used x 32 B,
 * the topology rt_bvh_build_host or a caller made) rewritten in place for prims[n] -- a leaf's box is
 * the min / max over its primitives' boxes (Scene::UpdateNodeBounds, template/scene.h:855-865), an
 * interior node's the union of its children's; leftFirst / count untouched.  With the primitives the
 * tree was built from it returns rt_bvh_build_host's bytes.  A plain tree only (every primitive in
 * exactly one leaf): RT_ERR_UNSUPPORTED for an SBVH's index array; the nodes are untouched on error. */
int rt_bvh_refit_host(const rt_prim *prims, const float *transforms, uint32_t n, void *nodes, uint32_t nodes_used,
                      const uint32_t *indices);
/* Tree cost, the per-node SAH term of calculateNodeCost (template/scene.h:203-207) summed over a tree.
 * Over every node index in [0, nodes_used) except 1 (the reference's unused node), from the float32
 * bounds: ex = (double)max.x - (double)min.x (ey, ez alike), area = ex*ey + ey*ez + ez*ex, left to
 * right in double without contraction (a plane's +-1e30 box overflows float32).  An interior node adds
 * area to interior_area; a leaf adds area to leaf_area and (double)count * area to leaf_cost; refs =
 * the sum of the leaf counts, max_leaf the largest; root_area = node 0's area.  The order of the
 * double sums is free. */
typedef struct {
    double sah;            /* (interior_area + leaf_cost) / root_area; 0 when root_area == 0 */
    double interior_area, leaf_area, leaf_cost, root_area;
    uint32_t interiors, leaves, refs, max_leaf;
} rt_bvh_cost;
/* no device: the cost of a BVHNode array (rt_bvh_build_host's, rt_scene_copy_bvh's) */
int rt_bvh_cost_host(const void *nodes, uint32_t nodes_used, rt_bvh_cost *out);
/* no device: the refit schedule of a plain tree (nodes_used x 32 B BVHNode, n primitive indices), the
 * definition rt_scene_copy_update_plan's arrays equal word for word.  list: node indices, treelet after
 * treelet (whole subtrees of at most 256 nodes, in pre-order of their roots), each sorted by height
 * above its deepest leaf, then the nodes above the cut, sorted the same way; lvl: per group the start
 * of each height in list and the group's end; grp: per group its first entry in lvl, the nodes above
 * the cut being group ntreelets, and one closing entry.  Library-allocated, free each with rt_free.
 * counts = list length, lvl length, ntreelets, has_top.  RT_ERR_UNSUPPORTED: a primitive in no leaf
 * slot or in two, or a node array that does not walk. */
int rt_bvh_refit_plan_host(const void *nodes, uint32_t nodes_used, const uint32_t *indices, uint32_t n,
                           uint32_t **list, uint32_t **lvl, uint32_t **grp, uint32_t counts[4]);
/* the opt-in spatial-split BVH (RT_BVH_SBVH) on the host: library-allocated nodes
 * (info->nodes_used x 32 B) and primitive-index array (info->num_refs; primitives may
 * repeat); free both with rt_free */
int rt_sbvh_build_host(const rt_prim *prims, const float *transforms, uint32_t n, void **nodes, uint32_t **indices,
                       rt_scene_info *info);
/* Surface::LoadImage (template/template.cpp:1579-1601) for PNG files (8/16-bit grey,
 * grey+alpha, RGB, RGBA, palette; not interlaced): pixels = 0x00RRGGBB; free with rt_free. */
int rt_image_load(const char *path, uint32_t **pixels, uint32_t *width, uint32_t *height);

/* ---- scene (Scene, template/scene.h:37-1014) ------------------------------ */
int rt_scene_create(const rt_scene_desc *desc, rt_scene **out);
/* the SURVEY.md 8(d) scenes: "teapotF", "teapot", "mig16", "cfg3", "cfg5"; and "default", the
 * reference's as-shipped Scene() (template/scene.h:40-128: light, glider, mig29 -- the other
 * models it names are not in its assets/).  mesh_dir holds <name>.rtmesh or the reference's
 * <name>.obj files. */
int rt_scene_create_recipe(const char *name, const char *mesh_dir, int32_t device, rt_scene **out);
/* the same with the BVH kind chosen (RT_BVH_PLAIN / RT_BVH_SBVH) */
int rt_scene_create_recipe_ex(const char *name, const char *mesh_dir, int32_t device, int32_t bvh_kind, rt_scene **out);
int rt_scene_destroy(rt_scene *s);
int rt_scene_get_info(const rt_scene *s, rt_scene_info *info);
/* How the primary+shadow frame kernel walks the BVH for camera rays (results identical):
 * RT_WALK_LANE -- one traversal per lane, the reference's order;
 * RT_WALK_WAVE -- the wave's 64 rays (an 8x8 tile) walk the union of their subtrees with
 *   a wave-uniform node and stack; lanes whose closest hit could depend on the visiting
 *   order (an exact distance tie, or a hit nearer than its leaf box's entry) are re-traced
 *   in the reference order.  Faster where rays share most of their walk (mig29 x16: 1.9x);
 *   slower where they split early (CFG3-sub);
 * RT_WALK_AUTO (default; LANE for scenes with cubes) -- each renderer times one frame of
 *   each after a warm-up frame and keeps the faster.
 * Only scenes whose nodes are not held in LDS use it.  RT_WAVE_PRIMARY=0/1 in the
 * environment forces LANE / WAVE at scene creation. */
enum { RT_WALK_LANE = 0, RT_WALK_WAVE = 1, RT_WALK_AUTO = 2 };
int rt_scene_set_camera_walk(rt_scene *s, int walk);
/* host copy of the BVH in use (nodes_used x 32 B, num_refs x u32), in the reference's node order;
 * after an in-place update the first call downloads the refitted boxes, after rt_scene_rebuild the
 * new nodes and indices */
int rt_scene_copy_bvh(const rt_scene *s, void *nodes, uint32_t *indices);
/* Animated geometry (the reference's "optionally animated" scene: Scene::SetTime, template/scene.h:213-224,
 * and Tick's animation branch, renderer.cpp:206-237).  Replace the vertices of triangle primitives
 * [first, first + count) and refit the BVH in place: topology, primitive ids, materials and leaf
 * membership are unchanged; the triangles' device records become those of a fresh rt_scene_create on
 * the new vertices, every node box the exact union of what lies below it (min / max of floats: no
 * rounding), and the wave walk's sticky boxes are recomputed.  verts_dev: DEVICE float[9 * count],
 * world-space A, B, C per triangle as rt_prim.v.  Blocks: it first waits for all outstanding work on
 * the scene's device (renderers run frames on their own streams), runs on `stream`, and returns when
 * the scene is ready for any stream.  The caller renders the next frame with reset = 1, as the
 * reference does (renderer.cpp:237).  Renderers keep their timed choices, tile orders and deals
 * (speed only; tests/test_edits_under_schedule_gpu.py holds the frames of a warm renderer after every
 * kind of edit to those of one without any such state), and the scene keeps its camera-walk policy.
 * The first update of a scene builds its refit schedule on the GPU, unless rt_scene_prepare_updates
 * did so at a moment of the caller's choosing.
 *   RT_ERR_INVALID      null pointer, range outside the primitives, a non-triangle primitive in the
 *                       range, or a NaN / infinite vertex -- the scene is untouched (the vertices are
 *                       checked in a pass of their own before anything is written);
 *   RT_ERR_UNSUPPORTED  an SBVH scene (num_refs != num_prims), or one built with RT_PT_QUADS=1.
 * count == 0 is RT_OK and does nothing.  Other kinds and the light move with rt_scene_update_prims,
 * whole meshes by matrix with rt_scene_transform_triangles; the topology changes with rt_scene_rebuild,
 * the number of triangles with rt_scene_splice_triangles. */
int rt_scene_update_triangles(rt_scene *s, uint32_t first, uint32_t count, const float *verts_dev, void *stream);
/* the same with the vertices in host memory (staged on the scene's private stream) */
int rt_scene_update_triangles_host(rt_scene *s, uint32_t first, uint32_t count, const float *verts);
/* Primitives of any kind in place (Primitive::UpdateTransform, Primitive.h:56-59; Scene::SetTime's bouncing
 * sphere, spinning cube and swinging quad light): new records for primitives [first, first + count),
 * triangles included, under the contract of rt_scene_update_triangles -- afterwards the scene is bit for
 * bit a fresh rt_scene_create of the new description over the same tree topology (leaf-slot records,
 * shading records, the cubes' and quads' side table, every node box, the sticky boxes), it blocks the
 * same way, and the next frame is rendered with reset = 1.  prims_dev: DEVICE rt_prim[count];
 * transforms_dev: DEVICE float[16 * count], one mat4 per record as rt_scene_desc.transforms (read for
 * RT_CUBE and RT_QUAD only), or NULL = identity for all.  A record's type and material must be the
 * scene's for that id.  If the range holds primitive 0, the light the renderers sample moves with it.
 *   RT_ERR_INVALID      null pointer, range outside the primitives, a record whose type or material
 *                       differs from the scene's, a NaN / infinite field that its kind reads, transform
 *                       (where one is read) or resulting box -- checked in a pass of its own before
 *                       anything is written: the scene is untouched;
 *   RT_ERR_UNSUPPORTED  an SBVH scene, or one built with RT_PT_QUADS=1.
 * count == 0 is RT_OK and does nothing. */
int rt_scene_update_prims(rt_scene *s, uint32_t first, uint32_t count, const rt_prim *prims_dev,
                          const float *transforms_dev, void *stream);
/* the same with records and transforms (may be NULL) in host memory */
int rt_scene_update_prims_host(rt_scene *s, uint32_t first, uint32_t count, const rt_prim *prims, const float *transforms);
/* Whole meshes moved rigidly (or by any affine mat4), many in one call: triangle primitives
 * [first, first + count) of each range take the world vertices TransformPosition(rest, M) -- the one
 * operation Scene::LoadModel places a mesh with (template/scene.h:185-191), exactly as
 * rt_mesh_to_prims computes it -- and everything after that is rt_scene_update_triangles: one finite
 * check over the transformed vertices, one update launch, one refit.  ranges: HOST, in any order;
 * rest_dev: DEVICE object-space A, B, C, 9 floats per triangle, the ranges' triangles back to back in the
 * order of `ranges`.
 *   RT_ERR_INVALID      null pointer, a range outside the primitives or over a non-triangle, ranges that
 *                       overlap (checked on the host), or a transformed vertex that is NaN or infinite --
 *                       the scene is untouched;
 *   RT_ERR_UNSUPPORTED  as above.
 * Ranges of count 0 are skipped; no range at all is RT_OK and does nothing. */
typedef struct { uint32_t first, count; float M[16]; } rt_tri_xform;
int rt_scene_transform_triangles(rt_scene *s, const rt_tri_xform *ranges, uint32_t num_ranges, const float *rest_dev,
                                 void *stream);
/* Stream-ordered forms of the three in-place updates: the same records written, the same refit, the
 * same "untouched on refusal" contract, but no host wait.  The call enqueues on `stream` and returns;
 * a host that animates every frame runs ahead of the GPU across updates and frames as it does across
 * frames.  *ticket (may be NULL) receives the update's number, 1, 2, ... per scene.
 * Refused at once, with the blocking call's code and without consuming a ticket: everything the
 * blocking call checks on the host (null pointers, ranges, non-triangles, overlapping ranges, SBVH or
 * RT_PT_QUADS=1 scenes); count == 0 / no range is RT_OK.  rt_scene_update_prims_async over a range
 * that holds primitive 0 is RT_ERR_UNSUPPORTED: the light's fields are computed on the host from its
 * record, so the light moves through the blocking call.
 * Refused on the device: the finiteness / admissibility check still runs as a pass of its own before
 * anything is written, but its flag is read by the kernels that follow, not by the host -- a flagged
 * update's write and refit launches store nothing (node bytes of a caller's loose prebuilt tree stay
 * as they were), and the outcome shows at rt_scene_update_sync.  Later updates in the queue do not
 * depend on an earlier refusal.
 * Ordering the library provides:
 *   1. the update runs after everything enqueued on `stream` before it, frames of any renderer
 *      submitted on that stream included (their kernels on renderer streams are joined into the
 *      submitting stream by the frame's finishing pass);
 *   2. everything enqueued after it that reads the scene waits for it, on whatever stream: frames
 *      (on renderer streams and on caller streams), shards and multi-GPU frames, rt_intersect*,
 *      rt_occluded, rt_trace, rt_bvh_visualize, rt_renderer_tile_work, and a later async update on
 *      another stream.  A scene that never had an async update pays one host branch per launch;
 *   3. work enqueued EARLIER on other streams of the caller's is the caller's to order (plain HIP
 *      semantics): a frame submitted on stream B and not yet finished may see an update enqueued
 *      afterwards on stream A;
 *   4. every blocking scene entry point (the blocking updates and their _host forms,
 *      rt_scene_prepare_updates, rt_scene_rebuild, the splices and compactions,
 *      rt_scene_set_prim_materials, rt_scene_copy_bvh, rt_scene_bvh_cost, rt_scene_update_plan_info,
 *      rt_scene_copy_update_plan, rt_scene_destroy) first does what rt_scene_update_sync does, so
 *      the two styles mix safely.
 * Pointer lifetime: verts_dev, rest_dev, prims_dev and transforms_dev must stay valid and unchanged
 * until the update has executed in stream order; the host `ranges` array is consumed before the
 * call returns (it travels through a scene-owned ring of 8 pinned slots: the call waits for the
 * update that used its slot 8 calls ago, i.e. only while all 8 are in flight, and a table larger
 * than any before it reallocates its slot).
 * Host waits that remain: where no refit schedule is ready (the first update of a scene, the first
 * after a rebuild or a splice) the call builds it inside itself and blocks that once, like the
 * blocking update -- rt_scene_prepare_updates beforehand keeps it non-blocking -- and a scene's
 * first async call creates its status block.
 * The next frame is rendered with reset = 1.  The host-side flags behind the fast paths
 * (bounds_finite, the wave walk's nesting) stay as they are until rt_scene_update_sync; frames are
 * identical either way. */
int rt_scene_update_triangles_async(rt_scene *s, uint32_t first, uint32_t count, const float *verts_dev,
                                    void *stream, uint64_t *ticket);
int rt_scene_transform_triangles_async(rt_scene *s, const rt_tri_xform *ranges, uint32_t num_ranges,
                                       const float *rest_dev, void *stream, uint64_t *ticket);
int rt_scene_update_prims_async(rt_scene *s, uint32_t first, uint32_t count, const rt_prim *prims_dev,
                                const float *transforms_dev, void *stream, uint64_t *ticket);
/* submitted: tickets handed out; applied, refused: updates that ran since the scene was created;
 * first_refused: ticket of the earliest refusal since the previous rt_scene_update_sync, 0 for none */
typedef struct { uint64_t submitted, applied, refused, first_refused; } rt_update_status;
/* Waits for every enqueued async update (not for frames), folds their outcomes into the scene's host
 * state and fills *out (may be NULL).  RT_OK also where an update was refused: first_refused says
 * so, and rt_last_error() then names that refusal.
 *   RT_ERR_INVALID      null scene. */
int rt_scene_update_sync(rt_scene *s, rt_update_status *out);
/* Rebuild the scene's plain BVH on the GPU from its CURRENT primitives (after any number of
 * in-place updates): afterwards the scene is bit for bit a fresh rt_scene_create of the current
 * description -- node array, primitive-index array, leaf-slot records in the new slot order,
 * sticky words, root word, stack depth, walk eligibility, bounds_finite -- i.e. the tree
 * rt_bvh_build_host returns for those primitives.  Blocks like the update calls (waits for the
 * scene's device, runs on `stream`, returns when the scene is ready for any stream).  The caller
 * renders the next frame with reset = 1 (exact-distance ties may resolve differently on a new tree).
 *   RT_ERR_UNSUPPORTED  an SBVH or RT_PT_QUADS=1 scene; a scene created with a NaN or infinite
 *                       primitive box; or the new tree breaks a kernel limit (leaf > 255,
 *                       depth > 64, > 2^24 nodes) -- the scene is untouched;
 *   RT_ERR_INVALID      null scene.
 * Renderers keep their timed choices and tile orders; the scene keeps its camera-walk policy where
 * the new tree still admits it.  The next in-place update rebuilds its refit schedule (or
 * rt_scene_prepare_updates, before it). */
int rt_scene_rebuild(rt_scene *s, void *stream);
/* diagnostics of the last rebuild: out[0] tree levels processed, out[1] nodes split by the
 * many-workgroup path, out[2] subtrees finished by the one-workgroup path, out[3] kernel launches */
int rt_scene_rebuild_stats(const rt_scene *s, uint32_t out[4]);
/* Put what the in-place updates need on the device NOW: the update state (slot map, slot boxes,
 * centroids) and the refit schedule of the current topology, built on the GPU from the device node
 * array.  Without this call the first rt_scene_update_* / rt_scene_transform_triangles after
 * creation, after rt_scene_rebuild and after rt_scene_splice_triangles does the same work inside
 * itself; with it that update costs what a later one costs.  Blocks like an update (waits for the
 * scene's device, runs on `stream`).  Idempotent: on an unchanged topology a second call launches
 * nothing.  Frames are unaffected.
 *   RT_ERR_UNSUPPORTED  where an update would return it (an SBVH or RT_PT_QUADS=1 scene) -- the
 *                       scene is untouched;
 *   RT_ERR_INVALID      null scene. */
int rt_scene_prepare_updates(rt_scene *s, void *stream);
/* the schedule on the device: out[0] ready (0 / 1), out[1] where it was built (0 none, 1 host,
 * 2 GPU in many launches, 3 GPU in one workgroup), out[2] ntreelets, out[3] has_top, out[4] list
 * length, out[5] lvl length, out[6] nodes above the cut, out[7] kernel launches of the call that last
 * asked for it (0 where it stood ready).  All 0 while none is ready (a rebuild or a splice drops it). */
int rt_scene_update_plan_info(const rt_scene *s, uint32_t out[8]);
/* download the schedule (rt_bvh_refit_plan_host's arrays: out[4] / out[5] / out[2] + 2 words); a
 * null pointer skips that array.  RT_ERR_INVALID when no schedule is ready. */
int rt_scene_copy_update_plan(const rt_scene *s, uint32_t *list, uint32_t *lvl, uint32_t *grp);
/* Add and remove triangles in a live scene.  Remove triangle primitives [first, first + remove) and
 * insert `insert` new triangles at id `first`; primitives behind the edit shift by insert - remove.
 * prims_dev: DEVICE rt_prim[insert] (type RT_TRIANGLE, v[0..8] world-space A, B, C, material an index
 * of the scene's materials).  first == num_prims appends.  Afterwards the scene is bit for bit a fresh
 * rt_scene_create of the spliced description -- the old primitive list with the range erased and the
 * new records inserted at `first`; materials, textures, sky and transforms as they were -- in
 * everything the kernels read: node array, primitive-index array, leaf-slot records in the new slot
 * order with the NEW ids in them, shading records per new id, sticky words, root word, stack depth,
 * walk eligibility, bounds_finite, and rt_scene_get_info.  The tree is the one rt_bvh_build_host
 * returns for the spliced list (also where the scene was created with a prebuilt BVH).  Blocks like
 * the update calls (waits for the scene's device, runs on `stream`, returns when the scene is ready
 * for any stream); the caller renders the next frame with reset = 1.  Renderers stay valid and keep
 * their accumulator buffers, tile orders and timed choices; the scene keeps its camera-walk policy
 * where the new tree admits it.  The next in-place update rebuilds its refit schedule.
 * Ids the caller holds for later rt_scene_update_triangles, rt_scene_transform_triangles or
 * rt_scene_update_prims calls shift with the edit: every id >= first + remove moves by
 * insert - remove.  That bookkeeping is the caller's.
 * Only triangles enter and leave through this call (primitives of other kinds may sit anywhere, also
 * behind the edit); every kind does through rt_scene_splice_prims below.
 *   RT_ERR_INVALID      null scene, or null records with insert > 0; first == 0 (primitive 0 is the
 *                       light and stays); first + remove > num_prims; a non-triangle in the removed
 *                       range; an inserted record that is no RT_TRIANGLE, whose material is outside
 *                       [0, num_materials), or with a NaN / infinite vertex (checked in a pass of its
 *                       own before anything is written);
 *   RT_ERR_UNSUPPORTED  an SBVH or RT_PT_QUADS=1 scene; a scene created with a NaN or infinite
 *                       primitive box; 2^24 primitives or more; or the new tree breaks a kernel limit
 *                       (leaf > 255, depth > 64, > 2^24 nodes);
 *   RT_ERR_HIP          an allocation failed.
 * After every refusal the scene is untouched.  remove == 0 && insert == 0 is RT_OK and does nothing. */
int rt_scene_splice_triangles(rt_scene *s, uint32_t first, uint32_t remove, const rt_prim *prims_dev, uint32_t insert,
                              void *stream);
/* the same with the records in host memory (staged on the scene's private stream) */
int rt_scene_splice_triangles_host(rt_scene *s, uint32_t first, uint32_t remove, const rt_prim *prims, uint32_t insert);
/* Several such edits in ONE rebuild.  edits: HOST memory, in any order; every `first` is an id of the
 * OLD id space.  prims_dev: DEVICE rt_prim, the inserted records of all edits back to back in the
 * order of `edits` (not in sorted order).  The result is the old list with every range
 * [first, first + remove) erased and that edit's records put in its place -- what the edits give when
 * applied one at a time through rt_scene_splice_triangles in descending order of `first`.  Contract,
 * blocking and what stays valid are rt_scene_splice_triangles' word for word; the caller's ids behind
 * an edit shift by the sum of insert - remove of the edits before them.  Adjacent ranges
 * (first2 == first1 + remove1) are fine.  Edits with remove == 0 && insert == 0 are skipped (but still
 * refused for first == 0); with no edit left the call is RT_OK and launches nothing.  No limit on
 * num_edits but memory.
 *   RT_ERR_INVALID      checked on the host before any HIP call: null scene, null edits with
 *                       num_edits > 0, null records with any insert > 0; per edit first == 0, a range
 *                       outside the primitives, a non-triangle in a removed range; two non-empty edits
 *                       with the same `first` (their order in the result would be ambiguous) or whose
 *                       removed ranges overlap.  Checked on the device in one pass over all records,
 *                       before anything is allocated or written: a record that is no RT_TRIANGLE,
 *                       a material outside [0, num_materials), a NaN / infinite vertex;
 *   RT_ERR_UNSUPPORTED, RT_ERR_HIP  as for rt_scene_splice_triangles.
 * After every refusal the scene is untouched. */
typedef struct { uint32_t first, remove, insert; } rt_tri_edit;
int rt_scene_splice_ranges(rt_scene *s, const rt_tri_edit *edits, uint32_t num_edits, const rt_prim *prims_dev, void *stream);
/* the same with the records in host memory (staged on the scene's private stream) */
int rt_scene_splice_ranges_host(rt_scene *s, const rt_tri_edit *edits, uint32_t num_edits, const rt_prim *prims);
/* Drop triangles by a keep-mask decided on the GPU, in one rebuild.  keep_dev: DEVICE memory,
 * num_prims bytes indexed by old id; primitive i stays where keep_dev[i] != 0.  Survivors keep their
 * relative order: the new id of a survivor is the number of survivors before it (an exclusive prefix
 * count on the GPU; the ranges never travel through the host).  Contract, blocking and what stays
 * valid are rt_scene_splice_triangles'.  The survivor count is read back; a mask that keeps everything
 * is RT_OK and does nothing further -- nothing is rebuilt, a ready refit schedule stays ready.
 *   RT_ERR_INVALID      null scene or mask; a mask that drops primitive 0 or any non-triangle
 *                       (checked on the GPU in a pass of its own before anything is written);
 *   RT_ERR_UNSUPPORTED, RT_ERR_HIP  as for rt_scene_splice_triangles.
 * After every refusal the scene is untouched.  Nothing enters through this call. */
int rt_scene_compact_triangles(rt_scene *s, const uint8_t *keep_dev, void *stream);
/* the same with the mask in host memory (staged on the scene's private stream) */
int rt_scene_compact_triangles_host(rt_scene *s, const uint8_t *keep);
/* Primitives of any kind enter and leave: rt_scene_splice_ranges with the kind restriction lifted.
 * Edits are in old ids and in any order; a single edit is num_edits == 1.  Removed ranges may hold any
 * kind; the inserted records, back to back in prims_dev in the order of `edits`, may be RT_SPHERE,
 * RT_PLANE, RT_CUBE, RT_QUAD or RT_TRIANGLE.  transforms_dev: DEVICE float[16 * total insert], one mat4
 * per inserted record, read for cubes and quads only; NULL = identity for all (rt_scene_update_prims'
 * convention).  A type change is remove = 1, insert = 1 at the same `first`.  Primitive 0, the light,
 * stays.
 * The contract is rt_scene_splice_triangles', extended: afterwards the scene is bit for bit a fresh
 * rt_scene_create of the edited description (materials, textures and sky as they were; per-primitive
 * transforms edited alongside the primitives) in everything the kernels read and the host can ask for --
 * nodes (sticky words included), the primitive-index array, leaf-slot records with the new ids and the
 * new side-table indices, shading records, the cubes' and quads' side table in its new rank order, slot
 * boxes, centroids, root word, stack depth, walk eligibility, and the kernel family: a scene that gains
 * its first cube or quad renders with the kernels such a scene needs, one that loses its last returns
 * to the core ones.  Where the new scene no longer admits the wave walk (a cube entered), the camera-
 * walk policy falls back to RT_WALK_LANE, as rt_scene_set_camera_walk would refuse RT_WALK_WAVE now; it
 * is not raised again when the cubes leave.  Blocks like an update; render the next frame with
 * reset = 1; renderers stay valid and keep their buffers; the next in-place update rebuilds its refit
 * schedule, and rt_scene_update_prims then addresses the new ids.
 *   RT_ERR_INVALID      checked on the host before any HIP call: null scene, null edits with
 *                       num_edits > 0, null records with any insert > 0; per edit first == 0, a range
 *                       outside the primitives; two non-empty edits with the same `first` or whose
 *                       removed ranges overlap.  Checked on the device in one pass over all records,
 *                       before anything of the scene is written: a type outside the five kinds, a
 *                       material outside [0, num_materials), a NaN / infinite field that the kind
 *                       reads, a NaN / infinite transform where one is read, a NaN / infinite box --
 *                       rt_scene_update_prims' rules without "same type and material as the scene";
 *   RT_ERR_UNSUPPORTED, RT_ERR_HIP  as for rt_scene_splice_triangles.
 * After every refusal the scene is untouched. */
typedef rt_tri_edit rt_prim_edit;   /* { uint32_t first, remove, insert; } */
int rt_scene_splice_prims(rt_scene *s, const rt_prim_edit *edits, uint32_t num_edits, const rt_prim *prims_dev,
                          const float *transforms_dev, void *stream);
/* the same with records and transforms in host memory (staged on the scene's private stream) */
int rt_scene_splice_prims_host(rt_scene *s, const rt_prim_edit *edits, uint32_t num_edits, const rt_prim *prims,
                               const float *transforms);
/* rt_scene_compact_triangles without the kind restriction: the mask may drop anything but primitive 0.
 * A mask that keeps everything still does nothing.  Contract as rt_scene_splice_prims. */
int rt_scene_compact_prims(rt_scene *s, const uint8_t *keep_dev, void *stream);
int rt_scene_compact_prims_host(rt_scene *s, const uint8_t *keep);
/* Materials change in place: the material of primitive first + i becomes materials_dev[i] (DEVICE
 * int32[count]).  No rebuild, no refit, a ready refit schedule stays ready; rt_scene_update_prims
 * checks its records against the new materials afterwards.  Blocks like an update; render the next
 * frame with reset = 1.  count == 0 is RT_OK.
 *   RT_ERR_INVALID      null scene or materials; a range that holds primitive 0 (the light's material
 *                       feeds the light sampling and the kernel family) or lies outside the
 *                       primitives; a material outside [0, num_materials), checked on the device in a
 *                       pass of its own before anything is written.
 * After every refusal the scene is untouched. */
int rt_scene_set_prim_materials(rt_scene *s, uint32_t first, uint32_t count, const int32_t *materials_dev, void *stream);
int rt_scene_set_prim_materials_host(rt_scene *s, uint32_t first, uint32_t count, const int32_t *materials);
/* rt_bvh_cost of the scene's CURRENT device tree -- the node records as they are after any number of
 * updates, rebuilds and splices -- reduced on the GPU (per workgroup, then over the workgroups' partial
 * sums; no copy of the tree to the host).  Blocks like rt_renderer_tile_work: runs on `stream` and
 * returns with *out filled.  "Refit or rebuild?": compare sah after a refit with its value after the
 * last rebuild.
 *   RT_ERR_INVALID      null argument;
 *   RT_ERR_UNSUPPORTED  a scene whose node bounds are not all finite -- *out is untouched. */
int rt_scene_bvh_cost(rt_scene *s, rt_bvh_cost *out, void *stream);

/* Batched Scene::IntersectBVH (template/scene.h:285-320): rays_dev[n] -> hits_dev[n]. */
int rt_intersect(rt_scene *s, const rt_ray *rays_dev, rt_hit *hits_dev, uint32_t n, void *stream);
/* Batched Scene::IsOccluded (template/scene.h:452-487): out_dev[i] = 1 if occluded. */
int rt_occluded(rt_scene *s, const rt_ray *rays_dev, uint8_t *out_dev, uint32_t n, void *stream);
/* Batched Scene::IntersectBVHPacket (template/scene.h:322-412, RayPacket Ray.h:34-64):
 * rays [64k, 64k + 64) form packet k (PACKET_SIZE 64) and share one first-active
 * traversal; the last packet may be partial (its missing slots take no part). */
int rt_intersect_packets(rt_scene *s, const rt_ray *rays_dev, rt_hit *hits_dev, uint32_t n, void *stream);
/* Host-pointer conveniences of the three above (copy in, launch, copy out, sync). */
int rt_intersect_host(rt_scene *s, const rt_ray *rays, rt_hit *hits, uint32_t n);
int rt_occluded_host(rt_scene *s, const rt_ray *rays, uint8_t *out, uint32_t n);
int rt_intersect_packets_host(rt_scene *s, const rt_ray *rays, rt_hit *hits, uint32_t n);
/* Batched Scene::BVHVisualization (template/scene.h:244-283): counts_dev[2i] = nodeTraversals,
 * counts_dev[2i+1] = intersections (leaves reached) of rays_dev[i]; the ray's tmax is its t.  The walk
 * is IntersectBVH's with the primitive tests taken out, so t never shrinks; the root's own box is
 * never tested (a root that is a leaf gives (1, 1) for every ray). */
int rt_bvh_visualize(rt_scene *s, const rt_ray *rays_dev, uint32_t *counts_dev, uint32_t n, void *stream);
int rt_bvh_visualize_host(rt_scene *s, const rt_ray *rays, uint32_t *counts, uint32_t n);
/* no device: the same walk over a BVHNode array (rt_bvh_build_host's, rt_scene_copy_bvh's).
 * RT_ERR_INVALID for a null pointer, a tree deeper than 64 or a child index outside nodes_used --
 * nothing is written then. */
int rt_bvh_visualize_nodes(const void *nodes, uint32_t nodes_used, const rt_ray *rays, uint32_t *counts, uint32_t n);

/* Batched Renderer::Trace(Ray&, bool lastSpecular, int depth) (renderer.h:9, renderer.cpp:17-72)
 * or, with mode RT_MODE_WHITTED, Renderer::WhittedTrace(Ray&, int depth) (renderer.h:13,
 * renderer.cpp:138-195); depth <= 32, 0 returns black as the reference does.
 *   rays_dev[n]        the rays (O, D, t);
 *   seeds_dev[n]       ray i's RNG state (the seed RandomFloat() advances,
 *                      template/template.cpp:673-704), updated in place to the state after
 *                      the call, so calls chain like the reference's global seed;
 *   flags_dev[n]       bit 0 = lastSpecular, bit 1 = Ray::inside; NULL = lastSpecular true,
 *                      outside (the reference's defaults);
 *   radiance_dev[3n]   the returned float3 per ray;
 *   hits_dev[n]        optional (NULL): the ray as the first Scene::IntersectBVH leaves it
 *                      (Trace takes Ray&, renderer.cpp:20);
 *   ray_counts_dev[2]  optional (NULL): shadow rays and bounce rays traced, added to. */
int rt_trace(rt_scene *s, int mode, const rt_ray *rays_dev, uint32_t *seeds_dev, const uint8_t *flags_dev,
             uint32_t depth, float *radiance_dev, rt_hit *hits_dev, uint64_t *ray_counts_dev, uint32_t n, void *stream);
/* Host-pointer convenience of rt_trace (all arrays in host memory; synchronous). */
int rt_trace_host(rt_scene *s, int mode, const rt_ray *rays, uint32_t *seeds, const uint8_t *flags, uint32_t depth,
                  float *radiance, rt_hit *hits, uint64_t *ray_counts, uint32_t n);

/* ---- renderer (Renderer, renderer.h:5-160) -------------------------------- */
/* Camera::Camera (camera.h:28-41) for a W x H target */
int rt_camera_default(uint32_t width, uint32_t height, rt_camera *out);
int rt_renderer_create(rt_scene *s, uint32_t width, uint32_t height, rt_renderer **out);
int rt_renderer_destroy(rt_renderer *r);
/* Renderer::Tick (renderer.cpp:200-309): trace every pixel, running average into
 * the float4 accumulator (235-241), RGBF32_to_RGB8 pack (template/precomp.h:432-448)
 * into rgb8_dev[W*H] (0x00RRGGBB).  One kernel launch. */
int rt_render_frame(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t *rgb8_dev, void *stream);
/* Same as rt_render_frame, RGB8 delivered to host memory (the reference's
 * screen->pixels, template/template.cpp:273-277); synchronous. */
int rt_render_frame_host(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t *rgb8_host);

/* ---- first-hit G-buffer of a frame's camera rays, and pixel picking ----------
 * The camera ray of a pixel of the frame p describes -- with the sub-pixel and lens jitter of
 * Camera::GetPrimaryRay (camera.h:43-52), drawn from the seed InitSeed(px + W*H*(sample + spp*frame))
 * of that sample of that frame -- traced to its first hit, and what lies there.  A query: it reads and
 * writes nothing of the renderer's frame state (accumulator, rt_counters, walk statistics, tile costs,
 * timed choices, frames in flight), and runs on the caller's stream behind the scene's pending
 * stream-ordered updates, as a frame does: rt_scene_update_*_async followed by rt_render_gbuffer sees the
 * updated scene with no host synchronisation. */
typedef struct { float nx, ny, nz; int32_t material; } rt_gnormal;  /* 16 B */
typedef struct { float r, g, b;   int32_t kind;     } rt_galbedo;  /* 16 B */

/* every plane optional (NULL = not written); at least one must be set */
typedef struct {
    rt_ray     *ray;     /* the camera ray as GetPrimaryRay returns it (tmax = the ray's initial t) */
    rt_hit     *hit;     /* the ray as IntersectBVH leaves it (template/scene.h:285-320) + finish_uv: t, obj (-1 = sky), u, v */
    rt_gnormal *normal;  /* Scene::GetNormal(obj, I, D) (template/scene.h:489-497; flipped against the ray), I = O + t*D;
                            material = the primitive's material id; sky: 0,0,0 and -1 */
    rt_galbedo *albedo;  /* the material's GetColor(ray) at the hit (Diffuse/Mirror/Light/DSMix colour, Checkerboard.h:28-37,
                            TextureMaterial.h:32-39, Dielectric.h:12-21 with inside = false), kind = RT_* material kind;
                            sky: skyColor(D) (renderer.h:15-22) and -1 */
} rt_gbuffer;

/* pixels [x0, x0+w) x [y0, y0+h) of the frame p describes; planes are rect-sized, row-major, stride w.
 * p->width, p->height, p->spp and p->frame define the ray (spp 0 counts as 1); p->depth, p->mode and
 * p->reset are ignored.  The camera walk is the scene's policy as a frame would take it: RT_WALK_LANE the
 * lane walk, RT_WALK_WAVE the wave walk, RT_WALK_AUTO whatever this renderer's primary+shadow frames
 * have settled on (the lane walk while nothing is settled; no timed choice starts or advances).
 *   RT_ERR_INVALID  null r / cam / p / out, all four planes NULL, sample >= max(1, spp), an empty
 *                   rectangle or one that leaves the frame, a width or height that is not the renderer's. */
int rt_render_gbuffer(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample,
                      uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const rt_gbuffer *out_dev, void *stream);
/* the same with the planes in host memory (through the scene's staging buffer; synchronous) */
int rt_render_gbuffer_host(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample,
                           uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, const rt_gbuffer *out);
/* picking: listed pixel indices (x + y*W, any order, duplicates allowed), planes indexed by list position;
 * always the lane walk (a list's lanes are not a tile).  n == 0 succeeds and launches nothing.
 *   RT_ERR_INVALID  as above, a null list with n > 0, and -- the _host form, which can read its list -- a
 *                   pixel index >= W*H.  The device form reads its list on the GPU only: an index
 *                   >= W*H there leaves that list position of every plane unwritten. */
int rt_gbuffer_pixels(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample,
                      const uint32_t *pixels_dev, uint32_t n, const rt_gbuffer *out_dev, void *stream);
int rt_gbuffer_pixels_host(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t sample,
                           const uint32_t *pixels, uint32_t n, const rt_gbuffer *out);
/* What the next rt_render_gbuffer (pixels = 0) or rt_gbuffer_pixels (pixels != 0) of this renderer launches
 * with, from the same place the launch takes it: *wave_walk = 1 the wave camera walk, 0 the lane walk;
 * *lds_bytes (optional) the launch's dynamic LDS per workgroup -- the lane stacks, plus the wave walk's
 * word stack when it runs.  Reads only; RT_ERR_INVALID for a null r or wave_walk. */
int rt_renderer_gbuffer_walk(const rt_renderer *r, int pixels, int *wave_walk, uint32_t *lds_bytes);
/* Screen-tile shard of a frame: the 8x8 tiles t with t % num_shards == shard,
 * packed as [tile][64] pixels into tiles_dev (rt_shard_capacity pixels). */
int rt_shard_capacity(uint32_t width, uint32_t height, uint32_t num_shards, uint32_t *pixels);
int rt_render_shard(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard,
                    uint32_t num_shards, uint32_t *tiles_dev, void *stream);
/* Rank-0 side of the per-frame gather: gathered_dev = num_shards consecutive shard
 * buffers (each rt_shard_capacity pixels) -> rgb8_dev[W*H]. */
int rt_assemble_shards(rt_renderer *r, const uint32_t *gathered_dev, uint32_t num_shards, uint32_t *rgb8_dev,
                       void *stream);
/* Explicit tile deals (cost-balanced multi-GPU frames).  A deal lists every 8x8 tile of the
 * frame (row-major tile index t = ty * ceil(W/8) + tx) once: shard k owns
 * deal_tiles[deal_off[k] .. deal_off[k+1]).
 * rt_tile_deal: the Morton-ordered tiles cut into num_shards runs of equal summed cost
 *   (cost[t] per tile, e.g. rt_renderer_tile_costs of a full frame; NULL = equal costs):
 *   deal_tiles[ceil(W/8) * ceil(H/8)], deal_off[num_shards + 1].
 * rt_render_shard_tiles: the listed tiles (in that order) of one frame, packed as [i][64]
 *   into tiles_dev -- Renderer::Tick's pixel loop over those tiles only.
 * rt_assemble_tiles: rank 0's unshuffle; shard k's packed tiles at gathered_dev + k * stride_px. */
int rt_tile_deal(uint32_t width, uint32_t height, const uint32_t *cost, uint32_t num_shards, uint32_t *deal_tiles,
                 uint32_t *deal_off);
int rt_render_shard_tiles(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, const uint32_t *tiles,
                          uint32_t num_tiles, uint32_t *tiles_dev, void *stream);
int rt_assemble_tiles(rt_renderer *r, const uint32_t *gathered_dev, uint32_t stride_px, const uint32_t *deal_tiles,
                      const uint32_t *deal_off, uint32_t num_shards, uint32_t *rgb8_dev, void *stream);
/* ---- multi-GPU frames (one process per GPU) ---------------
 * Replaces the OpenMP pixel loop of Renderer::Tick (renderer.cpp:213-245) across the GPUs of
 * a node: rank k renders the 8x8 tiles t with t % world == k, then ONE RCCL gather per frame
 * (ncclSend / ncclRecv to rank 0 in one group) and rank 0's assembly.  Every rank keeps its
 * own scene replica and accumulator.  RCCL (librccl.so.1) is loaded at first use. */
#define RT_COMM_ID_BYTES 128
typedef struct rt_comm rt_comm;
/* rank 0 makes the id (ncclGetUniqueId) and hands it to the other ranks out of band */
int rt_comm_unique_id(uint8_t id[RT_COMM_ID_BYTES]);
/* collective: every rank calls it with the same id (ncclCommInitRank); device = this rank's GPU */
int rt_comm_create(const uint8_t id[RT_COMM_ID_BYTES], int rank, int world, int device, rt_comm **out);
/* use a caller-owned ncclComm_t (from the same librccl.so.1; not destroyed by rt_comm_destroy) */
int rt_comm_wrap(void *nccl_comm, int device, rt_comm **out);
int rt_comm_info(const rt_comm *c, int *rank, int *world);
int rt_comm_destroy(rt_comm *c);
/* One frame on every rank (same camera and params everywhere).  flags 0: in stream order,
 * render this rank's tiles, gather, and on rank 0 assemble the frame into rgb8_dev (W*H;
 * ignored, may be NULL, on other ranks).  RT_MULTI_PIPELINED: the frame's gather runs on
 * the communicator's own stream beside the caller's next work, and the call completes the
 * PREVIOUS pipelined frame into rgb8_dev (nothing on the first call); rt_multi_flush
 * completes the last one.  Counters and the accumulator stay per rank. */
#define RT_MULTI_PIPELINED 1u
/* RT_MULTI_TIMING: HIP events around this rank's render and its gather, summed by rt_comm_timing */
#define RT_MULTI_TIMING 2u
/* RT_MULTI_BALANCED: the ranks render the cost-balanced compact deal of rt_tile_deal instead of
 * t % world.  Costs: the dry-run work map of each rank's tiles (rt_renderer_tile_work's node
 * visits + primitive tests, deterministic) for RT_MODE_PATH frames; the measured wave cycles
 * (rt_renderer_tile_costs) for the other modes, once every rank has them.  A parameter set
 * (camera, size, spp, depth, mode) tries on its 6th frame (then its 12th, 24th, ... while some
 * rank has no costs) -- one all-gather of [status, costs] blocks, after which every rank builds
 * the same deal -- and not again until a parameter changes; the deal in use is kept across
 * camera moves.  When tiles
 * change owner their accumulator values move to the new owner (point-to-point, in stream
 * order), except on frames with reset set, so accumulation goes on exactly.  Frames are
 * identical under any deal; every rank must pass the same flags. */
#define RT_MULTI_BALANCED 4u
int rt_render_frame_multi(rt_renderer *r, rt_comm *c, const rt_camera *cam, const rt_frame_params *p,
                          uint32_t *rgb8_dev, uint32_t flags, void *stream);
int rt_multi_flush(rt_renderer *r, rt_comm *c, uint32_t *rgb8_dev, void *stream);
/* Sum over the RT_MULTI_TIMING frames since the last call (waits for them): render_ms =
 * this rank's shard render, gather_ms = from the render's end to the gather's completion,
 * max(0, ...) per frame (exposed exchange latency; beside the next render in pipelined mode).
 * Pipelined rank 0 receives on the communicator's stream without waiting for its own render,
 * so its figure is how much later than its own tiles the peers' tiles arrived (0 when they
 * were there first); resets the sums. */
int rt_comm_timing(rt_comm *c, double *render_ms, double *gather_ms, uint64_t *frames);
/* The deal frames are rendered under now (every argument but c may be NULL): *balanced = 1 for a
 * cost-balanced deal, 0 for the interleaved one; *ntiles = this rank's tile count and tile_list
 * (room for *ntiles) its global tile indices in render order; stats: [0] balanced deals built,
 * [1] cost exchanges run, [2] accumulator moves run, [3] moves skipped on reset frames. */
int rt_comm_deal_info(const rt_comm *c, int *balanced, uint32_t *ntiles, uint32_t *tile_list, uint64_t stats[4]);
/* FNV-1a hash of the deal in use (every rank's tile lists and offsets): equal on every rank, and
 * in two runs that built the same deal -- every run of the same frames for RT_MODE_PATH deals,
 * whose costs are the deterministic work map.  (Cycle costs of the other modes are rounded to
 * 1/64 of the frame's mean tile cost first, so run-to-run noise rarely moves a cut.) */
int rt_comm_deal_hash(const rt_comm *c, uint64_t *hash);

int rt_renderer_counters(rt_renderer *r, rt_counters *out);
/* Overlapped primary+shadow frames (RT_PS_PIPELINE; no reference counterpart -- Renderer::Tick,
 * renderer.cpp:200-309, is one serial pass): *state = 1 this renderer's primary+shadow frames
 * run overlapped (frame kernel on a renderer stream, accumulate + RGB8 in a finishing pass on
 * the caller's stream), 0 serial, -1 not decided yet (RT_PS_PIPELINE=-1 times both modes on
 * the first eligible frames); ms (may be NULL) = the serial and 2-in-flight groups' milliseconds
 * (serial, overlapped, overlapped, serial) when decided by timing, else zeros. */
int rt_renderer_overlap(const rt_renderer *r, int *state, float ms[4]);
/* The same decision with its depth: *depth = primary+shadow frames in flight (1 serial, 2..6
 * overlapped on that many renderer streams; -1 not decided yet).  RT_PS_PIPELINE=-1 times groups
 * of eight frames in palindromic order -- serial, 2, 4, 6, 6, 4, 2, serial in flight for frames
 * of at most ~3 rounds of resident waves, serial, 2, 2, serial otherwise -- and keeps the
 * fastest; RT_PS_PIPELINE=1 forces RT_PS_DEPTH (default 2).  ms (may be NULL) = the groups' ms
 * (8 entries; unused ones 0). */
int rt_renderer_overlap_depth(const rt_renderer *r, int *depth, float ms[8]);
/* Device memory the renderer holds right now (diagnostics; INTEGRATION.md "Device memory per
 * renderer"): *bytes = the sum of what is allocated -- accumulator, counters, RGB8, path-state slots,
 * result, sample and sample-sum buffers, tile orders and cost maps (11 words per local tile), the work
 * map of rt_renderer_tile_work and the deal maps; *ps_buffers (may be NULL) = overlapped-frame result buffers allocated
 * (up to 7 while the frames-in-flight choice is timed, depth + 1 or 0 after it). */
int rt_renderer_device_bytes(const rt_renderer *r, uint64_t *bytes, uint32_t *ps_buffers);
/* The renderer's other timed choices for its current parameter set (diagnostics): *walk = the
 * camera-ray walk of primary+shadow frames (0 lane, 1 wave, -1 not decided); *split = the
 * half-tile split order of its costliest tiles (1 on, 0 off, -1 not decided / not applicable);
 * walk_ms / split_ms (may be NULL) = the four timed groups (A, B, B, A) in ms. */
int rt_renderer_choices(const rt_renderer *r, int *walk, int *split, float walk_ms[4], float split_ms[4]);
/* The measured cost map behind the longest-tile-first order of the renderer's current parameter
 * set (camera, size, spp, depth, mode, shard): costs[i] = wave cycles (s_memtime ticks) of
 * local tile i, recorded on one frame; *n_out = its tile count (0 until recorded: from the 2nd
 * frame of a parameter set on).  At most n entries are copied.  Diagnostics and cost-balanced
 * tile deals. */
int rt_renderer_tile_costs(const rt_renderer *r, uint32_t *costs, uint32_t n, uint32_t *n_out);
/* Deterministic work map of one whole frame (camera + params as rt_render_frame, RT_MODE_PATH
 * only): a dry run that traces the frame's rays -- same seeds, camera rays in the reference's
 * IntersectBVH order -- and writes nothing but counts; the accumulator, the frame count and the
 * ray counters are untouched.  work[t] (n >= ceil(W/8) * ceil(H/8), row-major tiles) = BVH node
 * visits + primitive tests of tile t's rays, summed over its pixels and samples.  pixel_work_dev
 * (device, may be NULL): 8 u32 per pixel -- [0] closest-hit node visits, [1] closest-hit primitive
 * tests, [2] any-hit (shadow) node visits, [3] any-hit primitive tests, [4] / [5] closest-hit
 * pops of an interior / leaf stack entry whose pushed entry distance is >= the ray's t at the pop
 * ([4]: pair loads an exact pop-time cull would skip; 0 for trees deeper than 28), [6] [7] 0.
 * Blocks on `stream`.  The multi-GPU deals (RT_MULTI_BALANCED) are cut on this map, so two runs
 * of a frame get the same deal. */
int rt_renderer_tile_work(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t *work, uint32_t n,
                          uint32_t *pixel_work_dev, void *stream);
/* Checks of the wave-coherent camera walk (RT_WALK_WAVE, or RT_WALK_AUTO once timed faster) of a
 * renderer's primary+shadow frames.  The walk always re-traces in the reference order every lane
 * whose result could depend on the visiting order (an exact-distance tie, or a hit nearer than
 * its leaf box's entry -- which covers every hit found in a box entered through the walk's 2^-18
 * cull margin).  Beyond that:
 *   RT_WALK_CHECK_OFF    (default) the production frame kernel, nothing counted;
 *   RT_WALK_CHECK_COUNT  a build of the frame kernel that counts camera rays walked, lanes
 *                        re-traced and boxes a lane entered only through the cull margin;
 *   RT_WALK_CHECK_VERIFY that build also re-traces EVERY walked lane in the reference order
 *                        (IntersectBVH, template/scene.h:285-320), keeps that result and counts the
 *                        lanes whose walk result (id, t, u, v bits) differed -- a diagnostic.
 * Frames are identical at every level. */
enum { RT_WALK_CHECK_OFF = 0, RT_WALK_CHECK_COUNT = 1, RT_WALK_CHECK_VERIFY = 2 };
int rt_renderer_set_walk_check(rt_renderer *r, int level);
/* Cumulative camera-walk counters of the frames rendered at RT_WALK_CHECK_COUNT / _VERIFY
 * (synchronises the device): out[0] camera rays the wave walk traced, out[1] boxes entered only
 * through its cull margin, out[2] lanes re-traced in the reference order, out[3]
 * RT_WALK_CHECK_VERIFY lanes whose walk result differed from the reference order's (0 expected). */
int rt_renderer_walk_stats(rt_renderer *r, uint64_t out[4]);
/* accumulator readback, W*H float4 */
int rt_renderer_read_accumulator(rt_renderer *r, float *host_out);
/* Name of the frame kernel rt_render_frame / rt_render_shard launch for these params
 * (as it appears in rocprofv3 kernel traces, template arguments abbreviated; "k_render_heat" for
 * RT_MODE_BVH_HEAT); for
 * profiling and the bench's roofline line.  NULL on a bad argument. */
const char *rt_frame_kernel_name(const rt_renderer *r, const rt_frame_params *p);
int rt_renderer_stream(rt_renderer *r, void **stream);
int rt_synchronize(rt_renderer *r);

#ifdef __cplusplus
}
#endif
#endif
