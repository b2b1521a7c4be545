// rt_internal.h -- host-side internals shared by rt_host.cpp, rt_scene_pack.cpp, rt_device.hip and rt_scene_edit.hip.
#pragma once
#include <string>
#include <vector>

#include "../../include/rt_amd.h"
#include "rt_dev_types.h"
#include "rt_math.h"
#include "rt_records.h"

namespace rt {

// thread-local error message for rt_last_error()
void set_error(const std::string &msg);
int fail(int code, const std::string &msg);

// 32-byte BVHNode (BVHNode.h:5-14): aabbMin, aabbMax, leftFirst, primitiveCount
struct Node {
    float mn[3], mx[3];
    uint32_t leftFirst, count;
};
static_assert(sizeof(Node) == 32, "BVHNode layout");

// The record encoders (rt_records.h) also hold the primitives' transforms and geometry -- PrimX,
// prim_transform, fast_inverse, PrimGeom, prim_geometry -- one text for the host and for gfx950.
void translate_matrix(float x, float y, float z, float M[16]);

// Plain binned-SAH BVH (template/scene.h:845-976).  nodes sized 2N+2, indices N.
struct Bvh {
    std::vector<Node> nodes;
    std::vector<uint32_t> indices;
    uint32_t nodes_used = 0, depth = 0, max_leaf = 0;
};
int build_bvh(const rt_prim *prims, const float *transforms, uint32_t n, Bvh &out);
// Spatial-split BVH (rt_sbvh.cpp): indices hold references (a primitive may repeat)
int build_sbvh(const rt_prim *prims, const float *transforms, uint32_t n, Bvh &out);

// The one walk of a node array (rt_host.cpp): pre-order from the root, left child first, over the
// first nodes_used nodes with leaves inside `slots` leaf slots.  order = the nodes as met, and per
// node index its parent (~0u: the root, or a node the walk never met) and its depth (root 0).
struct TreeWalk {
    std::vector<uint32_t> order, parent, depth;
    uint32_t max_leaf = 0;   // the widest leaf's count
};
enum { kTreeOk = 0, kTreeChildRange, kTreeLeafRange, kTreeCycle };
// kTreeChildRange: a child pair outside [2, nodes_used); kTreeLeafRange: a leaf past the slots;
// kTreeCycle: more nodes met than a tree of nodes_used nodes has.  The caller words the error.
int walk_tree(const Node *N, uint32_t nodes_used, size_t slots, TreeWalk &out);

// Scene creation up to the upload (rt_scene_pack.cpp): no HIP call, no environment variable.
struct PackOptions {
    int bvh_kind = RT_BVH_PLAIN;      // the tree built where the description brings none
    float walk_margin = 0x1p-12f;     // the wave walk's cull margin
    double sliver_lim = 0x1p-8;       // tri_sliver's sine limit (0: no triangle is a sliver)
    bool sticky_spheres = true;       // spheres and quads make their nodes sticky
    bool quads = false;               // build the two-level node records (build_quads)
};
struct ScenePack {            // everything scene_create computes before it touches the device
    Bvh bvh;
    std::vector<float4> nodes, prims, shade, xprims, quads;
    std::vector<DevMaterial> mats;
    std::vector<uint32_t> sky, texels;
    SceneView view;           // scalar fields only; pointers stay null
    // per primitive its type | sticky << 7 and its box (prim_geometry; 6 floats): what a refit
    // needs of the primitives that do not move
    std::vector<uint8_t> pinfo;
    std::vector<float> pbox;
    std::vector<float> pcen;  // ... and its centroid (3 floats), what a rebuild bins by
    uint32_t stack_depth;     // LDS stack entries per lane
    bool ext, has_cubes, nested, walk_fits, boxes_finite, has_quads;
    bool ext_fixed;           // ext for reasons no edit of the primitives changes (family_fixed)
};
// The kernel family a scene needs, one rule for creation (check_description) and for the commit of an
// edit that lets kinds enter and leave (rt_scene_splice_prims).  ext: the kext kernels -- a cube or a
// quad anywhere (the light included), or `fixed`: a light material other than the core four, a texture
// material.  has_cubes: cube acceptance depends on the visiting order, no wave walk.
// type_of(i): the type of primitive i.
inline bool family_fixed(const rt_material *mats, uint32_t num_materials, int32_t light_material) {
    const int lk = mats[light_material].kind;
    bool fixed = !(lk == RT_LIGHT || lk == RT_DIFFUSE || lk == RT_MIRROR || lk == RT_DSMIX);
    for (uint32_t i = 0; i < num_materials && !fixed; ++i) fixed = mats[i].kind == RT_TEXTURE;
    return fixed;
}
template <class TypeOf>
inline void kernel_family(uint32_t n, TypeOf type_of, bool fixed, bool &ext, bool &has_cubes) {
    ext = fixed;
    has_cubes = false;
    for (uint32_t i = 0; i < n; ++i) {
        const int t = type_of(i);
        if (t == RT_CUBE) has_cubes = true;
        if (t == RT_CUBE || t == RT_QUAD) ext = true;
    }
}
int pack_scene(const rt_scene_desc *d, const PackOptions &o, ScenePack &out);
// what follows from a tree's depth: the LDS stack entries per lane, and whether the wave walk's word
// stack fits beside the lane stacks (take_tree; rt_scene_rebuild)
uint32_t pick_stack(uint32_t depth);
bool stack_admits_walk(uint32_t stack_depth);

// frame size and device of a renderer (rt_multi.cpp)
int renderer_geometry(const rt_renderer *r, uint32_t *W, uint32_t *H, int *device);
// the 8x8 tiles whose running averages the renderer's accumulator holds (its last frame's tiles:
// all of them after a whole frame, a shard's after a shard); false before its first frame
bool renderer_held_tiles(const rt_renderer *r, std::vector<uint32_t> &tiles);
// the renderer's device accumulator (W*H float4 = 16 B each); and the accumulator values of
// the 8x8 tiles listed in DEVICE memory (tiles_dev) packed as [i][64] float4 into buf_dev /
// written back from it (pixels outside the frame: 0 / skipped), in stream order on `stream`
// with no host synchronisation -- rt_multi.cpp moves a pixel's running average to its new rank
// when a multi-GPU deal changes owners
int renderer_accumulator(rt_renderer *r, void **acc_dev, size_t *bytes);
int accumulator_pack(rt_renderer *r, const uint32_t *tiles_dev, uint32_t n, void *buf_dev, void *stream);
int accumulator_unpack(rt_renderer *r, const uint32_t *tiles_dev, uint32_t n, const void *buf_dev, void *stream);
// one rank's part of a multi-GPU frame (rt_multi.cpp): the interleaved shard `shard` of
// `nshards`, or the explicit tile list `tiles` (n tiles; n == 0 with tiles != NULL: none),
// written packed ([local tile][64], rt_render_shard's layout) or, packed == 0, straight into a
// row-major W x H frame at the tiles' own pixels (rank 0 renders its tiles into the output frame).
// fwd_src / fwd_dst (row-major only, may be NULL): as each pixel is stored, its value in fwd_src is
// first forwarded to fwd_dst (the previous frame handed to the caller within the same launch)
int render_part(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
                const uint32_t *tiles, uint32_t n, int packed, uint32_t *out_dev, void *stream,
                const uint32_t *fwd_src = nullptr, uint32_t *fwd_dst = nullptr);

// the dry-run work map of the same part of a frame (rt_renderer_tile_work): per local tile, node
// visits + primitive tests summed over its lanes and samples -- deterministic, the multi-GPU
// deals' cost input.  Blocks on `stream`.  RT_ERR_UNSUPPORTED for modes other than RT_MODE_PATH.
int render_work(rt_renderer *r, const rt_camera *cam, const rt_frame_params *p, uint32_t shard, uint32_t nshards,
                const uint32_t *tiles, uint32_t n, std::vector<uint32_t> &work, void *stream);

// SURVEY.md 8(d) scenes as descriptions
struct SceneSource {
    std::vector<rt_prim> prims;
    std::vector<rt_material> materials;
};
int recipe_source(const std::string &name, const std::string &mesh_dir, SceneSource &out);

}  // namespace rt
