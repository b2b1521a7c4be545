// rt_refit.h -- in-place updates: the refit plan of a scene's tree and the launchers of the kernels
// in rt_refit.hip (rt_scene_update_triangles, rt_scene_update_prims, rt_scene_transform_triangles;
// rt_device.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "rt_internal.h"

namespace rt {

// A treelet is a whole subtree of at most this many nodes; one workgroup refits it.
constexpr uint32_t kTreeletNodes = 256;

// The refit schedule of one tree (topology only, so it is built once per scene):
//   slot_of[id]  the leaf slot of primitive id (the inverse of Bvh::indices);
//   list         node indices: treelet 0's nodes sorted by height above their deepest leaf,
//                treelet 1's, ..., then the nodes above the cut (every subtree of more than
//                kTreeletNodes nodes), sorted by height too;
//   lvl          boundaries into list: a group (a treelet, or the top) of L heights owns L + 1
//                consecutive entries, the start of each height and the group's end;
//   grp[g]       the group's first entry in lvl (ntreelets + 2 entries; the top is group ntreelets).
// A node's children have smaller heights, so they sit in earlier levels of its group or, for a
// node above the cut, in a treelet.
struct RefitPlan {
    std::vector<uint32_t> slot_of, list, lvl, grp;
    uint32_t ntreelets = 0;
    bool has_top = false;
};
// false when the tree is not a plain one (a primitive in no leaf or in two)
bool build_refit_plan(const Bvh &b, uint32_t num_prims, RefitPlan &out);

struct RefitArgs {
    float4 *nodes, *prims, *shade;   // the scene's device records (SceneView)
    float4 *slot_box;                // 2 float4 per leaf slot: (box min, sticky flag), (box max, 0)
    const uint32_t *slot_of, *list, *lvl, *grp;
    float margin;                    // SceneView::walk_margin
    double sliver_lim;               // mark_sticky's sine limit
};
// *flag_dev = 1 if any of the n floats is NaN or infinite (untouched otherwise)
void launch_check_finite(const float *verts_dev, uint32_t n, uint32_t *flag_dev, hipStream_t st);
void launch_update_tris(const RefitArgs &A, uint32_t first, uint32_t count, const float *verts_dev, hipStream_t st);
// rt_scene_update_prims: records of any kind for primitives [first, first + count), one transform
// (16 floats) per record or none.  The check sets *flag_dev = 1 on a type or material that is not
// the scene's, a NaN / infinite field, transform or box; the update also takes the side table.
void launch_check_prims(const float4 *shade, uint32_t first, uint32_t count, const rt_prim *prims_dev,
                        const float *transforms_dev, uint32_t *flag_dev, hipStream_t st);
void launch_update_prims(const RefitArgs &A, float4 *xprims, uint32_t first, uint32_t count, const rt_prim *prims_dev,
                         const float *transforms_dev, hipStream_t st);
// rt_scene_transform_triangles' range table in device memory: range r moves triangles
// [first[r], first[r] + pre[r + 1] - pre[r]) by M[16 r ..]; pre[nr] = all triangles of the call
struct XformRanges {
    const uint32_t *first, *pre;
    const float *M;
    uint32_t nr;
};
// *flag_dev = 1 if a transformed vertex is NaN or infinite; then the triangles' records from them
void launch_check_xform(const XformRanges &R, uint32_t total, const float *rest_dev, uint32_t *flag_dev, hipStream_t st);
void launch_xform_tris(const RefitArgs &A, const XformRanges &R, uint32_t total, const float *rest_dev, hipStream_t st);
// the treelets, then (a second launch) the nodes above the cut
void launch_refit(const RefitArgs &A, uint32_t ntreelets, bool has_top, hipStream_t st);

}  // namespace rt
