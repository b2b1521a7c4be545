// rt_cost.h -- tree cost (rt_bvh_cost): the per-node term of calculateNodeCost (template/scene.h:203-207)
// summed over a node array.  One text for the host (rt_bvh_cost_host, rt_host.cpp) and for gfx950
// (rt_scene_bvh_cost, rt_cost.hip), under the same -ffp-contract=off, so a node's area has the same
// bits on both; only the order of the sums differs.
#pragma once
#include "rt_internal.h"
#include "rt_records.h"

namespace rt {

// the half area of a box in double, left to right: a plane's +-1e30 box overflows float32
RT_HD double box_area(f3 mn, f3 mx) {
    const double ex = (double)mx.x - (double)mn.x, ey = (double)mx.y - (double)mn.y, ez = (double)mx.z - (double)mn.z;
    return ex * ey + ey * ez + ez * ex;
}

// the sums of rt_bvh_cost over some of the nodes
struct CostPart {
    double interior_area, leaf_area, leaf_cost;
    uint32_t interiors, leaves, refs, max_leaf;
};
// one node: count == 0 is an interior node, else a leaf of count primitives
RT_HD void cost_add(CostPart &c, f3 mn, f3 mx, uint32_t count) {
    const double area = box_area(mn, mx);
    if (count == 0) {
        c.interior_area += area;
        c.interiors += 1u;
    } else {
        c.leaf_area += area;
        c.leaf_cost += (double)count * area;
        c.leaves += 1u;
        c.refs += count;
        c.max_leaf = count > c.max_leaf ? count : c.max_leaf;
    }
}
RT_HD void cost_merge(CostPart &a, const CostPart &b) {
    a.interior_area += b.interior_area;
    a.leaf_area += b.leaf_area;
    a.leaf_cost += b.leaf_cost;
    a.interiors += b.interiors;
    a.leaves += b.leaves;
    a.refs += b.refs;
    a.max_leaf = b.max_leaf > a.max_leaf ? b.max_leaf : a.max_leaf;
}
// the public record from the sums over every node but node 1 and the root's area
inline void cost_finish(const CostPart &c, double root_area, rt_bvh_cost *out) {
    out->interior_area = c.interior_area;
    out->leaf_area = c.leaf_area;
    out->leaf_cost = c.leaf_cost;
    out->root_area = root_area;
    out->sah = root_area == 0.0 ? 0.0 : (c.interior_area + c.leaf_cost) / root_area;
    out->interiors = c.interiors;
    out->leaves = c.leaves;
    out->refs = c.refs;
    out->max_leaf = c.max_leaf;
}

// The cost of the device node records d_nodes (2 float4 per node, node_pack's layout) on `st`: per
// workgroup, then over the workgroups' partial sums in a second launch; *d_buf is the scene's scratch
// for the partial sums (allocated here on first use).  Blocks; *out is written on success only.
int device_bvh_cost(const void *d_nodes, uint32_t nodes_used, void **d_buf, hipStream_t st, rt_bvh_cost *out);

}  // namespace rt
