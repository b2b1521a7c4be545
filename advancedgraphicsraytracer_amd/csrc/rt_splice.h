// rt_splice.h -- the per-lane text of rt_scene_splice_triangles: the step in front of
// the GPU builder (rt_build.h) that forms the new id space when triangles leave and enter a scene.
//
// One text for gfx950 and for the host, like rt_update.h and under the same -ffp-contract=off: the
// kernels of rt_splice.hip supply the lane index, a stand-alone host program runs the same lines in a
// loop (tests/cpp/splice_host.cpp).  No std:: algorithm.
//
// The edit removes ids [first, first + remove) and puts `insert` new triangles at id `first`.  The
// map from a new id j to where it comes from is closed-form, so no table travels:
//   j < first                       old id j;
//   first <= j < first + insert     inserted record j - first;
//   otherwise                       old id j - insert + remove.
// Everything is written in id order (slot = id) into fresh arrays: the builder then reads them with
// the identity as its old slot map, and its permute_slots puts the records into the new leaf order.
#pragma once
#include "rt_update.h"

namespace rt {

struct SpliceArgs {
    uint32_t n_new, first, remove, insert;
    const rt_prim *recs;             // the inserted triangles
    uint32_t num_materials;
    double sliver_lim;               // mark_sticky's sine limit (RefitState::sliver_lim)
    // the scene as it is: leaf-slot records and slot boxes per old slot, the rest per old id
    const float4 *old_prims, *old_shade, *old_cen, *old_box;
    const uint32_t *old_slot_of;
    // per new id: what the builder reads (leaf-slot record, slot box, the identity slot map) ...
    float4 *prims, *box;
    uint32_t *ident;
    // ... and what the scene keeps as it is written here (shading record, centroid)
    float4 *shade, *cen;
};

// The refusals that need neither the device nor the records' contents, in the order the header lists
// them; ptype[id] & 0x7f = the type of primitive id (RefitState::pinfo).  *bad: the non-triangle met.
enum { kSpliceOk = 0, kSpliceLight, kSpliceNull, kSpliceRange, kSpliceKind };
RT_HD int splice_range(uint32_t num_prims, const uint8_t *ptype, uint32_t first, uint32_t remove, uint32_t insert, const void *recs,
                       uint32_t *bad) {
    if (first == 0) return kSpliceLight;   // primitive 0 is the light and stays
    if (insert && !recs) return kSpliceNull;
    if ((uint64_t)first + remove > num_prims) return kSpliceRange;   // first == num_prims appends
    for (uint32_t id = first; id < first + remove; ++id)
        if ((ptype[id] & 0x7f) != RT_TRIANGLE) { *bad = id; return kSpliceKind; }
    return kSpliceOk;
}

// an inserted record is a triangle of one of the scene's materials with finite vertices
RT_HD bool splice_ok(const SpliceArgs &A, uint32_t i) {
    const rt_prim p = A.recs[i];
    return p.type == RT_TRIANGLE && p.material >= 0 && (uint32_t)p.material < A.num_materials && tri_ok(p.v);
}

// New id j.  A kept primitive copies its shading record, its centroid, its slot box and its leaf-slot
// record; the id is word q[0].w of every kind's record (tri_record, prim_record) and nothing else in
// any record depends on it -- a cube's or a quad's side-table index is its rank among cubes and quads,
// which triangles coming and going do not change.  An inserted triangle is written by the encoders
// that scene creation runs (pack_shade, pack_slots, pack_nodes and mark_sticky of rt_scene_pack.cpp).
RT_HD void splice_gather(const SpliceArgs &A, uint32_t j) {
    float4 q[3], b[2], s[2], c;
    if (j >= A.first && j < A.first + A.insert) {
        const rt_prim p = A.recs[j - A.first];
        const f3 N = tri_normal(p.v);
        s[0] = make_float4(N.x, N.y, N.z, ibits(p.material));
        s[1] = make_float4(ubits((uint32_t)RT_TRIANGLE), 0, 0, 0);
        tri_record(p.v, j, q);
        f3 mn, mx;
        tri_box(p.v, mn, mx);
        slot_box(mn, mx, tri_sliver(p.v, A.sliver_lim), b);
        c = tri_centroid(p.v);
    } else {
        const uint32_t o = j < A.first ? j : j - A.insert + A.remove;
        const uint32_t slot = A.old_slot_of[o];
        for (int k = 0; k < 2; ++k) s[k] = A.old_shade[2 * (size_t)o + k];
        c = A.old_cen[o];
        for (int k = 0; k < 2; ++k) b[k] = A.old_box[2 * (size_t)slot + k];
        for (int k = 0; k < 3; ++k) q[k] = A.old_prims[3 * (size_t)slot + k];
        q[0].w = ibits((int)j);
    }
    for (int k = 0; k < 2; ++k) A.shade[2 * (size_t)j + k] = s[k];
    A.cen[j] = c;
    for (int k = 0; k < 2; ++k) A.box[2 * (size_t)j + k] = b[k];
    for (int k = 0; k < 3; ++k) A.prims[3 * (size_t)j + k] = q[k];
    A.ident[j] = j;
}

}  // namespace rt
