// rt_records.h -- the encoders of the device scene records whose bits the frames depend on.
//
// One definition each, compiled from the same text for the host (rt_scene_pack.cpp at scene
// creation, rt_host.cpp) and for gfx950 (the refit kernels of rt_refit.hip), under the same
// -ffp-contract=off: a scene updated in place equals a freshly created one bit for bit
// because both run these functions.  Built on rt_math.h and the HIP vector types (rt_dev_types.h
// for the T_* tags); no std:: algorithm, so a plain host program compiles it too
// (tests/cpp/scene_pack_host.cpp).
#pragma once
#include "rt_dev_types.h"
#include "rt_math.h"

namespace rt {

RT_HD float ubits(uint32_t u) { float f; __builtin_memcpy(&f, &u, 4); return f; }
RT_HD float ibits(int32_t i) { float f; __builtin_memcpy(&f, &i, 4); return f; }
RT_HD uint32_t fbits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }

// ---- nodes.  A node is two float4: (mn.xyz, mx.x), (mx.y, mx.z, word, walk word) -- the
// reference's 32-byte BVHNode (BVHNode.h:5-14) with (leftFirst, count) folded into one word, so a
// 64-byte sibling-pair load carries everything a traversal needs.  The child index has 24 bits.
RT_HD uint32_t node_word(uint32_t leftFirst, uint32_t count) { return (leftFirst << 8) | count; }
RT_HD void node_pack(f3 mn, f3 mx, uint32_t word, float last, float4 out[2]) {
    out[0] = make_float4(mn.x, mn.y, mn.z, mx.x);
    out[1] = make_float4(mx.y, mx.z, ubits(word), last);
}
RT_HD void node_box(float4 a, float4 b, f3 &mn, f3 &mx) {
    mn = mk(a.x, a.y, a.z);
    mx = mk(a.w, b.x, b.y);
}
// The last word of a node is the wave walk's cull margin (SceneView::walk_margin), +inf for a
// sticky node, which the walk then culls only on a slab miss; the lane traversals
// never read it.
RT_HD float walk_word(bool sticky, float margin) { return sticky ? __builtin_huge_valf() : margin; }
RT_HD bool is_sticky(float word) { return word == __builtin_huge_valf(); }

// ---- triangles, v = the nine vertex floats A, B, C.  The identity-matrix tpos / tvec calls are
// part of the reference's evaluation order (Primitive::Transform is the identity for a triangle).
RT_HD f3 tri_vertex(const float v[9], int k) {
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    return tpos(I, mk(v[3 * k], v[3 * k + 1], v[3 * k + 2]));
}
// leaf-slot record (A | id, B-A | T_TRI, C-A): Intersect's per-test subtractions, Primitive.h:249-254
RT_HD void tri_record(const float v[9], uint32_t id, float4 q[3]) {
    const f3 A = tri_vertex(v, 0), AB = tri_vertex(v, 1) - A, AC = tri_vertex(v, 2) - A;
    q[0] = make_float4(A.x, A.y, A.z, ibits((int)id));
    q[1] = make_float4(AB.x, AB.y, AB.z, ubits(T_TRI));
    q[2] = make_float4(AC.x, AC.y, AC.z, 0.0f);
}
// shading normal: the cross product takes C-A before B-A (Primitive.h:308-310)
RT_HD f3 tri_normal(const float v[9]) {
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const f3 d0 = mk(v[0], v[1], v[2]), d1 = mk(v[3], v[4], v[5]), d2 = mk(v[6], v[7], v[8]);
    return tvec(I, normalize(cross(d2 - d0, d1 - d0)));
}
// GetAABBMin / GetAABBMax: min / max of the three transformed vertices (Primitive.h:319-388)
RT_HD void tri_box(const float v[9], f3 &mn, f3 &mx) {
    const f3 A = tri_vertex(v, 0), B = tri_vertex(v, 1), C = tri_vertex(v, 2);
    mn = fmin3(A, fmin3(B, C));
    mx = fmax3(A, fmax3(B, C));
}
// A sliver: the sine of the smallest corner angle, 2 area / (the two longest edges), is under lim
// -- the common denominator of t, u, v is then mostly rounding (Primitive.h:255-273), so the
// triangle's computed t can lie well before its leaf box's entry and its nodes are sticky.  In
// double on the float vertices; a NaN anywhere makes a sliver.
RT_HD bool tri_sliver(const float v[9], double lim) {
    double e[3][3], len[3];
    for (int k = 0; k < 3; ++k) {
        for (int a = 0; a < 3; ++a) e[k][a] = (double)v[3 * ((k + 1) % 3) + a] - (double)v[3 * k + a];
        len[k] = sqrt(e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2]);
    }
    const double cx = e[0][1] * e[2][2] - e[0][2] * e[2][1], cy = e[0][2] * e[2][0] - e[0][0] * e[2][2],
                 cz = e[0][0] * e[2][1] - e[0][1] * e[2][0];
    const double area2 = sqrt(cx * cx + cy * cy + cz * cz);
    // the two longest edges in ascending order: drop the shortest (ties: any, the values are the same)
    double l1, l2;
    if (len[0] <= len[1] && len[0] <= len[2]) { l1 = len[1]; l2 = len[2]; }
    else if (len[1] <= len[0] && len[1] <= len[2]) { l1 = len[0]; l2 = len[2]; }
    else { l1 = len[0]; l2 = len[1]; }
    if (l1 > l2) { const double t = l1; l1 = l2; l2 = t; }
    return !(area2 >= lim * l1 * l2);
}

// ---- the refit's per-slot box: (box min, sticky flag 0 / 1), (box max, 0)
RT_HD void slot_box(f3 mn, f3 mx, bool sticky, float4 out[2]) {
    out[0] = make_float4(mn.x, mn.y, mn.z, ubits(sticky ? 1u : 0u));
    out[1] = make_float4(mx.x, mx.y, mx.z, 0.0f);
}
RT_HD bool slot_sticky(float4 lo) { return fbits(lo.w) != 0u; }

}  // namespace rt
