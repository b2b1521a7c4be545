// rt_records.h -- the encoders of the device scene records whose bits the frames depend on.
//
// One definition each, compiled from the same text for the host (rt_scene_pack.cpp at scene
// creation, rt_host.cpp) and for gfx950 (the update kernels of rt_refit.hip, through rt_update.h), under the same
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

// ---- mat4, row-major, translation in column 3 (template/precomp.h:1007-1085)
RT_HD void mat4_identity(float M[16]) {
    for (int i = 0; i < 16; ++i) M[i] = (i % 5 == 0) ? 1.0f : 0.0f;
}
RT_HD void mat4_translate(float x, float y, float z, float M[16]) {
    mat4_identity(M);
    M[3] = x; M[7] = y; M[11] = z;
}
RT_HD void mat4_mul(const float *a, const float *b, float *out) {   // out may alias a or b
    float r[16];
    for (int i = 0; i < 16; i += 4)
        for (int j = 0; j < 4; ++j)
            r[i + j] = (a[i + 0] * b[j + 0]) + (a[i + 1] * b[j + 4]) + (a[i + 2] * b[j + 8]) + (a[i + 3] * b[j + 12]);
    for (int i = 0; i < 16; ++i) out[i] = r[i];
}
// mat4::FastInvertedTransformNoScale (template/precomp.h:1061-1085)
RT_HD void fast_inverse(const float *c, float *r) {
    mat4_identity(r);
    r[0] = c[0], r[1] = c[4], r[2] = c[8];
    r[4] = c[1], r[5] = c[5], r[6] = c[9];
    r[8] = c[2], r[9] = c[6], r[10] = c[10];
    r[3] = -(c[3] * r[0] + c[7] * r[1] + c[11] * r[2]);
    r[7] = -(c[3] * r[4] + c[7] * r[5] + c[11] * r[6]);
    r[11] = -(c[3] * r[8] + c[7] * r[9] + c[11] * r[10]);
}

// ---- every primitive kind.  Primitive::Transform and InvertedTransform (Primitive.h:28-29, 39-41):
// Translate(centre) for spheres, T * Translate(pos) (|pos| > FLT_EPSILON) or T for cubes, T for
// quads, identity otherwise.  T16 = the caller's mat4 (null = identity).
struct PrimX { float M[16], Minv[16]; };
RT_HD void prim_transform(const rt_prim &p, const float *T16, PrimX &x) {
    float T[16];
    if (T16) for (int i = 0; i < 16; ++i) T[i] = T16[i];
    else mat4_identity(T);
    if (p.type == RT_SPHERE) {
        mat4_translate(p.v[0], p.v[1], p.v[2], x.M);                 // createSphere, Primitive.h:690-698
    } else if (p.type == RT_CUBE) {                                   // createCube, Primitive.h:717-728
        const f3 pos = mk(p.v[0], p.v[1], p.v[2]);
        if (length(pos) > kFLT_EPSILON) {
            float Tr[16];
            mat4_translate(pos.x, pos.y, pos.z, Tr);
            mat4_mul(T, Tr, x.M);
        } else {
            for (int i = 0; i < 16; ++i) x.M[i] = T[i];
        }
    } else if (p.type == RT_QUAD) {
        for (int i = 0; i < 16; ++i) x.M[i] = T[i];
    } else {
        mat4_identity(x.M);
    }
    fast_inverse(x.M, x.Minv);
}

// the 8 cube corners / 4 quad corners in GetAABBMin/Max's order (Primitive.h:325-341)
RT_HD int box_corners(const rt_prim &p, const PrimX &x, f3 *c) {
    if (p.type == RT_CUBE) {
        const f3 a = -0.5f * mk(p.v[3], p.v[4], p.v[5]), b = 0.5f * mk(p.v[3], p.v[4], p.v[5]);
        c[0] = tpos(x.M, a);
        c[1] = tpos(x.M, mk(b.x, a.y, a.z));
        c[2] = tpos(x.M, mk(a.x, b.y, a.z));
        c[3] = tpos(x.M, mk(a.x, a.y, b.z));
        c[4] = tpos(x.M, b);
        c[5] = tpos(x.M, mk(a.x, b.y, b.z));
        c[6] = tpos(x.M, mk(b.x, a.y, b.z));
        c[7] = tpos(x.M, mk(b.x, b.y, a.z));
        return 8;
    }
    const float sz = 0.5f * p.v[0];
    c[0] = tpos(x.M, mk(-sz, 0, -sz));
    c[1] = tpos(x.M, mk(-sz, 0, sz));
    c[2] = tpos(x.M, mk(sz, 0, -sz));
    c[3] = tpos(x.M, mk(sz, 0, sz));
    return 4;
}

// Per-primitive geometry the builder, the uploader and the refit need, evaluated exactly as
// Primitive::GetCentroid / GetAABBMin / GetAABBMax (Primitive.h:42-50, 319-388, 443-445).
struct PrimGeom { f3 centroid, bmin, bmax; };
RT_HD void prim_geometry(const rt_prim &p, const PrimX &x, PrimGeom &g) {
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    if (p.type == RT_CUBE || p.type == RT_QUAD) {
        f3 c[8];
        const int n = box_corners(p, x, c);
        g.centroid = tpos(x.M, mk(0, 0, 0));                      // ctor leaves centroid 0
        g.bmin = g.bmax = c[0];
        for (int i = 1; i < n; ++i) { g.bmin = fmin3(g.bmin, c[i]); g.bmax = fmax3(g.bmax, c[i]); }
    } else if (p.type == RT_SPHERE) {
        f3 c = tpos(x.M, mk(0, 0, 0));
        float r = p.v[3];
        g.centroid = c;                       // centroid float3(0) through Transform
        g.bmin = c - mk(r, r, r);
        g.bmax = c + mk(r, r, r);
    } else if (p.type == RT_PLANE) {
        f3 n = mk(p.v[0], p.v[1], p.v[2]);
        g.centroid = tpos(I, (-n) * p.v[3]);
        g.bmin = mk(-1e30f, -1e30f, -1e30f);
        g.bmax = mk(1e30f, 1e30f, 1e30f);
    } else {
        f3 d0 = mk(p.v[0], p.v[1], p.v[2]), d1 = mk(p.v[3], p.v[4], p.v[5]), d2 = mk(p.v[6], p.v[7], p.v[8]);
        g.centroid = tpos(I, ((d0 + d1) + d2) / 3.0f);
        tri_box(p.v, g.bmin, g.bmax);
    }
}

// side-table entry of a cube or a quad, 8 float4: Minv rows 0..2, M rows 0..2, data[0], data[1]
RT_HD void prim_xentry(const rt_prim &p, const PrimX &x, float4 e[8]) {
    for (int r = 0; r < 3; ++r) e[r] = make_float4(x.Minv[4 * r], x.Minv[4 * r + 1], x.Minv[4 * r + 2], x.Minv[4 * r + 3]);
    for (int r = 0; r < 3; ++r) e[3 + r] = make_float4(x.M[4 * r], x.M[4 * r + 1], x.M[4 * r + 2], x.M[4 * r + 3]);
    if (p.type == RT_CUBE) {   // data[0] = -0.5 size, data[1] = 0.5 size (Primitive.h:724-725)
        const f3 sz = mk(p.v[3], p.v[4], p.v[5]), a = -0.5f * sz, b = 0.5f * sz;
        e[6] = make_float4(a.x, a.y, a.z, 0.0f);
        e[7] = make_float4(b.x, b.y, b.z, 0.0f);
    } else {                   // data[0].x = 0.5 size (Primitive.h:737)
        e[6] = make_float4(0.5f * p.v[0], 0.0f, 0.0f, 0.0f);
        e[7] = make_float4(0, 0, 0, 0);
    }
}
// shading record of any primitive, 2 float4: (normal / centre | material), (type, 1 / r, side-table
// entry, 0).  xi = the side-table entry of a cube or a quad (else unused).
RT_HD void prim_shade(const rt_prim &p, const PrimX &x, uint32_t xi, float4 s[2]) {
    s[1] = make_float4(ubits((uint32_t)p.type), 0, 0, 0);
    if (p.type == RT_CUBE || p.type == RT_QUAD) {
        // quad: constant normal TransformVector((0,-1,0), Transform) (Primitive.h:306-307)
        const f3 N = p.type == RT_QUAD ? tvec(x.M, mk(0, -1, 0)) : mk(0, 0, 0);
        s[0] = make_float4(N.x, N.y, N.z, ibits(p.material));
        s[1].z = ubits(xi);
    } else if (p.type == RT_TRIANGLE) {
        const f3 N = tri_normal(p.v);
        s[0] = make_float4(N.x, N.y, N.z, ibits(p.material));
    } else if (p.type == RT_SPHERE) {
        const f3 c = tpos(x.M, mk(0, 0, 0));
        s[0] = make_float4(c.x, c.y, c.z, ibits(p.material));
        s[1].y = 1.0f / p.v[3];                                      // data[0].z
    } else {
        s[0] = make_float4(p.v[0], p.v[1], p.v[2], ibits(p.material));
    }
}
// leaf-slot record of any primitive, 3 float4
RT_HD void prim_record(const rt_prim &p, const PrimX &x, uint32_t id, uint32_t xi, float4 q[3]) {
    if (p.type == RT_TRIANGLE) {
        tri_record(p.v, id, q);
        return;
    }
    q[2] = make_float4(0, 0, 0, 0);
    if (p.type == RT_SPHERE) {
        const f3 c = tpos(x.M, mk(0, 0, 0));
        const float r = p.v[3];
        q[0] = make_float4(c.x, c.y, c.z, ibits((int)id));
        q[1] = make_float4(r * r, 0.0f, 0.0f, ubits(T_SPH));   // data[0].y
    } else if (p.type == RT_PLANE) {
        q[0] = make_float4(p.v[0], p.v[1], p.v[2], ibits((int)id));
        q[1] = make_float4(p.v[3], 0.0f, 0.0f, ubits(T_PLANE));
    } else {
        q[0] = make_float4(0, 0, 0, ibits((int)id));
        q[1] = make_float4(ubits(xi), 0.0f, 0.0f, ubits(p.type == RT_CUBE ? T_CUBE : T_QUAD));
    }
}
// the light's SceneView fields from primitive 0 and its transform (Scene::GetRandomLight returns 0)
RT_HD void fill_light(const rt_prim &L, const float *T16, SceneView &v) {
    PrimX LX;
    prim_transform(L, T16, LX);
    for (int i = 0; i < 12; ++i) v.light_M[i] = LX.M[i];
    const f3 lc = tpos(LX.M, mk(0, 0, 0));
    v.light_c[0] = lc.x; v.light_c[1] = lc.y; v.light_c[2] = lc.z;
    v.light_mat = L.material;
    v.light_quad = L.type == RT_QUAD;
    if (v.light_quad) {
        v.light_qsize = 0.5f * L.v[0];
        const float side = 2.0f * v.light_qsize;                      // GetArea, Primitive.h:461-463
        v.light_area = side * side;
        const f3 N = tvec(LX.M, mk(0, -1, 0));
        v.light_N[0] = N.x; v.light_N[1] = N.y; v.light_N[2] = N.z;
    } else {
        v.light_r = L.v[3];
        v.light_r2 = L.v[3] * L.v[3];
        v.light_invr = 1.0f / L.v[3];
        v.light_area = 4.0f * kPI * v.light_r2;                        // Primitive.h:452
    }
}

// ---- the refit's per-slot box: (box min, sticky flag 0 / 1), (box max, 0)
RT_HD void slot_box(f3 mn, f3 mx, bool sticky, float4 out[2]) {
    out[0] = make_float4(mn.x, mn.y, mn.z, ubits(sticky ? 1u : 0u));
    out[1] = make_float4(mx.x, mx.y, mx.z, 0.0f);
}
RT_HD bool slot_sticky(float4 lo) { return fbits(lo.w) != 0u; }

}  // namespace rt
