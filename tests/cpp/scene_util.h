// Small scenes and their helpers for the stand-alone programs build_host.cpp, splice_host.cpp and
// update_host.cpp: three materials, primitive records, the KAT scene, a seeded generator, pack_scene
// over vectors, a pack's centroids as the device keeps them, the twist of the timing tools.
#pragma once
#include <cmath>
#include <initializer_list>
#include <vector>

#include "rt_internal.h"

inline rt_material material(int kind) {
    rt_material m{};
    m.kind = kind;
    m.color[0] = m.color[1] = m.color[2] = 0.8f;
    m.diffuse = -1.0f;
    return m;
}
inline const std::vector<rt_material> kMats = {material(RT_LIGHT), material(RT_DIFFUSE), material(RT_MIRROR)};
inline rt_prim sphere(float x, float y, float z, float r, int mat) { return rt_prim{RT_SPHERE, mat, {x, y, z, r}}; }
inline rt_prim tri(std::initializer_list<float> v, int mat) {
    rt_prim p{RT_TRIANGLE, mat, {}};
    int k = 0;
    for (float f : v) p.v[k++] = f;
    return p;
}
// tests/scenes_util.py kat_scene: every kind but cube and quad, a plane's +-1e30 box
inline std::vector<rt_prim> kat_prims() {
    return {sphere(0, 4, -2, 0.5f, 0), tri({0, 0, 5, 1, 0, 5, 0, 1, 5}, 1), tri({1, 0, 5, 1, 1, 5, 0, 1, 5}, 1),
            tri({-2, -1, 7, -1, -1, 7, -2, 0, 7}, 1), tri({-2, -1, 7, -1, -1, 7, -2, 0, 7}, 2), sphere(3, 0, 5, 1.0f, 2),
            sphere(-3, 2, 5, 0.25f, 1), rt_prim{RT_PLANE, 1, {0, 1, 0, 2.0f}}};
}

inline uint32_t lcg(uint32_t &s) { s = s * 1664525u + 1013904223u; return s >> 8; }
inline float unit(uint32_t &s) { return (float)(lcg(s) & 0xffffu) / 65536.0f; }

inline int pack(const std::vector<rt_prim> &p, const std::vector<rt_material> &m, const float *T, const rt::Bvh *tree, rt::ScenePack &out) {
    rt_scene_desc d{};
    d.prims = p.data(); d.num_prims = (uint32_t)p.size();
    d.materials = m.data(); d.num_materials = (uint32_t)m.size();
    d.transforms = T;
    if (tree) { d.bvh_nodes = tree->nodes.data(); d.bvh_num_nodes = tree->nodes_used; d.bvh_indices = tree->indices.data(); }
    return rt::pack_scene(&d, rt::PackOptions(), out);
}
inline std::vector<float4> centroids(const rt::ScenePack &p) {
    std::vector<float4> c(p.pcen.size() / 3);
    for (size_t i = 0; i < c.size(); ++i) c[i] = make_float4(p.pcen[3 * i], p.pcen[3 * i + 1], p.pcen[3 * i + 2], 0.0f);
    return c;
}

// twist about y by k radians per unit of y (tests/refit_util.py, tools/refit_time.py)
inline void twist(const float in[9], float k, float out[9]) {
    for (int v = 0; v < 3; ++v) {
        const double x = in[3 * v], y = in[3 * v + 1], z = in[3 * v + 2], a = (double)k * y, c = std::cos(a), s = std::sin(a);
        out[3 * v] = (float)(c * x - s * z);
        out[3 * v + 1] = (float)y;
        out[3 * v + 2] = (float)(s * x + c * z);
    }
}
