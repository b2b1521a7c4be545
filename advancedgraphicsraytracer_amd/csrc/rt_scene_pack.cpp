// rt_scene_pack.cpp -- scene creation up to the upload: a description in, every device record out
// (ScenePack, rt_internal.h).  No HIP call and no environment variable, so the bit-critical packing
// runs and is checked without a device (tests/cpp/scene_pack_host.cpp); rt_device.hip uploads the
// result.  The record layouts are in rt_device.hip's header comment, their encoders in rt_records.h.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "rt_internal.h"
#include "rt_records.h"
#include "rt_refit.h"

namespace rt {

// LDS stack entries per lane: a traversal pushes at most one entry per tree level, so the tree
// depth is enough.  Rounding it up to 8 cost occupancy where the stacks bound the workgroups
// per CU (mig29 x16: 26 levels, 32 KB per workgroup -> 5 per CU; exact: 26 KB -> 6): CFG3-sub
// 1.79 -> 1.65 ms, CFG5-sub 7.58 -> 7.47 ms, mig29 x16 0.330 -> 0.321 ms, TEAPOT-F unchanged
// (round 3, profiles/r03/ab_stack/).
#ifndef RT_STACK_ROUND
#define RT_STACK_ROUND 1u
#endif
uint32_t pick_stack(uint32_t depth) {   // entries needed <= tree depth (rounded up to RT_STACK_ROUND)
    uint32_t need = depth < 2 ? 2 : depth;
    return (need + RT_STACK_ROUND - 1u) / RT_STACK_ROUND * RT_STACK_ROUND;
}
// trees deeper than 60: the lane stacks (depth x 1 KB) leave no room for the walk's words
bool stack_admits_walk(uint32_t stack_depth) { return (size_t)stack_depth * (256u + 4u) * sizeof(uint32_t) <= kLdsLaunchMax; }
namespace {

// Two-level node records (the path tracer's lane kernel, k_pt_lanes<.., true>): one 128-B
// record per interior node x at even depth (the root at 0) holding the node entries of x's
// grandchildren -- slots 2h, 2h+1 = the children of x's child h -- or, for a leaf child h, that
// leaf's own entry in slot 2h (flag bit 0 in its .w word).  One load then serves two binary
// levels: the walk tests x's children on boxes rebuilt as the union of their children's (the
// reference's node bounds ARE that union -- each node's box is the min / max over its primitives'
// bounds, Scene::UpdateNodeBounds, template/scene.h:855-865 -- checked bit for bit here), then
// the nearer child's children on their own entries, in the reference's order and against the
// same r.t: the visits are the binary walk's exactly.  A popped odd-depth child is addressed by
// (its parent's record, half) and reads its children pair from that record.  Entry words: leaf
// (node_word) as in the binary array, even-depth interior node (record << 8), odd
// marker ((kQuadOdd | record << 1 | half) << 8).  false (no records) when a box is NaN, a parent is
// not the exact union of its children (a caller's prebuilt tree), or the tree is too large.
constexpr uint32_t kQuadOdd = 1u << 23;
bool build_quads(const Bvh &b, const TreeWalk &w, const std::vector<uint8_t> &sticky, std::vector<float4> &rec,
                 uint32_t &root_word) {
    const Node *N = b.nodes.data();
    if (b.nodes_used < 3 || N[0].count > 0) return false;
    std::vector<int32_t> id(b.nodes_used, -1);
    std::vector<uint32_t> order;
    for (uint32_t k : w.order)   // pre-order, even-depth interior nodes numbered as met
        if (N[k].count == 0 && !(w.depth[k] & 1u)) { id[k] = (int32_t)order.size(); order.push_back(k); }
    if (order.size() >= (kQuadOdd >> 1)) return false;
    // the union of two floats as the device's fminf / fmaxf gives it, or fail on NaN / +-0 ties
    auto pick = [&](float a, float c, bool mn, float want) {
        if (a != a || c != c || want != want) return false;
        if (a == c && fbits(a) != fbits(c)) return false;
        const float u = mn ? (a < c ? a : c) : (a > c ? a : c);
        return fbits(u) == fbits(want);
    };
    auto entry = [&](uint32_t g, float4 *q) {
        const Node &nd = N[g];
        const uint32_t word = nd.count > 0 ? node_word(nd.leftFirst, nd.count) : ((uint32_t)id[g] << 8);
        node_pack(mk(nd.mn[0], nd.mn[1], nd.mn[2]), mk(nd.mx[0], nd.mx[1], nd.mx[2]), word, 0.0f, q);
    };
    // the .w word of each entry: bit 0 (first slot of a half) the child is a leaf and this its entry,
    // bit 1 this entry's node is sticky (mark_sticky), bit 2 (first slot) the child itself is sticky
    rec.assign(8 * order.size(), make_float4(0, 0, 0, 0));
    for (size_t r = 0; r < order.size(); ++r) {
        const Node &x = N[order[r]];
        for (uint32_t h = 0; h < 2; ++h) {
            const uint32_t c = x.leftFirst + h;
            float4 *q = &rec[8 * r + 4 * h];
            const Node &cn = N[c];
            const uint32_t sc = sticky[c] ? 6u : 0u;
            if (cn.count > 0) {
                entry(c, q);
                q[1].w = ubits(1u | sc);
                continue;
            }
            const Node &g1 = N[cn.leftFirst], &g2 = N[cn.leftFirst + 1];
            for (int a = 0; a < 3; ++a)
                if (!pick(g1.mn[a], g2.mn[a], true, cn.mn[a]) || !pick(g1.mx[a], g2.mx[a], false, cn.mx[a])) return false;
            entry(cn.leftFirst, q);
            entry(cn.leftFirst + 1, q + 2);
            q[1].w = ubits((sticky[cn.leftFirst] ? 2u : 0u) | (sc & 4u));
            q[3].w = ubits(sticky[cn.leftFirst + 1] ? 2u : 0u);
        }
    }
    root_word = (uint32_t)id[0] << 8;
    return true;
}

int material_flag(const rt_material &m, float diffuse, float specular) {   // getFlag overrides
    switch (m.kind) {
    case RT_DIFFUSE: return F_DIFFUSE;
    case RT_MIRROR: return F_SPECULAR;
    case RT_DIELECTRIC: return F_DIELECTRIC;
    case RT_LIGHT: return F_LIGHT;
    default:
        if (diffuse < kFLT_EPSILON) return F_SPECULAR;
        if (specular < kFLT_EPSILON) return F_DIFFUSE;
        return F_MIX;
    }
}

constexpr uint32_t kMaxNodes = 1u << 24;   // the packed word's leftFirst field is 24 bits wide

// a caller's prebuilt tree: the indices a permutation, the walk in range, child pairs even
int validate_bvh(const Bvh &b, uint32_t n, TreeWalk &w) {
    if (b.nodes_used < 2 || b.nodes_used > b.nodes.size()) return fail(RT_ERR_INVALID, "BVH node count out of range");
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        if (b.indices[i] >= n || seen[b.indices[i]]) return fail(RT_ERR_INVALID, "BVH indices are not a permutation");
        seen[b.indices[i]] = 1;
    }
    switch (walk_tree(b.nodes.data(), b.nodes_used, n, w)) {
    case kTreeCycle: return fail(RT_ERR_INVALID, "BVH has a cycle");
    case kTreeLeafRange: return fail(RT_ERR_INVALID, "BVH leaf outside the index array");
    case kTreeChildRange: return fail(RT_ERR_INVALID, "BVH child pair out of range / misaligned");
    }
    for (uint32_t k : w.order)
        if (b.nodes[k].count == 0 && (b.nodes[k].leftFirst & 1u))
            return fail(RT_ERR_INVALID, "BVH child pair out of range / misaligned");
    return RT_OK;
}

inline const float *transform_of(const rt_scene_desc *d, uint32_t id) {
    return d->transforms ? d->transforms + 16 * (size_t)id : nullptr;
}

// ---------------------------------------------------------------- the steps of pack_scene, in order

int check_description(const rt_scene_desc *d, ScenePack &s) {
    if (!d || !d->prims || d->num_prims == 0 || !d->materials || d->num_materials == 0)
        return fail(RT_ERR_INVALID, "rt_scene_create: empty or null description");
    const uint32_t n = d->num_prims;
    if (n >= (1u << 24)) return fail(RT_ERR_UNSUPPORTED, "more than 2^24 primitives");
    for (uint32_t i = 0; i < n; ++i) {
        const rt_prim &p = d->prims[i];
        if (p.type < RT_SPHERE || p.type > RT_TRIANGLE)
            return fail(RT_ERR_INVALID, "primitive " + std::to_string(i) + ": unknown type");
        if (p.material < 0 || (uint32_t)p.material >= d->num_materials)
            return fail(RT_ERR_INVALID, "primitive " + std::to_string(i) + ": material out of range");
    }
    if (d->prims[0].type != RT_SPHERE && d->prims[0].type != RT_QUAD)
        return fail(RT_ERR_UNSUPPORTED, "primitive 0 must be the light, a sphere or a quad (Scene::GetRandomLight returns 0)");
    for (uint32_t i = 0; i < d->num_materials; ++i) {
        const rt_material &m = d->materials[i];
        if (m.kind < RT_DIFFUSE || m.kind > RT_TEXTURE) return fail(RT_ERR_INVALID, "unknown material kind");
        if (m.kind == RT_TEXTURE && (m.texture < 0 || (uint32_t)m.texture >= d->num_textures || !d->textures))
            return fail(RT_ERR_INVALID, "material " + std::to_string(i) + ": texture index out of range");
    }
    for (uint32_t i = 0; i < d->num_textures; ++i)
        if (!d->textures[i].pixels || !d->textures[i].width || !d->textures[i].height)
            return fail(RT_ERR_INVALID, "texture " + std::to_string(i) + " is empty");
    // needs the kext kernels: cubes, quads, textures, a light material other than the core four
    s.ext_fixed = family_fixed(d->materials, d->num_materials, d->prims[0].material);
    kernel_family(n, [d](uint32_t i) { return d->prims[i].type; }, s.ext_fixed, s.ext, s.has_cubes);
    if (d->sky_pixels) {
        uint32_t w = d->sky_width, h = d->sky_height;
        if (!w || !h || (w & (w - 1)) || (h & (h - 1)))
            return fail(RT_ERR_INVALID, "sky texture must have power-of-two sides (renderer.h:18)");
    }
    // interior nodes store a node index in the 24-bit leftFirst field of the packed device
    // word (node_word): trees with more than 2^24 nodes cannot be addressed
    if (d->bvh_nodes && d->bvh_num_nodes > kMaxNodes)
        return fail(RT_ERR_UNSUPPORTED, "prebuilt BVH with more than 2^24 nodes (24-bit child index)");
    if (d->bvh_kind != RT_BVH_PLAIN && d->bvh_kind != RT_BVH_SBVH) return fail(RT_ERR_INVALID, "unknown bvh_kind");
    return RT_OK;
}

// the tree: prebuilt (validated; depth and widest leaf measured) or built here, and its walk
int take_tree(const rt_scene_desc *d, const PackOptions &o, ScenePack &s, TreeWalk &w) {
    const uint32_t n = d->num_prims;
    Bvh &b = s.bvh;
    int rc;
    if (d->bvh_nodes) {
        if (!d->bvh_indices || d->bvh_num_nodes < 2) return fail(RT_ERR_INVALID, "prebuilt BVH incomplete");
        b.nodes.resize(d->bvh_num_nodes);
        std::memcpy(b.nodes.data(), d->bvh_nodes, sizeof(Node) * d->bvh_num_nodes);
        b.indices.assign(d->bvh_indices, d->bvh_indices + n);
        b.nodes_used = d->bvh_num_nodes;
        if ((rc = validate_bvh(b, n, w)) != RT_OK) return rc;
        // depth as Scene::maxDepthBVH (template/scene.h:144-154): interior levels, root leaf = 1
        b.max_leaf = w.max_leaf;
        for (uint32_t k : w.order)
            if (b.nodes[k].count > 0) b.depth = std::max(b.depth, k == 0 ? 1u : w.depth[k]);
    } else {
        // the option picks the tree only where the caller left the default
        const int kind = d->bvh_kind == RT_BVH_PLAIN ? o.bvh_kind : d->bvh_kind;
        if ((rc = (kind == RT_BVH_SBVH ? build_sbvh : build_bvh)(d->prims, d->transforms, n, b)) != RT_OK) return rc;
        if (walk_tree(b.nodes.data(), b.nodes_used, b.indices.size(), w) != kTreeOk)
            return fail(RT_ERR_INVALID, "the builder's tree does not walk");
    }
    if (b.nodes_used > kMaxNodes) return fail(RT_ERR_UNSUPPORTED, "BVH with more than 2^24 nodes (24-bit child index)");
    if (b.max_leaf > 255) return fail(RT_ERR_UNSUPPORTED, "BVH leaf with more than 255 primitives");
    if (b.depth > 64) return fail(RT_ERR_UNSUPPORTED, "BVH deeper than 64 (the reference's stack[64])");
    s.stack_depth = pick_stack(b.depth);
    s.walk_fits = stack_admits_walk(s.stack_depth);
    return RT_OK;
}

// The wave camera walk's sticky boxes (rt_kernels.inc, wave_closest_hit_fast): a node with a
// primitive below it whose computed t can lie well before its leaf box's entry -- a sliver
// triangle (tri_sliver: its smallest corner angle's sine under 2^RT_WALK_STICKY, default 2^-8), a
// sphere (t = -b - sqrt(d) near a tangent, Primitive.h:150-177) or a quad -- is sticky, and so is
// every ancestor; the walk culls it only on a slab miss (walk_word).  prim_flag: per primitive.
void mark_sticky(const Bvh &b, const TreeWalk &w, const rt_scene_desc *d, const PackOptions &o,
                 std::vector<uint8_t> &sticky, std::vector<uint8_t> &prim_flag) {
    prim_flag.resize(d->num_prims);
    for (uint32_t i = 0; i < d->num_prims; ++i) {
        const rt_prim &p = d->prims[i];
        // planes and cubes never: a plane's box is unbounded and entered from inside
        if (p.type == RT_SPHERE || p.type == RT_QUAD) prim_flag[i] = o.sticky_spheres;
        else prim_flag[i] = p.type == RT_TRIANGLE && tri_sliver(p.v, o.sliver_lim);
    }
    sticky.assign(b.nodes_used, 0);
    for (uint32_t i : w.order) {
        const Node &nd = b.nodes[i];
        bool st = false;
        for (uint32_t k = nd.leftFirst; k < nd.leftFirst + nd.count && !st; ++k) st = prim_flag[b.indices[k]] != 0;
        for (uint32_t j = i; st && j != ~0u && !sticky[j]; j = w.parent[j]) sticky[j] = 1;
    }
}

// the device node array, and what a refit needs of every primitive
void pack_nodes(const rt_scene_desc *d, const PackOptions &o, const std::vector<uint8_t> &sticky, ScenePack &s) {
    s.nodes.resize(2 * (size_t)s.bvh.nodes_used);
    for (uint32_t i = 0; i < s.bvh.nodes_used; ++i) {
        const Node &nd = s.bvh.nodes[i];
        node_pack(mk(nd.mn[0], nd.mn[1], nd.mn[2]), mk(nd.mx[0], nd.mx[1], nd.mx[2]), node_word(nd.leftFirst, nd.count),
                  walk_word(sticky[i] != 0, o.walk_margin), &s.nodes[2 * (size_t)i]);
    }
    const uint32_t n = d->num_prims;
    s.pbox.resize(6 * (size_t)n);
    s.pcen.resize(3 * (size_t)n);
    s.boxes_finite = true;
    for (uint32_t id = 0; id < n; ++id) {
        PrimX x;
        PrimGeom g;
        prim_transform(d->prims[id], transform_of(d, id), x);
        prim_geometry(d->prims[id], x, g);
        const float bx[6] = {g.bmin.x, g.bmin.y, g.bmin.z, g.bmax.x, g.bmax.y, g.bmax.z};
        for (int c = 0; c < 6; ++c) {
            s.pbox[6 * (size_t)id + c] = bx[c];
            if (!std::isfinite(bx[c])) s.boxes_finite = false;
        }
        s.pcen[3 * (size_t)id] = g.centroid.x; s.pcen[3 * (size_t)id + 1] = g.centroid.y; s.pcen[3 * (size_t)id + 2] = g.centroid.z;
        s.pinfo[id] = (uint8_t)(d->prims[id].type | (s.pinfo[id] ? 0x80 : 0));
    }
}

// cubes and quads keep their matrices and data in a side table (8 float4 each); xindex: per id
void pack_xprims(const rt_scene_desc *d, ScenePack &s, std::vector<uint32_t> &xindex) {
    std::vector<float4> &xprims = s.xprims;
    xindex.assign(d->num_prims, 0);
    for (uint32_t id = 0; id < d->num_prims; ++id) {
        const rt_prim &p = d->prims[id];
        if (p.type != RT_CUBE && p.type != RT_QUAD) continue;   // has_cubes: kernel_family's (check_description)
        PrimX x;
        prim_transform(p, transform_of(d, id), x);
        xindex[id] = (uint32_t)(xprims.size() / 8);
        xprims.resize(xprims.size() + 8);
        prim_xentry(p, x, &xprims[8 * (size_t)xindex[id]]);
    }
}

// per-id shading records
void pack_shade(const rt_scene_desc *d, const std::vector<uint32_t> &xindex, ScenePack &s) {
    s.shade.resize(2 * (size_t)d->num_prims);
    PrimX x{};
    for (uint32_t id = 0; id < d->num_prims; ++id) {
        const rt_prim &p = d->prims[id];
        if (p.type != RT_TRIANGLE) prim_transform(p, transform_of(d, id), x);   // a triangle's is the identity, unread
        prim_shade(p, x, xindex[id], &s.shade[2 * (size_t)id]);
    }
}

// leaf-order primitive records (an SBVH repeats primitives)
void pack_slots(const rt_scene_desc *d, const std::vector<uint32_t> &xindex, ScenePack &s) {
    const uint32_t nrefs = (uint32_t)s.bvh.indices.size();
    s.prims.resize(3 * (size_t)nrefs);
    PrimX x{};
    for (uint32_t k = 0; k < nrefs; ++k) {
        const uint32_t id = s.bvh.indices[k];
        const rt_prim &p = d->prims[id];
        if (p.type != RT_TRIANGLE) prim_transform(p, transform_of(d, id), x);
        prim_record(p, x, id, xindex[id], &s.prims[3 * (size_t)k]);
    }
    if (s.xprims.empty()) s.xprims.push_back(make_float4(0, 0, 0, 0));
}

void pack_materials(const rt_scene_desc *d, ScenePack &s) {
    std::vector<uint32_t> tex_offsets(d->num_textures, 0);   // where each starts in the concatenated texels
    for (uint32_t i = 1; i < d->num_textures; ++i)
        tex_offsets[i] = tex_offsets[i - 1] + d->textures[i - 1].width * d->textures[i - 1].height;
    s.mats.resize(d->num_materials);
    for (uint32_t i = 0; i < d->num_materials; ++i) {
        const rt_material &m = d->materials[i];
        DevMaterial &o = s.mats[i];
        std::memset(&o, 0, sizeof(o));
        o.kind = m.kind;
        for (int c = 0; c < 3; ++c) { o.c0[c] = m.color[c]; o.c1[c] = m.color2[c]; }
        o.ior = m.ior;
        // Checkerboard.h:6-14, TextureMaterial.h:6-17 (short ctor: diffuse 1, specular 0),
        // DSMix.h:6-9 (always clamped): clamp = fmaxf(a, fminf(f, b)), precomp.h:782
        if (m.kind == RT_CHECKERBOARD || m.kind == RT_TEXTURE || m.kind == RT_DSMIX) {
            if (m.diffuse < 0.0f && m.kind != RT_DSMIX) { o.diffuse = 1.0f; o.specular = 0.0f; }
            else { o.diffuse = tmax(0.0f, tmin(m.diffuse, 1.0f)); o.specular = 1.0f - o.diffuse; }
        }
        if (m.kind == RT_TEXTURE) {
            const rt_texture &t = d->textures[m.texture];
            o.tex_off = tex_offsets[m.texture];
            o.tex_w = t.width; o.tex_h = t.height;
        }
        o.flag = material_flag(m, o.diffuse, o.specular);
    }
}

// textures, concatenated, and the sky
void pack_sky_and_textures(const rt_scene_desc *d, ScenePack &s) {
    for (uint32_t i = 0; i < d->num_textures; ++i) {
        const rt_texture &t = d->textures[i];
        s.texels.insert(s.texels.end(), t.pixels, t.pixels + (size_t)t.width * t.height);
    }
    if (s.texels.empty()) s.texels.push_back(0);
    SceneView &v = s.view;
    v.sky_w = 1024; v.sky_h = 512;
    if (d->sky_pixels) {
        v.sky_w = d->sky_width; v.sky_h = d->sky_height;
        s.sky.assign(d->sky_pixels, d->sky_pixels + (size_t)v.sky_w * v.sky_h);
    } else {
        s.sky.assign((size_t)v.sky_w * v.sky_h, 0x406080u);
    }
    const uint32_t p = s.sky[0];
    v.sky_const = std::all_of(s.sky.begin(), s.sky.end(), [&](uint32_t t) { return t == p; }) ? 1 : 0;
    f3 c = mk((float)((p >> 16) & 255), (float)((p >> 8) & 255), (float)(p & 255)) * kSKY;
    v.sky_rgb[0] = c.x; v.sky_rgb[1] = c.y; v.sky_rgb[2] = c.z;
}

void tree_flags(ScenePack &s) {
    const Bvh &b = s.bvh;
    // every child box inside its parent's, compared as floats (the wave walk's pops and its leaf
    // check rely on it: a child's slab entry is then never below its parent's)
    s.nested = true;
    for (uint32_t i = 0; i < b.nodes_used && s.nested; ++i) {
        if (i == 1) continue;
        const Node &nd = b.nodes[i];
        if (nd.count > 0) continue;
        for (uint32_t c = nd.leftFirst; c < nd.leftFirst + 2 && s.nested; ++c) {
            const Node &ch = b.nodes[c];
            for (int a = 0; a < 3; ++a)
                if (!(ch.mn[a] >= nd.mn[a]) || !(ch.mx[a] <= nd.mx[a])) s.nested = false;
        }
    }
    s.view.bounds_finite = 1;
    for (uint32_t i = 0; i < b.nodes_used && s.view.bounds_finite; ++i) {
        if (i == 1) continue;
        const Node &nd = b.nodes[i];
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(nd.mn[c]) || !std::isfinite(nd.mx[c])) s.view.bounds_finite = 0;
    }
}

}  // namespace

int pack_scene(const rt_scene_desc *d, const PackOptions &o, ScenePack &s) {
    s = ScenePack();
    int rc = check_description(d, s);
    if (rc != RT_OK) return rc;
    TreeWalk w;
    if ((rc = take_tree(d, o, s, w)) != RT_OK) return rc;
    std::vector<uint8_t> sticky;
    std::vector<uint32_t> xindex;
    mark_sticky(s.bvh, w, d, o, sticky, s.pinfo);
    pack_nodes(d, o, sticky, s);
    SceneView &v = s.view;
    v.walk_margin = o.walk_margin;
    s.has_quads = o.quads && build_quads(s.bvh, w, sticky, s.quads, v.quad_root);
    pack_xprims(d, s, xindex);
    pack_shade(d, xindex, s);
    pack_slots(d, xindex, s);
    pack_materials(d, s);
    pack_sky_and_textures(d, s);
    fill_light(d->prims[0], transform_of(d, 0), v);
    v.root_word = node_word(s.bvh.nodes[0].leftFirst, s.bvh.nodes[0].count);
    v.stack_entries = s.stack_depth;
    tree_flags(s);
    return RT_OK;
}

// ---------------------------------------------------------------- what an in-place update starts from (rt_refit.h)

bool build_refit_plan(const Bvh &b, uint32_t num_prims, RefitPlan &out) {
    const uint32_t used = b.nodes_used;
    const Node *N = b.nodes.data();
    if (b.indices.size() != num_prims) return false;
    out = RefitPlan();
    out.slot_of.assign(num_prims, ~0u);
    for (uint32_t k = 0; k < num_prims; ++k) {
        const uint32_t id = b.indices[k];
        if (id >= num_prims || out.slot_of[id] != ~0u) return false;
        out.slot_of[id] = k;
    }
    // pre-order from the root; sizes and heights in reverse
    TreeWalk w;
    if (walk_tree(N, used, num_prims, w) != kTreeOk) return false;
    const std::vector<uint32_t> &order = w.order;
    std::vector<uint32_t> size(used, 0), height(used, 0);
    for (size_t i = order.size(); i-- > 0;) {
        const uint32_t k = order[i];
        size[k] = 1;
        if (N[k].count > 0) continue;
        const uint32_t l = N[k].leftFirst;
        size[k] += size[l] + size[l + 1];
        height[k] = 1 + std::max(height[l], height[l + 1]);
    }
    auto by_height = [&](uint32_t x, uint32_t y) { return height[x] < height[y]; };
    auto emit = [&](std::vector<uint32_t> &nodes) {   // one group: its nodes by height, its level boundaries
        std::stable_sort(nodes.begin(), nodes.end(), by_height);
        out.grp.push_back((uint32_t)out.lvl.size());
        for (size_t i = 0; i < nodes.size(); ++i) {
            if (i == 0 || height[nodes[i]] != height[nodes[i - 1]]) out.lvl.push_back((uint32_t)out.list.size());
            out.list.push_back(nodes[i]);
        }
        out.lvl.push_back((uint32_t)out.list.size());
    };
    std::vector<uint32_t> top, sub;
    for (size_t i = 0; i < order.size(); ++i) {   // pre-order: a treelet's size[k] nodes start at its root
        const uint32_t k = order[i];
        if (size[k] > kTreeletNodes) { top.push_back(k); continue; }
        if (k != 0 && size[w.parent[k]] <= kTreeletNodes) continue;   // inside a treelet
        sub.assign(order.begin() + i, order.begin() + i + size[k]);
        emit(sub);
        ++out.ntreelets;
    }
    out.has_top = !top.empty();
    emit(top);
    out.grp.push_back((uint32_t)out.lvl.size());
    return true;
}

void seed_slot_boxes(const Bvh &b, const std::vector<uint8_t> &pinfo, const std::vector<float> &pbox, std::vector<float4> &out) {
    out.resize(2 * b.indices.size());
    for (size_t k = 0; k < b.indices.size(); ++k) {
        const uint32_t id = b.indices[k];
        const float *x = &pbox[6 * (size_t)id];
        slot_box(mk(x[0], x[1], x[2]), mk(x[3], x[4], x[5]), (pinfo[id] & 0x80) != 0, &out[2 * k]);
    }
}

}  // namespace rt

// build_refit_plan through the C-ABI: the definition the device schedule (rt_plan.h) is compared with
extern "C" int rt_bvh_refit_plan_host(const void *nodes, uint32_t nodes_used, const uint32_t *indices, uint32_t n,
                                      uint32_t **list, uint32_t **lvl, uint32_t **grp, uint32_t counts[4]) {
    using namespace rt;
    if (!nodes || !indices || !list || !lvl || !grp || !counts || n == 0 || nodes_used < 2)
        return fail(RT_ERR_INVALID, "rt_bvh_refit_plan_host: null or empty argument");
    *list = *lvl = *grp = nullptr;
    try {
        Bvh b;
        b.nodes.resize(nodes_used);
        std::memcpy(b.nodes.data(), nodes, sizeof(Node) * nodes_used);
        b.indices.assign(indices, indices + n);
        b.nodes_used = nodes_used;
        RefitPlan p;
        if (!build_refit_plan(b, n, p)) return fail(RT_ERR_UNSUPPORTED, "rt_bvh_refit_plan_host: not a plain tree");
        uint32_t **dst[3] = {list, lvl, grp};
        const std::vector<uint32_t> *src[3] = {&p.list, &p.lvl, &p.grp};
        for (int k = 0; k < 3; ++k) {
            *dst[k] = static_cast<uint32_t *>(std::malloc(sizeof(uint32_t) * std::max<size_t>(1, src[k]->size())));
            if (!*dst[k]) {
                for (int j = 0; j < k; ++j) { std::free(*dst[j]); *dst[j] = nullptr; }
                return fail(RT_ERR_INVALID, "rt_bvh_refit_plan_host: out of memory");
            }
            std::memcpy(*dst[k], src[k]->data(), sizeof(uint32_t) * src[k]->size());
        }
        counts[0] = (uint32_t)p.list.size();
        counts[1] = (uint32_t)p.lvl.size();
        counts[2] = p.ntreelets;
        counts[3] = p.has_top ? 1u : 0u;
        return RT_OK;
    } catch (const std::exception &e) {
        return fail(RT_ERR_INVALID, std::string("rt_bvh_refit_plan_host: ") + e.what());
    }
}
