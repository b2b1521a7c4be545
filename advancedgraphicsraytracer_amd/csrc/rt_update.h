// rt_update.h -- the per-lane text of the in-place updates: what one lane of the
// check, write and refit kernels of rt_refit.hip does, as plain functions over arrays.
//
// One text for gfx950 and for the host, like rt_records.h and under the same -ffp-contract=off:
// the kernels only supply the lane index and the barrier between heights, so a stand-alone host
// program runs check -> write -> refit end to end with tid = 0, stride = 1
// (tests/cpp/update_host.cpp, tests/cpp/prim_records_host.cpp).  No std:: algorithm in what a lane
// runs; the host's making of rt_scene_transform_triangles' range table (xform_table) is marked as such.
//
// A *source* maps lane i of a call to "primitive id + its new geometry":
//   ok(A, i)     would the write of lane i produce a finite, admissible record?  Writes nothing;
//   write(A, i)  the leaf-slot record, the shading record, the slot box (and, for a cube or a quad,
//                the side-table entry) of that primitive.
#pragma once
#include <algorithm>
#include <cstring>
#include <utility>
#include <vector>

#include "rt_records.h"

namespace rt {

struct RefitArgs {
    float4 *nodes, *prims, *shade;   // the scene's records (SceneView)
    float4 *xprims;                  // the side table of cubes and quads
    float4 *slot_box;                // 2 float4 per leaf slot: (box min, sticky flag), (box max, 0)
    const uint32_t *slot_of, *list, *lvl, *grp;   // the refit plan (RefitPlan, rt_refit.h)
    float margin;                    // SceneView::walk_margin
    double sliver_lim;               // mark_sticky's sine limit
    float4 *cen;                     // per primitive id its centroid, what a rebuild bins by (rt_build.h); null: not kept
};

RT_HD bool finite_f(float f) { return (fbits(f) & 0x7f800000u) != 0x7f800000u; }
RT_HD bool finite_f3(f3 a) { return finite_f(a.x) && finite_f(a.y) && finite_f(a.z); }

// ---- triangles from nine world-space floats
RT_HD bool tri_ok(const float w[9]) {
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && finite_f(w[k]);
    return ok;
}
// prim_geometry's triangle centroid
RT_HD float4 tri_centroid(const float w[9]) {
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const f3 c = tpos(I, ((mk(w[0], w[1], w[2]) + mk(w[3], w[4], w[5])) + mk(w[6], w[7], w[8])) / 3.0f);
    return make_float4(c.x, c.y, c.z, 0.0f);
}
// the rt_records.h encoders that scene creation runs, so the records equal those of a fresh
// rt_scene_create on the new vertices; the material word of the shading record stays
RT_HD void write_tri(const RefitArgs &A, uint32_t id, const float w[9]) {
    const uint32_t slot = A.slot_of[id];
    const f3 N = tri_normal(w);
    A.shade[2 * (size_t)id] = make_float4(N.x, N.y, N.z, A.shade[2 * (size_t)id].w);
    tri_record(w, id, A.prims + 3 * (size_t)slot);
    f3 mn, mx;
    tri_box(w, mn, mx);
    slot_box(mn, mx, tri_sliver(w, A.sliver_lim), A.slot_box + 2 * (size_t)slot);
    if (A.cen) A.cen[id] = tri_centroid(w);
}

// rt_scene_update_triangles: triangle first + i from the nine floats at verts + 9 i
struct TriVerts {
    uint32_t first;
    const float *verts;
    RT_HD bool ok(const RefitArgs &, uint32_t i) const { return tri_ok(verts + 9u * (size_t)i); }
    RT_HD void write(const RefitArgs &A, uint32_t i) const { write_tri(A, first + i, verts + 9u * (size_t)i); }
};

// rt_scene_transform_triangles' range table: range r moves triangles
// [first[r], first[r] + pre[r + 1] - pre[r]) by M[16 r ..]; pre[nr] = all triangles of the call
struct XformRanges {
    const uint32_t *first, *pre;
    const float *M;
    uint32_t nr;
};
// Lane i of the back-to-back rest triangles finds its range by binary search over the prefix
// counts (pre[r] = triangles before range r).
RT_HD uint32_t range_of(const uint32_t *pre, uint32_t nr, uint32_t i) {
    uint32_t lo = 0, hi = nr;   // pre[lo] <= i < pre[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
// The host's part of rt_scene_transform_triangles, shared by its blocking and its stream-ordered entry
// point and the stand-alone program: the refusals that need no device, and the table.  Empty ranges are
// dropped; per kept range, in the caller's order: inside the primitives, at most 0xffffffff / 9 triangles
// so far (lane i reads rest[9 i] with 32-bit arithmetic), triangles all (ptype[id] & 0x7f, RefitState::pinfo;
// null: not looked at); then no triangle in two ranges, and the rest vertices last.  *where: the range
// (caller's index) or the primitive refused.  tab = first[nr] | pre[nr + 1] | M[16 nr].
enum { kXformOk = 0, kXformEmpty, kXformRange, kXformMany, kXformKind, kXformOverlap, kXformNullRest };
inline int xform_table(uint32_t num_prims, const uint8_t *ptype, const rt_tri_xform *ranges, uint32_t num_ranges, const void *rest,
                       std::vector<uint32_t> &tab, uint32_t *nr, uint32_t *where) {
    std::vector<uint32_t> kept;   // the non-empty ranges
    std::vector<std::pair<uint32_t, uint32_t>> spans;
    uint64_t total = 0;
    for (uint32_t r = 0; r < num_ranges; ++r) {
        const rt_tri_xform &x = ranges[r];
        if (x.count == 0) continue;
        *where = r;
        if ((uint64_t)x.first + x.count > num_prims) return kXformRange;
        if (total + x.count > 0xffffffffull / 9u) return kXformMany;
        for (uint32_t id = x.first; ptype && id < x.first + x.count; ++id)
            if ((ptype[id] & 0x7f) != RT_TRIANGLE) { *where = id; return kXformKind; }
        kept.push_back(r);
        spans.push_back({x.first, x.count});
        total += x.count;
    }
    if (kept.empty()) return kXformEmpty;
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
        if (spans[k - 1].first + spans[k - 1].second > spans[k].first) return kXformOverlap;
    if (!rest) return kXformNullRest;
    const size_t n = kept.size();
    tab.assign(n + (n + 1) + 16 * n, 0u);
    for (size_t k = 0; k < n; ++k) {
        const rt_tri_xform &x = ranges[kept[k]];
        tab[k] = x.first;
        tab[n + k + 1] = tab[n + k] + x.count;
        std::memcpy(&tab[2 * n + 1 + 16 * k], x.M, sizeof(x.M));
    }
    *nr = (uint32_t)n;
    return kXformOk;
}
struct TriXform {
    XformRanges R;
    const float *rest;   // object-space vertices, 9 floats per lane
    // world vertices = TransformPosition(rest, M) per vertex, as Scene::LoadModel places a mesh
    // (template/scene.h:185-191); returns the triangle's id
    RT_HD uint32_t world(uint32_t i, float w[9]) const {
        const uint32_t r = range_of(R.pre, R.nr, i);
        const float *M = R.M + 16u * (size_t)r;
        const float *q = rest + 9u * (size_t)i;
        for (int k = 0; k < 3; ++k) {
            const f3 v = tpos(M, mk(q[3 * k], q[3 * k + 1], q[3 * k + 2]));
            w[3 * k] = v.x; w[3 * k + 1] = v.y; w[3 * k + 2] = v.z;
        }
        return R.first[r] + (i - R.pre[r]);
    }
    RT_HD bool ok(const RefitArgs &, uint32_t i) const {
        float w[9];
        world(i, w);
        return tri_ok(w);
    }
    RT_HD void write(const RefitArgs &A, uint32_t i) const {
        float w[9];
        const uint32_t id = world(i, w);
        write_tri(A, id, w);
    }
};

// a record of one of the five kinds: every field the kind reads finite, its transform Ti finite
// where one is read (null: none), its box finite.  The rule rt_scene_update_prims and
// rt_scene_splice_prims (rt_splice.h) share
RT_HD bool prim_fields_ok(const rt_prim &p, const float *Ti) {
    bool ok = true;
    const int nf = p.type == RT_TRIANGLE ? 9 : p.type == RT_CUBE ? 6 : p.type == RT_QUAD ? 1 : 4;
    for (int k = 0; k < nf; ++k) ok = ok && finite_f(p.v[k]);
    for (int k = 0; Ti && k < 16; ++k) ok = ok && finite_f(Ti[k]);
    PrimX x;
    PrimGeom g;
    prim_transform(p, Ti, x);
    prim_geometry(p, x, g);
    return ok && finite_f3(g.bmin) && finite_f3(g.bmax);
}

// rt_scene_update_prims: record i of any kind for primitive first + i, with transform T + 16 i
// (T may be null) where its kind reads one -- cubes and quads
struct PrimRecs {
    uint32_t first;
    const rt_prim *prims;
    const float *T;
    RT_HD const float *transform(const rt_prim &p, uint32_t i) const {
        return (T && (p.type == RT_CUBE || p.type == RT_QUAD)) ? T + 16u * (size_t)i : nullptr;
    }
    // type and material as the scene holds them (the shading record's words), every field the
    // kind reads finite, its transform finite where one is read, its box finite
    RT_HD bool ok(const RefitArgs &A, uint32_t i) const {
        const uint32_t id = first + i;
        const rt_prim p = prims[i];
        if ((uint32_t)p.type != fbits(A.shade[2 * (size_t)id + 1].x) || (uint32_t)p.material != fbits(A.shade[2 * (size_t)id].w))
            return false;
        return prim_fields_ok(p, transform(p, i));
    }
    // the leaf-slot record, the shading record (material word kept), a cube's or a quad's
    // side-table entry (through the index its shading record holds) and the slot box; the sticky
    // flag is tri_sliver's for a triangle and stays as it is for every other kind (mark_sticky's
    // depends on the kind alone)
    RT_HD void write(const RefitArgs &A, uint32_t i) const {
        const uint32_t id = first + i, slot = A.slot_of[id];
        const rt_prim p = prims[i];
        PrimX x;
        PrimGeom g;
        prim_transform(p, transform(p, i), x);
        prim_geometry(p, x, g);
        const float4 old0 = A.shade[2 * (size_t)id], old1 = A.shade[2 * (size_t)id + 1];
        const uint32_t xi = fbits(old1.z);
        float4 s[2];
        prim_shade(p, x, xi, s);
        s[0].w = old0.w;
        A.shade[2 * (size_t)id] = s[0];
        A.shade[2 * (size_t)id + 1] = s[1];
        prim_record(p, x, id, xi, A.prims + 3 * (size_t)slot);
        if (p.type == RT_CUBE || p.type == RT_QUAD) prim_xentry(p, x, A.xprims + 8 * (size_t)xi);
        const bool sticky = p.type == RT_TRIANGLE ? tri_sliver(p.v, A.sliver_lim) : slot_sticky(A.slot_box[2 * (size_t)slot]);
        slot_box(g.bmin, g.bmax, sticky, A.slot_box + 2 * (size_t)slot);
        if (A.cen) A.cen[id] = make_float4(g.centroid.x, g.centroid.y, g.centroid.z, 0.0f);
    }
};

// ---- the refit.  A leaf folds its slots' boxes as Scene::UpdateNodeBounds does
// (template/scene.h:855-865); an interior node takes the union of its two children and the OR of
// their sticky bits.  min / max of floats are exact, so the boxes are the builder's bit for bit.
RT_HD void refit_node(const RefitArgs &A, uint32_t k) {
    const uint32_t word = fbits(A.nodes[2 * (size_t)k + 1].z), cnt = word & 255u, lf = word >> 8;
    f3 mn, mx;
    bool sticky = false;
    if (cnt) {
        mn = mk(1e30f, 1e30f, 1e30f);
        mx = mk(-1e30f, -1e30f, -1e30f);
        for (uint32_t s = lf; s < lf + cnt; ++s) {
            const float4 lo = A.slot_box[2 * (size_t)s], hi = A.slot_box[2 * (size_t)s + 1];
            mn = fmin3(mn, mk(lo.x, lo.y, lo.z));
            mx = fmax3(mx, mk(hi.x, hi.y, hi.z));
            sticky = sticky || slot_sticky(lo);
        }
    } else {
        const float4 *c = A.nodes + 2 * (size_t)lf;
        const float4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
        f3 lmn, lmx, rmn, rmx;
        node_box(l0, l1, lmn, lmx);
        node_box(r0, r1, rmn, rmx);
        mn = fmin3(lmn, rmn);
        mx = fmax3(lmx, rmx);
        sticky = is_sticky(l1.w) || is_sticky(r1.w);
    }
    node_pack(mn, mx, word, walk_word(sticky, A.margin), A.nodes + 2 * (size_t)k);
}
// One height of a group: entries [lvl[l], lvl[l + 1]) of the list, dealt tid, tid + stride, ...
// A group's heights run in order with a barrier between them (the nodes of a height read the
// heights below); a host caller runs them in order with tid = 0, stride = 1.
RT_HD void refit_level(const RefitArgs &A, uint32_t l, uint32_t tid, uint32_t stride) {
    const uint32_t e = A.lvl[l + 1];
    for (uint32_t i = A.lvl[l] + tid; i < e; i += stride) refit_node(A, A.list[i]);
}

// ---- stream-ordered updates: nobody on the host reads the check's flag.  It lives in
// the scene's status block; the write and the refit launches of the same update read it (the gate)
// and return without a store when it is set, and one lane then books the outcome and clears it for
// the next update (the settle step).  One stream order, one writer: plain loads and stores, the
// flag always written by an earlier launch than the one that reads it.
struct UpdateStatus {
    uint32_t flag, pad;       // the check of the update in flight refused it (k_check sets, settle_update clears)
    uint64_t applied, refused;   // updates since the scene was created
    uint64_t first_refused;   // ticket of the earliest refusal since the host last read the block (0: none)
};
// What rt_scene_update_triangles and rt_scene_update_prims, blocking or stream-ordered, refuse without
// the device or the records' contents, in order (the scene-kind refusals -- SBVH, RT_PT_QUADS -- come
// between kAsyncNullRecords and kAsyncRange).  Named for the stream-ordered forms it was written for; the
// blocking and the _host forms take their refusals from it too.  light_stays: rt_scene_update_prims_async,
// where primitive 0 moves through the blocking call alone.
enum { kAsyncOk = 0, kAsyncNullScene, kAsyncEmpty, kAsyncNullRecords, kAsyncRange, kAsyncLight };
RT_HD int async_arguments(bool scene, uint32_t num_prims, uint32_t first, uint32_t count, const void *recs, bool light_stays) {
    if (!scene) return kAsyncNullScene;
    if (count == 0) return kAsyncEmpty;
    if (!recs) return kAsyncNullRecords;
    if ((uint64_t)first + count > num_prims) return kAsyncRange;
    if (light_stays && first == 0) return kAsyncLight;
    return kAsyncOk;
}
RT_HD bool update_gated(const UpdateStatus *st) { return st->flag != 0u; }
RT_HD void settle_update(UpdateStatus *st, uint64_t ticket) {
    if (st->flag != 0u) {
        st->refused += 1u;
        if (st->first_refused == 0u) st->first_refused = ticket;
    } else {
        st->applied += 1u;
    }
    st->flag = 0u;
}

}  // namespace rt
