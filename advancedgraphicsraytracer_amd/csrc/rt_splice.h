// rt_splice.h -- the per-lane text of rt_scene_splice_triangles: the step in front of
// the GPU builder (rt_build.h) that forms the new id space when triangles leave and enter a scene.
//
// and of the batched edits rt_scene_splice_ranges and rt_scene_compact_triangles (below),
// and of rt_scene_splice_prims, rt_scene_compact_prims and rt_scene_set_prim_materials (at
// the end): the same routes with every kind of primitive, and a side table that follows them.
//
// One text for gfx950 and for the host, like rt_update.h and under the same -ffp-contract=off: the
// kernels of rt_splice.hip supply the lane index, a stand-alone host program runs the same lines in a
// loop (tests/cpp/splice_host.cpp, splice_many_host.cpp).  No std:: algorithm in what a lane runs; the
// host's sorting of a batched call's edits (splice_plan) is marked as such.
//
// The edit removes ids [first, first + remove) and puts `insert` new triangles at id `first`.  The
// map from a new id j to where it comes from is closed-form, so no table travels:
//   j < first                       old id j;
//   first <= j < first + insert     inserted record j - first;
//   otherwise                       old id j - insert + remove.
// Everything is written in id order (slot = id) into fresh arrays: the builder then reads them with
// the identity as its old slot map, and its permute_slots puts the records into the new leaf order.
#pragma once
#include <algorithm>
#include <vector>

#include "rt_build.h"

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
    // primitives of every kind (all null / unread on the triangle routes): one mat4 per
    // inserted record (null: identity), mark_sticky's rule for spheres and quads, the side table as it
    // is, per new id its side-table index (null: kept cubes and quads keep theirs, the identity map),
    // and the new side table
    const float *T;
    bool sticky_spheres;
    const float4 *old_xprims;
    const uint32_t *xrank;
    float4 *xprims;
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

// Where a new id comes from, as one word: an old id, or kSpliceNew | the index of an inserted record
// (ids stay below 2^24, so the top bit is free).
constexpr uint32_t kSpliceNew = 0x80000000u;

// mark_sticky's rule per kind (rt_scene_pack.cpp): a sliver triangle, a sphere or a quad where the scene
// was created with sticky spheres, never a plane or a cube
RT_HD bool splice_sticky(const SpliceArgs &A, const rt_prim &p) {
    if (p.type == RT_SPHERE || p.type == RT_QUAD) return A.sticky_spheres;
    return p.type == RT_TRIANGLE && tri_sliver(p.v, A.sliver_lim);
}
RT_HD bool has_xentry(uint32_t type) { return type == (uint32_t)RT_CUBE || type == (uint32_t)RT_QUAD; }

// New id j from source word w.  A kept primitive copies its shading record, its centroid, its slot box
// and its leaf-slot record; the id is word q[0].w of every kind's record (tri_record, prim_record).  A
// cube's or a quad's side-table index is its rank among cubes and quads: triangles coming and going do
// not change it (xrank null), any other kind coming or going does, and then the kept entry moves from
// its old index to xrank[j] and the two words that hold the index -- s[1].z of the shading record,
// q[1].x of the leaf-slot record -- follow.  An inserted record is written by the encoders that scene
// creation runs (pack_shade, pack_slots, pack_xprims, pack_nodes and mark_sticky of rt_scene_pack.cpp).
RT_HD void splice_put(const SpliceArgs &A, uint32_t j, uint32_t w) {
    float4 q[3], b[2], s[2], c;
    if (w & kSpliceNew) {
        const uint32_t i = w & ~kSpliceNew;
        const rt_prim p = A.recs[i];
        const bool side = has_xentry((uint32_t)p.type);
        const uint32_t xi = side && A.xrank ? A.xrank[j] : 0u;
        PrimX x;
        PrimGeom g;
        prim_transform(p, side && A.T ? A.T + 16u * (size_t)i : nullptr, x);
        prim_geometry(p, x, g);
        prim_shade(p, x, xi, s);
        prim_record(p, x, j, xi, q);
        if (side) prim_xentry(p, x, A.xprims + 8 * (size_t)xi);
        slot_box(g.bmin, g.bmax, splice_sticky(A, p), b);
        c = make_float4(g.centroid.x, g.centroid.y, g.centroid.z, 0.0f);
    } else {
        const uint32_t o = w;
        const uint32_t slot = A.old_slot_of[o];
        for (int k = 0; k < 2; ++k) s[k] = A.old_shade[2 * (size_t)o + k];
        c = A.old_cen[o];
        for (int k = 0; k < 2; ++k) b[k] = A.old_box[2 * (size_t)slot + k];
        for (int k = 0; k < 3; ++k) q[k] = A.old_prims[3 * (size_t)slot + k];
        q[0].w = ibits((int)j);
        if (A.xrank && has_xentry(fbits(s[1].x))) {
            const uint32_t xo = fbits(s[1].z), xn = A.xrank[j];
            for (int k = 0; k < 8; ++k) A.xprims[8 * (size_t)xn + k] = A.old_xprims[8 * (size_t)xo + k];
            s[1].z = ubits(xn);
            q[1].x = ubits(xn);
        }
    }
    for (int k = 0; k < 2; ++k) A.shade[2 * (size_t)j + k] = s[k];
    A.cen[j] = c;
    for (int k = 0; k < 2; ++k) A.box[2 * (size_t)j + k] = b[k];
    for (int k = 0; k < 3; ++k) A.prims[3 * (size_t)j + k] = q[k];
    A.ident[j] = j;
}
// the single range: the source word in closed form (the map at the top)
RT_HD void splice_gather(const SpliceArgs &A, uint32_t j) {
    const bool in = j >= A.first && j < A.first + A.insert;
    splice_put(A, j, in ? kSpliceNew | (j - A.first) : j < A.first ? j : j - A.insert + A.remove);
}

// ---- many edits in one rebuild: rt_scene_splice_ranges and rt_scene_compact_triangles.
// Both fill one source word per new id (src) and then run the one gather over them; they differ only
// in how the words come to be.
// The records of a batched call stand back to back in A.recs and get one pass of splice_ok.
RT_HD void splice_gather_src(const SpliceArgs &A, const uint32_t *src, uint32_t j) { splice_put(A, j, src[j]); }

// -- the ranges route.  One row per non-empty edit, sorted by `first`: the new id where its inserted
// records start, its old range, and where its records start in the caller's array.  Between two rows
// the kept primitives run on: new id start + insert is old id first + remove.
struct SpliceRow { uint32_t start, first, remove, insert, offset; };
// the source word of new id j: the last row whose start is <= j by binary search.  Two rows share a
// start only where the earlier one inserts nothing and the later one begins where it ends, and then the
// earlier one owns no new id.
RT_HD uint32_t splice_source(const SpliceRow *rows, uint32_t num_rows, uint32_t j) {
    uint32_t lo = 0, hi = num_rows;   // rows [0, lo) start at or before j, rows [hi, num_rows) after it
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (rows[mid].start <= j) lo = mid + 1u; else hi = mid;
    }
    if (lo == 0) return j;   // before the first edit
    const SpliceRow r = rows[lo - 1u];
    const uint32_t k = j - r.start;
    return k < r.insert ? kSpliceNew | (r.offset + k) : r.first + r.remove + (k - r.insert);
}

// The host's part of the ranges route, shared by the library and the stand-alone program: the refusals
// that need neither the device nor the records' contents, and the rows.  Per edit in the caller's order
// what splice_range refuses; then, over the non-empty edits sorted by first, the same first twice and
// overlapping removed ranges.  Without a scene (ptype null) the checks that need none still run, so
// that they come first for every caller.  *where: the edit (caller's index) or the primitive refused.
enum { kSpliceSameFirst = kSpliceKind + 1, kSpliceOverlap, kSpliceMany };
struct SplicePlan {
    std::vector<SpliceRow> rows;
    uint32_t n_new = 0, total_insert = 0;
};
// any_kind: rt_scene_splice_prims, whose removed ranges may hold any kind.
inline int splice_plan(uint32_t num_prims, const uint8_t *ptype, const rt_tri_edit *edits, uint32_t num_edits, const void *recs,
                       SplicePlan &out, uint32_t *where, bool any_kind = false) {
    out = SplicePlan();
    if (num_edits && !edits) return kSpliceNull;
    uint64_t offset = 0;
    std::vector<SpliceRow> rows;
    for (uint32_t e = 0; e < num_edits; ++e) {
        const rt_tri_edit &x = edits[e];
        *where = e;
        if (x.first == 0) return kSpliceLight;
        if (x.insert && !recs) return kSpliceNull;
        if (x.remove == 0 && x.insert == 0) continue;
        if (offset + x.insert >= (1u << 24)) return kSpliceMany;
        rows.push_back(SpliceRow{e, x.first, x.remove, x.insert, (uint32_t)offset});   // start: the caller's index for now
        offset += x.insert;
    }
    std::sort(rows.begin(), rows.end(), [](const SpliceRow &a, const SpliceRow &b) { return a.first < b.first || (a.first == b.first && a.start < b.start); });
    for (size_t k = 1; k < rows.size(); ++k) {
        *where = rows[k].start;
        if (rows[k - 1].first == rows[k].first) return kSpliceSameFirst;
        if ((uint64_t)rows[k - 1].first + rows[k - 1].remove > rows[k].first) return kSpliceOverlap;
    }
    if (!ptype) return kSpliceRange;   // no scene: every range is outside it
    for (const SpliceRow &r : rows) {
        *where = r.start;
        if ((uint64_t)r.first + r.remove > num_prims) return kSpliceRange;
    }
    for (const SpliceRow &r : rows)
        for (uint32_t id = r.first; id < r.first + r.remove && !any_kind; ++id)
            if ((ptype[id] & 0x7f) != RT_TRIANGLE) { *where = id; return kSpliceKind; }
    int64_t shift = 0;   // new id minus old id at the row's first
    for (SpliceRow &r : rows) {
        r.start = (uint32_t)((int64_t)r.first + shift);
        shift += (int64_t)r.insert - (int64_t)r.remove;
    }
    if ((int64_t)num_prims + shift >= (int64_t)(1u << 24)) return kSpliceMany;
    out.rows.swap(rows);
    out.n_new = (uint32_t)((int64_t)num_prims + shift);
    out.total_insert = (uint32_t)offset;
    return kSpliceOk;
}
// the type bytes of the new id space (RefitState::pinfo) from the rows; rec_types: per inserted record
// its type as the check wrote it (null: triangles all)
inline std::vector<uint8_t> splice_types(const std::vector<uint8_t> &ptype, const SplicePlan &plan, const uint8_t *rec_types = nullptr) {
    std::vector<uint8_t> out;
    out.reserve(plan.n_new);
    uint32_t at = 0;
    for (const SpliceRow &r : plan.rows) {
        out.insert(out.end(), ptype.begin() + at, ptype.begin() + r.first);
        if (rec_types) out.insert(out.end(), rec_types + r.offset, rec_types + r.offset + r.insert);
        else out.insert(out.end(), r.insert, (uint8_t)RT_TRIANGLE);
        at = r.first + r.remove;
    }
    out.insert(out.end(), ptype.begin() + at, ptype.end());
    return out;
}

// -- the mask route.  keep[i] != 0: old id i stays; survivors keep their order, so the new id of a
// survivor is the number of survivors before it -- an exclusive prefix count of the flags -- and
// src[that] = i.  A workgroup takes kMaskGroup consecutive old ids, every lane a run of consecutive ids
// of them (one id per lane on the device, the whole group for the host's one lane).  Nothing is handed
// from one workgroup to another inside a launch: mask_count writes a count per group, mask_top turns
// the counts into the groups' first new ids (one workgroup, as many counts at a time as it has lanes,
// with a running carry: no size is too large for it), mask_scatter writes the source words.
constexpr uint32_t kMaskGroup = 256;
struct MaskArgs {
    uint32_t n;                 // old primitives
    const uint8_t *keep;
    const float4 *old_shade;    // word [2 i + 1].x: the type of old id i, as the kernels read it
    uint32_t *sums;             // mask_groups(n) + 1 words: per group its count, then its first new id; last: the survivors
    uint32_t *src;
};
RT_HD uint32_t mask_groups(uint32_t n) { return (n + kMaskGroup - 1u) / kMaskGroup; }
// the mask drops neither primitive 0 nor anything but a triangle
RT_HD bool mask_ok(const MaskArgs &M, uint32_t i) {
    return M.keep[i] != 0 || (i != 0 && fbits(M.old_shade[2 * (size_t)i + 1].x) == (uint32_t)RT_TRIANGLE);
}
// the ids [r0, r1) of group g that lane tid of `stride` takes (stride divides kMaskGroup)
RT_HD void mask_run(uint32_t n, uint32_t g, uint32_t tid, uint32_t stride, uint32_t &r0, uint32_t &r1) {
    const uint32_t per = kMaskGroup / stride, a = g * kMaskGroup + tid * per;
    r0 = a < n ? a : n;
    r1 = a + per < n ? a + per : n;
}
// survivors in the lane's run, and before it in the group (scan: stride words); total: the group's
template <class P>
RT_HD uint32_t mask_before(const MaskArgs &M, uint32_t g, uint32_t *scan, uint32_t &total, P &par) {
    uint32_t r0, r1, c = 0;
    mask_run(M.n, g, par.tid, par.stride, r0, r1);
    for (uint32_t i = r0; i < r1; ++i) c += M.keep[i] != 0;
    return wg_scan(scan, c, total, par);
}
template <class P>
RT_HD void mask_count(const MaskArgs &M, uint32_t g, uint32_t *scan, P &par) {
    uint32_t total;
    mask_before(M, g, scan, total, par);
    if (par.tid == 0) M.sums[g] = total;
}
template <class P>
RT_HD void mask_top(const MaskArgs &M, uint32_t *scan, P &par) {
    const uint32_t ng = mask_groups(M.n);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < ng; base += par.stride) {
        const uint32_t g = base + par.tid, v = g < ng ? M.sums[g] : 0u;
        uint32_t total;
        const uint32_t before = wg_scan(scan, v, total, par);
        if (g < ng) M.sums[g] = carry + before;
        carry += total;
    }
    if (par.tid == 0) M.sums[ng] = carry;
}
template <class P>
RT_HD void mask_scatter(const MaskArgs &M, uint32_t g, uint32_t *scan, P &par) {
    uint32_t r0, r1, total;
    uint32_t at = M.sums[g] + mask_before(M, g, scan, total, par);
    mask_run(M.n, g, par.tid, par.stride, r0, r1);
    for (uint32_t i = r0; i < r1; ++i)
        if (M.keep[i] != 0) M.src[at++] = i;
}

// ---- primitives of every kind: rt_scene_splice_prims and rt_scene_compact_prims take the
// two routes above -- source words, one gather -- with three additions: a check that admits all five
// kinds, the side-table ranks of the new id space, and a gather that moves the side table (splice_put).

// an inserted record: one of the five kinds, one of the scene's materials, and prim_fields_ok -- PrimRecs::ok
// without its "as the scene holds them" test.  The lane also leaves the record's type byte for the host,
// which splices RefitState::pinfo from it without a copy of the records
RT_HD bool splice_prim_ok(const SpliceArgs &A, uint32_t i, uint8_t *types) {
    const rt_prim p = A.recs[i];
    types[i] = (uint8_t)p.type;
    if (p.type < RT_SPHERE || p.type > RT_TRIANGLE) return false;
    if (p.material < 0 || (uint32_t)p.material >= A.num_materials) return false;
    return prim_fields_ok(p, A.T && has_xentry((uint32_t)p.type) ? A.T + 16u * (size_t)i : nullptr);
}
// the mask drops anything but primitive 0
RT_HD bool mask_prims_ok(const MaskArgs &M, uint32_t i) { return M.keep[i] != 0 || i != 0; }

// Side-table ranks.  The new side-table index of new id j is the number of cubes and quads among the new
// ids below j -- an exclusive prefix count of a per-new-id flag, which is the mask route's count with
// the flag in the place of keep: rank_flag writes the flags (from the source word: the old shading
// record's type word, or the inserted record's type), mask_count and mask_top run over them unchanged
// (MaskArgs{n_new, flags, ..}), and mask_ranks, mask_scatter's sibling, writes every id's count-before
// instead of the survivors' ids.  sums[mask_groups(n_new)] is the new side table's size.
RT_HD void rank_flag(const SpliceArgs &A, const uint32_t *src, uint8_t *flags, uint32_t j) {
    const uint32_t w = src[j];
    const uint32_t type = w & kSpliceNew ? (uint32_t)A.recs[w & ~kSpliceNew].type : fbits(A.old_shade[2 * (size_t)w + 1].x);
    flags[j] = has_xentry(type) ? 1 : 0;
}
template <class P>
RT_HD void mask_ranks(const MaskArgs &M, uint32_t g, uint32_t *scan, uint32_t *rank, P &par) {
    uint32_t r0, r1, total;
    uint32_t at = M.sums[g] + mask_before(M, g, scan, total, par);
    mask_run(M.n, g, par.tid, par.stride, r0, r1);
    for (uint32_t i = r0; i < r1; ++i) {
        rank[i] = at;
        at += M.keep[i] != 0;
    }
}

// ---- rt_scene_set_prim_materials: the material word of the shading records of [first, first + count),
// nothing else; the check is a pass of its own
struct MatArgs {
    uint32_t first, count, num_materials;
    const int32_t *mats;
    float4 *shade;
};
RT_HD bool mats_ok(const MatArgs &M, uint32_t i) { return M.mats[i] >= 0 && (uint32_t)M.mats[i] < M.num_materials; }
RT_HD void mats_put(const MatArgs &M, uint32_t i) { M.shade[2 * (size_t)(M.first + i)].w = ibits(M.mats[i]); }

}  // namespace rt
