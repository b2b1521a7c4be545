// rt_scene_edit.hip -- the scene-edit half of the device C-ABI: every entry point that changes a live
// scene -- in-place updates (blocking and stream-ordered), the rebuild, the splices, the compactions,
// the material words -- and the refit schedule's queries.  No kernel lives here: an entry point checks
// its arguments, and the device work is rt_refit.hip's, rt_build.hip's, rt_splice.hip's or rt_plan.hip's.
//
// Each step the entry points share exists once: the call frame (edit_call, enter), the _host forms'
// staging (stage), the refusals per family (*_arguments; the host-decidable ones come from rt_update.h
// and rt_splice.h, where a stand-alone host program runs them too), and one body per pair of routes
// that differ in a flag (blocking / stream-ordered, triangles / any kind).
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "rt_scene.h"
#include "rt_splice.h"

using namespace rt;

// Waits for the enqueued async updates and folds their outcomes into the host's state.  The root of a
// checked refit over finite primitive boxes is finite by construction, so the flags rise as after a
// blocking update, without a read-back.  A scene without pending async updates pays one branch.
int rt::fold_updates(rt_scene *s) {
    if (!s->refit.async.issued) return RT_OK;
    HIP_TRY(hipSetDevice(s->device));
    uint64_t applied = 0;
    const int rc = drain_updates(s->refit, &applied);
    if (rc != RT_OK) return rc;
    if (applied) {
        s->view.bounds_finite = s->refit.boxes_finite ? 1 : 0;
        if (s->refit.boxes_finite) s->nested = true;
    }
    return RT_OK;
}

namespace {

// ---- the call frame.  An entry point's body runs under its name: whatever it throws becomes
// RT_ERR_INVALID "<who>: <what()>", and a Rebuilt it left half made is freed.
template <class Body>
int edit_call(const char *name, const char *suffix, Body body) {
    Rebuilt t;
    try {
        return body(std::string(name) + suffix, t);
    } catch (const std::exception &e) {
        free_rebuilt(t);
        return fail(RT_ERR_INVALID, std::string(name) + suffix + ": " + e.what());
    }
}
// ... and, its arguments accepted, enters the device: the async updates first (rt_scene_update_sync;
// the stream-ordered forms queue behind them instead), then the scene's device
int enter(rt_scene *s, bool fold = true) {
    if (fold)
        if (int rc = fold_updates(s); rc != RT_OK) return rc;
    HIP_TRY(hipSetDevice(s->device));
    return RT_OK;
}

// ---- the _host forms' staging: up to two host spans -- records, then (b non-null) transforms at the
// next 16-byte boundary -- into the scene's staging buffer, on its private stream.  Nothing to stage:
// nothing done, null pointers.
struct Staged { const char *a = nullptr, *b = nullptr; };
int stage(rt_scene *s, const void *a, size_t abytes, const void *b, size_t bbytes, Staged &d) {
    d = Staged();
    if (!abytes) return RT_OK;
    if (!b) bbytes = 0;
    HIP_TRY(hipSetDevice(s->device));
    HIP_TRY(hipDeviceSynchronize());   // the staging buffer may be in use by a batched call
    const size_t off = (abytes + 15u) & ~(size_t)15u;
    const int rc = grow(&s->d_scratch, &s->scratch_bytes, bbytes ? off + bbytes : abytes);
    if (rc != RT_OK) return rc;
    char *base = (char *)s->d_scratch;
    HIP_TRY(hipMemcpyAsync(base, a, abytes, hipMemcpyHostToDevice, s->stream));
    if (bbytes) HIP_TRY(hipMemcpyAsync(base + off, b, bbytes, hipMemcpyHostToDevice, s->stream));
    d.a = base;
    d.b = bbytes ? base + off : nullptr;
    return RT_OK;
}

// an in-place update needs a plain tree (every primitive in one leaf) with the binary node array alone
int refit_supported(const rt_scene *s, const std::string &who) {
    if (s->bvh.indices.size() != s->num_prims)
        return fail(RT_ERR_UNSUPPORTED, who + ": an SBVH scene (leaves share primitives) cannot be refitted");
    if (s->quads) return fail(RT_ERR_UNSUPPORTED, who + ": scene built with two-level node records (RT_PT_QUADS=1)");
    return RT_OK;
}
// ... and the builder's decisions are min / max over keys of the floats: a NaN box (kept from creation) has no place in them
int rebuild_supported(const rt_scene *s, const std::string &who) {
    const int rc = refit_supported(s, who);
    if (rc != RT_OK) return rc;
    if (!s->refit.boxes_finite) return fail(RT_ERR_UNSUPPORTED, who + ": a primitive's box is NaN or infinite");
    return RT_OK;
}
int not_a_triangle(const std::string &who, uint32_t id) {
    return fail(RT_ERR_INVALID, who + ": primitive " + std::to_string(id) + " is not a triangle");
}
int require_triangles(const rt_scene *s, uint32_t first, uint32_t count, const std::string &who) {
    for (uint32_t id = first; id < first + count; ++id)
        if ((s->refit.pinfo[id] & 0x7f) != RT_TRIANGLE) return not_a_triangle(who, id);
    return RT_OK;
}
SceneRecords records_of(rt_scene *s) {
    return SceneRecords{&s->bvh, s->num_prims, s->d_nodes, s->d_prims, s->d_shade, s->d_xprims, s->view.walk_margin};
}
// after an update: the scene's flags from the new root box
int settle(rt_scene *s, int rc, bool finite) {
    if (rc != RT_OK) return rc;
    s->view.bounds_finite = finite ? 1 : 0;
    if (finite) s->nested = true;   // every box is now the union of finite boxes below it
    return RT_OK;
}

// ---- in-place updates.  The entry points check their arguments; the device work -- check, write,
// refit, one path for all of them -- is update() of rt_refit.hip, or update_async:
// enqueued on the caller's stream, no host wait, the scene's host flags (bounds_finite, nested) staying
// until the outcomes are folded (fold_updates).  One body serves both forms of an entry point.

// the update entry points by kind (update_async's `kind`, rt_refit.h), a stream-ordered form appending
// _async, and why the device's check refuses one: said at once by a blocking form, at the next fold by
// a stream-ordered one (rt_scene_update_sync)
const char *const kUpdateNames[3] = {"rt_scene_update_triangles", "rt_scene_transform_triangles", "rt_scene_update_prims"};
const char *const kRefusals[3] = {
    "a vertex is NaN or infinite",
    "a transformed vertex is NaN or infinite",
    "a record's type or material is not the scene's, or a field, transform or box is NaN or infinite",
};
const char *form_of(bool async) { return async ? "_async" : ""; }

// async_arguments' refusals (rt_update.h) under the caller's name; scene_kind: with the scene-kind
// refusals in their place (a _host form leaves them, and what follows, to its device form).
// what: "vertices" or "records"; *empty: nothing to do
int update_refusals(const rt_scene *s, uint32_t first, uint32_t count, const void *recs, const char *what, bool light_stays,
                    bool scene_kind, const std::string &who, bool *empty) {
    const int k = async_arguments(s != nullptr, s ? s->num_prims : 0u, first, count, recs, light_stays);
    *empty = k == kAsyncEmpty;
    if (k == kAsyncNullScene) return fail(RT_ERR_INVALID, who + ": null scene");
    if (k == kAsyncEmpty) return RT_OK;
    if (k == kAsyncNullRecords) return fail(RT_ERR_INVALID, who + ": null " + what);
    if (scene_kind)
        if (int rc = refit_supported(s, who); rc != RT_OK) return rc;
    if (k == kAsyncRange) return fail(RT_ERR_INVALID, who + ": range outside the primitives");
    // the light's SceneView fields are computed on the host from its record (fill_light), which the async call never sees
    if (k == kAsyncLight) return fail(RT_ERR_UNSUPPORTED, who + ": the range holds primitive 0 (the light moves through rt_scene_update_prims)");
    return RT_OK;
}

int update_triangles(rt_scene *s, uint32_t first, uint32_t count, const float *verts_dev, void *stream, bool async, uint64_t *ticket) {
    return edit_call(kUpdateNames[0], form_of(async), [&](const std::string &who, Rebuilt &) -> int {
        bool empty = false;
        int rc = update_refusals(s, first, count, verts_dev, "vertices", false, true, who, &empty);
        if (rc != RT_OK || empty) return rc;
        if ((rc = require_triangles(s, first, count, who)) != RT_OK || (rc = enter(s, !async)) != RT_OK) return rc;
        const TriVerts src{first, verts_dev};
        if (async) return update_async(s->refit, records_of(s), src, count, (hipStream_t)stream, 0, nullptr, 0, ticket);
        bool finite = false;
        rc = update(s->refit, records_of(s), src, count, (hipStream_t)stream, who.c_str(), kRefusals[0], nullptr, 0, &finite);
        return settle(s, rc, finite);
    });
}

int update_prims(rt_scene *s, uint32_t first, uint32_t count, const rt_prim *prims_dev, const float *transforms_dev, void *stream,
                 bool async, uint64_t *ticket) {
    return edit_call(kUpdateNames[2], form_of(async), [&](const std::string &who, Rebuilt &) -> int {
        bool empty = false;
        int rc = update_refusals(s, first, count, prims_dev, "records", async, true, who, &empty);
        if (rc != RT_OK || empty || (rc = enter(s, !async)) != RT_OK) return rc;
        const PrimRecs src{first, prims_dev, transforms_dev};
        if (async) return update_async(s->refit, records_of(s), src, count, (hipStream_t)stream, 2, nullptr, 0, ticket);
        // the light's record and matrix come back with the check's flag
        rt_prim light{};
        float lightT[16];
        bool finite = false;
        const UpdateCopy back[2] = {{&light, prims_dev, sizeof(light), hipMemcpyDeviceToHost},
                                    {lightT, transforms_dev, sizeof(lightT), hipMemcpyDeviceToHost}};
        rc = update(s->refit, records_of(s), src, count, (hipStream_t)stream, who.c_str(), kRefusals[2], back,
                    first != 0 ? 0 : transforms_dev ? 2 : 1, &finite);
        // SceneView travels by value with every launch (renderers and the multi-GPU frames read
        // s->view per frame), so the light's fields change here and nowhere else
        if (rc == RT_OK && first == 0) fill_light(light, transforms_dev ? lightT : nullptr, s->view);
        return settle(s, rc, finite);
    });
}

int transform_triangles(rt_scene *s, const rt_tri_xform *ranges, uint32_t num_ranges, const float *rest_dev, void *stream, bool async,
                        uint64_t *ticket) {
    return edit_call(kUpdateNames[1], form_of(async), [&](const std::string &who, Rebuilt &) -> int {
        if (!s) return fail(RT_ERR_INVALID, who + ": null scene");
        if (num_ranges == 0) return RT_OK;
        if (!ranges) return fail(RT_ERR_INVALID, who + ": null ranges");
        int rc = refit_supported(s, who);
        if (rc != RT_OK) return rc;
        std::vector<uint32_t> tab;
        uint32_t nr = 0, at = 0;
        switch (xform_table(s->num_prims, s->refit.pinfo.data(), ranges, num_ranges, rest_dev, tab, &nr, &at)) {
        case kXformEmpty: return RT_OK;
        case kXformRange: return fail(RT_ERR_INVALID, who + ": range " + std::to_string(at) + " outside the primitives");
        case kXformMany: return fail(RT_ERR_INVALID, who + ": too many triangles");
        case kXformKind: return not_a_triangle(who, at);
        case kXformOverlap: return fail(RT_ERR_INVALID, who + ": ranges overlap");
        case kXformNullRest: return fail(RT_ERR_INVALID, who + ": null rest vertices");
        }
        if ((rc = enter(s, !async)) != RT_OK) return rc;
        if (async) return update_xform_async(s->refit, records_of(s), tab, nr, rest_dev, (hipStream_t)stream, ticket);
        bool finite = false;
        rc = update_xform(s->refit, records_of(s), tab, nr, rest_dev, (hipStream_t)stream, who.c_str(), kRefusals[1], &finite);
        return settle(s, rc, finite);
    });
}

// ---- the rebuild (rt_build.hip) and the splices (rt_splice.hip): built into fresh buffers, checked,
// and only then swapped in

// a Rebuilt's tree becomes the scene's (the splice sets s->num_prims first): the old buffers are freed
void swap_in_tree(rt_scene *s, const Rebuilt &t) {
    RefitState &R = s->refit;
    for (void *old : {s->d_nodes, s->d_prims, R.d_slot_box, R.d_slot_of, R.d_index})
        if (old) (void)hipFree(old);
    s->d_nodes = t.nodes;
    s->d_prims = t.prims;
    R.d_slot_box = t.slot_box;
    R.d_slot_of = t.slot_of;
    R.d_index = t.index;
    s->bvh.nodes_used = t.nodes_used;
    s->bvh.depth = t.depth;
    s->bvh.max_leaf = t.max_leaf;
    // the host tree and the refit schedule are the old topology's: the tree is downloaded whole
    // before its next use, the next update builds its schedule from it
    R.topo_stale = true;
    R.refit_ready = false;
    for (int k = 0; k < 4; ++k) R.rebuild_stats[k] = t.stats[k];
    // every box is the union of the finite boxes below it
    scene_tree_fields(s, t.root_word, true, t.finite);
}
// a splice's own: the new id space and the host's share of it (pinfo, indices: made by the caller
// before anything is swapped); then the tree, as after a rebuild
void swap_in_splice(rt_scene *s, const Rebuilt &t, std::vector<uint8_t> &pinfo, std::vector<uint32_t> &indices) {
    RefitState &R = s->refit;
    for (void *old : {s->d_shade, R.d_cen})
        if (old) (void)hipFree(old);
    s->d_shade = t.shade;
    R.d_cen = t.cen;
    s->view.shade = (const float4 *)s->d_shade;
    s->num_prims = (uint32_t)pinfo.size();
    R.pinfo.swap(pinfo);
    s->bvh.indices.swap(indices);
    swap_in_tree(s, t);
}
// the any-kind routes' own: the new side table, and the kernel family by the rule creation
// uses (kernel_family).  A scene that gained its first cube no longer admits the wave walk: the camera-walk
// policy falls back as rt_scene_set_camera_walk would refuse it now.  The renderers read s->ext, s->walk
// and the view per frame, so one created before the edit takes the new family with its next frame.
void swap_in_kinds(rt_scene *s, Rebuilt &t) {
    if (s->d_xprims) (void)hipFree(s->d_xprims);
    s->d_xprims = t.xprims;
    t.xprims = nullptr;
    s->view.xprims = (const float4 *)s->d_xprims;
    const std::vector<uint8_t> &types = s->refit.pinfo;
    kernel_family(s->num_prims, [&types](uint32_t i) { return types[i] & 0x7f; }, s->ext_fixed, s->ext, s->has_cubes);
    if (s->has_cubes && s->walk != RT_WALK_LANE) s->walk = RT_WALK_LANE;
}

// every refusal of rt_scene_splice_triangles that needs no device, in the order the header lists them;
// *empty: nothing to do
int splice_arguments(const rt_scene *s, uint32_t first, uint32_t remove, const rt_prim *prims, uint32_t insert, const std::string &w,
                     bool *empty) {
    *empty = false;
    uint32_t bad = 0;
    const int k = splice_range(s ? s->num_prims : 0u, s ? s->refit.pinfo.data() : nullptr, first, remove, insert, prims, &bad);
    if (k == kSpliceLight) return fail(RT_ERR_INVALID, w + ": first = 0 (primitive 0 is the light and stays)");
    if (k == kSpliceNull) return fail(RT_ERR_INVALID, w + ": null records");
    if (!s) return fail(RT_ERR_INVALID, w + ": null scene");
    if (k == kSpliceRange) return fail(RT_ERR_INVALID, w + ": range outside the primitives");
    if (remove == 0 && insert == 0) {
        *empty = true;
        return RT_OK;
    }
    const int rc = rebuild_supported(s, w);
    if (rc != RT_OK) return rc;
    if (k == kSpliceKind) return not_a_triangle(w, bad);
    if ((uint64_t)s->num_prims - remove + insert >= (1u << 24)) return fail(RT_ERR_UNSUPPORTED, w + ": more than 2^24 primitives");
    return RT_OK;
}

// ---- many edits in one rebuild, of triangles or (any_kind) of every kind

// every refusal of rt_scene_splice_ranges / rt_scene_splice_prims that needs no device, and the sorted
// rows; *empty: nothing to do
int ranges_arguments(const rt_scene *s, const rt_tri_edit *edits, uint32_t num_edits, const rt_prim *prims, const std::string &w,
                     SplicePlan &plan, bool *empty, bool any_kind) {
    *empty = false;
    uint32_t at = 0;
    const int k = splice_plan(s ? s->num_prims : 0u, s ? s->refit.pinfo.data() : nullptr, edits, num_edits, prims, plan, &at, any_kind);
    const std::string edit = ": edit " + std::to_string(at);
    if (k == kSpliceNull) return fail(RT_ERR_INVALID, w + (edits || !num_edits ? edit + ": null records" : ": null edits"));
    if (k == kSpliceLight) return fail(RT_ERR_INVALID, w + edit + ": first = 0 (primitive 0 is the light and stays)");
    if (k == kSpliceSameFirst) return fail(RT_ERR_INVALID, w + edit + ": the same first as another edit (their order would be ambiguous)");
    if (k == kSpliceOverlap) return fail(RT_ERR_INVALID, w + edit + ": its removed range overlaps another edit's");
    if (!s) return fail(RT_ERR_INVALID, w + ": null scene");
    if (k == kSpliceRange) return fail(RT_ERR_INVALID, w + edit + ": range outside the primitives");
    if (k == kSpliceOk && plan.rows.empty()) {
        *empty = true;
        return RT_OK;
    }
    const int rc = rebuild_supported(s, w);
    if (rc != RT_OK) return rc;
    if (k == kSpliceKind) return not_a_triangle(w, at);
    if (k == kSpliceMany) return fail(RT_ERR_UNSUPPORTED, w + ": more than 2^24 primitives");
    return RT_OK;
}

// The two routes differ in where the new type bytes come from -- made here for triangles, read off the
// inserted records by the device's check for any kind (SpliceKinds::types) -- and in the side table and
// kernel family, which only kinds other than triangles can change (swap_in_kinds).
int splice_edits(rt_scene *s, const rt_tri_edit *edits, uint32_t num_edits, const rt_prim *prims_dev, const float *transforms_dev,
                 void *stream, bool any_kind) {
    return edit_call(any_kind ? "rt_scene_splice_prims" : "rt_scene_splice_ranges", "", [&](const std::string &who, Rebuilt &t) -> int {
        SplicePlan plan;
        bool empty = false;
        int rc = ranges_arguments(s, edits, num_edits, prims_dev, who, plan, &empty, any_kind);
        if (rc != RT_OK || empty || (rc = enter(s)) != RT_OK) return rc;
        RefitState &R = s->refit;
        // the host's share, made before anything is swapped: the type bytes require_triangles reads
        // and an index array of the new size (sync_host_tree sizes its download from it)
        SpliceKinds K;
        K.T_dev = transforms_dev;
        if (!any_kind) K.types = splice_types(R.pinfo, plan);
        std::vector<uint32_t> indices(plan.n_new, 0u);
        rc = splice_ranges(R, records_of(s), plan.rows.data(), (uint32_t)plan.rows.size(), plan.n_new, plan.total_insert, prims_dev,
                           s->num_materials, (hipStream_t)stream, t, any_kind ? &K : nullptr);
        if (rc != RT_OK) return rc;
        swap_in_splice(s, t, K.types, indices);
        if (any_kind) swap_in_kinds(s, t);
        return RT_OK;
    });
}
int splice_edits_host(rt_scene *s, const rt_tri_edit *edits, uint32_t num_edits, const rt_prim *prims, const float *transforms,
                      bool any_kind) {
    return edit_call(any_kind ? "rt_scene_splice_prims_host" : "rt_scene_splice_ranges_host", "", [&](const std::string &who, Rebuilt &) -> int {
        SplicePlan plan;
        bool empty = false;
        Staged d;
        int rc = ranges_arguments(s, edits, num_edits, prims, who, plan, &empty, any_kind);
        if (rc != RT_OK || empty) return rc;
        if ((rc = stage(s, prims, sizeof(rt_prim) * (size_t)plan.total_insert, transforms, 64 * (size_t)plan.total_insert, d)) != RT_OK) return rc;
        return splice_edits(s, edits, num_edits, (const rt_prim *)d.a, (const float *)d.b, s->stream, any_kind);
    });
}

int compact_arguments(const rt_scene *s, const uint8_t *keep, const std::string &w) {
    if (!s) return fail(RT_ERR_INVALID, w + ": null scene");
    if (!keep) return fail(RT_ERR_INVALID, w + ": null mask");
    return rebuild_supported(s, w);
}
int compact(rt_scene *s, const uint8_t *keep_dev, void *stream, bool any_kind) {
    return edit_call(any_kind ? "rt_scene_compact_prims" : "rt_scene_compact_triangles", "", [&](const std::string &who, Rebuilt &t) -> int {
        int rc = compact_arguments(s, keep_dev, who);
        if (rc != RT_OK || (rc = enter(s)) != RT_OK) return rc;
        RefitState &R = s->refit;
        std::vector<uint8_t> keep;
        uint32_t n = 0;
        SpliceKinds K;
        rc = splice_mask(R, records_of(s), keep_dev, (hipStream_t)stream, keep, &n, t, any_kind ? &K : nullptr);
        if (rc != RT_OK || n == s->num_prims) return rc;   // all stay: nothing is swapped
        if (!any_kind) {
            K.types.reserve(n);
            for (uint32_t i = 0; i < s->num_prims; ++i)
                if (keep[i]) K.types.push_back(R.pinfo[i]);
        }
        std::vector<uint32_t> indices(n, 0u);
        swap_in_splice(s, t, K.types, indices);
        if (any_kind) swap_in_kinds(s, t);
        return RT_OK;
    });
}
int compact_host(rt_scene *s, const uint8_t *keep, bool any_kind) {
    Staged d;
    int rc = compact_arguments(s, keep, any_kind ? "rt_scene_compact_prims_host" : "rt_scene_compact_triangles_host");
    if (rc != RT_OK || (rc = stage(s, keep, s->num_prims, nullptr, 0, d)) != RT_OK) return rc;
    return compact(s, (const uint8_t *)d.a, s->stream, any_kind);
}

// every refusal of rt_scene_set_prim_materials that needs no device; *empty: nothing to do
int materials_arguments(const rt_scene *s, uint32_t first, uint32_t count, const int32_t *materials, const std::string &w, bool *empty) {
    *empty = false;
    if (!s) return fail(RT_ERR_INVALID, w + ": null scene");
    if (count == 0) {
        *empty = true;
        return RT_OK;
    }
    if (!materials) return fail(RT_ERR_INVALID, w + ": null materials");
    // the light's material feeds SceneView::light_mat and the kernel family
    if (first == 0) return fail(RT_ERR_INVALID, w + ": the range holds primitive 0 (the light's material stays)");
    if ((uint64_t)first + count > s->num_prims) return fail(RT_ERR_INVALID, w + ": range outside the primitives");
    return RT_OK;
}

}  // namespace

extern "C" {

int rt_scene_update_triangles(rt_scene *s, uint32_t first, uint32_t count, const float *verts_dev, void *stream) {
    return update_triangles(s, first, count, verts_dev, stream, false, nullptr);
}
int rt_scene_update_triangles_async(rt_scene *s, uint32_t first, uint32_t count, const float *verts_dev, void *stream,
                                    uint64_t *ticket) {
    return update_triangles(s, first, count, verts_dev, stream, true, ticket);
}
int rt_scene_update_triangles_host(rt_scene *s, uint32_t first, uint32_t count, const float *verts) {
    bool empty = false;
    Staged d;
    int rc = update_refusals(s, first, count, verts, "vertices", false, false, "rt_scene_update_triangles_host", &empty);
    if (rc != RT_OK || empty || (rc = stage(s, verts, 36 * (size_t)count, nullptr, 0, d)) != RT_OK) return rc;
    return rt_scene_update_triangles(s, first, count, (const float *)d.a, s->stream);
}

int rt_scene_update_prims(rt_scene *s, uint32_t first, uint32_t count, const rt_prim *prims_dev, const float *transforms_dev,
                          void *stream) {
    return update_prims(s, first, count, prims_dev, transforms_dev, stream, false, nullptr);
}
int rt_scene_update_prims_async(rt_scene *s, uint32_t first, uint32_t count, const rt_prim *prims_dev, const float *transforms_dev,
                                void *stream, uint64_t *ticket) {
    return update_prims(s, first, count, prims_dev, transforms_dev, stream, true, ticket);
}
int rt_scene_update_prims_host(rt_scene *s, uint32_t first, uint32_t count, const rt_prim *prims, const float *transforms) {
    bool empty = false;
    Staged d;
    int rc = update_refusals(s, first, count, prims, "records", false, false, "rt_scene_update_prims_host", &empty);
    if (rc != RT_OK || empty || (rc = stage(s, prims, sizeof(rt_prim) * (size_t)count, transforms, 64 * (size_t)count, d)) != RT_OK) return rc;
    return rt_scene_update_prims(s, first, count, (const rt_prim *)d.a, (const float *)d.b, s->stream);
}

int rt_scene_transform_triangles(rt_scene *s, const rt_tri_xform *ranges, uint32_t num_ranges, const float *rest_dev,
                                 void *stream) {
    return transform_triangles(s, ranges, num_ranges, rest_dev, stream, false, nullptr);
}
int rt_scene_transform_triangles_async(rt_scene *s, const rt_tri_xform *ranges, uint32_t num_ranges, const float *rest_dev,
                                       void *stream, uint64_t *ticket) {
    return transform_triangles(s, ranges, num_ranges, rest_dev, stream, true, ticket);
}

int rt_scene_update_sync(rt_scene *s, rt_update_status *out) {
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_update_sync: null scene");
    if (int rc = fold_updates(s); rc != RT_OK) return rc;
    AsyncUpdates &U = s->refit.async;
    if (out) *out = rt_update_status{U.submitted, U.applied, U.refused, U.first_refused};
    // the earliest refusal since the previous sync is named and then forgotten
    if (U.first_refused) (void)fail(RT_ERR_INVALID, std::string(kUpdateNames[U.first_kind]) + form_of(true) + ": " + kRefusals[U.first_kind]);
    U.first_refused = 0;
    U.first_kind = -1;
    return RT_OK;
}

int rt_scene_rebuild(rt_scene *s, void *stream) {
    return edit_call("rt_scene_rebuild", "", [&](const std::string &who, Rebuilt &t) -> int {
        if (!s) return fail(RT_ERR_INVALID, who + ": null scene");
        int rc = rebuild_supported(s, who);
        if (rc != RT_OK || (rc = enter(s)) != RT_OK || (rc = rebuild(s->refit, records_of(s), (hipStream_t)stream, t)) != RT_OK) return rc;
        swap_in_tree(s, t);
        return RT_OK;
    });
}
int rt_scene_rebuild_stats(const rt_scene *s, uint32_t out[4]) {
    if (!s || !out) return fail(RT_ERR_INVALID, "rt_scene_rebuild_stats: null argument");
    for (int k = 0; k < 4; ++k) out[k] = s->refit.rebuild_stats[k];
    return RT_OK;
}

int rt_scene_splice_triangles(rt_scene *s, uint32_t first, uint32_t remove, const rt_prim *prims_dev, uint32_t insert,
                              void *stream) {
    return edit_call("rt_scene_splice_triangles", "", [&](const std::string &who, Rebuilt &t) -> int {
        bool empty = false;
        int rc = splice_arguments(s, first, remove, prims_dev, insert, who, &empty);
        if (rc != RT_OK || empty || (rc = enter(s)) != RT_OK) return rc;
        const uint32_t n = s->num_prims - remove + insert;
        // the host's share, made before anything is swapped: the type bytes require_triangles reads
        // and an index array of the new size (sync_host_tree sizes its download from it)
        RefitState &R = s->refit;
        std::vector<uint8_t> pinfo;
        pinfo.reserve(n);
        pinfo.insert(pinfo.end(), R.pinfo.begin(), R.pinfo.begin() + first);
        pinfo.insert(pinfo.end(), insert, (uint8_t)RT_TRIANGLE);
        pinfo.insert(pinfo.end(), R.pinfo.begin() + first + remove, R.pinfo.end());
        std::vector<uint32_t> indices(n, 0u);
        const SpliceEdit e{first, remove, insert, prims_dev, s->num_materials};
        if ((rc = splice(R, records_of(s), e, (hipStream_t)stream, t)) != RT_OK) return rc;
        swap_in_splice(s, t, pinfo, indices);
        return RT_OK;
    });
}
int rt_scene_splice_triangles_host(rt_scene *s, uint32_t first, uint32_t remove, const rt_prim *prims, uint32_t insert) {
    bool empty = false;
    Staged d;
    int rc = splice_arguments(s, first, remove, prims, insert, "rt_scene_splice_triangles_host", &empty);
    if (rc != RT_OK || empty || (rc = stage(s, prims, sizeof(rt_prim) * (size_t)insert, nullptr, 0, d)) != RT_OK) return rc;
    return rt_scene_splice_triangles(s, first, remove, (const rt_prim *)d.a, insert, s->stream);
}

int rt_scene_splice_ranges(rt_scene *s, const rt_tri_edit *edits, uint32_t num_edits, const rt_prim *prims_dev, void *stream) {
    return splice_edits(s, edits, num_edits, prims_dev, nullptr, stream, false);
}
int rt_scene_splice_ranges_host(rt_scene *s, const rt_tri_edit *edits, uint32_t num_edits, const rt_prim *prims) {
    return splice_edits_host(s, edits, num_edits, prims, nullptr, false);
}
int rt_scene_splice_prims(rt_scene *s, const rt_prim_edit *edits, uint32_t num_edits, const rt_prim *prims_dev,
                          const float *transforms_dev, void *stream) {
    return splice_edits(s, edits, num_edits, prims_dev, transforms_dev, stream, true);
}
int rt_scene_splice_prims_host(rt_scene *s, const rt_prim_edit *edits, uint32_t num_edits, const rt_prim *prims,
                               const float *transforms) {
    return splice_edits_host(s, edits, num_edits, prims, transforms, true);
}

int rt_scene_compact_triangles(rt_scene *s, const uint8_t *keep_dev, void *stream) { return compact(s, keep_dev, stream, false); }
int rt_scene_compact_triangles_host(rt_scene *s, const uint8_t *keep) { return compact_host(s, keep, false); }
int rt_scene_compact_prims(rt_scene *s, const uint8_t *keep_dev, void *stream) { return compact(s, keep_dev, stream, true); }
int rt_scene_compact_prims_host(rt_scene *s, const uint8_t *keep) { return compact_host(s, keep, true); }

int rt_scene_set_prim_materials(rt_scene *s, uint32_t first, uint32_t count, const int32_t *materials_dev, void *stream) {
    return edit_call("rt_scene_set_prim_materials", "", [&](const std::string &who, Rebuilt &) -> int {
        bool empty = false;
        int rc = materials_arguments(s, first, count, materials_dev, who, &empty);
        if (rc != RT_OK || empty || (rc = enter(s)) != RT_OK) return rc;
        return set_materials(s->refit, records_of(s), first, count, materials_dev, s->num_materials, (hipStream_t)stream);
    });
}
int rt_scene_set_prim_materials_host(rt_scene *s, uint32_t first, uint32_t count, const int32_t *materials) {
    bool empty = false;
    Staged d;
    int rc = materials_arguments(s, first, count, materials, "rt_scene_set_prim_materials_host", &empty);
    if (rc != RT_OK || empty || (rc = stage(s, materials, sizeof(int32_t) * (size_t)count, nullptr, 0, d)) != RT_OK) return rc;
    return rt_scene_set_prim_materials(s, first, count, (const int32_t *)d.a, s->stream);
}

// ---- the refit schedule ahead of the first update (rt_plan.hip)

int rt_scene_prepare_updates(rt_scene *s, void *stream) {
    return edit_call("rt_scene_prepare_updates", "", [&](const std::string &who, Rebuilt &) -> int {
        if (!s) return fail(RT_ERR_INVALID, who + ": null scene");
        int rc = refit_supported(s, who);
        if (rc != RT_OK || (rc = enter(s)) != RT_OK) return rc;
        return prepare_updates(s->refit, records_of(s), (hipStream_t)stream);
    });
}

int rt_scene_update_plan_info(const rt_scene *s, uint32_t out[8]) {
    if (!s || !out) return fail(RT_ERR_INVALID, "rt_scene_update_plan_info: null argument");
    if (int frc = fold_updates(const_cast<rt_scene *>(s)); frc != RT_OK) return frc;
    const RefitState &R = s->refit;
    const PlanInfo none{}, &p = R.refit_ready ? R.plan_info : none;
    out[0] = R.refit_ready ? 1u : 0u;
    out[1] = p.route;
    out[2] = R.refit_ready ? R.plan.ntreelets : 0u;
    out[3] = R.refit_ready && R.plan.has_top ? 1u : 0u;
    out[4] = p.list_len;
    out[5] = p.lvl_len;
    out[6] = p.top_nodes;
    out[7] = p.launches;
    return RT_OK;
}

int rt_scene_copy_update_plan(const rt_scene *s, uint32_t *list, uint32_t *lvl, uint32_t *grp) {
    if (!s) return fail(RT_ERR_INVALID, "rt_scene_copy_update_plan: null scene");
    if (int frc = fold_updates(const_cast<rt_scene *>(s)); frc != RT_OK) return frc;
    const RefitState &R = s->refit;
    if (!R.refit_ready) return fail(RT_ERR_INVALID, "rt_scene_copy_update_plan: no schedule is ready (rt_scene_prepare_updates)");
    HIP_TRY(hipSetDevice(s->device));
    // the schedule's builder and every update block, so the arrays are settled
    if (list) HIP_TRY(hipMemcpy(list, R.d_list, sizeof(uint32_t) * R.plan_info.list_len, hipMemcpyDeviceToHost));
    if (lvl) HIP_TRY(hipMemcpy(lvl, R.d_lvl, sizeof(uint32_t) * R.plan_info.lvl_len, hipMemcpyDeviceToHost));
    if (grp) HIP_TRY(hipMemcpy(grp, R.d_grp, sizeof(uint32_t) * ((size_t)R.plan.ntreelets + 2), hipMemcpyDeviceToHost));
    return RT_OK;
}

}  // extern "C"
