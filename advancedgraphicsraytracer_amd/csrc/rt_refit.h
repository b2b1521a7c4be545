// rt_refit.h -- in-place updates: the refit plan of a scene's tree (built in rt_scene_pack.cpp),
// the update state a scene keeps, and the one host path of rt_refit.hip that every update entry
// point of rt_scene_edit.hip takes (rt_scene_update_triangles, rt_scene_update_prims,
// rt_scene_transform_triangles), with its stream-ordered form (update_async; the rt_scene_*_async
// entry points and rt_scene_update_sync).  The per-lane text is in rt_update.h.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <vector>

#include "rt_internal.h"
#include "rt_update.h"

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(e_ == hipErrorNoBinaryForGpu || e_ == hipErrorInvalidDeviceFunction    \
                            ? RT_ERR_NO_DEVICE : RT_ERR_HIP,                                   \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                   \
    } while (0)

namespace rt {

// An owned, growable device buffer: the one text that frees and allocates.  grow() leaves a buffer of
// at least `need` bytes (the old block is freed, its contents are not kept) and says what has to
// finish before the old block goes: nothing (hipFree itself), the stream that used it, or every
// stream of the device.  A buffer that is large enough costs one comparison.
enum class Wait { kNone, kStream, kDevice };
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;

    template <class T>
    T *as() const { return static_cast<T *>(p); }
    int release() {
        if (p) HIP_TRY(hipFree(p));
        p = nullptr;
        bytes = 0;
        return RT_OK;
    }
    int grow(size_t need, Wait wait = Wait::kNone, hipStream_t st = nullptr) {
        if (need <= bytes) return RT_OK;
        if (wait == Wait::kStream) HIP_TRY(hipStreamSynchronize(st));
        if (wait == Wait::kDevice) HIP_TRY(hipDeviceSynchronize());
        if (int rc = release(); rc != RT_OK) return rc;
        HIP_TRY(hipMalloc(&p, need));
        bytes = need;
        return RT_OK;
    }
};

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
// where and how the schedule on the device was built (rt_scene_update_plan_info): route 0 none,
// 1 host (build_refit_plan, uploaded), 2 GPU in many launches, 3 GPU in one workgroup (rt_plan.h);
// launches: of the call that last asked for the schedule -- 0 where it stood ready
struct PlanInfo { uint32_t route = 0, list_len = 0, lvl_len = 0, top_nodes = 0, launches = 0; };
// the slot boxes a refit starts from: per leaf slot k the box and sticky flag (pbox, pinfo of
// ScenePack) of primitive indices[k]
void seed_slot_boxes(const Bvh &b, const std::vector<uint8_t> &pinfo, const std::vector<float> &pbox, std::vector<float4> &out);

// What a scene keeps for its updates and for nothing else.  Kept from creation: per primitive its
// type | sticky << 7 (mark_sticky) and its box (prim_geometry; 6 floats) -- what a refit needs of
// the primitives that do not move -- and its centroid, which a rebuild bins by.  The first update or
// rebuild puts slot map, slot boxes and centroids on the device, where they live from there on; the
// schedule is built on the device (rt_plan.hip) by rt_scene_prepare_updates or else by the first
// update, and again after a rebuild (rt_build.hip).
// What a scene keeps for its stream-ordered updates, made by the first of them.
//   status   the device block the kernels gate on and book into (UpdateStatus, rt_update.h);
//   done     ONE event, recorded after every async update's settle step: whatever reads the scene
//            afterwards waits on it (hipStreamWaitEvent) while `issued` is set, and so does the next
//            async update, whose stream may be another -- the block has one writer at a time;
//   ring     rt_scene_transform_triangles_async's range tables: kXformSlots pinned host slots, each
//            with its device twin and the event of the update that read it.  A slot is taken again
//            kXformSlots updates later; the call waits for its event only then.
// The host's counts are folded from the block by drain_updates; kinds holds, per ticket since the
// last fold, which entry point it came from (update_async's `kind`).
constexpr int kXformSlots = 8;
struct XformSlot {
    void *host = nullptr;           // pinned, as large as dev
    DevBuf dev;
    hipEvent_t ev = nullptr;
    bool used = false;
};
struct AsyncUpdates {
    void *status = nullptr;
    hipEvent_t done = nullptr;
    bool issued = false;            // an async update was enqueued since the last fold
    uint64_t submitted = 0, applied = 0, refused = 0, first_refused = 0;
    uint64_t folded = 0;            // tickets <= this are folded into the counts
    int first_kind = -1;            // ... of the ticket first_refused (-1: none)
    std::vector<uint8_t> kinds;     // ticket folded + 1 + k -> index into the refusal texts
    XformSlot ring[kXformSlots];
    uint32_t ring_next = 0;
};

struct RefitState {
    std::vector<uint8_t> pinfo;
    std::vector<float> pbox;
    std::vector<float> pcen;        // and its centroid (3 floats): what a rebuild bins by (rt_build.h)
    double sliver_lim = 0.0;        // mark_sticky's sine limit at creation (RT_WALK_STICKY)
    bool sticky_spheres = true;     // ... and its rule for spheres and quads (RT_WALK_STICKY_SPHERES): both are
                                    // read at creation only, and an inserted record is marked by them
    bool boxes_finite = true;       // every primitive box was finite at creation
    bool state_ready = false;       // slot_of, slot_box and cen are on the device (and authoritative from there on)
    bool refit_ready = false;       // ... and so is the schedule of the current topology
    RefitPlan plan;                 // ntreelets and has_top of the device schedule (the vectors are not kept)
    PlanInfo plan_info;
    void *d_cen = nullptr;          // per id its centroid (float4)
    void *d_index = nullptr;        // after a rebuild: the new primitive-index array (slot -> id)
    bool topo_stale = false;        // a rebuild changed the topology: the host tree is downloaded whole before its next use
    uint32_t rebuild_stats[4] = {0, 0, 0, 0};
    void *d_slot_of = nullptr, *d_slot_box = nullptr, *d_list = nullptr, *d_lvl = nullptr, *d_grp = nullptr, *d_flag = nullptr;
    bool bvh_stale = false;         // the device boxes are newer than the host tree (rt_scene_copy_bvh downloads them)
    void *d_ranges = nullptr;       // rt_scene_transform_triangles' range table (first, prefix counts, matrices)
    size_t ranges_bytes = 0;
    void *d_types = nullptr;        // rt_scene_splice_prims' check: the inserted records' type bytes, kept between calls
    size_t types_bytes = 0;
    AsyncUpdates async;             // stream-ordered updates (update_async)
};
void free_refit(RefitState &R);

// the scene's side of an update: its tree and its device records
struct SceneRecords {
    Bvh *bvh;
    uint32_t num_prims;
    void *nodes, *prims, *shade, *xprims;
    float margin;   // SceneView::walk_margin
};

// the same for a pointer and a size kept apart (the scene's staging, its range table, its type bytes)
inline int grow(void **buf, size_t *have, size_t need) {
    DevBuf b{*buf, *have};
    const int rc = b.grow(need);
    *buf = b.p;
    *have = b.bytes;
    return rc;
}
template <typename T>
int upload(void **dst, const std::vector<T> &src) {
    HIP_TRY(hipMalloc(dst, std::max<size_t>(sizeof(T) * src.size(), 16)));
    if (!src.empty()) HIP_TRY(hipMemcpy(*dst, src.data(), sizeof(T) * src.size(), hipMemcpyHostToDevice));
    return RT_OK;
}

// a copy that rides along with an update, enqueued on its stream before the one synchronise that
// follows the check
struct UpdateCopy {
    void *dst;
    const void *src;
    size_t bytes;
    hipMemcpyKind kind;
};
// One in-place update of n lanes of `src` (TriVerts, TriXform or PrimRecs over device memory) on
// `st`: waits for the frames still reading the scene, builds the plan on the scene's first update,
// runs the check and reads its flag back -- a refusal (RT_ERR_INVALID, "<who>: <refusal>") has written
// nothing --, then the write, the refit of every treelet and of the nodes above the cut, and the
// new root box.  Blocks.  *finite = every box of the tree is finite now.
template <class Src>
int update(RefitState &R, const SceneRecords &S, const Src &src, uint32_t n, hipStream_t st, const char *who, const char *refusal,
           const UpdateCopy *copies, int ncopies, bool *finite);
// the same for ranges of triangles moved by one matrix each; tab = first[nr], prefix counts[nr + 1],
// matrices[16 nr], uploaded to the scene's range table
int update_xform(RefitState &R, const SceneRecords &S, const std::vector<uint32_t> &tab, uint32_t nr, const float *rest_dev,
                 hipStream_t st, const char *who, const char *refusal, bool *finite);
// The stream-ordered form of update(): everything is enqueued on `st` and the call returns.  Order:
// wait for the scene's previous async update (any stream), the copies, the check (its flag stays on
// the device), the gated write and refits, the settle step under `ticket` (= ++submitted), the
// scene's event.  Blocks only to build a missing schedule (ensure_refit) and to create the status
// block on a scene's first call.  `kind`: which entry point it is (0 rt_scene_update_triangles_async,
// 1 rt_scene_transform_triangles_async, 2 rt_scene_update_prims_async), kept per ticket for the text of a
// refusal (kRefusals, rt_scene_edit.hip).  *ticket_out may be null.
template <class Src>
int update_async(RefitState &R, const SceneRecords &S, const Src &src, uint32_t n, hipStream_t st, int kind,
                 const UpdateCopy *copies, int ncopies, uint64_t *ticket_out);
// ... for ranges of triangles: the table goes through the next slot of the ring (a bounded wait when
// all kXformSlots are in flight)
int update_xform_async(RefitState &R, const SceneRecords &S, const std::vector<uint32_t> &tab, uint32_t nr, const float *rest_dev,
                       hipStream_t st, uint64_t *ticket_out);
// Waits for every enqueued async update and folds the block into the host's counts; *applied_new =
// how many applied since the last fold.  Where none is pending it costs one branch.
int drain_updates(RefitState &R, uint64_t *applied_new);

// The schedule of the current topology (d_list, d_lvl, d_grp, plan.ntreelets, plan.has_top) built
// on `st` from the device node array (rt_plan.hip); blocks.  The host tree is neither read nor
// downloaded.  RT_OK with refit_ready still false: the nodes reached from the root are no tree
// (rt_plan.h, kPlanNotTree) and the caller takes the host's walk.
int plan_on_device(RefitState &R, const SceneRecords &S, hipStream_t st);
// rt_scene_prepare_updates: the update state and the schedule on the device now; blocks like an
// update, launches nothing where both stand ready
int prepare_updates(RefitState &R, const SceneRecords &S, hipStream_t st);

// the host tree from the device's after a refit (boxes) or a rebuild (nodes and indices)
int sync_host_tree(RefitState &R, Bvh &b, const void *d_nodes);
// slot_of, slot_box and the centroids on the device, from creation's host copies, once per scene
int ensure_state(RefitState &R, const SceneRecords &S);

// A rebuild's result (rt_build.hip): fresh device buffers for the caller to swap in, and the tree's figures.
struct Rebuilt {
    void *nodes = nullptr, *prims = nullptr, *slot_box = nullptr, *slot_of = nullptr, *index = nullptr;
    void *shade = nullptr, *cen = nullptr;   // a splice's new id space (rt_splice.hip); a rebuild leaves them null
    void *xprims = nullptr;                  // ... and its side table, where kinds entered or left (null: the scene's stays)
    uint32_t nodes_used = 0, depth = 0, max_leaf = 0, root_word = 0;
    bool finite = false;
    uint32_t stats[4] = {0, 0, 0, 0};
};
void free_rebuilt(Rebuilt &r);
// What the builder reads, all on the device: per id the centroid (float4), per old leaf slot the box
// (2 float4) and the leaf-slot record (3 float4), and id -> old slot.  who: the entry point, for messages.
struct BuildInputs {
    uint32_t n;
    const void *cen, *box, *slot_of, *prims;
    float margin;
    const char *who;
};
// Builds the tree rt_bvh_build_host would build for those primitives into fresh buffers on `st`
// (nodes, prims, slot_box, slot_of and index of `out`); blocks.  RT_ERR_UNSUPPORTED when the tree
// breaks a kernel limit; after any error every buffer of `out` is freed.
int build_tree(const BuildInputs &in, hipStream_t st, Rebuilt &out);
// The same for the scene's current primitives.  Nothing of the scene is written.
int rebuild(RefitState &R, const SceneRecords &S, hipStream_t st, Rebuilt &out);

// rt_scene_splice_triangles (rt_splice.hip): ids [first, first + remove) leave, `insert` triangles
// (recs_dev: DEVICE rt_prim) enter at id `first`
struct SpliceEdit {
    uint32_t first, remove, insert;
    const rt_prim *recs_dev;
    uint32_t num_materials;
};
// Checks the inserted records (RT_ERR_INVALID), forms the new id space in fresh buffers (shade and
// cen of `out`) and builds its tree (build_tree) on `st`; blocks.  Nothing of the scene is written,
// and after any error nothing is left allocated.
int splice(RefitState &R, const SceneRecords &S, const SpliceEdit &E, hipStream_t st, Rebuilt &out);
// rt_scene_splice_ranges: the same for many edits at once.  rows: HOST, the sorted table of splice_plan
// (rt_splice.h); recs_dev: DEVICE, total_insert records, every edit's back to back in the caller's order
// K (below) non-null: rt_scene_splice_prims, records of any kind.
struct SpliceRow;
struct SpliceKinds;
int splice_ranges(RefitState &R, const SceneRecords &S, const SpliceRow *rows, uint32_t num_rows, uint32_t n_new, uint32_t total_insert,
                  const rt_prim *recs_dev, uint32_t num_materials, hipStream_t st, Rebuilt &out, SpliceKinds *K = nullptr);
// rt_scene_compact_triangles: the primitives i with keep_dev[i] != 0 (DEVICE, num_prims bytes) stay.
// Checks the mask (RT_ERR_INVALID), counts the survivors into *n_new and downloads the mask into `keep`;
// where all stay, that is all it does and `out` stays empty.  Else as splice.
// K non-null: rt_scene_compact_prims, anything but primitive 0 may leave.
int splice_mask(RefitState &R, const SceneRecords &S, const uint8_t *keep_dev, hipStream_t st, std::vector<uint8_t> &keep, uint32_t *n_new,
                Rebuilt &out, SpliceKinds *K = nullptr);
// Primitives of every kind through the two routes above: the check admits the five kinds,
// the side-table ranks of the new id space are counted, and the gather writes a new side table
// (Rebuilt::xprims).  In: one mat4 per inserted record on the DEVICE (null: identity).  Out: the type
// bytes of the new id space, from which the caller takes RefitState::pinfo and the kernel family.
struct SpliceKinds {
    const float *T_dev = nullptr;
    std::vector<uint8_t> types;
};
// rt_scene_set_prim_materials: checks mats_dev[0 .. count) against num_materials in a pass of its own
// (RT_ERR_INVALID, nothing written), then writes the material words of [first, first + count).  Blocks.
int set_materials(RefitState &R, const SceneRecords &S, uint32_t first, uint32_t count, const int32_t *mats_dev, uint32_t num_materials,
                  hipStream_t st);

}  // namespace rt
