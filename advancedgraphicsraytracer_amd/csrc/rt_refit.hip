// rt_refit.hip -- in-place updates with a bottom-up BVH refit: the kernels and the one host path.
//
// The tree's topology, primitive ids and leaf membership stay; what moves is rewritten by
//   k_check<Src>       one lane per primitive of the call: would its write produce a finite,
//                      admissible record (Src::ok)?  Sets the flag, writes nothing else;
//   k_write<Src>       one lane per primitive: its leaf-slot record, its shading record, its slot box
//                      and, for a cube or a quad, its side-table entry (Src::write) -- the
//                      rt_records.h encoders that scene creation runs, under the same
//                      -ffp-contract=off, so the records equal those of a fresh rt_scene_create;
//   k_refit_treelets   one workgroup per treelet (a whole subtree of at most kTreeletNodes nodes),
//                      one height at a time (refit_level), a barrier between heights;
//   k_refit_top        one workgroup, the same over the nodes above the cut.
// The stream-ordered updates run k_check as it is and then
//   k_write_if<Src>, k_refit_treelets_if, k_refit_top_if   the same text behind the gate: one
//                      wave-uniform load of the check's flag (written by an EARLIER launch), and a
//                      flagged update returns without a store;
//   k_settle           one lane books the outcome into the scene's status block and clears the flag.
// Src is one of the three sources of rt_update.h -- TriVerts (rt_scene_update_triangles), TriXform
// (rt_scene_transform_triangles), PrimRecs (rt_scene_update_prims) -- and rt_update.h holds every
// line a lane runs, so the CPU tests run the kernels' own text.
// Boxes go through global memory: the waves of a workgroup share their CU's vector L1, so what one
// wave stored before the barrier another loads after it.  Nothing is handed from one workgroup to
// another inside a launch (the XCDs' L2s are not coherent with each other, and a CU's L1 is not
// refreshed by another CU's stores): the top reads the treelets' roots across the kernel boundary.
#include "rt_refit.h"

#include <cmath>
#include <cstddef>
#include <cstring>

namespace rt {

namespace {

template <class Src>
__global__ void __launch_bounds__(256) k_check(RefitArgs A, Src src, uint32_t n, uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && !src.ok(A, i)) *flag = 1u;
}
template <class Src>
__global__ void __launch_bounds__(256) k_write(RefitArgs A, Src src, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) src.write(A, i);
}

// group g's heights in turn; every wave of the workgroup takes every barrier
__device__ __forceinline__ void refit_group(const RefitArgs &A, uint32_t g) {
    const uint32_t l1 = A.grp[g + 1] - 1u;
    for (uint32_t l = A.grp[g]; l < l1; ++l) {
        refit_level(A, l, threadIdx.x, blockDim.x);
        __syncthreads();
    }
}
__global__ void __launch_bounds__(256) k_refit_treelets(RefitArgs A) { refit_group(A, blockIdx.x); }
__global__ void __launch_bounds__(1024) k_refit_top(RefitArgs A, uint32_t g) { refit_group(A, g); }

// ---- behind the gate (update_gated, rt_update.h).  The flag's address is the same for every lane and
// the launch that wrote it has ended, so every wave of a launch takes the same side: all of a
// workgroup's waves reach refit_group's barriers or none does.
template <class Src>
__global__ void __launch_bounds__(256) k_write_if(RefitArgs A, Src src, uint32_t n, const UpdateStatus *status) {
    if (update_gated(status)) return;
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) src.write(A, i);
}
__global__ void __launch_bounds__(256) k_refit_treelets_if(RefitArgs A, const UpdateStatus *status) {
    if (update_gated(status)) return;
    refit_group(A, blockIdx.x);
}
__global__ void __launch_bounds__(1024) k_refit_top_if(RefitArgs A, uint32_t g, const UpdateStatus *status) {
    if (update_gated(status)) return;
    refit_group(A, g);
}
__global__ void __launch_bounds__(64) k_settle(UpdateStatus *status, uint64_t ticket) {
    if (blockIdx.x == 0 && threadIdx.x == 0) settle_update(status, ticket);
}

// the refit schedule of the current topology on the device: built there (rt_plan.hip) on the first
// update of a scene and on the first after a rebuild, unless rt_scene_prepare_updates did so before
// (the slot map, the slot boxes and the centroids stay the device's)
int ensure_refit(RefitState &R, const SceneRecords &S, hipStream_t st) {
    if (R.refit_ready) return RT_OK;
    int rc = ensure_state(R, S);
    if (rc != RT_OK) return rc;
    if ((rc = plan_on_device(R, S, st)) != RT_OK || R.refit_ready) return rc;
    // no tree (a child pair with two parents in a caller's prebuilt node array): the host's walk
    // schedules what it meets, as it always did
    if ((rc = sync_host_tree(R, *S.bvh, S.nodes)) != RT_OK) return rc;
    if (!build_refit_plan(*S.bvh, S.num_prims, R.plan)) return fail(RT_ERR_UNSUPPORTED, "refit: not a plain tree");
    rc = upload(&R.d_list, R.plan.list);
    if (rc == RT_OK) rc = upload(&R.d_lvl, R.plan.lvl);
    if (rc == RT_OK) rc = upload(&R.d_grp, R.plan.grp);
    if (rc != RT_OK) {
        for (void **p : {&R.d_list, &R.d_lvl, &R.d_grp}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        return rc;
    }
    const uint32_t listed = (uint32_t)R.plan.list.size();
    R.plan_info = PlanInfo{1u, listed, (uint32_t)R.plan.lvl.size(), listed - R.plan.lvl[R.plan.grp[R.plan.ntreelets]], 0u};
    for (std::vector<uint32_t> *v : {&R.plan.slot_of, &R.plan.list, &R.plan.lvl, &R.plan.grp}) std::vector<uint32_t>().swap(*v);
    R.refit_ready = true;
    return RT_OK;
}

RefitArgs refit_args(const RefitState &R, const SceneRecords &S) {
    RefitArgs A{};
    A.nodes = (float4 *)S.nodes; A.prims = (float4 *)S.prims; A.shade = (float4 *)S.shade; A.xprims = (float4 *)S.xprims;
    A.slot_box = (float4 *)R.d_slot_box;
    A.slot_of = (const uint32_t *)R.d_slot_of; A.list = (const uint32_t *)R.d_list;
    A.lvl = (const uint32_t *)R.d_lvl; A.grp = (const uint32_t *)R.d_grp;
    A.margin = S.margin;
    A.sliver_lim = R.sliver_lim;
    A.cen = (float4 *)R.d_cen;
    return A;
}

}  // namespace

int ensure_state(RefitState &R, const SceneRecords &S) {
    if (R.state_ready) return RT_OK;
    // never updated, never rebuilt: the host tree and creation's per-primitive copies are current
    // a plain tree holds every id in exactly one slot (a tree out of build_tree does by construction)
    std::vector<uint32_t> slot_of(S.num_prims, ~0u);
    if (S.bvh->indices.size() != S.num_prims) return fail(RT_ERR_UNSUPPORTED, "refit: not a plain tree");
    for (uint32_t k = 0; k < S.num_prims; ++k) {
        const uint32_t id = S.bvh->indices[k];
        if (id >= S.num_prims || slot_of[id] != ~0u) return fail(RT_ERR_UNSUPPORTED, "refit: not a plain tree");
        slot_of[id] = k;
    }
    std::vector<float4> box, cen(S.num_prims);
    seed_slot_boxes(*S.bvh, R.pinfo, R.pbox, box);
    for (uint32_t i = 0; i < S.num_prims; ++i) cen[i] = make_float4(R.pcen[3 * (size_t)i], R.pcen[3 * (size_t)i + 1], R.pcen[3 * (size_t)i + 2], 0.0f);
    int rc = upload(&R.d_slot_of, slot_of);
    if (rc == RT_OK) rc = upload(&R.d_slot_box, box);
    if (rc == RT_OK) rc = upload(&R.d_cen, cen);
    if (rc == RT_OK && !R.d_flag && hipMalloc(&R.d_flag, 16) != hipSuccess) rc = fail(RT_ERR_HIP, "hipMalloc failed");
    if (rc != RT_OK) {
        for (void **p : {&R.d_slot_of, &R.d_slot_box, &R.d_cen}) {
            if (*p) (void)hipFree(*p);
            *p = nullptr;
        }
        return rc;
    }
    std::vector<float>().swap(R.pbox);   // the boxes and the centroids live on the device from here on
    std::vector<float>().swap(R.pcen);
    R.state_ready = true;
    return RT_OK;
}

int sync_host_tree(RefitState &R, Bvh &b, const void *d_nodes) {
    if (!R.bvh_stale && !R.topo_stale) return RT_OK;
    std::vector<float4> dn(2 * (size_t)b.nodes_used);
    HIP_TRY(hipMemcpy(dn.data(), d_nodes, sizeof(float4) * dn.size(), hipMemcpyDeviceToHost));
    if (R.topo_stale) {
        b.nodes.assign(std::max<size_t>(2 * b.indices.size() + 2, b.nodes_used), Node{});
        HIP_TRY(hipMemcpy(b.indices.data(), R.d_index, sizeof(uint32_t) * b.indices.size(), hipMemcpyDeviceToHost));
    }
    for (uint32_t i = 0; i < b.nodes_used; ++i) {
        Node &nd = b.nodes[i];
        f3 mn, mx;
        node_box(dn[2 * (size_t)i], dn[2 * (size_t)i + 1], mn, mx);
        nd.mn[0] = mn.x; nd.mn[1] = mn.y; nd.mn[2] = mn.z;
        nd.mx[0] = mx.x; nd.mx[1] = mx.y; nd.mx[2] = mx.z;
        if (R.topo_stale) {
            const uint32_t word = fbits(dn[2 * (size_t)i + 1].z);
            nd.leftFirst = word >> 8;
            nd.count = word & 255u;
        }
    }
    R.bvh_stale = R.topo_stale = false;
    return RT_OK;
}

int prepare_updates(RefitState &R, const SceneRecords &S, hipStream_t st) {
    HIP_TRY(hipDeviceSynchronize());   // frames still reading the scene on any stream
    if (R.refit_ready) {
        R.plan_info.launches = 0u;
        return RT_OK;
    }
    return ensure_refit(R, S, st);
}

void free_refit(RefitState &R) {
    R.state_ready = false;
    for (void **p : {&R.d_slot_of, &R.d_slot_box, &R.d_list, &R.d_lvl, &R.d_grp, &R.d_flag, &R.d_ranges, &R.d_cen, &R.d_index, &R.d_types}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    R.ranges_bytes = 0;
    R.types_bytes = 0;
    R.refit_ready = false;
    R.plan_info = PlanInfo{};
    AsyncUpdates &U = R.async;
    if (U.status) (void)hipFree(U.status);
    if (U.done) (void)hipEventDestroy(U.done);
    for (XformSlot &x : U.ring) {
        if (x.host) (void)hipHostFree(x.host);
        (void)x.dev.release();
        if (x.ev) (void)hipEventDestroy(x.ev);
    }
    U = AsyncUpdates{};
}

template <class Src>
int update(RefitState &R, const SceneRecords &S, const Src &src, uint32_t n, hipStream_t st, const char *who, const char *refusal,
           const UpdateCopy *copies, int ncopies, bool *finite) {
    HIP_TRY(hipDeviceSynchronize());   // frames still reading the scene on any stream
    int rc = ensure_refit(R, S, st);
    if (rc != RT_OK) return rc;
    const RefitArgs A = refit_args(R, S);
    const dim3 grid((n + 255u) / 256u), block(256);
    // the check is a pass of its own, its flag read back before anything is written
    uint32_t bad = 0;
    uint32_t *flag = (uint32_t *)R.d_flag;
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    for (const UpdateCopy *c = copies; c < copies + ncopies; ++c) HIP_TRY(hipMemcpyAsync(c->dst, c->src, c->bytes, c->kind, st));
    hipLaunchKernelGGL(k_check<Src>, grid, block, 0, st, A, src, n, flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(RT_ERR_INVALID, std::string(who) + ": " + refusal);
    hipLaunchKernelGGL(k_write<Src>, grid, block, 0, st, A, src, n);
    // the treelets, then (a second launch) the nodes above the cut
    hipLaunchKernelGGL(k_refit_treelets, dim3(R.plan.ntreelets), dim3(256), 0, st, A);
    if (R.plan.has_top) hipLaunchKernelGGL(k_refit_top, dim3(1), dim3(1024), 0, st, A, R.plan.ntreelets);
    HIP_TRY(hipGetLastError());
    R.bvh_stale = true;
    // the scene's flags follow from the new root box: every box is the union of the boxes below it
    float4 root[2];
    HIP_TRY(hipMemcpyAsync(root, S.nodes, sizeof(root), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *finite = R.boxes_finite;
    for (float f : {root[0].x, root[0].y, root[0].z, root[0].w, root[1].x, root[1].y}) *finite = *finite && std::isfinite(f);
    return RT_OK;
}
template int update<TriVerts>(RefitState &, const SceneRecords &, const TriVerts &, uint32_t, hipStream_t, const char *, const char *,
                              const UpdateCopy *, int, bool *);
template int update<PrimRecs>(RefitState &, const SceneRecords &, const PrimRecs &, uint32_t, hipStream_t, const char *, const char *,
                              const UpdateCopy *, int, bool *);

// ---- the stream-ordered path

int drain_updates(RefitState &R, uint64_t *applied_new) {
    AsyncUpdates &U = R.async;
    if (applied_new) *applied_new = 0;
    if (!U.issued) return RT_OK;
    HIP_TRY(hipEventSynchronize(U.done));   // every async update waited for the one before it
    UpdateStatus h{};
    HIP_TRY(hipMemcpy(&h, U.status, sizeof(h), hipMemcpyDeviceToHost));
    if (h.first_refused) {
        if (!U.first_refused) {
            U.first_refused = h.first_refused;
            U.first_kind = U.kinds[(size_t)(h.first_refused - U.folded - 1u)];
        }
        HIP_TRY(hipMemset((char *)U.status + offsetof(UpdateStatus, first_refused), 0, sizeof(uint64_t)));
    }
    if (applied_new) *applied_new = h.applied - U.applied;
    U.applied = h.applied;
    U.refused = h.refused;
    U.folded = U.submitted;
    U.kinds.clear();
    U.issued = false;
    return RT_OK;
}

// the status block and the event, once per scene (blocks: the block is cleared with a plain memset)
static int ensure_async(AsyncUpdates &U) {
    if (U.status) return RT_OK;
    if (!U.done) HIP_TRY(hipEventCreateWithFlags(&U.done, hipEventDisableTiming));
    void *p = nullptr;
    HIP_TRY(hipMalloc(&p, sizeof(UpdateStatus)));
    if (hipMemset(p, 0, sizeof(UpdateStatus)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        (void)hipFree(p);
        return fail(RT_ERR_HIP, "hipMemset failed");
    }
    U.status = p;
    return RT_OK;
}

template <class Src>
int update_async(RefitState &R, const SceneRecords &S, const Src &src, uint32_t n, hipStream_t st, int kind,
                 const UpdateCopy *copies, int ncopies, uint64_t *ticket_out) {
    AsyncUpdates &U = R.async;
    int rc = RT_OK;
    if (!R.refit_ready || !U.status) {
        // no schedule (the scene's first update, or the first after a rebuild), or no status block
        // yet: built here, behind everything that still reads the scene -- the one blocking case
        if ((rc = drain_updates(R, nullptr)) != RT_OK) return rc;
        HIP_TRY(hipDeviceSynchronize());
        if ((rc = ensure_refit(R, S, st)) != RT_OK || (rc = ensure_async(U)) != RT_OK) return rc;
    }
    const RefitArgs A = refit_args(R, S);
    UpdateStatus *status = (UpdateStatus *)U.status;
    const dim3 grid((n + 255u) / 256u), block(256);
    // behind the previous async update, whatever stream it ran on: the block has one writer
    if (U.issued) HIP_TRY(hipStreamWaitEvent(st, U.done, 0));
    for (const UpdateCopy *c = copies; c < copies + ncopies; ++c) HIP_TRY(hipMemcpyAsync(c->dst, c->src, c->bytes, c->kind, st));
    const uint64_t ticket = U.submitted + 1u;
    // the check is a pass of its own; its flag stays on the device, where the launches below read it
    hipLaunchKernelGGL(k_check<Src>, grid, block, 0, st, A, src, n, &status->flag);
    hipLaunchKernelGGL(k_write_if<Src>, grid, block, 0, st, A, src, n, (const UpdateStatus *)status);
    hipLaunchKernelGGL(k_refit_treelets_if, dim3(R.plan.ntreelets), dim3(256), 0, st, A, (const UpdateStatus *)status);
    if (R.plan.has_top)
        hipLaunchKernelGGL(k_refit_top_if, dim3(1), dim3(1024), 0, st, A, R.plan.ntreelets, (const UpdateStatus *)status);
    hipLaunchKernelGGL(k_settle, dim3(1), dim3(64), 0, st, status, ticket);
    const hipError_t launched = hipGetLastError();
    // whatever was enqueued, the scene's readers and the next update wait for it
    const hipError_t recorded = hipEventRecord(U.done, st);
    U.issued = true;
    R.bvh_stale = true;
    U.submitted = ticket;
    U.kinds.push_back((uint8_t)kind);
    HIP_TRY(launched);
    HIP_TRY(recorded);
    if (ticket_out) *ticket_out = ticket;
    return RT_OK;
}
template int update_async<TriVerts>(RefitState &, const SceneRecords &, const TriVerts &, uint32_t, hipStream_t, int,
                                    const UpdateCopy *, int, uint64_t *);
template int update_async<PrimRecs>(RefitState &, const SceneRecords &, const PrimRecs &, uint32_t, hipStream_t, int,
                                    const UpdateCopy *, int, uint64_t *);

int update_xform_async(RefitState &R, const SceneRecords &S, const std::vector<uint32_t> &tab, uint32_t nr, const float *rest_dev,
                       hipStream_t st, uint64_t *ticket_out) {
    AsyncUpdates &U = R.async;
    XformSlot &x = U.ring[U.ring_next];
    const size_t need = sizeof(uint32_t) * tab.size();
    // the slot's last update, kXformSlots calls ago, has read it: the one wait of this call, and it
    // returns at once unless all the slots are in flight
    if (x.used) HIP_TRY(hipEventSynchronize(x.ev));
    if (!x.ev) HIP_TRY(hipEventCreateWithFlags(&x.ev, hipEventDisableTiming));
    if (need > x.dev.bytes) {
        const size_t cap = std::max<size_t>(4096, 2 * need);
        if (int rc = x.dev.release(); rc != RT_OK) return rc;   // (first: the size that admits a table is the device twin's)
        if (x.host) HIP_TRY(hipHostFree(x.host));
        x.host = nullptr;
        HIP_TRY(hipHostMalloc(&x.host, cap, hipHostMallocDefault));
        if (int rc = x.dev.grow(cap); rc != RT_OK) return rc;
    }
    std::memcpy(x.host, tab.data(), need);
    TriXform src{};
    src.R.first = x.dev.as<const uint32_t>();
    src.R.pre = src.R.first + nr;
    src.R.M = (const float *)(src.R.pre + nr + 1);
    src.R.nr = nr;
    src.rest = rest_dev;
    const UpdateCopy table{x.dev.p, x.host, need, hipMemcpyHostToDevice};
    const uint64_t before = U.submitted;
    const int rc = update_async(R, S, src, tab[2 * (size_t)nr], st, 1, &table, 1, ticket_out);
    if (U.submitted != before) {   // enqueued (even where a later step failed): the slot is taken
        x.used = true;
        U.ring_next = (U.ring_next + 1u) % (uint32_t)kXformSlots;
        HIP_TRY(hipEventRecord(x.ev, st));
    }
    return rc;
}

int update_xform(RefitState &R, const SceneRecords &S, const std::vector<uint32_t> &tab, uint32_t nr, const float *rest_dev,
                 hipStream_t st, const char *who, const char *refusal, bool *finite) {
    const size_t need = sizeof(uint32_t) * tab.size();
    int rc = grow(&R.d_ranges, &R.ranges_bytes, need);
    if (rc != RT_OK) return rc;
    TriXform src{};
    src.R.first = (const uint32_t *)R.d_ranges;
    src.R.pre = src.R.first + nr;
    src.R.M = (const float *)(src.R.pre + nr + 1);
    src.R.nr = nr;
    src.rest = rest_dev;
    // the table has left the host vector at update's synchronise after the check
    const UpdateCopy table{R.d_ranges, tab.data(), need, hipMemcpyHostToDevice};
    return update(R, S, src, tab[2 * (size_t)nr], st, who, refusal, &table, 1, finite);
}

}  // namespace rt
