// rt_splice.hip -- triangles leave and enter a live scene: the kernels and the host
// path of rt::splice.
//
// rt_splice.h holds every line a lane runs; the kernels here supply the lane index:
//   k_splice_check    one lane per inserted record: a triangle of one of the scene's materials with
//                     finite vertices (splice_ok)?  Sets the flag, writes nothing else;
//   k_splice_gather   one lane per NEW id, consecutive lanes on consecutive ids: the kept primitives'
//                     records copied with the id word patched, the inserted triangles' written by the
//                     encoders scene creation runs, everything in id order into fresh buffers.
// The builder (build_tree of rt_build.hip) then runs over the new id space with the identity as its
// old slot map.  Nothing is handed from one workgroup to another inside a launch: launch boundaries
// order check -> gather -> build.  The scene's own buffers are only read; the caller swaps the new
// ones in when everything succeeded (rt_scene_splice_triangles in rt_device.hip).
#include "rt_refit.h"
#include "rt_splice.h"

namespace rt {

namespace {

__global__ void __launch_bounds__(256) k_splice_check(SpliceArgs A, uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < A.insert && !splice_ok(A, i)) *flag = 1u;
}
__global__ void __launch_bounds__(256) k_splice_gather(SpliceArgs A) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < A.n_new) splice_gather(A, j);
}

}  // namespace

int splice(RefitState &R, const SceneRecords &S, const SpliceEdit &E, hipStream_t st, Rebuilt &out) {
    const char *who = "rt_scene_splice_triangles";
    HIP_TRY(hipDeviceSynchronize());   // frames still reading the scene on any stream
    // A scene never updated seeds its state from the host tree.  One that has its state on the device
    // needs no host tree here: a stale one stays stale, and the download of a whole tree (0.2 ms for
    // mig29 x16) is left to whoever reads it next
    int rc = RT_OK;
    if (!R.state_ready) {
        rc = sync_host_tree(R, *S.bvh, S.nodes);
        if (rc == RT_OK) rc = ensure_state(R, S);
    }
    if (rc != RT_OK) return rc;
    const uint32_t n = S.num_prims - E.remove + E.insert;
    SpliceArgs A{};
    A.n_new = n; A.first = E.first; A.remove = E.remove; A.insert = E.insert;
    A.recs = E.recs_dev;
    A.num_materials = E.num_materials;
    A.sliver_lim = R.sliver_lim;
    A.old_prims = (const float4 *)S.prims; A.old_shade = (const float4 *)S.shade;
    A.old_cen = (const float4 *)R.d_cen; A.old_box = (const float4 *)R.d_slot_box;
    A.old_slot_of = (const uint32_t *)R.d_slot_of;
    const dim3 block(256);
    // the check is a pass of its own, its flag read back before anything is allocated or written
    if (E.insert) {
        uint32_t bad = 0;
        uint32_t *flag = (uint32_t *)R.d_flag;
        HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
        hipLaunchKernelGGL(k_splice_check, dim3((E.insert + 255u) / 256u), block, 0, st, A, flag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad)
            return fail(RT_ERR_INVALID, std::string(who) + ": an inserted record is not a triangle, its material is not one of "
                                        "the scene's, or a vertex is NaN or infinite");
    }
    // what the builder reads lives for the build only: records, boxes, the identity map, one allocation
    const size_t prims_bytes = sizeof(float4) * 3 * (size_t)n, box_bytes = sizeof(float4) * 2 * (size_t)n;
    void *stage = nullptr;
    auto alloc = [who](void **p, size_t bytes) {
        return hipMalloc(p, bytes) == hipSuccess ? RT_OK : fail(RT_ERR_HIP, std::string(who) + ": hipMalloc failed");
    };
    rc = alloc(&stage, prims_bytes + box_bytes + sizeof(uint32_t) * (size_t)n);
    if (rc == RT_OK) rc = alloc(&out.shade, sizeof(float4) * 2 * (size_t)n);
    if (rc == RT_OK) rc = alloc(&out.cen, sizeof(float4) * (size_t)n);
    if (rc == RT_OK) {
        A.prims = (float4 *)stage;
        A.box = (float4 *)((char *)stage + prims_bytes);
        A.ident = (uint32_t *)((char *)stage + prims_bytes + box_bytes);
        A.shade = (float4 *)out.shade;
        A.cen = (float4 *)out.cen;
        hipLaunchKernelGGL(k_splice_gather, dim3((n + 255u) / 256u), block, 0, st, A);
        if (hipGetLastError() != hipSuccess) rc = fail(RT_ERR_HIP, std::string(who) + ": launch failed");
    }
    if (rc == RT_OK) {
        rc = build_tree(BuildInputs{n, out.cen, A.box, A.ident, A.prims, S.margin, who}, st, out);
        if (rc == RT_OK) out.stats[3] += E.insert ? 2u : 1u;   // the check's and the gather's launches
    }
    if (rc != RT_OK) (void)hipStreamSynchronize(st);
    if (stage) (void)hipFree(stage);
    if (rc != RT_OK) free_rebuilt(out);
    return rc;
}

}  // namespace rt
