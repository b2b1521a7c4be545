// rt_build.hip -- the GPU BVH rebuild: the kernels and the host path, rt::build_tree
// over given inputs (rt::splice builds over a new id space with it) and rt::rebuild over the scene's own.
//
// rt_build.h holds every line a lane runs, the order of the launches (build_order) and the sizes of the
// arrays (build_carve); the kernels here supply the lane context (lane index, __syncthreads, integer
// atomics), and the host path the executor that turns a step of the order into a launch.
#include "rt_build.h"
#include "rt_refit.h"

#include <cmath>
#include <string>

namespace rt {

namespace {

struct DevLane {
    uint32_t tid, stride;
    __device__ __forceinline__ void bar() { __syncthreads(); }
    __device__ __forceinline__ void amax(uint32_t *p, uint32_t v) { atomicMax(p, v); }
    __device__ __forceinline__ uint32_t aadd(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
};
__device__ __forceinline__ DevLane wg_lane() { return DevLane{threadIdx.x, blockDim.x}; }
__device__ __forceinline__ uint32_t gtid() { return blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint32_t gstride() { return gridDim.x * blockDim.x; }

__global__ void __launch_bounds__(256) k_init(BuildArgs B) {
    DevLane par = wg_lane();
    build_init(B, gtid(), gstride(), par);
}
__global__ void __launch_bounds__(256) k_wide_bounds(BuildArgs B, uint32_t lv) {
    __shared__ uint32_t acc[kAccWords];
    DevLane par = wg_lane();
    wide_bounds(B, lv, blockIdx.x, acc, par);
}
__global__ void __launch_bounds__(256) k_wide_bins(BuildArgs B, uint32_t lv) {
    __shared__ uint32_t acc[kAccWords];
    DevLane par = wg_lane();
    wide_bins(B, lv, blockIdx.x, acc, par);
}
__global__ void __launch_bounds__(256) k_wide_plane(BuildArgs B, uint32_t lv) {
    __shared__ uint32_t acc[kAccWords];
    __shared__ uint32_t scan[256];
    DevLane par = wg_lane();
    wide_plane_count(B, lv, blockIdx.x, acc, scan, par);
}
__global__ void __launch_bounds__(256) k_wide_settle(BuildArgs B, uint32_t lv, uint32_t nw) {
    DevLane par = wg_lane();
    if (gtid() < nw) wide_settle(B, lv, gtid(), par);
}
__global__ void __launch_bounds__(256) k_wide_tables(BuildArgs B, uint32_t lv) {
    __shared__ uint32_t scan[256];
    DevLane par = wg_lane();
    wide_tables(B, lv, blockIdx.x, scan, par);
}
__global__ void __launch_bounds__(256) k_wide_move(BuildArgs B, uint32_t lv) {
    DevLane par = wg_lane();
    wide_move(B, lv, blockIdx.x, par);
}
__global__ void __launch_bounds__(256) k_wide_back(BuildArgs B, uint32_t lv) {
    DevLane par = wg_lane();
    wide_copy_back(B, lv, blockIdx.x, par);
}
__global__ void __launch_bounds__(256) k_subtrees(BuildArgs B) {
    __shared__ uint32_t acc[kAccWords];
    __shared__ uint32_t scan[256];
    __shared__ uint32_t stack[kBuildStack];
    DevLane par = wg_lane();
    build_subtree(B, B.slist[blockIdx.x], acc, scan, stack, par);
}
__global__ void __launch_bounds__(256) k_scan_sum(BuildArgs B) { scan_sum(B, gtid(), gstride()); }
__global__ void __launch_bounds__(64) k_scan_top(BuildArgs B) {
    if (gtid() == 0u) scan_top(B);
}
__global__ void __launch_bounds__(256) k_scan_apply(BuildArgs B) { scan_apply(B, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_emit(BuildArgs B) {
    DevLane par = wg_lane();
    emit_nodes(B, gtid(), gstride(), par);
}
__global__ void __launch_bounds__(256) k_permute(BuildArgs B) { permute_slots(B, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_boxes(BuildArgs B, uint32_t used, uint32_t d) { box_level(B, used, d, gtid(), gstride()); }

// one allocation carved into the build's work arrays
struct Arena {
    char *base = nullptr;
    size_t used = 0;
    template <typename T>
    T *take(size_t count) {
        T *p = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += (sizeof(T) * count + 255u) & ~(size_t)255u;
        return p;
    }
};
// build_order's executor on the device: a step is a launch on the stream; a launch's error shows at the next read
struct DevExec {
    const BuildArgs &B;
    hipStream_t st;
    int rc = RT_OK;   // of the call that failed, once a method has returned false

    template <class F>
    bool ok(F call) { return (rc = call()) == RT_OK; }
    bool zero(uint32_t *p, size_t words) {
        return ok([&]() -> int {
            HIP_TRY(hipMemsetAsync(p, 0, sizeof(uint32_t) * words, st));
            return RT_OK;
        });
    }
    bool read(uint32_t *dst, const uint32_t *src, size_t words) {
        return ok([&]() -> int {
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(dst, src, sizeof(uint32_t) * words, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return RT_OK;
        });
    }
    bool step(BuildStep s, uint32_t count, uint32_t arg) {
        const dim3 block(256), lanes((count + 255u) / 256u), wgs(count);
        switch (s) {
        case kStepInit: hipLaunchKernelGGL(k_init, lanes, block, 0, st, B); break;
        case kStepWideBounds: hipLaunchKernelGGL(k_wide_bounds, wgs, block, 0, st, B, arg); break;
        case kStepWideBins: hipLaunchKernelGGL(k_wide_bins, wgs, block, 0, st, B, arg); break;
        case kStepWidePlane: hipLaunchKernelGGL(k_wide_plane, wgs, block, 0, st, B, arg); break;
        case kStepWideSettle: hipLaunchKernelGGL(k_wide_settle, lanes, block, 0, st, B, arg, count); break;
        case kStepWideTables: hipLaunchKernelGGL(k_wide_tables, wgs, block, 0, st, B, arg); break;
        case kStepWideMove: hipLaunchKernelGGL(k_wide_move, wgs, block, 0, st, B, arg); break;
        case kStepWideBack: hipLaunchKernelGGL(k_wide_back, wgs, block, 0, st, B, arg); break;
        case kStepSubtrees: hipLaunchKernelGGL(k_subtrees, wgs, block, 0, st, B); break;
        case kStepScanSum: hipLaunchKernelGGL(k_scan_sum, lanes, block, 0, st, B); break;
        case kStepScanTop: hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(64), 0, st, B); break;
        case kStepScanApply: hipLaunchKernelGGL(k_scan_apply, lanes, block, 0, st, B); break;
        case kStepEmit: hipLaunchKernelGGL(k_emit, lanes, block, 0, st, B); break;
        case kStepPermute: hipLaunchKernelGGL(k_permute, lanes, block, 0, st, B); break;
        case kStepBoxes: hipLaunchKernelGGL(k_boxes, lanes, block, 0, st, B, count, arg); break;
        }
        return true;
    }
};

int run_build(const BuildArgs &B, hipStream_t st, const std::string &who, Rebuilt &out) {
    DevExec x{B, st};
    BuildFigures f;
    const int code = build_order(x, B, f);
    out.nodes_used = f.nodes_used;
    out.depth = f.depth;
    out.max_leaf = f.max_leaf;
    switch (code) {
    case kBuildOk: break;
    case kBuildExec: return x.rc;
    case kBuildLevels: return fail(RT_ERR_UNSUPPORTED, who + ": the new tree is deeper than 64");
    case kBuildTableOverrun: return fail(RT_ERR_HIP, who + ": level tables overrun");
    case kBuildListOverrun: return fail(RT_ERR_HIP, who + ": subtree list overrun");
    case kBuildDeep: return fail(RT_ERR_UNSUPPORTED, who + ": the new tree is deeper than 64 (the reference's stack[64])");
    case kBuildWideLeaf: return fail(RT_ERR_UNSUPPORTED, who + ": the new tree has a leaf with more than 255 primitives");
    case kBuildNodes: return fail(RT_ERR_UNSUPPORTED, who + ": the new tree has more than 2^24 nodes");
    }
    HIP_TRY(hipGetLastError());
    float4 root[2];
    HIP_TRY(hipMemcpyAsync(root, B.nodes, sizeof(root), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out.root_word = fbits(root[1].z);
    out.finite = true;
    for (float v : {root[0].x, root[0].y, root[0].z, root[0].w, root[1].x, root[1].y}) out.finite = out.finite && std::isfinite(v);
    out.stats[0] = f.levels;
    out.stats[1] = f.wide_splits;
    out.stats[2] = f.subtrees;
    out.stats[3] = f.launches;
    return RT_OK;
}

}  // namespace

void free_rebuilt(Rebuilt &r) {
    for (void **p : {&r.nodes, &r.prims, &r.slot_box, &r.slot_of, &r.index, &r.shade, &r.cen, &r.xprims}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

int build_tree(const BuildInputs &in, hipStream_t st, Rebuilt &out) {
    const uint32_t n = in.n;
    const std::string who = in.who;
    BuildArgs B{};
    B.n = n;
    B.cen = (const float4 *)in.cen;
    B.old_box = (const float4 *)in.box;
    B.old_slot_of = (const uint32_t *)in.slot_of;
    B.old_prims = (const float4 *)in.prims;
    B.margin = in.margin;
    Arena sizes;
    build_carve(sizes, n, B);
    void *work = nullptr;
    auto alloc = [&who](void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? RT_OK : fail(RT_ERR_HIP, who + ": hipMalloc failed"); };
    int rc = alloc(&work, sizes.used);
    if (rc == RT_OK) rc = alloc(&out.nodes, sizeof(float4) * build_nodes_len(n));
    if (rc == RT_OK) rc = alloc(&out.prims, sizeof(float4) * build_prims_len(n));
    if (rc == RT_OK) rc = alloc(&out.slot_box, sizeof(float4) * build_slot_box_len(n));
    if (rc == RT_OK) rc = alloc(&out.slot_of, sizeof(uint32_t) * build_ids_len(n));
    if (rc == RT_OK) rc = alloc(&out.index, sizeof(uint32_t) * build_ids_len(n));
    if (rc == RT_OK) {
        Arena a;
        a.base = (char *)work;
        build_carve(a, n, B);
        B.idx = (uint32_t *)out.index;
        B.nodes = (float4 *)out.nodes;
        B.prims = (float4 *)out.prims;
        B.slot_box = (float4 *)out.slot_box;
        B.slot_of = (uint32_t *)out.slot_of;
        rc = run_build(B, st, who, out);
        if (rc != RT_OK) (void)hipStreamSynchronize(st);
    }
    if (work) (void)hipFree(work);
    if (rc != RT_OK) free_rebuilt(out);
    return rc;
}

int rebuild(RefitState &R, const SceneRecords &S, hipStream_t st, Rebuilt &out) {
    HIP_TRY(hipDeviceSynchronize());   // frames still reading the scene on any stream
    int rc = sync_host_tree(R, *S.bvh, S.nodes);   // a scene never updated seeds its state from the host tree
    if (rc == RT_OK) rc = ensure_state(R, S);
    if (rc != RT_OK) return rc;
    return build_tree(BuildInputs{S.num_prims, R.d_cen, R.d_slot_box, R.d_slot_of, S.prims, S.margin, "rt_scene_rebuild"}, st, out);
}

}  // namespace rt
