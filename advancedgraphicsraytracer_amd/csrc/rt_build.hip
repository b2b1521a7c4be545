// rt_build.hip -- the GPU BVH rebuild: the kernels and the host path, rt::build_tree
// over given inputs (rt::splice builds over a new id space with it) and rt::rebuild over the scene's own.
//
// rt_build.h holds every line a lane runs; the kernels here supply the lane context (lane index,
// __syncthreads, integer atomics) and the launch order:
//   k_init                       the identity index array, the root
//   per level of the many-workgroup path (nodes of more than kBuildWide primitives, a workgroup per
//   kBuildChunk primitives):
//     k_wide_bounds, k_wide_bins     node box, centroid bounds, bins: LDS accumulators merged into the node's
//     k_wide_plane                   the plane, the cost abort, the chunk's left count
//     k_wide_settle                  per node: the chunk counts' prefix, the children, the next level's tasks
//     k_wide_tables, k_wide_move, k_wide_back   the partition
//   k_subtrees                   one workgroup per subtree of at most kBuildWide primitives, explicit stack
//   k_scan_sum / _top / _apply   the prefix count over the split boundaries that numbers the nodes
//   k_emit                       node words in the host's numbering, depths, widest leaf
//   k_permute                    leaf-slot records, slot boxes and the slot map in the new order
//   k_boxes                      per depth, deepest first: stored boxes and sticky words (refit_node)
// Nothing is handed from one workgroup to another inside a launch -- no flags, no spins, no fences
// (the rule of rt_refit.hip): launch boundaries order the steps of a level and the levels, and
// __syncthreads() orders the steps inside a workgroup, whose waves share their CU's vector L1.
// The launches of the level loop are bounded by the depth limit: kBuildMaxDepth + 1 levels.
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
void carve(Arena &a, uint32_t n, BuildArgs &B) {
    B.idx2 = a.take<uint32_t>(n);
    B.ptab = a.take<uint32_t>(n);
    B.qtab = a.take<uint32_t>(n);
    B.rk = a.take<uint32_t>(n);
    B.node = a.take<BNode>(2 * (size_t)n + 2);
    B.bflag = a.take<uint32_t>((size_t)n + 1);
    B.csum = a.take<uint32_t>(scan_runs(n) + 1u);
    B.ctr = a.take<uint32_t>(kCtrWords);
    B.wacc = a.take<uint32_t>((size_t)build_wide_cap(n) * kAccWords);
    for (int k = 0; k < 2; ++k) {
        B.wnode[k] = a.take<WNode>(build_wide_cap(n));
        B.task[k] = a.take<BTask>(build_task_cap(n));
    }
    B.chunkL = a.take<uint32_t>(build_task_cap(n));
    B.slist = a.take<uint32_t>((size_t)n + 1);
    B.depth_of = a.take<uint32_t>(2 * (size_t)n + 2);
}

int run_build(const BuildArgs &B, hipStream_t st, const std::string &who, Rebuilt &out) {
    const uint32_t n = B.n;
    const dim3 block(256);
    const dim3 per_prim((n + 255u) / 256u);
    uint32_t launches = 0;
    HIP_TRY(hipMemsetAsync(B.ctr, 0, sizeof(uint32_t) * kCtrWords, st));
    HIP_TRY(hipMemsetAsync(B.bflag, 0, sizeof(uint32_t) * ((size_t)n + 1), st));
    hipLaunchKernelGGL(k_init, per_prim, block, 0, st, B);
    ++launches;
    uint32_t lvl[2] = {0, 0}, levels = 0;   // nodes and tasks of the level
    HIP_TRY(hipMemcpyAsync(lvl, B.ctr + kCtrLevel, sizeof(lvl), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (uint32_t lv = 0; lvl[0] > 0; ++lv) {
        if (lv > kBuildMaxDepth) return fail(RT_ERR_UNSUPPORTED, who + ": the new tree is deeper than 64");
        if (lvl[0] > build_wide_cap(n) || lvl[1] > build_task_cap(n)) return fail(RT_ERR_HIP, who + ": level tables overrun");
        const dim3 tasks(lvl[1]);
        HIP_TRY(hipMemsetAsync(B.wacc, 0, sizeof(uint32_t) * kAccWords * (size_t)lvl[0], st));
        hipLaunchKernelGGL(k_wide_bounds, tasks, block, 0, st, B, lv);
        hipLaunchKernelGGL(k_wide_bins, tasks, block, 0, st, B, lv);
        hipLaunchKernelGGL(k_wide_plane, tasks, block, 0, st, B, lv);
        hipLaunchKernelGGL(k_wide_settle, dim3((lvl[0] + 255u) / 256u), block, 0, st, B, lv, lvl[0]);
        hipLaunchKernelGGL(k_wide_tables, tasks, block, 0, st, B, lv);
        hipLaunchKernelGGL(k_wide_move, tasks, block, 0, st, B, lv);
        hipLaunchKernelGGL(k_wide_back, tasks, block, 0, st, B, lv);
        launches += 7;
        ++levels;
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(lvl, B.ctr + kCtrLevel + 2u * (lv + 1u), sizeof(lvl), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    uint32_t ctr[kCtrLevel];
    HIP_TRY(hipMemcpyAsync(ctr, B.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const uint32_t nsmall = ctr[kCtrSmall];
    if (nsmall > n) return fail(RT_ERR_HIP, who + ": subtree list overrun");
    if (nsmall) {
        hipLaunchKernelGGL(k_subtrees, dim3(nsmall), block, 0, st, B);
        ++launches;
    }
    const dim3 runs((scan_runs(n) + 255u) / 256u);
    hipLaunchKernelGGL(k_scan_sum, runs, block, 0, st, B);
    hipLaunchKernelGGL(k_scan_top, dim3(1), dim3(64), 0, st, B);
    hipLaunchKernelGGL(k_scan_apply, runs, block, 0, st, B);
    hipLaunchKernelGGL(k_emit, per_prim, block, 0, st, B);
    launches += 4;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(ctr, B.ctr, sizeof(ctr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    // take_tree's limits, before anything reads the new node words
    out.nodes_used = 2u + 2u * ctr[kCtrSplits];
    out.depth = ctr[kCtrDepth];
    out.max_leaf = ctr[kCtrMaxLeaf];
    if ((ctr[kCtrErr] & kBuildErrDepth) || out.depth > kBuildMaxDepth)
        return fail(RT_ERR_UNSUPPORTED, who + ": the new tree is deeper than 64 (the reference's stack[64])");
    if (out.max_leaf > 255) return fail(RT_ERR_UNSUPPORTED, who + ": the new tree has a leaf with more than 255 primitives");
    if (out.nodes_used > (1u << 24)) return fail(RT_ERR_UNSUPPORTED, who + ": the new tree has more than 2^24 nodes");
    hipLaunchKernelGGL(k_permute, per_prim, block, 0, st, B);
    ++launches;
    const dim3 per_node((out.nodes_used + 255u) / 256u);
    for (uint32_t d = out.depth + 1u; d-- > 0u;) {
        hipLaunchKernelGGL(k_boxes, per_node, block, 0, st, B, out.nodes_used, d);
        ++launches;
    }
    HIP_TRY(hipGetLastError());
    float4 root[2];
    HIP_TRY(hipMemcpyAsync(root, B.nodes, sizeof(root), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    out.root_word = fbits(root[1].z);
    out.finite = true;
    for (float f : {root[0].x, root[0].y, root[0].z, root[0].w, root[1].x, root[1].y}) out.finite = out.finite && std::isfinite(f);
    out.stats[0] = levels;
    out.stats[1] = ctr[kCtrWideSplit];
    out.stats[2] = nsmall;
    out.stats[3] = launches;
    return RT_OK;
}

}  // namespace

void free_rebuilt(Rebuilt &r) {
    for (void **p : {&r.nodes, &r.prims, &r.slot_box, &r.slot_of, &r.index, &r.shade, &r.cen}) {
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
    carve(sizes, n, B);
    void *work = nullptr;
    auto alloc = [&who](void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? RT_OK : fail(RT_ERR_HIP, who + ": hipMalloc failed"); };
    int rc = alloc(&work, sizes.used);
    if (rc == RT_OK) rc = alloc(&out.nodes, sizeof(float4) * 2 * (2 * (size_t)n + 2));
    if (rc == RT_OK) rc = alloc(&out.prims, sizeof(float4) * 3 * (size_t)n);
    if (rc == RT_OK) rc = alloc(&out.slot_box, sizeof(float4) * 2 * (size_t)n);
    if (rc == RT_OK) rc = alloc(&out.slot_of, sizeof(uint32_t) * (size_t)n);
    if (rc == RT_OK) rc = alloc(&out.index, sizeof(uint32_t) * (size_t)n);
    if (rc == RT_OK) {
        Arena a;
        a.base = (char *)work;
        carve(a, n, B);
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
