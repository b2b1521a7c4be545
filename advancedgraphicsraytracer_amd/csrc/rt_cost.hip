// rt_cost.hip -- rt_scene_bvh_cost: the cost of a scene's current device tree, reduced on the GPU.
//
// The node records are read where the frames read them (after any update, rebuild or splice), 64 B
// per sibling pair, consecutive lanes on consecutive nodes:
//   k_cost_partial  up to kCostBlocks workgroups of 256 lanes stride over the nodes (node 1, the
//                   reference's unused one, is skipped); a lane keeps its sums in registers
//                   (rt_cost.h holds every line it runs), a wave folds them with shuffles, the
//                   workgroup's four waves through LDS, and lane 0 stores the workgroup's CostPart;
//   k_cost_final    one workgroup folds the partial sums the same way and adds the root's area.
// Nothing is handed from one workgroup to another inside a launch and no atomic is used: the second
// launch reads the first one's stores across the kernel boundary.
#include "rt_cost.h"

#include "rt_refit.h"

namespace rt {

namespace {

constexpr uint32_t kCostBlocks = 512;
struct CostResult {
    CostPart c;
    double root_area;
};

__device__ __forceinline__ void wave_fold(CostPart &c) {
    for (int o = 32; o > 0; o >>= 1) {
        CostPart b;
        b.interior_area = __shfl_xor(c.interior_area, o, 64);
        b.leaf_area = __shfl_xor(c.leaf_area, o, 64);
        b.leaf_cost = __shfl_xor(c.leaf_cost, o, 64);
        b.interiors = __shfl_xor(c.interiors, o, 64);
        b.leaves = __shfl_xor(c.leaves, o, 64);
        b.refs = __shfl_xor(c.refs, o, 64);
        b.max_leaf = __shfl_xor(c.max_leaf, o, 64);
        cost_merge(c, b);
    }
}
// the workgroup's sum in thread 0 (256 threads: four waves)
__device__ __forceinline__ void block_fold(CostPart &c) {
    __shared__ CostPart part[4];
    wave_fold(c);
    if ((threadIdx.x & 63u) == 0u) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < 4; ++w) cost_merge(c, part[w]);
}

__global__ void __launch_bounds__(256) k_cost_partial(const float4 *__restrict__ nodes, uint32_t n, CostPart *__restrict__ out) {
    CostPart c{};
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        if (i == 1u) continue;
        const float4 a = nodes[2 * (size_t)i], b = nodes[2 * (size_t)i + 1];
        f3 mn, mx;
        node_box(a, b, mn, mx);
        cost_add(c, mn, mx, fbits(b.z) & 255u);
    }
    block_fold(c);
    if (threadIdx.x == 0) out[blockIdx.x] = c;
}

__global__ void __launch_bounds__(256) k_cost_final(const float4 *__restrict__ nodes, const CostPart *__restrict__ part,
                                                    uint32_t nparts, CostResult *__restrict__ out) {
    CostPart c{};
    for (uint32_t i = threadIdx.x; i < nparts; i += 256u) cost_merge(c, part[i]);
    block_fold(c);
    if (threadIdx.x == 0) {
        f3 mn, mx;
        node_box(nodes[0], nodes[1], mn, mx);
        out->c = c;
        out->root_area = box_area(mn, mx);
    }
}

}  // namespace

int device_bvh_cost(const void *d_nodes, uint32_t nodes_used, void **d_buf, hipStream_t st, rt_bvh_cost *out) {
    if (!d_nodes || nodes_used == 0) return fail(RT_ERR_INVALID, "rt_scene_bvh_cost: the scene has no tree");
    if (!*d_buf) HIP_TRY(hipMalloc(d_buf, sizeof(CostPart) * kCostBlocks + sizeof(CostResult)));
    CostPart *part = (CostPart *)*d_buf;
    CostResult *res = (CostResult *)(part + kCostBlocks);
    const uint32_t blocks = std::min(kCostBlocks, (nodes_used + 255u) / 256u);
    hipLaunchKernelGGL(k_cost_partial, dim3(blocks), dim3(256), 0, st, (const float4 *)d_nodes, nodes_used, part);
    hipLaunchKernelGGL(k_cost_final, dim3(1), dim3(256), 0, st, (const float4 *)d_nodes, part, blocks, res);
    HIP_TRY(hipGetLastError());
    CostResult h{};
    HIP_TRY(hipMemcpyAsync(&h, res, sizeof(h), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    cost_finish(h.c, h.root_area, out);
    return RT_OK;
}

}  // namespace rt
