// rt_plan.hip -- the refit schedule built on the GPU: the kernels and the host path,
// rt::plan_on_device.
//
// rt_plan.h holds every line a lane runs, the order of the launches (plan_order) and the sizes of the
// arrays (plan_carve); the kernels here supply the lane context (lane index, __syncthreads, integer
// atomic add), and the host path the executor that turns a step of the order into a launch.
#include "rt_plan.h"

#include <string>

namespace rt {

namespace {

struct DevLane {
    uint32_t tid, stride;
    __device__ __forceinline__ void bar() { __syncthreads(); }
    __device__ __forceinline__ uint32_t aadd(uint32_t *p, uint32_t v) { return atomicAdd(p, v); }
};
__device__ __forceinline__ DevLane wg_lane() { return DevLane{threadIdx.x, blockDim.x}; }
__device__ __forceinline__ uint32_t gtid() { return blockIdx.x * blockDim.x + threadIdx.x; }
__device__ __forceinline__ uint32_t gstride() { return gridDim.x * blockDim.x; }

__global__ void __launch_bounds__(kPlanSmallLanes) k_plan_small(PlanArgs A) {
    __shared__ uint32_t lds[kPlanLds];
    DevLane par = wg_lane();
    plan_small(A, lds, par);
}
__global__ void __launch_bounds__(256) k_plan_init(PlanArgs A) { plan_init(A, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_plan_down(PlanArgs A, uint32_t d) { plan_down(A, d, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_plan_up(PlanArgs A, uint32_t d) { plan_up(A, d, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_plan_rank(PlanArgs A, uint32_t d) { plan_rank(A, d, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_plan_classify(PlanArgs A) { plan_classify(A, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_plan_scan_sum(PlanArgs A) { plan_scan_sum(A, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_plan_scan_top(PlanArgs A) {
    __shared__ uint32_t lds[kPlanLds];
    DevLane par = wg_lane();
    plan_scan_top(A, lds, par);
}
__global__ void __launch_bounds__(256) k_plan_scan_apply(PlanArgs A) { plan_scan_apply(A, gtid(), gstride()); }
__global__ void __launch_bounds__(256) k_plan_treelets(PlanArgs A) {
    __shared__ uint32_t lds[kPlanLds];
    DevLane par = wg_lane();
    plan_treelets(A, blockIdx.x, gridDim.x, lds, par);
}
__global__ void __launch_bounds__(256) k_plan_top(PlanArgs A) {
    __shared__ uint32_t lds[kPlanLds];
    DevLane par = wg_lane();
    plan_top(A, lds, par);
}

// one allocation carved into the work arrays
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
// plan_order's executor on the device: a step is a launch on the stream; a launch's error shows at the read
struct DevExec {
    const PlanArgs &A;
    hipStream_t st;
    int rc = RT_OK;

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
    bool step(PlanStep s, uint32_t count, uint32_t arg) {
        const dim3 block(256), lanes((count + 255u) / 256u), wgs(count), one(1);
        switch (s) {
        case kPlanStepSmall: hipLaunchKernelGGL(k_plan_small, one, dim3(kPlanSmallLanes), 0, st, A); break;
        case kPlanStepInit: hipLaunchKernelGGL(k_plan_init, lanes, block, 0, st, A); break;
        case kPlanStepDown: hipLaunchKernelGGL(k_plan_down, lanes, block, 0, st, A, arg); break;
        case kPlanStepUp: hipLaunchKernelGGL(k_plan_up, lanes, block, 0, st, A, arg); break;
        case kPlanStepRank: hipLaunchKernelGGL(k_plan_rank, lanes, block, 0, st, A, arg); break;
        case kPlanStepClassify: hipLaunchKernelGGL(k_plan_classify, lanes, block, 0, st, A); break;
        case kPlanStepScanSum: hipLaunchKernelGGL(k_plan_scan_sum, lanes, block, 0, st, A); break;
        case kPlanStepScanTop: hipLaunchKernelGGL(k_plan_scan_top, one, block, 0, st, A); break;
        case kPlanStepScanApply: hipLaunchKernelGGL(k_plan_scan_apply, lanes, block, 0, st, A); break;
        case kPlanStepTreelets: hipLaunchKernelGGL(k_plan_treelets, wgs, block, 0, st, A); break;
        case kPlanStepTop: hipLaunchKernelGGL(k_plan_top, one, block, 0, st, A); break;
        }
        return true;
    }
};

void free_plan_arrays(RefitState &R) {
    for (void **p : {&R.d_list, &R.d_lvl, &R.d_grp}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

}  // namespace

int plan_on_device(RefitState &R, const SceneRecords &S, hipStream_t st) {
    const uint32_t used = S.bvh->nodes_used;
    PlanArgs A{};
    A.nodes = (const float4 *)S.nodes;
    A.used = used;
    A.depth = S.bvh->depth;
    Arena sizes;
    plan_carve(sizes, used, A);
    free_plan_arrays(R);
    R.refit_ready = false;
    R.plan_info = PlanInfo{};
    void *work = nullptr;
    auto alloc = [](void **p, size_t bytes) { return hipMalloc(p, bytes) == hipSuccess ? RT_OK : fail(RT_ERR_HIP, "refit schedule: hipMalloc failed"); };
    int rc = alloc(&work, sizes.used);
    if (rc == RT_OK) rc = alloc(&R.d_list, sizeof(uint32_t) * plan_list_len(used));
    if (rc == RT_OK) rc = alloc(&R.d_lvl, sizeof(uint32_t) * plan_lvl_len(used));
    if (rc == RT_OK) rc = alloc(&R.d_grp, sizeof(uint32_t) * plan_grp_len(used));
    PlanFigures f{};
    int code = kPlanExec;
    if (rc == RT_OK) {
        Arena a;
        a.base = (char *)work;
        plan_carve(a, used, A);
        A.list = (uint32_t *)R.d_list;
        A.lvl = (uint32_t *)R.d_lvl;
        A.grp = (uint32_t *)R.d_grp;
        DevExec x{A, st};
        code = plan_order(x, A, plan_route(used), f);
        if (code == kPlanExec) {
            rc = x.rc;
            (void)hipStreamSynchronize(st);
        }
    }
    if (work) (void)hipFree(work);
    if (rc != RT_OK || code != kPlanOk) {   // kPlanNotTree: RT_OK, not ready -- ensure_refit takes the host's walk
        free_plan_arrays(R);
        return rc;
    }
    R.plan.ntreelets = f.ntreelets;
    R.plan.has_top = f.has_top != 0u;
    R.plan_info = PlanInfo{f.route, f.list_len, f.lvl_len, f.top_nodes, f.launches};
    R.refit_ready = true;
    return RT_OK;
}

}  // namespace rt
