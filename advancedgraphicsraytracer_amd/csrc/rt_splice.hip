// rt_splice.hip -- triangles leave and enter a live scene: the kernels and the host
// path of rt::splice.
//
// rt_splice.h holds every line a lane runs; the kernels here supply the lane index:
//   k_splice_check    one lane per inserted record: a triangle of one of the scene's materials with
//                     finite vertices (splice_ok)?  Sets the flag, writes nothing else;
//   k_splice_gather   one lane per NEW id, consecutive lanes on consecutive ids: the kept primitives'
//                     records copied with the id word patched, the inserted triangles' written by the
//                     encoders scene creation runs, everything in id order into fresh buffers.
// The batched edits fill one source word per new id and share one gather:
//   k_splice_sources  ranges route: one lane per new id, its source word by binary search in the rows;
//   k_mask_check      mask route: one lane per old id: does the mask drop primitive 0 or a non-triangle?
//   k_mask_count, k_mask_top, k_mask_scatter   the exclusive prefix count of the keep flags: a count per
//                     workgroup, the counts' prefix in one workgroup, the source words -- three launches;
//   k_splice_gather_src   k_splice_gather with the source word read instead of derived.
// Primitives of every kind take the same two routes with a check and a mask check of their
// own and, in front of the gather, the side-table ranks of the new id space:
//   k_splice_check_prims, k_mask_check_prims   any of the five kinds; anything but primitive 0 may go;
//   k_rank_flag, k_mask_count, k_mask_top, k_mask_ranks   per new id the cubes and quads before it -- the
//                     mask route's prefix count over a flag per new id;
//   k_mats_check, k_mats_put   rt_scene_set_prim_materials: the material words alone, in place.
// The builder (build_tree of rt_build.hip) then runs over the new id space with the identity as its
// old slot map.  Nothing is handed from one workgroup to another inside a launch: launch boundaries
// order check -> gather -> build.  The scene's own buffers are only read; the caller swaps the new
// ones in when everything succeeded (rt_scene_splice_triangles in rt_scene_edit.hip).
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

struct DevLane {
    uint32_t tid, stride;
    __device__ __forceinline__ void bar() { __syncthreads(); }
};
__global__ void __launch_bounds__(256) k_splice_sources(const SpliceRow *rows, uint32_t num_rows, uint32_t n_new, uint32_t *src) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < n_new) src[j] = splice_source(rows, num_rows, j);
}
__global__ void __launch_bounds__(256) k_splice_gather_src(SpliceArgs A, const uint32_t *src) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < A.n_new) splice_gather_src(A, src, j);
}
__global__ void __launch_bounds__(256) k_mask_check(MaskArgs M, uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < M.n && !mask_ok(M, i)) *flag = 1u;
}
__global__ void __launch_bounds__(256) k_mask_count(MaskArgs M) {
    __shared__ uint32_t scan[256];
    DevLane par{threadIdx.x, 256u};
    mask_count(M, blockIdx.x, scan, par);
}
__global__ void __launch_bounds__(256) k_mask_top(MaskArgs M) {
    __shared__ uint32_t scan[256];
    DevLane par{threadIdx.x, 256u};
    mask_top(M, scan, par);
}
__global__ void __launch_bounds__(256) k_mask_scatter(MaskArgs M) {
    __shared__ uint32_t scan[256];
    DevLane par{threadIdx.x, 256u};
    mask_scatter(M, blockIdx.x, scan, par);
}
static_assert(kMaskGroup == 256, "a workgroup of 256 lanes takes one id of its group each");

// primitives of every kind: the check that admits the five kinds and leaves the type bytes,
// the mask check that lets any kind go, the side-table ranks (flags; k_mask_count and k_mask_top over
// them; ranks), and rt_scene_set_prim_materials' two passes
__global__ void __launch_bounds__(256) k_splice_check_prims(SpliceArgs A, uint8_t *types, uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < A.insert && !splice_prim_ok(A, i, types)) *flag = 1u;
}
__global__ void __launch_bounds__(256) k_mask_check_prims(MaskArgs M, uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < M.n && !mask_prims_ok(M, i)) *flag = 1u;
}
__global__ void __launch_bounds__(256) k_rank_flag(SpliceArgs A, const uint32_t *src, uint8_t *flags) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    if (j < A.n_new) rank_flag(A, src, flags, j);
}
__global__ void __launch_bounds__(256) k_mask_ranks(MaskArgs M, uint32_t *rank) {
    __shared__ uint32_t scan[256];
    DevLane par{threadIdx.x, 256u};
    mask_ranks(M, blockIdx.x, scan, rank, par);
}
__global__ void __launch_bounds__(256) k_mats_check(MatArgs M, uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < M.count && !mats_ok(M, i)) *flag = 1u;
}
__global__ void __launch_bounds__(256) k_mats_put(MatArgs M) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < M.count) mats_put(M, i);
}

int alloc(void **p, size_t bytes, const char *who) {
    return hipMalloc(p, bytes) == hipSuccess ? RT_OK : fail(RT_ERR_HIP, std::string(who) + ": hipMalloc failed");
}
// waits for the frames still reading the scene on any stream.  A scene never updated seeds its state
// from the host tree; one that has its state on the device needs no host tree here
int begin(RefitState &R, const SceneRecords &S) {
    HIP_TRY(hipDeviceSynchronize());
    if (R.state_ready) return RT_OK;
    const int rc = sync_host_tree(R, *S.bvh, S.nodes);
    return rc == RT_OK ? ensure_state(R, S) : rc;
}
SpliceArgs scene_args(const RefitState &R, const SceneRecords &S, uint32_t n_new, const rt_prim *recs, uint32_t num_materials) {
    SpliceArgs A{};
    A.n_new = n_new;
    A.recs = recs;
    A.num_materials = num_materials;
    A.sliver_lim = R.sliver_lim;
    A.old_prims = (const float4 *)S.prims; A.old_shade = (const float4 *)S.shade;
    A.old_cen = (const float4 *)R.d_cen; A.old_box = (const float4 *)R.d_slot_box;
    A.old_slot_of = (const uint32_t *)R.d_slot_of;
    A.sticky_spheres = R.sticky_spheres;
    A.old_xprims = (const float4 *)S.xprims;
    return A;
}
// The batched routes' common end: the gather over the source words (src: n_new words on the device,
// filled by launches already enqueued on `st`) into fresh buffers, then the build, as splice() does it
// types: the type bytes of the new id space where kinds enter and leave, else null.  Then
// the side-table ranks are counted first -- flags, count, top, ranks: four launches over n ids -- and the
// gather writes a new side table of as many entries as the types hold cubes and quads (the host knows the
// size without reading the count back; an empty table is creation's one zero word)
int gather_and_build(SpliceArgs A, const uint32_t *src, float margin, uint32_t launches, const char *who, hipStream_t st, Rebuilt &out,
                     const std::vector<uint8_t> *types = nullptr) {
    const uint32_t n = A.n_new;
    const size_t prims_bytes = sizeof(float4) * 3 * (size_t)n, box_bytes = sizeof(float4) * 2 * (size_t)n;
    void *stage = nullptr, *ranks = nullptr;
    int rc = alloc(&stage, prims_bytes + box_bytes + sizeof(uint32_t) * (size_t)n, who);
    if (rc == RT_OK) rc = alloc(&out.shade, sizeof(float4) * 2 * (size_t)n, who);
    if (rc == RT_OK) rc = alloc(&out.cen, sizeof(float4) * (size_t)n, who);
    if (rc == RT_OK && types) {
        size_t nx = 0;
        for (uint8_t t : *types) nx += has_xentry(t & 0x7fu) ? 1u : 0u;
        const uint32_t ng = mask_groups(n);
        // per new id its rank, the groups' sums, then the flags (bytes)
        const size_t words = (size_t)n + ng + 1u;
        rc = alloc(&ranks, sizeof(uint32_t) * words + n, who);
        if (rc == RT_OK) rc = alloc(&out.xprims, std::max<size_t>(sizeof(float4) * 8 * nx, 16), who);
        if (rc == RT_OK && nx == 0 && hipMemsetAsync(out.xprims, 0, 16, st) != hipSuccess) rc = fail(RT_ERR_HIP, std::string(who) + ": memset failed");
        if (rc == RT_OK) {
            uint32_t *rank = (uint32_t *)ranks;
            uint8_t *flags = (uint8_t *)(rank + words);
            const MaskArgs M{n, flags, nullptr, rank + n, nullptr};
            hipLaunchKernelGGL(k_rank_flag, dim3(ng), dim3(256), 0, st, A, src, flags);
            hipLaunchKernelGGL(k_mask_count, dim3(ng), dim3(256), 0, st, M);
            hipLaunchKernelGGL(k_mask_top, dim3(1), dim3(256), 0, st, M);
            hipLaunchKernelGGL(k_mask_ranks, dim3(ng), dim3(256), 0, st, M, rank);
            if (hipGetLastError() != hipSuccess) rc = fail(RT_ERR_HIP, std::string(who) + ": launch failed");
            A.xrank = rank;
            A.xprims = (float4 *)out.xprims;
            launches += 4u;
        }
    }
    if (rc == RT_OK) {
        A.prims = (float4 *)stage;
        A.box = (float4 *)((char *)stage + prims_bytes);
        A.ident = (uint32_t *)((char *)stage + prims_bytes + box_bytes);
        A.shade = (float4 *)out.shade;
        A.cen = (float4 *)out.cen;
        hipLaunchKernelGGL(k_splice_gather_src, dim3((n + 255u) / 256u), dim3(256), 0, st, A, src);
        if (hipGetLastError() != hipSuccess) rc = fail(RT_ERR_HIP, std::string(who) + ": launch failed");
    }
    if (rc == RT_OK) {
        rc = build_tree(BuildInputs{n, out.cen, A.box, A.ident, A.prims, margin, who}, st, out);
        if (rc == RT_OK) out.stats[3] += launches + 1u;   // the route's own launches and the gather's
    }
    if (rc != RT_OK) (void)hipStreamSynchronize(st);
    if (stage) (void)hipFree(stage);
    if (ranks) (void)hipFree(ranks);
    if (rc != RT_OK) free_rebuilt(out);
    return rc;
}

}  // namespace

int splice_ranges(RefitState &R, const SceneRecords &S, const SpliceRow *rows, uint32_t num_rows, uint32_t n_new, uint32_t total_insert,
                  const rt_prim *recs_dev, uint32_t num_materials, hipStream_t st, Rebuilt &out, SpliceKinds *K) {
    const char *who = K ? "rt_scene_splice_prims" : "rt_scene_splice_ranges";
    int rc = begin(R, S);
    if (rc != RT_OK) return rc;
    SpliceArgs A = scene_args(R, S, n_new, recs_dev, num_materials);
    A.insert = total_insert;   // for the check: every record of the call
    A.T = K ? K->T_dev : nullptr;
    uint32_t launches = 1;     // the source words'
    std::vector<uint8_t> rec_types(K ? total_insert : 0u);
    if (total_insert) {
        uint32_t bad = 0;
        uint32_t *flag = (uint32_t *)R.d_flag;
        // the records' type bytes come back with the flag; their buffer is the scene's and grows as needed
        if (K && (rc = grow(&R.d_types, &R.types_bytes, total_insert)) != RT_OK) return rc;
        HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
        if (K) hipLaunchKernelGGL(k_splice_check_prims, dim3((total_insert + 255u) / 256u), dim3(256), 0, st, A, (uint8_t *)R.d_types, flag);
        else hipLaunchKernelGGL(k_splice_check, dim3((total_insert + 255u) / 256u), dim3(256), 0, st, A, flag);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st));
        if (K) HIP_TRY(hipMemcpyAsync(rec_types.data(), R.d_types, total_insert, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (bad && K)
            return fail(RT_ERR_INVALID, std::string(who) + ": an inserted record's type is not one of the five kinds, its material is "
                                        "not one of the scene's, or a field, transform or box is NaN or infinite");
        if (bad)
            return fail(RT_ERR_INVALID, std::string(who) + ": an inserted record is not a triangle, its material is not one of "
                                        "the scene's, or a vertex is NaN or infinite");
        ++launches;
    }
    if (K) {
        SplicePlan plan;
        plan.rows.assign(rows, rows + num_rows);
        plan.n_new = n_new;
        K->types = splice_types(R.pinfo, plan, rec_types.data());
    }
    // the rows and the source words live for the call only, one allocation; the rows are uploaded whole
    const size_t rows_bytes = (sizeof(SpliceRow) * (size_t)num_rows + 15u) & ~(size_t)15u;
    void *aux = nullptr;
    if ((rc = alloc(&aux, rows_bytes + sizeof(uint32_t) * (size_t)n_new, who)) != RT_OK) return rc;
    uint32_t *src = (uint32_t *)((char *)aux + rows_bytes);
    if (hipMemcpyAsync(aux, rows, sizeof(SpliceRow) * (size_t)num_rows, hipMemcpyHostToDevice, st) != hipSuccess)
        rc = fail(RT_ERR_HIP, std::string(who) + ": upload failed");
    if (rc == RT_OK) {
        hipLaunchKernelGGL(k_splice_sources, dim3((n_new + 255u) / 256u), dim3(256), 0, st, (const SpliceRow *)aux, num_rows, n_new, src);
        if (hipGetLastError() != hipSuccess) rc = fail(RT_ERR_HIP, std::string(who) + ": launch failed");
    }
    if (rc == RT_OK) rc = gather_and_build(A, src, S.margin, launches, who, st, out, K ? &K->types : nullptr);   // blocks
    else (void)hipStreamSynchronize(st);
    (void)hipFree(aux);
    return rc;
}

int splice_mask(RefitState &R, const SceneRecords &S, const uint8_t *keep_dev, hipStream_t st, std::vector<uint8_t> &keep, uint32_t *n_new,
                Rebuilt &out, SpliceKinds *K) {
    const char *who = K ? "rt_scene_compact_prims" : "rt_scene_compact_triangles";
    int rc = begin(R, S);
    if (rc != RT_OK) return rc;
    const uint32_t n = S.num_prims, ng = mask_groups(n);
    *n_new = n;
    keep.resize(n);
    // the groups' counts, the flag behind them and, once the survivors are counted, the source words
    void *aux = nullptr;
    if ((rc = alloc(&aux, sizeof(uint32_t) * ((size_t)ng + 2u), who)) != RT_OK) return rc;
    void *srcbuf = nullptr;
    MaskArgs M{n, keep_dev, (const float4 *)S.shade, (uint32_t *)aux, nullptr};
    uint32_t *flag = M.sums + ng + 1u;
    uint32_t back[2] = {0u, 0u};   // the survivors, the flag
    auto enqueue = [&]() -> int {
        HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
        if (K) hipLaunchKernelGGL(k_mask_check_prims, dim3(ng), dim3(256), 0, st, M, flag);
        else hipLaunchKernelGGL(k_mask_check, dim3(ng), dim3(256), 0, st, M, flag);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mask_count, dim3(ng), dim3(256), 0, st, M);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mask_top, dim3(1), dim3(256), 0, st, M);
        HIP_TRY(hipGetLastError());
        // the check's flag and the survivor count (it sizes the allocations) are read back before
        // anything is written; the mask rides along for the host's type bytes
        HIP_TRY(hipMemcpyAsync(back, M.sums + ng, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(keep.data(), keep_dev, n, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return RT_OK;
    };
    rc = enqueue();
    if (rc != RT_OK) (void)hipStreamSynchronize(st);
    if (rc == RT_OK && back[1])
        rc = fail(RT_ERR_INVALID, std::string(who) + (K ? ": the mask drops primitive 0 (the light stays)"
                                                        : ": the mask drops primitive 0 (the light stays) or a primitive that is not a triangle"));
    if (rc == RT_OK && back[0] < n) {   // else: everything stays, nothing further
        *n_new = back[0];
        rc = alloc(&srcbuf, sizeof(uint32_t) * (size_t)back[0], who);
        if (rc == RT_OK) {
            M.src = (uint32_t *)srcbuf;
            hipLaunchKernelGGL(k_mask_scatter, dim3(ng), dim3(256), 0, st, M);
            if (hipGetLastError() != hipSuccess) rc = fail(RT_ERR_HIP, std::string(who) + ": launch failed");
        }
        if (rc == RT_OK && K) {
            K->types.clear();
            for (uint32_t i = 0; i < n; ++i)
                if (keep[i]) K->types.push_back(R.pinfo[i]);
        }
        if (rc == RT_OK) rc = gather_and_build(scene_args(R, S, back[0], nullptr, 0u), M.src, S.margin, 4u, who, st, out, K ? &K->types : nullptr);   // blocks
        else (void)hipStreamSynchronize(st);
    }
    if (srcbuf) (void)hipFree(srcbuf);
    (void)hipFree(aux);
    return rc;
}

int set_materials(RefitState &R, const SceneRecords &S, uint32_t first, uint32_t count, const int32_t *mats_dev, uint32_t num_materials,
                  hipStream_t st) {
    HIP_TRY(hipDeviceSynchronize());   // frames still reading the scene on any stream
    if (!R.d_flag) HIP_TRY(hipMalloc(&R.d_flag, 16));
    const MatArgs M{first, count, num_materials, mats_dev, (float4 *)S.shade};
    const dim3 grid((count + 255u) / 256u), block(256);
    uint32_t bad = 0;
    uint32_t *flag = (uint32_t *)R.d_flag;
    HIP_TRY(hipMemsetAsync(flag, 0, 4, st));
    hipLaunchKernelGGL(k_mats_check, grid, block, 0, st, M, flag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(&bad, flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (bad) return fail(RT_ERR_INVALID, "rt_scene_set_prim_materials: a material is not one of the scene's");
    hipLaunchKernelGGL(k_mats_put, grid, block, 0, st, M);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return RT_OK;
}

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
