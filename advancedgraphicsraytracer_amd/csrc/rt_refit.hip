// rt_refit.hip -- in-place triangle updates with a bottom-up BVH refit (rt_scene_update_triangles).
//
// The tree's topology, primitive ids and leaf membership stay; three kernels rewrite what moves:
//   k_update_tris      one lane per updated triangle: its leaf-slot record (A | id, B-A | T_TRI, C-A),
//                      the normal of its shading record, its box (min / max of the three vertices,
//                      Primitive.h:319-388) and its sliver flag -- the rt_records.h encoders that
//                      scene creation runs, under the same -ffp-contract=off, so the records
//                      equal those of a fresh rt_scene_create on the new vertices;
//   k_refit_treelets   one workgroup per treelet (a whole subtree of at most kTreeletNodes nodes):
//                      leaves fold their slots' boxes as Scene::UpdateNodeBounds does
//                      (template/scene.h:855-865), then one height at a time, a barrier between
//                      heights, every interior node takes the union of its two children and the OR
//                      of their sticky bits;
//   k_refit_top        one workgroup, the same over the nodes above the cut.
// Two more front ends feed the same refit: rt_scene_update_prims (k_check_prims, k_update_prims:
// records of any kind, the light included) and rt_scene_transform_triangles (k_check_xform,
// k_xform_tris: ranges of triangles from object-space vertices and one matrix per range).
// Boxes go through global memory: the waves of a workgroup share their CU's vector L1, so what one
// wave stored before the barrier another loads after it.  Nothing is handed from one workgroup to
// another inside a launch (the XCDs' L2s are not coherent with each other, and a CU's L1 is not
// refreshed by another CU's stores): the top reads the treelets' roots across the kernel boundary.
// min / max of floats are exact, so the refit reproduces the builder's boxes bit for bit.
#include "rt_refit.h"

#include <algorithm>

#include "rt_records.h"

namespace rt {

bool build_refit_plan(const Bvh &b, uint32_t num_prims, RefitPlan &out) {
    const uint32_t used = b.nodes_used;
    const Node *N = b.nodes.data();
    if (b.indices.size() != num_prims) return false;
    out = RefitPlan();
    out.slot_of.assign(num_prims, ~0u);
    for (uint32_t k = 0; k < num_prims; ++k) {
        const uint32_t id = b.indices[k];
        if (id >= num_prims || out.slot_of[id] != ~0u) return false;
        out.slot_of[id] = k;
    }
    // pre-order from the root; sizes and heights in reverse
    TreeWalk w;
    if (walk_tree(N, used, num_prims, w) != kTreeOk) return false;
    const std::vector<uint32_t> &order = w.order;
    std::vector<uint32_t> size(used, 0), height(used, 0);
    for (size_t i = order.size(); i-- > 0;) {
        const uint32_t k = order[i];
        size[k] = 1;
        if (N[k].count > 0) continue;
        const uint32_t l = N[k].leftFirst;
        size[k] += size[l] + size[l + 1];
        height[k] = 1 + std::max(height[l], height[l + 1]);
    }
    auto by_height = [&](uint32_t x, uint32_t y) { return height[x] < height[y]; };
    auto emit = [&](std::vector<uint32_t> &nodes) {   // one group: its nodes by height, its level boundaries
        std::stable_sort(nodes.begin(), nodes.end(), by_height);
        out.grp.push_back((uint32_t)out.lvl.size());
        for (size_t i = 0; i < nodes.size(); ++i) {
            if (i == 0 || height[nodes[i]] != height[nodes[i - 1]]) out.lvl.push_back((uint32_t)out.list.size());
            out.list.push_back(nodes[i]);
        }
        out.lvl.push_back((uint32_t)out.list.size());
    };
    std::vector<uint32_t> top, sub;
    for (size_t i = 0; i < order.size(); ++i) {   // pre-order: a treelet's size[k] nodes start at its root
        const uint32_t k = order[i];
        if (size[k] > kTreeletNodes) { top.push_back(k); continue; }
        if (k != 0 && size[w.parent[k]] <= kTreeletNodes) continue;   // inside a treelet
        sub.assign(order.begin() + i, order.begin() + i + size[k]);
        emit(sub);
        ++out.ntreelets;
    }
    out.has_top = !top.empty();
    emit(top);
    out.grp.push_back((uint32_t)out.lvl.size());
    return true;
}

namespace {

constexpr uint32_t kExpMask = 0x7f800000u;

__global__ void __launch_bounds__(256) k_check_finite(const float *__restrict__ v, uint32_t n, uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && (__float_as_uint(v[i]) & kExpMask) == kExpMask) *flag = 1u;
}

__global__ void __launch_bounds__(256) k_update_tris(RefitArgs A, uint32_t first, uint32_t count,
                                                     const float *__restrict__ verts) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t id = first + i, slot = A.slot_of[id];
    const float *p = verts + 9u * (size_t)i;
    const f3 N = tri_normal(p);
    A.shade[2 * (size_t)id] = make_float4(N.x, N.y, N.z, A.shade[2 * (size_t)id].w);
    tri_record(p, id, A.prims + 3 * (size_t)slot);
    f3 mn, mx;
    tri_box(p, mn, mx);
    slot_box(mn, mx, tri_sliver(p, A.sliver_lim), A.slot_box + 2 * (size_t)slot);
}

__device__ __forceinline__ bool finite_f(float f) { return (__float_as_uint(f) & kExpMask) != kExpMask; }
__device__ __forceinline__ bool finite_f3(f3 a) { return finite_f(a.x) && finite_f(a.y) && finite_f(a.z); }

// rt_scene_update_prims' validation, one lane per record: type and material as the scene holds them
// (the shading record's words), every field its kind reads finite, its transform finite where one
// is read (cubes and quads), its box finite.  Writes nothing but the flag.
__global__ void __launch_bounds__(256) k_check_prims(const float4 *__restrict__ shade, uint32_t first, uint32_t count,
                                                     const rt_prim *__restrict__ prims, const float *__restrict__ T,
                                                     uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t id = first + i;
    const rt_prim p = prims[i];
    bool ok = (uint32_t)p.type == fbits(shade[2 * (size_t)id + 1].x) && (uint32_t)p.material == fbits(shade[2 * (size_t)id].w);
    if (ok) {
        const int nf = p.type == RT_TRIANGLE ? 9 : p.type == RT_CUBE ? 6 : p.type == RT_QUAD ? 1 : 4;
        for (int k = 0; k < nf; ++k) ok = ok && finite_f(p.v[k]);
        const float *Ti = (T && (p.type == RT_CUBE || p.type == RT_QUAD)) ? T + 16u * (size_t)i : nullptr;
        for (int k = 0; Ti && k < 16; ++k) ok = ok && finite_f(Ti[k]);
        PrimX x;
        PrimGeom g;
        prim_transform(p, Ti, x);
        prim_geometry(p, x, g);
        ok = ok && finite_f3(g.bmin) && finite_f3(g.bmax);
    }
    if (!ok) *flag = 1u;
}

// one lane per record: the leaf-slot record, the shading record (material word kept), a cube's or a
// quad's side-table entry (through the index its shading record holds) and the slot box; the sticky
// flag is tri_sliver's for a triangle and stays as it is for every other kind (mark_sticky's depends
// on the kind alone)
__global__ void __launch_bounds__(256) k_update_prims(RefitArgs A, float4 *__restrict__ xprims, uint32_t first,
                                                      uint32_t count, const rt_prim *__restrict__ prims,
                                                      const float *__restrict__ T) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= count) return;
    const uint32_t id = first + i, slot = A.slot_of[id];
    const rt_prim p = prims[i];
    const bool xf = p.type == RT_CUBE || p.type == RT_QUAD;
    PrimX x;
    PrimGeom g;
    prim_transform(p, (T && xf) ? T + 16u * (size_t)i : nullptr, x);
    prim_geometry(p, x, g);
    const float4 old0 = A.shade[2 * (size_t)id], old1 = A.shade[2 * (size_t)id + 1];
    const uint32_t xi = fbits(old1.z);
    float4 s[2];
    prim_shade(p, x, xi, s);
    s[0].w = old0.w;
    A.shade[2 * (size_t)id] = s[0];
    A.shade[2 * (size_t)id + 1] = s[1];
    prim_record(p, x, id, xi, A.prims + 3 * (size_t)slot);
    if (xf) prim_xentry(p, x, xprims + 8 * (size_t)xi);
    const bool sticky = p.type == RT_TRIANGLE ? tri_sliver(p.v, A.sliver_lim) : slot_sticky(A.slot_box[2 * (size_t)slot]);
    slot_box(g.bmin, g.bmax, sticky, A.slot_box + 2 * (size_t)slot);
}

// rt_scene_transform_triangles.  Lane i of the back-to-back rest triangles finds its range by binary
// search over the prefix counts (pre[r] = triangles before range r, pre[nr] = all of them).
__device__ __forceinline__ uint32_t range_of(const uint32_t *__restrict__ pre, uint32_t nr, uint32_t i) {
    uint32_t lo = 0, hi = nr;   // pre[lo] <= i < pre[hi]
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (pre[mid] <= i) lo = mid;
        else hi = mid;
    }
    return lo;
}
// world vertices = TransformPosition(rest, M) per vertex, as Scene::LoadModel places a mesh
// (template/scene.h:185-191)
__device__ __forceinline__ void xform_tri(const XformRanges &R, uint32_t i, const float *__restrict__ rest, float w[9],
                                          uint32_t &id) {
    const uint32_t r = range_of(R.pre, R.nr, i);
    const float *M = R.M + 16u * (size_t)r;
    const float *q = rest + 9u * (size_t)i;
    for (int k = 0; k < 3; ++k) {
        const f3 v = tpos(M, mk(q[3 * k], q[3 * k + 1], q[3 * k + 2]));
        w[3 * k] = v.x; w[3 * k + 1] = v.y; w[3 * k + 2] = v.z;
    }
    id = R.first[r] + (i - R.pre[r]);
}
__global__ void __launch_bounds__(256) k_check_xform(XformRanges R, uint32_t total, const float *__restrict__ rest,
                                                     uint32_t *flag) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    float w[9];
    uint32_t id;
    xform_tri(R, i, rest, w, id);
    bool ok = true;
    for (int k = 0; k < 9; ++k) ok = ok && finite_f(w[k]);
    if (!ok) *flag = 1u;
}
__global__ void __launch_bounds__(256) k_xform_tris(RefitArgs A, XformRanges R, uint32_t total,
                                                    const float *__restrict__ rest) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= total) return;
    float w[9];
    uint32_t id;
    xform_tri(R, i, rest, w, id);
    const uint32_t slot = A.slot_of[id];
    const f3 N = tri_normal(w);
    A.shade[2 * (size_t)id] = make_float4(N.x, N.y, N.z, A.shade[2 * (size_t)id].w);
    tri_record(w, id, A.prims + 3 * (size_t)slot);
    f3 mn, mx;
    tri_box(w, mn, mx);
    slot_box(mn, mx, tri_sliver(w, A.sliver_lim), A.slot_box + 2 * (size_t)slot);
}

__device__ __forceinline__ void refit_node(const RefitArgs &A, uint32_t k) {
    const uint32_t word = fbits(A.nodes[2 * (size_t)k + 1].z), cnt = word & 255u, lf = word >> 8;
    f3 mn, mx;
    bool sticky = false;
    if (cnt) {   // UpdateNodeBounds over the leaf's slots
        mn = mk(1e30f, 1e30f, 1e30f);
        mx = mk(-1e30f, -1e30f, -1e30f);
        for (uint32_t s = lf; s < lf + cnt; ++s) {
            const float4 lo = A.slot_box[2 * (size_t)s], hi = A.slot_box[2 * (size_t)s + 1];
            mn = fmin3(mn, mk(lo.x, lo.y, lo.z));
            mx = fmax3(mx, mk(hi.x, hi.y, hi.z));
            sticky = sticky || slot_sticky(lo);
        }
    } else {
        const float4 *c = A.nodes + 2 * (size_t)lf;
        const float4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
        f3 lmn, lmx, rmn, rmx;
        node_box(l0, l1, lmn, lmx);
        node_box(r0, r1, rmn, rmx);
        mn = fmin3(lmn, rmn);
        mx = fmax3(lmx, rmx);
        sticky = is_sticky(l1.w) || is_sticky(r1.w);
    }
    node_pack(mn, mx, word, walk_word(sticky, A.margin), A.nodes + 2 * (size_t)k);
}

// group g's heights in turn; every wave of the workgroup takes every barrier
__device__ __forceinline__ void refit_group(const RefitArgs &A, uint32_t g) {
    const uint32_t l0 = A.grp[g], l1 = A.grp[g + 1] - 1u;
    for (uint32_t l = l0; l < l1; ++l) {
        const uint32_t b = A.lvl[l], e = A.lvl[l + 1];
        for (uint32_t i = b + threadIdx.x; i < e; i += blockDim.x) refit_node(A, A.list[i]);
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_refit_treelets(RefitArgs A) { refit_group(A, blockIdx.x); }
__global__ void __launch_bounds__(1024) k_refit_top(RefitArgs A, uint32_t g) { refit_group(A, g); }

}  // namespace

void launch_check_finite(const float *verts_dev, uint32_t n, uint32_t *flag_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_check_finite, dim3((n + 255u) / 256u), dim3(256), 0, st, verts_dev, n, flag_dev);
}

void launch_update_tris(const RefitArgs &A, uint32_t first, uint32_t count, const float *verts_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_update_tris, dim3((count + 255u) / 256u), dim3(256), 0, st, A, first, count, verts_dev);
}

void launch_check_prims(const float4 *shade, uint32_t first, uint32_t count, const rt_prim *prims_dev,
                        const float *transforms_dev, uint32_t *flag_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_check_prims, dim3((count + 255u) / 256u), dim3(256), 0, st, shade, first, count, prims_dev,
                       transforms_dev, flag_dev);
}

void launch_update_prims(const RefitArgs &A, float4 *xprims, uint32_t first, uint32_t count, const rt_prim *prims_dev,
                         const float *transforms_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_update_prims, dim3((count + 255u) / 256u), dim3(256), 0, st, A, xprims, first, count, prims_dev,
                       transforms_dev);
}

void launch_check_xform(const XformRanges &R, uint32_t total, const float *rest_dev, uint32_t *flag_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_check_xform, dim3((total + 255u) / 256u), dim3(256), 0, st, R, total, rest_dev, flag_dev);
}

void launch_xform_tris(const RefitArgs &A, const XformRanges &R, uint32_t total, const float *rest_dev, hipStream_t st) {
    hipLaunchKernelGGL(k_xform_tris, dim3((total + 255u) / 256u), dim3(256), 0, st, A, R, total, rest_dev);
}

void launch_refit(const RefitArgs &A, uint32_t ntreelets, bool has_top, hipStream_t st) {
    hipLaunchKernelGGL(k_refit_treelets, dim3(ntreelets), dim3(256), 0, st, A);
    if (has_top) hipLaunchKernelGGL(k_refit_top, dim3(1), dim3(1024), 0, st, A, ntreelets);
}

}  // namespace rt
