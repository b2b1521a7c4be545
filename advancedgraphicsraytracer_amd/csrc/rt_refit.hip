// rt_refit.hip -- in-place triangle updates with a bottom-up BVH refit (rt_scene_update_triangles).
//
// The tree's topology, primitive ids and leaf membership stay; three kernels rewrite what moves:
//   k_update_tris      one lane per updated triangle: its leaf-slot record (A | id, B-A | T_TRI, C-A),
//                      the normal of its shading record, its box (min / max of the three vertices,
//                      Primitive.h:319-388) and its sliver flag (mark_sticky's test) -- the same
//                      rt_math.h expressions as scene_create under the same -ffp-contract=off, so
//                      the records equal those of a fresh rt_scene_create on the new vertices;
//   k_refit_treelets   one workgroup per treelet (a whole subtree of at most kTreeletNodes nodes):
//                      leaves fold their slots' boxes as Scene::UpdateNodeBounds does
//                      (template/scene.h:855-865), then one height at a time, a barrier between
//                      heights, every interior node takes the union of its two children and the OR
//                      of their sticky bits;
//   k_refit_top        one workgroup, the same over the nodes above the cut.
// Boxes go through global memory: the waves of a workgroup share their CU's vector L1, so what one
// wave stored before the barrier another loads after it.  Nothing is handed from one workgroup to
// another inside a launch (the XCDs' L2s are not coherent with each other, and a CU's L1 is not
// refreshed by another CU's stores): the top reads the treelets' roots across the kernel boundary.
// min / max of floats are exact, so the refit reproduces the builder's boxes bit for bit.
#include "rt_refit.h"

#include <algorithm>

#include "rt_dev_types.h"

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
    std::vector<uint32_t> order, parent(used, ~0u), size(used, 0), height(used, 0);
    order.reserve(used);
    std::vector<uint32_t> st{0u};
    while (!st.empty()) {
        const uint32_t k = st.back();
        st.pop_back();
        order.push_back(k);
        if (N[k].count > 0) continue;
        for (uint32_t c : {N[k].leftFirst + 1, N[k].leftFirst}) { parent[c] = k; st.push_back(c); }
    }
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
    for (uint32_t k : order) {   // pre-order: a treelet's nodes follow its root
        if (size[k] > kTreeletNodes) { top.push_back(k); continue; }
        if (k != 0 && size[parent[k]] <= kTreeletNodes) continue;   // inside a treelet
        sub.clear();
        st.assign(1, k);
        while (!st.empty()) {
            const uint32_t j = st.back();
            st.pop_back();
            sub.push_back(j);
            if (N[j].count == 0) { st.push_back(N[j].leftFirst + 1); st.push_back(N[j].leftFirst); }
        }
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
    const float I16[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const f3 d0 = mk(p[0], p[1], p[2]), d1 = mk(p[3], p[4], p[5]), d2 = mk(p[6], p[7], p[8]);
    const f3 N = tvec(I16, normalize(cross(d2 - d0, d1 - d0)));      // Primitive.h:308-310
    const f3 a = tpos(I16, d0), b = tpos(I16, d1), c = tpos(I16, d2);  // Intersect, Primitive.h:249-254
    const f3 AB = b - a, AC = c - a;
    A.shade[2 * (size_t)id] = make_float4(N.x, N.y, N.z, A.shade[2 * (size_t)id].w);
    float4 *q = A.prims + 3 * (size_t)slot;
    q[0] = make_float4(a.x, a.y, a.z, __int_as_float((int)id));
    q[1] = make_float4(AB.x, AB.y, AB.z, __uint_as_float(T_TRI));
    q[2] = make_float4(AC.x, AC.y, AC.z, 0.0f);
    // mark_sticky's sliver test, in double on the float vertices
    double v[3][3], e[3][3], len[3];
    for (int k = 0; k < 3; ++k)
        for (int x = 0; x < 3; ++x) v[k][x] = p[3 * k + x];
    for (int k = 0; k < 3; ++k) {
        for (int x = 0; x < 3; ++x) e[k][x] = v[(k + 1) % 3][x] - v[k][x];
        len[k] = sqrt(e[k][0] * e[k][0] + e[k][1] * e[k][1] + e[k][2] * e[k][2]);
    }
    const double cx = e[0][1] * e[2][2] - e[0][2] * e[2][1], cy = e[0][2] * e[2][0] - e[0][0] * e[2][2],
                 cz = e[0][0] * e[2][1] - e[0][1] * e[2][0];
    const double area2 = sqrt(cx * cx + cy * cy + cz * cz);
    // the two longest edges in ascending order: drop the shortest (ties: any, the values are the same)
    double l1, l2;
    if (len[0] <= len[1] && len[0] <= len[2]) { l1 = len[1]; l2 = len[2]; }
    else if (len[1] <= len[0] && len[1] <= len[2]) { l1 = len[0]; l2 = len[2]; }
    else { l1 = len[0]; l2 = len[1]; }
    if (l1 > l2) { const double t = l1; l1 = l2; l2 = t; }
    const bool sliver = !(area2 >= A.sliver_lim * l1 * l2);
    const f3 mn = fmin3(a, fmin3(b, c)), mx = fmax3(a, fmax3(b, c));   // Primitive.h:319-388
    A.slot_box[2 * (size_t)slot] = make_float4(mn.x, mn.y, mn.z, __uint_as_float(sliver ? 1u : 0u));
    A.slot_box[2 * (size_t)slot + 1] = make_float4(mx.x, mx.y, mx.z, 0.0f);
}

__device__ __forceinline__ void refit_node(const RefitArgs &A, uint32_t k) {
    const float4 old = A.nodes[2 * (size_t)k + 1];
    const uint32_t word = __float_as_uint(old.z), cnt = word & 255u, lf = word >> 8;
    f3 mn, mx;
    bool sticky = false;
    if (cnt) {   // UpdateNodeBounds over the leaf's slots
        mn = mk(1e30f, 1e30f, 1e30f);
        mx = mk(-1e30f, -1e30f, -1e30f);
        for (uint32_t s = lf; s < lf + cnt; ++s) {
            const float4 lo = A.slot_box[2 * (size_t)s], hi = A.slot_box[2 * (size_t)s + 1];
            mn = fmin3(mn, mk(lo.x, lo.y, lo.z));
            mx = fmax3(mx, mk(hi.x, hi.y, hi.z));
            sticky = sticky || __float_as_uint(lo.w) != 0u;
        }
    } else {
        const float4 *c = A.nodes + 2 * (size_t)lf;
        const float4 l0 = c[0], l1 = c[1], r0 = c[2], r1 = c[3];
        mn = fmin3(mk(l0.x, l0.y, l0.z), mk(r0.x, r0.y, r0.z));
        mx = fmax3(mk(l0.w, l1.x, l1.y), mk(r0.w, r1.x, r1.y));
        sticky = l1.w == HUGE_VALF || r1.w == HUGE_VALF;
    }
    A.nodes[2 * (size_t)k] = make_float4(mn.x, mn.y, mn.z, mx.x);
    A.nodes[2 * (size_t)k + 1] = make_float4(mx.y, mx.z, old.z, sticky ? HUGE_VALF : A.margin);
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

void launch_refit(const RefitArgs &A, uint32_t ntreelets, bool has_top, hipStream_t st) {
    hipLaunchKernelGGL(k_refit_treelets, dim3(ntreelets), dim3(256), 0, st, A);
    if (has_top) hipLaunchKernelGGL(k_refit_top, dim3(1), dim3(1024), 0, st, A, ntreelets);
}

}  // namespace rt
