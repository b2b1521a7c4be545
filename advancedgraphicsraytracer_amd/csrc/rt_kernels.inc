// rt_kernels.inc -- the gfx950 kernels (compiled twice: rt_kern_core.hip, rt_kern_ext.hip).
//
// Hot path (SURVEY.md 8(a)): Renderer::Tick -> Camera::GetPrimaryRay -> Renderer::Trace
// -> Scene::IntersectBVH / IsOccluded -> Primitive::Intersect / Hit, plus
// NextEventDirectIllumination, the Diffuse / Mirror / Dielectric / Checkerboard / Light
// materials, the sky lookup, the running-average accumulator and the RGB8 pack -- all in
// ONE kernel launch per frame (k_render).  Launch shape: 256-thread workgroups of four
// wave64s, one wave per 8x8 screen tile (the reference's PACKET_SIZE 64 / SQRT_PACKET_SIZE 8,
// Ray.h:3-5), one lane per pixel.  No MFMA: this is branchy scalar fp32.
//
// Device scene layout in HBM (built once by rt_scene_create):
//   nodes  : the reference's 32-byte BVHNode array (root 0, node 1 unused, sibling pairs
//            64-byte aligned) with (leftFirst, count) replaced by one packed word
//            (leftFirst << 8 | count) so a 64-byte sibling-pair load carries everything
//            the traversal needs;
//   prims  : leaf order (primitiveIndices applied), 48 B per slot: triangle A, B-A, C-A
//            (host-computed, bit-identical to the reference's per-test subtraction) and
//            the original primitive id -- no index indirection in the leaf loop;
//   shade  : per primitive id, 32 B: geometric normal (triangles, host-computed with the
//            reference's normalize(cross(..))), sphere centre / 1/r, material id;
//   per-lane traversal stack: LDS, [depth][256 lanes] u32, conflict-free.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <map>
#include <mutex>
#include <tuple>
#include <type_traits>

#include "rt_dev_types.h"
#include "rt_libm.h"
#include "rt_math.h"

#ifndef RT_KNS
#error "define RT_KNS (kcore / kext) and RT_EXT (0 / 1) before including rt_kernels.inc"
#endif

namespace rt {
namespace RT_KNS {

// the extension primitives / materials are compiled in only where the scene has them, so
// the hot kernels carry none of their registers
constexpr bool kExt = RT_EXT != 0;

// Phase stamps, diagnostic builds only (tools/build_variant.sh NAME -DRT_FRAME_PHASES, read by
// tools/frame_phases.py): the first active lane of a wave stores s_memtime at six points of the
// primary+shadow frame -- [0] wave start, [1] head done (ray ready), [2] camera traversal done,
// [3] shading done (shadow ray ready), [4] shadow traversal done, [5] wave end -- into
// rt_frame_phase_buf[unit * 8 + k] with ordinary vector stores.  Waves past kFramePhaseWaves are not
// recorded; a phase a wave never reaches stays 0.  The production build compiles none of it.
#ifdef RT_FRAME_PHASES
constexpr uint32_t kFramePhaseWaves = 65536;
__device__ unsigned long long rt_frame_phase_buf[kFramePhaseWaves * 8u];
__device__ __forceinline__ void frame_phase(uint32_t k) {
    const uint32_t unit = blockIdx.x * 4u + (threadIdx.x >> 6);
    const unsigned long long t = __builtin_amdgcn_s_memtime();
    const uint32_t first = (uint32_t)__builtin_ctzll(__ballot(1));
    if (unit < kFramePhaseWaves && (threadIdx.x & 63u) == first) rt_frame_phase_buf[unit * 8u + k] = t;
}
#else
__device__ __forceinline__ void frame_phase(uint32_t) {}
#endif


struct DRay {
    f3 O, D, rD;
    float t;
    int obj;
    int inside;
    float u, v;
};

__device__ __forceinline__ DRay make_ray(f3 O, f3 D, float t) {   // Ray.h:9-16
    DRay r;
    r.O = O; r.D = D; r.t = t; r.obj = -1; r.inside = 0; r.u = 0.0f; r.v = 0.0f;
    r.rD = mk(1 / D.x, 1 / D.y, 1 / D.z);
    return r;
}

// cold-path transcendentals (textured sky, sphere u/v): correctly rounded float via the
// double functions, as the oracle does; the hot cos/sin/exp come from rt_libm.h
__device__ __forceinline__ float cr_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }
__device__ __forceinline__ float cr_acos(float x) { return (float)acos((double)x); }
__device__ __forceinline__ float cr_asin(float x) { return (float)asin((double)x); }

// ------------------------------------------------------------------ slab tests (scene.h:414-450)
// EXACT: the reference's std::min/std::max selects, NaN behaviour included.
// FAST (chosen per wave when every active ray has a finite origin and finite 1/D and the
// scene's node bounds are NaN-free): no slab product can then be NaN, and on non-NaN
// inputs the selects equal IEEE minNum/maxNum up to the sign of a zero result, which no
// consumer can observe (the values are only compared) -- so v_min3/v_max3 give the
// identical decisions with a third of the instructions.
template <bool FAST>
__device__ __forceinline__ void slab(const DRay &r, float4 a, float4 b, float &tmn, float &tmx) {
    float tx1 = (a.x - r.O.x) * r.rD.x, tx2 = (a.w - r.O.x) * r.rD.x;
    float ty1 = (a.y - r.O.y) * r.rD.y, ty2 = (b.x - r.O.y) * r.rD.y;
    float tz1 = (a.z - r.O.z) * r.rD.z, tz2 = (b.y - r.O.z) * r.rD.z;
    if (FAST) {
        tmn = fmaxf(fmaxf(fminf(tx1, tx2), fminf(ty1, ty2)), fminf(tz1, tz2));
        tmx = fminf(fminf(fmaxf(tx1, tx2), fmaxf(ty1, ty2)), fmaxf(tz1, tz2));
    } else {
        tmn = smin(tx1, tx2); tmx = smax(tx1, tx2);
        tmn = smax(tmn, smin(ty1, ty2)); tmx = smin(tmx, smax(ty1, ty2));
        tmn = smax(tmn, smin(tz1, tz2)); tmx = smin(tmx, smax(tz1, tz2));
    }
}
template <bool FAST>
__device__ __forceinline__ float slab_dist(const DRay &r, float4 a, float4 b) {
    float tmn, tmx;
    slab<FAST>(r, a, b, tmn, tmx);
    return (tmx >= tmn && tmn < r.t && tmx > 0) ? tmn : 1e30f;
}
template <bool FAST>
__device__ __forceinline__ bool slab_hit(const DRay &r, float4 a, float4 b) {
    float tmn, tmx;
    slab<FAST>(r, a, b, tmn, tmx);
    return tmx >= tmn && tmn < r.t && tmx > 0;
}
__device__ __forceinline__ float slab_accept(const DRay &r, float tmn, float tmx) {
    return (tmx >= tmn && tmn < r.t && tmx > 0) ? tmn : 1e30f;
}

__device__ __forceinline__ bool ray_finite(const DRay &r) {
    return isfinite(r.O.x) && isfinite(r.O.y) && isfinite(r.O.z) && isfinite(r.rD.x) && isfinite(r.rD.y) &&
           isfinite(r.rD.z);
}

// ------------------------------------------------------------------ primitive tests (Primitive.h:64-279)
// TransformPosition / TransformVector with the matrix as three float4 rows (same order of
// operations as rt_math.h tpos / tvec)
__device__ __forceinline__ f3 tpos_rows(float4 r0, float4 r1, float4 r2, f3 a) {
    return mk(r0.x * a.x + r0.y * a.y + r0.z * a.z + r0.w * 1.0f, r1.x * a.x + r1.y * a.y + r1.z * a.z + r1.w * 1.0f,
              r2.x * a.x + r2.y * a.y + r2.z * a.z + r2.w * 1.0f);
}
__device__ __forceinline__ f3 tvec_rows(float4 r0, float4 r1, float4 r2, f3 a) {
    return mk(r0.x * a.x + r0.y * a.y + r0.z * a.z + r0.w * 0.0f, r1.x * a.x + r1.y * a.y + r1.z * a.z + r1.w * 0.0f,
              r2.x * a.x + r2.y * a.y + r2.z * a.z + r2.w * 0.0f);
}
// CUBE slab test in object space (Primitive.h:87-110 / 196-235); false on a miss
__device__ __forceinline__ bool cube_slab(const float4 *x, const DRay &r, float &tmin_o, float &tmax_o) {
    const f3 O = tpos_rows(x[0], x[1], x[2], r.O), D = tvec_rows(x[0], x[1], x[2], r.D);
    const float4 d0 = x[6], d1 = x[7];
    const float rDx = 1 / D.x, rDy = 1 / D.y, rDz = 1 / D.z;
    const bool sx = D.x < 0, sy = D.y < 0, sz = D.z < 0;
    float tmin = ((sx ? d1.x : d0.x) - O.x) * rDx;
    float tmax = ((sx ? d0.x : d1.x) - O.x) * rDx;
    const float tymin = ((sy ? d1.y : d0.y) - O.y) * rDy;
    const float tymax = ((sy ? d0.y : d1.y) - O.y) * rDy;
    if (tmin > tymax || tymin > tmax) return false;
    tmin = smax(tmin, tymin);
    tmax = smin(tmax, tymax);
    const float tzmin = ((sz ? d1.z : d0.z) - O.z) * rDz;
    const float tzmax = ((sz ? d0.z : d1.z) - O.z) * rDz;
    if (tmin > tzmax || tzmin > tmax) return false;
    tmin_o = smax(tmin, tzmin);
    tmax_o = smin(tmax, tzmax);
    return true;
}
// QUAD plane distance in object space (Primitive.h:111-117 / 236-247)
__device__ __forceinline__ float quad_t(const float4 *x, const DRay &r, f3 &O, f3 &D) {
    O = tpos_rows(x[0], x[1], x[2], r.O);
    D = tvec_rows(x[0], x[1], x[2], r.D);
    return O.y / -D.y;
}
// cubes and quads (off the hot path): Intersect; `tie` as in prim_intersect_t
__device__ __forceinline__ void xprim_intersect(const SceneView &S, uint32_t type, uint32_t xi, int id, DRay &r,
                                             bool &tie) {
    const float4 *x = S.xprims + 8 * xi;
    if (type == T_CUBE) {   // the acceptance test is on tmax (Primitive.h:221-233)
        float tmin, tmax;
        if (!cube_slab(x, r, tmin, tmax)) return;
        float t;
        if (tmin > kEPS) t = tmin;
        else if (tmax > kEPS) t = tmax;
        else return;
        if (tmax < r.t) { r.t = t; r.obj = id; }
        else if (tmax == r.t) tie = true;
    } else {
        f3 O, D;
        const float t = quad_t(x, r, O, D);
        const float size = x[6].x;
        if (t <= r.t && t > kEPS) {
            const f3 I = O + t * D;
            if (I.x > -size && I.x < size && I.z > -size && I.z < size) {
                if (t == r.t) tie = true;
                else { r.t = t; r.obj = id; r.u = 0.0f; r.v = 0.0f; }   // u, v unset there: 0
            }
        }
    }
}
__device__ __forceinline__ bool xprim_hit(const SceneView &S, uint32_t type, uint32_t xi, const DRay &r) {
    const float4 *x = S.xprims + 8 * xi;
    if (type == T_CUBE) {
        float tmin, tmax;
        if (!cube_slab(x, r, tmin, tmax)) return false;
        return (tmin > kEPS || tmax > kEPS) && tmax < r.t;
    }
    f3 O, D;
    const float t = quad_t(x, r, O, D);   // the quad's extent is not tested (reference quirk)
    return t < r.t && t > kEPS;
}
// P = the leaf-order primitive slots (global memory or the workgroup's LDS copy)
// A slot's three float4 are loaded together (round 5): the third is a triangle's AC edge, which
// loaded only after the type test (p1.w) cost a second dependent round trip per triangle in every
// leaf loop (TEAPOT-F 0.0957 -> 0.0937 ms, profiles/r05/primab); every slot holds three float4, so
// the eager load is always in bounds.
__device__ __forceinline__ void prim_record(const float4 *P, uint32_t k, float4 &p0, float4 &p1, float4 &p2) {
    p0 = P[3 * k];
    p1 = P[3 * k + 1];
    p2 = P[3 * k + 2];
    asm volatile("" : "+v"(p2.x), "+v"(p2.y), "+v"(p2.z));   // issued beside p0 / p1, not sunk under the type test
}
// Primitive::Intersect of one slot's record (p2 = a triangle's AC edge, unused otherwise)
__device__ __forceinline__ void prim_test(const SceneView &S, float4 p0, float4 p1, float4 p2, DRay &r) {
    uint32_t type = __float_as_uint(p1.w);
    int id = __float_as_int(p0.w);
    if (type == T_TRI) {
        f3 A = mk(p0.x, p0.y, p0.z), AB = mk(p1.x, p1.y, p1.z), AC = mk(p2.x, p2.y, p2.z);
        float denom = dot(cross(r.D, AC), AB);
        if (fabsf(denom) < kDENOM_EPS) return;
        f3 AO = r.O - A;
        const float nu = dot(cross(-r.D, AO), AC);
        float u = nu / denom;
        if (u < 0 || u > 1) return;
        const float nv = dot(cross(-r.D, AB), AO);
        float v = nv / denom;
        if (v < 0 || u + v > 1) return;
        const float nt = dot(cross(AO, AB), AC);
        float t = nt / denom;
        if (t < r.t && t > kEPS) { r.t = t; r.obj = id; r.u = u; r.v = v; }
    } else if (type == T_SPH) {
        f3 oc = r.O - mk(p0.x, p0.y, p0.z);
        float b = dot(oc, r.D);
        float c = dot(oc, oc) - p1.x;
        float d = b * b - c;
        if (d <= 0) return;
        d = sqrtf(d);
        float t = -b - d;
        if (!(t < r.t && t > kEPS)) {
            t = d - b;
            if (!(t < r.t && t > kEPS)) return;
        }
        r.t = t; r.obj = id;            // u, v filled in after traversal (finish_uv)
    } else if (type == T_PLANE) {
        f3 N = mk(p0.x, p0.y, p0.z);
        float t = -(dot(r.O, N) + p1.x) / (dot(r.D, N));
        if (t < r.t && t > kEPS) { r.t = t; r.obj = id; }
    } else if constexpr (kExt) {
        bool tie = false;
        xprim_intersect(S, type, __float_as_uint(p1.x), id, r, tie);
    }
}
__device__ __forceinline__ void prim_intersect(const SceneView &S, const float4 *P, uint32_t k, DRay &r) {
    float4 p0, p1, p2;
    prim_record(P, k, p0, p1, p2);
    prim_test(S, p0, p1, p2, r);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
// prim_intersect plus `tie`: set when the candidate distance equals the current r.t
// exactly (a second primitive at the same distance: the visiting order would decide).
// UNI: k is wave-uniform (the wave walk's leaves): the 48-B record comes in with two scalar loads
// instead of three vector loads returning 64 copies.
template <bool UNI = false>
__device__ __forceinline__ void prim_intersect_t(const SceneView &S, const float4 *P, uint32_t k, DRay &r, bool &tie) {
    float4 p0, p1, p2;
    if constexpr (UNI) {
        u32x8 a;
        u32x4 b;
        asm volatile("s_load_dwordx8 %0, %2, 0\n\ts_load_dwordx4 %1, %2, 32\n\ts_waitcnt lgkmcnt(0)"
                     : "=s"(a), "=s"(b) : "s"(P + 3 * k) : "memory");
        p0 = make_float4(__uint_as_float(a[0]), __uint_as_float(a[1]), __uint_as_float(a[2]), __uint_as_float(a[3]));
        p1 = make_float4(__uint_as_float(a[4]), __uint_as_float(a[5]), __uint_as_float(a[6]), __uint_as_float(a[7]));
        p2 = make_float4(__uint_as_float(b[0]), __uint_as_float(b[1]), __uint_as_float(b[2]), __uint_as_float(b[3]));
    } else {
        prim_record(P, k, p0, p1, p2);
    }
    uint32_t type = __float_as_uint(p1.w);
    int id = __float_as_int(p0.w);
    if (type == T_TRI) {
        f3 A = mk(p0.x, p0.y, p0.z), AB = mk(p1.x, p1.y, p1.z), AC = mk(p2.x, p2.y, p2.z);
        float denom = dot(cross(r.D, AC), AB);
        if (fabsf(denom) < kDENOM_EPS) return;
        f3 AO = r.O - A;
        const float nu = dot(cross(-r.D, AO), AC);
        float u = nu / denom;
        if (u < 0 || u > 1) return;
        const float nv = dot(cross(-r.D, AB), AO);
        float v = nv / denom;
        if (v < 0 || u + v > 1) return;
        const float nt = dot(cross(AO, AB), AC);
        float t = nt / denom;
        if (t <= r.t && t > kEPS) {
            if (t == r.t) tie = true;
            else { r.t = t; r.obj = id; r.u = u; r.v = v; }
        }
    } else if (type == T_SPH) {
        f3 oc = r.O - mk(p0.x, p0.y, p0.z);
        float b = dot(oc, r.D);
        float c = dot(oc, oc) - p1.x;
        float d = b * b - c;
        if (d <= 0) return;
        d = sqrtf(d);
        float t = -b - d;
        if (t == r.t && t > kEPS) tie = true;
        if (!(t < r.t && t > kEPS)) {
            t = d - b;
            if (t == r.t && t > kEPS) tie = true;
            if (!(t < r.t && t > kEPS)) return;
        }
        r.t = t; r.obj = id;
    } else if (type == T_PLANE) {
        f3 N = mk(p0.x, p0.y, p0.z);
        float t = -(dot(r.O, N) + p1.x) / (dot(r.D, N));
        if (t == r.t && t > kEPS) tie = true;
        if (t < r.t && t > kEPS) { r.t = t; r.obj = id; }
    } else if constexpr (kExt) {
        xprim_intersect(S, type, __float_as_uint(p1.x), id, r, tie);
    }
}

__device__ __forceinline__ bool prim_hit_rec(const SceneView &S, float4 p0, float4 p1, float4 p2, const DRay &r) {
    uint32_t type = __float_as_uint(p1.w);
    if (type == T_TRI) {
        f3 A = mk(p0.x, p0.y, p0.z), AB = mk(p1.x, p1.y, p1.z), AC = mk(p2.x, p2.y, p2.z);
        float denom = dot(cross(r.D, AC), AB);
        if (fabsf(denom) < kDENOM_EPS) return false;
        f3 AO = r.O - A;
        const float nu = dot(cross(-r.D, AO), AC);
        float u = nu / denom;
        if (u < 0 || u > 1) return false;
        const float nv = dot(cross(-r.D, AB), AO);
        float v = nv / denom;
        if (v < 0 || u + v > 1) return false;
        const float nt = dot(cross(AO, AB), AC);
        float t = nt / denom;
        return t < r.t && t > kEPS;
    } else if (type == T_SPH) {
        f3 oc = r.O - mk(p0.x, p0.y, p0.z);
        float b = dot(oc, r.D);
        float c = dot(oc, oc) - p1.x;
        float d = b * b - c;
        if (d <= 0) return false;
        d = sqrtf(d);
        float t = -b - d;
        if (t < r.t && t > kEPS) return true;
        t = d - b;
        return t < r.t && t > kEPS;
    } else if (type == T_PLANE) {
        f3 N = mk(p0.x, p0.y, p0.z);
        float t = -(dot(r.O, N) + p1.x) / (dot(r.D, N));
        return t < r.t && t > kEPS;
    } else if constexpr (kExt) {
        return xprim_hit(S, type, __float_as_uint(p1.x), r);
    }
    return false;
}
__device__ __forceinline__ bool prim_hit(const SceneView &S, const float4 *P, uint32_t k, const DRay &r) {
    float4 p0, p1, p2;
    prim_record(P, k, p0, p1, p2);
    return prim_hit_rec(S, p0, p1, p2, r);
}
// a leaf's primitives in slot order: closest hit (every slot) / any hit (stops at the first hit)
__device__ __forceinline__ void leaf_closest(const SceneView &S, const float4 *P, uint32_t lf, uint32_t cnt, DRay &r) {
    for (uint32_t k = lf; k < lf + cnt; ++k) prim_intersect(S, P, k, r);
}
__device__ __forceinline__ bool leaf_any(const SceneView &S, const float4 *P, uint32_t lf, uint32_t cnt, const DRay &r) {
    for (uint32_t k = lf; k < lf + cnt; ++k)
        if (prim_hit(S, P, k, r)) return true;
    return false;
}

// u, v of a sphere / plane hit, evaluated once for the final hit: identical to the
// reference's evaluation at acceptance time (same t, same centre).
__device__ __forceinline__ void finish_uv(const SceneView &S, DRay &r) {
    if (r.obj < 0) return;
    float4 s0 = S.shade[2 * r.obj], s1 = S.shade[2 * r.obj + 1];
    uint32_t type = __float_as_uint(s1.x);
    f3 I = r.O + r.t * r.D;
    if (type == T_SPH) {
        f3 cToI = normalize(I - mk(s0.x, s0.y, s0.z));
        r.u = 0.5f - cr_atan2(cToI.z, cToI.x) * kINV2PI;
        r.v = 0.5f - cr_asin(cToI.y) * kINVPI;
    } else if (type == T_PLANE) {
        if (s0.x < kFLT_EPSILON && s0.y < kFLT_EPSILON) { r.u = I.x; r.v = -I.y; }
        else if (s0.x < kFLT_EPSILON && s0.z < kFLT_EPSILON) { r.u = I.x; r.v = -I.z; }
        else if (s0.y < kFLT_EPSILON && s0.z < kFLT_EPSILON) { r.u = I.y; r.v = -I.z; }
        else { r.u = 0.0f; r.v = 0.0f; }   // left unset by the reference: defined as 0
    } else if (!kExt) {
        return;
    } else if (type == T_QUAD) {
        r.u = 0.0f; r.v = 0.0f;
    } else if (type == T_CUBE) {           // Primitive::setTextureCoordsCube, Primitive.h:752-797
        const float4 *x = S.xprims + 8 * __float_as_uint(s1.z);
        const f3 o = tpos_rows(x[0], x[1], x[2], I);
        const float4 d0 = x[6], d1 = x[7];
        float uc = o.z, vc = o.y;
        const float e0 = fabsf(o.x - d0.x), e1 = fabsf(o.x - d1.x), e2 = fabsf(o.y - d0.y), e3 = fabsf(o.y - d1.y);
        const float e4 = fabsf(o.z - d0.z), e5 = fabsf(o.z - d1.z);
        float minDist = e0;
        int face = 1;
        if (e1 < minDist) uc = -o.z, vc = o.y, face = 0, minDist = e1;
        if (e2 < minDist) uc = o.x, vc = o.z, face = 3, minDist = e2;
        if (e3 < minDist) uc = o.x, vc = -o.z, face = 2, minDist = e3;
        if (e4 < minDist) uc = -o.x, vc = o.y, face = 5, minDist = e4;
        if (e5 < minDist) uc = o.x, vc = o.y, face = 4;
        uc = -uc, vc = -vc;
        uc = 0.5f * (uc / d1.x + 1.0f);
        vc = 0.5f * (vc / d1.x + 1.0f);
        const float third = 1.0f / 3.0f;
        const float fu = face == 0 ? 2.0f : face == 1 ? 0.0f : face == 5 ? 3.0f : 1.0f;
        const float fv = face == 2 ? 0.0f : face == 3 ? 2.0f : 1.0f;
        r.u = 0.25f * (fu + uc);
        r.v = third * (fv + vc);
    }
}

// Scene::GetNormal (template/scene.h:489-497) of the hit primitive at I, not yet flipped:
// Primitive::GetNormal (Primitive.h:284-314)
__device__ __forceinline__ f3 prim_normal(const SceneView &S, float4 s0, float4 s1, f3 I) {
    const uint32_t type = __float_as_uint(s1.x);
    if (type == T_SPH) return (I - mk(s0.x, s0.y, s0.z)) * s1.y;
    if (!kExt || type != T_CUBE) return mk(s0.x, s0.y, s0.z);
    const float4 *x = S.xprims + 8 * __float_as_uint(s1.z);
    const f3 o = tpos_rows(x[0], x[1], x[2], I);
    const float4 d0 = x[6], d1 = x[7];
    f3 N = mk(-1, 0, 0);
    const float e0 = fabsf(o.x - d0.x), e1 = fabsf(o.x - d1.x), e2 = fabsf(o.y - d0.y), e3 = fabsf(o.y - d1.y);
    const float e4 = fabsf(o.z - d0.z), e5 = fabsf(o.z - d1.z);
    float minDist = e0;
    if (e1 < minDist) minDist = e1, N.x = 1;
    if (e2 < minDist) minDist = e2, N = mk(0, -1, 0);
    if (e3 < minDist) minDist = e3, N = mk(0, 1, 0);
    if (e4 < minDist) minDist = e4, N = mk(0, 0, -1);
    if (e5 < minDist) minDist = e5, N = mk(0, 0, 1);
    return tvec_rows(x[3], x[4], x[5], N);
}
__device__ __forceinline__ f3 prim_normal(const SceneView &S, int obj, f3 I) {
    return prim_normal(S, S.shade[2 * obj], S.shade[2 * obj + 1], I);
}

// Scene::GetNormal (flipped against the ray) and Scene::GetMaterial of a hit; a
// TextureMaterial also needs the hit's u, v (deferred by the traversal, finish_uv)
__device__ __forceinline__ const DevMaterial &hit_surface(const SceneView &S, DRay &ray, f3 I, f3 &N) {
    N = prim_normal(S, ray.obj, I);
    if (dot(N, ray.D) > 0) N = -N;
    const DevMaterial &m = S.mats[__float_as_int(S.shade[2 * ray.obj].w)];
    if (kExt && m.kind == RT_TEXTURE) finish_uv(S, ray);
    return m;
}

// hit_surface with whole records (the single-sample frame kernel): both float4 of the hit's shade
// record in one request, the material index taken from it, then the material's first 48 bytes
// (kind .. tex_off; the extension build: all 64) in one request -- two dependent round trips.  Field
// by field the compiler narrows each load to what its first user needs and fetches the rest where
// the next user stands: shade .xyz + type, shade .w again, flag, kind, colour -- five trips.  The
// empty asm keeps each group whole and where it is written.
// (gbuffer_store below repeats these two reads to keep the material index: a change here goes there too.)
__device__ __forceinline__ DevMaterial hit_surface_whole(const SceneView &S, DRay &ray, f3 I, f3 &N) {
    float4 s0 = S.shade[2 * ray.obj], s1 = S.shade[2 * ray.obj + 1];
    asm volatile("" : "+v"(s0.x), "+v"(s0.y), "+v"(s0.z), "+v"(s0.w), "+v"(s1.x), "+v"(s1.y), "+v"(s1.z), "+v"(s1.w));
    static_assert(sizeof(DevMaterial) == 64, "a material is four float4");
    const float4 *mp = reinterpret_cast<const float4 *>(S.mats + __float_as_int(s0.w));
    float4 q[4] = {mp[0], mp[1], mp[2], kExt ? mp[3] : make_float4(0, 0, 0, 0)};
    asm volatile("" : "+v"(q[0].x), "+v"(q[0].y), "+v"(q[0].z), "+v"(q[0].w), "+v"(q[1].x), "+v"(q[1].y), "+v"(q[1].z),
                      "+v"(q[1].w), "+v"(q[2].x), "+v"(q[2].y), "+v"(q[2].z), "+v"(q[2].w));
    if constexpr (kExt) asm volatile("" : "+v"(q[3].x), "+v"(q[3].y));
    DevMaterial m;
    __builtin_memcpy(&m, q, sizeof(m));
    N = prim_normal(S, s0, s1, I);
    if (dot(N, ray.D) > 0) N = -N;
    if (kExt && m.kind == RT_TEXTURE) finish_uv(S, ray);
    return m;
}

// ------------------------------------------------------------------ traversal (scene.h:285-320, 452-487)
// Where a traversal reads its nodes (the per-node layout in global memory, L1/L2-resident)
// and keeps its stack of node words (LDS lane column: entry i at stk[i * kStride], kStride =
// workgroup size, so consecutive lanes hit consecutive banks).  Round 4 removed the LDS-node
// layouts (the 64-B / 48-B interleaved child pairs of k_render_lds / k_render_lds48 and the
// lane kernel's LDS treelet): each measured slower than global nodes (docs/ROUND_LOG.md 4).
// COUNT (the dry-run work build, k_render_work): per-lane traversal counters in LDS at
// work[k * kStride] -- [0] closest-hit node visits (interior + leaf), [1] closest-hit primitive
// tests, [2] any-hit node visits, [3] any-hit primitive tests, [4] / [5] closest-hit pops of an
// interior / leaf entry whose box entry distance (kept beside the stack entry at its push, in
// `dist`) is >= the ray's t at the pop: the reference loads that interior node's child pair only
// to reject both children (each lies in its parent, so its entry is no nearer), so [4] is what
// an exact pop-time cull would skip; a leaf's primitives can still be hit by float rounding at a
// box face, so [5] cannot be skipped exactly.  Production builds carry none of it.
template <int STRIDE, bool COUNT = false>
struct Trav {
    static constexpr int kStride = STRIDE;
    static constexpr bool kCount = COUNT;
    const float4 *nodes;
    uint32_t *stk;
    const float4 *prims;     // leaf-order primitive slots
    uint32_t *work = nullptr;
    float *dist = nullptr;   // COUNT: entry distance of each stack entry (same layout as stk)
    __device__ __forceinline__ void add(int k, uint32_t n) const {
        if constexpr (COUNT) work[k * kStride] += n;
    }
    // closest hit only: the entry just pushed at slot sp - 1 / the entry just popped into slot sp
    __device__ __forceinline__ void pushed(int sp, float d) const {
        if constexpr (COUNT)
            if (dist) dist[(sp - 1) * kStride] = d;
    }
    __device__ __forceinline__ void popped(int sp, uint32_t w, float t) const {
        if constexpr (COUNT)
            if (dist && dist[sp * kStride] >= t) add((w & 0xffu) ? 5 : 4, 1);
    }
};

// both children of the interior node whose word has leftFirst = lf: slab interval ends and
// the children's words
// Uniform nodes: when every calling lane is at the same child pair (camera and shadow rays near
// the root, whole coherent tiles), the 64-B pair comes in with one scalar s_load_dwordx16 instead
// of four vector loads returning 64 lanes' copies of it: TEAPOT-F 1080p 0.1057 -> 0.1027 ms, mig29
// x16 0.502 -> 0.487 ms, CFG5-sub 9.44 -> 9.33 ms, CFG3-sub 2.40 -> 2.43 ms (profiles/r01/
// ab_uni_*.json).  Nodes are read-only after the upload.
typedef uint32_t u32x16 __attribute__((ext_vector_type(16)));
// a wave-uniform child pair (64 B at nodes + 2 lf) in one scalar load
__device__ __forceinline__ void pair_scalar(const float4 *nodes, uint32_t lf, float4 &a0, float4 &b0, float4 &a1,
                                            float4 &b1) {
    u32x16 v;
    asm volatile("s_load_dwordx16 %0, %1, 0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(nodes + 2 * lf) : "memory");
    a0 = make_float4(__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]), __uint_as_float(v[3]));
    b0 = make_float4(__uint_as_float(v[4]), __uint_as_float(v[5]), __uint_as_float(v[6]), __uint_as_float(v[7]));
    a1 = make_float4(__uint_as_float(v[8]), __uint_as_float(v[9]), __uint_as_float(v[10]), __uint_as_float(v[11]));
    b1 = make_float4(__uint_as_float(v[12]), __uint_as_float(v[13]), __uint_as_float(v[14]), __uint_as_float(v[15]));
}
// Uniform pairs compute their slabs in their own branch, on the scalar registers the pair arrived
// in: merged with the vector branch, the 16 loaded words were first copied into VGPRs (15 v_mov per
// uniform step; TEAPOT-F 1080p 0.0947 -> 0.0924 ms, profiles/r06/pairsplit).  The empty asm keeps
// the compiler from sinking both branches' slab code into their join.
template <bool FAST, class TR, bool UNI = true>
__device__ __forceinline__ void child_pair(const TR &T, const DRay &r, uint32_t lf, float &n1, float &x1, float &n2,
                                           float &x2, uint32_t &w1, uint32_t &w2) {
    // every calling lane at the same pair (coherent camera / shadow rays near the root):
    // one scalar load per wave instead of 64 lanes' worth of vector-memory returns
    const uint32_t lf0 = __builtin_amdgcn_readfirstlane(lf);
    float4 a0, b0, a1, b1;
    if constexpr (!UNI) {
        const float4 *q = T.nodes + 2 * lf;
        a0 = q[0]; b0 = q[1]; a1 = q[2]; b1 = q[3];
        slab<FAST>(r, a0, b0, n1, x1);
        slab<FAST>(r, a1, b1, n2, x2);
    } else if (__ballot(lf != lf0) == 0) {
        pair_scalar(T.nodes, lf0, a0, b0, a1, b1);
        slab<FAST>(r, a0, b0, n1, x1);
        slab<FAST>(r, a1, b1, n2, x2);
        asm volatile("; uniform pair" : "+v"(n1), "+v"(x1), "+v"(n2), "+v"(x2));
    } else {
        const float4 *q = T.nodes + 2 * lf;
        a0 = q[0]; b0 = q[1]; a1 = q[2]; b1 = q[3];
        slab<FAST>(r, a0, b0, n1, x1);
        slab<FAST>(r, a1, b1, n2, x2);
        asm volatile("; lane pair" : "+v"(n1), "+v"(x1), "+v"(n2), "+v"(x2));
    }
    w1 = __float_as_uint(b0.z); w2 = __float_as_uint(b1.z);
}
// push a child's word / pop the next node's word
template <class TR>
__device__ __forceinline__ void stack_push(const TR &T, int &sp, uint32_t w) {
    T.stk[sp++ * TR::kStride] = w;
}
template <class TR>
__device__ __forceinline__ uint32_t stack_pop(const TR &T, int &sp) {
    return T.stk[--sp * TR::kStride];
}

// Traversal loops are "while-while" (Aila & Laine 2009): a lane runs interior nodes until it
// reaches a leaf, then the leaf's primitives.  Each lane's visiting order is the reference's
// (the leaf is intersected before the next node is culled against r.t), only the schedule
// across the wave changes: leaf code runs when the lanes have gathered at leaves instead of
// on almost every iteration of an if/else loop.  TEAPOT-F 1080p 0.130 -> 0.121 ms, TEAPOT-F
// depth 10 1.45 -> 1.28 ms, CFG5-sub 11.2 -> 10.8 ms (profiles/r01/ab_ww_*.json).
template <bool FAST, class TR>
__device__ __forceinline__ void closest_hit_t(const SceneView &S, const TR &T, DRay &r) {
    uint32_t word = S.root_word;
    int sp = 0;
    for (;;) {
        while (!(word & 0xffu)) {
            const uint32_t lf = word >> 8;
            float n1, x1, n2, x2;
            uint32_t w1, w2;
            T.add(0, 1);
            child_pair<FAST>(T, r, lf, n1, x1, n2, x2, w1, w2);
            const float e1 = slab_accept(r, n1, x1), e2 = slab_accept(r, n2, x2);
            // nearer child first, as selects (the swap as a branch cost exec-mask moves)
            const bool sw = e1 > e2;
            const float d1 = sw ? e2 : e1, d2 = sw ? e1 : e2;
            const uint32_t wn = sw ? w2 : w1, wf = sw ? w1 : w2;
            w1 = wn; w2 = wf;
            if (d1 == 1e30f) {
                if (sp == 0) return;
                word = stack_pop(T, sp);
                T.popped(sp, word, r.t);
            } else {
                word = w1;
                if (d2 != 1e30f) {
                    stack_push(T, sp, w2);
                    T.pushed(sp, d2);
                }
            }
        }
        const uint32_t cnt = word & 0xffu, lf = word >> 8;
        T.add(0, 1);
        T.add(1, cnt);
        leaf_closest(S, T.prims, lf, cnt, r);
        if (sp == 0) return;
        word = stack_pop(T, sp);
        T.popped(sp, word, r.t);
    }
}

// Any hit: the answer is the OR over every leaf primitive reachable with the fixed r.t, so the
// child order is free (IsOccluded takes child 1 first, template/scene.h:452-487).  Shadow rays
// start on a surface and end at the light; the child whose box the ray enters later is taken
// first (the nearer one mostly holds the shading point's own neighbourhood, which cannot
// occlude past EPS): TEAPOT-F depth 10 1.28 -> 1.19 ms, mig29 x16 0.524 -> 0.501 ms
// (profiles/r01/ab_occ_div_*.json; nearer-first measured neutral).
template <bool FAST, class TR>
__device__ __forceinline__ bool occluded_t(const SceneView &S, const TR &T, const DRay &r) {
    uint32_t word = S.root_word;
    int sp = 0;
    for (;;) {
        while (!(word & 0xffu)) {
            const uint32_t lf = word >> 8;
            float n1, x1, n2, x2;
            uint32_t w1, w2;
            T.add(2, 1);
            child_pair<FAST>(T, r, lf, n1, x1, n2, x2, w1, w2);
            const bool h1 = x1 >= n1 && n1 < r.t && x1 > 0, h2 = x2 >= n2 && n2 < r.t && x2 > 0;
            if (h1 && h2) {                   // farther child first (see above)
                const bool sw = n2 > n1;
                word = sw ? w2 : w1;
                stack_push(T, sp, sw ? w1 : w2);
            }
            else if (!(h1 || h2)) { if (sp == 0) return false; word = stack_pop(T, sp); }
            else word = h1 ? w1 : w2;
        }
        const uint32_t cnt = word & 0xffu, lf = word >> 8;
        T.add(2, 1);
        if constexpr (TR::kCount) {
            for (uint32_t k = lf; k < lf + cnt; ++k) {
                T.add(3, 1);
                if (prim_hit(S, T.prims, k, r)) return true;
            }
        } else if (leaf_any(S, T.prims, lf, cnt, r)) {
            return true;
        }
        if (sp == 0) return false;
        word = stack_pop(T, sp);
    }
}

// ---- wave-coherent closest hit: the calling lanes walk the union of their subtrees with
// a wave-uniform node and stack (the stack lives in LDS past the lane stacks -- a VGPR lane-stack
// cannot be used because the caller may have lanes switched off).  Children are visited in the
// order most calling lanes prefer; a lane tests a leaf only if its slab test passed with its t at
// that moment.  Exactness (DESIGN 2.3): the result equals IntersectBVH's (template/scene.h:285-320)
// unless the lane is flagged -- `tie`: a second primitive met at exactly the lane's current t;
// `odd`: a hit nearer than its leaf box's computed entry -- and flagged lanes are re-traced in the
// reference order.  What the flags cannot see is a primitive this walk never tests: one in a box
// it culled because the box's entry lay past the lane's t.  If that primitive R is the reference's
// answer, its computed t_R is <= the lane's t at the cull (the walk's hits are the reference's
// candidates), so R's t lies before its culled ancestor's entry, hence before its own leaf's (every
// child box lies inside its parent's, `nested`, and a slab entry is monotone in the bound): a box
// is therefore culled only when its entry exceeds t * (1 + walk_margin) (2^-12, RT_WALK_MARGIN), so
// hiding R needs t_R more than the margin before its leaf's entry.  The rounding of a triangle's t
// grows as 1 / sin(smallest corner angle) (the common denominator of t, u and v, Primitive.h:255-273,
// is the triple product of two nearly parallel edges): sliver triangles report garbage t / u / v that
// the reference accepts (a mig29 sliver 2^-8.2 before its leaf's entry; a 2^-9 one 2^-15.4 before).
// Boxes holding a sliver triangle (sine under 2^-8, RT_WALK_STICKY), a sphere or a quad somewhere
// below them are marked "sticky" at rt_scene_create (node b.w = +inf instead of the margin): the walk
// culls them only on a slab miss, whatever the lane's t, so those primitives are never hidden and
// their early hits raise `odd`.
// For every other answer the exhaustive certificate (oracle or_walk_need over every camera ray of the
// bench's config-4 frames and the grazing cameras; tools/walk_certify.py) stays far below the margin.
// The wave's uniform stack of node words, in LDS past the lane stacks (the launch adds it when the
// walk may run: walk_bytes in rt_device.hip).  Every kernel that walks camera rays sets T.stk =
// (LDS base) + threadIdx.x with 256-thread workgroups.
// c ? a : b for wave-uniform c, a, b in scalar registers: written as a C select, the compiler
// turned the uniform condition into a lane mask and selected with v_cndmask + v_readfirstlane
__device__ __forceinline__ uint32_t sel_s(uint32_t c, uint32_t a, uint32_t b) {
    uint32_t r;
    asm("s_cmp_lg_u32 %1, 0\n\ts_cselect_b32 %0, %2, %3" : "=s"(r) : "s"(c), "s"(a), "s"(b) : "scc");
    return r;
}
__device__ __forceinline__ uint64_t sel_s64(uint32_t c, uint64_t a, uint64_t b) {
    uint64_t r;
    asm("s_cmp_lg_u32 %1, 0\n\ts_cselect_b64 %0, %2, %3" : "=s"(r) : "s"(c), "s"(a), "s"(b) : "scc");
    return r;
}
// 1 if the scalar word w is +inf's bit pattern, else 0
__device__ __forceinline__ uint32_t is_inf_s(uint32_t w) {
    uint32_t r;
    asm("s_cmp_eq_u32 %1, 0x7f800000\n\ts_cselect_b32 %0, 1, 0" : "=s"(r) : "s"(w) : "scc");
    return r;
}
// the walk's child order, m1 != 0 && (m2 == 0 || v1 >= v2), on scalar registers
__device__ __forceinline__ uint32_t first_child1(uint64_t m1, uint64_t m2, uint32_t v1, uint32_t v2) {
    uint32_t r;
    asm("s_cmp_ge_u32 %3, %4\n\ts_cselect_b32 %0, 1, 0\n\ts_cmp_eq_u64 %2, 0\n\ts_cselect_b32 %0, 1, %0\n\t"
        "s_cmp_lg_u64 %1, 0\n\ts_cselect_b32 %0, %0, 0"
        : "=&s"(r) : "s"(m1), "s"(m2), "s"(v1), "s"(v2) : "scc");
    return r;
}
template <class TR>
__device__ __forceinline__ uint32_t *walk_words(const SceneView &S, const TR &T) {
    uint32_t *base = T.stk - threadIdx.x;
    return base + (size_t)S.stack_entries * TR::kStride + (threadIdx.x >> 6) * S.stack_entries;
}
// A push keeps, beside the pushed node's word (wave-uniform, walk_words), each lane's own accepted
// entry distance of it in the lane's stack column (1e30 where the lane rejected it or was not in
// the parent).  A pop then decides from that distance and the lane's current t alone -- no reload
// of the node's box: re-testing the box gives the same answer, since the slab values are the same
// floats, t only decreases, and a lane that rejected an ancestor rejects the node too (`nested`).
// Round 5: one dependent node load less per pop.  The kept distance's lowest mantissa bit is the
// node's sticky mark (1: culled only on a miss): a lane-local bit, so the pop needs no uniform
// read before its test (a separate uniform mark cost 6 % of the walk).  A sticky entry's distance
// rises by at most one ulp, a plain one's falls by at most one: the odd check then flags slightly
// more, or misses a hit at most one ulp before its box's entry -- DESIGN 2.3 carries that ulp.
// Two-level records on this walk (one 128-B load per two levels, RT_WALK_QUADS in round 6,
// commit 92f864b) were bit-exact but measured slower on serial frames (mig29 x16 1080p 0.353 ->
// 0.382 ms, TEAPOT-F 0.117 -> 0.130) and 2 % faster with 4 frames in flight (0.2575 -> 0.2530;
// profiles/r06/quadwalk): the box unions and the second vote cost more issue than the saved
// scalar-cache round trip, so the walk stays binary.
// nmargin (wave-uniform): lanes x boxes entered only through the margin or a sticky mark (entry at
// or past the lane's t), counted in the BOXES build
template <bool BOXES, class TR>
__device__ __forceinline__ void wave_closest_hit_fast(const SceneView &S, const TR &T, DRay &r, bool &flag,
                                                      uint32_t &nmargin) {
    const float4 *nodes = S.nodes;                    // the per-node layout whatever TR reads
    uint32_t *ww = walk_words(S, T);                  // the wave's uniform stack (node words)
    uint32_t *wd = T.stk;                             // this lane's pushed entry distances (float bits)
    uint32_t word = __builtin_amdgcn_readfirstlane(S.root_word);
    const bool count_boxes = BOXES && S.walk_check >= RT_WALK_CHECK_COUNT;
    const float m = S.walk_margin;
    bool in = true;
    float tb = -1e30f;                                // my slab entry distance of the current node
    uint32_t sp = 0;
    for (;;) {
        const uint32_t cnt = word & 0xffu, lf = word >> 8;
        if (cnt) {
            if (in)
                for (uint32_t k = lf; k < lf + cnt; ++k) {
                    const float t0 = r.t;
                    prim_intersect_t<true>(S, T.prims, k, r, flag);   // the walk's records through the scalar cache
                    if (r.t != t0 && r.t < tb) flag = true;          // hit nearer than its box's entry
                }
        } else {
            float4 a0, b0, a1, b1;
            pair_scalar(nodes, lf, a0, b0, a1, b1);   // the pair is wave-uniform: one scalar load
            float n1, x1, n2, x2;
            slab<true>(r, a0, b0, n1, x1);
            slab<true>(r, a1, b1, n2, x2);
            // accept: a slab hit, and an entry below t (1 + the child's margin): b.w holds the walk's
            // cull margin per node, +inf for a sticky one (culled only on a miss; t > 0, so t * inf
            // is inf) -- the sticky rule costs no instruction in the step
            // (bitwise: evaluated without branches -- the short-circuit form cost exec-mask branches)
            const float d1 = (in & (x1 >= n1) & (x1 > 0) & (n1 < r.t + r.t * b0.w)) ? n1 : 1e30f;
            const float d2 = (in & (x2 >= n2) & (x2 > 0) & (n2 < r.t + r.t * b1.w)) ? n2 : 1e30f;
            const bool h1 = d1 != 1e30f, h2 = d2 != 1e30f;
            const uint64_t m1 = __ballot(h1), m2 = __ballot(h2);
            if (count_boxes)
                nmargin += (uint32_t)__popcll(__ballot(h1 && d1 >= r.t)) + (uint32_t)__popcll(__ballot(h2 && d2 >= r.t));
            if (m1 | m2) {
                // the vote, on lane masks: lanes preferring child 1 (v1) / child 2 (v2)
                const uint64_t lt21 = __ballot(d2 < d1), le12 = __ballot(d1 <= d2);
                const uint32_t v1 = (uint32_t)__popcll(m1 & ~(m2 & lt21));
                const uint32_t v2 = (uint32_t)__popcll(m2 & ~(m1 & le12));
                const uint32_t f1 = first_child1(m1, m2, v1, v2);   // child 1 first (wave-uniform 0 / 1)
                const bool first1 = __builtin_amdgcn_inverse_ballot_w64(sel_s64(f1, ~0ull, 0ull));
                if (m1 && m2) {
                    const float dp = first1 ? d2 : d1;
                    const uint32_t db = __float_as_uint(dp);
                    // the pushed child's word and margin word: scalar selects of the scalar-loaded pair
                    const uint32_t wfar = sel_s(f1, __float_as_uint(b1.z), __float_as_uint(b0.z));
                    const uint32_t mfar = sel_s(f1, __float_as_uint(b1.w), __float_as_uint(b0.w));
                    const uint32_t stp = is_inf_s(mfar);   // sticky (+inf margin): 1, else 0
                    wd[sp * TR::kStride] = dp == 1e30f ? db : ((db & ~1u) | stp);
                    ww[sp] = wfar;
                    ++sp;
                }
                word = sel_s(f1, __float_as_uint(b0.z), __float_as_uint(b1.z));
                in = __builtin_amdgcn_inverse_ballot_w64(sel_s64(f1, m1, m2));
                tb = first1 ? d1 : d2;
                continue;
            }
        }
        // pop, testing each entry's kept distance against the lanes' current t (sticky: only a miss)
        for (;;) {
            if (sp == 0) return;
            --sp;
            const uint32_t db = wd[sp * TR::kStride];
            const float d = __uint_as_float(db);
            tb = ((d != 1e30f) & (((db & 1u) != 0u) | (d < r.t + r.t * m))) ? d : 1e30f;   // the accept with today's t
            in = tb != 1e30f;
            if (count_boxes) nmargin += (uint32_t)__popcll(__ballot(in && tb >= r.t));
            if (__ballot(in)) {
                word = __builtin_amdgcn_readfirstlane(ww[sp]);
                break;
            }
        }
    }
}

template <class TR>
__device__ __forceinline__ void closest_hit(const SceneView &S, const TR &T, DRay &r) {
    if (__all(S.bounds_finite && ray_finite(r))) closest_hit_t<true>(S, T, r);
    else closest_hit_t<false>(S, T, r);
}
// camera rays: the wave-coherent walk where the scene asks for it (SceneView::wave_primary).
// Its counters go to the renderer's counter slot of this wave (SceneView::walk_stats): [2]
// boxes entered through the margin, [3] lanes re-traced for a tie / odd hit, [4] camera rays
// walked, [5] RT_WALK_CHECK_VERIFY lanes whose walk result differed from the reference order's
// (which is then the one kept) -- one atomic per counter and wave, from its first active lane.
// CHECK: the counters and the verify re-trace are compiled into the frame kernel's walk-check
// build only (k_render_walkcheck, chosen when the renderer's RT_WALK_CHECK level is COUNT or
// VERIFY): they keep 2-9 more VGPRs live, which cost the production frame kernel a wave per SIMD
// (71 -> 73 / 80 VGPRs, 7 -> 6 waves).
template <bool CHECK = false, class TR>
__device__ __forceinline__ void closest_hit_primary(const SceneView &S, const TR &T, DRay &r) {
    if (S.wave_primary && __all(S.bounds_finite && ray_finite(r))) {
        const DRay r0 = r;
        bool flag = false;
        uint32_t nmargin = 0;
        wave_closest_hit_fast<CHECK>(S, T, r, flag, nmargin);
        bool differs = false;
        if constexpr (CHECK) {
            const bool verify = S.walk_check >= RT_WALK_CHECK_VERIFY;
            if (flag || verify) {
                const DRay w = r;
                r = r0;
                closest_hit_t<true>(S, T, r);
                differs = !flag && (w.obj != r.obj || __float_as_uint(w.t) != __float_as_uint(r.t) ||
                                    __float_as_uint(w.u) != __float_as_uint(r.u) || __float_as_uint(w.v) != __float_as_uint(r.v));
            }
        } else if (flag) {
            r = r0;
            closest_hit_t<true>(S, T, r);
        }
        if (CHECK && S.walk_stats) {
            const uint64_t act = __ballot(true);
            const uint32_t nre = (uint32_t)__popcll(__ballot(flag)), ndiff = (uint32_t)__popcll(__ballot(differs));
            if (__lane_id() == (uint32_t)__ffsll((long long)act) - 1u) {
                const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
                unsigned long long *c = S.walk_stats + (size_t)(wave % kCounterSlots) * 8u;
                atomicAdd(&c[4], (unsigned long long)__popcll(act));
                if (nmargin) atomicAdd(&c[2], (unsigned long long)nmargin);
                if (nre) atomicAdd(&c[3], (unsigned long long)nre);
                if (ndiff) atomicAdd(&c[5], (unsigned long long)ndiff);
            }
        }
        return;
    }
    closest_hit(S, T, r);
}
template <class TR>
__device__ __forceinline__ bool occluded(const SceneView &S, const TR &T, const DRay &r) {
    if (__all(S.bounds_finite && ray_finite(r))) return occluded_t<true>(S, T, r);
    return occluded_t<false>(S, T, r);
}

// ------------------------------------------------------------------ packet traversal (scene.h:322-412)
// Scene::IntersectBVHPacket with the packet = the wave: lane l holds ray l of the 64-ray
// packet.  The node, the stack and the "first active" ray are wave-uniform (node and
// primitive loads are scalar, the stack lives in one VGPR: entry i in lane i); each lane
// tests its own ray and a ballot finds the lowest hitting lane.  Inactive lanes (past the
// end of the batch / off screen) never test and never lead.  The VGPR lane-stack needs all
// 64 lanes switched on: callers invoke it from wave-uniform control flow only.
__device__ __forceinline__ float readlane_f(float v, uint32_t l) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), (int)l));
}

template <bool FAST>
__device__ __forceinline__ void packet_closest_hit_t(const SceneView &S, DRay &r, bool active) {
    const uint32_t lane = __lane_id();
    uint32_t fa = 0, ni = 0, sp = 0;
    int stackv = 0;                                   // lane i: stack entry i (node index, depth < 64)
    for (;;) {
        ni = __builtin_amdgcn_readfirstlane(ni);
        const float4 a = S.nodes[2 * ni], b = S.nodes[2 * ni + 1];
        const uint32_t word = __float_as_uint(b.z), cnt = word & 0xffu, lf = word >> 8;
        const uint64_t m = __ballot(active && slab_hit<FAST>(r, a, b));
        uint32_t first = 0;                           // lanes >= first test a leaf
        bool visit = true;
        if (!((m >> fa) & 1u)) {
            if (m == 0) visit = false;
            else first = fa = (uint32_t)__ffsll((long long)m) - 1u;
        }
        if (visit && cnt == 0) {                      // interior: order by the leader's distances
            const float4 *q = S.nodes + 2 * lf;
            float d1 = readlane_f(slab_dist<FAST>(r, q[0], q[1]), fa);
            float d2 = readlane_f(slab_dist<FAST>(r, q[2], q[3]), fa);
            uint32_t c1 = lf, c2 = lf + 1;
            if (d1 > d2) { c1 = lf + 1; c2 = lf; }
            stackv = lane == sp ? (int)c2 : stackv;   // writelane
            ++sp;
            ni = c1;
            continue;
        }
        if (visit && active && lane >= first)
            for (uint32_t k = lf; k < lf + cnt; ++k) prim_intersect(S, S.prims, k, r);
        if (sp == 0) break;
        --sp;
        ni = (uint32_t)__builtin_amdgcn_readlane(stackv, (int)sp);
    }
}
__device__ __forceinline__ void packet_closest_hit(const SceneView &S, DRay &r, bool active) {
    if (__all(S.bounds_finite && (!active || ray_finite(r)))) packet_closest_hit_t<true>(S, r, active);
    else packet_closest_hit_t<false>(S, r, active);
}

// ------------------------------------------------------------------ shading
// TEX_SKY = false: every texel is equal (the synthetic sky), so the lookup's index is
// irrelevant and the colour is the precomputed texel -- bit-identical, no atan2/acos.
template <bool TEX_SKY>
__device__ __forceinline__ f3 sky_color(const SceneView &S, f3 D) {   // renderer.h:15-22
    if (!TEX_SKY) return mk(S.sky_rgb[0], S.sky_rgb[1], S.sky_rgb[2]);
    uint32_t u = f2u_wrap((float)S.sky_w * cr_atan2(D.z, D.x) * kINV2PI - 0.5f);
    uint32_t v = f2u_wrap((float)S.sky_h * cr_acos(D.y) * kINVPI - 0.5f);
    uint32_t p = S.sky[(u & (S.sky_w - 1)) + (v & (S.sky_h - 1)) * S.sky_w];
    return mk((float)((p >> 16) & 255), (float)((p >> 8) & 255), (float)(p & 255)) * kSKY;
}

// ObjectMaterial::DiffuseReflection + mapToNormalAxis (ObjectMaterial.h:18-53)
__device__ __forceinline__ f3 diffuse_dir(f3 N, uint32_t &seed) {
    float r0 = rnd_f(seed), r1 = rnd_f(seed);
    float r = sqrtf(r0), theta = kTWOPI * r1;
    float st, ct;
    sincos_f(theta, st, ct);
    float x = r * ct, y = r * st, z = sqrtf(1 - r0);
    f3 a0 = mk(0.0f, -1.0f, 0.0f), a1 = mk(-1.0f, 0.0f, 0.0f);
    if (N.z + 1.0f > kFLT_EPSILON) {
        float a = 1.0f / (1.0f + N.z);
        float b = -N.x * N.y * a;
        a0 = mk(1.0f - N.x * N.x * a, b, -N.x);
        a1 = mk(b, 1.0f - N.y * N.y * a, -N.y);
    }
    return normalize(x * a0 + y * a1 + z * N);
}

__device__ __forceinline__ float fresnel(float n1, float n2, float cost, float cosi) {   // ObjectMaterial.h:55-60
    float s = (n1 * cosi - n2 * cost) / (n1 * cosi + n2 * cost);
    float p = (n1 * cost - n2 * cosi) / (n1 * cost + n2 * cosi);
    return 0.5f * ((s * s) + (p * p));
}

// ObjectMaterial::scatter overrides.  With last = true the bounce ray is never traced
// (Trace(.., depth 0) returns 0), so only the RNG draws and the specular flag are kept.
__device__ __forceinline__ bool scatter(const DevMaterial &m, const DRay &in, f3 I, f3 N, DRay &out, uint32_t &seed,
                                        bool last) {
    switch (m.kind) {
    case RT_DIFFUSE:                                                   // Diffuse.h:16-19
        if (last) { rnd_u(seed); rnd_u(seed); }
        else out = make_ray(I, diffuse_dir(N, seed), 1e34f);
        return false;
    case RT_MIRROR:                                                    // Mirror.h:16-19
        if (!last) out = make_ray(I, normalize(reflect(in.D, N)), 1e34f);
        return true;
    case RT_DIELECTRIC: {                                              // Dielectric.h:23-54
        float n1 = 1, n2 = m.ior;
        float n12 = n1 / n2;
        float cosi = dot(N, in.D);
        if (in.inside) n12 = 1 / n12;
        float k = 1 - (n12 * n12) * (1 - (cosi * cosi));
        if (k < 0) {
            if (!last) { out = make_ray(I, normalize(reflect(in.D, N)), 1e34f); out.inside = 1; }
        } else {
            float Fr = 0;
            if (!in.inside) {
                float sini = length(cross(N, in.D));
                float sq = n12 * sini;
                float cost = sqrtf(1 - sq * sq);
                Fr = fresnel(n1, n2, cost, -cosi);
            }
            if (Fr > kFLT_EPSILON && rnd_f(seed) < Fr) {
                if (!last) out = make_ray(I, normalize(reflect(in.D, N)), 1e34f);
            } else if (!last) {
                f3 T = normalize(n12 * in.D - (n12 * cosi + sqrtf(k)) * N);
                out = make_ray(I, T, 1e34f);
                out.inside = !in.inside;
            }
        }
        return true;
    }
    case RT_LIGHT:
        return false;
    default:                                                           // Checkerboard.h:39-58
        if (m.diffuse < kFLT_EPSILON) {
            if (!last) out = make_ray(I, normalize(reflect(in.D, N)), 1e34f);
            return true;
        }
        if (m.specular < kFLT_EPSILON) {
            if (last) { rnd_u(seed); rnd_u(seed); }
            else out = make_ray(I, diffuse_dir(N, seed), 1e34f);
            return false;
        }
        if (rnd_f(seed) < m.specular) {
            if (!last) out = make_ray(I, normalize(reflect(in.D, N)), 1e34f);
            return true;
        }
        if (last) { rnd_u(seed); rnd_u(seed); }
        else out = make_ray(I, diffuse_dir(N, seed), 1e34f);
        return false;
    }
}

// TextureMaterial::GetColor (TextureMaterial.h:30-37); scale = 1/255 (correction) or
// SKYDOME_CORRECTION (getColorModifier) -- the same float
__device__ __forceinline__ f3 texture_color(const SceneView &S, const DevMaterial &m, const DRay &in) {
    const uint32_t u = f2u_wrap((float)m.tex_w * in.u), v = f2u_wrap((float)m.tex_h * in.v);
    const uint32_t p = S.tex[m.tex_off + (u & (m.tex_w - 1)) + (v & (m.tex_h - 1)) * m.tex_w];
    return mk((float)((p >> 16) & 255), (float)((p >> 8) & 255), (float)(p & 255)) * (1.0f / 255.0f);
}

__device__ __forceinline__ f3 mat_color(const SceneView &S, const DevMaterial &m, const DRay &in, f3 I) {
    if (kExt && m.kind == RT_TEXTURE) return texture_color(S, m, in);
    if (m.kind == RT_DIELECTRIC) {                                     // Dielectric.h:12-21
        f3 c = mk(1, 1, 1);
        if (in.inside) { c.x = exp_f(-m.c0[0] * in.t); c.y = exp_f(-m.c0[1] * in.t); c.z = exp_f(-m.c0[2] * in.t); }
        return c;
    }
    if (m.kind == RT_CHECKERBOARD) {                                   // Checkerboard.h:28-37
        bool ex = abs(((int)floorf(I.x)) % 2) == 0;
        bool ez = abs(((int)floorf(I.z)) % 2) == 0;
        return ex == ez ? mk(m.c0[0], m.c0[1], m.c0[2]) : mk(m.c1[0], m.c1[1], m.c1[2]);
    }
    return mk(m.c0[0], m.c0[1], m.c0[2]);
}

// Scene::GetLightPos = Primitive::GetRandomPoint of the light (Primitive.h:394-402, 423-427)
__device__ __forceinline__ f3 light_point(const SceneView &S, uint32_t &seed) {
    if (kExt && S.light_quad) {   // Primitive.h:423-427: the point lies in object z = 0 (reference quirk)
        const float a = S.light_qsize * (rnd_f(seed) - 1.0f);
        const float b = S.light_qsize * (rnd_f(seed) - 1.0f);
        return tpos(S.light_M, mk(a, b, 0.0f));
    }
    f3 pt = mk(1, 1, 1);
    while (dot(pt, pt) > 1) {
        float x = rnd_sym(seed);
        float y = rnd_sym(seed);
        float z = rnd_sym(seed);
        pt = mk(x, y, z);
    }
    return tpos(S.light_M, normalize(pt) * S.light_r);
}

// Renderer::NextEventDirectIllumination, renderer.h:44-75 (light = prim 0, a sphere)
// EARLY (the single-sample frame kernel): the light's area and, in the core build, its colour are
// requested before the shadow ray is traced, not inside its result's branch
template <class TR, bool EARLY = false>
__device__ __forceinline__ f3 nee(const SceneView &S, const TR &T, f3 I, f3 N, f3 BRDF, uint32_t &seed,
                                  uint32_t &nshadow) {
    f3 Il = light_point(S, seed);
    float area = S.light_area;                                         // GetArea, Primitive.h:450-468
    f3 lc0 = mk(0, 0, 0);
    if constexpr (EARLY) {
        if constexpr (!kExt) {
            const DevMaterial &lm = S.mats[S.light_mat];
            lc0 = mk(lm.c0[0], lm.c0[1], lm.c0[2]);
            asm volatile("" : "+v"(lc0.x), "+v"(lc0.y), "+v"(lc0.z));
        }
        asm volatile("" : "+v"(area));
    }
    f3 L = Il - I;
    float dist = length(L);
    L = L / dist;
    f3 Nl = (kExt && S.light_quad) ? mk(S.light_N[0], S.light_N[1], S.light_N[2])
                                   : (Il - mk(S.light_c[0], S.light_c[1], S.light_c[2])) * S.light_invr;
    if (dot(Nl, L) > 0) Nl = -Nl;                                      // Scene::GetNormal flip
    float dotNL = dot(N, L), dotNlL = dot(Nl, -L);
    f3 Ld = mk(0, 0, 0);
    frame_phase(3);
    if (dotNL > 0 && dotNlL > 0) {
        DRay sh = make_ray(I, L, dist - 2.0f * kEPS);
        ++nshadow;
        if (!occluded(S, T, sh)) {
            float solid = (dotNlL * area) / (dist * dist);
            float lightPDF = 1.0f / solid;
            const DevMaterial &lm = S.mats[S.light_mat];                // GetLightColor(0, toLight)
            // the core build only sees Light / Diffuse / Mirror / DSMix light materials (colour c0)
            const f3 lc = !kExt ? (EARLY ? lc0 : mk(lm.c0[0], lm.c0[1], lm.c0[2])) : mat_color(S, lm, sh, sh.O + sh.t * sh.D);
            Ld = (lc * BRDF) * (dotNL / lightPDF);
        }
    }
    frame_phase(4);
    return Ld;
}

// Renderer::Trace (renderer.cpp:17-72) as a loop.  The recursion's result
// BRDF * ((Trace * dot) / PDF) + Ld is folded innermost-first from per-level records,
// so the float evaluation order is the reference's.
// CAMWAVE: 0 camera rays take closest_hit, 1 closest_hit_primary (the wave walk where the scene
// asks for it), 2 the same with the walk checks compiled in (k_render_walkcheck)
// WHOLE: the hit's shade record and material are fetched whole (hit_surface_whole) and NEE's light
// fields early -- the single-sample frame kernel
template <int MAXD, bool TEX_SKY, class TR, int CAMWAVE = 0, bool WHOLE = false>
__device__ f3 trace_path(const SceneView &S, const TR &T, DRay ray, int depth, uint32_t &seed,
                         uint32_t &nshadow, uint32_t &nbounce, bool lastSpec = true) {
    f3 lv_mul[MAXD], lv_add[MAXD];
    float lv_c[MAXD];
    bool lv_diff[MAXD];
    int levels = 0;
    f3 term = mk(0, 0, 0);
    for (int d = depth; d > 0 && levels < MAXD; --d) {
        if (d != depth) ++nbounce;
        if constexpr (CAMWAVE) {
            if (d == depth) closest_hit_primary<CAMWAVE == 2>(S, T, ray);
            else closest_hit(S, T, ray);
        } else {
            closest_hit(S, T, ray);
        }
        frame_phase(2);
        if (ray.obj == -1) { term = sky_color<TEX_SKY>(S, ray.D); break; }
        f3 I = ray.O + ray.t * ray.D;
        f3 N;
        DevMaterial m_whole;
        if constexpr (WHOLE) m_whole = hit_surface_whole(S, ray, I, N);
        const DevMaterial &m = WHOLE ? m_whole : hit_surface(S, ray, I, N);
        if (m.flag == F_LIGHT) { term = lastSpec ? mk(m.c0[0], m.c0[1], m.c0[2]) : mk(0, 0, 0); break; }
        const bool last = MAXD == 1 || d == 1;   // MAXD 1: the bounce ray is never traced
        DRay out;
        bool spec = scatter(m, ray, I, N, out, seed, last);
        f3 albedo = mat_color(S, m, ray, I);
        if (m.flag == F_DIFFUSE || (m.flag == F_MIX && !spec)) {
            f3 BRDF = albedo * kINVPI;
            lv_add[levels] = nee<TR, WHOLE>(S, T, I, N, BRDF, seed, nshadow);
            lv_mul[levels] = BRDF;
            lv_c[levels] = last ? 0.0f : dot(N, out.D);
            lv_diff[levels] = true;
        } else {
            lv_mul[levels] = albedo;
            lv_add[levels] = mk(0, 0, 0);
            lv_c[levels] = 0.0f;
            lv_diff[levels] = false;
        }
        ++levels;
        if (last) break;
        ray = out;
        lastSpec = spec;
    }
    f3 r = term;
    for (int k = levels - 1; k >= 0; --k)
        r = lv_diff[k] ? lv_mul[k] * ((r * lv_c[k]) / kINV2PI) + lv_add[k] : lv_mul[k] * r;
    return r;
}

// Renderer::TracePacket's per-ray shading (renderer.cpp:78-133): the primary hit comes
// from the packet traversal, every bounce is a Trace(ray_out, specularBounce, depth).
template <int MAXD, bool TEX_SKY, class TR>
__device__ f3 shade_packet(const SceneView &S, const TR &T, DRay ray, int depth, uint32_t &seed,
                           uint32_t &nshadow, uint32_t &nbounce) {
    if (ray.obj == -1) return sky_color<TEX_SKY>(S, ray.D);
    f3 I = ray.O + ray.t * ray.D;
    f3 N;
    const DevMaterial &m = hit_surface(S, ray, I, N);
    const bool last = depth == 0;                  // Trace(.., 0) returns 0: the bounce is never traced
    DRay out;
    bool spec = scatter(m, ray, I, N, out, seed, last);
    f3 albedo = mat_color(S, m, ray, I);
    if (m.flag == F_LIGHT) return albedo;
    const bool diffuse = m.flag == F_DIFFUSE || m.flag == F_MIX;
    // MIX + specular bounce: the ray is traced for a result that is then overwritten
    // (renderer.cpp:111-114) and traced again after NEE (116-120).  One call site.
    const int passes = (m.flag == F_MIX && spec) ? 2 : 1;
    const f3 BRDF = albedo * kINVPI;
    f3 Ld = mk(0, 0, 0), Li = mk(0, 0, 0);
    for (int p = 0; p < passes; ++p) {
        if (diffuse && p == passes - 1) Ld = nee(S, T, I, N, BRDF, seed, nshadow);
        nbounce += last ? 0u : 1u;
        Li = trace_path<MAXD, TEX_SKY>(S, T, out, depth, seed, nshadow, nbounce, spec);
    }
    if (!diffuse) return albedo * Li;
    f3 Ei = (Li * (last ? 0.0f : dot(N, out.D))) / kINV2PI;
    return BRDF * Ei + Ld;
}

// ------------------------------------------------------------------ Whitted (the K key)
// ObjectMaterial::getColorModifier overrides: colour in c, colorVars[3] in c3 and the
// refraction direction colorVars[4..6] in T (Diffuse.h:21-23, Mirror.h:21-23,
// Light.h:20-22, Checkerboard.h:60-71, Dielectric.h:56-85).
__device__ __forceinline__ void color_modifier(const SceneView &S, const DevMaterial &m, const DRay &in, f3 I, f3 N, f3 &c, float &c3,
                                               f3 &T) {
    c3 = 0.0f;
    T = mk(0, 0, 0);
    switch (m.kind) {
    case RT_LIGHT:   // clamp = fmaxf(a, fminf(f, b)), template/precomp.h:782
        c = mk(fmaxf(0.0f, fminf(m.c0[0], 1.0f)), fmaxf(0.0f, fminf(m.c0[1], 1.0f)), fmaxf(0.0f, fminf(m.c0[2], 1.0f)));
        return;
    case RT_CHECKERBOARD:
    case RT_TEXTURE:                 // TextureMaterial.h:62-71 (kext only)
        c = mat_color(S, m, in, I);
        c3 = m.diffuse;
        return;
    case RT_DSMIX:                   // DSMix.h:48-50
        c = mk(m.c0[0], m.c0[1], m.c0[2]);
        c3 = m.diffuse;
        return;
    case RT_DIELECTRIC: {
        float n1 = 1, n2 = m.ior, n12 = n1 / n2;
        float cosi = dot(N, in.D);
        c = mk(1, 1, 1);
        if (in.inside) {
            c = mk(exp_f(-m.c0[0] * in.t), exp_f(-m.c0[1] * in.t), exp_f(-m.c0[2] * in.t));
            n12 = 1 / n12;
        }
        float k = 1 - (n12 * n12) * (1 - (cosi * cosi));
        if (k < 0) { c3 = -1.0f; return; }   // TIR
        if (!in.inside) {
            float sini = length(cross(N, in.D));
            float sq = n12 * sini;
            float cost = sqrtf(1 - sq * sq);
            c3 = fresnel(n1, n2, cost, -cosi);
        }
        T = normalize(n12 * in.D - (n12 * cosi + sqrtf(k)) * N);
        return;
    }
    default:
        c = mk(m.c0[0], m.c0[1], m.c0[2]);
        return;
    }
}

// Renderer::DirectIllumination, renderer.h:24-42: 4 light-sphere samples, spotlight test
// against GetLightDir (0,-1,0), GetLightColor (24,24,22) (template/scene.h:234-242).
template <class TR>
__device__ __forceinline__ f3 direct_illumination(const SceneView &S, const TR &T, f3 I, f3 N,
                                                  uint32_t &seed, uint32_t &nshadow) {
    f3 result = mk(0, 0, 0);
    const f3 ldir = mk(0.0f, -1.0f, 0.0f), lcol = mk(24.0f, 24.0f, 22.0f);
    for (int i = 0; i < 4; ++i) {
        f3 L = light_point(S, seed) - I;
        float dist = length(L);
        L = L / dist;
        float dotDN = dot(L, N);
        if (dotDN < 0 || dot(ldir, L) > 0) continue;
        DRay sh = make_ray(I, L, dist - (2 * kEPS));
        ++nshadow;
        if (occluded(S, T, sh)) continue;
        result = result + (dotDN / (dist * dist)) * lcol;
    }
    return result / 4.0f;
}

// Renderer::WhittedTrace (renderer.cpp:138-195) as a depth-first walk with an explicit
// frame stack.  A frame holds the parent's colour modifier and its partial sum; a child's
// value is added (scaled by Fr, Ft or 1 - diffuse) when it returns, and the dielectric's
// refraction child starts only after the reflection child is finished -- the reference's
// evaluation and RNG order, so results are bit-identical to the recursion.
constexpr int kWHITTED_MAX = 32;
struct WFrame {
    f3 col, res, I, T;
    float w, ft;
    int flags;   // 1: scale the child by w, 2: refraction child pending, 4: its inside flag
};

template <bool TEX_SKY, class TR>
__device__ f3 trace_whitted(const SceneView &S, const TR &T, DRay ray, int depth, uint32_t &seed,
                            uint32_t &nshadow, uint32_t &nbounce) {
    WFrame st[kWHITTED_MAX];
    int sp = 0;
    bool primary = true;
    for (;;) {
        // ---- evaluate WhittedTrace(ray, depth - sp) up to its first child
        f3 ret = mk(0, 0, 0);
        if (depth - sp > 0) {
            if (!primary) ++nbounce;
            primary = false;
            closest_hit(S, T, ray);
            if (ray.obj == -1) {
                ret = sky_color<TEX_SKY>(S, ray.D);
            } else {
                f3 I = ray.O + ray.t * ray.D;
                f3 N;
                const DevMaterial &m = hit_surface(S, ray, I, N);
                f3 col, Tdir;
                float c3;
                color_modifier(S, m, ray, I, N, col, c3, Tdir);
                f3 res = mk(0, 0, 0);
                WFrame f;
                f.col = col; f.w = 1.0f; f.ft = 0.0f; f.flags = 0;
                bool push = false, child_inside = false;
                f3 childD = mk(0, 0, 0);
                if (m.flag == F_LIGHT) {
                    res = res + mk(24.0f, 24.0f, 22.0f);
                } else if (m.flag == F_DIFFUSE) {
                    res = res + direct_illumination(S, T, I, N, seed, nshadow);
                } else if (m.flag == F_SPECULAR) {
                    push = true; childD = normalize(reflect(ray.D, N));
                } else if (m.flag == F_MIX) {
                    res = res + c3 * direct_illumination(S, T, I, N, seed, nshadow);
                    push = true; childD = normalize(reflect(ray.D, N));
                    f.w = 1.0f - c3; f.flags = 1;
                } else if (m.flag == F_DIELECTRIC) {
                    if (c3 < 0) {
                        push = true; childD = normalize(reflect(ray.D, N)); child_inside = true;
                    } else {
                        float Fr = c3, Ft = 1 - Fr;
                        if (Fr > kFLT_EPSILON) {
                            push = true; childD = normalize(reflect(ray.D, N));
                            f.w = Fr; f.flags = 1;
                            if (Ft > kFLT_EPSILON) {
                                f.flags |= 2 | (ray.inside ? 0 : 4);
                                f.ft = Ft; f.I = I; f.T = Tdir;
                            }
                        } else if (Ft > kFLT_EPSILON) {
                            push = true; childD = Tdir; child_inside = !ray.inside;
                            f.w = Ft; f.flags = 1;
                        }
                    }
                }
                if (push) {
                    f.res = res;
                    st[sp++] = f;
                    ray = make_ray(I, childD, 1e34f);
                    ray.inside = child_inside ? 1 : 0;
                    continue;
                }
                ret = col * res;
            }
        }
        // ---- return ret to the parents until one has a child left to trace
        bool descend = false;
        while (sp > 0) {
            WFrame &f = st[sp - 1];
            f.res = f.res + ((f.flags & 1) ? f.w * ret : ret);
            if (f.flags & 2) {
                ray = make_ray(f.I, f.T, 1e34f);
                ray.inside = (f.flags & 4) ? 1 : 0;
                f.w = f.ft;
                f.flags &= ~2;
                descend = true;
                break;
            }
            ret = f.col * f.res;
            --sp;
        }
        if (!descend) return ret;
    }
}

// Camera::GetPrimaryRay (camera.h:43-52) + randomInUnitDisk (20-26)
__device__ __forceinline__ DRay primary_ray(const FrameArgs &F, uint32_t x, uint32_t y, uint32_t &seed) {
    float u = (float)x * F.rw + rnd_f(seed) * F.rw;
    float v = (float)y * F.rh + rnd_f(seed) * F.rh;
    f3 p;
    for (;;) {
        float px = rnd_sym(seed);
        float py = rnd_sym(seed);
        p = mk(px, py, 0);
        if (!(dot(p, p) >= 1)) break;
    }
    f3 rd = F.lens * p;
    f3 offset = mk(u * rd.x, v * rd.y, 0);
    f3 pos = mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2]);
    f3 tl = mk(F.cam_tl[0], F.cam_tl[1], F.cam_tl[2]);
    f3 tr = mk(F.cam_tr[0], F.cam_tr[1], F.cam_tr[2]);
    f3 bl = mk(F.cam_bl[0], F.cam_bl[1], F.cam_bl[2]);
    f3 P = tl + u * (tr - tl) + v * (bl - tl);
    return make_ray(pos + offset, normalize(P - pos - offset), 1e34f);
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// RGBF32_to_RGB8, template/precomp.h:441-444
__device__ __forceinline__ uint32_t pack_rgb8(float4 a) {
    uint32_t r = f2u_wrap(255.0f * smin(1.0f, a.x));
    uint32_t g = f2u_wrap(255.0f * smin(1.0f, a.y));
    uint32_t b = f2u_wrap(255.0f * smin(1.0f, a.z));
    return (r << 16) + (g << 8) + b;
}

// ------------------------------------------------------------------ kernels
// global (row-major 8x8) tile of a shard's local tile: the explicit deal's map, or the
// interleaved deal t % nshards == shard
__device__ __forceinline__ uint32_t global_tile(const FrameArgs &F, uint32_t local_tile) {
    return F.tile_map ? F.tile_map[local_tile] : local_tile * F.nshards + F.shard;
}

// the wave's shadow / bounce ray counts into counter slot `wave` (kCounterSlots)
// BINARY: every lane's shadow count is 0 or 1 and no lane bounces (one sample at Trace depth 1), so
// the wave's count is a ballot's popcount instead of wave_sum's six dependent LDS round trips
template <bool BINARY = false>
__device__ __forceinline__ void count_rays(const FrameArgs &F, uint32_t wave, uint32_t lane, uint32_t nshadow,
                                           uint32_t nbounce) {
    if constexpr (BINARY) {
        nshadow = (uint32_t)__popcll(__ballot(nshadow != 0u));
        nbounce = 0u;
    } else {
        nshadow = wave_sum(nshadow);
        nbounce = wave_sum(nbounce);
    }
    if (lane == 0) {
        unsigned long long *c = F.counters + (size_t)(wave % kCounterSlots) * 8u;
        if (nshadow) atomicAdd(&c[0], (unsigned long long)nshadow);
        if (nbounce) atomicAdd(&c[1], (unsigned long long)nbounce);
    }
}

// One screen tile (8x8, one wave) of one frame: per pixel spp x Trace / WhittedTrace /
// TracePacket (the tile is the packet, renderer.cpp:247-285), running average into the
// accumulator (renderer.cpp:235-241), RGB8 pack; per-wave ray counters.
enum : int { M_PATH = RT_MODE_PATH, M_WHITTED = RT_MODE_WHITTED, M_PACKET = RT_MODE_PACKET };

//
// Work unit = (local tile, sample chunk): with F.nchunks > 1 (sample split, PATH / WHITTED
// frames whose tile count alone would not fill the GPU with enough rounds of waves, e.g.
// a 1/8 screen shard at spp 8) the unit traces its chunk of the pixel's samples and stores
// each sample's value in F.samples; k_pt_finish then sums them in sample order.  Overlapped
// primary+shadow frames (launch_render) store their samples the same way with one chunk.
// ONE: every unit traces one sample (spp 1, or a sample split into single-sample chunks): no
// sample loop and no running sum across the traversal.  F must then be the record in place in the
// kernel-argument segment (k_render_w8): the early accumulator read addresses it as constant memory.
// DRY: the dry-run work frame (k_render_work) -- the same rays, nothing written (no accumulator,
// frame, samples, ray counters or cycle costs)
template <int MODE, int MAXD, bool TEX_SKY, class TR, bool WALKCHECK = false, bool ONE = false, bool DRY = false>
__device__ __forceinline__ void render_tile(const SceneView &S, const FrameArgs &F, const TR &T,
                                            uint32_t unit, uint32_t lane) {
    // tile-major units: a workgroup's waves take the chunks of the same tiles (coherent rays,
    // shared cache lines); sample-major was 40 % slower on a 1/8 shard at spp 8
    frame_phase(0);
    const uint32_t slot = F.nchunks <= 1 ? unit : unit / F.nchunks;
    const uint32_t entry = F.order ? F.order[slot] : slot;       // measured-cost dispatch order
    const uint32_t local_tile = entry & 0x0fffffffu;
    const bool part_tile = (entry >> 31) != 0u;                     // one part of the tile only: lanes
                                                                     // [part << part_shift, +1 << part_shift)
    const uint32_t chunk = F.nchunks <= 1 ? 0u : unit % F.nchunks;
    const uint64_t t_start = F.tile_cost ? __builtin_amdgcn_s_memtime() : 0;
    const uint32_t s_begin = chunk * F.spp / F.nchunks, s_end = (chunk + 1u) * F.spp / F.nchunks;
    const uint32_t tile = global_tile(F, local_tile);
    const uint32_t x = (tile % F.tiles_x) * 8u + (lane & 7u), y = (tile / F.tiles_x) * 8u + (lane >> 3);
    const bool on = x < F.W && y < F.H && (!part_tile || (lane >> F.part_shift) == ((entry >> 28) & 7u));
    const uint32_t px = x + y * F.W;
    // The single-sample build requests the pixel's accumulator here, before the rays, and consumes
    // it in the epilogue: the frame's one long read (Infinity Cache or HBM) returns under the
    // traversals instead of standing alone at the wave's end.  Only lanes that will write the pixel
    // read it (on: inside the image and inside the entry's part), and only on frames that accumulate
    // here (no reset, no stored samples).  Such a kernel runs on the caller's stream behind every
    // earlier write of the accumulator (launch_render: frames on the renderer's streams store
    // samples, and k_pt_finish accumulates them on the caller's stream).
    // The three fields are read through an address the compiler cannot match with F's: merged with
    // the epilogue's reads they would hold four scalar registers across both traversals, which the
    // kernel does not have at 8 waves (4 v_writelane / 6 v_readlane).
    constexpr bool kEarlyAcc = ONE && !DRY;
    float4 acc_in = make_float4(0, 0, 0, 0);
    if constexpr (kEarlyAcc) {
        uintptr_t fa = (uintptr_t)&F;
        asm volatile("" : "+s"(fa));
        const auto *Fh = (const __attribute__((address_space(4))) FrameArgs *)fa;
        const uint32_t reset = Fh->reset;
        const float4 *const samples = Fh->samples, *const acc = Fh->acc;
        if (on & (reset == 0u) & (samples == nullptr)) {
            typedef float f32x4 __attribute__((ext_vector_type(4)));
            const f32x4 v = *(const __attribute__((address_space(1))) f32x4 *)(uintptr_t)(acc + px);
            acc_in = make_float4(v.x, v.y, v.z, v.w);
        }
    }
    // the wave-coherent camera-ray walk is compiled into the global-node primary+shadow
    // kernel only (SceneView::wave_primary picks it at run time)
    constexpr int kCamWave = (MODE == M_PATH && MAXD == 1 && TR::kStride == 256) ? (WALKCHECK ? 2 : 1) : 0;
    uint32_t nshadow = 0, nbounce = 0;
    f3 sum = mk(0, 0, 0);
    if (MODE == M_PACKET) {                           // the traversal is wave-wide: no early exit
        for (uint32_t s = 0; s < F.spp; ++s) {
            uint32_t seed = init_seed(px + F.W * F.H * (s + F.spp * F.frame));
            DRay ray = on ? primary_ray(F, x, y, seed) : make_ray(mk(0, 0, 0), mk(0, 0, 1), 1e34f);
            packet_closest_hit(S, ray, on);
            if (on) sum = sum + shade_packet<MAXD, TEX_SKY>(S, T, ray, (int)F.depth, seed, nshadow, nbounce);
        }
    } else if (ONE && on) {
        uint32_t seed = init_seed(px + F.W * F.H * (s_begin + F.spp * F.frame));
        DRay ray = primary_ray(F, x, y, seed);
        frame_phase(1);
        sum = trace_path<MAXD, TEX_SKY, TR, kCamWave, true>(S, T, ray, (int)F.depth, seed, nshadow, nbounce);
        if (F.samples) {
            F.samples[((size_t)s_begin * F.ntiles_local + local_tile) * 64u + lane] = make_float4(sum.x, sum.y, sum.z, 0.0f);
        }
    } else if (on) {
        for (uint32_t s = s_begin; s < s_end; ++s) {
            uint32_t seed = init_seed(px + F.W * F.H * (s + F.spp * F.frame));
            DRay ray = primary_ray(F, x, y, seed);
            f3 v;
            if constexpr (MODE == M_WHITTED) v = trace_whitted<TEX_SKY>(S, T, ray, (int)F.depth, seed, nshadow, nbounce);
            else v = trace_path<MAXD, TEX_SKY, TR, kCamWave>(S, T, ray, (int)F.depth, seed, nshadow, nbounce);
            if (F.samples) F.samples[((size_t)s * F.ntiles_local + local_tile) * 64u + lane] = make_float4(v.x, v.y, v.z, 0.0f);
            else sum = sum + v;
        }
    }
    if constexpr (DRY) return;
    if (on && !F.samples) {
        f3 res = (1.0f / (float)F.spp) * sum;
        float4 a;
        if constexpr (kEarlyAcc) a = acc_in;
        else a = F.reset ? make_float4(0, 0, 0, 0) : F.acc[px];
        a.w += 1;                                                      // renderer.cpp:237-240
        const float w = a.w, inv = 1.0f / w;
        a = make_float4(a.x + inv * (res.x - a.x), a.y + inv * (res.y - a.y), a.z + inv * (res.z - a.z),
                        a.w + inv * (w - a.w));
        F.acc[px] = a;
        const uint32_t rgb = pack_rgb8(a);
        if (F.packed_out) F.out[local_tile * 64u + lane] = rgb;
        else {
            if (F.fwd_dst) F.fwd_dst[px] = F.fwd_src[px];
            F.out[px] = rgb;
        }
    }
    count_rays<MODE == M_PATH && MAXD == 1 && ONE>(F, unit, lane, nshadow, nbounce);
    if (F.tile_cost && lane == 0) F.tile_cost[local_tile] = (uint32_t)(__builtin_amdgcn_s_memtime() - t_start);
    frame_phase(5);
}

// Global-node variant: 256-thread workgroups, wave w of workgroup b owns local tile b*4+w.
#ifndef RT_RENDER_WAVES_PER_SIMD
#define RT_RENDER_WAVES_PER_SIMD 1
#endif
template <int MODE, int MAXD, bool TEX_SKY>
__global__ __launch_bounds__(256, RT_RENDER_WAVES_PER_SIMD) void k_render(SceneView S, FrameArgs F) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t tid = threadIdx.x;
    const uint32_t unit = blockIdx.x * 4u + (tid >> 6);
    if (unit >= F.nunits) return;
    Trav<256> T{S.nodes, lds_stack + tid, S.prims};
    render_tile<MODE, MAXD, TEX_SKY>(S, F, T, unit, tid & 63u);
}
// The primary+shadow frame for work units of one sample (spp 1, or a sample split into single-
// sample chunks): render_tile without the sample loop and its running sum, which the plain build
// carries across the traversal -- 51 VGPRs instead of 71, no spill, so 8 waves/SIMD where the LDS
// stacks allow (TEAPOT-F 1080p serial 0.1025 -> 0.096 ms).  Round 4; frame_variant picks it.
// The two argument records (about 110 dwords) are read where they are used, from the kernel-
// argument segment: named as parameters they are all loaded at entry, more scalars than the
// kernel has registers for, and the compiler parked them in the lanes of a VGPR (42 v_writelane /
// 70 v_readlane, which issue as VALU).  Read in place, the traversal's fields are loaded before
// its loops and the shading / epilogue fields after them.
struct FrameKernArgs { SceneView S; FrameArgs F; };   // the segment's layout of (SceneView, FrameArgs)
template <bool TEX_SKY>
__global__ __launch_bounds__(256, 8) void k_render_w8(SceneView, FrameArgs) {
    const auto *ka = (const FrameKernArgs *)__builtin_amdgcn_kernarg_segment_ptr();
    const SceneView &S = ka->S;
    const FrameArgs &F = ka->F;
    extern __shared__ uint32_t lds_stack[];
    const uint32_t tid = threadIdx.x;
    const uint32_t unit = blockIdx.x * 4u + (tid >> 6);
    if (unit >= F.nunits) return;
    Trav<256> T{S.nodes, lds_stack + tid, S.prims};
    render_tile<M_PATH, 1, TEX_SKY, Trav<256>, false, true>(S, F, T, unit, tid & 63u);
}
// The primary+shadow frame with the camera walk's checks compiled in (RT_WALK_CHECK_COUNT:
// walked rays, re-traced lanes, margin boxes; _VERIFY: every walked lane re-traced and compared);
// same frames.
template <bool TEX_SKY>
__global__ __launch_bounds__(256, RT_RENDER_WAVES_PER_SIMD) void k_render_walkcheck(SceneView S, FrameArgs F) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t tid = threadIdx.x;
    const uint32_t unit = blockIdx.x * 4u + (tid >> 6);
    if (unit >= F.nunits) return;
    Trav<256> T{S.nodes, lds_stack + tid, S.prims};
    render_tile<M_PATH, 1, TEX_SKY, Trav<256>, true>(S, F, T, unit, tid & 63u);
}

// Dry-run work frame (rt_renderer_tile_work; the multi-GPU deals' cost input): the frame's rays
// traced as render_tile traces them -- same seeds, the reference-order lane walk for camera rays
// (the caller clears SceneView::wave_primary) -- with the counting traversal, writing nothing but
// the counts: per tile the sum over its lanes and samples of node visits + primitive tests
// (deterministic, unlike wave cycles: two runs of the same frame give the same deal), and with
// pixel_work the per-lane counters of every pixel (Trav COUNT's [0..5] at [8 * px + k], [6], [7]
// zero; summed over its samples).  Work units are whole tiles (F.nchunks == 1, no order); LDS
// holds the stack, then the stack entries' distances, then the 8 counters.
template <int MAXD, bool TEX_SKY>
__global__ __launch_bounds__(256) void k_render_work(SceneView S, FrameArgs F, uint32_t *__restrict__ tile_work,
                                                     uint32_t *__restrict__ pixel_work, int with_dist) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t unit = blockIdx.x * 4u + (tid >> 6);
    if (unit >= F.nunits) return;
    float *dist = with_dist ? reinterpret_cast<float *>(lds_stack + (size_t)S.stack_entries * 256u) + tid : nullptr;
    uint32_t *work = lds_stack + (size_t)S.stack_entries * (with_dist ? 512u : 256u) + tid;
    for (int k = 0; k < 8; ++k) work[k * 256] = 0u;
    Trav<256, true> T{S.nodes, lds_stack + tid, S.prims, work, dist};
    render_tile<M_PATH, MAXD, TEX_SKY, Trav<256, true>, false, false, true>(S, F, T, unit, lane);
    const uint32_t c0 = work[0], c1 = work[256], c2 = work[512], c3 = work[768];
    const uint32_t tot = wave_sum(c0 + c1 + c2 + c3);
    if (lane == 0) atomicAdd(&tile_work[unit], tot);
    if (pixel_work) {
        const uint32_t tile = global_tile(F, unit);
        const uint32_t x = (tile % F.tiles_x) * 8u + (lane & 7u), y = (tile / F.tiles_x) * 8u + (lane >> 3);
        if (x < F.W && y < F.H) {
            uint4 *q = reinterpret_cast<uint4 *>(pixel_work) + 2u * (x + (size_t)y * F.W);
            q[0] = make_uint4(c0, c1, c2, c3);
            q[1] = make_uint4(work[1024], work[1280], 0u, 0u);
        }
    }
}

__global__ __launch_bounds__(256) void k_intersect(SceneView S, const rt_ray *__restrict__ rays, rt_hit *__restrict__ hits,
                                                   uint32_t n) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    rt_ray q = rays[i];
    DRay r = make_ray(mk(q.ox, q.oy, q.oz), mk(q.dx, q.dy, q.dz), q.tmax);
    Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
    closest_hit(S, T, r);
    finish_uv(S, r);
    rt_hit h;
    h.t = r.t; h.obj = r.obj; h.u = r.u; h.v = r.v;
    hits[i] = h;
}

// batched Scene::IntersectBVHPacket: wave w traces rays [64w, 64w + 64) as one packet
__global__ __launch_bounds__(256) void k_intersect_packet(SceneView S, const rt_ray *__restrict__ rays,
                                                          rt_hit *__restrict__ hits, uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if ((i & ~63u) >= n) return;                      // whole waves only
    const bool active = i < n;
    DRay r = make_ray(mk(0, 0, 0), mk(0, 0, 1), 1e34f);
    if (active) {
        rt_ray q = rays[i];
        r = make_ray(mk(q.ox, q.oy, q.oz), mk(q.dx, q.dy, q.dz), q.tmax);
    }
    packet_closest_hit(S, r, active);
    if (!active) return;
    finish_uv(S, r);
    rt_hit h;
    h.t = r.t; h.obj = r.obj; h.u = r.u; h.v = r.v;
    hits[i] = h;
}

__global__ __launch_bounds__(256) void k_occluded(SceneView S, const rt_ray *__restrict__ rays, uint8_t *__restrict__ out,
                                                  uint32_t n) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    rt_ray q = rays[i];
    DRay r = make_ray(mk(q.ox, q.oy, q.oz), mk(q.dx, q.dy, q.dz), q.tmax);
    Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
    out[i] = occluded(S, T, r) ? 1 : 0;
}

// ------------------------------------------------------------------ first-hit G-buffer
// The camera ray of one sample of one pixel of a frame, traced to its first hit and no further
// (rt_render_gbuffer, rt_gbuffer_pixels): primary_ray from the frame's own seed, the closest hit,
// finish_uv, then the surface -- Scene::GetNormal flipped against the ray and the material's
// GetColor(ray) -- or skyColor(D).  A query: it touches nothing of F's accumulator, output, samples,
// counters or costs, and S.walk_stats stays unread (closest_hit_primary<false> compiles no counter).
// Which planes are stored is wave-uniform: branches on the kernel-argument pointers.  The surface costs
// the two dependent trips of hit_surface_whole -- the shade record as two whole float4, whose .w is the
// material id the normal plane reports, then the material as a whole record -- and is skipped
// entirely when neither the normal nor the albedo plane is asked for.  Each 16-B record plane takes one
// store per lane, so a tile row of 8 lanes fills one 128-B segment; the 28-B rt_ray goes out as dwords.
template <bool TEX_SKY>
__device__ __forceinline__ void gbuffer_store(const SceneView &S, const GBufferArgs &G, DRay &r, size_t i) {
    finish_uv(S, r);
    if (G.hit) {
        rt_hit h;
        h.t = r.t; h.obj = r.obj; h.u = r.u; h.v = r.v;
        G.hit[i] = h;
    }
    if (!G.normal && !G.albedo) return;
    rt_gnormal n;
    rt_galbedo a;
    if (r.obj < 0) {
        const f3 c = sky_color<TEX_SKY>(S, r.D);
        n.nx = 0.0f; n.ny = 0.0f; n.nz = 0.0f; n.material = -1;
        a.r = c.x; a.g = c.y; a.b = c.z; a.kind = -1;
    } else {
        const f3 I = r.O + r.t * r.D;
        // A copy of hit_surface_whole's two reads, pins included, made because that function does not hand
        // out the material index (s0.w) and no shared function may change here: it must follow every change
        // of hit_surface_whole, until that one returns the index and this calls it.
        float4 s0 = S.shade[2 * r.obj], s1 = S.shade[2 * r.obj + 1];
        asm volatile("" : "+v"(s0.x), "+v"(s0.y), "+v"(s0.z), "+v"(s0.w), "+v"(s1.x), "+v"(s1.y), "+v"(s1.z), "+v"(s1.w));
        const int mi = __float_as_int(s0.w);
        const float4 *mp = reinterpret_cast<const float4 *>(S.mats + mi);
        float4 q[4] = {mp[0], mp[1], mp[2], kExt ? mp[3] : make_float4(0, 0, 0, 0)};
        asm volatile("" : "+v"(q[0].x), "+v"(q[0].y), "+v"(q[0].z), "+v"(q[0].w), "+v"(q[1].x), "+v"(q[1].y), "+v"(q[1].z),
                          "+v"(q[1].w), "+v"(q[2].x), "+v"(q[2].y), "+v"(q[2].z), "+v"(q[2].w));
        if constexpr (kExt) asm volatile("" : "+v"(q[3].x), "+v"(q[3].y));
        DevMaterial m;
        __builtin_memcpy(&m, q, sizeof(m));
        f3 N = prim_normal(S, s0, s1, I);              // template/scene.h:489-497
        if (dot(N, r.D) > 0) N = -N;
        const f3 c = mat_color(S, m, r, I);            // (the hit's u, v are final: finish_uv above)
        n.nx = N.x; n.ny = N.y; n.nz = N.z; n.material = mi;
        a.r = c.x; a.g = c.y; a.b = c.z; a.kind = m.kind;
    }
    if (G.normal) G.normal[i] = n;
    if (G.albedo) G.albedo[i] = a;
}
__device__ __forceinline__ void gbuffer_store_ray(const GBufferArgs &G, const DRay &r, size_t i) {
    if (!G.ray) return;
    float *q = reinterpret_cast<float *>(G.ray + i);
    q[0] = r.O.x; q[1] = r.O.y; q[2] = r.O.z; q[3] = r.D.x; q[4] = r.D.y; q[5] = r.D.z; q[6] = r.t;
}

// k_render_heat's launch shape over the frame's own tile grid -- one wave per 8x8 tile, so a wave holds
// the 64 pixels the frame's wave holds and the wave walk sees the frame's coherence -- for the
// G.ntiles tiles the rectangle touches (G.ntx columns from tile (G.tx0, G.ty0)).  Lanes outside the
// rectangle (which lies inside the image) take no part in the traversal, as off-image lanes in
// render_tile.  Camera walk: S.wave_primary, set per launch by the host (gbuffer_wave_walk); the
// extension build has the lane walk only, as its frames do.
template <bool TEX_SKY>
__global__ __launch_bounds__(256) void k_gbuffer(SceneView S, FrameArgs F, GBufferArgs G) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t k = blockIdx.x * 4u + (tid >> 6);
    if (k >= G.ntiles) return;
    Trav<256> T{S.nodes, lds_stack + tid, S.prims};
    const uint32_t x = (G.tx0 + k % G.ntx) * 8u + (lane & 7u), y = (G.ty0 + k / G.ntx) * 8u + (lane >> 3);
    if (!(x >= G.x0 && x - G.x0 < G.w && y >= G.y0 && y - G.y0 < G.h)) return;
    const uint32_t px = x + y * F.W;
    const size_t i = (size_t)(y - G.y0) * G.w + (x - G.x0);
    uint32_t seed = init_seed(px + F.W * F.H * (G.sample + F.spp * F.frame));
    DRay r = primary_ray(F, x, y, seed);
    gbuffer_store_ray(G, r, i);
    if constexpr (kExt) closest_hit(S, T, r);
    else closest_hit_primary(S, T, r);
    gbuffer_store<TEX_SKY>(S, G, r, i);
}

// one lane per listed pixel, as k_intersect is laid out: the lane walk (a list's lanes are no tile).
// An index outside the frame (the device form's list is read here only) writes nothing.
template <bool TEX_SKY>
__global__ __launch_bounds__(256) void k_gbuffer_pixels(SceneView S, FrameArgs F, GBufferArgs G) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= G.n) return;
    const uint32_t px = G.pixels[i];
    if (px >= F.W * F.H) return;
    Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
    uint32_t seed = init_seed(px + F.W * F.H * (G.sample + F.spp * F.frame));
    DRay r = primary_ray(F, px % F.W, px / F.W, seed);
    gbuffer_store_ray(G, r, i);
    closest_hit(S, T, r);
    gbuffer_store<TEX_SKY>(S, G, r, i);
}

#if RT_EXT == 0
// ------------------------------------------------------------------ BVH analysis (scene.h:244-283)
// Scene::BVHVisualization: the walk of closest_hit_t with leaf_closest taken out, so r.t never
// shrinks -- nearer child first, the farther one pushed when its distance is not 1e30f; the root's
// own box is never tested.  visits counts every node met (interior or leaf), leaves the leaves; both
// live in registers.  It reads nodes only (no primitive, shading or material record), which is why
// it is compiled into the core build alone: the host launches that build for every scene (the node
// array, root word and stack depth mean the same to both builds).  The stack needs what
// closest_hit_t's needs: an entry per interior ancestor.
template <bool FAST, class TR>
__device__ __forceinline__ void heat_walk_t(const SceneView &S, const TR &T, const DRay &r, uint32_t &visits,
                                            uint32_t &leaves) {
    uint32_t word = S.root_word;
    int sp = 0;
    for (;;) {
        ++visits;
        if (word & 0xffu) {
            ++leaves;
            if (sp == 0) return;
            word = stack_pop(T, sp);
            continue;
        }
        float n1, x1, n2, x2;
        uint32_t w1, w2;
        child_pair<FAST>(T, r, word >> 8, n1, x1, n2, x2, w1, w2);
        const float e1 = slab_accept(r, n1, x1), e2 = slab_accept(r, n2, x2);
        const bool sw = e1 > e2;
        const float d1 = sw ? e2 : e1, d2 = sw ? e1 : e2;
        if (d1 == 1e30f) {
            if (sp == 0) return;
            word = stack_pop(T, sp);
        } else {
            word = sw ? w2 : w1;
            if (d2 != 1e30f) stack_push(T, sp, sw ? w1 : w2);
        }
    }
}
template <class TR>
__device__ __forceinline__ void heat_walk(const SceneView &S, const TR &T, const DRay &r, uint32_t &visits,
                                          uint32_t &leaves) {
    if (__all(S.bounds_finite && ray_finite(r))) heat_walk_t<true>(S, T, r, visits, leaves);
    else heat_walk_t<false>(S, T, r, visits, leaves);
}

// The RT_MODE_BVH_HEAT frame (the BVH_ANALYSIS build of Tick, renderer.cpp:224-226): k_render's launch
// shape -- one wave per 8x8 tile, the tiles in their plain order (no measured order, no sample split,
// no stored samples) -- with BVHVisualization's colour as the sample's value, then render_tile's
// accumulate / pack / store.  F.depth holds the TREE's depth (bvhDepth), not a Trace depth.
__global__ __launch_bounds__(256) void k_render_heat(SceneView S, FrameArgs F) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t local_tile = blockIdx.x * 4u + (tid >> 6);
    if (local_tile >= F.ntiles_local) return;
    Trav<256> T{S.nodes, lds_stack + tid, S.prims};
    const uint32_t tile = global_tile(F, local_tile);
    const uint32_t x = (tile % F.tiles_x) * 8u + (lane & 7u), y = (tile / F.tiles_x) * 8u + (lane >> 3);
    if (!(x < F.W && y < F.H)) return;
    const uint32_t px = x + y * F.W;
    const float depth = (float)F.depth;
    f3 sum = mk(0, 0, 0);
    for (uint32_t s = 0; s < F.spp; ++s) {
        uint32_t seed = init_seed(px + F.W * F.H * (s + F.spp * F.frame));
        const DRay ray = primary_ray(F, x, y, seed);
        uint32_t visits = 0, leaves = 0;
        heat_walk(S, T, ray, visits, leaves);
        sum = sum + mk((float)leaves / depth, (0.25f * (float)visits) / depth, 0.0f);   // scene.h:282
    }
    f3 res = (1.0f / (float)F.spp) * sum;
    float4 a = F.reset ? make_float4(0, 0, 0, 0) : F.acc[px];
    a.w += 1;                                                          // renderer.cpp:237-240
    const float w = a.w, inv = 1.0f / w;
    a = make_float4(a.x + inv * (res.x - a.x), a.y + inv * (res.y - a.y), a.z + inv * (res.z - a.z),
                    a.w + inv * (w - a.w));
    F.acc[px] = a;
    const uint32_t rgb = pack_rgb8(a);
    if (F.packed_out) F.out[local_tile * 64u + lane] = rgb;
    else {
        if (F.fwd_dst) F.fwd_dst[px] = F.fwd_src[px];
        F.out[px] = rgb;
    }
}

// batched BVHVisualization on caller rays (rt_bvh_visualize): one lane per ray, counts[2i] = nodes
// visited, counts[2i + 1] = leaves reached
__global__ __launch_bounds__(256) void k_bvh_visualize(SceneView S, const rt_ray *__restrict__ rays,
                                                       uint32_t *__restrict__ counts, uint32_t n) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    rt_ray q = rays[i];
    const DRay r = make_ray(mk(q.ox, q.oy, q.oz), mk(q.dx, q.dy, q.dz), q.tmax);
    Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
    uint32_t visits = 0, leaves = 0;
    heat_walk(S, T, r, visits, leaves);
    counts[2 * (size_t)i] = visits;
    counts[2 * (size_t)i + 1] = leaves;
}
#endif

// Batched Renderer::Trace(ray, lastSpecular, depth) (renderer.cpp:17-72) / WhittedTrace(ray,
// depth) (renderer.cpp:138-195): one lane per caller ray, the ray's own RNG state in and out.
// The optional hit record is the ray as the first IntersectBVH leaves it (renderer.cpp:20),
// from a separate closest-hit walk of the same ray (same result, taken only when asked for).
template <int MODE, int MAXD, bool TEX_SKY>
__global__ __launch_bounds__(256) void k_trace(SceneView S, TraceArgs A) {
    extern __shared__ uint32_t lds_stack[];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool on = i < A.n;
    uint32_t nshadow = 0, nbounce = 0;
    if (on) {
        const rt_ray q = A.rays[i];
        DRay r = make_ray(mk(q.ox, q.oy, q.oz), mk(q.dx, q.dy, q.dz), q.tmax);
        const uint32_t fl = A.flags ? A.flags[i] : 1u;
        r.inside = (fl & 2u) != 0u;
        Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
        if (A.hits) {
            DRay h = r;
            if (A.depth > 0) {          // Trace(.., 0) returns before intersecting (renderer.cpp:18)
                closest_hit(S, T, h);
                finish_uv(S, h);
            }
            rt_hit o;
            o.t = h.t; o.obj = h.obj; o.u = h.u; o.v = h.v;
            A.hits[i] = o;
        }
        uint32_t seed = A.seeds[i];
        f3 v;
        if constexpr (MODE == M_WHITTED) v = trace_whitted<TEX_SKY>(S, T, r, (int)A.depth, seed, nshadow, nbounce);
        else v = trace_path<MAXD, TEX_SKY>(S, T, r, (int)A.depth, seed, nshadow, nbounce, (fl & 1u) != 0u);
        A.radiance[3u * i] = v.x;
        A.radiance[3u * i + 1u] = v.y;
        A.radiance[3u * i + 2u] = v.z;
        A.seeds[i] = seed;
    }
    if (A.counts) {                      // every lane of the wave takes part in the sums
        nshadow = wave_sum(nshadow);
        nbounce = wave_sum(nbounce);
        if ((threadIdx.x & 63u) == 0u) {
            if (nshadow) atomicAdd(&A.counts[0], (unsigned long long)nshadow);
            if (nbounce) atomicAdd(&A.counts[1], (unsigned long long)nbounce);
        }
    }
}

// ------------------------------------------------------------------ wavefront path tracing
// Renderer::Trace (renderer.cpp:17-72) for Trace depth >= 2, one bounce level per launch
// (PathArgs in rt_dev_types.h).  Each path runs exactly trace_path's arithmetic and RNG
// draws; only the scheduling differs: after every level the live paths are compacted, so a
// deep level that keeps 10 % of the paths alive runs 10 % of the waves, all full.  The
// fold of a path's records is innermost-first, and k_pt_finish sums a pixel's samples in
// sample order, so pixel values are bit-identical to the one-kernel path tracer.
__device__ __forceinline__ f3 fold_record(f3 r, f3 mul, float c, f3 add, bool diff) {
    return diff ? mul * ((r * c) / kINV2PI) + add : mul * r;
}

// One bounce of one path (the body of trace_path's loop).  Returns true when the path
// goes on: its fold record is then stored at rec[levels - 1] and the state holds the
// bounce ray; otherwise the folded path value is stored in result[p].
// Path-state streams (state, fold records, results, level queues) are touched once per path
// and level.  Plain loads / stores: non-temporal ones (so that the streams would not evict BVH
// nodes from L1 / L2) measured CFG5-sub -1 %, CFG3-sub neutral, TEAPOT-F depth 10 +5.5 %
// (profiles/r02/ab_nt*_*.json) and were removed in round 6.
template <class T>
__device__ __forceinline__ T ld_stream(const T *p) { return *p; }
template <class T>
__device__ __forceinline__ void st_stream(T *p, T v) { *p = v; }
__device__ __forceinline__ float4 ld_stream4(const float4 *p) { return *p; }
__device__ __forceinline__ void st_stream4(float4 *p, float4 v) { *p = v; }

struct PathLane {
    DRay ray;
    uint32_t seed, p;
    int d, levels;
    bool lastSpec;
};

// a parked path's state (PathArgs::state) back into a lane
__device__ __forceinline__ void pt_load(const PathArgs &P, PathLane &L) {
    const float4 a = ld_stream4(P.state + 2 * (size_t)L.p), b = ld_stream4(P.state + 2 * (size_t)L.p + 1);
    const uint32_t meta = __float_as_uint(b.w);
    L.seed = __float_as_uint(a.w);
    L.d = (int)(meta & 0xffu);
    L.levels = (int)((meta >> 8) & 0xffu);
    L.lastSpec = (meta >> 16) & 1u;
    L.ray = make_ray(mk(a.x, a.y, a.z), mk(b.x, b.y, b.z), 1e34f);
    L.ray.inside = (int)((meta >> 17) & 1u);
}

// One bounce of one path (the body of trace_path's loop).  Returns true when the path goes
// on: its bounce ray is then parked in PathArgs::state (written before the NEE shadow ray,
// so the ray's registers are not live across that traversal) and its fold record stored at
// rec[levels - 1]; otherwise the folded path value is stored in result[p].
// CAM: 1 = every path is at its camera ray (the level-0 kernel), -1 = none is (levels >= 1),
// 0 = decided per path
template <bool TEX_SKY, int CAM = 0, class TR>
__device__ __forceinline__ bool pt_step(const SceneView &S, const TR &T, const FrameArgs &F, const PathArgs &P,
                                        PathLane &L, uint32_t &nshadow, uint32_t &nbounce) {
    const int depth = (int)F.depth;
    const bool cam = CAM == 1 ? true : CAM == -1 ? false : L.d == depth;
    if (!cam) ++nbounce;
    if (cam) closest_hit_primary(S, T, L.ray);   // camera rays: the wave walk if the scene asks
    else closest_hit(S, T, L.ray);
    f3 term = mk(0, 0, 0);
    bool rec = false, rdiff = false;
    f3 rmul = mk(0, 0, 0), radd = mk(0, 0, 0);
    float rc = 0.0f;
    if (L.ray.obj == -1) {
        term = sky_color<TEX_SKY>(S, L.ray.D);
    } else {
        f3 I = L.ray.O + L.ray.t * L.ray.D;
        f3 N;
        const DevMaterial &m = hit_surface(S, L.ray, I, N);
        if (m.flag == F_LIGHT) {
            term = L.lastSpec ? mk(m.c0[0], m.c0[1], m.c0[2]) : mk(0, 0, 0);
        } else {
            const bool last = L.d == 1;
            bool spec;
            {
                DRay out;
                spec = scatter(m, L.ray, I, N, out, L.seed, last);
                rdiff = m.flag == F_DIFFUSE || (m.flag == F_MIX && !spec);
                if (!last) {                           // park the bounce ray now
                    if (rdiff) rc = dot(N, out.D);
                    const uint32_t meta = (uint32_t)(L.d - 1) | ((uint32_t)(L.levels + 1) << 8) |
                                          ((spec ? 1u : 0u) << 16) | ((out.inside ? 1u : 0u) << 17);
                    st_stream4(P.state + 2 * (size_t)L.p, make_float4(out.O.x, out.O.y, out.O.z, 0.0f));
                    st_stream4(P.state + 2 * (size_t)L.p + 1, make_float4(out.D.x, out.D.y, out.D.z, __uint_as_float(meta)));
                }
            }
            const f3 albedo = mat_color(S, m, L.ray, I);
            rec = true;
            if (rdiff) {
                const f3 BRDF = albedo * kINVPI;
                radd = nee(S, T, I, N, BRDF, L.seed, nshadow);
                rmul = BRDF;
            } else {
                rmul = albedo;
            }
            ++L.levels;
            if (!last) {                               // the path goes on
                st_stream(reinterpret_cast<uint32_t *>(P.state + 2 * (size_t)L.p) + 3, L.seed);
                float4 *rp = P.rec + 2 * ((size_t)(L.levels - 1) * P.npaths + L.p);
                st_stream4(rp, make_float4(rmul.x, rmul.y, rmul.z, rc));
                st_stream4(rp + 1, make_float4(radd.x, radd.y, radd.z, rdiff ? 1.0f : 0.0f));
                return true;
            }
        }
    }
    f3 r = term;                                       // the path ends: fold innermost-first
    int k = L.levels - 1;
    if (rec) { r = fold_record(r, rmul, rc, radd, rdiff); --k; }
    for (; k >= 0; --k) {
        const float4 *rp = P.rec + 2 * ((size_t)k * P.npaths + L.p);
        const float4 q0 = ld_stream4(rp), q1 = ld_stream4(rp + 1);
        r = fold_record(r, mk(q0.x, q0.y, q0.z), q0.w, mk(q1.x, q1.y, q1.z), q1.w != 0.0f);
    }
    st_stream4(P.result + L.p, make_float4(r.x, r.y, r.z, 0.0f));
    return false;
}

// One bounce level of the batch's paths: live paths are parked and compacted into the
// next level's queue -- or, when the level holds no more paths than P.drain_below (about
// one round of resident waves, where a level is one latency chain long, not work bound)
// or P.level >= P.drain_level, the launch drains: each lane runs its path to the end, so
// the deep levels' latency chains overlap in one launch instead of each level paying its
// own kernel-wide tail (the later launches then find empty queues and exit).
#ifndef RT_PT_WAVES_PER_SIMD
#define RT_PT_WAVES_PER_SIMD 5   // 96 VGPRs + 88 B spill: CFG5-sub -6 %, CFG3-sub +2 % (profiles/r01/ab_pt_park_*.json)
#endif
// LV0: compiled for level 0 only (camera rays; no queue reads, no drain loop), so the
// level-0 kernel's registers are not sized by the bounce levels' code; BOUNCE: levels >= 1
// only (the lane kernel's drained levels: no camera-ray code)
template <bool TEX_SKY, uint32_t WPB = 4, class TR = Trav<256>, bool LV0 = false, bool BOUNCE = false>
__device__ __forceinline__ void pt_level_run(const SceneView &S, const FrameArgs &F, const PathArgs &P, const TR &T) {
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t level = LV0 ? 0u : P.level;
    static_assert(!(LV0 && BOUNCE), "level 0 is the camera level");
    // this level's entries: segment k holds segp[k + 1] - segp[k] paths (LDS prefix sums)
    __shared__ uint32_t segp[kQueueSegs + 1];
    if (tid == 0) {
        uint32_t acc = 0;
        segp[0] = 0;
        for (uint32_t k = 0; k < kQueueSegs; ++k) {
            acc += level == 0 ? 0u : __atomic_load_n(&P.qcount[(level * kQueueSegs + k) * 16u], __ATOMIC_RELAXED);
            segp[k + 1] = acc;
        }
    }
    __syncthreads();
    const uint32_t n = level == 0 ? P.npaths : segp[kQueueSegs];
    if (n == 0) return;                                // a level after the drain
    const bool DRAIN = !LV0 && (level >= P.drain_level || (level > 0 && n <= P.drain_below));
    const uint32_t nwaves = gridDim.x * WPB;
    uint32_t nshadow = 0, nbounce = 0;
    // chunks of 64 entries: level 0 and static mode walk them wave-strided; dynamic mode
    // (levels >= 1) takes the next chunk from one of 8 head counters (head h hands out the
    // chunks j = h mod 8; an exhausted head sends the wave to the next one), so the level
    // ends when the work ends, not when the unluckiest wave's share does
    const bool dyn = P.dynamic && level > 0 && !DRAIN;   // a drain level has at most one chunk per wave
    uint32_t head = (blockIdx.x * WPB + (tid >> 6)) % 8u, heads_left = 8u;
    uint32_t w = blockIdx.x * WPB + (tid >> 6);
    for (;;) {                                         // wave-uniform loop
        if (dyn) {
            uint32_t *hp = &P.qhead[(level * 8u + head) * 16u];
            uint32_t c = 0;
            // the wave's own head: straight to the atomic; another head (after its own ran
            // dry) is read first, so an exhausted head costs no atomic -- the waves leave a
            // level together and would otherwise queue 8 atomics each on the same lines
            if (lane == 0) {
                c = heads_left == 8u ? 0u : __atomic_load_n(hp, __ATOMIC_RELAXED);
                if ((head + 8u * c) * 64u < n) c = atomicAdd(hp, 1u);
            }
            w = head + 8u * __builtin_amdgcn_readfirstlane(c);
            if (w * 64u >= n) {
                if (--heads_left == 0) break;
                head = (head + 1u) % 8u;
                continue;
            }
        } else if (w * 64u >= n) {
            break;
        }
        const uint32_t i = w * 64u + lane;
        bool act = i < n;
        PathLane L;
        L.p = i; L.seed = 0; L.d = (int)F.depth; L.levels = 0; L.lastSpec = true;
        if (!BOUNCE && act && level == 0) {            // camera ray of (pixel, sample)
            const uint32_t t = i >> 6, lt = t % F.ntiles_local, sl = t / F.ntiles_local;
            const uint32_t tile = global_tile(F, lt);
            const uint32_t x = (tile % F.tiles_x) * 8u + (lane & 7u), y = (tile / F.tiles_x) * 8u + (lane >> 3);
            act = x < F.W && y < F.H;
            if (act) {
                const uint32_t px = x + y * F.W;
                L.seed = init_seed(px + F.W * F.H * (P.s0 + sl + F.spp * F.frame));
                L.ray = primary_ray(F, x, y, L.seed);
            }
        } else if (!LV0 && act) {
            uint32_t k = 0;                            // segment of entry i: binary search
            for (uint32_t step = kQueueSegs / 2; step; step >>= 1)
                if (i >= segp[k + step]) k += step;
            L.p = ld_stream(P.queue_in + k * P.seg_cap + (i - segp[k]));
            pt_load(P, L);
        }
        bool cont = false;
        const uint64_t t_start = (LV0 && P.tile_cost) ? __builtin_amdgcn_s_memtime() : 0;
        if (act) {
            cont = pt_step<TEX_SKY, LV0 ? 1 : BOUNCE ? -1 : 0>(S, T, F, P, L, nshadow, nbounce);   // a live path is parked in P.state
            if (DRAIN)
                while (cont) {
                    pt_load(P, L);
                    cont = pt_step<TEX_SKY, -1>(S, T, F, P, L, nshadow, nbounce);
                }
        }
        if (LV0 && P.tile_cost && lane == 0)   // this chunk = one (tile, sample) of the camera level
            atomicAdd(&P.tile_cost[w % F.ntiles_local], (uint32_t)(__builtin_amdgcn_s_memtime() - t_start));
        if (!DRAIN) {   // compaction: one atomic per wave reserves the slots of its live paths
            const uint64_t live = __ballot(cont);
            if (live) {
                uint32_t base = 0;
                const uint32_t seg = w % kQueueSegs;
                if (lane == 0) base = atomicAdd(&P.qcount[((level + 1) * kQueueSegs + seg) * 16u], (uint32_t)__popcll(live));
                base = __builtin_amdgcn_readfirstlane(base);
                const uint32_t rk = (uint32_t)__popcll(live & ((1ull << lane) - 1ull));
                if (cont) st_stream(P.queue_out + seg * P.seg_cap + base + rk, L.p);
            }
        }
        // level 0 runs one wave per chunk (launch_pt_level's grid): no second iteration, so no
        // state carried around the loop (81 -> fewer VGPRs in k_pt_level0)
        if (LV0) break;   // k_pt_level0's grid has one wave per chunk: no loop kept live (81 -> 49 VGPRs, round 4)
        if (!dyn) w += nwaves;
    }
    count_rays(F, blockIdx.x * WPB + (tid >> 6), lane, nshadow, nbounce);
}

template <bool TEX_SKY>
__global__ __launch_bounds__(256, RT_PT_WAVES_PER_SIMD) void k_pt_level(SceneView S, FrameArgs F, PathArgs P) {
    extern __shared__ uint32_t lds_stack[];
    Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
    pt_level_run<TEX_SKY>(S, F, P, T);
}
#ifndef RT_PT_LV0_WAVES
#define RT_PT_LV0_WAVES 6   // 81 VGPRs unconstrained; 5 -> 6 waves: CFG5-sub 7.94 -> 7.74 ms (round 3)
#endif
template <bool TEX_SKY>
__global__ __launch_bounds__(256, RT_PT_LV0_WAVES) void k_pt_level0(SceneView S, FrameArgs F, PathArgs P) {
    extern __shared__ uint32_t lds_stack[];
    Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
    pt_level_run<TEX_SKY, 4, Trav<256>, true>(S, F, P, T);
}

// ---- lane state machine for the incoherent levels (>= 1) -------------------------------
// At a bounce level the 64 paths of a wave traverse unrelated parts of the BVH: a wave that
// runs each lane's whole closest-hit + NEE traversal before taking new paths keeps ~10 % of
// its lanes busy (SQ_THREAD_CYCLES_VALU / 64 SQ_INSTS_VALU on CFG5-sub level 1).  Here every
// lane owns one path at a time and advances it by bounded traversal steps; a lane whose
// traversal finished shades, starts its shadow ray or hands the path on, and a lane without
// a path takes the next one from the level queue -- so lanes stay busy until the queue runs
// dry.  The steps of each path are closest_hit_t / occluded_t's iterations in their order,
// and the shading is pt_step's, split at the shadow ray: results are bit-identical.

// Round 3: one step function for both traversals (tr_step) instead of ch_step and oc_step side
// by side -- a wave whose lanes are in both traversals issued both bodies every step -- with
// one shared primitive loop, and without the wave-uniform scalar node load (+1 % with it):
// CFG5-sub 8.71 -> 8.09 ms, CFG3-sub 2.00 -> 1.90 ms, TEAPOT-F depth 10 0.837 -> 0.764 ms
// (pipelined frames; profiles/r03/ab_merged_step.txt).
// one iteration of closest_hit_t's loop (ch) or occluded_t's loop (!ch) with the interior
// node code shared: lanes of a wave in either traversal load and slab-test their child pair in
// the same instructions (ch_step and oc_step side by side issue both).  The visiting order of
// each traversal is unchanged: ch takes the nearer accepted child first (the reference's
// IntersectAABB distances, 1e30 = miss), oc the farther one.  true when the traversal is over.
// the two-level node records (build_quads in rt_device.hip, RT_PT_QUADS=1): odd-depth marker bit of
// an entry's 24-bit field, and the union box of two node entries (the x's-child box the walk tests)
constexpr uint32_t kQuadOddDev = 1u << 23;
__device__ __forceinline__ void entry_union(float4 a0, float4 b0, float4 a1, float4 b1, float4 &ua, float4 &ub) {
    ua = make_float4(fminf(a0.x, a1.x), fminf(a0.y, a1.y), fminf(a0.z, a1.z), fmaxf(a0.w, a1.w));
    ub = make_float4(fmaxf(b0.x, b1.x), fmaxf(b0.y, b1.y), 0.0f, 0.0f);
}
// the binary step's decision at a node whose children's slab intervals are (n1, x1), (n2, x2):
// false = go on with `word`, true = the traversal is over
template <class TR>
__device__ __forceinline__ bool pair_decide(const TR &T, const DRay &r, float n1, float x1, float n2, float x2, uint32_t w1,
                                            uint32_t w2, uint32_t &word, int &sp, bool ch) {
    // ch: slab_accept's distance != 1e30; oc: the plain hit test
    const bool h1 = x1 >= n1 && n1 < r.t && x1 > 0 && (!ch || n1 != 1e30f);
    const bool h2 = x2 >= n2 && n2 < r.t && x2 > 0 && (!ch || n2 != 1e30f);
    if (!(h1 || h2)) {
        if (sp == 0) return true;
        word = stack_pop(T, sp);
        return false;
    }
    const bool second = (h1 && h2) ? (ch ? n1 > n2 : n2 > n1) : h2;   // child 2 first
    word = second ? w2 : w1;
    if (h1 && h2) stack_push(T, sp, second ? w1 : w2);
    return false;
}
template <bool FAST, class TR, bool QUAD = false>
__device__ __forceinline__ bool tr_step(const SceneView &S, const TR &T, DRay &r, uint32_t &word, int &sp, bool ch,
                                        bool &hit) {
    const uint32_t cnt = word & 0xffu, lf = word >> 8;
    if (cnt) {
        if constexpr (!kExt) {
            // one primitive loop for both: prim_hit(k) is exactly "prim_intersect(k) would take
            // it" (t < r.t && t > EPS, both sphere roots) for triangles, spheres and planes, and an
            // any-hit lane stops at its first hit, so the t it overwrote is never read again
            for (uint32_t k = lf; k < lf + cnt; ++k) {
                const uint32_t t0 = __float_as_uint(r.t);
                prim_intersect(S, T.prims, k, r);
                if (!ch && __float_as_uint(r.t) != t0) { hit = true; return true; }
            }
        } else if (ch) {
            leaf_closest(S, T.prims, lf, cnt, r);
        } else if (leaf_any(S, T.prims, lf, cnt, r)) {
            hit = true;
            return true;
        }
        if (sp == 0) return true;
        word = stack_pop(T, sp);
        return false;
    }
    float n1, x1, n2, x2;
    uint32_t w1, w2;
    if constexpr (QUAD) {
        if (lf & kQuadOddDev) {   // a popped odd-depth child: its children are half of its parent's record
            const float4 *q = S.quads + 8u * ((lf & (kQuadOddDev - 1u)) >> 1) + 4u * (lf & 1u);
            const float4 a0 = q[0], b0 = q[1], a1 = q[2], b1 = q[3];
            slab<FAST>(r, a0, b0, n1, x1);
            slab<FAST>(r, a1, b1, n2, x2);
            return pair_decide(T, r, n1, x1, n2, x2, __float_as_uint(b0.z), __float_as_uint(b1.z), word, sp, ch);
        }
        // an even-depth node's record: its children's boxes as unions of their children's (a
        // leaf child's own entry in its first slot), then the nearer interior child's children --
        // the binary walk's two steps with the same r.t, from one 128-B load
        const float4 *q = S.quads + 8u * lf;
        const float4 s0 = q[0], s1 = q[1], s2 = q[2], s3 = q[3], s4 = q[4], s5 = q[5], s6 = q[6], s7 = q[7];
        const bool la = (__float_as_uint(s1.w) & 1u) != 0u, lb = (__float_as_uint(s5.w) & 1u) != 0u;
        float4 ua = s0, ub = s1, va = s4, vb = s5;
        if (!la) entry_union(s0, s1, s2, s3, ua, ub);
        if (!lb) entry_union(s4, s5, s6, s7, va, vb);
        slab<FAST>(r, ua, ub, n1, x1);
        slab<FAST>(r, va, vb, n2, x2);
        w1 = la ? __float_as_uint(s1.z) : ((kQuadOddDev | (lf << 1)) << 8);
        w2 = lb ? __float_as_uint(s5.z) : ((kQuadOddDev | (lf << 1) | 1u) << 8);
        const bool h1 = x1 >= n1 && n1 < r.t && x1 > 0 && (!ch || n1 != 1e30f);
        const bool h2 = x2 >= n2 && n2 < r.t && x2 > 0 && (!ch || n2 != 1e30f);
        if (!(h1 || h2)) {
            if (sp == 0) return true;
            word = stack_pop(T, sp);
            return false;
        }
        const bool second = (h1 && h2) ? (ch ? n1 > n2 : n2 > n1) : h2;
        if (h1 && h2) stack_push(T, sp, second ? w1 : w2);
        if (second ? lb : la) {   // the nearer child is a leaf: its primitives next
            word = second ? w2 : w1;
            return false;
        }
        const float4 c0 = second ? s4 : s0, d0 = second ? s5 : s1, c1 = second ? s6 : s2, d1 = second ? s7 : s3;
        slab<FAST>(r, c0, d0, n1, x1);
        slab<FAST>(r, c1, d1, n2, x2);
        return pair_decide(T, r, n1, x1, n2, x2, __float_as_uint(d0.z), __float_as_uint(d1.z), word, sp, ch);
    } else {
        child_pair<FAST, TR, false>(T, r, lf, n1, x1, n2, x2, w1, w2);
        return pair_decide(T, r, n1, x1, n2, x2, w1, w2, word, sp, ch);
    }
}

enum : uint32_t { PH_FETCH = 0, PH_TRACE = 1, PH_SHADOW = 2, PH_DONE = 3, PH_TRACED = 4, PH_SHADOWED = 5 };
#ifndef RT_PT_BATCH
#define RT_PT_BATCH 24   // lanes that must be waiting before a wave shades / refills (unless nothing else is left)
#endif

#ifndef RT_PT_STEPS
#define RT_PT_STEPS 32  // traversal steps between two shading / refill points
#endif
template <bool TEX_SKY, uint32_t WPB, class TR, bool QUAD = false>
__device__ __forceinline__ void pt_lanes_run(const SceneView &S, const FrameArgs &F, const PathArgs &P, const TR &T) {
    const uint32_t root = QUAD ? S.quad_root : S.root_word;   // the first entry of every traversal
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t level = P.level;
    __shared__ uint32_t segp[kQueueSegs + 1];
    if (tid == 0) {
        uint32_t acc = 0;
        segp[0] = 0;
        for (uint32_t k = 0; k < kQueueSegs; ++k) {
            acc += __atomic_load_n(&P.qcount[(level * kQueueSegs + k) * 16u], __ATOMIC_RELAXED);
            segp[k + 1] = acc;
        }
    }
    __syncthreads();
    const uint32_t n = segp[kQueueSegs];
    if (n == 0) return;
    const uint32_t per = (n + kQueueSegs - 1u) / kQueueSegs;   // entries per head
    // a level small enough to drain is latency-bound: k_pt_level's drain (each wave takes one
    // chunk and runs its paths to the end) measured faster there than the lane refill
    if (level >= P.drain_level || n <= P.drain_below) {
        pt_level_run<TEX_SKY, WPB, TR, false, true>(S, F, P, T);   // drained levels: no camera-ray code
        return;
    }
    const bool drain = false;
    const uint32_t wave = blockIdx.x * WPB + (tid >> 6);
    // kQueueSegs head counters: head h hands out this level's entries [h per, (h+1) per)
    // (contiguous runs); a path from head h goes on
    // into segment h of the next queue (<= per = ceil(n / 16) entries, within seg_cap)
    uint32_t head = wave % kQueueSegs, heads_left = kQueueSegs, src = 0;
    uint32_t nshadow = 0, nbounce = 0;
    const int depth = (int)F.depth;

    uint32_t phase = PH_FETCH;
    PathLane L;
    L.p = 0; L.seed = 0; L.d = 0; L.levels = 0; L.lastSpec = true;
    uint32_t word = 0;
    int sp = 0;
    bool fast = false, hitsh = false, fresh = false;
    // shading state carried across the shadow ray
    f3 BRDF = mk(0, 0, 0);
    float rc = 0.0f, dotNL = 0.0f, dotNlL = 0.0f, dist = 0.0f;
    bool goes_on = false;
    DRay ray = make_ray(mk(0, 0, 0), mk(0, 0, 1), 1e34f);

    for (;;) {
        // 1. lanes without a path take the next ones from the queue (once enough are idle)
        const uint64_t want = __ballot(phase == PH_FETCH);
        const uint64_t busy = __ballot(phase == PH_TRACE || phase == PH_SHADOW);
        if (want && (__popcll(want) >= RT_PT_BATCH || !busy)) {
            uint32_t got = 0;                          // entries this wave obtained (wave-uniform)
            uint32_t base = 0;
            const uint32_t k = (uint32_t)__popcll(want);
            while (heads_left) {
                const uint32_t lo = head * per, hi = min(n, lo + per);   // head h: entries [h per, (h+1) per)
                uint32_t c = 0;
                if (lane == 0) {
                    uint32_t *hp = &P.qhead[(level * kQueueSegs + head) * 16u];
                    c = __atomic_load_n(hp, __ATOMIC_RELAXED);
                    if (lo + c < hi) c = atomicAdd(hp, k);
                }
                c = __builtin_amdgcn_readfirstlane(c);
                if (lo + c < hi) {
                    base = lo + c;
                    got = min(k, hi - base);           // unread entries of this head
                    break;
                }
                --heads_left;
                head = (head + 1u) % kQueueSegs;
            }
            if (phase == PH_FETCH) {
                const uint32_t r = (uint32_t)__popcll(want & ((1ull << lane) - 1ull));
                if (r < got) {
                    const uint32_t i = base + r;
                    src = head;
                    fresh = true;
                    phase = PH_TRACE;
                    uint32_t sg = 0;
                    for (uint32_t step = kQueueSegs / 2; step; step >>= 1)
                        if (i >= segp[sg + step]) sg += step;
                    L.p = ld_stream(P.queue_in + sg * P.seg_cap + (i - segp[sg]));
                    pt_load(P, L);
                    ray = L.ray;
                } else if (!heads_left) {
                    phase = PH_DONE;
                }
            }
        }
        if (!__ballot(phase != PH_DONE && phase != PH_FETCH)) {
            if (!__ballot(phase == PH_FETCH)) break;   // every lane done
            continue;                                  // (lanes still waiting for entries)
        }
        const bool had_ready = __ballot(phase == PH_TRACED || phase == PH_SHADOWED) != 0;
        // 2. bounded traversal steps
        if (phase == PH_TRACE && fresh) {              // a fresh closest-hit traversal
            fresh = false;
            word = root;
            sp = 0;
            fast = S.bounds_finite && ray_finite(ray);
            if (L.d != depth) ++nbounce;
        }
        for (int st = 0; st < RT_PT_STEPS; ++st) {
            if (phase == PH_TRACE || phase == PH_SHADOW) {
                const bool ch = phase == PH_TRACE;
                if (fast ? tr_step<true, TR, QUAD>(S, T, ray, word, sp, ch, hitsh)
                         : tr_step<false, TR, QUAD>(S, T, ray, word, sp, ch, hitsh))
                    phase = ch ? PH_TRACED : PH_SHADOWED;
            }
            if (!__ballot(phase == PH_TRACE || phase == PH_SHADOW)) break;
        }
        // shade only once enough lanes wait for it (or nothing else can make progress)
        const uint64_t ready = __ballot(phase == PH_TRACED || phase == PH_SHADOWED);
        const bool shade_now = __popcll(ready) >= RT_PT_BATCH || !__ballot(phase == PH_TRACE || phase == PH_SHADOW) ||
                               (had_ready && __popcll(ready) >= RT_PT_BATCH / 2);
        // 3. closest hit found: shade up to the shadow ray (pt_step, first half)
        bool finish = false;                           // this lane's path leaves the level now
        f3 term = mk(0, 0, 0), radd = mk(0, 0, 0), rmul = mk(0, 0, 0);
        bool rec = false, rdiff = false;
        if (shade_now && phase == PH_TRACED) {
            word = 0; sp = 0;
            L.ray = ray;
            if (ray.obj == -1) {
                term = sky_color<TEX_SKY>(S, ray.D);
                finish = true;
            } else {
                f3 I = ray.O + ray.t * ray.D;
                f3 N;
                const DevMaterial &m = hit_surface(S, L.ray, I, N);
                if (m.flag == F_LIGHT) {
                    term = L.lastSpec ? mk(m.c0[0], m.c0[1], m.c0[2]) : mk(0, 0, 0);
                    finish = true;
                } else {
                    const bool last = L.d == 1;
                    bool spec;
                    rc = 0.0f;
                    {
                        DRay out;
                        spec = scatter(m, L.ray, I, N, out, L.seed, last);
                        rdiff = m.flag == F_DIFFUSE || (m.flag == F_MIX && !spec);
                        if (!last) {
                                    if (rdiff) rc = dot(N, out.D);
                            const uint32_t meta = (uint32_t)(L.d - 1) | ((uint32_t)(L.levels + 1) << 8) |
                                                  ((spec ? 1u : 0u) << 16) | ((out.inside ? 1u : 0u) << 17);
                            st_stream4(P.state + 2 * (size_t)L.p, make_float4(out.O.x, out.O.y, out.O.z, 0.0f));
                            st_stream4(P.state + 2 * (size_t)L.p + 1, make_float4(out.D.x, out.D.y, out.D.z, __uint_as_float(meta)));
                        }
                    }
                    const f3 albedo = mat_color(S, m, L.ray, I);
                    goes_on = !last;
                    ++L.levels;
                    rec = true;
                    if (rdiff) {                       // NextEventDirectIllumination up to the shadow ray
                        BRDF = albedo * kINVPI;
                        f3 Il = light_point(S, L.seed);
                        f3 Lv = Il - I;
                        dist = length(Lv);
                        Lv = Lv / dist;
                        f3 Nl = (kExt && S.light_quad) ? mk(S.light_N[0], S.light_N[1], S.light_N[2])
                                                       : (Il - mk(S.light_c[0], S.light_c[1], S.light_c[2])) * S.light_invr;
                        if (dot(Nl, Lv) > 0) Nl = -Nl;
                        dotNL = dot(N, Lv);
                        dotNlL = dot(Nl, -Lv);
                        if (dotNL > 0 && dotNlL > 0) {
                            ray = make_ray(I, Lv, dist - 2.0f * kEPS);
                            ++nshadow;
                            phase = PH_SHADOW;
                            word = root;
                            sp = 0;
                            hitsh = false;
                            fast = S.bounds_finite && ray_finite(ray);
                        } else {
                            rmul = BRDF;
                            rdiff = true;
                            finish = true;
                        }
                    } else {
                        rmul = albedo;
                        finish = true;
                    }
                }
            }
        } else if (shade_now && phase == PH_SHADOWED) {   // 4. the shadow ray is answered
            word = 0; sp = 0;
            if (!hitsh) {
                const float area = S.light_area;
                float solid = (dotNlL * area) / (dist * dist);
                float lightPDF = 1.0f / solid;
                const DevMaterial &lm = S.mats[S.light_mat];
                const f3 lc = !kExt ? mk(lm.c0[0], lm.c0[1], lm.c0[2]) : mat_color(S, lm, ray, ray.O + ray.t * ray.D);
                radd = (lc * BRDF) * (dotNL / lightPDF);
            }
            rmul = BRDF;
            rec = true;
            rdiff = true;
            finish = true;
        }
        // 5. the path leaves this level: record + hand on, or fold
        bool enqueue = false;
        if (finish) {
            if (rec && goes_on) {
                st_stream(reinterpret_cast<uint32_t *>(P.state + 2 * (size_t)L.p) + 3, L.seed);
                float4 *rp = P.rec + 2 * ((size_t)(L.levels - 1) * P.npaths + L.p);
                st_stream4(rp, make_float4(rmul.x, rmul.y, rmul.z, rc));
                st_stream4(rp + 1, make_float4(radd.x, radd.y, radd.z, rdiff ? 1.0f : 0.0f));
                if (drain) {                           // next bounce in this lane
                    pt_load(P, L);
                    ray = L.ray;
                    phase = PH_TRACE;
                    fresh = true;
                } else {
                    enqueue = true;
                    phase = PH_FETCH;
                }
            } else {
                f3 r = term;
                int k = L.levels - 1;
                if (rec) { r = fold_record(r, rmul, rc, radd, rdiff); --k; }
                for (; k >= 0; --k) {
                    const float4 *rp = P.rec + 2 * ((size_t)k * P.npaths + L.p);
                    const float4 q0 = ld_stream4(rp), q1 = ld_stream4(rp + 1);
                    r = fold_record(r, mk(q0.x, q0.y, q0.z), q0.w, mk(q1.x, q1.y, q1.z), q1.w != 0.0f);
                }
                st_stream4(P.result + L.p, make_float4(r.x, r.y, r.z, 0.0f));
                phase = PH_FETCH;
            }
            goes_on = false;
        }
        uint64_t rem = __ballot(enqueue);
        while (rem) {                                  // one round per source head present
            const uint32_t seg = __builtin_amdgcn_readlane(src, (int)__builtin_ctzll(rem));
            const uint64_t m = __ballot(enqueue && src == seg);
            rem &= ~m;
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&P.qcount[((level + 1) * kQueueSegs + seg) * 16u], (uint32_t)__popcll(m));
            base = __builtin_amdgcn_readfirstlane(base);
            const uint32_t rk = (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (enqueue && src == seg) st_stream(P.queue_out + seg * P.seg_cap + base + rk, L.p);
        }
    }
    count_rays(F, wave, lane, nshadow, nbounce);
}

template <bool TEX_SKY, bool QUAD>
#ifndef RT_PT_LANES_WAVES
#define RT_PT_LANES_WAVES RT_PT_WAVES_PER_SIMD
#endif
__global__ __launch_bounds__(256, RT_PT_LANES_WAVES) void k_pt_lanes(SceneView S, FrameArgs F, PathArgs P) {
    extern __shared__ uint32_t lds_stack[];
    Trav<256> T{S.nodes, lds_stack + threadIdx.x, S.prims};
    pt_lanes_run<TEX_SKY, 4, Trav<256>, QUAD>(S, F, P, T);
}

// per pixel: add this batch's samples to the running sum in sample order; after the last
// batch the running average and the RGB8 pack exactly as render_tile
__global__ __launch_bounds__(256) void k_pt_finish(FrameArgs F, PathArgs P, int last) {
    const uint32_t g = blockIdx.x * 256u + threadIdx.x;
    if (g >= F.ntiles_local * 64u) return;
    const uint32_t lt = g >> 6, lane = g & 63u;
    const uint32_t tile = global_tile(F, lt);
    const uint32_t x = (tile % F.tiles_x) * 8u + (lane & 7u), y = (tile / F.tiles_x) * 8u + (lane >> 3);
    if (x >= F.W || y >= F.H) return;
    f3 sum = mk(0, 0, 0);
    if (P.s0 != 0) { const float4 q = P.sum[g]; sum = mk(q.x, q.y, q.z); }
    for (uint32_t sl = 0; sl < P.batch_spp; ++sl) {
        const float4 q = P.result[(size_t)(sl * F.ntiles_local + lt) * 64u + lane];
        sum = sum + mk(q.x, q.y, q.z);
    }
    if (!last) { P.sum[g] = make_float4(sum.x, sum.y, sum.z, 0.0f); return; }
    const uint32_t px = x + y * F.W;
    f3 res = (1.0f / (float)F.spp) * sum;
    float4 a = F.reset ? make_float4(0, 0, 0, 0) : F.acc[px];
    a.w += 1;                                                          // renderer.cpp:237-240
    const float wt = a.w, inv = 1.0f / wt;
    a = make_float4(a.x + inv * (res.x - a.x), a.y + inv * (res.y - a.y), a.z + inv * (res.z - a.z),
                    a.w + inv * (wt - a.w));
    F.acc[px] = a;
    const uint32_t rgb = pack_rgb8(a);
    if (F.packed_out) F.out[lt * 64u + lane] = rgb;
    else {
        if (F.fwd_dst) F.fwd_dst[px] = F.fwd_src[px];
        F.out[px] = rgb;
    }
}

// ------------------------------------------------------------------ launchers
// Each family's (variant -> kernel) pairing is written once, as a lookup of the kernel's host
// address: launch_kernel starts it, resident_blocks asks its occupancy.  The P... are the kernel's
// parameter types, which the builds of one family share.
template <class... P>
static void launch_kernel(const void *fn, dim3 grid, size_t lds, hipStream_t st, const P &...args) {
    void *argv[] = {const_cast<void *>(static_cast<const void *>(&args))...};
    (void)hipLaunchKernel(fn, grid, dim3(256), argv, lds, st);   // (an error stays for the caller's hipGetLastError)
}
#define RT_SKY(TEX, K) ((TEX) ? (const void *)K<true> : (const void *)K<false>)
#define RT_SKY_OF(TEX, K, ...) ((TEX) ? (const void *)K<__VA_ARGS__, true> : (const void *)K<__VA_ARGS__, false>)
// k_render / k_render_w8 / k_render_walkcheck (SceneView, FrameArgs)
static const void *frame_kernel(const FrameVariant &v) {
    if (v.build == FrameBuild::WalkCheck) return RT_SKY(v.tex, k_render_walkcheck);
    if (v.build == FrameBuild::SingleSample) return RT_SKY(v.tex, k_render_w8);
    switch (v.mode * 64 + v.maxd) {   // depth = the bounces' Trace depth (PACKET: 0 allowed)
    case M_PATH * 64 + 1: return RT_SKY_OF(v.tex, k_render, M_PATH, 1);
    case M_PATH * 64 + 4: return RT_SKY_OF(v.tex, k_render, M_PATH, 4);
    case M_PATH * 64 + 10: return RT_SKY_OF(v.tex, k_render, M_PATH, 10);
    case M_PATH * 64 + 32: return RT_SKY_OF(v.tex, k_render, M_PATH, 32);
    case M_WHITTED * 64 + 1: return RT_SKY_OF(v.tex, k_render, M_WHITTED, 1);
    case M_PACKET * 64 + 1: return RT_SKY_OF(v.tex, k_render, M_PACKET, 1);
    case M_PACKET * 64 + 10: return RT_SKY_OF(v.tex, k_render, M_PACKET, 10);
    case M_PACKET * 64 + 32: return RT_SKY_OF(v.tex, k_render, M_PACKET, 32);
    }
    return nullptr;   // no such build (rt_variants.h computes none): the launch fails
}
// k_render_work (SceneView, FrameArgs, tile work, pixel work, with distances)
static const void *work_kernel(const FrameVariant &v) {
    return v.maxd == 1 ? RT_SKY_OF(v.tex, k_render_work, 1) : RT_SKY_OF(v.tex, k_render_work, 32);
}
// k_trace (SceneView, TraceArgs)
static const void *trace_kernel(const FrameVariant &v) {
    switch (v.mode * 64 + v.maxd) {
    case M_PATH * 64 + 1: return RT_SKY_OF(v.tex, k_trace, M_PATH, 1);
    case M_PATH * 64 + 4: return RT_SKY_OF(v.tex, k_trace, M_PATH, 4);
    case M_PATH * 64 + 10: return RT_SKY_OF(v.tex, k_trace, M_PATH, 10);
    case M_PATH * 64 + 32: return RT_SKY_OF(v.tex, k_trace, M_PATH, 32);
    case M_WHITTED * 64 + 1: return RT_SKY_OF(v.tex, k_trace, M_WHITTED, 1);
    }
    return nullptr;
}
// k_pt_level0 (camera rays: the level-0-only build) / k_pt_level, k_pt_lanes (SceneView, FrameArgs, PathArgs)
static const void *pt_level_kernel(bool level0, bool tex) {
    return level0 ? RT_SKY(tex, k_pt_level0) : RT_SKY(tex, k_pt_level);
}
static const void *pt_lanes_kernel(bool quad, bool tex) {
    return quad ? (tex ? (const void *)k_pt_lanes<true, true> : (const void *)k_pt_lanes<false, true>)
                : (tex ? (const void *)k_pt_lanes<true, false> : (const void *)k_pt_lanes<false, false>);
}
// k_gbuffer / k_gbuffer_pixels (SceneView, FrameArgs, GBufferArgs)
static const void *gbuffer_kernel(const GBufferVariant &v) {
    return v.pixels ? RT_SKY(v.tex, k_gbuffer_pixels) : RT_SKY(v.tex, k_gbuffer);
}
#undef RT_SKY
#undef RT_SKY_OF

static void launch_work(const SceneView &S, const FrameArgs &F, const FrameLaunch &L, uint32_t *tile_work, uint32_t *pixel_work) {
    // stack, entry distances (counters [4] / [5], left out past 64 KB: trees deeper than 28), counters
    const size_t cnt = kWorkCounterBytes;
    const int wd = 2u * L.lds_bytes + cnt <= kLdsLaunchMax ? 1 : 0;
    const size_t lds = (wd ? 2u : 1u) * L.lds_bytes + cnt;
    launch_kernel<SceneView, FrameArgs, uint32_t *, uint32_t *, int>(work_kernel(L.v), L.grid, lds, L.stream, S, F, tile_work,
                                                                     pixel_work, wd);
}
static void launch_frame(const SceneView &S, const FrameArgs &F, const FrameLaunch &L) {
    launch_kernel<SceneView, FrameArgs>(frame_kernel(L.v), L.grid, L.lds_bytes, L.stream, S, F);
}
// workgroups of 256 threads of kernel fn resident per CU with lds bytes of dynamic LDS, on the
// current device; cached per (device, kernel, lds bytes): scenes with deeper trees need more
// LDS stack per workgroup, and renderers may run on several devices and host threads
static int resident_blocks(const void *fn, size_t lds) {
    static std::mutex mu;
    static std::map<std::tuple<int, const void *, size_t>, int> cache;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(mu);
    const auto key = std::make_tuple(dev, fn, lds);
    auto it = cache.find(key);
    if (it != cache.end()) return it->second;
    int b = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&b, fn, 256, lds) != hipSuccess || b <= 0) b = 2;
    cache.emplace(key, b);
    return b;
}
// one bounce level of the wavefront path tracer: as many workgroups as stay resident
// (the level's queue is walked wave-strided, so every wave gets an equal share)
static int launch_pt_level(const SceneView &S, const FrameArgs &F, const PathArgs &P, bool tex, size_t lds, uint32_t num_cus,
                           hipStream_t st) {
    const int pc = resident_blocks(pt_level_kernel(false, tex), lds);
    // level 0 (every path, costs vary by tile): one wave per 64 paths, balanced by the
    // hardware dispatcher; deeper levels: as many workgroups as stay resident walk the
    // queue wave-strided (a full grid of mostly empty workgroups measured 9-14 % slower)
    const uint32_t need = (P.npaths + 255u) / 256u;
    const uint32_t grid = P.level == 0 ? need : std::min(need, (uint32_t)pc * num_cus);
    launch_kernel<SceneView, FrameArgs, PathArgs>(pt_level_kernel(P.level == 0, tex), dim3(grid), lds, st, S, F, P);
    return pc * (int)num_cus * 256;   // resident lanes
}
// the lane state-machine kernel for a level (resident grid)
static void launch_pt_lanes(const SceneView &S, const FrameArgs &F, const PathArgs &P, bool tex, size_t lds, uint32_t num_cus,
                            hipStream_t st) {
    const void *fn = pt_lanes_kernel(S.quad_lanes && S.quads, tex);
    const uint32_t grid = std::min((P.npaths + 255u) / 256u, (uint32_t)resident_blocks(fn, lds) * num_cus);
    launch_kernel<SceneView, FrameArgs, PathArgs>(fn, dim3(grid), lds, st, S, F, P);
}
static void launch_pt_finish(const FrameArgs &F, const PathArgs &P, bool last, hipStream_t st) {
    hipLaunchKernelGGL(k_pt_finish, dim3((F.ntiles_local * 64u + 255u) / 256u), dim3(256), 0, st, F, P, last ? 1 : 0);
}
static void launch_trace(const SceneView &S, const TraceArgs &A, const FrameVariant &v, size_t lds, hipStream_t st) {
    launch_kernel<SceneView, TraceArgs>(trace_kernel(v), dim3((A.n + 255u) / 256u), lds, st, S, A);
}
static void launch_intersect(const SceneView &S, const rt_ray *rays, rt_hit *hits, uint32_t n, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_intersect, dim3((n + 255) / 256), dim3(256), lds, st, S, rays, hits, n);
}
static void launch_occluded(const SceneView &S, const rt_ray *rays, uint8_t *out, uint32_t n, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_occluded, dim3((n + 255) / 256), dim3(256), lds, st, S, rays, out, n);
}
static void launch_intersect_packet(const SceneView &S, const rt_ray *rays, rt_hit *hits, uint32_t n, hipStream_t st) {
    hipLaunchKernelGGL(k_intersect_packet, dim3((n + 255) / 256), dim3(256), 0, st, S, rays, hits, n);
}
// the rectangle form: one wave per touched tile; the list form: one lane per listed pixel
static void launch_gbuffer(const SceneView &S, const FrameArgs &F, const GBufferArgs &G, const GBufferVariant &v, size_t lds,
                           hipStream_t st) {
    const uint32_t grid = v.pixels ? (G.n + 255u) / 256u : (G.ntiles + 3u) / 4u;
    launch_kernel<SceneView, FrameArgs, GBufferArgs>(gbuffer_kernel(v), dim3(grid), lds, st, S, F, G);
}
// (a function's static, not a namespace-scope constant: the device pass would emit that one too)
const Launchers &launchers() {
    static const Launchers table = {launch_frame,    launch_work,     launch_intersect, launch_occluded, launch_intersect_packet,
                                    launch_pt_level, launch_pt_lanes, launch_pt_finish, launch_trace,    launch_gbuffer};
    return table;
}
#if RT_EXT == 0
void launch_heat(const SceneView &S, const FrameArgs &F, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_render_heat, dim3((F.ntiles_local + 3u) / 4u), dim3(256), lds, st, S, F);
}
void launch_visualize(const SceneView &S, const rt_ray *rays, uint32_t *counts, uint32_t n, size_t lds, hipStream_t st) {
    hipLaunchKernelGGL(k_bvh_visualize, dim3((n + 255) / 256), dim3(256), lds, st, S, rays, counts, n);
}
#endif

}  // namespace RT_KNS


#if RT_EXT == 0
// rank-0 side of the per-frame gather: packed shard tiles -> row-major frame
// One thread per (tile, pixel row): 32 B read from the shard's packed tile, 32 B written to
// the image row; the 64 threads of a wave cover 8 horizontally adjacent tiles x 8 rows, so a
// wave's stores are 8 contiguous 256-B row segments (the per-pixel form wrote 32-B pieces).
// first = 1: the multi-GPU frame's rank 0 rendered its own tiles straight into `out`, the
// buffer holds shards 1 .. nshards-1 only (shard s at (s - 1) x cap) and shard-0 tiles are left.
__global__ __launch_bounds__(256) void k_assemble(const uint32_t *__restrict__ gathered, uint32_t cap, uint32_t nshards,
                                                  const uint32_t *__restrict__ where, uint32_t tiles_x, uint32_t ntiles,
                                                  uint32_t W, uint32_t H, uint32_t first, uint32_t *__restrict__ out) {
    const uint32_t wave = blockIdx.x * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    const uint32_t groups_x = (tiles_x + 7u) / 8u;                  // 8-tile groups per tile row
    const uint32_t trow = wave / groups_x, tcol = (wave % groups_x) * 8u + (lane & 7u);
    const uint32_t tiles_y = (ntiles + tiles_x - 1u) / tiles_x;
    if (trow >= tiles_y || tcol >= tiles_x) return;
    const uint32_t tile = trow * tiles_x + tcol, row = lane >> 3;
    const uint32_t y = trow * 8u + row, x = tcol * 8u;
    if (y >= H) return;
    const uint32_t w = where ? where[tile] : 0u;
    const uint32_t shard = where ? (w >> 24) : tile % nshards, local = where ? (w & 0xffffffu) : tile / nshards;
    if (shard < first) return;
    const uint32_t *src = gathered + (size_t)(shard - first) * cap + local * 64u + row * 8u;
    uint32_t *dst = out + (size_t)y * W + x;
    if (x + 8u <= W && ((size_t)y * W + x) % 4u == 0u) {
        const uint4 a = reinterpret_cast<const uint4 *>(src)[0], b = reinterpret_cast<const uint4 *>(src)[1];
        reinterpret_cast<uint4 *>(dst)[0] = a;
        reinterpret_cast<uint4 *>(dst)[1] = b;
    } else {
        for (uint32_t i = 0; i < 8u && x + i < W; ++i) dst[i] = src[i];
    }
}


void launch_assemble(const uint32_t *gathered, uint32_t cap, uint32_t nshards, const uint32_t *where, uint32_t tiles_x,
                     uint32_t ntiles, uint32_t W, uint32_t H, uint32_t *out, hipStream_t st, uint32_t first) {
    const uint32_t waves = ((tiles_x + 7u) / 8u) * ((ntiles + tiles_x - 1u) / tiles_x);
    hipLaunchKernelGGL(k_assemble, dim3((waves + 3u) / 4u), dim3(256), 0, st, gathered, cap, nshards, where, tiles_x,
                       ntiles, W, H, first, out);
}
#endif

}  // namespace rt

#if defined(RT_FRAME_PHASES) && !RT_EXT
// diagnostic builds: the stamps of the core build's last frames (n <= kFramePhaseWaves * 8 words), and their reset
extern "C" __attribute__((visibility("default"))) int rt_debug_frame_phases(unsigned long long *out, size_t n) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(rt::kcore::rt_frame_phase_buf), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
extern "C" __attribute__((visibility("default"))) int rt_debug_frame_phases_clear() {
    void *p = nullptr;
    if (hipDeviceSynchronize() != hipSuccess || hipGetSymbolAddress(&p, HIP_SYMBOL(rt::kcore::rt_frame_phase_buf)) != hipSuccess) return -1;
    return hipMemset(p, 0, sizeof(unsigned long long) * 8u * rt::kcore::kFramePhaseWaves) == hipSuccess ? 0 : -1;
}
#endif
