// rt_build.h -- the text of the GPU BVH rebuild: the reference's binned-SAH builder
// (template/scene.h:845-976, Builder in rt_host.cpp) as steps over arrays that many lanes run at once.
//
// One text for gfx950 and for the host, like rt_update.h and under the same -ffp-contract=off.  The
// kernels of rt_build.hip supply a *lane context* P -- the lane index and count (tid, stride), the
// workgroup barrier (bar) and integer atomics (amax, aadd) -- and the stand-alone host programs run the
// same steps with SerialLane: tid = 0, stride = 1, no barrier, plain stores.  The order of the steps
// (build_order) and the sizes of the arrays (build_carve) are here too, once for both: the device
// supplies an executor that launches, the host one that loops (tests/cpp/host_build.h).  No std:: algorithm.
//
// Why many lanes reproduce the sequential builder bit for bit: every *decision* is order-independent.
// Node and bin boxes and the centroid bounds are min / max, here integer atomic max over
// order-preserving keys of the floats; bin counts are integer adds; nothing is summed in float across
// lanes.  The 31 plane costs per axis are then the host's own expressions over those values, and the
// partition -- the one sequential loop whose output order matters -- has a closed form (part_tables,
// part_move).  The sign of a zero can differ from the host's fold (-0 < +0 as keys, while a<b?a:b
// keeps whichever came later), and no decision sees it: comparisons treat +-0 alike, (c - lo) * scale
// truncates to bin 0 either way, lo + step * (i + 1) is the same float for lo = +-0 (step > 0), and a
// box extent of +-0 only feeds products that are compared.  The boxes the scene *stores* do not come
// from the atomics: a bottom-up pass with refit_node's rules folds them in slot order (box_level).
#pragma once
#include "rt_update.h"

namespace rt {

// A node of more than kBuildWide primitives is split by many workgroups, kBuildChunk primitives each,
// one tree level per round of launches; a subtree of at most kBuildWide primitives is built whole
// by one workgroup with an explicit stack.  A workgroup works through its subtree one node after the
// other, about 20 us each, so the subtrees are kept small: with 1024 for both constants the rebuild of
// mig29 x16 took 25.4 ms and TEAPOT-F's 18.9 ms, with these 9.3 and 2.3 ms (profiles/rebuild/).
constexpr uint32_t kBuildWide = 64;
constexpr uint32_t kBuildChunk = 256;
constexpr uint32_t kBuildStack = 72;       // the one-workgroup path's stack: it holds (depth below the root) + 1
constexpr uint32_t kBuildMaxDepth = 64;    // take_tree's limit, the reference's stack[64]
constexpr uint32_t kBuildScanRun = 64;     // boundary flags one lane sums in the renumbering's prefix count

// ---- order-preserving keys: a < b as floats <=> fkey(a) < fkey(b) (no NaN; -0 below +0)
RT_HD uint32_t fkey(float f) { const uint32_t u = fbits(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
RT_HD float unkey(uint32_t k) { return ubits((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
// An accumulator word is 0 while nothing was folded in; a maximum holds fkey, a minimum ~fkey, so one
// atomic max serves both.  dec_* fold the word into the builder's start value.
RT_HD float dec_min(uint32_t w, float init) { if (!w) return init; const float v = unkey(~w); return v < init ? v : init; }
RT_HD float dec_max(uint32_t w, float init) { if (!w) return init; const float v = unkey(w); return v > init ? v : init; }

// a node's accumulators, uint32 words: its box, its centroid bounds, per axis 32 bins of box and count
constexpr uint32_t kAccBox = 0, kAccCen = 6, kAccBin = 12, kAccCnt = kAccBin + 3 * 32 * 6, kAccRes = kAccCnt + 3 * 32;
constexpr uint32_t kAccMerge = kAccRes;        // words [0, kAccCnt) merge by max, [kAccCnt, kAccRes) by add
constexpr uint32_t kAccWords = kAccRes + 6;    // + per axis its best (cost, position)

// a node while the tree is built: its range of the index array, the left turns and the edges on its
// path from the root, and where it was split (0: a leaf so far).  The children of the node split at
// boundary b = first + left count live at 2 b and 2 b + 1: every interior node has its own b in
// [1, n - 1], so no allocation counter is shared and node 1 stays unused.
struct BNode { uint32_t first, count, ld, depth, split, pad[3]; };
// a node of the many-workgroup path during its level: its BNode, its first task and what was decided
struct WNode { uint32_t id, task0, leaf, nL, axis; float pos; uint32_t pad[2]; };
struct BTask { uint32_t wi, chunk; };

// counters (BuildArgs::ctr), zero at the start
enum { kCtrSmall = 0, kCtrMaxLeaf, kCtrDepth, kCtrErr, kCtrWideSplit, kCtrSplits, kCtrLevel = 16 };   // kCtrLevel + 2 lv: nodes, tasks of level lv
constexpr uint32_t kCtrWords = kCtrLevel + 2 * (kBuildMaxDepth + 2);
enum { kBuildErrDepth = 1u };

struct BuildArgs {
    uint32_t n;
    // in: per id the centroid; per old leaf slot the box and sticky flag; id -> old slot
    const float4 *cen, *old_box;
    const uint32_t *old_slot_of;
    const float4 *old_prims;
    // work
    uint32_t *idx, *idx2, *ptab, *qtab, *rk;   // n each: the index array, the partition's output and tables
    BNode *node;                                // 2 n + 2
    uint32_t *bflag;                            // n + 1: 1 at a split boundary; then their inclusive prefix counts
    uint32_t *csum;                             // n / kBuildScanRun + 1
    uint32_t *ctr;                              // kCtrWords
    uint32_t *wacc;                             // per node of a level kAccWords
    WNode *wnode[2];                            // the levels' nodes, alternating
    BTask *task[2];
    uint32_t *chunkL;                           // per task: its chunk's left count, then the count before it
    uint32_t *slist;                            // roots of the one-workgroup subtrees
    // out
    float4 *nodes, *prims, *slot_box;
    uint32_t *slot_of, *depth_of;               // depth_of: per final node its depth (~0u: node 1)
    float margin;
};
RT_HD uint32_t build_wide_cap(uint32_t n) { return n / kBuildWide + 2u; }
RT_HD uint32_t build_task_cap(uint32_t n) { return n / kBuildChunk + n / kBuildWide + 4u; }

// the host's lane context
struct SerialLane {
    uint32_t tid = 0, stride = 1;
    void bar() {}
    void amax(uint32_t *p, uint32_t v) { if (v > *p) *p = v; }
    uint32_t aadd(uint32_t *p, uint32_t v) { const uint32_t o = *p; *p = o + v; return o; }
};

// the part of a node one workgroup handles: positions [s0, s1) of its range [first, first + count)
struct Part { uint32_t first, count, s0, s1; };

struct ElemGeom { f3 c, mn, mx; };
RT_HD ElemGeom elem_geom(const BuildArgs &B, uint32_t id) {
    const float4 c = B.cen[id];
    const uint32_t s = B.old_slot_of[id];
    const float4 lo = B.old_box[2 * (size_t)s], hi = B.old_box[2 * (size_t)s + 1];
    ElemGeom g;
    g.c = mk(c.x, c.y, c.z);
    g.mn = mk(lo.x, lo.y, lo.z);
    g.mx = mk(hi.x, hi.y, hi.z);
    return g;
}

template <class P>
RT_HD void acc_clear(uint32_t *acc, P &par) {
    for (uint32_t i = par.tid; i < kAccWords; i += par.stride) acc[i] = 0u;
}
// words [w0, w1) of src into dst
template <class P>
RT_HD void acc_merge(uint32_t *dst, const uint32_t *src, uint32_t w0, uint32_t w1, P &par) {
    for (uint32_t i = w0 + par.tid; i < w1; i += par.stride) {
        const uint32_t v = src[i];
        if (!v) continue;
        if (i < kAccCnt) par.amax(dst + i, v);
        else par.aadd(dst + i, v);
    }
}

// UpdateNodeBounds (min of the box minima, max of the maxima) and FindBestSplitPlane's centroid bounds
template <class P>
RT_HD void acc_bounds(const BuildArgs &B, Part pt, uint32_t *acc, P &par) {
    uint32_t k[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t x = pt.s0 + par.tid; x < pt.s1; x += par.stride) {
        const ElemGeom g = elem_geom(B, B.idx[pt.first + x]);
        for (int a = 0; a < 3; ++a) {
            const uint32_t v[4] = {~fkey(comp(g.mn, a)), fkey(comp(g.mx, a)), ~fkey(comp(g.c, a)), fkey(comp(g.c, a))};
            for (int j = 0; j < 4; ++j) k[3 * j + a] = v[j] > k[3 * j + a] ? v[j] : k[3 * j + a];
        }
    }
    for (int j = 0; j < 12; ++j)
        if (k[j]) par.amax(acc + kAccBox + j, k[j]);
}
RT_HD void node_bounds(const uint32_t *acc, f3 &mn, f3 &mx) {
    mn = mk(dec_min(acc[kAccBox], 1e30f), dec_min(acc[kAccBox + 1], 1e30f), dec_min(acc[kAccBox + 2], 1e30f));
    mx = mk(dec_max(acc[kAccBox + 3], -1e30f), dec_max(acc[kAccBox + 4], -1e30f), dec_max(acc[kAccBox + 5], -1e30f));
}
// the 32 bins of each axis whose centroids differ (bounds: the accumulators acc_bounds filled)
template <class P>
RT_HD void acc_bins(const BuildArgs &B, Part pt, const uint32_t *bounds, uint32_t *acc, P &par) {
    float lo[3], scale[3];
    bool on[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = dec_min(bounds[kAccCen + a], 1e30f);
        const float hi = dec_max(bounds[kAccCen + 3 + a], -1e30f);
        on[a] = !(lo[a] == hi);
        scale[a] = 32 / (hi - lo[a]);
    }
    for (uint32_t x = pt.s0 + par.tid; x < pt.s1; x += par.stride) {
        const ElemGeom g = elem_geom(B, B.idx[pt.first + x]);
        // a bin grows by both corners (grow(bins[b], bmin); grow(bins[b], bmax))
        const f3 mn = fmin3(g.mn, g.mx), mx = fmax3(g.mn, g.mx);
        for (int a = 0; a < 3; ++a) {
            if (!on[a]) continue;
            int b = static_cast<int>((comp(g.c, a) - lo[a]) * scale[a]);
            b = b < 31 ? b : 31;
            b = b < 0 ? 0 : b;   // never on finite centroids; keeps the index inside the bins
            uint32_t *w = acc + kAccBin + 6u * (uint32_t)(a * 32 + b);
            for (int c = 0; c < 3; ++c) {
                par.amax(w + c, ~fkey(comp(mn, c)));
                par.amax(w + 3 + c, fkey(comp(mx, c)));
            }
            par.aadd(acc + kAccCnt + (uint32_t)(a * 32 + b), 1u);
        }
    }
}

struct BBox { f3 mn, mx; };
RT_HD BBox bbox_empty() { BBox b; b.mn = mk(1e34f, 1e34f, 1e34f); b.mx = mk(-1e34f, -1e34f, -1e34f); return b; }   // aabb default
RT_HD void bbox_grow(BBox &b, const BBox &o) { b.mn = fmin3(b.mn, o.mn); b.mx = fmax3(b.mx, o.mx); }
RT_HD float bbox_area(const BBox &b) {   // aabb::Area; an empty box overflows to inf
    const float e0 = b.mx.x - b.mn.x, e1 = b.mx.y - b.mn.y, e2 = b.mx.z - b.mn.z;
    return smax(0.0f, e0 * e1 + e0 * e2 + e1 * e2);
}
// FindBestSplitPlane's two sweeps and 31 costs for axis a, from best = 1e30: the first strictly
// smallest cost of the axis (an empty side's cost is NaN, never <).  res = (cost, position) bits.
RT_HD void axis_plane(const uint32_t *acc, int a, uint32_t *res) {
    float best = 1e30f, pos = 0.0f;
    const float lo = dec_min(acc[kAccCen + a], 1e30f), hi = dec_max(acc[kAccCen + 3 + a], -1e30f);
    if (!(lo == hi)) {
        float la[31], ra[31];
        uint32_t lc[31], rc[31];
        BBox L = bbox_empty(), R = bbox_empty();
        uint32_t ls = 0, rs = 0;
        for (int i = 0; i < 31; ++i) {
            for (int side = 0; side < 2; ++side) {
                const uint32_t b = (uint32_t)(a * 32 + (side ? 31 - i : i));
                const uint32_t *w = acc + kAccBin + 6u * b;
                BBox bin;
                bin.mn = mk(dec_min(w[0], 1e34f), dec_min(w[1], 1e34f), dec_min(w[2], 1e34f));
                bin.mx = mk(dec_max(w[3], -1e34f), dec_max(w[4], -1e34f), dec_max(w[5], -1e34f));
                if (!side) { ls += acc[kAccCnt + b]; lc[i] = ls; bbox_grow(L, bin); la[i] = bbox_area(L); }
                else { rs += acc[kAccCnt + b]; rc[30 - i] = rs; bbox_grow(R, bin); ra[30 - i] = bbox_area(R); }
            }
        }
        const float step = (hi - lo) / 32;
        for (int i = 0; i < 31; ++i) {
            const float cost = (float)(int)lc[i] * la[i] + (float)(int)rc[i] * ra[i];
            if (cost < best) { pos = lo + step * (float)(i + 1); best = cost; }
        }
    }
    res[2 * a] = fbits(best);
    res[2 * a + 1] = fbits(pos);
}
struct Plane { float cost, pos; int axis; };
// axis-major, strict <: an axis takes over only where its best beats every earlier axis's
RT_HD Plane best_plane(const uint32_t *res) {
    Plane p;
    p.cost = 1e30f; p.pos = 0.0f; p.axis = 0;
    for (int a = 0; a < 3; ++a) {
        const float c = ubits(res[2 * a]);
        if (c < p.cost) { p.cost = c; p.pos = ubits(res[2 * a + 1]); p.axis = a; }
    }
    return p;
}
// Subdivide's first abort: splitting is no cheaper than the node as a leaf
RT_HD bool plane_aborts(const uint32_t *acc, uint32_t count, float cost) {
    f3 mn, mx;
    node_bounds(acc, mn, mx);
    const float ex = mx.x - mn.x, ey = mx.y - mn.y, ez = mx.z - mn.z;
    return cost >= (float)count * (ex * ey + ey * ez + ez * ex);
}

// inclusive-to-exclusive prefix count over the lanes of a workgroup (buf: stride words); total: all lanes'
template <class P>
RT_HD uint32_t wg_scan(uint32_t *buf, uint32_t v, uint32_t &total, P &par) {
    buf[par.tid] = v;
    par.bar();
    for (uint32_t off = 1; off < par.stride; off <<= 1) {
        const uint32_t t = par.tid >= off ? buf[par.tid - off] : 0u;
        par.bar();
        buf[par.tid] += t;
        par.bar();
    }
    total = buf[par.stride - 1];
    const uint32_t incl = buf[par.tid];
    par.bar();
    return incl - v;
}

// ---- the partition.  The reference's loop (scene.h:878-886)
//     while (i <= j) if (centroid[axis] < pos) ++i; else swap(ix[i], ix[j--]);
// as a map from positions to positions.  With flags L (centroid < pos) / R over positions 0 .. n - 1,
// nL = #L, front F = [0, nL), back B = [nL, n), p_1 < ... < p_m the R positions in F, q_1 > ... > q_m
// the L positions in B (as many), q_0 = n:
//   an L in F stays; the L at q_k goes to p_k; the R at p_k goes to q_(k-1) - 1;
//   an R in B at x goes to x - 1, but the R at position nL (if one is there) goes to q_m - 1.
// Checked against the loop for every flag string up to length 16 (tests/cpp/build_host.cpp).
// Every lane takes a run of consecutive positions, so three prefix counts place an element.
RT_HD void part_run(Part pt, uint32_t tid, uint32_t stride, uint32_t &r0, uint32_t &r1) {
    const uint32_t len = pt.s1 - pt.s0, per = (len + stride - 1u) / stride;
    r0 = pt.s0 + tid * per;
    r0 = r0 < pt.s1 ? r0 : pt.s1;
    r1 = r0 + per < pt.s1 ? r0 + per : pt.s1;
}
RT_HD bool elem_left(const BuildArgs &B, uint32_t slot, int axis, float pos) {
    const float4 c = B.cen[B.idx[slot]];
    return comp(mk(c.x, c.y, c.z), axis) < pos;
}
// the L's before this lane's run within the part, and the part's total
template <class P>
RT_HD uint32_t part_count(const BuildArgs &B, Part pt, int axis, float pos, uint32_t *scan, uint32_t &total, P &par) {
    uint32_t r0, r1, c = 0;
    part_run(pt, par.tid, par.stride, r0, r1);
    for (uint32_t x = r0; x < r1; ++x) c += elem_left(B, pt.first + x, axis, pos) ? 1u : 0u;
    return wg_scan(scan, c, total, par);
}
// per position its flag and the L's before it (rk), and the tables p_k (ptab[first + k - 1]) and
// q_k (qtab[first + k - 1]); before = the L's of the node before this lane's run
template <class P>
RT_HD void part_tables(const BuildArgs &B, Part pt, int axis, float pos, uint32_t before, uint32_t nL, P &par) {
    uint32_t r0, r1, pl = before;
    part_run(pt, par.tid, par.stride, r0, r1);
    for (uint32_t x = r0; x < r1; ++x) {
        const bool L = elem_left(B, pt.first + x, axis, pos);
        B.rk[pt.first + x] = pl | (L ? 0x80000000u : 0u);
        if (x < nL) {
            if (!L) B.ptab[pt.first + (x + 1u - pl) - 1u] = x;   // the k-th R of F, k = x + 1 - pl
        } else if (L) {
            B.qtab[pt.first + (nL - pl) - 1u] = x;               // the k-th L of B from the end, k = nL - pl
        }
        pl += L ? 1u : 0u;
    }
}
template <class P>
RT_HD void part_move(const BuildArgs &B, Part pt, uint32_t nL, P &par) {
    for (uint32_t x = pt.s0 + par.tid; x < pt.s1; x += par.stride) {
        const uint32_t r = B.rk[pt.first + x], pl = r & 0x7fffffffu;
        const bool L = (r >> 31) != 0u;
        uint32_t dest;
        if (x < nL) {
            if (L) dest = x;
            else {
                const uint32_t k = x + 1u - pl;
                dest = (k == 1u ? pt.count : B.qtab[pt.first + k - 2u]) - 1u;
            }
        } else if (L) {
            dest = B.ptab[pt.first + (nL - pl) - 1u];
        } else if (x == nL) {
            const uint32_t m = nL - pl;   // pl = the L's of F here
            dest = (m == 0u ? pt.count : B.qtab[pt.first + m - 1u]) - 1u;
        } else {
            dest = x - 1u;
        }
        B.idx2[pt.first + dest] = B.idx[pt.first + x];
    }
}
template <class P>
RT_HD void part_copy_back(const BuildArgs &B, Part pt, P &par) {
    for (uint32_t x = pt.s0 + par.tid; x < pt.s1; x += par.stride) B.idx[pt.first + x] = B.idx2[pt.first + x];
}

// ---- the tree
// a new node goes to the next level's many-workgroup list (with one task per chunk) or to the roots
// of the one-workgroup subtrees; one lane
template <class P>
RT_HD void dispatch_node(const BuildArgs &B, uint32_t id, uint32_t lv, P &par) {
    const uint32_t count = B.node[id].count;
    if (count > kBuildWide) {
        const uint32_t wi = par.aadd(B.ctr + kCtrLevel + 2u * lv, 1u), nch = (count + kBuildChunk - 1u) / kBuildChunk;
        const uint32_t t0 = par.aadd(B.ctr + kCtrLevel + 2u * lv + 1u, nch);
        WNode w{};
        w.id = id;
        w.task0 = t0;
        B.wnode[lv & 1u][wi] = w;
        for (uint32_t j = 0; j < nch; ++j) {
            BTask t;
            t.wi = wi; t.chunk = j;
            B.task[lv & 1u][t0 + j] = t;
        }
    } else {
        B.slist[par.aadd(B.ctr + kCtrSmall, 1u)] = id;
    }
}
// the two children of node id, split with nL on the left (0 < nL < count); one lane.  Returns the left child.
template <class P>
RT_HD uint32_t make_children(const BuildArgs &B, uint32_t id, uint32_t nL, P &par) {
    const BNode nd = B.node[id];
    const uint32_t b = nd.first + nL;
    BNode l{}, r{};
    l.first = nd.first; l.count = nL; l.ld = nd.ld + 1u; l.depth = nd.depth + 1u;
    r.first = b; r.count = nd.count - nL; r.ld = nd.ld; r.depth = nd.depth + 1u;
    B.node[2 * (size_t)b] = l;
    B.node[2 * (size_t)b + 1] = r;
    B.node[id].split = b;
    B.bflag[b] = 1u;
    if (nd.depth + 1u > kBuildMaxDepth) par.amax(B.ctr + kCtrErr, (uint32_t)kBuildErrDepth);
    return 2u * b;
}
// the start: the identity index array; the root (one lane)
template <class P>
RT_HD void build_init(const BuildArgs &B, uint32_t gtid, uint32_t gstride, P &par) {
    for (uint32_t i = gtid; i < B.n; i += gstride) B.idx[i] = i;
    if (gtid == 0) {
        BNode root{};
        root.count = B.n;
        B.node[0] = root;
        dispatch_node(B, 0u, 0u, par);
    }
}

// ---- the many-workgroup path: one level is the steps w1 .. w7 over its tasks, a launch each
RT_HD Part wide_part(const BuildArgs &B, uint32_t lv, uint32_t g, uint32_t &wi) {
    const BTask t = B.task[lv & 1u][g];
    wi = t.wi;
    const BNode nd = B.node[B.wnode[lv & 1u][wi].id];
    Part pt;
    pt.first = nd.first; pt.count = nd.count;
    pt.s0 = t.chunk * kBuildChunk;
    pt.s1 = pt.s0 + kBuildChunk < nd.count ? pt.s0 + kBuildChunk : nd.count;
    return pt;
}
// acc: the workgroup's own accumulators (LDS), merged into the node's
template <class P>
RT_HD void wide_bounds(const BuildArgs &B, uint32_t lv, uint32_t g, uint32_t *acc, P &par) {
    uint32_t wi;
    const Part pt = wide_part(B, lv, g, wi);
    acc_clear(acc, par);
    par.bar();
    acc_bounds(B, pt, acc, par);
    par.bar();
    acc_merge(B.wacc + (size_t)wi * kAccWords, acc, kAccBox, kAccBin, par);
}
template <class P>
RT_HD void wide_bins(const BuildArgs &B, uint32_t lv, uint32_t g, uint32_t *acc, P &par) {
    uint32_t wi;
    const Part pt = wide_part(B, lv, g, wi);
    acc_clear(acc, par);
    par.bar();
    acc_bins(B, pt, B.wacc + (size_t)wi * kAccWords, acc, par);
    par.bar();
    acc_merge(B.wacc + (size_t)wi * kAccWords, acc, kAccBin, kAccMerge, par);
}
// every workgroup of a node finds the node's plane (the same values, the same result); chunk 0 records it
template <class P>
RT_HD void wide_plane_count(const BuildArgs &B, uint32_t lv, uint32_t g, uint32_t *acc, uint32_t *scan, P &par) {
    uint32_t wi;
    const Part pt = wide_part(B, lv, g, wi);
    const uint32_t *node_acc = B.wacc + (size_t)wi * kAccWords;
    for (uint32_t a = par.tid; a < 3u; a += par.stride) axis_plane(node_acc, (int)a, acc + kAccRes);
    par.bar();
    const Plane pl = best_plane(acc + kAccRes);
    const bool leaf = plane_aborts(node_acc, pt.count, pl.cost);
    WNode *w = B.wnode[lv & 1u] + wi;
    if (pt.s0 == 0u && par.tid == 0u) {
        w->leaf = leaf ? 1u : 0u;
        w->axis = (uint32_t)pl.axis;
        w->pos = pl.pos;
    }
    if (leaf) return;
    uint32_t total;
    part_count(B, pt, pl.axis, pl.pos, scan, total, par);
    if (par.tid == 0u) B.chunkL[g] = total;
}
// one lane per node of the level: the chunks' left counts become the counts before them; the children
template <class P>
RT_HD void wide_settle(const BuildArgs &B, uint32_t lv, uint32_t wi, P &par) {
    WNode *w = B.wnode[lv & 1u] + wi;
    if (w->leaf) return;
    const BNode nd = B.node[w->id];
    const uint32_t nch = (nd.count + kBuildChunk - 1u) / kBuildChunk;
    uint32_t run = 0;
    for (uint32_t j = 0; j < nch; ++j) {
        const uint32_t c = B.chunkL[w->task0 + j];
        B.chunkL[w->task0 + j] = run;
        run += c;
    }
    w->nL = run;
    if (run == 0u || run == nd.count) return;   // Subdivide's second abort; the range is reordered all the same
    const uint32_t l = make_children(B, w->id, run, par);
    par.aadd(B.ctr + kCtrWideSplit, 1u);
    dispatch_node(B, l, lv + 1u, par);
    dispatch_node(B, l + 1u, lv + 1u, par);
}
template <class P>
RT_HD void wide_tables(const BuildArgs &B, uint32_t lv, uint32_t g, uint32_t *scan, P &par) {
    uint32_t wi;
    const Part pt = wide_part(B, lv, g, wi);
    const WNode w = B.wnode[lv & 1u][wi];
    if (w.leaf) return;
    uint32_t total;
    const uint32_t before = part_count(B, pt, (int)w.axis, w.pos, scan, total, par);
    part_tables(B, pt, (int)w.axis, w.pos, B.chunkL[g] + before, w.nL, par);
}
template <class P>
RT_HD void wide_move(const BuildArgs &B, uint32_t lv, uint32_t g, P &par) {
    uint32_t wi;
    const Part pt = wide_part(B, lv, g, wi);
    const WNode w = B.wnode[lv & 1u][wi];
    if (!w.leaf) part_move(B, pt, w.nL, par);
}
template <class P>
RT_HD void wide_copy_back(const BuildArgs &B, uint32_t lv, uint32_t g, P &par) {
    uint32_t wi;
    const Part pt = wide_part(B, lv, g, wi);
    if (!B.wnode[lv & 1u][wi].leaf) part_copy_back(B, pt, par);
}

// ---- the one-workgroup path: the whole recursion under root, depth first, left child first.
// acc (kAccWords), scan (stride words) and stack (kBuildStack words) are the workgroup's own.  Every
// lane takes the same branches: what they depend on is read from acc / stack after a barrier.
template <class P>
RT_HD void build_subtree(const BuildArgs &B, uint32_t root, uint32_t *acc, uint32_t *scan, uint32_t *stack, P &par) {
    uint32_t sp = 1;
    if (par.tid == 0u) stack[0] = root;
    for (;;) {
        par.bar();   // the stack's last pushes; the last node's reads of acc
        if (sp == 0u) return;
        const uint32_t id = stack[--sp];
        const BNode nd = B.node[id];
        Part pt;
        pt.first = nd.first; pt.count = nd.count; pt.s0 = 0u; pt.s1 = nd.count;
        par.bar();
        acc_clear(acc, par);
        par.bar();
        acc_bounds(B, pt, acc, par);
        par.bar();
        acc_bins(B, pt, acc, acc, par);
        par.bar();
        for (uint32_t a = par.tid; a < 3u; a += par.stride) axis_plane(acc, (int)a, acc + kAccRes);
        par.bar();
        const Plane pl = best_plane(acc + kAccRes);
        if (plane_aborts(acc, nd.count, pl.cost)) continue;
        uint32_t nL;
        const uint32_t before = part_count(B, pt, pl.axis, pl.pos, scan, nL, par);
        part_tables(B, pt, pl.axis, pl.pos, before, nL, par);
        par.bar();
        part_move(B, pt, nL, par);
        par.bar();
        part_copy_back(B, pt, par);
        if (nL == 0u || nL == nd.count) continue;
        if (sp + 2u > kBuildStack) {   // deeper than any tree the kernels take
            if (par.tid == 0u) par.amax(B.ctr + kCtrErr, (uint32_t)kBuildErrDepth);
            return;
        }
        if (par.tid == 0u) {
            const uint32_t l = make_children(B, id, nL, par);
            stack[sp] = l + 1u;
            stack[sp + 1u] = l;
        }
        sp += 2u;
    }
}

// ---- numbering.  The host hands out child pairs in the recursion's pre-order: a node's pair is
// 2 + 2 I, I = the interior nodes before it in pre-order = the split boundaries at or below its first
// position (the nodes left of it, and the ancestors it hangs to the right of) + the left turns on its
// path (the ancestors it hangs to the left of).  So one prefix count over the boundary flags numbers
// every node on its own.  Three steps: runs, their sums (one lane), the counts in place.
RT_HD uint32_t scan_runs(uint32_t n) { return (n + 1u + kBuildScanRun - 1u) / kBuildScanRun; }
RT_HD void scan_sum(const BuildArgs &B, uint32_t gtid, uint32_t gstride) {
    for (uint32_t c = gtid; c < scan_runs(B.n); c += gstride) {
        uint32_t s = 0;
        for (uint32_t i = c * kBuildScanRun; i < (c + 1u) * kBuildScanRun && i <= B.n; ++i) s += B.bflag[i];
        B.csum[c] = s;
    }
}
RT_HD void scan_top(const BuildArgs &B) {
    uint32_t run = 0;
    for (uint32_t c = 0; c < scan_runs(B.n); ++c) { const uint32_t s = B.csum[c]; B.csum[c] = run; run += s; }
    B.ctr[kCtrSplits] = run;
}
RT_HD void scan_apply(const BuildArgs &B, uint32_t gtid, uint32_t gstride) {
    for (uint32_t c = gtid; c < scan_runs(B.n); c += gstride) {
        uint32_t run = B.csum[c];
        for (uint32_t i = c * kBuildScanRun; i < (c + 1u) * kBuildScanRun && i <= B.n; ++i) { run += B.bflag[i]; B.bflag[i] = run; }
    }
}
RT_HD uint32_t pair_of(const BuildArgs &B, const BNode &nd) { return 2u + 2u * (B.bflag[nd.first] + nd.ld); }
// node t of the build becomes node f of the tree: its word (the box comes with box_level), its
// depth, and for a leaf the tree's widest leaf and depth (Scene::maxDepthBVH: a root leaf counts 1)
template <class P>
RT_HD void emit_node(const BuildArgs &B, uint32_t t, uint32_t f, P &par) {
    const BNode nd = B.node[t];
    // a leaf wider than 255 does not fit its word; the tree is refused before anything reads it
    const uint32_t word = nd.split ? node_word(pair_of(B, nd), 0u) : node_word(nd.first, nd.count & 255u);
    node_pack(mk(0, 0, 0), mk(0, 0, 0), word, 0.0f, B.nodes + 2 * (size_t)f);
    B.depth_of[f] = nd.depth;
    if (!nd.split) {
        par.amax(B.ctr + kCtrMaxLeaf, nd.count);
        par.amax(B.ctr + kCtrDepth, f == 0u ? 1u : nd.depth);
    }
}
// lane b: the root and the unused node 1 (b = 0), the two children of the node split at b
template <class P>
RT_HD void emit_nodes(const BuildArgs &B, uint32_t gtid, uint32_t gstride, P &par) {
    for (uint32_t b = gtid; b < B.n; b += gstride) {
        if (b == 0u) {
            emit_node(B, 0u, 0u, par);
            node_pack(mk(0, 0, 0), mk(0, 0, 0), 0u, walk_word(false, B.margin), B.nodes + 2);
            B.depth_of[1] = ~0u;
        } else if (B.bflag[b] != B.bflag[b - 1u]) {
            const uint32_t pair = pair_of(B, B.node[2 * (size_t)b]) - 2u;   // the left child's I is its parent's + 1
            emit_node(B, 2u * b, pair, par);
            emit_node(B, 2u * b + 1u, pair + 1u, par);
        }
    }
}
// the leaf-slot records and slot boxes in the new slot order, and the new slot of every id
RT_HD void permute_slots(const BuildArgs &B, uint32_t gtid, uint32_t gstride) {
    for (uint32_t k = gtid; k < B.n; k += gstride) {
        const uint32_t id = B.idx[k], o = B.old_slot_of[id];
        for (int j = 0; j < 3; ++j) B.prims[3 * (size_t)k + j] = B.old_prims[3 * (size_t)o + j];
        for (int j = 0; j < 2; ++j) B.slot_box[2 * (size_t)k + j] = B.old_box[2 * (size_t)o + j];
        B.slot_of[id] = k;
    }
}
// the stored boxes and sticky words, bottom up: every node of depth d by refit_node's rules (a leaf
// folds its slots' boxes in slot order, an interior node takes tmin / tmax of its children and the OR
// of their sticky bits); the depths run from the deepest to 0 with a launch boundary between them
RT_HD void box_level(const BuildArgs &B, uint32_t nodes_used, uint32_t d, uint32_t gtid, uint32_t gstride) {
    RefitArgs A{};
    A.nodes = B.nodes;
    A.slot_box = B.slot_box;
    A.margin = B.margin;
    for (uint32_t k = gtid; k < nodes_used; k += gstride)
        if (B.depth_of[k] == d) refit_node(A, k);
}

// ---- the array sizes, in elements: the work arrays (A: anything with take<T>(count) -- the device
// carves one allocation, the host programs give every array a heap block of its own) and the outputs
template <class A>
void build_carve(A &a, uint32_t n, BuildArgs &B) {
    B.idx2 = a.template take<uint32_t>(n);
    B.ptab = a.template take<uint32_t>(n);
    B.qtab = a.template take<uint32_t>(n);
    B.rk = a.template take<uint32_t>(n);
    B.node = a.template take<BNode>(2 * (size_t)n + 2);
    B.bflag = a.template take<uint32_t>((size_t)n + 1);
    B.csum = a.template take<uint32_t>(scan_runs(n) + 1u);
    B.ctr = a.template take<uint32_t>(kCtrWords);
    B.wacc = a.template take<uint32_t>((size_t)build_wide_cap(n) * kAccWords);
    for (int k = 0; k < 2; ++k) {
        B.wnode[k] = a.template take<WNode>(build_wide_cap(n));
        B.task[k] = a.template take<BTask>(build_task_cap(n));
    }
    B.chunkL = a.template take<uint32_t>(build_task_cap(n));
    B.slist = a.template take<uint32_t>((size_t)n + 1);
    B.depth_of = a.template take<uint32_t>(2 * (size_t)n + 2);
}
inline size_t build_nodes_len(uint32_t n) { return 2 * (2 * (size_t)n + 2); }   // float4: BuildArgs::nodes
inline size_t build_prims_len(uint32_t n) { return 3 * (size_t)n; }             // float4: prims
inline size_t build_slot_box_len(uint32_t n) { return 2 * (size_t)n; }          // float4: slot_box
inline size_t build_ids_len(uint32_t n) { return n; }                           // uint32: slot_of, idx

// ---- the launch order.  A step is one kernel of rt_build.hip, or on the host a loop over its workgroups:
//   kStepInit                    the identity index array, the root
//   per level of the many-workgroup path (nodes of more than kBuildWide primitives, a workgroup per
//   kBuildChunk primitives):
//     kStepWideBounds, -Bins         node box, centroid bounds, bins: LDS accumulators merged into the node's
//     kStepWidePlane                 the plane, the cost abort, the chunk's left count
//     kStepWideSettle                per node: the chunk counts' prefix, the children, the next level's tasks
//     kStepWideTables, -Move, -Back  the partition
//   kStepSubtrees                one workgroup per subtree of at most kBuildWide primitives, explicit stack
//   kStepScanSum / -Top / -Apply the prefix count over the split boundaries that numbers the nodes
//   kStepEmit                    node words in the host's numbering, depths, widest leaf
//   kStepPermute                 leaf-slot records, slot boxes and the slot map in the new order
//   kStepBoxes                   per depth, deepest first: stored boxes and sticky words (refit_node)
// Nothing is handed from one workgroup to another inside a launch -- no flags, no spins, no fences
// (the rule of rt_refit.hip): launch boundaries order the steps of a level and the levels, and
// __syncthreads() orders the steps inside a workgroup, whose waves share their CU's vector L1.
// The launches of the level loop are bounded by the depth limit: kBuildMaxDepth + 1 levels.
enum BuildStep {
    kStepInit, kStepWideBounds, kStepWideBins, kStepWidePlane, kStepWideSettle, kStepWideTables, kStepWideMove, kStepWideBack,
    kStepSubtrees, kStepScanSum, kStepScanTop, kStepScanApply, kStepEmit, kStepPermute, kStepBoxes
};
// what build_order returns: kBuildOk, the executor's own failure, or the refusal
enum { kBuildOk = 0, kBuildExec, kBuildLevels, kBuildTableOverrun, kBuildListOverrun, kBuildDeep, kBuildWideLeaf, kBuildNodes };
struct BuildFigures { uint32_t nodes_used, depth, max_leaf, levels, wide_splits, subtrees, launches; };

// The executor X runs the steps where the arrays live; each method returns false on a failure of its own:
//   zero(ptr, words)          uint32 words to 0
//   read(dst, src, words)     uint32 words of an array to the host, after every step before it
//   step(BuildStep, count, arg)
//       count: the lanes of a per-element step (Init, WideSettle, Scan*, Emit, Permute, Boxes), the
//       workgroups of a per-workgroup step; arg: the level of a Wide step, the depth of Boxes
// Plain C++: no HIP, no std:: algorithm.
template <class X>
int build_order(X &x, const BuildArgs &B, BuildFigures &f) {
    const uint32_t n = B.n;
    f = BuildFigures{};
    if (!x.zero(B.ctr, kCtrWords) || !x.zero(B.bflag, (size_t)n + 1)) return kBuildExec;
    if (!x.step(kStepInit, n, 0u)) return kBuildExec;
    ++f.launches;
    uint32_t lvl[2] = {0, 0};   // nodes and tasks of the level
    if (!x.read(lvl, B.ctr + kCtrLevel, 2)) return kBuildExec;
    for (uint32_t lv = 0; lvl[0] > 0; ++lv) {
        if (lv > kBuildMaxDepth) return kBuildLevels;
        if (lvl[0] > build_wide_cap(n) || lvl[1] > build_task_cap(n)) return kBuildTableOverrun;
        if (!x.zero(B.wacc, kAccWords * (size_t)lvl[0])) return kBuildExec;
        if (!x.step(kStepWideBounds, lvl[1], lv) || !x.step(kStepWideBins, lvl[1], lv) || !x.step(kStepWidePlane, lvl[1], lv) ||
            !x.step(kStepWideSettle, lvl[0], lv) || !x.step(kStepWideTables, lvl[1], lv) || !x.step(kStepWideMove, lvl[1], lv) ||
            !x.step(kStepWideBack, lvl[1], lv))
            return kBuildExec;
        f.launches += 7;
        ++f.levels;
        if (!x.read(lvl, B.ctr + kCtrLevel + 2u * (lv + 1u), 2)) return kBuildExec;
    }
    uint32_t ctr[kCtrLevel];
    if (!x.read(ctr, B.ctr, kCtrLevel)) return kBuildExec;
    f.subtrees = ctr[kCtrSmall];
    if (f.subtrees > n) return kBuildListOverrun;
    if (f.subtrees) {
        if (!x.step(kStepSubtrees, f.subtrees, 0u)) return kBuildExec;
        ++f.launches;
    }
    if (!x.step(kStepScanSum, scan_runs(n), 0u) || !x.step(kStepScanTop, 1u, 0u) || !x.step(kStepScanApply, scan_runs(n), 0u) ||
        !x.step(kStepEmit, n, 0u))
        return kBuildExec;
    f.launches += 4;
    if (!x.read(ctr, B.ctr, kCtrLevel)) return kBuildExec;
    // take_tree's limits, before anything reads the new node words
    f.nodes_used = 2u + 2u * ctr[kCtrSplits];
    f.depth = ctr[kCtrDepth];
    f.max_leaf = ctr[kCtrMaxLeaf];
    f.wide_splits = ctr[kCtrWideSplit];
    if ((ctr[kCtrErr] & kBuildErrDepth) || f.depth > kBuildMaxDepth) return kBuildDeep;
    if (f.max_leaf > 255) return kBuildWideLeaf;
    if (f.nodes_used > (1u << 24)) return kBuildNodes;
    if (!x.step(kStepPermute, n, 0u)) return kBuildExec;
    ++f.launches;
    for (uint32_t d = f.depth + 1u; d-- > 0u;) {
        if (!x.step(kStepBoxes, f.nodes_used, d)) return kBuildExec;
        ++f.launches;
    }
    return kBuildOk;
}

}  // namespace rt
