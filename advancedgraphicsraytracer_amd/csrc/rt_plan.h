// rt_plan.h -- the text of the GPU refit schedule: RefitPlan's list / lvl / grp
// (rt_refit.h) from the device node array alone, word for word what build_refit_plan
// (rt_scene_pack.cpp) makes of the same tree on the host.
//
// One text for gfx950 and for the host, like rt_build.h: the kernels of rt_plan.hip supply the lane
// context -- tid, stride, bar, integer aadd -- and tests/cpp/plan_host.cpp runs the same steps with
// SerialLane.  The order of the steps (plan_order) and the sizes of the arrays (plan_carve,
// plan_*_len) are here too, once for both.  No std:: algorithm, no HIP call, integer work only.
//
// Why integer prefix counts reproduce the host's stable_sort.  The host walks the tree in pre-order
// (walk_tree's `order`), hands every maximal subtree of at most kTreeletNodes nodes -- a treelet, a
// contiguous run of `order` that starts at its root -- to emit(), which sorts the run stably by
// height, and emits the remaining nodes, the top, the same way at the end.  A stable sort by a key
// puts an element at (elements of a smaller key) + (earlier elements of the same key): two counts
// that no order of evaluation changes.  And a node's place in `order` is a count too:
// rank(root) = 0, rank(left) = rank(parent) + 1, rank(right) = rank(parent) + 1 + size(left).  So
// every word of the schedule is a sum of integers over a fixed set, and many lanes write what the
// host's loop writes.
#pragma once
#include "rt_build.h"
#include "rt_refit.h"

namespace rt {

// A tree of at most kPlanSmall nodes runs every step in ONE launch of one workgroup, with bar()
// where the many-launch order has a launch boundary (the waves of a workgroup share their CU's L1:
// rt_refit.hip).  Not derived, measured (tools/plan_time.py's soups, prepare_updates after a rebuild,
// DESIGN 4.12): with 4,096 the one workgroup took 0.15 / 0.23 / 0.39 ms at 1,000 / 2,000 / 4,000 nodes
// -- about 0.07 ms + 0.08 ms per 1,000 nodes, every pass a round trip to memory -- and the launches
// 0.27 ms at 4,120, 4,400 and 8,000 nodes (49-52 launches), so the routes cross near 2,500 nodes;
// 2,048 is two nodes per lane of the 1,024-lane workgroup and keeps TEAPOT-F (2,040) on one launch.
constexpr uint32_t kPlanSmall = 2048;
constexpr uint32_t kPlanMaxDepth = 64;      // take_tree's limit: the level loops run at most this often
constexpr uint32_t kPlanHeights = 66;       // heights 0 .. 64 and one spare word
constexpr uint32_t kPlanScanRun = 16;       // rank positions one lane sums in the prefix counts
constexpr uint32_t kPlanBatch = 4;          // nodes a lane takes per turn of a level step, their loads issued together
constexpr uint32_t kPlanTopChunk = 64;      // top nodes the one workgroup of plan_top places per pass: a wave's worth
constexpr uint32_t kPlanLds = 1024;         // uint32 words of workgroup memory any step uses (wg_scan: one per lane)
constexpr uint32_t kPlanSmallLanes = 1024;  // the one workgroup of the small route

// counters (PlanArgs::ctr)
enum { kPcTreelets = 0, kPcTop, kPcLvlSum, kPcSeen, kPcRootSize, kPcListLen, kPcLvlLen, kPcWords = 8 };

struct PlanArgs {
    // in: the device node array as the frames read it (the word at [2 i + 1].z, node 1 unused),
    // nodes_used and the tree's depth (Scene::maxDepthBVH: the deepest leaf; a root leaf counts 1)
    const float4 *nodes;
    uint32_t used, depth;
    // work, `used` words each: per node its depth (~0u: not reached from the root), parent, subtree
    // size, height above its deepest leaf and pre-order rank; the node of every rank
    uint32_t *depth_of, *parent, *size, *height, *rank, *by_rank;
    uint32_t *cw;                     // per rank its class word (plan_classify)
    uint32_t *csum;                   // 4 per run of kPlanScanRun rank positions
    uint32_t *troot, *tlist, *topc;   // per treelet its root and its first list entry; the top nodes in rank order
    uint32_t *ctr;                    // kPcWords
    // out
    uint32_t *list, *lvl, *grp;
};
RT_HD uint32_t plan_runs(uint32_t used) { return (used + kPlanScanRun - 1u) / kPlanScanRun; }
// workgroups of the treelet step: each takes treelets wg, wg + count, ... (their number is known
// only on the device, and the one read-back is at the end)
RT_HD uint32_t plan_treelet_wgs(uint32_t used) { const uint32_t w = used / 64u + 1u; return w < 1024u ? w : 1024u; }

RT_HD uint32_t plan_word(const PlanArgs &A, uint32_t k) { return fbits(A.nodes[2 * (size_t)k + 1].z); }
// the left child of interior node k, or 0 for a leaf and for a pair outside the array (no validated tree has one)
RT_HD uint32_t plan_left(const PlanArgs &A, uint32_t k) {
    const uint32_t w = plan_word(A, k), l = w >> 8;
    return ((w & 255u) == 0u && l >= 2u && l + 1u < A.used) ? l : 0u;
}
RT_HD uint32_t plan_height(const PlanArgs &A, uint32_t k) {
    const uint32_t h = k < A.used ? A.height[k] : 0u;
    return h < kPlanMaxDepth ? h : kPlanMaxDepth;
}
// the cut: 2 above it (a subtree of more than kTreeletNodes nodes), 1 a treelet's root, 0 inside a treelet
RT_HD uint32_t plan_class(const PlanArgs &A, uint32_t k) {
    if (A.size[k] > kTreeletNodes) return 2u;
    return (k == 0u || A.size[A.parent[k]] > kTreeletNodes) ? 1u : 0u;
}

// ---- the per-node steps: lanes gtid, gtid + gstride, ... over all nodes, as box_level strides
RT_HD void plan_init(const PlanArgs &A, uint32_t gtid, uint32_t gstride) {
    for (uint32_t k = gtid; k < A.used; k += gstride) {
        A.depth_of[k] = k == 0u ? 0u : ~0u;
        A.parent[k] = ~0u;
        A.size[k] = 1u;      // a leaf's; plan_up gives the interior nodes theirs
        A.height[k] = 0u;
        A.rank[k] = 0u;
        A.by_rank[k] = k == 0u ? 0u : ~0u;
    }
}
// A level step takes the nodes of one depth.  A lane's turn is kPlanBatch nodes (k0, k0 + gstride, ...):
// first every load of the turn, then its stores, so the loads' latencies overlap -- in the
// one-workgroup route a lane has several nodes, and a pass costs one round trip, not one per node.
// l[q]: the left child of the turn's q-th node where that node is interior and of depth d, else 0.
RT_HD void plan_level_nodes(const PlanArgs &A, uint32_t d, uint32_t k0, uint32_t gstride, uint32_t l[kPlanBatch]) {
    uint32_t dep[kPlanBatch];
    for (uint32_t q = 0; q < kPlanBatch; ++q) {
        const uint32_t k = k0 + q * gstride;
        dep[q] = k < A.used ? A.depth_of[k] : ~0u;
    }
    for (uint32_t q = 0; q < kPlanBatch; ++q) l[q] = dep[q] == d ? plan_left(A, k0 + q * gstride) : 0u;
}
// top down: an interior node of depth d gives its children their depth and parent
RT_HD void plan_down(const PlanArgs &A, uint32_t d, uint32_t gtid, uint32_t gstride) {
    for (uint32_t k0 = gtid; k0 < A.used; k0 += kPlanBatch * gstride) {
        uint32_t l[kPlanBatch];
        plan_level_nodes(A, d, k0, gstride, l);
        for (uint32_t q = 0; q < kPlanBatch; ++q) {
            if (!l[q]) continue;
            A.depth_of[l[q]] = A.depth_of[l[q] + 1u] = d + 1u;
            A.parent[l[q]] = A.parent[l[q] + 1u] = k0 + q * gstride;
        }
    }
}
// bottom up: size = 1 + size(l) + size(l + 1), height = 1 + max(height(l), height(l + 1))
RT_HD void plan_up(const PlanArgs &A, uint32_t d, uint32_t gtid, uint32_t gstride) {
    for (uint32_t k0 = gtid; k0 < A.used; k0 += kPlanBatch * gstride) {
        uint32_t l[kPlanBatch], sz[kPlanBatch], h[kPlanBatch];
        plan_level_nodes(A, d, k0, gstride, l);
        for (uint32_t q = 0; q < kPlanBatch; ++q) {
            if (!l[q]) continue;
            const uint32_t hl = A.height[l[q]], hr = A.height[l[q] + 1u];
            sz[q] = 1u + A.size[l[q]] + A.size[l[q] + 1u];
            h[q] = 1u + (hl > hr ? hl : hr);
        }
        for (uint32_t q = 0; q < kPlanBatch; ++q) {
            if (!l[q]) continue;
            A.size[k0 + q * gstride] = sz[q];
            A.height[k0 + q * gstride] = h[q];
        }
    }
}
// top down again: the pre-order rank of the children, and the node of every rank (walk_tree's order)
RT_HD void plan_rank(const PlanArgs &A, uint32_t d, uint32_t gtid, uint32_t gstride) {
    for (uint32_t k0 = gtid; k0 < A.used; k0 += kPlanBatch * gstride) {
        uint32_t l[kPlanBatch], rl[kPlanBatch], rr[kPlanBatch];
        plan_level_nodes(A, d, k0, gstride, l);
        for (uint32_t q = 0; q < kPlanBatch; ++q) {
            if (!l[q]) continue;
            rl[q] = A.rank[k0 + q * gstride] + 1u;
            rr[q] = rl[q] + A.size[l[q]];
        }
        for (uint32_t q = 0; q < kPlanBatch; ++q) {
            if (!l[q]) continue;
            A.rank[l[q]] = rl[q];
            A.rank[l[q] + 1u] = rr[q];
            if (rl[q] < A.used) A.by_rank[rl[q]] = l[q];          // always, in a tree: a rank is below the node count
            if (rr[q] < A.used) A.by_rank[rr[q]] = l[q] + 1u;
        }
    }
}

// ---- offsets by prefix count over the rank positions, the three-step shape of scan_sum / scan_top /
// scan_apply.  Four counts: treelet roots, top nodes, height + 2 of the treelet roots (a treelet of
// height h holds every height 0 .. h, so it owns h + 2 boundaries of lvl) and -- over node indices,
// not ranks -- the nodes reached from the root.  What a rank adds to them is found by every lane for
// itself first (plan_classify: rank -> node -> size, parent -> the parent's size, a chain of
// dependent loads) and kept as one word, so the lanes that sum runs read consecutive words:
//   bits 0-1 the class of the rank's node (plan_class), bits 2-8 height + 2 of a treelet root,
//   bit 16 the node of that INDEX is reached
struct PlanSums { uint32_t v[4]; };
RT_HD void plan_classify(const PlanArgs &A, uint32_t gtid, uint32_t gstride) {
    for (uint32_t r = gtid; r < A.used; r += gstride) {
        const uint32_t k = A.by_rank[r], cls = k < A.used ? plan_class(A, k) : 0u;
        A.cw[r] = cls | (cls == 1u ? (plan_height(A, k) + 2u) << 2 : 0u) | (A.depth_of[r] != ~0u ? 1u << 16 : 0u);
    }
}
RT_HD void plan_add(uint32_t w, PlanSums &s) {
    s.v[0] += (w & 3u) == 1u ? 1u : 0u;
    s.v[1] += (w & 3u) == 2u ? 1u : 0u;
    s.v[2] += (w >> 2) & 127u;
    s.v[3] += w >> 16;
}
RT_HD void plan_scan_sum(const PlanArgs &A, uint32_t gtid, uint32_t gstride) {
    for (uint32_t c = gtid; c < plan_runs(A.used); c += gstride) {
        PlanSums s{};
        for (uint32_t r = c * kPlanScanRun; r < (c + 1u) * kPlanScanRun && r < A.used; ++r) plan_add(A.cw[r], s);
        for (int j = 0; j < 4; ++j) A.csum[4 * (size_t)c + j] = s.v[j];
    }
}
// one workgroup: every lane sums a stretch of runs, wg_scan places the stretches; lds: stride words
template <class P>
RT_HD void plan_scan_top(const PlanArgs &A, uint32_t *lds, P &par) {
    const uint32_t runs = plan_runs(A.used), per = (runs + par.stride - 1u) / par.stride;
    const uint32_t c0 = par.tid * per < runs ? par.tid * per : runs, c1 = c0 + per < runs ? c0 + per : runs;
    uint32_t sum[4] = {0, 0, 0, 0}, before[4], total[4];
    for (uint32_t c = c0; c < c1; ++c)
        for (int j = 0; j < 4; ++j) sum[j] += A.csum[4 * (size_t)c + j];
    for (int j = 0; j < 4; ++j) before[j] = wg_scan(lds, sum[j], total[j], par);
    for (uint32_t c = c0; c < c1; ++c)
        for (int j = 0; j < 4; ++j) {
            const uint32_t v = A.csum[4 * (size_t)c + j];
            A.csum[4 * (size_t)c + j] = before[j];
            before[j] += v;
        }
    if (par.tid == 0u) {
        A.ctr[kPcTreelets] = total[0];
        A.ctr[kPcTop] = total[1];
        A.ctr[kPcLvlSum] = total[2];
        A.ctr[kPcSeen] = total[3];
        A.ctr[kPcRootSize] = A.size[0];
    }
}
// treelet root number g: its node, its first list entry (rank - top nodes before it) and grp[g];
// top node number t: its place in the compacted array
RT_HD void plan_scan_apply(const PlanArgs &A, uint32_t gtid, uint32_t gstride) {
    for (uint32_t c = gtid; c < plan_runs(A.used); c += gstride) {
        PlanSums s{};
        for (int j = 0; j < 4; ++j) s.v[j] = A.csum[4 * (size_t)c + j];
        uint32_t w[kPlanScanRun];
        for (uint32_t i = 0; i < kPlanScanRun; ++i) w[i] = c * kPlanScanRun + i < A.used ? A.cw[c * kPlanScanRun + i] : 0u;
        for (uint32_t i = 0; i < kPlanScanRun; ++i) {
            const uint32_t r = c * kPlanScanRun + i, g = s.v[0], t = s.v[1], lv = s.v[2], cls = w[i] & 3u;
            plan_add(w[i], s);
            if (cls == 1u) { A.troot[g] = A.by_rank[r]; A.tlist[g] = r - t; A.grp[g] = lv; }
            if (cls == 2u) A.topc[t] = A.by_rank[r];
        }
    }
}

RT_HD size_t plan_list_len(uint32_t used) { return used; }                   // uint32: PlanArgs::list
RT_HD size_t plan_lvl_len(uint32_t used) { return 2 * (size_t)used + 2; }    // lvl: (nodes + 1) per group at most
RT_HD size_t plan_grp_len(uint32_t used) { return (size_t)used + 2; }        // grp: a treelet per node at most

// ---- one workgroup per treelet: its nodes are by_rank[rank(root) .. + size), at most kTreeletNodes.
// Their heights go to workgroup memory (lds: kTreeletNodes words); node i lands at (heights below
// its own) + (earlier nodes of its height), boundary hh at (heights below hh).  Workgroup wg of nwg
// takes treelets wg, wg + nwg, ...
template <class P>
RT_HD void plan_treelets(const PlanArgs &A, uint32_t wg, uint32_t nwg, uint32_t *lds, P &par) {
    const uint32_t nt = A.ctr[kPcTreelets];
    for (uint32_t g = wg; g < nt; g += nwg) {
        const uint32_t root = A.troot[g], r0 = A.rank[root], list0 = A.tlist[g], lvl0 = A.grp[g], h = plan_height(A, root);
        uint32_t sz = A.size[root] < kTreeletNodes ? A.size[root] : kTreeletNodes;
        if (r0 >= A.used) sz = 0u;
        else if (sz > A.used - r0) sz = A.used - r0;
        for (uint32_t i = par.tid; i < sz; i += par.stride) lds[i] = plan_height(A, A.by_rank[r0 + i]);
        par.bar();
        for (uint32_t i = par.tid; i < sz; i += par.stride) {
            const uint32_t hi = lds[i];
            uint32_t pos = 0;
            for (uint32_t j = 0; j < sz; ++j) pos += (lds[j] < hi || (lds[j] == hi && j < i)) ? 1u : 0u;
            A.list[list0 + pos] = A.by_rank[r0 + i];   // list0 <= r0 and pos < sz <= used - r0
        }
        for (uint32_t hh = par.tid; hh <= h + 1u; hh += par.stride) {
            uint32_t below = 0;
            for (uint32_t j = 0; j < sz; ++j) below += lds[j] < hh ? 1u : 0u;
            if (lvl0 + hh < plan_lvl_len(A.used)) A.lvl[lvl0 + hh] = list0 + below;
        }
        par.bar();   // the next treelet's heights
    }
}

// ---- the top, one workgroup: the nodes above the cut, compacted in rank order (topc).  Count per
// height with integer adds; the boundaries of the heights that occur (the top's heights need not be
// consecutive) and the closing entries of lvl and grp -- an empty top still owns one entry of each;
// then the nodes, kPlanTopChunk at a time with running per-height counters, each at (nodes of smaller
// height) + (earlier nodes of its height).  lds: kPlanTopChunk + 2 kPlanHeights words.
template <class P>
RT_HD void plan_top(const PlanArgs &A, uint32_t *lds, P &par) {
    uint32_t *hts = lds, *run = lds + kPlanTopChunk, *cnt = run + kPlanHeights;
    const uint32_t nt = A.ctr[kPcTreelets], ntop = A.ctr[kPcTop], lvl0 = A.ctr[kPcLvlSum], all = A.ctr[kPcRootSize];
    const uint32_t list0 = all > ntop ? all - ntop : 0u;
    for (uint32_t i = par.tid; i < kPlanHeights; i += par.stride) cnt[i] = 0u;
    par.bar();
    for (uint32_t i = par.tid; i < ntop; i += par.stride) par.aadd(cnt + plan_height(A, A.topc[i]), 1u);
    par.bar();
    if (par.tid == 0u) {
        uint32_t before = 0, l = lvl0;
        A.grp[nt] = lvl0;
        for (uint32_t hh = 0; hh < kPlanHeights; ++hh) {
            run[hh] = before;
            if (cnt[hh] && l < plan_lvl_len(A.used)) A.lvl[l++] = list0 + before;
            before += cnt[hh];
        }
        if (l < plan_lvl_len(A.used)) A.lvl[l++] = list0 + ntop;
        A.grp[nt + 1u] = l;
        A.ctr[kPcListLen] = list0 + ntop;
        A.ctr[kPcLvlLen] = l;
    }
    par.bar();
    for (uint32_t c0 = 0; c0 < ntop; c0 += kPlanTopChunk) {
        const uint32_t m = ntop - c0 < kPlanTopChunk ? ntop - c0 : kPlanTopChunk;
        for (uint32_t i = par.tid; i < m; i += par.stride) hts[i] = plan_height(A, A.topc[c0 + i]);
        par.bar();
        for (uint32_t i = par.tid; i < m; i += par.stride) {
            const uint32_t hi = hts[i];
            uint32_t earlier = 0;
            for (uint32_t j = 0; j < i; ++j) earlier += hts[j] == hi ? 1u : 0u;
            const uint32_t at = list0 + run[hi] + earlier;
            if (at < plan_list_len(A.used)) A.list[at] = A.topc[c0 + i];
        }
        par.bar();
        for (uint32_t hh = par.tid; hh < kPlanHeights; hh += par.stride) {
            uint32_t c = 0;
            for (uint32_t j = 0; j < m; ++j) c += hts[j] == hh ? 1u : 0u;
            run[hh] += c;
        }
        par.bar();
    }
}

// ---- the small route: the same steps in one workgroup, bar() where the other route has a launch boundary
template <class P>
RT_HD void plan_small(const PlanArgs &A, uint32_t *lds, P &par) {
    const uint32_t depth = A.depth < kPlanMaxDepth ? A.depth : kPlanMaxDepth;
    plan_init(A, par.tid, par.stride);
    par.bar();
    for (uint32_t d = 0; d < depth; ++d) { plan_down(A, d, par.tid, par.stride); par.bar(); }
    for (uint32_t d = depth; d-- > 0u;) { plan_up(A, d, par.tid, par.stride); par.bar(); }
    for (uint32_t d = 0; d < depth; ++d) { plan_rank(A, d, par.tid, par.stride); par.bar(); }
    plan_classify(A, par.tid, par.stride);
    par.bar();
    plan_scan_sum(A, par.tid, par.stride);
    par.bar();
    plan_scan_top(A, lds, par);
    par.bar();
    plan_scan_apply(A, par.tid, par.stride);
    par.bar();
    plan_treelets(A, 0u, 1u, lds, par);
    par.bar();
    plan_top(A, lds, par);
}

// ---- the array sizes, in elements (A: anything with take<T>(count), as build_carve's)
template <class A>
void plan_carve(A &a, uint32_t used, PlanArgs &P) {
    P.depth_of = a.template take<uint32_t>(used);
    P.parent = a.template take<uint32_t>(used);
    P.size = a.template take<uint32_t>(used);
    P.height = a.template take<uint32_t>(used);
    P.rank = a.template take<uint32_t>(used);
    P.by_rank = a.template take<uint32_t>(used);
    P.cw = a.template take<uint32_t>(used);
    P.csum = a.template take<uint32_t>(4 * (size_t)plan_runs(used));
    P.troot = a.template take<uint32_t>(used);
    P.tlist = a.template take<uint32_t>(used);
    P.topc = a.template take<uint32_t>(used);
    P.ctr = a.template take<uint32_t>(kPcWords);
}

// ---- the launch order.  A step is one kernel of rt_plan.hip, or on the host a loop over its workgroups:
//   kPlanStepSmall                 a tree of at most kPlanSmall nodes: everything, one workgroup (plan_small)
//   kPlanStepInit                  per node: not reached, a leaf's size and height; the root
//   kPlanStepDown                  per depth from the root: the children's depth and parent
//   kPlanStepUp                    per depth from the deepest: size and height
//   kPlanStepRank                  per depth from the root: pre-order ranks, the node of every rank
//   kPlanStepClassify              per rank: what it adds to the prefix counts
//   kPlanStepScanSum / -Top / -Apply   the prefix counts over the ranks: treelet roots, top nodes, lvl offsets
//   kPlanStepTreelets              the treelets' parts of list and lvl, a workgroup each
//   kPlanStepTop                   the top's part, the closing entries, the lengths; one workgroup
// Nothing is handed from one workgroup to another inside a launch -- no flags, no spins, no fences;
// plain stores; the one atomic is an integer add into workgroup memory (plan_top).  The level loops
// are bounded by kPlanMaxDepth.  One read-back, at the end.
enum PlanStep {
    kPlanStepSmall, kPlanStepInit, kPlanStepDown, kPlanStepUp, kPlanStepRank, kPlanStepClassify, kPlanStepScanSum, kPlanStepScanTop,
    kPlanStepScanApply, kPlanStepTreelets, kPlanStepTop
};
// what plan_order returns: kPlanOk, the executor's own failure, or kPlanNotTree -- the nodes reached
// from the root are not a tree (a child pair with two parents: only a caller's prebuilt node array
// can hold one), which the host's walk still schedules and this text does not
enum { kPlanOk = 0, kPlanExec, kPlanNotTree };
struct PlanFigures { uint32_t ntreelets, has_top, list_len, lvl_len, top_nodes, launches, route; };
enum { kPlanRouteNone = 0, kPlanRouteHost, kPlanRouteLaunches, kPlanRouteSmall };   // rt_scene_update_plan_info's second word

RT_HD uint32_t plan_route(uint32_t used) { return used <= kPlanSmall ? kPlanRouteSmall : kPlanRouteLaunches; }

// The executor X (as build_order's): zero(ptr, words), read(dst, src, words), step(PlanStep, count, arg)
//   count: the lanes of a per-node or per-run step, the workgroups of kPlanStepTreelets; arg: the depth
// route: plan_route(A.used) -- a test may run a small tree through the many-launch order as well
template <class X>
int plan_order(X &x, const PlanArgs &A, uint32_t route, PlanFigures &f) {
    f = PlanFigures{};
    const uint32_t depth = A.depth < kPlanMaxDepth ? A.depth : kPlanMaxDepth;
    if (!x.zero(A.ctr, kPcWords)) return kPlanExec;
    if (route == kPlanRouteSmall) {
        if (!x.step(kPlanStepSmall, 1u, 0u)) return kPlanExec;
        f.launches = 1;
        f.route = kPlanRouteSmall;
    } else {
        if (!x.step(kPlanStepInit, A.used, 0u)) return kPlanExec;
        for (uint32_t d = 0; d < depth; ++d)
            if (!x.step(kPlanStepDown, A.used, d)) return kPlanExec;
        for (uint32_t d = depth; d-- > 0u;)
            if (!x.step(kPlanStepUp, A.used, d)) return kPlanExec;
        for (uint32_t d = 0; d < depth; ++d)
            if (!x.step(kPlanStepRank, A.used, d)) return kPlanExec;
        if (!x.step(kPlanStepClassify, A.used, 0u) || !x.step(kPlanStepScanSum, plan_runs(A.used), 0u) || !x.step(kPlanStepScanTop, 1u, 0u) ||
            !x.step(kPlanStepScanApply, plan_runs(A.used), 0u) || !x.step(kPlanStepTreelets, plan_treelet_wgs(A.used), 0u) ||
            !x.step(kPlanStepTop, 1u, 0u))
            return kPlanExec;
        f.launches = 3u * depth + 7u;
        f.route = kPlanRouteLaunches;
    }
    uint32_t ctr[kPcWords];
    if (!x.read(ctr, A.ctr, kPcWords)) return kPlanExec;
    if (ctr[kPcSeen] != ctr[kPcRootSize]) return kPlanNotTree;
    f.ntreelets = ctr[kPcTreelets];
    f.top_nodes = ctr[kPcTop];
    f.has_top = f.top_nodes ? 1u : 0u;
    f.list_len = ctr[kPcListLen];
    f.lvl_len = ctr[kPcLvlLen];
    return kPlanOk;
}

}  // namespace rt
