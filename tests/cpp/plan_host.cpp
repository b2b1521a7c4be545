// Stand-alone host run of the GPU refit schedule -- the per-lane text, the launch order (plan_order)
// and the array sizes (plan_carve, plan_*_len) of csrc/rt_plan.h that rt_plan.hip runs -- against its
// definition, build_refit_plan (rt_scene_pack.cpp), with no device and no Python
// (tests/test_plan_host.py builds it with AddressSanitizer and UBSan):
//   g++ -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       -D__HIP_PLATFORM_AMD__ -I$ROCM/include -I advancedgraphicsraytracer_amd/csrc tests/cpp/plan_host.cpp
//       advancedgraphicsraytracer_amd/csrc/{rt_scene_pack,rt_host,rt_sbvh}.cpp -lz -pthread -o plan_host
//   ./plan_host advancedgraphicsraytracer_amd/data
// Two orders: the many-launch one, the workgroups of every step looped in descending order and every
// array a heap block of its own (so an overrun meets a red zone), and the one-workgroup one with
// tid = 0, stride = 1.  list, lvl, grp, ntreelets and has_top are compared word for word.
#include <cstdio>
#include <cstring>
#include <vector>

#include "host_build.h"
#include "rt_plan.h"
#include "scene_util.h"

using namespace rt;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED: %s (line %d): %s\n", #c, __LINE__, rt_last_error()); return 1; } } while (0)

// plan_order's executor on the host.  A per-node or per-run step of `count` lanes runs as
// ceil(count / 256) workgroups, last first, each one lane wide; a per-workgroup step loops its
// workgroups last first.
struct PlanHostExec {
    const PlanArgs &A;
    std::vector<uint32_t> lds = std::vector<uint32_t>(kPlanLds);

    bool zero(uint32_t *p, size_t words) { std::memset(p, 0, sizeof(uint32_t) * words); return true; }
    bool read(uint32_t *dst, const uint32_t *src, size_t words) { std::memcpy(dst, src, sizeof(uint32_t) * words); return true; }
    bool step(PlanStep s, uint32_t count, uint32_t arg) {
        SerialLane par;
        const uint32_t nwg = (count + 255u) / 256u;
        switch (s) {
        case kPlanStepSmall: plan_small(A, lds.data(), par); break;
        case kPlanStepInit: for (uint32_t g = nwg; g-- > 0;) plan_init(A, g, nwg); break;
        case kPlanStepDown: for (uint32_t g = nwg; g-- > 0;) plan_down(A, arg, g, nwg); break;
        case kPlanStepUp: for (uint32_t g = nwg; g-- > 0;) plan_up(A, arg, g, nwg); break;
        case kPlanStepRank: for (uint32_t g = nwg; g-- > 0;) plan_rank(A, arg, g, nwg); break;
        case kPlanStepClassify: for (uint32_t g = nwg; g-- > 0;) plan_classify(A, g, nwg); break;
        case kPlanStepScanSum: for (uint32_t g = nwg; g-- > 0;) plan_scan_sum(A, g, nwg); break;
        case kPlanStepScanTop: plan_scan_top(A, lds.data(), par); break;
        case kPlanStepScanApply: for (uint32_t g = nwg; g-- > 0;) plan_scan_apply(A, g, nwg); break;
        case kPlanStepTreelets: for (uint32_t g = count; g-- > 0;) plan_treelets(A, g, count, lds.data(), par); break;
        case kPlanStepTop: plan_top(A, lds.data(), par); break;
        }
        return true;
    }
};

// a tree's topology as the device holds it: the word of node i at [2 i + 1].z
static std::vector<float4> device_nodes(const Bvh &b) {
    std::vector<float4> n(2 * (size_t)b.nodes_used, make_float4(0, 0, 0, 0));
    for (uint32_t i = 0; i < b.nodes_used; ++i) n[2 * (size_t)i + 1].z = ubits(node_word(b.nodes[i].leftFirst, b.nodes[i].count));
    return n;
}
static uint32_t depth_of_tree(const Bvh &b) {   // Scene::maxDepthBVH, as take_tree measures it
    TreeWalk w;
    if (walk_tree(b.nodes.data(), b.nodes_used, b.indices.size(), w) != kTreeOk) return ~0u;
    uint32_t d = 0;
    for (uint32_t k : w.order)
        if (b.nodes[k].count > 0) d = std::max(d, k == 0 ? 1u : w.depth[k]);
    return d;
}

static int run_route(const char *name, const Bvh &b, const RefitPlan &want, uint32_t route) {
    const std::vector<float4> nodes = device_nodes(b);
    PlanArgs A{};
    A.nodes = nodes.data();
    A.used = b.nodes_used;
    A.depth = depth_of_tree(b);
    CHECK(A.depth <= kPlanMaxDepth);
    HeapBlocks work;
    plan_carve(work, A.used, A);
    std::vector<uint32_t> list(plan_list_len(A.used), 0xdeadbeefu), lvl(plan_lvl_len(A.used), 0xdeadbeefu), grp(plan_grp_len(A.used), 0xdeadbeefu);
    A.list = list.data(); A.lvl = lvl.data(); A.grp = grp.data();
    PlanHostExec x{A};
    PlanFigures f;
    CHECK(plan_order(x, A, route, f) == kPlanOk);
    const bool same = f.ntreelets == want.ntreelets && (f.has_top != 0u) == want.has_top && f.list_len == want.list.size() &&
                      f.lvl_len == want.lvl.size() &&
                      std::memcmp(list.data(), want.list.data(), sizeof(uint32_t) * want.list.size()) == 0 &&
                      std::memcmp(lvl.data(), want.lvl.data(), sizeof(uint32_t) * want.lvl.size()) == 0 &&
                      want.grp.size() == (size_t)f.ntreelets + 2 &&
                      std::memcmp(grp.data(), want.grp.data(), sizeof(uint32_t) * want.grp.size()) == 0;
    if (!same)
        std::printf("%s (route %u): %u / %u treelets, list %u / %zu, lvl %u / %zu, top %u\n", name, route, f.ntreelets, want.ntreelets,
                    f.list_len, want.list.size(), f.lvl_len, want.lvl.size(), f.top_nodes);
    CHECK(same);
    CHECK(f.route == route && f.launches == (route == kPlanRouteSmall ? 1u : 3u * A.depth + 7u));
    return 0;
}

// the host plan of the tree, and both orders where the tree is small; *top: the nodes above the cut
static int plan_case(const char *name, const Bvh &b, RefitPlan &want, uint32_t *top = nullptr) {
    CHECK(build_refit_plan(b, (uint32_t)b.indices.size(), want));
    CHECK(want.grp.size() == want.ntreelets + 2u && want.grp.back() == want.lvl.size());
    const uint32_t ntop = (uint32_t)want.list.size() - want.lvl[want.grp[want.ntreelets]];
    if (top) *top = ntop;
    CHECK(run_route(name, b, want, kPlanRouteLaunches) == 0);
    if (b.nodes_used <= kPlanSmall) CHECK(run_route(name, b, want, kPlanRouteSmall) == 0);
    CHECK(plan_route(b.nodes_used) == (b.nodes_used <= kPlanSmall ? (uint32_t)kPlanRouteSmall : (uint32_t)kPlanRouteLaunches));
    std::printf("%-12s %7u nodes, %5u treelets, %5u above the cut: ok\n", name, b.nodes_used, want.ntreelets, ntop);
    return 0;
}
static int prim_case(const char *name, const std::vector<rt_prim> &prims, RefitPlan &want, uint32_t *top = nullptr) {
    Bvh b;
    CHECK(build_bvh(prims.data(), nullptr, (uint32_t)prims.size(), b) == RT_OK);
    return plan_case(name, b, want, top);
}

// the light and n - 1 small random triangles in a 10 x 4 x 6 box (build_host.cpp's)
static std::vector<rt_prim> soup(uint32_t n, uint32_t seed) {
    std::vector<rt_prim> p{sphere(0, 8, 0, 0.5f, 0)};
    while (p.size() < n) {
        const float c[3] = {10.0f * unit(seed) - 5.0f, 4.0f * unit(seed) - 2.0f, 6.0f * unit(seed) + 2.0f};
        rt_prim t{RT_TRIANGLE, 1, {}};
        for (int k = 0; k < 9; ++k) t.v[k] = c[k % 3] + 0.3f * (unit(seed) - 0.5f);
        p.push_back(t);
    }
    return p;
}
// tests/scenes_util.py chain_scene's topology: P one-primitive leaves, every interior node a leaf and the rest
static Bvh chain(uint32_t P) {
    Bvh b;
    b.nodes.assign(2 * (size_t)P, Node{});
    b.nodes_used = 2 * P;
    for (uint32_t i = 0; i < P; ++i) b.indices.push_back(i);
    b.nodes[0].leftFirst = 2;
    for (uint32_t j = 0; j + 1 < P; ++j) {
        b.nodes[2 + 2 * j].leftFirst = j; b.nodes[2 + 2 * j].count = 1;
        Node &rest = b.nodes[3 + 2 * j];
        if (j == P - 2) { rest.leftFirst = P - 1; rest.count = 1; }
        else rest.leftFirst = 4 + 2 * j;
    }
    return b;
}
// a hand-made tree over `leaves` one-primitive leaves, split in halves (the left takes the odd one),
// child pairs handed out as met: 2 leaves - 1 nodes below and with the root
static void halves(Bvh &b, uint32_t k, uint32_t first, uint32_t leaves) {
    if (leaves == 1) { b.nodes[k].leftFirst = first; b.nodes[k].count = 1; return; }
    const uint32_t l = b.nodes_used, nl = (leaves + 1) / 2;
    b.nodes_used += 2;
    b.nodes[k].leftFirst = l;
    halves(b, l, first, nl);
    halves(b, l + 1, first + nl, leaves - nl);
}
static Bvh halves_tree(uint32_t leaves) {
    Bvh b;
    b.nodes.assign(2 * (size_t)leaves + 2, Node{});
    b.nodes_used = 2;
    for (uint32_t i = 0; i < leaves; ++i) b.indices.push_back(i);
    halves(b, 0, 0, leaves);
    return b;
}

int main(int argc, char **argv) {
    if (argc < 2) { std::printf("usage: plan_host <mesh dir>\n"); return 2; }
    RefitPlan p;
    uint32_t top = 0;
    CHECK(prim_case("kat", kat_prims(), p, &top) == 0);
    CHECK(p.ntreelets == 1 && top == 0);
    {   // the root is a leaf: one node, one treelet, no top -- the empty top's entry of grp and of lvl, and the closing one
        Bvh leaf;
        leaf.nodes.assign(2, Node{});
        leaf.nodes[0].count = 2;
        leaf.indices = {1, 0};
        leaf.nodes_used = 2;
        CHECK(plan_case("leaf", leaf, p, &top) == 0);
        CHECK(p.ntreelets == 1 && !p.has_top && p.list.size() == 1 && p.lvl.size() == 3 && p.grp.size() == 3 && p.grp[1] == 2 && p.grp[2] == 3);
    }
    {   // 64 levels: heights 0 .. 63 in one treelet, and the level loops at their bound
        const Bvh b = chain(65);
        CHECK(depth_of_tree(b) == kPlanMaxDepth);
        CHECK(plan_case("chain", b, p, &top) == 0);
        CHECK(p.ntreelets == 1 && p.lvl.size() == 64 + 1 + 1 + 1);
    }
    {
        SceneSource teapot;
        CHECK(recipe_source("teapotF", argv[1], teapot) == RT_OK);
        CHECK(prim_case("teapotF", teapot.prims, p, &top) == 0);
        CHECK(p.ntreelets == 13 && top == 12);
    }
    {   // at least 2 treelets and a top of at least 2 heights
        CHECK(prim_case("4 wide + 3", soup(4u * kBuildWide + 3u, 24u), p, &top) == 0);
        const uint32_t g = p.ntreelets;
        CHECK(p.ntreelets >= 2 && p.has_top && p.grp[g + 1] - p.grp[g] >= 3);
    }
    {   // the top does not fit two passes of plan_top; the many-launch order alone
        Bvh b;
        const std::vector<rt_prim> prims = soup(20001u, 5u);
        CHECK(build_bvh(prims.data(), nullptr, (uint32_t)prims.size(), b) == RT_OK);
        CHECK(b.nodes_used > kPlanSmall);
        CHECK(plan_case("soup 20000", b, p, &top) == 0);
        CHECK(top > 2u * kPlanTopChunk);
    }
    // The cut's boundary.  A subtree of full pairs has an odd number of nodes, so the sizes next to
    // kTreeletNodes = 256 are 255 (128 leaves: the root is a treelet's) and 257 (129 leaves: the root
    // alone is above the cut); and both as the two children of one root.
    static_assert(kTreeletNodes == 256, "the hand-made trees sit on either side of 256 nodes");
    CHECK(plan_case("255 nodes", halves_tree(128), p, &top) == 0);
    CHECK(p.list.size() == 255 && p.ntreelets == 1 && top == 0);
    CHECK(plan_case("257 nodes", halves_tree(129), p, &top) == 0);
    CHECK(p.list.size() == 257 && p.ntreelets == 2 && top == 1);
    {
        Bvh b = halves_tree(128 + 129);   // the left half takes 129 leaves (257 nodes), the right 128 (255)
        CHECK(plan_case("257 | 255", b, p, &top) == 0);
        CHECK(p.ntreelets == 3 && top == 2);
    }
    std::printf("plan_host ok\n");
    return 0;
}
