// The GPU builder on the host, for the stand-alone programs build_host.cpp and splice_host.cpp: the
// launch order (build_order) and the array sizes (build_carve, build_*_len) are csrc/rt_build.h's own,
// the ones rt_build.hip's run_build and build_tree use; this header supplies what the device supplies.
//   HostExec    a step is a loop where the device has a grid, every lane's text run with SerialLane.
//               The workgroups of a per-workgroup step run in descending order: any order within a
//               launch must give the same bytes.
//   HeapBlocks  every work array is a heap block of its own, of exactly the size build_carve asks
//               for, so AddressSanitizer's red zones lie between the arrays (one carved arena would
//               hide an overrun from one array into the next).
//   HostBuild   the outputs, each a vector of exactly its build_*_len, the figures and the refusal code.
#pragma once
#include <cstring>
#include <memory>
#include <vector>

#include "rt_build.h"

struct HeapBlocks {
    std::vector<std::unique_ptr<char[]>> blocks;
    template <typename T>
    T *take(size_t count) {
        blocks.emplace_back(new char[sizeof(T) * count]());
        return reinterpret_cast<T *>(blocks.back().get());
    }
};

struct HostExec {
    const rt::BuildArgs &B;
    std::vector<uint32_t> acc = std::vector<uint32_t>(rt::kAccWords), scan = std::vector<uint32_t>(1),
                          stack = std::vector<uint32_t>(rt::kBuildStack);

    bool zero(uint32_t *p, size_t words) { std::memset(p, 0, sizeof(uint32_t) * words); return true; }
    bool read(uint32_t *dst, const uint32_t *src, size_t words) { std::memcpy(dst, src, sizeof(uint32_t) * words); return true; }
    bool step(rt::BuildStep s, uint32_t count, uint32_t arg) {
        using namespace rt;
        SerialLane par;
        uint32_t *a = acc.data(), *sc = scan.data();
        switch (s) {
        case kStepInit: build_init(B, 0, 1, par); break;
        case kStepWideBounds: for (uint32_t g = count; g-- > 0;) wide_bounds(B, arg, g, a, par); break;
        case kStepWideBins: for (uint32_t g = count; g-- > 0;) wide_bins(B, arg, g, a, par); break;
        case kStepWidePlane: for (uint32_t g = count; g-- > 0;) wide_plane_count(B, arg, g, a, sc, par); break;
        case kStepWideSettle: for (uint32_t w = 0; w < count; ++w) wide_settle(B, arg, w, par); break;
        case kStepWideTables: for (uint32_t g = count; g-- > 0;) wide_tables(B, arg, g, sc, par); break;
        case kStepWideMove: for (uint32_t g = count; g-- > 0;) wide_move(B, arg, g, par); break;
        case kStepWideBack: for (uint32_t g = count; g-- > 0;) wide_copy_back(B, arg, g, par); break;
        case kStepSubtrees: for (uint32_t k = count; k-- > 0;) build_subtree(B, B.slist[k], a, sc, stack.data(), par); break;
        case kStepScanSum: scan_sum(B, 0, 1); break;
        case kStepScanTop: scan_top(B); break;
        case kStepScanApply: scan_apply(B, 0, 1); break;
        case kStepEmit: emit_nodes(B, 0, 1, par); break;
        case kStepPermute: permute_slots(B, 0, 1); break;
        case kStepBoxes: box_level(B, count, arg, 0, 1); break;
        }
        return true;
    }
};

struct HostBuild {
    std::vector<uint32_t> idx, slot_of;
    std::vector<float4> nodes, prims, slot_box;
    rt::BuildFigures f{};
    int code = rt::kBuildOk;   // build_order's: kBuildOk or the refusal

    // the inputs are build_tree's; nodes is trimmed to the tree's once it stands
    int run(uint32_t n, const float4 *cen, const float4 *old_box, const uint32_t *old_slot_of, const float4 *old_prims, float margin) {
        rt::BuildArgs B{};
        B.n = n;
        B.cen = cen; B.old_box = old_box; B.old_slot_of = old_slot_of; B.old_prims = old_prims;
        B.margin = margin;
        HeapBlocks work;
        rt::build_carve(work, n, B);
        idx.assign(rt::build_ids_len(n), 0);
        slot_of.assign(rt::build_ids_len(n), 0);
        nodes.assign(rt::build_nodes_len(n), make_float4(0, 0, 0, 0));
        prims.assign(rt::build_prims_len(n), make_float4(0, 0, 0, 0));
        slot_box.assign(rt::build_slot_box_len(n), make_float4(0, 0, 0, 0));
        B.idx = idx.data(); B.nodes = nodes.data(); B.prims = prims.data(); B.slot_box = slot_box.data(); B.slot_of = slot_of.data();
        HostExec x{B};
        code = rt::build_order(x, B, f);
        if (code == rt::kBuildOk) nodes.resize(2 * (size_t)f.nodes_used);
        return code;
    }
};
