// The in-place update path on the host, for the stand-alone programs prim_records_host.cpp and
// update_host.cpp: a RefitArgs over a ScenePack's own vectors (slot map and slot boxes from
// build_refit_plan / seed_slot_boxes, as ensure_refit makes them on the device) and the refit of
// every group, one height after another, through the kernels' refit_level.
#pragma once
#include <cstring>
#include <vector>

#include "rt_internal.h"
#include "rt_refit.h"
#include "rt_update.h"

struct HostScene {
    rt::ScenePack pack;
    rt::RefitPlan plan;
    std::vector<float4> slots;
    rt::RefitArgs A{};

    bool prepare(const rt::PackOptions &o) {
        if (!rt::build_refit_plan(pack.bvh, (uint32_t)pack.pinfo.size(), plan)) return false;
        rt::seed_slot_boxes(pack.bvh, pack.pinfo, pack.pbox, slots);
        A.nodes = pack.nodes.data(); A.prims = pack.prims.data(); A.shade = pack.shade.data(); A.xprims = pack.xprims.data();
        A.slot_box = slots.data();
        A.slot_of = plan.slot_of.data(); A.list = plan.list.data(); A.lvl = plan.lvl.data(); A.grp = plan.grp.data();
        A.margin = o.walk_margin;
        A.sliver_lim = o.sliver_lim;
        return true;
    }
    // k_refit_treelets (groups 0 .. ntreelets - 1), then k_refit_top (group ntreelets)
    void refit() const {
        for (uint32_t g = 0; g + 1 < plan.grp.size(); ++g)
            for (uint32_t l = plan.grp[g]; l + 1 < plan.grp[g + 1]; ++l) rt::refit_level(A, l, 0, 1);
    }
};

template <typename T>
static bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(T) * a.size()) == 0;
}
