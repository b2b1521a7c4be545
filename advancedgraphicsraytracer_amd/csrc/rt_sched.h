// rt_sched.h -- the arithmetic that lays a frame out, host only: the tile grid and a rank's share of
// it, the sample split, the measured-cost tile orders (plain, split, XCD-grouped) and the sizing of a
// wavefront path-traced frame's batches, queues and path-state slots.  Pure functions of integers and
// a cost vector; rt_device.hip calls them between its HIP calls (tests/cpp/sched_host.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace rt {

// ---- the grid of 8 x 8 tiles, and the tiles of it that one launch covers
struct TileGrid {
    uint32_t tiles_x, tiles_y, ntiles;
};
inline TileGrid tile_grid(uint32_t W, uint32_t H) {
    const uint32_t tx = (W + 7) / 8, ty = (H + 7) / 8;
    return {tx, ty, tx * ty};
}
// tiles of the interleaved shard `shard` of `nshards`: shard, shard + nshards, ...
inline uint32_t local_tiles(uint32_t ntiles, uint32_t shard, uint32_t nshards) {
    return shard < ntiles ? (ntiles - shard + nshards - 1) / nshards : 0;
}
// pixels covered by a frame / shard launch (primary rays per sample): the tiles of `list` (an explicit
// deal, ntiles_local entries), else of the interleaved shard
inline uint64_t frame_pixels(uint32_t W, uint32_t H, uint32_t ntiles_local, uint32_t shard, uint32_t nshards,
                             const uint32_t *list) {
    uint64_t px = (uint64_t)ntiles_local * 64u;
    if ((W & 7u) || (H & 7u)) {
        const TileGrid g = tile_grid(W, H);
        px = 0;
        auto add = [&](uint32_t t) {
            uint32_t tx = t % g.tiles_x, ty = t / g.tiles_x;
            px += (uint64_t)std::min(8u, W - tx * 8) * std::min(8u, H - ty * 8);
        };
        if (list)
            for (uint32_t i = 0; i < ntiles_local; ++i) add(list[i]);
        else
            for (uint32_t t = shard; t < g.ntiles; t += nshards) add(t);
    }
    return px;
}
// the tiles whose running averages an accumulator holds: kind 0 none yet, 1 every tile, 2 the
// interleaved shard, 3 the explicit list
inline bool held_tiles(int kind, uint32_t ntiles, uint32_t shard, uint32_t nshards, const std::vector<uint32_t> &list,
                       std::vector<uint32_t> &tiles) {
    tiles.clear();
    switch (kind) {
    case 1:
        for (uint32_t t = 0; t < ntiles; ++t) tiles.push_back(t);
        return true;
    case 2:
        for (uint32_t t = shard; t < ntiles; t += nshards) tiles.push_back(t);
        return true;
    case 3:
        tiles = list;
        return true;
    default:
        return false;
    }
}

// ---- sample split
// A frame (or a shard of one) with few tiles and several samples per pixel is cut into (tile, sample
// chunk) units, so the dispatcher still balances about split_units waves of uneven cost (a 1/8 shard
// at spp 8 would otherwise be one round of whole-tile waves, as long as its slowest tile).
// (first measured on TEAPOT-F shards, tools/shard_time.py: split below ~5 rounds of
// waves, until ~10 rounds, chunks of equal sample counts.  Round 3: whole 1080p frames at
// spp > 1 gain from it too -- CFG5-sub scene spp 16 2.41 -> 1.44 ms, mig29 x16 spp 4 1.49
// -> 0.76 ms, TEAPOT-F spp 4 0.390 -> 0.386 ms, frames identical (profiles/r03/split_ab/) --
// so the threshold is 40,000 tiles instead of 20,000; 80,000 measured the same or slower)
inline uint32_t sample_chunks(uint32_t spp, uint32_t ntiles_local, uint32_t split_units, bool eligible) {
    uint32_t nchunks = 1;
    if (eligible && spp > 1 && ntiles_local < split_units)
        while (ntiles_local * nchunks < 2u * split_units && nchunks < spp) {
            uint32_t d = nchunks + 1;                  // next divisor of spp: equal chunks
            while (spp % d) ++d;
            nchunks = d;
        }
    return nchunks;
}

// ---- the measured-cost tile order
// A tile's cost is its wave's residence time, so sum / slots is the frame's throughput time and the
// costliest tile its latency floor (mig29 x16 1080p: 3.6x, its 1/2 shard 7x; TEAPOT-F 1080p
// 1.2-1.3x).  A sample-split frame's map holds one chunk's cycles per tile (the last unit of the
// tile to finish writes it): nchunks of them run.  True: the costliest tile outlasts 2 x the frame's
// mean time per resident wave slot.
inline bool tail_bound(const std::vector<uint32_t> &cost, uint32_t num_cus, uint32_t nchunks) {
    double sum = 0, mx = 0;
    for (uint32_t c : cost) { sum += c; mx = std::max<double>(mx, c); }
    const double slots = (double)num_cus * 4.0 * 7.0;
    return sum > 0 && mx * slots > 2.0 * sum * std::max(1u, nchunks);
}
// leading tiles of the split order that run as `parts` units each (RT_SPLIT_HEAVY: -1 = n / 32)
inline uint32_t split_count(uint32_t n, int32_t heavy_split, bool split_ok) {
    if (!split_ok) return 0;
    return std::min<uint32_t>(n, heavy_split < 0 ? n / 32u : (uint32_t)heavy_split);
}
// lanes per part of a split tile = 1 << part_shift (FrameArgs::part_shift; 5: halves)
inline uint32_t part_shift(uint32_t parts) { return parts == 8 ? 3u : parts == 4 ? 4u : 5u; }
// the frame's units: (tile, sample chunk) pairs, plus the extra parts of the split tiles (split only with nchunks 1)
inline uint32_t order_units(uint32_t ntiles_local, uint32_t nchunks, bool split, uint32_t order_split, uint32_t order_parts) {
    return ntiles_local * nchunks + (split ? order_split * (order_parts - 1u) : 0u);
}
// entries of plain order (n) | split order: n + (parts - 1) x the split tiles -- up to 9 n with 8 parts
// and every tile split (RT_SPLIT_PARTS / RT_SPLIT_HEAVY; 3 n overflowed a balanced rank's short tile
// list with 4 parts and 500 split tiles, round 5)
inline uint64_t order_capacity(uint32_t n) { return 9ull * n; }

// where an order's local tiles lie on the screen: tile = map ? map[local] : local * nshards + shard
struct TileWhere {
    uint32_t tiles_x, shard, nshards;
    const uint32_t *map;
};

// XCD-grouped measured order (RT_XCD_ORDER=1): the frame kernel's block b (4 waves = slots
// 4b .. 4b+3) runs on the XCD of blocks b % 8 (blocks are dealt round-robin over the 8 XCDs,
// MI355X_MICROARCH.md), so group g = b % 8 gets one compact screen region -- a run of the
// tiles in Morton order holding 1/8 of the measured cost -- costliest tile first.  Each XCD's
// L2 then holds the nodes of its region only, not of the whole frame.  A group whose region
// ran out takes tiles from the region with the most cost left.
inline std::vector<uint32_t> xcd_grouped_order(const TileWhere &F, const std::vector<uint32_t> &entries,
                                               const std::vector<uint32_t> &cost, uint32_t parts) {
    // entries: order entries (local tile | split bits); an entry's cost is its tile's, divided
    // by the parts of a split tile (bit 31)
    const uint32_t n = (uint32_t)entries.size();
    auto morton = [](uint32_t x, uint32_t y) {
        uint64_t m = 0;
        for (int b = 0; b < 16; ++b) m |= (uint64_t)((x >> b) & 1u) << (2 * b) | (uint64_t)((y >> b) & 1u) << (2 * b + 1);
        return m;
    };
    std::vector<uint32_t> z(n);
    std::vector<uint64_t> code(n);
    std::vector<double> ec(n);
    double total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t e = entries[i], lt = e & 0x0fffffffu;
        const uint32_t tile = F.map ? F.map[lt] : lt * F.nshards + F.shard;
        code[i] = morton(tile % F.tiles_x, tile / F.tiles_x) * 16u + (e >> 28);
        ec[i] = (e >> 31) ? cost[lt] / (double)parts : (double)cost[lt];
        z[i] = i;
        total += ec[i];
    }
    std::stable_sort(z.begin(), z.end(), [&](uint32_t a, uint32_t b) { return code[a] < code[b]; });
    std::vector<std::vector<uint32_t>> region(8);
    std::vector<double> left(8, 0.0);
    double acc = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t g = std::min<uint32_t>(7u, (uint32_t)(acc * 8.0 / std::max(total, 1.0)));
        region[g].push_back(z[i]);
        left[g] += ec[z[i]];
        acc += ec[z[i]];
    }
    for (auto &rg : region)   // costliest first within a region (sorted ascending: taken from the back)
        std::stable_sort(rg.begin(), rg.end(), [&](uint32_t a, uint32_t b) { return ec[a] < ec[b]; });
    std::vector<uint32_t> out;
    out.reserve(n);
    for (uint32_t b = 0; out.size() < n; ++b) {
        for (uint32_t w = 0; w < 4 && out.size() < n; ++w) {
            uint32_t g = b % 8u;
            if (region[g].empty()) {   // out.size() < n: some region still holds entries
                int best = -1;
                for (uint32_t h = 0; h < 8; ++h)
                    if (!region[h].empty() && (best < 0 || left[h] > left[best])) best = (int)h;
                g = (uint32_t)best;
            }
            const uint32_t i = region[g].back();
            region[g].pop_back();
            left[g] -= ec[i];
            out.push_back(entries[i]);
        }
    }
    return out;
}

// Longest-tile-first dispatch (LPT): tiles differ in cost by an order of magnitude (sky vs mesh), and
// the dispatcher hands out workgroups in index order, so expensive tiles that come last leave most
// CUs idle at the end of the frame.  From a frame's per-tile wave cycles: the plain order (slot i
// renders the i-th most expensive tile; cost.size() entries), followed by the split order.
// The costliest tiles can bound the frame's tail (one wave's latency chain): the split order runs
// the first k of them as `parts` waves of a part each -- 2 (rows 0-3 / 4-7), 4 or 8, RT_SPLIT_PARTS --
// entry bit 31 = split, the part number from bit 28 up.  It shortens tail-bound frames (mig29 x16
// -10 %, 720p TEAPOT-F -9 %) and lengthens throughput-bound ones (1080p TEAPOT-F +9 %: the half-
// empty waves cost issue slots), so with RT_SPLIT_HEAVY = -1 (default) both orders are timed on two
// frames each and the faster one is kept; frames are identical either way.
// xcd: both orders grouped by XCD (global-node frame kernel).
inline std::vector<uint32_t> build_tile_order(const std::vector<uint32_t> &cost, uint32_t k, uint32_t parts, bool xcd,
                                              const TileWhere &where) {
    const uint32_t n = (uint32_t)cost.size();
    std::vector<uint32_t> ord(n);
    for (uint32_t i = 0; i < n; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    std::vector<uint32_t> ent(ord), sp;
    for (uint32_t i = 0; i < k; ++i)
        for (uint32_t q = 0; q < parts; ++q) sp.push_back(ord[i] | 0x80000000u | (q << 28));
    for (uint32_t i = k; i < n; ++i) sp.push_back(ord[i]);
    if (xcd) {
        ent = xcd_grouped_order(where, ord, cost, parts);
        sp = xcd_grouped_order(where, sp, cost, parts);
    }
    ent.insert(ent.end(), sp.begin(), sp.end());
    return ent;
}

// ---- wavefront path-traced frames (launch_pt_frame)
// The samples of a frame of npix pixels run in batches whose path state fits `budget` bytes
// (RT_PT_MEM_MB): per path 32 B of state, 16 B of radiance, 8 B of queue entries and 32 B of record
// per bounce level; a batch never holds more than 2^31 paths (their indices are 32 bits wide).
//   np       paths of a whole batch;
//   seg_cap  entries of one of the `segs` queue segments: segment k takes the survivors of chunks
//            j = k (mod segs); the grid's wave count is a multiple of segs, so a segment never gets more;
//   qbytes   one level queue; cbytes: queue counts + head counters of every level;
//   need     a path-state slot without its results.
struct PathPlan {
    uint64_t per_path, batch, np, seg_cap, qbytes, cbytes, need;
};
inline PathPlan path_plan(uint32_t spp, uint32_t depth, uint64_t npix, uint64_t budget, uint32_t segs) {
    PathPlan p{};
    p.per_path = 32u + 16u + 8u + (uint64_t)(depth - 1) * 32u;
    p.batch = std::max<uint64_t>(1, budget / (p.per_path * npix));
    p.batch = std::min<uint64_t>(p.batch, spp);
    if (p.batch * npix > 0xffffffffull / 2) p.batch = std::max<uint64_t>(1, (0xffffffffull / 2) / npix);
    p.np = p.batch * npix;
    p.seg_cap = ((p.np / 64u + segs - 1) / segs + 1) * 64u;
    p.qbytes = p.seg_cap * segs * 4u;
    p.cbytes = (uint64_t)(depth + 1) * (2u * segs) * 64u;
    p.need = p.np * (p.per_path - 8u) + 2 * p.qbytes + p.cbytes + 4096u;
    return p;
}
// Path-state slots of pipelined frames: `forced` (RT_PT_SLOTS) or else as many as fit beside 8 GB of
// headroom in `avail` bytes, at least 2.
// A frame of a few M paths (a multi-GPU rank's 1/8 of config 5: 4.1 M) is as long as its deep paths'
// latency chain, and 8 frames in flight overlap more of it (1/8 shard 1.24 -> 1.16-1.18 ms); whole
// 1080p x 16 spp frames lose with more than 4 (7.51 -> 7.61 / 7.72 ms with 6 / 8; profiles/r04/slots)
// (measured with GPU_MAX_HW_QUEUES=8, as bench.py runs path-traced and multi-GPU workloads; with
// HIP's default of 4 queues eight slot streams share them and the measurement does not carry over,
// so the small-batch default is 8 only when the process has at least 8 hardware queues -- ADVICE r4)
inline uint32_t path_slots(uint32_t forced, uint64_t np, int hw_queues, uint64_t need, double avail) {
    uint32_t k = forced ? forced : (np <= (8400u << 10) && hw_queues >= 8 ? 8u : 4u);
    while (k > 2 && (double)k * need + (8ull << 30) > avail) --k;
    return k;
}

}  // namespace rt
