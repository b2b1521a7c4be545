// sched_host.cpp -- the frame-layout arithmetic (csrc/rt_sched.h) on the CPU.  No expectation is
// computed by the header: the oracle is the text the header replaced, transcribed below as old_*
// functions (the sort and split loop of tile_order_step, xcd_grouped_order over its FrameArgs,
// sample_split's loop, frame_pixels, the sizing expressions of launch_pt_frame), and explicit
// properties are checked beside it.  Exits non-zero with a message on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>

#include "rt_sched.h"

using namespace rt;

#define CHECK(cond, ...)                                            \
    do {                                                            \
        if (!(cond)) {                                              \
            std::printf("%s:%d: %s: ", __FILE__, __LINE__, #cond);  \
            std::printf(__VA_ARGS__);                               \
            std::printf("\n");                                      \
            std::exit(1);                                           \
        }                                                           \
    } while (0)

static uint32_t g_rng = 0x9e3779b9u;
static uint32_t rnd() {   // xorshift32
    g_rng ^= g_rng << 13, g_rng ^= g_rng >> 17, g_rng ^= g_rng << 5;
    return g_rng;
}

// ---------------------------------------------------------------- the replaced text
struct OldFrame {   // the fields of FrameArgs and rt_renderer that the old text read
    uint32_t W, H, ntiles_local, shard, nshards, tiles_x, nchunks;
    const uint32_t *tile_map;
    std::vector<uint32_t> map_host;
};

static uint64_t old_frame_pixels(const OldFrame &F, uint32_t shard, uint32_t nshards, uint32_t tiles_x, uint32_t ntiles) {
    uint64_t px = (uint64_t)F.ntiles_local * 64u;
    if ((F.W & 7u) || (F.H & 7u)) {
        px = 0;
        auto add = [&](uint32_t t) {
            uint32_t tx = t % tiles_x, ty = t / tiles_x;
            px += (uint64_t)std::min(8u, F.W - tx * 8) * std::min(8u, F.H - ty * 8);
        };
        if (F.tile_map)
            for (uint32_t t : F.map_host) add(t);
        else
            for (uint32_t t = shard; t < ntiles; t += nshards) add(t);
    }
    return px;
}

static std::vector<uint32_t> old_xcd_grouped_order(const OldFrame &F, const uint32_t *map, const std::vector<uint32_t> &entries,
                                                   const std::vector<uint32_t> &cost, uint32_t parts) {
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
        const uint32_t tile = map ? map[lt] : lt * F.nshards + F.shard;
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
    for (auto &rg : region)
        std::stable_sort(rg.begin(), rg.end(), [&](uint32_t a, uint32_t b) { return ec[a] < ec[b]; });
    std::vector<uint32_t> out;
    out.reserve(n);
    for (uint32_t b = 0; out.size() < n; ++b) {
        for (uint32_t w = 0; w < 4 && out.size() < n; ++w) {
            uint32_t g = b % 8u;
            if (region[g].empty()) {
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

// tile_order_step between the cost read-back and the copy to d_order; *k_out, *tail_out: what it kept
static std::vector<uint32_t> old_tile_order(const OldFrame &F, const std::vector<uint32_t> &cost, bool split_ok, int32_t heavy_split,
                                            uint32_t split_parts, bool xcd_order, uint32_t num_cus, uint32_t *k_out, bool *tail_out) {
    const uint32_t n = F.ntiles_local;
    std::vector<uint32_t> ord(n);
    {
        double sum = 0, mx = 0;
        for (uint32_t c : cost) { sum += c; mx = std::max<double>(mx, c); }
        const double slots = (double)num_cus * 4.0 * 7.0;
        *tail_out = sum > 0 && mx * slots > 2.0 * sum * std::max(1u, F.nchunks);
    }
    for (uint32_t i = 0; i < n; ++i) ord[i] = i;
    std::stable_sort(ord.begin(), ord.end(), [&](uint32_t a, uint32_t b) { return cost[a] > cost[b]; });
    uint32_t k = 0;
    if (split_ok) {
        const int32_t hs = heavy_split;
        k = std::min<uint32_t>(n, hs < 0 ? n / 32u : (uint32_t)hs);
    }
    const uint32_t parts = split_parts;
    std::vector<uint32_t> ent(ord), sp;
    for (uint32_t i = 0; i < k; ++i)
        for (uint32_t q = 0; q < parts; ++q) sp.push_back(ord[i] | 0x80000000u | (q << 28));
    for (uint32_t i = k; i < n; ++i) sp.push_back(ord[i]);
    if (xcd_order && split_ok) {
        const uint32_t *map = F.tile_map ? F.map_host.data() : nullptr;
        ent = old_xcd_grouped_order(F, map, ord, cost, parts);
        sp = old_xcd_grouped_order(F, map, sp, cost, parts);
    }
    ent.insert(ent.end(), sp.begin(), sp.end());
    *k_out = k;
    return ent;
}

static uint32_t old_sample_split(uint32_t spp, bool eligible, uint32_t ntiles_local, uint32_t split_units) {
    uint32_t nchunks = 1;
    if (eligible && spp > 1 && ntiles_local < split_units)
        while (ntiles_local * nchunks < 2u * split_units && nchunks < spp) {
            uint32_t d = nchunks + 1;
            while (spp % d) ++d;
            nchunks = d;
        }
    return nchunks;
}

constexpr uint32_t kQueueSegs = 16;   // rt_dev_types.h
struct OldPlan {
    uint64_t per_path, batch, np, seg_cap;
    size_t qbytes, cbytes, need;
};
static OldPlan old_path_plan(uint32_t spp, uint32_t depth, uint64_t npix, uint64_t budget) {
    const uint64_t per_path = 32u + 16u + 8u + (uint64_t)(depth - 1) * 32u;
    uint64_t batch = std::max<uint64_t>(1, budget / (per_path * npix));
    batch = std::min<uint64_t>(batch, spp);
    if (batch * npix > 0xffffffffull / 2) batch = std::max<uint64_t>(1, (0xffffffffull / 2) / npix);
    const uint64_t np = batch * npix;
    const uint64_t seg_cap = ((np / 64u + kQueueSegs - 1) / kQueueSegs + 1) * 64u;
    const size_t qbytes = (size_t)seg_cap * kQueueSegs * 4u;
    const size_t cbytes = (size_t)(depth + 1) * (2u * kQueueSegs) * 64u;
    const size_t need = (size_t)(np * (per_path - 8u) + 2 * qbytes + cbytes + 4096u);
    return {per_path, batch, np, seg_cap, qbytes, cbytes, need};
}
static uint32_t old_path_slots(uint32_t pt_slots, uint64_t np, int hw_queues, size_t need, double avail) {
    uint32_t k = pt_slots ? pt_slots : (np <= (8400u << 10) && hw_queues >= 8 ? 8u : 4u);
    while (k > 2 && (double)k * need + (8ull << 30) > avail) --k;
    return k;
}

// ---------------------------------------------------------------- orders
static void check_order_properties(const std::vector<uint32_t> &got, const std::vector<uint32_t> &cost, uint32_t k, uint32_t parts,
                                   const char *what) {
    const uint32_t n = (uint32_t)cost.size();
    CHECK(got.size() == (size_t)n + n + (size_t)k * (parts - 1u), "%s: %zu entries", what, got.size());
    CHECK(got.size() <= order_capacity(n), "%s: %zu entries, capacity %llu", what, got.size(), (unsigned long long)order_capacity(n));
    if (k == n && parts == 8) CHECK(got.size() == order_capacity(n), "%s: every tile in eighths fills the capacity", what);
    std::vector<uint32_t> seen(n, 0);
    for (uint32_t i = 0; i < n; ++i) {   // the plain order: a permutation
        CHECK(got[i] < n && !seen[got[i]], "%s: plain entry %u = %08x", what, i, got[i]);
        seen[got[i]] = 1;
    }
    std::vector<uint32_t> whole(n, 0), mask(n, 0);
    for (size_t i = n; i < got.size(); ++i) {
        const uint32_t e = got[i], t = e & 0x0fffffffu;
        CHECK(t < n, "%s: split-order entry %zu = %08x", what, i, e);
        if (e >> 31) {
            const uint32_t q = (e >> 28) & 7u;
            CHECK(q < parts && !(mask[t] >> q & 1u), "%s: tile %u part %u twice or out of range", what, t, q);
            mask[t] |= 1u << q;
            // the kernel's lanes of part q are [q << shift, (q + 1) << shift): all 64 lanes over `parts` parts
            CHECK(((q + 1u) << part_shift(parts)) <= 64u && (parts << part_shift(parts)) == 64u, "%s: part_shift", what);
        } else {
            CHECK(e == t, "%s: a whole tile's entry carries part bits: %08x", what, e);
            whole[t] += 1;
        }
    }
    uint32_t nsplit = 0, min_split = 0xffffffffu, max_whole = 0;
    for (uint32_t t = 0; t < n; ++t) {
        if (mask[t]) {
            CHECK(mask[t] == (1u << parts) - 1u && whole[t] == 0, "%s: tile %u parts %x whole %u", what, t, mask[t], whole[t]);
            ++nsplit;
            min_split = std::min(min_split, cost[t]);
        } else {
            CHECK(whole[t] == 1, "%s: tile %u appears %u times", what, t, whole[t]);
            max_whole = std::max(max_whole, cost[t]);
        }
    }
    CHECK(nsplit == k, "%s: %u tiles split, %u wanted", what, nsplit, k);
    if (k && k < n) CHECK(min_split >= max_whole, "%s: a split tile is cheaper than a whole one", what);
    CHECK(order_units(n, 1, true, k, parts) == got.size() - n, "%s: order_units of the split order", what);
    CHECK(order_units(n, 1, false, k, parts) == n, "%s: order_units of the plain order", what);
}

static void test_orders() {
    const uint32_t sizes[] = {1, 2, 3, 4, 5, 31, 32, 33, 47, 64, 257, 2025};
    const uint32_t part_counts[] = {2, 4, 8};
    const uint32_t shards[4][2] = {{0, 1}, {1, 2}, {7, 8}, {0, 1}};   // the fourth: an explicit shuffled map
    size_t cases = 0;
    for (uint32_t n : sizes) {
        const int32_t heavy[] = {-1, 0, 1, 4, 64, (int32_t)n + 5};
        for (int place = 0; place < 4; ++place) {
            OldFrame F{};
            F.ntiles_local = n;
            F.shard = shards[place][0];
            F.nshards = shards[place][1];
            F.tiles_x = 25;
            F.nchunks = 1;
            if (place == 3) {   // n of n + n / 3 + 1 global tiles, shuffled
                std::vector<uint32_t> all(n + n / 3 + 1);
                std::iota(all.begin(), all.end(), 0u);
                for (size_t i = all.size() - 1; i > 0; --i) std::swap(all[i], all[rnd() % (i + 1)]);
                F.map_host.assign(all.begin(), all.begin() + n);
                F.tile_map = F.map_host.data();   // (the device list: only its presence is read)
            }
            const TileWhere where{F.tiles_x, F.shard, F.nshards, F.tile_map ? F.map_host.data() : nullptr};
            for (int kind = 0; kind < 4; ++kind) {
                std::vector<uint32_t> cost(n);
                for (uint32_t i = 0; i < n; ++i)
                    cost[i] = kind == 0 ? 1000u : kind == 1 ? 0u : kind == 2 ? (i == n / 2 ? 0xffffffffu : 1u) : rnd() % 5000u;
                for (uint32_t parts : part_counts)
                    for (int32_t hs : heavy)
                        for (int split_ok = 0; split_ok < 2; ++split_ok)
                            for (int xcd = 0; xcd < 2; ++xcd) {
                                char what[128];
                                std::snprintf(what, sizeof(what), "n %u place %d cost %d parts %u heavy %d split_ok %d xcd %d", n, place,
                                              kind, parts, hs, split_ok, xcd);
                                uint32_t k_want = 0;
                                bool tail_want = false;
                                const std::vector<uint32_t> want =
                                    old_tile_order(F, cost, split_ok != 0, hs, parts, xcd != 0, 256, &k_want, &tail_want);
                                const uint32_t k = split_count(n, hs, split_ok != 0);
                                CHECK(k == k_want, "%s: split_count %u, the old text %u", what, k, k_want);
                                CHECK(tail_bound(cost, 256, F.nchunks) == tail_want, "%s: tail_bound", what);
                                const std::vector<uint32_t> got = build_tile_order(cost, k, parts, xcd != 0 && split_ok != 0, where);
                                CHECK(got == want, "%s: the order differs from the old text's", what);
                                check_order_properties(got, cost, k, parts, what);
                                if (kind == 0 && !xcd)   // equal costs: the stable sort keeps the tiles' own order
                                    for (uint32_t i = 0; i < n; ++i) CHECK(got[i] == i, "%s: stability at %u", what, i);
                                ++cases;
                            }
            }
        }
    }
    // the case test_edits_under_schedule_gpu names: shard 1 of 8 of 375 tiles, every one of its 47 tiles in eighths
    {
        std::vector<uint32_t> cost(47);
        for (uint32_t &c : cost) c = rnd() % 100000u;
        CHECK(local_tiles(375, 1, 8) == 47, "47 tiles");
        const uint32_t k = split_count(47, 64, true);
        CHECK(k == 47, "every tile split");
        for (int xcd = 0; xcd < 2; ++xcd) {
            const std::vector<uint32_t> got = build_tile_order(cost, k, 8, xcd != 0, TileWhere{25, 1, 8, nullptr});
            CHECK(got.size() - 47 == 9u * 47u - 47u && got.size() == 47u + 8u * 47u, "n 47: %zu entries", got.size());
            CHECK(got.size() == order_capacity(47) && order_capacity(47) == 9u * 47u, "n 47: capacity");
            check_order_properties(got, cost, k, 8, "n 47 parts 8");
        }
    }
    // tail_bound over chunk counts and CU counts, against the old expression
    for (uint32_t nchunks : {0u, 1u, 2u, 16u})
        for (uint32_t cus : {1u, 64u, 256u})
            for (int rep = 0; rep < 50; ++rep) {
                OldFrame F{};
                F.ntiles_local = 1 + rnd() % 300;
                F.nshards = 1, F.tiles_x = 25, F.nchunks = nchunks;
                std::vector<uint32_t> cost(F.ntiles_local);
                for (uint32_t &c : cost) c = rnd() % 1000u;
                if (rep & 1) cost[rnd() % cost.size()] = 50000u * (1 + rnd() % 200);
                uint32_t k = 0;
                bool want = false;
                old_tile_order(F, cost, false, 0, 2, false, cus, &k, &want);
                CHECK(tail_bound(cost, cus, nchunks) == want, "tail_bound cus %u nchunks %u", cus, nchunks);
            }
    CHECK(part_shift(2) == 5 && part_shift(4) == 4 && part_shift(8) == 3, "part_shift");
    // order_units with sample chunks (never split then) as the old expression
    for (uint32_t n : {1u, 47u, 510u})
        for (uint32_t c : {1u, 2u, 8u})
            for (uint32_t k : {0u, 5u})
                for (uint32_t parts : {2u, 4u, 8u})
                    for (int split = 0; split < 2; ++split)
                        CHECK(order_units(n, c, split != 0, k, parts) == n * c + (split ? k * (parts - 1u) : 0u), "order_units");
    std::printf("orders: %zu cases\n", cases);
}

// ---------------------------------------------------------------- sample chunks
static void test_sample_chunks() {
    for (uint32_t spp = 1; spp <= 64; ++spp)
        for (uint32_t nt : {1u, 7u, 47u, 510u, 39999u, 40000u})
            for (uint32_t units : {0u, 1u, 40000u, 1000000u})
                for (int eligible = 0; eligible < 2; ++eligible) {
                    const uint32_t got = sample_chunks(spp, nt, units, eligible != 0);
                    CHECK(got == old_sample_split(spp, eligible != 0, nt, units), "sample_chunks spp %u tiles %u units %u: %u", spp, nt,
                          units, got);
                    CHECK(got >= 1 && got <= spp && spp % got == 0, "sample_chunks spp %u tiles %u units %u: %u does not divide", spp, nt,
                          units, got);
                    if (!eligible || units == 0 || nt >= units) CHECK(got == 1, "sample_chunks: split where it must not");
                }
}

// ---------------------------------------------------------------- the grid and the pixels
static uint64_t pixel_count(uint32_t W, uint32_t H, const std::vector<uint32_t> &tiles) {   // one pixel at a time
    const uint32_t tx = (W + 7) / 8, ty = (H + 7) / 8;
    std::vector<uint8_t> in(tx * ty, 0);
    for (uint32_t t : tiles) in[t] = 1;
    uint64_t px = 0;
    for (uint32_t y = 0; y < H; ++y)
        for (uint32_t x = 0; x < W; ++x) px += in[(y / 8) * tx + x / 8];
    return px;
}

static void test_pixels() {
    const uint32_t sizes[][4] = {{8, 8, 1, 1}, {9, 9, 2, 2}, {60, 36, 8, 5}, {64, 40, 8, 5}, {1920, 1080, 240, 135}};
    for (const auto &sz : sizes) {
        const uint32_t W = sz[0], H = sz[1];
        const TileGrid g = tile_grid(W, H);
        CHECK(g.tiles_x == sz[2] && g.tiles_y == sz[3] && g.ntiles == sz[2] * sz[3], "tile_grid %u x %u", W, H);
        const uint32_t shards[][2] = {{0, 1}, {3, 8}};
        for (const auto &sh : shards) {
            std::vector<uint32_t> tiles;
            for (uint32_t t = sh[0]; t < g.ntiles; t += sh[1]) tiles.push_back(t);
            const uint32_t nl = local_tiles(g.ntiles, sh[0], sh[1]);
            CHECK(nl == tiles.size(), "local_tiles %u x %u shard %u/%u: %u", W, H, sh[0], sh[1], nl);
            CHECK(nl == (sh[0] < g.ntiles ? (g.ntiles - sh[0] + sh[1] - 1) / sh[1] : 0), "local_tiles: the old formula");
            OldFrame F{};
            F.W = W, F.H = H, F.ntiles_local = nl;
            const uint64_t got = frame_pixels(W, H, nl, sh[0], sh[1], nullptr);
            CHECK(got == old_frame_pixels(F, sh[0], sh[1], g.tiles_x, g.ntiles), "frame_pixels %u x %u shard %u/%u", W, H, sh[0], sh[1]);
            CHECK(got == pixel_count(W, H, tiles), "frame_pixels %u x %u shard %u/%u: %llu", W, H, sh[0], sh[1], (unsigned long long)got);
        }
        // lists: every tile shuffled, a prefix of it (with the partial edge tiles somewhere in it), none
        std::vector<uint32_t> all(g.ntiles);
        std::iota(all.begin(), all.end(), 0u);
        for (size_t i = all.size() - 1; i > 0; --i) std::swap(all[i], all[rnd() % (i + 1)]);
        for (size_t take : {all.size(), (all.size() + 1) / 2, (size_t)1, (size_t)0}) {
            OldFrame F{};
            F.W = W, F.H = H, F.ntiles_local = (uint32_t)take;
            F.map_host.assign(all.begin(), all.begin() + take);
            F.tile_map = all.data();
            const uint64_t got = frame_pixels(W, H, (uint32_t)take, 0, 1, all.data());   // its first `take` entries
            CHECK(got == old_frame_pixels(F, 0, 1, g.tiles_x, g.ntiles), "frame_pixels %u x %u list of %zu", W, H, take);
            CHECK(got == pixel_count(W, H, F.map_host), "frame_pixels %u x %u list of %zu: %llu", W, H, take, (unsigned long long)got);
        }
    }
    // a shard past the last tile is empty
    CHECK(local_tiles(1, 3, 8) == 0 && frame_pixels(8, 8, 0, 3, 8, nullptr) == 0 && frame_pixels(9, 9, 0, 5, 8, nullptr) == 0, "empty shard");
}

static void test_held_tiles() {
    const TileGrid g = tile_grid(60, 36);
    CHECK(g.ntiles == 40, "60 x 36 is 40 tiles");
    std::vector<uint32_t> got{7, 7, 7};
    const std::vector<uint32_t> list{39, 0, 17, 8};
    CHECK(!held_tiles(0, g.ntiles, 0, 1, list, got) && got.empty(), "held kind 0: nothing yet");
    CHECK(held_tiles(1, g.ntiles, 5, 8, list, got) && got.size() == 40, "held kind 1");
    for (uint32_t t = 0; t < 40; ++t) CHECK(got[t] == t, "held kind 1: tile %u", t);
    CHECK(held_tiles(2, g.ntiles, 3, 8, list, got) && got == (std::vector<uint32_t>{3, 11, 19, 27, 35}), "held kind 2: shard 3 of 8");
    CHECK(held_tiles(2, g.ntiles, 7, 8, list, got) && got == (std::vector<uint32_t>{7, 15, 23, 31, 39}), "held kind 2: shard 7 of 8");
    CHECK(held_tiles(3, g.ntiles, 3, 8, list, got) && got == list, "held kind 3: the list as given");
    CHECK(!held_tiles(4, g.ntiles, 0, 1, list, got) && got.empty(), "held: unknown kind");
}

// ---------------------------------------------------------------- path-traced frames
static void test_path_plan() {
    const uint64_t kDefaultBudget = 12288ull << 20, kHuge = ~(uint64_t)0 >> 8;   // RT_PT_MEM_MB's default
    std::vector<uint64_t> npixes;
    const uint32_t dims[][2] = {{8, 8}, {60, 36}, {200, 120}, {1280, 720}, {1920, 1080}};
    for (const auto &wh : dims) npixes.push_back((uint64_t)tile_grid(wh[0], wh[1]).ntiles * 64u);
    CHECK(npixes.front() == 64 && npixes.back() == 240u * 135u * 64u, "npix from 64 to 1920 x 1080 rounded to tiles");
    npixes.push_back(0xffffffffull / 2 + 64);   // one sample is already past the 32-bit path cap
    size_t capped = 0, batch_one = 0, batch_all = 0;
    for (uint32_t depth : {2u, 4u, 10u, 32u})
        for (uint32_t spp : {1u, 4u, 16u, 64u})
            for (uint64_t npix : npixes) {
                const uint64_t per_path = 32 + 16 + 8 + (uint64_t)(depth - 1) * 32;
                for (uint64_t budget : {per_path * npix - 1, kDefaultBudget, kHuge}) {
                    const OldPlan w = old_path_plan(spp, depth, npix, budget);
                    const PathPlan p = path_plan(spp, depth, npix, budget, kQueueSegs);
                    CHECK(p.per_path == w.per_path && p.batch == w.batch && p.np == w.np && p.seg_cap == w.seg_cap && p.qbytes == w.qbytes &&
                              p.cbytes == w.cbytes && p.need == w.need,
                          "path_plan depth %u spp %u npix %llu budget %llu", depth, spp, (unsigned long long)npix, (unsigned long long)budget);
                    CHECK(p.per_path == per_path && p.batch >= 1 && p.batch <= spp && p.np == p.batch * npix, "path_plan: batch");
                    if (budget < per_path * npix) {
                        CHECK(p.batch == 1, "a budget below one path set: one sample a batch");
                        ++batch_one;
                    }
                    if (budget == kHuge && (uint64_t)spp * npix <= 0xffffffffull / 2) {
                        CHECK(p.batch == spp, "a huge budget: one batch");
                        ++batch_all;
                    }
                    if (npix > 0xffffffffull / 2) {
                        CHECK(p.batch == 1, "past the path cap: batch 1");
                        ++capped;
                    } else {
                        CHECK(p.np <= 0xffffffffull / 2, "a batch holds at most 2^31 paths");
                    }
                    // the segments together hold every path of the batch
                    CHECK(p.seg_cap % 64 == 0 && p.seg_cap * kQueueSegs >= p.np, "seg_cap");
                    // slots
                    for (uint32_t forced = 2; forced <= 8; ++forced)
                        CHECK(path_slots(forced, p.np, 4, p.need, 1e18) == forced && old_path_slots(forced, p.np, 4, w.need, 1e18) == forced,
                              "forced slots");
                    for (int hw : {4, 8})
                        for (double avail : {1e18, 3.0 * (double)p.need + (double)(8ull << 30), 0.0}) {
                            const uint32_t k = path_slots(0, p.np, hw, p.need, avail);
                            CHECK(k == old_path_slots(0, p.np, hw, w.need, avail), "path_slots hw %d avail %g", hw, avail);
                            if (avail == 0.0) CHECK(k == 2, "no memory trims to 2 slots");
                            if (avail == 1e18) CHECK(k == (hw >= 8 && p.np <= (8400ull << 10) ? 8u : 4u), "default slots: %u", k);
                            CHECK(path_slots(8, p.np, hw, p.need, avail) == old_path_slots(8, p.np, hw, w.need, avail), "forced 8, trimmed");
                        }
                }
            }
    CHECK(capped && batch_one && batch_all, "every budget class was reached");
    // either side of 8400 << 10 paths
    const uint64_t edge = 8400ull << 10;
    for (uint64_t np : {edge - 1, edge + 0, edge + 1})
        for (int hw : {4, 7, 8, 32}) {
            const uint32_t want = np <= edge && hw >= 8 ? 8u : 4u;
            CHECK(path_slots(0, np, hw, 1 << 20, 1e18) == want && old_path_slots(0, np, hw, 1 << 20, 1e18) == want, "slots at %llu paths, %d queues",
                  (unsigned long long)np, hw);
        }
    // the trim: k slots fit exactly, k + 1 do not
    const uint64_t need = 3ull << 30;
    for (uint32_t fit = 1; fit <= 8; ++fit) {
        const double avail = (double)fit * need + (double)(8ull << 30);
        for (uint32_t forced : {0u, 8u}) {
            const uint32_t start = forced ? forced : 4u;
            const uint32_t want = std::max(2u, std::min(start, fit));
            CHECK(path_slots(forced, edge + 1, 8, need, avail) == want, "trim: %u fit, forced %u", fit, forced);
            CHECK(old_path_slots(forced, edge + 1, 8, need, avail) == want, "trim (old text): %u fit, forced %u", fit, forced);
        }
    }
}

int main() {
    test_orders();
    test_sample_chunks();
    test_pixels();
    test_held_tiles();
    test_path_plan();
    std::printf("sched_host ok\n");
    return 0;
}
