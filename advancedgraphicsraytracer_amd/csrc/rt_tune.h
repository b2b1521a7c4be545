// rt_tune.h -- the schedule of the renderer's timed choices (camera walk, half-tile split order,
// frames in flight), host only: which group a frame belongs to, which of the caller's events go
// around it, when a group restarts, what the group times decide (tests/cpp/tune_host.cpp).
#pragma once

#include <cstdint>

namespace rt {

// The timed choices between two variants (camera walk, split order) time four groups of
// kTuneGroup frames in the order A, B, B, A (a clock drift over the groups cancels) and keep
// the faster -- single frames were too noisy to decide on (ranks with equal work came out 35 %
// apart in round-3 shard timings)
constexpr int kTuneGroup = 4;
// A timed choice between the default (groups 0 and 3) and an alternative (groups 1 and 2),
// groups run A, B, B, A: the alternative must win by kTuneMargin.  The palindrome cancels a
// linear clock drift, not a first group that still runs slow: TEAPOT-F 1080p timed its plain
// order at 0.4986 / 0.4195 ms per group against 0.4531 / 0.4551 for the half-tile split, whose
// sum looked 1 % faster -- and its frames then ran at 0.114 instead of 0.104 ms (bench config 2
// after a config-4 run on the same box, round 3).  The choices that pay win by 8-40 %.
constexpr float kTuneMargin = 0.03f;
inline bool tuned_alternative(const float ms[4]) { return ms[1] + ms[2] < (ms[0] + ms[3]) * (1.0f - kTuneMargin); }
// A timed group assumes frames submitted back to back.  When the caller synchronises inside a
// group (bench.py's clock ramp every 20 frames, multi_overhead.py every 50), the GPU idles between
// two of its frames and the group times the host, not the frames: TEAPOT-F 1080p with 8 hardware
// queues timed its first serial group at 2.48 ms against 1.58 for the last, picked 2 frames in
// flight and ran at 0.0995 ms against 0.097 serial (round 5, profiles/r05/hwq/).  So while a group
// runs, an event after each frame is queried when the next frame is submitted: if the previous
// frame had already completed, the GPU ran dry in between (`stalled`) and the group restarts (at
// most kTuneRestarts times per group, so a caller that syncs every frame still gets a decision).
constexpr int kTuneRestarts = 4;

struct TimedFrame {   // what TimedGroups::next says about the frame being submitted
    int group = -1, index = -1;          // -1: not a timed frame (warm-up, held back, nothing running)
    int ev_before = -1, ev_after = -1;   // the caller's events to record before / after the frame
    bool decide = false;                 // every group has run: read the group times and decide
};

// `groups` groups of `frames` frames each, after `warmup` untimed frames.  Group g is timed from
// event 2g to event 2g + 1: 2g before the group's first frame (skip 0), or after its frame `skip`
// (the frames before it fill a pipeline); 2g + 1 after its last frame.
struct TimedGroups {
    int groups = 0, frames = 0, skip = 0, warmup = 0;
    int phase = 0;                // -warmup .. -1 warm-up, then groups x frames timed frames, then decide
    bool on = false;              // started and not decided yet
    int rg = -1, restarts = 0;    // restarts used by group rg

    void start(int g, int f, int s, int w = 0) { groups = g, frames = f, skip = s, warmup = w, reset(); }
    void reset() { on = true, phase = -warmup, rg = -1, restarts = 0; }   // from the start again
    void stop() { on = false; }
    bool active() const { return on; }
    bool running() const { return on && phase >= 0 && phase < groups * frames; }   // timed frames to come
    bool finished() const { return on && phase == groups * frames; }                // decision pending

    // Once per frame.  `go` false holds the schedule back (the tuning gate), but not a pending
    // decision; `stalled`: the previous frame had completed before this one was submitted.
    TimedFrame next(bool go, bool stalled) {
        TimedFrame f;
        if (!on) return f;
        if (finished()) { f.decide = true, on = false; return f; }
        if (!go) return f;
        if (phase < 0) { ++phase; return f; }
        if (phase / frames != rg) rg = phase / frames, restarts = 0;
        if (stalled && phase % frames != 0 && restarts < kTuneRestarts)
            phase -= phase % frames, ++restarts;   // redo the group from its first frame
        f.group = phase / frames, f.index = phase % frames;
        if (f.index == skip) (skip ? f.ev_after : f.ev_before) = 2 * f.group;
        if (f.index == frames - 1) f.ev_after = 2 * f.group + 1;
        ++phase;
        return f;
    }
};

// Two-way choices: groups A, B, B, A.  The camera walk runs one warm-up frame first and records
// each walk's tile costs on the first frame of its first group (walk_cost_map: 0 lane, 1 wave).
inline void start_two_way(TimedGroups &t, bool warmup) { t.start(4, kTuneGroup, 0, warmup ? 1 : 0); }
inline bool alternative_group(const TimedFrame &f) { return f.group == 1 || f.group == 2; }
inline int walk_cost_map(const TimedFrame &f) { return f.index == 0 && (f.group == 0 || f.group == 1) ? f.group : -1; }

// Frames in flight.  Groups in palindromic order: serial, 2, 4, 6, 6, 4, 2, serial (deep) or serial,
// 2, 2, serial (shallow).  A group's first frames fill its pipeline (every renderer stream starts
// behind the previous group), and their completions bunch up: timed from the first frame's
// completion, a 6-deep group of 16 frames measured 0.23-0.25 ms per frame on mig29 x16 whose 6-deep
// frames then ran at 0.272 ms against 0.256 with 4 (round 5).  Deep timings run 32-frame groups and
// time them from the completion of frame 8 (23 periods), shallow ones 16 frames from frame 2.
constexpr int kPsGroup = 16;  // frames per timed group of the overlap decision (8 in round 3)
constexpr uint32_t kPsDeep[8] = {0, 2, 4, 6, 6, 4, 2, 0}, kPsShallow[4] = {0, 2, 2, 0};
inline const uint32_t *overlap_depths(int groups) { return groups == 8 ? kPsDeep : kPsShallow; }
inline void start_overlap(TimedGroups &t, bool deep) { deep ? t.start(8, 2 * kPsGroup, 8) : t.start(4, kPsGroup, 2); }
// Group g and its mirror groups - 1 - g ran the same depth.  Shallow candidates (serial, 2): 2 in
// flight replaces serial only when it beats it by kTuneMargin, so noise does not buy frames in
// flight.  Deep candidates (tail-bound or small frames: serial, 2, 4, 6): 4 in flight is the
// default, which another depth replaces only when it beats it by kTuneMargin -- the deep groups
// time a deeper pipeline's gain short (mig29 x16: 4 in flight 1.9 % ahead of 2 in its groups, 3.5 %
// ahead in steady state, 0.236-0.238 against 0.246 ms; profiles/r05/c4depth), so with serial as
// the default the choice between 2 and 4 was a coin toss
inline uint32_t tuned_depth(const float *ms, int groups) {
    const uint32_t *depths = overlap_depths(groups);
    const int pref = groups == 8 ? 2 : 0;
    float best = ms[pref] + ms[groups - 1 - pref];
    uint32_t use = depths[pref];
    for (int g = 0; g < groups / 2; ++g) {
        const float t = ms[g] + ms[groups - 1 - g];
        if (g != pref && t < best * (1.0f - kTuneMargin)) { best = t; use = depths[g]; }
    }
    return use;
}

}  // namespace rt
