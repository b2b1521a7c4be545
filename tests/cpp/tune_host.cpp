// tune_host.cpp -- the timed choices' group schedule (csrc/rt_tune.h) driven with scripted inputs
// on the CPU: which group and event every frame gets, how often a stalled group restarts, what
// the measured group times decide.  Exits non-zero with a message on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

#include "rt_tune.h"

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

// Runs the schedule to its decision; `stall(t)` is the caller's stall flag for the frame about to
// be submitted.  Returns every timed frame.
static std::vector<TimedFrame> run(TimedGroups &t, const std::function<bool(const TimedGroups &)> &stall) {
    std::vector<TimedFrame> out;
    for (int n = 0; n < 100000 && !t.finished(); ++n) {
        const TimedFrame f = t.next(true, stall(t));
        CHECK(!f.decide, "decide before the last timed frame (call %d)", n);
        if (f.group >= 0) out.push_back(f);
    }
    CHECK(t.finished(), "the schedule never finished");
    return out;
}
static bool never(const TimedGroups &) { return false; }
static bool always(const TimedGroups &) { return true; }

// frames per group, and the events of every group: start event 2g on each frame with in-group
// index `start_index` (before it when `before`), end event 2g + 1 after the group's last frame
static void check_groups(const std::vector<TimedFrame> &fr, const TimedGroups &t, int per_group, int start_index, bool before) {
    CHECK((int)fr.size() == per_group * t.groups, "%d frames, want %d", (int)fr.size(), per_group * t.groups);
    for (int k = 0; k < (int)fr.size(); ++k) {
        const TimedFrame &f = fr[k];
        CHECK(f.group == k / per_group, "frame %d in group %d", k, f.group);
        const int start = f.index == start_index ? 2 * f.group : -1, end = f.index == t.frames - 1 ? 2 * f.group + 1 : -1;
        CHECK(f.ev_before == (before ? start : -1), "frame %d: event %d before it", k, f.ev_before);
        CHECK(f.ev_after == (before ? end : start >= 0 ? start : end), "frame %d: event %d after it", k, f.ev_after);
        CHECK((k + 1) % per_group != 0 || f.index == t.frames - 1, "group %d does not end on its last frame", f.group);
    }
}

static void two_way() {
    TimedGroups t;
    CHECK(!t.active() && !t.running() && !t.finished(), "a fresh schedule is off");
    CHECK(t.next(true, true).group < 0 && !t.next(true, true).decide, "a schedule that is off times nothing");
    start_two_way(t, false);
    std::string cand;
    for (int k = 0; k < 16; ++k) {
        CHECK(t.running() && !t.finished(), "frame %d: still running", k);
        const TimedFrame f = t.next(true, false);
        cand += alternative_group(f) ? 'B' : 'A';
        CHECK(f.group == k / 4 && f.index == k % 4, "frame %d is %d.%d", k, f.group, f.index);
        CHECK(f.ev_before == (k % 4 == 0 ? k / 2 : -1), "frame %d: event %d before", k, f.ev_before);       // 0 2 4 6
        CHECK(f.ev_after == (k % 4 == 3 ? k / 2 : -1), "frame %d: event %d after", k, f.ev_after);          // 1 3 5 7
    }
    CHECK(cand == "AAAABBBBBBBBAAAA", "candidates %s", cand.c_str());
    CHECK(t.finished() && !t.running(), "finished after frame 15");
    const TimedFrame d = t.next(false, true);   // decided whatever the gate and the stall flag say
    CHECK(d.decide && d.group < 0 && d.ev_before < 0 && d.ev_after < 0, "the 17th call decides");
    CHECK(!t.active() && !t.next(true, false).decide, "decided once");

    // stalled on every call: 1 + kTuneRestarts restarts + 3 frames per group, the start event again on each restart
    start_two_way(t, false);
    std::vector<TimedFrame> fr = run(t, always);
    check_groups(fr, t, 8, 0, true);
    for (int k = 0; k < 32; ++k) CHECK(fr[k].index == (k % 8 < 5 ? 0 : k % 8 - 4), "frame %d has index %d", k, fr[k].index);

    // stalled only before in-group frame 3: 4 restarts of 3 frames, then the 4 frames of the group
    start_two_way(t, false);
    fr = run(t, [](const TimedGroups &s) { return s.phase % s.frames == 3; });
    check_groups(fr, t, 16, 0, true);
    for (int k = 0; k < 64; ++k) CHECK(fr[k].index == (k % 16 < 12 ? k % 16 % 3 : k % 16 - 12), "frame %d has index %d", k, fr[k].index);
}

static void overlap() {
    TimedGroups t;
    start_overlap(t, true);   // deep: 8 groups of 32, timed from the completion of frame 8
    std::vector<TimedFrame> fr = run(t, never);
    check_groups(fr, t, 32, 8, false);
    CHECK(fr.size() == 256, "deep: %d frames", (int)fr.size());
    const uint32_t deep[8] = {0, 2, 4, 6, 6, 4, 2, 0}, shallow[4] = {0, 2, 2, 0};
    for (int g = 0; g < 8; ++g) CHECK(overlap_depths(t.groups)[g] == deep[g], "deep group %d", g);
    CHECK(fr[8].ev_after == 0 && fr[31].ev_after == 1 && fr[32 * 7 + 8].ev_after == 14 && fr[255].ev_after == 15, "deep events");
    start_overlap(t, true);
    check_groups(run(t, always), t, 36, 8, false);

    start_overlap(t, false);   // shallow: 4 groups of 16, timed from the completion of frame 2
    fr = run(t, never);
    check_groups(fr, t, 16, 2, false);
    CHECK(fr.size() == 64 && fr[2].ev_after == 0 && fr[15].ev_after == 1 && fr[63].ev_after == 7, "shallow events");
    for (int g = 0; g < 4; ++g) CHECK(overlap_depths(t.groups)[g] == shallow[g], "shallow group %d", g);
    start_overlap(t, false);
    check_groups(run(t, always), t, 20, 2, false);

    // interrupted in the middle of a deep timing: from frame 0 again, and the shape may change
    start_overlap(t, true);
    for (int k = 0; k < 100; ++k) t.next(true, false);
    CHECK(t.running() && t.phase == 100, "in the fourth deep group");
    t.reset();
    CHECK(t.phase == 0 && t.groups == 8, "reset: the same shape from its first frame");
    TimedFrame f = t.next(true, true);
    CHECK(f.group == 0 && f.index == 0, "the first frame after a reset is %d.%d", f.group, f.index);
    t.stop();
    CHECK(!t.active() && !t.running(), "stopped");
    start_overlap(t, false);
    fr = run(t, never);
    check_groups(fr, t, 16, 2, false);
}

static void walk() {
    TimedGroups t;
    start_two_way(t, true);
    CHECK(t.active() && !t.running(), "before the warm-up frame");
    for (int k = 0; k < 3; ++k) CHECK(t.next(false, false).group < 0 && !t.running(), "the gate holds the warm-up back");
    TimedFrame f = t.next(true, true);
    CHECK(f.group < 0 && f.ev_before < 0 && f.ev_after < 0 && !f.decide && walk_cost_map(f) < 0, "the warm-up frame is untimed");
    CHECK(t.running(), "timed frames follow the warm-up");
    for (int k = 0; k < 6; ++k) {
        f = t.next(true, false);
        CHECK(f.group == k / 4 && f.index == k % 4, "timed frame %d is %d.%d", k, f.group, f.index);
        CHECK(walk_cost_map(f) == (k == 0 ? 0 : k == 4 ? 1 : -1), "timed frame %d: cost map %d", k, walk_cost_map(f));
    }
    t.reset();   // the parameter set changed at a timed frame
    CHECK(!t.running() && t.next(true, false).group < 0, "back to the warm-up");
    for (int k = 0; k < 16; ++k) {
        for (int h = 0; h < 3; ++h) {   // a closed gate freezes the phase
            const int before = t.phase;
            f = t.next(false, true);
            CHECK(f.group < 0 && !f.decide && t.phase == before, "frame %d ran with the gate closed", k);
        }
        f = t.next(true, false);
        CHECK(f.group == k / 4 && f.index == k % 4, "timed frame %d is %d.%d", k, f.group, f.index);
        CHECK(walk_cost_map(f) == (k == 0 ? 0 : k == 4 ? 1 : -1), "timed frame %d: cost map %d", k, walk_cost_map(f));
        CHECK(walk_cost_map(f) < 0 || f.ev_before == 2 * f.group, "the cost map goes with the group's first frame");
    }
    CHECK(t.finished(), "16 timed frames");
    CHECK(t.next(false, false).decide, "a closed gate does not hold the decision back");
}

static void decisions() {
    const float eq[4] = {1, 1, 1, 1}, b2[4] = {1, 0.98f, 0.98f, 1}, b4[4] = {1, 0.96f, 0.96f, 1};
    CHECK(!tuned_alternative(eq) && !tuned_alternative(b2) && tuned_alternative(b4), "two-way: A, A, B");
    CHECK(tuned_depth(eq, 4) == 0 && tuned_depth(b2, 4) == 0 && tuned_depth(b4, 4) == 2, "shallow depth: 0, 0, 2");
    float d[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    CHECK(tuned_depth(d, 8) == 4, "deep, all equal: %u", tuned_depth(d, 8));
    d[0] = d[7] = 0.95f;
    CHECK(tuned_depth(d, 8) == 0, "deep, serial 5 %% ahead: %u", tuned_depth(d, 8));
    d[0] = d[7] = 1;
    d[1] = d[6] = 0.96f;   // 2 in flight beats 4 by the margin; 6 beats 4 by more, but not 2 by the margin
    d[3] = d[4] = 0.95f;
    CHECK(tuned_depth(d, 8) == 2, "deep, 2 then 6: %u", tuned_depth(d, 8));
    d[1] = d[6] = 1;
    CHECK(tuned_depth(d, 8) == 6, "deep, 6 alone 5 %% ahead: %u", tuned_depth(d, 8));
}

int main() {
    two_way();
    overlap();
    walk();
    decisions();
    std::printf("tune_host ok\n");
    return 0;
}
