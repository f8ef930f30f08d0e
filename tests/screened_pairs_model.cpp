// Host program of tests/test_screened_pairs_cpu.py — a helper of that test, not part of the library.
//
// It compiles csrc/mcr_events.h (the event row and the pair cursor, the very code path_kernel's paired consumer runs) with
// the host compiler and holds it to plain restatements:
//
//   schedule   the paired consumer's loops (csrc/mcr_hip.hip, "PAIRS"), restated here statement for statement without the
//              arithmetic, against the consumer of the other split kernels (begin_month: a barrier in front of every even
//              row) and against both producer forms (one producer wave set: a barrier behind every pair; two producer waves:
//              the `handover` hooks of NPROD = 2).  A barrier is a workgroup barrier, so wave by wave the k-th barrier must be
//              the same one: same count, same pair, same vote flag, and for the consumers the same row in front of which it stands.
//              The outcome of vote v is an input (`dead_vote`: the vote that finds no lane alive; -1: none).
//   events     the event row against the month's own tests on every row: the window predicate (unsigned)(row - s) < n and
//              the priority compare chain.
//
// Prints one line per section, "schedule ok <cases>" / "events ok <cases>"; on a mismatch a description, exit status 1.
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mcr_events.h"

namespace {
constexpr int kMPY = 12, kVotePairs = 16, kStageLen = 6 * 64;

struct Barrier { int pair, row, vote; unsigned off; };     // row: the row the wave stands in front of (-1: a producer)
using Trace = std::vector<Barrier>;

// ---- the paired consumer, as csrc/mcr_hip.hip states it ----
Trace paired_consumer(int wm, int ry, int dead_vote) {
    Trace t;
    PairCursor PC{0, 0u};
    int row = 0, dead = 0, votes = 0;
    auto handover = [&]() {
        if (dead) return;
        const bool vote = pair_votes(PC, kVotePairs);
        t.push_back({PC.pair, row, vote ? 1 : 0, PC.off});
        if (vote && votes++ == dead_vote) { dead = 1; return; }
        pair_advance(PC, (unsigned)kStageLen);
    };
    auto month = [&]() { ++row; };
    {
        int m = 1;
        for (; m < wm; m += 2) { handover(); month(); month(); }
        if (m == wm) { handover(); month(); }
    }
    auto ret_years = [&](bool odd) {
        for (int year = 0; year < ry; ++year) {
            if (dead) break;
            for (int mi = 0; mi < kMPY; mi += 2) {
                if (odd) { month(); handover(); month(); }
                else { handover(); month(); month(); }
            }
        }
    };
    ret_years((wm & 1) != 0);
    return t;
}
// ---- the consumer of the other split kernels: begin_month in front of every month, the loops that call it ----
Trace classic_consumer(int wm, int ry, int dead_vote) {
    Trace t;
    bool wg_dead = false;
    int votes = 0;
    auto begin_month = [&](int row) {
        if ((row & 1) != 0 || wg_dead) return;
        const bool vote = ((row >> 1) & (kVotePairs - 1)) == 0;
        t.push_back({row >> 1, row, vote ? 1 : 0, (unsigned)(((row >> 1) & 1) * kStageLen)});
        if (vote && votes++ == dead_vote) wg_dead = true;
    };
    for (int m = 1; m <= wm; ++m) begin_month(m - 1);
    for (int year = 0; year < ry; ++year) {
        if (wg_dead) break;
        for (int mi = 0; mi < kMPY; ++mi) begin_month(wm + year * kMPY + mi);
    }
    return t;
}
// ---- one producer wave set (NPROD = 1): rows [0, total_months), a pair and its barrier per turn ----
Trace single_producer(int total, int dead_vote) {
    Trace t;
    int votes = 0;
    for (int row = 0; row < total; row += 2) {
        const bool vote = ((row >> 1) & (kVotePairs - 1)) == 0;
        t.push_back({row >> 1, -1, vote ? 1 : 0, (unsigned)(((row >> 1) & 1) * kStageLen)});
        if (vote && votes++ == dead_vote) return t;
    }
    return t;
}
// ---- producer h of two (NPROD = 2): pairs h, h + 2, ...; barrier p - 1 in the middle of pair p, barrier p behind it ----
Trace half_producer(int H, int total, int dead_vote) {
    Trace t;
    const int n_pairs = (total + 1) >> 1;
    int votes = 0;
    bool stop = false;
    auto handover = [&](int q) {
        const bool vote = (q & (kVotePairs - 1)) == 0;
        t.push_back({q, -1, vote ? 1 : 0, (unsigned)((q & 1) * kStageLen)});
        if (vote && votes++ == dead_vote) stop = true;
    };
    int p = H;
    for (; p < n_pairs; p += 2) {
        if (p > 0) handover(p - 1);
        if (stop) return t;
        handover(p);
        if (stop) return t;
    }
    if (p == n_pairs && p > 0) handover(p - 1);
    return t;
}

bool same(const Trace& a, const Trace& b, bool rows, const char* what, int wm, int ry, int dead_vote) {
    bool ok = a.size() == b.size();
    for (size_t k = 0; ok && k < a.size(); ++k)
        ok = a[k].pair == b[k].pair && a[k].vote == b[k].vote && a[k].off == b[k].off && (!rows || a[k].row == b[k].row);
    if (!ok) std::printf("schedule MISMATCH %s: working_months %d retirement_years %d dead_vote %d: %zu vs %zu barriers\n", what, wm, ry, dead_vote, a.size(), b.size());
    return ok;
}

int schedules() {
    int cases = 0;
    const int years[] = {1, 2, 40};
    for (int wm = 0; wm < 48; ++wm)            // every working_months % 24 twice over, hence every total_months % 4
        for (int ry : years) {
            const int total = wm + kMPY * ry, n_pairs = (total + 1) >> 1, n_votes = (n_pairs + kVotePairs - 1) / kVotePairs;
            for (int dead_vote = -1; dead_vote < n_votes; ++dead_vote) {
                const Trace c = paired_consumer(wm, ry, dead_vote);
                bool ok = same(c, classic_consumer(wm, ry, dead_vote), true, "paired vs classic consumer", wm, ry, dead_vote)
                       && same(c, single_producer(total, dead_vote), false, "paired consumer vs the producer of the 256-path form", wm, ry, dead_vote)
                       && same(c, half_producer(0, total, dead_vote), false, "paired consumer vs producer 0 of two", wm, ry, dead_vote)
                       && same(c, half_producer(1, total, dead_vote), false, "paired consumer vs producer 1 of two", wm, ry, dead_vote);
                // barrier p stands in front of row 2 p, hands over buffer p & 1, votes at every 16th; none is left out
                for (size_t k = 0; ok && k < c.size(); ++k)
                    ok = c[k].pair == (int)k && c[k].row == 2 * (int)k && c[k].off == (unsigned)((k & 1) * kStageLen) && c[k].vote == ((k % kVotePairs) == 0 ? 1 : 0);
                if (ok && dead_vote < 0) ok = (int)c.size() == n_pairs;
                if (ok && dead_vote >= 0) ok = (int)c.size() == dead_vote * kVotePairs + 1;
                if (!ok) { std::printf("schedule FAILED: working_months %d retirement_years %d dead_vote %d\n", wm, ry, dead_vote); return 1; }
                ++cases;
            }
        }
    std::printf("schedule ok %d\n", cases);
    return 0;
}

// the event row over rows [0, total) against the month's own tests
bool events_case(const EventPlan& e, int total, const char* what) {
    EventRow ev = event_begin(e);
    int fired = 0;
    for (int row = 0; row < total; ++row) {
        int prio = -1;
        if (row == ev.next) { prio = event_fire(ev, e, row); ++fired; }
        const int w0 = (unsigned)(row - e.s0) < e.n0 ? 1 : 0, w1 = (unsigned)(row - e.s1) < e.n1 ? 1 : 0;
        const int want = row == e.t1 ? 2 : row == e.t2 ? 1 : row == e.t3 ? 0 : -1;
        if (ev.w0 != w0 || ev.w1 != w1 || prio != want || ev.next <= row) {
            std::printf("events MISMATCH %s: t %d %d %d  s0 %d n0 %u  s1 %d n1 %u  row %d: flags %d %d want %d %d, prio %d want %d, next %d\n",
                        what, e.t1, e.t2, e.t3, e.s0, e.n0, e.s1, e.n1, row, ev.w0, ev.w1, w0, w1, prio, want, ev.next);
            return false;
        }
    }
    if (fired > 7) { std::printf("events %s: %d hits, a plan has at most seven rows with an event\n", what, fired); return false; }
    return true;
}
EventPlan plan_of(int total, int s0, unsigned n0, int s1, unsigned n1) { return EventPlan{total / 2, (total * 3) / 4, (total * 9) / 10, s0, n0, s1, n1}; }

int events() {
    int cases = 0;
    const int total = 40;                      // thresholds 20, 30, 36
    const unsigned never0 = (unsigned)(INT_MAX - 20), never1 = (unsigned)(INT_MAX - 7);
    struct Named { const char* what; EventPlan e; int total; };
    const Named named[] = {
        {"both windows open on a threshold row and close on another", plan_of(total, 20, 10u, 20, 16u), total},
        {"an edge of each window and a threshold on one row", plan_of(total, 30, 3u, 25, 5u), total},
        {"a window of length 0 on a threshold row", plan_of(total, 20, 0u, 36, 0u), total},
        {"a window open at row 0", plan_of(total, 0, 5u, 0, 40u), total},
        {"a window that never closes", plan_of(total, 20, never0, 7, never1), total},
        {"a window that opens behind the last row", plan_of(total, 40, 5u, INT_MAX, 0u), total},
        {"one month: all three thresholds on row 0", plan_of(1, 0, 1u, 0, 0u), 1},
        {"two months", plan_of(2, 1, 1u, 0, 1u), 2},
        {"three months", plan_of(3, 1, 2u, 2, never1), 3},
    };
    for (const Named& c : named) { if (!events_case(c.e, c.total, c.what)) return 1; ++cases; }
    // every placement of two windows over a short path: all coincidences of edges with each other and with the thresholds
    const int T = 12;                          // thresholds 6, 9, 10
    for (int s0 = 0; s0 <= T + 1; ++s0)
        for (int s1 = 0; s1 <= T + 1; ++s1)
            for (unsigned k0 = 0; k0 <= (unsigned)T + 2u; ++k0)
                for (unsigned k1 = 0; k1 <= (unsigned)T + 2u; ++k1) {
                    const unsigned n0 = k0 == (unsigned)T + 2u ? (unsigned)(INT_MAX - s0) : k0, n1 = k1 == (unsigned)T + 2u ? (unsigned)(INT_MAX - s1) : k1;
                    if (!events_case(plan_of(T, s0, n0, s1, n1), T, "sweep")) return 1;
                    ++cases;
                }
    std::printf("events ok %d\n", cases);
    return 0;
}
}  // namespace

int main() {
    const int a = schedules(), b = events();
    return (a || b) ? 1 : 0;
}
