// Wave-uniform bookkeeping of the split re-run's consumer wave (path_kernel under SPLIT && LIST): the EVENT ROW and the PAIR
// CURSOR.  A lone consumer wave issues in order, so every scalar instruction of its month is on the path's dependent chain;
// what a month used to test every time (three priority thresholds, two income windows, the stage's parity, the vote period)
// is kept here as state that changes on a handful of rows of a path.  Plain C++ without a device dependency: the same code
// is compiled into the kernel and into the host program of tests/test_screened_pairs_cpu.py.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MCR_EV_FN __host__ __device__ __forceinline__
#else
#define MCR_EV_FN inline
#endif
// On the device the three words of the state are made opaque 32-bit scalars where they are set: left to itself the compiler
// turns a 0 / 1 flag into a condition, carries it from block to block as a lane mask, parks it in a VGPR, and the month tests it
// with v_cmp + s_cbranch_vcc instead of s_cmp + s_cbranch_scc.  (v_readfirstlane first, on the few rows with an event: an "s"
// constraint on the value itself is refused as an illegal VGPR to SGPR copy; the empty asm second, or the compiler still
// knows the word to be 0 or 1 and makes a condition of it again.)
#if defined(__HIP_DEVICE_COMPILE__)
#define MCR_EV_SCALAR(x) do { (x) = __builtin_amdgcn_readfirstlane(x); asm volatile("" : "+s"(x)); } while (0)
#else
#define MCR_EV_SCALAR(x) ((void)(x))
#endif

// The rows at which something happens to the wave: the priority falls at t1 <= t2 <= t3 (path_kernel's prio_t1 .. prio_t3), and
// window k of StreamRegs is open on the rows s_k <= row < s_k + n_k, i.e. (unsigned)(row - s_k) < n_k (n_k = 0: never).
struct EventPlan { int t1, t2, t3; int s0; unsigned n0; int s1; unsigned n1; };
// next: the first row >= the current one at which an event falls (INT32_MAX: none is left); w0 / w1: window k is open on the
// current row.  Rows come up in order 0, 1, 2, ..., so a month compares its row with `next` once and reads the two flags.
struct EventRow { int next; int w0, w1; };

// the row on which a window closes; INT32_MAX when it never does (no row reaches INT32_MAX)
MCR_EV_FN int event_close_row(int s, unsigned n) {
    const unsigned c = (unsigned)s + n;
    return (c < (unsigned)s || c >= (unsigned)INT32_MAX) ? INT32_MAX : (int)c;
}
// the first row >= from at which an event falls
MCR_EV_FN int event_next(const EventPlan& e, int from) {
    int r = INT32_MAX;
    auto take = [&](int x) { if (x >= from && x < r) r = x; };
    take(e.t1); take(e.t2); take(e.t3);
    if (e.n0 != 0u) { take(e.s0); take(event_close_row(e.s0, e.n0)); }
    if (e.n1 != 0u) { take(e.s1); take(event_close_row(e.s1, e.n1)); }
    return r;
}
// the state in front of row 0: nothing is open yet (a window that opens AT row 0 is row 0's event)
MCR_EV_FN EventRow event_begin(const EventPlan& e) {
    EventRow ev{event_next(e, 0), 0, 0};
    MCR_EV_SCALAR(ev.w0); MCR_EV_SCALAR(ev.w1); MCR_EV_SCALAR(ev.next);
    return ev;
}
// Row `row` == ev.next: every event of the row fires.  The window flags are restated from the month's own predicate, so an
// edge of each window, or edges and a threshold, on one row need no order among them.  Returns the priority the wave falls
// to on this row (2, 1, 0: the first threshold that matches, as the compare chain of the other kernels' month has it), or -1.
MCR_EV_FN int event_fire(EventRow& ev, const EventPlan& e, int row) {
    ev.w0 = (unsigned)(row - e.s0) < e.n0 ? 1 : 0;
    ev.w1 = (unsigned)(row - e.s1) < e.n1 ? 1 : 0;
    ev.next = event_next(e, row + 1);
    MCR_EV_SCALAR(ev.w0); MCR_EV_SCALAR(ev.w1); MCR_EV_SCALAR(ev.next);
    return row == e.t1 ? 2 : row == e.t2 ? 1 : row == e.t3 ? 0 : -1;
}

// The consumer's place in the hand-over of staged pairs.  Barrier p hands pair p (rows 2 p, 2 p + 1) over in stage buffer
// p & 1; every kVotePairs-th barrier, starting with barrier 0, is also the workgroup's stop vote.  `pair` is the index of the
// next barrier, `off` the offset (in doubles) of the buffer that barrier hands over.
struct PairCursor { int pair; unsigned off; };
MCR_EV_FN bool pair_votes(const PairCursor& c, int vote_pairs) { return (c.pair & (vote_pairs - 1)) == 0; }
MCR_EV_FN void pair_advance(PairCursor& c, unsigned stage_len) { ++c.pair; c.off ^= stage_len; }
