"""Hand-over between the segments of a time-sliced path block (PHASE 3 / 4 of the path kernel; csrc/mcr_hip.hip)
in EVERY order the segments can run.  MCR_K1_SEGMENT_ORDER sends the sliced grid out as the whole blocks followed by one
launch per segment, in the given order: with a small poll budget a segment whose predecessor has not run yet times out and
recomputes its block, one whose predecessor has run resumes from the hand-over slot.  Whatever the schedule, every output
must be bit-identical (NaN included) to the plain launch (MCR_K1_SEGMENTS=0), which the rest of the suite pins to the CPU
oracle.  The mixed case (some successors resume, some recompute) is the one that can go wrong: a late predecessor overwrote
the slot of a segment that had already recomputed, and the next segment resumed from a stale year."""

from __future__ import annotations

import contextlib
import itertools
import os

import numpy as np
import pytest

from conftest import load_golden
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

KNOBS = ("MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS", "MCR_K1_SEGMENT_ORDER")
N_COUNT = 393_216 + 999         # count-only: just above 256 CUs x 6 resident workgroups x 256 paths, so the launch slices
N_OUT = 330_000                 # per-path outputs: 1 290 path blocks on 256 x 5 resident slots
EDGES = np.geomspace(1.0, 1e13, 65)
PLAIN = {"MCR_K1_SEGMENTS": "0"}


@contextlib.contextmanager
def _knobs(env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _counts(p, wm, n, env):
    with _knobs(env):
        r = E.run_batch_host(p, 4242, 1, 2**33 + 5, n, wm, want_summary=False, want_trajectories=False, hist_edges=EDGES)
    return np.concatenate([r["counters"], r["ruin_year_bins"], r["wr_obs_counts"], r["hist_bins"]]).astype(np.int64)


def _outputs(p, wm, n, env, want_trajectories):
    with _knobs(env):
        return E.run_batch_host(p, 4242, 1, 7, n, wm, want_trajectories=want_trajectories)


def _scenarios():
    inj = {g["name"]: g for g in load_golden("paths_injected.json")}
    c1 = inj["C1_config_json_wm233"]["cfg"]                       # one frozen stream (a lock column travels with the state)
    failing = inj["FAILING_wm24"]["cfg"]                          # half of the paths fail: dead lanes and dead waves cross segments
    yield "config.json wm=233 (odd resume rows, terminal tax period)", c1, 233
    yield "annual tax wm=50", inj["ANNUAL_wm50"]["cfg"], 50       # annual-gains tax: the gain accumulators travel too
    yield "failing wm=24", failing, 24
    yield "failing wm=7", dict(failing, retirement_years=9), 7    # few retirement years: one-to-three-year segments
    yield "mixed wm=36", inj["MIXED_wm36"]["cfg"], 36


def _q(segments, cfgd):
    """The segment count the launcher plans (plan_segments): the request, at most 8 and at most one per two retirement years."""
    return min(segments, 8, cfgd["retirement_years"] // 2)


def _order(perm):
    return ",".join(str(k) for k in perm)


def _diff(got, ref):
    return np.nonzero(got != ref)[0][:8].tolist()


def test_every_segment_order_count_only():
    """Four segments, all 24 orders: counters, ruin-year bins, withdrawal-rate counts and final-balance histogram bins."""
    for name, cfgd, wm in _scenarios():
        assert _q(4, cfgd) == 4, name
        p = params_from_config(Config(**cfgd))
        plain = _counts(p, wm, N_COUNT, PLAIN)
        assert int(plain[1]) == N_COUNT and 0 < int(plain[0]) <= N_COUNT, name
        bad = []
        for perm in itertools.permutations(range(4)):
            env = {"MCR_K1_SEGMENTS": "4", "MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_POLLS": "2", "MCR_K1_SEGMENT_ORDER": _order(perm)}
            got = _counts(p, wm, N_COUNT, env)
            if not np.array_equal(got, plain):
                bad.append((_order(perm), _diff(got, plain)))
        assert not bad, (name, bad)


def _orders8(rng):
    ident = list(range(8))
    yield ident
    yield ident[::-1]
    for i in range(7):                                            # every adjacent pair swapped
        o = list(ident)
        o[i], o[i + 1] = o[i + 1], o[i]
        yield o
    for _ in range(8):
        yield rng.permutation(8).tolist()


def test_eight_segment_orders_count_only():
    """Eight segments (scenarios with at least 16 retirement years): identity, reversed, each adjacent swap, 8 random orders."""
    checked = 0
    for name, cfgd, wm in _scenarios():
        if _q(8, cfgd) != 8:
            continue
        p = params_from_config(Config(**cfgd))
        plain = _counts(p, wm, N_COUNT, PLAIN)
        bad = []
        for perm in _orders8(np.random.default_rng(8)):
            env = {"MCR_K1_SEGMENTS": "8", "MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_POLLS": "2", "MCR_K1_SEGMENT_ORDER": _order(perm)}
            got = _counts(p, wm, N_COUNT, env)
            if not np.array_equal(got, plain):
                bad.append((_order(perm), _diff(got, plain)))
        assert not bad, (name, bad)
        checked += 1
    assert checked >= 4


@pytest.mark.parametrize("want_trajectories", [False, True])
def test_segment_orders_with_per_path_outputs(want_trajectories):
    """Summary (mode 1) and trajectory (mode 2) variants: every per-path field, trajectory sample and withdrawal rate."""
    for name, cfgd, wm in _scenarios():
        p = params_from_config(Config(**cfgd))
        plain = _outputs(p, wm, N_OUT, PLAIN, want_trajectories)
        bad = []
        for order in ("0,1,2,3", "1,0,2,3", "0,2,1,3", "3,2,1,0", "0,1,3,2"):
            env = {"MCR_K1_SEGMENTS": "4", "MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_POLLS": "2", "MCR_K1_SEGMENT_ORDER": order}
            got = _outputs(p, wm, N_OUT, env, want_trajectories)
            assert set(got) == set(plain)
            bad += [(order, k) for k in plain if not np.array_equal(got[k], plain[k], equal_nan=True)]
        assert not bad, (name, bad)


def test_segment_orders_probe_window():
    """PHASE 4: the search's verification window (17 candidate months over 50 000 paths, resumed from their accumulation
    snapshots) in three segments, all 6 orders: per-candidate counters equal the plain shared-prefix route."""
    cfgd = [g for g in load_golden("paths_injected.json") if g["name"] == "C1_config_json_wm233"][0]["cfg"]
    p = params_from_config(Config(**cfgd))
    months = list(range(217, 234))
    n = 50_000

    def probes(env):
        with _knobs(env):
            return E.probe_months(p, 4242, 0, 11, n, months).cpu().numpy()

    plain = probes(PLAIN)
    assert plain[:, 1].tolist() == [n] * len(months) and 0 < int(plain[0, 0]) <= n
    bad = []
    for perm in itertools.permutations(range(3)):
        env = {"MCR_K1_SEGMENTS": "3", "MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_POLLS": "2", "MCR_K1_SEGMENT_ORDER": _order(perm)}
        got = probes(env)
        if not np.array_equal(got, plain):
            bad.append((_order(perm), np.argwhere(got != plain)[:4].tolist()))
    assert not bad, bad


@pytest.mark.parametrize("polls", [1, 2, 3, 8, 64])
def test_small_poll_budgets_on_the_dispatcher(polls):
    """One launch, the hardware's own interleavings, a poll budget small enough that some successors time out while others
    resume: count-only and summary outputs equal the plain launch.  (Not deterministic: the ordered tests above are.)"""
    for name, cfgd, wm in _scenarios():
        p = params_from_config(Config(**cfgd))
        env = {"MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_POLLS": str(polls)}
        plain, got = _counts(p, wm, N_COUNT, PLAIN), _counts(p, wm, N_COUNT, env)
        assert np.array_equal(got, plain), (name, polls, _diff(got, plain))
        plain, got = _outputs(p, wm, N_OUT, PLAIN, False), _outputs(p, wm, N_OUT, env, False)
        for k in plain:
            assert np.array_equal(got[k], plain[k], equal_nan=True), (name, polls, k)


def _c1():
    cfgd = [g for g in load_golden("paths_injected.json") if g["name"] == "C1_config_json_wm233"][0]["cfg"]
    return params_from_config(Config(**cfgd))


@pytest.mark.parametrize("order, n", [("0,1,1,3", N_COUNT),          # not a permutation
                                      ("0,1,2", N_COUNT),            # wrong length (the plan has 4 segments)
                                      ("0,1,2,3", 10_000)])          # a launch too small to slice
def test_segment_order_knob_errors(order, n):
    p = _c1()
    env = {"MCR_K1_SEGMENTS": "4", "MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENT_ORDER": order}
    with pytest.raises(RuntimeError, match="MCR_K1_SEGMENT_ORDER"):
        _counts(p, 233, n, env)
    got = _counts(p, 233, n, {"MCR_K1_SEGMENTS": "4", "MCR_K1_SEGMENTS_ALWAYS": "1"})
    assert int(got[1]) == n and np.array_equal(got, _counts(p, 233, n, PLAIN))
