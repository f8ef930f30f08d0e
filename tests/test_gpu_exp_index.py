"""The narrow exp's table position (csrc/mcr_math.h: fexp<., NARROW> adds the shifter 1.5 2^52 + 256 and reads the low word of the
sum as a position of a table loaded ROTATED; tests/test_exp_index_cpu.py has the arithmetic).  Two parts on the device:

(a) the helper that evaluates the general and the narrow form side by side (MCR_HELPER_MATH_EXP_FORMS), bit for bit, on 2 10^5
    arguments: uniform draws over the window, the doubles on either side of every half-way point (k + 1/2) ln 2 / 512, where
    rint moves to the neighbour, and the window's own extreme doubles (found in exact arithmetic: the last arguments whose k is
    still -256 and 255);
(b) whole launches whose volatility puts the host's bound on |k| near the window's end, so that real launches read far into
    both halves of the rotated table: masks 3 and 1 against MCR_K1_GROWTH_FORM=0 bit for bit on counters, ruin-year bins,
    withdrawal-rate observation counts and histogram bins, and the counts against the CPU oracle.  300 paths, one full and one
    partial 256-path block; plain, and with a wave that straddles 2^32.  The time-sliced kernel cannot run on 300 paths (the
    launcher slices only what exceeds the resident slots, whatever MCR_K1_SEGMENTS_ALWAYS says), so that case runs at the
    smallest size that slices, with the segment order given — an error unless the launch really slices — and is held to the
    plain mask-0 launch of the same paths instead of the oracle (3 10^8 path-months are minutes of the oracle).

The oracle's outcomes on the 300-path cases are checked to be mixed without a GPU (the one test here that is not marked gpu)."""

from __future__ import annotations

import functools
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E

gpu = pytest.mark.gpu

STEP = math.log(2.0) / 512.0
EXP_SCALE = float.fromhex("0x1.71547652b82fep+9")         # kExpScale (csrc/mcr_tables.h), 512 / ln 2
ZMAX = math.sqrt(66.0 * math.log(2.0))                    # the generator's own bound on |z| (mcr_hip.hip: kGrowthZMax)
KNOBS = ("MCR_K1_GROWTH_FORM", "MCR_K1_SPLIT_MAX_WAVES", "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS",
         "MCR_K1_SEGMENT_ORDER")
PLAIN = {"MCR_K1_SPLIT_MAX_WAVES": "0", "MCR_K1_SEGMENTS": "0"}     # the unsplit whole-path kernel, whatever the size
SLICED = {"MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENTS": "2", "MCR_K1_SEGMENT_ORDER": "0,1"}   # (the order: an error unless it slices)
EDGES = np.geomspace(1.0, 1e13, 65)
SEED, STREAM, WM, N_PATHS = 4242, 1, 233, 300
COUNT_KEYS = ("counters", "ruin_year_bins", "wr_obs_counts")
# inv1_returns_volatility: 15.8 % (host bound on |k| 209), and the last hundredth of a percent for which the launch still qualifies (253.9)
VOLS = (0.158, 0.1939)
BEGINS = {"plain": 0, "straddling wave": 2**32 - 100}     # paths 2^32 - 100 .. 2^32 + 199: lane 36 of the second wavefront is path 2^32


def _k_of(x: float) -> int:
    """k as the kernel's FMA forms it: x kExpScale exactly, rounded half to even onto the unit grid."""
    q = Fraction(x) * Fraction(EXP_SCALE)
    f = math.floor(q)
    r = q - f
    return f + 1 if (r > Fraction(1, 2) or (r == Fraction(1, 2) and f % 2 == 1)) else f


def _extreme(h: float, outward: float, k_end: int) -> float:
    """The window's extreme double near the half-way point h: the last one, going outward, whose k is still k_end."""
    x = h
    for _ in range(8):                                    # (h itself is within a few ulp of the true boundary)
        x = float(np.nextafter(x, 0.0))
    assert _k_of(x) == k_end
    for _ in range(16):
        y = float(np.nextafter(x, outward))
        if _k_of(y) != k_end:
            return float(x)
        x = y
    raise AssertionError("no boundary within 16 ulp of the half-way point")


@gpu
def test_helper_forms_agree_bit_for_bit_on_2e5_arguments():
    lo, hi = _extreme(-256.5 * STEP, -1.0, -256), _extreme(255.5 * STEP, 1.0, 255)
    assert _k_of(float(np.nextafter(lo, -1.0))) == -257 and _k_of(float(np.nextafter(hi, 1.0))) == 256
    rng = np.random.default_rng(20260)
    half = (np.arange(-256, 255, dtype=np.float64) + 0.5) * STEP       # the 511 half-way points inside the window
    x = np.concatenate([rng.uniform(lo, hi, 198_000), np.nextafter(half, -1.0), half, np.nextafter(half, 1.0),
                        [lo, hi, float(np.nextafter(lo, 0.0)), float(np.nextafter(hi, 0.0)), -256 * STEP, 255 * STEP, 0.0, -0.0]])
    assert 199_000 < x.size < 201_000 and lo <= x.min() and x.max() <= hi
    assert set(np.rint(x / STEP).astype(int).tolist()) >= set(range(-256, 256))          # (every k; which k an end takes: _k_of above)
    got = E.eval_helper_host(N.MCR_HELPER_MATH_EXP_FORMS, None, x.reshape(-1, 1))
    general, narrow = got[:, 0], got[:, 1]
    bad = np.nonzero(general.view(np.uint64) != narrow.view(np.uint64))[0]
    assert bad.size == 0, (bad.size, x[bad[:5]].tolist(), general[bad[:5]].tolist(), narrow[bad[:5]].tolist())
    assert np.max(np.abs(general / np.exp(x) - 1.0)) < 1e-14           # (and both are exp, in its path form)


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return dict(json.load(fh), **over)


def _params(vol):
    return params_from_config(Config(**_config(inv1_returns_volatility=vol)))


def _k_bound(p):
    """The host's bound on |k| for the equity series, xmax 512 / ln 2 with xmax = |a| + |b| ZMAX (mcr_hip.hip: growth_form_qualified)."""
    return (abs(p.inv1_mu_log) / 12.0 + abs(p.inv1_sigma_log) / math.sqrt(12.0) * ZMAX) / STEP


@functools.lru_cache(maxsize=None)
def _oracle_counts(vol, begin):
    from oracle import oracle as O

    r = O.run_batch(_params(vol), SEED, STREAM, begin, N_PATHS, WM, want_trajectories=False)
    return {k: np.asarray(r[k]).astype(np.int64) for k in COUNT_KEYS}


def _run(p, n, begin, env):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return E.run_batch_host(p, SEED, STREAM, begin, n, WM, want_summary=False, want_trajectories=False, hist_edges=EDGES)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _ints(r):
    return np.concatenate([r["counters"], r["ruin_year_bins"], r["wr_obs_counts"], r["hist_bins"]]).astype(np.int64)


def _masks_agree(p, n, begin, env, what):
    general = _run(p, n, begin, dict(env, MCR_K1_GROWTH_FORM="0"))
    own = _run(p, n, begin, env)                          # the launch's own choice: mask 3 (checked by the caller)
    assert int(general["counters"][1]) == n, what
    for m, r in (("own", own), (3, _run(p, n, begin, dict(env, MCR_K1_GROWTH_FORM="3"))), (1, _run(p, n, begin, dict(env, MCR_K1_GROWTH_FORM="1")))):
        assert np.array_equal(_ints(r), _ints(general)), (what, m, np.nonzero(_ints(r) != _ints(general))[0][:8].tolist())
    return general, own


@pytest.mark.parametrize("vol", VOLS)
def test_the_volatilities_sit_under_the_bound_and_the_oracle_gives_mixed_outcomes(vol):
    """No GPU: the form is the host's decision, the outcomes are the oracle's."""
    p = _params(vol)
    assert p.equity_inflation_rho == 0.0 and E.growth_form(p, WM) == 3
    assert 200.0 < _k_bound(p) <= 254.0
    if vol == max(VOLS):                                  # just under: |k| may reach 250, and a hundredth of a percent more does not qualify
        assert _k_bound(p) > 250.0 and E.growth_form(_params(vol + 1e-4), WM) == 0
    for begin in BEGINS.values():
        c = _oracle_counts(vol, begin)["counters"]
        assert int(c[1]) == N_PATHS and N_PATHS // 4 < int(c[0]) < 3 * N_PATHS // 4, (vol, begin, c.tolist())


@gpu
@pytest.mark.parametrize("vol", VOLS)
@pytest.mark.parametrize("case", list(BEGINS))
def test_launches_near_the_bound_every_mask_and_the_oracle(case, vol):
    p, begin = _params(vol), BEGINS[case]
    assert E.growth_form(p, WM) == 3
    general, own = _masks_agree(p, N_PATHS, begin, PLAIN, (case, vol))
    counts = _oracle_counts(vol, begin)
    for r in (general, own):
        for k in COUNT_KEYS:
            got = np.asarray(r[k]).astype(np.int64)
            assert np.array_equal(got, counts[k]), (case, vol, k, got.tolist(), counts[k].tolist())
    assert 0 < int(own["counters"][0]) < N_PATHS


@gpu
@pytest.mark.parametrize("vol", VOLS)
def test_time_sliced_launch_near_the_bound_every_mask(vol):
    import torch

    n = torch.cuda.get_device_properties(0).multi_processor_count * 6 * 256 + 1      # one path block more than the resident slots
    p = _params(vol)
    assert E.growth_form(p, WM) == 3
    general, _ = _masks_agree(p, n, 5, SLICED, ("time-sliced", vol))
    plain = _run(p, n, 5, dict(PLAIN, MCR_K1_GROWTH_FORM="0"))
    assert np.array_equal(_ints(general), _ints(plain))
    assert 0 < int(plain["counters"][0]) < n
