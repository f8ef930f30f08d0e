"""The GROWTH FORMS of the count-only path kernel (csrc/mcr_device.h: kGrowthNarrowExp | kGrowthRhoZero; DESIGN.md "growth
forms"): compile-time variants that leave out work a launch's own parameters make unnecessary — the exponent insertion of exp
when every argument lies in the narrow window, the rho term of the inflation log-return when rho = 0.  Both claim to keep every
bit: exp's two forms are compared value by value over the whole window, and whole launches through MCR_K1_GROWTH_FORM, mask by
mask, on counters, ruin-year bins, withdrawal-rate observation counts and histogram bins."""

from __future__ import annotations

import json
import math
import os

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E

pytestmark = pytest.mark.gpu

STEP = math.log(2.0) / 512.0
KNOBS = ("MCR_K1_GROWTH_FORM", "MCR_K1_SPLIT_MAX_WAVES", "MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_POLLS",
         "MCR_K1_SEGMENT_ORDER")


def test_exp_forms_agree_bit_for_bit_over_the_whole_window():
    """Every k = rint(x 512 / ln 2) in [-256, 255], seven residues each: the centre, both ends of the reduction interval (the
    half-way points, where rint moves to the neighbour — whichever k the kernel picks there, both forms pick the same), a
    hair inside either end, and two interior points.  The window's own ends stop a hair inside -256.5 and 255.5."""
    k = np.arange(-256, 256, dtype=np.float64)
    hair = 1e-7
    xs = []
    for f in (0.0, -0.25, 1.0 / 3.0, -0.5 + hair, 0.5 - hair):
        xs.append((k + f) * STEP)
    xs.append((k[1:] - 0.5) * STEP)            # half-way between k - 1 and k, for k = -255 .. 255
    xs.append(np.array([-256 * STEP, -1 * STEP, 0.0, -0.0, 255 * STEP]))
    x = np.concatenate(xs)
    assert 3000 < x.size < 5000
    seen = np.rint(x / STEP)
    assert set(seen.astype(int).tolist()) == set(range(-256, 256))
    got = E.eval_helper_host(N.MCR_HELPER_MATH_EXP_FORMS, None, x.reshape(-1, 1))
    general, narrow = got[:, 0], got[:, 1]
    bad = np.nonzero(general.view(np.uint64) != narrow.view(np.uint64))[0]
    assert bad.size == 0, (bad[:5].tolist(), x[bad[:5]].tolist(), general[bad[:5]].tolist(), narrow[bad[:5]].tolist())
    # and the general column is the path form of exp the other tests know (MCR_HELPER_MATH_EXP_PATH), i.e. exp to 1e-14
    path = E.eval_helper_host(N.MCR_HELPER_MATH_EXP_PATH, None, x.reshape(-1, 1))[:, 0]
    assert np.array_equal(general.view(np.uint64), path.view(np.uint64))
    assert np.max(np.abs(general / np.exp(x) - 1.0)) < 1e-14


def _config(**over):
    with open(os.path.join(REPO, "scenarios", "config.json")) as fh:
        return dict(json.load(fh), **over)


def _run(p, wm, n, begin, env, edges):
    old = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        r = E.run_batch_host(p, 4242, 1, begin, n, wm, want_summary=False, want_trajectories=False, hist_edges=edges)
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return np.concatenate([r["counters"], r["ruin_year_bins"], r["wr_obs_counts"], r["hist_bins"]]).astype(np.int64)


def _masks_agree(p, wm, n, begin, env, masks, what):
    edges = np.geomspace(1.0, 1e13, 65)
    assert E.growth_form(p, wm) == masks[0], what            # the launch's own choice is the highest mask compared
    own = _run(p, wm, n, begin, env, edges)
    assert int(own[1]) == n, what
    for m in masks:
        got = _run(p, wm, n, begin, dict(env, MCR_K1_GROWTH_FORM=str(m)), edges)
        assert np.array_equal(got, own), (what, m, np.nonzero(got != own)[0][:8].tolist())
    return own


PLAIN = {"MCR_K1_SPLIT_MAX_WAVES": "0", "MCR_K1_SEGMENTS": "0"}     # the unsplit whole-path kernel, whatever the size


def test_plain_launch_every_mask_gives_the_same_integers():
    own = _masks_agree(params_from_config(Config(**_config())), 233, 20_000, 0, PLAIN, (3, 1, 0), "config.json plain")
    assert 0 < int(own[0]) < 20_000


def test_a_forced_form_the_launch_does_not_have_is_an_error():
    p = params_from_config(Config(**_config()))
    edges = np.geomspace(1.0, 1e13, 65)
    with pytest.raises(RuntimeError, match="MCR_K1_GROWTH_FORM"):        # 2 000 paths: the producer / consumer kernel, no variants
        _run(p, 233, 2_000, 0, {"MCR_K1_GROWTH_FORM": "3"}, edges)
    s60 = params_from_config(Config(**_config(equity_inflation_correlation=0.3)))
    with pytest.raises(RuntimeError, match="MCR_K1_GROWTH_FORM"):        # rho = 0.3: bit 1 is not available
        _run(s60, 233, 2_000, 0, dict(PLAIN, MCR_K1_GROWTH_FORM="3"), edges)


def test_time_sliced_launch_every_mask_gives_the_same_integers():
    """The smallest launch that slices: one path block more than the resident slots (6 workgroups per CU), two segments, the
    order given — which is an error unless the launch really is time-sliced."""
    import torch

    slots = torch.cuda.get_device_properties(0).multi_processor_count * 6
    n = slots * 256 + 1
    env = {"MCR_K1_SEGMENTS_ALWAYS": "1", "MCR_K1_SEGMENTS": "2", "MCR_K1_SEGMENT_ORDER": "0,1"}
    p = params_from_config(Config(**_config()))
    sliced = _masks_agree(p, 233, n, 5, env, (3, 1, 0), "config.json time-sliced")
    plain = _run(p, 233, n, 5, dict(PLAIN, MCR_K1_GROWTH_FORM="0"), np.geomspace(1.0, 1e13, 65))
    assert np.array_equal(sliced, plain)


def test_wave_that_straddles_2_to_the_32_every_mask_gives_the_same_integers():
    """Paths 2^32 - 100 .. 2^32 + 411: the second wavefront of the first block runs the general generator form (per-lane
    path_hi) behind the uniform one, with the same growth form."""
    p = params_from_config(Config(**_config()))
    _masks_agree(p, 233, 512, 2**32 - 100, PLAIN, (3, 1, 0), "straddling wave")


@pytest.mark.parametrize("rho", [0.0, 0.3])
def test_near_the_bound_every_mask_gives_the_same_integers(rho):
    """Monthly drifts of +215, +225 and -235 table steps with log-volatilities of 0.5 % a year: every exp of the launch has
    |k| > 200 (checked below from the parameters), of both signs, and the launch still qualifies.  48 months, so that balances
    and the price level stay inside the kernel's range (growth ~ e^(0.3 x 48))."""
    p = params_from_config(Config(**_config(retirement_years=4, equity_inflation_correlation=rho)))
    p.inv1_mu_log, p.inf_mu_log, p.prem_mu_log = 12 * 215 * STEP, 12 * 225 * STEP, -12 * 235 * STEP
    p.inv1_sigma_log = p.inf_sigma_log = p.prem_sigma_log = 0.005
    zmax = math.sqrt(-2.0 * math.log(2.0 ** -33))
    c_inf = abs(rho) + math.sqrt(1.0 - rho * rho)
    for mu, sigma, c in ((p.inv1_mu_log, p.inv1_sigma_log, 1.0), (p.inf_mu_log, p.inf_sigma_log, c_inf), (p.prem_mu_log, p.prem_sigma_log, 1.0)):
        spread = c * sigma / math.sqrt(12.0) * zmax / STEP
        assert abs(mu) / 12.0 / STEP - spread > 200.5 and abs(mu) / 12.0 / STEP + spread <= 254.0
    masks = (3, 1, 0) if rho == 0.0 else (1, 0)
    _masks_agree(p, 0, 20_000, 0, PLAIN, masks, f"near the bound, rho = {rho}")
