"""Allocation probes (`mcr_probe_allocations_rng` and its joint and outcome forms, `engine.probe_allocations*`) on the GPU.

The contract: option k's counters equal, bit for bit, those of a count-only launch with (initial_balance, monthly_contribution,
monthly_expenses, allocation_inv1_pct) = option k (`engine.probe_months` of a parameter block that differs only there) -- on the
allocation fan-out route (`PHASE == 12`: Philox, <= 16 streams, tolerance month) and on the per-option route (NumPy stream,
history stream, longer stream lists, the exact month, or forced).  The joint form's masks are the `success` columns of summary
launches of the options and its matrix their co-occurrence counts; the outcome form's rows are where(success, final_balance,
NaN) and years_to_ruin of those launches, bit for bit on both routes."""

from __future__ import annotations

import ctypes as C
import json
import math

import numpy as np
import pytest

from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_expense_probe import SCENARIOS as EXPENSE_SCENARIOS
from test_gpu_joint_outcomes import expected, plain_flags, unpack
from test_gpu_option_outcomes import reference_rows, same_bits
from test_gpu_scenario_probe import FROZEN8, STRADDLE

pytestmark = pytest.mark.gpu
SEED = 0xA110_C8
KNOB = "MCR_ALLOCATION_FANOUT_MIN_WAVES"
FIELDS = ("initial_balance", "monthly_contribution", "monthly_expenses", "allocation_inv1_pct")
SCENARIOS = dict(EXPENSE_SCENARIOS)       # config, jorge_rho, no_tax, annual_tax, streams17 and exact_month (the last two: per-option route)
PER_OPTION = ("streams17", "exact_month")
SENTINEL = -12345.678


def _records(cfgd, L):
    """L options (a prefix of the list): the config's own four values; everything in the second asset (the first one's
    balance is dust from month 0); everything in the first; a duplicate of the first option; an even split; the largest
    double below 1 (the second asset's weight is 2^-53); the smallest double above 0 (the first asset's balance underflows);
    then a spread in which the three amounts differ as well."""
    own = tuple(float(cfgd[f]) for f in FIELDS)
    head = [own, own[:3] + (0.0,), own[:3] + (1.0,), own, own[:3] + (0.5,), own[:3] + (math.nextafter(1.0, 0.0),), own[:3] + (5e-324,)]
    spread = [(round(max(own[0], 1000.0) * (0.1 + 0.9 * k), 2), round(max(own[1], 100.0) * (2.5 - 0.07 * k), 2),
               round(max(own[2], 100.0) * (0.4 + 0.09 * k), 2), (0.03 + 0.0731 * k) % 1.0) for k in range(max(0, L - len(head)))]
    return (head + spread)[:L]


def _config_of(cfgd, record):
    return dict(cfgd, **dict(zip(FIELDS, record)))


def _launches():
    return N.load_library().mcr_probe_allocations_last_fanout_launches()


_REFERENCE = {}   # (config, seed, stream, path range, month, record) -> counters of the plain launch: computed once, shared


def _plain(cfgd, seed, stream, begin, n, wm, record):
    q = params_from_config(Config(**_config_of(cfgd, record)))
    if not isinstance(seed, int):   # (a NumPy- or history-stream descriptor: a few small cases, not shared)
        return E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist()
    key = (json.dumps(cfgd, sort_keys=True, default=str), seed, stream, begin, n, wm, record)
    if key not in _REFERENCE:
        _REFERENCE[key] = E.probe_months(q, seed, stream, begin, n, [wm]).cpu().numpy()[0].tolist()
    return _REFERENCE[key]


def _check(cfgd, seed, wm, n, begin, records, stream=0, groups=None):
    """`groups`: the fan-out launches the call must report (None: not checked)."""
    p = params_from_config(Config(**cfgd))
    got = E.probe_allocations(p, seed, stream, begin, n, wm, records).cpu().numpy().tolist()
    launches = _launches()
    want = [_plain(cfgd, seed, stream, begin, n, wm, r) for r in records]
    assert got == want, (wm, n, begin, len(records), [k for k in range(len(records)) if got[k] != want[k]])
    if groups is not None:
        assert launches == groups, (launches, groups, len(records))
    return got


def _sweep(cfgd, per_launch):
    """wm x n x L as the scenario probe's sweep; `per_launch`: options a fan-out launch takes (0: the per-option route)."""
    Ls = [1, 2, 8, 15, 16, 40]
    i = 0
    for wm in (0, 1, 13, 233):
        for n in (1, 63, 65, 50_000):
            begin = (0, 12_345)[i % 2]
            L = Ls[i % len(Ls)]
            i += 1
            groups = 0 if (per_launch == 0 or L == 1) else -(-L // per_launch)
            got = _check(cfgd, SEED, wm, n, begin, _records(cfgd, L), groups=groups)
            assert all(c[1] == n for c in got)
            if L >= 4:
                assert got[3] == got[0]   # the duplicate


@pytest.mark.parametrize("name", list(SCENARIOS))
def test_counts_equal_plain_launches(name):
    _sweep(SCENARIOS[name], 0 if name in PER_OPTION else N.MCR_MAX_EXPENSE_FANOUT)


def test_counts_with_eleven_records_per_launch():
    """8 frozen streams = 8 lock columns per consumer wave: 64 KB of LDS hold 11 waves of them."""
    _sweep(FROZEN8, 11)
    for L, groups in ((11, 1), (12, 2), (15, 2), (40, 4)):   # one full launch, 6 + 6, 8 + 7, 4 x 10
        _check(FROZEN8, SEED, 120, 2000, 77, _records(FROZEN8, L), groups=groups)


def test_the_options_do_differ():
    """The sweep is not vacuous: at a month and size with mixed outcomes the splits give different counts."""
    cfgd = SCENARIOS["config"]
    got = _check(cfgd, SEED, 233, 50_000, 0, _records(cfgd, 15), groups=1)
    print("successes of the 15 options:", [c[0] for c in got])
    assert len({c[0] for c in got}) >= 3, got
    assert got[1] != got[2]                   # everything in the second asset against everything in the first


def test_counts_straddling_2_pow_32():
    cfgd = SCENARIOS["config"]
    for n, L in ((65, 3), (20_000, 8)):
        _check(cfgd, SEED, 233, n, STRADDLE, _records(cfgd, L), groups=1)


def test_own_allocation_equals_the_scenario_probe():
    cfgd = SCENARIOS["jorge_rho"]
    p = params_from_config(Config(**cfgd))
    a = float(cfgd["allocation_inv1_pct"])
    triples = [r[:3] for r in _records(cfgd, 15)]
    for wm, n in ((0, 65), (150, 20_000)):
        got = E.probe_allocations(p, SEED, 0, 5, n, wm, [t + (a,) for t in triples]).cpu().numpy().tolist()
        assert _launches() == 1
        assert got == E.probe_scenarios(p, SEED, 0, 5, n, wm, triples).cpu().numpy().tolist()


def test_numpy_and_history_streams_take_the_per_option_route():
    cfgd = SCENARIOS["config"]
    for wm, n, L in ((0, 65, 2), (13, 1000, 8), (233, 5000, 16)):
        _check(cfgd, N.numpy_rng(1234, child_offset=0), wm, n, 0, _records(cfgd, L), stream=1, groups=0)
    history = N.history_rng(SEED, np.random.default_rng(1).standard_normal((240, 3)), 12)
    for wm, n, L in ((13, 1000, 8), (233, 5000, 16)):
        _check(cfgd, history, wm, n, 0, _records(cfgd, L), groups=0)


def test_forced_per_option_route_agrees(monkeypatch):
    cfgd = SCENARIOS["config"]
    p = params_from_config(Config(**cfgd))
    records = _records(cfgd, 15)
    monkeypatch.setenv(KNOB, "0")
    fan = E.probe_allocations(p, SEED, 0, 0, 50_000, 240, records).cpu().numpy()
    assert _launches() == 1
    monkeypatch.setenv(KNOB, str(2**40))
    per = E.probe_allocations(p, SEED, 0, 0, 50_000, 240, records).cpu().numpy()
    assert _launches() == 0
    assert fan.tolist() == per.tolist()
    # the knob counts path-wavefronts: 782 of them here
    monkeypatch.setenv(KNOB, "782")
    E.probe_allocations(p, SEED, 0, 0, 50_000, 240, records)
    assert _launches() == 1
    monkeypatch.setenv(KNOB, "783")
    E.probe_allocations(p, SEED, 0, 0, 50_000, 240, records)
    assert _launches() == 0


def test_permuting_options_permutes_counts():
    cfgd = SCENARIOS["jorge_rho"]
    p = params_from_config(Config(**cfgd))
    records = _records(cfgd, 12)
    perm = np.random.default_rng(3).permutation(len(records))
    a = E.probe_allocations(p, SEED, 0, 0, 20_000, 120, records).cpu().numpy()
    b = E.probe_allocations(p, SEED, 0, 0, 20_000, 120, [records[i] for i in perm]).cpu().numpy()
    assert b.tolist() == a[perm].tolist()


# ---- the joint form ------------------------------------------------------------------------------------------------------------
JOINT = dict(begin=12_345, n=4133, wm=233)      # 64 whole 64-path blocks + 37, a range that does not start at a multiple of 64


def _check_joint(cfgd, L, groups, seed=SEED, stream=0, masks=True):
    records = _records(cfgd, L)
    p = params_from_config(Config(**cfgd))
    counts, joint, extremes, mk = E.probe_allocations_joint(p, seed, stream, JOINT["begin"], JOINT["n"], JOINT["wm"], records, masks=masks)
    assert _launches() == groups
    flags = np.stack([plain_flags(_config_of(cfgd, r), seed=seed, stream=stream, **JOINT) for r in records])
    want_joint, want_extremes = expected(flags)
    assert joint.cpu().numpy().tolist() == want_joint.tolist()
    assert extremes.cpu().numpy().tolist() == want_extremes
    if masks:
        got, tail = unpack(mk, JOINT["n"])
        assert not tail.any(), "bits beyond n_paths must be 0"
        assert np.array_equal(got, flags), [int(x) for x in np.flatnonzero((got != flags).any(axis=1))]
    else:
        assert mk is None
    counts = counts.cpu().numpy()
    assert counts.tolist() == E.probe_allocations(p, seed, stream, JOINT["begin"], JOINT["n"], JOINT["wm"], records).cpu().numpy().tolist()
    assert counts[:, 0].tolist() == want_joint.diagonal().tolist() and counts[:, 1].tolist() == [JOINT["n"]] * L
    return want_joint


@pytest.mark.parametrize("L", [2, 15, 17, 32])
def test_joint_masks_and_matrix_equal_summary_launches(L):
    want = _check_joint(SCENARIOS["config"], L, -(-L // N.MCR_MAX_EXPENSE_FANOUT))
    if L >= 15:
        assert want[0, 3] == want[0, 0] == want[3, 3]                 # the duplicate
        assert len(set(want.diagonal().tolist())) >= 3                # the options do differ


def test_joint_on_the_per_option_routes(monkeypatch):
    _check_joint(SCENARIOS["config"], 1, 0)
    _check_joint(SCENARIOS["streams17"], 5, 0)
    _check_joint(SCENARIOS["config"], 5, 0, seed=N.numpy_rng(1234, child_offset=0), stream=1)
    _check_joint(SCENARIOS["config"], 9, 1, masks=None)               # the library's own scratch masks
    monkeypatch.setenv(KNOB, str(2**40))
    _check_joint(SCENARIOS["config"], 9, 0)
    _check_joint(SCENARIOS["config"], 9, 0, masks=None)


# ---- the outcome form ----------------------------------------------------------------------------------------------------------
def _check_outcomes(cfgd, L, groups, n=321, begin=0, wm=233, stride=None, want_final=True, want_ruin=True):
    import torch

    records = _records(cfgd, L)
    p = params_from_config(Config(**cfgd))
    width = (n + 63) // 64 * 64 if stride is None else stride
    slab = lambda want: torch.full((L, width), SENTINEL, dtype=torch.float64, device="cuda") if want else None  # noqa: E731
    counts, fin, ruin = E.probe_allocations_outcomes(p, SEED, 0, begin, n, wm, records, final_balance=slab(want_final),
                                                     years_to_ruin=slab(want_ruin), path_stride=width)
    assert _launches() == groups
    refs = [reference_rows(_config_of(cfgd, r), seed=SEED, stream=0, begin=begin, n=n, wm=wm) for r in records]
    want_fin, want_ruin_rows = np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])
    for got, want, asked in ((fin, want_fin, want_final), (ruin, want_ruin_rows, want_ruin)):
        if not asked:
            assert got is None
            continue
        got = got.cpu().numpy()
        assert got.shape == (L, width)
        assert same_bits(got[:, :n], want), [int(k) for k in range(L) if not same_bits(got[k, :n], want[k])]
        assert np.all(got[:, n:] == SENTINEL), "columns at or beyond n_paths must not be written"
    counts = counts.cpu().numpy()
    assert counts[:, 0].tolist() == (~np.isnan(want_fin)).sum(axis=1).tolist() and counts[:, 1].tolist() == [n] * L
    return want_fin


@pytest.mark.parametrize("begin", [0, 2**32 - 100])
@pytest.mark.parametrize("n", [321, 512])
def test_outcome_rows_equal_summary_launches(n, begin):
    want_fin = _check_outcomes(SCENARIOS["config"], 9, 1, n=n, begin=begin, stride=n + 37)
    mixed = [k for k in range(9) if 0 < np.isnan(want_fin[k]).sum() < n]
    assert len(mixed) >= 2, mixed                                     # rows with both outcomes: final balances and ruin years to compare


def test_outcome_rows_in_two_groups_with_annual_tax_and_on_the_per_option_routes(monkeypatch):
    _check_outcomes(SCENARIOS["config"], 17, 2, stride=384 + 64)
    _check_outcomes(SCENARIOS["annual_tax"], 8, 1)
    _check_outcomes(SCENARIOS["jorge_rho"], 8, 1, wm=75)
    _check_outcomes(SCENARIOS["config"], 8, 1, want_ruin=False)
    _check_outcomes(SCENARIOS["config"], 8, 1, want_final=False)
    _check_outcomes(SCENARIOS["config"], 1, 0, stride=400)
    _check_outcomes(SCENARIOS["exact_month"], 5, 0, stride=400)
    monkeypatch.setenv(KNOB, str(2**40))
    _check_outcomes(SCENARIOS["config"], 9, 0, stride=321 + 37)
    _check_outcomes(SCENARIOS["config"], 9, 0, want_ruin=False)


# ---- errors ----------------------------------------------------------------------------------------------------------------------
def test_invalid_options_leave_the_device_outputs_untouched():
    import torch

    p = params_from_config(Config(**SCENARIOS["config"]))
    lib = N.load_library()
    rng = N.philox_rng(SEED)
    stream = torch.cuda.current_stream(0).cuda_stream
    sentinel = -0x1234_5678
    good = (1000.0, 10.0, 20.0, 0.5)
    cases = [(f, bad) for f in FIELDS[:3] for bad in (float("nan"), -0.01, float("inf"))]
    cases += [("allocation_inv1_pct", bad) for bad in (-0.1, 1.0000001, float("nan"), -5e-324)]
    for field, bad in cases:
        counts = torch.full((3, 2), sentinel, dtype=torch.int64, device="cuda")
        masks = torch.full((3, 16), sentinel, dtype=torch.int64, device="cuda")
        joint = torch.full((3, 3), sentinel, dtype=torch.int64, device="cuda")
        extremes = torch.full((2,), sentinel, dtype=torch.int64, device="cuda")
        fin = torch.full((3, 1024), SENTINEL, dtype=torch.float64, device="cuda")
        ruin = torch.full((3, 1024), SENTINEL, dtype=torch.float64, device="cuda")
        arr = (N.McrAllocationOption * 3)(*[N.McrAllocationOption(*good) for _ in range(3)])
        setattr(arr[1], field, bad)
        head = (C.byref(p), C.byref(rng), 0, 0, 1000, 12, arr, 3, C.c_void_p(counts.data_ptr()))
        rows = N.McrOptionOutcomes(fin.data_ptr(), ruin.data_ptr(), 1024)
        for rc in (lib.mcr_probe_allocations_rng(*head, 0, C.c_void_p(stream)),
                   lib.mcr_probe_allocations_joint_rng(*head, C.c_void_p(masks.data_ptr()), C.c_void_p(joint.data_ptr()),
                                                       C.c_void_p(extremes.data_ptr()), 0, C.c_void_p(stream)),
                   lib.mcr_probe_allocations_outcomes_rng(*head, C.byref(rows), 0, C.c_void_p(stream))):
            assert rc == N.MCR_ERR_INVALID_ARG and f"options[1].{field}" in N.last_error(), (field, bad, N.last_error())
            assert _launches() == 0
        torch.cuda.synchronize()
        for t in (counts, masks, joint, extremes):
            assert (t.cpu() == sentinel).all()
        assert (fin.cpu() == SENTINEL).all() and (ruin.cpu() == SENTINEL).all()
    counts = torch.full((1, 2), sentinel, dtype=torch.int64, device="cuda")
    rc = lib.mcr_probe_allocations_rng(C.byref(p), C.byref(rng), 0, 0, 1000, 12, None, 0, C.c_void_p(counts.data_ptr()), 0, C.c_void_p(stream))
    torch.cuda.synchronize()
    assert rc == 0 and (counts.cpu() == sentinel).all()
    with pytest.raises(RuntimeError, match=r"options\[1\]\.allocation_inv1_pct"):
        E.probe_allocations(p, SEED, 0, 0, 100, 12, [good, (1.0, 1.0, 1.0, 1.5)])
    with pytest.raises(ValueError, match="every option is"):
        E.probe_allocations(p, SEED, 0, 0, 100, 12, [(1.0, 1.0, 1.0)])
    assert E.probe_allocations(p, SEED, 0, 0, 100, 12, []).shape == (0, 2)
    with pytest.raises(ValueError, match="MCR_MAX_JOINT_OPTIONS"):
        E.probe_allocations_joint(p, SEED, 0, 0, 100, 12, [good] * (N.MCR_MAX_JOINT_OPTIONS + 1))
