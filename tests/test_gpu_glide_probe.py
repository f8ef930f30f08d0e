"""Glide probes (`mcr_probe_glide_paths_rng` and its joint and outcome forms, `engine.probe_glide_paths*`) on the GPU, on
scenarios/config.json at 321 and 512 paths.  Every comparison is bit for bit.

  - a constant table, of length 1 or of the horizon's length, gives the allocation probes' counters, masks, matrix and rows;
  - an option probed among others equals the option probed alone, which is the single-option launch (one consumer wave);
  - working_months 0, 1, 11, 12, 13 and 233 under a table that changes in every year: entries past the horizon are never read,
    a table cut short holds its last entry, and the flags and ruin months are the CPU model's (tests/glide_model.cpp);
  - 1, 2, 15, 16 and 31 options: the groups after the first launch read their own weights;
  - an option's row depends neither on its position nor on its neighbours' table lengths;
  - host validation errors leave every output untouched; the NumPy and history streams, and a shape below
    MCR_GLIDE_FANOUT_MIN_WAVES, are refused with MCR_ERR_UNSUPPORTED."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import glide_fuzz as GF
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_expense_probe import SCENARIOS
from test_gpu_option_outcomes import same_bits

pytestmark = pytest.mark.gpu
SEED = 0x611D_E
KNOB = "MCR_GLIDE_FANOUT_MIN_WAVES"
CFGD = SCENARIOS["config"]
PATHS = (321, 512)
RY = int(CFGD["retirement_years"])
AMOUNTS = tuple(float(CFGD[f]) for f in ("initial_balance", "monthly_contribution", "monthly_expenses"))
OWN = float(CFGD["allocation_inv1_pct"])
SENTINEL = -12345.678


def _p():
    return params_from_config(Config(**CFGD))


def _years(wm):
    return (wm + 12 * RY + 11) // 12


def _yearly(wm, phase=0):
    """A table that changes in every year of the horizon."""
    return tuple(round(0.05 + 0.9 * (((7 * y + phase) % 19) / 18.0), 6) for y in range(_years(wm)))


def _option(table, amounts=AMOUNTS):
    return amounts + (tuple(float(x) for x in table),)


def _launches():
    return N.load_library().mcr_probe_glide_paths_last_fanout_launches()


def _rows(options, n, wm=233, begin=0):
    """(counts, final rows, ruin rows) of `options` as numpy arrays, the rows cut to n columns."""
    counts, fin, ruin = E.probe_glide_paths_outcomes(_p(), SEED, 0, begin, n, wm, options)
    return counts.cpu().numpy(), fin.cpu().numpy()[:, :n], ruin.cpu().numpy()[:, :n]


_ALONE = {}   # (option, n, wm, begin) -> its rows from a single-option call: computed once, shared


def _alone(option, n, wm=233, begin=0):
    key = (option, n, wm, begin)
    if key not in _ALONE:
        got = _rows([option], n, wm, begin)
        assert _launches() == 1
        _ALONE[key] = tuple(x[0] for x in got)
    return _ALONE[key]


def _assert_rows_are_the_options_alone(options, n, wm=233, begin=0, groups=None):
    counts, fin, ruin = _rows(options, n, wm, begin)
    if groups is not None:
        assert _launches() == groups
    for k, o in enumerate(options):
        c, f, r = _alone(o, n, wm, begin)
        assert counts[k].tolist() == c.tolist() and same_bits(fin[k], f) and same_bits(ruin[k], r), (k, len(options), n, wm)
    return counts, fin, ruin


@pytest.mark.parametrize("n", PATHS)
def test_constant_tables_equal_the_allocation_probes(n):
    p, wm, begin = _p(), 233, 12_345
    splits = [OWN, 0.0, 1.0, 0.35, 0.9]
    alloc = [AMOUNTS + (a,) for a in splits]
    for length in (1, _years(wm)):
        glide = [_option([a] * length) for a in splits]
        want_c, want_f, want_r = E.probe_allocations_outcomes(p, SEED, 0, begin, n, wm, alloc)
        got_c, got_f, got_r = E.probe_glide_paths_outcomes(p, SEED, 0, begin, n, wm, glide)
        assert _launches() == 1
        assert got_c.cpu().numpy().tolist() == want_c.cpu().numpy().tolist()
        # (columns at or beyond n_paths of a row are never written: compare the paths' columns only)
        assert same_bits(got_f.cpu().numpy()[:, :n], want_f.cpu().numpy()[:, :n]) and same_bits(got_r.cpu().numpy()[:, :n], want_r.cpu().numpy()[:, :n])
        want = E.probe_allocations_joint(p, SEED, 0, begin, n, wm, alloc)
        got = E.probe_glide_paths_joint(p, SEED, 0, begin, n, wm, glide)
        assert _launches() == 1
        for a, b in zip(got, want):
            assert a.cpu().numpy().tolist() == b.cpu().numpy().tolist()
        assert E.probe_glide_paths(p, SEED, 0, begin, n, wm, glide).cpu().numpy().tolist() == want_c.cpu().numpy().tolist()
    assert len({int(c) for c in want_c.cpu().numpy()[:, 0]}) >= 3       # the splits do differ


@pytest.mark.parametrize("n", PATHS)
def test_own_among_others_equals_own_alone(n):
    own = _option([OWN])
    options = [_option(_yearly(233)), own, _option([1.0, 0.0]), _option([0.2] * 7 + [0.8])]
    counts, fin, ruin = _assert_rows_are_the_options_alone(options, n, groups=1)
    c, f, r = _alone(own, n)
    assert 0 < int(c[0]) < n                                             # both outcomes: final balances and ruin years to compare
    want = E.probe_allocations_outcomes(_p(), SEED, 0, 0, n, 233, [AMOUNTS + (OWN,)])      # (one option: the plain summary launch)
    assert c.tolist() == want[0].cpu().numpy()[0].tolist()
    assert same_bits(f, want[1].cpu().numpy()[0, :n]) and same_bits(r, want[2].cpu().numpy()[0, :n])
    # the plain and the joint form of the single option
    assert E.probe_glide_paths(_p(), SEED, 0, 0, n, 233, [own]).cpu().numpy()[0].tolist() == c.tolist()
    jc, joint, extremes, masks = E.probe_glide_paths_joint(_p(), SEED, 0, 0, n, 233, [own])
    assert _launches() == 1
    assert jc.cpu().numpy()[0].tolist() == c.tolist() and joint.cpu().numpy().tolist() == [[int(c[0])]]
    bits = np.unpackbits(masks.cpu().numpy().view(np.uint8), bitorder="little")
    assert bits[:n].tolist() == (~np.isnan(f)).astype(np.uint8).tolist() and not bits[n:].any()


@pytest.mark.parametrize("wm", [0, 1, 11, 12, 13, 233])
def test_a_table_that_changes_every_year_at_every_month_alignment(oracle, wm):
    n = PATHS[wm % 2]
    table = _yearly(wm)
    Y = _years(wm)
    assert len(table) == Y and all(table[y] != table[y + 1] for y in range(Y - 1))
    cut = max(1, Y // 2)
    options = [
        _option(table),
        _option(table + (0.123, 0.987, 0.5)),                  # entries past the horizon are never read
        _option(table[:cut]),                                  # a table cut short holds its last entry
        _option(table[:cut] + (table[cut - 1],) * (Y - cut)),
        _option(_yearly(wm, phase=5)),
    ]
    counts, fin, ruin = _assert_rows_are_the_options_alone(options, n, wm=wm, groups=1)
    assert same_bits(fin[0], fin[1]) and same_bits(ruin[0], ruin[1]) and counts[0].tolist() == counts[1].tolist()
    assert same_bits(fin[2], fin[3]) and same_bits(ruin[2], ruin[3]) and counts[2].tolist() == counts[3].tolist()
    # the weight of the row: the model's flags and ruin months (exact below the 2^33 money scale), for the distinct tables
    for k in (0, 2, 4):
        run = GF.run_model(oracle, _p(), SEED, 0, 0, n, wm, options[k][3])
        assert float(np.abs(run["trajectory"]).max()) < 2.0 ** 33
        assert np.array_equal(~np.isnan(fin[k]), run["success"].astype(bool)), (wm, k)
        np.testing.assert_array_equal(ruin[k], run["years_to_ruin"])
    if wm == 233:
        assert not same_bits(ruin[0], ruin[4]) or not same_bits(fin[0], fin[4])     # the phase of the table matters


@pytest.mark.parametrize("L", [1, 2, 15, 16, 31])
def test_groups_after_the_first_read_their_own_weights(L):
    n = PATHS[L % 2]
    pool = [_option(_yearly(233, phase=k)[:3 + 2 * k]) for k in range(8)] + [_option([OWN]), _option([1.0, 0.0])]
    options = [pool[(3 * k) % len(pool)] if k % 4 else _option(_yearly(233, phase=k), (AMOUNTS[0] * (1 + 0.01 * k), AMOUNTS[1], AMOUNTS[2]))
               for k in range(L)]
    _assert_rows_are_the_options_alone(options, n, groups=-(-L // N.MCR_MAX_EXPENSE_FANOUT))
    counts = E.probe_glide_paths(_p(), SEED, 0, 0, n, 233, options).cpu().numpy()
    assert _launches() == -(-L // N.MCR_MAX_EXPENSE_FANOUT)
    assert counts.tolist() == [_alone(o, n)[0].tolist() for o in options]
    jc, joint, _, _ = E.probe_glide_paths_joint(_p(), SEED, 0, 0, n, 233, options)
    assert jc.cpu().numpy().tolist() == counts.tolist() and joint.cpu().numpy().diagonal().tolist() == counts[:, 0].tolist()


def test_a_row_depends_neither_on_position_nor_on_its_neighbours():
    n = 321
    target = _option(_yearly(233, phase=2))
    for neighbours in ([_option([0.5])], [_option([0.1] * 60), _option([0.9, 0.2])], [_option(_yearly(233)[:k]) for k in (1, 5, 40, 9)]):
        for at in range(len(neighbours) + 1):
            options = neighbours[:at] + [target] + neighbours[at:]
            counts, fin, ruin = _rows(options, n)
            c, f, r = _alone(target, n)
            assert counts[at].tolist() == c.tolist() and same_bits(fin[at], f) and same_bits(ruin[at], r), (at, len(neighbours))
    options = [_option(_yearly(233, phase=k)[:1 + k]) for k in range(12)]
    perm = np.random.default_rng(3).permutation(len(options))
    a = _rows(options, n)
    b = _rows([options[i] for i in perm], n)
    for x, y in zip(a, b):
        assert same_bits(y, x[perm])


def _raw_call_buffers(L):
    import torch

    sentinel = -0x1234_5678
    ints = [torch.full(shape, sentinel, dtype=torch.int64, device="cuda") for shape in ((L, 2), (L, 16), (L, L), (2,))]
    rows = [torch.full((L, 1024), SENTINEL, dtype=torch.float64, device="cuda") for _ in range(2)]
    return sentinel, ints, rows


def _raw_calls(p, rng, n, wm, weights, records, ints, rows):
    """The three entry points on raw records; returns their return codes."""
    import torch

    lib = N.load_library()
    stream = torch.cuda.current_stream(0).cuda_stream
    L = len(records)
    table = (C.c_double * max(1, len(weights)))(*weights)
    arr = (N.McrGlideOption * L)(*[N.McrGlideOption(*r) for r in records])
    head = (C.byref(p), C.byref(rng), 0, 0, n, wm, table, len(weights), arr, L, C.c_void_p(ints[0].data_ptr()))
    out = N.McrOptionOutcomes(rows[0].data_ptr(), rows[1].data_ptr(), 1024)
    rcs = []
    for call in (lambda: lib.mcr_probe_glide_paths_rng(*head, 0, C.c_void_p(stream)),
                 lambda: lib.mcr_probe_glide_paths_joint_rng(*head, C.c_void_p(ints[1].data_ptr()), C.c_void_p(ints[2].data_ptr()),
                                                             C.c_void_p(ints[3].data_ptr()), 0, C.c_void_p(stream)),
                 lambda: lib.mcr_probe_glide_paths_outcomes_rng(*head, C.byref(out), 0, C.c_void_p(stream))):
        rcs.append((call(), N.last_error(), _launches()))
    torch.cuda.synchronize()
    return rcs


def _untouched(sentinel, ints, rows):
    return all((t.cpu() == sentinel).all() for t in ints) and all((t.cpu() == SENTINEL).all() for t in rows)


def test_invalid_options_leave_the_device_outputs_untouched():
    p, rng = _p(), N.philox_rng(SEED)
    weights = [0.5, 0.6, 0.7, 0.8]
    good = (1000.0, 10.0, 20.0, 0, 4)
    cases = []
    for i, f in enumerate(("initial_balance", "monthly_contribution", "monthly_expenses")):
        for bad in (float("nan"), -0.01, float("inf")):
            cases.append((weights, good[:i] + (bad,) + good[i + 1:], f"options[1].{f}"))
    cases += [(weights, good[:3] + (0, 0), "options[1].n_weights"), (weights, good[:3] + (1, -2), "options[1].n_weights"),
              (weights, good[:3] + (-1, 2), "options[1].first_weight"), (weights, good[:3] + (2, 3), "options[1].first_weight"),
              (weights, good[:3] + (4, 1), "options[1].first_weight")]
    for bad in (-0.1, 1.0000001, float("nan"), float("inf"), -5e-324):
        cases.append(([0.5, 0.6, bad, 0.8], good[:3] + (1, 3), "options[1].weights[1]"))
    for w, record, name in cases:
        sentinel, ints, rows = _raw_call_buffers(3)
        for rc, message, launches in _raw_calls(p, rng, 1000, 12, w, [good[:3] + (0, 2), record, good[:3] + (0, 2)], ints, rows):
            assert rc == N.MCR_ERR_INVALID_ARG and name in message and launches == 0, (record, w, rc, message)
        assert _untouched(sentinel, ints, rows), (record, w)
    # a weight that no option names is not looked at
    sentinel, ints, rows = _raw_call_buffers(2)
    assert [rc for rc, _, _ in _raw_calls(p, rng, 1000, 12, [0.5, float("nan"), 7.0, 0.25], [good[:3] + (0, 1), good[:3] + (3, 1)], ints, rows)] == [0, 0, 0]
    assert ints[0].cpu().numpy()[:, 1].tolist() == [1000, 1000]
    with pytest.raises(RuntimeError, match=r"options\[1\]\.weights\[2\]"):
        E.probe_glide_paths(p, SEED, 0, 0, 100, 12, [_option([0.5]), _option([0.1, 0.2, 1.5])])
    with pytest.raises(ValueError, match="every option is"):
        E.probe_glide_paths(p, SEED, 0, 0, 100, 12, [(1.0, 1.0, 1.0)])
    with pytest.raises(ValueError, match="at least one weight"):
        E.probe_glide_paths(p, SEED, 0, 0, 100, 12, [(1.0, 1.0, 1.0, ())])
    assert E.probe_glide_paths(p, SEED, 0, 0, 100, 12, []).shape == (0, 2)
    with pytest.raises(ValueError, match="MCR_MAX_JOINT_OPTIONS"):
        E.probe_glide_paths_joint(p, SEED, 0, 0, 100, 12, [_option([0.5])] * (N.MCR_MAX_JOINT_OPTIONS + 1))


def test_numpy_and_history_streams_are_refused():
    p = _p()
    weights, records = [0.5, 0.6], [(1000.0, 10.0, 20.0, 0, 2), (1000.0, 10.0, 20.0, 1, 1)]
    history = N.history_rng(SEED, np.random.default_rng(1).standard_normal((240, 3)), 12)
    for rng, word in ((N.numpy_rng(1234, child_offset=0), "NumPy stream"), (history, "history stream")):
        sentinel, ints, rows = _raw_call_buffers(2)
        for rc, message, launches in _raw_calls(p, rng, 321, 13, weights, records, ints, rows):
            assert rc == N.MCR_ERR_UNSUPPORTED and word in message and launches == 0, (rc, message)
        assert _untouched(sentinel, ints, rows)
    with pytest.raises(RuntimeError, match="NumPy stream is not supported under a glide path"):
        E.probe_glide_paths(p, N.numpy_rng(1234, child_offset=0), 1, 0, 321, 13, [_option([0.5, 0.6])])


def test_min_waves_above_the_shape_is_unsupported(monkeypatch):
    p, rng = _p(), N.philox_rng(SEED)
    weights, records = [0.5, 0.6], [(1000.0, 10.0, 20.0, 0, 2), (1000.0, 10.0, 20.0, 1, 1)]
    monkeypatch.setenv(KNOB, "6")          # 321 paths are six path-wavefronts
    sentinel, ints, rows = _raw_call_buffers(2)
    assert [(rc, launches) for rc, _, launches in _raw_calls(p, rng, 321, 13, weights, records, ints, rows)] == [(0, 1)] * 3
    monkeypatch.setenv(KNOB, "7")
    sentinel, ints, rows = _raw_call_buffers(2)
    for rc, message, launches in _raw_calls(p, rng, 321, 13, weights, records, ints, rows):
        assert rc == N.MCR_ERR_UNSUPPORTED and KNOB in message and launches == 0, (rc, message)
    assert _untouched(sentinel, ints, rows)
