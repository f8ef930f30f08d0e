"""`allocation.GlidePath`, `allocation.glide_records` and the glide probes' declarations, without a GPU: the constructors'
tables, immutability and validation; the records' layout (equal tables stored once, amounts defaulted from the config) and
their error messages; the record's size against include/mcr.h; and the host validation of the library, which runs before a
device is looked for."""

from __future__ import annotations

import ctypes as C
import os
import re

import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, load_config_from_json, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd.allocation import GLIDE_OPTION_FIELDS, GlidePath, default_glide_paths, glide_paths_of, glide_records


@pytest.fixture(scope="module")
def cfg():
    return Config(**load_config_from_json(os.path.join(REPO, "scenarios", "config.json")))


def test_constructors():
    assert GlidePath.constant(0.6).weights == (0.6,) and len(GlidePath.constant(0.6)) == 1
    g = GlidePath.linear(0.9, 0.4, 0, 5)
    assert len(g) == 6 and g.weights[0] == 0.9 and g.weights[-1] == 0.4
    assert all(abs(w - (0.9 - 0.1 * y)) < 1e-12 for y, w in enumerate(g.weights))
    g = GlidePath.linear(0.3, 0.6, 20, 35)          # holds `start` before from_year and `end` after to_year
    assert len(g) == 36 and set(g.weights[:21]) == {0.3} and g.weights[35] == 0.6 and g.weight_at(12 * 500) == 0.6
    assert all(a < b for a, b in zip(g.weights[20:35], g.weights[21:36]))
    assert GlidePath.linear(0.3, 0.6, 2, 2).weights == (0.3, 0.3, 0.3, 0.6)
    assert GlidePath.linear(0.5, 0.5, 0, 9) == GlidePath([0.5] * 10) != GlidePath.constant(0.5)
    # around retirement: R = 233 // 12 = 19
    g = GlidePath.around_retirement(233, 0.9, 0.5, 0.4, 5, 3)
    assert len(g) == 23 and set(g.weights[:15]) == {0.9} and g.weights[19] == 0.5 and g.weights[22] == 0.4
    assert all(a > b for a, b in zip(g.weights[14:22], g.weights[15:23]))
    rising = GlidePath.around_retirement(233, 0.6, 0.3, 0.6, 10, 15)
    assert min(rising.weights) == rising.weights[19] == 0.3 and rising.weights[0] == rising.weights[-1] == 0.6
    early = GlidePath.around_retirement(24, 0.9, 0.5, 0.4, 10, 2)     # the line would begin before today: it begins today, on the line
    assert abs(early.weights[0] - (0.9 - 0.4 * 8 / 10)) < 1e-12 and early.weights[2] == 0.5 and early.weights[4] == 0.4
    assert GlidePath.around_retirement(0, 0.9, 0.5, 0.4, 0, 0).weights == (0.5,)
    assert GlidePath.parse("0.9>0.4@0-20") == GlidePath.linear(0.9, 0.4, 0, 20) and GlidePath.parse(" 0.6 ") == GlidePath.constant(0.6)
    assert GlidePath.parse("0.9>0.4@0-20").describe() == "0.9>0.4@0-20" and GlidePath.constant(0.6).describe() == "constant 0.6"
    assert GlidePath([0.9, 0.5, 0.4]).describe() == "0.9 -> 0.4 over 3 years" and GlidePath([0.5], "mine").describe() == "mine"


def test_weight_at_is_the_definition():
    g = GlidePath([0.1, 0.2, 0.3])
    assert [g.weight_at(t) for t in (0, 11, 12, 23, 24, 35, 36, 10_000)] == [0.1, 0.1, 0.2, 0.2, 0.3, 0.3, 0.3, 0.3]
    with pytest.raises(ValueError):
        g.weight_at(-1)


def test_immutable_and_validated():
    g = GlidePath([0.1, 0.2])
    with pytest.raises(AttributeError):
        g.weights = (0.5,)
    with pytest.raises(AttributeError):
        g.other = 1
    assert isinstance(g.weights, tuple) and hash(g) == hash(GlidePath((0.1, 0.2)))
    for bad, words in (([], "at least one"), ([0.5, 1.5], r"weights\[1\]"), ([float("nan")], r"weights\[0\]"), ([-0.1], r"weights\[0\]"),
                       (["x"], "must be a number"), (5, "sequence")):
        with pytest.raises(ValueError, match=words):
            GlidePath(bad)
    for call in (lambda: GlidePath.constant(1.01), lambda: GlidePath.linear(0.9, 0.4, 5, 2), lambda: GlidePath.linear(0.9, 0.4, -1, 2),
                 lambda: GlidePath.linear(0.9, 0.4, 0, 2.5), lambda: GlidePath.around_retirement(120, 0.9, 0.5, 1.4, 5, 5),
                 lambda: GlidePath.parse("0.9>0.4@20"), lambda: GlidePath.parse("a>b@1-2"), lambda: GlidePath.parse("")):
        with pytest.raises(ValueError):
            call()


def test_records_layout(cfg):
    own = (float(cfg.initial_balance), float(cfg.monthly_contribution), float(cfg.monthly_expenses))
    options = [0.5, [0.1, 0.2], GlidePath.constant(0.5), "0.3>0.6@1-3", {"glide_path": [0.1, 0.2], "monthly_expenses": 9.0},
               {"glide_path": 0.25, "initial_balance": 1.0, "monthly_contribution": 2.0}]
    records, table = glide_records(cfg, options)
    assert table == [0.5, 0.1, 0.2] + list(GlidePath.linear(0.3, 0.6, 1, 3).weights) + [0.25]        # equal tables are stored once
    assert records == [own + (0, 1), own + (1, 2), own + (0, 1), own + (3, 4), own[:2] + (9.0, 1, 2), (1.0, 2.0, own[2], 7, 1)]
    assert all(table[r[3]:r[3] + r[4]] == list(g.weights) for r, g in zip(records, glide_paths_of(options)))
    assert glide_records(cfg, []) == ([], [])
    assert GLIDE_OPTION_FIELDS == ("initial_balance", "monthly_contribution", "monthly_expenses", "glide_path")


def test_records_errors_name_the_option_and_the_field(cfg):
    for options, words in (([0.5, {"glide_path": 0.5, "inv1_returns_mean": 0.1}], r"glide_paths\[1\]: unknown key\(s\) \['inv1_returns_mean'\]"),
                           ([{"monthly_expenses": 1.0}], r"glide_paths\[0\]\.glide_path is missing"),
                           ([0.5, [0.2, 1.5]], r"glide_paths\[1\]: weights\[1\] = 1\.5"),
                           ([1.5], r"glide_paths\[0\]: allocation = 1\.5"),
                           ([[]], r"glide_paths\[0\]: a glide path has at least one weight"),
                           (["0.9>0.4"], r"glide_paths\[0\]: glide path '0\.9>0\.4'"),
                           ([{"glide_path": 0.5, "monthly_expenses": -1.0}], r"glide_paths\[0\]\.monthly_expenses = -1\.0: must be finite and >= 0"),
                           ([{"glide_path": 0.5, "initial_balance": "x"}], r"glide_paths\[0\]\.initial_balance = 'x': must be a number")):
        with pytest.raises(ValueError, match=words):
            glide_records(cfg, options)


def test_default_catalogue(cfg):
    for wm in (0, 7, 240, 500):
        catalogue = default_glide_paths(cfg, wm)
        assert [g.weights for g in catalogue[:3]] == [(float(cfg.allocation_inv1_pct),), (1.0,), (0.0,)]
        assert len(catalogue) == 6 and len({g.describe() for g in catalogue}) == 6
        r = wm // 12
        for g in catalogue[3:5]:                     # declining: never rises, and does fall
            assert all(a >= b for a, b in zip(g.weights, g.weights[1:])) and g.weights[0] > g.weights[-1]
        rising = catalogue[5].weights
        assert rising[r] == min(rising) and rising[-1] > rising[r]
        glide_records(cfg, catalogue)


def test_header_record_and_symbols():
    header = open(os.path.join(REPO, "include", "mcr.h")).read()
    assert C.sizeof(N.McrGlideOption) == 32 and N.McrGlideOption.first_weight.offset == 24 and N.McrGlideOption.n_weights.offset == 28
    assert re.search(r"typedef struct mcr_glide_option \{[^}]*int32_t first_weight;[^}]*int32_t n_weights;[^}]*\} mcr_glide_option;", header)
    assert "w(t)   = W[min(t div 12, n - 1)]" in header and "MCR_GLIDE_FANOUT_MIN_WAVES" in header
    for name in ("mcr_probe_glide_paths_rng", "mcr_probe_glide_paths_joint_rng", "mcr_probe_glide_paths_outcomes_rng",
                 "mcr_probe_glide_paths_last_fanout_launches"):
        assert f"int {name}(" in header and name in N.ABI_SYMBOLS


def test_host_validation_needs_no_device(cfg):
    lib = N.load_library()
    p, rng = params_from_config(cfg), N.philox_rng(1)
    weights = (C.c_double * 3)(0.5, 0.6, 1.5)
    counts = (C.c_uint64 * 4)(7, 7, 7, 7)        # (never touched: every call fails before a device is looked for)

    def call(records, n_weights=3, rng=rng, n_paths=100):
        arr = (N.McrGlideOption * len(records))(*[N.McrGlideOption(*r) for r in records])
        rc = lib.mcr_probe_glide_paths_rng(C.byref(p), C.byref(rng), 0, 0, n_paths, 12, weights, n_weights, arr, len(records),
                                           C.cast(counts, C.c_void_p), 0, None)
        return rc, N.last_error()

    good = (1000.0, 10.0, 20.0, 0, 2)
    for record, words in (((1000.0, 10.0, 20.0, 0, 0), "options[1].n_weights"), ((1000.0, 10.0, 20.0, 2, 2), "options[1].first_weight"),
                          ((1000.0, 10.0, 20.0, -1, 1), "options[1].first_weight"), ((1000.0, 10.0, 20.0, 1, 2), "options[1].weights[1]"),
                          ((1000.0, -1.0, 20.0, 0, 1), "options[1].monthly_contribution")):
        rc, message = call([good, record])
        assert rc == N.MCR_ERR_INVALID_ARG and words in message, (record, rc, message)
    rc, message = call([good], rng=N.numpy_rng(5))
    assert rc == N.MCR_ERR_UNSUPPORTED and "NumPy stream is not supported under a glide path" in message
    rc, message = call([good], n_paths=2 ** 31 + 1)
    assert rc == N.MCR_ERR_UNSUPPORTED and "2^31" in message
    assert list(counts) == [7, 7, 7, 7]
    assert lib.mcr_probe_glide_paths_last_fanout_launches() == 0
