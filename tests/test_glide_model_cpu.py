"""The oracle's model of a glide path (tests/glide_model.cpp, through tests/glide_fuzz.py), anchored on the CPU.

The model is the project's oracle's path loop over the steps the oracle exports, with the weight of the row in every place the
loop reads a weight.  It is the reference of tests/test_gpu_glide_vs_oracle.py, so it is held to the unmodified oracle first:

  - under a CONSTANT table every block copy it hands to the oracle's steps equals the plan's block with that split, so every
    per-path column must equal `oracle.run_batch`'s bit for bit -- for every plan of the six classes the glide fan-out serves and
    every constant split of tests/allocation_fuzz.py, as a table of length 1 and as a table three entries longer than the horizon;
  - the glide options of tests/glide_fuzz.py are worth running: every one but `own` changes the success flag of at least one path
    on MOST plans (more than half of them: an option that moved paths on fewer plans than it left alone would mostly re-test the
    constant split), and every model run stays below count_fuzz.SCALE_LIMIT, the money scale up to which identical flags are
    demanded of the GPU."""

from __future__ import annotations

import numpy as np
import pytest

import allocation_fuzz as AF
import count_fuzz as F
import glide_fuzz as GF

CLASSES = tuple(c for c in F.CLASSES if c != "generic")
COLUMNS = ("start_balance", "final_balance", "years_to_ruin", "first_year_gross_withdrawal", "first_year_real_gross_withdrawal",
           "inflation_at_retirement", "success", "trajectory", "real_trajectory", "withdrawal_rate_trajectory")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("cls", CLASSES)
def test_constant_tables_equal_the_oracle_bit_for_bit(oracle, cls):
    checked = 0
    for scn, runs in AF.class_runs(oracle, cls):
        Y = GF.horizon_years(scn)
        for name, split, want in zip(AF.NAMES, AF.splits(scn), runs):
            for length in (1, Y + 3):
                got = GF.model_run(oracle, scn, [float(split)] * length)
                for col in COLUMNS:
                    assert _same_bits(got[col], want[col]), (col, name, length, scn.context("glide model, constant table"))
                checked += 1
    assert checked == F.KEPT[cls] * len(AF.NAMES) * 2


def test_the_options_move_paths_and_stay_in_range(oracle):
    plans, moved = 0, {name: 0 for name in GF.NAMES[1:]}
    for cls in CLASSES:
        for scn, runs in GF.class_runs(oracle, cls):
            plans += 1
            for name, run in zip(GF.NAMES, runs):
                assert F.money_scale(run) < F.SCALE_LIMIT, (name, scn.context("glide model: money scale"))
            flags = GF.oracle_flags(runs)
            assert flags.shape == (len(GF.NAMES), scn.n)
            for k, name in enumerate(GF.NAMES[1:], start=1):
                moved[name] += int((flags[k] != flags[0]).any())
    print(f"glide options: plans on which the option changes a success flag, of {plans}: {moved}")
    assert plans == sum(F.KEPT[c] for c in CLASSES)
    for name, count in moved.items():
        assert 2 * count > plans, (name, count, plans)


def test_the_model_refuses_what_is_not_a_glide_path(oracle):
    scn = F.scenarios(oracle, "mask0")[0]
    for table in ([1.5], [0.5, float("nan")], [-0.1]):
        with pytest.raises(RuntimeError):
            GF.run_model(oracle, scn.params(), scn.seed, scn.stream, scn.begin, 4, scn.wm, table, trajectories=False)
