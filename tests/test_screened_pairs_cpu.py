"""The wave-uniform bookkeeping of the split re-run's consumer wave (csrc/mcr_events.h; path_kernel's "PAIRS"), on the CPU.

The consumer of a screened launch's split re-run runs its months two to a loop turn, with the hand-over barrier at a fixed
place of the turn, and keeps one event row instead of the month's threshold and window tests.  A barrier too many or too few
is a hung workgroup, so the schedule is proved here, without a GPU: tests/screened_pairs_model.cpp compiles the header the
kernel compiles, restates the kernel's loops without their arithmetic, and compares

  - the paired consumer's barriers (count, pair, row, stage buffer, vote flag) with the other split kernels' consumer and with
    both producer forms, for every working_months in 0 .. 47 (every working_months % 24, every total_months % 4), retirements
    of 1, 2 and 40 years, and a workgroup voted dead at each of its votes or at none;
  - the event row with the month's own tests on every row: window edges and priority thresholds that coincide, windows of
    length 0, open at row 0, never closing, opening behind the last row, and every placement of two windows over a
    twelve-month path.
"""

from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def model_output(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "a host C++ compiler"
    exe = str(tmp_path_factory.mktemp("pairs") / "screened_pairs_model")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "monte_carlo_retirement_amd", "csrc"),
                    os.path.join(REPO, "tests", "screened_pairs_model.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout


def _section(model_output, name):
    rc, out = model_output
    lines = [x for x in out.splitlines() if x.startswith(name)]
    assert lines and lines[-1].startswith(f"{name} ok "), out[-2000:]
    return int(lines[-1].split()[-1])


def test_paired_consumer_executes_the_barriers_and_votes_of_the_producers(model_output):
    # 48 working_months x 3 retirement lengths x (no dead vote + one case per vote of the path)
    votes = lambda wm, ry: ((wm + 12 * ry + 1) // 2 + 15) // 16      # noqa: E731
    assert _section(model_output, "schedule") == sum(1 + votes(wm, ry) for wm in range(48) for ry in (1, 2, 40))


def test_event_row_equals_the_months_own_tests_on_every_row(model_output):
    assert _section(model_output, "events") == 9 + 14 * 14 * 15 * 15
    assert model_output[0] == 0
