"""Glide options for the stratified random plans of tests/count_fuzz.py, with the answer of the CPU oracle's MODEL of a glide
path to each.

The unmodified oracle runs one split per run, and no `Config` override is a glide path.  tests/glide_model.cpp is the oracle's own
path loop over the steps the oracle exports, with the weight of the row in every place the loop reads a weight (include/mcr.h:
GLIDE PATH); it is compiled here with the host compiler, the oracle's flags, and linked to the oracle's library.
tests/test_glide_model_cpu.py anchors it: under a constant table it equals `oracle.run_batch` bit for bit in every per-path
column.  Its per-path columns are the reference of tests/test_gpu_glide_vs_oracle.py.

Options of a plan whose own split is a (`allocation_inv1_pct`; the three amounts stay the plan's own), Y the horizon in whole
years (ceil(total_months / 12)), wm its working months:
    own:     [a]
    step:    [a] x (ceil(wm / 12) + 1) + [1 - a]     switches inside the first retirement year: off the retirement-year boundary
                                                     whenever wm % 12 != 0
    linear:  Y entries from a to 1 - a
    short:   [1.0, 0.0]                              the table is clipped, and an asset turns to dust at month 12
    long:    Y + 5 entries alternating a and allocation_fuzz's `toward`: entries past the horizon are never read"""

from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import count_fuzz as F
from conftest import REPO
from monte_carlo_retirement_amd._native import McrOutputs, McrParams
from option_fuzz import SCENARIO_FIELDS, oracle_flags, oracle_rows  # noqa: F401  (the same rows and flags, re-exported)

NAMES = ("own", "step", "linear", "short", "long")

_MODEL = None
_RUNS = {}


def model(O) -> C.CDLL:
    """tests/glide_model.cpp as a shared library in a temporary directory, built once per process."""
    global _MODEL
    if _MODEL is None:
        O.lib()                                       # (builds the oracle's library where it is missing)
        cxx = shutil.which("g++") or shutil.which("c++")
        assert cxx, "a host C++ compiler"
        oracle_dir = os.path.join(REPO, "oracle")
        so = os.path.join(tempfile.mkdtemp(prefix="glide_model_"), "libglide_model.so")
        subprocess.run([cxx, "-std=c++17", "-O2", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-Wextra", "-Werror",
                        "-I", os.path.join(REPO, "include"), os.path.join(REPO, "tests", "glide_model.cpp"), "-o", so,
                        "-L", oracle_dir, "-l:liboracle.so", f"-Wl,-rpath,{oracle_dir}", "-lm"], check=True, capture_output=True, text=True)
        L = C.CDLL(so)
        L.glide_model_run_batch.restype = C.c_int
        L.glide_model_run_batch.argtypes = [C.POINTER(McrParams), C.c_uint64, C.c_uint32, C.c_uint64, C.c_uint64, C.c_int32,
                                            C.POINTER(C.c_double), C.c_int32, C.POINTER(McrOutputs)]
        _MODEL = L
    return _MODEL


def horizon_years(scn, wm=None) -> int:
    wm = scn.wm if wm is None else int(wm)
    return (wm + 12 * int(scn.cfgd["retirement_years"]) + 11) // 12


def toward(a: float) -> float:
    return a + 0.35 if a < 0.5 else a - 0.35


def tables(scn, wm=None):
    """The five tables of the plan, in NAMES' order."""
    wm = scn.wm if wm is None else int(wm)
    a = float(scn.cfgd["allocation_inv1_pct"])
    Y = horizon_years(scn, wm)
    return [
        [a],
        [a] * ((wm + 11) // 12 + 1) + [1.0 - a],
        [float(x) for x in np.linspace(a, 1.0 - a, Y)],
        [1.0, 0.0],
        [a if y % 2 == 0 else toward(a) for y in range(Y + 5)],
    ]


def records(scn, wm=None):
    """The options as `engine.probe_glide_paths*` takes them."""
    own = tuple(float(scn.cfgd[f]) for f in SCENARIO_FIELDS)
    return [own + (tuple(t),) for t in tables(scn, wm)]


def run_model(O, params, seed, stream, begin, n, wm, table, trajectories=True):
    """The model's `run_batch` under `table`: the oracle's dictionary (per-path columns; no counters)."""
    sz = O.query_sizes(params, wm)
    n = int(n)
    res = {}
    o = McrOutputs()
    o.path_stride = n
    for k in ("start_balance", "final_balance", "years_to_ruin", "first_year_gross_withdrawal", "first_year_real_gross_withdrawal",
              "inflation_at_retirement"):
        res[k] = np.empty(n, dtype=np.float64)
        setattr(o, k, res[k].ctypes.data)
    res["success"] = np.empty(n, dtype=np.uint8)
    o.success = res["success"].ctypes.data
    if trajectories:
        res["trajectory"] = np.empty((sz.trajectory_len, n), dtype=np.float64)
        res["real_trajectory"] = np.empty((sz.trajectory_len, n), dtype=np.float64)
        res["withdrawal_rate_trajectory"] = np.empty((sz.retirement_years, n), dtype=np.float64)
        o.trajectory = res["trajectory"].ctypes.data
        o.real_trajectory = res["real_trajectory"].ctypes.data
        o.withdrawal_rate_trajectory = res["withdrawal_rate_trajectory"].ctypes.data
    w = (C.c_double * len(table))(*[float(x) for x in table])
    rc = model(O).glide_model_run_batch(C.byref(params), int(seed), int(stream), int(begin), n, int(wm), w, len(table), C.byref(o))
    if rc != 0:
        raise RuntimeError(f"glide_model_run_batch failed: {rc}")
    return res


def model_run(O, scn, table, wm=None, n=None):
    """`run_model` of plan `scn` under `table` (at `wm` months, over `n` paths), with trajectories: cached."""
    wm = scn.wm if wm is None else int(wm)
    n = scn.n if n is None else int(n)
    key = (scn.cls, scn.index, scn.seed, scn.begin, scn.cfgd["monthly_expenses"], n, wm, tuple(float(x) for x in table))
    if key not in _RUNS:
        _RUNS[key] = run_model(O, scn.params(), scn.seed, scn.stream, scn.begin, n, wm, table)
    return _RUNS[key]


def class_runs(O, cls, threads: int = 8):
    """[(plan, [the model's trajectory run of each option])] of class `cls`: on host threads (the model is a C call), cached."""
    plans = F.scenarios(O, cls)
    model(O)
    jobs = [(scn, t) for scn in plans for t in tables(scn)]
    with ThreadPoolExecutor(max_workers=threads) as pool:
        runs = list(pool.map(lambda j: model_run(O, *j), jobs))
    n = len(NAMES)
    return [(scn, runs[n * k: n * k + n]) for k, scn in enumerate(plans)]
