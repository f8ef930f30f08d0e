"""Outcome probes (`mcr_probe_*_outcomes_rng`, `engine.probe_*_outcomes`) and `mcr_ruin_month_counts` on the GPU.

The contract: row k of `final_rows` / `ruin_rows` holds, bit for bit, ``where(success, final_balance, NaN)`` and
``years_to_ruin`` of a summary batch of the parameter block with option k's fields replaced (`engine.run_batch_host`); `counts`
is the plain probe's tensor; columns at or beyond `n_paths` are never written -- on the fan-out route (the consumer waves of the
fan-out kernel store the rows) and on the per-option route (summary launches into the rows, failed paths' balances NaN-ed),
which must agree to the byte.  `mcr_ruin_month_counts` equals ``np.bincount(np.rint(12 * y[~isnan(y)]))``."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import aggregation as A
from monte_carlo_retirement_amd import engine as E
from option_outcomes_dist_worker import CLAIMS, N_PATHS as DIST_PATHS, make_simulator as _sim, outcomes_document
from test_gpu_expense_probe import _cfg
from test_gpu_joint_outcomes import Probe

pytestmark = pytest.mark.gpu
SEED = 0x0C7_0BE5
WM = 233
SENTINEL = -12345.678
CONFIGS = {"config": _cfg(), "jorge": _cfg("jorge.json")}
WMS = {"config": WM, "jorge": 75}       # months at which a plan's options both fail and succeed (jorge.json never fails at 233)
KNOBS = {"scenarios": "MCR_SCENARIO_FANOUT_MIN_WAVES", "assumptions": "MCR_ASSUMPTION_FANOUT_MIN_WAVES", "income": "MCR_INCOME_FANOUT_MIN_WAVES"}
KINDS = ("scenarios", "assumptions", "income")

_REFERENCE = {}   # (config, seed, stream, path range, month) -> (final row, ruin row) of the summary batch: computed once, shared


def reference_rows(cfgd, seed=SEED, stream=0, begin=0, n=321, wm=WM):
    key = (json.dumps(cfgd, sort_keys=True, default=str), seed, stream, begin, n, wm)
    if key not in _REFERENCE:
        r = E.run_batch_host(params_from_config(Config(**cfgd)), seed, stream, begin, n, wm, want_trajectories=False, want_bins=False)
        ok = r["success"].astype(bool)
        assert np.array_equal(np.isnan(r["years_to_ruin"]), ok)           # (YearsToRuin is NaN exactly on the paths that succeed)
        fin, ruin = np.where(ok, r["final_balance"], np.nan), r["years_to_ruin"].copy()
        fin.setflags(write=False)
        ruin.setflags(write=False)
        _REFERENCE[key] = (fin, ruin)
    return _REFERENCE[key]


def same_bits(a, b):
    """Equal as doubles, NaN = NaN, and -0.0 != 0.0: NaNs compared as NaNs (their payload is not part of the contract), the
    rest as bit patterns."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


class OutcomesProbe(Probe):
    def outcomes(self, seed=SEED, stream=0, begin=0, n=321, wm=WM, records=None, **kw):
        fn = {"scenarios": E.probe_scenarios_outcomes, "assumptions": E.probe_assumptions_outcomes, "income": E.probe_income_outcomes}[self.kind]
        out = fn(params_from_config(Config(**self.cfgd)), seed, stream, begin, n, wm, *self._args(self.records if records is None else records), **kw)
        return out, self.launches()

    def rows(self, **kw):
        refs = [reference_rows(c, **kw) for c in self.configs]
        return np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs])


def where(**kw):
    """The launch a test means: this file's defaults (not the joint tests') with `kw` on top."""
    return dict(dict(seed=SEED, stream=0, begin=0, n=321, wm=WM), **kw)


def check(probe, fanout=True, stride=None, want_final=True, want_ruin=True, **kw):
    import torch

    kw = where(**kw)
    n, L = kw["n"], len(probe.records)
    width = (n + 63) // 64 * 64 if stride is None else stride
    slab = lambda want: torch.full((L, width), SENTINEL, dtype=torch.float64, device="cuda") if want else None  # noqa: E731
    (counts, fin, ruin), launches = probe.outcomes(final_balance=slab(want_final), years_to_ruin=slab(want_ruin), path_stride=width, **kw)
    want_fin, want_ruin_rows = probe.rows(**kw)
    for got, want, asked in ((fin, want_fin, want_final), (ruin, want_ruin_rows, want_ruin)):
        if not asked:
            assert got is None
            continue
        got = got.cpu().numpy()
        assert got.shape == (L, width)
        assert same_bits(got[:, :n], want), (probe.kind, [int(k) for k in range(L) if not same_bits(got[k, :n], want[k])])
        assert np.all(got[:, n:] == SENTINEL), "columns at or beyond n_paths must not be written"
    counts = counts.cpu().numpy()
    assert counts.tolist() == probe.plain(**kw).cpu().numpy().tolist()
    assert counts[:, 0].tolist() == (~np.isnan(want_fin)).sum(axis=1).tolist() and counts[:, 1].tolist() == [n] * L
    if launches is not None:
        assert (launches >= 1) if fanout else (launches == 0), launches
    return counts, fin, ruin


# ---- 1. rows against the library's own summary launches ---------------------------------------------------------------------
@pytest.mark.parametrize("begin", [0, 2**32 - 100])
@pytest.mark.parametrize("n", [321, 512])
@pytest.mark.parametrize("cfg", sorted(CONFIGS))
@pytest.mark.parametrize("kind", KINDS)
def test_rows_equal_summary_launches(kind, cfg, n, begin):
    counts, fin, ruin = check(OutcomesProbe(kind, CONFIGS[cfg], 5), n=n, begin=begin, wm=WMS[cfg], stride=n + 37)
    ruin = ruin.cpu().numpy()[:, :n]
    assert np.isnan(ruin).any() and (~np.isnan(ruin)).any()                 # both outcomes occur


@pytest.mark.parametrize("kind", KINDS)
def test_two_launch_groups_one_option_no_option_one_row(kind):
    probe = OutcomesProbe(kind, CONFIGS["config"], 17)
    counts, fin, ruin = check(probe)
    if kind != "scenarios":
        assert probe.launches() == 2
    # one option: its own launch, equal to its row of the fan-out
    one = OutcomesProbe(kind, CONFIGS["config"], 17)
    one.records, one.configs = probe.records[6:7], probe.configs[6:7]
    c1, f1, r1 = check(one, fanout=False)
    assert f1.cpu().numpy().tobytes() == fin[6:7].cpu().numpy().tobytes() and r1.cpu().numpy().tobytes() == ruin[6:7].cpu().numpy().tobytes()
    assert c1.tolist() == counts[6:7].tolist()
    # no option
    (c0, f0, r0), _ = probe.outcomes(records=[])
    assert c0.shape == (0, 2) and f0.shape[0] == 0 and r0.shape[0] == 0
    # one of the two rows
    five = OutcomesProbe(kind, CONFIGS["config"], 5)
    check(five, want_ruin=False)
    check(five, want_final=False)
    # neither: the plain probe
    (c, f, r), _ = five.outcomes(final_balance=False, years_to_ruin=False)
    assert f is None and r is None and c.cpu().numpy().tolist() == five.plain(**where()).cpu().numpy().tolist()


@pytest.mark.parametrize("kind", KINDS)
def test_forced_per_option_route_is_byte_identical(kind, monkeypatch):
    for cfg, L, n, begin in (("config", 5, 321, 0), ("jorge", 5, 512, 2**32 - 100), ("config", 17, 321, 0)):
        probe = OutcomesProbe(kind, CONFIGS[cfg], L)
        monkeypatch.setenv(KNOBS[kind], "0")
        fan = check(probe, fanout=True, n=n, begin=begin, wm=WMS[cfg], stride=n + 37)
        launches = probe.launches()
        assert launches is None or launches == (2 if L == 17 else 1)
        monkeypatch.setenv(KNOBS[kind], str(2**40))
        per = check(probe, fanout=False, n=n, begin=begin, wm=WMS[cfg], stride=n + 37)
        assert probe.launches() in (None, 0)
        assert fan[0].tolist() == per[0].tolist()
        for a, b in zip(fan[1:], per[1:]):
            assert same_bits(a.cpu().numpy(), b.cpu().numpy())
        check(probe, fanout=False, n=n, begin=begin, wm=WMS[cfg], want_ruin=False)      # the ruin column in the library's scratch
        check(probe, fanout=False, n=n, begin=begin, wm=WMS[cfg], want_final=False)
    one = OutcomesProbe(kind, CONFIGS["config"], 5)
    one.records, one.configs = one.records[1:2], one.configs[1:2]
    check(one, fanout=False)


@pytest.mark.parametrize("kind", KINDS)
def test_numpy_stream_takes_the_per_option_route(kind):
    rng = N.numpy_rng(1234, child_offset=0)
    probe = OutcomesProbe(kind, CONFIGS["config"], 5)
    (counts, fin, ruin), launches = probe.outcomes(seed=rng, stream=1, begin=0, n=321, wm=13)
    assert launches in (None, 0)
    for k, c in enumerate(probe.configs):
        r = E.run_batch_host(params_from_config(Config(**c)), rng, 1, 0, 321, 13, want_trajectories=False, want_bins=False)
        assert same_bits(fin[k, :321].cpu().numpy(), np.where(r["success"].astype(bool), r["final_balance"], np.nan))
        assert same_bits(ruin[k, :321].cpu().numpy(), r["years_to_ruin"])


# ---- 2. the ruin-month reduction ---------------------------------------------------------------------------------------------
def bincount(rows, n, ry):
    out = np.zeros((rows.shape[0], 12 * ry + 1), dtype=np.int64)
    for k, row in enumerate(rows):
        y = row[:n]
        m = np.rint(12.0 * y[~np.isnan(y)])
        m = m[(m >= 0) & (m <= 12 * ry)].astype(np.int64)         # (months outside the table are dropped)
        out[k] = np.bincount(m, minlength=12 * ry + 1)
    return out


def test_ruin_month_counts_of_the_probes_rows():
    for cfg in sorted(CONFIGS):
        ry = int(CONFIGS[cfg]["retirement_years"])
        probe = OutcomesProbe("income", CONFIGS[cfg], 5)
        for n in (321, 512):
            (counts, fin, ruin), _ = probe.outcomes(n=n, wm=WMS[cfg], path_stride=n + 37)
            got = E.ruin_month_counts(ruin, n, ry).cpu().numpy()
            want = bincount(probe.rows(n=n, wm=WMS[cfg])[1], n, ry)
            assert got.tolist() == want.tolist()
            assert (got.sum(axis=1) + counts.cpu().numpy()[:, 0]).tolist() == [n] * 5
            assert got.sum() > 0 and (got > 0).sum() > 5


@pytest.mark.parametrize("ry", [1, 60, 400])       # 400: 4 801 cells, past the 4 096 cells of the LDS histogram -> global atomics
def test_ruin_month_counts_equal_bincount(ry):
    import torch

    rng = np.random.default_rng(7 + ry)
    for n in (0, 1, 63, 65, 5003):
        stride = n + 29
        months = rng.integers(0, 12 * ry + 1, size=(4, stride))
        if ry > 1:
            months[1] = rng.integers(0, 3, size=stride) * (6 * ry)     # three cells take everything: colliding lanes
        y = months.astype(np.float64) / 12.0
        y[rng.random(size=y.shape) < 0.4] = np.nan
        y[2] = np.nan                                               # a row of paths that all succeed
        y[3, : min(n, 5)] = [-1.0 / 12.0, ry + 1.0 / 12.0, 1e300, -1e300, ry][: min(n, 5)]     # outside the table (dropped), and the last cell
        dev = torch.as_tensor(y, device="cuda")
        got = E.ruin_month_counts(dev, n, ry)
        want = bincount(y, n, ry)
        assert got.cpu().numpy().tolist() == want.tolist(), (ry, n)
        assert got[2].sum().item() == 0
        again = E.ruin_month_counts(dev, n, ry, into=got)             # a second call into the same table accumulates
        assert again is got and got.cpu().numpy().tolist() == (2 * want).tolist(), (ry, n)
    with pytest.raises(ValueError):
        E.ruin_month_counts(torch.zeros((2, 10), dtype=torch.float64, device="cuda"), 11, ry)


# ---- 3. quantiles of the successful cohort -----------------------------------------------------------------------------------
def test_final_balance_quantiles_equal_pandas():
    import pandas as pd

    qs = [0.05, 0.25, 0.5, 0.75, 0.95]
    for kind in KINDS:
        probe = OutcomesProbe(kind, CONFIGS["config"], 5)
        (counts, fin, ruin), _ = probe.outcomes(n=512)
        got, cohort = A.row_quantiles(fin, 512, qs)
        assert cohort.tolist() == counts.cpu().numpy()[:, 0].tolist()
        host = fin.cpu().numpy()[:, :512]
        for k in range(5):
            want = pd.Series(host[k]).quantile(qs).to_numpy()
            if cohort[k] == 0:
                assert np.isnan(want).all()
            else:
                np.testing.assert_allclose(got[k], want, rtol=0, atol=0)
        assert (cohort > 0).any()


# ---- 4. argument errors ------------------------------------------------------------------------------------------------------
def test_argument_errors_leave_the_outputs_untouched():
    import ctypes as C

    import torch

    p = params_from_config(Config(**CONFIGS["config"]))
    lib = N.load_library()
    n, L = 321, 3
    counts = torch.full((L, 2), -7, dtype=torch.int64, device="cuda")
    fin = torch.full((L, n), SENTINEL, dtype=torch.float64, device="cuda")
    ruin = torch.full((L, n), SENTINEL, dtype=torch.float64, device="cuda")
    rng = E._as_rng(SEED)
    stream = C.c_void_p(torch.cuda.current_stream(0).cuda_stream)

    def call(records, stride):
        arr, k = E._scenario_records(records)
        rows = N.McrOptionOutcomes(fin.data_ptr(), ruin.data_ptr(), stride)
        return lib.mcr_probe_scenarios_outcomes_rng(C.byref(p), C.byref(rng), 0, 0, n, WM, arr, k, counts.data_ptr(), C.byref(rows), 0, stream)

    good = [(1e5, 100.0, 3000.0)] * L
    assert call(good, n - 1) == N.MCR_ERR_INVALID_ARG and "path_stride" in N.last_error()
    assert call(good[:2] + [(1e5, 100.0, float("nan"))], n) == N.MCR_ERR_INVALID_ARG and "scenarios[2].monthly_expenses" in N.last_error()
    torch.cuda.synchronize()
    assert torch.all(counts == -7) and torch.all(fin == SENTINEL) and torch.all(ruin == SENTINEL)
    assert call(good, n) == 0
    torch.cuda.synchronize()
    assert counts[:, 1].tolist() == [n] * L and not torch.any(ruin == SENTINEL)
    with pytest.raises(RuntimeError, match=r"options\[0\]\.start_at_age"):
        E.probe_income_outcomes(p, SEED, 0, 0, n, WM, 0, [(1.0, 1.0, 1.0, 1.0, 121.0, None)])
    with pytest.raises(RuntimeError, match=r"records\[0\]\.equity_inflation_rho"):
        E.probe_assumptions_outcomes(p, SEED, 0, 0, n, WM, [(1.0, 1.0, 1.0, 0.05, 0.1, 0.02, 0.01, 0.01, 0.01, 1.5)])
    with pytest.raises(ValueError, match="row slab"):
        E.probe_scenarios_outcomes(p, SEED, 0, 0, n, WM, good, final_balance=torch.zeros((L, n), dtype=torch.float64, device="cuda"), path_stride=n + 1)


# ---- 5. the simulator, two ranks, the command line ---------------------------------------------------------------------------
def test_simulator_outcomes_agree_with_the_plain_methods_and_the_rows():
    sim, n = _sim(), 3000
    out = sim.option_outcomes_by_income_options(240, "State Pension", CLAIMS, n)
    plain = sim.success_probability_by_income_options(240, "State Pension", CLAIMS, n)
    assert out.probabilities.dtype == plain.dtype and out.probabilities.tobytes() == plain.tobytes()
    assert len(out) == len(CLAIMS) and out.n_paths == n and out.horizon_months == 12 * sim.params_model.retirement_years
    assert (out.successes + out.ruin_months.sum(axis=1)).tolist() == [n] * len(CLAIMS)
    assert out.cohort.tolist() == out.successes.tolist()
    assert out.ruin_months[1].tolist() == out.ruin_months[2].tolist()              # the duplicate
    assert out.retirement_age == sim.params_model.current_age + 20.0
    scenarios = [{}, {"monthly_expenses": 9000.0}, {"initial_balance": 0.0}]
    assert sim.option_outcomes_by_scenarios(240, scenarios, n).probabilities.tobytes() == sim.success_probability_by_scenarios(240, scenarios, n).tobytes()
    records = [{}, {"inv1_returns_mean": 0.03}, {"inflation_rate_mean": 0.06}]
    assert sim.option_outcomes_by_assumptions(240, records, n).probabilities.tobytes() == sim.success_probability_by_assumptions(240, records, n).tobytes()
    assert len(sim.option_outcomes_by_scenarios(240, [], n)) == 0
    custom = sim.option_outcomes_by_scenarios(240, scenarios, n, quantiles=(0.5,))
    assert custom.quantiles == (0.5,) and custom.final_quantiles.shape == (3, 1)


OUTCOME_KEYS = {"lasts_until_age", "median_ruin_age", "final_balance"}


def test_outcome_documents_extend_the_plain_ones():
    sim, n = _sim(), 3000
    plain = sim.compare_claiming_options(240, "State Pension", CLAIMS, n)
    rich = sim.compare_claiming_options(240, "State Pension", CLAIMS, n, outcomes=True)
    assert set(rich) == set(plain)
    assert dict(rich, options=[{k: v for k, v in r.items() if k not in OUTCOME_KEYS} for r in rich["options"]]) == plain
    for r in rich["options"]:
        assert set(r["lasts_until_age"]) == {"90", "95", "99"} and set(r["final_balance"]) == {"p5", "p25", "p50", "p75", "p95"}
        ages = [r["lasts_until_age"][c] for c in ("99", "95", "90")]
        known = [a for a in ages if a is not None]
        assert known == sorted(known)                                            # less confidence, a later age
        if r["probability"] < 100.0:
            assert r["median_ruin_age"] is not None
        fb = r["final_balance"]
        if r["probability"] > 0.0:
            assert fb["p5"] <= fb["p25"] <= fb["p50"] <= fb["p75"] <= fb["p95"]
    both = sim.compare_claiming_options(240, "State Pension", CLAIMS, n, paired=True, outcomes=True)
    paired = sim.compare_claiming_options(240, "State Pension", CLAIMS, n, paired=True)
    assert dict(both, options=[{k: v for k, v in r.items() if k not in OUTCOME_KEYS} for r in both["options"]]) == paired
    shifts = [("equity -2", {"inv1_returns_mean": -0.02}), ("inflation +2", {"inflation_rate_mean": 0.02})]
    plain = sim.stress_test(240, shifts, n)
    rich = sim.stress_test(240, shifts, n, outcomes=True)
    assert [{k: v for k, v in r.items() if k not in OUTCOME_KEYS} for r in rich] == plain
    assert all(OUTCOME_KEYS <= set(r) for r in rich)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_return_the_single_process_outcomes(tmp_path):
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "option_outcomes_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        stdout, _ = p.communicate(timeout=600)
        assert p.returncode == 0, stdout.decode()[-3000:]
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    whole = outcomes_document(_sim().option_outcomes_by_income_options(240, "State Pension", CLAIMS, DIST_PATHS))
    for r in res:
        assert r["outcomes"] == whole
        assert r["shard"][1] < DIST_PATHS                                        # each rank ran a part of the range only
    assert sorted(tuple(r["shard"]) for r in res) == [(0, 2502), (2502, 2501)]


def test_cli_outcomes_smoke():
    cmd = [sys.executable, *(["-s"] if sys.flags.no_user_site else []), os.path.join(REPO, "examples", "run_scenario.py"),
           os.path.join(REPO, "scenarios", "config.json"), "--seed", "7", "--paths", "2000", "--working-months", "240",
           "--income-options", "State Pension", "--claim-ages", "62,67,70", "--outcomes"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(doc["options"]) == 3 and all(OUTCOME_KEYS <= set(o) for o in doc["options"])
