"""Joint probes (`mcr_probe_*_joint_rng`, `engine.probe_*_joint`, `engine.joint_counts`) on the GPU.

The contract: row k of `masks` holds, bit for bit, the per-path `success` column of a plain full-output launch of the
parameter block with option k's fields replaced (`engine.run_batch_host`); ``joint = F @ F.T`` of those flags, ``extremes`` =
{paths on which all options succeed, paths on which none does}; `counts` is the plain probe's tensor and ``joint``'s diagonal its
success column -- on the fan-out route (the ballots of the fan-out kernel's consumer waves) and on the per-option route (a
success column per launch, packed), which must agree to the byte."""

from __future__ import annotations

import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import count_fuzz as F
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from monte_carlo_retirement_amd.income import INCOME_OPTION_FIELDS
from monte_carlo_retirement_amd.stress import assumption_records
from joint_dist_worker import CLAIMS, make_simulator as _sim
from test_gpu_assumption_probe import _overrides
from test_gpu_expense_probe import _cfg, _stream
from test_gpu_income_probe import _options, _replaced
from test_gpu_scenario_probe import FIELDS, SCENARIOS, _records

pytestmark = pytest.mark.gpu
SEED = 0x101_27
N_PATHS = 4133          # 64 whole 64-path blocks + 37
BEGIN = 12_345          # not a multiple of 64
WM = 233
CONFIG = SCENARIOS["config"]           # scenarios/config.json
#: 10 paying non-indexed streams = 10 lock columns per consumer wave: a launch takes 9 options (8 of the assumption probe),
#: so 11 options go as 6 + 5 and 17 as 9 + 8 (6 + 6 + 5)
FROZEN10 = _cfg(other_income_streams=[dict(_stream(i), inflation_indexed=False) for i in range(10)])


def unpack(masks, n_paths):
    """Device int64 mask rows -> uint8 flags [n, n_paths]; also returns the tail bits beyond n_paths (must be 0)."""
    words = masks.cpu().numpy().view(np.uint64)
    bits = np.unpackbits(words.view(np.uint8).reshape(words.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n_paths], bits[:, n_paths:]


def expected(flags):
    f = flags.astype(np.int64)
    return f @ f.T, [int(f.all(axis=0).sum()), int((~f.any(axis=0)).sum())]


# ---- 1. the reduction alone ------------------------------------------------------------------------------------------------
def _random_masks(rng, n, n_paths, dirty_tail):
    words = (n_paths + 63) // 64
    m = rng.integers(0, 2**64, size=(n, words), dtype=np.uint64)
    clean = m.copy()
    if n_paths % 64:
        clean[:, -1] &= np.uint64((1 << (n_paths % 64)) - 1)
    if dirty_tail and n_paths % 64:
        m = clean.copy()
        m[:, -1] |= np.uint64(~((1 << (n_paths % 64)) - 1) & (2**64 - 1))     # every bit beyond n_paths set
    else:
        m = clean
    bits = np.unpackbits(clean.view(np.uint8).reshape(n, -1), axis=1, bitorder="little")[:, :n_paths]
    return m, bits


@pytest.mark.parametrize("n", [1, 2, 15, 17, 32])
def test_joint_counts_equal_numpy(n):
    import torch

    rng = np.random.default_rng(100 + n)
    for n_paths in (1, 63, 64, 65, 4133, 64 * 1000):
        for dirty in ((False, True) if n_paths in (63, 65, 4133) else (False,)):
            m, bits = _random_masks(rng, n, n_paths, dirty)
            joint, extremes = E.joint_counts(torch.as_tensor(m.view(np.int64), device="cuda"), n_paths)
            want_joint, want_extremes = expected(bits)
            assert joint.cpu().numpy().tolist() == want_joint.tolist(), (n, n_paths, dirty)
            assert extremes.cpu().numpy().tolist() == want_extremes, (n, n_paths, dirty)


def test_joint_counts_of_constant_and_identical_rows():
    import torch

    n_paths = 4133
    rng = np.random.default_rng(5)
    m, bits = _random_masks(rng, 6, n_paths, False)
    m[1] = np.uint64(2**64 - 1)          # all ones (its tail too: the kernel clears it)
    bits[1] = 1
    m[2] = 0
    bits[2] = 0
    m[4] = m[0]
    bits[4] = bits[0]
    joint, extremes = E.joint_counts(torch.as_tensor(m.view(np.int64), device="cuda"), n_paths)
    joint = joint.cpu().numpy()
    want_joint, want_extremes = expected(bits)
    assert joint.tolist() == want_joint.tolist() and extremes.cpu().numpy().tolist() == want_extremes
    assert joint[1, 1] == n_paths and joint[2].tolist() == [0] * 6 and joint[0, 4] == joint[0, 0] == joint[4, 4]
    assert joint[1].tolist() == joint.diagonal().tolist()      # against all ones: every option's own count
    assert want_extremes[0] == 0                               # (a row of zeros: no path on which all succeed)
    ones = torch.full((3, (n_paths + 63) // 64), -1, dtype=torch.int64, device="cuda")
    joint, extremes = E.joint_counts(ones, n_paths)
    assert joint.cpu().numpy().tolist() == [[n_paths] * 3] * 3 and extremes.cpu().numpy().tolist() == [n_paths, 0]
    joint, extremes = E.joint_counts(torch.zeros_like(ones), n_paths)
    assert joint.cpu().numpy().tolist() == [[0] * 3] * 3 and extremes.cpu().numpy().tolist() == [0, n_paths]
    with pytest.raises(ValueError):
        E.joint_counts(torch.zeros((33, 65), dtype=torch.int64, device="cuda"), n_paths)
    with pytest.raises(ValueError):
        E.joint_counts(torch.zeros((3, 64), dtype=torch.int64, device="cuda"), n_paths)


# ---- 2. masks and matrix against plain launches, per probe -----------------------------------------------------------------
_FLAGS = {}   # (config, seed, stream, path range, month) -> the plain launch's success column: computed once, shared


def plain_flags(cfgd, seed=SEED, stream=0, begin=BEGIN, n=N_PATHS, wm=WM):
    def run():
        return E.run_batch_host(params_from_config(Config(**cfgd)), seed, stream, begin, n, wm, want_trajectories=False,
                                want_bins=False)["success"].astype(np.uint8)

    if not isinstance(seed, int):   # (a NumPy-stream descriptor: one small case per probe, not shared)
        return run()
    key = (json.dumps(cfgd, sort_keys=True, default=str), seed, stream, begin, n, wm)
    if key not in _FLAGS:
        _FLAGS[key] = run()
    return _FLAGS[key]


class Probe:
    """One of the three probes over a config: its option list, the configs the options stand for, the joint and plain calls."""

    def __init__(self, kind, cfgd, L, stream_index=0, income=None):
        self.kind, self.cfgd, self.idx = kind, cfgd, stream_index
        cfg = Config(**cfgd)
        if income is not None:      # (records, configs) given
            self.records, self.configs = income
        elif kind == "scenarios":
            self.records = _records(cfgd, L)
            self.configs = [dict(cfgd, **dict(zip(FIELDS, r))) for r in self.records]
        elif kind == "assumptions":
            overrides = _overrides(cfgd, L)
            self.records = assumption_records(cfg, overrides)
            self.configs = [dict(cfgd, **o) for o in overrides]
        else:
            self.records = _options(cfgd, stream_index, L)
            self.configs = [_replaced(cfgd, stream_index, o) for o in self.records]
        assert len(self.records) == L

    def _args(self, records):
        return (self.idx, records) if self.kind == "income" else (records,)

    def joint(self, seed=SEED, stream=0, begin=BEGIN, n=N_PATHS, wm=WM, records=None, **kw):
        fn = {"scenarios": E.probe_scenarios_joint, "assumptions": E.probe_assumptions_joint, "income": E.probe_income_joint}[self.kind]
        out = fn(params_from_config(Config(**self.cfgd)), seed, stream, begin, n, wm, *self._args(self.records if records is None else records), **kw)
        return out, self.launches()

    def plain(self, seed=SEED, stream=0, begin=BEGIN, n=N_PATHS, wm=WM):
        fn = {"scenarios": E.probe_scenarios, "assumptions": E.probe_assumptions, "income": E.probe_income}[self.kind]
        return fn(params_from_config(Config(**self.cfgd)), seed, stream, begin, n, wm, *self._args(self.records))

    def launches(self):
        lib = N.load_library()
        return {"scenarios": lambda: None, "assumptions": lib.mcr_probe_assumptions_last_fanout_launches,
                "income": lib.mcr_probe_income_last_fanout_launches}[self.kind]()

    def flags(self, **kw):
        return np.stack([plain_flags(c, **kw) for c in self.configs])


def check(probe, fanout=True, **kw):
    (counts, joint, extremes, masks), launches = probe.joint(**kw)
    n = kw.get("n", N_PATHS)
    flags = probe.flags(**kw)
    got, tail = unpack(masks, n)
    assert not tail.any(), "bits beyond n_paths must be 0"
    assert np.array_equal(got, flags), (probe.kind, [int(x) for x in np.flatnonzero((got != flags).any(axis=1))])
    want_joint, want_extremes = expected(flags)
    joint = joint.cpu().numpy()
    assert joint.tolist() == want_joint.tolist()
    assert extremes.cpu().numpy().tolist() == want_extremes
    counts = counts.cpu().numpy()
    assert counts.tolist() == probe.plain(**kw).cpu().numpy().tolist()
    assert joint.diagonal().tolist() == counts[:, 0].tolist() and counts[:, 1].tolist() == [n] * len(counts)
    if launches is not None:
        assert (launches >= 1) if fanout else (launches == 0), launches
    return counts, joint, extremes, masks


@pytest.mark.parametrize("L", [2, 5, 15, 17, 32])
@pytest.mark.parametrize("kind", ["scenarios", "assumptions", "income"])
def test_masks_and_matrix_equal_plain_launches(kind, L):
    counts, joint, _, _ = check(Probe(kind, CONFIG, L))
    if L >= 15:
        assert len(set(counts[:, 0].tolist())) > 2                     # the options do differ


# ---- 3. fewer options per launch than fifteen, uneven groups --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scenarios", "assumptions", "income"])
def test_uneven_launch_groups(kind):
    for L in (11, 17):
        check(Probe(kind, FROZEN10, L, stream_index=3))
    if kind != "scenarios":
        _, launches = Probe(kind, FROZEN10, 17, stream_index=3).joint()
        assert launches == {"income": 2, "assumptions": 3}[kind]       # 9 + 8; 6 + 6 + 5


# ---- 4. the per-option route -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scenarios", "assumptions", "income"])
def test_numpy_stream_takes_the_per_option_route(kind):
    rng = N.numpy_rng(1234, child_offset=0)
    check(Probe(kind, CONFIG, 5), fanout=False, seed=rng, stream=1, begin=0, n=1000, wm=13)


def test_generic_plan_takes_the_per_option_route(oracle):
    from test_gpu_income_vs_oracle import plan_jobs

    scn = next(s for s in F.scenarios(oracle, "generic") if s.cfgd["other_income_streams"])
    where = dict(seed=scn.seed, stream=scn.stream, begin=scn.begin, n=scn.n, wm=scn.wm)
    for kind in ("scenarios", "assumptions"):
        check(Probe(kind, scn.cfgd, 5), fanout=False, **where)
    idx, opts, lists = plan_jobs(scn)
    own = scn.cfgd["other_income_streams"][idx]
    money = tuple(float(scn.cfgd[f]) for f in FIELDS)
    records = [money + tuple(o.get(f, own[f]) for f in INCOME_OPTION_FIELDS[3:]) for o in opts]
    check(Probe("income", scn.cfgd, 5, stream_index=idx, income=(records, [dict(scn.cfgd, other_income_streams=l) for l in lists])),
          fanout=False, **where)


@pytest.mark.parametrize("kind", ["scenarios", "assumptions", "income"])
def test_one_option_equals_its_row_of_the_fanout(kind):
    probe = Probe(kind, CONFIG, 2)
    (counts2, joint2, _, masks2), _ = probe.joint()
    (counts1, joint1, extremes1, masks1), launches = probe.joint(records=probe.records[1:])
    assert launches in (None, 0)
    assert masks1.cpu().numpy().tobytes() == masks2[1:].cpu().numpy().tobytes()
    assert counts1.cpu().numpy().tolist() == counts2[1:].cpu().numpy().tolist()
    ok = int(counts1[0, 0])
    assert joint1.cpu().numpy().tolist() == [[ok]] == [[int(joint2[1, 1])]]
    assert extremes1.cpu().numpy().tolist() == [ok, N_PATHS - ok]


@pytest.mark.parametrize("kind,knob", [("scenarios", "MCR_SCENARIO_FANOUT_MIN_WAVES"), ("assumptions", "MCR_ASSUMPTION_FANOUT_MIN_WAVES"),
                                       ("income", "MCR_INCOME_FANOUT_MIN_WAVES")])
def test_forced_per_option_route_is_byte_identical(kind, knob, monkeypatch):
    probe = Probe(kind, CONFIG, 17)
    monkeypatch.setenv(knob, "0")
    fan, launches = probe.joint()
    assert launches is None or launches == 2
    monkeypatch.setenv(knob, str(2**40))
    per, launches = probe.joint()
    assert launches is None or launches == 0
    for a, b in zip(fan, per):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    flags, _ = unpack(per[3], N_PATHS)
    assert np.array_equal(flags, probe.flags())


# ---- 5. masks kept by the library -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["scenarios", "assumptions", "income"])
def test_library_scratch_masks_give_the_same_matrix(kind, monkeypatch):
    probe = Probe(kind, CONFIG, 17)
    knob = {"scenarios": "MCR_SCENARIO_FANOUT_MIN_WAVES", "assumptions": "MCR_ASSUMPTION_FANOUT_MIN_WAVES", "income": "MCR_INCOME_FANOUT_MIN_WAVES"}[kind]
    for waves in ("0", str(2**40)):                                    # the fan-out route and the per-option route
        monkeypatch.setenv(knob, waves)
        (counts, joint, extremes, masks), _ = probe.joint()
        (counts0, joint0, extremes0, masks0), _ = probe.joint(masks=None)
        assert masks0 is None and masks is not None
        assert joint0.cpu().numpy().tolist() == joint.cpu().numpy().tolist()
        assert extremes0.cpu().numpy().tolist() == extremes.cpu().numpy().tolist()
        assert counts0.cpu().numpy().tolist() == counts.cpu().numpy().tolist()


def test_rows_kept_from_two_probes_combine():
    """`engine.joint_counts` over mask rows of a scenario probe and an income probe of the same path range."""
    import torch

    a, b = Probe("scenarios", CONFIG, 5), Probe("income", CONFIG, 5)
    ma, mb = a.joint()[0][3], b.joint()[0][3]
    joint, extremes = E.joint_counts(torch.cat([ma, mb]), N_PATHS)
    want_joint, want_extremes = expected(np.concatenate([a.flags(), b.flags()]))
    assert joint.cpu().numpy().tolist() == want_joint.tolist() and extremes.cpu().numpy().tolist() == want_extremes


def test_argument_checks_on_the_device():
    p = params_from_config(Config(**CONFIG))
    with pytest.raises(ValueError, match="MCR_MAX_JOINT_OPTIONS"):
        E.probe_scenarios_joint(p, SEED, 0, 0, 100, 12, _records(CONFIG, 33))
    with pytest.raises(RuntimeError, match=r"scenarios\[1\]\.monthly_expenses"):
        E.probe_scenarios_joint(p, SEED, 0, 0, 100, 12, [(1.0, 1.0, 1.0), (1.0, 1.0, float("nan"))])
    counts, joint, extremes, masks = E.probe_scenarios_joint(p, SEED, 0, 0, 100, 12, [])
    assert counts.shape == (0, 2) and joint.shape == (0, 0) and masks.shape == (0, 2) and extremes.tolist() == [0, 0]
    counts, joint, extremes, masks = E.probe_scenarios_joint(p, SEED, 0, 0, 0, 12, _records(CONFIG, 3))      # no paths
    assert counts.tolist() == [[0, 0]] * 3 and joint.tolist() == [[0] * 3] * 3 and extremes.tolist() == [0, 0] and masks.shape == (3, 0)


# ---- 7. the simulator -----------------------------------------------------------------------------------------------------------
DIFFERENCE_KEYS = {"delta", "se", "se_unpaired", "p_value", "rescued"}


def test_simulator_probabilities_equal_the_plain_methods():
    sim, n = _sim(), 3000
    outcomes = sim.joint_outcomes_by_income_options(240, "State Pension", CLAIMS, n)
    plain = sim.success_probability_by_income_options(240, "State Pension", CLAIMS, n)
    assert outcomes.probabilities.dtype == plain.dtype and outcomes.probabilities.tobytes() == plain.tobytes()
    assert outcomes.n_paths == n and len(outcomes) == len(CLAIMS)
    assert outcomes.joint[1].tolist() == outcomes.joint[2].tolist()           # the duplicate
    assert outcomes.pair(1, 2)["only_a"] == outcomes.pair(1, 2)["only_b"] == 0
    assert 0 <= outcomes.all_succeed <= outcomes.successes.min() and 0 <= outcomes.none_succeed <= n - outcomes.successes.max()
    scenarios = [{}, {"monthly_expenses": 9000.0}, {"initial_balance": 0.0}]
    assert sim.joint_outcomes_by_scenarios(240, scenarios, n).probabilities.tobytes() == \
        sim.success_probability_by_scenarios(240, scenarios, n).tobytes()
    records = [{}, {"inv1_returns_mean": 0.03}, {"inflation_rate_mean": 0.06}]
    assert sim.joint_outcomes_by_assumptions(240, records, n).probabilities.tobytes() == \
        sim.success_probability_by_assumptions(240, records, n).tobytes()
    assert len(sim.joint_outcomes_by_scenarios(240, [], n)) == 0


def test_paired_documents_extend_the_plain_ones():
    sim, n = _sim(), 3000
    plain = sim.compare_claiming_options(240, "State Pension", CLAIMS, n)
    paired = sim.compare_claiming_options(240, "State Pension", CLAIMS, n, paired=True)
    assert set(paired) == set(plain) | {"tied_with_best", "all_succeed", "none_succeed"}
    stripped = dict({k: v for k, v in paired.items() if k in plain}, options=[{k: v for k, v in r.items() if k != "vs_best"} for r in paired["options"]])
    assert stripped == plain
    assert all(set(r["vs_best"]) == DIFFERENCE_KEYS for r in paired["options"])
    best = paired["best"]
    assert paired["options"][best]["vs_best"]["delta"] == 0.0 and best in paired["tied_with_best"]
    assert all(r["vs_best"]["delta"] >= 0.0 for r in paired["options"])
    assert all(r["vs_best"]["se"] <= r["vs_best"]["se_unpaired"] for r in paired["options"])
    assert all(set(r) == set(INCOME_OPTION_FIELDS) | {"probability", "vs_best"} for r in paired["options"])
    shifts = [("equity -2", {"inv1_returns_mean": -0.02}), ("inflation +2", {"inflation_rate_mean": 0.02})]
    plain = sim.stress_test(240, shifts, n)
    paired = sim.stress_test(240, shifts, n, paired=True)
    assert [{k: v for k, v in r.items() if k != "vs_base"} for r in paired] == plain
    for r in paired:
        v = r["vs_base"]
        assert set(v) == DIFFERENCE_KEYS | {"hurt", "helped"}
        assert v["delta"] == pytest.approx(-r["delta"], abs=1e-9) and v["delta"] == 100.0 * (v["hurt"] - v["helped"]) / n
    assert paired[0]["vs_base"]["hurt"] == paired[0]["vs_base"]["helped"] == 0 and paired[1]["vs_base"]["hurt"] > 0


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_return_the_single_process_matrix(tmp_path):
    out = str(tmp_path / "res")
    port = _free_port()
    procs = []
    for rank in range(2):
        env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK=str(rank),
                   OMP_NUM_THREADS="1")
        procs.append(subprocess.Popen([sys.executable, *(["-s"] if sys.flags.no_user_site else []),
                                       os.path.join(REPO, "tests", "joint_dist_worker.py"), out], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    for p in procs:
        stdout, _ = p.communicate(timeout=600)
        assert p.returncode == 0, stdout.decode()[-3000:]
    res = [json.load(open(f"{out}.{r}")) for r in range(2)]
    sim = _sim()
    whole = sim.joint_outcomes_by_income_options(240, "State Pension", CLAIMS, 5003)
    for r in res:
        assert r["joint"] == whole.joint.tolist() and r["extremes"] == list(whole.extremes) and r["n_paths"] == 5003
        assert r["probabilities"] == whole.probabilities.tolist()
        assert r["shard"][1] < 5003                                           # each rank ran a part of the range only
    assert sorted(tuple(r["shard"]) for r in res) == [(0, 2502), (2502, 2501)]
