"""The glide whole-path launches on the GPU (`mcr_run_glide_rng`, `mcr_run_glide_year_bins_rng`, `_host_rng`: path_kernel's GLIDE
form in MODE 0, 1 and 3), held to what the tree already computes:

1. under a constant table they are the plain launches (`mcr_run_batch_rng`, `mcr_run_year_bins_rng`), bit for bit and cell for cell;
2. under any table they are the glide probes' option: the count, the joint probe's ballots, the outcome probe's rows bit for bit;
4. the internal identities of a yearly-bins launch (tests/glide_run.py: `check_identities`), on every plan and table of 2.;
5. the shapes the weight can go wrong at, each against the probes bit for bit and against the model (tests/glide_model.cpp);
6. the `generic` class is MCR_ERR_UNSUPPORTED from all three entries, sentinel-filled outputs untouched;
7. any subset of the tables NULL, and the 512-bin LDS cap.

(3., the model on every plan, is tests/test_gpu_glide_run_vs_oracle.py; 8., the simulator and the document, is
tests/test_gpu_glide_run_simulator.py.)  The plans are the stratified random ones of tests/count_fuzz.py (321 and 512 paths: a
ragged last wave and workgroup) under the five tables of tests/glide_fuzz.py; the shapes of 5. are 600 paths of
tests/spending_rule_model.py's plans, and one 5 003-path case."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import count_fuzz as F
import glide_fuzz as GF
import glide_run as G
import spending_rule_model as M
from conftest import REPO
from monte_carlo_retirement_amd import Config, params_from_config
from monte_carlo_retirement_amd import _native as N
from monte_carlo_retirement_amd import engine as E
from test_gpu_count_routes_vs_oracle import _env
from test_gpu_differential import ABS, REL
from test_gpu_joint_outcomes import unpack

pytestmark = pytest.mark.gpu
CLASSES = tuple(c for c in F.CLASSES if c != "generic")
N_PATHS = 600
SEED, STREAM = M.SEED, M.STREAM
EDGES, WR_EDGES = E.default_year_edges(64), E.default_wr_edges(64)
TABLES = G.BLOCKS[3:]


def _at(scn):
    return scn.seed, scn.stream, scn.begin, scn.n


def _device_bins(p, at, wm, table, edges=None, wr_edges=None):
    batch = E.YearBinsBatch(p, wm, edges, wr_edges, glide_path=table)
    batch.launch(*at)
    return batch.host()


# ---- 1. constant tables are the plain launches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_constant_tables_are_the_plain_launches(oracle, cls):
    for scn in F.scenarios(oracle, cls):
        p, at, a = scn.params(), _at(scn), float(scn.cfgd["allocation_inv1_pct"])
        horizon = GF.horizon_years(scn)
        with _env({}):
            plain = E.run_batch_host(p, *at, scn.wm, want_trajectories=False)
            plain_bins = E.run_year_bins_host(p, *at, scn.wm)
            for name, table in (("[a]", [a]), ("[a, a, a]", [a, a, a]), ("[a] * horizon + [1 - a] * 5", [a] * horizon + [1.0 - a] * 5)):
                ctx = scn.context(f"glide launch under the constant table {name}")
                summary = E.run_glide_host(p, *at, scn.wm, table, want="summary")
                counts = E.run_glide_host(p, *at, scn.wm, table, want="counts")
                for k in G.INTEGERS:
                    assert summary[k].tolist() == plain[k].tolist() == counts[k].tolist(), (k, ctx)
                for k in G.COLUMNS:
                    assert G.same_bits(summary[k], plain[k]), (k, ctx)
                host = E.run_glide_year_bins_host(p, *at, scn.wm, table)
                dev = _device_bins(p, at, scn.wm, table)
                for k in G.BLOCKS:
                    assert np.array_equal(host[k], plain_bins[k]), (k, ctx)
                    assert np.array_equal(dev[k].astype(np.uint64), plain_bins[k]), (k, "device entry", ctx)


# ---- 2. the launch is the probe's option; 4. the identities of a yearly-bins launch ------------------------------------------------
@pytest.mark.parametrize("cls", CLASSES)
def test_the_launch_is_the_probes_option(oracle, cls):
    for scn in F.scenarios(oracle, cls):
        p, at, records = scn.params(), _at(scn), GF.records(scn)
        with _env({}):
            counts = E.probe_glide_paths(p, *at, scn.wm, records).cpu().numpy()
            _, _, _, masks = E.probe_glide_paths_joint(p, *at, scn.wm, records)
            _, fin_t, ruin_t = E.probe_glide_paths_outcomes(p, *at, scn.wm, records)
            ballots, tail = unpack(masks, scn.n)
            assert not tail.any()
            fin, ruin = fin_t.cpu().numpy()[:, :scn.n], ruin_t.cpu().numpy()[:, :scn.n]
            for j, (name, table) in enumerate(zip(GF.NAMES, GF.tables(scn))):
                ctx = scn.context(f"glide launch under table {name} = {table}")
                summ = E.run_glide_host(p, *at, scn.wm, table, want="summary")
                cnt = E.run_glide_host(p, *at, scn.wm, table, want="counts")
                ok = summ["success"].astype(bool)
                assert summ["counters"].tolist() == cnt["counters"].tolist() == counts[j].tolist() == [int(ok.sum()), scn.n], ctx
                assert np.array_equal(summ["success"], ballots[j].astype(np.uint8)), ctx
                # the probe's NaN convention: final is NaN where the path failed, ruin is NaN where it succeeded
                assert G.same_bits(np.where(ok, summ["final_balance"], np.nan), fin[j]), ctx
                assert G.same_bits(summ["years_to_ruin"], ruin[j]) and np.array_equal(np.isnan(ruin[j]), ok), ctx
                for k in ("wr_obs_counts", "ruin_year_bins"):
                    assert summ[k].tolist() == cnt[k].tolist(), (k, ctx)
                yb = E.run_glide_year_bins_host(p, *at, scn.wm, table)
                G.check_identities(yb, summ, scn.n, scn.wm, ctx)


# ---- 5. shapes the weight can go wrong at -------------------------------------------------------------------------------------------
def _plan(plan, wm, level="neutral", **over):
    return Config(**dict(dict(M.plan_config(plan, REPO, wm), monthly_expenses=M.LEVELS[plan, wm][level]), **over))


def _step(a, wm):
    return [a] * ((wm + 11) // 12 + 1) + [1.0 - a]


def _against_probe_and_model(oracle, cfg, wm, table, n=N_PATHS, begin=0, what=""):
    """One table's three launches over [begin, begin + n): against the probes bit for bit, the model within the path contract, and
    the identities of the yearly-bins launch.  Returns the summary launch and the tables."""
    p = params_from_config(cfg)
    at = (SEED, STREAM, begin, n)
    record = [(float(cfg.initial_balance), float(cfg.monthly_contribution), float(cfg.monthly_expenses), tuple(table))]
    with _env({}):
        summ = E.run_glide_host(p, *at, wm, table, want="summary")
        cnt = E.run_glide_host(p, *at, wm, table, want="counts")
        yb = E.run_glide_year_bins_host(p, *at, wm, table, edges=EDGES, wr_edges=WR_EDGES)
        counts, fin_t, ruin_t = E.probe_glide_paths_outcomes(p, *at, wm, record)
    ok = summ["success"].astype(bool)
    assert counts.cpu().numpy().tolist() == [summ["counters"].tolist()] == [cnt["counters"].tolist()], what
    assert G.same_bits(np.where(ok, summ["final_balance"], np.nan), fin_t.cpu().numpy()[0, :n]), what
    assert G.same_bits(summ["years_to_ruin"], ruin_t.cpu().numpy()[0, :n]), what
    G.check_identities(yb, summ, n, wm, what)
    ry = int(cfg.retirement_years)
    ref = G.with_integers(GF.run_model(oracle, p, SEED, STREAM, begin, n, wm, table), ry)
    assert F.money_scale(ref) < F.SCALE_LIMIT, what
    assert np.array_equal(summ["success"], ref["success"]) and np.array_equal(summ["years_to_ruin"], ref["years_to_ruin"], equal_nan=True), what
    for k in G.INTEGERS:
        assert summ[k].tolist() == ref[k].tolist() == cnt[k].tolist(), (k, what)
    scale = np.maximum(1.0, np.abs(ref["trajectory"]).max(axis=0))
    for k in ("start_balance", "final_balance", "first_year_gross_withdrawal", "first_year_real_gross_withdrawal", "inflation_at_retirement"):
        err = np.abs(summ[k] - ref[k])
        assert np.all(err <= ABS + REL * np.maximum(np.abs(ref[k]), scale)), (k, float(err.max()), what)
    return summ, yb, ref


SHAPES = [
    ("wm % 12 != 0, a switch inside the first retirement year", "realized", 7, lambda a, wm, Y: _step(a, wm)),
    ("wm = 0", "streams", 0, lambda a, wm, Y: [float(x) for x in np.linspace(a, 1.0 - a, Y)]),
    ("wm = 7, a linear table", "streams", 7, lambda a, wm, Y: [float(x) for x in np.linspace(a, 1.0 - a, Y)]),
    ("[1.0, 0.0]: an asset turns to dust at row 12", "realized", 120, lambda a, wm, Y: [1.0, 0.0]),
    ("[1.0, 0.0] at wm = 7", "streams", 7, lambda a, wm, Y: [1.0, 0.0]),
    ("the annual-gains tax with total_months % 12 != 0: the settlement on the last row's weight", "annual", 7,
     lambda a, wm, Y: [a] * (Y - 1) + [1.0 - a]),
    ("the annual-gains tax, a table longer than the horizon", "annual", 120, lambda a, wm, Y: [a if y % 2 == 0 else GF.toward(a) for y in range(Y + 5)]),
]


@pytest.mark.parametrize("what,plan,wm,make", SHAPES, ids=[s[0] for s in SHAPES])
def test_shapes_the_weight_can_go_wrong_at(oracle, what, plan, wm, make):
    cfg = _plan(plan, wm)
    a = float(cfg.allocation_inv1_pct)
    Y = (wm + 12 * int(cfg.retirement_years) + 11) // 12
    table = make(a, wm, Y)
    summ, _, _ = _against_probe_and_model(oracle, cfg, wm, table, what=what)
    failed = N_PATHS - int(summ["counters"][0])
    assert 0 < failed < N_PATHS, (what, failed)
    if len(table) > 1 and table != [1.0, 0.0]:           # the table matters: the constant split's flags or balances differ
        p = params_from_config(cfg)
        const = E.run_glide_host(p, SEED, STREAM, 0, N_PATHS, wm, [a], want="summary")
        assert not G.same_bits(const["final_balance"], summ["final_balance"]), what


def test_the_last_rows_weight_settles_the_terminal_period(oracle):
    """total_months % 12 != 0 under the annual-gains tax: a table that differs from the constant split in its LAST entry alone
    changes only rows of the last calendar year -- the terminal settlement and its closing rebalance among them."""
    plan, wm = "annual", 7
    cfg = _plan(plan, wm)
    a, ry = float(cfg.allocation_inv1_pct), int(cfg.retirement_years)
    Y = (wm + 12 * ry + 11) // 12
    assert (wm + 12 * ry) % 12 != 0
    p = params_from_config(cfg)
    last = E.run_glide_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, [a] * (Y - 1) + [1.0 - a])      # (the default 256 + 256 bins)
    const = E.run_glide_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, [a] * Y)
    T = last["trajectory_bins"].shape[0]
    assert np.array_equal(last["trajectory_bins"][:T - 1], const["trajectory_bins"][:T - 1])        # the samples before the last calendar year
    assert not np.array_equal(last["trajectory_bins"][T - 1], const["trajectory_bins"][T - 1])


def test_several_workgroups_per_cu(oracle):
    """5 003 paths (20 workgroups, the last ragged)."""
    cfg = _plan("streams", 7)
    a = float(cfg.allocation_inv1_pct)
    _against_probe_and_model(oracle, cfg, 7, _step(a, 7), n=5003, what="5 003 paths")


@pytest.mark.parametrize("begin", (2 ** 32 - 100, 2 ** 40), ids=("2^32 - 100", "2^40"))
def test_path_ranges_beyond_32_bits(oracle, begin):
    cfg = _plan("realized", 120)
    a = float(cfg.allocation_inv1_pct)
    Y = (120 + 12 * int(cfg.retirement_years) + 11) // 12
    _against_probe_and_model(oracle, cfg, 120, [float(x) for x in np.linspace(a, 1.0 - a, Y)], begin=begin, what=f"path_begin {begin}")


def test_two_sub_ranges_sum_to_the_whole_range():
    cfg = _plan("annual", 120)
    a = float(cfg.allocation_inv1_pct)
    p, wm, table = params_from_config(cfg), 120, _step(a, 120)
    whole = E.run_glide_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, table, edges=EDGES, wr_edges=WR_EDGES)
    two = E.run_glide_year_bins_host(p, SEED, STREAM, 0, 333, wm, table, edges=EDGES, wr_edges=WR_EDGES)
    E.run_glide_year_bins_host(p, SEED, STREAM, 333, N_PATHS - 333, wm, table, edges=EDGES, wr_edges=WR_EDGES, into=two)
    for k in G.BLOCKS:
        assert np.array_equal(whole[k], two[k]), k
    c = [E.run_glide_host(p, SEED, STREAM, b, n, wm, table) for b, n in ((0, N_PATHS), (0, 333), (333, N_PATHS - 333))]
    for k in G.INTEGERS:
        assert c[0][k].tolist() == (c[1][k] + c[2][k]).tolist() == whole[k].tolist(), k
    b = E.YearBinsBatch(p, wm, EDGES, WR_EDGES, glide_path=table)            # the device-resident batch: two launches, one vector
    b.launch(SEED, STREAM, 0, 333)
    b.launch(SEED, STREAM, 333, N_PATHS - 333)
    host = b.host()
    for k in G.BLOCKS:
        assert np.array_equal(host[k].astype(np.uint64), whole[k]), k
    with pytest.raises(ValueError):
        E.run_glide_year_bins_host(p, SEED, STREAM, 0, 8, wm, table, edges=E.default_year_edges(8), wr_edges=WR_EDGES, into=two)
    # a plan on which nearly every path fails: whole waves leave the year loop early and pad their rows, barrier for barrier
    hard = params_from_config(_plan("annual", 120, monthly_expenses=3.0 * M.LEVELS["annual", 120]["symmetric"]))
    summ = E.run_glide_host(hard, SEED, STREAM, 0, N_PATHS, wm, table, want="summary")
    assert int(summ["counters"][0]) < 0.1 * N_PATHS
    yb = E.run_glide_year_bins_host(hard, SEED, STREAM, 0, N_PATHS, wm, table, edges=EDGES, wr_edges=WR_EDGES)
    G.check_identities(yb, summ, N_PATHS, wm, "a mostly failing plan")
    assert int(yb["wr_obs_counts"][-1]) == int(summ["counters"][0])


# ---- 6. the generic class ------------------------------------------------------------------------------------------------------------
def test_the_generic_class_is_unsupported_and_touches_nothing(oracle):
    import torch

    lib = N.load_library()
    stream = torch.cuda.current_stream(0).cuda_stream
    sentinel, fsentinel = -0x1234_5678, -12345.678
    for scn in F.scenarios(oracle, "generic"):
        ctx = scn.context("glide launches, generic class")
        p, rng = scn.params(), N.philox_rng(scn.seed)
        sz = E.query_sizes(p, scn.wm)
        T, ry = sz.trajectory_len, sz.retirement_years
        ints = [torch.full(shape, sentinel, dtype=torch.int64, device="cuda")
                for shape in ((2,), (ry,), (sz.ruin_bins,), (T, 66), (T, 66), (ry, 66), (66,))]
        cols = [torch.full((1024,), fsentinel, dtype=torch.float64, device="cuda") for _ in E.SUMMARY_FIELDS]
        flags = torch.full((1024,), 0x5A, dtype=torch.uint8, device="cuda")
        edges, wr_edges = torch.as_tensor(EDGES, device="cuda"), torch.as_tensor(WR_EDGES, device="cuda")
        host = [np.full(tuple(t.shape), 7, dtype=np.uint64) for t in ints]
        table = E.glide_table(GF.tables(scn)[1])

        def outputs(ptrs, e, we, summary):
            o = N.McrOutputs()
            o.counters, o.wr_obs_counts, o.ruin_year_bins = ptrs[:3]
            o.path_stride = 1024
            if summary:
                for k, t in zip(E.SUMMARY_FIELDS, cols):
                    setattr(o, k, t.data_ptr())
                o.success = flags.data_ptr()
            y = N.McrYearBins()
            y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e, 64, we, 64
            y.trajectory_bins, y.real_trajectory_bins, y.wr_bins, y.final_success_bins = ptrs[3:]
            return o, y

        head = (C.byref(p), C.byref(rng), scn.stream, scn.begin, scn.n, scn.wm, table, len(table))
        dev_ptrs = [t.data_ptr() for t in ints]
        with _env({}):
            for summary in (False, True):
                o, _ = outputs(dev_ptrs, edges.data_ptr(), wr_edges.data_ptr(), summary)
                rc = lib.mcr_run_glide_rng(*head, C.byref(o), 0, C.c_void_p(stream))
                assert rc == N.MCR_ERR_UNSUPPORTED and "glide path:" in N.last_error() and "supported" in N.last_error(), (rc, N.last_error(), ctx)
            o, y = outputs(dev_ptrs, edges.data_ptr(), wr_edges.data_ptr(), False)
            rc = lib.mcr_run_glide_year_bins_rng(*head, C.byref(o), C.byref(y), 0, C.c_void_p(stream))
            assert rc == N.MCR_ERR_UNSUPPORTED and "glide path:" in N.last_error() and "supported" in N.last_error(), (rc, N.last_error(), ctx)
            o, y = outputs([h.ctypes.data for h in host], EDGES.ctypes.data, WR_EDGES.ctypes.data, False)
            rc = lib.mcr_run_glide_year_bins_host_rng(*head, C.byref(o), C.byref(y), 0)
            assert rc == N.MCR_ERR_UNSUPPORTED and "glide path:" in N.last_error() and "supported" in N.last_error(), (rc, N.last_error(), ctx)
        torch.cuda.synchronize()
        for t in ints:
            assert (t.cpu() == sentinel).all(), ctx
        for t in cols:
            assert (t.cpu() == fsentinel).all(), ctx
        assert (flags.cpu() == 0x5A).all() and all(np.all(h == 7) for h in host), ctx


# ---- 7. any subset of the tables NULL; the LDS cap -------------------------------------------------------------------------------------
def _raw_call(p, wm, table, edges, wr_edges, skip=(), n=N_PATHS):
    """The host entry point with any subset of the tables NULL; returns the tables it was given (zeroed before)."""
    sz = E.query_sizes(p, wm)
    T, ry = sz.trajectory_len, sz.retirement_years
    e, we = (np.ascontiguousarray(x, dtype=np.float64) for x in (edges, wr_edges))
    nb, nw = e.size - 1, we.size - 1
    res = {"counters": np.zeros(2, np.uint64), "wr_obs_counts": np.zeros(ry, np.uint64), "ruin_year_bins": np.zeros(sz.ruin_bins, np.uint64),
           "trajectory_bins": np.zeros((T, nb + 2), np.uint64), "real_trajectory_bins": np.zeros((T, nb + 2), np.uint64),
           "wr_bins": np.zeros((ry, nw + 2), np.uint64), "final_success_bins": np.zeros(nb + 2, np.uint64)}
    ptr = {k: (None if k in skip else v.ctypes.data) for k, v in res.items()}
    o = N.McrOutputs()
    o.counters, o.wr_obs_counts, o.ruin_year_bins = ptr["counters"], ptr["wr_obs_counts"], ptr["ruin_year_bins"]
    y = N.McrYearBins()
    y.edges, y.n_bins, y.wr_edges, y.n_wr_bins = e.ctypes.data, nb, we.ctypes.data, nw
    for k in TABLES:
        setattr(y, k, ptr[k])
    w, rng = E.glide_table(table), N.philox_rng(SEED)
    rc = N.load_library().mcr_run_glide_year_bins_host_rng(C.byref(p), C.byref(rng), STREAM, 0, n, wm, w, len(w), C.byref(o), C.byref(y), 0)
    N.check(rc, "mcr_run_glide_year_bins_host_rng")
    return res


def test_null_tables_and_the_lds_cap():
    plan, wm = "streams", 7
    cfg = _plan(plan, wm)
    p, a = params_from_config(cfg), float(cfg.allocation_inv1_pct)
    table = _step(a, wm)
    full = _raw_call(p, wm, table, EDGES, WR_EDGES)
    ref = E.run_glide_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, table, edges=EDGES, wr_edges=WR_EDGES)
    for k in G.BLOCKS:
        assert np.array_equal(full[k], ref[k]), k
    subsets = [("trajectory_bins",), ("wr_bins",), TABLES, ("trajectory_bins", "real_trajectory_bins", "final_success_bins"),
               ("trajectory_bins", "wr_bins"), ("counters", "wr_obs_counts", "ruin_year_bins"),
               ("real_trajectory_bins", "final_success_bins", "wr_obs_counts"), tuple(k for k in G.BLOCKS if k != "wr_bins")]
    for skip in subsets:
        got = _raw_call(p, wm, table, EDGES, WR_EDGES, skip=skip)
        for k in G.BLOCKS:
            assert np.array_equal(got[k], np.zeros_like(full[k]) if k in skip else full[k]), (skip, k)
    # 512 + 512 bins, the LDS cap, on the rule test's shape (a plan without a frozen stream: its column would not fit beside them)
    cfg2 = _plan("realized", wm)
    p2, a2 = params_from_config(cfg2), float(cfg2.allocation_inv1_pct)
    plain = E.run_batch_host(p2, SEED, STREAM, 0, N_PATHS, wm, want_trajectories=False)
    top = float(plain["final_balance"].max())
    big_e, big_w = E.default_year_edges(N.MCR_MAX_YEAR_BINS, hi=max(top * 4.0, 1e7)), E.default_wr_edges(N.MCR_MAX_YEAR_BINS, 50.0)
    big_plain = E.run_year_bins_host(p2, SEED, STREAM, 0, N_PATHS, wm, edges=big_e, wr_edges=big_w)
    big = E.run_glide_year_bins_host(p2, SEED, STREAM, 0, N_PATHS, wm, [a2, a2], edges=big_e, wr_edges=big_w)
    assert big["trajectory_bins"].shape[1] == 514 and big["wr_bins"].shape[1] == 514
    for k in G.BLOCKS:
        assert np.array_equal(big[k], big_plain[k]), k
    t2 = _step(a2, wm)
    moving = E.run_glide_year_bins_host(p2, SEED, STREAM, 0, N_PATHS, wm, t2, edges=big_e, wr_edges=big_w)
    G.check_identities(moving, E.run_glide_host(p2, SEED, STREAM, 0, N_PATHS, wm, t2, want="summary"), N_PATHS, wm, "512-bin tables")


def test_lock_columns_beside_the_yearly_tables():
    """Frozen income streams whose lock columns do not fit beside the yearly tables in the LDS of four resident workgroups: the
    plain yearly-bins launch takes its generic form, the glide launch, which has none, gives up resident workgroups.  One frozen
    stream at 512 + 512 bins (no column left of the four-resident budget) and five at the default 256 + 256 (three left): a
    constant table gives the plain launch's tables cell for cell, a table that moves keeps the identities against its own summary
    launch and the probe's rows.  (What does not fit into the workgroup's 64 KB either is refused: tests/test_glide_run_cpu.py.)"""
    wm = 7
    frozen = [{"name": f"f{i}", "monthly_amount_today": 150.0 + 10 * i, "start_at_age": 58.0 + 2 * i, "duration_years": None if i % 2 else 9,
               "inflation_indexed": False, "tax_rate": 0.1} for i in range(5)]
    for what, streams, bins in (("one frozen stream, 512 + 512 bins", frozen[:1], N.MCR_MAX_YEAR_BINS), ("five frozen streams, 256 + 256 bins", frozen, 256)):
        cfg = _plan("realized", wm, other_income_streams=streams)
        p, a = params_from_config(cfg), float(cfg.allocation_inv1_pct)
        assert p.n_streams == len(streams), what
        e, we = E.default_year_edges(bins, hi=1e9), E.default_wr_edges(bins, 50.0)
        plain = E.run_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, edges=e, wr_edges=we)
        const = E.run_glide_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, [a, a], edges=e, wr_edges=we)
        for k in G.BLOCKS:
            assert np.array_equal(const[k], plain[k]), (what, k)
        assert 0 < int(plain["counters"][0]) < N_PATHS, what
        table = _step(a, wm)
        summ = E.run_glide_host(p, SEED, STREAM, 0, N_PATHS, wm, table, want="summary")
        G.check_identities(E.run_glide_year_bins_host(p, SEED, STREAM, 0, N_PATHS, wm, table, edges=e, wr_edges=we), summ, N_PATHS, wm, what)
        G.check_identities(_device_bins(p, (SEED, STREAM, 0, N_PATHS), wm, table, e, we), summ, N_PATHS, wm, what + ", device entry")
