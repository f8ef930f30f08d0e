"""The output modes of the DEFAULT stream (Philox: path_kernel<MODE, 0, ...>) against the CPU oracle, value for value, on the
stratified random plans of tests/count_fuzz.py.

The Philox summary-only (MODE 1), full-output (MODE 2) and yearly-bins (MODE 3) kernels are instantiations of their own, with
launch bounds of their own (five workgroups a SIMD where the NumPy and history kernels have four), and they are what `bench.py`
times and every caller runs.  tests/test_gpu_count_routes_vs_oracle.py holds them to the oracle on their integers; the
comparisons that look at every per-path value and every table cell (`same_full_output`, `same_summary`, `same_year_bins` of
tests/test_gpu_numpy_stream_vs_oracle.py) were applied to the NumPy stream and the history schemes only.  Here they are applied
to the Philox launches of every plan: 512 and 321 paths (a ragged last wavefront and workgroup), path ranges from 0, from
2^32 - 100 (a wave that straddles 2^32) and from 2^40, 0 to 199 working months, 4 to 40 retirement years, every tax mask, the
annual-gains kernels, 17 to 20 paying streams and the exact month.  The scenario and assumption outcome and joint probes are
compared elsewhere with these launches, so an error in a Philox summary column that leaves the flags alone would pass there.

No tolerance is new: ``ABS + REL x max(|ref|, the path's money scale)`` and ``rtol=1e-8, atol=1e-9`` for withdrawal rates are
tests/test_gpu_differential.py's, and the yearly tables go through the rule of tests/bin_rule.py, under which the oracle's rows
of these plans have no entry near an edge (tests/test_bin_rule_cpu.py): the tables are compared cell for cell.

Printed per class: the worst error of MODE 1 and MODE 2 against the oracle, relative to max(|ref|, the path's money scale).
Measured on an MI355X with the suite's seed (LABNOTES R37): 6.8e-13 (annual) to 7.2e-12 (generic), against the bound's 1e-9."""

from __future__ import annotations

import numpy as np
import pytest

import count_fuzz as F
from monte_carlo_retirement_amd import engine as E
from test_gpu_count_routes_vs_oracle import _env
from test_gpu_numpy_stream_vs_oracle import SUMMARY, same_full_output, same_summary, same_year_bins

pytestmark = pytest.mark.gpu


def _ctx(scn, route):
    return scn.context(f"{route}; Philox stream")


def _worst_scaled(got, ora, keys) -> float:
    """max |got - ref| / max(|ref|, the path's money scale) over `keys` (what the path tolerance bounds by REL, ABS aside)."""
    scale = np.maximum(1.0, np.abs(ora["trajectory"]).max(axis=0))
    worst = 0.0
    for key in keys:
        if got[key].shape == ora[key].shape:
            err = np.abs(got[key] - ora[key]) / np.maximum(np.abs(ora[key]), scale)
            worst = max(worst, float(np.max(err)) if err.size else 0.0)
    return worst


@pytest.mark.parametrize("cls", F.CLASSES)
def test_philox_output_modes_equal_the_oracle(oracle, cls):
    """Summary-only (MODE 1), full output (MODE 2) and yearly bins (MODE 3: the host entry, and the device entry through
    YearBinsBatch) of every plan of the class."""
    plans = F.scenarios(oracle, cls)
    F.oracle_runs(oracle, [((scn,), dict(trajectories=True)) for scn in plans])       # (on host threads; cached and shared)
    worst = {"MODE 1": 0.0, "MODE 2": 0.0}
    try:
        for scn in plans:
            ora = F.oracle_run(oracle, scn, trajectories=True)
            assert F.money_scale(ora) < F.SCALE_LIMIT, _ctx(scn, "money scale")
            p, at = scn.params(), (scn.seed, scn.stream, scn.begin, scn.n)
            with _env({}):
                full = E.run_batch_host(p, *at, scn.wm)
                summary = E.run_batch_host(p, *at, scn.wm, want_trajectories=False)
                bins = E.run_year_bins_host(p, *at, scn.wm)
                batch = E.YearBinsBatch(p, scn.wm)
                batch.launch(*at)
                device_bins = batch.host()
            worst["MODE 2"] = max(worst["MODE 2"], _worst_scaled(full, ora, ("trajectory", "real_trajectory") + SUMMARY))
            worst["MODE 1"] = max(worst["MODE 1"], _worst_scaled(summary, ora, SUMMARY))
            assert "trajectory" not in summary or summary["trajectory"].size == 0, _ctx(scn, "summary-only: a trajectory came back")
            same_full_output(scn, full, ora, "full output (MODE 2)", ctx=_ctx)
            same_summary(scn, summary, ora, "summary-only (MODE 1)", ctx=_ctx)
            same_year_bins(scn, bins, ora, "year bins (MODE 3, host buffers)", ctx=_ctx)
            same_year_bins(scn, device_bins, ora, "year bins (MODE 3, YearBinsBatch)", ctx=_ctx)
    finally:
        print(f"{cls}: worst error against the oracle relative to max(|ref|, the path's money scale): "
              f"MODE 1 {worst['MODE 1']:.3e}, MODE 2 {worst['MODE 2']:.3e} ({len(plans)} plans)")
