"""Bits of the Philox growth factors (growth_rows2 in csrc/mcr_device.h and the math of csrc/mcr_math.h), pinned by hashes.

The growth factors feed every output of every Philox variant, so a change to how they are computed that moves a single
bit shows here.  Each case hashes (SHA-256) the outputs of one launch family for fixed seeds: per-path summaries and
flags, trajectory slabs, counters and histogram bins of the path kernel in MODE 0 / 1 / 2, the time-sliced count-only
launch, the search probe window, the expense fan-out and grid probes, and launches whose path range crosses 2^32 inside a
wavefront (path_hi not the same in every lane: the generator's general form), through every launch form that draws the
factors: the plain and the producer / consumer (SPLIT) count-only launches, the time-sliced one, per-path outputs, and the
search, expense and grid probes.

    python tests/test_gpu_growth_bits.py --write tests/golden/growth_bits.json     (records the fixture with this build)
"""

from __future__ import annotations

import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)

from conftest import load_golden  # noqa: E402
from monte_carlo_retirement_amd import Config, params_from_config  # noqa: E402
from monte_carlo_retirement_amd import engine as E  # noqa: E402

SEED = 0x5DEECE66D
EDGES = np.geomspace(1.0, 1e13, 65)
STRADDLE = 2**32 - 37        # the first wavefront holds paths 2^32 - 37 .. 2^32 + 26


def _config(name):
    with open(os.path.join(os.path.dirname(HERE), "scenarios", name)) as fh:
        return json.load(fh)


def _digest(d) -> str:
    h = hashlib.sha256()
    for k in sorted(d):
        a = np.ascontiguousarray(np.asarray(d[k]))
        h.update(k.encode())
        h.update(str(a.dtype).encode())
        h.update(str(a.shape).encode())
        h.update(a.tobytes())
    return h.hexdigest()


def _batch(p, begin, n, wm, mode, seed=SEED, stream=1):
    r = E.run_batch_host(p, seed, stream, begin, n, wm, want_summary=mode >= 1, want_trajectories=mode >= 2,
                         hist_edges=EDGES)
    return {k: v for k, v in r.items() if isinstance(v, np.ndarray)}


def _cases():
    cfg = _config("config.json")
    p = params_from_config(Config(**cfg))
    inj = {g["name"]: g for g in load_golden("paths_injected.json")}
    jorge = inj["C3_jorge_wm75_rho03"]
    pj = params_from_config(Config(**jorge["cfg"]))
    return {
        "config_wm233_mode0": lambda: _batch(p, 0, 20_000, 233, 0),
        "config_wm233_mode1": lambda: _batch(p, 0, 20_000, 233, 1),
        "config_wm233_mode2": lambda: _batch(p, 0, 3_000, 233, 2),
        # 400 000 count-only paths: more path blocks than resident slots, so the launch is time-sliced (PHASE 3)
        "config_wm233_sliced_count": lambda: _batch(p, 0, 400_000, 233, 0),
        "jorge_rho03_mode2": lambda: _batch(pj, 11, 4_000, jorge["working_months"], 2),
        "probe_months_window": lambda: {"counts": E.probe_months(p, SEED, 0, 0, 50_000, list(range(225, 242))).cpu().numpy()},
        "probe_expenses": lambda: {"counts": E.probe_expenses(p, SEED, 0, 0, 20_000, 233,
                                                               [3000.0, 4000.0, 5000.0, 6000.0, 7000.0]).cpu().numpy()},
        "probe_grid": lambda: {"counts": E.probe_grid(p, SEED, 0, 0, 20_000, [200, 233],
                                                      [[4000.0, 6000.0], [4500.0, 6500.0]]).cpu().numpy()},
        "straddle_2p32_mode2": lambda: _batch(p, STRADDLE, 3_000, 233, 2),
        # 20 000 count-only paths: the producer / consumer (SPLIT) launch, whose producers run the general form too
        "straddle_2p32_split_count": lambda: _batch(p, STRADDLE, 20_000, 233, 0),
        # 300 000 count-only paths: above the SPLIT limit, below the resident slots (the plain whole-path launch)
        "straddle_2p32_plain_count": lambda: _batch(p, 2**32 - 150_001, 300_000, 233, 0),
        "straddle_2p32_probe_grid": lambda: {"counts": E.probe_grid(p, SEED, 0, STRADDLE, 20_000, [200, 233],
                                                                     [[4000.0, 6000.0], [4500.0, 6500.0]]).cpu().numpy()},
        "straddle_2p32_mode1": lambda: _batch(p, STRADDLE, 20_000, 233, 1),
        # sliced, with one wavefront in the middle of the range straddling 2^32
        "straddle_2p32_sliced_count": lambda: _batch(p, 2**32 - 200_003, 400_000, 233, 0),
        "straddle_2p32_probe_months": lambda: {"counts": E.probe_months(p, SEED, 0, STRADDLE, 20_000, [200, 233]).cpu().numpy()},
        "straddle_2p32_probe_expenses": lambda: {"counts": E.probe_expenses(p, SEED, 0, STRADDLE, 20_000, 233,
                                                                             [4000.0, 6000.0]).cpu().numpy()},
    }


def compute():
    return {name: _digest(run()) for name, run in _cases().items()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(_cases()))
def test_growth_bits(name):
    want = load_golden("growth_bits.json")[name]
    assert _digest(_cases()[name]()) == want, f"{name}: outputs differ from the recorded bits"


if __name__ == "__main__":
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--write", default=None)
    args = ap.parse_args()
    got = compute()
    print(json.dumps(got, indent=1, sort_keys=True))
    if args.write:
        with open(args.write, "w") as fh:
            json.dump(got, fh, indent=1, sort_keys=True)
            fh.write("\n")
