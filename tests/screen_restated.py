"""The screening kernel's month AS RESTATED (csrc/mcr_screen.h, "the month as restated") in plain NumPy, float32 throughout —
a helper of tests/test_screen_restated_cpu.py, not a test.  tests/screen_model.py is the reference and stays what it was: the
month as the fp64 state machine's closed form states it.  This file restates the same month the way the kernel now computes
it, so that the restatement can be held to the reference on the CPU before any kernel runs:

    need level   need = max(0, price x E), E the wave-uniform net level of the month's window state: expenses, less the netted
                 amount of each income record whose window holds the month, derived in double and rounded once
    price level  carried as its base-2 logarithm: L += x_inf each month, price = exp2(L) in retirement months only, and asset 2
                 grows by exp2(x_inf + x_prem); the growth coefficients are pre-scaled by log2(e) as screen_params does
    no clamps    the sold fraction is need / capacity and the rebalance sells drift / (bs - w G), neither clamped to 1
    balances     one running minimum of both balances over the path, compared with the dollar once at the end
    angle        `angle` = True moves every normal as a Box-Muller angle that is 2^-23 revolution short moves it: the cosine
                 member of a pair by + z_sin d, the sine member by - z_cos d, d = 2 pi 2^-23 (pairs: the half's normals
                 (0, 1), (2, 3), (4, 5), normal 3 r + k being shock k of the half's month r).  The oracle's inflation shock has
                 rho mixed in; the pairs are taken on the shocks as drawn, which bounds the effect rather than reproducing it.

Returns what screen_model.model returns, except `slack`."""

from __future__ import annotations

import math
from typing import Dict

import numpy as np

import screen_model as M

LOG2E = 1.4426950408889634074
ANGLE_STEP = 2.0 * math.pi * 2.0 ** -23


def _short_angle(z: np.ndarray) -> np.ndarray:
    """[n, months, 3] shocks with every Box-Muller pair turned back by ANGLE_STEP."""
    n, months, _ = z.shape
    pad = (-months) % 2
    flat = np.concatenate([z, np.zeros((n, pad, 3))], axis=1).reshape(n, -1, 3, 2)      # a half's six normals as three pairs
    cos, sin = flat[..., 0], flat[..., 1]
    out = np.stack([cos + sin * ANGLE_STEP, sin - cos * ANGLE_STEP], axis=-1)
    return out.reshape(n, months + pad, 3)[:, :months]


def model(params, cfgd: dict, wm: int, seed: int, stream: int, begin: int, n: int, angle: bool = False) -> Dict[str, np.ndarray]:
    f = np.float32
    cast = lambda x: np.asarray(x, dtype=f)        # noqa: E731
    wm, n = int(wm), int(n)
    total_months = wm + int(params.retirement_years) * M.MONTHS_PER_YEAR
    z = M.shocks(params, wm, seed, stream, begin, n)
    if angle:
        z = _short_angle(z)
    sqrt12 = math.sqrt(M.MONTHS_PER_YEAR)
    a1, s1 = f(params.inv1_mu_log / M.MONTHS_PER_YEAR * LOG2E), f(params.inv1_sigma_log / sqrt12 * LOG2E)
    ai, si = f(params.inf_mu_log / M.MONTHS_PER_YEAR * LOG2E), f(params.inf_sigma_log / sqrt12 * LOG2E)
    ap, sp = f(params.prem_mu_log / M.MONTHS_PER_YEAR * LOG2E), f(params.prem_sigma_log / sqrt12 * LOG2E)
    alloc1 = f(params.allocation_inv1_pct)
    rate1 = M._effective_rate(params.inv1_use_realized_gains_tax_system, params.inv1_realized_gains_tax_rate)
    rate2 = M._effective_rate(params.inv2_use_realized_gains_tax_system, params.inv2_realized_gains_tax_rate)
    w1, w2 = f(params.allocation_inv1_pct * rate1), f((1.0 - params.allocation_inv1_pct) * rate2)
    rate1, rate2 = f(rate1), f(rate2)
    windows = M.income_windows(params, cfgd, wm)
    grows = params.contribution_growth_rate_annual > 0
    growth = f(1.0 + params.contribution_growth_rate_annual)
    contrib = f(params.monthly_contribution)
    zero = f(0.0)
    margin, peak_div, min_balance = f(M.NEED_MARGIN), f(M.PEAK_DIV), f(M.MIN_BALANCE)

    first = params.initial_balance * params.allocation_inv1_pct
    b1 = np.full(n, f(first), dtype=f)
    b2 = np.full(n, f(params.initial_balance - first), dtype=f)
    c1, c2 = b1.copy(), b2.copy()
    level = np.zeros(n, dtype=f)
    peak = cast(b1 + b2)
    low = np.minimum(b1, b2)
    safe = np.ones(n, dtype=bool)
    min_ratio = np.full(n, np.inf, dtype=f)
    moy = 0

    with np.errstate(all="ignore"):
        for m in range(total_months):
            ze, zi, zp = cast(z[:, m, 0]), cast(z[:, m, 1]), cast(z[:, m, 2])
            g1 = cast(np.exp2(cast(a1 + cast(s1 * ze))))
            x_inf = cast(ai + cast(si * zi))
            g2 = cast(np.exp2(cast(x_inf + cast(ap + cast(sp * zp)))))
            if m < wm:
                if moy == M.MONTHS_PER_YEAR:
                    moy = 0
                    if grows:
                        contrib = f(contrib * growth)
                moy += 1
                k1 = f(contrib * alloc1)
                k2 = f(contrib - k1)
                b1, b2, level = cast(b1 * g1), cast(b2 * g2), cast(level + x_inf)
                b1, c1, b2, c2 = cast(b1 + k1), cast(c1 + k1), cast(b2 + k2), cast(c2 + k2)
            else:
                price = cast(np.exp2(level))
                net = float(params.monthly_expenses) - sum(a for a, start, end in windows if start <= m < end)
                need = cast(np.maximum(zero, cast(price * f(net))))
                b1, b2, level = cast(b1 * g1), cast(b2 * g2), cast(level + x_inf)
                v1 = cast(b1 - cast(np.maximum(zero, cast(b1 - c1)) * rate1))
                v2 = cast(b2 - cast(np.maximum(zero, cast(b2 - c2)) * rate2))
                cap = cast(v1 + v2)
                safe &= (cap >= cast(margin * need)) & (cap >= cast(peak / peak_div))
                ratio = cast(np.where(need > zero, cast(cap / need), np.inf))
                min_ratio = cast(np.fmin(min_ratio, ratio))
                keep = cast(f(1.0) - cast(need / cap))
                b1, c1, b2, c2 = cast(b1 * keep), cast(c1 * keep), cast(b2 * keep), cast(c2 * keep)
            total = cast(b1 + b2)
            drift1 = cast(b1 - cast(total * alloc1))
            sell1 = drift1 > zero
            bs, cs = cast(np.where(sell1, b1, b2)), cast(np.where(sell1, c1, c2))
            rate_s, w_s = cast(np.where(sell1, rate1, rate2)), cast(np.where(sell1, w1, w2))
            gain = cast(np.maximum(zero, cast(bs - cs)))
            fraction = cast(cast(np.abs(drift1)) / cast(bs - cast(w_s * gain)))
            bought = cast(fraction * cast(bs - cast(gain * rate_s)))
            left = cast(f(1.0) - fraction)
            nbs, ncs = cast(bs * left), cast(cs * left)
            b1, c1, b2, c2 = (cast(np.where(sell1, nbs, cast(b1 + bought))), cast(np.where(sell1, ncs, cast(c1 + bought))),
                              cast(np.where(sell1, cast(b2 + bought), nbs)), cast(np.where(sell1, cast(c2 + bought), ncs)))
            peak = cast(np.maximum(peak, total))
            low = cast(np.fmin(low, np.fmin(b1, b2)))
        safe &= low > min_balance
        safe &= peak < f(M.MAX_TOTAL)
        final_total = cast(b1 + b2)
    safe &= np.isfinite(final_total)
    return {"safe": safe, "min_ratio": min_ratio, "final_total": final_total}
