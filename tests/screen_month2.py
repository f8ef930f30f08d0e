"""The screening kernel's month after its SECOND restatement (csrc/mcr_screen.h, "the month as restated") in plain NumPy,
float32 throughout — a helper of tests/test_screen_month2_cpu.py, not a test.  It is tests/screen_restated.py (the first
restatement, which stays what it was) with exactly the arithmetic that changed:

    radius       a normal is sqrt(-log2 u) x trig, the constant sqrt(2 ln 2) folded into the growth slopes in double and rounded
                 once (screen_params); here a shock of the reference is divided by the constant and rounded to float32, which
                 is the kernel's normal to a rounding
    need level   the four net levels are clamped at zero where they are derived, and need = price x level has no maximum
    one compare  cap >= max(24 need, peak / 64); the two-compare form is evaluated beside it and `same_class` says, per path,
                 whether both gave the same answer in every month
    balances     the rebalance leaves b1 = alloc1 x T' and b2 = T' - b1, T' = (T - f bs) + net_purchase the total less the tax on
                 the realised share; the cost bases keep their selects

Returns what screen_restated.model returns, and `same_class`."""

from __future__ import annotations

import math
from typing import Dict

import numpy as np

import screen_model as M

LOG2E = 1.4426950408889634074
RADIUS = math.sqrt(2.0 * math.log(2.0))


def model(params, cfgd: dict, wm: int, seed: int, stream: int, begin: int, n: int) -> Dict[str, np.ndarray]:
    f = np.float32
    cast = lambda x: np.asarray(x, dtype=f)        # noqa: E731
    wm, n = int(wm), int(n)
    total_months = wm + int(params.retirement_years) * M.MONTHS_PER_YEAR
    z = M.shocks(params, wm, seed, stream, begin, n) / RADIUS
    sqrt12 = math.sqrt(M.MONTHS_PER_YEAR)
    a1, s1 = f(params.inv1_mu_log / M.MONTHS_PER_YEAR * LOG2E), f(params.inv1_sigma_log / sqrt12 * LOG2E * RADIUS)
    ai, si = f(params.inf_mu_log / M.MONTHS_PER_YEAR * LOG2E), f(params.inf_sigma_log / sqrt12 * LOG2E * RADIUS)
    ap, sp = f(params.prem_mu_log / M.MONTHS_PER_YEAR * LOG2E), f(params.prem_sigma_log / sqrt12 * LOG2E * RADIUS)
    alloc1 = f(params.allocation_inv1_pct)
    rate1 = M._effective_rate(params.inv1_use_realized_gains_tax_system, params.inv1_realized_gains_tax_rate)
    rate2 = M._effective_rate(params.inv2_use_realized_gains_tax_system, params.inv2_realized_gains_tax_rate)
    taxed = rate1 > 0.0 or rate2 > 0.0
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
    same_class = np.ones(n, dtype=bool)
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
                need = cast(price * f(max(0.0, net)))
                b1, b2, level = cast(b1 * g1), cast(b2 * g2), cast(level + x_inf)
                v1 = cast(b1 - cast(np.maximum(zero, cast(b1 - c1)) * rate1))
                v2 = cast(b2 - cast(np.maximum(zero, cast(b2 - c2)) * rate2))
                cap = cast(v1 + v2)
                one = cap >= cast(np.maximum(cast(margin * need), cast(peak / peak_div)))
                two = (cap >= cast(margin * need)) & (cap >= cast(peak / peak_div))
                same_class &= one == two
                safe &= one
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
            ncs = cast(cs - cast(cs * fraction))
            after = cast(cast(total - cast(fraction * bs)) + bought) if taxed else total
            c1, c2 = cast(np.where(sell1, ncs, cast(c1 + bought))), cast(np.where(sell1, cast(c2 + bought), ncs))
            b1 = cast(after * alloc1)
            b2 = cast(after - b1)
            peak = cast(np.maximum(peak, total))
            low = cast(np.fmin(low, np.fmin(b1, b2)))
        safe &= low > min_balance
        safe &= peak < f(M.MAX_TOTAL)
        final_total = cast(b1 + b2)
    safe &= np.isfinite(final_total)
    return {"safe": safe, "min_ratio": min_ratio, "final_total": final_total, "same_class": same_class}
