// mcr_screen.h — device-side building blocks of the SCREENING kernel (screen_kernel, mcr_hip.hip).
//
// A count-only launch returns integers: how many paths succeed, in which retirement year the others fail, how many years
// each was observed.  For almost every path the classification is never in doubt, so the launch first runs the whole path in
// fp32 on the hardware's transcendentals (v_log_f32, v_sqrt_f32, v_sin_f32 / v_cos_f32, v_exp_f32) and asks one question per
// retirement month: is the liquidation value still at least kScreenNeedMargin times the month's net need, and at least
// 1 / kScreenPeakDiv of the largest total the path has held?  A path that answers yes every month is SAFE: it succeeds with
// every year observed, and is counted here.  Every other path is DOUBTFUL: its index goes to a list, and the fp64 state
// machine (path_kernel's LIST form) alone decides its flags, ruin year and observed years.
//
// Soundness: the fp64 month fails a path only when capacity < need - 1e-6.  A SAFE path could be misclassified only if the fp32
// capacity were off by a factor of kScreenNeedMargin (a relative deviation of 0.95) where the expected deviation of the fp32
// path from the fp64 one is 1e-5 to 1e-4 (833 months of fp32 roundings and ~1e-6 absolute on each normal variate).
//
// The month as restated.  The kernel is bound to the fp64 month by a tolerance, not bit for bit, so the month is stated the way
// that costs the fewest VALU instructions: need = price x E, E one of the four wave-uniform net levels of ScreenParams, clamped
// at zero where they are derived (price > 0, so max(0, price x E) = price x max(0, E)) and chosen with scalar selects of their
// words (ScreenLevels, mcr_hip.hip); the price level is carried as its base-2 logarithm L (L += x_inf every month, price = exp2(L)
// in retirement months only); the yearly contribution step sits behind a scalar branch; the two capacity tests are one compare,
// cap >= max(24 need, peak / 64), the same predicate bit for bit; the Box-Muller radius is sqrt(-log2 u), its constant
// sqrt(2 ln 2) folded into the growth slopes in double; the rebalance states the balances in closed form (screen_rebalance:
// b1 = alloc1 T', b2 = T' - b1, T' = T - f bs + net_purchase, which moves them by fp32 roundings of the total a month, inside
// the tolerance); and the balance test is one running minimum rmin = min3(rmin, b1, b2), compared with kScreenMinBalance where
// the class is read: at the exit, and in the whole-wave vote every 16th row.  A lane is doubtful when rmin <= kScreenMinBalance
// exactly as when the test ran every month.  The rows run four to a loop iteration (screen_rows, mcr_hip.hip): both halves of
// a Philox block triple straight-line, the pair carry local to the iteration, one loop per Philox form.
//
// Two clamps of the fp64 month are dead here and are not restated.  (1) min(need, cap): a lane that is still ok has
// cap >= 24 need, so the minimum is `need`; a lane that is not ok stays doubtful whatever its state becomes (`ok` only ever
// falls, rmin only ever falls).  (2) min(1, fraction_sold) of the rebalance: with w the sold asset's allocation, rate <= 1 and
// 0 <= G <= bs, drift <= (1 - w) bs <= bs - w rate G, so the quotient f is at most 1 up to rounding, for every qualifying
// parameter block (allocations and rates in [0, 1]), and it comes near 1 only where w (bs - rate G) is near 0: the seller's
// allocation is 0, or rate = 1 with a cost basis of 0.  With closed-form balances a rounding of f above 1 no longer turns the
// seller's balance negative; what it does is bounded instead.  f = 1 + e (e a few 2^-24) leaves the seller's cost basis at
// cs' = -e cs, a rounding's worth of cs below zero, which enters later months only through G = max(0, b - c): a gain larger by
// e cs.  T' = T - f rate G is linear in f with no sign to lose: it moves by e rate G <= e T, a rounding of the total like any
// other.  And the two cases that bring f near 1 are doubtful on their own: with w = 0 the seller's new balance is w T' = 0,
// which rmin holds from then on; a cost basis of 0 needs a balance of 0 at the start or a sale of f = 1 exactly, the first case.
//
// Random numbers: the Philox words of growth_parts2_form (mcr_device.h), the same word-to-pair assignment and row order, so
// normal j of month k is the fp64 kernel's variate to fp32 accuracy.  No LDS tables, no stage.
#pragma once

#include "mcr_device.h"

namespace mcr {

constexpr float kScreenNeedMargin = 24.0f;       // SAFE needs capacity >= 24 x the month's net need ...
constexpr float kScreenPeakDiv = 64.0f;          // ... and capacity >= (running maximum of b1 + b2) / 64
constexpr float kScreenMinBalance = 1.0f;        // a balance at or below one dollar: doubtful (the fp64 month's dust fix-ups are not restated)
constexpr float kScreenMaxTotal = 1e30f;         // a total beyond this: doubtful (every fp32 intermediate of a SAFE path is finite)

// Wave-uniform parameter block of the screening kernel, derived on the host in double and rounded once (screen_params,
// mcr_hip.hip).  The growth coefficients are pre-scaled by log2(e), the slopes b also by sqrt(2 ln 2) (the Box-Muller radius
// constant, screen_factors2): a factor is exp2(fma(b', sqrt(-log2 u) t, a')).
struct ScreenParams {
    float a1, b1, ainf, binf_rho, binf_rho_c, aprem, bprem;
    float b1_0, b2_0;                  // initial balances (initial_balance alloc1, initial_balance - that)
    float contrib, contrib_growth_factor, alloc1;
    float rate1, rate2, ar1, ar2;      // realized-gains rates, and weight x rate (lane_params_tol)
    float e00, e10, e01, e11;          // net need LEVEL per window state of the (at most two) indexed income records: expenses, less
                                       // the first record's netted amount (e10), less the second's (e01), less both (e11); each >= 0
    int32_t s0, s1;                    // the records' first ROW (start + wm, saturated) ...
    uint32_t n0, n1;                   // ... and length in months (StreamRegs of path_kernel)
    int32_t working_months, retirement_years, total_months, contrib_grows;
};

// The launch constants that meet a second scalar operand in an FMA or a select (the three growth intercepts, the rebalance's
// weight x rate pair): held in VGPRs across the path, opaque to the compiler (screen_kernel), since a VALU instruction reads one
// SGPR and the compiler otherwise copies them into a VGPR again every month.
struct ScreenConsts { float a1, ainf, aprem, ar1, ar2; };

// The growth of the two months of a HALF (growth_parts2_form's halves, words and carry), in registers: per month the equity
// factor g1, the base-2 logarithm x_inf of the inflation factor and the inv2 factor exp2(x_inf + x_prem) (inflation x premium
// under one exponential).  UNIFORM: philox_path_rounds with the wave's path_hi (PhiloxPath::hi_uniform).  RHO0: the launch's
// rho is 0, binf_rho an exact zero, and its term is left out.
template <int HALF, bool UNIFORM, bool RHO0>
__device__ __forceinline__ void screen_factors2(const ScreenParams& S, const ScreenConsts& K, const PhiloxPath& Q, uint64_t seed, uint32_t t, PairCarry& C, float (&g)[6]) {
    float rad[3], trig[6];
    auto parts = [&](uint32_t xr, uint32_t xa, int i) {
        // u = (w + 0.5) 2^-32 in (0, 1]; radius = sqrt(-2 ln u) = sqrt(2 ln 2) sqrt(-log2 u), the constant folded into the slopes
        // (screen_params), the negation a source modifier of v_sqrt_f32; angle in revolutions
        const float u = __builtin_fmaf((float)xr, 0x1p-32f, 0x1p-33f);
        rad[i] = __builtin_amdgcn_sqrtf(-__builtin_amdgcn_logf(u));
        const float rev = (float)xa * 0x1p-32f;
        trig[2 * i] = __builtin_amdgcn_cosf(rev);
        trig[2 * i + 1] = __builtin_amdgcn_sinf(rev);
    };
    uint32_t x[4];
    if (HALF == 0) {
        philox_path_rounds<UNIFORM>(Q, 3u * t, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        parts(x[0], x[1], 0);
        parts(x[2], x[3], 1);
        philox_path_rounds<UNIFORM>(Q, 3u * t + 1u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        parts(x[0], x[1], 2);
        C.w2 = x[2]; C.w3 = x[3];
    } else {
        parts(C.w2, C.w3, 0);
        philox_path_rounds<UNIFORM>(Q, 3u * t + 2u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        parts(x[0], x[1], 1);
        parts(x[2], x[3], 2);
    }
#pragma unroll
    for (int r = 0; r < 2; ++r) {      // growth_factors_row on normals 3 r, 3 r + 1, 3 r + 2 of the half
        const int je = 3 * r, ji = 3 * r + 1, jp = 3 * r + 2;
        const float ne = rad[je >> 1] * trig[je], ni = rad[ji >> 1] * trig[ji], np = rad[jp >> 1] * trig[jp];
        const float g1 = __builtin_amdgcn_exp2f(__builtin_fmaf(S.b1, ne, K.a1));
        float xinf = __builtin_fmaf(S.binf_rho_c, ni, K.ainf);
        if (!RHO0) xinf = __builtin_fmaf(S.binf_rho, ne, xinf);
        const float xprem = __builtin_fmaf(S.bprem, np, K.aprem);
        g[3 * r + 0] = g1; g[3 * r + 1] = xinf; g[3 * r + 2] = __builtin_amdgcn_exp2f(xinf + xprem);
    }
}

// rebalance_tol (mcr_device.h) in fp32: selects stay selects, no guard and no dust fix-ups (a lane whose balance falls to
// kScreenMinBalance is doubtful; with both balances above it every denominator is positive).  Returns b1 + b2 before the trade.
template <int TAXED, bool EQR>
__device__ __forceinline__ float screen_rebalance(const ScreenParams& S, const ScreenConsts& K, float& b1, float& c1, float& b2, float& c2) {
    const float total = b1 + b2;
    const float drift1 = __builtin_fmaf(-total, S.alloc1, b1);
    const bool sell1 = drift1 > 0.0f;
    const float bs = sell1 ? b1 : b2, cs = sell1 ? c1 : c2;
    const float drift = __builtin_fabsf(drift1);
    float fraction_sold, net_purchase;
    if (TAXED != 0) {
        const float rate_s = EQR ? S.rate1 : sell1 ? S.rate1 : S.rate2;
        const float ar_s = sell1 ? K.ar1 : K.ar2;
        const float G = __builtin_fmaxf(0.0f, bs - cs);
        fraction_sold = drift * __builtin_amdgcn_rcpf(__builtin_fmaf(-ar_s, G, bs));
        net_purchase = fraction_sold * __builtin_fmaf(-G, rate_s, bs);
    } else {
        fraction_sold = drift * __builtin_amdgcn_rcpf(bs);
        net_purchase = fraction_sold * bs;
    }
    const float ncs = __builtin_fmaf(-cs, fraction_sold, cs);
    const float r1c = c1 + net_purchase, r2c = c2 + net_purchase;
    c1 = sell1 ? ncs : r1c; c2 = sell1 ? r2c : ncs;
    // the balances in closed form: the trade leaves b1 = alloc1 T' and b2 = T' - b1 whoever sells, T' the total less the tax on
    // the realised share (untaxed: the total itself)
    const float after = TAXED != 0 ? __builtin_fmaf(-fraction_sold, bs, total) + net_purchase : total;
    b1 = after * S.alloc1; b2 = after - b1;
    return total;
}

}  // namespace mcr
