// mcr_device.h — device-side building blocks of the Monte Carlo retirement path kernel (gfx950).
//
// One simulated path lives in ONE LANE: the monthly state (two balances, two cost bases, two
// gain accumulators, the price level, the contribution) stays in VGPRs for the whole horizon;
// scenario parameters are wave-uniform kernel arguments (SGPRs).  All arithmetic is IEEE fp64
// and the translation unit is compiled with -ffp-contract=off: the STATE MACHINE's a*b+c rounds
// twice, as in the reference (CPython floats); FMAs appear only where they are spelled out
// (__builtin_fma / inline v_fma_f64): inside exp / log / sincos, the Newton steps of the
// divisions, and the log-returns a + b z of monthly_gross / growth_rows2 (one rounding there
// instead of the reference's two, 1e-16 |x| on the argument of exp: part of the 1e-9 budget).
// Each function cites the reference lines it replaces (rflamino/monte_carlo_retirement,
// backend/simulation.py).
//
// Data-dependent branches of the reference (sell inv1 / sell inv2, early-outs) are written
// branch-free with selected operands: the lanes of a wavefront diverge on them almost every
// month, so both sides would otherwise be executed under exec masks.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/mcr.h"
#include "mcr_math.h"

// `if (c) { MCR_MASKED_MOVE; x = y; }`: the empty asm keeps the assignment a BRANCH under the exec mask (v_cmp, s_and_saveexec,
// moves, s_or) where the compiler would if-convert it into v_cndmask pairs — a 64-bit select costs two fp64 issue slots, the
// masked move one and often none (LABNOTES.md, rounds 1-3 section 5).  MM (a template parameter in scope at every use) = false leaves the
// choice to the compiler: the producer / consumer SPLIT launches are bound by each wave's dependency chain, not by issue
// slots, and there the compare -> scalar mask -> branch -> move round trip is the slower form (lone 50 000-path probe
// 0.84 -> 0.79 ms, measured).  Same values either way.
#define MCR_MASKED_MOVE do { if (MM) asm volatile(""); } while (0)
namespace mcr {

constexpr double kEps = MCR_SMALL_EPSILON;
constexpr int kMPY = MCR_MONTHS_PER_YEAR;
constexpr int kBlock = 256;  // threads per workgroup = 4 wavefronts, one per SIMD (128 measured: no better)

// Per-stream data prepared on the host (mcr_abi: derive_params) from mcr_stream.
struct DevStream {
    double amount;        // monthly_amount_today
    double keep;          // 1.0 - tax_rate                      (simulation.py:675-677)
    double amount_keep;   // amount * keep: the tolerance form of the month nets the amount first ((a k) price instead of (a price) k)
    int32_t start_month;  // stream_payment_start_month_index    (:47-63, :603-608)
    int32_t end_month;    // start + duration_years*12, INT32_MAX for None (:609-613, :653-656)
    int32_t indexed;      // inflation_indexed
    int32_t lock_slot;    // column of the frozen nominal amount (non-indexed streams), else -1: slots below
                          // DevParams::n_lock_slots are LDS columns, the others rows of DevParams::lock_overflow
};
// Records past the by-value block live in a device table that the kernel reads through the CONSTANT address space:
// scalar loads (s_load_dwordx8, the record lands in SGPRs like a kernel argument) whatever the alias analysis makes of the
// kernel's own stores.
typedef const __attribute__((address_space(4))) DevStream* DevStreamTable;

// Wave-uniform scenario block (kernel argument -> SGPRs).
struct DevParams {
    double initial_balance, monthly_contribution, contrib_growth_factor /* 1 + g */, monthly_expenses;
    double alloc1, alloc2;             // allocation_inv1_pct, 1.0 - allocation_inv1_pct (config.py:124-126)
    double real_rate1, real_rate2;     // realized-gains rate if the asset uses that system, else 0.0
    double annual_rate1, annual_rate2; // annual-gains rate if the asset does NOT use the realized system, else 0.0
    double a1, b1;                     // inv1:      mu_log/12, sigma_log/sqrt(12)   (:473)
    double ainf, binf;                 // inflation: idem
    double aprem, bprem;               // inv2 premium over inflation: idem
    double rho, rho_c;                 // rho, sqrt(max(0, 1 - rho^2))               (:460-464)
    double binf_rho, binf_rho_c;       // binf * rho, binf * rho_c: the inflation log-return straight from two normals (growth_rows2)
    int32_t working_months, retirement_years, total_months, shock_rows;
    int32_t num_working_years, trajectory_len;
    int32_t n_streams;                 // records in `streams` below: min(len(other_income_streams), MCR_INLINE_STREAMS)
    int32_t n_lock_slots;              // lock slots kept in LDS ([n_lock_slots][kBlock] doubles); the launcher decides (LDS budget)
    int32_t contrib_grows;             // contribution_growth_rate_annual > 0        (:516)
    int32_t any_annual_tax;            // annual_rate1 > 0 || annual_rate2 > 0
    int32_t any_real_rate;             // real_rate1 > 0 || real_rate2 > 0
    int32_t tax_mask;                  // bit 0: real_rate1 > 0, bit 1: real_rate2 > 0  -> selects the TAXED kernel variant (0 .. 3)
    int32_t exact_month;               // a realized-gains rate above 1 - 1e-6: the reference's denominator clamps can bind -> exact forms, generic variants
    int32_t reserved_;
    DevStream streams[MCR_INLINE_STREAMS];
    // other_income_streams beyond the by-value block (the list has any length, config.py:99)
    int32_t n_extra_streams;           // records in `extra_streams`
    int32_t n_lock_slots_total;        // non-indexed streams of the whole list (derive_params numbers their slots in list order)
    const DevStream* extra_streams;    // DEVICE table [n_extra_streams] (read through DevStreamTable), nullptr if none
    double* lock_overflow;             // DEVICE [n_lock_slots_total - n_lock_slots][lock_stride]: the slots that did not fit in LDS
    int64_t lock_stride;               // = grid.x * kBlock: every lane of the launch has its own column
    double fast_floor;                 // 1e-6 / (1 - max(real_rate1, real_rate2)) (>= 1e-6): both balances above it -> capacity > 1e-6
};

// The four parameters that feed per-lane SELECTS (seller's weight / seller's rate).  They are
// wave-uniform, but a select between two SGPR pairs costs two v_mov per dword (one constant-bus
// operand per VALU instruction) and the kernel is already SGPR-bound (57 spills): the path kernel keeps
// a VGPR-resident copy.
struct LaneParams {
    double alloc1, alloc2, real_rate1, real_rate2;
};
__device__ __forceinline__ LaneParams lane_params(const DevParams& P) {
    LaneParams L{P.alloc1, P.alloc2, P.real_rate1, P.real_rate2};
    asm volatile("" : "+v"(L.alloc1), "+v"(L.alloc2), "+v"(L.real_rate1), "+v"(L.real_rate2));
    return L;
}
// PHASE 12 (the allocation fan-out, mcr_hip.hip): what the tolerance month's helpers read of the parameter block (rebalance_tol:
// the weight; annual_gain_taxes: the annual-gains bill), with the CONSUMER WAVE's own weight in place of the block's.  Wave-uniform
// like the block: scalar registers.  alloc2 = 1.0 - alloc1 is derive_params' operation on the block, made by the wave.
struct WaveAllocParams {
    double alloc1, alloc2;
    double annual_rate1, annual_rate2;
    int32_t any_annual_tax;
};
struct NoWaveAlloc { static constexpr double alloc1 = 0.0; };   // (named, never read: `kAlcFan ? WA.alloc1 : P.alloc1` folds to the block's)
// PHASE 13 (the glide fan-out): the same view, whose weight the wave reloads at every calendar-year change from its own table
// W[0 .. n - 1] (include/mcr.h: GLIDE PATH).  `w` stands at the entry in force, `left` counts the entries behind it, `moy` the
// rows of the calendar year that are done: three scalars.  The helpers above and below take it as its base.  The table is read
// through the CONSTANT address space like DevStreamTable: nothing writes it while the kernel runs, and the year's reload is a
// scalar load (s_load_dwordx2) whatever the alias analysis makes of the kernel's own stores (through a plain pointer the
// decumulation's reload came out as a vector load of a uniform address).
typedef const __attribute__((address_space(4))) double* GlideTable;
struct WaveGlideParams : WaveAllocParams {
    GlideTable w;
    int32_t left;
    int32_t moy;
};
// The tolerance form of the month (below) selects the seller's rate and the seller's weight x rate; it needs neither weight
// on its own (the drift of asset 2 is minus the drift of asset 1).  In the SAME struct, so that the helpers keep one
// signature: alloc1 / alloc2 then hold the products.
// EQR (the month form kMonthEqualRates, below): the two rates are one value — one VGPR pair holds it for both assets.
template <bool EQR = false>
__device__ __forceinline__ LaneParams lane_params_tol(const DevParams& P) {
    LaneParams L{P.alloc1 * P.real_rate1, P.alloc2 * P.real_rate2, P.real_rate1, P.real_rate2};
    if (EQR) {
        asm volatile("" : "+v"(L.alloc1), "+v"(L.alloc2), "+v"(L.real_rate1));
        L.real_rate2 = L.real_rate1;
    } else {
        asm volatile("" : "+v"(L.alloc1), "+v"(L.alloc2), "+v"(L.real_rate1), "+v"(L.real_rate2));
    }
    return L;
}
// ... of a PHASE 12 consumer wave: the same two products, of the wave's weights (the single fp64 multiplies the plain launch
// applies to its block; the fan-outs run the tolerance month and none of the month forms)
__device__ __forceinline__ LaneParams lane_params_tol(const WaveAllocParams& W, const DevParams& P) {
    LaneParams L{W.alloc1 * P.real_rate1, W.alloc2 * P.real_rate2, P.real_rate1, P.real_rate2};
    asm volatile("" : "+v"(L.alloc1), "+v"(L.alloc2), "+v"(L.real_rate1), "+v"(L.real_rate2));
    return L;
}
// the path kernel's resident copy: the block's in the launch's month form, or the consumer wave's
template <bool TOL, bool EQR>
__device__ __forceinline__ LaneParams month_lane_params(const NoWaveAlloc&, const DevParams& P) { return TOL ? lane_params_tol<EQR>(P) : lane_params(P); }
template <bool TOL, bool EQR>
__device__ __forceinline__ LaneParams month_lane_params(const WaveAllocParams& W, const DevParams& P) {
    if (TOL) return lane_params_tol(W, P);
    LaneParams L{W.alloc1, W.alloc2, P.real_rate1, P.real_rate2};    // (lane_params': the exact month's diagnostic build)
    asm volatile("" : "+v"(L.alloc1), "+v"(L.alloc2), "+v"(L.real_rate1), "+v"(L.real_rate2));
    return L;
}
// PHASE 13, at the top of every row t = 0, 1, ... of the consumer's path (wave-uniform): behind it W.alloc1 = W[min(t / 12, n - 1)]
// (include/mcr.h: GLIDE PATH).  The weight changes where t % 12 == 0, t > 0, and only while the table has an entry left: one
// scalar load, derive_params' subtraction, the lanes' products again.
template <bool TOL, bool EQR>
__device__ __forceinline__ void glide_row(WaveGlideParams& W, const DevParams& P, LaneParams& L) {
    if (W.moy == kMPY) {
        W.moy = 0;
        if (W.left > 0) {
            --W.left;
            ++W.w;
            W.alloc1 = *W.w;
            W.alloc2 = 1.0 - W.alloc1;
            L = month_lane_params<TOL, EQR>(W, P);
        }
    }
    ++W.moy;
}

// ---------------------------------------------------------------------------------------------
// RNG: Philox4x32-10 (Salmon et al. SC'11, Random123 constants).  Counter = (path_lo, path_hi,
// month, stream_id), key = (seed_lo, seed_hi).  The key schedule is wave-uniform (scalar ALU).
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3,
                                              uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    // The key is wave-uniform.  Left alone, the compiler hoists all ten round keys out of the month loop and then
    // spills them (18 SGPRs -> v_readlane + s_nop per use); behind this barrier it bumps the key with two scalar adds
    // per round instead, which are free next to the VALU work.
    asm volatile("" : "+s"(k0), "+s"(k1));
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        // hi ^ counter ^ key as ONE v_bitop3_b32 (truth table 0x96 = three-way xor; gfx950) once all three operands are
        // per-lane values — in the first rounds parts are still wave-uniform and fold into scalar xors
        const uint32_t n0 = r >= 2 ? __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96) : (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = r >= 1 ? __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96) : (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// MCR_RNG_HISTORY (include/mcr.h): a lane's place in the recorded market.  Shock row r = k B + j of a path reads row
// (s_k + j) mod H of the record, s_k = hi32(x_k H) with x_k = word k & 3 of Philox block k >> 2 of the path.  Rows come in
// order, so the cursor steps: the row of the record goes up by one and wraps, and every B-th month a new start is taken
// (every 4 B-th a new Philox block).  r, j and k are wave-uniform (the month index is): scalar registers and scalar
// branches; per lane the cursor is the row and the block's four words.  Any other row (the first one, or a caller that
// skips) is reached from its definition, by division.  The other two schemes of the header use the same cursor: the stationary
// bootstrap its row and the words of Philox block r >> 1, the cohort replay its row alone.
struct HistoryCursor {
    uint32_t w[4];   // Philox block k >> 2 of the path (stationary: block r >> 1)
    uint32_t cur;    // the row of the record at shock row r
    int r;           // the shock row the cursor stands at (-2: none yet)
    uint32_t j, k;   // r = k B + j, j < B
};
__device__ __forceinline__ HistoryCursor history_cursor() { return HistoryCursor{{0u, 0u, 0u, 0u}, 0u, -2, 0u, 0u}; }
__device__ __forceinline__ uint32_t history_block_start(const HistoryCursor& C, uint32_t H) {
    const uint32_t q = C.k & 3u;
    const uint32_t x = q == 0u ? C.w[0] : q == 1u ? C.w[1] : q == 2u ? C.w[2] : C.w[3];
    return __umulhi(x, H);     // ((uint64_t)x * H) >> 32 < H
}
// MCR_HISTORY_STATIONARY: row rr, the cursor standing at row rr - 1 (or anywhere, for rr = 0).  Every even row a new Philox
// block (wave-uniform timing); per lane a compare and a select, no branch: umulhi(u, B) == 0 restarts at umulhi(v, H).
__device__ __forceinline__ void history_step_stationary(HistoryCursor& C, int rr, uint32_t H, uint32_t B, uint64_t seed, uint32_t stream_id, uint64_t path) {
    uint32_t u = C.w[2], v = C.w[3];      // an odd row: the second half of the block its predecessor made
    if ((rr & 1) == 0) {
        uint32_t w[4];
        philox4x32_10((uint32_t)path, (uint32_t)(path >> 32), (uint32_t)rr >> 1, stream_id, (uint32_t)seed, (uint32_t)(seed >> 32), w);
        u = w[0]; v = w[1]; C.w[2] = w[2]; C.w[3] = w[3];
    }
    const uint32_t next = C.cur + 1u == H ? 0u : C.cur + 1u;
    C.cur = (rr == 0 || __umulhi(u, B) == 0u) ? __umulhi(v, H) : next;
}
// SCHEMES = false: the block rule alone, the code it always was (the kernels of MCR_HISTORY_BLOCK launches keep their
// instructions and registers).  SCHEMES = true: the other two rules; `scheme` (include/mcr.h: MCR_HISTORY_STATIONARY or
// MCR_HISTORY_COHORTS) is launch-constant, a scalar branch.
template <bool SCHEMES = false>
__device__ __forceinline__ void history_seek(HistoryCursor& C, int r, uint32_t H, uint32_t B, uint32_t scheme, uint64_t seed, uint32_t stream_id, uint64_t path) {
    if (r == C.r) return;      // (the reference's clamp repeats the last row)
    if constexpr (SCHEMES) {
        if (scheme == MCR_HISTORY_STATIONARY) {
            if (r != C.r + 1)      // (no launch does this: whole-path launches start at row 0) walk from row 0, which restarts
                for (int rr = 0; rr < r; ++rr) history_step_stationary(C, rr, H, B, seed, stream_id, path);
            history_step_stationary(C, r, H, B, seed, stream_id, path);
        } else if (r == C.r + 1 && C.r >= 0) {      // MCR_HISTORY_COHORTS: the record run forward
            if (++C.cur == H) C.cur = 0u;
        } else {               // once per path: path mod H in 32-bit pieces, 2^32 mod H = (2^32 - 1) mod H + 1 (or H itself: the same class)
            const uint32_t t = 0xFFFFFFFFu % H + 1u;
            C.cur = (((uint32_t)(path >> 32) % H) * t + (uint32_t)path % H + (uint32_t)r % H) % H;      // < 2^23: H <= MCR_MAX_HISTORY_MONTHS
        }
    } else if (r == C.r + 1) {
        if (++C.j == B) {
            C.j = 0u;
            if ((++C.k & 3u) == 0u)
                philox4x32_10((uint32_t)path, (uint32_t)(path >> 32), C.k >> 2, stream_id, (uint32_t)seed, (uint32_t)(seed >> 32), C.w);
            C.cur = history_block_start(C, H);
        } else if (++C.cur == H) {
            C.cur = 0u;
        }
    } else {
        C.k = (uint32_t)r / B;
        C.j = (uint32_t)r % B;
        philox4x32_10((uint32_t)path, (uint32_t)(path >> 32), C.k >> 2, stream_id, (uint32_t)seed, (uint32_t)(seed >> 32), C.w);
        const uint32_t t = history_block_start(C, H) + C.j % H;      // both terms < H <= MCR_MAX_HISTORY_MONTHS
        C.cur = t >= H ? t - H : t;
    }
    C.r = r;
}

// The same generator for the path kernel's blocks, counter = (path_lo, path_hi, block, stream_id) with the parts of rounds
// 0 and 1 that do not depend on the block computed once per path (philox_path, at a point where the whole wave is
// active): round 0's M0 path_lo, and round 1's M1 c2 — c2 = hi(M0 path_lo) ^ stream_id ^ key_hi is block-free.  path_hi is
// the same in every lane unless the wave straddles a 2^32 path boundary; one ballot per path decides, and then round 0's
// c0 and round 1's M0 c0 are scalar work.  Same words as philox4x32_10 for every counter and key.
struct PhiloxPath {
    uint64_t hi_mask;      // lanes whose path_hi is not hi_s (wave-uniform; 0 on all but a wave that straddles 2^32)
    uint32_t hi_s, hi_o;   // path_hi of the wave's first active lane, and of the others (the paths of a wave span < 2^32)
    uint32_t lo0;          // lo(M0 path_lo): word 3 after round 0
    uint32_t b_lo, b_hi;   // M1 (hi(M0 path_lo) ^ stream_id ^ key_hi): round 1's second product
    bool hi_uniform;       // hi_mask == 0 (readfirstlane: a scalar branch, not an exec-masked one)
};
__device__ __forceinline__ PhiloxPath philox_path(uint64_t path, uint32_t stream_id, uint64_t seed) {
    PhiloxPath Q;
    const uint32_t hi = (uint32_t)(path >> 32);
    Q.hi_s = (uint32_t)__builtin_amdgcn_readfirstlane((int)hi);
    Q.hi_mask = __builtin_amdgcn_ballot_w64(hi != Q.hi_s);
    Q.hi_uniform = __builtin_amdgcn_readfirstlane((int)(Q.hi_mask == 0ull)) != 0;
    Q.hi_o = Q.hi_mask ? (uint32_t)__builtin_amdgcn_readlane((int)hi, (int)__builtin_ctzll(Q.hi_mask)) : Q.hi_s;
    const uint64_t p0 = (uint64_t)0xD2511F53u * (uint32_t)path;
    Q.lo0 = (uint32_t)p0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * ((uint32_t)(p0 >> 32) ^ stream_id ^ (uint32_t)(seed >> 32));
    Q.b_lo = (uint32_t)p1;
    Q.b_hi = (uint32_t)(p1 >> 32);
    return Q;
}
template <bool HI_UNIFORM>
__device__ __forceinline__ void philox_path_rounds(const PhiloxPath& Q, uint32_t block, uint32_t k0, uint32_t k1, uint32_t (&out)[4]) {
    asm volatile("" : "+s"(k0), "+s"(k1));          // (the key barrier of philox4x32_10)
    // round 0 (key k): c0 = hi(M1 block) ^ path_hi ^ k0; c1 = lo(M1 block); c2, c3 from Q
    const uint64_t q1 = (uint64_t)0xCD9E8D57u * block;
    // path_hi: rebuilt from the wave's mask on the rare straddling wave (no VGPR held for it through the path)
    const uint32_t ph = HI_UNIFORM ? Q.hi_s : (((Q.hi_mask >> __lane_id()) & 1ull) ? Q.hi_o : Q.hi_s);
    const uint32_t n0 = (uint32_t)(q1 >> 32) ^ ph ^ k0;
    // round 1 (key k + W): the products M0 n0 (scalar when path_hi is) and Q.b
    const uint64_t r0 = (uint64_t)0xD2511F53u * n0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
    uint32_t c0 = Q.b_hi ^ ((uint32_t)q1 ^ k0);
    uint32_t c1 = Q.b_lo;
    uint32_t c2 = (uint32_t)(r0 >> 32) ^ Q.lo0 ^ k1;
    uint32_t c3 = (uint32_t)r0;
#pragma unroll
    for (int r = 2; r < 10; ++r) {
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0r = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96);
        // round 2's c3 is still wave-uniform when path_hi is: one xor with a scalar
        const uint32_t n2r = (HI_UNIFORM && r == 2) ? (uint32_t)(p0 >> 32) ^ (c3 ^ k1)
                                                     : __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96);
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0r;
        c2 = n2r;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// The path's standard-normal sequence n[0], n[1], ... : pair j = Box-Muller of Philox words
// (2(j&1), 2(j&1)+1) of block j>>1 (counter = (path_lo, path_hi, block, stream_id)):
//   n[2j] = sqrt(-2 ln u_r) cos(2 pi u_a), n[2j+1] = ... sin(...),  u = (x + 0.5) 2^-32.
// Shock row k = (n[3k], rho n[3k] + rho_c n[3k+1], n[3k+2])  (replaces _draw_shock_path, :452-466),
// a pure function of (seed, stream, path, k): common random numbers across working-month candidates
// and across any sharding.  Rows are consumed in order, so a lane carries the half-used pair / block:
// 4 rows cost 3 Philox blocks and 6 (log, sqrt, sincos) pairs instead of 4 and 8.
__device__ __forceinline__ void bm_pair(uint32_t xr, uint32_t xa, const double* tab, const MathRegs& R, double& zc, double& zs) {
    const double r = fsqrt(neg2_log_u32(xr, tab, R));  // radius and angle straight from the Philox integers
    double s, c;
    sincos_u32<true>(xa, tab, R, s, c);
    zc = r * c;
    zs = r * s;
}

// The same pair as its PARTS: radius r and the angle's (cos, sin), the two normals being r cos and r sin.  growth_rows2
// folds the products into the log-returns instead of forming the normals first.
template <bool BYTE_OFFSET = false>
__device__ __forceinline__ void bm_parts(uint32_t xr, uint32_t xa, const double* tab, const MathRegs& R, double& r, double& c, double& s) {
    r = fsqrt(neg2_log_u32<true, BYTE_OFFSET>(xr, tab, R));      // path forms of the series (mcr_math.h)
    sincos_u32<true, true>(xa, tab, R, s, c);
}

struct ShockGen {      // per-lane carry between consecutive rows
    double carry_z;    // second normal of a pair whose first was used by the previous row
    uint32_t cw0, cw1; // words 2,3 of the last Philox block (the next pair)
};

// Row `k` for k % 4 == PHASE, given that rows 0..k-1 of this path were generated by this ShockGen in order.
// PHASE is a template parameter: which words feed which pair, whether a Philox block is drawn and what is carried
// are then fixed at compile time — no per-row selects or carry shuffles between the four cases (the caller
// dispatches on the wave-uniform k & 3 with scalar branches).
//   PHASE 0: block 3t   -> A = words 0,1, B = words 2,3          row = (A.cos, A.sin, B.cos), carry B.sin
//   PHASE 1: block 3t+1 -> A = words 0,1; words 2,3 carried      row = (carried, A.cos, A.sin)
//   PHASE 2: block 3t+2 -> A = carried words, B = words 0,1      row = (A.cos, A.sin, B.cos), carry B.sin, words 2,3
//   PHASE 3: no block   -> A = carried words                     row = (carried, A.cos, A.sin)
template <int PHASE>
__device__ __forceinline__ void shock_row_phase(ShockGen& G, uint64_t seed, uint32_t stream_id, uint64_t path,
                                                uint32_t k, double rho, double rho_c, const double* tab,
                                                double& z_eq, double& z_inf, double& z_prem) {
    uint32_t x[4] = {0u, 0u, 0u, 0u};
    if (PHASE != 3)
        philox4x32_10((uint32_t)path, (uint32_t)(path >> 32), 3u * (k >> 2) + (uint32_t)PHASE, stream_id, (uint32_t)seed,
                      (uint32_t)(seed >> 32), x);
    const uint32_t ar = PHASE < 2 ? x[0] : G.cw0, aa = PHASE < 2 ? x[1] : G.cw1;
    double ac, as;
    bm_pair(ar, aa, tab, MathRegs::literals(), ac, as);
    double n0, n1, n2;
    if ((PHASE & 1) == 0) {
        const uint32_t br = PHASE == 0 ? x[2] : x[0], ba = PHASE == 0 ? x[3] : x[1];
        double bc, bs;
        bm_pair(br, ba, tab, MathRegs::literals(), bc, bs);
        n0 = ac; n1 = as; n2 = bc;
        G.carry_z = bs;
    } else {
        n0 = G.carry_z; n1 = ac; n2 = as;
    }
    if (PHASE == 1 || PHASE == 2) { G.cw0 = x[2]; G.cw1 = x[3]; }
    z_eq = n0;
    z_inf = __builtin_fma(rho, n0, rho_c * n1);
    z_prem = n2;
}

// Row `k`, given that rows 0..k-1 of this path were generated by this ShockGen in order (k is wave-uniform).
__device__ __forceinline__ void shock_row_seq(ShockGen& G, uint64_t seed, uint32_t stream_id, uint64_t path,
                                              uint32_t k, double rho, double rho_c, const double* tab,
                                              double& z_eq, double& z_inf, double& z_prem) {
    switch (__builtin_amdgcn_readfirstlane((int)(k & 3u))) {
        case 0: shock_row_phase<0>(G, seed, stream_id, path, k, rho, rho_c, tab, z_eq, z_inf, z_prem); break;
        case 1: shock_row_phase<1>(G, seed, stream_id, path, k, rho, rho_c, tab, z_eq, z_inf, z_prem); break;
        case 2: shock_row_phase<2>(G, seed, stream_id, path, k, rho, rho_c, tab, z_eq, z_inf, z_prem); break;
        default: shock_row_phase<3>(G, seed, stream_id, path, k, rho, rho_c, tab, z_eq, z_inf, z_prem); break;
    }
}

// _monthly_gross_from_shock (:468-474) with a = mu_log/12 and b = sigma_log/sqrt(12) precomputed.
__device__ __forceinline__ double monthly_gross(double a, double b, double z, const double* tab, const MathRegs& R = MathRegs::literals()) {
    return fexp(__builtin_fma(b, z, a), tab, R);   // (one rounding instead of the reference's two: 1e-16 |x| on the argument)
}

// TWO consecutive months at once.  Rows 4t .. 4t+3 of a path use exactly Philox blocks 3t .. 3t+2 -> Box-Muller
// pairs P0 .. P5 (normals n[12t + 2i], n[12t + 2i + 1] = Pi.cos, Pi.sin), so with a PAIR of rows as the unit which
// word feeds which pair is fixed at compile time by the half (no per-row selects, nothing shuffled between rows):
//   HALF 0 (rows 4t, 4t+1):   blocks 3t and 3t+1;  P0 = (w0,w1), P1 = (w2,w3) of 3t, P2 = (w0,w1) of 3t+1,
//                             words 2,3 of 3t+1 are carried;   rows = (P0.c, P0.s, P1.c), (P1.s, P2.c, P2.s)
//   HALF 1 (rows 4t+2, 4t+3): block 3t+2;  P3 = carried words, P4 = (w0,w1), P5 = (w2,w3);
//                             rows = (P3.c, P3.s, P4.c), (P4.s, P5.c, P5.s)
// The path kernel calls this at every even row (wave-uniform) and stages the two months' gross factors
// (g1, g_inflation, g2 = g_inflation * g_premium; :522-532) in the lane's own LDS column:
// `stage[j * COLS]`, j = 3 * (row & 1) + {0, 1, 2} (COLS = kBlock: 12 KB per workgroup; the expense fan-out's 64-path
// workgroups stage 64 columns).  The six pairs of a HALF are
// independent straight-line work (lots of instruction-level parallelism next to the serial month bodies of
// the other waves).  The normals are shock_row_seq's; the log-returns are associated on their parts (below).
struct PairCarry { uint32_t w2, w3; };
// GEN: how the Philox blocks are drawn.  kGenPlain = philox4x32_10 on the whole counter; kGenUniform = philox_path_rounds
// with the wave's path_hi (wave-uniform: right only when PhiloxPath::hi_uniform); kGenGeneral = philox_path_rounds with each
// lane's path_hi.  All three give the same words wherever they are right.
// Side effects: the lane's stage slots (six factors, growth_rows2_form; nine parts, growth_parts2_stage_form) and, in HALF 0,
// the carry — nothing else.  growth_rows2 and growth_parts2 rely on that (a straddling wave runs the form twice and the second
// pass overwrites the first); an output added here must be overwritten the same way.
enum { kGenPlain = 0, kGenUniform = 1, kGenGeneral = 2 };
// GF: the launch's GROWTH FORM, a two-bit mask of what its parameters make unnecessary (chosen on the host, mcr_hip.hip:
// growth_form_of; every value is bit for bit the general form's wherever it may be used).
//   kGrowthNarrowExp: every argument of exp has k in fexp's narrow window -> fexp<., NARROW> on a ROTATED table: the biased shifter's low word is the
//                     table position, no mask (mcr_math.h)
//   kGrowthRhoZero:   rho = 0 -> binf_rho is an exact zero and x_inf's first term, fma(+-0 r0, t0, y) = y, is dropped (only the
//                     sign of a zero sum can differ, and exp maps both zeros to 1)
enum { kGrowthNarrowExp = 1, kGrowthRhoZero = 2 };
// The form in two steps.  growth_parts2_form: the PARTS of the half's six normals — they depend on the path alone (Philox
// rounds, Box-Muller radius and angle).  growth_factors_row: a month's three factors (equity, inflation, premium) from the parts and a MARKET, any
// object with the seven members a1, b1, ainf, binf_rho, binf_rho_c, aprem, bprem (DevParams, or a record of the assumption
// fan-out, path_kernel PHASE 9, whose consumer waves each apply their own market to the parts the producer staged).
template <int HALF, int GEN>
__device__ __forceinline__ void growth_parts2_form(const MathRegs& M, uint64_t seed, uint32_t stream_id, uint64_t path, const PhiloxPath& Q,
                                                   uint32_t t, const double* tab, double (&rad)[3], double (&trig)[6], PairCarry& C) {
    auto draw = [&](uint32_t block, uint32_t (&x)[4]) {
        if (GEN == kGenPlain)
            philox4x32_10((uint32_t)path, (uint32_t)(path >> 32), block, stream_id, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        else
            philox_path_rounds<GEN == kGenUniform>(Q, block, (uint32_t)seed, (uint32_t)(seed >> 32), x);
    };
    // pair i: radius rad[i], trig[2 i] = cos, trig[2 i + 1] = sin; normal j of the half = rad[j >> 1] * trig[j]
    uint32_t x[4];
    if (HALF == 0) {
        draw(3u * t, x);
        bm_parts<GEN != kGenPlain>(x[0], x[1], tab, M, rad[0], trig[0], trig[1]);
        bm_parts<GEN != kGenPlain>(x[2], x[3], tab, M, rad[1], trig[2], trig[3]);
        draw(3u * t + 1u, x);
        bm_parts<GEN != kGenPlain>(x[0], x[1], tab, M, rad[2], trig[4], trig[5]);
        C.w2 = x[2]; C.w3 = x[3];
    } else {
        bm_parts<GEN != kGenPlain>(C.w2, C.w3, tab, M, rad[0], trig[0], trig[1]);
        draw(3u * t + 2u, x);
        bm_parts<GEN != kGenPlain>(x[0], x[1], tab, M, rad[1], trig[2], trig[3]);
        bm_parts<GEN != kGenPlain>(x[2], x[3], tab, M, rad[2], trig[4], trig[5]);
    }
}
// The three log-returns of a month, x = a + b z (:473) with z_inf = rho n0 + rho_c n1 (:461-464), written on the
// PARTS of the normals: x_eq = (b1 r) t + a1, x_inf = (binf rho r0) t0 + ((binf rho_c r1) t1 + a_inf), x_prem
// likewise — the same eight fp64 operations as "normals first", but every FMA now has ONE scalar operand (a VOP3
// instruction reads at most one: b z + a with a and b both in SGPRs cost two v_mov_b32 per evaluation, six a month).
// The product is associated differently from shock_row_seq's (b (r t) vs (b r) t): the arguments of exp agree to
// ~1e-17, a tenth of an ulp of the growth factor.
// (re, te), (ri, ti), (rp, tp): radius and cosine / sine of the month's equity, inflation and premium normals.
// SADD: the market is wave-uniform in SGPRs and the addend of each FMA is spelled out as the scalar operand (v_fma_f64: left
// to itself the compiler picks the two-address v_fmac_f64 and copies the scalar into its accumulator first — the very two
// v_mov_b32 this arrangement is there to avoid).  SADD = false: the same operations on a market held in VGPRs.
template <int GF, bool SADD, typename MARKET>
__device__ __forceinline__ void growth_factors_row(const MARKET& K, double re, double te, double ri, double ti, double rp, double tp,
                                                   const double* tab, const MathRegs& M, double& g1, double& ginf, double& gprem) {
    auto fma_vvs = [](double a, double b, double c_scalar) {
        double d;
        if constexpr (SADD) asm("v_fma_f64 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c_scalar));
        else d = __builtin_fma(a, b, c_scalar);
        return d;
    };
    const double x_eq = fma_vvs(K.b1 * re, te, K.a1);
    const double x_inf = (GF & kGrowthRhoZero) ? fma_vvs(K.binf_rho_c * ri, ti, K.ainf)
                                               : __builtin_fma(K.binf_rho * re, te, fma_vvs(K.binf_rho_c * ri, ti, K.ainf));
    const double x_prem = fma_vvs(K.bprem * rp, tp, K.aprem);
    constexpr bool kNarrow = (GF & kGrowthNarrowExp) != 0;
    g1 = fexp<true, kNarrow>(x_eq, tab, M);
    ginf = fexp<true, kNarrow>(x_inf, tab, M);
    gprem = fexp<true, kNarrow>(x_prem, tab, M);      // (the caller forms g2 = ginf * gprem, :532, where it uses it)
}
// ... and the second step: the two months' factors from the parts of a half, staged
template <int COLS, int GF = 0>
__device__ __forceinline__ void growth_stage_rows(const DevParams& P, const MathRegs& M, const double (&rad)[3], const double (&trig)[6],
                                                  const double* tab, double* stage) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int je = 3 * r, ji = 3 * r + 1, jp = 3 * r + 2;
        double g1, ginf, gprem;
        growth_factors_row<GF, true>(P, rad[je >> 1], trig[je], rad[ji >> 1], trig[ji], rad[jp >> 1], trig[jp], tab, M, g1, ginf, gprem);
        stage[(3 * r + 0) * COLS] = g1;
        stage[(3 * r + 1) * COLS] = ginf;
        stage[(3 * r + 2) * COLS] = ginf * gprem;                               // :532
    }
}
template <int HALF, int COLS, int GEN, int GF = 0>
__device__ __forceinline__ void growth_rows2_form(const DevParams& P, const MathRegs& M, uint64_t seed, uint32_t stream_id, uint64_t path,
                                                  const PhiloxPath& Q, uint32_t t, const double* tab, double* stage, PairCarry& C) {
    double rad[3], trig[6];
    growth_parts2_form<HALF, GEN>(M, seed, stream_id, path, Q, t, tab, rad, trig, C);
    growth_stage_rows<COLS, GF>(P, M, rad, trig, tab, stage);
}
// growth_rows2 (PER_PATH) for a producer wave that stages only the pairs of ITS half (path_kernel NPROD = 2: one wave runs every
// HALF 0, another every HALF 1), with a hook between the two steps of the form.  Such a wave has no carry from the half before:
// a HALF 1 draws block 3t + 1 again for its words 2 and 3 (one more block of integer work against the pair's fp64 work).
// `mid()` runs once, at a wave-uniform point behind the parts (a straddling wave has made both passes by then) and in front of
// the factors and every store to the stage: the caller's workgroup barrier, which therefore also orders the stores.
template <int HALF, int COLS, typename MID>
__device__ __forceinline__ void growth_rows2_own_half(const DevParams& P, const MathRegs& M, uint64_t seed, uint32_t stream_id, uint64_t path,
                                                      const PhiloxPath& Q, uint32_t t, const double* tab, double* stage, MID&& mid) {
    double rad[3], trig[6];
    PairCarry C{0u, 0u};
    uint32_t x[4];
    if (HALF == 1) {
        philox_path_rounds<true>(Q, 3u * t + 1u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
        C.w2 = x[2]; C.w3 = x[3];
    }
    growth_parts2_form<HALF, kGenUniform>(M, seed, stream_id, path, Q, t, tab, rad, trig, C);
    if (__builtin_expect(!Q.hi_uniform, 0)) {
        if (HALF == 1) {
            philox_path_rounds<false>(Q, 3u * t + 1u, (uint32_t)seed, (uint32_t)(seed >> 32), x);
            C.w2 = x[2]; C.w3 = x[3];
        }
        asm volatile("" : "+v"(C.w2), "+v"(C.w3));      // (growth_rows2: keeps the general form a branch)
        growth_parts2_form<HALF, kGenGeneral>(M, seed, stream_id, path, Q, t, tab, rad, trig, C);
    }
    mid();
    growth_stage_rows<COLS>(P, M, rad, trig, tab, stage);
}
// The assumption fan-out's producer (path_kernel PHASE 9) stages the PARTS of a half instead of its factors: nine doubles per
// lane, `stage[i * COLS]` = rad[i] for i < 3 and `stage[(3 + j) * COLS]` = trig[j].  Side effects as growth_rows2_form's: the
// lane's nine slots and, in HALF 0, the carry (a straddling wave's second pass overwrites both).
constexpr int kPartsPerPair = 9;
template <int HALF, int COLS, int GEN>
__device__ __forceinline__ void growth_parts2_stage_form(const MathRegs& M, uint64_t seed, uint32_t stream_id, uint64_t path,
                                                         const PhiloxPath& Q, uint32_t t, const double* tab, double* stage, PairCarry& C) {
    double rad[3], trig[6];
    growth_parts2_form<HALF, GEN>(M, seed, stream_id, path, Q, t, tab, rad, trig, C);
#pragma unroll
    for (int i = 0; i < 3; ++i) stage[i * COLS] = rad[i];
#pragma unroll
    for (int j = 0; j < 6; ++j) stage[(3 + j) * COLS] = trig[j];
}
// ... and a consumer's month `row` of the staged pair (r = row & 1, wave-uniform) under its own market: row 0 of a pair is
// normals 0, 1, 2 of the half (radii 0, 0, 1), row 1 is normals 3, 4, 5 (radii 1, 2, 2)
template <int COLS, typename MARKET>
__device__ __forceinline__ void growth_factors_staged(const MARKET& K, const double* pair, int r, const double* tab, const MathRegs& M,
                                                      double& g1, double& ginf, double& g2) {
    const double* rd = pair + (size_t)r * COLS;                 // rad[r], rad[2 r] = rd[r COLS], rad[1 + r] = rd[COLS]
    const double* tg = pair + (size_t)(3 + 3 * r) * COLS;       // trig[3 r ..]
    double gprem;
    growth_factors_row<0, false>(K, rd[0], tg[0], rd[(size_t)r * COLS], tg[COLS], rd[COLS], tg[2 * COLS], tab, M, g1, ginf, gprem);
    g2 = ginf * gprem;                                                          // :532
}
// PER_PATH (the count-only kernels without an annual-gains tax: the issue-bound launches): every wavefront runs the form
// with a wave-uniform path_hi — one straight-line block, the Philox words interleaved with the fp64 work of the pairs (a
// wave-uniform branch around the first rounds alone split that block and cost as much time as the rounds saved).  The rare
// wavefront whose paths straddle a multiple of 2^32 then runs the general form as well, which overwrites what the first
// pass staged and carried with the right words (HALF 0 carries only words it draws, HALF 1 only reads the carry).
// Otherwise the plain generator: in the variants with per-path outputs or an annual-gains tax the second form's registers
// cost scratch, and those launches are not bound by the generator's issue slots.
template <int HALF, int COLS = kBlock, bool PER_PATH = false, int GF = 0>
__device__ __forceinline__ void growth_rows2(const DevParams& P, const MathRegs& M, uint64_t seed, uint32_t stream_id, uint64_t path,
                                             const PhiloxPath& Q, uint32_t t, const double* tab, double* stage, PairCarry& C) {
    static_assert(GF == 0 || PER_PATH, "the growth forms exist for the issue-bound per-path launches");
    if (!PER_PATH) {
        growth_rows2_form<HALF, COLS, kGenPlain>(P, M, seed, stream_id, path, Q, t, tab, stage, C);
        return;
    }
    growth_rows2_form<HALF, COLS, kGenUniform, GF>(P, M, seed, stream_id, path, Q, t, tab, stage, C);
    if (__builtin_expect(!Q.hi_uniform, 0)) {
        // the barrier keeps the general form a branch (left alone the compiler computes both forms and selects) and its
        // inputs opaque (no values of the first pass kept live into it: both forms then fit the same registers)
        PairCarry C2 = C;
        asm volatile("" : "+v"(C2.w2), "+v"(C2.w3));
        growth_rows2_form<HALF, COLS, kGenGeneral, GF>(P, M, seed, stream_id, path, Q, t, tab, stage, C2);
        C = C2;
    }
}
// growth_rows2 for the assumption fan-out's producer: the parts of the pair, staged (growth_parts2_stage_form)
template <int HALF, int COLS, bool PER_PATH>
__device__ __forceinline__ void growth_parts2(const MathRegs& M, uint64_t seed, uint32_t stream_id, uint64_t path, const PhiloxPath& Q,
                                              uint32_t t, const double* tab, double* stage, PairCarry& C) {
    if (!PER_PATH) {
        growth_parts2_stage_form<HALF, COLS, kGenPlain>(M, seed, stream_id, path, Q, t, tab, stage, C);
        return;
    }
    growth_parts2_stage_form<HALF, COLS, kGenUniform>(M, seed, stream_id, path, Q, t, tab, stage, C);
    if (__builtin_expect(!Q.hi_uniform, 0)) {
        PairCarry C2 = C;
        asm volatile("" : "+v"(C2.w2), "+v"(C2.w3));
        growth_parts2_stage_form<HALF, COLS, kGenGeneral>(M, seed, stream_id, path, Q, t, tab, stage, C2);
        C = C2;
    }
}
constexpr int kStageDoubles = 6 * kBlock;   // 12 KB of LDS per workgroup

// STRICT vs path form of the helpers.  Inside the path kernel the state obeys 0 <= balance,
// 0 <= cost basis, 0 <= rate <= 1 and "amount sold <= amount held" by construction, which makes several
// clamps of the reference exact no-ops in IEEE arithmetic (x <= y => fl(y - x) >= 0; f <= 1, c >= 0 =>
// fl(c f) <= c; fl(x / y) <= 1 for x <= y).  STRICT = true keeps every clamp for arbitrary inputs (the
// unit-function entry point, bit-exact vs the reference on its test vectors); STRICT = false drops the
// provable no-ops — identical results on every reachable state, ~3 % fewer VALU instructions.

// _net_liquidation_value (:256-272); rate = realized rate if that system applies else 0.0.
// TAXED = false is the compile-time variant for scenarios in which NEITHER asset has an effective
// realized-gains rate (the reference's DEFAULT configuration, config.py:74-75,80-81).  With rate == 0 every
// product with it is exactly +0, t / 1 = t, so the untaxed forms are bit-identical to the general ones and
// skip the dead arithmetic (two of the three divisions in withdraw / rebalance): +13 % paths/s there.
// (A run-time branch instead cost the taxed kernel 4 %, hence a template parameter.)
template <bool STRICT = true, bool TAXED = true, bool MM = true>
__device__ __forceinline__ double net_liquidation_value(double bal, double cb, double rate) {
    double v = bal;  // rate == 0: tax = 0, max(0, bal - 0) = bal for bal > eps
    if (TAXED) {
        const double tax = fmax(0.0, bal - cb) * rate;
        v = STRICT ? fmax(0.0, bal - tax) : bal - tax;  // tax <= bal when cb >= 0, rate <= 1
    }
    if (STRICT) return bal <= kEps ? 0.0 : v;
    if (bal <= kEps) { MCR_MASKED_MOVE; v = 0.0; }   // path form: exec-masked move instead of a select (see withdraw)
    return v;
}

// _calculate_withdrawal_and_update (:201-254): every lane evaluates the arithmetic; only the final selections differ by form.
template <bool STRICT = true, bool TAXED = true, bool MM = true>
__device__ __forceinline__ void withdraw(double& bal, double& cb, double net_target, double rate,
                                         double& gross_out, double& net_out) {
    const bool skip = (bal <= kEps) || (net_target <= 0.0);              // :218
    const double inv_bal = recip_nr<STRICT>(bal);                        // shared by the two divisions by bal
    double gross;
    if (TAXED) {
        const double gain_fraction = div_by(fmax(0.0, bal - cb), bal, inv_bal);  // :221
        const double net_fraction = fmax(kEps, 1.0 - gain_fraction * rate);  // :222-227
        gross = fmin(fdiv<STRICT>(net_target, net_fraction), bal);       // :228-231
    } else {
        gross = fmin(net_target, bal);                                   // net_fraction = max(eps, 1 - g*0) = 1; t / 1 = t
    }
    const double sold = div_by(gross, bal, inv_bal);
    const double fraction_sold = STRICT ? fmin(1.0, sold) : sold;        // :233  (gross <= bal)
    const double basis_part = cb * fraction_sold;
    const double basis_removed = STRICT ? fmin(cb, basis_part) : basis_part;  // :234  (fraction <= 1, cb >= 0)
    double net_cash = gross;                                             // rate == 0: tax_paid = 0, max(0, gross) = gross
    if (TAXED) {
        const double taxable_gain = fmax(0.0, gross - basis_removed);    // :235
        const double tax_paid = taxable_gain * rate;                     // :236-240
        net_cash = STRICT ? fmax(0.0, gross - tax_paid) : gross - tax_paid;  // :241 (tax <= gross)
    }
    double nb = STRICT ? fmax(0.0, bal - gross) : bal - gross;           // :243
    double ncb = STRICT ? fmax(0.0, cb - basis_removed) : cb - basis_removed;  // :244
    const bool dust = nb <= kEps;                                        // :245-247
    if (STRICT) {
        nb = dust ? 0.0 : nb;
        ncb = dust ? 0.0 : ncb;
        bal = skip ? fmax(0.0, bal) : nb;                                // :219
        cb = skip ? fmax(0.0, cb) : ncb;
        gross_out = skip ? 0.0 : gross;
        net_out = skip ? 0.0 : net_cash;
    } else {
        // Path form: the same selections as exec-masked moves.  A 64-bit select is two v_cndmask at a full issue slot
        // each; a move under an exec mask costs about half of that, and the scalar mask bookkeeping is free next to
        // the VALU work.  (The empty asm keeps the compiler from converting the branches back into selects.)
        double rb = nb, rc = ncb, rg = gross, rn = net_cash;
        if (dust) { MCR_MASKED_MOVE; rb = 0.0; rc = 0.0; }
        if (skip) { MCR_MASKED_MOVE; rb = bal; rc = cb; rg = 0.0; rn = 0.0; }   // bal, cb >= 0 already
        bal = rb; cb = rc; gross_out = rg; net_out = rn;
    }
}

// Path form of TWO independent evaluations of the same helper (the two assets of one month): all the arithmetic of
// both first — two independent dependency chains the scheduler can interleave —, then the exec-masked fix-ups
// (each branch ends a basic block; placed between the two chains they would serialise them).
// (T1 / T2: does asset 1 / 2 carry an effective realized-gains rate?  Per asset since round 3: the reference's DEFAULT
//  configuration taxes realized gains on inv2 only, config.py:74-75,80-81 — with a rate of exactly 0 every product with it is
//  +0 and t / 1 = t, so the untaxed form of ONE asset is bit-identical too and skips its dead divisions.)
template <bool T1, bool T2 = T1, bool MM = true>
__device__ __forceinline__ void net_liquidation_values2(double b1, double c1, double r1, double b2, double c2, double r2,
                                                        double& v1, double& v2) {
    v1 = b1; v2 = b2;
    if (T1) v1 = b1 - fmax(0.0, b1 - c1) * r1;                   // tax <= bal when cb >= 0, rate <= 1
    if (T2) v2 = b2 - fmax(0.0, b2 - c2) * r2;
    if (b1 <= kEps) { MCR_MASKED_MOVE; v1 = 0.0; }
    if (b2 <= kEps) { MCR_MASKED_MOVE; v2 = 0.0; }
}

struct WithdrawCand { double nb, ncb, gross, net; };   // (the dust / skip tests are evaluated at the fix-up: a compare there
                                                       //  is one instruction, a flag carried across the other chain's blocks is two)
template <bool TAXED>
__device__ __forceinline__ WithdrawCand withdraw_arith(double bal, double cb, double net_target, double rate) {
    WithdrawCand w;
    const double inv_bal = recip_nr<false>(bal);
    if (TAXED) {
        const double gain_fraction = div_by(fmax(0.0, bal - cb), bal, inv_bal);  // :221
        const double net_fraction = fmax(kEps, 1.0 - gain_fraction * rate);  // :222-227
        w.gross = fmin(fdiv<false>(net_target, net_fraction), bal);      // :228-231
    } else {
        w.gross = fmin(net_target, bal);
    }
    const double fraction_sold = div_by(w.gross, bal, inv_bal);         // :233  (gross <= bal)
    const double basis_removed = cb * fraction_sold;                    // :234  (fraction <= 1, cb >= 0)
    w.net = w.gross;
    if (TAXED) {
        const double taxable_gain = fmax(0.0, w.gross - basis_removed); // :235
        w.net = w.gross - taxable_gain * rate;                          // :236-241 (tax <= gross)
    }
    w.nb = bal - w.gross;                                               // :243
    w.ncb = cb - basis_removed;                                         // :244
    return w;
}
template <bool MM = true>
__device__ __forceinline__ void withdraw_fixup(WithdrawCand& w, double& bal, double& cb, double net_target, double& gross_out,
                                               double& net_out) {
    if (w.nb <= kEps) { MCR_MASKED_MOVE; w.nb = 0.0; w.ncb = 0.0; }                        // :245-247
    if ((bal <= kEps) || (net_target <= 0.0)) {                                             // :218
        MCR_MASKED_MOVE;
        w.nb = bal; w.ncb = cb; w.gross = 0.0; w.net = 0.0;                                 // bal, cb >= 0 already (:219)
    }
    bal = w.nb; cb = w.ncb; gross_out = w.gross; net_out = w.net;
}
template <bool T1, bool T2 = T1, bool MM = true>
__device__ __forceinline__ void withdraw2(double& b1, double& c1, double t1, double r1, double& g1, double& n1,
                                          double& b2, double& c2, double t2, double r2, double& g2, double& n2) {
    WithdrawCand w1 = withdraw_arith<T1>(b1, c1, t1, r1);
    WithdrawCand w2 = withdraw_arith<T2>(b2, c2, t2, r2);
    withdraw_fixup<MM>(w1, b1, c1, t1, g1, n1);
    withdraw_fixup<MM>(w2, b2, c2, t2, g2, n2);
}

// _rebalance_portfolio (:274-359): every lane evaluates the arithmetic with the over-weight asset as the seller.
template <bool STRICT = true, bool TAXED = true, bool MM = true>
__device__ __forceinline__ void rebalance(const LaneParams& P, double& b1, double& c1, double& b2,
                                          double& c2) {
    const double total = b1 + b2;                                  // :288
    const double drift1 = b1 - total * P.alloc1;                   // :293-294
    const bool act = (total > kEps) && (fabs(drift1) > kEps);      // :290-296
    // Wave-uniform early-out: the rebalance that closes the yearly tax step runs right after the monthly
    // one, when every lane is already within eps of its target (nothing to do for the whole wave).
    // (the two compares are balloted separately: each folds into its v_cmp, whereas a ballot of their AND can come
    //  out as a 0/1 VGPR that is compared again)
    if ((__builtin_amdgcn_ballot_w64(total > kEps) & __builtin_amdgcn_ballot_w64(fabs(drift1) > kEps)) == 0ull) return;
    const bool sell1 = drift1 > 0.0;                               // :298
    const double drift2 = b2 - total * P.alloc2;                   // :328
    const double bs = sell1 ? b1 : b2, cs = sell1 ? c1 : c2;       // seller
    const double bb = sell1 ? b2 : b1, cbuy = sell1 ? c2 : c1;     // buyer
    const double drift = sell1 ? drift1 : drift2;
    const double alloc_s = sell1 ? P.alloc1 : P.alloc2;            // the SOLD asset's own weight (:309,:337)
    const double rate_s = sell1 ? P.real_rate1 : P.real_rate2;
    const double inv_bs = recip_nr<STRICT>(bs);                    // shared by the two divisions by bs
    double gross_sale;
    if (TAXED) {
        const double gain_fraction = div_by(fmax(0.0, bs - cs), bs, inv_bs);  // :301 / :329
        const double tax_per_dollar = gain_fraction * rate_s;      // :302-306
        const double denom = fmax(kEps, 1.0 - alloc_s * tax_per_dollar);  // :307-310
        gross_sale = fmin(bs, fdiv<STRICT>(drift, denom));         // :311
    } else {
        gross_sale = fmin(bs, drift);                              // tax_per_dollar = 0, denom = 1, drift / 1 = drift
    }
    const double fraction_sold = div_by(gross_sale, bs, inv_bs);   // :312
    const double basis_part = cs * fraction_sold;
    const double basis_removed = STRICT ? fmin(cs, basis_part) : basis_part;  // :313 (gross_sale <= bs, cs >= 0)
    double net_purchase = gross_sale;                              // rates 0: tax_paid = 0
    if (TAXED) {
        const double taxable_gain = fmax(0.0, gross_sale - basis_removed);  // :314
        const double tax_paid = taxable_gain * rate_s;             // :315-319
        net_purchase = gross_sale - tax_paid;                      // :320
    }
    double nbs = STRICT ? fmax(0.0, bs - gross_sale) : bs - gross_sale;        // :322
    double ncs = STRICT ? fmax(0.0, cs - basis_removed) : cs - basis_removed;  // :323
    double nbb = bb + net_purchase;                                // :324
    double ncb = cbuy + net_purchase;                              // :325
    const bool dust_s = nbs <= kEps, dust_b = nbb <= kEps;         // :355-358
    if (STRICT) {
        nbs = dust_s ? 0.0 : nbs;
        ncs = dust_s ? 0.0 : ncs;
        nbb = dust_b ? 0.0 : nbb;
        ncb = dust_b ? 0.0 : ncb;
        const double r1 = sell1 ? nbs : nbb, rc1 = sell1 ? ncs : ncb;
        const double r2 = sell1 ? nbb : nbs, rc2 = sell1 ? ncb : ncs;
        b1 = act ? r1 : b1;
        c1 = act ? rc1 : c1;
        b2 = act ? r2 : b2;
        c2 = act ? rc2 : c2;
    } else {   // path form: the same selections as exec-masked moves (see withdraw)
        if (dust_s) { MCR_MASKED_MOVE; nbs = 0.0; ncs = 0.0; }
        if (dust_b) { MCR_MASKED_MOVE; nbb = 0.0; ncb = 0.0; }
        if (act) {
            MCR_MASKED_MOVE;
            if (sell1) { MCR_MASKED_MOVE; b1 = nbs; c1 = ncs; b2 = nbb; c2 = ncb; }
            else { MCR_MASKED_MOVE; b1 = nbb; c1 = ncb; b2 = nbs; c2 = ncs; }
        }
    }
}

// Path form of _rebalance_portfolio (:274-359).  Same arithmetic as rebalance<false, TAXED>; what differs is how the
// results land.  The whole update runs under the exec mask of the lanes that act, so nothing has to be selected
// back for the others; the buyer is not selected on the way in: the net purchase is added to BOTH assets in place
// (:324-325 / :352-353 for whichever is the buyer) and the seller's pair is then overwritten under its own mask
// (:322-323 / :350-351).  10 v_cndmask + 4 masked moves, against 14 + 8 for the select-in / select-out form.
template <bool TAXED, bool MM = true>
__device__ __forceinline__ void rebalance_path(const LaneParams& P, double& b1, double& c1, double& b2, double& c2) {
    const double total = b1 + b2;                                  // :288
    const double drift1 = b1 - total * P.alloc1;                   // :293-294
    // (A wave in which no lane acts — e.g. the rebalance that closes the yearly tax step, right after the monthly
    //  one — skips the block through the s_cbranch_execz of this branch: no separate ballot is needed.)
    if ((total > kEps) && (fabs(drift1) > kEps)) {                 // :290-296
        MCR_MASKED_MOVE;
        const bool sell1 = drift1 > 0.0;                           // :298
        const double drift2 = b2 - total * P.alloc2;               // :328
        const double bs = sell1 ? b1 : b2, cs = sell1 ? c1 : c2;   // seller
        const double drift = sell1 ? drift1 : drift2;
        const double alloc_s = sell1 ? P.alloc1 : P.alloc2;        // the SOLD asset's own weight (:309,:337)
        const double rate_s = sell1 ? P.real_rate1 : P.real_rate2;
        const double inv_bs = recip_nr<false>(bs);                 // shared by the two divisions by bs
        double gross_sale;
        if (TAXED) {
            const double gain_fraction = div_by(fmax(0.0, bs - cs), bs, inv_bs);  // :301 / :329
            const double tax_per_dollar = gain_fraction * rate_s;  // :302-306
            const double denom = fmax(kEps, 1.0 - alloc_s * tax_per_dollar);  // :307-310
            gross_sale = fmin(bs, fdiv<false>(drift, denom));      // :311
        } else {
            gross_sale = fmin(bs, drift);                          // tax_per_dollar = 0, denom = 1, drift / 1 = drift
        }
        const double fraction_sold = div_by(gross_sale, bs, inv_bs);   // :312
        const double basis_removed = cs * fraction_sold;           // :313 (gross_sale <= bs, cs >= 0: the min is a no-op)
        double net_purchase = gross_sale;                          // rates 0: tax_paid = 0
        if (TAXED) {
            const double taxable_gain = fmax(0.0, gross_sale - basis_removed);  // :314
            net_purchase = gross_sale - taxable_gain * rate_s;     // :315-320
        }
        const double nbs = bs - gross_sale;                        // :322 (>= 0)
        const double ncs = cs - basis_removed;                     // :323 (>= 0)
        // (locals, not the references: a store of one value to either of two addresses would be merged into a store
        //  through a selected pointer, which pins the whole state in scratch memory)
        double r1b = b1 + net_purchase, r1c = c1 + net_purchase;   // :324-325 for the buyer; the seller's pair is replaced below
        double r2b = b2 + net_purchase, r2c = c2 + net_purchase;
        if (sell1) { MCR_MASKED_MOVE; r1b = nbs; r1c = ncs; }
        else { MCR_MASKED_MOVE; r2b = nbs; r2c = ncs; }
        if (r1b <= kEps) { MCR_MASKED_MOVE; r1b = 0.0; r1c = 0.0; }  // :355-358
        if (r2b <= kEps) { MCR_MASKED_MOVE; r2b = 0.0; r2c = 0.0; }
        b1 = r1b; c1 = r1c; b2 = r2b; c2 = r2c;
    }
}

// MF: the launch's MONTH FORM, a mask of what its parameters make unnecessary in the month's own arithmetic (chosen on the
// host, mcr_hip.hip: month_form_of; the kernels that have growth forms have month forms).  Every value is bit for bit the
// general form's wherever the bit may be used.
//   kMonthEqualRates: both assets are taxed on realized gains at the SAME rate -> rebalance_tol<..., EQR>
enum { kMonthEqualRates = 1 };

// SF: the launch's STREAM FORM, likewise for what its income-stream list makes unnecessary (host: stream_form_of; the same
// kernels, in the tolerance form of the month).
//   kStreamsInRegs: at most two records reach the kernel (the zero-amount ones are dropped on the host), none in the extra
//   table, and every one is inflation-indexed -> the records sit in SGPRs for the whole launch and the month issues their
//   FMAs in list order behind two window tests: no loop over the list, no record re-read, no lock column.
enum { kStreamsInRegs = 1 };

// ---------------------------------------------------------------------------------------------
// TOLERANCE FORM of the month (what the path kernel runs since round 4; the forms above stay the unit API, the corner
// configurations below and the A/B build -DMCR_K1_EXACT_MONTH).  The forms above mirror the reference's roundings operation
// by operation; the stated tolerance of the path is 1e-9, six orders above one rounding, so inside the month loop the same
// quantities are computed from the CLOSED FORM of the reference's formulas, fused multiply-adds and uncorrected reciprocals
// (v_rcp_f64 + one Newton step, 2^-50):
//
//  withdrawal (:726-790).  With G_i = max(0, b_i - c_i) the liquidation value is cap_i = b_i - r_i G_i (:256-272), the asset's
//    net fraction 1 - gf_i r_i = cap_i / b_i (:221-227), and its net target t_i = target cap_i / cap (:750-765).  Hence
//        gross_i = t_i / (cap_i / b_i) = b_i (target / cap):
//    BOTH assets sell the same fraction phi = target / cap of their balance, basis and gain (:233-244):
//        b_i <- b_i (1 - phi),  c_i <- c_i (1 - phi),  net cash = phi cap = target,  gross = phi (b1 + b2).
//    One reciprocal (of cap) instead of five, no per-asset quotient; the net-cash test (:784-790) IS the capacity test
//    (:743-748).  min(gross, bal) (:228-231) is phi <= 1.
//  rebalance (:274-359).  With G = max(0, bs - cs) of the seller, gross_sale = drift / (1 - a_s r_s G / bs) and
//    fraction_sold = gross_sale / bs (:301-312) are ONE quotient: fraction_sold = drift / (bs - a_s r_s G); the tax is
//    fraction_sold G r_s (:314-319: max(0, gross - basis_removed) IS fraction_sold G); the drift of asset 2 is minus the
//    drift of asset 1 (:328).
//
// Validity: the reference clamps its denominators at 1e-6 (:227, :307-310).  1 - gf r >= 1 - r and 1 - a gf r >= 1 - r, so
// with both effective realized-gains rates <= 1 - 1e-6 the clamps never bind and the closed form is the reference's
// arithmetic up to roundings (DevParams::exact_month = 0, derive_params).  Configurations with a rate above that (a 100 % tax
// on realized gains) run the exact forms in the generic kernel variants.  One sub-case is not covered by the closed form:
// alive, total balance > 1e-6 but total liquidation value <= 1e-6 (needs a total balance below 1e-6 / (1 - r) dollars): the
// reference then splits the target by the allocation weights instead of the capacity shares (:750-755), which leaves up to
// 1e-6 / (1 - r) dollars where the closed form sells out.  Those lanes run the exact forms (the path kernel's wave-uniform
// slow month; DevParams::fast_floor keeps them out of the straight-line one).  Every other difference is a relative
// perturbation of ~1e-16 per operation — what a rounding is; measured against the oracle (profiles/r04/k1_accuracy_*.txt,
// tests/test_gpu_high_rate_month.py): worst path-level error relative to the path's money scale, flips of Success flags.

// WAVE-UNIFORM fix-ups (UNIFORM = true below; the issue-bound launches, MM = true).  The dust / empty tests of the month
// (balance <= 1e-6: :218-219, :245-247, :290-296, :355-358) almost never hold, yet every one of them costs its lane-mask round
// trip (compare, s_and_saveexec, a taken s_cbranch_execz, s_or exec) every month.  With UNIFORM the compare goes into one
// wave ballot instead: when no active lane of the wave qualifies, every fix-up would have been a no-op and the straight-line
// body runs; otherwise the fix-ups run exactly as in the UNIFORM = false form.  The same values by construction.
__device__ __forceinline__ bool wave_any(bool c) { return __builtin_amdgcn_ballot_w64(c) != 0ull; }

// liquidation values (:256-272, :726-737); returns cap1 + cap2.  UNIFORM: the caller has established that no active lane of the
// wave holds a balance <= 1e-6 (the two fix-ups are no-ops).
template <bool T1, bool T2 = T1, bool MM = true, bool UNIFORM = false>
__device__ __forceinline__ double capacity_tol(double b1, double c1, double r1, double b2, double c2, double r2) {
    double v1 = b1, v2 = b2;
    if (T1) v1 = __builtin_fma(-fmax(0.0, b1 - c1), r1, b1);
    if (T2) v2 = __builtin_fma(-fmax(0.0, b2 - c2), r2, b2);
    if (!UNIFORM) {
        if (b1 <= kEps) { MCR_MASKED_MOVE; v1 = 0.0; }
        if (b2 <= kEps) { MCR_MASKED_MOVE; v2 = 0.0; }
    }
    return v1 + v2;
}
// both assets sell the fraction phi (:757-776 as derived above).  UNIFORM: as capacity_tol (the last two fix-ups are no-ops).
template <bool MM = true, bool UNIFORM = false>
__device__ __forceinline__ void sell_fraction_tol(double phi, double& b1, double& c1, double& b2, double& c2) {
    double nb1 = __builtin_fma(-b1, phi, b1), nc1 = __builtin_fma(-c1, phi, c1);     // :243-244
    double nb2 = __builtin_fma(-b2, phi, b2), nc2 = __builtin_fma(-c2, phi, c2);
    if (!UNIFORM || wave_any(fmin(nb1, nb2) <= kEps)) {
        if (nb1 <= kEps) { MCR_MASKED_MOVE; nb1 = 0.0; nc1 = 0.0; }                   // :245-247
        if (nb2 <= kEps) { MCR_MASKED_MOVE; nb2 = 0.0; nc2 = 0.0; }
    }
    if (!UNIFORM) {
        if (b1 <= kEps) { MCR_MASKED_MOVE; nb1 = b1; nc1 = c1; }                     // :218-219: an asset without a balance is left alone
        if (b2 <= kEps) { MCR_MASKED_MOVE; nb2 = b2; nc2 = c2; }
    }
    b1 = nb1; c1 = nc1; b2 = nb2; c2 = nc2;
}
// (:274-359)  L = lane_params_tol(P): L.alloc1 / L.alloc2 hold weight x rate of asset 1 / 2.  UNIFORM: the guard and the dust
// fix-ups are tested wave-wide (self-contained: no precondition); a wave with a lane that does not act takes the UNIFORM = false form.
// EQR (the launch's MONTH FORM has kMonthEqualRates, below): both assets carry the SAME realized-gains rate, so the seller's
// rate is not a per-lane choice and its select goes (the seller's weight x rate keeps its own).  The rate is read from the
// lanes' resident copy, not from the scalar block: the kernel has no SGPR pair to spare (as a scalar operand it came back as
// v_readlane + s_nop at every use).
// MASKSEL (the lone consumer wave of the screened launch's split re-run): the seller's three selects take their condition
// from an SGPR pair (v_cndmask_b32_e64 with the compare's ballot) instead of the VCC-implicit encoding behind v_cmp + s_nop
// (tools/ubench/valu_cost.hip: 4.7 against 22.6 cycles an instruction); the same words either way.
__device__ __forceinline__ void seller_select3(bool sell1, double a1, double a2, double b1, double b2, double c1, double c2, double& a, double& b, double& c) {
    const unsigned long long m = __builtin_amdgcn_ballot_w64(sell1);
    auto bits = [](double x) { return (unsigned long long)__double_as_longlong(x); };
    const unsigned long long a1b = bits(a1), a2b = bits(a2), b1b = bits(b1), b2b = bits(b2), c1b = bits(c1), c2b = bits(c2);
    uint32_t alo, ahi, blo, bhi, clo, chi;
    asm("s_nop 1\n\tv_cndmask_b32_e64 %0, %7, %6, %18\n\tv_cndmask_b32_e64 %1, %9, %8, %18\n\tv_cndmask_b32_e64 %2, %11, %10, %18\n\t"
        "v_cndmask_b32_e64 %3, %13, %12, %18\n\tv_cndmask_b32_e64 %4, %15, %14, %18\n\tv_cndmask_b32_e64 %5, %17, %16, %18"
        : "=&v"(alo), "=&v"(ahi), "=&v"(blo), "=&v"(bhi), "=&v"(clo), "=&v"(chi)
        : "v"((uint32_t)a1b), "v"((uint32_t)a2b), "v"((uint32_t)(a1b >> 32)), "v"((uint32_t)(a2b >> 32)),
          "v"((uint32_t)b1b), "v"((uint32_t)b2b), "v"((uint32_t)(b1b >> 32)), "v"((uint32_t)(b2b >> 32)),
          "v"((uint32_t)c1b), "v"((uint32_t)c2b), "v"((uint32_t)(c1b >> 32)), "v"((uint32_t)(c2b >> 32)), "s"(m));
    auto f64 = [](uint32_t hi, uint32_t lo) { return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo)); };
    a = f64(ahi, alo); b = f64(bhi, blo); c = f64(chi, clo);
}
// PT: the parameter block, or the allocation fan-out's WaveAllocParams (the consumer wave's own weight; L then holds its products).
template <bool TAXED, bool MM = true, bool UNIFORM = false, bool EQR = false, bool MASKSEL = false, typename PT = DevParams>
__device__ __forceinline__ void rebalance_tol(const PT& P, const LaneParams& L, double& b1, double& c1, double& b2, double& c2) {
    const double total = b1 + b2;                                  // :288
    const double drift1 = __builtin_fma(-total, P.alloc1, b1);     // :293-294
    if (UNIFORM && wave_any(fmin(total, fabs(drift1)) <= kEps)) {  // (one compare: a ballot of an OR comes out as a 0/1 VGPR compared again)
        rebalance_tol<TAXED, MM, false, EQR, MASKSEL>(P, L, b1, c1, b2, c2);
        return;
    }
    if (UNIFORM || ((total > kEps) && (fabs(drift1) > kEps))) {   // :290-296
        MCR_MASKED_MOVE;
        const bool sell1 = drift1 > 0.0;                           // :298
        constexpr bool kMaskSel = MASKSEL && TAXED && EQR;         // (the form the headline launch takes; the others keep their selects)
        [[maybe_unused]] double m_ar = 0.0, m_bs = 0.0, m_cs = 0.0;
        if constexpr (kMaskSel) seller_select3(sell1, L.alloc1, L.alloc2, b1, b2, c1, c2, m_ar, m_bs, m_cs);
        const double bs = kMaskSel ? m_bs : sell1 ? b1 : b2, cs = kMaskSel ? m_cs : sell1 ? c1 : c2;   // seller
        const double drift = fabs(drift1);                         // :328: b2 - total (1 - alloc1) = -(b1 - total alloc1)
        double fraction_sold, net_purchase;
        if (TAXED) {
            const double rate_s = EQR ? L.real_rate1 : sell1 ? L.real_rate1 : L.real_rate2;
            const double ar_s = kMaskSel ? m_ar : sell1 ? L.alloc1 : L.alloc2;       // the SOLD asset's own weight (:309,:337) x its rate
            const double G = fmax(0.0, bs - cs);                   // :301 / :329 (x bs)
            fraction_sold = fmin(1.0, drift * recip_nr<false>(__builtin_fma(-ar_s, G, bs)));   // :302-312
            net_purchase = fraction_sold * __builtin_fma(-G, rate_s, bs);                       // :314-320: gross - (fraction G) rate
        } else {
            fraction_sold = fmin(1.0, drift * recip_nr<false>(bs));
            net_purchase = fraction_sold * bs;
        }
        const double nbs = __builtin_fma(-bs, fraction_sold, bs);  // :322
        const double ncs = __builtin_fma(-cs, fraction_sold, cs);  // :313, :323
        double r1b = b1 + net_purchase, r1c = c1 + net_purchase;   // :324-325 for the buyer; the seller's pair is replaced below
        double r2b = b2 + net_purchase, r2c = c2 + net_purchase;
        if (sell1) { MCR_MASKED_MOVE; r1b = nbs; r1c = ncs; }
        else { MCR_MASKED_MOVE; r2b = nbs; r2c = ncs; }
        if (!UNIFORM || wave_any(fmin(r1b, r2b) <= kEps)) {
            if (r1b <= kEps) { MCR_MASKED_MOVE; r1b = 0.0; r1c = 0.0; }  // :355-358
            if (r2b <= kEps) { MCR_MASKED_MOVE; r2b = 0.0; r2c = 0.0; }
        }
        b1 = r1b; c1 = r1c; b2 = r2b; c2 = r2c;
    }
}

// TOL: the closing rebalance in its tolerance form (then L = lane_params_tol(P)); EQR: rebalance_tol's.
template <bool STRICT = true, bool TAXED = true, bool ANNUAL = true, bool T1 = TAXED, bool T2 = TAXED, bool MM = true, bool TOL = false, bool EQR = false, typename PT = DevParams>
__device__ __forceinline__ bool annual_gain_taxes(const PT& P, const LaneParams& L, double& b1, double& c1,
                                                  double& b2, double& c2, double gain1, double gain2) {
    bool tax_failed = false;
    if (ANNUAL && P.any_annual_tax) {  // wave-uniform: with no annual-tax asset the bill is 0 (:380-390)
        const double due1 = fmax(0.0, gain1) * P.annual_rate1;        // :380-384
        const double due2 = fmax(0.0, gain2) * P.annual_rate2;        // :385-389
        const double total_due = due1 + due2;                         // :390
        const double cap1 = net_liquidation_value<STRICT, T1, MM>(b1, c1, L.real_rate1);  // :392-397
        const double cap2 = net_liquidation_value<STRICT, T2, MM>(b2, c2, L.real_rate2);  // :398-403
        const double cap = cap1 + cap2;                               // :404
        const double pay = fmin(total_due, cap);                      // :405
        tax_failed = pay < total_due - kEps;                          // :406
        if (cap > kEps && pay > 0.0) {                                // :408
            const double share1 = fdiv<STRICT>(cap1, cap);            // :409
            const double share2 = 1.0 - share1;                       // :410
            double g, net1, net2;
            withdraw<STRICT, T1, MM>(b1, c1, pay * share1, L.real_rate1, g, net1);  // :411-419
            withdraw<STRICT, T2, MM>(b2, c2, pay * share2, L.real_rate2, g, net2);  // :420-428
            tax_failed = tax_failed || (net1 + net2 < total_due - kEps);  // :429-430
        }
    }
    if (STRICT) rebalance<true, TAXED, MM>(L, b1, c1, b2, c2);  // :432-442 (always)
    else if (TOL) rebalance_tol<TAXED, MM, false, EQR>(P, L, b1, c1, b2, c2);
    else rebalance_path<TAXED, MM>(L, b1, c1, b2, c2);
    return tax_failed;
}

// The path kernel's calls of the two helpers above that read the weights: on the block in every kernel but PHASE 12's
// consumers, which hand over their wave's view in its place (L = month_lane_params of the same object).
template <bool TAXED, bool MM = true, bool UNIFORM = false, bool EQR = false, bool MASKSEL = false>
__device__ __forceinline__ void month_rebalance_tol(const NoWaveAlloc&, const DevParams& P, const LaneParams& L, double& b1, double& c1, double& b2, double& c2) {
    rebalance_tol<TAXED, MM, UNIFORM, EQR, MASKSEL>(P, L, b1, c1, b2, c2);
}
template <bool TAXED, bool MM = true, bool UNIFORM = false, bool EQR = false, bool MASKSEL = false>
__device__ __forceinline__ void month_rebalance_tol(const WaveAllocParams& W, const DevParams&, const LaneParams& L, double& b1, double& c1, double& b2, double& c2) {
    rebalance_tol<TAXED, MM, UNIFORM, EQR, MASKSEL>(W, L, b1, c1, b2, c2);
}
template <bool STRICT = true, bool TAXED = true, bool ANNUAL = true, bool T1 = TAXED, bool T2 = TAXED, bool MM = true, bool TOL = false, bool EQR = false>
__device__ __forceinline__ bool month_annual_gain_taxes(const NoWaveAlloc&, const DevParams& P, const LaneParams& L, double& b1, double& c1,
                                                        double& b2, double& c2, double gain1, double gain2) {
    return annual_gain_taxes<STRICT, TAXED, ANNUAL, T1, T2, MM, TOL, EQR>(P, L, b1, c1, b2, c2, gain1, gain2);
}
template <bool STRICT = true, bool TAXED = true, bool ANNUAL = true, bool T1 = TAXED, bool T2 = TAXED, bool MM = true, bool TOL = false, bool EQR = false>
__device__ __forceinline__ bool month_annual_gain_taxes(const WaveAllocParams& W, const DevParams&, const LaneParams& L, double& b1, double& c1,
                                                        double& b2, double& c2, double gain1, double gain2) {
    return annual_gain_taxes<STRICT, TAXED, ANNUAL, T1, T2, MM, TOL, EQR>(W, L, b1, c1, b2, c2, gain1, gain2);
}

// Market step shared by both phases (:522-538 and :695-714), given the month's gross factors.
template <bool ANNUAL = true, bool TOL = false>
__device__ __forceinline__ void market_step(double g1, double ginf, double g2, double& b1, double& b2,
                                            double& gacc1, double& gacc2, double& infl) {
    if (ANNUAL) {                     // the accumulators only feed the annual tax bill
        if (TOL) {
            gacc1 = __builtin_fma(b1, g1 - 1.0, gacc1);
            gacc2 = __builtin_fma(b2, g2 - 1.0, gacc2);
        } else {
            gacc1 += b1 * (g1 - 1.0);     // :534
            gacc2 += b2 * (g2 - 1.0);     // :535
        }
    }
    b1 *= g1;                         // :536
    b2 *= g2;                         // :537
    infl *= ginf;                     // :538
}

}  // namespace mcr
