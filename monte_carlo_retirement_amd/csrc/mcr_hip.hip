// mcr_hip.hip — kernels + C ABI (include/mcr.h) of the MI355X Monte Carlo retirement engine.
//
// K1  path_kernel<MODE, RNG>   one path per lane; the whole horizon in registers
//       MODE 0: success count only          (no per-path HBM traffic; BASELINE config 2)
//       MODE 1: + per-path summary fields   (SoA, 49 B/path)
//       MODE 2: + yearly trajectories       (time-major [T][N]: 512 contiguous bytes per wave store)
//       MODE 3: yearly bins                 (every lane bins its yearly samples on the caller's edges: no per-path HBM traffic)
//       RNG 0: Philox4x32-10 + Box-Muller (mcr_device.h);  RNG 1: NumPy's SeedSequence -> PCG64 ->
//              ziggurat stream (mcr_numpy_rng.h), for literal seed parity with the reference;  RNG 2: block bootstrap of a
//              recorded market (include/mcr.h: MCR_RNG_HISTORY), the months' growth factors read from a table in LDS
//     reductions: wave ballot+popcount -> LDS -> one global atomic per workgroup.
// Helpers: helper_kernel (device unit functions + the specialised math of mcr_math.h),
//          shocks_kernel / np_shocks_kernel (_draw_shock_path).
// Aggregation kernels (quantiles / histogram) live in mcr_aggregate.hip.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see csrc/build.py).  gfx950 only.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <mutex>
#include <optional>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "mcr_device.h"
#include "mcr_events.h"
#include "mcr_numpy_rng.h"
#include "mcr_screen.h"
#include "mcr_host.h"

namespace mcr {

// ---------------------------------------------------------------------------------------------
// K1: the per-path state machine (_run_single_simulation_path, simulation.py:476-950)
// ---------------------------------------------------------------------------------------------
constexpr int kMaxSegments = 8;
// path_kernel's RNG parameter is mcr_rng.kind, and for a history launch of a scheme other than MCR_HISTORY_BLOCK this value:
// kernels of their own (history_seek<true>, mcr_device.h), so that the block rule's kernels stay the instructions they were
constexpr int kRngHistorySchemes = 3;
struct KernelIO {
    uint64_t seed;           // Philox key
    uint64_t path_begin;
    uint64_t n_paths;
    const double* injected;  // [n_paths][shock_rows][3] or nullptr
    mcr_outputs out;
    uint32_t stream_id;
    // MCR_RNG_NUMPY (mcr_numpy_rng.h).  MCR_RNG_HISTORY reads none of it: its table, length and block length share the bytes
    // of the seed-word count, the first seed word and the explicit seeds, so the kernel arguments keep their size and layout
    union { uint32_t n_entropy; uint32_t history_months; };
    union { uint32_t entropy[MCR_MAX_ENTROPY_WORDS]; struct { uint32_t history_block, history_scheme; }; };   // (the scheme over entropy[1])
    uint64_t child_offset;
    union {
        const uint32_t* path_seeds;  // [n_paths] explicit seeds or nullptr
        const double* history;       // MCR_RNG_HISTORY: Z[history_months][3]
    };
    // search probes that share their accumulation phase (PHASE 1 / 2 of path_kernel; mcr_probe_months_rng)
    double* snap;                    // [n_snap][kSnapFields][snap_stride] state at the end of month snap_months[c]
    int64_t snap_stride;
    int32_t n_snap;
    int32_t snap_months[MCR_MAX_PROBE_CANDIDATES];   // ascending
    int32_t cand_out[MCR_MAX_PROBE_CANDIDATES];      // PHASE 2: counter block of candidate c = counters + cand_out[c] * MCR_N_COUNTERS
    // PHASE 3 (time-sliced path blocks, see path_kernel): the first seg_n_split path blocks of the launch are cut into seg_q
    // segments at retirement-year boundaries; `snap` holds their hand-over state, seg_flags says which segments are done
    int32_t seg_n_split, seg_n_full, seg_q;
    int32_t seg_blocks_per_cand;                     // PHASE 4: path blocks per search candidate (the launch lists candidate-major)
    double* seg_state;                               // [seg_n_split][fields][kBlock] hand-over state
    int32_t seg_year[kMaxSegments + 1];              // segment k covers retirement years [seg_year[k], seg_year[k + 1]); segment 0 also the accumulation
    int32_t seg_bid_base;                            // MCR_K1_SEGMENT_ORDER (launch_sliced): workgroup blockIdx.x of this launch is workgroup
                                                     // seg_bid_base + blockIdx.x of the single sliced launch (0 when it is one launch)
    unsigned int* seg_flags;                         // [seg_n_split][seg_q], zeroed before the launch: 0 pending, 1 state handed over, 2 recomputed
    int32_t seg_max_polls;                           // x ~1 us: how long a successor looks for its predecessor's flag before it recomputes the block itself
    // PHASE 5 / 7 (expense / contribution fan-out, mcr_probe_expenses_rng / mcr_probe_contributions_rng): consumer wave j runs
    // level fan_expenses[j] (monthly_expenses / monthly_contribution) and adds its counts to counters + j * MCR_N_COUNTERS;
    // fan_n = blockDim.x / 64 - 1 levels.  PHASE 8 / 9 (scenario / assumption fan-out, mcr_probe_scenarios_rng /
    // mcr_probe_assumptions_rng) read fan_n only: their records are a device table (path_kernel's `cand_params`).  PHASE 10
    // (income fan-out, mcr_probe_income_rng) likewise, and fan_stream below
    int32_t fan_n;
    // MODE 3 (yearly bins, mcr_run_year_bins_rng) shares the bytes of the fan-out levels: no launch is both, and the layout
    // of the kernel arguments every other variant reads stays what it was
    struct YearBins {
        const double* edges;                  // [n_bins + 1]
        const double* wr_edges;               // [n_wr_bins + 1]
        unsigned long long* trajectory;       // [T][n_bins + 2] or nullptr
        unsigned long long* real_trajectory;  // [T][n_bins + 2] or nullptr
        unsigned long long* wr;               // [ry][n_wr_bins + 2] or nullptr
        unsigned long long* final_success;    // [n_bins + 2] or nullptr
        int32_t n_bins, n_wr_bins;            // (0: the group is not requested)
    };
    // PHASE 8 / 9 / 10, outcome probes (mcr_probe_*_outcomes_rng; path_kernel's OUT): [fan_n][row_stride] rows or nullptr; lane l of
    // consumer wave j stores its path's outcome to element 64 blockIdx.x + l of row j.  These launches read no fan-out level, so
    // the rows share those bytes too (behind the word of PHASE 10's fan_stream): the kernel arguments keep their size and layout
    struct FanRows {
        int64_t fan_stream_word;
        double* final_balance;
        double* years_to_ruin;
        int64_t row_stride;
    };
    // keep = 1 - cut and grow = 1 + raise, formed once on the host (the same two fp64 operations include/mcr.h states)
    struct RuleIO {
        double upper, lower, keep, grow, floor, ceiling;
        unsigned long long* year_counts;      // [ry][MCR_RULE_N_COUNTS] or nullptr, accumulated into
        double* multipliers;                  // [ry][stride] or nullptr
        int64_t stride;
    };
    struct FanRuleRows {
        FanRows rows;
        unsigned long long* year_counts;
    };
    union {
        double fan_expenses[MCR_MAX_EXPENSE_FANOUT];   // the fan-out levels
        YearBins yb;
        int32_t fan_stream;                            // PHASE 10: which of the kept records (DevParams::streams) the consumer waves replace
        FanRows fan_rows;                              // PHASE 8 / 9 / 10, outcome probes (behind fan_stream's word)
        // LIST (the re-run of a screened launch, path_kernel's LIST): lane i of the launch runs local path path_list[i] for
        // i < *path_list_count, both written by screen_kernel earlier on the stream.  Such a launch reads no fan-out level.
        struct { const uint32_t* path_list; const uint32_t* path_list_count; };
        // RULE (mcr_run_rule_rng, path_kernel's RULE): the spending rule as the year's decision reads it and the rule outputs.
        // Such a launch is a plain whole-path one: it reads no fan-out level, so the block shares those bytes as well.
        RuleIO rule;
        // PHASE 11 (rule fan-out, mcr_probe_rules_rng): the outcome rows where the other outcome probes keep them, and behind them
        // the options' year counts, [fan_n][ry][MCR_RULE_N_COUNTS] or nullptr.  The rules themselves travel in the device table.
        FanRuleRows fan_rule;
    };
    // PHASE 8 / 9 / 10, joint probes (mcr_probe_*_joint_rng): [fan_n][(n_paths + 63) / 64] success masks or nullptr; consumer wave j
    // stores its 64 paths' ballot to word blockIdx.x of row j.  Last, so every other field keeps its place in the kernel arguments
    uint64_t* fan_masks;
};
static_assert(sizeof(KernelIO::YearBins) <= sizeof(double) * MCR_MAX_EXPENSE_FANOUT, "the yearly-bins block must fit the bytes it overlays");
static_assert(sizeof(KernelIO::FanRows) <= sizeof(double) * MCR_MAX_EXPENSE_FANOUT, "the outcome rows must fit the bytes they overlay");
static_assert(sizeof(KernelIO::RuleIO) <= sizeof(double) * MCR_MAX_EXPENSE_FANOUT, "the spending rule must fit the bytes it overlays");
static_assert(sizeof(KernelIO::FanRuleRows) <= sizeof(double) * MCR_MAX_EXPENSE_FANOUT && offsetof(KernelIO::FanRuleRows, rows) == 0,
              "the rule fan-out's rows must fit the bytes they overlay, the outcome rows where every outcome probe reads them");
// path_kernel(DevParams, KernelIO, const DevParams*): a field of the second argument read from the kernel-argument segment at
// the point of use (the arguments lie there in order, each at its natural alignment).  Wave-uniform: a scalar load.
constexpr size_t kKernelIOArgOffset = (sizeof(DevParams) + alignof(KernelIO) - 1) / alignof(KernelIO) * alignof(KernelIO);
template <typename T> __device__ __forceinline__ T late_arg(size_t offset_in_io) {
    typedef const char __attribute__((address_space(4)))* KernArg;
    return *(const T __attribute__((address_space(4)))*)((KernArg)__builtin_amdgcn_kernarg_segment_ptr() + kKernelIOArgOffset + offset_in_io);
}
// PHASE 6 (grid probe, mcr_probe_grid_rng): one record per grid row (blockIdx.y) of a launch, in device memory; path_kernel's
// `cand_params` points at the launch's records.  Everything a row needs is wave-uniform there: scalar loads.
struct GridCell {
    DevParams p;                                  // the row's parameter block (working_months, stream start months, horizon)
    double levels[MCR_MAX_EXPENSE_FANOUT];        // consumer wave j runs monthly_expenses = levels[j]
    uint64_t* counters;                           // level j's counters: counters + j * MCR_N_COUNTERS
    int32_t snap;                                 // the snapshot column of the row's month
    int32_t pad;
};
// PHASE 6 with RULE (rule grid probe, mcr_probe_rule_grid_rng): the row's record under a spending rule.  The grid's own record
// first, so the kernel reads the row's block, levels, counters and snapshot column where PHASE 6 reads them; behind it the rule as
// the year's decision reads it (KernelIO::RuleIO's six values, formed on the host by the two operations launch_rule performs) and
// the year counts of the row's first level of the launch: level j counts at year_counts + j * ry * MCR_RULE_N_COUNTS
struct RuleGridCell {
    GridCell cell;
    double upper, lower, keep, grow, floor, ceiling;
    unsigned long long* year_counts;              // [lg][ry][MCR_RULE_N_COUNTS] or nullptr, accumulated into
};
static_assert(offsetof(RuleGridCell, cell) == 0 && sizeof(RuleGridCell) == sizeof(GridCell) + 7 * sizeof(double),
              "RuleGridCell is GridCell, six packed doubles and a pointer");
// PHASE 8 (scenario probe, mcr_probe_scenarios_rng): consumer wave j of a launch runs record j of the launch's device table of
// mcr_scenario (initial_balance, monthly_contribution, monthly_expenses), through `cand_params` like the grid's records
static_assert(sizeof(mcr_scenario) == 3 * sizeof(double), "mcr_scenario is three packed doubles");
static_assert(sizeof(mcr_allocation_option) == 4 * sizeof(double), "mcr_allocation_option is four packed doubles: the allocation fan-out's table as it comes");
// PHASE 13 (glide probe, mcr_probe_glide_paths_rng): consumer wave j of a launch runs record j of the launch's device table, the
// caller's mcr_glide_option with first_weight replaced by the distance, in doubles, from the record ITSELF to its first weight
// (the weights stand behind the last record of the whole table): a group's launch, which gets the table at its own first record,
// finds its weights without knowing where the table began
struct GlideRecord {
    double initial_balance, monthly_contribution, monthly_expenses;
    int32_t weights;       // doubles from this record to W[0]
    int32_t n_weights;     // >= 1
};
static_assert(sizeof(mcr_glide_option) == 4 * sizeof(double) && sizeof(GlideRecord) == sizeof(mcr_glide_option) &&
              offsetof(mcr_glide_option, first_weight) == offsetof(GlideRecord, weights) && offsetof(mcr_glide_option, n_weights) == offsetof(GlideRecord, n_weights) &&
              offsetof(mcr_glide_option, monthly_expenses) == offsetof(mcr_allocation_option, monthly_expenses),
              "mcr_glide_option is 32 bytes and begins like mcr_allocation_option: the kernel reads the three amounts through either");
// PHASE 9 (assumption probe, mcr_probe_assumptions_rng): consumer wave j of a launch runs record j of the launch's device table,
// through `cand_params` as well: PHASE 8's three values and the market as growth_factors_row reads it (mcr_device.h), derived on
// the host by the function derive_params uses (derive_market)
// PHASE 10 (income probe, mcr_probe_income_rng): consumer wave j of a launch runs record j of the launch's device table, through
// `cand_params` as well: PHASE 8's three values and ONE income stream's amount and window, derived on the host by the function
// derive_params uses for a stream (derive_stream).  The stream's keep, indexed and lock_slot are the parameter block's own.
struct IncomeRecord {
    double initial_balance, monthly_contribution, monthly_expenses;
    double amount, amount_keep;
    int32_t start_month, end_month;
};
static_assert(sizeof(IncomeRecord) == 6 * sizeof(double), "IncomeRecord is five packed doubles and two months");
// PHASE 11 (rule probe, mcr_probe_rules_rng): consumer wave j of a launch runs record j of the launch's device table, through
// `cand_params` as well: PHASE 8's three values and the option's spending rule as the year's decision reads it (KernelIO::RuleIO's
// six values: keep = 1 - cut and grow = 1 + raise formed on the host by the two operations launch_rule performs)
struct RuleRecord {
    double initial_balance, monthly_contribution, monthly_expenses;
    double upper, lower, keep, grow, floor, ceiling;
};
static_assert(sizeof(RuleRecord) == 9 * sizeof(double), "RuleRecord is nine packed doubles");
// MODE 3 with RULE (rule yearly bins, mcr_run_rule_year_bins_rng): a whole-path launch, whose `cand_params` is otherwise null, reads
// ONE record there: the rule as the year's decision reads it (RuleIO's six values), the year counts, and the multiplier table with
// its edges.  KernelIO::yb stays where it is: the rule block it overlays does not exist in this launch.  Scalar loads, once.
struct RuleBinsRecord {
    double upper, lower, keep, grow, floor, ceiling;
    unsigned long long* year_counts;      // [ry][MCR_RULE_N_COUNTS] or nullptr, accumulated into
    unsigned long long* multiplier_bins;  // [ry][n_m_bins + 2] or nullptr, accumulated into
    const double* m_edges;                // [n_m_bins + 1]
    int32_t n_m_bins, pad;                // (0: the table is not requested)
};
static_assert(sizeof(RuleBinsRecord) == 10 * sizeof(double), "RuleBinsRecord is six packed doubles, three pointers and a count");
struct AssumptionRecord {
    double initial_balance, monthly_contribution, monthly_expenses;
    double a1, b1, ainf, binf_rho, binf_rho_c, aprem, bprem;
};
static_assert(sizeof(AssumptionRecord) == 10 * sizeof(double), "AssumptionRecord is ten packed doubles");
// ... and the market a consumer wave keeps of its record (growth_factors_row's MARKET); NoMarket in every other kernel
struct Market { double a1, b1, ainf, binf_rho, binf_rho_c, aprem, bprem; };
struct NoMarket {};
constexpr int kSplitVotePairs = 16;   // SPLIT: pairs of months between two stop votes of a workgroup (a power of two)
constexpr int kSnapFields = 10;   // b1 b2 c1 c2 gacc1 gacc2 infl contrib | pre_fail | Philox carry words
// Fields per lane of a time-sliced block's hand-over state in front of its lock columns: path_kernel's kSegFixedFields
// (PHASE 3 in the three output modes; PHASE 4 is count-only)
constexpr int seg_fixed_fields(int mode) { return mode >= 1 ? 14 : 9; }

// NaN OUTPUT values travel as integer bit patterns (robust against any no-NaN math assumption: the
// state machine itself never produces a NaN for valid scenarios).
// (YearsToRuin of successful paths, withdrawal rates after failure.)
constexpr unsigned long long kNanBits = 0x7ff8000000000000ull;
__device__ __forceinline__ unsigned long long f64_bits(double x) { return (unsigned long long)__double_as_longlong(x); }
__device__ __forceinline__ void store_bits(double* p, unsigned long long bits) { *reinterpret_cast<unsigned long long*>(p) = bits; }

// MODE 3 of path_kernel (yearly bins): the workgroup's LDS behind its block counters — both edge arrays, two row buffers
// [trajectory | real | wr] of 32-bit cells and the cells of final_success_bins
struct YearBinsLds {
    double* edges; double* wedges;       // [n + 1], [wn + 1]
    unsigned int* buf; unsigned int* fin;  // [2][row], [cells]
    int n, wn, cells, wcells, row;       // row = 2 cells + wcells
};
// per-thread state of the form: the LDS plan, rows binned so far (picks the row buffer), and the value of row T - 1 where the
// terminal partial period writes that row a second time (the row is binned once, after it)
struct YearBinsState { YearBinsLds L; int k; double last; };
struct NoYearBins {};
// ... under a spending rule (RULE): a fourth segment of the row, [trajectory | real | wr | multiplier], with its edges behind the
// withdrawal-rate ones, and the launch's rule (FanRule, below: the year's decision is rule_year_from's statements)
struct YearBinsLdsRule : YearBinsLds {
    double* medges;                      // [mn + 1]
    unsigned long long* mbins;           // the global table, [ry][mcells], or nullptr
    int mn, mcells;
};
__device__ __forceinline__ YearBinsLds year_bins_lds(const KernelIO::YearBins& yb, unsigned int* after_blk) {
    YearBinsLds L;
    L.n = yb.n_bins; L.wn = yb.n_wr_bins;
    L.cells = L.n + 2; L.wcells = L.wn + 2; L.row = 2 * L.cells + L.wcells;
    L.edges = reinterpret_cast<double*>((reinterpret_cast<uintptr_t>(after_blk) + 7u) & ~(uintptr_t)7u);
    L.wedges = L.edges + (L.n + 1);
    L.buf = reinterpret_cast<unsigned int*>(L.wedges + (L.wn + 1));
    L.fin = L.buf + 2 * L.row;
    return L;
}
// (the plan by the type of the state's L: the plain form's is the function above, and its code is what it was)
__device__ __forceinline__ void year_bins_plan(YearBinsLds& L, const KernelIO::YearBins& yb, const void*, unsigned int* after_blk) { L = year_bins_lds(yb, after_blk); }
__device__ __forceinline__ void year_bins_plan(YearBinsLdsRule& L, const KernelIO::YearBins& yb, const void* record, unsigned int* after_blk) {
    const RuleBinsRecord* const rec = static_cast<const RuleBinsRecord*>(record);
    static_cast<YearBinsLds&>(L) = year_bins_lds(yb, after_blk);
    L.mn = rec->n_m_bins; L.mcells = L.mn + 2; L.mbins = rec->multiplier_bins;
    L.medges = L.wedges + (L.wn + 1);
    L.buf = reinterpret_cast<unsigned int*>(L.medges + (L.mn + 1));
    L.row = 2 * L.cells + L.wcells + L.mcells;
    L.fin = L.buf + 2 * L.row;
}
__device__ __forceinline__ void year_bins_load_m_edges(const YearBinsLds&, const void*, int, int) {}
__device__ __forceinline__ void year_bins_load_m_edges(const YearBinsLdsRule& L, const void* record, int thread, int n_threads) {
    const double* const e = static_cast<const RuleBinsRecord*>(record)->m_edges;
    if (L.mn > 0) for (int k = thread; k <= L.mn; k += n_threads) L.medges[k] = e[k];
}
// where cell c of a flushed row goes when it lies in the multiplier segment (nothing in the plain form: its row ends before it)
__device__ __forceinline__ void year_bins_m_dst(const YearBinsLds&, int, int, unsigned long long*&) {}
__device__ __forceinline__ void year_bins_m_dst(const YearBinsLdsRule& L, int y, int c, unsigned long long*& dst) {
    const int c0 = 2 * L.cells + L.wcells;
    if (c >= c0) dst = (y >= 0 && L.mbins) ? L.mbins + (size_t)y * L.mcells + (c - c0) : nullptr;
}
// the cell of x in a row of n bins: 0 below e[0], n + 1 above e[n], else 1 + np.histogram's bin (the last one closed)
__device__ __forceinline__ int year_bins_cell(const double* e, int n, double x) {
    if (x < e[0]) return 0;
    if (x > e[n]) return n + 1;
    int lo = 0, hi = n;                  // e[lo] <= x and (hi == n or x < e[hi])
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (e[mid] <= x) lo = mid; else hi = mid;
    }
    return lo + 1;
}
// One row of the tables; call k of the workgroup (every thread makes the same calls: one barrier each).  nominal / px go to row t
// of trajectory_bins / real_trajectory_bins (has_sample), wr_bits (NaN: not counted) to row y of wr_bins (y < 0: none).
template <typename LDS>
__device__ __forceinline__ void year_bins_row(const KernelIO::YearBins& yb, const LDS& L, int k, bool valid, int t, bool has_sample,
                                              double nominal, double px, int y, unsigned long long wr_bits) {
    unsigned int* const b = L.buf + (k & 1) * L.row;
    if (valid) {
        if (has_sample) {
            if (yb.trajectory) atomicAdd(&b[year_bins_cell(L.edges, L.n, nominal)], 1u);
            if (yb.real_trajectory) atomicAdd(&b[L.cells + year_bins_cell(L.edges, L.n, px > kEps ? nominal / px : 0.0)], 1u);
        }
        if (y >= 0 && yb.wr && wr_bits != kNanBits)
            atomicAdd(&b[2 * L.cells + year_bins_cell(L.wedges, L.wn, __longlong_as_double((long long)wr_bits))], 1u);
    }
    __syncthreads();
    for (int c0 = 0; c0 < L.row; c0 += kBlock) {      // (wave-uniform trip count: the ballot below)
        const int c = c0 + (int)threadIdx.x;
        const unsigned int v = c < L.row ? b[c] : 0u;
        if (__builtin_amdgcn_ballot_w64(v != 0u) == 0ull) continue;    // an all-zero group of 64 cells
        if (c >= L.row) continue;
        if (v) b[c] = 0u;
        unsigned long long* dst = nullptr;
        if (c < L.cells) dst = yb.trajectory ? yb.trajectory + (size_t)t * L.cells + c : nullptr;
        else if (c < 2 * L.cells) dst = yb.real_trajectory ? yb.real_trajectory + (size_t)t * L.cells + (c - L.cells) : nullptr;
        else if (y >= 0 && yb.wr) dst = yb.wr + (size_t)y * L.wcells + (c - 2 * L.cells);
        year_bins_m_dst(L, y, c, dst);
        // every lane of the group adds, zeros included: consecutive cells, contiguous 8-byte atomics.  Adding only the non-zero
        // cells measured the same (LABNOTES R10: 6.33 / 6.47 ms against 6.30 / 6.51 at 64 / 256 bins)
        if (dst) atomicAdd(dst, (unsigned long long)v);
    }
}
__device__ __forceinline__ void year_bins_flush_final(const KernelIO::YearBins& yb, const YearBinsLds& L) {   // (behind a barrier)
    if (!yb.final_success) return;
    for (int c0 = 0; c0 < L.cells; c0 += kBlock) {
        const int c = c0 + (int)threadIdx.x;
        const unsigned int v = c < L.cells ? L.fin[c] : 0u;
        if (__builtin_amdgcn_ballot_w64(v != 0u) == 0ull) continue;
        if (c < L.cells) atomicAdd(yb.final_success + c, (unsigned long long)v);
    }
}

// Resident waves per SIMD are worth more than a few spilled registers: the trimmed count-only kernel loses 4.4 % on
// large batches at 4 instead of 6 workgroups per CU (measured with a larger LDS footprint, LABNOTES.md rounds 1-3 section 9), and the Philox
// variants with per-path outputs gain 4.5 % (summary) / 3 % (trajectories) at 5 waves (<= 96 VGPRs, 4-10 of them
// spilled) over 4 (up to 128); at 6 the summary variant spills too much and gives that back.  The NumPy-stream and
// injection variants keep 4 (they need 107-128).  The count-only Philox
// variants are held to 6 waves per SIMD (<= 80 VGPRs): the BASELINE workload of 1e6 paths is 15.26 waves per SIMD, and
// with 5 resident waves that is 5 + 5 + 5 + a lone fourth round (+9 %, LABNOTES.md rounds 1-3 section 5); the annual-tax variant sat at 81.
// INJ = true: shocks come from io.injected (the parity hook) instead of the RNG; only instantiated with MODE 2
// (every output is null-checked), so the hot variants carry neither the injection branches nor their registers.
// PHASE 0: the whole path.  PHASE 1 / 2 split it at retirement for the search (simulation.py:1180-1194 re-simulates the
// accumulation months for every probed candidate although, under common random numbers, they do not depend on it,
// :513-579): PHASE 1 runs the accumulation once to the largest candidate and stores the state at the end of every
// candidate month; PHASE 2 (grid.y = candidate) resumes each candidate's decumulation from its snapshot.
// SPLIT = true (count-only Philox variants; launches that leave SIMDs idle — a lone 50 000-path search probe is 782
// wavefronts on 1 024 SIMDs and runs at ~12 cycles per instruction, latency-bound): the workgroup has 2 x kBlock threads
// for its kBlock paths.  Threads kBlock .. 2 kBlock - 1 are PRODUCERS: they run growth_rows2 (Philox, Box-Muller, exp) one
// pair of months ahead into a double-buffered stage; threads 0 .. kBlock - 1 are CONSUMERS: the state machine.  The two
// halves of a month's dependency chain then run on different SIMDs of the CU.  One workgroup barrier per pair of months
// hands a buffer over; every wave executes the same number of them (no early exit when all lanes have failed) or has
// terminated.  The arithmetic of every path is unchanged: counts are bit-identical to SPLIT = false.
// PHASE 3 (Philox launches of a few rounds of workgroups, any output mode; launch_paths): TIME-SLICED path blocks.  A launch of B
// equal workgroups on W resident slots ends when the busiest slot has run ceil(B / W) of them: 10^6 paths are 15.26 workgroups
// per CU-slot, so the chip idles through most of a sixteenth round (measured: 5.15 ms where 4.77 would do, LABNOTES R4.6).
// Small work items at the END of the dispatch order fix that (longest-processing-time-first): the first S path blocks of the
// launch are cut into Q segments at retirement-year boundaries, and the grid is ordered [segment 0 of the S blocks] [the
// other blocks, whole] [segment 1 x S] ... [segment Q - 1 x S].  A segment ends by storing its lanes' state (balances, bases,
// gain accumulators, price level, flags, Philox carry, lock columns) and raising a flag; its successor — dispatched at least
// S workgroups later, i.e. after it has long finished — loads it.  A successor that does not see the flag within a bounded
// number of polls recomputes the block from month 0 itself: no workgroup ever waits on another one to make progress.  Such a
// segment does not write the hand-over state (flag 2, not 1), and its successors recompute too: one writer per slot at a time.
// The arithmetic of every path is unchanged: counts and bins are bit-identical to PHASE 0.
// XS = true ("extended streams"): the variants that can read income-stream records beyond the by-value block from the device
// table and keep lock slots beyond the LDS budget in the global overflow block (DevParams::extra_streams / lock_overflow:
// other_income_streams has no length limit in the reference, config.py:99).  A compile-time variant because the headline
// kernels have no SGPR to spare for the two extra tests a month; instantiated for the generic tax form only (TAXED = 3,
// ANNUAL = true: exact zeros for a zero rate, like the NumPy-stream variants).
// PHASE 5 (SPLIT = true; mcr_probe_expenses_rng): EXPENSE FAN-OUT.  The workgroup covers ONE 64-path block with 64 (L + 1)
// threads: the last wave is the producer (the SPLIT producer, resumed like PHASE 2 from the single PHASE 1 snapshot), waves
// 0 .. L - 1 are consumers that all resume the same 64 paths from that snapshot and run the retirement months with their own
// wave-uniform monthly_expenses = io.fan_expenses[j].  The factors a producer stages once feed L months, so the random-number
// half of the month (growth_rows2, ~64 % of its cost) is shared by L spending levels.  Every consumer wave executes the
// barriers of PHASE 2's SPLIT consumers (same row range, same vote schedule); each keeps its own lock columns in LDS and its
// own success count (blk[j]).  The month is the issue-bound one (MM, WAVE-UNIFORM fix-ups): counts are bit-identical to a
// count-only launch with monthly_expenses = fan_expenses[j].
// PHASE 6 (SPLIT = true; mcr_probe_grid_rng): GRID FAN-OUT = PHASE 5 with grid.y = grid row (a working month and its own
// levels).  Same workgroup shape, barriers and votes; the row's record (GridCell, through `cand_params`) holds its parameter
// block (as in PHASE 2), its snapshot column of a PHASE 1 sweep that stored every distinct month, its levels and its counters.
// PHASE 7 (SPLIT = true; mcr_probe_contributions_rng): CONTRIBUTION FAN-OUT = PHASE 5's workgroup over the WHOLE path.  The
// levels differ from month 0 (contributions enter every accumulation month), so there is no snapshot to share: the producer
// wave stages rows [0, total_months) from a zero Philox carry (PHASE 0's SPLIT producer), and consumer wave j starts from
// the initial state with its own wave-uniform monthly_contribution = io.fan_expenses[j], runs the accumulation and then the
// retirement months with the scenario's own monthly_expenses.  Consumers execute the barriers and votes of PHASE 0's SPLIT
// consumers over rows 0 .. total_months - 1; lock columns and success counts per level as in PHASE 5.  The month is the
// issue-bound one (MM): counts are bit-identical to a count-only launch with monthly_contribution = fan_expenses[j].
// PHASE 8 (SPLIT = true; mcr_probe_scenarios_rng): SCENARIO FAN-OUT = PHASE 7's workgroup, barriers and votes, with three
// wave-uniform values per consumer wave instead of one: wave j starts from its own initial_balance (the two operations of
// the plain initial state, in their order), contributes its own monthly_contribution and spends its own monthly_expenses.
// The launch's records are a device table of mcr_scenario behind `cand_params` (scalar loads, as PHASE 6 reads its GridCell).
// Counts are bit-identical to a count-only launch with the three fields of the parameter block replaced by record j.
// PHASE 9 (SPLIT = true; mcr_probe_assumptions_rng): ASSUMPTION FAN-OUT = PHASE 8's workgroup, barriers and votes, with the
// MARKET per consumer wave as well.  The market enters a month only in the last third of growth_rows2 (x = a + b z and the three
// exps); the Philox rounds and the Box-Muller radius and angle depend on the path alone.  So the producer stages the PARTS of the
// pair's six normals (growth_parts2: nine doubles per lane instead of six factors; the stage is 2 x 9 x 64 doubles), and consumer
// wave j computes its own three factors from them with its record's a1, b1, ainf, binf_rho, binf_rho_c, aprem, bprem — the
// operations of growth_rows2_form in their order (growth_factors_row) — then runs PHASE 8's month.  The seven values sit in
// VGPRs: the fan-out kernels have no SGPRs to spare.  Counts are bit-identical to a count-only launch with the ten fields of
// the parameter block replaced by record j.
// PHASE 10 (SPLIT = true; mcr_probe_income_rng): INCOME FAN-OUT = PHASE 8's workgroup, barriers and votes, with ONE INCOME STREAM
// per consumer wave as well: claim ages, annuity sizes, bridge-job lengths over the same random numbers.  The launch's records are
// a device table of IncomeRecord behind `cand_params` (scalar loads): PHASE 8's three values, and the netted amount and the window
// [start_month, end_month) of kept record io.fan_stream of the parameter block, derived on the host by the code derive_params
// runs for a stream.  The record keeps its LIST POSITION (the tolerance month subtracts the streams in list order, one FMA or one
// subtraction each: the order is part of the bits): kept record 0 or 1 lives in S0 / S1, which the wave sets from its record
// once; a later one is substituted at its wave-uniform index of the stream loop (four scalar moves under a scalar compare).  Its keep, indexed
// and lock_slot stay the block's own, so every consumer wave has the same lock-column layout, and each wave has its own columns:
// the first-active-month store works per wave unchanged.  The host always hands the kernel the probed stream, also when the
// list's own amount is 0; a record with amount 0 then subtracts an exact zero, as the plain launch that drops it.  Counts are
// bit-identical to a count-only launch with the six fields replaced by record j.
// PHASE 11 (SPLIT = true, RULE = true; mcr_probe_rules_rng): RULE FAN-OUT = PHASE 8's workgroup, barriers and votes, with a SPENDING
// RULE per consumer wave as well: which guardrail, over the same random numbers.  The launch's records are a device table of
// RuleRecord behind `cand_params` (scalar loads): PHASE 8's three values and the rule as the year's decision reads it.  The lanes
// carry the rule launch's RuleState through its overloads; the year's decision and ballots are rule_year_from on the wave's own
// FanRule (its six values and option j's table of the launch's year counts), the month spends (scn_expenses m) price.  No
// multiplier rows.  Mask 3 only, like the rule launch.  Counts and year counts are bit-identical to a count-only rule launch
// with the three fields replaced by record j under record j's rule.
// PHASE 6 with RULE (mcr_probe_rule_grid_rng): RULE GRID FAN-OUT = PHASE 6's workgroup, snapshots, barriers and votes under ONE
// spending rule: how much sooner can I retire if I accept the guardrail?  A rule acts only after retirement, so a row resumes
// from its snapshot column exactly as PHASE 6 does; the row's record is RuleGridCell (the grid's record, the rule, the row's year
// counts).  The lanes carry the rule launch's RuleState from the resumed balance and price level; the year's decision and ballots
// are rule_year_from on the wave's own FanRule, as in PHASE 11; the month spends (levels[j] m) price.  No multiplier rows.  Mask 3
// only, like every rule kernel.  Counts and year counts are bit-identical to a count-only rule launch at the row's month with
// monthly_expenses = levels[j].
// EXACT = true: the month in its exact-rounding forms (mcr_device.h) instead of the tolerance form — for configurations whose
// realized-gains rate lets the reference's denominator clamps bind (DevParams::exact_month), instantiated for the generic XS
// variants only; -DMCR_K1_EXACT_MONTH builds a library that runs every variant that way (A/B).
#ifdef MCR_K1_EXACT_MONTH
constexpr bool kExactMonthDefault = true;
#else
constexpr bool kExactMonthDefault = false;
#endif
// -DMCR_K1_GENERAL_MONTH (tests only: tests/test_gpu_month_fast_path.py) builds a library whose tolerance month always takes the
// lane-masked fix-ups: the reference the wave-uniform form is compared with, bit for bit.
#ifdef MCR_K1_GENERAL_MONTH
constexpr bool kUniformFixups = false;
#else
constexpr bool kUniformFixups = true;
#endif
// Scalar month counters of the kernels that have growth, month and stream forms (kScalarCounters in path_kernel): the month's
// wave-uniform bookkeeping in running scalars instead of a multiply, a modulo and a compare chain a month.  Every other kernel
// holds the empty object and the expressions it always had (the overloads below), so that its code is what it was.
//   row: the row of the retirement month that comes up next; moy: the accumulation month of the year, 1 .. 12;
//   ye_mi: the month mi of a retirement year in which a year of the plan ends, (wm + mi + 1) % 12 == 0;
//   prio_next: the next row at which the wave's priority falls (rows come up in order, so one compare a month is enough).
struct MonthCounters { int prio_next, row, moy, ye_mi; };
struct NoMonthCounters {};
struct NoHistoryCursor {};
// (each call site passes the one value its variant reads, chosen by a constant condition: the other is not even evaluated)
__device__ __forceinline__ bool year_opens(const MonthCounters& c, int) { return c.moy == 1; }
__device__ __forceinline__ bool year_opens(const NoMonthCounters&, int months_done) { return months_done % kMPY == 0; }
__device__ __forceinline__ bool year_closes(const MonthCounters& c, int) { return c.moy == kMPY; }
__device__ __forceinline__ bool year_closes(const NoMonthCounters&, int m) { return m % kMPY == 0; }
__device__ __forceinline__ int month_row(const MonthCounters& c, int) { return c.row; }
__device__ __forceinline__ int month_row(const NoMonthCounters&, int row) { return row; }
// the first of the ascending thresholds t1 <= t2 <= t3 that is >= r
__device__ __forceinline__ int prio_from(int t1, int t2, int t3, int r) { return t1 >= r ? t1 : t2 >= r ? t2 : t3 >= r ? t3 : INT32_MAX; }
// Stream form kStreamsInRegs: the netted amounts of the launch's (at most two) indexed records, and each window as its first
// ROW (start + wm, saturated) and its length in months — the month tests (unsigned)(row - first) < length
struct StreamRegs { double a0, a1; int s0, s1; unsigned n0, n1; };
struct NoStreamRegs {};
// OUT (outcome probes): the lane's month of failure, for the years_to_ruin row
struct RuinMonth { int month; };
struct NoRuinMonth {};
// PHASE 10: what a consumer wave keeps of its record's stream, and which of the kept records (DevParams::streams) it replaces
struct IncomeRegs { double amount, amount_keep; int32_t start_month, end_month; int k; };
struct NoIncomeRegs {};
// RULE (mcr_run_rule_rng): the lane's spending multiplier m, r0 = B0 / P0 and whether the rule applies to the path at all
struct RuleState { double m, r0; bool on; };
struct NoRuleState {};
// (the one value the month reads of it, chosen by overload like the month counters': every other kernel's expression is what it was)
__device__ __forceinline__ double rule_scaled(const RuleState& r, double e) { return e * r.m; }
__device__ __forceinline__ double rule_scaled(const NoRuleState&, double e) { return e; }
// At retirement: m = 1; the rule is inert (m stays 1) for a path that starts retirement with B0 <= 1e-6.  One IEEE division a
// path, none in the year loop.
__device__ __forceinline__ void rule_begin(RuleState& r, double start_balance, double infl_ret) {
    r.m = 1.0; r.on = start_balance > kEps; r.r0 = r.on ? start_balance / infl_ret : 0.0;
}
__device__ __forceinline__ void rule_begin(NoRuleState&, double, double) {}
// Top of retirement year `year` (the whole wave is here).  The year's decision (include/mcr.h, mcr_spending_rule): B = b1 + b2
// and P = infl are the yearly sample and its price level at the end of the year before.  q > upper  <=>  (m r0) P > upper B,
// q < lower  <=>  (m r0) P < lower B (B >= 0; upper >= lower, so at most one holds): multiplies, two compares and selects, no
// lane-divergent branch.  Lanes that do not begin the year keep their m: it is never read again.  Then the year's four counts,
// wave ballots whose popcounts one lane adds with 64-bit vector atomics (zero counts skipped), and the multiplier row: the
// lane's m, NaN (as a bit pattern) for a year the path does not begin.
// The rule and its outputs come from a SOURCE R: KernelIO::RuleIO, the launch's one rule in the kernel arguments (the plain rule
// launch, rule_year below), or FanRule, a consumer wave's own rule and year counts (the rule fan-out, PHASE 11).
template <typename SRC>
__device__ __forceinline__ void rule_year_from(RuleState& r, const SRC& R, int year, bool valid, bool alive, double b1, double b2, double infl, uint64_t li) {
    if (year >= 1) {                                             // (wave-uniform)
        const double B = b1 + b2;
        const double lhs = (r.m * r.r0) * infl;
        const bool go = alive && r.on;
        const bool cut = go && lhs > R.upper * B;
        const bool up = go && lhs < R.lower * B;
        const double m_cut = fmax(R.floor, r.m * R.keep);
        const double m_up = fmin(R.ceiling, r.m * R.grow);
        r.m = cut ? m_cut : up ? m_up : r.m;
    }
    const bool begun = valid && alive;
    const unsigned long long n_alive = __builtin_amdgcn_ballot_w64(begun);
    const unsigned long long n_cut = __builtin_amdgcn_ballot_w64(begun && r.m < 1.0);
    const unsigned long long n_floor = __builtin_amdgcn_ballot_w64(begun && R.floor < 1.0 && r.m <= R.floor);
    const unsigned long long n_up = __builtin_amdgcn_ballot_w64(begun && r.m > 1.0);
    unsigned long long* const yc = R.year_counts;
    if (yc && (threadIdx.x & 63) == 0) {
        unsigned long long* const c = yc + (size_t)year * MCR_RULE_N_COUNTS;
        if (n_alive) atomicAdd(&c[MCR_RULE_ALIVE], (unsigned long long)__popcll(n_alive));
        if (n_cut) atomicAdd(&c[MCR_RULE_CUT], (unsigned long long)__popcll(n_cut));
        if (n_floor) atomicAdd(&c[MCR_RULE_FLOOR], (unsigned long long)__popcll(n_floor));
        if (n_up) atomicAdd(&c[MCR_RULE_RAISED], (unsigned long long)__popcll(n_up));
    }
    if (R.multipliers && valid) store_bits(&R.multipliers[(int64_t)year * R.stride + (int64_t)li], alive ? f64_bits(r.m) : kNanBits);
}
template <typename IO>
__device__ __forceinline__ void rule_year(RuleState& r, const IO& io, int year, bool valid, bool alive, double b1, double b2, double infl, uint64_t li) {
    rule_year_from(r, io.rule, year, valid, alive, b1, b2, infl, li);
}
// PHASE 11: what a consumer wave keeps of its record's rule (wave-uniform values), and its option's year counts.  The form
// writes no multiplier rows: the null pointer is a constant, and rule_year_from's store is not compiled.
struct FanRule {
    double upper, lower, keep, grow, floor, ceiling;
    unsigned long long* year_counts;
    static constexpr double* multipliers = nullptr;
    static constexpr int64_t stride = 0;
};
struct NoFanRule {};
// MODE 3 with RULE: the yearly-bins state with the launch's rule, and the top of a retirement year: rule_year_from's decision and
// counts on that rule, then the lane's m into the multiplier segment of the row buffer the year's own year_bins_row call (call
// B.k, at the end of this year or in the pad loop) flushes behind its barrier.  The thread has passed barrier B.k - 1, behind
// which every wave had flushed that buffer's row B.k - 2: the binning needs no barrier of its own.
struct YearBinsRuleState { YearBinsLdsRule L; int k; double last; FanRule R; };
__device__ __forceinline__ void rule_year_binned(RuleState& r, const YearBinsRuleState& B, int year, bool valid, bool alive, double b1, double b2, double infl, uint64_t li) {
    rule_year_from(r, B.R, year, valid, alive, b1, b2, infl, li);
    if (B.L.mbins && valid && alive)
        atomicAdd(&B.L.buf[(B.k & 1) * B.L.row + 2 * B.L.cells + B.L.wcells + year_bins_cell(B.L.medges, B.L.mn, r.m)], 1u);
}
__device__ __forceinline__ void rule_bins_begin(YearBinsRuleState& B, const void* record) {
    const RuleBinsRecord* const rec = static_cast<const RuleBinsRecord*>(record);
    B.R.upper = rec->upper; B.R.lower = rec->lower; B.R.keep = rec->keep; B.R.grow = rec->grow; B.R.floor = rec->floor; B.R.ceiling = rec->ceiling;
    B.R.year_counts = rec->year_counts;
}
__device__ __forceinline__ void rule_bins_begin(YearBinsState&, const void*) {}
template <typename IO>
__device__ __forceinline__ void rule_year(NoRuleState&, const IO&, int, bool, bool, double, double, double, uint64_t) {}
// a year the whole wave does not begin (the pad loop): NaN in the multiplier row
template <typename IO>
__device__ __forceinline__ void rule_pad(const RuleState&, const IO& io, int year, bool valid, uint64_t li) {
    if (io.rule.multipliers && valid) store_bits(&io.rule.multipliers[(int64_t)year * io.rule.stride + (int64_t)li], kNanBits);
}
template <typename IO>
__device__ __forceinline__ void rule_pad(const NoRuleState&, const IO&, int, bool, uint64_t) {}
__device__ __forceinline__ void income_put(DevStream& S, const IncomeRegs& R) {
    S.amount = R.amount; S.amount_keep = R.amount_keep; S.start_month = R.start_month; S.end_month = R.end_month;
}

template <int MODE, int RNG, int TAXED, bool ANNUAL, bool INJ = false, int PHASE = 0, bool SPLIT = false, bool XS = false, bool EXACT = kExactMonthDefault, int GF = 0, int MF = 0, int SF = 0, bool OUT = false, bool LIST = false, int NPROD = 1, bool RULE = false, bool GLIDE = false>
__global__ __launch_bounds__((PHASE == 5 || PHASE == 6 || PHASE == 7 || PHASE == 8 || PHASE == 9 || PHASE == 10 || PHASE == 11 || PHASE == 12 || PHASE == 13) ? 64 * (MCR_MAX_EXPENSE_FANOUT + 1) : NPROD == 2 ? 3 * 64 : SPLIT ? 2 * kBlock : kBlock, SPLIT ? 4 : (MODE == 0 && RNG == 0 && (PHASE == 0 || PHASE == 3 || PHASE == 4)) ? 6 : ((MODE == 1 || MODE == 2) && RNG == 0 && !INJ) ? 5 : 4) void path_kernel(const DevParams P_arg, const KernelIO io,
                                                         const DevParams* __restrict__ cand_params) {
    // MODE 3 (mcr_run_year_bins_rng): YEARLY BINS.  The arithmetic of MODE 2, but wherever that variant stores a yearly sample
    // (nominal balance, real balance, withdrawal rate) the lane bins it instead: cell 0 = below edges[0], cells 1 .. n = the
    // bins of np.histogram(row, bins=edges), cell n + 1 = above edges[n].  A row of a table is accumulated by the WORKGROUP in
    // LDS (32-bit cells, ds atomics) and flushed once: after one barrier every wave adds its 64-cell groups of the row to the
    // global table with contiguous 64-bit atomic adds, skipping groups that are all zero.  Two row buffers alternate, so one
    // barrier per row is enough (a buffer is binned into again two rows later, i.e. behind the NEXT row's barrier, which every
    // wave passes after its own flush).  Every wave of the workgroup executes the same number of barriers: it visits every row
    // exactly once, in the year loop or, once all its lanes have failed, in the pad loop.  The row the trajectory variant writes
    // twice (the terminal partial period overwrites row T - 1 of successful paths) is binned once, after the settlement, with
    // the value that variant leaves in memory.  The edges live in LDS (two 8-step searches per path-year are dependent reads).
    // Held to 4 waves per SIMD (<= 128 VGPRs): no scratch.
    static_assert(MODE != 3 || (PHASE == 0 && !SPLIT && !INJ), "the yearly-bins form is a whole-path launch on the engine's own streams");
    static_assert(!SPLIT || (MODE == 0 && RNG == 0 && !INJ), "the producer / consumer split exists for the count-only Philox variants");
    static_assert(!XS || (PHASE == 0 && !SPLIT && TAXED == 3 && ANNUAL), "extended stream lists run the generic whole-path form");
    static_assert(PHASE != 5 || SPLIT, "the expense fan-out is a producer / consumer form");
    static_assert(PHASE != 6 || SPLIT, "the grid fan-out is a producer / consumer form");
    static_assert(PHASE != 7 || SPLIT, "the contribution fan-out is a producer / consumer form");
    static_assert(PHASE != 8 || SPLIT, "the scenario fan-out is a producer / consumer form");
    static_assert(PHASE != 9 || SPLIT, "the assumption fan-out is a producer / consumer form");
    static_assert(PHASE != 10 || SPLIT, "the income fan-out is a producer / consumer form");
    static_assert(PHASE != 11 || (SPLIT && RULE), "the rule fan-out is a producer / consumer form of the rule kernels");
    static_assert(PHASE != 12 || SPLIT, "the allocation fan-out is a producer / consumer form");
    static_assert(PHASE != 13 || SPLIT, "the glide fan-out is a producer / consumer form");
    // OUT (mcr_probe_*_outcomes_rng): the PHASE 8 / 9 / 10 consumer waves also store their paths' outcome rows (KernelIO::fan_final,
    // fan_ruin) in the epilogue.  A template flag, not a null check: the month of failure is one more VGPR through the month loop,
    // which the plain and the joint probes' kernels do not pay.
    static_assert(!OUT || PHASE == 8 || PHASE == 9 || PHASE == 10 || PHASE == 11 || PHASE == 12 || PHASE == 13, "outcome rows exist for the scenario, assumption, income, rule, allocation and glide fan-outs");
    // LIST (the re-run of a screened launch; launch_screened): the lanes' local path indices come from a device list that
    // screen_kernel filled earlier on the stream, io.path_list[i] for i < *io.path_list_count; lanes beyond the count behave
    // like tail lanes, and a workgroup whose first index is at or beyond the count returns at once (the host sizes the grid
    // from a bound: it cannot read the count without a synchronisation).  Last, with a default: every other instantiation
    // keeps its instruction stream.
    static_assert(!LIST || (MODE == 0 && RNG == (int)MCR_RNG_PHILOX && !ANNUAL && !INJ && PHASE == 0 && !XS), "path lists exist for the whole-path count-only Philox launches, split or not");
    // The split LIST kernels (either NPROD) run in the launch's stream and month forms: screen_qualified gives every screened
    // launch kStreamsInRegs, so the consumer fills StreamRegs once (the producers have returned by then) and its month tests
    // two windows against wm + rmi; MF follows month_form_qualified; and the month is the straight-line one (MM below).  Re-run
    // of 10^6 config.json paths, 256-path form 0.588 -> 0.515 ms, 64-path form 0.498 -> 0.456 ms (LABNOTES R30).
    // NPROD = 2 (the re-run of a screened launch whose expected list is at most kRerunTwoProducersMaxList paths, or MCR_K1_RERUN_PRODUCERS=2): the SPLIT form
    // on ONE 64-path block per workgroup, one consumer wave and TWO producer waves (192 threads).  A short list then spreads
    // over every CU, about a wave to a SIMD, and the consumer no longer waits for its producer: producer 0 stages every HALF 0
    // of the path, producer 1 every HALF 1 (growth_rows2_own_half), each with two barrier intervals for its pair.  The stage
    // is the SPLIT form's two pair buffers (6 KB at 64 columns: a producer keeps its pair in registers until barrier p - 1
    // and stores behind it, so one buffer is being read and one written at any time).  Barriers: pair p is handed over at barrier p, which every wave of
    // the workgroup executes — the consumer in begin_month of row 2 p, the producer of pair p behind its stores, the other
    // producer in the middle of pair p + 1 (between the parts and the factors).  The votes are PHASE 0's.  Every staged
    // factor is the SPLIT form's.  The chain that is left is the consumer's own, so its month is the fan-out consumers' one
    // (MM, WAVE-UNIFORM fix-ups: straight-line code where the SPLIT month branches on lane masks; re-run of 10^6 config.json
    // paths 0.548 -> 0.503 ms on a development tree, LABNOTES R25), bit for bit the same counts.  Last, with a default, like LIST.
    static_assert(NPROD == 1 || (NPROD == 2 && SPLIT && LIST), "two producers exist for the split re-run of a screened launch");
    // RULE (mcr_run_rule_rng; the guardrail spending rule of include/mcr.h): every lane carries a spending multiplier m (1 in
    // retirement year 0) that scales the month's base expenses, (monthly_expenses m) price, and is decided again at the top of
    // every retirement year y >= 1 from the balance and the price level the year starts with.  The decision is a handful of
    // fp64 multiplies, two compares and selects: no lane-divergent branch.  The year's four counts are wave ballots, added by
    // one lane; the optional multiplier row is one 512-byte wave store a year.  Last, with a default: everything it adds stands
    // in overloads on the state object RS (rule_begin, rule_year, rule_pad, rule_scaled: empty for every other kernel's empty
    // object, like the month counters' helpers), and every other instantiation keeps its registers.  (The same statements
    // written in place under `if constexpr (RULE)` cost the time-sliced trajectory kernels, which never run them, one or two
    // spilled SGPRs each.)
    static_assert(!RULE || (RNG == (int)MCR_RNG_PHILOX && TAXED == 3 && !INJ && !XS && EXACT == kExactMonthDefault && GF == 0 && MF == 0 && SF == 0 && !LIST && NPROD == 1 &&
                            (((MODE == 0 || MODE == 1 || MODE == 3) && PHASE == 0 && !SPLIT && !OUT) || (MODE == 0 && PHASE == 11 && SPLIT) || (MODE == 0 && PHASE == 6 && SPLIT && !OUT))),
                  "the spending rule exists for the plain whole-path Philox launches, count-only, summary and yearly bins, and for the rule and the rule grid fan-outs, on the generic tax mask");
    // GLIDE (mcr_run_glide_rng, mcr_run_glide_year_bins_rng; include/mcr.h: GLIDE PATH): the plain whole-path launch whose split
    // between the assets follows a table W[0 .. n - 1] by calendar year.  Every wave of a launch stands in the same row, so the
    // weight in force is launch-uniform: PHASE 13's statement (WaveGlideParams, glide_row) with ONE record for the whole launch,
    // behind `cand_params`, which is otherwise null on a whole-path launch (MODE 3 with RULE reads its one record the same way).
    // Every read of a weight on the path is the row's: the initial split, the contribution split, the rebalance, the dust
    // sub-case, the annual tax with its closing rebalance, and the terminal settlement on the last row's.  A wave that leaves the
    // year loop because all its lanes have failed never reads the weight again (the pad loop bins zeros; the settlement runs for
    // lanes that succeeded).  Last, with a default, like RULE: every other instantiation keeps its instruction stream.
    static_assert(!GLIDE || (RNG == (int)MCR_RNG_PHILOX && TAXED == 3 && !INJ && !XS && EXACT == kExactMonthDefault && GF == 0 && MF == 0 && SF == 0 && !LIST && NPROD == 1 &&
                             !RULE && !OUT && (MODE == 0 || MODE == 1 || MODE == 3) && PHASE == 0 && !SPLIT),
                  "the glide path exists for the plain whole-path Philox launches, count-only, summary and yearly bins, on the generic tax mask");
    // PHASE 4 = PHASE 2 (a candidate's decumulation resumed from its accumulation snapshot) time-sliced like PHASE 3: the
    // 17-month verification window of the search is 17 x 196 workgroups = 2.17 rounds of the resident slots.
    constexpr bool kExpFan = PHASE == 5 || PHASE == 6;    // expense fan-out: the levels are monthly_expenses, resumed at retirement
    constexpr bool kConFan = PHASE == 7;                  // contribution fan-out: the levels are monthly_contribution, the whole path
    constexpr bool kAsmFan = PHASE == 9;                  // assumption fan-out: the scenario fan-out with the market per wave as well
    constexpr bool kStreamRegs = SPLIT && !kAsmFan && !(LIST && (SF & kStreamsInRegs) != 0);   // the first two income streams stay in SGPRs for the whole launch (S0, S1 below; the split re-run's stream form keeps StreamRegs instead)
    constexpr bool kIncFan = PHASE == 10;                 // income fan-out: the scenario fan-out with one income stream per wave as well
    constexpr bool kRuleFan = PHASE == 11;                // rule fan-out: the scenario fan-out with a spending rule per wave as well
    constexpr bool kGldFan = PHASE == 13;                 // glide fan-out: the allocation fan-out whose wave reloads its split once a calendar year from its own table
    constexpr bool kAlcFan = PHASE == 12 || kGldFan;      // allocation fan-out: the scenario fan-out with the split between the assets per wave as well
    constexpr bool kGlide = kGldFan || GLIDE;             // the weight in force is reloaded once a calendar year (glide_row): the glide fan-out's consumer wave, or a GLIDE launch
    constexpr bool kOwnAlloc = kAlcFan || GLIDE;          // the month reads the weight of WA, not the block's
    constexpr bool kScnFan = PHASE == 8 || kAsmFan || kIncFan || kRuleFan || kAlcFan;   // scenario fan-out: balance, contribution and spending per wave, the whole path
    constexpr bool kFan = kExpFan || kConFan || kScnFan;  // fan-out workgroup: one 64-path block, L consumer waves (levels), one producer wave
    constexpr bool kGrid = PHASE == 6;                    // ... of grid row blockIdx.y (GridCell)
    constexpr bool kRuleGrid = kGrid && RULE;             // ... under a spending rule (RuleGridCell: the row's record carries the rule)
    constexpr bool kWaveRule = kRuleFan || kRuleGrid;     // the consumer wave decides the year on its own FanRule
    constexpr bool kCand = PHASE == 2 || PHASE == 4 || kExpFan;   // resumes from a PHASE 1 snapshot (PHASE 2 / 4: per-candidate parameter block)
    constexpr bool kSliced = PHASE == 3 || PHASE == 4;    // time-sliced path blocks
    // the kernels that have growth, month and stream forms (kHasGrowthForms on the host) keep the month's wave-uniform counters
    // in running scalars: the row, the month of the year, the next priority threshold ("Scalar month counters" below)
    // (not the GF 3, MF 0 kernels at SF 0: with the counters they spill one to four SGPRs more than they did — LABNOTES R15 —
    // so they keep the month's old bookkeeping; their SF 1 forms read the running row and have it)
    constexpr bool kSIR = (SF & kStreamsInRegs) != 0;     // stream form (mcr_device.h): at most two records, all indexed, held in SGPRs
    constexpr bool kScalarCounters = MODE == 0 && RNG == 0 && !ANNUAL && !INJ && (PHASE == 0 || PHASE == 3) && !SPLIT && !XS &&
                                     (kSIR || !(GF == (kGrowthNarrowExp | kGrowthRhoZero) && MF == 0));
    // (both objects are declared HERE, with the phase constants: declared where they are first used, further down, the empty
    // objects reorder scalar instructions of eight time-sliced kernels that never read them — LABNOTES R15)
    [[maybe_unused]] std::conditional_t<kScalarCounters, MonthCounters, NoMonthCounters> SC;    // (an empty object in every other variant)
    [[maybe_unused]] std::conditional_t<kSIR, StreamRegs, NoStreamRegs> SR;    // (an empty object in every other variant)
    [[maybe_unused]] std::conditional_t<kIncFan, IncomeRegs, NoIncomeRegs> IR;   // (likewise)
    [[maybe_unused]] std::conditional_t<OUT, RuinMonth, NoRuinMonth> RM;         // (likewise: the outcome probes' month of failure)
    [[maybe_unused]] std::conditional_t<RULE, RuleState, NoRuleState> RS;        // (likewise: the spending rule's multiplier)
    [[maybe_unused]] std::conditional_t<kWaveRule, FanRule, NoFanRule> FR;       // (likewise: PHASE 11 and PHASE 6 with RULE, the consumer wave's own rule)
    [[maybe_unused]] std::conditional_t<kGlide, WaveGlideParams, std::conditional_t<kAlcFan, WaveAllocParams, NoWaveAlloc>> WA;   // (likewise: PHASE 12 / 13, the consumer wave's own weights, mcr_device.h; GLIDE: the launch's)
    static_assert(!kSliced || (RNG == 0 && !INJ && !SPLIT && !XS), "time-sliced blocks exist for the plain Philox variants");
    static_assert(PHASE != 4 || MODE == 0, "the search probes count only");
    // TAXED: which assets carry an effective realized-gains rate (bit 0: inv1, bit 1: inv2; DevParams::tax_mask)
    static_assert(TAXED >= 0 && TAXED <= 3, "TAXED is a two-bit mask");
    constexpr bool T1 = (TAXED & 1) != 0, T2 = (TAXED & 2) != 0, TANY = TAXED != 0;
    static_assert(!EXACT || XS || kExactMonthDefault, "the exact month is instantiated for the generic variants only");
    // GF: the launch's growth form (mcr_device.h: kGrowthNarrowExp | kGrowthRhoZero; masks 0, 1 and 3), for the issue-bound
    // whole-path count-only launches, plain or time-sliced.  Last, with a default: the names of the mask-0 variants are a prefix
    // of the others'.  A kernel with kGrowthNarrowExp loads the exp2 table ROTATED: growth_rows2 is its only reader there.
    static_assert(GF == 0 || GF == kGrowthNarrowExp || GF == (kGrowthNarrowExp | kGrowthRhoZero), "growth forms: masks 0, 1 and 3");
    static_assert(GF == 0 || (MODE == 0 && RNG == (int)MCR_RNG_PHILOX && !ANNUAL && !INJ && (PHASE == 0 || PHASE == 3) && !SPLIT && !XS),
                  "growth forms exist for the per-path Philox count-only launches (kPerPathPhilox), whole path or time-sliced");
    // MF: the launch's month form (mcr_device.h: kMonthEqualRates; masks 0 and 1), for the kernels that have growth forms.  Behind
    // GF, with a default, for the same reason.
    static_assert(MF == 0 || MF == kMonthEqualRates, "month forms: masks 0 and 1");
    static_assert(MF == 0 || (MODE == 0 && RNG == (int)MCR_RNG_PHILOX && !ANNUAL && !INJ && (PHASE == 0 || PHASE == 3) && (!SPLIT || LIST) && !XS && !EXACT),
                  "month forms exist for the kernels that have growth forms and for the split re-run of a screened launch, in the tolerance form of the month");
    static_assert(!(MF & kMonthEqualRates) || TAXED == 3, "equal realized-gains rates: both assets are taxed");
    constexpr bool EQR = (MF & kMonthEqualRates) != 0;
    // SF: the launch's stream form (mcr_device.h: kStreamsInRegs; masks 0 and 1), for the same kernels.  Behind MF, with a default.
    static_assert(SF == 0 || SF == kStreamsInRegs, "stream forms: masks 0 and 1");
    static_assert(SF == 0 || (MODE == 0 && RNG == (int)MCR_RNG_PHILOX && !ANNUAL && !INJ && (PHASE == 0 || PHASE == 3) && (!SPLIT || LIST) && !XS && !EXACT),
                  "stream forms exist for the kernels that have growth forms and for the split re-run of a screened launch, in the tolerance form of the month");
    constexpr bool TOL = !EXACT;         // the month in its tolerance form (mcr_device.h: "TOLERANCE FORM of the month")
    constexpr bool MM = !SPLIT || kFan || NPROD == 2 || LIST;  // exec-masked moves (issue-bound launches, and the consumer waves of a screened launch's re-run, either form) vs the compiler's selects (the lone probes' latency-bound SPLIT launches): MCR_MASKED_MOVE, mcr_device.h
    // the tolerance month's dust / empty fix-ups tested once per wave (mcr_device.h: WAVE-UNIFORM fix-ups), issue-bound launches only
    constexpr bool kFastMonth = TOL && MM && kUniformFixups;
    // The split re-run's consumer wave runs its months in PAIRS, on an event row (mcr_events.h; "PAIRS" below)
    constexpr bool kPairs = SPLIT && LIST;
    // (MODE 0, PHASE 0: the block runs the WHOLE path from month 1 and year 0 behind the statements that set the retirement's
    // initial state — no snapshot, no time slice, no candidate — and keeps none of the summary's columns)
    static_assert(!kPairs || (MODE == 0 && PHASE == 0 && kSIR && TOL && MM && !ANNUAL && !OUT && !RULE && !kFan),
                  "the paired consumer is stated for the re-run's own forms: a whole-path count-only launch, the tolerance month, the stream form");
    constexpr int kPaths = (kFan || NPROD == 2) ? 64 : kBlock;   // paths of a workgroup = columns of every per-path LDS array
    const int kThreads = kFan ? (int)blockDim.x : NPROD == 2 ? 3 * 64 : SPLIT ? 2 * kBlock : kBlock;
    const int tid = SPLIT ? (int)(threadIdx.x & (kPaths - 1)) : (int)threadIdx.x;    // the path's lane column in every per-path LDS array
    // PHASE 5 / 7: the wave's level (wave-uniform: an SGPR); the producer is wave fan_n
    const int fan_j = kFan ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : 0;
    const bool producer = kFan ? fan_j == io.fan_n : (SPLIT && threadIdx.x >= (unsigned)kPaths);   // wave-uniform (kPaths = 4 wavefronts, or 1)
    // PHASE 2: the parameter block of candidate blockIdx.y, in device memory (a separate const __restrict__ kernel
    // argument so that its loads are provably invariant and uniform: scalar loads, like the by-value block)
    // time-sliced launches (1-D grid): which path block (of which candidate) and which segment of it this workgroup runs (seg < 0: a whole block)
    int seg = -1, seg_block = 0;
    unsigned int path_block = blockIdx.x, cand = (PHASE == 2 || kGrid) ? blockIdx.y : 0u;
    if (kSliced) {
        const int S = io.seg_n_split, F = io.seg_n_full, bid = (int)blockIdx.x + io.seg_bid_base;
        unsigned int lb = (unsigned)bid;                  // the block's position in the launch's list of (candidate, path block) pairs
        if (bid < S) { seg = 0; seg_block = bid; }
        else if (bid >= S + F) { const int k = bid - S - F; seg = 1 + k / S; seg_block = k % S; lb = (unsigned)seg_block; }
        if (PHASE == 4) { cand = lb / (unsigned)io.seg_blocks_per_cand; path_block = lb % (unsigned)io.seg_blocks_per_cand; }
        else path_block = lb;
    }
    if constexpr (LIST) {
        if ((uint64_t)blockIdx.x * kPaths >= (uint64_t)*io.path_list_count) return;     // (wave-uniform; every thread of the workgroup, before any barrier)
    }
    const GridCell* cell = kRuleGrid ? &(reinterpret_cast<const RuleGridCell*>(cand_params) + cand)->cell    // (RULE: the grid's record heads the row's)
                           : kGrid ? reinterpret_cast<const GridCell*>(cand_params) + cand : nullptr;   // PHASE 6: the row's record
    const DevParams& P = kGrid ? cell->p : (kCand && !kFan) ? cand_params[cand] : P_arg;
    const int snap_c = kGrid ? cell->snap : (int)cand;   // snapshot column the row resumes from
    // LDS.  STATIC: the math tables (mcr_math.h) and, for the Philox stream, the [6][kBlock] stage of two months' gross
    // factors — static because the compiler then knows their addresses (offset 0 ...) and a table lookup is index << 3 +
    // ds_read with an immediate offset; against the dynamic region every address is `base + ...` with a base it only learns
    // to be 0 after instruction selection: v_lshl_add_u32 x, 3, 0 (a 3-operand op, 4.6 cycles instead of 2.7) or a literal
    // v_add_u32 0.  DYNAMIC: the NumPy ziggurat tables, [n_lock_slots][kBlock] doubles (frozen nominal stream amounts),
    // the block counters.  (The history stream's factor table stands where the ziggurat tables do.)
    constexpr bool kStaged = RNG == (int)MCR_RNG_PHILOX && !INJ;
    constexpr bool kHistory = (RNG == (int)MCR_RNG_HISTORY || RNG == kRngHistorySchemes) && !INJ;   // (its math tables are needed before the first month only: dynamic LDS, below)
    __shared__ __align__(16) double tab_s[kHistory ? 1 : kTabDoubles];
    constexpr int kStageLen = (kAsmFan ? kPartsPerPair : 6) * kPaths;   // = kStageDoubles for kBlock-path workgroups (PHASE 9 stages the normals' parts)
    constexpr int kStageRing = SPLIT ? 2 : 1;   // pair buffers of the stage (a power of two)
    __shared__ __align__(16) double stage_s[kStaged ? kStageRing * kStageLen : 1];
    // Per-path values that are written once or twice in a lifetime and read at the very end (first-year withdrawals,
    // YearsToRuin) live in the lane's own LDS column in the variants with per-path outputs: held to 5 waves per SIMD those
    // variants had no registers for them (round 2: 12 / 36 bytes of scratch per lane, 4-12 VGPRs spilled).
    // A/B on one box (tools/k1_modes_ab.py): summary output, 2e7 S60 paths 126.44 -> 126.23 ms; trajectories, 1e7 jorge paths
    // 50.28 -> 50.07 ms, 4e6 config.json paths 29.59 -> 29.40 ms.  A fourth column (the start-of-retirement balance) frees the
    // trajectory variant of its last 12 bytes of scratch but its 2 KB cost a resident workgroup as soon as the scenario has a
    // non-indexed income stream (one more LDS column): 50.07 -> 52.2 ms on jorge.json.  Three it is.
    constexpr bool kBins = MODE == 3;
    constexpr bool kSumLds = (MODE == 1 || MODE == 2) && kStaged;
    __shared__ __align__(16) double sum_s[kSumLds ? 3 * kBlock : 1];
    extern __shared__ __align__(16) unsigned char smem_raw[];
#ifdef MCR_K1_TIMELINE   // diagnostic build only (tools/k1_timeline.py): per-wave start / end stamps and placement
    const unsigned long long tl_t0 = wall_clock64();
#endif
    double* tab = kHistory ? reinterpret_cast<double*>(smem_raw) : tab_s;
    load_math_tables<(GF & kGrowthNarrowExp) != 0>(tab, threadIdx.x, kThreads);
    ZigTables zig{nullptr, nullptr, nullptr, nullptr};
    if (RNG == (int)MCR_RNG_NUMPY) { zig = load_zig_tables(smem_raw, threadIdx.x, kThreads); zig.math_tab = tab; }
    // History stream: G[H][3] = (g1, ginf, g2 = ginf gprem) of every month of the record under THIS launch's market, made by the
    // workgroup from Z with the injected route's operations in its order (growth(), below): the two routes agree bit for bit.  Rows
    // of three doubles: a lane's month is one address and three reads at immediate offsets (the lanes of a wave stand at 64
    // unrelated rows either way).  H x 3 exp per workgroup against 256 x total_months x 3 on the engine's own stream.  The math
    // tables serve these exps and nothing after them, so the table takes their place: every thread makes its (at most 8) rows in
    // registers, and stores them once the whole workgroup has read the tables for the last time.  A 2048-month record is then
    // 48 KB a workgroup, three to a CU, where table + math tables were two.
    [[maybe_unused]] const double* const hist_tab = reinterpret_cast<const double*>(smem_raw);
    [[maybe_unused]] std::conditional_t<kHistory, HistoryCursor, NoHistoryCursor> HC;    // (an empty object in every other variant)
    if constexpr (kHistory) {
        constexpr int kRowsPerThread = MCR_MAX_HISTORY_MONTHS / kBlock;
        static_assert(kRowsPerThread * kBlock == MCR_MAX_HISTORY_MONTHS, "every row of the longest record has a thread");
        HC = history_cursor();
        __syncthreads();     // the math tables are in place
        const int H = (int)io.history_months;
        double g[kRowsPerThread][3];
#pragma unroll
        for (int i = 0; i < kRowsPerThread; ++i) {
            const int k = (int)threadIdx.x + i * kBlock;
            g[i][0] = g[i][1] = g[i][2] = 0.0;
            if (k < H) {
                const double ze = io.history[3 * k + 0], zi = io.history[3 * k + 1], zp = io.history[3 * k + 2];
                g[i][0] = monthly_gross(P.a1, P.b1, ze, tab);
                g[i][1] = monthly_gross(P.ainf, P.binf, zi, tab);
                g[i][2] = g[i][1] * monthly_gross(P.aprem, P.bprem, zp, tab);  // :532
            }
        }
        __syncthreads();     // nobody reads the math tables any more
        double* const G = reinterpret_cast<double*>(smem_raw);
#pragma unroll
        for (int i = 0; i < kRowsPerThread; ++i) {
            const int k = (int)threadIdx.x + i * kBlock;
            if (k < H) { G[3 * k + 0] = g[i][0]; G[3 * k + 1] = g[i][1]; G[3 * k + 2] = g[i][2]; }
        }
    }
    // Philox stream: the gross factors of two months at a time, staged per lane (growth_rows2)
    double* stage = stage_s + (kStaged ? tid : 0);
    double* sum_col = sum_s + (kSumLds ? tid : 0);     // [0] first-year gross, [kBlock] first-year real gross, [2 kBlock] YearsToRuin bits
    // lock columns: [n_lock_slots][kPaths] doubles; PHASE 5: one such block per consumer wave
    double* lock_lds = reinterpret_cast<double*>(smem_raw + (RNG == (int)MCR_RNG_NUMPY ? (size_t)kZigLdsBytes
                                                             : kHistory ? (size_t)io.history_months * 3u * sizeof(double) : (size_t)0));
    unsigned int* blk = reinterpret_cast<unsigned int*>(lock_lds + (size_t)P.n_lock_slots * kPaths * (kFan ? io.fan_n : 1));
    if (kFan && !producer) lock_lds += (size_t)fan_j * P.n_lock_slots * kPaths;
    // blk[0] = success count; blk[1 .. 1+ry+2) = ruin bins; then [ry+1] done-years histogram; then the
    // [hist_n_bins] final-balance histogram of the workgroup (mcr_outputs.hist_bins), when requested
    const int ry = P.retirement_years;
    const int n_blk = kFan ? MCR_MAX_EXPENSE_FANOUT : 1 + (ry + 2) + (ry + 1);   // (PHASE 5: blk[j] = level j's success count)
    const int n_hist = ((PHASE == 0 || PHASE == 3) && io.out.hist_bins != nullptr) ? io.out.hist_n_bins : 0;
    for (int k = threadIdx.x; k < n_blk + n_hist; k += kThreads) blk[k] = 0u;
    // MODE 3: behind the block counters the edge arrays, the row buffers and the final_success cells (YearBinsLds)
    // (RULE: the state with the rule and the multiplier segment, from the launch's one record behind `cand_params`)
    constexpr bool kBinsRule = kBins && RULE;
    [[maybe_unused]] std::conditional_t<kBins, std::conditional_t<kBinsRule, YearBinsRuleState, YearBinsState>, NoYearBins> YB;    // (an empty object in every other variant)
    if constexpr (kBins) {
        year_bins_plan(YB.L, io.yb, cand_params, blk + n_blk + n_hist);
        rule_bins_begin(YB, cand_params);
        YB.k = 0; YB.last = 0.0;
        const YearBinsLds& YL = YB.L;
        if (YL.n > 0) for (int k = threadIdx.x; k <= YL.n; k += kThreads) YL.edges[k] = io.yb.edges[k];
        if (YL.wn > 0) for (int k = threadIdx.x; k <= YL.wn; k += kThreads) YL.wedges[k] = io.yb.wr_edges[k];
        year_bins_load_m_edges(YB.L, cand_params, (int)threadIdx.x, kThreads);
        for (int k = threadIdx.x; k < 2 * YL.row + YL.cells; k += kThreads) YL.buf[k] = 0u;
    }
    __syncthreads();

    uint64_t local = (uint64_t)path_block * kPaths + (unsigned)tid;
    bool valid = local < io.n_paths;
    if constexpr (LIST) {     // the lane's position in the list, then the entry there (a local path index below n_paths)
        const uint64_t list_n = *io.path_list_count;
        valid = local < list_n;
        if (valid) local = io.path_list[local];
    }
    const uint64_t li = valid ? local : (io.n_paths - 1);  // tail lanes shadow the last path, write nothing
    const uint64_t path = io.path_begin + li;
    // growth_rows2's per-path Philox rounds (mcr_device.h), in the count-only kernels without an annual-gains tax
    constexpr bool kPerPathPhilox = MODE == 0 && !ANNUAL;
    const PhiloxPath PQ = kPerPathPhilox ? philox_path(path, io.stream_id, io.seed) : PhiloxPath{};   // (the whole wave is here: philox_path's ballot)
    const int64_t stride = io.out.path_stride;
    const double* inj = INJ ? io.injected + (size_t)li * 3u * (size_t)P.shock_rows : nullptr;

    constexpr bool kSummary = MODE >= 1;
    constexpr bool kTraj = MODE == 2;
    double* traj = kTraj ? io.out.trajectory : nullptr;
    double* rtraj = kTraj ? io.out.real_trajectory : nullptr;
    double* wrt = kTraj ? io.out.withdrawal_rate_trajectory : nullptr;

    auto put_sample = [&](int t, double nominal, double px) {  // :574-576, :928-931
        if (kTraj && valid) {
            if (traj) traj[(int64_t)t * stride + (int64_t)li] = nominal;
            if (rtraj) rtraj[(int64_t)t * stride + (int64_t)li] = px > kEps ? nominal / px : 0.0;
        }
        if constexpr (kBins) year_bins_row(io.yb, YB.L, YB.k++, valid, t, true, nominal, px, -1, kNanBits);
    };
    Pcg64 gen;  // NumPy stream: one generator per path, rows are consumed strictly in order
    if (RNG == (int)MCR_RNG_NUMPY && !INJ) {
        const uint32_t s32 = io.path_seeds ? io.path_seeds[li]
                                           : np_path_seed(io.entropy, (int)io.n_entropy, io.stream_id, io.child_offset + path);
        pcg64_seed_u32(gen, s32);
    }
    // Top of every month (wave-uniform, outside any divergent region): rows are visited in order 0, 1, 2, ... across
    // both phases, so each pair of rows is generated exactly when its first row comes up.
    PairCarry carry{0u, 0u};
    const MathRegs GR = kStaged ? MathRegs::pinned_path() : MathRegs::literals();
    // Wave priority falls as the path advances (s_setprio takes an immediate: four levels).  The SIMD arbitrates VALU
    // issue by priority, then age; left alone, the oldest wave of a SIMD runs far ahead and the youngest is left to
    // finish ALONE at the end of the launch, at a fraction of the SIMD's issue rate (measured with per-wave
    // s_memrealtime stamps: waves of one 10^6-path launch took 1.2 to 3.6 ms and the drain was 3 of its 8.4 ms).
    // With laggards served first the waves of a SIMD finish together, the bands narrowing towards the end of the
    // path: 8.40 -> 7.98 ms at exactly 10^6 paths (profiles/r02/k1_timeline_*.txt).
    const int prio_t1 = P.total_months / 2, prio_t2 = (P.total_months * 3) / 4, prio_t3 = (P.total_months * 9) / 10;
    __builtin_amdgcn_s_setprio(3);
    bool wg_dead = false;      // SPLIT: no consumer lane of the workgroup is alive any more (wave-uniform, agreed at a barrier)
    bool lane_alive = true;    // SPLIT: this consumer lane still has months to simulate
    // Scalar month counters (MonthCounters above): a month compares its row with the NEXT threshold only; the chain, and the
    // threshold after it, run in the three months a path hits one
    if constexpr (kScalarCounters) { SC.prio_next = prio_t1; SC.row = 0; SC.moy = 0; SC.ye_mi = kMPY - 1 - P.working_months % kMPY; }   // (prio_t1 = prio_from(.., 0))
    auto begin_month = [&](int row) {
        if constexpr (kScalarCounters) {
            if (row == SC.prio_next) {
                if (row == prio_t1) __builtin_amdgcn_s_setprio(2);
                else if (row == prio_t2) __builtin_amdgcn_s_setprio(1);
                else if (row == prio_t3) __builtin_amdgcn_s_setprio(0);
                SC.prio_next = prio_from(prio_t1, prio_t2, prio_t3, row + 1);
            }
        } else {
        if (row == prio_t1) __builtin_amdgcn_s_setprio(2);
        else if (row == prio_t2) __builtin_amdgcn_s_setprio(1);
        else if (row == prio_t3) __builtin_amdgcn_s_setprio(0);
        }
        if (kStaged && (row & 1) == 0) {
            if (SPLIT) {
                // the producers have staged the pair (row, row + 1) in buffer (row >> 1) & 1.  Every kSplitVotePairs-th pair the barrier
                // also votes (a voting barrier costs about two plain ones: every 6th pair 0.93 ms per lone probe, every 16th 0.88): once no consumer lane of the workgroup is alive, producers and consumers stop together (the unsplit
                // kernel lets a wave leave as soon as all of ITS lanes have failed)
                if (wg_dead) return;
                if (((row >> 1) & (kSplitVotePairs - 1)) == 0) { if (__syncthreads_or(__builtin_amdgcn_ballot_w64(lane_alive) != 0ull ? 1 : 0) == 0) wg_dead = true; }
                else __syncthreads();
            } else {
                if ((row & 2) == 0) growth_rows2<0, kPaths, kPerPathPhilox, GF>(P, GR, io.seed, io.stream_id, path, PQ, (uint32_t)row >> 2, tab, stage, carry);
                else growth_rows2<1, kPaths, kPerPathPhilox, GF>(P, GR, io.seed, io.stream_id, path, PQ, (uint32_t)row >> 2, tab, stage, carry);
            }
        }
    };
    // gross factors of month `row` (:522-532)
    [[maybe_unused]] std::conditional_t<kAsmFan, Market, NoMarket> MK;   // PHASE 9: the consumer wave's market (VGPRs), set below
    auto growth = [&](int row, double& g1, double& ginf, double& g2) {
        if constexpr (kAsmFan) {    // this wave's factors from the staged parts of the pair
            growth_factors_staged<kPaths>(MK, stage + (size_t)((row >> 1) & 1) * kStageLen, row & 1, tab, GR, g1, ginf, g2);
            return;
        }
        if (kStaged) {
            const double* c = stage + (size_t)(3 * (row & 1)) * kPaths + (SPLIT ? (size_t)((row >> 1) & (kStageRing - 1)) * kStageLen : 0);
            g1 = c[0]; ginf = c[kPaths]; g2 = c[2 * kPaths];
            return;
        }
        if constexpr (kHistory) {
            const int r = row < P.shock_rows - 1 ? row : P.shock_rows - 1;  // :692, like an injected row
            history_seek<RNG == kRngHistorySchemes>(HC, r, io.history_months, io.history_block, io.history_scheme, io.seed, io.stream_id, path);
            const double* const c = hist_tab + 3u * HC.cur;
            g1 = c[0]; ginf = c[1]; g2 = c[2];
            return;
        }
        double ze, zi, zp;
        if (INJ) {
            const int r = row < P.shock_rows - 1 ? row : P.shock_rows - 1;  // :692
            ze = inj[3 * r + 0]; zi = inj[3 * r + 1]; zp = inj[3 * r + 2];
        } else {
            const double z0 = np_standard_normal(gen, zig);  // standard_normal((n, 3)) fills row-major (:458)
            const double z1 = np_standard_normal(gen, zig);
            const double z2 = np_standard_normal(gen, zig);
            ze = z0;
            zi = P.rho * z0 + P.rho_c * z1;                  // :461-464
            zp = z2;
        }
        g1 = monthly_gross(P.a1, P.b1, ze, tab);
        ginf = monthly_gross(P.ainf, P.binf, zi, tab);
        g2 = ginf * monthly_gross(P.aprem, P.bprem, zp, tab);  // :532
    };

    // PHASE 12: the wave's weights from its record (wave-uniform: scalar loads from the launch's table, like PHASE 11's rule), and
    // what else the month's helpers read of the block beside them.  alloc2 = 1.0 - alloc1: derive_params' operation.  The producer,
    // wave fan_n, stands one past the group's records: it reads record 0's, and uses none of it.
    // PHASE 13: the record names the wave's table instead, GlideRecord::weights doubles behind the record itself (probe_glide_paths_fanout:
    // the host's offset, so that a group's launch, which gets the table at ITS first record, reads its own weights); W[0] is in
    // force from row 0, `left` = n - 1 entries stand behind it.
    // GLIDE: the launch's one record (launch_glide: the weights stand directly behind it), the same statements.
    if constexpr (kGlide) {
        const GlideRecord* const rec = reinterpret_cast<const GlideRecord*>(cand_params) + ((GLIDE || producer) ? 0 : fan_j);
        WA.w = (GlideTable)(reinterpret_cast<const double*>(rec) + rec->weights);
        WA.left = rec->n_weights - 1;
        WA.moy = 0;
        WA.alloc1 = *WA.w;
        WA.alloc2 = 1.0 - WA.alloc1;
        WA.annual_rate1 = P.annual_rate1; WA.annual_rate2 = P.annual_rate2; WA.any_annual_tax = P.any_annual_tax;
    } else
    if constexpr (kAlcFan) {
        const mcr_allocation_option* const rec = reinterpret_cast<const mcr_allocation_option*>(cand_params) + (producer ? 0 : fan_j);
        WA.alloc1 = rec->allocation_inv1_pct;
        WA.alloc2 = 1.0 - WA.alloc1;
        WA.annual_rate1 = P.annual_rate1; WA.annual_rate2 = P.annual_rate2; WA.any_annual_tax = P.any_annual_tax;
    }
    std::conditional_t<kGlide, LaneParams, const LaneParams> L = month_lane_params<TOL, EQR>(WA, P);    // (mutable in PHASE 13 and under GLIDE only)
    // PHASE 13, at the top of every row t (wave-uniform, outside every lane mask): where t % 12 == 0, t > 0 -- a calendar year
    // from today has closed, which is NOT a retirement-year boundary unless working_months % 12 == 0 -- the weight in force
    // becomes W[min(t / 12, n - 1)]: one scalar load unless the table is exhausted, then derive_params' subtraction and the two
    // products of month_lane_params again.  The row's every read of a weight, its annual tax and closing rebalance included,
    // comes behind this.  A scalar counter of its own: the variants without the annual-gains tax have no year-close branch.
    // Lanes that have failed run no month and read none of it.  glide_row (mcr_device.h) is the statement; its two calls below
    // stand under `if constexpr (kGlide)`, which every other instantiation discards.

    // ---- initial state (:490-510) ----
    double b1 = P.initial_balance * (GLIDE ? WA.alloc1 : P.alloc1);  // :499 (GLIDE: W[0])
    double b2 = P.initial_balance - b1;        // :500
    double c1 = b1, c2 = b2;                   // :501-502
    double contrib = P.monthly_contribution;   // :504
    double gacc1 = 0.0, gacc2 = 0.0;           // :505-506
    double infl = 1.0;                         // :508
    bool pre_fail = false;                     // :510
    int t_idx = 0;
    put_sample(t_idx++, P.initial_balance, 1.0);  // :490-492
    const int wm = P.working_months;
    // snapshot c, field f of local path li: snap[(c * kSnapFields + f) * snap_stride + li]
    auto snap_at = [&](int c, int f) { return io.snap + ((size_t)c * kSnapFields + (size_t)f) * (size_t)io.snap_stride + (size_t)li; };
    int snap_i = 0;
    auto save_snapshot = [&]() {
        if (valid) {
            *snap_at(snap_i, 0) = b1; *snap_at(snap_i, 1) = b2; *snap_at(snap_i, 2) = c1; *snap_at(snap_i, 3) = c2;
            *snap_at(snap_i, 4) = gacc1; *snap_at(snap_i, 5) = gacc2; *snap_at(snap_i, 6) = infl; *snap_at(snap_i, 7) = contrib;
            *snap_at(snap_i, 8) = pre_fail ? 1.0 : 0.0;
            if (!SPLIT) store_bits(snap_at(snap_i, 9), ((unsigned long long)carry.w3 << 32) | (unsigned long long)carry.w2);   // (SPLIT: the producer's)
        }
        ++snap_i;
    };
    if constexpr (NPROD == 2) {
        if (producer) {
            // Producer h = 0 / 1 stages the pairs p = h, h + 2, ... below n_pairs, pair p in buffer p & 1.  Barriers 0 .. n_pairs - 1
            // in order, each exactly once unless a vote ends the workgroup first (then no wave executes another): barrier p - 1 in
            // the middle of pair p (not for p = 0: there is none), barrier p behind it, and behind the loop the last barrier where
            // it belongs to the other producer's pair.  The consumer executes barrier p at row 2 p (begin_month), p < n_pairs.
            // Buffer p & 1 is read between barriers p and p + 1 and written again for pair p + 2 behind barrier p + 1: every store of
            // growth_rows2_own_half comes behind its hook, i.e. behind barrier (p + 2) - 1.
            const int n_pairs = (P.total_months + 1) >> 1;
            bool stop = false;
            auto handover = [&](int q) {      // barrier q, a vote at the consumer's vote rows (producers vote 0)
                if ((q & (kSplitVotePairs - 1)) == 0) { if (__syncthreads_or(0) == 0) stop = true; }
                else __syncthreads();
            };
            auto run = [&](auto half) {
                constexpr int H = decltype(half)::value;
                int p = H;
                for (; p < n_pairs; p += 2) {
                    growth_rows2_own_half<H, kPaths>(P, GR, io.seed, io.stream_id, path, PQ, (uint32_t)p >> 1, tab, stage + (size_t)(p & (kStageRing - 1)) * kStageLen,
                                                     [&]() { if (p > 0) handover(p - 1); });
                    if (stop) return;
                    handover(p);
                    if (stop) return;
                }
                if (p == n_pairs && p > 0) handover(p - 1);
            };
            if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 1) run(std::integral_constant<int, 0>{});
            else run(std::integral_constant<int, 1>{});
            return;
        }
    }
    if (SPLIT && producer) {
        // Rows [first_row, last_row), a pair per iteration, one barrier per pair: exactly the barriers the consumers execute
        // in begin_month at every even row they visit (they visit every row of this range, in order, and never leave early).
        const int first_row = kCand ? (wm & ~1) : 0;                      // PHASE 2 / 5 resume with the pair that holds row wm
        const int last_row = PHASE == 1 ? wm : P.total_months;
        if (kCand) {
            const unsigned long long cw = f64_bits(*snap_at(snap_c, 9));
            carry.w2 = (uint32_t)cw; carry.w3 = (uint32_t)(cw >> 32);
        }
        // PHASE 1: the Philox words carried past the end of candidate month m are those in hand once the pair that holds row
        // m - 1 has been generated (m = 0: none yet) — what the unsplit kernel stores from its single `carry`
        auto put_carry = [&]() {
            if (valid) store_bits(snap_at(snap_i, 9), ((unsigned long long)carry.w3 << 32) | (unsigned long long)carry.w2);
            ++snap_i;
        };
        if (PHASE == 1) while (snap_i < io.n_snap && io.snap_months[snap_i] == 0) put_carry();
        for (int row = first_row; row < last_row; row += 2) {
            double* st = stage + (size_t)((row >> 1) & 1) * kStageLen;
            if constexpr (kAsmFan) {
                if ((row & 2) == 0) growth_parts2<0, kPaths, kPerPathPhilox>(GR, io.seed, io.stream_id, path, PQ, (uint32_t)row >> 2, tab, st, carry);
                else growth_parts2<1, kPaths, kPerPathPhilox>(GR, io.seed, io.stream_id, path, PQ, (uint32_t)row >> 2, tab, st, carry);
            } else {
                if ((row & 2) == 0) growth_rows2<0, kPaths, kPerPathPhilox>(P, GR, io.seed, io.stream_id, path, PQ, (uint32_t)row >> 2, tab, st, carry);
                else growth_rows2<1, kPaths, kPerPathPhilox>(P, GR, io.seed, io.stream_id, path, PQ, (uint32_t)row >> 2, tab, st, carry);
            }
            if (PHASE == 1) while (snap_i < io.n_snap && ((io.snap_months[snap_i] - 1) >> 1) == (row >> 1)) put_carry();
            if (((row >> 1) & (kSplitVotePairs - 1)) == 0) { if (__syncthreads_or(0) == 0) return; }   // (the consumers' vote, begin_month)
            else __syncthreads();
        }
        return;
    }
    if (kConFan) contrib = io.fan_expenses[fan_j];   // PHASE 7: this consumer wave's contribution level (the producer has returned)
    // PHASE 8: this consumer wave's record (the producer has returned: fan_j < fan_n, inside the launch's table), three SGPR
    // pairs; the initial state again, from the record's balance
    double scn_expenses = 0.0;
    if constexpr (kAsmFan) {                     // PHASE 9: the record's three values likewise, and its market into VGPRs
        const AssumptionRecord* const rec = reinterpret_cast<const AssumptionRecord*>(cand_params) + fan_j;
        const double rec_balance = rec->initial_balance;
        b1 = rec_balance * P.alloc1;             // :499
        b2 = rec_balance - b1;                   // :500
        c1 = b1; c2 = b2;                        // :501-502
        contrib = rec->monthly_contribution;     // :504
        scn_expenses = rec->monthly_expenses;
        MK.a1 = rec->a1; MK.b1 = rec->b1; MK.ainf = rec->ainf; MK.binf_rho = rec->binf_rho; MK.binf_rho_c = rec->binf_rho_c;
        MK.aprem = rec->aprem; MK.bprem = rec->bprem;
        asm volatile("" : "+v"(MK.a1), "+v"(MK.b1), "+v"(MK.ainf), "+v"(MK.binf_rho), "+v"(MK.binf_rho_c), "+v"(MK.aprem), "+v"(MK.bprem));
    } else if constexpr (kIncFan) {              // PHASE 10: the record's three values likewise (its stream: at S0 / S1 below)
        const IncomeRecord* const rec = reinterpret_cast<const IncomeRecord*>(cand_params) + fan_j;
        const double rec_balance = rec->initial_balance;
        b1 = rec_balance * P.alloc1;             // :499
        b2 = rec_balance - b1;                   // :500
        c1 = b1; c2 = b2;                        // :501-502
        contrib = rec->monthly_contribution;     // :504
        scn_expenses = rec->monthly_expenses;
    } else if constexpr (kRuleFan) {             // PHASE 11: the record's three values likewise, and its rule (wave-uniform: scalar loads)
        const RuleRecord* const rec = reinterpret_cast<const RuleRecord*>(cand_params) + fan_j;
        const double rec_balance = rec->initial_balance;
        b1 = rec_balance * P.alloc1;             // :499
        b2 = rec_balance - b1;                   // :500
        c1 = b1; c2 = b2;                        // :501-502
        contrib = rec->monthly_contribution;     // :504
        scn_expenses = rec->monthly_expenses;
        FR.upper = rec->upper; FR.lower = rec->lower; FR.keep = rec->keep; FR.grow = rec->grow; FR.floor = rec->floor; FR.ceiling = rec->ceiling;
        // option j's own table of the launch's year counts (the pointer is a launch constant read late, like the epilogue's)
        unsigned long long* const yc = late_arg<unsigned long long*>(offsetof(KernelIO, fan_rule) + offsetof(KernelIO::FanRuleRows, year_counts));
        FR.year_counts = yc ? yc + (size_t)fan_j * (size_t)P.retirement_years * MCR_RULE_N_COUNTS : nullptr;
    } else if constexpr (kRuleGrid) {            // PHASE 6 with RULE: the row's rule and this level's table of the row's year counts (scalar loads)
        const RuleGridCell* const rec = reinterpret_cast<const RuleGridCell*>(cand_params) + cand;
        FR.upper = rec->upper; FR.lower = rec->lower; FR.keep = rec->keep; FR.grow = rec->grow; FR.floor = rec->floor; FR.ceiling = rec->ceiling;
        unsigned long long* const yc = rec->year_counts;
        FR.year_counts = yc ? yc + (size_t)fan_j * (size_t)P.retirement_years * MCR_RULE_N_COUNTS : nullptr;
    } else if constexpr (kAlcFan) {              // PHASE 12 / 13: the record's three values likewise, split by the wave's own weight (WA, above; PHASE 13: W[0])
        // (the two records begin alike: mcr_glide_option's static_assert)
        const mcr_allocation_option* const rec = reinterpret_cast<const mcr_allocation_option*>(cand_params) + fan_j;
        const double rec_balance = rec->initial_balance;
        b1 = rec_balance * WA.alloc1;            // :499
        b2 = rec_balance - b1;                   // :500
        c1 = b1; c2 = b2;                        // :501-502
        contrib = rec->monthly_contribution;     // :504
        scn_expenses = rec->monthly_expenses;
    } else if constexpr (kScnFan) {
        const mcr_scenario* const scn = reinterpret_cast<const mcr_scenario*>(cand_params) + fan_j;
        const double scn_balance = scn->initial_balance;
        b1 = scn_balance * P.alloc1;             // :499
        b2 = scn_balance - b1;                   // :500
        c1 = b1; c2 = b2;                        // :501-502
        contrib = scn->monthly_contribution;     // :504
        scn_expenses = scn->monthly_expenses;
    }
    if (PHASE == 1) while (snap_i < io.n_snap && io.snap_months[snap_i] == 0) save_snapshot();
    // PHASE 3: a later segment of a time-sliced block takes its lanes' state over from its predecessor
    // b1 b2 c1 c2 gacc1 gacc2 infl | flags | Philox carry | (per-path outputs: balance and price level at retirement, the
    // three write-once columns) ; then the lock columns
    constexpr int kSegFixedFields = MODE >= 1 ? 14 : 9;
    double seg_start_balance = 0.0, seg_infl_ret = 0.0;
    auto seg_at = [&](int f) { return io.seg_state + ((size_t)seg_block * (size_t)(kSegFixedFields + P.n_lock_slots) + (size_t)f) * kBlock + (size_t)tid; };
    __shared__ int seg_ok_s;
    bool seg_resumed = false;
    int y_begin = 0, y_end = ry;
    unsigned long long seg_state_flags = 0ull;
    if (kSliced && seg >= 0) {
        y_end = io.seg_year[seg + 1];
        if (seg > 0) {
            if (threadIdx.x == 0) {
                // the predecessor's flag: 0 pending, 1 state handed over, 2 recomputed (the slot is not its state).  Resume on 1
                // only; on 2, or when the budget runs out, recompute at once (see the hand-over at the end of the segment)
                const unsigned int* f = io.seg_flags + (size_t)seg_block * (size_t)io.seg_q + (size_t)(seg - 1);
                unsigned int v = 0u;
                for (int spin = 0; spin < io.seg_max_polls; ++spin) {
                    if ((v = __hip_atomic_load(f, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)) != 0u) break;
                    __builtin_amdgcn_s_sleep(32);
                }
                seg_ok_s = v == 1u;
            }
            __syncthreads();
            seg_resumed = seg_ok_s != 0;     // (otherwise: this workgroup runs the block from month 0 itself, up to its own end)
            if (seg_resumed) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                b1 = *seg_at(0); b2 = *seg_at(1); c1 = *seg_at(2); c2 = *seg_at(3);
                if (ANNUAL) { gacc1 = *seg_at(4); gacc2 = *seg_at(5); }    // (otherwise identically 0 and never read)
                infl = *seg_at(6);
                seg_state_flags = f64_bits(*seg_at(7));
                const unsigned long long cw = f64_bits(*seg_at(8));
                carry.w2 = (uint32_t)cw; carry.w3 = (uint32_t)(cw >> 32);
                for (int k = 0; k < P.n_lock_slots; ++k) lock_lds[(size_t)k * kBlock + tid] = *seg_at(kSegFixedFields + k);
                if (MODE >= 1) {
                    seg_start_balance = *seg_at(9); seg_infl_ret = *seg_at(10);
                    sum_col[0] = *seg_at(11); sum_col[kBlock] = *seg_at(12); sum_col[2 * kBlock] = *seg_at(13);
                }
                y_begin = io.seg_year[seg];
                const int r0 = wm + kMPY * y_begin;
                if (r0 >= prio_t3) __builtin_amdgcn_s_setprio(0);
                else if (r0 >= prio_t2) __builtin_amdgcn_s_setprio(1);
                else if (r0 >= prio_t1) __builtin_amdgcn_s_setprio(2);
                if constexpr (kScalarCounters) { SC.prio_next = prio_from(prio_t1, prio_t2, prio_t3, r0 - (r0 & 1)); SC.row = r0; }
                if (r0 & 1) begin_month(r0 - 1);  // the pair of rows (r0 - 1, r0) was staged by the predecessor: stage it again
            }
        }
    }

    if (kCand && !seg_resumed) {   // (a segment that took its predecessor's state over needs neither the snapshot nor the re-staged pair)
        const int c = snap_c;
        b1 = *snap_at(c, 0); b2 = *snap_at(c, 1); c1 = *snap_at(c, 2); c2 = *snap_at(c, 3);
        gacc1 = *snap_at(c, 4); gacc2 = *snap_at(c, 5); infl = *snap_at(c, 6); contrib = *snap_at(c, 7);
        pre_fail = *snap_at(c, 8) != 0.0;
        const unsigned long long cw = f64_bits(*snap_at(c, 9));
        carry.w2 = (uint32_t)cw; carry.w3 = (uint32_t)(cw >> 32);
        if (wm & 1) begin_month(wm - 1);   // the pair of rows (wm - 1, wm) was staged during the accumulation: stage it again
    }
    // ---- accumulation (:513-579): no lane leaves this loop early ----
    // (kScalarCounters: moy = m mod 12 in 1 .. 12, a running month of the year instead of the two % kMPY tests)
    for (int m = 1; m <= ((kPairs || kCand || (kSliced && seg_resumed)) ? 0 : wm); ++m) {    // (kPairs: in pairs, below)
        if constexpr (kScalarCounters) ++SC.moy;
        if constexpr (kGlide) glide_row<TOL, EQR>(WA, P, L);           // (PHASE 13, GLIDE: row m - 1's weight)
        if (P.contrib_grows && year_opens(SC, m - 1) && m > 1) {  // :514-517 (wave-uniform: a scalar branch, not a select)
            asm volatile("");
            contrib *= P.contrib_growth_factor;
        }
        begin_month(m - 1);
        double g1, ginf, g2;
        growth(m - 1, g1, ginf, g2);                                   // :519-532
        market_step<ANNUAL, TOL>(g1, ginf, g2, b1, b2, gacc1, gacc2, infl); // :534-538
        const double k1 = contrib * (kOwnAlloc ? WA.alloc1 : P.alloc1);   // :540-542
        const double k2 = contrib - k1;                                // :543
        b1 += k1; c1 += k1; b2 += k2; c2 += k2;                        // :544-547
        if (TOL) month_rebalance_tol<TANY, MM, kFastMonth, EQR>(WA, P, L, b1, c1, b2, c2);  // :549-553
        else rebalance_path<TANY, MM>(L, b1, c1, b2, c2);
        if (year_closes(SC, m)) {                                      // :557
            if constexpr (kScalarCounters) SC.moy = 0;
            pre_fail |= month_annual_gain_taxes<false, TANY, ANNUAL, T1, T2, MM, TOL, EQR>(WA, P, L, b1, c1, b2, c2, gacc1, gacc2);  // :558-573
            put_sample(t_idx++, b1 + b2, infl);                        // :574-576
            gacc1 = 0.0; gacc2 = 0.0;                                  // :578-579
        }
        if (PHASE == 1 && snap_i < io.n_snap && m == io.snap_months[snap_i]) save_snapshot();
    }
    if (PHASE == 1) return;   // (every thread of the workgroup: nothing below is needed)
    if constexpr (kScalarCounters) { if (!(kSliced && seg_resumed)) SC.row = wm; }   // (a resumed segment starts at its own row)
    double start_balance = b1 + b2;        // :581 (kPairs: the accumulation runs further down, so this is the INITIAL balance there, like infl_ret, alive, succeeded and ruin_bin below — stale and, in a count-only kernel, unread; the block sets the last three again)
    double infl_ret = infl;                // :582
    if (kSliced && seg_resumed) { start_balance = seg_start_balance; infl_ret = seg_infl_ret; t_idx = P.trajectory_len - ry + y_begin; }
    else if (wm > 0 && wm % kMPY != 0) put_sample(t_idx++, start_balance, infl_ret);  // :590-594
    rule_begin(RS, start_balance, infl_ret);         // (RULE: m = 1 at retirement; nothing in every other kernel)

    // ---- decumulation (:632-868) ----
    double fy_gross = 0.0, fy_real = 0.0;            // :623-624
    bool alive = !pre_fail;                          // :627, :633
    bool succeeded = !pre_fail;
    unsigned long long ytr_bits = pre_fail ? f64_bits(0.0) : kNanBits;  // YearsToRuin (:497, :628-629)
    if (kSumLds && !(kSliced && seg_resumed)) { sum_col[0] = 0.0; sum_col[kBlock] = 0.0; store_bits(&sum_col[2 * kBlock], ytr_bits); }
    // A launch that cannot fill the chip (SPLIT) is bound by each wave's dependency chain, and re-reading a stream's record
    // from the kernel arguments every month is three dependent scalar loads on it (the compiler loads start, then end, then
    // the rest): the first two records stay in SGPRs there (82 + 16 of them; the unsplit kernel has none to spare).
    // PHASE 9 does not: its consumers also hold fexp's constants, and the 12 SGPRs of the two records are what the kernel then
    // lacks (3 to 8 SGPRs spilled with them); its 15 consumer waves a workgroup hide the loads as the unsplit kernel's waves do.
    // (kStreamRegs is declared with the phase constants above: declared here, the same constant reorders a few scalar
    // instructions of the time-sliced kernels, which never read it)
    DevStream S0 = {}, S1 = {};
    // PHASE 10: the wave's version of kept record IR.k (wave-uniform values: SGPRs)
    if constexpr (kIncFan) {
        const IncomeRecord* const rec = reinterpret_cast<const IncomeRecord*>(cand_params) + fan_j;
        IR.k = io.fan_stream;
        IR.amount = rec->amount; IR.amount_keep = rec->amount_keep; IR.start_month = rec->start_month; IR.end_month = rec->end_month;
    }
    if (kStreamRegs) {
        if (P.n_streams > 0) S0 = P.streams[0];
        if (P.n_streams > 1) S1 = P.streams[1];
        if constexpr (kIncFan) {   // kept record 0 or 1 is the probed one: this wave's version of it, for the whole launch
            if (IR.k == 0) income_put(S0, IR);
            if (IR.k == 1) income_put(S1, IR);
        }
        // (opaque to the compiler from here on: kernel-argument loads are otherwise rematerialised in the loop)
        if (TOL) {   // (the tolerance form of the month reads the netted amount only)
            asm volatile("" : "+s"(S0.amount_keep), "+s"(S0.start_month), "+s"(S0.end_month), "+s"(S0.indexed), "+s"(S0.lock_slot));
            asm volatile("" : "+s"(S1.amount_keep), "+s"(S1.start_month), "+s"(S1.end_month), "+s"(S1.indexed), "+s"(S1.lock_slot));
        } else {
            asm volatile("" : "+s"(S0.amount), "+s"(S0.keep), "+s"(S0.start_month), "+s"(S0.end_month), "+s"(S0.indexed), "+s"(S0.lock_slot));
            asm volatile("" : "+s"(S1.amount), "+s"(S1.keep), "+s"(S1.start_month), "+s"(S1.end_month), "+s"(S1.indexed), "+s"(S1.lock_slot));
        }
    }
    // Stream form kStreamsInRegs (the host gives it to a launch whose kept records are at most two, all inflation-indexed):
    // the records are read once and pinned in SGPRs like S0 / S1 above — 8 SGPRs, against the 8 that the list's pointer,
    // counter and temporaries held.  An absent record has length 0.
    if constexpr (kSIR) {
        auto to_row = [&](int32_t m) { return m > INT32_MAX - wm ? INT32_MAX : m + wm; };
        // (the host gives 0 <= start <= end; a record with end < start has the empty window the loop form's two tests give it)
        auto window_months = [](int first, int end) { return end > first ? (unsigned)(end - first) : 0u; };
        SR = StreamRegs{0.0, 0.0, 0, 0, 0u, 0u};
        if (P.n_streams > 0) { SR.a0 = P.streams[0].amount_keep; SR.s0 = to_row(P.streams[0].start_month); SR.n0 = window_months(SR.s0, to_row(P.streams[0].end_month)); }
        if (P.n_streams > 1) { SR.a1 = P.streams[1].amount_keep; SR.s1 = to_row(P.streams[1].start_month); SR.n1 = window_months(SR.s1, to_row(P.streams[1].end_month)); }
        asm volatile("" : "+s"(SR.a0), "+s"(SR.s0), "+s"(SR.n0));
        asm volatile("" : "+s"(SR.a1), "+s"(SR.s1), "+s"(SR.n1));
    }
    // PHASE 5: this wave's spending level, an SGPR (kernel-argument array, wave-uniform index)
    const double fan_expenses = kGrid ? cell->levels[fan_j] : kExpFan ? io.fan_expenses[fan_j] : 0.0;
    int ruin_bin = pre_fail ? 0 : -1;
    // OUT: YearsToRuin as an integer, 12 x the column's value (-1: none).  0 = a pre-retirement tax failure, fail_rmi + 1 = a
    // failure inside retirement, 12 ry = a terminal-settlement failure: one conversion and one IEEE division in the epilogue
    // give the bits a summary launch stores (12 ry / 12 is exact)
    if constexpr (OUT) RM.month = pre_fail ? 0 : -1;
    int done_years = 0;  // completed (observed) retirement years = non-NaN WR entries
    int year = 0;
    if (kSliced && seg_resumed) {   // flags of the hand-over state: alive | succeeded << 1 | (ruin_bin + 1) << 8 | done_years << 24
        alive = (seg_state_flags & 1ull) != 0ull;
        succeeded = (seg_state_flags & 2ull) != 0ull;
        ruin_bin = (int)((seg_state_flags >> 8) & 0xFFFFull) - 1;
        done_years = (int)(seg_state_flags >> 24);
        year = y_begin;
    }
    // ---- PAIRS (kPairs: the consumer wave of a screened launch's split re-run, either form) ----
    // One consumer wave issues in order, and in the 64-path form it is alone on its SIMD: every scalar instruction of its
    // month stands on the path's dependent chain, where the throughput kernels' eight waves hide it.  So the whole path, both
    // loops, is restated here with the month's wave-uniform bookkeeping taken off the month (mcr_events.h):
    //  - EVENT ROW.  The row is compared with the next row at which anything happens, once; only there the priority falls or
    //    an income window's flag flips.  The month reads the two flags; the income FMAs stay FMAs behind scalar branches, in
    //    list order.
    //  - PAIRS.  Twelve is even, so a retirement month's row has the parity of working_months for the whole path: the loop is
    //    chosen once on it and runs two months to an iteration, like the accumulation.  The barrier stands at a fixed place
    //    of the body, the stage buffer alternates by a toggled offset, the vote is a pair counter tested once a pair.
    //    THE BARRIER SCHEDULE IS THE OTHER KERNELS' begin_month's: barrier p at row 2 p, in front of that row's month, for
    //    every p < ceil(total_months / 2) until a vote has ended the workgroup; a vote at every kSplitVotePairs-th barrier from
    //    barrier 0 on, on lane_alive as the retirement year began with it (tests/test_screened_pairs_cpu.py holds the loops below,
    //    restated on the host, to the producers' schedule).  That restatement (tests/screened_pairs_model.cpp: paired_consumer) is a
    //    COPY of the loops below, not this code: any change to their structure — where handover() stands in a body, the
    //    accumulation's odd tail, the `dead` tests — goes into the copy first and passes there BEFORE a GPU run; a barrier too
    //    many or too few hangs the workgroup.
    //  - FACTORS EARLY.  The six staged factors of a pair are read directly behind its barrier, into registers: no month
    //    behind the first waits for LDS at its head.
    // The arithmetic of a lane, its order and every rounding are the other loops': the statements are theirs, less what a
    // count-only kernel without an annual-gains tax never reads.
    if constexpr (kPairs) {
        static_assert(kMPY % 2 == 0, "a retirement year is a whole number of pairs");
        constexpr bool kSel = true;     // the seller's selects of the month's rebalance on an SGPR-pair mask (rebalance_tol's MASKSEL)
        const EventPlan EP{prio_t1, prio_t2, prio_t3, SR.s0, SR.n0, SR.s1, SR.n1};
        EventRow EV = event_begin(EP);
        PairCursor PC{0, 0u};
        int row = 0;
        int dead = 0;          // the workgroup has voted to stop (wave-uniform: an SGPR, not a lane mask)
        double f0 = 0.0, f1 = 0.0, f2 = 0.0, f3 = 0.0, f4 = 0.0, f5 = 0.0;   // the pair in hand: g1, ginf, g2 of its even row, then of its odd row
        auto handover = [&]() __attribute__((always_inline)) {     // barrier PC.pair, then the pair it hands over
            if (dead) return;
            if (pair_votes(PC, kSplitVotePairs)) {
                const int any = __syncthreads_or(__builtin_amdgcn_ballot_w64(lane_alive) != 0ull ? 1 : 0);
                if (__builtin_amdgcn_readfirstlane(any) == 0) { dead = 1; return; }
            } else __syncthreads();
            const double* const c = stage + PC.off;
            f0 = c[0]; f1 = c[kPaths]; f2 = c[2 * kPaths]; f3 = c[3 * kPaths]; f4 = c[4 * kPaths]; f5 = c[5 * kPaths];
            pair_advance(PC, (unsigned)kStageLen);
        };
        auto events = [&]() __attribute__((always_inline)) {
            if (row == EV.next) {
                const int p = event_fire(EV, EP, row);
                if (p == 2) __builtin_amdgcn_s_setprio(2);
                else if (p == 1) __builtin_amdgcn_s_setprio(1);
                else if (p == 0) __builtin_amdgcn_s_setprio(0);
            }
        };
        // the factors of the pair's even (half 0) or odd (half 1) row; `half` is a constant at every call
        auto factors = [&](int half, double& g1, double& ginf, double& g2) __attribute__((always_inline)) {
            g1 = half ? f3 : f0; ginf = half ? f4 : f1; g2 = half ? f5 : f2;
        };
        // accumulation (:513-579), month m = row + 1; moy = months of the plan year behind it
        int moy = 0;
        auto acc_month = [&](int m, int half) __attribute__((always_inline)) {
            if (P.contrib_grows && moy == 0 && m > 1) {                    // :514-517
                asm volatile("");
                contrib *= P.contrib_growth_factor;
            }
            events();
            double g1, ginf, g2;
            factors(half, g1, ginf, g2);
            market_step<ANNUAL, TOL>(g1, ginf, g2, b1, b2, gacc1, gacc2, infl); // :534-538
            const double k1 = contrib * (kOwnAlloc ? WA.alloc1 : P.alloc1);   // :540-542
            const double k2 = contrib - k1;                                // :543
            b1 += k1; c1 += k1; b2 += k2; c2 += k2;                        // :544-547
            month_rebalance_tol<TANY, MM, kFastMonth, EQR, kSel>(WA, P, L, b1, c1, b2, c2);  // :549-553
            if (++moy == kMPY) {                                           // :557
                moy = 0;
                pre_fail |= month_annual_gain_taxes<false, TANY, ANNUAL, T1, T2, MM, TOL, EQR>(WA, P, L, b1, c1, b2, c2, gacc1, gacc2);  // :558-573
                gacc1 = 0.0; gacc2 = 0.0;                                  // :578-579
            }
            ++row;
        };
        {
            int m = 1;
            for (; m < wm; m += 2) { handover(); acc_month(m, 0); acc_month(m + 1, 1); }
            if (m == wm) { handover(); acc_month(m, 0); }        // (working_months odd: the pair's second row is retirement's first)
        }
        // decumulation (:632-868)
        alive = !pre_fail; succeeded = !pre_fail; ruin_bin = pre_fail ? 0 : -1;
        const int ye_mi = kMPY - 1 - wm % kMPY;      // the month of a retirement year in which a year of the plan ends
        auto ret_month = [&](int mi, int half, bool& yfail) __attribute__((always_inline)) {
            events();
            if (alive && !yfail) {
                const double price = infl;                                 // :644
                const double expenses = P.monthly_expenses * price;        // :645-647
                double income = expenses;                                  // :649 (tolerance form: runs down from the expenses)
                if (EV.w0) { asm volatile(""); income = __builtin_fma(-SR.a0, price, income); }
                if (EV.w1) { asm volatile(""); income = __builtin_fma(-SR.a1, price, income); }
                const double need = fmax(0.0, income);                     // :679-682
                bool stop = false;
                if (b1 + b2 <= kEps && need > kEps) {                      // :684-690 (FAIL-1, no shock consumed)
                    yfail = true; stop = true;
                }
                auto tol_month = [&](auto fast_tag) __attribute__((always_inline)) {   // (the other loop's, less the summary columns)
                    constexpr bool FAST = decltype(fast_tag)::value;
                    const double cap = capacity_tol<T1, T2, MM, FAST>(b1, c1, L.real_rate1, b2, c2, L.real_rate2);   // :726-738
                    const double target = fmin(need, cap);                            // :739-742
                    bool fail = need > kEps && target < need - kEps;                  // :743-748 (FAIL-3) = :784-790 (FAIL-4)
                    double phi = target * recip_nr<false>(cap);                       // :750-765
                    if (!FAST && wave_any(!(cap > kEps))) {                           // the dust sub-case
                        if (!(cap > kEps)) {
                            MCR_MASKED_MOVE;
                            double cap1, cap2, gw1, nw1, gw2, nw2;
                            net_liquidation_values2<T1, T2, MM>(b1, c1, L.real_rate1, b2, c2, L.real_rate2, cap1, cap2);
                            const double xcap = cap1 + cap2, xtarget = fmin(need, xcap);
                            const double prop1 = xcap > kEps ? fdiv<false>(cap1, xcap) : (kOwnAlloc ? WA.alloc1 : P.alloc1);
                            withdraw2<T1, T2, MM>(b1, c1, xtarget * prop1, L.real_rate1, gw1, nw1,
                                                  b2, c2, xtarget * (1.0 - prop1), L.real_rate2, gw2, nw2);
                            fail = need > kEps && (xtarget < need - kEps || nw1 + nw2 < need - kEps);
                            phi = 0.0;
                        }
                    }
                    if (fail) yfail = true;
                    sell_fraction_tol<MM, FAST>(phi, b1, c1, b2, c2);                 // :757-776
                    month_rebalance_tol<TANY, MM, kFastMonth, EQR, kSel>(WA, P, L, b1, c1, b2, c2);   // :792-796
                    if (!yfail && mi == ye_mi) {                                      // :798-804
                        const bool tf = month_annual_gain_taxes<false, TANY, ANNUAL, T1, T2, MM, true, EQR>(WA, P, L, b1, c1, b2, c2, gacc1, gacc2);  // :805-818
                        gacc1 = 0.0; gacc2 = 0.0;                                     // :819-820
                        yfail = yfail || tf;                                          // :821-822
                    }
                };
                if (!stop) {
                    double g1, ginf, g2;
                    factors(half, g1, ginf, g2);
                    market_step<ANNUAL, TOL>(g1, ginf, g2, b1, b2, gacc1, gacc2, infl);  // :706-714
                    if (kFastMonth && !wave_any(fmin(b1, b2) <= P.fast_floor)) {
                        tol_month(std::true_type{});
                    } else {
                        if (b1 + b2 <= kEps && need > kEps) {              // :717-724 (FAIL-2)
                            MCR_MASKED_MOVE;
                            b1 = fmax(0.0, b1); b2 = fmax(0.0, b2);
                            yfail = true; stop = true;
                        }
                        if (!stop) tol_month(std::false_type{});
                    }
                }
            }
            ++row;
        };
        auto ret_years = [&](auto odd_tag) __attribute__((always_inline)) {
            constexpr bool ODD = decltype(odd_tag)::value;     // the parity of every row wm + 12 year + mi with mi even
            for (; year < ry; ++year) {
                lane_alive = alive;
                if (dead) break;
                bool yfail = false;                            // :638
#pragma nounroll
                for (int mi = 0; mi < kMPY; mi += 2) {
                    if constexpr (ODD) {
                        ret_month(mi, 1, yfail);
                        handover();
                        ret_month(mi + 1, 0, yfail);
                    } else {
                        handover();
                        ret_month(mi, 0, yfail);
                        ret_month(mi + 1, 1, yfail);
                    }
                }
                if (alive) {                                   // :830-868, the counts' part
                    if (yfail) { succeeded = false; ruin_bin = 1 + year; alive = false; }
                    else done_years = year + 1;
                }
            }
        };
        if (wm & 1) ret_years(std::true_type{}); else ret_years(std::false_type{});
    }
    for (; !kPairs && year < (kSliced ? y_end : ry); ++year) {
        if (!SPLIT && __builtin_amdgcn_ballot_w64(alive) == 0ull) break;  // every lane of this wave has failed: nothing left to simulate
        if (SPLIT) { lane_alive = alive; if (wg_dead) break; }           // (SPLIT: the wave keeps pace with its producers' barriers until the workgroup votes to stop)
        if constexpr (kWaveRule) rule_year_from(RS, FR, year, valid, alive, b1, b2, infl, li);   // (PHASE 11, PHASE 6 with RULE: the wave's own rule and year counts, no multiplier row)
        else if constexpr (kBinsRule) rule_year_binned(RS, YB, year, valid, alive, b1, b2, infl, li);   // (MODE 3: the record's rule; m binned, no multiplier row)
        else
        rule_year(RS, io, year, valid, alive, b1, b2, infl, li);      // (RULE: the year's decision, counts and multiplier row; nothing in every other kernel)
        double tg1 = 0.0, tg2 = 0.0, treal = 0.0;  // :635-637
        bool yfail = false;                        // :638
        int fail_rmi = 0;
        for (int mi = 0; mi < kMPY; ++mi) {
            const int rmi = year * kMPY + mi;  // :641-643
            if constexpr (kGlide) glide_row<TOL, EQR>(WA, P, L);       // (PHASE 13, GLIDE: row wm + rmi's weight)
            begin_month(month_row(SC, wm + rmi));
            if (alive && !yfail) {
                double g1, ginf, g2;
                if (kStaged) growth(month_row(SC, wm + rmi), g1, ginf, g2);    // staged factors: the LDS reads are issued early
                const double price = infl;                             // :644
                // (RULE: the multiplier comes in HERE, not inside tol_month: (monthly_expenses m) price, so that m == 1.0 leaves every bit alone)
                const double expenses = (kExpFan ? rule_scaled(RS, fan_expenses) : kScnFan ? rule_scaled(RS, scn_expenses) : rule_scaled(RS, P.monthly_expenses)) * price;   // :645-647
                // exact form: income accumulates (:649-677) and need = max(0, expenses - income); tolerance form: `income` runs
                // DOWN from the expenses, one FMA per indexed stream ((amount keep) price), one subtraction per frozen stream
                // (its slot holds the netted amount): need = max(0, what is left)
                double income = TOL ? expenses : 0.0;                  // :649
                auto stream_income = [&](const DevStream& S) {
                    if (rmi < S.start_month || rmi >= S.end_month) return;    // :653-658
                    double nominal = 0.0;
                    if (S.indexed) {
                        if (TOL) { income = __builtin_fma(-S.amount_keep, price, income); return; }
                        nominal = S.amount * price;                    // :661-665
                    } else if (!XS || S.lock_slot < P.n_lock_slots) {      // (wave-uniform; without XS every slot is an LDS column)
                        double* slot = lock_lds + (size_t)S.lock_slot * kPaths + tid;
                        if (rmi == S.start_month) *slot = (TOL ? S.amount_keep : S.amount) * price;  // :667-671 (first active month)
                        nominal = *slot;                               // :672-674
                    } else {                                           // a slot beyond the LDS budget: the lane's column of the overflow block
                        double* slot = P.lock_overflow + (size_t)(S.lock_slot - P.n_lock_slots) * (size_t)P.lock_stride + (size_t)local;
                        if (rmi == S.start_month) *slot = (TOL ? S.amount_keep : S.amount) * price;
                        nominal = *slot;
                    }
                    if (TOL) income -= nominal;
                    else income += nominal * S.keep;                   // :675-677
                };
                int s = 0;
                if (kStreamRegs) {      // the first two streams sit in SGPRs for the whole launch (see S0, S1 above)
                    if (P.n_streams > 0) stream_income(S0);
                    if (P.n_streams > 1) stream_income(S1);
                    s = 2;
                }
                if constexpr (kSIR && SPLIT && LIST) {   // the split re-run: the same two tests on the month's own row (it keeps no running counters)
                    if ((unsigned)(wm + rmi - SR.s0) < SR.n0) { asm volatile(""); income = __builtin_fma(-SR.a0, price, income); }
                    if ((unsigned)(wm + rmi - SR.s1) < SR.n1) { asm volatile(""); income = __builtin_fma(-SR.a1, price, income); }
                } else
                if constexpr (kSIR) {   // the whole list: two indexed records in SGPRs, the same FMAs in list order
                    // (wave-uniform: scalar branches, not selects; one unsigned compare tests both ends of a window)
                    if ((unsigned)(SC.row - SR.s0) < SR.n0) { asm volatile(""); income = __builtin_fma(-SR.a0, price, income); }
                    if ((unsigned)(SC.row - SR.s1) < SR.n1) { asm volatile(""); income = __builtin_fma(-SR.a1, price, income); }
                } else if constexpr (kIncFan) {   // the list in its order, this wave's version of record IR.k in its place
                    for (; s < P.n_streams; ++s) {
                        DevStream S = P.streams[s];
                        if (s == IR.k) income_put(S, IR);
                        stream_income(S);
                    }
                } else for (; s < P.n_streams; ++s) stream_income(P.streams[s]);    // :650 (wave-uniform; the record is re-read from the kernel arguments)
                if (XS && P.n_extra_streams > 0) {                                 // the rest of the list (config.py:99 has no length limit): scalar loads from the device table
                    const DevStreamTable xs = (DevStreamTable)P.extra_streams;
                    for (int x = 0; x < P.n_extra_streams; ++x) {
                        DevStream S;
                        S.amount = xs[x].amount; S.keep = xs[x].keep; S.amount_keep = xs[x].amount_keep; S.start_month = xs[x].start_month;
                        S.end_month = xs[x].end_month; S.indexed = xs[x].indexed; S.lock_slot = xs[x].lock_slot;
                        stream_income(S);
                    }
                }
                const double need = fmax(0.0, TOL ? income : expenses - income);      // :679-682
                bool stop = false;
                if (b1 + b2 <= kEps && need > kEps) {                  // :684-690 (FAIL-1, no shock consumed)
                    yfail = true; stop = true;
                }
                // the withdrawal in closed form (mcr_device.h): both assets sell the fraction target / capacity.  FAST: no active
                // lane of the wave holds a balance <= 1e-6 after the market step (kFastMonth below)
                auto tol_month = [&](auto fast_tag) {
                    constexpr bool FAST = decltype(fast_tag)::value;
                    const double cap = capacity_tol<T1, T2, MM, FAST>(b1, c1, L.real_rate1, b2, c2, L.real_rate2);   // :726-738
                    const double target = fmin(need, cap);                            // :739-742
                    bool fail = need > kEps && target < need - kEps;                  // :743-748 (FAIL-3) = :784-790 (FAIL-4): the net cash is the target
                    double phi = target * recip_nr<false>(cap);                       // :750-765
                    // :766, :777: gross withdrawals of the month (an asset holding <= 1e-6 is left alone, :218-219: it sells nothing)
                    double gross = phi * (FAST ? b1 + b2 : (b1 > kEps ? b1 : 0.0) + (b2 > kEps ? b2 : 0.0));
                    // The dust sub-case (mcr_device.h; FAST excludes it): the reference's allocation-weight split (:739-790) in the
                    // exact forms, FAIL-3 and FAIL-4 on its values; phi = 0 leaves the result alone below.  Behind a wave ballot: the
                    // SPLIT variants (MM = false) would otherwise select-convert the block and run it every month.
                    if (!FAST && wave_any(!(cap > kEps))) {
                        if (!(cap > kEps)) {
                            MCR_MASKED_MOVE;
                            double cap1, cap2, gw1, nw1, gw2, nw2;
                            net_liquidation_values2<T1, T2, MM>(b1, c1, L.real_rate1, b2, c2, L.real_rate2, cap1, cap2);
                            const double xcap = cap1 + cap2, xtarget = fmin(need, xcap);
                            const double prop1 = xcap > kEps ? fdiv<false>(cap1, xcap) : (kOwnAlloc ? WA.alloc1 : P.alloc1);
                            withdraw2<T1, T2, MM>(b1, c1, xtarget * prop1, L.real_rate1, gw1, nw1,
                                                  b2, c2, xtarget * (1.0 - prop1), L.real_rate2, gw2, nw2);
                            fail = need > kEps && (xtarget < need - kEps || nw1 + nw2 < need - kEps);
                            phi = 0.0;
                            gross = gw1 + gw2;
                        }
                    }
                    if (fail) yfail = true;
                    if (kSummary) {
                        tg1 += gross;
                        treal = __builtin_fma(gross * infl_ret, recip_nr<false>(fmax(price, kEps)), treal);  // :778-782
                    }
                    sell_fraction_tol<MM, FAST>(phi, b1, c1, b2, c2);                 // :757-776
                    month_rebalance_tol<TANY, MM, kFastMonth, EQR>(WA, P, L, b1, c1, b2, c2);   // :792-796
                    // (the counters' form in a branch of its own: named in the other kernels' month, SC would be one more capture of
                    // this lambda, which is enough to reorder their code)
                    if constexpr (kScalarCounters) {
                        if (!yfail && mi == SC.ye_mi) {                               // :798-804
                            const bool tf = month_annual_gain_taxes<false, TANY, ANNUAL, T1, T2, MM, true, EQR>(WA, P, L, b1, c1, b2, c2, gacc1, gacc2);  // :805-818
                            gacc1 = 0.0; gacc2 = 0.0;                                 // :819-820
                            yfail = yfail || tf;                                      // :821-822
                        }
                    } else
                    if (!yfail && (wm + rmi + 1) % kMPY == 0) {                       // :798-804
                        const bool tf = month_annual_gain_taxes<false, TANY, ANNUAL, T1, T2, MM, true, EQR>(WA, P, L, b1, c1, b2, c2, gacc1, gacc2);  // :805-818
                        gacc1 = 0.0; gacc2 = 0.0;                                     // :819-820
                        yfail = yfail || tf;                                          // :821-822
                    }
                };
                if (!stop) {
                    if (!kStaged) growth(month_row(SC, wm + rmi), g1, ginf, g2);      // :692-705 (sequential generators draw here)
                    market_step<ANNUAL, TOL>(g1, ginf, g2, b1, b2, gacc1, gacc2, infl);  // :706-714
                    // Both balances > fast_floor >= 1e-6 in every active lane: FAIL-2 cannot fire (b1 + b2 > 1e-6), no capacity is
                    // zeroed, each is > 0 (cap_i >= b_i (1 - r_i), r_i <= 1 - 1e-6 in the tolerance form), no asset is left alone,
                    // and cap >= (b1 + b2) (1 - r_max) > 2e-6: no lane is in the dust sub-case.
                    if (kFastMonth && !wave_any(fmin(b1, b2) <= P.fast_floor)) {
                        tol_month(std::true_type{});
                    } else {
                        if (b1 + b2 <= kEps && need > kEps) {          // :717-724 (FAIL-2)
                            MCR_MASKED_MOVE;                          // keep it a branch: no lane takes it in most months
                            b1 = fmax(0.0, b1); b2 = fmax(0.0, b2);
                            yfail = true; stop = true;
                        }
                        if (!stop && TOL) tol_month(std::false_type{});
                    }
                }
                if (!stop && !TOL) {
                    double cap1, cap2;
                    net_liquidation_values2<T1, T2, MM>(b1, c1, L.real_rate1, b2, c2, L.real_rate2, cap1, cap2);  // :726-737
                    const double cap = cap1 + cap2;                                   // :738
                    const double target = fmin(need, cap);                            // :739-742 (need, cap >= 0: the max(0, .) is a no-op)
                    if (need > kEps && target < need - kEps) yfail = true;            // :743-748 (FAIL-3)
                    double prop1 = fdiv<false>(cap1, cap);                            // :750-754
                    if (!(cap > kEps)) { MCR_MASKED_MOVE; prop1 = kOwnAlloc ? WA.alloc1 : P.alloc1; }   // (exec-masked move, not a select)
                    const double prop2 = 1.0 - prop1;                                 // :755
                    double gw1, nw1, gw2, nw2;
                    withdraw2<T1, T2, MM>(b1, c1, target * prop1, L.real_rate1, gw1, nw1,  // :757-765
                                     b2, c2, target * prop2, L.real_rate2, gw2, nw2);  // :768-776
                    tg1 += gw1;                                                       // :766
                    tg2 += gw2;                                                       // :777
                    if (kSummary) treal += fdiv<false>((gw1 + gw2) * infl_ret, fmax(price, kEps));  // :778-782
                    if (need > kEps && nw1 + nw2 < need - kEps) yfail = true;         // :784-790 (FAIL-4)
                    rebalance_path<TANY, MM>(L, b1, c1, b2, c2);                      // :792-796
                    if (!yfail && (wm + rmi + 1) % kMPY == 0) {                       // :798-804
                        const bool tf = month_annual_gain_taxes<false, TANY, ANNUAL, T1, T2, MM>(WA, P, L, b1, c1, b2, c2, gacc1, gacc2);  // :805-818
                        gacc1 = 0.0; gacc2 = 0.0;                                     // :819-820
                        yfail = yfail || tf;                                          // :821-822
                    }
                }
                if (yfail) fail_rmi = rmi;  // :825-828, :844-847
            }
            if constexpr (kScalarCounters) ++SC.row;
        }
        // ---- year end (:830-868); lanes that were already dead pad with 0 / NaN (:902-916,:934-935) ----
        double sample = 0.0;
        unsigned long long wr_bits = kNanBits;
        if (alive) {
            const double ygw = tg1 + tg2;                                              // :830-832
            const double wr_pct = start_balance > kEps ? (treal / start_balance) * 100.0 : 0.0;  // :834-840
            if (year == 0) {                                                           // :852-856, :861-865
                if (kSumLds) { sum_col[0] = ygw; sum_col[kBlock] = treal; }
                else { fy_gross = ygw; fy_real = treal; }
            }
            if (yfail) {
                succeeded = false;                                                     // :843
                if (kSumLds) sum_col[2 * kBlock] = (double)(fail_rmi + 1) / (double)kMPY;  // :825-827, :844-847
                else ytr_bits = f64_bits((double)(fail_rmi + 1) / (double)kMPY);
                if constexpr (OUT) RM.month = fail_rmi + 1;
                ruin_bin = 1 + year;
                sample = fmax(0.0, b1 + b2);                                           // :848
                alive = false;                                                         // :857
            } else {
                wr_bits = f64_bits(wr_pct);                                            // :859
                sample = b1 + b2;                                                      // :867
                done_years = year + 1;
            }
        }
        if constexpr (kBins) {   // the year's row of all three tables behind one barrier; a last row that is written again below waits for that value
            // (ry >= 1 on every launch: query_sizes, through derive_params, rejects retirement_years <= 0 — so the year of row T - 1
            //  always comes up here or in the pad loop, and the row is binned exactly once)
            const bool defer = P.total_months % kMPY != 0 && year == ry - 1;     // wave-uniform
            if (defer) YB.last = sample;
            year_bins_row(io.yb, YB.L, YB.k++, valid, t_idx, !defer, sample, infl, year, wr_bits);
        } else put_sample(t_idx, sample, infl);  // dead lanes: 0 / px = 0 (:906-916, :928-931)
        ++t_idx;
        if (kTraj && valid && wrt) store_bits(&wrt[(int64_t)year * stride + (int64_t)li], wr_bits);  // :851, :859, :934-935
    }
    for (; year < (kSliced ? y_end : ry); ++year) {  // the whole wave failed early: pad (:902-916, :934-935)
        if constexpr (kBins) year_bins_row(io.yb, YB.L, YB.k++, valid, t_idx++, !(P.total_months % kMPY != 0 && year == ry - 1), 0.0, infl, year, kNanBits);
        else put_sample(t_idx++, 0.0, infl);
        if (kTraj && valid && wrt) store_bits(&wrt[(int64_t)year * stride + (int64_t)li], kNanBits);
        if constexpr (!kWaveRule && !kBinsRule) rule_pad(RS, io, year, valid, li);   // (PHASE 11, PHASE 6 with RULE and MODE 3 write no multiplier row)
    }
    if (kSliced && seg >= 0 && seg < io.seg_q - 1) {
        // Not the block's last segment: raise the flag, to 1 with the lanes' state handed over, or to 2 (every wave gets here:
        // no early return above).  SINGLE WRITER: only segment 0 and a segment that resumed from flag 1 write the block's one
        // slot; a segment that recomputed (its predecessor's flag stayed 0 for the whole budget, or was 2) leaves the slot alone
        // and raises 2, and its successors recompute too.  So the writers of a slot are segments 0, 1, ..., j, each the end of a
        // chain of flag-1 hand-overs back to segment 0: segment k reads and then writes (each lane its own column, in program
        // order) only after its acquire of flag k - 1 == 1, which segment k - 1 released after its own write.  The slot's reads
        // and writes are totally ordered by those release / acquire pairs: a resumed segment reads exactly its predecessor's
        // state, never a stale or torn one.  (A late predecessor of a segment that timed out still writes, but no one reads the
        // slot after that: the timed-out segment raised 2, and every later segment of the block recomputes.)
        // (seg_resumed re-read from LDS: kept live to here it costs the summary variants 3 VGPRs; an atomic load, or the compiler
        // forwards the first load)
        const bool hand_over = seg == 0 || __hip_atomic_load(&seg_ok_s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0;
        if (hand_over) {
            *seg_at(0) = b1; *seg_at(1) = b2; *seg_at(2) = c1; *seg_at(3) = c2;
            if (ANNUAL) { *seg_at(4) = gacc1; *seg_at(5) = gacc2; }
            *seg_at(6) = infl;
            store_bits(seg_at(7), (alive ? 1ull : 0ull) | (succeeded ? 2ull : 0ull) | ((unsigned long long)(ruin_bin + 1) << 8) | ((unsigned long long)done_years << 24));
            store_bits(seg_at(8), ((unsigned long long)carry.w3 << 32) | (unsigned long long)carry.w2);
            for (int k = 0; k < P.n_lock_slots; ++k) *seg_at(kSegFixedFields + k) = lock_lds[(size_t)k * kBlock + tid];
            if (MODE >= 1) {
                *seg_at(9) = start_balance; *seg_at(10) = infl_ret;
                *seg_at(11) = sum_col[0]; *seg_at(12) = sum_col[kBlock]; *seg_at(13) = sum_col[2 * kBlock];
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        }
        __syncthreads();
        if (threadIdx.x == 0)
            __hip_atomic_store(io.seg_flags + (size_t)seg_block * (size_t)io.seg_q + (size_t)seg, hand_over ? 1u : 2u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        return;
    }

    // ---- terminal partial tax period (:873-898) ----
    if (P.total_months % kMPY != 0) {  // wave-uniform
        if (succeeded) {
            const bool tf = month_annual_gain_taxes<false, TANY, ANNUAL, T1, T2, MM, TOL, EQR>(WA, P, L, b1, c1, b2, c2, gacc1, gacc2);  // :880-893
            if (tf) {                                                            // :894-896
                succeeded = false; ruin_bin = ry + 1;
                if (kSumLds) sum_col[2 * kBlock] = (double)ry; else ytr_bits = f64_bits((double)ry);
                if constexpr (OUT) RM.month = kMPY * ry;
            }
            if constexpr (kBins) YB.last = b1 + b2;                              // (binned below: no barrier under a lane mask)
            else put_sample(P.trajectory_len - 1, b1 + b2, infl);                // :897-898
        }
        if constexpr (kBins) year_bins_row(io.yb, YB.L, YB.k++, valid, P.trajectory_len - 1, true, YB.last, infl, -1, kNanBits);
    }
    const double final_balance = fmax(0.0, b1 + b2);  // :900, :941

    // ---- outputs ----
    if (kSumLds) { fy_gross = sum_col[0]; fy_real = sum_col[kBlock]; ytr_bits = f64_bits(sum_col[2 * kBlock]); }
    if (kSummary && valid) {
        const mcr_outputs& o = io.out;
        if (o.start_balance) o.start_balance[li] = start_balance;
        if (o.final_balance) o.final_balance[li] = final_balance;
        if (o.years_to_ruin) store_bits(&o.years_to_ruin[li], ytr_bits);
        if (o.first_year_gross_withdrawal) o.first_year_gross_withdrawal[li] = fy_gross;
        if (o.first_year_real_gross_withdrawal) o.first_year_real_gross_withdrawal[li] = fy_real;
        if (o.inflation_at_retirement) o.inflation_at_retirement[li] = infl_ret;
        if (o.success) o.success[li] = succeeded ? 1 : 0;
    }
#ifdef MCR_K1_TIMELINE   // the stamps go to a buffer of their own (the otherwise unused path_seeds pointer of a Philox launch)
    if (MODE == 0 && RNG == 0 && io.path_seeds && (threadIdx.x & 63) == 0) {
        unsigned long long* tl = (unsigned long long*)io.path_seeds + ((size_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 3;
        tl[0] = tl_t0; tl[1] = wall_clock64();
        tl[2] = ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32) | __builtin_amdgcn_s_getreg(4 | (31 << 11));  // XCC_ID | HW_ID
    }
#endif
    // success count: wave ballot + popcount -> LDS -> one atomic per workgroup
    const unsigned long long ok = __builtin_amdgcn_ballot_w64(valid && succeeded);
    if (kFan) {   // one count per level: consumer wave j -> blk[j] -> counters of level j (the producer has returned)
        if ((threadIdx.x & 63) == 0) blk[fan_j] = (unsigned int)__popcll(ok);
        if constexpr (kScnFan) {
            // PHASE 8 / 9 / 10 read the launch constants of this epilogue from the kernel-argument segment HERE (late_arg) instead
            // of through `io`, whose fields are loaded at kernel entry and held in SGPRs through the month loop: the mask pointer
            // of the joint probes then costs no register there, and the three other values stop costing theirs
            const int fan_n = late_arg<int32_t>(offsetof(KernelIO, fan_n));
            const uint64_t n_paths = late_arg<uint64_t>(offsetof(KernelIO, n_paths));
            uint64_t* const fan_ctr = late_arg<uint64_t*>(offsetof(KernelIO, out) + offsetof(mcr_outputs, counters));
            // joint probes keep the ballot: bit b of word path_block of row j = path 64 path_block + b under option j
            uint64_t* const fan_masks = late_arg<uint64_t*>(offsetof(KernelIO, fan_masks));
            if (fan_masks && (threadIdx.x & 63) == 0) fan_masks[(size_t)fan_j * ((n_paths + 63) >> 6) + path_block] = ok;
            // outcome probes keep the path's outcome: one 512-byte wave store per requested row, lanes beyond n_paths store nothing.
            // final_balance = "Final Balance" where the path succeeds, else NaN (row 2 of mcr_summary_stat_rows); years_to_ruin =
            // the summary launch's column.  NaNs go out as bit patterns (the device code is built without NaN semantics).
            if constexpr (OUT) {
                double* const fan_final = late_arg<double*>(offsetof(KernelIO, fan_rows) + offsetof(KernelIO::FanRows, final_balance));
                double* const fan_ruin = late_arg<double*>(offsetof(KernelIO, fan_rows) + offsetof(KernelIO::FanRows, years_to_ruin));
                const int64_t row_stride = late_arg<int64_t>(offsetof(KernelIO, fan_rows) + offsetof(KernelIO::FanRows, row_stride));
                const uint64_t col = (uint64_t)path_block * kPaths + (threadIdx.x & 63);
                if (col < n_paths) {
                    const size_t at = (size_t)fan_j * (size_t)row_stride + (size_t)col;
                    if (fan_final) store_bits(&fan_final[at], succeeded ? f64_bits(final_balance) : kNanBits);
                    if (fan_ruin) store_bits(&fan_ruin[at], RM.month < 0 ? kNanBits : f64_bits((double)RM.month / (double)kMPY));
                }
            }
            __syncthreads();
            if (threadIdx.x < (unsigned)fan_n && fan_ctr) {
                uint64_t* c = fan_ctr + (size_t)threadIdx.x * MCR_N_COUNTERS;
                const uint64_t first = (uint64_t)path_block * kPaths;
                const uint64_t cnt = n_paths - first < (uint64_t)kPaths ? n_paths - first : (uint64_t)kPaths;
                atomicAdd((unsigned long long*)&c[MCR_CTR_SUCCESS], (unsigned long long)blk[threadIdx.x]);
                atomicAdd((unsigned long long*)&c[MCR_CTR_PATHS], (unsigned long long)cnt);
            }
            return;
        }
        __syncthreads();
        uint64_t* const fan_ctr = kGrid ? cell->counters : io.out.counters;
        if (threadIdx.x < (unsigned)io.fan_n && fan_ctr) {
            uint64_t* c = fan_ctr + (size_t)threadIdx.x * MCR_N_COUNTERS;
            const uint64_t first = (uint64_t)path_block * kPaths;
            const uint64_t cnt = io.n_paths - first < (uint64_t)kPaths ? io.n_paths - first : (uint64_t)kPaths;
            atomicAdd((unsigned long long*)&c[MCR_CTR_SUCCESS], (unsigned long long)blk[threadIdx.x]);
            atomicAdd((unsigned long long*)&c[MCR_CTR_PATHS], (unsigned long long)cnt);
        }
        return;
    }
    if ((threadIdx.x & 63) == 0) atomicAdd(&blk[0], (unsigned int)__popcll(ok));
    const bool want_bins = io.out.ruin_year_bins != nullptr || io.out.wr_obs_counts != nullptr;
    if (want_bins && valid) {
        if (ruin_bin >= 0) atomicAdd(&blk[1 + ruin_bin], 1u);
        atomicAdd(&blk[1 + (ry + 2) + done_years], 1u);
    }
    // "Final Balance" of the successful cohort on the caller's bin edges (plotting.py:44-59; np.histogram(x, bins=edges):
    // bin k = [e_k, e_k+1), the last one closed, values outside the edges dropped).  Once per path, after 10^2..10^3
    // months of arithmetic: a per-lane binary search straight over the (L2-resident) edge array costs nothing measurable.
    if ((PHASE == 0 || PHASE == 3) && n_hist > 0 && valid && succeeded) {
        const double* __restrict__ e = io.out.hist_edges;
        if (final_balance >= e[0] && final_balance <= e[n_hist]) {
            int lo = 0, hi = n_hist;             // e[lo] <= x and (hi == n_hist or x < e[hi])
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (e[mid] <= final_balance) lo = mid; else hi = mid;
            }
            atomicAdd(&blk[n_blk + lo], 1u);
        }
    }
    if constexpr (kBins) { if (io.yb.final_success && valid && succeeded) atomicAdd(&YB.L.fin[year_bins_cell(YB.L.edges, YB.L.n, final_balance)], 1u); }
    __syncthreads();
    if constexpr (kBins) year_bins_flush_final(io.yb, YB.L);
    uint64_t* ctr = io.out.counters ? io.out.counters + (kCand ? (size_t)io.cand_out[cand] * MCR_N_COUNTERS : 0) : nullptr;
    if (threadIdx.x == 0 && ctr) {
        atomicAdd((unsigned long long*)&ctr[MCR_CTR_SUCCESS], (unsigned long long)blk[0]);
        const uint64_t first = (uint64_t)path_block * kPaths;
        const uint64_t cnt = io.n_paths - first < (uint64_t)kPaths ? io.n_paths - first : (uint64_t)kPaths;
        if constexpr (LIST) {     // the list's entries in this workgroup's range
            const uint64_t list_n = *io.path_list_count;
            atomicAdd((unsigned long long*)&ctr[MCR_CTR_PATHS], (unsigned long long)(list_n - first < (uint64_t)kPaths ? list_n - first : (uint64_t)kPaths));
        } else
        atomicAdd((unsigned long long*)&ctr[MCR_CTR_PATHS], (unsigned long long)cnt);
    }
    if (want_bins) {
        for (int k = threadIdx.x; k < ry + 2; k += kPaths) {
            if (io.out.ruin_year_bins && blk[1 + k])
                atomicAdd((unsigned long long*)&io.out.ruin_year_bins[k], (unsigned long long)blk[1 + k]);
        }
        // wr_obs_counts[y] = #paths with done_years > y   (wr_df.count(axis=1), :1111-1113)
        for (int y = threadIdx.x; y < ry; y += kPaths) {
            unsigned int c = 0;
            for (int d = y + 1; d <= ry; ++d) c += blk[1 + (ry + 2) + d];
            if (io.out.wr_obs_counts && c)
                atomicAdd((unsigned long long*)&io.out.wr_obs_counts[y], (unsigned long long)c);
        }
    }
    for (int k = threadIdx.x; k < n_hist; k += kPaths)   // one global atomic per non-empty bin per workgroup (the fan-outs have returned: kPaths consumer threads)
        if (blk[n_blk + k]) atomicAdd((unsigned long long*)&io.out.hist_bins[k], (unsigned long long)blk[n_blk + k]);
}

// ---------------------------------------------------------------------------------------------
// Screening kernel of a count-only launch (mcr_screen.h; launch_screened): one path per lane, the whole path in fp32 on the
// hardware's transcendentals, no LDS tables and no stage.  The month is the closed tolerance form of path_kernel
// (capacity_tol, sell_fraction_tol, rebalance_tol, the income FMAs of the stream form) restated in fp32: selects stay selects,
// and instead of the dust fix-ups a lane becomes DOUBTFUL when a balance falls to one dollar.  (The rebalance that closes a
// tax year without an annual-gains tax comes right behind the month's own and moves a rounding's worth: it is left out.)
// The month is stated as mcr_screen.h's "month as restated" says: one net need level per window state, the price level as a
// logarithm, no dead clamps, one compare for both capacity tests, closed-form balances, a running minimum of the balances.
// The rows run four to a loop iteration, one loop per Philox form (screen_rows).  RHO0: a launch whose rho is 0 (screen_factors2).
// A lane is SAFE only if in every retirement month cap >= kScreenNeedMargin need and cap >= peak / kScreenPeakDiv, `need` and
// `cap` the month's own values and `peak` the running maximum of b1 + b2 (need <= 0: the second test alone decides, as the
// first then holds for any positive cap).  SAFE lanes are counted as path_kernel's epilogue counts a successful path whose
// every year was observed; DOUBTFUL lanes append their local index to io.list, one atomic per wave; tail lanes do neither.
// HOOK (mcr_screen_paths_rng, tests and tools): per path the class, the lowest cap / need seen and the final b1 + b2.
// Held to 8 waves per SIMD (<= 64 VGPRs), no scratch.  Wave priority falls as the path advances, as in path_kernel (laggards
// first: 8 waves a SIMD over 1.9 rounds otherwise leave the youngest to finish alone; median 2.22-2.25 -> 2.14-2.17 ms at 10^6 paths, LABNOTES R25).
struct ScreenIO {
    uint64_t seed, path_begin, n_paths;
    uint32_t stream_id, reserved;
    uint64_t* counters;          // [MCR_N_COUNTERS] or nullptr
    uint64_t* wr_obs_counts;     // [ry] or nullptr
    uint32_t* list;              // [n_paths] local indices of the doubtful paths, or nullptr (HOOK)
    uint32_t* list_count;        // zeroed before the launch
    uint8_t* cls;                // HOOK: [n_paths] MCR_SCREEN_SAFE / MCR_SCREEN_DOUBTFUL
    float* min_ratio;            // HOOK: [n_paths] lowest cap / need of the months the lane ran (+inf: no month with a need)
    float* final_total;          // HOOK: [n_paths] b1 + b2 where the lane stopped
};
// One lane's state across the path
struct ScreenLane { float b1, c1, b2, c2, lvl, peak, contrib, k1, k2, rmin, min_ratio; bool ok; };
// The four net levels as words in SGPRs, opaque to the compiler (screen_kernel): selected with s_cselect_b32.  Passed by
// value: by reference the selects become one indexed read of a 16-byte table, which the backend places in LDS
struct ScreenLevels { uint32_t e00, e10, e01, e11; };
// One month of one lane: row m (wave-uniform), its growth (screen_factors2), `moy` the accumulation month of the year
template <int TAXED, bool EQR, bool HOOK>
__device__ __forceinline__ void screen_month(const ScreenParams& S, const ScreenConsts& K, const ScreenLevels E, ScreenLane& L, int& moy, int m, float g1, float xinf, float g2) {
    constexpr bool T1 = (TAXED & 1) != 0, T2 = (TAXED & 2) != 0;
    if (m < S.working_months) {                              // accumulation (:513-553)
        if (moy == kMPY) {
            moy = 0;
            if (S.contrib_grows) {
                asm volatile("");                            // (keeps the yearly step a scalar branch: if-converted, it costs six VALU every month)
                L.contrib *= S.contrib_growth_factor; L.k1 = L.contrib * S.alloc1; L.k2 = L.contrib - L.k1;
            }
        }
        ++moy;
        L.b1 *= g1; L.b2 *= g2; L.lvl += xinf;
        L.b1 += L.k1; L.c1 += L.k1; L.b2 += L.k2; L.c2 += L.k2;
    } else {                                                 // decumulation (:644-796)
        const float price = __builtin_amdgcn_exp2f(L.lvl);
        const bool w0 = (unsigned)(m - S.s0) < S.n0, w1 = (unsigned)(m - S.s1) < S.n1;
        const float level = __builtin_bit_cast(float, w0 ? (w1 ? E.e11 : E.e10) : (w1 ? E.e01 : E.e00));     // (s_cselect_b32)
        const float need = price * level;                            // (level >= 0: clamped where it is derived, screen_params)
        L.b1 *= g1; L.b2 *= g2; L.lvl += xinf;
        const float v1 = T1 ? __builtin_fmaf(-__builtin_fmaxf(0.0f, L.b1 - L.c1), S.rate1, L.b1) : L.b1;
        const float v2 = T2 ? __builtin_fmaf(-__builtin_fmaxf(0.0f, L.b2 - L.c2), EQR ? S.rate1 : S.rate2, L.b2) : L.b2;
        const float cap = v1 + v2;
        L.ok = L.ok && cap >= __builtin_fmaxf(kScreenNeedMargin * need, L.peak * (1.0f / kScreenPeakDiv));      // (both tests under one compare)
        const float inv_cap = __builtin_amdgcn_rcpf(cap);
        const float phi = need * inv_cap;
        if constexpr (HOOK) { if (need > 0.0f) L.min_ratio = __builtin_fminf(L.min_ratio, cap * __builtin_amdgcn_rcpf(need)); }
        L.b1 = __builtin_fmaf(-L.b1, phi, L.b1); L.c1 = __builtin_fmaf(-L.c1, phi, L.c1);
        L.b2 = __builtin_fmaf(-L.b2, phi, L.b2); L.c2 = __builtin_fmaf(-L.c2, phi, L.c2);
    }
    L.peak = __builtin_fmaxf(L.peak, screen_rebalance<TAXED, EQR>(S, K, L.b1, L.c1, L.b2, L.c2));
    L.rmin = __builtin_fminf(L.rmin, __builtin_fminf(L.b1, L.b2));
}
// The rows of a path, four to an iteration: HALF 0 and HALF 1 of one Philox block triple straight-line, the pair carry local to
// the iteration (carried across a two-row loop's back edge it travelled between two register pairs, four v_mov a row pair, and
// the four-arm choice of half and form left three v_readfirstlane_b32 of undefined values in the loop header).  Functions over
// a state struct, not lambdas: a capturing lambda of this size is inlined too late for its captures to leave private memory,
// and every scalar select then becomes a v_cndmask.  UNIFORM: screen_factors2, chosen once outside the loop.
template <int TAXED, bool EQR, bool RHO0, bool HOOK, bool UNIFORM>
__device__ __forceinline__ void screen_rows(const ScreenParams& S, const ScreenConsts& K, const ScreenLevels E, const PhiloxPath& PQ, uint64_t seed, ScreenLane& L) {
    const int total = S.total_months;
    // laggards first, as in path_kernel: the wave's priority falls at half, three quarters and nine tenths of the path (even rows)
    const int prio_t1 = (total / 2) & ~1, prio_t2 = ((total * 3) / 4) & ~1, prio_t3 = ((total * 9) / 10) & ~1;
    int prio_next = prio_t1;
    int moy = 0;                                                     // accumulation month of the year, 0 .. 11
    auto prio = [&](int row) {
        if (row == prio_next) {
            if (row == prio_t1) __builtin_amdgcn_s_setprio(2);
            else if (row == prio_t2) __builtin_amdgcn_s_setprio(1);
            else if (row == prio_t3) __builtin_amdgcn_s_setprio(0);
            prio_next = prio_from(prio_t1, prio_t2, prio_t3, row + 2);
        }
    };
    for (int row = 0; row < total; row += 4) {
        // every lane of the wave is doubtful: nothing left to decide (asked every 16th row)
        if ((row & 12) == 0 && __builtin_amdgcn_ballot_w64(L.ok && L.rmin > kScreenMinBalance) == 0ull) break;
        PairCarry carry;
        float g[6];
        prio(row);
        screen_factors2<0, UNIFORM, RHO0>(S, K, PQ, seed, (uint32_t)row >> 2, carry, g);
        screen_month<TAXED, EQR, HOOK>(S, K, E, L, moy, row, g[0], g[1], g[2]);
        if (row + 1 >= total) break;
        screen_month<TAXED, EQR, HOOK>(S, K, E, L, moy, row + 1, g[3], g[4], g[5]);
        if (row + 2 >= total) break;
        prio(row + 2);
        screen_factors2<1, UNIFORM, RHO0>(S, K, PQ, seed, (uint32_t)row >> 2, carry, g);
        screen_month<TAXED, EQR, HOOK>(S, K, E, L, moy, row + 2, g[0], g[1], g[2]);
        if (row + 3 >= total) break;
        screen_month<TAXED, EQR, HOOK>(S, K, E, L, moy, row + 3, g[3], g[4], g[5]);
    }
}
template <int TAXED, bool EQR, bool RHO0, bool HOOK = false>
__global__ __launch_bounds__(kBlock, 8) void screen_kernel(const ScreenParams S, const ScreenIO io) {
    static_assert(TAXED >= 0 && TAXED <= 3 && (!EQR || TAXED == 3), "TAXED is path_kernel's mask; equal rates need both assets taxed");
    __shared__ unsigned int safe_s;
    if (threadIdx.x == 0) safe_s = 0u;
    __syncthreads();
    const uint64_t local = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = local < io.n_paths;
    const uint64_t path = io.path_begin + (valid ? local : io.n_paths - 1);   // tail lanes shadow the last path
    const PhiloxPath PQ = philox_path(path, io.stream_id, io.seed);           // (the whole wave is here: philox_path's ballot)
    ScreenLane L;
    L.b1 = S.b1_0; L.b2 = S.b2_0; L.c1 = L.b1; L.c2 = L.b2;
    L.lvl = 0.0f;                                                    // log2 of the price level
    L.peak = L.b1 + L.b2;
    L.contrib = S.contrib; L.k1 = L.contrib * S.alloc1; L.k2 = L.contrib - L.k1;
    L.ok = true;
    L.rmin = __builtin_fminf(L.b1, L.b2);
    L.min_ratio = __builtin_inff();
    ScreenConsts K{S.a1, S.ainf, S.aprem, S.ar1, S.ar2};
    asm volatile("" : "+v"(K.a1), "+v"(K.ainf), "+v"(K.aprem), "+v"(K.ar1), "+v"(K.ar2));      // (ScreenConsts: VGPRs for the whole path)
    ScreenLevels E{__builtin_bit_cast(uint32_t, S.e00), __builtin_bit_cast(uint32_t, S.e10), __builtin_bit_cast(uint32_t, S.e01), __builtin_bit_cast(uint32_t, S.e11)};
    asm volatile("" : "+s"(E.e00), "+s"(E.e10), "+s"(E.e01), "+s"(E.e11));                     // (ScreenLevels: SGPRs, selected as words)
    __builtin_amdgcn_s_setprio(3);
    if (PQ.hi_uniform) screen_rows<TAXED, EQR, RHO0, HOOK, true>(S, K, E, PQ, io.seed, L);
    else screen_rows<TAXED, EQR, RHO0, HOOK, false>(S, K, E, PQ, io.seed, L);                  // (a wave that straddles a multiple of 2^32 paths)
    bool ok = L.ok && L.rmin > kScreenMinBalance;
    ok = ok && L.peak < kScreenMaxTotal;
    const bool safe = valid && ok, doubt = valid && !ok;
    const unsigned long long safe_mask = __builtin_amdgcn_ballot_w64(safe), doubt_mask = __builtin_amdgcn_ballot_w64(doubt);
    const unsigned int lane = threadIdx.x & 63u;
    if (lane == 0u && safe_mask) atomicAdd(&safe_s, (unsigned int)__popcll(safe_mask));
    if (io.list && doubt_mask) {                                     // wave-uniform
        unsigned int base = 0u;
        if (lane == 0u) base = atomicAdd(io.list_count, (unsigned int)__popcll(doubt_mask));
        base = (unsigned int)__builtin_amdgcn_readfirstlane((int)base);
        const unsigned int before = __builtin_amdgcn_mbcnt_hi((unsigned int)(doubt_mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)doubt_mask, 0u));
        if (doubt) io.list[base + before] = (uint32_t)local;         // (at most n_paths entries in all: one per valid lane)
    }
    if constexpr (HOOK) {
        if (valid) {
            if (io.cls) io.cls[local] = ok ? MCR_SCREEN_SAFE : MCR_SCREEN_DOUBTFUL;
            if (io.min_ratio) io.min_ratio[local] = L.min_ratio;
            if (io.final_total) io.final_total[local] = L.b1 + L.b2;
        }
    }
    __syncthreads();
    const unsigned int n_safe = safe_s;
    if (n_safe == 0u) return;
    if (threadIdx.x == 0 && io.counters) {
        atomicAdd((unsigned long long*)&io.counters[MCR_CTR_SUCCESS], (unsigned long long)n_safe);
        atomicAdd((unsigned long long*)&io.counters[MCR_CTR_PATHS], (unsigned long long)n_safe);
    }
    // wr_obs_counts[y] = #paths with done_years > y: a SAFE path has done_years = ry, and no ruin bin
    if (io.wr_obs_counts)
        for (int y = threadIdx.x; y < S.retirement_years; y += kBlock) atomicAdd((unsigned long long*)&io.wr_obs_counts[y], (unsigned long long)n_safe);
}

// ---------------------------------------------------------------------------------------------
// Device unit functions exposed for the reference's helper-level tests
// ---------------------------------------------------------------------------------------------
// MCR_HELPER_MATH_EXP_FORMS: the path form of exp as the general kernels run it and as the narrow-window growth form runs it
// (fexp<true, true> on a ROTATED table), side by side: out = (general, narrow).  A kernel of its own: the two forms read
// different tables.
__global__ void exp_forms_kernel(const double* in, double* out, int64_t n) {
    __shared__ double tab[kTabDoubles], tab_c[kTabDoubles];
    load_math_tables(tab, threadIdx.x, blockDim.x);
    load_math_tables<true>(tab_c, threadIdx.x, blockDim.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[2 * i] = fexp<true>(in[i], tab, MathRegs::literals_path());
    out[2 * i + 1] = fexp<true, true>(in[i], tab_c, MathRegs::literals_path());
}
__global__ void helper_kernel(int which, const DevParams P, const double* in, double* out, int64_t n) {
    __shared__ double tab[kTabDoubles];
    load_math_tables(tab, threadIdx.x, blockDim.x);
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    switch (which) {
        case MCR_HELPER_WITHDRAW: {
            const double* x = in + 5 * i;
            double bal = x[0], cb = x[1], g, nt;
            const double rate = (x[3] != 0.0 && x[4] > 0.0) ? x[4] : 0.0;  // use_real_tax and rate > 0 (:224)
            withdraw(bal, cb, x[2], rate, g, nt);
            out[4 * i + 0] = bal; out[4 * i + 1] = cb; out[4 * i + 2] = g; out[4 * i + 3] = nt;
            break;
        }
        case MCR_HELPER_NLV: {
            const double* x = in + 4 * i;
            const double rate = (x[2] != 0.0 && x[3] > 0.0) ? x[3] : 0.0;  // :269
            out[i] = net_liquidation_value(x[0], x[1], rate);
            break;
        }
        case MCR_HELPER_REBALANCE: {
            const double* x = in + 4 * i;
            double b1 = x[0], c1 = x[1], b2 = x[2], c2 = x[3];
            rebalance(lane_params(P), b1, c1, b2, c2);
            out[4 * i + 0] = b1; out[4 * i + 1] = c1; out[4 * i + 2] = b2; out[4 * i + 3] = c2;
            break;
        }
        case MCR_HELPER_ANNUAL_TAX: {
            const double* x = in + 6 * i;
            double b1 = x[0], c1 = x[1], b2 = x[2], c2 = x[3];
            const bool tf = annual_gain_taxes(P, lane_params(P), b1, c1, b2, c2, x[4], x[5]);
            out[5 * i + 0] = b1; out[5 * i + 1] = c1; out[5 * i + 2] = b2; out[5 * i + 3] = c2;
            out[5 * i + 4] = tf ? 1.0 : 0.0;
            break;
        }
        case MCR_HELPER_MONTHLY_GROSS: {
            const double* x = in + 3 * i;
            out[i] = monthly_gross(x[0] / (double)kMPY, x[1] / sqrt((double)kMPY), x[2], tab);  // :473
            break;
        }
        case MCR_HELPER_MATH_EXP: out[i] = fexp(in[i], tab, MathRegs::literals()); break;
        case MCR_HELPER_MATH_DIV: out[i] = fdiv(in[2 * i], in[2 * i + 1]); break;
        case MCR_HELPER_MATH_DIV_PATH: out[i] = fdiv<false>(in[2 * i], in[2 * i + 1]); break;
        case MCR_HELPER_MATH_SQRT: out[i] = fsqrt(in[i]); break;
        case MCR_HELPER_WITHDRAW2_PATH: {
            const double* x = in + 6 * i;
            const LaneParams L = lane_params(P);
            double b1 = x[0], c1 = x[1], b2 = x[3], c2 = x[4], g1, n1, g2, n2;
            switch (P.tax_mask) {   // the per-asset forms the path kernel runs for this parameter block
                case 0: withdraw2<false, false>(b1, c1, x[2], L.real_rate1, g1, n1, b2, c2, x[5], L.real_rate2, g2, n2); break;
                case 1: withdraw2<true, false>(b1, c1, x[2], L.real_rate1, g1, n1, b2, c2, x[5], L.real_rate2, g2, n2); break;
                case 2: withdraw2<false, true>(b1, c1, x[2], L.real_rate1, g1, n1, b2, c2, x[5], L.real_rate2, g2, n2); break;
                default: withdraw2<true, true>(b1, c1, x[2], L.real_rate1, g1, n1, b2, c2, x[5], L.real_rate2, g2, n2); break;
            }
            double* o = out + 8 * i;
            o[0] = b1; o[1] = c1; o[2] = g1; o[3] = n1; o[4] = b2; o[5] = c2; o[6] = g2; o[7] = n2;
            break;
        }
        case MCR_HELPER_NLV2_PATH: {
            const double* x = in + 4 * i;
            const LaneParams L = lane_params(P);
            double v1, v2;
            switch (P.tax_mask) {
                case 0: net_liquidation_values2<false, false>(x[0], x[1], L.real_rate1, x[2], x[3], L.real_rate2, v1, v2); break;
                case 1: net_liquidation_values2<true, false>(x[0], x[1], L.real_rate1, x[2], x[3], L.real_rate2, v1, v2); break;
                case 2: net_liquidation_values2<false, true>(x[0], x[1], L.real_rate1, x[2], x[3], L.real_rate2, v1, v2); break;
                default: net_liquidation_values2<true, true>(x[0], x[1], L.real_rate1, x[2], x[3], L.real_rate2, v1, v2); break;
            }
            out[2 * i] = v1; out[2 * i + 1] = v2;
            break;
        }
        case MCR_HELPER_REBALANCE_PATH: {
            const double* x = in + 4 * i;
            double b1 = x[0], c1 = x[1], b2 = x[2], c2 = x[3];
            if (P.any_real_rate) rebalance_path<true>(lane_params(P), b1, c1, b2, c2);
            else rebalance_path<false>(lane_params(P), b1, c1, b2, c2);
            out[4 * i + 0] = b1; out[4 * i + 1] = c1; out[4 * i + 2] = b2; out[4 * i + 3] = c2;
            break;
        }
        case MCR_HELPER_ANNUAL_TAX_PATH: {
            const double* x = in + 6 * i;
            double b1 = x[0], c1 = x[1], b2 = x[2], c2 = x[3];
            const LaneParams L = lane_params(P);
            bool tf;
#define MCR_ATAX(T1_, T2_) (P.any_annual_tax ? annual_gain_taxes<false, (T1_) || (T2_), true, T1_, T2_>(P, L, b1, c1, b2, c2, x[4], x[5]) \
                                             : annual_gain_taxes<false, (T1_) || (T2_), false, T1_, T2_>(P, L, b1, c1, b2, c2, x[4], x[5]))
            switch (P.tax_mask) {
                case 0: tf = MCR_ATAX(false, false); break;
                case 1: tf = MCR_ATAX(true, false); break;
                case 2: tf = MCR_ATAX(false, true); break;
                default: tf = MCR_ATAX(true, true); break;
            }
#undef MCR_ATAX
            out[5 * i + 0] = b1; out[5 * i + 1] = c1; out[5 * i + 2] = b2; out[5 * i + 3] = c2;
            out[5 * i + 4] = tf ? 1.0 : 0.0;
            break;
        }
        case MCR_HELPER_WITHDRAW_MONTH: {   // the month's withdrawal as the path kernel runs it for this parameter block
            const double* x = in + 5 * i;
            double b1 = x[0], c1 = x[1], b2 = x[2], c2 = x[3];
            const double need = x[4];
            double gross, net;
            if (P.exact_month) {            // (:726-790 in the exact path forms, as in path_kernel<..., EXACT = true>)
                const LaneParams L = lane_params(P);
                double cap1, cap2, g1, n1, g2, n2;
                net_liquidation_values2<true, true>(b1, c1, L.real_rate1, b2, c2, L.real_rate2, cap1, cap2);
                const double cap = cap1 + cap2, target = fmin(need, cap);
                double prop1 = fdiv<false>(cap1, cap);
                if (!(cap > kEps)) prop1 = P.alloc1;
                withdraw2<true, true>(b1, c1, target * prop1, L.real_rate1, g1, n1, b2, c2, target * (1.0 - prop1), L.real_rate2, g2, n2);
                gross = g1 + g2; net = n1 + n2;
            } else {                        // the closed form (mcr_device.h: TOLERANCE FORM of the month)
                const LaneParams L = lane_params_tol(P);
                const double cap = P.tax_mask == 3 ? capacity_tol<true, true>(b1, c1, L.real_rate1, b2, c2, L.real_rate2)
                                 : P.tax_mask == 2 ? capacity_tol<false, true>(b1, c1, L.real_rate1, b2, c2, L.real_rate2)
                                 : P.tax_mask == 1 ? capacity_tol<true, false>(b1, c1, L.real_rate1, b2, c2, L.real_rate2)
                                                   : capacity_tol<false, false>(b1, c1, L.real_rate1, b2, c2, L.real_rate2);
                const double target = fmin(need, cap);
                if (cap > kEps) {
                    const double phi = target * recip_nr<false>(cap);
                    gross = phi * ((b1 > kEps ? b1 : 0.0) + (b2 > kEps ? b2 : 0.0)); net = target;   // (:218-219)
                    sell_fraction_tol<true>(phi, b1, c1, b2, c2);
                } else {                    // the dust sub-case: the reference's allocation-weight split in the exact forms
                    double cap1, cap2, g1, n1, g2, n2;
                    net_liquidation_values2<true, true>(b1, c1, L.real_rate1, b2, c2, L.real_rate2, cap1, cap2);
                    const double xcap = cap1 + cap2, xtarget = fmin(need, xcap);
                    const double prop1 = xcap > kEps ? fdiv<false>(cap1, xcap) : P.alloc1;
                    withdraw2<true, true>(b1, c1, xtarget * prop1, L.real_rate1, g1, n1, b2, c2, xtarget * (1.0 - prop1), L.real_rate2, g2, n2);
                    gross = g1 + g2; net = n1 + n2;
                }
            }
            double* o = out + 6 * i;
            o[0] = b1; o[1] = c1; o[2] = b2; o[3] = c2; o[4] = gross; o[5] = net;
            break;
        }
        case MCR_HELPER_REBALANCE_MONTH: {  // the month's rebalance as the path kernel runs it for this parameter block
            const double* x = in + 4 * i;
            double b1 = x[0], c1 = x[1], b2 = x[2], c2 = x[3];
            if (P.exact_month) rebalance_path<true>(lane_params(P), b1, c1, b2, c2);
            else if (P.any_real_rate) rebalance_tol<true>(P, lane_params_tol(P), b1, c1, b2, c2);
            else rebalance_tol<false>(P, lane_params_tol(P), b1, c1, b2, c2);
            out[4 * i + 0] = b1; out[4 * i + 1] = c1; out[4 * i + 2] = b2; out[4 * i + 3] = c2;
            break;
        }
        case MCR_HELPER_MATH_NEG2LOG: out[i] = neg2_log_u32((uint32_t)in[i], tab, MathRegs::literals()); break;
        case MCR_HELPER_MATH_EXP_PATH: out[i] = fexp<true>(in[i], tab, MathRegs::literals_path()); break;
        case MCR_HELPER_MATH_NEG2LOG_PATH: out[i] = neg2_log_u32<true>((uint32_t)in[i], tab, MathRegs::literals_path()); break;
        case MCR_HELPER_MATH_SINCOS_PATH: {
            double sn, cs;
            sincos_u32<true, true>((uint32_t)in[i], tab, MathRegs::literals_path(), sn, cs);
            out[2 * i] = sn; out[2 * i + 1] = cs;
            break;
        }
        case MCR_HELPER_MATH_SINCOS: {
            double sn, cs;
            sincos_u32<true>((uint32_t)in[i], tab, MathRegs::literals(), sn, cs);
            out[2 * i] = sn; out[2 * i + 1] = cs;
            break;
        }
        default: break;
    }
}

// _draw_shock_path (:452-466): out[n_paths][n_months][3]; one thread per path, rows in order
__global__ void shocks_kernel(uint64_t seed, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                              int32_t n_months, double rho, double rho_c, double* out) {
    __shared__ double tab[kTabDoubles];
    load_math_tables(tab, threadIdx.x, blockDim.x);
    __syncthreads();
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_paths) return;
    ShockGen G{0.0, 0u, 0u};
    double* o = out + (size_t)p * 3u * (size_t)n_months;
    for (int32_t m = 0; m < n_months; ++m)
        shock_row_seq(G, seed, stream_id, path_begin + p, (uint32_t)m, rho, rho_c, tab, o[3 * m], o[3 * m + 1], o[3 * m + 2]);
}

// _draw_shock_path with the reference's NumPy stream: one thread per path, rows in order
__global__ void np_shocks_kernel(const KernelIO io, int32_t n_months, double rho, double rho_c, double* out) {
    __shared__ __align__(16) unsigned char zraw[kZigLdsBytes];
    __shared__ double mtab[kTabDoubles];
    load_math_tables(mtab, threadIdx.x, blockDim.x);
    ZigTables zig = load_zig_tables(zraw, threadIdx.x, blockDim.x);
    zig.math_tab = mtab;
    __syncthreads();
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= io.n_paths) return;
    Pcg64 g;
    const uint32_t s32 = io.path_seeds ? io.path_seeds[i]
                                       : np_path_seed(io.entropy, (int)io.n_entropy, io.stream_id, io.child_offset + io.path_begin + i);
    pcg64_seed_u32(g, s32);
    double* o = out + (size_t)i * 3u * (size_t)n_months;
    for (int32_t m = 0; m < n_months; ++m) {
        const double z0 = np_standard_normal(g, zig), z1 = np_standard_normal(g, zig), z2 = np_standard_normal(g, zig);
        o[3 * m + 0] = z0; o[3 * m + 1] = rho * z0 + rho_c * z1; o[3 * m + 2] = z2;
    }
}

// The history stream's rows (include/mcr.h: MCR_RNG_HISTORY): out[n_paths][n_months][3] = Z[row]; one thread per path, rows in
// order through the path kernel's cursor
__global__ void history_shocks_kernel(uint64_t seed, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths, int32_t n_months,
                                      const double* __restrict__ z, uint32_t history_months, uint32_t history_block, uint32_t history_scheme,
                                      double* out) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = p < n_paths;
    const uint64_t q = valid ? p : n_paths - 1;       // (tail lanes shadow the last path: the cursor's branches stay wave-uniform)
    HistoryCursor C = history_cursor();
    double* o = out + (size_t)q * 3u * (size_t)n_months;
    for (int32_t m = 0; m < n_months; ++m) {
        if (history_scheme == MCR_HISTORY_BLOCK) history_seek<false>(C, m, history_months, history_block, history_scheme, seed, stream_id, path_begin + q);
        else history_seek<true>(C, m, history_months, history_block, history_scheme, seed, stream_id, path_begin + q);
        if (valid) { o[3 * m + 0] = z[3u * C.cur + 0]; o[3 * m + 1] = z[3u * C.cur + 1]; o[3 * m + 2] = z[3u * C.cur + 2]; }
    }
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int hip_fail(hipError_t e, const char* what) {
    set_error("%s: %s", what, hipGetErrorString(e));
    return MCR_ERR_HIP;
}

int use_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        set_error("no usable HIP device (the engine has no CPU fallback)");
        return MCR_ERR_NO_DEVICE;
    }
    if (device < 0 || device >= n) {
        set_error("device %d out of range (%d devices)", device, n);
        return MCR_ERR_INVALID_ARG;
    }
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    return MCR_OK;
}

// ---- leased per-device resources (mcr_host.h: HostCtx, StreamFork): one process-wide idle pool per kind, keyed by device ----
// acquire() hands out the most recently used idle entry of the device, or makes one (Create: nullptr on failure); release()
// puts it back and, above kIdlePerDevice idle entries of that device, destroys the least recently used one — outside the
// lock, on the device of the call that is ending (it is still current: Destroy expects the device set).
template <class T, int kIdlePerDevice, T* (*Create)(int), void (*Destroy)(T*)>
class IdlePool {
public:
    T* acquire(int device) {
        {
            std::lock_guard<std::mutex> lock(mu_);
            for (size_t i = idle_.size(); i-- > 0;)
                if (idle_[i]->device == device) return take(i);
        }
        return Create(device);
    }
    void release(T* t) {
        T* surplus = nullptr;
        {
            std::lock_guard<std::mutex> lock(mu_);
            idle_.push_back(t);
            int same = 0;
            for (T* o : idle_) same += o->device == t->device;
            for (size_t i = 0; same > kIdlePerDevice && !surplus; ++i)
                if (idle_[i]->device == t->device) surplus = take(i);
        }
        if (surplus) Destroy(surplus);
    }
    // mcr_release_cached: destroys the idle entries of `device` (< 0: of every device), each on its own device
    int release_cached(int device) {
        std::vector<T*> gone;
        {
            std::lock_guard<std::mutex> lock(mu_);
            for (size_t i = idle_.size(); i-- > 0;)
                if (device < 0 || idle_[i]->device == device) gone.push_back(take(i));
        }
        int rc = MCR_OK;
        for (T* t : gone) {
            DeviceScope scope(t->device);
            if (scope.rc != MCR_OK) rc = scope.rc;   // (device gone: drop the bookkeeping anyway)
            Destroy(t);
        }
        return rc;
    }
    // An entry for the duration of a scope; p == nullptr: Create failed
    struct Lease {
        IdlePool& pool;
        T* const p;
        Lease(IdlePool& pool_, int device) : pool(pool_), p(pool_.acquire(device)) {}
        Lease(const Lease&) = delete;
        Lease& operator=(const Lease&) = delete;
        ~Lease() { if (p) pool.release(p); }
    };

private:
    T* take(size_t i) {   // (under the lock)
        T* t = idle_[i];
        idle_.erase(idle_.begin() + (long)i);
        return t;
    }
    std::mutex mu_;
    std::vector<T*> idle_;   // most recently used last
};

static HostCtx* host_ctx_create(int device) {   // (error set on failure)
    HostCtx* c = new HostCtx{device, nullptr, nullptr, 0};
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { (void)hip_fail(e, "hipStreamCreate (host context)"); delete c; return nullptr; }
    return c;
}
static void host_ctx_destroy(HostCtx* c) {
    if (c->block) (void)hipFree(c->block);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;
}
using HostCtxPool = IdlePool<HostCtx, kHostCtxIdlePerDevice, host_ctx_create, host_ctx_destroy>;
static HostCtxPool g_host_ctx;

// Fork/join streams (mcr_host.h: StreamFork): a few non-blocking side streams + events, leased for the duration of ONE
// call's enqueue.  A lease only has to cover the host-side enqueue: the side streams are in-order, and a stream that waits
// on an event waits for the record that preceded the wait call, so the next lessee's records cannot disturb work that is
// still running.  User: mcr_probe_months_rng (candidates forked onto side streams; mcr_row_quantiles' row-group pipelining
// was measured and dropped in round 3).
static void stream_fork_destroy(StreamFork* f) {   // pending work on a destroyed stream still completes (stream-ordered release)
    for (int i = 0; i < kForkStreams; ++i) {
        if (f->done[i]) (void)hipEventDestroy(f->done[i]);
        if (f->side[i]) (void)hipStreamDestroy(f->side[i]);
    }
    if (f->fork) (void)hipEventDestroy(f->fork);
    delete f;
}
static StreamFork* stream_fork_create(int device) {   // nullptr: out of resources
    StreamFork* f = new StreamFork();
    std::memset(f, 0, sizeof(*f));
    f->device = device;
    bool ok = hipEventCreateWithFlags(&f->fork, hipEventDisableTiming) == hipSuccess;
    for (int i = 0; ok && i < kForkStreams; ++i)
        ok = hipStreamCreateWithFlags(&f->side[i], hipStreamNonBlocking) == hipSuccess &&
             hipEventCreateWithFlags(&f->done[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); stream_fork_destroy(f); return nullptr; }
    return f;
}
using StreamForkPool = IdlePool<StreamFork, kStreamForkIdlePerDevice, stream_fork_create, stream_fork_destroy>;
static StreamForkPool g_stream_fork;

// Preconditions of the path kernel (its STRICT = false forms drop clamps that are no-ops only for rates and
// weights in [0, 1] and non-negative amounts; fexp needs |x| < 700).  The reference enforces the same ranges
// in its pydantic Config (backend/config.py:56-99); a ctypes caller that bypasses Config gets an error here,
// not silently different arithmetic.
// other_income_streams has any length (backend/config.py:99): the first MCR_INLINE_STREAMS records sit in the block, the
// rest behind mcr_params.extra_streams (a host pointer)
static inline const mcr_stream& stream_at(const mcr_params* p, int s) {
    return s < MCR_INLINE_STREAMS ? p->streams[s] : p->extra_streams[s - MCR_INLINE_STREAMS];
}
static int check_stream_list(const mcr_params* p) {
    if (p->n_streams < 0) { set_error("n_streams %d must be >= 0", p->n_streams); return MCR_ERR_INVALID_ARG; }
    if (p->n_streams > MCR_INLINE_STREAMS && !p->extra_streams) {
        set_error("n_streams = %d but extra_streams is NULL (entries %d.. of the list go there)", p->n_streams, MCR_INLINE_STREAMS);
        return MCR_ERR_INVALID_ARG;
    }
    return MCR_OK;
}

// monthly log-growth a + b z with |z| < 40 (Box-Muller of 32-bit uniforms: |z| < 6.8, rho-mix < 9.6; ziggurat tail far
// below 40) must stay inside fexp's domain: the rule validate_params and the assumption probe's records share
static bool log_growth_in_domain(double mu, double sg) {
    return std::isfinite(mu) && std::isfinite(sg) && sg >= 0.0 && std::fabs(mu) / kMPY + 40.0 * sg / std::sqrt((double)kMPY) < 700.0;
}

static int validate_params(const mcr_params* p) {
    if (!p) { set_error("null params"); return MCR_ERR_INVALID_ARG; }
    auto bad = [](const char* name, double v, const char* want) {
        set_error("params.%s = %g: must be %s", name, v, want);
        return MCR_ERR_INVALID_ARG;
    };
    auto unit = [](double v) { return v >= 0.0 && v <= 1.0; };            // false for NaN
    auto nonneg = [](double v) { return v >= 0.0 && std::isfinite(v); };
    if (!nonneg(p->initial_balance)) return bad("initial_balance", p->initial_balance, "finite and >= 0 (config.py:56)");
    if (!nonneg(p->monthly_contribution)) return bad("monthly_contribution", p->monthly_contribution, "finite and >= 0 (config.py:57)");
    if (!nonneg(p->contribution_growth_rate_annual)) return bad("contribution_growth_rate_annual", p->contribution_growth_rate_annual, "finite and >= 0 (config.py:58)");
    if (!nonneg(p->monthly_expenses)) return bad("monthly_expenses", p->monthly_expenses, "finite and >= 0 (config.py:59)");
    if (!std::isfinite(p->current_age)) return bad("current_age", p->current_age, "finite (config.py:62)");
    if (!unit(p->allocation_inv1_pct)) return bad("allocation_inv1_pct", p->allocation_inv1_pct, "in [0, 1] (config.py:70)");
    if (!unit(p->inv1_annual_tax_on_gains_rate)) return bad("inv1_annual_tax_on_gains_rate", p->inv1_annual_tax_on_gains_rate, "in [0, 1] (config.py:73)");
    if (!unit(p->inv1_realized_gains_tax_rate)) return bad("inv1_realized_gains_tax_rate", p->inv1_realized_gains_tax_rate, "in [0, 1] (config.py:74)");
    if (!unit(p->inv2_annual_tax_on_gains_rate)) return bad("inv2_annual_tax_on_gains_rate", p->inv2_annual_tax_on_gains_rate, "in [0, 1] (config.py:79)");
    if (!unit(p->inv2_realized_gains_tax_rate)) return bad("inv2_realized_gains_tax_rate", p->inv2_realized_gains_tax_rate, "in [0, 1] (config.py:80)");
    if (!(p->equity_inflation_rho >= -1.0 && p->equity_inflation_rho <= 1.0)) return bad("equity_inflation_rho", p->equity_inflation_rho, "in [-1, 1] (config.py:85)");
    const double mu[3] = {p->inv1_mu_log, p->inf_mu_log, p->prem_mu_log}, sg[3] = {p->inv1_sigma_log, p->inf_sigma_log, p->prem_sigma_log};
    const char* nm[3] = {"inv1", "inf", "prem"};
    for (int i = 0; i < 3; ++i) {
        if (!log_growth_in_domain(mu[i], sg[i])) {
            set_error("params.%s_mu_log / %s_sigma_log = %g / %g: need finite values, sigma >= 0 and |mu|/12 + 40 sigma/sqrt(12) < 700",
                      nm[i], nm[i], mu[i], sg[i]);
            return MCR_ERR_INVALID_ARG;
        }
    }
    if (int rc = check_stream_list(p)) return rc;
    for (int s = 0; s < p->n_streams; ++s) {
        const mcr_stream& st = stream_at(p, s);
        if (!nonneg(st.monthly_amount_today) || !unit(st.tax_rate) || !std::isfinite(st.start_at_age)) {
            set_error("params.streams[%d]: monthly_amount_today %g must be finite and >= 0, tax_rate %g in [0, 1], start_at_age %g finite "
                      "(config.py:18,23,45)", s, st.monthly_amount_today, st.tax_rate, st.start_at_age);
            return MCR_ERR_INVALID_ARG;
        }
    }
    return MCR_OK;
}

static int query_sizes(const mcr_params* p, int32_t wm, mcr_sizes* s) {
    if (!p || !s) { set_error("null argument"); return MCR_ERR_INVALID_ARG; }
    if (wm < 0) { set_error("working_months must be >= 0 (got %d)", wm); return MCR_ERR_INVALID_ARG; }
    if (p->retirement_years <= 0) { set_error("retirement_years must be > 0"); return MCR_ERR_INVALID_ARG; }
    if (int rc = check_stream_list(p)) return rc;
    if ((int64_t)wm + (int64_t)p->retirement_years * kMPY > (int64_t)INT32_MAX / 4) {
        set_error("horizon too long");
        return MCR_ERR_INVALID_ARG;
    }
    s->total_months = wm + p->retirement_years * kMPY;                   // simulation.py:487
    s->shock_rows = s->total_months > 1 ? s->total_months : 1;           // :488
    s->num_working_years = wm > 0 ? (wm + kMPY - 1) / kMPY : 0;          // :585-589
    s->trajectory_len = 1 + s->num_working_years + p->retirement_years;  // :902
    s->retirement_years = p->retirement_years;
    s->ruin_bins = p->retirement_years + 2;
    return MCR_OK;
}

// stream_payment_start_month_index (simulation.py:47-63)
static int32_t start_month_index(double current_age, int32_t wm, double start_at_age) {
    const double retirement_start = current_age + (double)wm / (double)kMPY;  // :34
    const double eligible = start_at_age > retirement_start ? start_at_age : retirement_start;  // max(ret, start) :44
    const double c = std::ceil((eligible - retirement_start) * (double)kMPY - kEps);            // :58-61
    if (!(c > 0.0)) return 0;
    if (c > (double)(INT32_MAX / 2)) return INT32_MAX / 2;
    return (int32_t)c;
}

// The market's part of the parameter block, from the seven lognormal parameters alone: derive_params fills DevParams with it,
// the assumption probe its records (AssumptionRecord).  ONE function, not inlined, so that a record holds the bits a parameter
// block with the same seven fields holds.
struct DevMarket { double a1, b1, ainf, binf, aprem, bprem, rho, rho_c, binf_rho, binf_rho_c; };
__attribute__((noinline)) static DevMarket derive_market(double inv1_mu_log, double inv1_sigma_log, double inf_mu_log, double inf_sigma_log,
                                                         double prem_mu_log, double prem_sigma_log, double rho) {
    DevMarket m;
    const double sqrt12 = std::sqrt((double)kMPY);
    m.a1 = inv1_mu_log / (double)kMPY;   m.b1 = inv1_sigma_log / sqrt12;     // :473
    m.ainf = inf_mu_log / (double)kMPY;  m.binf = inf_sigma_log / sqrt12;
    m.aprem = prem_mu_log / (double)kMPY; m.bprem = prem_sigma_log / sqrt12;
    m.rho = rho;
    const double om = 1.0 - m.rho * m.rho;
    m.rho_c = std::sqrt(om > 0.0 ? om : 0.0);  // :463
    m.binf_rho = m.binf * m.rho;
    m.binf_rho_c = m.binf * m.rho_c;
    return m;
}

// One income stream's amount and window: derive_params fills a DevStream with it, the income probe its records (IncomeRecord).
// ONE function, not inlined, so that a record holds the bits a parameter block with the same stream holds.
struct DevStreamWindow { double amount, keep, amount_keep; int32_t start_month, end_month; };
__attribute__((noinline)) static DevStreamWindow derive_stream(double current_age, int32_t wm, double monthly_amount_today, double tax_rate,
                                                               double start_at_age, int32_t duration_years) {
    DevStreamWindow o;
    o.amount = monthly_amount_today;
    o.keep = 1.0 - tax_rate;  // :676
    o.amount_keep = o.amount * o.keep;
    o.start_month = start_month_index(current_age, wm, start_at_age);  // :603-608
    if (duration_years < 0) {
        o.end_month = INT32_MAX;  // None: forever (:654)
    } else {
        const int64_t e = (int64_t)o.start_month + (int64_t)duration_years * kMPY;  // :609-613,:655
        o.end_month = e > INT32_MAX ? INT32_MAX : (int32_t)e;
    }
    return o;
}

// Host-side derivation of the wave-uniform parameter block (same fp64 expressions as the reference).
// `extra` receives the records of the streams beyond the by-value block (device-table layout); callers that cannot carry
// such a table pass nullptr and get MCR_ERR_UNSUPPORTED for longer lists.
static int derive_params(const mcr_params* p, int32_t wm, DevParams* d, std::vector<DevStream>* extra = nullptr,
                         std::vector<std::pair<int, int>>* kept = nullptr /* (list index, lock slot) of the records the kernel gets */,
                         int keep_index = -1 /* a list index whose record the kernel gets even if it pays nothing (the income probe's) */) {
    mcr_sizes sz;
    int rc = query_sizes(p, wm, &sz);
    if (rc != MCR_OK) return rc;
    rc = validate_params(p);
    if (rc != MCR_OK) return rc;
    std::memset(d, 0, sizeof(*d));
    d->initial_balance = p->initial_balance;
    d->monthly_contribution = p->monthly_contribution;
    d->contrib_growth_factor = 1 + p->contribution_growth_rate_annual;  // :517
    d->contrib_grows = p->contribution_growth_rate_annual > 0;          // :516
    d->monthly_expenses = p->monthly_expenses;
    d->alloc1 = p->allocation_inv1_pct;
    d->alloc2 = 1.0 - p->allocation_inv1_pct;  // config.py:124-126
    // "use_real_tax and rate > 0" (:224,:238,:269) and "if use_realized" (:304,:317): a zero rate
    // multiplies to exactly 0.0, so one effective rate covers both spellings.
    d->real_rate1 = (p->inv1_use_realized_gains_tax_system && p->inv1_realized_gains_tax_rate > 0) ? p->inv1_realized_gains_tax_rate : 0.0;
    d->real_rate2 = (p->inv2_use_realized_gains_tax_system && p->inv2_realized_gains_tax_rate > 0) ? p->inv2_realized_gains_tax_rate : 0.0;
    d->annual_rate1 = !p->inv1_use_realized_gains_tax_system ? p->inv1_annual_tax_on_gains_rate : 0.0;  // :380-384
    d->annual_rate2 = !p->inv2_use_realized_gains_tax_system ? p->inv2_annual_tax_on_gains_rate : 0.0;  // :385-389
    d->any_annual_tax = (d->annual_rate1 > 0.0) || (d->annual_rate2 > 0.0);
    d->any_real_rate = (d->real_rate1 > 0.0) || (d->real_rate2 > 0.0);
    d->tax_mask = (d->real_rate1 > 0.0 ? 1 : 0) | (d->real_rate2 > 0.0 ? 2 : 0);
    // the tolerance form of the month is the reference's arithmetic while its denominator clamps (max(1e-6, 1 - gf r), :227,
    // :307-310) cannot bind: both effective rates <= 1 - 1e-6 (mcr_device.h).  Otherwise: exact forms, generic variants.
    d->exact_month = (d->real_rate1 > 1.0 - kEps || d->real_rate2 > 1.0 - kEps) ? 1 : 0;
    // the straight-line month's ballot (path kernel): both balances above this floor -> capacity >= (b1 + b2)(1 - r_max) > 2e-6,
    // outside the dust sub-case.  1e-6 itself without a realized-gains rate.
    d->fast_floor = d->exact_month ? kEps : kEps / (1.0 - std::fmax(d->real_rate1, d->real_rate2));
    const DevMarket mk = derive_market(p->inv1_mu_log, p->inv1_sigma_log, p->inf_mu_log, p->inf_sigma_log, p->prem_mu_log, p->prem_sigma_log,
                                       p->equity_inflation_rho);
    d->a1 = mk.a1; d->b1 = mk.b1; d->ainf = mk.ainf; d->binf = mk.binf; d->aprem = mk.aprem; d->bprem = mk.bprem;
    d->rho = mk.rho; d->rho_c = mk.rho_c; d->binf_rho = mk.binf_rho; d->binf_rho_c = mk.binf_rho_c;
    d->working_months = wm;
    d->retirement_years = p->retirement_years;
    d->total_months = sz.total_months;
    d->shock_rows = sz.shock_rows;
    d->num_working_years = sz.num_working_years;
    d->trajectory_len = sz.trajectory_len;
    // A record that pays nothing (monthly_amount_today == 0) contributes an exact zero to every month's income, frozen or
    // indexed: income - 0 and fma(-0, price, income) are `income` (the price level is finite), and the exact form adds 0 keep
    // = +0 to a non-negative sum.  The kernel is not given it: no record to test every month, no lock column, no field in a
    // time-sliced block's hand-over.  The kept records keep their list order; lock slots are numbered over them.  (keep_index:
    // the income probe's stream is kept whatever it pays, with its lock slot if it is frozen — its consumer waves pay their own.)
    int kept_n = 0;
    for (int s = 0; s < p->n_streams; ++s) kept_n += stream_at(p, s).monthly_amount_today != 0.0 || s == keep_index;
    d->n_streams = kept_n < MCR_INLINE_STREAMS ? kept_n : MCR_INLINE_STREAMS;
    d->n_extra_streams = kept_n - d->n_streams;
    if (extra) extra->assign((size_t)d->n_extra_streams, DevStream{});
    if (kept) kept->clear();
    int slots = 0, k = 0;
    for (int s = 0; s < p->n_streams; ++s) {
        const mcr_stream& in = stream_at(p, s);
        if (in.monthly_amount_today == 0.0 && s != keep_index) continue;
        DevStream scratch;
        DevStream& o = k < MCR_INLINE_STREAMS ? d->streams[k] : (extra ? (*extra)[(size_t)(k - MCR_INLINE_STREAMS)] : scratch);
        ++k;
        const DevStreamWindow w = derive_stream(p->current_age, wm, in.monthly_amount_today, in.tax_rate, in.start_at_age, in.duration_years);
        o.amount = w.amount; o.keep = w.keep; o.amount_keep = w.amount_keep; o.start_month = w.start_month; o.end_month = w.end_month;
        o.indexed = in.inflation_indexed ? 1 : 0;
        o.lock_slot = o.indexed ? -1 : slots++;
        if (kept) kept->push_back({s, o.lock_slot});
    }
    d->n_lock_slots_total = slots;
    d->n_lock_slots = slots;     // (the launcher lowers it to what its kernel variant's LDS budget holds: plan_lock_slots)
    return MCR_OK;
}

// The GROWTH FORM of a launch (mcr_device.h: kGrowthNarrowExp | kGrowthRhoZero), from its parameter block alone.
// Narrow exp window: every argument of the month's three exps is x = a + b z, and |z| is bounded by the generator itself — a
// normal is radius x (cos | sin), the radius sqrt(-2 ln u) with u = (w + 0.5) 2^-32 >= 2^-33: kGrowthZMax.  So
//     xmax = |a| + c |b| kGrowthZMax,    c = 1 (equity, premium),  c = |rho| + |rho_c| (inflation: rho n0 + rho_c n1),
// and the form holds when xmax 512 / ln 2 <= kExpNarrowMaxK - 1 for all three series: k = rint(x 512 / ln 2) then lies in
// fexp's window [-256, 255].  The 1 of margin covers rint's half step and the roundings of a + b z and of the kernel's radius
// and sine / cosine (1e-14 relative: 1e-11 of a step).
// rho = 0: binf_rho = binf * rho is then an exact zero (of either sign).
static const double kGrowthZMax = std::sqrt(66.0 * std::log(2.0));   // sqrt(-2 ln 2^-33) = 6.7637
static int growth_form_qualified(const DevParams& d) {
    const double k_per_x = 512.0 / std::log(2.0), kmax = (double)(kExpNarrowMaxK - 1);
    const double c_inf = std::fabs(d.rho) + std::fabs(d.rho_c);
    const double x_eq = std::fabs(d.a1) + std::fabs(d.b1) * kGrowthZMax;
    const double x_inf = std::fabs(d.ainf) + c_inf * std::fabs(d.binf) * kGrowthZMax;
    const double x_prem = std::fabs(d.aprem) + std::fabs(d.bprem) * kGrowthZMax;
    const bool narrow = x_eq * k_per_x <= kmax && x_inf * k_per_x <= kmax && x_prem * k_per_x <= kmax;
    if (!narrow) return 0;
    return d.rho == 0.0 ? (kGrowthNarrowExp | kGrowthRhoZero) : kGrowthNarrowExp;
}
// ... and what the launch runs: MCR_K1_GROWTH_FORM=0|1|3 (A/B, tests; read at every launch) forces a LOWER mask.  A bit the
// parameters do not qualify for, or a non-zero mask on a launch whose kernel has no growth variants (`has_variants` false:
// anything but a whole-path or time-sliced count-only Philox launch without an annual-gains tax), is an error: the knob never
// yields a wrong table, and a test never compares a kernel with itself.
static int growth_form_of(const DevParams& d, bool has_variants, int* mask) {
    const int q = growth_form_qualified(d);
    *mask = has_variants ? q : 0;
    const char* e = std::getenv("MCR_K1_GROWTH_FORM");
    if (!e || !*e) return MCR_OK;
    char* end = nullptr;
    const long want = std::strtol(e, &end, 10);
    if (*end != '\0' || (want != 0 && want != kGrowthNarrowExp && want != (kGrowthNarrowExp | kGrowthRhoZero))) {
        set_error("MCR_K1_GROWTH_FORM=%s: the growth forms are 0, 1 and 3", e);
        return MCR_ERR_INVALID_ARG;
    }
    if (want != 0 && !has_variants) {
        set_error("MCR_K1_GROWTH_FORM=%s set on a launch whose kernel has no growth variants", e);
        return MCR_ERR_INVALID_ARG;
    }
    if (((int)want & ~q) != 0) {
        set_error("MCR_K1_GROWTH_FORM=%s: the parameters qualify for mask %d only (narrow exp window: |a| + c |b| %.4f <= %d ln 2 / 512; rho = 0)",
                  e, q, kGrowthZMax, kExpNarrowMaxK - 1);
        return MCR_ERR_INVALID_ARG;
    }
    *mask = (int)want;
    return MCR_OK;
}

// The MONTH FORM of a launch (mcr_device.h: kMonthEqualRates), from its parameter block alone: both assets taxed on realized
// gains (tax mask 3) at the same rate, in the tolerance form of the month, with no annual-gains tax (the kernels that have the
// variants).  MCR_K1_MONTH_FORM=0|1 forces a LOWER mask, under the rules of MCR_K1_GROWTH_FORM: a bit the parameters do not
// qualify for, or a non-zero mask on a launch whose kernel has no variants, is an error.  A library built with
// -DMCR_K1_EXACT_MONTH runs every kernel in the exact month, which has no month forms: no launch qualifies there.
static int month_form_qualified(const DevParams& d) {
    if (kExactMonthDefault) return 0;
    return (d.tax_mask == 3 && d.real_rate1 == d.real_rate2 && !d.any_annual_tax && !d.exact_month) ? kMonthEqualRates : 0;
}
static int month_form_of(const DevParams& d, bool has_variants, int* mask) {
    const int q = month_form_qualified(d);
    *mask = has_variants ? q : 0;
    const char* e = std::getenv("MCR_K1_MONTH_FORM");
    if (!e || !*e) return MCR_OK;
    char* end = nullptr;
    const long want = std::strtol(e, &end, 10);
    if (*end != '\0' || (want != 0 && want != kMonthEqualRates)) {
        set_error("MCR_K1_MONTH_FORM=%s: the month forms are 0 and 1", e);
        return MCR_ERR_INVALID_ARG;
    }
    if (want != 0 && !has_variants) {
        set_error("MCR_K1_MONTH_FORM=%s set on a launch whose kernel has no month variants", e);
        return MCR_ERR_INVALID_ARG;
    }
    if (((int)want & ~q) != 0) {
        set_error("MCR_K1_MONTH_FORM=%s: the parameters qualify for mask %d only (both assets taxed on realized gains at one rate, no annual-gains tax)", e, q);
        return MCR_ERR_INVALID_ARG;
    }
    *mask = (int)want;
    return MCR_OK;
}

// The STREAM FORM of a launch (mcr_device.h: kStreamsInRegs), from its parameter block alone: the records handed to the
// kernel (derive_params has dropped the ones that pay nothing) are at most two, none sits in the extra table, and every one
// is inflation-indexed — in the tolerance form of the month, with no annual-gains tax (the kernels that have the variants).
// An empty list qualifies.  MCR_K1_STREAM_FORM=0|1 forces a LOWER mask, under the rules of MCR_K1_MONTH_FORM.  A library built
// with -DMCR_K1_EXACT_MONTH has no stream forms: no launch qualifies there.
static int stream_form_qualified(const DevParams& d) {
    if (kExactMonthDefault) return 0;
    if (d.any_annual_tax || d.exact_month || d.n_extra_streams > 0 || d.n_streams > 2) return 0;
    for (int s = 0; s < d.n_streams; ++s) if (!d.streams[s].indexed) return 0;
    return kStreamsInRegs;
}
static int stream_form_of(const DevParams& d, bool has_variants, int* mask) {
    const int q = stream_form_qualified(d);
    *mask = has_variants ? q : 0;
    const char* e = std::getenv("MCR_K1_STREAM_FORM");
    if (!e || !*e) return MCR_OK;
    char* end = nullptr;
    const long want = std::strtol(e, &end, 10);
    if (*end != '\0' || (want != 0 && want != kStreamsInRegs)) {
        set_error("MCR_K1_STREAM_FORM=%s: the stream forms are 0 and 1", e);
        return MCR_ERR_INVALID_ARG;
    }
    if (want != 0 && !has_variants) {
        set_error("MCR_K1_STREAM_FORM=%s set on a launch whose kernel has no stream variants", e);
        return MCR_ERR_INVALID_ARG;
    }
    if (((int)want & ~q) != 0) {
        set_error("MCR_K1_STREAM_FORM=%s: the parameters qualify for mask %d only (at most two paying income streams, all inflation-indexed, no annual-gains tax)", e, q);
        return MCR_ERR_INVALID_ARG;
    }
    *mask = (int)want;
    return MCR_OK;
}

// LDS of one path_kernel launch.  STATIC part of the variant — it mirrors the __shared__ declarations at the top of the
// kernel: the math tables, the stage of growth factors (Philox stream without injection; twice for the producer / consumer
// form) and the three per-path summary columns (those variants with per-path outputs) — plus the launch's DYNAMIC part: the
// ziggurat tables (NumPy stream), the block counters / year bins / histogram bins, and as many [kBlock] lock columns of
// non-indexed income streams as keep FOUR workgroups resident on a CU (160 KB of LDS: 40 KB each), never more than the 64 KB
// a workgroup may use without opting in; the remaining slots go to a global overflow block (DevParams::lock_overflow).
// Measured at 10^6 config.json paths (tools/streams_timing.py, profiles/r04): 16 frozen streams with every column in LDS
// (2 resident workgroups) 18.4 ms count-only, all in the overflow block 12.5 ms; 8 frozen streams (4 resident workgroups
// with all columns in LDS) 8.7 vs 8.9 ms.  MCR_K1_LDS_LOCK_SLOTS=n in the environment overrides the occupancy rule: up to n
// slots in LDS (A/B, tests).
constexpr size_t kLdsPerWorkgroup = 64 * 1024;
constexpr size_t kLdsForFourResident = 40 * 1024;
static size_t path_kernel_static_lds(int mode, uint32_t rng_kind, bool injected, bool split) {
    const bool staged = rng_kind == MCR_RNG_PHILOX && !injected;
    const bool history = rng_kind == MCR_RNG_HISTORY && !injected;     // (its math tables lie in the dynamic part, under its factor table)
    return (history ? (size_t)16 : (size_t)kMathTabBytes) + (staged ? (size_t)(split ? 2 : 1) * kStageDoubles * sizeof(double) : 16) +
           (((mode == 1 || mode == 2) && staged) ? (size_t)3 * kBlock * sizeof(double) : 16);
}
// LDS of the yearly-bins form (MODE 3 of path_kernel) behind the block counters: both edge arrays as doubles, two row buffers
// [trajectory | real | wr] and the final_success cells as 32-bit counts — 8 + 5 x 4 = 28 bytes per balance bin, 8 + 2 x 4 = 16
// per withdrawal-rate bin (+ 8 of alignment)
static size_t year_bins_lds(int n_bins, int n_wr_bins) {
    const size_t cells = (size_t)n_bins + 2, wcells = (size_t)n_wr_bins + 2;
    return 8 + ((size_t)n_bins + 1 + (size_t)n_wr_bins + 1) * sizeof(double) + (2 * (2 * cells + wcells) + cells) * sizeof(unsigned int);
}
// The history stream (rng_kind MCR_RNG_HISTORY, not injected) holds its factor table, history_months x 3 doubles, in the
// dynamic part — where the math tables stand until the table is made, so the part is never smaller than they are — and has
// no stage.  A long record alone costs resident workgroups (2048 months: 48 KB = three on a CU); its lock columns then get
// what is left of the budget of THAT number of workgroups, not of four.
constexpr size_t kLdsPerCu = 160 * 1024;
static int plan_path_kernel_lds(DevParams& d, int mode, uint32_t rng_kind, bool injected, bool split, int n_hist_bins, size_t* dynamic_bytes,
                                size_t year_bins_bytes = 0, uint32_t history_months = 0,
                                bool whole_workgroup = false /* a launch with no generic form behind it: lock columns up to the workgroup's own LDS, at the price of resident workgroups */) {
    const size_t table_bytes = injected ? (size_t)0 : rng_kind == MCR_RNG_NUMPY ? (size_t)kZigLdsBytes
                               : rng_kind == MCR_RNG_HISTORY ? (size_t)history_months * 3u * sizeof(double) : (size_t)0;
    size_t fixed = path_kernel_static_lds(mode, rng_kind, injected, split) + table_bytes +
                         (size_t)(1 + (d.retirement_years + 2) + (d.retirement_years + 1) + n_hist_bins) * sizeof(unsigned int) + year_bins_bytes;
    if (rng_kind == MCR_RNG_HISTORY && !injected) fixed = std::max(fixed, path_kernel_static_lds(mode, rng_kind, injected, split) + (size_t)kMathTabBytes);
    if (fixed > kLdsPerWorkgroup) { set_error("too many retirement years / histogram bins for the LDS of a workgroup"); return MCR_ERR_UNSUPPORTED; }
    constexpr size_t kSlotBytes = (size_t)kBlock * sizeof(double);
    long slots = (long)((kLdsPerWorkgroup - fixed) / kSlotBytes);
    size_t budget = whole_workgroup ? kLdsPerWorkgroup : kLdsForFourResident;
    if (rng_kind == MCR_RNG_HISTORY && !injected && fixed >= kLdsForFourResident) budget = std::min(kLdsPerWorkgroup, kLdsPerCu / (kLdsPerCu / fixed));
    const char* e = std::getenv("MCR_K1_LDS_LOCK_SLOTS");
    if (e && *e) slots = std::min(slots, std::max(0l, std::strtol(e, nullptr, 10)));
    else slots = std::min(slots, fixed < budget ? (long)((budget - fixed) / kSlotBytes) : 0l);
    d.n_lock_slots = (int32_t)std::min<long>(slots, d.n_lock_slots_total);
    *dynamic_bytes = fixed - path_kernel_static_lds(mode, rng_kind, injected, split) + (size_t)d.n_lock_slots * kBlock * sizeof(double);
    return MCR_OK;
}

// Scope guard of one stream-ordered allocation: freed behind the work enqueued so far, by release() or at scope exit
struct StreamAlloc {
    void* p = nullptr;
    hipStream_t stream;
    explicit StreamAlloc(hipStream_t s) : stream(s) {}
    StreamAlloc(const StreamAlloc&) = delete;
    StreamAlloc& operator=(const StreamAlloc&) = delete;
    ~StreamAlloc() { (void)release(); }
    hipError_t alloc_status(size_t bytes) {     // refused: nothing enqueued, the HIP error cleared
        const hipError_t e = hipMallocAsync(&p, bytes, stream);
        if (e != hipSuccess) { (void)hipGetLastError(); p = nullptr; }
        return e;
    }
    bool alloc(size_t bytes) { return alloc_status(bytes) == hipSuccess; }
    hipError_t release() {
        if (!p) return hipSuccess;
        const hipError_t e = hipFreeAsync(p, stream);
        p = nullptr;
        return e;
    }
};
// The device side of a launch's stream list: the table of the records beyond the by-value block and the overflow block of
// lock slots, ONE stream-ordered allocation (freed behind the kernel).  The host copy of the table is owned by the stream
// until the upload has run (hipLaunchHostFunc): nothing here waits for the device.
struct StreamSideBlock {
    StreamAlloc mem;
    explicit StreamSideBlock(hipStream_t s) : mem(s) {}
    int attach(DevParams& d, const std::vector<DevStream>& extra, unsigned grid_x) {
        const int n_over = d.n_lock_slots_total - d.n_lock_slots;
        if (extra.empty() && n_over <= 0) return MCR_OK;
        d.lock_stride = (int64_t)grid_x * kBlock;
        const size_t table_bytes = (extra.size() * sizeof(DevStream) + 255) & ~(size_t)255;
        const size_t over_bytes = (size_t)(n_over > 0 ? n_over : 0) * (size_t)d.lock_stride * sizeof(double);
        hipError_t e = mem.alloc_status(table_bytes + over_bytes);
        if (e != hipSuccess) return hip_fail(e, "income-stream table / lock-slot overflow allocation");
        if (!extra.empty()) {
            void* host = std::malloc(extra.size() * sizeof(DevStream));
            if (!host) { set_error("out of host memory"); return MCR_ERR_HIP; }
            std::memcpy(host, extra.data(), extra.size() * sizeof(DevStream));
            e = hipMemcpyAsync(mem.p, host, extra.size() * sizeof(DevStream), hipMemcpyHostToDevice, mem.stream);
            const hipError_t ef = hipLaunchHostFunc(mem.stream, [](void* h) { std::free(h); }, host);
            if (ef != hipSuccess) { (void)hipStreamSynchronize(mem.stream); std::free(host); }
            if (e != hipSuccess) return hip_fail(e, "income-stream table upload");
            d.extra_streams = (const DevStream*)mem.p;
        }
        if (n_over > 0) d.lock_overflow = (double*)((char*)mem.p + table_bytes);
        return MCR_OK;
    }
    hipError_t release() { return mem.release(); }
};

// Launches of at most this many path-wavefronts take the producer / consumer split (SPLIT = true): up to 3 per SIMD a
// wavefront is latency-bound and the second wave per path hides half of its chain; above it the chip is busy either way
// and the split only adds barriers.  MCR_K1_SPLIT_MAX_WAVES overrides it (0 = never).
static unsigned split_max_waves() {   // (read at every launch: tests compare both forms in one process)
    const char* e = std::getenv("MCR_K1_SPLIT_MAX_WAVES");
    return (e && *e) ? (unsigned)std::strtoul(e, nullptr, 10) : 3072u;
}
// Plan of a time-sliced launch (PHASE 3 of path_kernel): how many path blocks are sliced, into how many segments, at which
// retirement years.  Resident slots = CUs x 6 workgroups (count-only) or x 5 (variants with per-path outputs); the slices are equal in COST
// (an accumulation month is ~0.83 of a retirement month: no withdrawal).
struct SegmentPlan { int n_split, n_full, q, max_polls, year[kMaxSegments + 1]; };
static bool plan_segments(const DevParams& d, unsigned n_blocks, int mode, SegmentPlan* plan, bool retirement_only = false) {
    int q = -1;     // (chosen below from the shape of the launch unless the environment says otherwise)
    if (const char* e = std::getenv("MCR_K1_SEGMENTS")) q = std::atoi(e);
    if (q >= 0 && q < 2) return false;
    static int cus_cached = 0;         // (one device model per process in practice; a wrong figure costs time, not results)
    if (cus_cached == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
        cus_cached = cus;
    }
    const unsigned slots = (unsigned)cus_cached * (mode == 0 ? 6u : 5u);     // resident workgroups: the variants' launch bounds
    if (n_blocks <= slots || d.retirement_years < 4 || d.n_extra_streams > 0 || d.n_lock_slots < d.n_lock_slots_total) return false;
    if (q < 0) q = n_blocks < 2 * slots ? 8 : 6;     // (measured: 500 000 paths 3.12 ms plain, 2.77 with 4 segments, 2.58 with 6; 10^6 and 2 10^6: 6 = 4 - 0.4 %)
    q = std::min(std::min(q, kMaxSegments), d.retirement_years / 2);
    // Worth it where the last round of a plain launch is mostly empty: rounds r = blocks / slots, loss of the plain launch up to
    // ceil(r) / r.  Measured (10^6-path neighbourhood, tools/k1_segments_ab.py): r = 2.54 -3.8 %, 2.29 -7 %, 5.09 -5.6 %, 1.27
    // -11 %; r = 2.0, 3.0 +2 % (nothing to gain, the extra workgroups cost), 2.8 +1 %, 3.81 0.  MCR_K1_SEGMENTS_ALWAYS=1 (tests).
    const double r = (double)n_blocks / (double)slots;
    const char* always = std::getenv("MCR_K1_SEGMENTS_ALWAYS");
    if (!(always && always[0] == '1') && std::ceil(r) / r < 1.08) return false;
    plan->max_polls = 20000;            // x ~1 us; a successor is dispatched long after its predecessor has finished
    if (const char* e = std::getenv("MCR_K1_SEGMENT_POLLS")) plan->max_polls = std::max(0, std::atoi(e));   // (0: every successor recomputes — tests)
    plan->q = q;
    plan->n_split = (int)slots;
    plan->n_full = (int)(n_blocks - slots);
    const double acc = retirement_only ? 0.0 : 0.83 * d.working_months, total = acc + (double)kMPY * d.retirement_years;   // (PHASE 4: the candidates resume at retirement)
    plan->year[0] = 0;
    for (int k = 1; k < q; ++k) {
        int y = (int)std::lround((total * k / q - acc) / kMPY);
        y = std::max(y, plan->year[k - 1] + (k == 1 ? 0 : 1));
        plan->year[k] = std::min(y, d.retirement_years - (q - k));
        if (plan->year[k] < plan->year[k - 1]) return false;
    }
    plan->year[q] = d.retirement_years;
    return true;
}
// MCR_K1_SEGMENT_ORDER=k_0,k_1,...,k_(q-1) (tests; read at every launch): a time-sliced grid goes out as 1 + q launches on the
// stream instead of one — the whole blocks first, then the pieces of n_split workgroups of segment k_0, k_1, ... — so that every
// order in which the segments of a block can run is reproducible: launches on one stream run one after another, so a segment
// whose predecessor's piece comes later sees its flag at 0 for its whole poll budget, and one whose predecessor's piece came
// earlier sees it raised at its first poll.  Set on a launch that does not slice, or not a permutation of 0 .. q - 1: an error
// (a test must never pass by comparing the plain launch with itself).
static const char* segment_order_env() {
    const char* e = std::getenv("MCR_K1_SEGMENT_ORDER");
    return (e && *e) ? e : nullptr;
}
static int parse_segment_order(const char* e, int q, int* order) {
    int n = 0;
    unsigned seen = 0u;
    for (const char* s = e;; ) {
        char* end = nullptr;
        const long k = std::strtol(s, &end, 10);
        if (end == s || k < 0 || k >= q || n >= q || ((seen >> k) & 1u) || (*end != ',' && *end != '\0')) {
            set_error("MCR_K1_SEGMENT_ORDER=%s is not a permutation of the launch's %d segments 0..%d", e, q, q - 1);
            return MCR_ERR_INVALID_ARG;
        }
        seen |= 1u << k;
        order[n++] = (int)k;
        if (*end == '\0') break;
        s = end + 1;
    }
    if (n != q) { set_error("MCR_K1_SEGMENT_ORDER=%s is not a permutation of the launch's %d segments 0..%d", e, q, q - 1); return MCR_ERR_INVALID_ARG; }
    return MCR_OK;
}
// The time-sliced grid [segment 0 x S] [F whole blocks] [segment 1 x S] ... [segment q - 1 x S]: one launch, or (order != nullptr,
// MCR_K1_SEGMENT_ORDER) the F whole blocks followed by one launch of S workgroups per segment in the given order.
template <typename Kernel>
static void launch_sliced(Kernel kernel, const SegmentPlan& plan, const int* order, dim3 block, size_t lds, hipStream_t stream,
                          const DevParams& d, KernelIO io, const DevParams* cand) {
    if (!order) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)(plan.n_full + plan.q * plan.n_split)), block, lds, stream, d, io, cand);
        return;
    }
    if (plan.n_full > 0) {
        io.seg_bid_base = plan.n_split;
        hipLaunchKernelGGL(kernel, dim3((unsigned)plan.n_full), block, lds, stream, d, io, cand);
    }
    for (int i = 0; i < plan.q; ++i) {
        io.seg_bid_base = order[i] == 0 ? 0 : plan.n_split + plan.n_full + (order[i] - 1) * plan.n_split;
        hipLaunchKernelGGL(kernel, dim3((unsigned)plan.n_split), block, lds, stream, d, io, cand);
    }
}

// host_table: rng->history is host memory (the *_host_rng entry points), so its entries can be checked too
static int check_rng(const mcr_rng* rng, bool host_table = false) {
    if (!rng) { set_error("null rng"); return MCR_ERR_INVALID_ARG; }
    if (rng->kind != MCR_RNG_PHILOX && rng->kind != MCR_RNG_NUMPY && rng->kind != MCR_RNG_HISTORY) { set_error("unknown rng kind %u", rng->kind); return MCR_ERR_INVALID_ARG; }
    if (rng->kind == MCR_RNG_HISTORY) {
        if (!rng->history) { set_error("history rng: null history table"); return MCR_ERR_INVALID_ARG; }
        if (rng->history_months < 1 || rng->history_months > MCR_MAX_HISTORY_MONTHS) {
            set_error("history rng: history_months = %u (1..%d)", rng->history_months, MCR_MAX_HISTORY_MONTHS);
            return MCR_ERR_INVALID_ARG;
        }
        if (rng->history_block < 1 || rng->history_block > (uint32_t)INT32_MAX) {
            set_error("history rng: history_block = %u (1..%d)", rng->history_block, INT32_MAX);
            return MCR_ERR_INVALID_ARG;
        }
        if (rng->history_scheme > MCR_HISTORY_COHORTS) {
            set_error("history rng: history_scheme = %u (0..%u)", rng->history_scheme, MCR_HISTORY_COHORTS);
            return MCR_ERR_INVALID_ARG;
        }
        if (rng->history_reserved != 0u) {
            set_error("history rng: history_reserved = %u (must be 0)", rng->history_reserved);
            return MCR_ERR_INVALID_ARG;
        }
        if (host_table)
            for (uint32_t k = 0; k < 3u * rng->history_months; ++k)
                if (!std::isfinite(rng->history[k])) {
                    set_error("history rng: history[%u][%u] = %g: the table must be finite", k / 3u, k % 3u, rng->history[k]);
                    return MCR_ERR_INVALID_ARG;
                }
    }
    if (rng->kind == MCR_RNG_NUMPY && !rng->path_seeds &&
        (rng->n_entropy_words < 1 || rng->n_entropy_words > MCR_MAX_ENTROPY_WORDS)) {
        set_error("numpy rng: main seed must have 1..%d uint32 words (got %u)", MCR_MAX_ENTROPY_WORDS, rng->n_entropy_words);
        return MCR_ERR_INVALID_ARG;
    }
    return MCR_OK;
}

// A history descriptor of a *_host_rng call is judged before the device is entered: a bad table is the caller's error with or
// without a GPU (the other kinds keep their order: device first)
static int check_history_host(const mcr_rng* rng) { return rng && rng->kind == MCR_RNG_HISTORY ? check_rng(rng, true) : MCR_OK; }

// path_kernel's RNG template argument for a launch on this descriptor
static uint32_t kernel_rng_kind(const mcr_rng* rng) {
    return rng->kind == MCR_RNG_HISTORY && rng->history_scheme != MCR_HISTORY_BLOCK ? (uint32_t)kRngHistorySchemes : rng->kind;
}

static void fill_io_rng(KernelIO& io, const mcr_rng* rng, const uint32_t* device_path_seeds) {
    io.seed = rng->philox_seed;
    io.n_entropy = rng->n_entropy_words;
    for (int i = 0; i < MCR_MAX_ENTROPY_WORDS; ++i) io.entropy[i] = rng->entropy[i];
    io.child_offset = rng->child_offset;
    io.path_seeds = device_path_seeds;
    if (rng->kind == MCR_RNG_HISTORY) {      // (a DEVICE table here: the fields lie over the NumPy stream's, KernelIO)
        io.history = rng->history; io.history_months = rng->history_months; io.history_block = rng->history_block;
        io.history_scheme = rng->history_scheme;
    }
}

static KernelIO make_io(const mcr_rng* rng, const uint32_t* device_path_seeds, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths) {
    KernelIO io;
    std::memset(&io, 0, sizeof(io));
    fill_io_rng(io, rng, device_path_seeds);
    io.stream_id = stream_id; io.path_begin = path_begin; io.n_paths = n_paths;
    return io;
}
static mcr_outputs counters_only(uint64_t* counters) {
    mcr_outputs o;
    std::memset(&o, 0, sizeof(o));
    o.counters = counters;
    return o;
}

// Run-time properties of a launch -> template arguments of path_kernel: each helper calls the generic lambda `f` with
// std::integral_constant values, and the lambda names its variant with decltype(T)::value.  A call site instantiates its
// lambda for every value its helper can pass, no more: the helpers a launch goes through ARE its list of compiled variants.
template <int V> using int_c = std::integral_constant<int, V>;
template <typename F> static inline void for_bool(bool b, F&& f) { if (b) f(std::true_type{}); else f(std::false_type{}); }
// f(T, A): T = the tax mask (which of the two assets is taxed on realized gains), A = any annual-gains tax
template <typename F> static inline void for_tax_variant(const DevParams& d, F&& f) {
    for_bool(d.any_annual_tax, [&](auto A) {
        switch (d.tax_mask) { case 0: f(int_c<0>{}, A); break; case 1: f(int_c<1>{}, A); break; case 2: f(int_c<2>{}, A); break; default: f(int_c<3>{}, A); break; }
    });
}
// f(G): G = the launch's growth form (growth_form_of): the masks path_kernel is instantiated for
template <typename F> static inline void for_growth_form(int gf, F&& f) {
    if (gf == (kGrowthNarrowExp | kGrowthRhoZero)) f(int_c<kGrowthNarrowExp | kGrowthRhoZero>{});
    else if (gf == kGrowthNarrowExp) f(int_c<kGrowthNarrowExp>{});
    else f(int_c<0>{});
}
// f(F): F = the launch's month form (month_form_of).  T = the kernel's tax mask: only mask 3 has the equal-rates variant
// (month_form_of gives the bit to no other launch), so the others instantiate the general month alone — as does every kernel
// of the exact-month build (kExactMonthDefault), where the variant does not exist
template <int T, typename F> static inline void for_month_form(int mf, F&& f) {
    if constexpr (T == 3 && !kExactMonthDefault) { if (mf == kMonthEqualRates) { f(int_c<kMonthEqualRates>{}); return; } }
    f(int_c<0>{});
}
// f(S): S = the launch's stream form (stream_form_of); the exact-month build has none
template <typename F> static inline void for_stream_form(int sf, F&& f) {
    if constexpr (!kExactMonthDefault) { if (sf == kStreamsInRegs) { f(int_c<kStreamsInRegs>{}); return; } }
    f(int_c<0>{});
}
// whether path_kernel<MODE, RNG, ., ANNUAL, ...> of a whole-path or time-sliced launch has growth variants (kPerPathPhilox)
template <int MODE, int RNG, bool ANNUAL, bool XS> constexpr bool kHasGrowthForms = MODE == 0 && RNG == 0 && !ANNUAL && !XS;
template <typename F> static inline void for_output_mode(int mode, F&& f) {
    if (mode == 2) f(int_c<2>{}); else if (mode == 1) f(int_c<1>{}); else f(int_c<0>{});
}

// rng_kind: mcr_rng.kind, or kernel_rng_kind() of the descriptor (a history launch's scheme chooses between two sets of kernels).
// f(R, T, A, X, E) = (stream, tax mask, annual-gains tax, extended streams, exact month) of a whole-path launch (PHASE 0, not
// split, no injection) — the one place that says which variants such a launch has: the generic form (mask 3, annual) for
// extended streams / the exact month; the engine's own stream per tax mask; the NumPy and history streams taxed / untaxed
// only (mask 3 computes a zero-rate asset's tax arithmetic as exact zeros)
template <typename F> static inline void for_whole_path_variant(const DevParams& d, uint32_t rng_kind, bool xs, bool exact, F&& f) {
    auto with_stream = [&](auto R) {
        if (xs) {
            if (exact) f(R, int_c<3>{}, std::true_type{}, std::true_type{}, std::true_type{});
            else f(R, int_c<3>{}, std::true_type{}, std::true_type{}, std::false_type{});
        } else if constexpr (decltype(R)::value == 0) {
            for_tax_variant(d, [&](auto T, auto A) { f(R, T, A, std::false_type{}, std::false_type{}); });
        } else {
            for_bool(d.any_annual_tax, [&](auto A) {
                if (d.any_real_rate) f(R, int_c<3>{}, A, std::false_type{}, std::false_type{});
                else f(R, int_c<0>{}, A, std::false_type{}, std::false_type{});
            });
        }
    };
    if (rng_kind == (uint32_t)kRngHistorySchemes) with_stream(int_c<kRngHistorySchemes>{});
    else if (rng_kind == MCR_RNG_HISTORY) with_stream(int_c<(int)MCR_RNG_HISTORY>{});
    else if (rng_kind == MCR_RNG_NUMPY) with_stream(int_c<(int)MCR_RNG_NUMPY>{});
    else with_stream(int_c<0>{});
}
// The generic variants (XS) carry what the lean ones leave out: records beyond the by-value block and both forms of the month
static bool needs_exact_month(const DevParams& d) { return d.exact_month && !kExactMonthDefault; }
static bool needs_generic_variant(const DevParams& d) { return d.n_extra_streams > 0 || needs_exact_month(d); }
// The producer / consumer forms count on both halves of a workgroup executing the same number of barriers: producers run
// rows [first, total_months), consumers the accumulation months + 12 months per retirement year.  (They also count on gfx9's
// s_barrier not waiting for waves that have ended — producers return while consumers still reduce their counts.)
// Two producers (path_kernel's NPROD = 2): barrier p hands pair p over, p < ceil(total_months / 2) — the consumer executes it
// at row 2 p, which it visits for exactly those p when its months add up to total_months; each producer executes it behind
// its own pair p or in the middle of (or, at the end, instead of) its pair p + 1.  The same identity, and at least one month.
static int check_barrier_counts(const DevParams& d, int producers = 1) {
    if (d.total_months == d.working_months + kMPY * d.retirement_years && (producers == 1 || d.total_months >= 1)) return MCR_OK;
    set_error("internal: total_months != working_months + 12 retirement_years");
    return MCR_ERR_INVALID_ARG;
}

// The hand-over memory of a time-sliced launch (PHASE 3 / 4): [n_split][n_fields][kBlock] state + [n_split][q] flags, zeroed.
struct SegmentHandOver {
    StreamAlloc mem;
    explicit SegmentHandOver(hipStream_t s) : mem(s) {}
    // false: the allocation was refused; otherwise *zeroed is the status of the flags' memset, and io.seg_* are filled if it succeeded
    bool attach(KernelIO& io, const SegmentPlan& plan, int n_fields, hipError_t* zeroed) {
        const size_t state_bytes = (size_t)plan.n_split * (size_t)n_fields * kBlock * sizeof(double);
        const size_t flag_bytes = (size_t)plan.n_split * (size_t)plan.q * sizeof(unsigned int);
        if (!mem.alloc(state_bytes + flag_bytes)) return false;
        *zeroed = hipMemsetAsync((char*)mem.p + state_bytes, 0, flag_bytes, mem.stream);
        if (*zeroed != hipSuccess) return true;
        io.seg_state = (double*)mem.p;
        io.seg_flags = (unsigned int*)((char*)mem.p + state_bytes);
        io.seg_n_split = plan.n_split; io.seg_n_full = plan.n_full; io.seg_q = plan.q; io.seg_max_polls = plan.max_polls;
        for (int k = 0; k <= plan.q; ++k) io.seg_year[k] = plan.year[k];
        return true;
    }
    hipError_t release() { return mem.release(); }
};

// ---------------------------------------------------------------------------------------------
// The SCREENED route of a count-only launch (mcr_screen.h): screen_kernel classifies every path in fp32 and counts the SAFE
// ones; path_kernel's LIST form re-runs the DOUBTFUL ones in fp64 and adds its counts to the same vectors.
// ---------------------------------------------------------------------------------------------
// Which parameter blocks can be screened: the launches that have growth, month and stream forms (no annual-gains tax, the
// tolerance month, no extended streams) whose kept income records are at most two, all indexed (kStreamsInRegs).
static bool screen_qualified(const DevParams& d) {
    return !kExactMonthDefault && !d.any_annual_tax && !d.exact_month && d.n_extra_streams == 0 && stream_form_qualified(d) == kStreamsInRegs;
}
// Smallest launch that takes the route by default: the measured crossover (LABNOTES R24); MCR_K1_SCREEN_MIN_PATHS moves it.
constexpr uint64_t kScreenMinPathsDefault = 500000;
// The knobs that address the classic kernels: a launch under any of them takes the classic route
static const char* const kClassicKnobs[] = {"MCR_K1_SEGMENTS", "MCR_K1_SEGMENTS_ALWAYS", "MCR_K1_SEGMENT_ORDER", "MCR_K1_SEGMENT_POLLS",
                                            "MCR_K1_GROWTH_FORM", "MCR_K1_MONTH_FORM", "MCR_K1_STREAM_FORM"};
// Producer waves per consumer wave of the re-run's producer / consumer form: 1 = the 256-path workgroup of the lone probes
// (four consumer and four producer waves), 2 = one 64-path block per workgroup with one consumer and two producer waves
// (path_kernel's NPROD).  MCR_K1_RERUN_PRODUCERS, read at every launch, forces one; left alone, a launch whose EXPECTED list
// (n x MCR_K1_SCREEN_EXPECTED) is at most kRerunTwoProducersMaxList paths takes the 64-path form and every other one the
// 256-path form.  The limit is the largest measured size at which the 64-path form is not the slower one: faster by 0.11 ms
// at 250 000 and 500 000 paths, by 0.058 ms of the re-run at 10^6, SLOWER by 0.09 ms at 2 10^6 (LABNOTES R30; nothing was
// measured between the last two, so the limit stands at the lower).  `expected_list` < 0: the caller only validates the knob.
constexpr int kRerunProducersDefault = 1;
constexpr double kRerunTwoProducersMaxList = 80000.0;     // = 10^6 paths x the default MCR_K1_SCREEN_EXPECTED
static int rerun_producers_of(int* producers, double expected_list = -1.0) {
    *producers = (expected_list >= 0.0 && expected_list <= kRerunTwoProducersMaxList) ? 2 : kRerunProducersDefault;
    if (const char* e = std::getenv("MCR_K1_RERUN_PRODUCERS"); e && *e) {
        if ((e[0] != '1' && e[0] != '2') || e[1] != '\0') { set_error("MCR_K1_RERUN_PRODUCERS=%s: 1 (the 256-path form) or 2 (64 paths, two producer waves)", e); return MCR_ERR_INVALID_ARG; }
        *producers = e[0] - '0';
    }
    return MCR_OK;
}
// *screened = whether a count-only launch (no per-path output, no injected shocks, `hist_n_bins` histogram bins) of n_paths
// paths of `d` on `rng` takes the screened route.  MCR_K1_SCREEN=0 turns the route off, =1 forces it on at any size.
static int screen_route_of(const DevParams& d, const mcr_rng* rng, uint64_t n_paths, int hist_n_bins, bool* screened) {
    *screened = false;
    int force = -1;
    if (const char* e = std::getenv("MCR_K1_SCREEN"); e && *e) {
        if ((e[0] != '0' && e[0] != '1') || e[1] != '\0') { set_error("MCR_K1_SCREEN=%s: 0 (never) or 1 (whenever the launch qualifies)", e); return MCR_ERR_INVALID_ARG; }
        force = e[0] - '0';
    }
    int producers = 0;
    if (int rc = rerun_producers_of(&producers)) return rc;      // (junk in the re-run's knob is an error wherever the route is asked about)
    if (force == 0 || !screen_qualified(d) || (rng && rng->kind != MCR_RNG_PHILOX) || hist_n_bins != 0) return MCR_OK;
    if (n_paths == 0 || n_paths > (uint64_t)UINT32_MAX) return MCR_OK;     // (the list holds 32-bit local indices)
    for (const char* knob : kClassicKnobs) { const char* e = std::getenv(knob); if (e && *e) return MCR_OK; }
    uint64_t min_paths = kScreenMinPathsDefault;
    if (const char* e = std::getenv("MCR_K1_SCREEN_MIN_PATHS"); e && *e) {
        char* end = nullptr;
        min_paths = std::strtoull(e, &end, 10);
        if (*end != '\0') { set_error("MCR_K1_SCREEN_MIN_PATHS=%s: a path count", e); return MCR_ERR_INVALID_ARG; }
    }
    *screened = force == 1 || n_paths >= min_paths;
    return MCR_OK;
}
// Share of a screened launch's paths expected on the list: sizes the choice between the two forms of the re-run
static double screen_expected() {
    const char* e = std::getenv("MCR_K1_SCREEN_EXPECTED");
    const double v = (e && *e) ? std::strtod(e, nullptr) : 0.08;
    return v > 0.0 ? v : 0.08;
}
// The screening kernel's parameter block: every value derived in double, rounded once
static ScreenParams screen_params(const DevParams& d) {
    const double log2e = 1.4426950408889634074;
    const double bscale = log2e * 1.1774100225154746910;      // the slopes carry sqrt(2 ln 2): a normal is sqrt(-log2 u) x trig (screen_factors2)
    ScreenParams s;
    std::memset(&s, 0, sizeof(s));
    s.a1 = (float)(d.a1 * log2e); s.b1 = (float)(d.b1 * bscale);
    s.ainf = (float)(d.ainf * log2e); s.binf_rho = (float)(d.binf_rho * bscale); s.binf_rho_c = (float)(d.binf_rho_c * bscale);
    s.aprem = (float)(d.aprem * log2e); s.bprem = (float)(d.bprem * bscale);
    const double b1 = d.initial_balance * d.alloc1;
    s.b1_0 = (float)b1; s.b2_0 = (float)(d.initial_balance - b1);
    s.contrib = (float)d.monthly_contribution; s.contrib_growth_factor = (float)d.contrib_growth_factor;
    s.alloc1 = (float)d.alloc1;
    const double keep0 = d.n_streams > 0 ? d.streams[0].amount_keep : 0.0, keep1 = d.n_streams > 1 ? d.streams[1].amount_keep : 0.0;
    auto lvl0 = [](double e) { return (float)(e < 0.0 ? 0.0 : e); };       // (price > 0: max(0, price x E) = price x max(0, E))
    s.e00 = lvl0(d.monthly_expenses); s.e10 = lvl0(d.monthly_expenses - keep0);
    s.e01 = lvl0(d.monthly_expenses - keep1); s.e11 = lvl0(d.monthly_expenses - keep0 - keep1);
    s.rate1 = (float)d.real_rate1; s.rate2 = (float)d.real_rate2;
    s.ar1 = (float)(d.alloc1 * d.real_rate1); s.ar2 = (float)(d.alloc2 * d.real_rate2);
    const int wm = d.working_months;
    auto to_row = [&](int32_t m) { return m > INT32_MAX - wm ? INT32_MAX : m + wm; };      // (path_kernel's StreamRegs)
    auto window_months = [](int first, int end) { return end > first ? (uint32_t)(end - first) : 0u; };
    if (d.n_streams > 0) { s.s0 = to_row(d.streams[0].start_month); s.n0 = window_months(s.s0, to_row(d.streams[0].end_month)); }
    if (d.n_streams > 1) { s.s1 = to_row(d.streams[1].start_month); s.n1 = window_months(s.s1, to_row(d.streams[1].end_month)); }
    s.working_months = wm; s.retirement_years = d.retirement_years; s.total_months = d.total_months; s.contrib_grows = d.contrib_grows;
    return s;
}
template <bool HOOK>
static void launch_screen_kernel(const DevParams& d, const ScreenParams& sp, const ScreenIO& sio, dim3 grid, hipStream_t stream) {
    const bool eqr = month_form_qualified(d) == kMonthEqualRates;
    const bool rho0 = d.rho == 0.0;          // (growth_form_qualified's test: binf_rho is then an exact zero)
    auto go = [&](auto R) {
        constexpr bool RHO0 = decltype(R)::value;
        switch (d.tax_mask) {
            case 0: hipLaunchKernelGGL((screen_kernel<0, false, RHO0, HOOK>), grid, dim3(kBlock), 0, stream, sp, sio); break;
            case 1: hipLaunchKernelGGL((screen_kernel<1, false, RHO0, HOOK>), grid, dim3(kBlock), 0, stream, sp, sio); break;
            case 2: hipLaunchKernelGGL((screen_kernel<2, false, RHO0, HOOK>), grid, dim3(kBlock), 0, stream, sp, sio); break;
            default:
                if (eqr) hipLaunchKernelGGL((screen_kernel<3, true, RHO0, HOOK>), grid, dim3(kBlock), 0, stream, sp, sio);
                else hipLaunchKernelGGL((screen_kernel<3, false, RHO0, HOOK>), grid, dim3(kBlock), 0, stream, sp, sio);
        }
    };
    if (rho0) go(std::true_type{}); else go(std::false_type{});
}
// One screened launch.  `d` is the launch's parameter block (screen_qualified), `io` its kernel arguments (count-only).  The
// list and its count are one stream-ordered allocation, 4 n + 8 bytes, the count zeroed on the stream and the block freed
// behind the re-run.  The host never reads the count: the re-run's grid is sized from the bound ceil(n / 256) (ceil(n / 64)
// for the 64-path form), and its workgroups beyond the count return at once.  The re-run takes a producer / consumer form
// when the EXPECTED list (n x MCR_K1_SCREEN_EXPECTED) is a latency-bound launch: the 64-path form with two producer waves, or
// the 256-path one (rerun_producers_of), both in the launch's stream and month forms (screen_qualified gives every screened
// launch the stream form).  MCR_ERR_UNSUPPORTED: the allocation was refused, nothing enqueued.
static int launch_screened(DevParams d, KernelIO io, hipStream_t stream) {
    const uint64_t n = io.n_paths;
    int producers = 1;
    int rc = rerun_producers_of(&producers, (double)n * screen_expected());
    if (rc != MCR_OK) return rc;
    StreamAlloc mem(stream);
    if (!mem.alloc(4 * (size_t)n + 8)) return MCR_ERR_UNSUPPORTED;
    uint32_t* const count = (uint32_t*)mem.p;
    uint32_t* const list = (uint32_t*)((char*)mem.p + 8);
    hipError_t e = hipMemsetAsync(count, 0, 8, stream);
    if (e != hipSuccess) return hip_fail(e, "screened launch: zeroing the list's count");
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock)), block(kBlock);
    ScreenIO sio;
    std::memset(&sio, 0, sizeof(sio));
    sio.seed = io.seed; sio.path_begin = io.path_begin; sio.n_paths = n; sio.stream_id = io.stream_id;
    sio.counters = io.out.counters; sio.wr_obs_counts = io.out.wr_obs_counts; sio.list = list; sio.list_count = count;
    launch_screen_kernel<false>(d, screen_params(d), sio, grid, stream);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "screen_kernel launch");
    bool split = (double)n * screen_expected() / 64.0 <= (double)split_max_waves();
    rc = split ? check_barrier_counts(d, producers) : MCR_OK;
    if (rc != MCR_OK) return rc;
    size_t lds = 0;
    rc = plan_path_kernel_lds(d, 0, MCR_RNG_PHILOX, false, split, 0, &lds);     // (the plan counts the 256-path form's 24 KB stage and 256 columns: a bound for the 64-path form's 6 KB and 64)
    if (rc != MCR_OK) return rc;
    io.path_list = list; io.path_list_count = count;
    const DevParams* const no_cand = nullptr;
    const int mf = month_form_qualified(d);
    if (split && producers == 2) {
        // the grid's bound is ceil(n / 64) workgroups of one 64-path block; those beyond the count return at once
        const dim3 grid64((unsigned)((n + 63) / 64));
        for_tax_variant(d, [&](auto T, auto A) {
            if constexpr (!decltype(A)::value && !kExactMonthDefault)
                for_month_form<decltype(T)::value>(mf, [&](auto F) {
                    hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, false, false, 0, true, false, false, 0, decltype(F)::value, kStreamsInRegs, false, true, 2>),
                                       grid64, dim3(3 * 64), lds, stream, d, io, no_cand);
                });
        });
    } else if (split) {
        for_tax_variant(d, [&](auto T, auto A) {
            if constexpr (!decltype(A)::value && !kExactMonthDefault)
                for_month_form<decltype(T)::value>(mf, [&](auto F) {
                    hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, false, false, 0, true, false, false, 0, decltype(F)::value, kStreamsInRegs, false, true>),
                                       grid, dim3(2 * kBlock), lds, stream, d, io, no_cand);
                });
        });
    } else {
        const int gf = growth_form_qualified(d);
        for_tax_variant(d, [&](auto T, auto A) {
            if constexpr (!decltype(A)::value && !kExactMonthDefault)
                for_growth_form(gf, [&](auto G) {
                    for_month_form<decltype(T)::value>(mf, [&](auto F) {
                        hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, false, false, 0, false, false, false, decltype(G)::value, decltype(F)::value, kStreamsInRegs, false, true>),
                                           grid, block, lds, stream, d, io, no_cand);
                    });
                });
        });
    }
    e = hipGetLastError();
    const hipError_t ef = mem.release();
    if (e != hipSuccess) return hip_fail(e, "path_kernel launch (screened re-run)");
    if (ef != hipSuccess) return hip_fail(ef, "screened launch: list release");
    return MCR_OK;
}

static int launch_paths(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                        uint64_t n_paths, int32_t wm, const double* injected, const mcr_outputs* out,
                        hipStream_t stream) {
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, wm, &d, &extra);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    if (!out) { set_error("null outputs"); return MCR_ERR_INVALID_ARG; }
    if (n_paths == 0) return MCR_OK;
    if (n_paths > (uint64_t)INT32_MAX * kBlock) { set_error("n_paths too large for one launch"); return MCR_ERR_INVALID_ARG; }
    if (path_begin + n_paths < path_begin) { set_error("path range overflows 64 bits"); return MCR_ERR_INVALID_ARG; }
    const bool want_traj = out->trajectory || out->real_trajectory || out->withdrawal_rate_trajectory;
    const bool want_summary = out->start_balance || out->final_balance || out->years_to_ruin ||
                              out->first_year_gross_withdrawal || out->first_year_real_gross_withdrawal ||
                              out->inflation_at_retirement || out->success;
    KernelIO io = make_io(rng, rng->path_seeds, stream_id, path_begin, n_paths);
    io.injected = injected; io.out = *out;
    if (io.out.path_stride <= 0) io.out.path_stride = (int64_t)n_paths;
    if (want_traj && (uint64_t)io.out.path_stride < n_paths) {
        set_error("path_stride %lld < n_paths %llu", (long long)io.out.path_stride, (unsigned long long)n_paths);
        return MCR_ERR_INVALID_ARG;
    }
    const uint32_t rng_kind = rng->kind;
    const bool np_rng = rng_kind != MCR_RNG_PHILOX;      // the NumPy or the history stream: whole-path launches only
    if (io.out.hist_bins == nullptr || io.out.hist_n_bins == 0) { io.out.hist_bins = nullptr; io.out.hist_edges = nullptr; io.out.hist_n_bins = 0; }
    if (io.out.hist_bins && (io.out.hist_n_bins < 0 || io.out.hist_n_bins > MCR_MAX_HIST_BINS || !io.out.hist_edges)) {
        set_error("hist_bins requested with hist_n_bins = %d (1..%d) / hist_edges = %p", io.out.hist_n_bins, MCR_MAX_HIST_BINS, (const void*)io.out.hist_edges);
        return MCR_ERR_INVALID_ARG;
    }
    const dim3 grid((unsigned)((n_paths + kBlock - 1) / kBlock)), block(kBlock);
    const int mode = injected ? 2 : (want_traj ? 2 : (want_summary ? 1 : 0));
    // kernel variant: output mode x RNG x (any effective realized-gains rate?) x (any annual-gains tax?); injected
    // shocks (parity hook) always take the full-output variant, whose every store is null-checked
    bool split = !injected && !np_rng && mode == 0 && (uint64_t)grid.x * (kBlock / 64) <= split_max_waves();
    if (split && (rc = check_barrier_counts(d)) != MCR_OK) return rc;
    size_t lds = 0;
    rc = plan_path_kernel_lds(d, mode, rng_kind, injected != nullptr, split, io.out.hist_n_bins, &lds, 0, rng->history_months);
    if (rc != MCR_OK) return rc;
    if (split && (d.n_lock_slots < d.n_lock_slots_total || needs_generic_variant(d))) {
        // the producer / consumer form doubles the stage: where only IT cannot hold every lock column, the unsplit kernel runs
        split = false;
        rc = plan_path_kernel_lds(d, mode, rng_kind, false, false, io.out.hist_n_bins, &lds);
        if (rc != MCR_OK) return rc;
    }
    // XS: records beyond the by-value block and / or lock slots beyond the LDS budget -> the extended-stream variants
    //     (and configurations that need the exact month: the generic variants carry both forms of it)
    const bool exact = needs_exact_month(d);
    const bool xs = d.n_lock_slots < d.n_lock_slots_total || needs_generic_variant(d);
    const char* seg_order = segment_order_env();
    if (seg_order && (np_rng || injected || xs || split)) {
        set_error("MCR_K1_SEGMENT_ORDER=%s set on a launch that is not time-sliced (%s)", seg_order,
                  rng_kind == MCR_RNG_HISTORY ? "history stream" : np_rng ? "NumPy stream" : injected ? "injected shocks" : xs ? "extended streams / exact month" : "producer / consumer split");
        return MCR_ERR_INVALID_ARG;
    }
    // growth form of the launch: the whole-path and time-sliced count-only kernels of the engine's own stream have the variants
    int gf = 0;
    rc = growth_form_of(d, !np_rng && !injected && !xs && !split && mode == 0 && !d.any_annual_tax, &gf);
    if (rc != MCR_OK) return rc;
    int mf = 0;     // ... and its month form: the same kernels
    rc = month_form_of(d, !np_rng && !injected && !xs && !split && mode == 0 && !d.any_annual_tax, &mf);
    if (rc != MCR_OK) return rc;
    int sf = 0;     // ... and its stream form
    rc = stream_form_of(d, !np_rng && !injected && !xs && !split && mode == 0 && !d.any_annual_tax, &sf);
    if (rc != MCR_OK) return rc;
    // the screened route (launch_screened): count-only launches of the engine's own stream whose parameters qualify
    if (!injected && !np_rng && mode == 0 && !xs) {
        bool screened = false;
        rc = screen_route_of(d, rng, n_paths, io.out.hist_n_bins, &screened);
        if (rc != MCR_OK) return rc;
        if (screened) {
            rc = launch_screened(d, io, stream);
            if (rc != MCR_ERR_UNSUPPORTED) return rc;      // (allocation refused: the classic route below)
        }
    }
    StreamSideBlock side(stream);
    rc = side.attach(d, extra, grid.x);
    if (rc != MCR_OK) return rc;
    const DevParams* const no_cand = nullptr;
    // the whole-path variants of the engine's streams (for_whole_path_variant), output mode M
    auto launch_whole_path = [&]() {
        for_output_mode(mode, [&](auto M) {
            for_whole_path_variant(d, kernel_rng_kind(rng), xs, exact, [&](auto R, auto T, auto A, auto X, auto EX) {
                if constexpr (kHasGrowthForms<decltype(M)::value, decltype(R)::value, decltype(A)::value, decltype(X)::value>) {
                    for_growth_form(gf, [&](auto G) {
                        for_month_form<decltype(T)::value>(mf, [&](auto F) {
                            for_stream_form(sf, [&](auto S) {
                                hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, false, false, 0, false, false, kExactMonthDefault, decltype(G)::value, decltype(F)::value, decltype(S)::value>),
                                                   grid, block, lds, stream, d, io, no_cand);
                            });
                        });
                    });
                } else {
                    hipLaunchKernelGGL((path_kernel<decltype(M)::value, decltype(R)::value, decltype(T)::value, decltype(A)::value, false, 0, false,
                                                    decltype(X)::value, (decltype(X)::value && decltype(EX)::value) || kExactMonthDefault>),
                                       grid, block, lds, stream, d, io, no_cand);
                }
            });
        });
    };
    if (xs) {
        if (injected) {
            if (exact) hipLaunchKernelGGL((path_kernel<2, 0, 3, true, true, 0, false, true, true>), grid, block, lds, stream, d, io, no_cand);
            else hipLaunchKernelGGL((path_kernel<2, 0, 3, true, true, 0, false, true>), grid, block, lds, stream, d, io, no_cand);
        } else launch_whole_path();
        hipError_t ex = hipGetLastError();
        const hipError_t ef = side.release();
        if (ex != hipSuccess) return hip_fail(ex, "path_kernel launch (extended streams)");
        if (ef != hipSuccess) return hip_fail(ef, "path_kernel launch (extended streams): side block release");
        return MCR_OK;
    }
    // Time-sliced path blocks (PHASE 3 of path_kernel): Philox launches of a few rounds of resident workgroups whose last round
    // would be mostly empty (plan_segments).  MCR_K1_SEGMENTS = segments per sliced block (default 6 or 8; 0 or 1 = never).
    if (!np_rng && !injected && !xs && !split) {
        SegmentPlan plan;
        const bool sliced = plan_segments(d, grid.x, mode, &plan);
        int order[kMaxSegments];
        if (seg_order) {
            if (!sliced) { set_error("MCR_K1_SEGMENT_ORDER=%s set on a launch that is not time-sliced (%u workgroups)", seg_order, grid.x); return MCR_ERR_INVALID_ARG; }
            rc = parse_segment_order(seg_order, plan.q, order);
            if (rc != MCR_OK) return rc;
        }
        SegmentHandOver hand(stream);
        hipError_t e = hipSuccess;
        if (sliced && hand.attach(io, plan, seg_fixed_fields(mode) + d.n_lock_slots, &e)) {
            if (e == hipSuccess) {
                for_output_mode(mode, [&](auto M) {
                    for_tax_variant(d, [&](auto T, auto A) {
                        if constexpr (kHasGrowthForms<decltype(M)::value, 0, decltype(A)::value, false>) {
                            for_growth_form(gf, [&](auto G) {
                                for_month_form<decltype(T)::value>(mf, [&](auto F) {
                                    for_stream_form(sf, [&](auto S) {
                                        launch_sliced(&path_kernel<0, 0, decltype(T)::value, false, false, 3, false, false, kExactMonthDefault, decltype(G)::value, decltype(F)::value, decltype(S)::value>, plan,
                                                      seg_order ? order : nullptr, block, lds, stream, d, io, no_cand);
                                    });
                                });
                            });
                        } else {
                            launch_sliced(&path_kernel<decltype(M)::value, 0, decltype(T)::value, decltype(A)::value, false, 3>, plan,
                                          seg_order ? order : nullptr, block, lds, stream, d, io, no_cand);
                        }
                    });
                });
                e = hipGetLastError();
            }
            const hipError_t ef = hand.release();
            if (e != hipSuccess) return hip_fail(e, "path_kernel launch (time-sliced blocks)");
            if (ef != hipSuccess) return hip_fail(ef, "path_kernel launch (time-sliced blocks): state release");
            return MCR_OK;
        }
        // (allocation refused: the plain launch below)
        if (sliced && seg_order) { set_error("MCR_K1_SEGMENT_ORDER=%s: the hand-over state could not be allocated", seg_order); return MCR_ERR_HIP; }
    }
    if (split) {
        for_tax_variant(d, [&](auto T, auto A) {
            hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, 0, true>), grid, dim3(2 * kBlock), lds, stream, d, io, no_cand);
        });
        hipError_t es = hipGetLastError();
        if (es != hipSuccess) return hip_fail(es, "path_kernel launch (split)");
        return MCR_OK;
    }
    // the parity hook: taxed / untaxed only, like the NumPy stream
    if (injected) {
        for_bool(d.any_annual_tax, [&](auto A) {
            if (d.any_real_rate) hipLaunchKernelGGL((path_kernel<2, 0, 3, decltype(A)::value, true>), grid, block, lds, stream, d, io, no_cand);
            else hipLaunchKernelGGL((path_kernel<2, 0, 0, decltype(A)::value, true>), grid, block, lds, stream, d, io, no_cand);
        });
    } else launch_whole_path();
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "path_kernel launch");
    return MCR_OK;
}

// Spending rule (RULE of path_kernel; mcr_run_rule_rng).  The ranges of include/mcr.h; no device is needed.
static int validate_spending_rule(const mcr_spending_rule* r) {
    if (!r) { set_error("null spending rule"); return MCR_ERR_INVALID_ARG; }
    const struct { const char* name; double v; } fields[] = {{"upper", r->upper}, {"lower", r->lower}, {"cut", r->cut},
                                                             {"raise", r->raise}, {"floor", r->floor}, {"ceiling", r->ceiling}};
    for (const auto& f : fields)
        if (!std::isfinite(f.v)) { set_error("spending rule: %s = %g must be finite", f.name, f.v); return MCR_ERR_INVALID_ARG; }
    if (!(r->upper >= 1.0)) { set_error("spending rule: upper = %g must be >= 1", r->upper); return MCR_ERR_INVALID_ARG; }
    if (!(r->lower >= 0.0 && r->lower <= 1.0)) { set_error("spending rule: lower = %g must be in [0, 1]", r->lower); return MCR_ERR_INVALID_ARG; }
    if (!(r->cut >= 0.0 && r->cut < 1.0)) { set_error("spending rule: cut = %g must be in [0, 1)", r->cut); return MCR_ERR_INVALID_ARG; }
    if (!(r->raise >= 0.0)) { set_error("spending rule: raise = %g must be >= 0", r->raise); return MCR_ERR_INVALID_ARG; }
    if (!(r->floor >= 0.0 && r->floor <= 1.0)) { set_error("spending rule: floor = %g must be in [0, 1]", r->floor); return MCR_ERR_INVALID_ARG; }
    if (!(r->ceiling >= 1.0)) { set_error("spending rule: ceiling = %g must be >= 1", r->ceiling); return MCR_ERR_INVALID_ARG; }
    return MCR_OK;
}

// One plain whole-path launch of the rule kernels: path_kernel<MODE 0 | 1, Philox, mask 3, annual-gains tax or not, ..., RULE>,
// four instantiations.  Everything else a caller can ask for is refused by name before anything is enqueued.
static int launch_rule(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths, int32_t wm,
                       const mcr_spending_rule* rule, const mcr_outputs* out, const mcr_rule_outputs* rule_out, hipStream_t stream) {
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, wm, &d, &extra);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    rc = validate_spending_rule(rule);
    if (rc != MCR_OK) return rc;
    if (!out) { set_error("null outputs"); return MCR_ERR_INVALID_ARG; }
    if (n_paths > (uint64_t)INT32_MAX * kBlock) { set_error("n_paths too large for one launch"); return MCR_ERR_INVALID_ARG; }
    if (path_begin + n_paths < path_begin) { set_error("path range overflows 64 bits"); return MCR_ERR_INVALID_ARG; }
    if (rng->kind == MCR_RNG_NUMPY) { set_error("spending rule: the NumPy stream is not supported (the engine's own stream only)"); return MCR_ERR_UNSUPPORTED; }
    if (rng->kind == MCR_RNG_HISTORY) { set_error("spending rule: the history stream is not supported (the engine's own stream only)"); return MCR_ERR_UNSUPPORTED; }
    if (out->trajectory || out->real_trajectory || out->withdrawal_rate_trajectory) {
        set_error("spending rule: trajectories are not supported (counters and per-path summary columns only)");
        return MCR_ERR_UNSUPPORTED;
    }
    if (out->hist_bins && out->hist_n_bins != 0) { set_error("spending rule: the in-kernel histogram (hist_bins) is not supported"); return MCR_ERR_UNSUPPORTED; }
    if (p->n_streams > MCR_INLINE_STREAMS && d.n_extra_streams > 0) {
        set_error("spending rule: %d income streams need the generic variant (at most %d are supported)", (int)p->n_streams, MCR_INLINE_STREAMS);
        return MCR_ERR_UNSUPPORTED;
    }
    if (needs_generic_variant(d)) { set_error("spending rule: the exact month (a realized-gains rate above 1 - 1e-6) needs the generic variant, which is not supported"); return MCR_ERR_UNSUPPORTED; }
    KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    io.out = *out;
    io.out.hist_bins = nullptr; io.out.hist_edges = nullptr; io.out.hist_n_bins = 0;
    if (io.out.path_stride <= 0) io.out.path_stride = (int64_t)n_paths;
    io.rule.upper = rule->upper; io.rule.lower = rule->lower; io.rule.keep = 1.0 - rule->cut; io.rule.grow = 1.0 + rule->raise;
    io.rule.floor = rule->floor; io.rule.ceiling = rule->ceiling;
    if (rule_out) {
        io.rule.year_counts = (unsigned long long*)rule_out->year_counts; io.rule.multipliers = rule_out->multipliers;
        io.rule.stride = rule_out->path_stride > 0 ? rule_out->path_stride : (int64_t)n_paths;
        if (io.rule.multipliers && (uint64_t)io.rule.stride < n_paths) {
            set_error("rule_out->path_stride %lld < n_paths %llu", (long long)io.rule.stride, (unsigned long long)n_paths);
            return MCR_ERR_INVALID_ARG;
        }
    }
    if (n_paths == 0) return MCR_OK;
    const bool want_summary = out->start_balance || out->final_balance || out->years_to_ruin || out->first_year_gross_withdrawal ||
                              out->first_year_real_gross_withdrawal || out->inflation_at_retirement || out->success;
    const int mode = want_summary ? 1 : 0;
    size_t lds = 0;
    rc = plan_path_kernel_lds(d, mode, MCR_RNG_PHILOX, false, false, 0, &lds);
    if (rc != MCR_OK) return rc;
    if (d.n_lock_slots < d.n_lock_slots_total) {
        set_error("spending rule: %d frozen income streams exceed the LDS budget and need the generic variant, which is not supported", (int)d.n_lock_slots_total);
        return MCR_ERR_UNSUPPORTED;
    }
    const dim3 grid((unsigned)((n_paths + kBlock - 1) / kBlock)), block(kBlock);
    const DevParams* const no_cand = nullptr;
    for_bool(d.any_annual_tax, [&](auto A) {
        for_bool(mode == 1, [&](auto S) {
            hipLaunchKernelGGL((path_kernel<decltype(S)::value ? 1 : 0, 0, 3, decltype(A)::value, false, 0, false, false, kExactMonthDefault, 0, 0, 0, false, false, 1, true>),
                               grid, block, lds, stream, d, io, no_cand);
        });
    });
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "path_kernel launch (spending rule)");
    return MCR_OK;
}

// Yearly bins (MODE 3 of path_kernel; mcr_run_year_bins_rng).  Checks of the arguments both entry points share: nothing is
// enqueued, and no table touched, unless they all pass.
static int check_year_bins(const mcr_outputs* out, const mcr_year_bins* yb) {
    if (!out || !yb) { set_error("null outputs / year bins"); return MCR_ERR_INVALID_ARG; }
    if (out->start_balance || out->final_balance || out->years_to_ruin || out->first_year_gross_withdrawal ||
        out->first_year_real_gross_withdrawal || out->inflation_at_retirement || out->success || out->trajectory ||
        out->real_trajectory || out->withdrawal_rate_trajectory) {
        set_error("year bins: `out` may carry counters, wr_obs_counts, ruin_year_bins and hist_* only (no per-path or trajectory output)");
        return MCR_ERR_INVALID_ARG;
    }
    if (yb->trajectory_bins || yb->real_trajectory_bins || yb->final_success_bins) {
        if (yb->n_bins < 1 || yb->n_bins > MCR_MAX_YEAR_BINS) { set_error("year bins: n_bins = %d (1..%d)", yb->n_bins, MCR_MAX_YEAR_BINS); return MCR_ERR_INVALID_ARG; }
        if (!yb->edges) { set_error("year bins: null edges under a requested table"); return MCR_ERR_INVALID_ARG; }
    }
    if (yb->wr_bins) {
        if (yb->n_wr_bins < 1 || yb->n_wr_bins > MCR_MAX_YEAR_BINS) { set_error("year bins: n_wr_bins = %d (1..%d)", yb->n_wr_bins, MCR_MAX_YEAR_BINS); return MCR_ERR_INVALID_ARG; }
        if (!yb->wr_edges) { set_error("year bins: null wr_edges under wr_bins"); return MCR_ERR_INVALID_ARG; }
    }
    if (out->hist_bins && out->hist_n_bins != 0 && (out->hist_n_bins < 0 || out->hist_n_bins > MCR_MAX_HIST_BINS || !out->hist_edges)) {
        set_error("hist_bins requested with hist_n_bins = %d (1..%d) / hist_edges = %p", out->hist_n_bins, MCR_MAX_HIST_BINS, (const void*)out->hist_edges);
        return MCR_ERR_INVALID_ARG;
    }
    return MCR_OK;
}
static int check_edges_host(const char* what, const double* e, int n) {   // np.histogram: "bins must increase monotonically"
    for (int k = 0; k <= n; ++k)
        if (!std::isfinite(e[k]) || (k > 0 && e[k] < e[k - 1])) { set_error("%s[%d] = %g: edges must be finite and ascending", what, k, e[k]); return MCR_ERR_INVALID_ARG; }
    return MCR_OK;
}
// The edge arrays of a yearly-bins request, where they are HOST pointers (`third`: hist_edges, or a rule's m_edges; null: not requested)
static bool wants_balance_tables(const mcr_year_bins* yb) { return yb->trajectory_bins || yb->real_trajectory_bins || yb->final_success_bins; }
static int check_year_bins_edges_host(const mcr_year_bins* yb, const char* third_name, const double* third, int n_third) {
    int rc;
    if (wants_balance_tables(yb) && (rc = check_edges_host("edges", yb->edges, yb->n_bins)) != MCR_OK) return rc;
    if (yb->wr_bins && (rc = check_edges_host("wr_edges", yb->wr_edges, yb->n_wr_bins)) != MCR_OK) return rc;
    return third ? check_edges_host(third_name, third, n_third) : MCR_OK;
}
// The kernel's view of a yearly-bins request: the edges and bin counts only of the tables that are asked for
static void fill_io_year_bins(KernelIO& io, const mcr_year_bins* yb) {
    const bool balance_tables = wants_balance_tables(yb);
    io.yb.edges = balance_tables ? yb->edges : nullptr;
    io.yb.n_bins = balance_tables ? yb->n_bins : 0;
    io.yb.wr_edges = yb->wr_bins ? yb->wr_edges : nullptr;
    io.yb.n_wr_bins = yb->wr_bins ? yb->n_wr_bins : 0;
    io.yb.trajectory = (unsigned long long*)yb->trajectory_bins;
    io.yb.real_trajectory = (unsigned long long*)yb->real_trajectory_bins;
    io.yb.wr = (unsigned long long*)yb->wr_bins;
    io.yb.final_success = (unsigned long long*)yb->final_success_bins;
}
// The launch: device pointers in `out` / `yb`.  Variants: the Philox stream per tax mask, the NumPy stream taxed / untaxed, and
// the generic (XS) form for stream lists beyond the by-value block, lock slots beyond the LDS budget and the exact month.
static int launch_year_bins(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                            int32_t wm, const mcr_outputs* out, const mcr_year_bins* yb, hipStream_t stream) {
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, wm, &d, &extra);
    if (rc != MCR_OK) return rc;
    if ((rc = check_rng(rng)) != MCR_OK) return rc;
    if ((rc = check_year_bins(out, yb)) != MCR_OK) return rc;
    if (n_paths == 0) return MCR_OK;
    if (n_paths > (uint64_t)INT32_MAX * kBlock) { set_error("n_paths too large for one launch"); return MCR_ERR_INVALID_ARG; }
    if (path_begin + n_paths < path_begin) { set_error("path range overflows 64 bits"); return MCR_ERR_INVALID_ARG; }
    KernelIO io = make_io(rng, rng->path_seeds, stream_id, path_begin, n_paths);
    io.out = *out;
    io.out.path_stride = (int64_t)n_paths;
    if (io.out.hist_bins == nullptr || io.out.hist_n_bins == 0) { io.out.hist_bins = nullptr; io.out.hist_edges = nullptr; io.out.hist_n_bins = 0; }
    fill_io_year_bins(io, yb);
    const uint32_t rng_kind = rng->kind;
    const dim3 grid((unsigned)((n_paths + kBlock - 1) / kBlock)), block(kBlock);
    size_t lds = 0;
    rc = plan_path_kernel_lds(d, 3, rng_kind, false, false, io.out.hist_n_bins, &lds, year_bins_lds(io.yb.n_bins, io.yb.n_wr_bins), rng->history_months);
    if (rc != MCR_OK) return rc;
    const bool exact = needs_exact_month(d);
    const bool xs = d.n_lock_slots < d.n_lock_slots_total || needs_generic_variant(d);
    StreamSideBlock side(stream);
    rc = side.attach(d, extra, grid.x);
    if (rc != MCR_OK) return rc;
    const DevParams* const no_cand = nullptr;
    for_whole_path_variant(d, kernel_rng_kind(rng), xs, exact, [&](auto R, auto T, auto A, auto X, auto EX) {
        hipLaunchKernelGGL((path_kernel<3, decltype(R)::value, decltype(T)::value, decltype(A)::value, false, 0, false, decltype(X)::value,
                                        (decltype(X)::value && decltype(EX)::value) || kExactMonthDefault>),
                           grid, block, lds, stream, d, io, no_cand);
    });
    const hipError_t e = hipGetLastError();
    const hipError_t ef = side.release();
    if (e != hipSuccess) return hip_fail(e, "path_kernel launch (yearly bins)");
    if (ef != hipSuccess) return hip_fail(ef, "path_kernel launch (yearly bins): side block release");
    return MCR_OK;
}

// Yearly bins under a spending rule (MODE 3 of path_kernel with RULE; mcr_run_rule_year_bins_rng): path_kernel<3, Philox, mask 3,
// annual-gains tax or not, ..., RULE>, two instantiations.  The checks need no device: check_year_bins' rules for `out` / `yb`,
// validate_spending_rule's for the rule, the multiplier table's own, and by name everything launch_rule refuses.  On success the
// parameter block and the launch's dynamic LDS are planned.
static int plan_rule_year_bins(const mcr_params* p, const mcr_rng* rng, uint64_t path_begin, uint64_t n_paths, int32_t wm,
                               const mcr_spending_rule* rule, const mcr_outputs* out, const mcr_year_bins* yb,
                               const mcr_rule_year_bins* rule_yb, DevParams* d_out, size_t* lds) {
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, wm, &d, &extra);
    if (rc != MCR_OK) return rc;
    if ((rc = check_rng(rng)) != MCR_OK) return rc;
    if ((rc = validate_spending_rule(rule)) != MCR_OK) return rc;
    if ((rc = check_year_bins(out, yb)) != MCR_OK) return rc;
    if (!rule_yb) { set_error("rule year bins: null rule_yb"); return MCR_ERR_INVALID_ARG; }
    if (rule_yb->multiplier_bins) {
        if (rule_yb->n_m_bins < 1 || rule_yb->n_m_bins > MCR_MAX_YEAR_BINS) {
            set_error("rule year bins: n_m_bins = %d (1..%d)", rule_yb->n_m_bins, MCR_MAX_YEAR_BINS);
            return MCR_ERR_INVALID_ARG;
        }
        if (!rule_yb->m_edges) { set_error("rule year bins: null m_edges under multiplier_bins"); return MCR_ERR_INVALID_ARG; }
    }
    if (n_paths > (uint64_t)INT32_MAX * kBlock) { set_error("n_paths too large for one launch"); return MCR_ERR_INVALID_ARG; }
    if (path_begin + n_paths < path_begin) { set_error("path range overflows 64 bits"); return MCR_ERR_INVALID_ARG; }
    if (rng->kind == MCR_RNG_NUMPY) { set_error("spending rule: the NumPy stream is not supported (the engine's own stream only)"); return MCR_ERR_UNSUPPORTED; }
    if (rng->kind == MCR_RNG_HISTORY) { set_error("spending rule: the history stream is not supported (the engine's own stream only)"); return MCR_ERR_UNSUPPORTED; }
    if (out->hist_bins && out->hist_n_bins != 0) { set_error("spending rule: the in-kernel histogram (hist_bins) is not supported"); return MCR_ERR_UNSUPPORTED; }
    if (p->n_streams > MCR_INLINE_STREAMS && d.n_extra_streams > 0) {
        set_error("spending rule: %d income streams need the generic variant (at most %d are supported)", (int)p->n_streams, MCR_INLINE_STREAMS);
        return MCR_ERR_UNSUPPORTED;
    }
    if (needs_generic_variant(d)) { set_error("spending rule: the exact month (a realized-gains rate above 1 - 1e-6) needs the generic variant, which is not supported"); return MCR_ERR_UNSUPPORTED; }
    const bool balance_tables = yb->trajectory_bins || yb->real_trajectory_bins || yb->final_success_bins;
    const int n_m = rule_yb->multiplier_bins ? rule_yb->n_m_bins : 0;
    // the multiplier segment: its edges as doubles and a cell in each row buffer, 8 + 2 x 4 = 16 bytes per bin like a withdrawal-rate bin
    const size_t m_bytes = ((size_t)n_m + 1) * sizeof(double) + 2 * ((size_t)n_m + 2) * sizeof(unsigned int);
    rc = plan_path_kernel_lds(d, 3, MCR_RNG_PHILOX, false, false, 0, lds,
                              year_bins_lds(balance_tables ? yb->n_bins : 0, yb->wr_bins ? yb->n_wr_bins : 0) + m_bytes);
    if (rc != MCR_OK) return rc;
    if (d.n_lock_slots < d.n_lock_slots_total) {
        set_error("spending rule: %d frozen income streams exceed the LDS budget and need the generic variant, which is not supported", (int)d.n_lock_slots_total);
        return MCR_ERR_UNSUPPORTED;
    }
    *d_out = d;
    return MCR_OK;
}
// The launch: device pointers in `out` / `yb` / `rule_yb`.  The rule and the rule's tables travel in ONE device record behind
// path_kernel's third argument (RuleBinsRecord; a stream-ordered allocation released behind the launch, like a fan-out's table):
// KernelIO keeps its size and every field its place.
static int launch_rule_year_bins(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                 int32_t wm, const mcr_spending_rule* rule, const mcr_outputs* out, const mcr_year_bins* yb,
                                 const mcr_rule_year_bins* rule_yb, hipStream_t stream) {
    DevParams d;
    size_t lds = 0;
    int rc = plan_rule_year_bins(p, rng, path_begin, n_paths, wm, rule, out, yb, rule_yb, &d, &lds);
    if (rc != MCR_OK) return rc;
    if (n_paths == 0) return MCR_OK;
    KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    io.out = *out;
    io.out.path_stride = (int64_t)n_paths;
    io.out.hist_bins = nullptr; io.out.hist_edges = nullptr; io.out.hist_n_bins = 0;
    fill_io_year_bins(io, yb);
    RuleBinsRecord host = {rule->upper, rule->lower, 1.0 - rule->cut, 1.0 + rule->raise, rule->floor, rule->ceiling,
                           (unsigned long long*)rule_yb->year_counts, (unsigned long long*)rule_yb->multiplier_bins,
                           rule_yb->multiplier_bins ? rule_yb->m_edges : nullptr, rule_yb->multiplier_bins ? rule_yb->n_m_bins : 0, 0};
    StreamAlloc record(stream);
    if (!record.alloc(sizeof(host))) { set_error("rule year bins: the device record's allocation was refused"); return MCR_ERR_HIP; }
    hipError_t e = hipMemcpyAsync(record.p, &host, sizeof(host), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((n_paths + kBlock - 1) / kBlock)), block(kBlock);
        for_bool(d.any_annual_tax, [&](auto A) {
            hipLaunchKernelGGL((path_kernel<3, 0, 3, decltype(A)::value, false, 0, false, false, kExactMonthDefault, 0, 0, 0, false, false, 1, true>),
                               grid, block, lds, stream, d, io, (const DevParams*)record.p);
        });
        e = hipGetLastError();
    }
    const hipError_t ef = record.release();
    if (e != hipSuccess) return hip_fail(e, "path_kernel launch (rule yearly bins)");
    if (ef != hipSuccess) return hip_fail(ef, "path_kernel launch (rule yearly bins): record release");
    return MCR_OK;
}

// ---------------------------------------------------------------------------------------------
// Search probes: several candidates (months, spending or contribution levels, or a grid of both) over the same paths
// ---------------------------------------------------------------------------------------------
// The route every probe can fall back to: one count-only launch per candidate, launch(k, side stream) for k in [0, n), on the
// side streams of a leased StreamFork; the caller's stream waits for all of them.  Returns the first error.
template <typename Launch>
static int fork_join(int device, hipStream_t main, int n, Launch&& launch) {
    StreamForkPool::Lease fork_lease(g_stream_fork, device);
    StreamFork* f = fork_lease.p;
    if (!f) { set_error("could not create probe streams"); return MCR_ERR_HIP; }
    const int used = n < kForkStreams ? n : kForkStreams;
    hipError_t e;
    if ((e = hipEventRecord(f->fork, main)) != hipSuccess) return hip_fail(e, "probe fork");
    for (int i = 0; i < used; ++i)
        if ((e = hipStreamWaitEvent(f->side[i], f->fork, 0)) != hipSuccess) return hip_fail(e, "probe fork wait");
    int first_rc = MCR_OK;
    for (int k = 0; k < n && first_rc == MCR_OK; ++k) first_rc = launch(k, f->side[k % used]);
    // always join, also after a failed launch: `main` must not run ahead of work already forked
    for (int i = 0; i < used; ++i) {
        if ((e = hipEventRecord(f->done[i], f->side[i])) != hipSuccess) return hip_fail(e, "probe join record");
        if ((e = hipStreamWaitEvent(main, f->done[i], 0)) != hipSuccess) return hip_fail(e, "probe join wait");
    }
    return first_rc;
}
// Probes validate every candidate BEFORE enqueueing anything, so a bad one leaves no half-forked work behind and `counts` untouched
static int validate_months(const mcr_params* p, const int32_t* working_months, int32_t n) {
    for (int32_t c = 0; c < n; ++c) {
        DevParams d;
        const int rc = derive_params(p, working_months[c], &d);
        if (rc != MCR_OK) return rc;
    }
    return MCR_OK;
}
static int zero_counters(uint64_t* counts, size_t n_blocks, hipStream_t stream) {
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(uint64_t) * MCR_N_COUNTERS * n_blocks, stream);
    return e == hipSuccess ? MCR_OK : hip_fail(e, "probe counters memset");
}

// Ascending order of a probe's candidate months (stable): order[i] = index into `months` of the i-th smallest
static void sort_candidates(const int32_t* months, int n, int* order) {
    for (int i = 0; i < n; ++i) {
        int k = i;
        while (k > 0 && months[order[k - 1]] > months[i]) { order[k] = order[k - 1]; --k; }
        order[k] = i;
    }
}
// The device memory of a shared-accumulation probe: ONE stream-ordered allocation of n_snap snapshot columns (io.snap, the
// paths padded to whole wavefronts) followed by the launch's parameter records, uploaded from the host.
constexpr size_t kSnapshotCapBytes = (size_t)4 << 30;   // huge probes are throughput-bound anyway: they take the plain route
struct SnapshotBlock {
    StreamAlloc mem;
    const void* records = nullptr;
    explicit SnapshotBlock(hipStream_t s) : mem(s) {}
    // false: snapshots above `cap`, or the allocation was refused (nothing enqueued); otherwise *upload is the copy's status
    bool attach(KernelIO& io, int n_snap, const void* host_records, size_t records_bytes, hipError_t* upload, size_t cap = kSnapshotCapBytes) {
        io.n_snap = n_snap;
        io.snap_stride = (int64_t)((io.n_paths + 63) / 64 * 64);
        const size_t snap_bytes = (size_t)n_snap * kSnapFields * (size_t)io.snap_stride * sizeof(double);
        if (snap_bytes > cap || !mem.alloc(snap_bytes + records_bytes)) return false;
        io.snap = (double*)mem.p;
        records = (char*)mem.p + snap_bytes;
        *upload = records_bytes ? hipMemcpyAsync((char*)mem.p + snap_bytes, host_records, records_bytes, hipMemcpyHostToDevice, mem.stream) : hipSuccess;
        return true;
    }
};
// The accumulation sweep of a shared-accumulation probe (PHASE 1: stores the state at the end of every io.snap_months[c]); it
// takes the producer / consumer split on its own while its launch leaves SIMDs idle
static void launch_accumulation(const DevParams& d, const KernelIO& io, const DevParams* cand, size_t lds, hipStream_t stream) {
    const dim3 g1((unsigned)((io.n_paths + kBlock - 1) / kBlock));
    const bool split1 = (uint64_t)g1.x * (kBlock / 64) <= split_max_waves();
    for_tax_variant(d, [&](auto T, auto A) {
        constexpr int t = decltype(T)::value;
        constexpr bool a = decltype(A)::value;
        if (split1) hipLaunchKernelGGL((path_kernel<0, 0, t, a, false, 1, true>), g1, dim3(2 * kBlock), lds, stream, d, io, cand);
        else hipLaunchKernelGGL((path_kernel<0, 0, t, a, false, 1>), g1, dim3(kBlock), lds, stream, d, io, cand);
    });
}

// Several candidates over the same paths, Philox stream: ONE accumulation sweep to the largest candidate that stores the
// state at the end of every candidate month (PHASE 1), then ONE launch whose grid.y is the candidate and which resumes
// every decumulation from its snapshot (PHASE 2).  The candidates' parameter blocks (stream start months, horizon) go to
// device memory; snapshots and blocks are stream-ordered allocations.  Counts are identical to one launch per candidate.
static int probe_shared_prefix(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                               const int32_t* working_months, int32_t n_cand, uint64_t* counts, hipStream_t stream) {
    if (n_cand < 2 || n_paths == 0 || n_paths > ((uint64_t)1 << 31)) return MCR_ERR_UNSUPPORTED;
    int order[MCR_MAX_PROBE_CANDIDATES];
    sort_candidates(working_months, n_cand, order);
    for (int i = 1; i < n_cand; ++i)
        if (working_months[order[i]] == working_months[order[i - 1]]) return MCR_ERR_UNSUPPORTED;   // duplicates: plain route
    std::vector<DevParams> blocks((size_t)n_cand);
    for (int i = 0; i < n_cand; ++i) {
        const int rc = derive_params(p, working_months[order[i]], &blocks[(size_t)i]);
        if (rc != MCR_OK) return rc;
    }
    DevParams& top = blocks[(size_t)n_cand - 1];
    // (stream lists beyond the by-value block, or lock slots beyond the LDS of the split form, take one launch per candidate:
    //  each then carries its own device table / overflow block)
    if (needs_generic_variant(top)) return MCR_ERR_UNSUPPORTED;
    size_t lds = 0;
    if (plan_path_kernel_lds(top, 0, MCR_RNG_PHILOX, false, true, 0, &lds) != MCR_OK || top.n_lock_slots < top.n_lock_slots_total) return MCR_ERR_UNSUPPORTED;
    for (DevParams& b : blocks) b.n_lock_slots = top.n_lock_slots;
    KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    io.out.counters = counts;
    for (int i = 0; i < n_cand; ++i) { io.snap_months[i] = working_months[order[i]]; io.cand_out[i] = order[i]; }
    SnapshotBlock snap(stream);
    hipError_t e = hipSuccess;
    if (!snap.attach(io, n_cand, blocks.data(), (size_t)n_cand * sizeof(DevParams), &e)) return MCR_ERR_UNSUPPORTED;
    const DevParams* d_blocks = (const DevParams*)snap.records;
    if (e == hipSuccess) {
        if (int rc = check_barrier_counts(top)) return rc;
        // (the decumulation launch takes the producer / consumer split on its own, like the sweep)
        const dim3 g2((unsigned)((n_paths + kBlock - 1) / kBlock), (unsigned)n_cand);
        const bool split2 = (uint64_t)g2.x * g2.y * (kBlock / 64) <= split_max_waves();
        // the candidates' decumulations time-sliced (PHASE 4) where their workgroups are a few rounds of the resident slots
        // with a mostly empty last one: the search's 17-month verification window at 50 000 paths is 3 332 workgroups = 2.17 rounds
        SegmentPlan plan;
        SegmentHandOver hand(stream);
        bool sliced = false;
        const char* seg_order = segment_order_env();
        int seg_perm[kMaxSegments];
        if (!split2 && plan_segments(top, g2.x * g2.y, 0, &plan, true)) {
            if (seg_order)
                if (int rc = parse_segment_order(seg_order, plan.q, seg_perm)) return rc;
            hipError_t ez = hipSuccess;
            sliced = hand.attach(io, plan, seg_fixed_fields(0) + top.n_lock_slots, &ez) && ez == hipSuccess;
            if (sliced) io.seg_blocks_per_cand = (int32_t)g2.x;
            else { (void)hipGetLastError(); (void)hand.release(); }   // (refused: the un-sliced launch)
        }
        if (seg_order && !sliced) {
            set_error("MCR_K1_SEGMENT_ORDER=%s set on a shared-prefix probe whose decumulation launch is not time-sliced", seg_order);
            return MCR_ERR_INVALID_ARG;
        }
        launch_accumulation(top, io, d_blocks, lds, stream);
        for_tax_variant(top, [&](auto T, auto A) {
            constexpr int t = decltype(T)::value;
            constexpr bool a = decltype(A)::value;
            if (split2) hipLaunchKernelGGL((path_kernel<0, 0, t, a, false, 2, true>), g2, dim3(2 * kBlock), lds, stream, top, io, d_blocks);
            else if (sliced) launch_sliced(&path_kernel<0, 0, t, a, false, 4>, plan, seg_order ? seg_perm : nullptr, dim3(kBlock), lds, stream, top, io, d_blocks);
            else hipLaunchKernelGGL((path_kernel<0, 0, t, a, false, 2>), g2, dim3(kBlock), lds, stream, top, io, d_blocks);
        });
        e = hipGetLastError();
        (void)hand.release();
    }
    const hipError_t ef = snap.mem.release();
    if (e != hipSuccess) return hip_fail(e, "shared-prefix probe");
    if (ef != hipSuccess) return hip_fail(ef, "shared-prefix probe (free)");
    return MCR_OK;
}

// LDS of a level fan-out launch (path_kernel PHASE 5 / 6 / 7 / 8): STATIC = the math tables and the double-buffered 64-column stage
// (+ the unused summary / segment words); DYNAMIC = the level counters and [n_lock_slots][64] lock columns per consumer wave.
// Every lock slot stays in LDS (no overflow block in this form): the levels per launch are lowered until they fit.
// `parts`: PHASE 9, whose stage holds the nine parts of a pair's normals per lane instead of six factors (+3 072 B).
static size_t fanout_static_lds(bool parts = false) {   // (16 640 B compiled; PHASE 9: 19 712 B)
    return (size_t)kMathTabBytes + (size_t)2 * (parts ? kPartsPerPair : 6) * 64 * sizeof(double) + 512;
}
static size_t fanout_dynamic_lds(const DevParams& d, int levels) {
    return (size_t)MCR_MAX_EXPENSE_FANOUT * sizeof(unsigned int) + (size_t)levels * (size_t)d.n_lock_slots_total * 64 * sizeof(double);
}
static int fanout_max_levels(const DevParams& d, bool parts = false) {
    int l = MCR_MAX_EXPENSE_FANOUT;
    while (l > 0 && fanout_static_lds(parts) + fanout_dynamic_lds(d, l) > kLdsPerWorkgroup) --l;
    return l;
}
// Below this many path-wavefronts per level (n_paths / 64) the per-level route runs instead of a fan-out: the environment
// variable overrides it (0 = always fan out where the shape allows; a huge value = never).
static uint64_t fanout_min_waves(const char* env_name = "MCR_EXPENSE_FANOUT_MIN_WAVES") {
    const char* e = std::getenv(env_name);
    return (e && *e) ? (uint64_t)std::strtoull(e, nullptr, 10) : 0u;
}
// Fan-out launches take n_levels in groups of near-equal size, none above lmax: f(g, first, lg) for group g = levels [first, first + lg)
struct LevelGroups {
    int n_levels, n_groups;
    LevelGroups(int n_levels, int lmax) : n_levels(n_levels), n_groups((n_levels + lmax - 1) / lmax) {}
    template <typename F> void for_each(F&& f) const {
        for (int g = 0, first = 0; g < n_groups; ++g) {
            const int lg = n_levels / n_groups + (g < n_levels % n_groups ? 1 : 0);
            f(g, first, lg);
            first += lg;
        }
    }
};
// What the expense and the contribution fan-out ask of a probe's shape.  MCR_OK: *d = the parameter block with every lock slot
// in LDS, *lmax = levels per launch; MCR_ERR_UNSUPPORTED for shapes the form does not cover.
static int plan_level_fanout(const mcr_params* p, const mcr_rng* rng, uint64_t n_paths, int32_t wm, int32_t n_levels, uint64_t min_waves,
                             DevParams* d, int* lmax, bool parts = false /* PHASE 9's larger stage */,
                             int keep_index = -1, std::vector<std::pair<int, int>>* kept = nullptr /* PHASE 10: derive_params' */,
                             int min_levels = 2 /* PHASE 13: 1, the family has no plain launch for a single option */) {
    if (rng->kind != MCR_RNG_PHILOX || n_levels < min_levels || n_paths == 0 || n_paths > ((uint64_t)1 << 31)) return MCR_ERR_UNSUPPORTED;
    if ((n_paths + 63) / 64 < min_waves) return MCR_ERR_UNSUPPORTED;
    int rc = derive_params(p, wm, d, nullptr, kept, keep_index);
    if (rc != MCR_OK) return rc;
    if (needs_generic_variant(*d)) return MCR_ERR_UNSUPPORTED;
    if ((rc = check_barrier_counts(*d)) != MCR_OK) return rc;
    *lmax = fanout_max_levels(*d, parts);
    if (*lmax < 2) return MCR_ERR_UNSUPPORTED;
    d->n_lock_slots = d->n_lock_slots_total;
    return MCR_OK;
}
// The fan-out launches of a level probe: consumer wave j of a group's launch runs level first + j and counts into its block.
// PHASE 5: spending levels, resumed from the snapshot; PHASE 7: contribution levels, from month 0.
template <int PHASE>
static void launch_level_fanout(const DevParams& d, const KernelIO& io, const double* levels, const LevelGroups& groups, uint64_t* counts,
                                hipStream_t stream) {
    const dim3 grid((unsigned)((io.n_paths + 63) / 64));
    for_tax_variant(d, [&](auto T, auto A) {
        groups.for_each([&](int, int first, int lg) {
            KernelIO fio = io;
            fio.out.counters = counts + (size_t)first * MCR_N_COUNTERS;
            fio.fan_n = lg;
            for (int k = 0; k < lg; ++k) fio.fan_expenses[k] = levels[first + k];
            hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, PHASE, true>), grid, dim3(64 * (lg + 1)),
                               fanout_dynamic_lds(d, lg), stream, d, fio, (const DevParams*)nullptr);
        });
    });
}

// Several spending levels over the same paths, Philox stream: ONE accumulation sweep to working_months (PHASE 1, one
// snapshot), then expense fan-out launches (PHASE 5) over groups of at most MCR_MAX_EXPENSE_FANOUT levels.  Returns
// MCR_ERR_UNSUPPORTED, having enqueued nothing, for shapes this form does not cover.
static int probe_expenses_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                 int32_t wm, const double* levels, int32_t n_levels, uint64_t* counts, hipStream_t stream) {
    DevParams d;
    int lmax = 0;
    if (int rc = plan_level_fanout(p, rng, n_paths, wm, n_levels, fanout_min_waves(), &d, &lmax)) return rc;
    DevParams d1 = d;    // (PHASE 1 never reads a lock column: its plan may lower the LDS slots)
    size_t lds1 = 0;
    if (plan_path_kernel_lds(d1, 0, MCR_RNG_PHILOX, false, true, 0, &lds1) != MCR_OK) { (void)hipGetLastError(); return MCR_ERR_UNSUPPORTED; }
    KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    io.snap_months[0] = wm;
    SnapshotBlock snap(stream);
    hipError_t e = hipSuccess;
    if (!snap.attach(io, 1, nullptr, 0, &e, SIZE_MAX)) return MCR_ERR_UNSUPPORTED;   // (one column: no cap, the allocator decides)
    launch_accumulation(d1, io, nullptr, lds1, stream);
    launch_level_fanout<5>(d, io, levels, LevelGroups(n_levels, lmax), counts, stream);
    e = hipGetLastError();
    const hipError_t ef = snap.mem.release();
    if (e != hipSuccess) return hip_fail(e, "expense fan-out probe");
    if (ef != hipSuccess) return hip_fail(ef, "expense fan-out probe (free)");
    return MCR_OK;
}

// Several contribution levels over the same paths, Philox stream: contribution fan-out launches (PHASE 7) over groups of at
// most fanout_max_levels levels.  The levels differ from month 0, so there is no accumulation sweep and no snapshot: each
// launch runs the whole path.  Returns MCR_ERR_UNSUPPORTED, having enqueued nothing, for shapes this form does not cover.
static int probe_contributions_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                      uint64_t n_paths, int32_t wm, const double* levels, int32_t n_levels, uint64_t* counts,
                                      hipStream_t stream) {
    DevParams d;
    int lmax = 0;
    if (int rc = plan_level_fanout(p, rng, n_paths, wm, n_levels, fanout_min_waves("MCR_CONTRIBUTION_FANOUT_MIN_WAVES"), &d, &lmax)) return rc;
    const KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    launch_level_fanout<7>(d, io, levels, LevelGroups(n_levels, lmax), counts, stream);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "contribution fan-out probe");
    return MCR_OK;
}

// Outcome probes (mcr_probe_*_outcomes_rng): a fan-out launch over options [first, first + lg) gets the rows at option `first`
static void set_fan_rows(KernelIO& fio, const mcr_option_outcomes* rows, int first) {
    if (!rows) return;
    fio.fan_rows.row_stride = rows->path_stride;
    fio.fan_rows.final_balance = rows->final_balance ? rows->final_balance + (size_t)first * (size_t)rows->path_stride : nullptr;
    fio.fan_rows.years_to_ruin = rows->years_to_ruin ? rows->years_to_ruin + (size_t)first * (size_t)rows->path_stride : nullptr;
}

// The record fan-outs (PHASE 8 .. 11: scenarios, assumptions, income options, spending rules) share this skeleton: fan-out
// launches over groups of at most `lmax` records, the whole path each, like the contribution fan-out.  The records (`host`, as
// the kernel reads them) go to ONE stream-ordered device table (SnapshotBlock's records, no snapshot column), filled with one
// async copy and released behind the launches; group g's launch gets the table at its first record through `cand_params`, its
// counters, masks and rows at that record, and whatever `launch(fio, first, grid, block, lds, table)` adds before it launches
// the family's kernel.  One parameter block `d` (plan_level_fanout's) serves every record: each family says below why.
// `launches`, where given, counts the launches and is reset when they report an error; `what` names the probe in HIP errors.
// Returns MCR_ERR_UNSUPPORTED, having enqueued nothing, when the table's allocation is refused.
template <typename Record, typename Launch>
static int launch_record_fanout(const DevParams& d, int lmax, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                const Record* host, int32_t n_records, uint64_t* counts, hipStream_t stream, uint64_t* masks,
                                const mcr_option_outcomes* rows, int* launches, const char* what, Launch&& launch,
                                size_t tail_bytes = 0 /* PHASE 13: what `host` holds behind its records (the weights), uploaded with them */) {
    KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    SnapshotBlock table(stream);
    hipError_t e = hipSuccess;
    if (!table.attach(io, 0, host, (size_t)n_records * sizeof(Record) + tail_bytes, &e, SIZE_MAX)) return MCR_ERR_UNSUPPORTED;
    io.snap = nullptr;   // (no snapshot column: the block is the table alone)
    if (e == hipSuccess) {
        const Record* d_table = (const Record*)table.records;
        const dim3 grid((unsigned)((n_paths + 63) / 64));
        LevelGroups(n_records, lmax).for_each([&](int, int first, int lg) {
            KernelIO fio = io;
            fio.out.counters = counts + (size_t)first * MCR_N_COUNTERS;
            fio.fan_n = lg;
            fio.fan_masks = masks ? masks + (size_t)first * ((n_paths + 63) / 64) : nullptr;
            set_fan_rows(fio, rows, first);
            launch(fio, first, grid, dim3(64 * (lg + 1)), fanout_dynamic_lds(d, lg), (const DevParams*)(d_table + first));
            if (launches) ++*launches;
        });
        e = hipGetLastError();
    }
    const hipError_t ef = table.mem.release();
    if (e != hipSuccess && launches) *launches = 0;
    if (e != hipSuccess) return hip_fail(e, what);
    if (ef != hipSuccess) return hip_fail(ef, (std::string(what) + " (free)").c_str());
    return MCR_OK;
}

// Several (initial_balance, monthly_contribution, monthly_expenses) records over the same paths, Philox stream (PHASE 8).  The
// records are the table as they come.  Nothing derive_params, the lock-slot plan or the tax variant reads depends on the three
// fields (they are copied through).  Returns MCR_ERR_UNSUPPORTED, having enqueued nothing, for shapes this form does not cover.
static int probe_scenarios_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                  int32_t wm, const mcr_scenario* scenarios, int32_t n_scenarios, uint64_t* counts, hipStream_t stream,
                                  uint64_t* masks = nullptr /* joint probes: KernelIO::fan_masks of the whole option list */,
                                  const mcr_option_outcomes* rows = nullptr /* outcome probes: the rows of the whole option list */) {
    DevParams d;
    int lmax = 0;
    if (int rc = plan_level_fanout(p, rng, n_paths, wm, n_scenarios, fanout_min_waves("MCR_SCENARIO_FANOUT_MIN_WAVES"), &d, &lmax)) return rc;
    return launch_record_fanout(d, lmax, rng, stream_id, path_begin, n_paths, scenarios, n_scenarios, counts, stream, masks, rows, nullptr,
                                "scenario fan-out probe", [&](const KernelIO& fio, int, dim3 grid, dim3 block, size_t lds, const DevParams* table) {
        for_tax_variant(d, [&](auto T, auto A) {
            for_bool(rows != nullptr, [&](auto O) {
                hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, 8, true, false, kExactMonthDefault, 0, 0, 0, decltype(O)::value>),
                                   grid, block, lds, stream, d, fio, table);
            });
        });
    });
}

// Several records of (initial_balance, monthly_contribution, monthly_expenses, the market's seven lognormal parameters) over the
// same paths, Philox stream (PHASE 9, groups of at most fanout_max_levels(parts) records).  The records are derived on the host
// (derive_market: the bits derive_params gives a block with those seven fields).  Of everything the host derives from the
// parameter block only a1 .. binf_rho_c, rho and rho_c depend on the seven fields, and the kernel reads them in growth_rows2
// alone — which PHASE 9's consumers replace by their record's; the tax variant, needs_generic_variant, the lock-slot plan, the
// kept streams and the barrier counts read none of the ten fields.  Returns MCR_ERR_UNSUPPORTED, having enqueued nothing, for
// shapes this form does not cover.
static thread_local int g_last_assumption_fanout_launches = 0;   // (mcr_probe_assumptions_last_fanout_launches)
static int probe_assumptions_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                    int32_t wm, const mcr_assumptions* records, int32_t n_records, uint64_t* counts, hipStream_t stream,
                                  uint64_t* masks = nullptr /* joint probes: KernelIO::fan_masks of the whole option list */,
                                  const mcr_option_outcomes* rows = nullptr /* outcome probes: the rows of the whole option list */) {
    DevParams d;
    int lmax = 0;
    if (int rc = plan_level_fanout(p, rng, n_paths, wm, n_records, fanout_min_waves("MCR_ASSUMPTION_FANOUT_MIN_WAVES"), &d, &lmax, true)) return rc;
    std::vector<AssumptionRecord> host((size_t)n_records);
    for (int32_t k = 0; k < n_records; ++k) {
        const mcr_assumptions& r = records[k];
        const DevMarket mk = derive_market(r.inv1_mu_log, r.inv1_sigma_log, r.inf_mu_log, r.inf_sigma_log, r.prem_mu_log, r.prem_sigma_log,
                                           r.equity_inflation_rho);
        host[(size_t)k] = AssumptionRecord{r.initial_balance, r.monthly_contribution, r.monthly_expenses,
                                           mk.a1, mk.b1, mk.ainf, mk.binf_rho, mk.binf_rho_c, mk.aprem, mk.bprem};
    }
    return launch_record_fanout(d, lmax, rng, stream_id, path_begin, n_paths, host.data(), n_records, counts, stream, masks, rows,
                                &g_last_assumption_fanout_launches, "assumption fan-out probe",
                                [&](const KernelIO& fio, int, dim3 grid, dim3 block, size_t lds, const DevParams* table) {
        for_tax_variant(d, [&](auto T, auto A) {
            for_bool(rows != nullptr, [&](auto O) {
                hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, 9, true, false, kExactMonthDefault, 0, 0, 0, decltype(O)::value>),
                                   grid, block, lds, stream, d, fio, table);
            });
        });
    });
}

// Several versions of ONE income stream (and of the scenario fan-out's three fields) over the same paths, Philox stream (PHASE
// 10).  The records are derived on the host (derive_stream: the bits derive_params gives a block whose stream has those fields).
// The parameter block is derived with the probed stream KEPT whatever its own amount (derive_params' keep_index), so the kernel
// has a record to replace at the stream's list position and, for a frozen stream, a lock column per consumer wave; the stream's
// keep, indexed and lock_slot are the list's own for every record, and nothing else derive_params, the lock-slot plan or the tax
// variant reads depends on the six fields.  Returns MCR_ERR_UNSUPPORTED, having enqueued nothing, for shapes this form does not
// cover.
static thread_local int g_last_income_fanout_launches = 0;   // (mcr_probe_income_last_fanout_launches)
static int probe_income_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                               int32_t wm, int32_t stream_index, const mcr_income_option* options, int32_t n_options, uint64_t* counts,
                               hipStream_t stream, uint64_t* masks = nullptr /* joint probes: KernelIO::fan_masks of the whole option list */,
                               const mcr_option_outcomes* rows = nullptr /* outcome probes: the rows of the whole option list */) {
    DevParams d;
    int lmax = 0;
    std::vector<std::pair<int, int>> kept;
    if (int rc = plan_level_fanout(p, rng, n_paths, wm, n_options, fanout_min_waves("MCR_INCOME_FANOUT_MIN_WAVES"), &d, &lmax, false,
                                   stream_index, &kept)) return rc;
    int kept_k = -1;   // the probed stream's position among the kept records (all of them in the by-value block here)
    for (size_t i = 0; i < kept.size(); ++i) if (kept[i].first == stream_index) kept_k = (int)i;
    if (kept_k < 0 || kept_k >= d.n_streams) return MCR_ERR_UNSUPPORTED;
    const mcr_stream& own = stream_at(p, stream_index);
    std::vector<IncomeRecord> host((size_t)n_options);
    for (int32_t k = 0; k < n_options; ++k) {
        const mcr_income_option& r = options[k];
        const DevStreamWindow w = derive_stream(p->current_age, wm, r.monthly_amount_today, own.tax_rate, r.start_at_age, r.duration_years);
        host[(size_t)k] = IncomeRecord{r.initial_balance, r.monthly_contribution, r.monthly_expenses, w.amount, w.amount_keep, w.start_month, w.end_month};
    }
    return launch_record_fanout(d, lmax, rng, stream_id, path_begin, n_paths, host.data(), n_options, counts, stream, masks, rows,
                                &g_last_income_fanout_launches, "income fan-out probe",
                                [&](KernelIO& fio, int, dim3 grid, dim3 block, size_t lds, const DevParams* table) {
        fio.fan_stream = kept_k;
        for_tax_variant(d, [&](auto T, auto A) {
            for_bool(rows != nullptr, [&](auto O) {
                hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, 10, true, false, kExactMonthDefault, 0, 0, 0, decltype(O)::value>),
                                   grid, block, lds, stream, d, fio, table);
            });
        });
    });
}

// Several (initial_balance, monthly_contribution, monthly_expenses, spending rule) options over the same paths, Philox stream
// (PHASE 11).  The records are made on the host (keep = 1 - cut, grow = 1 + raise: launch_rule's two operations).  The kernels
// are the generic tax mask's (TAXED = 3), like the plain rule launch's: a zero-rate asset's arithmetic is exact zeros there.
// Group g's launch counts the years of its options into year_counts at its first option.  Returns MCR_ERR_UNSUPPORTED, having
// enqueued nothing, for shapes this form does not cover.
static thread_local int g_last_rule_fanout_launches = 0;   // (mcr_probe_rules_last_fanout_launches)
static int probe_rules_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                              int32_t wm, const mcr_rule_option* options, int32_t n_options, uint64_t* counts, uint64_t* year_counts,
                              hipStream_t stream, uint64_t* masks = nullptr /* joint probes: KernelIO::fan_masks of the whole option list */,
                              const mcr_option_outcomes* rows = nullptr /* outcome probes: the rows of the whole option list */) {
    DevParams d;
    int lmax = 0;
    if (int rc = plan_level_fanout(p, rng, n_paths, wm, n_options, fanout_min_waves("MCR_RULE_FANOUT_MIN_WAVES"), &d, &lmax)) return rc;
    std::vector<RuleRecord> host((size_t)n_options);
    for (int32_t k = 0; k < n_options; ++k) {
        const mcr_rule_option& r = options[k];
        host[(size_t)k] = RuleRecord{r.initial_balance, r.monthly_contribution, r.monthly_expenses,
                                     r.rule.upper, r.rule.lower, 1.0 - r.rule.cut, 1.0 + r.rule.raise, r.rule.floor, r.rule.ceiling};
    }
    return launch_record_fanout(d, lmax, rng, stream_id, path_begin, n_paths, host.data(), n_options, counts, stream, masks, rows,
                                &g_last_rule_fanout_launches, "rule fan-out probe",
                                [&](KernelIO& fio, int first, dim3 grid, dim3 block, size_t lds, const DevParams* table) {
        // (fan_rule.rows are fan_rows' bytes, which the skeleton has set; the rest of the block is make_io's zeros)
        fio.fan_rule.year_counts = year_counts ? (unsigned long long*)year_counts + (size_t)first * (size_t)d.retirement_years * MCR_RULE_N_COUNTS : nullptr;
        for_bool(d.any_annual_tax, [&](auto A) {
            for_bool(rows != nullptr, [&](auto O) {
                hipLaunchKernelGGL((path_kernel<0, 0, 3, decltype(A)::value, false, 11, true, false, kExactMonthDefault, 0, 0, 0, decltype(O)::value, false, 1, true>),
                                   grid, block, lds, stream, d, fio, table);
            });
        });
    });
}

// Several (initial_balance, monthly_contribution, monthly_expenses, allocation_inv1_pct) options over the same paths, Philox
// stream (PHASE 12).  The records are the table as they come.  Of everything derive_params gives the block only alloc1 / alloc2
// depend on the fourth field, and the consumers read their record's in every place the path reads them (the initial split, the
// contribution split, the rebalances, the dust sub-case, lane_params_tol's two products); the tax variant, needs_generic_variant,
// the lock-slot plan, the kept streams and the barrier counts read neither.  Returns MCR_ERR_UNSUPPORTED, having enqueued
// nothing, for shapes this form does not cover.
static thread_local int g_last_allocation_fanout_launches = 0;   // (mcr_probe_allocations_last_fanout_launches)
static int probe_allocations_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                    int32_t wm, const mcr_allocation_option* options, int32_t n_options, uint64_t* counts, hipStream_t stream,
                                    uint64_t* masks = nullptr /* joint probes: KernelIO::fan_masks of the whole option list */,
                                    const mcr_option_outcomes* rows = nullptr /* outcome probes: the rows of the whole option list */) {
    DevParams d;
    int lmax = 0;
    if (int rc = plan_level_fanout(p, rng, n_paths, wm, n_options, fanout_min_waves("MCR_ALLOCATION_FANOUT_MIN_WAVES"), &d, &lmax)) return rc;
    return launch_record_fanout(d, lmax, rng, stream_id, path_begin, n_paths, options, n_options, counts, stream, masks, rows,
                                &g_last_allocation_fanout_launches, "allocation fan-out probe",
                                [&](const KernelIO& fio, int, dim3 grid, dim3 block, size_t lds, const DevParams* table) {
        for_tax_variant(d, [&](auto T, auto A) {
            for_bool(rows != nullptr, [&](auto O) {
                hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, 12, true, false, kExactMonthDefault, 0, 0, 0, decltype(O)::value>),
                                   grid, block, lds, stream, d, fio, table);
            });
        });
    });
}

// The three amounts every probe record carries (validate_params' rule for each), of record `k` of the list `list` names.
template <typename Record>
static bool amounts_valid(const char* list, int32_t k, const Record& r) {
    static const struct { double Record::*field; const char* name; int config_line; } kAmounts[3] = {
        {&Record::initial_balance, "initial_balance", 56},
        {&Record::monthly_contribution, "monthly_contribution", 57},
        {&Record::monthly_expenses, "monthly_expenses", 59}};
    for (const auto& f : kAmounts) {
        const double v = r.*(f.field);
        if (!(std::isfinite(v) && v >= 0.0)) {
            set_error("%s[%d].%s = %g: must be finite and >= 0 (config.py:%d)", list, k, f.name, v, f.config_line);
            return false;
        }
    }
    return true;
}

// A level probe (mcr_probe_expenses_rng / mcr_probe_contributions_rng): n_levels values of one field of the parameter block,
// `name` (config.py:`config_line`) in messages.  kFanout, the shared-work route, is tried first; where it answers
// MCR_ERR_UNSUPPORTED (unsupported shape / allocation refused) one launch per level runs instead.
using LevelFanout = int(const mcr_params*, const mcr_rng*, uint32_t, uint64_t, uint64_t, int32_t, const double*, int32_t, uint64_t*, hipStream_t);
template <LevelFanout* kFanout>
static int probe_levels(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths, int32_t wm,
                        double mcr_params::*field, const char* name, int config_line, const double* levels, int32_t n_levels,
                        uint64_t* counts, int device, hipStream_t main) {
    if (n_levels < 0) { set_error("n_levels %d must be >= 0", n_levels); return MCR_ERR_INVALID_ARG; }
    if (n_levels == 0) return MCR_OK;
    if (!levels || !counts) { set_error("null levels / counts"); return MCR_ERR_INVALID_ARG; }
    // validate every level BEFORE enqueueing anything (counts stay untouched on an error)
    int rc = validate_months(p, &wm, 1);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    for (int32_t k = 0; k < n_levels; ++k)
        if (!(std::isfinite(levels[k]) && levels[k] >= 0.0)) {
            set_error("%s[%d] = %g: must be finite and >= 0 (config.py:%d)", name, k, levels[k], config_line);
            return MCR_ERR_INVALID_ARG;
        }
    rc = zero_counters(counts, (size_t)n_levels, main);
    if (rc != MCR_OK) return rc;
    mcr_params q = *p;
    auto launch_level = [&](int k, hipStream_t s) {
        q.*field = levels[k];
        const mcr_outputs o = counters_only(counts + (size_t)k * MCR_N_COUNTERS);
        return launch_paths(&q, rng, stream_id, path_begin, n_paths, wm, nullptr, &o, s);
    };
    if (n_levels == 1) return launch_level(0, main);
    rc = kFanout(p, rng, stream_id, path_begin, n_paths, wm, levels, n_levels, counts, main);
    if (rc != MCR_ERR_UNSUPPORTED) return rc;
    return fork_join(device, main, n_levels, launch_level);
}

// A grid of working months x spending levels over the same paths, Philox stream: ONE accumulation sweep (PHASE 1) stores
// the state at the end of every distinct month, then grid fan-out launches (PHASE 6, grid.y = row) resume every row's
// decumulation with up to fanout_max_levels of its levels per launch.  Rows of a repeated month share its snapshot column.
// Returns MCR_ERR_UNSUPPORTED, having enqueued nothing, for shapes this form does not cover.
// The skeleton serves the plain grid (Cell = GridCell) and the grid under a spending rule (Cell = RuleGridCell): the month
// sorting, the snapshot plan, the rows' records level group by level group and the sweep are the same.  `fill(cell, row, first)`
// adds what the family's record carries beyond the grid's; `launch(gio, grid, block, lds, top, table)` launches the family's
// kernel for one level group on the group's records.  `launches`, where given, counts the fan-out launches and is reset when
// they report an error; `what` names the probe in HIP errors.
static GridCell& grid_part(GridCell& x) { return x; }
static GridCell& grid_part(RuleGridCell& x) { return x.cell; }
template <typename Cell, typename Fill, typename Launch>
static int launch_grid_fanout(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                              const int32_t* working_months, int32_t n_rows, const double* levels, int32_t n_levels, uint64_t* counts,
                              hipStream_t stream, int* launches, const char* what, Fill&& fill, Launch&& launch) {
    if (rng->kind != MCR_RNG_PHILOX || n_rows < 2 || n_paths == 0 || n_paths > ((uint64_t)1 << 31)) return MCR_ERR_UNSUPPORTED;
    if ((n_paths + 63) / 64 < fanout_min_waves()) return MCR_ERR_UNSUPPORTED;
    std::vector<int> order((size_t)n_rows), col((size_t)n_rows);
    sort_candidates(working_months, n_rows, order.data());
    std::vector<int32_t> months;    // distinct months, ascending = the snapshot columns
    for (int i = 0; i < n_rows; ++i) {
        const int32_t m = working_months[order[(size_t)i]];
        if (months.empty() || months.back() != m) months.push_back(m);
        col[(size_t)order[(size_t)i]] = (int)months.size() - 1;
    }
    const int n_cand = (int)months.size();
    if (n_cand < 2 || n_cand > MCR_MAX_PROBE_CANDIDATES) return MCR_ERR_UNSUPPORTED;
    std::vector<DevParams> blocks((size_t)n_cand);
    for (int c = 0; c < n_cand; ++c) {
        DevParams& b = blocks[(size_t)c];
        int rc = derive_params(p, months[(size_t)c], &b);
        if (rc != MCR_OK) return rc;
        if ((rc = check_barrier_counts(b)) != MCR_OK) return rc;
        b.n_lock_slots = b.n_lock_slots_total;   // (the same for every month: it depends on the stream list only)
    }
    const DevParams& top = blocks[(size_t)n_cand - 1];
    if (needs_generic_variant(top)) return MCR_ERR_UNSUPPORTED;
    const int lmax = fanout_max_levels(top);
    if (lmax < 1) return MCR_ERR_UNSUPPORTED;
    DevParams d1 = top;    // (PHASE 1 never reads a lock column: its plan may lower the LDS slots)
    size_t lds1 = 0;
    if (plan_path_kernel_lds(d1, 0, MCR_RNG_PHILOX, false, true, 0, &lds1) != MCR_OK) { (void)hipGetLastError(); return MCR_ERR_UNSUPPORTED; }
    KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    for (int c = 0; c < n_cand; ++c) io.snap_months[c] = months[(size_t)c];
    // the rows' records, level group by level group: group g covers levels [first, first + lg) of every row
    const LevelGroups groups(n_levels, lmax);
    std::vector<Cell> cells((size_t)groups.n_groups * (size_t)n_rows);
    std::memset(static_cast<void*>(cells.data()), 0, cells.size() * sizeof(Cell));
    groups.for_each([&](int g, int first, int lg) {
        for (int r = 0; r < n_rows; ++r) {
            GridCell& x = grid_part(cells[(size_t)g * n_rows + r]);
            x.p = blocks[(size_t)col[(size_t)r]];
            x.snap = col[(size_t)r];
            x.counters = counts + ((size_t)r * n_levels + first) * MCR_N_COUNTERS;
            for (int k = 0; k < lg; ++k) x.levels[k] = levels[(size_t)r * n_levels + first + k];
            fill(cells[(size_t)g * n_rows + r], r, first);
        }
    });
    SnapshotBlock snap(stream);
    hipError_t e = hipSuccess;
    if (!snap.attach(io, n_cand, cells.data(), cells.size() * sizeof(Cell), &e)) return MCR_ERR_UNSUPPORTED;
    const Cell* d_cells = (const Cell*)snap.records;
    if (e == hipSuccess) {
        const dim3 g6((unsigned)((n_paths + 63) / 64), (unsigned)n_rows);
        launch_accumulation(d1, io, nullptr, lds1, stream);
        groups.for_each([&](int g, int, int lg) {
            KernelIO gio = io;
            gio.fan_n = lg;
            launch(gio, g6, dim3(64 * (lg + 1)), fanout_dynamic_lds(top, lg), top, (const DevParams*)(d_cells + (size_t)g * n_rows));
            if (launches) ++*launches;
        });
        e = hipGetLastError();
    }
    const hipError_t ef = snap.mem.release();
    if (e != hipSuccess && launches) *launches = 0;
    if (e != hipSuccess) return hip_fail(e, what);
    if (ef != hipSuccess) return hip_fail(ef, (std::string(what) + " (free)").c_str());
    return MCR_OK;
}
static int probe_grid_shared(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                             const int32_t* working_months, int32_t n_rows, const double* levels, int32_t n_levels, uint64_t* counts,
                             hipStream_t stream) {
    return launch_grid_fanout<GridCell>(p, rng, stream_id, path_begin, n_paths, working_months, n_rows, levels, n_levels, counts, stream,
                                        nullptr, "grid probe", [](GridCell&, int, int) {},
                                        [&](const KernelIO& gio, dim3 grid, dim3 block, size_t lds, const DevParams& top, const DevParams* table) {
        for_tax_variant(top, [&](auto T, auto A) {
            hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, 6, true>), grid, block, lds, stream, top, gio, table);
        });
    });
}

// The grid under ONE spending rule (mcr_probe_rule_grid_rng): the grid probe's sweep and records, then rule grid fan-out launches
// (PHASE 6 with RULE) on the generic tax mask, like every rule kernel.  A row's record carries the rule (keep = 1 - cut, grow =
// 1 + raise: launch_rule's two operations) and the year counts of its first level of the group.  Returns MCR_ERR_UNSUPPORTED,
// having enqueued nothing, for shapes the grid probe's form does not cover.
static thread_local int g_last_rule_grid_fanout_launches = 0;   // (mcr_probe_rule_grid_last_fanout_launches)
static int probe_rule_grid_shared(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                  const int32_t* working_months, int32_t n_rows, const double* levels, int32_t n_levels,
                                  const mcr_spending_rule* rule, uint64_t* counts, uint64_t* year_counts, hipStream_t stream) {
    const size_t year_block = (size_t)p->retirement_years * MCR_RULE_N_COUNTS;   // one cell's year counts
    return launch_grid_fanout<RuleGridCell>(p, rng, stream_id, path_begin, n_paths, working_months, n_rows, levels, n_levels, counts, stream,
                                            &g_last_rule_grid_fanout_launches, "rule grid probe", [&](RuleGridCell& x, int r, int first) {
        x.upper = rule->upper; x.lower = rule->lower; x.keep = 1.0 - rule->cut; x.grow = 1.0 + rule->raise;
        x.floor = rule->floor; x.ceiling = rule->ceiling;
        x.year_counts = year_counts ? (unsigned long long*)year_counts + ((size_t)r * n_levels + first) * year_block : nullptr;
    }, [&](const KernelIO& gio, dim3 grid, dim3 block, size_t lds, const DevParams& top, const DevParams* table) {
        for_bool(top.any_annual_tax, [&](auto A) {
            hipLaunchKernelGGL((path_kernel<0, 0, 3, decltype(A)::value, false, 6, true, false, kExactMonthDefault, 0, 0, 0, false, false, 1, true>),
                               grid, block, lds, stream, top, gio, table);
        });
    });
}

// ---------------------------------------------------------------------------------------------
// Joint probes (mcr_probe_*_joint_rng): the per-path success bits of every option and their co-occurrence matrix
// ---------------------------------------------------------------------------------------------
struct JointOut { uint64_t* masks; uint64_t* joint; uint64_t* extremes; };   // (the *_joint_rng arguments; null = a plain probe)
// What a joint entry point checks before it touches the device or its outputs
static int check_joint_args(int32_t n_options, const uint64_t* joint) {
    if (n_options < 0 || n_options > MCR_MAX_JOINT_OPTIONS) {
        set_error("n_options %d: a joint probe takes 0 .. MCR_MAX_JOINT_OPTIONS = %d options", n_options, MCR_MAX_JOINT_OPTIONS);
        return MCR_ERR_INVALID_ARG;
    }
    if (n_options > 0 && !joint) { set_error("null joint"); return MCR_ERR_INVALID_ARG; }
    return MCR_OK;
}
// The routes of a scenario / assumption / income probe once its arguments are validated and `counts` zeroed.
//   fanout(masks): the probe's probe_*_fanout (MCR_ERR_UNSUPPORTED, nothing enqueued, for shapes it does not cover);
//   launch(k, stream, success, final_balance, years_to_ruin): option k's whole-path launch into its counter block and, where
//   non-null, a uint8 [n_paths] column and the two summary columns.
// `fan_one` (the glide probes, whose family has no plain launch): a single option takes the fan-out like several, in all three forms.
// Plain (jo == nullptr): one option -> its launch; else the fan-out; else one count-only launch per option (fork_join).
// Joint: the fan-out stores its ballots to the mask rows; where it does not run, one launch per option with `success` and
// `counters` set fills a scratch uint8 [n][n_paths] and pack_success_kernel turns each column into its row on the option's side
// stream.  Either way joint_counts_kernel then reduces the rows.  Masks the caller does not keep and the flag columns are
// stream-ordered scratch, released behind the work.
// Outcomes (rows != nullptr, never with jo): the fan-out's OUT kernels store the rows; where it does not run, option k's launch
// is a summary launch whose final_balance / years_to_ruin columns ARE its rows (years_to_ruin in scratch where the caller does
// not ask for it), and nan_failed_kernel then NaNs the final balances of the failed paths on the option's side stream.
template <typename Fanout, typename Launch>
static int run_probe_routes(int device, hipStream_t main, int n, uint64_t n_paths, const JointOut* jo, const mcr_option_outcomes* rows,
                            Fanout&& fanout, Launch&& launch, bool fan_one = false /* the glide probes: a single option fans out too */) {
    const bool one = n == 1 && !fan_one;     // a single option takes its plain launch
    if (rows && n_paths > 0) {
        int rc = one ? MCR_ERR_UNSUPPORTED : fanout(nullptr, rows);
        if (rc != MCR_ERR_UNSUPPORTED) return rc;
        StreamAlloc own_ruin(main);
        double* ruin = rows->years_to_ruin;
        size_t ruin_stride = (size_t)rows->path_stride;
        if (!ruin) {
            if (!own_ruin.alloc((size_t)n * n_paths * sizeof(double))) { set_error("outcome probe: could not allocate %d ruin columns", n); return MCR_ERR_HIP; }
            ruin = (double*)own_ruin.p;
            ruin_stride = (size_t)n_paths;
        }
        rc = fork_join(device, main, n, [&](int k, hipStream_t s) {
            double* const fin = rows->final_balance ? rows->final_balance + (size_t)k * (size_t)rows->path_stride : nullptr;
            double* const ytr = ruin + (size_t)k * ruin_stride;
            const int rck = launch(k, s, nullptr, fin, ytr);
            return rck == MCR_OK && fin ? launch_nan_failed(fin, ytr, n_paths, s) : rck;
        });
        const hipError_t ef = own_ruin.release();
        if (rc == MCR_OK && ef != hipSuccess) rc = hip_fail(ef, "outcome probe (free)");
        return rc;
    }
    auto per_option = [&](uint8_t* flags, uint64_t* masks) {
        return fork_join(device, main, n, [&](int k, hipStream_t s) {
            uint8_t* const col = flags ? flags + (size_t)k * n_paths : nullptr;
            const int rc = launch(k, s, col, nullptr, nullptr);
            return rc == MCR_OK && col ? launch_pack_success(col, n_paths, masks + (size_t)k * joint_mask_words(n_paths), s) : rc;
        });
    };
    if (!jo || n_paths == 0) {
        int rc = MCR_OK;
        if (one) rc = launch(0, main, nullptr, nullptr, nullptr);
        else if ((rc = fanout(nullptr, nullptr)) == MCR_ERR_UNSUPPORTED) rc = per_option(nullptr, nullptr);   // (unsupported shape / allocation refused)
        return rc == MCR_OK && jo ? launch_joint_counts(nullptr, n, 0, jo->joint, jo->extremes, main) : rc;
    }
    const size_t words = (size_t)joint_mask_words(n_paths);
    StreamAlloc own_masks(main), flags(main);
    uint64_t* masks = jo->masks;
    if (!masks) {
        if (!own_masks.alloc((size_t)n * words * sizeof(uint64_t))) { set_error("joint probe: could not allocate %d mask rows", n); return MCR_ERR_HIP; }
        masks = (uint64_t*)own_masks.p;
    }
    int rc = one ? MCR_ERR_UNSUPPORTED : fanout(masks, nullptr);
    if (rc == MCR_ERR_UNSUPPORTED) {
        if (!flags.alloc((size_t)n * n_paths)) { set_error("joint probe: could not allocate %d success columns", n); return MCR_ERR_HIP; }
        rc = per_option((uint8_t*)flags.p, masks);
        const hipError_t ef = flags.release();
        if (rc == MCR_OK && ef != hipSuccess) rc = hip_fail(ef, "joint probe (free)");
    }
    if (rc == MCR_OK) rc = launch_joint_counts(masks, n, n_paths, jo->joint, jo->extremes, main);
    const hipError_t ef = own_masks.release();
    if (rc == MCR_OK && ef != hipSuccess) rc = hip_fail(ef, "joint probe (free)");
    return rc;
}
// counters_only plus the per-path columns of the joint and the outcome probes' per-option route (all null: counters alone)
static mcr_outputs counters_and_columns(uint64_t* counters, uint8_t* success, double* final_balance, double* years_to_ruin) {
    mcr_outputs o = counters_only(counters);
    o.success = success;
    o.final_balance = final_balance;
    o.years_to_ruin = years_to_ruin;
    return o;
}
// What an outcomes entry point checks before it touches the device or its outputs; *rows = nullptr where no row is requested
static int check_outcome_args(const mcr_option_outcomes** rows, uint64_t n_paths) {
    if (*rows && !(*rows)->final_balance && !(*rows)->years_to_ruin) *rows = nullptr;
    if (*rows && ((*rows)->path_stride < 0 || (uint64_t)(*rows)->path_stride < n_paths)) {
        set_error("rows->path_stride %lld < n_paths %llu", (long long)(*rows)->path_stride, (unsigned long long)n_paths);
        return MCR_ERR_INVALID_ARG;
    }
    return MCR_OK;
}

// ---------------------------------------------------------------------------------------------
// Host-buffer calls (the *_host_rng entry points): NumPy pointers in, device work on a leased context, NumPy pointers out
// ---------------------------------------------------------------------------------------------
// The plan of one host-buffer call.  The entry point lists its buffers (plan / plan_rows / plan_rng), begin() leases a context
// of the device, carves every device buffer from the context's block (256-byte aligned slices), points the planned device
// slots at them and uploads; the entry point launches on stream(); finish() downloads, synchronises and maps the errors.
class HostCall {
public:
    HostCall() = default;
    HostCall(const HostCall&) = delete;
    HostCall& operator=(const HostCall&) = delete;
    ~HostCall() {   // a block above the keep limit does not go back to the pool
        HostCtx* c = lease_ ? lease_->p : nullptr;
        if (c && c->capacity > kHostCtxKeepBytes) { (void)hipFree(c->block); c->block = nullptr; c->capacity = 0; }
    }
    // A flat buffer of `bytes`: *dev_slot becomes its device address.  A null host pointer or no bytes plans nothing.
    template <class T>
    void plan(T** dev_slot, const void* host, size_t bytes, bool upload, bool download) {
        add({(void**)dev_slot, const_cast<void*>(host), 1, bytes, 0, 0, 0, upload, download});
    }
    // A pitched matrix (download only): `rows` rows of row_bytes, dev_pitch apart on the device and host_pitch apart at the caller
    template <class T>
    void plan_rows(T** dev_slot, const void* host, size_t rows, size_t row_bytes, size_t dev_pitch, size_t host_pitch) {
        add({(void**)dev_slot, const_cast<void*>(host), rows, row_bytes, dev_pitch, host_pitch, 0, false, true});
    }
    // The host tables of an rng descriptor (per-path seeds of n_paths, the history record): uploaded, and *rng — the call's own
    // copy of the descriptor — pointed at the device copies
    void plan_rng(mcr_rng* rng, uint64_t n_paths) {
        plan(&rng->path_seeds, rng->path_seeds, (size_t)n_paths * sizeof(uint32_t), true, false);
        if (rng->kind == MCR_RNG_HISTORY) plan(&rng->history, rng->history, (size_t)rng->history_months * 3 * sizeof(double), true, false);
    }
    // `what`: the allocation's name in the error text.  A failed upload is waited for before it is reported.
    int begin(int device, const char* what) {
        lease_.emplace(g_host_ctx, device);
        HostCtx* ctx = lease_->p;
        if (!ctx) return MCR_ERR_HIP;
        hipError_t e = hipSuccess;
        if (total_ > ctx->capacity) {   // grow the block (contents are not preserved)
            if (ctx->block) { (void)hipFree(ctx->block); ctx->block = nullptr; ctx->capacity = 0; }
            e = hipMalloc(&ctx->block, total_);
            if (e != hipSuccess) { ctx->block = nullptr; return hip_fail(e, what); }
            ctx->capacity = total_;
        }
        for (Buf& b : bufs_) {   // accumulated blocks start from the caller's current values
            *b.dev = (char*)ctx->block + b.offset;
            if (b.upload && e == hipSuccess) e = hipMemcpyAsync(*b.dev, b.host, b.row_bytes, hipMemcpyHostToDevice, ctx->stream);
        }
        if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return hip_fail(e, "upload"); }
        return MCR_OK;
    }
    hipStream_t stream() const { return lease_->p->stream; }
    // rc: the launch's.  ONE synchronisation, of this call's stream only, also behind a failed launch or copy.  `staged`: the flat
    // downloads land in staging copies and reach the caller only if the whole call succeeded; pitched matrices always go straight
    // to the caller (staging them would double host memory and copy time).  `what`: the execution's name in the error text.
    int finish(int rc, bool staged, const char* what) {
        const hipStream_t s = stream();
        std::vector<std::vector<unsigned char>> stage(staged ? bufs_.size() : 0);
        hipError_t e = hipSuccess;
        for (size_t i = 0; i < bufs_.size() && rc == MCR_OK && e == hipSuccess; ++i) {
            const Buf& b = bufs_[i];
            if (!b.download) continue;
            if (b.rows != 1) { e = hipMemcpy2DAsync(b.host, b.host_pitch, *b.dev, b.dev_pitch, b.row_bytes, b.rows, hipMemcpyDeviceToHost, s); continue; }
            if (staged) stage[i].resize(b.row_bytes);
            e = hipMemcpyAsync(staged ? stage[i].data() : b.host, *b.dev, b.row_bytes, hipMemcpyDeviceToHost, s);
        }
        const hipError_t es = hipStreamSynchronize(s);
        if (rc != MCR_OK) return rc;
        if (e != hipSuccess) return hip_fail(e, "download");
        if (es != hipSuccess) return hip_fail(es, what);
        for (size_t i = 0; i < stage.size(); ++i)
            if (!stage[i].empty()) std::memcpy(bufs_[i].host, stage[i].data(), bufs_[i].row_bytes);
        return MCR_OK;
    }

private:
    struct Buf { void** dev; void* host; size_t rows, row_bytes, dev_pitch, host_pitch, offset; bool upload, download; };
    void add(Buf b) {
        if (!b.host || b.row_bytes == 0) return;
        b.offset = total_;
        total_ += ((b.rows == 1 ? b.row_bytes : b.rows * b.dev_pitch) + 255) & ~(size_t)255;
        bufs_.push_back(b);
    }
    std::vector<Buf> bufs_;
    size_t total_ = 0;
    std::optional<HostCtxPool::Lease> lease_;
};

// The accumulated integer blocks of a host-buffer call, in one list: the caller's pointer, the slot of the copy that a device
// or a shard works on, and the length.  The host forms upload, download and sum them alike.
struct IntBlock { uint64_t* const* src; uint64_t** dst; size_t n; };
static std::vector<IntBlock> output_blocks(const mcr_sizes& sz, const mcr_outputs* in, mcr_outputs* o) {
    const bool hist = in->hist_bins && in->hist_n_bins > 0;
    return {{&in->counters, &o->counters, MCR_N_COUNTERS}, {&in->wr_obs_counts, &o->wr_obs_counts, (size_t)sz.retirement_years},
            {&in->ruin_year_bins, &o->ruin_year_bins, (size_t)sz.ruin_bins}, {&in->hist_bins, &o->hist_bins, hist ? (size_t)in->hist_n_bins : 0}};
}
struct YearBinsOut { mcr_outputs o; mcr_year_bins y; };   // what a yearly-bins call writes to
static std::vector<IntBlock> year_bins_blocks(const mcr_sizes& sz, const YearBinsOut& in, YearBinsOut* o) {
    const size_t T = (size_t)sz.trajectory_len, ry = (size_t)sz.retirement_years;
    const size_t cells = (size_t)in.y.n_bins + 2, wcells = (size_t)in.y.n_wr_bins + 2;
    std::vector<IntBlock> blocks = output_blocks(sz, &in.o, &o->o);
    blocks.insert(blocks.end(), {{&in.y.trajectory_bins, &o->y.trajectory_bins, T * cells}, {&in.y.real_trajectory_bins, &o->y.real_trajectory_bins, T * cells},
                                 {&in.y.wr_bins, &o->y.wr_bins, ry * wcells}, {&in.y.final_success_bins, &o->y.final_success_bins, cells}});
    return blocks;
}

// One host-buffer call sharded over a device list (null / empty: every device): contiguous global path ranges of
// ceil(n_paths / W) paths, one host thread per entry that has paths (each leases its own context), every integer block summed
// on the host.  No collective is needed: what the devices exchange is a few KB and lands in host memory anyway.
//   blocks(Out* shard): the integer blocks, src in `caller`, dst in *shard — each shard gets zeroed blocks of its own there
//   run(device, begin, count, shard_out): the one-device call on paths [begin, begin + count) of the range
// One device in the list: run(device, 0, n_paths, caller) on the calling thread.  The first failing shard's error is reported
// with its device in front.
template <class Out, class Blocks, class Run>
static int run_sharded(const int32_t* devices, int32_t n_devices, uint64_t n_paths, const Out& caller, Blocks blocks, Run run) {
    std::vector<int> devs;
    if (!devices || n_devices <= 0) {
        const int n = mcr_device_count();
        if (n <= 0) { set_error("no usable HIP device (the engine has no CPU fallback)"); return MCR_ERR_NO_DEVICE; }
        for (int i = 0; i < n; ++i) devs.push_back(i);
    } else {
        devs.assign(devices, devices + n_devices);
    }
    const size_t W = devs.size();
    if (W == 1) return run(devs[0], (uint64_t)0, n_paths, caller);
    const uint64_t per = (n_paths + W - 1) / W;
    struct Shard {
        int rc = MCR_OK;
        char err[512] = "";
        Out out;
        std::vector<std::vector<uint64_t>> mem;   // empty: the shard has no paths
    };
    std::vector<Shard> shards(W);
    std::vector<std::thread> threads;
    for (size_t w = 0; w < W; ++w) {
        const uint64_t begin = std::min<uint64_t>(w * per, n_paths);
        const uint64_t count = std::min<uint64_t>(per, n_paths - begin);
        if (count == 0) continue;
        Shard& S = shards[w];
        S.out = caller;
        for (const IntBlock& b : blocks(&S.out)) {
            S.mem.emplace_back(*b.src && b.n ? b.n : 0, 0);
            *b.dst = S.mem.back().empty() ? nullptr : S.mem.back().data();
        }
        threads.emplace_back([&shards, &devs, &run, w, begin, count]() {
            Shard& T = shards[w];
            T.rc = run(devs[w], begin, count, T.out);
            if (T.rc != MCR_OK) std::snprintf(T.err, sizeof(T.err), "device %d: %s", devs[w], mcr_last_error());
        });
    }
    for (std::thread& t : threads) t.join();
    for (const Shard& S : shards)
        if (S.rc != MCR_OK) { set_error("%s", S.err); return S.rc; }
    Out scratch = caller;
    const std::vector<IntBlock> sums = blocks(&scratch);
    for (const Shard& S : shards)
        for (size_t i = 0; i < S.mem.size(); ++i)
            for (size_t k = 0; k < S.mem[i].size(); ++k) (*sums[i].src)[k] += S.mem[i][k];
    return MCR_OK;
}

}  // namespace mcr

// =============================================================================================
// C ABI
// =============================================================================================
using namespace mcr;

extern "C" {

int mcr_abi_version(void) { return MCR_ABI_VERSION; }

int mcr_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

const char* mcr_last_error(void) { return g_err; }

int mcr_query_sizes(const mcr_params* p, int32_t working_months, mcr_sizes* out) {
    return query_sizes(p, working_months, out);
}

// mcr_k1_*_form: the mask a launch on this parameter block runs, by the form's own rule (growth_form_of, ...)
static int k1_form(const mcr_params* p, int32_t working_months, int32_t* mask, int (*form_of)(const DevParams&, bool, int*)) {
    if (!mask) { set_error("null mask"); return MCR_ERR_INVALID_ARG; }
    DevParams d;
    int rc = derive_params(p, working_months, &d);
    if (rc != MCR_OK) return rc;
    int m = 0;
    rc = form_of(d, true, &m);
    if (rc != MCR_OK) return rc;
    *mask = m;
    return MCR_OK;
}
int mcr_k1_growth_form(const mcr_params* p, int32_t working_months, int32_t* mask) { return k1_form(p, working_months, mask, growth_form_of); }
int mcr_k1_month_form(const mcr_params* p, int32_t working_months, int32_t* mask) { return k1_form(p, working_months, mask, month_form_of); }
int mcr_k1_stream_form(const mcr_params* p, int32_t working_months, int32_t* mask) { return k1_form(p, working_months, mask, stream_form_of); }

int mcr_k1_screen(const mcr_params* p, const mcr_rng* rng, int32_t working_months, uint64_t n_paths, int32_t hist_n_bins, int32_t* screened) {
    if (!screened) { set_error("null screened"); return MCR_ERR_INVALID_ARG; }
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, working_months, &d, &extra);
    if (rc != MCR_OK) return rc;
    if (rng && (rc = check_rng(rng)) != MCR_OK) return rc;
    bool s = false;
    rc = screen_route_of(d, rng, n_paths, hist_n_bins, &s);
    if (rc != MCR_OK) return rc;
    *screened = s ? 1 : 0;
    return MCR_OK;
}

int mcr_screen_paths_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                         int32_t working_months, uint8_t* cls, float* min_ratio, float* final_total, int device) {
    MCR_ENTER_DEVICE(device);
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, working_months, &d, &extra);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    if (rng->kind != MCR_RNG_PHILOX || !screen_qualified(d)) { set_error("the launch does not qualify for screening (mcr_k1_screen)"); return MCR_ERR_UNSUPPORTED; }
    if (n_paths == 0) return MCR_OK;
    if (n_paths > (uint64_t)UINT32_MAX) { set_error("n_paths too large for one screening launch"); return MCR_ERR_INVALID_ARG; }
    if (path_begin + n_paths < path_begin) { set_error("path range overflows 64 bits"); return MCR_ERR_INVALID_ARG; }
    DeviceArena arena;
    ScreenIO sio;
    std::memset(&sio, 0, sizeof(sio));
    sio.seed = rng->philox_seed; sio.path_begin = path_begin; sio.n_paths = n_paths; sio.stream_id = stream_id;
    hipError_t e = hipSuccess;
    if (cls) e = arena.alloc((void**)&sio.cls, (size_t)n_paths);
    if (e == hipSuccess && min_ratio) e = arena.alloc((void**)&sio.min_ratio, (size_t)n_paths * sizeof(float));
    if (e == hipSuccess && final_total) e = arena.alloc((void**)&sio.final_total, (size_t)n_paths * sizeof(float));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    launch_screen_kernel<true>(d, screen_params(d), sio, dim3((unsigned)((n_paths + kBlock - 1) / kBlock)), nullptr);
    e = hipGetLastError();
    if (e == hipSuccess && cls) e = hipMemcpy(cls, sio.cls, (size_t)n_paths, hipMemcpyDeviceToHost);
    if (e == hipSuccess && min_ratio) e = hipMemcpy(min_ratio, sio.min_ratio, (size_t)n_paths * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess && final_total) e = hipMemcpy(final_total, sio.final_total, (size_t)n_paths * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) return hip_fail(e, "screen_kernel");
    return MCR_OK;
}

int mcr_k1_kept_streams(const mcr_params* p, int32_t working_months, int32_t* index, int32_t* lock_slot, int32_t cap, int32_t* n) {
    if (!n || cap < 0 || (cap > 0 && (!index || !lock_slot))) { set_error("null argument"); return MCR_ERR_INVALID_ARG; }
    DevParams d;
    std::vector<DevStream> extra;
    std::vector<std::pair<int, int>> kept;
    const int rc = derive_params(p, working_months, &d, &extra, &kept);
    if (rc != MCR_OK) return rc;
    for (size_t i = 0; i < kept.size() && i < (size_t)cap; ++i) { index[i] = kept[i].first; lock_slot[i] = kept[i].second; }
    *n = (int32_t)kept.size();
    return MCR_OK;
}

int32_t mcr_stream_start_month_index(double current_age, int32_t working_months, double start_at_age) {
    return start_month_index(current_age, working_months, start_at_age);
}

static mcr_rng philox_rng(uint64_t seed) {
    mcr_rng r;
    std::memset(&r, 0, sizeof(r));
    r.kind = MCR_RNG_PHILOX;
    r.philox_seed = seed;
    return r;
}

int mcr_run_batch_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                      uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                      const mcr_outputs* out, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return launch_paths(p, rng, stream_id, path_begin, n_paths, working_months, injected_shocks, out,
                        (hipStream_t)hip_stream);
}

int mcr_validate_spending_rule(const mcr_spending_rule* rule) { return validate_spending_rule(rule); }

int mcr_run_rule_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                     int32_t working_months, const mcr_spending_rule* rule, mcr_outputs* out, mcr_rule_outputs* rule_out,
                     int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return launch_rule(p, rng, stream_id, path_begin, n_paths, working_months, rule, out, rule_out, (hipStream_t)hip_stream);
}

int mcr_probe_months_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                         uint64_t n_paths, const int32_t* working_months, int32_t n_candidates,
                         uint64_t* counts, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    if (!working_months || !counts || n_candidates < 0) { set_error("null candidates / counts"); return MCR_ERR_INVALID_ARG; }
    if (n_candidates == 0) return MCR_OK;
    int rc = validate_months(p, working_months, n_candidates);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    hipStream_t main = (hipStream_t)hip_stream;
    rc = zero_counters(counts, (size_t)n_candidates, main);
    if (rc != MCR_OK) return rc;
    auto launch_candidate = [&](int c, hipStream_t s) {
        const mcr_outputs o = counters_only(counts + (size_t)c * MCR_N_COUNTERS);
        return launch_paths(p, rng, stream_id, path_begin, n_paths, working_months[c], nullptr, &o, s);
    };
    if (n_candidates == 1) return launch_candidate(0, main);
    if (rng->kind == MCR_RNG_PHILOX && n_candidates <= MCR_MAX_PROBE_CANDIDATES) {
        rc = probe_shared_prefix(p, rng, stream_id, path_begin, n_paths, working_months, n_candidates, counts, main);
        if (rc != MCR_ERR_UNSUPPORTED) return rc;     // (unsupported shape / allocation refused: one launch per candidate below)
    }
    return fork_join(device, main, n_candidates, launch_candidate);
}

int mcr_probe_expenses_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                           uint64_t n_paths, int32_t working_months, const double* monthly_expenses, int32_t n_levels,
                           uint64_t* counts, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return probe_levels<probe_expenses_fanout>(p, rng, stream_id, path_begin, n_paths, working_months, &mcr_params::monthly_expenses,
                                               "monthly_expenses", 59, monthly_expenses, n_levels, counts, device, (hipStream_t)hip_stream);
}

int mcr_probe_contributions_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                uint64_t n_paths, int32_t working_months, const double* monthly_contributions, int32_t n_levels,
                                uint64_t* counts, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return probe_levels<probe_contributions_fanout>(p, rng, stream_id, path_begin, n_paths, working_months, &mcr_params::monthly_contribution,
                                                    "monthly_contribution", 57, monthly_contributions, n_levels, counts, device, (hipStream_t)hip_stream);
}

// mcr_probe_scenarios_rng (jo == nullptr, rows == nullptr), mcr_probe_scenarios_joint_rng and mcr_probe_scenarios_outcomes_rng,
// on the entered device
static int probe_scenarios(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                           int32_t working_months, const mcr_scenario* scenarios, int32_t n_scenarios, uint64_t* counts,
                           const JointOut* jo, const mcr_option_outcomes* rows, int device, hipStream_t main) {
    if (n_scenarios < 0) { set_error("n_scenarios %d must be >= 0", n_scenarios); return MCR_ERR_INVALID_ARG; }
    if (n_scenarios == 0) return MCR_OK;
    if (!scenarios || !counts) { set_error("null scenarios / counts"); return MCR_ERR_INVALID_ARG; }
    // validate every record BEFORE enqueueing anything (counts stay untouched on an error)
    int rc = validate_months(p, &working_months, 1);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    for (int32_t k = 0; k < n_scenarios; ++k)
        if (!amounts_valid("scenarios", k, scenarios[k])) return MCR_ERR_INVALID_ARG;
    rc = zero_counters(counts, (size_t)n_scenarios, main);
    if (rc != MCR_OK) return rc;
    mcr_params q = *p;
    auto launch_scenario = [&](int k, hipStream_t s, uint8_t* success, double* final_balance, double* years_to_ruin) {
        q.initial_balance = scenarios[k].initial_balance;
        q.monthly_contribution = scenarios[k].monthly_contribution;
        q.monthly_expenses = scenarios[k].monthly_expenses;
        const mcr_outputs o = counters_and_columns(counts + (size_t)k * MCR_N_COUNTERS, success, final_balance, years_to_ruin);
        return launch_paths(&q, rng, stream_id, path_begin, n_paths, working_months, nullptr, &o, s);
    };
    auto fanout = [&](uint64_t* masks, const mcr_option_outcomes* fan_rows) {
        return probe_scenarios_fanout(p, rng, stream_id, path_begin, n_paths, working_months, scenarios, n_scenarios, counts, main, masks, fan_rows);
    };
    return run_probe_routes(device, main, n_scenarios, n_paths, jo, rows, fanout, launch_scenario);
}

int mcr_probe_scenarios_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                            uint64_t n_paths, int32_t working_months, const mcr_scenario* scenarios,
                            int32_t n_scenarios, uint64_t* counts, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return probe_scenarios(p, rng, stream_id, path_begin, n_paths, working_months, scenarios, n_scenarios, counts, nullptr, nullptr, device,
                           (hipStream_t)hip_stream);
}

int mcr_probe_scenarios_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                  uint64_t n_paths, int32_t working_months, const mcr_scenario* scenarios,
                                  int32_t n_scenarios, uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes,
                                  int device, void* hip_stream) {
    if (int rc = check_joint_args(n_scenarios, joint)) return rc;
    MCR_ENTER_DEVICE(device);
    const JointOut jo{masks, joint, extremes};
    return probe_scenarios(p, rng, stream_id, path_begin, n_paths, working_months, scenarios, n_scenarios, counts, &jo, nullptr, device,
                           (hipStream_t)hip_stream);
}

int mcr_probe_scenarios_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                     uint64_t n_paths, int32_t working_months, const mcr_scenario* scenarios,
                                     int32_t n_scenarios, uint64_t* counts, const mcr_option_outcomes* rows, int device, void* hip_stream) {
    if (int rc = check_outcome_args(&rows, n_paths)) return rc;
    MCR_ENTER_DEVICE(device);
    return probe_scenarios(p, rng, stream_id, path_begin, n_paths, working_months, scenarios, n_scenarios, counts, nullptr, rows, device,
                           (hipStream_t)hip_stream);
}

// mcr_probe_assumptions_rng (jo == nullptr, rows == nullptr), mcr_probe_assumptions_joint_rng and
// mcr_probe_assumptions_outcomes_rng, on the entered device
static int probe_assumptions(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                             int32_t working_months, const mcr_assumptions* records, int32_t n_records, uint64_t* counts,
                             const JointOut* jo, const mcr_option_outcomes* rows, int device, hipStream_t main) {
    g_last_assumption_fanout_launches = 0;
    if (n_records < 0) { set_error("n_records %d must be >= 0", n_records); return MCR_ERR_INVALID_ARG; }
    if (n_records == 0) return MCR_OK;
    if (!records || !counts) { set_error("null records / counts"); return MCR_ERR_INVALID_ARG; }
    // validate the block itself (validate_months derives it, its own ten fields included: *p must be valid on every route,
    // whatever the records replace) and every record BEFORE enqueueing anything (counts stay untouched on an error):
    // validate_params' rules
    int rc = validate_months(p, &working_months, 1);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    static const struct { double mcr_assumptions::*mu; double mcr_assumptions::*sigma; const char* name; } kSeries[3] = {
        {&mcr_assumptions::inv1_mu_log, &mcr_assumptions::inv1_sigma_log, "inv1"},
        {&mcr_assumptions::inf_mu_log, &mcr_assumptions::inf_sigma_log, "inf"},
        {&mcr_assumptions::prem_mu_log, &mcr_assumptions::prem_sigma_log, "prem"}};
    for (int32_t k = 0; k < n_records; ++k) {
        const mcr_assumptions& r = records[k];
        if (!amounts_valid("records", k, r)) return MCR_ERR_INVALID_ARG;
        for (const auto& f : kSeries) {
            const double mu = r.*(f.mu), sg = r.*(f.sigma);
            if (!log_growth_in_domain(mu, sg)) {
                set_error("records[%d].%s_mu_log / records[%d].%s_sigma_log = %g / %g: need finite values, sigma >= 0 and |mu|/12 + 40 sigma/sqrt(12) < 700",
                          k, f.name, k, f.name, mu, sg);
                return MCR_ERR_INVALID_ARG;
            }
        }
        if (!(r.equity_inflation_rho >= -1.0 && r.equity_inflation_rho <= 1.0)) {
            set_error("records[%d].equity_inflation_rho = %g: must be in [-1, 1] (config.py:85)", k, r.equity_inflation_rho);
            return MCR_ERR_INVALID_ARG;
        }
    }
    rc = zero_counters(counts, (size_t)n_records, main);
    if (rc != MCR_OK) return rc;
    mcr_params q = *p;
    auto launch_record = [&](int k, hipStream_t s, uint8_t* success, double* final_balance, double* years_to_ruin) {
        const mcr_assumptions& r = records[k];
        q.initial_balance = r.initial_balance; q.monthly_contribution = r.monthly_contribution; q.monthly_expenses = r.monthly_expenses;
        q.inv1_mu_log = r.inv1_mu_log; q.inv1_sigma_log = r.inv1_sigma_log;
        q.inf_mu_log = r.inf_mu_log; q.inf_sigma_log = r.inf_sigma_log;
        q.prem_mu_log = r.prem_mu_log; q.prem_sigma_log = r.prem_sigma_log;
        q.equity_inflation_rho = r.equity_inflation_rho;
        const mcr_outputs o = counters_and_columns(counts + (size_t)k * MCR_N_COUNTERS, success, final_balance, years_to_ruin);
        return launch_paths(&q, rng, stream_id, path_begin, n_paths, working_months, nullptr, &o, s);
    };
    auto fanout = [&](uint64_t* masks, const mcr_option_outcomes* fan_rows) {
        return probe_assumptions_fanout(p, rng, stream_id, path_begin, n_paths, working_months, records, n_records, counts, main, masks, fan_rows);
    };
    return run_probe_routes(device, main, n_records, n_paths, jo, rows, fanout, launch_record);
}

int mcr_probe_assumptions_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const mcr_assumptions* records,
                              int32_t n_records, uint64_t* counts, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return probe_assumptions(p, rng, stream_id, path_begin, n_paths, working_months, records, n_records, counts, nullptr, nullptr, device,
                             (hipStream_t)hip_stream);
}

int mcr_probe_assumptions_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                    uint64_t n_paths, int32_t working_months, const mcr_assumptions* records,
                                    int32_t n_records, uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes,
                                    int device, void* hip_stream) {
    if (int rc = check_joint_args(n_records, joint)) return rc;
    MCR_ENTER_DEVICE(device);
    const JointOut jo{masks, joint, extremes};
    return probe_assumptions(p, rng, stream_id, path_begin, n_paths, working_months, records, n_records, counts, &jo, nullptr, device,
                             (hipStream_t)hip_stream);
}

int mcr_probe_assumptions_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                       uint64_t n_paths, int32_t working_months, const mcr_assumptions* records,
                                       int32_t n_records, uint64_t* counts, const mcr_option_outcomes* rows, int device, void* hip_stream) {
    if (int rc = check_outcome_args(&rows, n_paths)) return rc;
    MCR_ENTER_DEVICE(device);
    return probe_assumptions(p, rng, stream_id, path_begin, n_paths, working_months, records, n_records, counts, nullptr, rows, device,
                             (hipStream_t)hip_stream);
}

int mcr_probe_assumptions_last_fanout_launches(void) { return g_last_assumption_fanout_launches; }

// mcr_probe_income_rng (jo == nullptr, rows == nullptr), mcr_probe_income_joint_rng and mcr_probe_income_outcomes_rng, on the
// entered device
static int probe_income(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                        int32_t working_months, int32_t stream_index, const mcr_income_option* options, int32_t n_options,
                        uint64_t* counts, const JointOut* jo, const mcr_option_outcomes* rows, int device, hipStream_t main) {
    g_last_income_fanout_launches = 0;
    if (n_options < 0) { set_error("n_options %d must be >= 0", n_options); return MCR_ERR_INVALID_ARG; }
    if (n_options == 0) return MCR_OK;
    if (!options || !counts) { set_error("null options / counts"); return MCR_ERR_INVALID_ARG; }
    // validate the block, the index and every record BEFORE enqueueing anything (counts stay untouched on an error)
    int rc = validate_months(p, &working_months, 1);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    if (stream_index < 0 || stream_index >= p->n_streams) {
        set_error("stream_index = %d: must be in [0, n_streams = %d)", stream_index, p->n_streams);
        return MCR_ERR_INVALID_ARG;
    }
    for (int32_t k = 0; k < n_options; ++k) {
        const mcr_income_option& r = options[k];
        if (!amounts_valid("options", k, r)) return MCR_ERR_INVALID_ARG;
        if (!(std::isfinite(r.monthly_amount_today) && r.monthly_amount_today >= 0.0)) {
            set_error("options[%d].monthly_amount_today = %g: must be finite and >= 0 (config.py:18)", k, r.monthly_amount_today);
            return MCR_ERR_INVALID_ARG;
        }
        if (!(std::isfinite(r.start_at_age) && r.start_at_age >= 0.0 && r.start_at_age <= 120.0)) {
            set_error("options[%d].start_at_age = %g: must be finite and in [0, 120] (config.py:23)", k, r.start_at_age);
            return MCR_ERR_INVALID_ARG;
        }
        if (r.duration_years < -1) {
            set_error("options[%d].duration_years = %d: must be >= 0, or -1 for None (config.py:33)", k, r.duration_years);
            return MCR_ERR_INVALID_ARG;
        }
        if (r.reserved != 0) {
            set_error("options[%d].reserved = %d: must be 0", k, r.reserved);
            return MCR_ERR_INVALID_ARG;
        }
    }
    rc = zero_counters(counts, (size_t)n_options, main);
    if (rc != MCR_OK) return rc;
    // the per-option route's parameter block: a copy whose stream `stream_index` is rewritten per launch (launch_paths derives
    // its records, the extra table's included, before it returns)
    mcr_params q = *p;
    std::vector<mcr_stream> q_extra;
    if (p->n_streams > MCR_INLINE_STREAMS) {
        q_extra.assign(p->extra_streams, p->extra_streams + (p->n_streams - MCR_INLINE_STREAMS));
        q.extra_streams = q_extra.data();
    }
    mcr_stream& qs = stream_index < MCR_INLINE_STREAMS ? q.streams[stream_index] : q_extra[(size_t)(stream_index - MCR_INLINE_STREAMS)];
    auto launch_option = [&](int k, hipStream_t s, uint8_t* success, double* final_balance, double* years_to_ruin) {
        const mcr_income_option& r = options[k];
        q.initial_balance = r.initial_balance; q.monthly_contribution = r.monthly_contribution; q.monthly_expenses = r.monthly_expenses;
        qs.monthly_amount_today = r.monthly_amount_today; qs.start_at_age = r.start_at_age; qs.duration_years = r.duration_years;
        const mcr_outputs o = counters_and_columns(counts + (size_t)k * MCR_N_COUNTERS, success, final_balance, years_to_ruin);
        return launch_paths(&q, rng, stream_id, path_begin, n_paths, working_months, nullptr, &o, s);
    };
    auto fanout = [&](uint64_t* masks, const mcr_option_outcomes* fan_rows) {
        return probe_income_fanout(p, rng, stream_id, path_begin, n_paths, working_months, stream_index, options, n_options, counts, main, masks, fan_rows);
    };
    return run_probe_routes(device, main, n_options, n_paths, jo, rows, fanout, launch_option);
}

int mcr_probe_income_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                         uint64_t n_paths, int32_t working_months, int32_t stream_index,
                         const mcr_income_option* options, int32_t n_options,
                         uint64_t* counts, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return probe_income(p, rng, stream_id, path_begin, n_paths, working_months, stream_index, options, n_options, counts, nullptr, nullptr, device,
                        (hipStream_t)hip_stream);
}

int mcr_probe_income_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                               uint64_t n_paths, int32_t working_months, int32_t stream_index,
                               const mcr_income_option* options, int32_t n_options,
                               uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes, int device, void* hip_stream) {
    if (int rc = check_joint_args(n_options, joint)) return rc;
    MCR_ENTER_DEVICE(device);
    const JointOut jo{masks, joint, extremes};
    return probe_income(p, rng, stream_id, path_begin, n_paths, working_months, stream_index, options, n_options, counts, &jo, nullptr, device,
                        (hipStream_t)hip_stream);
}

int mcr_probe_income_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                  uint64_t n_paths, int32_t working_months, int32_t stream_index,
                                  const mcr_income_option* options, int32_t n_options,
                                  uint64_t* counts, const mcr_option_outcomes* rows, int device, void* hip_stream) {
    if (int rc = check_outcome_args(&rows, n_paths)) return rc;
    MCR_ENTER_DEVICE(device);
    return probe_income(p, rng, stream_id, path_begin, n_paths, working_months, stream_index, options, n_options, counts, nullptr, rows,
                        device, (hipStream_t)hip_stream);
}

int mcr_probe_income_last_fanout_launches(void) { return g_last_income_fanout_launches; }

// What the allocation probes check on the host, before a device is looked for: the block, the month, the stream, every option
static int check_allocation_probe(const mcr_params* p, const mcr_rng* rng, int32_t working_months, const mcr_allocation_option* options,
                                  int32_t n_options, const uint64_t* counts) {
    if (n_options < 0) { set_error("n_options %d must be >= 0", n_options); return MCR_ERR_INVALID_ARG; }
    if (n_options == 0) return MCR_OK;
    if (!options || !counts) { set_error("null options / counts"); return MCR_ERR_INVALID_ARG; }
    int rc = validate_months(p, &working_months, 1);
    if (rc != MCR_OK) return rc;
    if ((rc = check_rng(rng)) != MCR_OK) return rc;
    for (int32_t k = 0; k < n_options; ++k) {
        if (!amounts_valid("options", k, options[k])) return MCR_ERR_INVALID_ARG;
        const double a = options[k].allocation_inv1_pct;
        if (!(std::isfinite(a) && a >= 0.0 && a <= 1.0)) {
            set_error("options[%d].allocation_inv1_pct = %.17g: must be finite and in [0, 1] (config.py:70)", k, a);
            return MCR_ERR_INVALID_ARG;
        }
    }
    return MCR_OK;
}
// mcr_probe_allocations_rng (jo == nullptr, rows == nullptr), mcr_probe_allocations_joint_rng and
// mcr_probe_allocations_outcomes_rng, on the entered device, their arguments checked
static int probe_allocations(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                             int32_t working_months, const mcr_allocation_option* options, int32_t n_options, uint64_t* counts,
                             const JointOut* jo, const mcr_option_outcomes* rows, int device, hipStream_t main) {
    int rc = zero_counters(counts, (size_t)n_options, main);
    if (rc != MCR_OK) return rc;
    mcr_params q = *p;
    auto launch_option = [&](int k, hipStream_t s, uint8_t* success, double* final_balance, double* years_to_ruin) {
        const mcr_allocation_option& r = options[k];
        q.initial_balance = r.initial_balance; q.monthly_contribution = r.monthly_contribution; q.monthly_expenses = r.monthly_expenses;
        q.allocation_inv1_pct = r.allocation_inv1_pct;
        const mcr_outputs o = counters_and_columns(counts + (size_t)k * MCR_N_COUNTERS, success, final_balance, years_to_ruin);
        return launch_paths(&q, rng, stream_id, path_begin, n_paths, working_months, nullptr, &o, s);
    };
    auto fanout = [&](uint64_t* masks, const mcr_option_outcomes* fan_rows) {
        return probe_allocations_fanout(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, main, masks, fan_rows);
    };
    return run_probe_routes(device, main, n_options, n_paths, jo, rows, fanout, launch_option);
}

int mcr_probe_allocations_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const mcr_allocation_option* options, int32_t n_options,
                              uint64_t* counts, int device, void* hip_stream) {
    g_last_allocation_fanout_launches = 0;
    if (int rc = check_allocation_probe(p, rng, working_months, options, n_options, counts)) return rc;
    if (n_options == 0) return MCR_OK;
    MCR_ENTER_DEVICE(device);
    return probe_allocations(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, nullptr, nullptr, device,
                             (hipStream_t)hip_stream);
}

int mcr_probe_allocations_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                    uint64_t n_paths, int32_t working_months, const mcr_allocation_option* options, int32_t n_options,
                                    uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes, int device, void* hip_stream) {
    g_last_allocation_fanout_launches = 0;
    if (int rc = check_joint_args(n_options, joint)) return rc;
    if (int rc = check_allocation_probe(p, rng, working_months, options, n_options, counts)) return rc;
    if (n_options == 0) return MCR_OK;
    MCR_ENTER_DEVICE(device);
    const JointOut jo{masks, joint, extremes};
    return probe_allocations(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, &jo, nullptr, device,
                             (hipStream_t)hip_stream);
}

int mcr_probe_allocations_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                       uint64_t n_paths, int32_t working_months, const mcr_allocation_option* options, int32_t n_options,
                                       uint64_t* counts, const mcr_option_outcomes* rows, int device, void* hip_stream) {
    g_last_allocation_fanout_launches = 0;
    if (int rc = check_outcome_args(&rows, n_paths)) return rc;
    if (int rc = check_allocation_probe(p, rng, working_months, options, n_options, counts)) return rc;
    if (n_options == 0) return MCR_OK;
    MCR_ENTER_DEVICE(device);
    return probe_allocations(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, nullptr, rows, device,
                             (hipStream_t)hip_stream);
}

int mcr_probe_allocations_last_fanout_launches(void) { return g_last_allocation_fanout_launches; }

// ---- glide probes (PHASE 13; include/mcr.h: GLIDE PATH) ----
// What the glide probes check on the host, before a device is looked for: the block, the month, the stream, every option and
// every weight an option names
// One table's entries: finite and in [0, 1].  `owner` heads the field's name ("options[2]." for a probe's record, "" for a launch's own table).
static bool glide_weights_valid(const char* owner, const double* w, int32_t n) {
    for (int32_t i = 0; i < n; ++i) {
        const double a = w[i];
        if (!(std::isfinite(a) && a >= 0.0 && a <= 1.0)) {
            set_error("%sweights[%d] = %.17g: must be finite and in [0, 1] (config.py:70)", owner, i, a);
            return false;
        }
    }
    return true;
}
static int check_glide_probe(const mcr_params* p, const mcr_rng* rng, int32_t working_months, const double* weights, int32_t n_weights,
                             const mcr_glide_option* options, int32_t n_options, const uint64_t* counts) {
    if (n_options < 0) { set_error("n_options %d must be >= 0", n_options); return MCR_ERR_INVALID_ARG; }
    if (n_options == 0) return MCR_OK;
    if (!options || !counts) { set_error("null options / counts"); return MCR_ERR_INVALID_ARG; }
    if (n_weights < 0 || (n_weights > 0 && !weights)) { set_error("weights: n_weights %d must be >= 0 and the table non-null", n_weights); return MCR_ERR_INVALID_ARG; }
    int rc = validate_months(p, &working_months, 1);
    if (rc != MCR_OK) return rc;
    if ((rc = check_rng(rng)) != MCR_OK) return rc;
    for (int32_t k = 0; k < n_options; ++k) {
        const mcr_glide_option& o = options[k];
        if (!amounts_valid("options", k, o)) return MCR_ERR_INVALID_ARG;
        if (o.n_weights < 1) { set_error("options[%d].n_weights = %d: a glide path has at least one entry", k, o.n_weights); return MCR_ERR_INVALID_ARG; }
        if (o.first_weight < 0 || (int64_t)o.first_weight + (int64_t)o.n_weights > (int64_t)n_weights) {
            set_error("options[%d].first_weight = %d with n_weights = %d: outside the table of %d weights", k, o.first_weight, o.n_weights, n_weights);
            return MCR_ERR_INVALID_ARG;
        }
        char owner[32];
        std::snprintf(owner, sizeof owner, "options[%d].", k);
        if (!glide_weights_valid(owner, weights + (size_t)o.first_weight, o.n_weights)) return MCR_ERR_INVALID_ARG;
    }
    return MCR_OK;
}
// The shape of a glide probe: MCR_OK with *d, *lmax = plan_level_fanout's (a single option included), or MCR_ERR_UNSUPPORTED with
// a message that says what the glide fan-out does not cover -- the family has no per-option route behind it.  Host only.
static int plan_glide_fanout(const mcr_params* p, const mcr_rng* rng, uint64_t n_paths, int32_t wm, int32_t n_options, int32_t n_weights,
                             DevParams* d, int* lmax) {
    auto unsupported = [](const char* why) { set_error("glide probe: %s is not supported under a glide path", why); return MCR_ERR_UNSUPPORTED; };
    if (rng->kind == MCR_RNG_NUMPY) return unsupported("the NumPy stream");
    if (rng->kind != MCR_RNG_PHILOX) return unsupported("the history stream");
    if (n_paths > ((uint64_t)1 << 31)) return unsupported("a range of more than 2^31 paths");
    const uint64_t min_waves = fanout_min_waves("MCR_GLIDE_FANOUT_MIN_WAVES");
    if ((n_paths + 63) / 64 < min_waves) return unsupported("a range of fewer than MCR_GLIDE_FANOUT_MIN_WAVES path-wavefronts");
    // (a record names its table by a 32-bit distance in doubles: records and weights of one call stay below 2^31 doubles)
    if ((int64_t)n_options * (int64_t)(sizeof(GlideRecord) / sizeof(double)) + (int64_t)n_weights > (int64_t)INT32_MAX) return unsupported("a table of 2^31 doubles or more");
    const int rc = plan_level_fanout(p, rng, n_paths, wm, n_options, min_waves, d, lmax, false, -1, nullptr, 1);
    if (rc != MCR_ERR_UNSUPPORTED) return rc;
    DevParams probe;
    if (derive_params(p, wm, &probe) == MCR_OK) {
        if (needs_exact_month(probe)) return unsupported("the exact month");
        if (probe.n_extra_streams > 0) return unsupported("a stream list longer than MCR_INLINE_STREAMS (the generic variant)");
    }
    return unsupported("a plan whose lock slots do not fit LDS (the generic variant)");
}
// Several glide paths over the same paths, Philox stream (PHASE 13).  The device table is the caller's records, each naming its
// table by the distance in doubles from the record itself (GlideRecord), and the caller's weights behind the last record: group
// g's launch, which gets the table at its first record, needs nothing else.  Of everything derive_params gives the block only
// alloc1 / alloc2 depend on a weight, as in PHASE 12.  `d`, `lmax`: plan_glide_fanout's.
static thread_local int g_last_glide_fanout_launches = 0;   // (mcr_probe_glide_paths_last_fanout_launches)
static int probe_glide_paths_fanout(const DevParams& d, int lmax, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                    const double* weights, int32_t n_weights, const mcr_glide_option* options, int32_t n_options,
                                    uint64_t* counts, hipStream_t stream, uint64_t* masks, const mcr_option_outcomes* rows) {
    constexpr size_t kRecDoubles = sizeof(GlideRecord) / sizeof(double);
    std::vector<GlideRecord> host((size_t)n_options + ((size_t)n_weights + kRecDoubles - 1) / kRecDoubles);
    for (int32_t k = 0; k < n_options; ++k) {
        const mcr_glide_option& o = options[k];
        host[(size_t)k] = GlideRecord{o.initial_balance, o.monthly_contribution, o.monthly_expenses,
                                      (int32_t)((int64_t)(n_options - k) * (int64_t)kRecDoubles + (int64_t)o.first_weight), o.n_weights};
    }
    if (n_weights > 0) std::memcpy((void*)(host.data() + n_options), weights, (size_t)n_weights * sizeof(double));
    return launch_record_fanout(d, lmax, rng, stream_id, path_begin, n_paths, host.data(), n_options, counts, stream, masks, rows,
                                &g_last_glide_fanout_launches, "glide fan-out probe",
                                [&](const KernelIO& fio, int, dim3 grid, dim3 block, size_t lds, const DevParams* table) {
        for_tax_variant(d, [&](auto T, auto A) {
            for_bool(rows != nullptr, [&](auto O) {
                hipLaunchKernelGGL((path_kernel<0, 0, decltype(T)::value, decltype(A)::value, false, 13, true, false, kExactMonthDefault, 0, 0, 0, decltype(O)::value>),
                                   grid, block, lds, stream, d, fio, table);
            });
        });
    }, (size_t)n_weights * sizeof(double));
}
// mcr_probe_glide_paths_rng (jo == nullptr, rows == nullptr), mcr_probe_glide_paths_joint_rng and
// mcr_probe_glide_paths_outcomes_rng, their arguments checked.  The shape is decided before a device is entered and before an
// output is touched; run_probe_routes then has the fan-out alone (a single option too: `fan_one`), and its per-option route,
// reached only when the table's allocation is refused, answers MCR_ERR_UNSUPPORTED.
static int probe_glide_paths(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                             int32_t working_months, const double* weights, int32_t n_weights, const mcr_glide_option* options,
                             int32_t n_options, uint64_t* counts, const JointOut* jo, const mcr_option_outcomes* rows, int device, void* hip_stream) {
    DevParams d;
    int lmax = 0;
    if (n_paths > 0) { if (int rc = plan_glide_fanout(p, rng, n_paths, working_months, n_options, n_weights, &d, &lmax)) return rc; }
    MCR_ENTER_DEVICE(device);
    const hipStream_t main = (hipStream_t)hip_stream;
    int rc = zero_counters(counts, (size_t)n_options, main);
    if (rc != MCR_OK) return rc;
    if (n_paths == 0) return jo ? launch_joint_counts(nullptr, n_options, 0, jo->joint, jo->extremes, main) : MCR_OK;   // (an empty range: zeroes)
    auto launch_option = [&](int, hipStream_t, uint8_t*, double*, double*) {
        set_error("glide probe: the device table could not be allocated, and a glide path has no per-option launch");
        return (int)MCR_ERR_UNSUPPORTED;
    };
    auto fanout = [&](uint64_t* masks, const mcr_option_outcomes* fan_rows) {
        return probe_glide_paths_fanout(d, lmax, rng, stream_id, path_begin, n_paths, weights, n_weights, options, n_options, counts, main, masks, fan_rows);
    };
    return run_probe_routes(device, main, n_options, n_paths, jo, rows, fanout, launch_option, true);
}

int mcr_probe_glide_paths_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const double* weights, int32_t n_weights,
                              const mcr_glide_option* options, int32_t n_options, uint64_t* counts, int device, void* hip_stream) {
    g_last_glide_fanout_launches = 0;
    if (int rc = check_glide_probe(p, rng, working_months, weights, n_weights, options, n_options, counts)) return rc;
    if (n_options == 0) return MCR_OK;
    return probe_glide_paths(p, rng, stream_id, path_begin, n_paths, working_months, weights, n_weights, options, n_options, counts, nullptr, nullptr,
                             device, hip_stream);
}

int mcr_probe_glide_paths_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                    uint64_t n_paths, int32_t working_months, const double* weights, int32_t n_weights,
                                    const mcr_glide_option* options, int32_t n_options, uint64_t* counts, uint64_t* masks,
                                    uint64_t* joint, uint64_t* extremes, int device, void* hip_stream) {
    g_last_glide_fanout_launches = 0;
    if (int rc = check_joint_args(n_options, joint)) return rc;
    if (int rc = check_glide_probe(p, rng, working_months, weights, n_weights, options, n_options, counts)) return rc;
    if (n_options == 0) return MCR_OK;
    const JointOut jo{masks, joint, extremes};
    return probe_glide_paths(p, rng, stream_id, path_begin, n_paths, working_months, weights, n_weights, options, n_options, counts, &jo, nullptr,
                             device, hip_stream);
}

int mcr_probe_glide_paths_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                       uint64_t n_paths, int32_t working_months, const double* weights, int32_t n_weights,
                                       const mcr_glide_option* options, int32_t n_options, uint64_t* counts,
                                       const mcr_option_outcomes* rows, int device, void* hip_stream) {
    g_last_glide_fanout_launches = 0;
    if (int rc = check_outcome_args(&rows, n_paths)) return rc;
    if (int rc = check_glide_probe(p, rng, working_months, weights, n_weights, options, n_options, counts)) return rc;
    if (n_options == 0) return MCR_OK;
    return probe_glide_paths(p, rng, stream_id, path_begin, n_paths, working_months, weights, n_weights, options, n_options, counts, nullptr, rows,
                             device, hip_stream);
}

int mcr_probe_glide_paths_last_fanout_launches(void) { return g_last_glide_fanout_launches; }

// Everything launch_rule refuses of a launch's shape, for a probe that has no route behind the rule kernels: `who` heads the
// message ("spending rule" gives launch_rule's own words).  `d` = derive_params' block of the probed month; `summary`: the
// launches behind the probe are summary launches.
static int refuse_rule_shapes(const char* who, const mcr_params* p, const mcr_rng* rng, uint64_t path_begin, uint64_t n_paths, DevParams& d,
                              bool summary) {
    if (n_paths > (uint64_t)INT32_MAX * kBlock) { set_error("n_paths too large for one launch"); return MCR_ERR_INVALID_ARG; }
    if (path_begin + n_paths < path_begin) { set_error("path range overflows 64 bits"); return MCR_ERR_INVALID_ARG; }
    if (rng->kind == MCR_RNG_NUMPY) { set_error("%s: the NumPy stream is not supported (the engine's own stream only)", who); return MCR_ERR_UNSUPPORTED; }
    if (rng->kind == MCR_RNG_HISTORY) { set_error("%s: the history stream is not supported (the engine's own stream only)", who); return MCR_ERR_UNSUPPORTED; }
    if (p->n_streams > MCR_INLINE_STREAMS && d.n_extra_streams > 0) {
        set_error("%s: %d income streams need the generic variant (at most %d are supported)", who, (int)p->n_streams, MCR_INLINE_STREAMS);
        return MCR_ERR_UNSUPPORTED;
    }
    if (needs_generic_variant(d)) { set_error("%s: the exact month (a realized-gains rate above 1 - 1e-6) needs the generic variant, which is not supported", who); return MCR_ERR_UNSUPPORTED; }
    size_t lds = 0;
    const int rc = plan_path_kernel_lds(d, summary ? 1 : 0, MCR_RNG_PHILOX, false, false, 0, &lds);
    if (rc != MCR_OK) return rc;
    if (d.n_lock_slots < d.n_lock_slots_total) {
        set_error("%s: %d frozen income streams exceed the LDS budget and need the generic variant, which is not supported", who, (int)d.n_lock_slots_total);
        return MCR_ERR_UNSUPPORTED;
    }
    return MCR_OK;
}

// What the rule probes check on the host, before the device and their outputs are touched: the block and the month, the stream,
// every record (the message names options[k].<field> / options[k].rule.<field>), and everything launch_rule refuses -- there is
// no route behind the rule kernels.  `summary`: the per-option route's launches are summary launches (joint, outcomes).
static int check_rule_probe(const mcr_params* p, const mcr_rng* rng, uint64_t path_begin, uint64_t n_paths, int32_t working_months,
                            const mcr_rule_option* options, int32_t n_options, const uint64_t* counts, bool summary) {
    if (n_options < 0) { set_error("n_options %d must be >= 0", n_options); return MCR_ERR_INVALID_ARG; }
    if (n_options == 0) return MCR_OK;
    if (!options || !counts) { set_error("null options / counts"); return MCR_ERR_INVALID_ARG; }
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, working_months, &d, &extra);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    for (int32_t k = 0; k < n_options; ++k) {
        if (!amounts_valid("options", k, options[k])) return MCR_ERR_INVALID_ARG;
        if (validate_spending_rule(&options[k].rule) != MCR_OK) {
            // "spending rule: <field> = ..." -> "options[k].rule.<field> = ..."
            const std::string msg = g_err;
            const size_t at = msg.find(": ");
            set_error("options[%d].rule.%s", k, at == std::string::npos ? msg.c_str() : msg.c_str() + at + 2);
            return MCR_ERR_INVALID_ARG;
        }
    }
    return refuse_rule_shapes("rule probe", p, rng, path_begin, n_paths, d, summary);
}

// mcr_probe_rules_rng (jo == nullptr, rows == nullptr), mcr_probe_rules_joint_rng and mcr_probe_rules_outcomes_rng, on the entered
// device, their arguments checked (check_rule_probe)
static int probe_rules(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                       int32_t working_months, const mcr_rule_option* options, int32_t n_options, uint64_t* counts, uint64_t* year_counts,
                       const JointOut* jo, const mcr_option_outcomes* rows, int device, hipStream_t main) {
    if (n_options == 0) return MCR_OK;
    int rc = zero_counters(counts, (size_t)n_options, main);
    if (rc != MCR_OK) return rc;
    const size_t year_block = (size_t)p->retirement_years * MCR_RULE_N_COUNTS;   // one option's year counts
    if (year_counts) {
        const hipError_t e = hipMemsetAsync(year_counts, 0, sizeof(uint64_t) * year_block * (size_t)n_options, main);
        if (e != hipSuccess) return hip_fail(e, "rule probe year counts memset");
    }
    mcr_params q = *p;
    auto launch_option = [&](int k, hipStream_t s, uint8_t* success, double* final_balance, double* years_to_ruin) {
        const mcr_rule_option& r = options[k];
        q.initial_balance = r.initial_balance; q.monthly_contribution = r.monthly_contribution; q.monthly_expenses = r.monthly_expenses;
        const mcr_outputs o = counters_and_columns(counts + (size_t)k * MCR_N_COUNTERS, success, final_balance, years_to_ruin);
        const mcr_rule_outputs ro{year_counts ? year_counts + (size_t)k * year_block : nullptr, nullptr, 0};
        return launch_rule(&q, rng, stream_id, path_begin, n_paths, working_months, &r.rule, &o, &ro, s);
    };
    auto fanout = [&](uint64_t* masks, const mcr_option_outcomes* fan_rows) {
        return probe_rules_fanout(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, year_counts, main, masks, fan_rows);
    };
    return run_probe_routes(device, main, n_options, n_paths, jo, rows, fanout, launch_option);
}

int mcr_probe_rules_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                        uint64_t n_paths, int32_t working_months, const mcr_rule_option* options, int32_t n_options,
                        uint64_t* counts, uint64_t* year_counts, int device, void* hip_stream) {
    g_last_rule_fanout_launches = 0;
    if (int rc = check_rule_probe(p, rng, path_begin, n_paths, working_months, options, n_options, counts, false)) return rc;
    MCR_ENTER_DEVICE(device);
    return probe_rules(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, year_counts, nullptr, nullptr, device,
                       (hipStream_t)hip_stream);
}

int mcr_probe_rules_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const mcr_rule_option* options, int32_t n_options,
                              uint64_t* counts, uint64_t* year_counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes,
                              int device, void* hip_stream) {
    g_last_rule_fanout_launches = 0;
    if (int rc = check_joint_args(n_options, joint)) return rc;
    if (int rc = check_rule_probe(p, rng, path_begin, n_paths, working_months, options, n_options, counts, true)) return rc;
    MCR_ENTER_DEVICE(device);
    const JointOut jo{masks, joint, extremes};
    return probe_rules(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, year_counts, &jo, nullptr, device,
                       (hipStream_t)hip_stream);
}

int mcr_probe_rules_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                 uint64_t n_paths, int32_t working_months, const mcr_rule_option* options, int32_t n_options,
                                 uint64_t* counts, uint64_t* year_counts, const mcr_option_outcomes* rows,
                                 int device, void* hip_stream) {
    g_last_rule_fanout_launches = 0;
    if (int rc = check_outcome_args(&rows, n_paths)) return rc;
    if (int rc = check_rule_probe(p, rng, path_begin, n_paths, working_months, options, n_options, counts, rows != nullptr)) return rc;
    MCR_ENTER_DEVICE(device);
    return probe_rules(p, rng, stream_id, path_begin, n_paths, working_months, options, n_options, counts, year_counts, nullptr, rows, device,
                       (hipStream_t)hip_stream);
}

int mcr_probe_rules_last_fanout_launches(void) { return g_last_rule_fanout_launches; }

int mcr_probe_grid_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                       uint64_t n_paths, const int32_t* working_months, int32_t n_candidates,
                       const double* monthly_expenses, int32_t n_levels, uint64_t* counts, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    if (n_candidates < 0 || n_levels < 0) { set_error("n_candidates %d / n_levels %d must be >= 0", n_candidates, n_levels); return MCR_ERR_INVALID_ARG; }
    if (n_candidates == 0 || n_levels == 0) return MCR_OK;
    if (!working_months || !monthly_expenses || !counts) { set_error("null months / levels / counts"); return MCR_ERR_INVALID_ARG; }
    int rc = validate_months(p, working_months, n_candidates);
    if (rc != MCR_OK) return rc;
    rc = check_rng(rng);
    if (rc != MCR_OK) return rc;
    const size_t n_cells = (size_t)n_candidates * (size_t)n_levels;
    for (size_t k = 0; k < n_cells; ++k)
        if (!(std::isfinite(monthly_expenses[k]) && monthly_expenses[k] >= 0.0)) {
            set_error("monthly_expenses[%d][%d] = %g: must be finite and >= 0 (config.py:59)", (int)(k / (size_t)n_levels),
                      (int)(k % (size_t)n_levels), monthly_expenses[k]);
            return MCR_ERR_INVALID_ARG;
        }
    bool one_month = true;
    for (int32_t c = 1; c < n_candidates; ++c) one_month = one_month && working_months[c] == working_months[0];
    // one distinct month: the rows' levels, concatenated, are one expense probe whose counters are the [rows][levels] block
    if (one_month && n_cells <= (size_t)INT32_MAX)
        return mcr_probe_expenses_rng(p, rng, stream_id, path_begin, n_paths, working_months[0], monthly_expenses, (int32_t)n_cells,
                                      counts, device, hip_stream);
    hipStream_t main = (hipStream_t)hip_stream;
    rc = zero_counters(counts, n_cells, main);
    if (rc != MCR_OK) return rc;
    rc = probe_grid_shared(p, rng, stream_id, path_begin, n_paths, working_months, n_candidates, monthly_expenses, n_levels, counts, main);
    if (rc != MCR_ERR_UNSUPPORTED) return rc;     // (unsupported shape / allocation refused: the per-month route below)
    rc = MCR_OK;
    for (int32_t c = 0; c < n_candidates && rc == MCR_OK; ++c)
        rc = mcr_probe_expenses_rng(p, rng, stream_id, path_begin, n_paths, working_months[c], monthly_expenses + (size_t)c * n_levels,
                                    n_levels, counts + (size_t)c * n_levels * MCR_N_COUNTERS, device, hip_stream);
    return rc;
}

// The grid under one spending rule.  Everything is checked on the host before a device is looked for: the months (and, month by
// month, whatever launch_rule refuses, by its words), every level, the rule.  Then the shared route (probe_rule_grid_shared) or,
// where it answers MCR_ERR_UNSUPPORTED (one distinct month, more than MCR_MAX_PROBE_CANDIDATES of them, a launch below the
// fan-out's minimum wave count, the allocation refused), one rule probe per row over the row's levels.
int mcr_probe_rule_grid_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                            uint64_t n_paths, const int32_t* working_months, int32_t n_candidates,
                            const double* monthly_expenses, int32_t n_levels, const mcr_spending_rule* rule,
                            uint64_t* counts, uint64_t* year_counts, int device, void* hip_stream) {
    g_last_rule_grid_fanout_launches = 0;
    if (n_candidates < 0 || n_levels < 0) { set_error("n_candidates %d / n_levels %d must be >= 0", n_candidates, n_levels); return MCR_ERR_INVALID_ARG; }
    if (n_candidates == 0 || n_levels == 0) return MCR_OK;
    if (!working_months || !monthly_expenses || !counts) { set_error("null months / levels / counts"); return MCR_ERR_INVALID_ARG; }
    int rc = validate_months(p, working_months, n_candidates);
    if (rc != MCR_OK) return rc;
    if ((rc = check_rng(rng)) != MCR_OK) return rc;
    const size_t n_cells = (size_t)n_candidates * (size_t)n_levels;
    for (size_t k = 0; k < n_cells; ++k)
        if (!(std::isfinite(monthly_expenses[k]) && monthly_expenses[k] >= 0.0)) {
            set_error("monthly_expenses[%d][%d] = %g: must be finite and >= 0 (config.py:59)", (int)(k / (size_t)n_levels),
                      (int)(k % (size_t)n_levels), monthly_expenses[k]);
            return MCR_ERR_INVALID_ARG;
        }
    if ((rc = validate_spending_rule(rule)) != MCR_OK) return rc;
    for (int32_t c = 0; c < n_candidates; ++c) {
        DevParams d;
        std::vector<DevStream> extra;
        if ((rc = derive_params(p, working_months[c], &d, &extra)) != MCR_OK) return rc;
        if ((rc = refuse_rule_shapes("spending rule", p, rng, path_begin, n_paths, d, false)) != MCR_OK) return rc;
    }
    MCR_ENTER_DEVICE(device);
    hipStream_t main = (hipStream_t)hip_stream;
    const size_t year_block = (size_t)p->retirement_years * MCR_RULE_N_COUNTS;   // one cell's year counts
    rc = zero_counters(counts, n_cells, main);
    if (rc != MCR_OK) return rc;
    if (year_counts) {
        const hipError_t e = hipMemsetAsync(year_counts, 0, sizeof(uint64_t) * year_block * n_cells, main);
        if (e != hipSuccess) return hip_fail(e, "rule grid probe year counts memset");
    }
    rc = probe_rule_grid_shared(p, rng, stream_id, path_begin, n_paths, working_months, n_candidates, monthly_expenses, n_levels, rule,
                                counts, year_counts, main);
    if (rc != MCR_ERR_UNSUPPORTED) return rc;     // (unsupported shape / allocation refused: the per-row route below)
    std::vector<mcr_rule_option> options((size_t)n_levels);
    rc = MCR_OK;
    for (int32_t c = 0; c < n_candidates && rc == MCR_OK; ++c) {
        for (int32_t k = 0; k < n_levels; ++k)
            options[(size_t)k] = mcr_rule_option{p->initial_balance, p->monthly_contribution, monthly_expenses[(size_t)c * n_levels + k], *rule};
        rc = mcr_probe_rules_rng(p, rng, stream_id, path_begin, n_paths, working_months[c], options.data(), n_levels,
                                 counts + (size_t)c * n_levels * MCR_N_COUNTERS,
                                 year_counts ? year_counts + (size_t)c * n_levels * year_block : nullptr, device, hip_stream);
    }
    return rc;
}

int mcr_probe_rule_grid_last_fanout_launches(void) { return g_last_rule_grid_fanout_launches; }

int mcr_run_batch(const mcr_params* p, uint64_t seed, uint32_t stream_id, uint64_t path_begin,
                  uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                  const mcr_outputs* out, int device, void* hip_stream) {
    const mcr_rng r = philox_rng(seed);
    return mcr_run_batch_rng(p, &r, stream_id, path_begin, n_paths, working_months, injected_shocks, out, device, hip_stream);
}

int mcr_run_batch_host(const mcr_params* p, uint64_t seed, uint32_t stream_id, uint64_t path_begin,
                       uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                       const mcr_outputs* out, int device) {
    const mcr_rng r = philox_rng(seed);
    return mcr_run_batch_host_rng(p, &r, stream_id, path_begin, n_paths, working_months, injected_shocks, out, device);
}

// One host-buffer batch on `device` (HostCall): the per-path columns and trajectory slabs come straight back to the caller
static int run_batch_host_on(int device, const mcr_params* p, const mcr_rng* rng_in, uint32_t stream_id, uint64_t path_begin,
                             uint64_t n_paths, int32_t working_months, const double* injected_shocks, const mcr_outputs* out) {
    MCR_ENTER_DEVICE(device);
    int rc = check_rng(rng_in, true);
    if (rc != MCR_OK) return rc;
    mcr_sizes sz;
    rc = query_sizes(p, working_months, &sz);
    if (rc != MCR_OK) return rc;
    if (!out) { set_error("null outputs"); return MCR_ERR_INVALID_ARG; }
    if (n_paths == 0) return MCR_OK;
    const int64_t hstride = out->path_stride > 0 ? out->path_stride : (int64_t)n_paths;
    if ((uint64_t)hstride < n_paths) { set_error("path_stride < n_paths"); return MCR_ERR_INVALID_ARG; }
    const size_t n = (size_t)n_paths;
    mcr_outputs d = {};
    d.path_stride = (int64_t)((n + 63) / 64 * 64);  // device rows padded to whole wavefronts
    HostCall call;
    auto vec = [&](double* host, double** dev) { call.plan(dev, host, n * sizeof(double), false, true); };
    auto mat = [&](double* host, double** dev, int rows) {
        call.plan_rows(dev, host, (size_t)rows, n * sizeof(double), (size_t)d.path_stride * sizeof(double), (size_t)hstride * sizeof(double));
    };
    vec(out->start_balance, &d.start_balance);
    vec(out->final_balance, &d.final_balance);
    vec(out->years_to_ruin, &d.years_to_ruin);
    vec(out->first_year_gross_withdrawal, &d.first_year_gross_withdrawal);
    vec(out->first_year_real_gross_withdrawal, &d.first_year_real_gross_withdrawal);
    vec(out->inflation_at_retirement, &d.inflation_at_retirement);
    call.plan(&d.success, out->success, n, false, true);
    mat(out->trajectory, &d.trajectory, sz.trajectory_len);
    mat(out->real_trajectory, &d.real_trajectory, sz.trajectory_len);
    mat(out->withdrawal_rate_trajectory, &d.withdrawal_rate_trajectory, sz.retirement_years);
    if (out->hist_bins && out->hist_n_bins != 0) {   // in-kernel final-balance histogram on the caller's edges
        const int nb = out->hist_n_bins;
        if (nb < 0 || nb > MCR_MAX_HIST_BINS || !out->hist_edges) { set_error("hist_bins requested with hist_n_bins = %d (1..%d) / null hist_edges", nb, MCR_MAX_HIST_BINS); return MCR_ERR_INVALID_ARG; }
        if ((rc = check_edges_host("hist_edges", out->hist_edges, nb)) != MCR_OK) return rc;   // host pointer: the edges can be checked here
        d.hist_n_bins = nb;
        call.plan(&d.hist_edges, out->hist_edges, (size_t)(nb + 1) * sizeof(double), true, false);
    }
    // accumulated counters: the device copy starts from the caller's current values
    for (const IntBlock& b : output_blocks(sz, out, &d)) call.plan(b.dst, *b.src, b.n * sizeof(uint64_t), true, true);
    double* d_inj = nullptr;
    call.plan(&d_inj, injected_shocks, n * (size_t)sz.shock_rows * 3 * sizeof(double), true, false);
    mcr_rng rng = *rng_in;
    call.plan_rng(&rng, n_paths);
    if ((rc = call.begin(device, "device allocation (host-buffer batch)")) != MCR_OK) return rc;
    rc = launch_paths(p, &rng, stream_id, path_begin, n_paths, working_months, d_inj, &d, call.stream());
    return call.finish(rc, false, "path_kernel execution");
}

// The same batch sharded over several devices (run_sharded): a shard's per-path columns are the caller's, shifted to its range
static int run_batch_host_multi(const int32_t* devices, int32_t n_devices, const mcr_params* p, const mcr_rng* rng_in,
                                uint32_t stream_id, uint64_t path_begin, uint64_t n_paths, int32_t working_months,
                                const double* injected_shocks, const mcr_outputs* out) {
    if (!out || !rng_in) { set_error("null outputs / rng"); return MCR_ERR_INVALID_ARG; }
    mcr_sizes sz;
    int rc = query_sizes(p, working_months, &sz);
    if (rc != MCR_OK) return rc;
    const int64_t hstride = out->path_stride > 0 ? out->path_stride : (int64_t)n_paths;
    return run_sharded(devices, n_devices, n_paths, *out,
        [&](mcr_outputs* shard) { return output_blocks(sz, out, shard); },
        [&](int device, uint64_t begin, uint64_t count, const mcr_outputs& shard) {
            mcr_outputs o = shard;    // host pointers of this shard's columns
            auto shift = [&](double*& ptr) { if (ptr) ptr += begin; };
            shift(o.start_balance); shift(o.final_balance); shift(o.years_to_ruin);
            shift(o.first_year_gross_withdrawal); shift(o.first_year_real_gross_withdrawal); shift(o.inflation_at_retirement);
            if (o.success) o.success += begin;
            shift(o.trajectory); shift(o.real_trajectory); shift(o.withdrawal_rate_trajectory);
            o.path_stride = hstride;
            mcr_rng r = *rng_in;
            if (r.path_seeds) r.path_seeds += begin;
            const double* inj = injected_shocks ? injected_shocks + (size_t)begin * (size_t)sz.shock_rows * 3u : nullptr;
            return run_batch_host_on(device, p, &r, stream_id, path_begin + begin, count, working_months, inj, &o);
        });
}

int mcr_run_batch_host_rng(const mcr_params* p, const mcr_rng* rng_in, uint32_t stream_id, uint64_t path_begin,
                           uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                           const mcr_outputs* out, int device) {
    const int rc = check_history_host(rng_in);
    if (rc != MCR_OK) return rc;
    if (device == MCR_DEVICE_ALL)
        return run_batch_host_multi(nullptr, 0, p, rng_in, stream_id, path_begin, n_paths, working_months, injected_shocks, out);
    return run_batch_host_on(device, p, rng_in, stream_id, path_begin, n_paths, working_months, injected_shocks, out);
}

int mcr_run_batch_multi_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                 uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                                 const mcr_outputs* out, const int32_t* devices, int32_t n_devices) {
    const int rc = check_history_host(rng);
    if (rc != MCR_OK) return rc;
    return run_batch_host_multi(devices, n_devices, p, rng, stream_id, path_begin, n_paths, working_months, injected_shocks, out);
}

// ---- yearly bins -------------------------------------------------------------------------------------------------------
int mcr_run_year_bins_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                          int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb, int device, void* hip_stream) {
    MCR_ENTER_DEVICE(device);
    return launch_year_bins(p, rng, stream_id, path_begin, n_paths, working_months, out, yb, (hipStream_t)hip_stream);
}

// Everything that can be checked on the host, before any device work
static int check_year_bins_host(const mcr_params* p, const mcr_rng* rng, int32_t working_months, const mcr_outputs* out,
                                const mcr_year_bins* yb, mcr_sizes* sz) {
    int rc = check_rng(rng, true);
    if (rc != MCR_OK) return rc;
    if ((rc = query_sizes(p, working_months, sz)) != MCR_OK) return rc;
    if ((rc = validate_params(p)) != MCR_OK) return rc;
    if ((rc = check_year_bins(out, yb)) != MCR_OK) return rc;
    return check_year_bins_edges_host(yb, "hist_edges", out->hist_bins && out->hist_n_bins > 0 ? out->hist_edges : nullptr, out->hist_n_bins);
}
// The buffers every yearly-bins form plans: the integer blocks of `host` (up and down) and the edges of the requested tables (up)
static void plan_year_bins(HostCall& call, const mcr_sizes& sz, const YearBinsOut& host, YearBinsOut* dev) {
    dev->y.n_bins = host.y.n_bins; dev->y.n_wr_bins = host.y.n_wr_bins;
    for (const IntBlock& b : year_bins_blocks(sz, host, dev)) call.plan(b.dst, *b.src, b.n * sizeof(uint64_t), true, true);
    if (wants_balance_tables(&host.y)) call.plan(&dev->y.edges, host.y.edges, (size_t)(host.y.n_bins + 1) * sizeof(double), true, false);
    if (host.y.wr_bins) call.plan(&dev->y.wr_edges, host.y.wr_edges, (size_t)(host.y.n_wr_bins + 1) * sizeof(double), true, false);
}
// One device (HostCall): the tables come back through staging copies, so the caller's stay untouched unless the whole call succeeds
static int run_year_bins_host_on(int device, const mcr_params* p, const mcr_rng* rng_in, uint32_t stream_id, uint64_t path_begin,
                                 uint64_t n_paths, int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb) {
    MCR_ENTER_DEVICE(device);
    mcr_sizes sz;
    int rc = check_year_bins_host(p, rng_in, working_months, out, yb, &sz);
    if (rc != MCR_OK) return rc;
    if (n_paths == 0) return MCR_OK;
    const YearBinsOut host = {*out, *yb};
    YearBinsOut d = {};
    HostCall call;
    plan_year_bins(call, sz, host, &d);
    if (out->hist_bins && out->hist_n_bins > 0) {
        d.o.hist_n_bins = out->hist_n_bins;
        call.plan(&d.o.hist_edges, out->hist_edges, (size_t)(out->hist_n_bins + 1) * sizeof(double), true, false);
    }
    mcr_rng rng = *rng_in;
    call.plan_rng(&rng, n_paths);
    if ((rc = call.begin(device, "device allocation (yearly bins)")) != MCR_OK) return rc;
    rc = launch_year_bins(p, &rng, stream_id, path_begin, n_paths, working_months, &d.o, &d.y, call.stream());
    return call.finish(rc, true, "path_kernel execution (yearly bins)");
}

// Sharded over a device list (run_sharded): a shard has no per-path pointer but its seeds
static int run_year_bins_host_multi(const int32_t* devices, int32_t n_devices, const mcr_params* p, const mcr_rng* rng_in, uint32_t stream_id,
                                    uint64_t path_begin, uint64_t n_paths, int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb) {
    if (!rng_in) { set_error("null rng"); return MCR_ERR_INVALID_ARG; }
    mcr_sizes sz;
    int rc = check_year_bins_host(p, rng_in, working_months, out, yb, &sz);
    if (rc != MCR_OK) return rc;
    const YearBinsOut caller = {*out, *yb};
    return run_sharded(devices, n_devices, n_paths, caller,
        [&](YearBinsOut* shard) { return year_bins_blocks(sz, caller, shard); },
        [&](int device, uint64_t begin, uint64_t count, const YearBinsOut& shard) {
            mcr_rng r = *rng_in;
            if (r.path_seeds) r.path_seeds += begin;
            return run_year_bins_host_on(device, p, &r, stream_id, path_begin + begin, count, working_months, &shard.o, &shard.y);
        });
}

int mcr_run_year_bins_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                               int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb, int device) {
    if (device == MCR_DEVICE_ALL) return run_year_bins_host_multi(nullptr, 0, p, rng, stream_id, path_begin, n_paths, working_months, out, yb);
    return run_year_bins_host_on(device, p, rng, stream_id, path_begin, n_paths, working_months, out, yb);
}

int mcr_run_year_bins_multi_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                     int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb, const int32_t* devices,
                                     int32_t n_devices) {
    return run_year_bins_host_multi(devices, n_devices, p, rng, stream_id, path_begin, n_paths, working_months, out, yb);
}

// ---- yearly bins under a spending rule ---------------------------------------------------------------------------------
// (both entry points check every argument before they look for a device: a refusal names its field with no GPU in the box)
int mcr_run_rule_year_bins_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                               int32_t working_months, const mcr_spending_rule* rule, const mcr_outputs* out, const mcr_year_bins* yb,
                               const mcr_rule_year_bins* rule_yb, int device, void* hip_stream) {
    DevParams d;
    size_t lds = 0;
    const int rc = plan_rule_year_bins(p, rng, path_begin, n_paths, working_months, rule, out, yb, rule_yb, &d, &lds);
    if (rc != MCR_OK) return rc;
    MCR_ENTER_DEVICE(device);
    return launch_rule_year_bins(p, rng, stream_id, path_begin, n_paths, working_months, rule, out, yb, rule_yb, (hipStream_t)hip_stream);
}

// HOST pointers, one device: run_year_bins_host_on's plan with both rule tables and the multiplier edges added
int mcr_run_rule_year_bins_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                    int32_t working_months, const mcr_spending_rule* rule, const mcr_outputs* out, const mcr_year_bins* yb,
                                    const mcr_rule_year_bins* rule_yb, int device) {
    mcr_sizes sz;
    DevParams dp;
    size_t lds = 0;
    int rc = check_rng(rng, true);
    if (rc != MCR_OK) return rc;
    if ((rc = query_sizes(p, working_months, &sz)) != MCR_OK) return rc;
    if ((rc = validate_params(p)) != MCR_OK) return rc;
    if ((rc = plan_rule_year_bins(p, rng, path_begin, n_paths, working_months, rule, out, yb, rule_yb, &dp, &lds)) != MCR_OK) return rc;
    if ((rc = check_year_bins_edges_host(yb, "m_edges", rule_yb->multiplier_bins ? rule_yb->m_edges : nullptr, rule_yb->n_m_bins)) != MCR_OK) return rc;
    MCR_ENTER_DEVICE(device);
    if (n_paths == 0) return MCR_OK;
    const YearBinsOut host = {*out, *yb};
    YearBinsOut d = {};
    mcr_rule_year_bins dr = {};
    dr.n_m_bins = rule_yb->n_m_bins;
    HostCall call;
    plan_year_bins(call, sz, host, &d);
    const size_t ry = (size_t)sz.retirement_years;
    call.plan(&dr.year_counts, rule_yb->year_counts, ry * MCR_RULE_N_COUNTS * sizeof(uint64_t), true, true);
    if (rule_yb->multiplier_bins) {
        call.plan(&dr.multiplier_bins, rule_yb->multiplier_bins, ry * ((size_t)rule_yb->n_m_bins + 2) * sizeof(uint64_t), true, true);
        call.plan(&dr.m_edges, rule_yb->m_edges, (size_t)(rule_yb->n_m_bins + 1) * sizeof(double), true, false);
    }
    if ((rc = call.begin(device, "device allocation (rule yearly bins)")) != MCR_OK) return rc;
    rc = launch_rule_year_bins(p, rng, stream_id, path_begin, n_paths, working_months, rule, &d.o, &d.y, &dr, call.stream());
    return call.finish(rc, true, "path_kernel execution (rule yearly bins)");
}

// ---- glide whole-path launches (GLIDE of path_kernel; include/mcr.h: GLIDE PATH) -------------------------------------------
// One table for the whole launch: path_kernel<MODE 0 | 1 | 3, Philox, mask 3, annual-gains tax or not, ..., GLIDE>, six
// instantiations.  Everything is checked on the host before a device is looked for, and everything else a caller can ask for
// is refused by name (launch_rule's list, through refuse_rule_shapes).  `yb` null: a count-only or summary launch, whose `out`
// follows mcr_run_rule_rng's contract; otherwise a yearly-bins launch under check_year_bins' rules.  On success the parameter
// block and the launch's dynamic LDS are planned.
static int plan_glide_run(const mcr_params* p, const mcr_rng* rng, uint64_t path_begin, uint64_t n_paths, int32_t wm, const double* weights,
                          int32_t n_weights, const mcr_outputs* out, const mcr_year_bins* yb, bool host_edges, DevParams* d_out, int* mode_out, size_t* lds) {
    DevParams d;
    std::vector<DevStream> extra;
    int rc = derive_params(p, wm, &d, &extra);
    if (rc != MCR_OK) return rc;
    if ((rc = check_rng(rng, host_edges)) != MCR_OK) return rc;
    if (!weights) { set_error("glide path: null weights"); return MCR_ERR_INVALID_ARG; }
    if (n_weights < 1) { set_error("glide path: n_weights = %d: a glide path has at least one entry", n_weights); return MCR_ERR_INVALID_ARG; }
    if (!glide_weights_valid("", weights, n_weights)) return MCR_ERR_INVALID_ARG;
    if (!out) { set_error(yb ? "null outputs / year bins" : "null outputs"); return MCR_ERR_INVALID_ARG; }
    if (out->trajectory || out->real_trajectory || out->withdrawal_rate_trajectory) {
        set_error("glide path: trajectories are not supported (counters, per-path summary columns and yearly bins only)");
        return MCR_ERR_UNSUPPORTED;
    }
    if (yb) {
        if ((rc = check_year_bins(out, yb)) != MCR_OK) return rc;
        if (host_edges && (rc = check_year_bins_edges_host(yb, nullptr, nullptr, 0)) != MCR_OK) return rc;
    }
    if (out->hist_bins && out->hist_n_bins != 0) { set_error("glide path: the in-kernel histogram (hist_bins) is not supported"); return MCR_ERR_UNSUPPORTED; }
    const bool want_summary = out->start_balance || out->final_balance || out->years_to_ruin || out->first_year_gross_withdrawal ||
                              out->first_year_real_gross_withdrawal || out->inflation_at_retirement || out->success;
    const int mode = yb ? 3 : want_summary ? 1 : 0;
    // (refuse_rule_shapes decides on a count-only or summary plan at the four-resident LDS budget: the rule of the MODE 0 / 1 launches,
    //  and the stricter one where lock columns are concerned -- a yearly-bins launch, which plans again below and may take the whole
    //  workgroup's LDS, is refused here first for a stream list that a count-only launch under the same table would be refused for)
    if ((rc = refuse_rule_shapes("glide path", p, rng, path_begin, n_paths, d, mode == 1)) != MCR_OK) return rc;
    const size_t bins_bytes = yb ? year_bins_lds(wants_balance_tables(yb) ? yb->n_bins : 0, yb->wr_bins ? yb->n_wr_bins : 0) : 0;
    if ((rc = plan_path_kernel_lds(d, mode, MCR_RNG_PHILOX, false, false, 0, lds, bins_bytes)) != MCR_OK) return rc;
    // THIS launch's plan, not refuse_rule_shapes': the edges and row buffers of a yearly-bins launch take LDS that a count-only plan
    // leaves to the lock columns of frozen income streams.  The plain yearly-bins launch then takes its generic form; the glide
    // kernels have none, and would write the columns that do not fit over the counters, edges and cells behind them.  So the
    // launch gives up resident workgroups instead (columns up to the workgroup's own 64 KB), and what does not fit even then is
    // refused by name.
    if (d.n_lock_slots < d.n_lock_slots_total &&
        (rc = plan_path_kernel_lds(d, mode, MCR_RNG_PHILOX, false, false, 0, lds, bins_bytes, 0, true)) != MCR_OK) return rc;
    if (d.n_lock_slots < d.n_lock_slots_total) {
        set_error("glide path: %d frozen income streams exceed the LDS budget beside the yearly tables and need the generic variant, which is not supported",
                  (int)d.n_lock_slots_total);
        return MCR_ERR_UNSUPPORTED;
    }
    *d_out = d;
    *mode_out = mode;
    return MCR_OK;
}
// The launch: device pointers in `out` / `yb`, the table a HOST array.  The record and the weights behind it are one
// stream-ordered device block filled from the host and released behind the launch, like a fan-out's table; the record is
// PHASE 13's (GlideRecord), so the kernel finds its table by the same statement.
static int launch_glide(const DevParams& d, int mode, size_t lds, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                        const double* weights, int32_t n_weights, const mcr_outputs* out, const mcr_year_bins* yb, hipStream_t stream) {
    if (n_paths == 0) return MCR_OK;
    KernelIO io = make_io(rng, nullptr, stream_id, path_begin, n_paths);
    io.out = *out;
    io.out.hist_bins = nullptr; io.out.hist_edges = nullptr; io.out.hist_n_bins = 0;
    if (yb) { io.out.path_stride = (int64_t)n_paths; fill_io_year_bins(io, yb); }
    else if (io.out.path_stride <= 0) io.out.path_stride = (int64_t)n_paths;
    constexpr size_t kRecDoubles = sizeof(GlideRecord) / sizeof(double);
    // (pageable host memory: hipMemcpyAsync has staged it when it returns, as for the fan-outs' tables in SnapshotBlock::attach)
    std::vector<double> host(kRecDoubles + (size_t)n_weights);
    const GlideRecord rec = {d.initial_balance, d.monthly_contribution, d.monthly_expenses, (int32_t)kRecDoubles, n_weights};
    std::memcpy(host.data(), &rec, sizeof rec);
    std::memcpy(host.data() + kRecDoubles, weights, (size_t)n_weights * sizeof(double));
    StreamAlloc table(stream);
    if (!table.alloc(host.size() * sizeof(double))) { set_error("glide path: the device table's allocation was refused"); return MCR_ERR_HIP; }
    hipError_t e = hipMemcpyAsync(table.p, host.data(), host.size() * sizeof(double), hipMemcpyHostToDevice, stream);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((n_paths + kBlock - 1) / kBlock)), block(kBlock);
        for_bool(d.any_annual_tax, [&](auto A) {
            auto go = [&](auto M) {
                hipLaunchKernelGGL((path_kernel<decltype(M)::value, 0, 3, decltype(A)::value, false, 0, false, false, kExactMonthDefault, 0, 0, 0, false, false, 1, false, true>),
                                   grid, block, lds, stream, d, io, (const DevParams*)table.p);
            };
            if (mode == 3) go(std::integral_constant<int, 3>{});
            else if (mode == 1) go(std::integral_constant<int, 1>{});
            else go(std::integral_constant<int, 0>{});
        });
        e = hipGetLastError();
    }
    const hipError_t ef = table.release();
    if (e != hipSuccess) return hip_fail(e, "path_kernel launch (glide path)");
    if (ef != hipSuccess) return hip_fail(ef, "path_kernel launch (glide path): table release");
    return MCR_OK;
}

int mcr_run_glide_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                      int32_t working_months, const double* weights, int32_t n_weights, mcr_outputs* out, int device, void* hip_stream) {
    DevParams d;
    int mode = 0;
    size_t lds = 0;
    const int rc = plan_glide_run(p, rng, path_begin, n_paths, working_months, weights, n_weights, out, nullptr, false, &d, &mode, &lds);
    if (rc != MCR_OK) return rc;
    MCR_ENTER_DEVICE(device);
    return launch_glide(d, mode, lds, rng, stream_id, path_begin, n_paths, weights, n_weights, out, nullptr, (hipStream_t)hip_stream);
}

int mcr_run_glide_year_bins_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                int32_t working_months, const double* weights, int32_t n_weights, const mcr_outputs* out,
                                const mcr_year_bins* yb, int device, void* hip_stream) {
    DevParams d;
    int mode = 0;
    size_t lds = 0;
    if (!yb) { set_error("null outputs / year bins"); return MCR_ERR_INVALID_ARG; }
    const int rc = plan_glide_run(p, rng, path_begin, n_paths, working_months, weights, n_weights, out, yb, false, &d, &mode, &lds);
    if (rc != MCR_OK) return rc;
    MCR_ENTER_DEVICE(device);
    return launch_glide(d, mode, lds, rng, stream_id, path_begin, n_paths, weights, n_weights, out, yb, (hipStream_t)hip_stream);
}

// HOST pointers, one device: run_year_bins_host_on's plan, the launch under the table
int mcr_run_glide_year_bins_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                     int32_t working_months, const double* weights, int32_t n_weights, const mcr_outputs* out,
                                     const mcr_year_bins* yb, int device) {
    mcr_sizes sz;
    DevParams dp;
    int mode = 0;
    size_t lds = 0;
    int rc;
    if (!yb) { set_error("null outputs / year bins"); return MCR_ERR_INVALID_ARG; }
    if ((rc = query_sizes(p, working_months, &sz)) != MCR_OK) return rc;
    if ((rc = validate_params(p)) != MCR_OK) return rc;
    if ((rc = plan_glide_run(p, rng, path_begin, n_paths, working_months, weights, n_weights, out, yb, true, &dp, &mode, &lds)) != MCR_OK) return rc;
    MCR_ENTER_DEVICE(device);
    if (n_paths == 0) return MCR_OK;
    const YearBinsOut host = {*out, *yb};
    YearBinsOut d = {};
    HostCall call;
    plan_year_bins(call, sz, host, &d);
    if ((rc = call.begin(device, "device allocation (glide yearly bins)")) != MCR_OK) return rc;
    rc = launch_glide(dp, mode, lds, rng, stream_id, path_begin, n_paths, weights, n_weights, &d.o, &d.y, call.stream());
    return call.finish(rc, true, "path_kernel execution (glide yearly bins)");
}

int mcr_validate_params(const mcr_params* p) { return validate_params(p); }

// numpy.random.RandomState(seed).choice(n, k, replace=False) without shuffling an n-element array (include/mcr.h).
// MT19937 as NumPy's legacy generator runs it: init_genrand seeding (numpy/random/src/mt19937/mt19937.c: mt19937_seed),
// tempered 32-bit outputs, bounded draws by masked rejection (legacy-distributions.c: legacy_random_interval ->
// random_interval), Fisher-Yates from i = n - 1 down to 1 (_mt19937 / mtrand.pyx: _shuffle_raw).
// Host-only and on the critical path of the class API at large n (10^7 paths: 81 ms in round 3's form, twice the path
// kernel): the generator refills 624 tempered words at a time (plain loops the compiler vectorises), the rejection loop is
// branch-free (a draw is written to J[i] either way, i moves on only when it is accepted: the ~30 % of rejected draws were
// mispredicted branches), and the trace-back keeps its <= 8 tracked positions in one vector register (one compare pair and
// a test per step, AVX2 when the CPU has it).  10^7 paths: 135 -> 44 ms on the build container's Xeon.
extern "C++" {
namespace {
struct Mt19937Block {
    uint32_t mt[624];
    uint32_t out[624];   // the tempered outputs of the current block
    void seed(uint32_t s) {
        mt[0] = s;
        for (int i = 1; i < 624; ++i) mt[i] = 1812433253u * (mt[i - 1] ^ (mt[i - 1] >> 30)) + (uint32_t)i;
    }
    __attribute__((always_inline)) void refill() {      // (inlined into the dispatched cores below: AVX2 code where the CPU has it)
        constexpr uint32_t kUpper = 0x80000000u, kLower = 0x7fffffffu, kMatrix = 0x9908b0dfu;
        uint32_t* m = mt;
        for (int i = 0; i < 227; ++i) { const uint32_t y = (m[i] & kUpper) | (m[i + 1] & kLower); m[i] = m[i + 397] ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrix); }
        for (int i = 227; i < 623; ++i) { const uint32_t y = (m[i] & kUpper) | (m[i + 1] & kLower); m[i] = m[i - 227] ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrix); }
        { const uint32_t y = (m[623] & kUpper) | (m[0] & kLower); m[623] = m[396] ^ (y >> 1) ^ ((0u - (y & 1u)) & kMatrix); }
        for (int i = 0; i < 624; ++i) { uint32_t y = m[i]; y ^= y >> 11; y ^= (y << 7) & 0x9d2c5680u; y ^= (y << 15) & 0xefc60000u; y ^= y >> 18; out[i] = y; }
    }
};
// the value that ends at position p started at the position found by undoing the swaps, last one first: J[i] = the partner
// drawn at step i.  Eight tracked positions in one vector (clang vector extensions: AVX2 under the target attribute below,
// two SSE2 halves otherwise).
typedef uint32_t u32x8 __attribute__((vector_size(32)));
typedef int32_t i32x8 __attribute__((vector_size(32)));
template <int>
__attribute__((always_inline)) inline void trace_back8(const uint32_t* J, uint64_t n, uint32_t* where8) {
    u32x8 w;
    std::memcpy(&w, where8, sizeof(w));
    for (uint64_t t = 1; t < n; ++t) {
        const uint32_t j = J[t], ii = (uint32_t)t;
        const u32x8 vi = {ii, ii, ii, ii, ii, ii, ii, ii}, vj = {j, j, j, j, j, j, j, j};
        const i32x8 ei = (i32x8)(w == vi), ej = (i32x8)(w == vj);
        const i32x8 any = ei | ej;
        if (__builtin_reduce_or(any)) w = (u32x8)((ei & (i32x8)vj) | (ej & (i32x8)vi) | (~any & (i32x8)w));
    }
    std::memcpy(where8, &w, sizeof(w));
}
// the n - 1 bounded draws of the shuffle into J, then the trace-back of positions 0 .. k - 1 (where[64], identity on entry)
template <int>
__attribute__((always_inline)) inline void sample_core(Mt19937Block* g, uint32_t* J, uint64_t n, int k, uint32_t* where) {
    int pos = 624;
    uint64_t i = n - 1;                                  // (i <= 2^32 - 1: the 32-bit branch of random_interval)
    while (i >= 1) {
        uint64_t mask = i;
        mask |= mask >> 1; mask |= mask >> 2; mask |= mask >> 4; mask |= mask >> 8; mask |= mask >> 16;
        const uint32_t lo = (uint32_t)((mask >> 1) + 1);    // the smallest i with this mask
        const uint32_t m32 = (uint32_t)mask;
        uint32_t ii = (uint32_t)i;
        while (ii >= lo) {
            if (pos == 624) { g->refill(); pos = 0; }
            int q = pos;
            for (; q < 624 && ii >= lo; ++q) { const uint32_t v = g->out[q] & m32; J[ii] = v; ii -= (v <= ii) ? 1u : 0u; }   // masked rejection, branch-free
            pos = q;
        }
        i = ii;
    }
    if (k <= 8) {
        trace_back8<0>(J, n, where);
    } else {
        for (uint64_t t = 1; t < n; ++t) {
            const uint32_t j = J[t], ii = (uint32_t)t;
            for (int p = 0; p < k; ++p) {
                const uint32_t w = where[p];
                where[p] = w == ii ? j : (w == j ? ii : w);
            }
        }
    }
}
__attribute__((target("avx2"))) void sample_core_avx2(Mt19937Block* g, uint32_t* J, uint64_t n, int k, uint32_t* w) { sample_core<1>(g, J, n, k, w); }
void sample_core_generic(Mt19937Block* g, uint32_t* J, uint64_t n, int k, uint32_t* w) { sample_core<0>(g, J, n, k, w); }
}  // namespace
}  // extern "C++"

int mcr_sample_columns(uint32_t seed, uint64_t n, int32_t k, int64_t* out) {
    if (!out || k < 1 || k > 64 || (uint64_t)k > n || n > ((uint64_t)1 << 32)) { set_error("mcr_sample_columns: need 1 <= k <= min(n, 64), n <= 2^32"); return MCR_ERR_INVALID_ARG; }
    if (n == 1) { out[0] = 0; return MCR_OK; }
    if (n > 50000000ull) {   // once per process: the draw is sequential host work, O(n) time and 4 n bytes of host scratch
        static std::once_flag once;
        std::call_once(once, [n] { std::fprintf(stderr, "mcr_sample_columns: %llu paths: the sampled-column draw (NumPy's RandomState.choice, MT19937, "
                                                        "sequential) takes ~5 ns and 4 bytes of host scratch per path\n", (unsigned long long)n); });
    }
    // J[i] = the partner position drawn at step i (i = n - 1 ... 1); J[0] unused
    uint32_t* J = (uint32_t*)std::malloc((size_t)n * sizeof(uint32_t));
    if (!J) { set_error("mcr_sample_columns: out of host memory (%llu bytes)", (unsigned long long)(n * 4)); return MCR_ERR_INVALID_ARG; }
    Mt19937Block* g = new Mt19937Block;
    g->seed(seed);
    uint32_t where[64];
    for (int p = 0; p < 64; ++p) where[p] = (uint32_t)p;
    if (__builtin_cpu_supports("avx2")) sample_core_avx2(g, J, n, k, where); else sample_core_generic(g, J, n, k, where);
    delete g;
    std::free(J);
    for (int p = 0; p < k; ++p) out[p] = (int64_t)where[p];
    return MCR_OK;
}

int mcr_release_cached(int device) {
    const int rc_ctx = g_host_ctx.release_cached(device), rc_fork = g_stream_fork.release_cached(device);
    return rc_fork != MCR_OK ? rc_fork : rc_ctx;
}

int mcr_draw_shocks_host(uint64_t seed, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                         int32_t n_months, double rho, double* out, int device) {
    const mcr_rng r = philox_rng(seed);
    return mcr_draw_shocks_host_rng(&r, stream_id, path_begin, n_paths, n_months, rho, out, device);
}

int mcr_draw_shocks_host_rng(const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                             int32_t n_months, double rho, double* out, int device) {
    MCR_ENTER_DEVICE(device);
    int rc = MCR_OK;
    rc = check_rng(rng, true);
    if (rc != MCR_OK) return rc;
    const uint64_t seed = rng->philox_seed;
    if (!out || n_months < 0) { set_error("bad arguments"); return MCR_ERR_INVALID_ARG; }
    const uint64_t total = n_paths * (uint64_t)n_months;
    if (total == 0) return MCR_OK;
    if (total > ((uint64_t)1 << 31)) { set_error("too many shock rows for one call"); return MCR_ERR_INVALID_ARG; }
    DeviceArena arena;
    double* d = nullptr;
    hipError_t e = arena.alloc((void**)&d, (size_t)total * 3 * sizeof(double));
    if (e != hipSuccess) return hip_fail(e, "hipMalloc");
    const double om = 1.0 - rho * rho;
    const double rho_c = std::sqrt(om > 0.0 ? om : 0.0);
    if (rng->kind == MCR_RNG_HISTORY) {      // the gathered rows of the record (rho is not applied)
        double* d_z = nullptr;
        const size_t z_bytes = (size_t)rng->history_months * 3 * sizeof(double);
        e = arena.alloc((void**)&d_z, z_bytes);
        if (e == hipSuccess) e = hipMemcpy(d_z, rng->history, z_bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "history table upload");
        hipLaunchKernelGGL(history_shocks_kernel, dim3((unsigned)((n_paths + 63) / 64)), dim3(64), 0, nullptr, seed, stream_id, path_begin,
                           n_paths, n_months, d_z, rng->history_months, rng->history_block, rng->history_scheme, d);
    } else if (rng->kind == MCR_RNG_NUMPY) {
        KernelIO io;
        std::memset(&io, 0, sizeof(io));
        uint32_t* d_seeds = nullptr;
        if (rng->path_seeds) {
            e = arena.alloc((void**)&d_seeds, (size_t)n_paths * sizeof(uint32_t));
            if (e == hipSuccess) e = hipMemcpy(d_seeds, rng->path_seeds, (size_t)n_paths * sizeof(uint32_t), hipMemcpyHostToDevice);
            if (e != hipSuccess) return hip_fail(e, "seed upload");
        }
        fill_io_rng(io, rng, d_seeds);
        io.stream_id = stream_id; io.path_begin = path_begin; io.n_paths = n_paths;
        hipLaunchKernelGGL(np_shocks_kernel, dim3((unsigned)((n_paths + 63) / 64)), dim3(64), 0, nullptr, io, n_months, rho, rho_c, d);
    } else {
        hipLaunchKernelGGL(shocks_kernel, dim3((unsigned)((n_paths + 63) / 64)), dim3(64), 0, nullptr, seed,
                           stream_id, path_begin, n_paths, n_months, rho, rho_c, d);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, d, (size_t)total * 3 * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "shocks_kernel");
    return MCR_OK;
}

int mcr_eval_helper_host(int which, const mcr_params* p, const double* in, double* out, int64_t n, int device) {
    MCR_ENTER_DEVICE(device);
    int rc = MCR_OK;
    int n_in, n_out;
    switch (which) {
        case MCR_HELPER_WITHDRAW: n_in = 5; n_out = 4; break;
        case MCR_HELPER_NLV: n_in = 4; n_out = 1; break;
        case MCR_HELPER_REBALANCE: n_in = 4; n_out = 4; break;
        case MCR_HELPER_ANNUAL_TAX: n_in = 6; n_out = 5; break;
        case MCR_HELPER_MONTHLY_GROSS: n_in = 3; n_out = 1; break;
        case MCR_HELPER_MATH_EXP: n_in = 1; n_out = 1; break;
        case MCR_HELPER_MATH_DIV: n_in = 2; n_out = 1; break;
        case MCR_HELPER_MATH_DIV_PATH: n_in = 2; n_out = 1; break;
        case MCR_HELPER_WITHDRAW2_PATH: n_in = 6; n_out = 8; break;
        case MCR_HELPER_NLV2_PATH: n_in = 4; n_out = 2; break;
        case MCR_HELPER_REBALANCE_PATH: n_in = 4; n_out = 4; break;
        case MCR_HELPER_ANNUAL_TAX_PATH: n_in = 6; n_out = 5; break;
        case MCR_HELPER_MATH_SQRT: n_in = 1; n_out = 1; break;
        case MCR_HELPER_MATH_NEG2LOG: n_in = 1; n_out = 1; break;
        case MCR_HELPER_MATH_SINCOS: n_in = 1; n_out = 2; break;
        case MCR_HELPER_MATH_EXP_PATH: n_in = 1; n_out = 1; break;
        case MCR_HELPER_MATH_NEG2LOG_PATH: n_in = 1; n_out = 1; break;
        case MCR_HELPER_MATH_SINCOS_PATH: n_in = 1; n_out = 2; break;
        case MCR_HELPER_WITHDRAW_MONTH: n_in = 5; n_out = 6; break;
        case MCR_HELPER_REBALANCE_MONTH: n_in = 4; n_out = 4; break;
        case MCR_HELPER_MATH_EXP_FORMS: n_in = 1; n_out = 2; break;
        default: set_error("unknown helper %d", which); return MCR_ERR_INVALID_ARG;
    }
    if (!in || !out || n < 0) { set_error("bad arguments"); return MCR_ERR_INVALID_ARG; }
    if (n == 0) return MCR_OK;
    DevParams d;
    std::memset(&d, 0, sizeof(d));
    if (which == MCR_HELPER_REBALANCE || which == MCR_HELPER_ANNUAL_TAX || which == MCR_HELPER_WITHDRAW2_PATH ||
        which == MCR_HELPER_NLV2_PATH || which == MCR_HELPER_REBALANCE_PATH || which == MCR_HELPER_ANNUAL_TAX_PATH ||
        which == MCR_HELPER_WITHDRAW_MONTH || which == MCR_HELPER_REBALANCE_MONTH) {
        if (!p) { set_error("helper %d needs params", which); return MCR_ERR_INVALID_ARG; }
        rc = derive_params(p, 0, &d);
        if (rc != MCR_OK) return rc;
    }
    DeviceArena arena;
    double *din = nullptr, *dout = nullptr;
    hipError_t e = arena.alloc((void**)&din, (size_t)n * n_in * sizeof(double));
    if (e == hipSuccess) e = arena.alloc((void**)&dout, (size_t)n * n_out * sizeof(double));
    if (e == hipSuccess) e = hipMemcpy(din, in, (size_t)n * n_in * sizeof(double), hipMemcpyHostToDevice);
    if (e != hipSuccess) return hip_fail(e, "helper upload");
    if (which == MCR_HELPER_MATH_EXP_FORMS) hipLaunchKernelGGL(exp_forms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, din, dout, n);
    else hipLaunchKernelGGL(helper_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr, which, d, din, dout, n);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * n_out * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return hip_fail(e, "helper_kernel");
    return MCR_OK;
}

}  // extern "C"
