/*
 * mcr.h — C ABI of the MI355X-native Monte Carlo retirement path engine.
 *
 * This is the drop-in boundary for ONE hot path of rflamino/monte_carlo_retirement:
 * the per-path loop `RetirementMonteCarloSimulator._run_single_simulation_path`
 * (reference backend/simulation.py:476-950) and the batch driver above it
 * (`run_monte_carlo_simulations`, backend/simulation.py:952-1128).  The reference
 * has no FFI layer of its own (it is pure Python); these entry points are what a
 * ctypes binding inside the reference's `run_monte_carlo_simulations` would call
 * (see INTEGRATION.md).  Plain C types only: no torch, no C++ in the signatures.
 *
 * Every compute entry point runs hand-written HIP kernels on a gfx950 device.
 * There is NO CPU fallback in this library: without a usable HIP device every
 * compute call returns MCR_ERR_NO_DEVICE and sets mcr_last_error().
 *
 * All arithmetic on the path is IEEE fp64, as in the reference (Python float).
 */
#ifndef MCR_H_
#define MCR_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCR_ABI_VERSION 8
#define MCR_INLINE_STREAMS 16   /* other_income_streams entries carried INSIDE mcr_params; the rest of the list (any length,
                                   backend/config.py:99) follows through mcr_params.extra_streams */
#define MCR_MAX_PROBE_CANDIDATES 32 /* candidates of one mcr_probe_months_rng call that can share their accumulation sweep */
#define MCR_MAX_EXPENSE_FANOUT 15  /* spending levels one expense fan-out workgroup evaluates (mcr_probe_expenses_rng) */
#define MCR_MAX_JOINT_OPTIONS 32    /* options of one joint probe / mcr_joint_counts call (the co-occurrence matrix is n x n) */
#define MCR_MAX_HIST_BINS 4096  /* bins of the in-kernel final-balance histogram (mcr_outputs.hist_bins) */
#define MCR_MAX_YEAR_BINS 512   /* bins per row of the yearly-bins tables (mcr_year_bins); each balance bin costs 28 bytes of a
                                   workgroup's LDS and each withdrawal-rate bin 16: 2.9 KB at 64 + 64 bins, 11.4 KB at 256 + 256,
                                   22.6 KB at the cap — above about 256 + 256 a CU holds one workgroup fewer */
#define MCR_MONTHS_PER_YEAR 12  /* backend/constants.py:1 */
#define MCR_SMALL_EPSILON 1e-6  /* backend/constants.py:3 (absolute dollar threshold) */

/* error codes (0 = success); message text via mcr_last_error() */
#define MCR_OK 0
#define MCR_ERR_INVALID_ARG (-1)
#define MCR_ERR_NO_DEVICE (-2)
#define MCR_ERR_HIP (-3)
#define MCR_ERR_UNSUPPORTED (-4)

/* Seed streams: replaces SeedSequence(main).spawn(2) (backend/simulation.py:147-151). */
#define MCR_STREAM_SEARCH 0u
#define MCR_STREAM_FINAL 1u

/*
 * Random stream of a batch.
 *  MCR_RNG_PHILOX  the engine's native stream: Philox4x32-10, key = philox_seed, counter =
 *                  (path_lo, path_hi, month, stream_id) -> Box-Muller (3 normals / month).
 *  MCR_RNG_NUMPY   the REFERENCE's own stream, reproduced on the device: path i of the batch is
 *                  child (stream_id, child_offset + i) of SeedSequence(main_seed) -> generate_state(1)
 *                  -> default_rng(seed32) = PCG64 -> Generator.standard_normal (ziggurat), exactly
 *                  what backend/simulation.py:148-149,195-197,457-458 executes through NumPy.
 *                  `entropy` = main_seed as little-endian uint32 words; `child_offset` = the stream's
 *                  SeedSequence.n_children_spawned when the reference would spawn this batch's seeds;
 *                  `path_seeds` (optional) = explicit uint32 seed per path instead of the derivation
 *                  (what _run_single_simulation_path(working_months, path_seed) receives).
 *  MCR_RNG_HISTORY a BLOCK BOOTSTRAP of a recorded market: `history` = Z[history_months][3], the record's monthly
 *                  (equity, inflation, premium) standard shocks; a path reads them in blocks of `history_block`
 *                  consecutive months that start at uniformly drawn months of the record and wrap around its end.
 *                  Shock row r of global path `path` (r = the row an injected launch would read, clamped to
 *                  shock_rows - 1 like it):
 *                      k = r / B, j = r % B                                  (B = history_block, H = history_months)
 *                      x = word (k & 3) of Philox4x32-10(counter = (path_lo, path_hi, k >> 2, stream_id),
 *                                                        key = (seed_lo, seed_hi))        (seed = philox_seed)
 *                      s = ((uint64_t)x * H) >> 32       block start; each start is drawn with probability within
 *                                                        H / 2^32 (< 5e-7) of 1 / H
 *                      row = (s + j) mod H               circular
 *                      (z_equity, z_inflation, z_premium) = Z[row]
 *                  The triple is used exactly as an injected row: equity_inflation_correlation is NOT applied (the
 *                  record carries its own co-movement).  Row r is a pure function of (seed, stream_id, path, r):
 *                  common random numbers across working-month candidates, probe levels and any sharding, like the
 *                  Philox stream.  B = 1 is an i.i.d. month bootstrap; B >= total_months draws one start per path
 *                  and runs the record forward.  A record of standardised log returns replays "the history as it
 *                  was" under its own fitted parameters, and "the history's shape around other means" under any
 *                  other mcr_params: the growth factors are made from Z with the launch's parameters.
 *                  Whole-path launches only: the fan-out probe forms answer MCR_ERR_UNSUPPORTED inside the probe
 *                  entry points, which then run one launch per level.  Kinds 0 and 1 never read the history fields.
 *
 *                  `history_scheme` chooses which row of the record shock row r reads; the rule above is
 *                  MCR_HISTORY_BLOCK (0, what a zeroed descriptor asks for).  The other two, with the same H, B and r:
 *
 *                  MCR_HISTORY_STATIONARY  the stationary bootstrap (Politis & Romano 1994): block lengths geometric
 *                  with mean B instead of all equal, so no month of a path is a seam in every path and the resampled
 *                  series is stationary.
 *                      q = r >> 1, a = 2 (r & 1)
 *                      (w0..w3) = Philox4x32-10(counter = (path_lo, path_hi, q, stream_id), key = (seed_lo, seed_hi))
 *                      u = w[a], v = w[a + 1]                               one Philox block serves two months
 *                      restart = (r == 0) || (((uint64_t)u * B) >> 32) == 0  probability ceil(2^32 / B) / 2^32: mean
 *                                                                            block length B to within B / 2^32
 *                      row_r   = restart ? ((uint64_t)v * H) >> 32 : (row_{r-1} + 1) mod H
 *                  B = 1 restarts every month (an i.i.d. month bootstrap); B = 2^31 - 1 practically never restarts
 *                  after row 0.  Row r is reached by walking from row 0, which always restarts, so it is still a pure
 *                  function of (seed, stream_id, path, r).  The counters coincide with some of the block rule's at the
 *                  same seed; that does not matter, because one launch has one scheme.
 *
 *                  MCR_HISTORY_COHORTS  the every-start replay, the historical backtest itself: path i starts at month
 *                  i mod H of the record and runs it forward.
 *                      row_r = ((path mod H) + r) mod H                      path = the 64-bit global path index
 *                  No random numbers: philox_seed and history_block are not read (but validated as before).  Paths i
 *                  and i + H are the same path; a count over n paths weighs the starts equally when n is a multiple
 *                  of H.
 */
#define MCR_RNG_PHILOX 0u
#define MCR_RNG_NUMPY 1u
#define MCR_RNG_HISTORY 2u
#define MCR_MAX_ENTROPY_WORDS 8
#define MCR_MAX_HISTORY_MONTHS 2048 /* 170 years: 48 KB of growth factors in a workgroup's LDS */
#define MCR_HISTORY_BLOCK      0u   /* fixed block length */
#define MCR_HISTORY_STATIONARY 1u   /* geometric block lengths of mean history_block */
#define MCR_HISTORY_COHORTS    2u   /* path i starts at month i mod history_months */
typedef struct mcr_rng {
    uint32_t kind;
    uint32_t n_entropy_words;                /* 1..MCR_MAX_ENTROPY_WORDS (numpy) */
    uint32_t entropy[MCR_MAX_ENTROPY_WORDS]; /* numpy: main_seed words, least significant first */
    uint64_t philox_seed;                    /* philox key; history: the key of the block starts */
    uint64_t child_offset;                   /* numpy */
    const uint32_t* path_seeds;              /* numpy, optional; DEVICE ptr for mcr_run_batch_rng, HOST ptr for *_host_rng */
    const double* history;                   /* history: Z[history_months][3], finite; DEVICE ptr for the hip_stream entry
                                                points, HOST ptr for *_host_rng (uploaded like path_seeds) */
    uint32_t history_months;                 /* history: 1..MCR_MAX_HISTORY_MONTHS */
    uint32_t history_block;                  /* history: block length in months (stationary: its mean), 1..2^31 - 1 */
    uint32_t history_scheme;                 /* history: MCR_HISTORY_BLOCK / _STATIONARY / _COHORTS */
    uint32_t history_reserved;               /* 0 */
} mcr_rng;

/* One `OtherIncomeStreamConfig` (backend/config.py:12-47), raw field values. */
typedef struct mcr_stream {
    double monthly_amount_today; /* config.py:18 */
    double start_at_age;         /* config.py:23 */
    double tax_rate;             /* config.py:45 */
    int32_t duration_years;      /* config.py:33; -1 encodes None (paid indefinitely) */
    int32_t inflation_indexed;   /* config.py:41 (0/1) */
} mcr_stream;

/*
 * The scalars of `Config` (backend/config.py:48-126) that the path reads, plus the
 * lognormal parameters `RetirementMonteCarloSimulator.__init__` derives from them
 * (backend/simulation.py:156-170, via arithmetic_to_log_params :14-29).
 */
typedef struct mcr_params {
    double initial_balance;                 /* config.py:56 */
    double monthly_contribution;            /* config.py:57 */
    double contribution_growth_rate_annual; /* config.py:58 */
    double monthly_expenses;                /* config.py:59 */
    double current_age;                     /* config.py:62 */
    double allocation_inv1_pct;             /* config.py:70 */
    double inv1_annual_tax_on_gains_rate;   /* config.py:73 */
    double inv1_realized_gains_tax_rate;    /* config.py:74 */
    double inv2_annual_tax_on_gains_rate;   /* config.py:79 */
    double inv2_realized_gains_tax_rate;    /* config.py:80 */
    double inv1_mu_log, inv1_sigma_log;     /* simulation.py:157-159 */
    double inf_mu_log, inf_sigma_log;       /* simulation.py:160-162 */
    double prem_mu_log, prem_sigma_log;     /* simulation.py:163-166 */
    double equity_inflation_rho;            /* simulation.py:170 */
    int32_t retirement_years;               /* config.py:68 (> 0) */
    int32_t inv1_use_realized_gains_tax_system; /* config.py:75 (0/1) */
    int32_t inv2_use_realized_gains_tax_system; /* config.py:81 (0/1) */
    int32_t n_streams;                      /* len(other_income_streams): ANY length >= 0, as in the reference (config.py:99) */
    mcr_stream streams[MCR_INLINE_STREAMS]; /* config.py:99, list order preserved: entries 0 .. min(n_streams, 16) - 1 */
    /* Entries MCR_INLINE_STREAMS .. n_streams - 1 of the list, in order (a HOST pointer on every entry point: the
     * parameter block is always host memory; the library copies the records into a device table next to the launch).
     * Must be non-NULL when n_streams > MCR_INLINE_STREAMS; ignored otherwise.  The loop over the streams is the
     * reference's (backend/simulation.py:602-621, 649-677): O(n_streams) per retirement month, whatever the length. */
    const mcr_stream* extra_streams;
} mcr_params;

/* Shapes implied by (params, working_months); simulation.py:487,585-589,902. */
typedef struct mcr_sizes {
    int32_t total_months;      /* working_months + retirement_years*12 */
    int32_t shock_rows;        /* max(total_months, 1)  (simulation.py:488) */
    int32_t num_working_years; /* ceil(working_months/12) */
    int32_t trajectory_len;    /* T = 1 + num_working_years + retirement_years */
    int32_t retirement_years;  /* rows of the withdrawal-rate trajectory */
    int32_t ruin_bins;         /* retirement_years + 2, see mcr_outputs.ruin_year_bins */
} mcr_sizes;

/* indices into mcr_outputs.counters */
#define MCR_CTR_SUCCESS 0 /* number of paths with Success == True */
#define MCR_CTR_PATHS 1   /* number of paths simulated */
#define MCR_N_COUNTERS 2

/*
 * Output buffers of one batch.  Any pointer may be NULL = "not requested"; the kernel
 * variant is chosen from what is requested (success-count only / + per-path summary /
 * + yearly trajectories).  Layout is struct-of-arrays; trajectories are TIME-MAJOR
 * (`row[t*path_stride + i]` for local path i) so that one wavefront store is 512
 * contiguous bytes.  Field meanings follow the dict returned by
 * _run_single_simulation_path (simulation.py:939-950).
 *
 * For mcr_run_batch the pointers are DEVICE pointers; for mcr_run_batch_host they are
 * HOST pointers.  Counters / bins are ACCUMULATED into (the caller zeroes them), so
 * several launches (or several GPUs before an all-reduce) can share one vector.
 */
typedef struct mcr_outputs {
    double* start_balance;                    /* [n] "Start Balance" */
    double* final_balance;                    /* [n] "Final Balance" = max(0, .) */
    double* years_to_ruin;                    /* [n] "YearsToRuin" (NaN if success) */
    double* first_year_gross_withdrawal;      /* [n] */
    double* first_year_real_gross_withdrawal; /* [n] */
    double* inflation_at_retirement;          /* [n] */
    uint8_t* success;                         /* [n] "Success" (0/1) */
    double* trajectory;                       /* [T][path_stride]  "Trajectory" */
    double* real_trajectory;                  /* [T][path_stride]  "RealTrajectory" */
    double* withdrawal_rate_trajectory;       /* [ry][path_stride] NaN-padded */
    int64_t path_stride;                      /* >= n_paths (elements) */
    uint64_t* counters;                       /* [MCR_N_COUNTERS] */
    uint64_t* wr_obs_counts;                  /* [ry]   wr_df.count(axis=1), simulation.py:1111-1113 */
    uint64_t* ruin_year_bins;                 /* [ry+2] [0]=pre-retirement tax failure (YearsToRuin 0.0,
                                                 simulation.py:628-629); [1+y]=failed in retirement year y;
                                                 [ry+1]=failed at the terminal tax settlement (:894-896) */
    /* In-kernel histogram of "Final Balance" over the successful cohort (the CLI's chart, backend/plotting.py:44-59) on
     * CALLER-SUPPLIED bin edges: hist_bins[k] += #{successful paths: hist_edges[k] <= Final Balance < hist_edges[k+1]}, the
     * last bin closed on the right, values outside [hist_edges[0], hist_edges[hist_n_bins]] dropped — exactly
     * np.histogram(final_balance[success], bins=hist_edges); with hist_edges = np.linspace(lo, hi, n + 1) that is also
     * np.histogram(..., bins=n, range=(lo, hi)), and any other monotone spacing (np.geomspace for log-spaced bins) works
     * the same way.  Every lane bins its own path at the end of the horizon (binary search over the edges, LDS-privatised
     * bins, one global atomic per non-empty bin per workgroup): no per-path output, no second kernel, and the bins sit in
     * the same accumulated integer block as the counters — a multi-GPU caller sums everything with ONE all-reduce.
     * hist_edges: [hist_n_bins + 1] ascending finite doubles (DEVICE pointer for mcr_run_batch*, HOST for *_host*);
     * hist_n_bins in 1..MCR_MAX_HIST_BINS (above 512 bins the LDS footprint costs one resident workgroup per CU);
     * hist_bins == NULL or hist_n_bins == 0: not requested. */
    const double* hist_edges;
    uint64_t* hist_bins;                      /* [hist_n_bins], accumulated into like the counters */
    int32_t hist_n_bins;
    int32_t hist_reserved;                    /* 0 */
} mcr_outputs;

/* ---- library / device ------------------------------------------------------------ */
int mcr_abi_version(void);
/* Number of usable HIP devices (0 if none; never fails). */
int mcr_device_count(void);
/* Thread-local message of the last failing call on this thread ("" if none). */
const char* mcr_last_error(void);

/* Frees the library's idle cached device resources on `device` (< 0: every device): the leased-context pool of the
 * *_host entry points (streams + scratch blocks, see mcr_run_batch_host) and the side streams of mcr_probe_months_rng.
 * Contexts that are in use by concurrent calls are untouched.  Safe to call at any time from any thread. */
int mcr_release_cached(int device);

/* ---- host-side derivations (no device needed) -------------------------------------- */
/* Shapes for (params, working_months).  Returns MCR_ERR_INVALID_ARG for working_months<0,
 * retirement_years<=0, n_streams<0. */
int mcr_query_sizes(const mcr_params* p, int32_t working_months, mcr_sizes* out);
/* The growth form a whole-path count-only launch of (params, working_months) on the engine's own stream runs (DESIGN.md,
 * "growth forms"): bit 0 = every argument of the month's exps lies in the narrow window, bit 1 = rho is 0; masks 0, 1 and 3.
 * MCR_K1_GROWTH_FORM in the environment forces a lower mask, as at a launch; a mask the parameters do not qualify for
 * returns MCR_ERR_INVALID_ARG. */
int mcr_k1_growth_form(const mcr_params* p, int32_t working_months, int32_t* mask);
/* The month form of the same launch ("month forms"): bit 0 = both assets are taxed on realized gains at the same
 * rate, with no annual-gains tax; masks 0 and 1.  MCR_K1_MONTH_FORM in the environment forces a lower mask, as at a launch; a
 * mask the parameters do not qualify for returns MCR_ERR_INVALID_ARG. */
int mcr_k1_month_form(const mcr_params* p, int32_t working_months, int32_t* mask);
/* The stream form of the same launch ("stream form"): bit 0 = the records the kernel is given (mcr_k1_kept_streams)
 * are at most two, all inflation-indexed, with no annual-gains tax: they stay in registers for the whole launch; masks 0 and 1.
 * MCR_K1_STREAM_FORM in the environment forces a lower mask, as at a launch; a mask the parameters do not qualify for returns
 * MCR_ERR_INVALID_ARG. */
int mcr_k1_stream_form(const mcr_params* p, int32_t working_months, int32_t* mask);
/* Whether a count-only launch of n_paths paths of (params, working_months) on `rng` (NULL: the engine's own stream), with
 * hist_n_bins bins of the in-kernel histogram (0: none), takes the SCREENED route ("screened count-only launches"):
 * every path is first classified in fp32, and only the doubtful ones run the fp64 state machine.  *screened = 1 when the
 * parameters qualify (no annual-gains tax, the tolerance month, at most two paying income records, all inflation-indexed),
 * the stream is MCR_RNG_PHILOX, no histogram is requested, n_paths < 2^32 and n_paths >= MCR_K1_SCREEN_MIN_PATHS (default
 * 500 000).  MCR_K1_SCREEN=0 in the environment turns the route off, =1 takes it at any size; a launch under any knob that
 * addresses the classic kernels (MCR_K1_SEGMENTS, _SEGMENTS_ALWAYS, _SEGMENT_ORDER, _SEGMENT_POLLS, _GROWTH_FORM, _MONTH_FORM,
 * _STREAM_FORM) takes the classic route.  Same counters, wr_obs_counts and ruin_year_bins either way, bit for bit. */
int mcr_k1_screen(const mcr_params* p, const mcr_rng* rng, int32_t working_months, uint64_t n_paths, int32_t hist_n_bins, int32_t* screened);
/* Test hook (tests and tools only): runs the screening kernel of that route ALONE over global paths [path_begin, path_begin +
 * n_paths) and returns per path, in HOST arrays (any may be NULL): its class, the lowest capacity / need of the retirement months
 * it ran (+inf: no month with a need) and b1 + b2 where it stopped (a SAFE path: at the end of the horizon).
 * MCR_ERR_UNSUPPORTED when the parameters or the stream do not qualify.  Synchronous. */
#define MCR_SCREEN_SAFE 0      /* succeeds with every retirement year observed: counted by the screening kernel */
#define MCR_SCREEN_DOUBTFUL 1  /* decided by the fp64 state machine */
int mcr_screen_paths_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                         int32_t working_months, uint8_t* cls, float* min_ratio, float* final_total, int device);
/* The other_income_streams records the path kernel is given for (params, working_months), in list order: a record with
 * monthly_amount_today == 0 pays an exact zero every month and is left out; lock slots (non-indexed streams; -1 for an indexed
 * one) are numbered over the kept records.  Writes min(*n, cap) entries of index[] (position in the caller's list) and
 * lock_slot[]; *n = the number kept. */
int mcr_k1_kept_streams(const mcr_params* p, int32_t working_months, int32_t* index, int32_t* lock_slot, int32_t cap, int32_t* n);
/* Range check of a parameter block — what the reference's pydantic Config enforces (backend/config.py:56-99)
 * and the kernel relies on: amounts finite and >= 0, rates / allocation / stream tax rates in [0, 1], rho in
 * [-1, 1], finite log-parameters with sigma >= 0 and |mu|/12 + 40 sigma/sqrt(12) < 700 (domain of the kernel's
 * exp), n_streams >= 0 (with extra_streams set beyond MCR_INLINE_STREAMS).  Every compute entry point applies it and returns
 * MCR_ERR_INVALID_ARG (message via mcr_last_error) instead of computing with out-of-range inputs.  Not
 * checkable up front: balances are assumed to stay within 1e-6 .. 1e15 (unscaled fp64 division). */
int mcr_validate_params(const mcr_params* p);
/* The five sampled paths of run_monte_carlo_simulations: trajectory_df.sample(n=5, axis=1, random_state=main_seed)
 * (simulation.py:1063-1078) = numpy.random.RandomState(seed).choice(n, k, replace=False), i.e. the first k entries of
 * RandomState(seed).permutation(n): MT19937 seeded with init_genrand(seed), a Fisher-Yates shuffle from the top with
 * masked-rejection bounded draws.  NumPy shuffles an n-element array to get them (7 ms at n = 1e6, 0.7 s at 1e8 — as
 * long as the path kernel takes for n paths); this restatement only generates the n - 1 draws and traces the k wanted
 * positions back through the swaps (branch-free rejection, the tracked positions in one vector register): the same
 * indices, bit for bit (tests/test_abi_cpu.py), in a fifth of NumPy's time.  Host-only (no device needed).  out: HOST int64[k].
 * Needs 1 <= k <= 64, k <= n, n <= 2^32; seed is the 32-bit seed (RandomState rejects larger ones).  Allocates 4 n bytes
 * of scratch on the host for the call and takes ~4 ns per path of sequential host time (MT19937 cannot be split): 40 ms and
 * 40 MB at 10^7 paths, 0.4 s and 400 MB at 10^8 — above 5 x 10^7 paths the call says so once on stderr.  Callers hide it on
 * a host thread next to the asynchronous kernel launch (the drop-in class does). */
int mcr_sample_columns(uint32_t seed, uint64_t n, int32_t k, int64_t* out);
/* stream_payment_start_month_index (simulation.py:47-63). */
int32_t mcr_stream_start_month_index(double current_age, int32_t working_months, double start_at_age);

/* ---- the hot path ------------------------------------------------------------------ */
/*
 * Simulate global paths [path_begin, path_begin+n_paths) for `working_months`, replacing
 * the loop over _path_seeds in run_monte_carlo_simulations (simulation.py:987-990) with one
 * kernel launch (one path per lane).  Shocks: Philox4x32-10 keyed by (seed), counter
 * (path_lo, path_hi, month, stream_id) -> Box-Muller -> rho-mix (replaces _draw_shock_path,
 * simulation.py:452-466).  Row k depends only on (seed, stream, path, k): common random
 * numbers across working-month candidates and across any sharding of the path range.
 *
 * injected_shocks (optional, device pointer, may be NULL): [n_paths][shock_rows][3] doubles
 * (equity, inflation, premium) used INSTEAD of the RNG — the parity hook that mirrors
 * assigning `sim._draw_shock_path` in the reference.
 *
 * out: device pointers.  hip_stream: a hipStream_t (NULL = default stream).  The call is
 * asynchronous: it enqueues on hip_stream and returns.  device: HIP device ordinal.
 * (Count-only Philox launches of at most 3 072 path-wavefronts — 196 608 paths — run a latency-oriented form of the kernel,
 * two waves per 64 paths: same results, bit for bit.  MCR_K1_SPLIT_MAX_WAVES in the environment moves the limit, 0 = never.
 * Philox launches of a few rounds of resident workgroups whose last round would be mostly empty — 10^6 paths are 2.54 rounds —
 * run TIME-SLICED: some path blocks are cut into segments at retirement-year boundaries and dispatched so that the small
 * work items come last; the hand-over state lives in a stream-ordered allocation of the call.  Same results, bit for bit;
 * MCR_K1_SEGMENTS = segments per sliced block, 0 = never.)
 */
int mcr_run_batch(const mcr_params* p, uint64_t seed, uint32_t stream_id,
                  uint64_t path_begin, uint64_t n_paths, int32_t working_months,
                  const double* injected_shocks, const mcr_outputs* out,
                  int device, void* hip_stream);

/* Same, with HOST buffers in `out` / `injected_shocks` (the entry point for non-torch callers, e.g. a ctypes
 * binding inside the reference's run_monte_carlo_simulations, simulation.py:952-1010): the call LEASES a context
 * (a private non-blocking stream + a scratch block its device buffers are carved from) out of a process-wide pool
 * keyed by device, runs uploads / kernel / downloads on that stream, returns after ONE synchronisation of it and
 * hands the context back — concurrent calls from several host threads (the reference's server runs requests on
 * executor threads, server.py:309,405) overlap on the GPU, and short-lived caller threads leave nothing behind.
 * Retention: at most 4 idle contexts per device stay cached, each with a block of at most 256 MiB (larger blocks are
 * freed on return); mcr_release_cached() frees them on demand.
 * device: a HIP device ordinal, or MCR_DEVICE_ALL = shard the path range over every visible device (below). */
#define MCR_DEVICE_ALL (-2)
int mcr_run_batch_host(const mcr_params* p, uint64_t seed, uint32_t stream_id,
                       uint64_t path_begin, uint64_t n_paths, int32_t working_months,
                       const double* injected_shocks, const mcr_outputs* out, int device);

/* The same three entry points with an explicit random-stream descriptor (mcr_rng); the functions
 * above are the MCR_RNG_PHILOX special case. */
int mcr_run_batch_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                      uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                      const mcr_outputs* out, int device, void* hip_stream);
int mcr_run_batch_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                           uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                           const mcr_outputs* out, int device);
int mcr_draw_shocks_host_rng(const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                             int32_t n_months, double rho, double* out, int device);

/*
 * Multi-GPU form of mcr_run_batch_host_rng for callers that bind the C ABI without torch.distributed — what
 * replaces the reference's only parallelism, Pool.starmap over independent paths (simulation.py:996-1001):
 * the global path range is cut into contiguous shards, one per listed device (devices == NULL or
 * n_devices <= 0: every visible device), each shard runs on its own host thread / stream / scratch, per-path
 * outputs land in the caller's HOST arrays at the shard's columns, and the counter / bin vectors (< 2 KB) are
 * summed on the host.  The Philox counter carries the GLOBAL path index, so the result is bit-identical to
 * a single-device call whatever the device list.  A device may be listed more than once.
 */
int mcr_run_batch_multi_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                 uint64_t n_paths, int32_t working_months, const double* injected_shocks,
                                 const mcr_outputs* out, const int32_t* devices, int32_t n_devices);

/*
 * Search driver support (find_minimum_working_months, simulation.py:1138-1342): success counts of
 * SEVERAL candidate working-month counts over the same path range — what the reference obtains by
 * calling run_monte_carlo_simulations(candidate, num_simulations_search) once per candidate and taking
 * _success_probability of each summary (simulation.py:1186-1199).  Philox stream, 2..32 distinct candidates: the
 * accumulation months do not depend on the candidate under common random numbers (simulation.py:513-579), so ONE sweep
 * runs them to the largest candidate and stores the state at the end of every candidate month, and ONE launch
 * (grid.y = candidate) resumes every decumulation from its snapshot; the snapshots are a stream-ordered allocation
 * (80 B per path and candidate; requests that would need more than 4 GiB of them, stream lists beyond the by-value block and
 * parameter blocks that need the exact month take the route below).  Otherwise: one count-only launch per candidate, forked onto internal HIP streams
 * so the candidates share the GPU concurrently, joined back onto `hip_stream`.  Asynchronous like mcr_run_batch.
 * counts: DEVICE uint64 [n_candidates][MCR_N_COUNTERS] = {successes, paths} per candidate (zeroed by
 * the call).  Common random numbers across candidates hold as in the reference (same path range, same
 * stream).
 */
int mcr_probe_months_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                         uint64_t n_paths, const int32_t* working_months, int32_t n_candidates,
                         uint64_t* counts, int device, void* hip_stream);

/*
 * Maximum-spending search support: success counts of SEVERAL monthly_expenses levels at one working-month count over the
 * same path range.  counts[k] equals, bit for bit, the counters of a count-only mcr_run_batch_rng call with the same
 * arguments and p->monthly_expenses = monthly_expenses[k].  monthly_expenses is a HOST array of n_levels >= 0 values (duplicates
 * allowed), each finite and >= 0 (config.py:59); every level is validated before anything is enqueued.  One level: the plain
 * count-only launch.  Philox stream, at most MCR_INLINE_STREAMS income streams, the tolerance month: ONE accumulation sweep
 * to working_months stores its state (80 B per path, a stream-ordered allocation), then EXPENSE FAN-OUT launches resume it:
 * a workgroup per 64 paths, one wave generating the random numbers for up to MCR_MAX_EXPENSE_FANOUT consumer waves, one per
 * level.  Otherwise (NumPy stream, longer stream lists, the exact month, allocation refused): one count-only launch per level
 * on internal side streams, joined back onto `hip_stream`.  counts: DEVICE uint64 [n_levels][MCR_N_COUNTERS] = {successes,
 * paths} (zeroed by the call).  Asynchronous like mcr_probe_months_rng.
 */
int mcr_probe_expenses_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                           uint64_t n_paths, int32_t working_months, const double* monthly_expenses, int32_t n_levels,
                           uint64_t* counts, int device, void* hip_stream);

/*
 * Minimum-contribution search support: success counts of SEVERAL monthly_contribution levels at one working-month count over
 * the same path range.  counts[k] equals, bit for bit, the counters of a count-only mcr_run_batch_rng call with the same
 * arguments and p->monthly_contribution = monthly_contributions[k].  monthly_contributions is a HOST array of n_levels >= 0
 * values (duplicates allowed), each finite and >= 0 (config.py:57); every level is validated before anything is enqueued
 * (counts stay untouched on an error).  One level: the plain count-only launch.  Philox stream, at most MCR_INLINE_STREAMS
 * income streams, the tolerance month, n_paths <= 2^31: CONTRIBUTION FAN-OUT launches, a workgroup per 64 paths, one wave
 * generating the random numbers of the whole path for up to MCR_MAX_EXPENSE_FANOUT consumer waves, one per level (the levels
 * differ from month 0: nothing is shared but the random numbers, and nothing is allocated).  Otherwise (NumPy stream, longer
 * stream lists, the exact month, or fewer path-wavefronts than MCR_CONTRIBUTION_FANOUT_MIN_WAVES in the environment): one
 * count-only launch per level on internal side streams, joined back onto `hip_stream`.  counts: DEVICE uint64
 * [n_levels][MCR_N_COUNTERS] = {successes, paths} (zeroed by the call).  Asynchronous like mcr_probe_months_rng.
 */
int mcr_probe_contributions_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                uint64_t n_paths, int32_t working_months, const double* monthly_contributions, int32_t n_levels,
                                uint64_t* counts, int device, void* hip_stream);

/*
 * What-if scenarios: success counts of SEVERAL (initial_balance, monthly_contribution, monthly_expenses) records at one
 * working-month count over the same path range — the probe of the required-starting-balance search and of the
 * safe-withdrawal-rate curve (balance and spending vary together).  counts[k] equals, bit for bit, the counters of a
 * count-only mcr_run_batch_rng call with the same arguments and those three fields of *p replaced by scenarios[k].  scenarios
 * is a HOST array of n_scenarios >= 0 records (0 does nothing; duplicates allowed); every field of every record must be finite
 * and >= 0 (config.py:56, 57, 59) and everything is validated before anything is enqueued: on an error counts stay untouched
 * and the message names scenarios[k].<field>.  One scenario: the plain count-only launch.  Philox stream, at most
 * MCR_INLINE_STREAMS income streams, the tolerance month, n_paths <= 2^31 and at least MCR_SCENARIO_FANOUT_MIN_WAVES
 * path-wavefronts (environment, default 0): SCENARIO FAN-OUT launches, the contribution fan-out's workgroup (a workgroup per
 * 64 paths, one wave generating the random numbers of the whole path for up to MCR_MAX_EXPENSE_FANOUT consumer waves) with one
 * record per consumer wave; the records travel in a stream-ordered device table of 24 B each, released behind the launches.
 * Otherwise (NumPy stream, longer stream lists, the exact month, allocation refused): one count-only launch per scenario on
 * internal side streams, joined back onto `hip_stream`.  counts: DEVICE uint64 [n_scenarios][MCR_N_COUNTERS] = {successes,
 * paths} (zeroed by the call).  Asynchronous like mcr_probe_contributions_rng.
 */
typedef struct mcr_scenario { double initial_balance, monthly_contribution, monthly_expenses; } mcr_scenario;
int mcr_probe_scenarios_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                            uint64_t n_paths, int32_t working_months, const mcr_scenario* scenarios,
                            int32_t n_scenarios, uint64_t* counts, int device, void* hip_stream);

/*
 * Market-assumption stress: success counts of SEVERAL records of (initial_balance, monthly_contribution, monthly_expenses, the
 * lognormal parameters of equity, inflation and the premium over inflation, their correlation) at one working-month count over
 * the same path range — the probe of the stress table and of the break-even assumption search.  counts[k] equals, bit for
 * bit, the counters of a count-only mcr_run_batch_rng call with the same arguments and those ten fields of *p replaced by
 * records[k].  records is a HOST array of n_records >= 0 records (0 does nothing; duplicates allowed); every record is held to
 * mcr_validate_params' rules for the same fields (amounts finite and >= 0; finite mu, sigma >= 0 and |mu|/12 + 40
 * sigma/sqrt(12) < 700; rho in [-1, 1]) and everything is validated before anything is enqueued: on an error counts stay
 * untouched and the message names records[k].<field>.  One record: the plain count-only launch.  Philox stream, at most
 * MCR_INLINE_STREAMS income streams, the tolerance month, n_paths <= 2^31 and at least MCR_ASSUMPTION_FANOUT_MIN_WAVES
 * path-wavefronts (environment, default 0): ASSUMPTION FAN-OUT launches, the scenario fan-out's workgroup in which the producer
 * wave stages the path's standard normals (as radius and cosine / sine: they depend on the path alone) and each of up to
 * MCR_MAX_EXPENSE_FANOUT consumer waves applies its own record's market to them — the operations of the plain launch in
 * their order; the records travel in a stream-ordered device table of 80 B each, derived by the host code that derives a
 * parameter block, released behind the launches.  Otherwise (NumPy stream, longer stream lists, the exact month, allocation
 * refused): one count-only launch per record on internal side streams, joined back onto `hip_stream`.  counts: DEVICE uint64
 * [n_records][MCR_N_COUNTERS] = {successes, paths} (zeroed by the call).  Asynchronous like mcr_probe_scenarios_rng.
 * *p itself must pass mcr_validate_params, its own ten fields included, on every route (checked first, with the records).
 * mcr_probe_assumptions_last_fanout_launches reports, for the calling thread's last call, how many assumption fan-out
 * launches it enqueued: ceil(n_records / records per launch) on the fan-out route, 0 on the others and after an error.
 */
typedef struct mcr_assumptions {
    double initial_balance, monthly_contribution, monthly_expenses;
    double inv1_mu_log, inv1_sigma_log, inf_mu_log, inf_sigma_log, prem_mu_log, prem_sigma_log;
    double equity_inflation_rho;
} mcr_assumptions;
int mcr_probe_assumptions_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const mcr_assumptions* records,
                              int32_t n_records, uint64_t* counts, int device, void* hip_stream);
int mcr_probe_assumptions_last_fanout_launches(void);

/*
 * Income options: success counts of SEVERAL versions of ONE income stream (claim at 62, 67 or 70; a larger or smaller
 * annuity; a bridge job of three years or five) at one working-month count over the same path range — the probe of the
 * claiming-option table and of the required-income search.  counts[k] equals, bit for bit, the counters of a count-only
 * mcr_run_batch_rng call with the same arguments and six fields of *p replaced by options[k]: initial_balance,
 * monthly_contribution, monthly_expenses, and monthly_amount_today, start_at_age and duration_years (-1 = None) of entry
 * stream_index of the stream list (the index counts the whole list, extra_streams included).  The stream's tax_rate and
 * inflation_indexed stay the list's own.  options is a HOST array of n_options >= 0 records (0 does nothing; duplicates
 * allowed).  0 <= stream_index < n_streams; the three amounts and monthly_amount_today finite and >= 0 (config.py:56, 57, 59,
 * 18), start_at_age finite and in [0, 120] (config.py `Age`), duration_years >= -1, reserved == 0; everything is validated
 * before anything is enqueued: on an error counts stay untouched and the message names options[k].<field>.  One option: the
 * plain count-only launch.  Philox stream, at most MCR_INLINE_STREAMS kept income streams (the probed one always counts), the
 * tolerance month, n_paths <= 2^31 and at least MCR_INCOME_FANOUT_MIN_WAVES path-wavefronts (environment, default 0): INCOME
 * FAN-OUT launches, the scenario fan-out's workgroup in which each of up to MCR_MAX_EXPENSE_FANOUT consumer waves also carries
 * its own record of the one stream (netted amount, first and last month), derived by the host code that derives a parameter
 * block's stream records; the records travel in a stream-ordered device table of 48 B each, released behind the launches.
 * Otherwise (NumPy stream, longer stream lists, the exact month, allocation refused): one count-only launch per option on
 * internal side streams, joined back onto `hip_stream`.  counts: DEVICE uint64 [n_options][MCR_N_COUNTERS] = {successes,
 * paths} (zeroed by the call).  Asynchronous like mcr_probe_scenarios_rng.
 * mcr_probe_income_last_fanout_launches reports, for the calling thread's last call, how many income fan-out launches it
 * enqueued: ceil(n_options / options per launch) on the fan-out route, 0 on the others and after an error.
 */
typedef struct mcr_income_option {
    double initial_balance, monthly_contribution, monthly_expenses;   /* as mcr_scenario */
    double monthly_amount_today, start_at_age;                        /* of stream `stream_index` */
    int32_t duration_years;                                           /* -1 = None */
    int32_t reserved;                                                 /* 0 */
} mcr_income_option;
int mcr_probe_income_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                         uint64_t n_paths, int32_t working_months, int32_t stream_index,
                         const mcr_income_option* options, int32_t n_options,
                         uint64_t* counts, int device, void* hip_stream);
int mcr_probe_income_last_fanout_launches(void);

/*
 * JOINT OUTCOMES: what the scenario, assumption and income probes know beyond their counts.  Every option of such a probe runs
 * over the SAME paths, so the per-path outcomes of two options are paired: the difference between their success
 * probabilities is known far better than either probability.  The *_joint_rng calls take the arguments of their plain probe
 * (same validation, same routes, `counts` bit for bit the plain probe's) plus
 *   masks:    DEVICE uint64 [n][mcr_joint_mask_words(n_paths)] or NULL.  Row k is option k's success mask: bit b of word w is 1
 *             iff path path_begin + 64 w + b succeeds under option k; bits of paths at or beyond n_paths are 0.  Every word is
 *             written.  NULL: the call keeps the masks in stream-ordered scratch of its own, released behind the work.
 *   joint:    DEVICE uint64 [n][n], required: joint[i][j] = paths on which options i AND j both succeed (symmetric, both
 *             triangles filled; the diagonal is each option's success count = counts[k][MCR_CTR_SUCCESS]).
 *   extremes: DEVICE uint64 [2] or NULL: {paths on which EVERY option succeeds, paths on which NONE does}.
 * n > MCR_MAX_JOINT_OPTIONS or < 0 and a null `joint` are MCR_ERR_INVALID_ARG (the message names the cap), checked first, before
 * the device is touched; n == 0 does nothing.  All outputs are zeroed or overwritten by the call; asynchronous on hip_stream
 * like the plain probes.  On the fan-out route (the plain probe's conditions) the fan-out kernel's consumer waves store their
 * success ballots as the mask words -- no extra launch but the reduction; option lists longer than one launch's share need
 * nothing special, the matrix is counted from the rows afterwards.  Where the plain probe would run one launch per option
 * (NumPy stream, more than MCR_INLINE_STREAMS kept streams, the exact month, one option, the MCR_*_FANOUT_MIN_WAVES knobs) each
 * option's launch also writes its uint8 success column to scratch and a pack kernel turns the column into the mask row.
 * mcr_probe_*_last_fanout_launches report the route as for the plain probes.
 * mcr_joint_counts is the reduction alone, for callers that combine mask rows kept from several probes: joint / extremes as
 * above from n_options rows of mcr_joint_mask_words(n_paths) words.  The kernel clears the bits beyond n_paths of the last
 * word as it reads, so rows need not be tail-clean.  n_paths == 0: zeroes.
 */
uint64_t mcr_joint_mask_words(uint64_t n_paths);   /* (n_paths + 63) / 64 */
int mcr_probe_scenarios_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                  uint64_t n_paths, int32_t working_months, const mcr_scenario* scenarios,
                                  int32_t n_scenarios, uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes,
                                  int device, void* hip_stream);
int mcr_probe_assumptions_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                    uint64_t n_paths, int32_t working_months, const mcr_assumptions* records,
                                    int32_t n_records, uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes,
                                    int device, void* hip_stream);
int mcr_probe_income_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                               uint64_t n_paths, int32_t working_months, int32_t stream_index,
                               const mcr_income_option* options, int32_t n_options,
                               uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes, int device, void* hip_stream);
int mcr_joint_counts(const uint64_t* masks, int32_t n_options, uint64_t n_paths, uint64_t* joint, uint64_t* extremes,
                     int device, void* hip_stream);

/*
 * PER-OPTION OUTCOMES: when a path fails, and what a path that succeeds has left.  The *_outcomes_rng calls take the arguments
 * of their plain probe (same validation, same routes, `counts` bit for bit the plain probe's,
 * mcr_probe_*_last_fanout_launches report as before) plus `rows`, two DEVICE slabs of doubles, [n][path_stride] each:
 *   row k of final_balance = where(success, final_balance, NaN), and row k of years_to_ruin = years_to_ruin (NaN on success),
 *   of a summary mcr_run_batch_rng call with option k's fields replaced -- bit for bit, on every route.
 * years_to_ruin is 0.0 for a pre-retirement tax failure, (month of retirement + 1) / 12 for a failure inside retirement and
 * (double)retirement_years for a failure at the terminal settlement.  Elements of a row at or beyond n_paths are never
 * written.  rows == NULL, or both pointers NULL, is the plain probe.  path_stride < n_paths is MCR_ERR_INVALID_ARG, checked
 * before the device is touched; on any error `counts` and the rows stay untouched.  On the fan-out route the consumer waves of
 * the fan-out kernel store their 64 paths' outcomes in their epilogue (one 512-byte store per wave and row; an option list
 * longer than one launch's share needs nothing special).  Where the plain probe runs one launch per option (NumPy stream, more
 * than MCR_INLINE_STREAMS kept streams, the exact month, one option, the MCR_*_FANOUT_MIN_WAVES knobs) each option's launch is
 * a summary launch into the caller's rows (years_to_ruin into scratch where it is not requested) and a small kernel NaNs the
 * failed paths' final balances.  The final_balance rows are mcr_row_quantiles input as they stand (NaNs are skipped there: the
 * quantiles are those of the successful cohort, and the counts it returns are the success counts).
 * mcr_ruin_month_counts reduces years_to_ruin rows: counts is DEVICE uint64 [n_rows][12 retirement_years + 1], ACCUMULATED
 * into (the caller zeroes it); counts[r][m] += the non-NaN entries y of row r with rint(12 y) == m.  Entries whose month falls
 * outside [0, 12 retirement_years] are dropped (the kernels write none).  One read of the slab; rows of up to 4096 cells
 * (retirement_years <= 341) are counted in an LDS histogram per workgroup and flushed with one 64-bit atomic per non-empty
 * cell, longer rows go straight to global atomics.  n == 0 or n_rows == 0 does nothing; row_stride >= n, retirement_years >= 1.
 */
typedef struct mcr_option_outcomes {
    double* final_balance;   /* DEVICE [n][path_stride] or NULL = not requested */
    double* years_to_ruin;   /* DEVICE [n][path_stride] or NULL = not requested */
    int64_t path_stride;     /* >= n_paths */
} mcr_option_outcomes;
int mcr_probe_scenarios_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                     uint64_t n_paths, int32_t working_months, const mcr_scenario* scenarios,
                                     int32_t n_scenarios, uint64_t* counts, const mcr_option_outcomes* rows,
                                     int device, void* hip_stream);
int mcr_probe_assumptions_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                       uint64_t n_paths, int32_t working_months, const mcr_assumptions* records,
                                       int32_t n_records, uint64_t* counts, const mcr_option_outcomes* rows,
                                       int device, void* hip_stream);
int mcr_probe_income_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                  uint64_t n_paths, int32_t working_months, int32_t stream_index,
                                  const mcr_income_option* options, int32_t n_options,
                                  uint64_t* counts, const mcr_option_outcomes* rows, int device, void* hip_stream);
int mcr_ruin_month_counts(const double* years_to_ruin, int64_t row_stride, int32_t n_rows, int64_t n,
                          int32_t retirement_years, uint64_t* counts, int device, void* hip_stream);

/*
 * Retirement-month x spending grid: counts[c][k] equals, bit for bit, the counters of a count-only mcr_run_batch_rng call with
 * working_months[c] and p->monthly_expenses = monthly_expenses[c][k], everything else unchanged.  working_months: n_candidates
 * >= 0 months (any order, repeats allowed); monthly_expenses: HOST [n_candidates][n_levels] row-major, each finite and >= 0.
 * Every month and level is validated before anything is enqueued (counts stay untouched on an error); n_candidates == 0 or
 * n_levels == 0 does nothing.  Philox stream, at most MCR_INLINE_STREAMS income streams, the tolerance month, 2 ..
 * MCR_MAX_PROBE_CANDIDATES distinct months and at most 4 GiB of snapshots: ONE accumulation sweep stores the state at every
 * distinct month, then one GRID FAN-OUT launch per group of levels resumes every row (grid.y) with one consumer wave per
 * level.  One distinct month: mcr_probe_expenses_rng over the rows' levels.  Otherwise: mcr_probe_expenses_rng per row.
 * counts: DEVICE uint64 [n_candidates][n_levels][MCR_N_COUNTERS] = {successes, paths} (zeroed by the call).  Asynchronous like
 * mcr_probe_months_rng.
 */
int mcr_probe_grid_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                       uint64_t n_paths, const int32_t* working_months, int32_t n_candidates,
                       const double* monthly_expenses, int32_t n_levels, uint64_t* counts, int device, void* hip_stream);

/*
 * YEARLY BINS: the fan chart of any number of paths with no per-path output.  The whole-path kernel runs as for full output, but
 * wherever it would store a yearly sample every lane bins the value on CALLER-SUPPLIED edges instead:
 *   trajectory_bins[t]       <- the nominal balance of yearly sample t            (mcr_outputs.trajectory[t])
 *   real_trajectory_bins[t]  <- the same in today's money                         (mcr_outputs.real_trajectory[t])
 *   wr_bins[y]               <- the withdrawal rate of retirement year y, percent (mcr_outputs.withdrawal_rate_trajectory[y]; NaN
 *                               entries are not counted)
 *   final_success_bins       <- Final Balance of the successful paths
 * Every row has n + 2 cells: cell 0 counts values below edges[0], cells 1 .. n are exactly np.histogram(row, bins=edges) (bin k =
 * [e_k, e_k+1), the last one closed on the right, zero-width bins allowed), cell n + 1 counts values above edges[n].  So every
 * trajectory row sums to the number of paths, wr_bins[y] to wr_obs_counts[y] and final_success_bins to the success counter, and
 * each quantile of a row is known to within one bin.  The values binned are bit for bit those the full-output launch stores.
 * Tables are accumulated into like the counters (the caller zeroes them); any table may be NULL = not requested.  Rows are
 * accumulated per workgroup in LDS and added to the tables with contiguous 64-bit atomic adds: nothing is allocated per path, and a
 * multi-GPU caller that keeps counters and tables in one vector sums everything with ONE all-reduce.
 * edges / wr_edges: [n + 1] ascending finite doubles, n in 1..MCR_MAX_YEAR_BINS (required under a requested table; the *_host
 * forms check finiteness and order, the device form cannot).
 */
typedef struct mcr_year_bins {
    const double* edges;     int32_t n_bins;     /* trajectory, real trajectory, final_success: [n_bins+1] ascending finite */
    const double* wr_edges;  int32_t n_wr_bins;  /* withdrawal rate (percent) */
    uint64_t* trajectory_bins;       /* [T][n_bins+2]   any table may be NULL = not requested */
    uint64_t* real_trajectory_bins;  /* [T][n_bins+2] */
    uint64_t* wr_bins;               /* [ry][n_wr_bins+2] */
    uint64_t* final_success_bins;    /* [n_bins+2] */
} mcr_year_bins;
/* `out` may carry only counters, wr_obs_counts, ruin_year_bins and the hist_* fields (any per-path or trajectory pointer in it:
 * MCR_ERR_INVALID_ARG).  Philox and NumPy streams, every tax variant, stream lists of any length; there are no injected shocks
 * on this route.  Everything is validated before anything is enqueued: on an error the tables are untouched.
 * mcr_run_year_bins_rng: DEVICE pointers in `out` / `yb`, asynchronous on hip_stream like mcr_run_batch_rng.
 * mcr_run_year_bins_host_rng: HOST pointers; leases a pooled context like mcr_run_batch_host_rng; device = a HIP ordinal or
 * MCR_DEVICE_ALL.  mcr_run_year_bins_multi_host_rng: the same over an explicit device list (entries may repeat), sharded and
 * summed on the host like mcr_run_batch_multi_host_rng: the same tables whatever the list. */
int mcr_run_year_bins_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                          int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb, int device, void* hip_stream);
int mcr_run_year_bins_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                               int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb, int device);
int mcr_run_year_bins_multi_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                     uint64_t n_paths, int32_t working_months, const mcr_outputs* out, const mcr_year_bins* yb,
                                     const int32_t* devices, int32_t n_devices);

/*
 * SPENDING RULE: a withdrawal-rate guardrail in the style of Guyton-Klinger.  The reference spends the same real amount every
 * month of retirement whatever the portfolio does; under a rule the household cuts back when it is drawing too fast and loosens
 * up when it is drawing slowly.  Every path carries a spending multiplier m, 1.0 in retirement year 0, and the month's base
 * expenses (simulation.py:645-647) become
 *     expenses = (monthly_expenses * m) * price             in this order: m == 1.0 leaves every bit of the month unchanged
 * Income streams are not scaled.  With
 *     B0 = the path's "Start Balance", P0 = its "inflation_at_retirement" (mcr_outputs),
 *     B, P = the total balance and the price level at the start of retirement year y: the yearly trajectory sample of the end
 *            of year y - 1 (mcr_outputs.trajectory row T - ry + y - 1) and the price level real_trajectory divides it by,
 * the path's real withdrawal rate relative to its initial one is q = m (B0 / P0) / (B / P).  At the start of every retirement
 * year y >= 1 that the path begins alive (it has not failed in an earlier year), in fp64, each operation rounded once:
 *     r0  = B0 / P0                       one IEEE division per path, before the year loop
 *     lhs = (m * r0) * P
 *     if      lhs > upper * B:  m = max(floor,   m * (1.0 - cut))          "q > upper": cut
 *     else if lhs < lower * B:  m = min(ceiling, m * (1.0 + raise))        "q < lower": raise
 *     else                      m unchanged
 * (products, no division in the year loop; upper >= 1 >= lower and B >= 0, so the two tests never both hold; B == 0 with
 * lhs > 0 cuts.)  The rule is inert, m stays 1.0, for a path with B0 <= MCR_SMALL_EPSILON and for a path that failed before
 * retirement (it begins no year).  cut = 0 and raise = 0 give the neutral rule: every result equals the plain launch's.
 * Ranges (mcr_validate_spending_rule; every value finite): upper >= 1, 0 <= lower <= 1, 0 <= cut < 1, raise >= 0,
 * 0 <= floor <= 1 <= ceiling.
 */
typedef struct mcr_spending_rule { double upper, lower, cut, raise, floor, ceiling; } mcr_spending_rule;
/* columns of mcr_rule_outputs.year_counts: per retirement year, over the paths that BEGIN the year alive, after its decision */
#define MCR_RULE_ALIVE 0   /* paths that begin the year */
#define MCR_RULE_CUT 1     /* ... with m < 1 */
#define MCR_RULE_FLOOR 2   /* ... with m <= floor, where floor < 1 */
#define MCR_RULE_RAISED 3  /* ... with m > 1 */
#define MCR_RULE_N_COUNTS 4
typedef struct mcr_rule_outputs {
    uint64_t* year_counts;   /* DEVICE [retirement_years][MCR_RULE_N_COUNTS], ACCUMULATED into like the counters (the caller
                                zeroes it); NULL = not requested */
    double* multipliers;     /* DEVICE [retirement_years][path_stride], time-major like the trajectory slab: m of local path i in
                                year y at [y * path_stride + i], NaN for a year the path does not begin; NULL = not requested */
    int64_t path_stride;     /* >= n_paths (elements); <= 0: n_paths */
} mcr_rule_outputs;
/* Host only (no device needed): MCR_ERR_INVALID_ARG with the offending field named in mcr_last_error(). */
int mcr_validate_spending_rule(const mcr_spending_rule* rule);
/*
 * mcr_run_batch_rng under a spending rule: global paths [path_begin, path_begin + n_paths), DEVICE pointers in `out` and
 * `rule_out`, asynchronous on hip_stream like mcr_run_batch_rng.  `out` carries the counters, wr_obs_counts, ruin_year_bins and
 * the per-path summary columns (start_balance .. success): a count-only launch without them, a summary launch with any of them.
 * rule_out may be NULL.  One plain whole-path launch on the generic tax variant (both assets' tax arithmetic; a zero-rate
 * asset's is exact zeros): under the neutral rule the counters and every summary column equal mcr_run_batch_rng's bit for bit.
 * A path's multipliers are a pure function of (params, seed, stream_id, path): any partition of the path range gives the same
 * rows and year_counts that sum to the whole range's.
 * MCR_ERR_UNSUPPORTED, with a message that names what was asked and nothing computed, for: trajectory pointers in `out`; the
 * in-kernel histogram (hist_bins); the NumPy and history streams; a parameter block that needs the generic variant (more than
 * MCR_INLINE_STREAMS kept income streams, frozen streams beyond the LDS budget, or the exact month of a realized-gains rate
 * above 1 - 1e-6).  There are no injected shocks, time-sliced, split or screened forms of this launch; its yearly-bins form, the
 * fan charts of balance and spending under a rule, is mcr_run_rule_year_bins_rng, and several rules over the same paths are
 * mcr_probe_rules_rng's, both below.
 */
int mcr_run_rule_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                     int32_t working_months, const mcr_spending_rule* rule, mcr_outputs* out, mcr_rule_outputs* rule_out,
                     int device, void* hip_stream);

/*
 * YEARLY BINS UNDER A SPENDING RULE: mcr_run_year_bins_rng's tables for paths that spend (monthly_expenses * m) * price, the fan
 * chart of the balance under a guardrail, and with them the rule's own yearly outputs, still with nothing allocated per path:
 *   year_counts[y]      exactly mcr_run_rule_rng's mcr_rule_outputs.year_counts
 *   multiplier_bins[y]  <- the multiplier m of every path that BEGINS retirement year y alive (the non-NaN entries of row y of
 *                          mcr_rule_outputs.multipliers, bit for bit), on the caller's m_edges, in the cell convention of
 *                          mcr_year_bins (n_m_bins + 2 cells a row): row y sums to year_counts[y][MCR_RULE_ALIVE].  The spending
 *                          fan chart: monthly_expenses * m is the real monthly spending of the year.
 * Both are accumulated into like the other tables; either may be NULL.  trajectory_bins, real_trajectory_bins, wr_bins,
 * final_success_bins, counters, wr_obs_counts and ruin_year_bins mean what they mean in mcr_run_year_bins_rng; under the neutral
 * rule they equal that launch's cell for cell.  Each multiplier bin costs 16 bytes of a workgroup's LDS, like a withdrawal-rate bin.
 */
typedef struct mcr_rule_year_bins {
    const double* m_edges;  int32_t n_m_bins;   /* [n_m_bins+1] ascending finite, n_m_bins in 1..MCR_MAX_YEAR_BINS; required under multiplier_bins */
    uint64_t* multiplier_bins;                  /* [ry][n_m_bins+2], accumulated into; NULL = not requested */
    uint64_t* year_counts;                      /* [ry][MCR_RULE_N_COUNTS], accumulated into; NULL = not requested */
} mcr_rule_year_bins;
/* `out` / `yb` as mcr_run_year_bins_rng takes them, `rule` as mcr_validate_spending_rule checks it.  Everything is validated,
 * on the host and before a device is looked for, before anything is enqueued: on any error every table is untouched.
 * MCR_ERR_UNSUPPORTED, by name and with nothing computed, for what mcr_run_rule_rng refuses: the NumPy and history streams, the
 * in-kernel histogram (hist_bins), more than MCR_INLINE_STREAMS kept income streams, frozen streams beyond the LDS budget and the
 * exact month.  One launch of the generic tax variant, like mcr_run_rule_rng.
 * mcr_run_rule_year_bins_rng: DEVICE pointers in `out` / `yb` / `rule_yb`, asynchronous on hip_stream (the rule travels in a small
 * stream-ordered device record, released behind the launch).
 * mcr_run_rule_year_bins_host_rng: HOST pointers; leases a pooled context on ONE device (a HIP ordinal; there is no multi-device
 * host form: several GPUs sum their tables with one all-reduce); also checks the three edge arrays finite and ascending. */
int mcr_run_rule_year_bins_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                               int32_t working_months, const mcr_spending_rule* rule, const mcr_outputs* out, const mcr_year_bins* yb,
                               const mcr_rule_year_bins* rule_yb, int device, void* hip_stream);
int mcr_run_rule_year_bins_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                    int32_t working_months, const mcr_spending_rule* rule, const mcr_outputs* out, const mcr_year_bins* yb,
                                    const mcr_rule_year_bins* rule_yb, int device);

/*
 * Rule options: SEVERAL spending rules (and versions of the scenario probe's three fields) at one working-month count over the
 * same path range -- a tight band with small cuts against a wide band with large ones, cut-only, fixed spending -- the probe of
 * the rule comparison table and of the rule's spending search.  Row k of counts and of year_counts equals, bit for bit, the
 * counters and the year_counts of a count-only mcr_run_rule_rng call with the same arguments, initial_balance,
 * monthly_contribution and monthly_expenses of *p replaced by options[k]'s, and rule = options[k].rule.
 *   counts:      DEVICE uint64 [n_options][MCR_N_COUNTERS] = {successes, paths};
 *   year_counts: DEVICE uint64 [n_options][retirement_years][MCR_RULE_N_COUNTS] or NULL = not requested.
 * Both are ZEROED by the call (like every probe's counts; mcr_run_rule_rng accumulates).  options is a HOST array of
 * n_options >= 0 records (0 does nothing; duplicates allowed).  The three amounts finite and >= 0 (config.py:56, 57, 59), every
 * rule in mcr_validate_spending_rule's ranges; everything is validated on the host before the device is touched and before
 * anything is enqueued: on any error every output stays untouched and the message names options[k].<field> or
 * options[k].rule.<field>.
 * What mcr_run_rule_rng refuses is refused here, MCR_ERR_UNSUPPORTED with nothing computed: the NumPy and history streams, more
 * than MCR_INLINE_STREAMS kept income streams, frozen streams beyond the LDS budget, the exact month.  There is no route for
 * them to fall back to.  One option: the plain rule launch.  Otherwise, with n_paths <= 2^31 and at least
 * MCR_RULE_FANOUT_MIN_WAVES path-wavefronts (environment, default 0, read per call): RULE FAN-OUT launches, the scenario
 * fan-out's workgroup in which each of up to MCR_MAX_EXPENSE_FANOUT consumer waves also carries its own rule and multiplier;
 * the records (the three amounts, upper, lower, 1 - cut, 1 + raise, floor, ceiling) travel in a stream-ordered device table of
 * 72 B each, released behind the launches.  Where the knob rules the fan-out out: one mcr_run_rule_rng launch per option on
 * internal side streams, joined back onto `hip_stream`.  No multiplier rows in this form.  Asynchronous like
 * mcr_probe_scenarios_rng.
 * mcr_probe_rules_joint_rng and mcr_probe_rules_outcomes_rng add the arguments of mcr_probe_scenarios_joint_rng and
 * mcr_probe_scenarios_outcomes_rng with their contracts (JOINT OUTCOMES and PER-OPTION OUTCOMES above; the cap
 * MCR_MAX_JOINT_OPTIONS and a null `joint`, and rows->path_stride < n_paths, are checked first): the mask rows are the success
 * columns, and the rows are where(success, final_balance, NaN) and years_to_ruin, of summary mcr_run_rule_rng launches of the
 * options, bit for bit on both routes; elements of a row at or beyond n_paths are never written.
 * mcr_probe_rules_last_fanout_launches reports, for the calling thread's last call, how many rule fan-out launches it
 * enqueued: ceil(n_options / options per launch) on the fan-out route, 0 on the others and after an error.
 */
typedef struct mcr_rule_option {
    double initial_balance, monthly_contribution, monthly_expenses;   /* as mcr_scenario */
    mcr_spending_rule rule;
} mcr_rule_option;                                                     /* 72 bytes */
int mcr_probe_rules_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                        uint64_t n_paths, int32_t working_months, const mcr_rule_option* options, int32_t n_options,
                        uint64_t* counts, uint64_t* year_counts, int device, void* hip_stream);
int mcr_probe_rules_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const mcr_rule_option* options, int32_t n_options,
                              uint64_t* counts, uint64_t* year_counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes,
                              int device, void* hip_stream);
int mcr_probe_rules_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                 uint64_t n_paths, int32_t working_months, const mcr_rule_option* options, int32_t n_options,
                                 uint64_t* counts, uint64_t* year_counts, const mcr_option_outcomes* rows,
                                 int device, void* hip_stream);
int mcr_probe_rules_last_fanout_launches(void);

/*
 * Retirement-month x spending grid UNDER ONE SPENDING RULE: how much sooner can I retire if I accept the guardrail?  The probe of
 * the month search and of the max-spending frontier under a rule.  Cell [c][k] of counts and of year_counts equals, bit for
 * bit, the counters and the year_counts of a count-only mcr_run_rule_rng call at working_months[c] with p->monthly_expenses =
 * monthly_expenses[c][k] under `rule`, over the same path range; under the neutral rule (cut = raise = 0) the counters are
 * mcr_probe_grid_rng's.
 *   working_months:   n_candidates >= 0 months (any order, repeats allowed);
 *   monthly_expenses: HOST [n_candidates][n_levels] row-major, each finite and >= 0 (config.py:59);
 *   counts:           DEVICE uint64 [n_candidates][n_levels][MCR_N_COUNTERS] = {successes, paths};
 *   year_counts:      DEVICE uint64 [n_candidates][n_levels][retirement_years][MCR_RULE_N_COUNTS] or NULL = not requested.
 * Both are ZEROED by the call.  n_candidates == 0 or n_levels == 0 does nothing.  Every month, every level and the rule
 * (mcr_validate_spending_rule's ranges) are validated on the host before a device is looked for and before anything is
 * enqueued: on any error both outputs stay untouched.  What mcr_run_rule_rng refuses is refused here by the same words,
 * MCR_ERR_UNSUPPORTED with nothing computed: the NumPy and history streams, more than MCR_INLINE_STREAMS kept income streams,
 * frozen streams beyond the LDS budget, the exact month.
 * A rule acts only after retirement, so the grid probe's form fits: with 2 .. MCR_MAX_PROBE_CANDIDATES distinct months, n_paths
 * <= 2^31, at least MCR_EXPENSE_FANOUT_MIN_WAVES path-wavefronts (the grid probe's knob) and at most 4 GiB of snapshots, ONE
 * accumulation sweep (the grid probe's own) stores the state at every distinct month, then one RULE GRID FAN-OUT launch per group
 * of levels resumes every row (grid.y) with one consumer wave per level; each wave carries its lanes' multiplier from the resumed
 * balance and price level and counts its own years.  The rows' records (the grid's record, upper, lower, 1 - cut, 1 + raise,
 * floor, ceiling, the row's year counts) travel behind the snapshots in the same stream-ordered allocation.  The kernels are the
 * generic tax mask's, like every rule kernel.  Any other shape, one distinct month included: mcr_probe_rules_rng per row over the
 * row's levels.  Whichever route runs, the integers are the same.  Asynchronous like mcr_probe_grid_rng.
 * mcr_probe_rule_grid_last_fanout_launches reports, for the calling thread's last call, how many rule grid fan-out launches it
 * enqueued: the number of level groups on the shared route, 0 on the per-row route and after an error.
 */
int mcr_probe_rule_grid_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                            uint64_t n_paths, const int32_t* working_months, int32_t n_candidates,
                            const double* monthly_expenses, int32_t n_levels, const mcr_spending_rule* rule,
                            uint64_t* counts, uint64_t* year_counts, int device, void* hip_stream);
int mcr_probe_rule_grid_last_fanout_launches(void);

/*
 * Allocation options: SEVERAL splits between the two assets (and versions of the scenario probe's three fields) at one
 * working-month count over the same path range -- how should the money be divided?  The probe of the allocation comparison
 * table and of the best-split search.  counts[k] equals, bit for bit, the counters of a count-only mcr_run_batch_rng call with
 * the same arguments and initial_balance, monthly_contribution, monthly_expenses and allocation_inv1_pct of *p replaced by
 * options[k]'s; the second asset's weight is 1.0 - allocation_inv1_pct, the operation the plain launch performs on its block.
 *   counts: DEVICE uint64 [n_options][MCR_N_COUNTERS] = {successes, paths}, ZEROED by the call.
 * options is a HOST array of n_options >= 0 records (0 does nothing; duplicates allowed).  Everything is validated on the host
 * before a device is looked for and before anything is enqueued: *p by mcr_validate_params' rules, the three amounts finite and
 * >= 0 (config.py:56, 57, 59), the allocation finite and in [0, 1] (config.py:70); on any error every output stays untouched
 * and the message names options[k].<field>.
 * One option: the plain count-only launch.  Otherwise, on the Philox stream with at most MCR_INLINE_STREAMS kept income streams,
 * every lock slot in LDS, the tolerance month, n_paths <= 2^31 and at least MCR_ALLOCATION_FANOUT_MIN_WAVES path-wavefronts
 * (environment, default 0, read per call): ALLOCATION FAN-OUT launches, the scenario fan-out's workgroup in which each of up to
 * MCR_MAX_EXPENSE_FANOUT consumer waves also carries its own pair of weights; the 32-byte records are the stream-ordered device
 * table as they come, released behind the launches.  Any other shape (the NumPy and history streams, longer stream lists, the
 * exact month, a refused allocation of the table): one count-only launch per option on internal side streams, joined back onto
 * `hip_stream`.  Whichever route runs, the integers are the same.  Asynchronous like mcr_probe_scenarios_rng.
 * mcr_probe_allocations_joint_rng and mcr_probe_allocations_outcomes_rng add the arguments of mcr_probe_scenarios_joint_rng and
 * mcr_probe_scenarios_outcomes_rng with their contracts (JOINT OUTCOMES and PER-OPTION OUTCOMES above; the cap
 * MCR_MAX_JOINT_OPTIONS and a null `joint`, and rows->path_stride < n_paths, are checked first): the mask rows are the success
 * columns, and the rows are where(success, final_balance, NaN) and years_to_ruin, of summary launches of the options, bit for
 * bit on both routes; elements of a row at or beyond n_paths are never written.
 * mcr_probe_allocations_last_fanout_launches reports, for the calling thread's last call, how many allocation fan-out launches
 * it enqueued: ceil(n_options / options per launch) on the fan-out route, 0 on the others and after an error.
 */
typedef struct mcr_allocation_option {
    double initial_balance, monthly_contribution, monthly_expenses;   /* as mcr_scenario */
    double allocation_inv1_pct;                                       /* config.py:70, in [0, 1] */
} mcr_allocation_option;                                              /* 32 bytes */
int mcr_probe_allocations_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const mcr_allocation_option* options, int32_t n_options,
                              uint64_t* counts, int device, void* hip_stream);
int mcr_probe_allocations_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                    uint64_t n_paths, int32_t working_months, const mcr_allocation_option* options, int32_t n_options,
                                    uint64_t* counts, uint64_t* masks, uint64_t* joint, uint64_t* extremes,
                                    int device, void* hip_stream);
int mcr_probe_allocations_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                       uint64_t n_paths, int32_t working_months, const mcr_allocation_option* options, int32_t n_options,
                                       uint64_t* counts, const mcr_option_outcomes* rows, int device, void* hip_stream);
int mcr_probe_allocations_last_fanout_launches(void);

/*
 * GLIDE PATH: a split between the two assets that changes with the calendar.  A glide path is a table W[0 .. n - 1], n >= 1, of
 * values of allocation_inv1_pct, every entry finite and in [0, 1], indexed by WHOLE YEARS FROM TODAY.  Let row t be the 0-based
 * month from today: accumulation month m (simulation.py:513) is row m - 1, retirement month rmi (simulation.py:641) is row
 * working_months + rmi.  The weight in force while row t is processed is
 *     w(t)   = W[min(t div 12, n - 1)]
 *     alloc2 = 1.0 - w(t)                      the operation the plain launch performs on its block, rounded once
 * and it stands in every place the path reads a weight: the initial split reads W[0]; the contribution split, the monthly
 * rebalance, the dust sub-case of the withdrawal proportion (capacity <= MCR_SMALL_EPSILON) and the annual-gains tax with its
 * closing rebalance read w(t) of the row being processed (the annual tax closes row t when (t + 1) % 12 == 0); the terminal
 * settlement uses the last row's weight, w(total_months - 1).  The weight changes only where t % 12 == 0, t > 0: the closes of
 * calendar years from today, NOT the retirement-year boundaries unless working_months % 12 == 0 -- so a table means the same
 * thing at every working-month count.  A table of length 1, or with all entries equal, is a constant split: every result is
 * the allocation probe's, bit for bit.  Entries past the horizon are never read; a table shorter than the horizon holds its
 * last entry.  Paths that have failed read no weight.
 *
 * Glide probes: SEVERAL glide paths (and versions of the scenario probe's three fields) at one working-month count over the
 * same path range.  `weights` is a HOST array of n_weights doubles, the tables of all options one behind the other in any
 * order (they may overlap or be shared); option k's table is weights[first_weight .. first_weight + n_weights).
 *   counts: DEVICE uint64 [n_options][MCR_N_COUNTERS] = {successes, paths}, ZEROED by the call.
 * options is a HOST array of n_options >= 0 records (0 does nothing; duplicates allowed).  Everything is validated on the host
 * before a device is looked for and before anything is enqueued: *p by mcr_validate_params' rules, the three amounts finite and
 * >= 0, options[k].n_weights >= 1, options[k].first_weight >= 0 and first_weight + n_weights within the table, and every weight
 * an option names finite and in [0, 1]; on any error every output stays untouched and the message names options[k].<field> (a
 * weight: options[k].weights[i]).
 * The probes run every option, a single one included, in GLIDE FAN-OUT launches (the whole-path launches further down take ONE
 * table; the probes never route through them): the allocation fan-out's workgroup in which each of up to MCR_MAX_EXPENSE_FANOUT consumer waves carries its own table and reloads
 * its weight once a calendar year with one scalar load.  The records, with the weights behind them, are ONE stream-ordered
 * device table, released behind the launches.  The shapes the fan-out does not cover have no per-option route here and return
 * MCR_ERR_UNSUPPORTED, every output untouched, with a message that says which: the NumPy stream, the history stream, stream
 * lists longer than MCR_INLINE_STREAMS or lock slots beyond LDS (the generic variant), the exact month, n_paths > 2^31, fewer
 * than MCR_GLIDE_FANOUT_MIN_WAVES path-wavefronts (environment, default 0, read per call).  (A refused allocation of the device
 * table also returns MCR_ERR_UNSUPPORTED, with the counters zeroed.  n_paths == 0 zeroes the counters, and the joint form's
 * matrix and extremes, and launches nothing.)  Asynchronous like mcr_probe_scenarios_rng.
 * mcr_probe_glide_paths_joint_rng and mcr_probe_glide_paths_outcomes_rng add the arguments of mcr_probe_scenarios_joint_rng and
 * mcr_probe_scenarios_outcomes_rng with their contracts (the cap MCR_MAX_JOINT_OPTIONS and a null `joint`, and
 * rows->path_stride < n_paths, are checked first); elements of a row at or beyond n_paths are never written.
 * mcr_probe_glide_paths_last_fanout_launches reports, for the calling thread's last call, how many glide fan-out launches it
 * enqueued: ceil(n_options / options per launch), 0 after an error.
 * The probes return counts, ballots and outcome rows only; the summary columns and the yearly tables of ONE glide path come from
 * the whole-path launches below.
 *
 * Glide whole-path launches: ONE glide path over a path range, as a plain launch of the engine's own stream (every wave of the
 * launch stands in the same row, so the weight in force is launch-uniform and its yearly reload one scalar load).  `weights` is a
 * HOST array of n_weights >= 1 doubles, the table W; the launch keeps it in a small stream-ordered device block, released behind
 * the kernel.  *p's allocation_inv1_pct is not read on the path (derived values that do not depend on it are).
 *   mcr_run_glide_rng: `out` follows mcr_run_rule_rng's contract -- DEVICE counters, wr_obs_counts, ruin_year_bins (accumulated
 *     into) and any of the per-path summary columns; count-only without a summary column, a summary launch with any of them.
 *   mcr_run_glide_year_bins_rng / _host_rng: mcr_run_year_bins_rng / _host_rng exactly -- the cell convention, tables accumulated
 *     into, any table NULL, DEVICE pointers in the first and HOST pointers (edges checked) in the second, which runs on one device.
 * Everything is validated on the host before a device is looked for: *p and the month, the stream descriptor, n_weights >= 1,
 * every weight finite and in [0, 1] (the message names weights[i]), and in the yearly-bins forms whatever mcr_run_year_bins_rng
 * checks of `out` / `yb`.  On any error every output is untouched.  MCR_ERR_UNSUPPORTED, by name and with nothing computed
 * ("glide path: ... is not supported"): trajectory pointers, hist_bins, the NumPy and the history stream, stream lists longer than
 * MCR_INLINE_STREAMS or lock slots beyond LDS (the generic variant), the exact month.  (A yearly-bins launch keeps the lock
 * columns of frozen income streams beside its tables in the workgroup's LDS and gives up resident workgroups where the plain
 * launch would take its generic form; only columns beyond the workgroup's 64 KB are refused.)  A table whose every entry
 * equals *p's allocation_inv1_pct gives mcr_run_batch_rng's / mcr_run_year_bins_rng's results for *p bit for bit (a one-entry table
 * of another value a gives them for *p with allocation_inv1_pct = a); any table
 * gives, path for path, what the glide probes report for the same option.  Asynchronous like mcr_run_batch_rng (the host form
 * returns with its tables filled).
 * Not offered under a glide path: trajectories, a spending rule together with a glide path, time-sliced, split and screened
 * forms, the NumPy and history streams, and a retirement-month grid or any search (the probes' records carry their own three
 * amounts for that).
 */
typedef struct mcr_glide_option {
    double initial_balance, monthly_contribution, monthly_expenses;   /* as mcr_scenario */
    int32_t first_weight;                                             /* index of W[0] in `weights` */
    int32_t n_weights;                                                /* n >= 1 */
} mcr_glide_option;                                                   /* 32 bytes */
int mcr_probe_glide_paths_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                              uint64_t n_paths, int32_t working_months, const double* weights, int32_t n_weights,
                              const mcr_glide_option* options, int32_t n_options, uint64_t* counts, int device, void* hip_stream);
int mcr_probe_glide_paths_joint_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                    uint64_t n_paths, int32_t working_months, const double* weights, int32_t n_weights,
                                    const mcr_glide_option* options, int32_t n_options, uint64_t* counts, uint64_t* masks,
                                    uint64_t* joint, uint64_t* extremes, int device, void* hip_stream);
int mcr_probe_glide_paths_outcomes_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin,
                                       uint64_t n_paths, int32_t working_months, const double* weights, int32_t n_weights,
                                       const mcr_glide_option* options, int32_t n_options, uint64_t* counts,
                                       const mcr_option_outcomes* rows, int device, void* hip_stream);
int mcr_probe_glide_paths_last_fanout_launches(void);
int mcr_run_glide_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                      int32_t working_months, const double* weights, int32_t n_weights, mcr_outputs* out, int device, void* hip_stream);
int mcr_run_glide_year_bins_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                int32_t working_months, const double* weights, int32_t n_weights, const mcr_outputs* out,
                                const mcr_year_bins* yb, int device, void* hip_stream);
int mcr_run_glide_year_bins_host_rng(const mcr_params* p, const mcr_rng* rng, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                     int32_t working_months, const double* weights, int32_t n_weights, const mcr_outputs* out,
                                     const mcr_year_bins* yb, int device);

/* _draw_shock_path (simulation.py:452-466) for n_paths paths: host out [n_paths][n_months][3]. */
int mcr_draw_shocks_host(uint64_t seed, uint32_t stream_id, uint64_t path_begin,
                         uint64_t n_paths, int32_t n_months, double rho, double* out,
                         int device);

/* ---- device unit functions (the scalar helpers the reference's tests call directly) ---- */
#define MCR_HELPER_WITHDRAW 0      /* _calculate_withdrawal_and_update :201-254; in[5]=(bal,cb,net_target,use_real,rate) out[4]=(bal,cb,gross,net) */
#define MCR_HELPER_NLV 1           /* _net_liquidation_value :256-272;           in[4]=(bal,cb,use_real,rate) out[1] */
#define MCR_HELPER_REBALANCE 2     /* _rebalance_portfolio :274-359;             in[4]=(b1,cb1,b2,cb2) out[4] */
#define MCR_HELPER_ANNUAL_TAX 3    /* _apply_annual_gain_taxes :361-450;         in[6]=(b1,cb1,b2,cb2,g1,g2) out[5]=(b1,cb1,b2,cb2,tax_failed) */
#define MCR_HELPER_MONTHLY_GROSS 4 /* _monthly_gross_from_shock :468-474;        in[3]=(mu_log,sigma_log,z) out[1] */
/* the kernel's specialised fp64 math (csrc/mcr_math.h), exposed so its accuracy can be measured */
#define MCR_HELPER_MATH_EXP 5      /* in[1]=(x)            out[1]=exp(x)                              */
#define MCR_HELPER_MATH_DIV 6      /* in[2]=(a,b)          out[1]=a/b (Newton sequence, no scaling)   */
#define MCR_HELPER_MATH_SQRT 7     /* in[1]=(w)            out[1]=sqrt(w)                             */
#define MCR_HELPER_MATH_NEG2LOG 8  /* in[1]=(x as uint32)  out[1]=-2 ln((x+0.5) 2^-32)                */
#define MCR_HELPER_MATH_SINCOS 9   /* in[1]=(x as uint32)  out[2]=(sin, cos)(2 pi (x+0.5) 2^-32)      */
#define MCR_HELPER_MATH_DIV_PATH 10 /* in[2]=(a,b)         out[1]=a/b as the path kernel divides (1 Newton step) */
/* The PATH FORMS of the state-machine helpers — the code the path kernel actually runs (clamps that are provable no-ops
 * on reachable states dropped, selections as masked moves, compile-time tax variants chosen from the parameter block as
 * the launcher does).  Inputs must be reachable states: balances and cost bases >= 0, targets >= 0.  Rates, allocation
 * and the tax systems come from the parameter block. */
#define MCR_HELPER_WITHDRAW2_PATH 11  /* in[6]=(b1,cb1,target1,b2,cb2,target2) out[8]=(b1,cb1,gross1,net1,b2,cb2,gross2,net2) */
#define MCR_HELPER_NLV2_PATH 12       /* in[4]=(b1,cb1,b2,cb2) out[2] */
#define MCR_HELPER_REBALANCE_PATH 13  /* in[4]=(b1,cb1,b2,cb2) out[4] */
#define MCR_HELPER_ANNUAL_TAX_PATH 14 /* in[6]=(b1,cb1,b2,cb2,g1,g2) out[5]=(b1,cb1,b2,cb2,tax_failed) */
/* the PATH FORMS of the math (shorter series inside the month loop: their truncation errors are sized to the 1e-9 path
 * tolerance instead of the last ulp — csrc/mcr_math.h; bounds measured in tests/test_gpu_math.py) */
#define MCR_HELPER_MATH_EXP_PATH 15     /* in[1]=(x)            out[1]=exp(x), r^2/24 -> a^2/40 (|err| <= 3.5e-15, mean 0) */
#define MCR_HELPER_MATH_NEG2LOG_PATH 16 /* in[1]=(x as uint32)  out[1]=-2 ln((x+0.5) 2^-32), series to r^4 (<= 3.6e-13 absolute) */
#define MCR_HELPER_MATH_SINCOS_PATH 17  /* in[1]=(x as uint32)  out[2]=(sin, cos), cos series to dl^4 (<= 4.7e-15 absolute)  */
/* The month as the path kernel RUNS it since ABI v7 (csrc/mcr_device.h, "TOLERANCE FORM of the month"): the reference's
 * formulas in closed form — both assets sell the fraction target / capacity of their balance, the rebalance is one quotient —
 * with fused multiply-adds and uncorrected reciprocals: equal to the reference's arithmetic up to roundings (~1e-16 relative per
 * operation) while both effective realized-gains rates are <= 1 - 1e-6; parameter blocks with a higher rate run the exact path
 * forms above (the reference's denominator clamps, simulation.py:227,:307-310, can bind there), and so do these two helpers. */
#define MCR_HELPER_WITHDRAW_MONTH 18   /* :726-790  in[5]=(b1,cb1,b2,cb2,need) out[6]=(b1,cb1,b2,cb2,gross withdrawn,net cash) */
#define MCR_HELPER_REBALANCE_MONTH 19  /* :274-359  in[4]=(b1,cb1,b2,cb2) out[4] */
/* exp's path form as the general kernels run it and in its narrow-window form (csrc/mcr_math.h: fexp<., NARROW>, for
 * k = rint(x 512 / ln 2) in [-256, 255]; the two agree bit for bit there — tests/test_gpu_growth_forms.py) */
#define MCR_HELPER_MATH_EXP_FORMS 20   /* in[1]=(x)  out[2]=(general form, narrow form) */
/* Evaluates helper `which` ON THE DEVICE for n rows (host buffers, row-major). */
int mcr_eval_helper_host(int which, const mcr_params* p, const double* in, double* out,
                         int64_t n, int device);

/* ---- device-side aggregation (replaces the pandas block, simulation.py:1045-1118) ---- */
/*
 * Row-wise quantiles with pandas' semantics (linear interpolation between order statistics,
 * NaNs skipped): for each of n_rows rows of `n` doubles at rows[r*row_stride + i], writes
 * out[r*n_q + j] = quantile(q[j]) (NaN for an all-NaN row) and, if counts != NULL,
 * counts[r] = number of non-NaN entries.  rows/out/counts are DEVICE pointers (out / counts may also be pinned,
 * device-visible host memory — a few KB the kernels write directly: no download after the call); q is HOST.
 * scratch: device buffer of mcr_row_quantiles_scratch_bytes(n_rows, n_q, n) bytes (selection state, digit and
 * sub-bin histograms, per-row candidate buffers of n/64 + 4096 keys and n/8 + 4096 values, cell lists); 0 =
 * unsupported shape.
 *
 * mcr_row_quantiles picks the route by row length.  Short rows: the exact radix select (8 digit passes,
 * 4 of them over the slab), fully asynchronous.  Rows of >= 2^14 entries, SEVEN launches: the first 4096 entries of
 * every row are sorted in LDS (coarse brackets); a counting pass over a sample (the first n/32 entries) and a small
 * per-row kernel turn them into fine brackets; ONE pass over the slab counts the entries around the brackets (with
 * sub-histograms inside them) and compacts the few % inside — two kernels side by side: rows whose bracket bounds fit a
 * 2048-bucket value table take the table-driven one (-0.0 is counted and returned as +0.0 there), the others a generic
 * search; two per-row kernels locate every target in one
 * sub-bin, collect that bin's keys and select among them.  Rows whose counts do not prove their brackets right
 * take the radix passes afterwards.  The result is exact on either route.  The second route reads one word back
 * from the device (how many rows need the radix passes): it synchronises hip_stream ONCE per call.
 * mcr_row_quantiles_last_fallback_rows reports, for the calling thread's last call, -1 (radix route) or the
 * number of rows that needed the radix passes (diagnostics / tests).
 */
int64_t mcr_row_quantiles_scratch_bytes(int32_t n_rows, int32_t n_q, int64_t n);
/*
 * The same selection as separate steps, for rows SHARDED across GPUs (each rank holds n_local of the
 * n_total entries of every row): begin once, then for pass = 0..7: hist (rank-local digit histograms;
 * pass 3 also compacts candidates) -> the caller sums the dense 32-bit counter block of the scratch
 * buffer across ranks (byte offset / word count from mcr_row_quantiles_reduce_block; one small
 * all-reduce per pass, the trajectories themselves never move) -> scan (identical on every rank).
 * After pass 7, `out`/`counts` hold the exact global quantiles on every rank.
 */
int64_t mcr_row_quantiles_reduce_block(int32_t n_rows, int64_t* n_words);
int mcr_row_quantiles_begin(void* scratch, int32_t n_rows, int device, void* hip_stream);
int mcr_row_quantiles_hist(const double* rows, int64_t row_stride, int32_t n_rows, int64_t n_local, int32_t n_q,
                           int32_t pass, void* scratch, int device, void* hip_stream);
int mcr_row_quantiles_scan(int32_t n_rows, int64_t n_total, const double* q, int32_t n_q, int32_t pass, double* out,
                           uint64_t* counts, void* scratch, int device, void* hip_stream);
int mcr_row_quantiles(const double* rows, int64_t row_stride, int32_t n_rows, int64_t n,
                      const double* q, int32_t n_q, double* out, uint64_t* counts,
                      void* scratch, int device, void* hip_stream);
int mcr_row_quantiles_last_fallback_rows(void);
/*
 * The bracketed route for rows SHARDED across GPUs (rank r holds n_local of the n_total entries of every row; the
 * trajectories never move).  Between its stages the library calls `reduce(ctx, device_buf, count, dtype)`, which
 * must SUM the `count` elements of `device_buf` (MCR_DT_I32: int32, MCR_DT_I64: int64; always inside `scratch`)
 * across all ranks, in place, ordered after the work already enqueued on hip_stream (an RCCL all-reduce on that stream,
 * or a synchronising host implementation), and return 0.  About ten such calls per invocation, the largest the two
 * sub-histogram blocks (n_rows * 64 KiB) and the cell lists (n_rows * 96 KiB).  Every rank must call with the same
 * n_rows, n_total, q; every rank returns the same exact quantiles.  Needs rank 0 to hold >= 4096 entries, world <= 64,
 * fewer than 16 quantiles: otherwise MCR_ERR_UNSUPPORTED (use the stepwise radix select above) — on EVERY rank: the one
 * condition that depends on a single rank's shard (rank 0's first sample) is agreed through the first `reduce` call, so no
 * rank leaves while its peers wait in a collective.  A `reduce` callback that fails on one rank only is the caller's to
 * avoid (the peers would wait in the collective it skipped).  Synchronises hip_stream a few times.
 * scratch: mcr_row_quantiles_scratch_bytes(n_rows, n_q, n_local).
 */
#define MCR_DT_I32 0
#define MCR_DT_I64 1
typedef int (*mcr_reduce_fn)(void* ctx, void* device_buf, int64_t count, int32_t dtype);
int mcr_row_quantiles_sharded(const double* rows, int64_t row_stride, int32_t n_rows, int64_t n_local, int64_t n_total,
                              const double* q, int32_t n_q, double* out, uint64_t* counts, void* scratch, int32_t rank,
                              int32_t world, mcr_reduce_fn reduce, void* reduce_ctx, int device, void* hip_stream);

/*
 * Histogram of final balances over the successful cohort (the CLI's 100-bin chart,
 * backend/plotting.py:53-59, np.histogram semantics: n_bins equal-width bins over
 * [lo, hi], last bin closed).  values/success: DEVICE [n].  minmax: DEVICE [2] doubles;
 * if use_given_range == 0 the kernel first reduces min/max of the cohort into it.
 * bins: DEVICE [n_bins] uint64, accumulated into (caller zeroes).
 */
int mcr_minmax_success(const double* values, const uint8_t* success, int64_t n,
                       double* minmax, int device, void* hip_stream);
int mcr_histogram_success(const double* values, const uint8_t* success, int64_t n,
                          const double* minmax, int32_t n_bins, uint64_t* bins,
                          int device, void* hip_stream);

/*
 * Rows for the summary statistics of the response document (backend/server.py:446-458 and
 * median_first_year_withdrawal_rate, backend/simulation.py:78-96), laid out for mcr_row_quantiles
 * (which skips NaN exactly as pandas' median/quantile do):
 *   row 0 = Start Balance                      row 1 = Final Balance
 *   row 2 = Final Balance where Success, else NaN
 *   row 3 = First Year Real Gross Withdrawal / Start Balance * 100 where Start Balance > 1e-6, else NaN
 * Inputs: DEVICE [n].  rows: DEVICE [4][row_stride] (row_stride >= n).
 */
#define MCR_N_STAT_ROWS 4
int mcr_summary_stat_rows(const double* start_balance, const double* final_balance,
                          const double* first_year_real_gross, const uint8_t* success, int64_t n,
                          double* rows, int64_t row_stride, int device, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MCR_H_ */
