#!/usr/bin/env python3
"""CLI-shaped caller of the drop-in simulator: the reference's run flow (backend/server.py:231-266 and the
SSE body :341-394; backend/main.py:54-133 follows the same sequence) through
`monte_carlo_retirement_amd.results.run_scenario` — load a scenario JSON, search the minimum working months,
switch to the final seed stream, run the final batch, print the response document.

    python examples/run_scenario.py scenarios/jorge.json --seed 12345 --rng numpy
    python examples/run_scenario.py scenarios/config.json --paths 10000000 --working-months 233 --compact
    python examples/run_scenario.py scenarios/config.json --events --full > response.json
    python examples/run_scenario.py scenarios/config.json --working-months 240 --max-expenses
    python examples/run_scenario.py scenarios/config.json --working-months 180 --min-contribution
    python examples/run_scenario.py scenarios/config.json --min-initial-balance
    python examples/run_scenario.py scenarios/config.json --min-initial-balance --at-expenses 3000,4000,5000
    python examples/run_scenario.py scenarios/config.json --working-months 240 --income-options "State Pension" \
        --claim-ages 62,67,70 --claim-amounts 2800,4000,4960
    python examples/run_scenario.py scenarios/config.json --working-months 240 --min-income "State Pension" --claim-age 67
    python examples/run_scenario.py scenarios/config.json --working-months 240 --stress
    python examples/run_scenario.py scenarios/config.json --working-months 240 --breakeven inv1_returns_mean,inflation_rate_mean
    python examples/run_scenario.py scenarios/config.json --frontier 180,240,300
    python examples/run_scenario.py scenarios/config.json --grid-months 180,240 --grid-expenses 3000,4000,5000
    python examples/run_scenario.py scenarios/config.json --history record.csv --history-block 12 [--history-as-recorded]
    python examples/run_scenario.py scenarios/config.json --history record.csv --history-scheme stationary
    python examples/run_scenario.py scenarios/config.json --history record.csv --history-scheme cohorts \
        --history-first-month 1926-01 --working-months 240 --cohorts
    python examples/run_scenario.py scenarios/config.json --working-months 240 --spending-rule 1.2,0.8,0.1,0.1,0.5,1.5 [--max-expenses]
    python examples/run_scenario.py scenarios/config.json --working-months 240 --spending-rule 1.2,0.8,0.1,0.1,0.5,1.5 --streamed
    python examples/run_scenario.py scenarios/config.json --spending-rule 1.2,0.8,0.1,0.1,0.5,1.5 --earliest-retirement
    python examples/run_scenario.py scenarios/config.json --spending-rule 1.2,0.8,0.1,0.1,0.5,1.5 --frontier 180,240,300
    python examples/run_scenario.py scenarios/config.json --working-months 240 --allocations 0,0.2,0.4,0.6,0.8,1 [--paired] [--outcomes]
    python examples/run_scenario.py scenarios/config.json --working-months 240 --best-allocation [--allocation-resolution 0.01]
    python examples/run_scenario.py scenarios/config.json --working-months 240 --glide-paths "0.9>0.4@0-20;0.6;0.3>0.6@20-35" [--paired] [--outcomes]
    python examples/run_scenario.py scenarios/config.json --working-months 240 --glide-path "0.9>0.4@0-20" --streamed

`--rng numpy` uses the reference's own NumPy stream (same seed -> the reference's numbers); `--rng philox`
(default) the engine's counter-based stream.  `--history FILE.csv` asks every question of a recorded market instead: months
resampled in blocks of `--history-block` (default 12) from the file's columns `equity`, `inflation` and `inv2` (simple monthly
returns, one row per month, oldest first; `premium` instead of `inv2` when the file holds the premium over inflation) — the
record's sequence of surprises around the config's own means and volatilities, or, with `--history-as-recorded`, around the
record's own fitted ones: the history as it was.  The response document then carries a `market` key (months, block_months,
as_recorded, the fitted values), and so does every other object this script prints.  `--history-scheme stationary` makes the
block lengths geometric with mean `--history-block` (the stationary bootstrap) and `--history-scheme cohorts` draws nothing:
path i starts at month i of the record (mod its length) and runs it forward, so `--paths` should be a multiple of the
record's length.  `--cohorts` (with `--history-scheme cohorts` and `--working-months`) prints the historical backtest instead:
one path per start month, which starts failed, which were the worst, the success share over all starts and over those whose
horizon fits inside the record; `--history-first-month YYYY-MM` labels the starts.  `--compact` assembles the document from device-side aggregates
only (no per-path lists: for batches far beyond the UI's); `--streamed` from yearly bins taken inside the path kernel (no
memory per path at all: any number of paths, under `torchrun` too; bands are known to within one bin).  `--events` writes the progress events the SSE
endpoint would stream to stderr, one JSON per line.  Without `--full` only the `summary` block (plus timings
and sizes) is printed.  `--max-expenses` answers the other planning question instead: the largest monthly spending
(whole cents) that still reaches the target when retiring after `--working-months` (or the searched minimum), printed
with its probability and the search curve as one JSON object.  `--frontier` runs that search for several retirement months
at once (one grid probe per round) and prints a JSON list of `{working_months, max_monthly_expenses, probability,
levels_evaluated}`; `--grid-months` with `--grid-expenses` prints the success-probability table of those months x levels.
`--min-contribution` answers the third one: the smallest monthly contribution (whole cents) that reaches the target when
retiring after `--working-months` (required), printed with its probability and the search curve as one JSON object.
`--min-initial-balance` answers the fourth: the smallest starting balance (whole cents) that reaches the target when retiring
after `--working-months` (default 0: "retire today"), printed the same way; with `--at-expenses a,b,c` the search runs at each
of those monthly spending levels in lockstep and the object gains a `frontier` list of `{monthly_expenses,
min_initial_balance, probability, withdrawal_rate_pct}` — the safe-withdrawal-rate curve, `1200 * expenses / balance`.
`--stress` prints the market-assumption stress table at `--working-months` (or the searched minimum): the success probability
under the config's market and under one-at-a-time shifts of its means, volatilities and correlation, one probe over the same
random numbers.  `--breakeven FIELD[,FIELD...]` runs the break-even search for each listed mean or volatility: the most adverse
value at which the target is still met (`--window`, `--breakeven-resolution`).  Both may be given together.
`--income-options STREAM` (a list index into `other_income_streams`, or a unique name) with `--claim-ages` and / or
`--claim-amounts` prints the claiming-option table of that stream at `--working-months` (default 0): `{stream, options:
[{the six fields, probability}], best}` over the same random numbers; lists of unequal length are an error.  `--min-income
STREAM [--claim-age A]` answers "how large does this income have to be": the smallest monthly amount (whole cents) of that
stream, started at age A (default: its own), that reaches the target, printed like `--min-initial-balance`.
`--paired` (with `--income-options` and / or `--stress`) says whether the table's gaps are real: the options run over the same
paths, so every row also gets the paired difference against the best option (`vs_best`) or the base market (`vs_base`: also
`hurt` / `helped` path counts) with its standard error and the exact McNemar p-value, and the claiming table gains
`tied_with_best`, `all_succeed` and `none_succeed`.
`--outcomes` (with `--income-options` and / or `--stress`, alone or with `--paired`) says when it goes wrong and what is left:
every row also gets `lasts_until_age` (the age the money lasts to with 90 / 95 / 99 % confidence; null = the whole horizon),
`median_ruin_age` (among the failing paths) and `final_balance` (p5 .. p95 of the successful paths' nominal final balance).
`--spending-rule R --earliest-retirement` answers "how much sooner can I retire if I accept the guardrail": both month searches
on the same search stream, printed as `{fixed_spending: {working_months, ...}, with_spending_rule: {working_months, ...},
months_sooner}` (`--full` adds both search curves).  `--frontier M1,M2,... --spending-rule R` adds the rule's frontier beside the
fixed one: every row gains `with_spending_rule: {max_initial_monthly_expenses, probability, levels_evaluated}`.
`--allocations a,b,c` (with `--working-months`) prints the allocation table: the success probability of each split between the
two assets (`allocation_inv1_pct`) over the same random numbers, `{options: [{the three amounts, allocation_inv1_pct,
probability}], best}`; `--paired` and `--outcomes` add what they add to the claiming table.  `--best-allocation` searches the
split with the highest success probability on the search stream (a grid 0, 0.1, ..., 1 refined around its best point down to
`--allocation-resolution`) and prints `{best_allocation_inv1_pct, probability, tied, probes, curve}`; `tied` lists the splits of
the first grid that a paired test on the same paths cannot tell from the answer.
`--glide-paths "P;P;..."` (with `--working-months`) prints the glide table: the success probability of each GLIDE PATH, a split
that changes with the calendar (a table of `allocation_inv1_pct` by whole years from today), over the same random numbers,
`{options: [{name, the three amounts, weights, probability}], best}`.  A path is a constant (`0.6`) or `start>end@from-to`
(`start` until year `from`, a straight line to `end` in year `to`, `end` after it).  With no value it compares a small
catalogue built for `--working-months`: the config's own constant split, all and none of asset 1, two declining target-date
shapes and one rising-equity shape.  `--paired` and `--outcomes` add what they add to the allocation table.  Engine stream only.
`--glide-path P --streamed` (with `--working-months`) prints the streamed document of ONE glide path, from yearly bins taken
inside the path kernel under it: the fan charts, the start balance, the final balances of the paths that succeed, and
`glide_path` / `allocation_by_sample` (the split at each yearly sample).  Engine stream only; not together with
`--spending-rule`, `--history` or `--glide-paths`."""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, REPO)

from monte_carlo_retirement_amd import Config, load_config_from_json  # noqa: E402
from monte_carlo_retirement_amd import results as R  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("config")
    ap.add_argument("--seed", type=int, default=None)
    ap.add_argument("--rng", choices=["philox", "numpy"], default="philox")
    ap.add_argument("--history", default=None, metavar="FILE.csv",
                    help="resample months from this record (columns equity, inflation, inv2 | premium) instead of drawing them")
    ap.add_argument("--history-block", type=int, default=12, help="--history: months per resampled block")
    ap.add_argument("--history-scheme", choices=["block", "stationary", "cohorts"], default="block",
                    help="--history: fixed blocks, geometric block lengths of mean --history-block, or path i from month i of the record")
    ap.add_argument("--history-first-month", default=None, metavar="YYYY-MM", help="--history: the month of the record's first row (labels cohorts)")
    ap.add_argument("--cohorts", action="store_true",
                    help="--history-scheme cohorts: print the historical backtest at --working-months, one path per start month, instead")
    ap.add_argument("--history-as-recorded", action="store_true",
                    help="--history: use the record's own fitted means and volatilities instead of the config's")
    ap.add_argument("--paths", type=int, default=None, help="override num_simulations_main")
    ap.add_argument("--search-paths", type=int, default=None, help="override num_simulations_search")
    ap.add_argument("--working-months", type=int, default=None, help="skip the search")
    ap.add_argument("--compact", action="store_true", help="device-aggregated document (large batches)")
    ap.add_argument("--streamed", action="store_true",
                    help="document from in-kernel yearly bins: no memory per path, any number of paths (bands bracketed)")
    ap.add_argument("--events", action="store_true", help="progress events to stderr")
    ap.add_argument("--full", action="store_true", help="print the whole response document")
    ap.add_argument("--max-expenses", action="store_true", help="search the maximum monthly expenses instead")
    ap.add_argument("--min-contribution", action="store_true",
                    help="search the minimum monthly contribution at --working-months instead")
    ap.add_argument("--min-initial-balance", action="store_true",
                    help="search the minimum initial balance at --working-months (default 0: retire today) instead")
    ap.add_argument("--at-expenses", default=None,
                    help="--min-initial-balance: comma-separated monthly expenses, one search each (the withdrawal-rate curve)")
    ap.add_argument("--resolution", type=float, default=1.0,
                    help="--max-expenses / --min-contribution / --min-initial-balance: stop when the bracket is this narrow")
    ap.add_argument("--stress", action="store_true", help="print the market-assumption stress table instead")
    ap.add_argument("--breakeven", default=None,
                    help="comma-separated Config names of market means / volatilities: the break-even search for each")
    ap.add_argument("--window", type=float, default=0.25, help="--breakeven: half-width of the searched window")
    ap.add_argument("--breakeven-resolution", type=float, default=1e-4, help="--breakeven: the level grid (default one basis point)")
    ap.add_argument("--income-options", default=None, metavar="STREAM",
                    help="index or name of an income stream: the table of --claim-ages / --claim-amounts options instead")
    ap.add_argument("--claim-ages", default=None, help="--income-options: comma-separated start_at_age, one per option")
    ap.add_argument("--claim-amounts", default=None, help="--income-options: comma-separated monthly_amount_today, one per option")
    ap.add_argument("--paired", action="store_true",
                    help="--income-options / --stress: add the paired comparison over the shared paths (difference, its standard "
                         "error, the exact McNemar p-value, paths helped and hurt)")
    ap.add_argument("--outcomes", action="store_true",
                    help="--income-options / --stress: add when each option fails and what it leaves (lasts_until_age, "
                         "median_ruin_age, final_balance percentiles of the successful paths)")
    ap.add_argument("--min-income", default=None, metavar="STREAM",
                    help="index or name of an income stream: search its minimum monthly amount at --working-months (default 0) instead")
    ap.add_argument("--claim-age", type=float, default=None, help="--min-income: the stream's start_at_age (default: its own)")
    ap.add_argument("--frontier", default=None, help="comma-separated working months: maximum monthly expenses at each")
    ap.add_argument("--grid-months", default=None, help="comma-separated working months of a success-probability table")
    ap.add_argument("--grid-expenses", default=None, help="comma-separated monthly expenses of that table")
    ap.add_argument("--spending-rule", default=None, metavar="UPPER,LOWER,CUT,RAISE,FLOOR,CEILING",
                    help="a guardrail spending rule: alone, what it does to the plan year by year; with --max-expenses, the "
                         "maximum spending to begin with under the rule beside the fixed-spending answer; with --streamed, the "
                         "response document under the rule from in-kernel yearly bins: balance and spending fan charts "
                         "(needs --working-months)")
    ap.add_argument("--earliest-retirement", action="store_true",
                    help="--spending-rule: how much sooner can I retire?  Searches the minimum working months with fixed spending "
                         "and under the rule, and prints both with their difference in months")
    ap.add_argument("--compare-rules", default=None, metavar="RULE;RULE;...",
                    help="spending rules compared over the same paths at --working-months: each UPPER,LOWER,CUT,RAISE,FLOOR,CEILING "
                         "or 'none' (fixed spending), separated by ';'; composes with --paired and --outcomes")
    ap.add_argument("--allocations", default=None, metavar="A,B,...",
                    help="comma-separated allocation_inv1_pct values compared over the same paths at --working-months; composes with "
                         "--paired and --outcomes")
    ap.add_argument("--best-allocation", action="store_true",
                    help="search the allocation_inv1_pct with the highest success probability at --working-months")
    ap.add_argument("--allocation-resolution", type=float, default=0.01, help="--best-allocation: the grid the answer lies on")
    ap.add_argument("--glide-paths", nargs="?", const="", default=None, metavar="P;P;...",
                    help="glide paths compared over the same paths at --working-months: each a constant split or start>end@from-to "
                         "(years from today), separated by ';'; with no value a default catalogue; composes with --paired and --outcomes")
    ap.add_argument("--glide-path", default=None, metavar="P",
                    help="ONE glide path (a constant split or start>end@from-to) held by every path of the --streamed document at "
                         "--working-months")
    args = ap.parse_args()
    if args.glide_path is not None:
        from monte_carlo_retirement_amd.allocation import GlidePath

        if args.working_months is None:
            ap.error("--glide-path needs --working-months")
        if args.glide_paths is not None:
            ap.error("--glide-path (one path's document) and --glide-paths (a comparison) are separate questions")
        if args.spending_rule is not None:
            ap.error("--glide-path and --spending-rule together are not supported")
        if args.rng != "philox" or args.history:
            ap.error("--glide-path runs on the engine's own stream (not with --history or --rng numpy)")
        if not args.streamed:
            ap.error("--glide-path goes with --streamed")
        if (args.allocations is not None or args.best_allocation or args.min_initial_balance or args.min_contribution or args.max_expenses
                or args.income_options is not None or args.min_income is not None or args.compare_rules is not None
                or args.stress or args.breakeven or args.cohorts or args.frontier or args.grid_months
                or args.grid_expenses or args.earliest_retirement or args.compact):
            ap.error("--glide-path and the other questions are separate")
        try:
            args.glide_path = GlidePath.parse(args.glide_path)
        except ValueError as e:
            ap.error(f"--glide-path: {e}")
    if args.glide_paths is not None:
        from monte_carlo_retirement_amd.allocation import GlidePath

        if args.working_months is None:
            ap.error("--glide-paths needs --working-months")
        if (args.allocations is not None or args.best_allocation or args.min_initial_balance or args.min_contribution or args.max_expenses
                or args.income_options is not None or args.min_income is not None or args.compare_rules is not None
                or args.spending_rule is not None or args.stress or args.breakeven or args.cohorts or args.frontier or args.grid_months
                or args.grid_expenses or args.earliest_retirement or args.streamed or args.compact):
            ap.error("--glide-paths and the other questions are separate")
        try:
            args.glide_paths = [GlidePath.parse(t) for t in args.glide_paths.split(";")] if args.glide_paths.strip() else None
        except ValueError as e:
            ap.error(f"--glide-paths: {e}")
        args.glide_table = True
    if args.allocations is not None or args.best_allocation:
        if args.working_months is None:
            ap.error("--allocations / --best-allocation need --working-months")
        if args.allocations is not None and args.best_allocation:
            ap.error("--allocations and --best-allocation are separate questions")
        if (args.min_initial_balance or args.min_contribution or args.max_expenses or args.income_options is not None or args.min_income is not None
                or args.compare_rules is not None or args.spending_rule is not None or args.stress or args.breakeven or args.cohorts
                or args.frontier or args.grid_months or args.grid_expenses or args.earliest_retirement or args.streamed or args.compact):
            ap.error("--allocations / --best-allocation and the other questions are separate")
        if args.allocations is not None:
            try:
                if not _csv(args.allocations, float):
                    ap.error("--allocations needs at least one value")
            except ValueError:
                ap.error("--allocations takes comma-separated numbers")
        units = 1.0 / args.allocation_resolution if args.allocation_resolution > 0 else 0.0
        if args.best_allocation and (units < 1.0 or abs(round(units) - units) > 1e-9 * units):
            ap.error("--allocation-resolution: 1 / resolution must be a whole number (0.1, 0.05, 0.01, ...)")
    elif args.allocation_resolution != 0.01:
        ap.error("--allocation-resolution goes with --best-allocation")
    if args.compare_rules is not None:
        from monte_carlo_retirement_amd.spending_rules import SpendingRule

        if args.working_months is None:
            ap.error("--compare-rules needs --working-months")
        if args.rng != "philox" or args.history:
            ap.error("--compare-rules runs on the engine's own stream")
        if args.spending_rule is not None:
            ap.error("--compare-rules and --spending-rule are separate questions")
        try:
            args.compare_rules = [None if t.strip().lower() == "none" else SpendingRule.parse(t) for t in args.compare_rules.split(";") if t.strip()]
        except ValueError as e:
            ap.error(str(e))
        if not args.compare_rules:
            ap.error("--compare-rules needs at least one rule")
    if args.spending_rule is not None:
        from monte_carlo_retirement_amd.spending_rules import SpendingRule

        if args.working_months is None and not (args.earliest_retirement or args.frontier):
            ap.error("--spending-rule needs --working-months")
        if args.earliest_retirement and (args.frontier or args.max_expenses or args.streamed):
            ap.error("--earliest-retirement and --frontier / --max-expenses / --streamed are separate questions")
        if args.rng != "philox" or args.history:
            ap.error("--spending-rule runs on the engine's own stream")
        try:
            args.spending_rule = SpendingRule.parse(args.spending_rule)
        except ValueError as e:
            ap.error(str(e))
    if args.earliest_retirement and args.spending_rule is None:
        ap.error("--earliest-retirement goes with --spending-rule")
    if args.min_contribution and args.working_months is None:
        ap.error("--min-contribution needs --working-months")
    if args.min_contribution and args.max_expenses:
        ap.error("--min-contribution and --max-expenses are separate questions")
    if args.min_initial_balance and (args.min_contribution or args.max_expenses):
        ap.error("--min-initial-balance, --min-contribution and --max-expenses are separate questions")
    if args.at_expenses and not args.min_initial_balance:
        ap.error("--at-expenses goes with --min-initial-balance")
    if (args.income_options is not None or args.min_income is not None) and (args.min_initial_balance or args.min_contribution or args.max_expenses):
        ap.error("--income-options / --min-income and the other searches are separate questions")
    if args.income_options is not None and args.min_income is not None:
        ap.error("--income-options and --min-income are separate questions")
    glide_table = getattr(args, "glide_table", False)
    if args.paired and args.income_options is None and not args.stress and args.compare_rules is None and args.allocations is None and not glide_table:
        ap.error("--paired goes with --income-options, --stress, --compare-rules, --allocations or --glide-paths")
    if args.outcomes and args.income_options is None and not args.stress and args.compare_rules is None and args.allocations is None and not glide_table:
        ap.error("--outcomes goes with --income-options, --stress, --compare-rules, --allocations or --glide-paths")
    if (args.claim_ages or args.claim_amounts) and args.income_options is None:
        ap.error("--claim-ages / --claim-amounts go with --income-options")
    if args.claim_age is not None and args.min_income is None:
        ap.error("--claim-age goes with --min-income")
    if args.income_options is not None:
        if not (args.claim_ages or args.claim_amounts):
            ap.error("--income-options needs --claim-ages and / or --claim-amounts")
        if args.claim_ages and args.claim_amounts and len(_csv(args.claim_ages, float)) != len(_csv(args.claim_amounts, float)):
            ap.error("--claim-ages and --claim-amounts must list one value per option each (equal lengths)")

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank0 = int(os.environ.get("RANK", "0")) == 0
    if world > 1:  # one process per GPU (python -m torch.distributed.run --nproc-per-node N examples/run_scenario.py ...)
        import torch
        import torch.distributed as dist

        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")) % max(1, torch.cuda.device_count()))
        dist.init_process_group(os.environ.get("MCR_BACKEND", "nccl"))
        if args.compact:
            ap.error("--compact is a single-process document")
    raw = load_config_from_json(args.config)
    if args.paths:
        raw["num_simulations_main"] = args.paths
    if args.search_paths:
        raw["num_simulations_search"] = args.search_paths
    config = Config(**raw)
    args.market_history = None
    if args.history_as_recorded and not args.history:
        ap.error("--history-as-recorded goes with --history")
    if (args.history_scheme != "block" or args.history_first_month is not None) and not args.history:
        ap.error("--history-scheme / --history-first-month go with --history")
    if args.cohorts and not (args.history and args.history_scheme == "cohorts"):
        ap.error("--cohorts needs --history with --history-scheme cohorts")
    if args.cohorts and args.working_months is None:
        ap.error("--cohorts needs --working-months")
    if args.history:
        if args.rng != "philox":
            ap.error("--history is a random stream of its own: leave --rng out")
        from monte_carlo_retirement_amd.history import MarketHistory, with_fitted_market

        with open(args.history, "r", encoding="utf-8") as fh:
            columns = [c.strip() for c in fh.readline().split(",")]
        over = {"inv2": None, "premium": "premium"} if "premium" in columns and "inv2" not in columns else {}
        try:
            args.market_history = MarketHistory.from_csv(args.history, block_months=args.history_block, scheme=args.history_scheme,
                                                         first_month=args.history_first_month, **over)
        except ValueError as e:
            ap.error(str(e))
        args.rng = "history"
        if args.history_as_recorded:
            config = with_fitted_market(config, args.market_history)

    marks = {"t0": time.perf_counter()}
    seen = []

    def emit(event: dict) -> None:
        seen.append(event["type"])
        if event["type"] in ("search_complete", "error") or (event["type"] == "phase" and event["phase"] == "final_sim"):
            marks.setdefault("search_done", time.perf_counter())
        if args.events and rank0 and event["type"] != "result":
            print(json.dumps(event), file=sys.stderr)

    if args.cohorts:
        return cohorts(args, config, world, rank0)
    if glide_table:
        return glide_table_document(args, config, world, rank0)
    if args.glide_path is not None:
        return glide_path_document(args, config, world, rank0)
    if args.allocations is not None:
        return allocation_table(args, config, world, rank0)
    if args.best_allocation:
        return best_allocation(args, config, world, rank0)
    if args.compare_rules is not None:
        return compare_rules(args, config, world, rank0)
    if args.earliest_retirement:
        return earliest_retirement(args, config, world, rank0)
    if args.spending_rule is not None and not args.max_expenses and not args.frontier:
        return spending_rule(args, config, world, rank0)
    if args.max_expenses:
        return max_expenses(args, config, world, rank0)
    if args.min_contribution:
        return min_contribution(args, config, world, rank0)
    if args.min_initial_balance:
        return min_initial_balance(args, config, world, rank0)
    if args.income_options is not None:
        return income_table(args, config, world, rank0)
    if args.min_income is not None:
        return min_income(args, config, world, rank0)
    if args.stress or args.breakeven:
        return stress(args, config, world, rank0)
    if args.frontier or args.grid_months or args.grid_expenses:
        if args.frontier and (args.grid_months or args.grid_expenses):
            ap.error("--frontier and --grid-* are separate questions")
        if not args.frontier and not (args.grid_months and args.grid_expenses):
            ap.error("--grid-months and --grid-expenses go together")
        return frontier_or_grid(args, config, world, rank0)
    if args.compact and args.streamed:
        ap.error("--compact and --streamed are two ways to build the document")
    builder = R.streamed_result if args.streamed else R.compact_result if args.compact else R.build_result
    doc = R.run_scenario(config, args.working_months, emit=emit, result_builder=builder,
                         main_seed_override=args.seed, rng=args.rng,
                         **({"market_history": args.market_history, "market_as_recorded": args.history_as_recorded} if args.market_history else {}))
    t_end = time.perf_counter()
    rc = 0
    if doc is None:
        rc = 1
        out = {"error": "see the last event", "events": seen[-3:]}
    elif args.full:
        out = doc
    else:
        out = {
            "scenario": doc["scenario"], "rng": args.rng, "summary": doc["summary"], **({"market": doc["market"]} if "market" in doc else {}),
            "search_probes": seen.count("search_iter"),
            "trajectory_points": len(doc["trajectory"]["years"]),
            "sample_paths": len(doc["trajectory"]["sample_paths"]),
            "failure_count": doc["ruin_histogram"]["failure_count"],
            "document_bytes": len(json.dumps(doc)),
            "seconds": {"search": round(marks.get("search_done", t_end) - marks["t0"], 3),
                        "final_run_and_document": round(t_end - marks.get("search_done", t_end), 3)},
        }
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return rc


def cohorts(args, config: Config, world: int, rank0: bool) -> int:
    """Every rank replays the (small) record's cohorts in full; rank 0 prints."""
    out = _simulator(args, config).historical_cohorts(args.working_months).to_document()
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def max_expenses(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    wm = args.working_months
    searched = wm is None
    if searched:
        wm = sim.find_minimum_working_months(verbose=False)[0]
    rc = 0
    if wm < 0:
        out = {"error": "the target is not reachable within the working-month search horizon"}
        rc = 1
    else:
        events = []
        expenses, prob, curve = sim.find_maximum_monthly_expenses(wm, verbose=False, progress_callback=events.append,
                                                                  resolution=args.resolution)
        out = {
            "scenario": config.Nickname, "rng": args.rng, "working_months": int(wm), "working_months_searched": searched,
            "target_probability": config.target_probability, "max_monthly_expenses": expenses, "probability": prob,
            "probes": len({e["iteration"] for e in events}), "curve": curve,
            "seconds": round(time.perf_counter() - t0, 3),
        }
        if args.spending_rule is not None:    # both answers side by side: fixed spending, and spending that follows the rule
            t1 = time.perf_counter()
            r_expenses, r_prob, r_curve = sim.find_maximum_initial_expenses(wm, args.spending_rule, resolution=args.resolution, verbose=False)
            out["with_spending_rule"] = {"rule": args.spending_rule.as_dict(), "max_initial_monthly_expenses": r_expenses,
                                         "probability": r_prob, "levels": len(r_curve), "seconds": round(time.perf_counter() - t1, 3)}
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return rc


def spending_rule(args, config: Config, world: int, rank0: bool) -> int:
    """What the rule does to the plan at --working-months: success % and, per retirement year, the shares alive / cut / at
    the floor / raised."""
    sim = _simulator(args, config)
    if args.streamed:    # the whole document from yearly bins under the rule: balance and spending fan charts, no per-path memory
        sim.use_final_seeds()
        doc = R.streamed_result(config, sim, int(args.working_months), rule=args.spending_rule)
        if rank0:
            print(json.dumps(doc))
        if world > 1:
            import torch.distributed as dist

            dist.barrier()
            dist.destroy_process_group()
        return 0
    outcomes = sim.spending_rule_outcomes(args.working_months, args.spending_rule)
    out = {"scenario": config.Nickname, "rng": args.rng, "working_months": int(args.working_months),
           "rule": args.spending_rule.as_dict(), **outcomes.row()}
    if rank0:
        if args.full:
            print(json.dumps(out))
        else:
            print(f"{config.Nickname}: success {outcomes.probability:.2f}% over {outcomes.n_paths} paths under {args.spending_rule.as_dict()}")
            print(f"{'year':>4} {'age':>6} {'alive':>7} {'cut':>7} {'floor':>7} {'raised':>7}")
            for y in out["years"]:
                print(f"{y['year']:>4} {y['age']:>6.1f} {100 * y['alive']:>6.1f}% {100 * y['cut']:>6.1f}% {100 * y['at_floor']:>6.1f}% {100 * y['raised']:>6.1f}%")
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def glide_path_document(args, config: Config, world: int, rank0: bool) -> int:
    """The streamed document of ONE glide path at --working-months: yearly bins under the path, no per-path memory."""
    sim = _simulator(args, config)
    sim.use_final_seeds()
    rc = 0
    try:
        doc = R.streamed_result(config, sim, int(args.working_months), glide_path=args.glide_path)
    except (ValueError, RuntimeError) as e:      # (RuntimeError: a shape the glide launch does not support, in the library's words)
        doc, rc = {"error": str(e)}, 1
    if rank0:
        print(json.dumps(doc))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return rc


def earliest_retirement(args, config: Config, world: int, rank0: bool) -> int:
    """How much sooner can I retire?  The minimum working months with fixed spending and under --spending-rule, on the same
    search stream, and their difference."""
    sim = _simulator(args, config)
    fixed = sim.find_minimum_working_months(verbose=False)
    ruled = sim.find_minimum_working_months_with_rule(args.spending_rule, verbose=False)
    sooner = None if fixed[0] < 0 or ruled[0] < 0 else int(fixed[0] - ruled[0])
    out = {"scenario": config.Nickname, "rng": args.rng, "rule": args.spending_rule.as_dict(),
           "num_simulations": int(config.num_simulations_search), "target_probability": float(config.target_probability),
           "fixed_spending": {"working_months": int(fixed[0]), "probability": fixed[1], "months_evaluated": len(fixed[2])},
           "with_spending_rule": {"working_months": int(ruled[0]), "probability": ruled[1], "months_evaluated": len(ruled[2])},
           "months_sooner": sooner}
    if rank0:
        if args.full:
            print(json.dumps(dict(out, fixed_curve=fixed[2], rule_curve=ruled[2])))
        else:
            print(json.dumps(out))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def compare_rules(args, config: Config, world: int, rank0: bool) -> int:
    """--compare-rules: which guardrail to choose.  One row per rule over the same paths: success %, the shares of all paths
    that are cut / at the floor in the last retirement year, and with --paired the gap to the best rule and whether it is real."""
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    sim.use_final_seeds()
    table = sim.compare_spending_rules(int(args.working_months), [{"rule": r} for r in args.compare_rules], **_table_flags(args))
    out = {"scenario": config.Nickname, "rng": args.rng, "working_months": int(args.working_months),
           "num_simulations": int(config.num_simulations_main), "target_probability": config.target_probability, **table,
           "seconds": round(time.perf_counter() - t0, 3)}
    if rank0:
        if args.full:
            print(json.dumps(out))
        else:
            print(f"{config.Nickname}: {len(table['options'])} spending rules over {out['num_simulations']} shared paths, best = #{table['best']}")
            print(f"{'#':>2} {'rule':<32} {'success':>8} {'cut@end':>8} {'floor@end':>9}" + (f" {'vs best':>8} {'se':>6} {'p':>7}" if args.paired else "")
                  + (f" {'lasts 95%':>9} {'median left':>12}" if args.outcomes else ""))
            for i, row in enumerate(table["options"]):
                r, last = row["rule"], row["years"][-1]
                name = "fixed spending" if r is None else ",".join(f"{r[k]:g}" for k in ("upper", "lower", "cut", "raise", "floor", "ceiling"))
                line = f"{i:>2} {name:<32} {row['probability']:>7.2f}% {100 * last['cut']:>7.1f}% {100 * last['at_floor']:>8.1f}%"
                if args.paired:
                    d = row["vs_best"]
                    line += f" {d['delta']:>8.2f} {d['se']:>6.2f} {d['p_value']:>7.4f}"
                if args.outcomes:
                    age, med = row["lasts_until_age"]["95"], row["final_balance"]["p50"]
                    line += f" {'horizon' if age is None else format(age, '.1f'):>9} {'-' if med is None else format(med, ',.0f'):>12}"
                print(line)
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def stress(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    wm = args.working_months
    searched = wm is None
    if searched:
        wm = sim.find_minimum_working_months(verbose=False)[0]
    rc = 0
    if wm < 0:
        out = {"error": "the target is not reachable within the working-month search horizon"}
        rc = 1
    else:
        out = {"scenario": config.Nickname, "rng": args.rng, "working_months": int(wm), "working_months_searched": searched,
               "target_probability": config.target_probability}
        if args.stress:
            sim.use_final_seeds()
            out["stress"] = sim.stress_test(wm, **_table_flags(args))
        if args.breakeven:
            out["breakeven"] = []
            for field in [f.strip() for f in args.breakeven.split(",") if f.strip()]:
                events = []
                value, prob, curve, status = sim.find_breakeven_assumption(
                    wm, field, window=args.window, resolution=args.breakeven_resolution, verbose=False, progress_callback=events.append)
                out["breakeven"].append({"field": field, "base": getattr(config, field), "value": value, "probability": prob,
                                         "status": status, "probes": len({e["iteration"] for e in events}),
                                         "levels_evaluated": len(curve)})
        out["seconds"] = round(time.perf_counter() - t0, 3)
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return rc


def min_contribution(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    events = []
    contribution, prob, curve = sim.find_minimum_monthly_contribution(args.working_months, verbose=False,
                                                                      progress_callback=events.append,
                                                                      resolution=args.resolution)
    out = {
        "scenario": config.Nickname, "rng": args.rng, "working_months": int(args.working_months),
        "target_probability": config.target_probability, "min_monthly_contribution": contribution, "probability": prob,
        "probes": len({e["iteration"] for e in events}), "curve": curve,
        "seconds": round(time.perf_counter() - t0, 3),
    }
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def min_initial_balance(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    wm = 0 if args.working_months is None else int(args.working_months)   # (retire today)
    events = []
    if args.at_expenses:
        levels = _csv(args.at_expenses, float)
        results = sim.find_minimum_initial_balance_by_expenses(wm, levels, verbose=False, progress_callback=events.append,
                                                               resolution=args.resolution)
        # the headline entry: the search at the config's own spending where it is among the levels, else the first
        head = levels.index(float(config.monthly_expenses)) if float(config.monthly_expenses) in levels else 0
        balance, prob, curve = results[head]
        probes = max((e["iteration"] for e in events), default=0)   # (one probe a round, shared by the searches)
    else:
        balance, prob, curve = sim.find_minimum_initial_balance(wm, verbose=False, progress_callback=events.append,
                                                                resolution=args.resolution)
        probes = len({e["iteration"] for e in events})
    out = {
        "scenario": config.Nickname, "rng": args.rng, "working_months": wm,
        "target_probability": config.target_probability, "min_initial_balance": balance, "probability": prob,
        "probes": probes, "curve": curve,
        "seconds": round(time.perf_counter() - t0, 3),
    }
    if args.at_expenses:
        out["frontier"] = [{"monthly_expenses": e, "min_initial_balance": b, "probability": pr,
                            "withdrawal_rate_pct": 1200.0 * e / b if b > 0 else None}
                           for e, (b, pr, _) in zip(levels, results)]
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def _table_flags(args) -> dict:
    """--paired / --outcomes as keyword arguments of `compare_claiming_options` / `stress_test` (neither: none at all)"""
    return {k: True for k in ("paired", "outcomes") if getattr(args, k)}


def _stream_arg(text: str):
    """STREAM of --income-options / --min-income: a list index where it reads as one, else a name"""
    return int(text) if text.strip().lstrip("+").isdigit() else text


def income_table(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    wm = 0 if args.working_months is None else int(args.working_months)
    ages = _csv(args.claim_ages, float) if args.claim_ages else None
    amounts = _csv(args.claim_amounts, float) if args.claim_amounts else None
    options = [{} for _ in (ages or amounts)]
    for k, o in enumerate(options):
        if ages:
            o["start_at_age"] = ages[k]
        if amounts:
            o["monthly_amount_today"] = amounts[k]
    sim.use_final_seeds()
    table = sim.compare_claiming_options(wm, _stream_arg(args.income_options), options, **_table_flags(args))
    out = {"scenario": config.Nickname, "rng": args.rng, "working_months": wm, "num_simulations": int(config.num_simulations_main),
           "target_probability": config.target_probability, **table, "seconds": round(time.perf_counter() - t0, 3)}
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def allocation_table(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    sim.use_final_seeds()
    try:
        table = sim.compare_allocations(int(args.working_months), _csv(args.allocations, float), **_table_flags(args))
    except ValueError as e:
        print(json.dumps({"error": str(e)}))
        return 2
    out = {"scenario": config.Nickname, "rng": args.rng, "working_months": int(args.working_months),
           "num_simulations": int(config.num_simulations_main), **table, "seconds": round(time.perf_counter() - t0, 3)}
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def glide_table_document(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    sim.use_final_seeds()
    try:
        table = sim.compare_glide_paths(int(args.working_months), args.glide_paths, **_table_flags(args))
    except (ValueError, RuntimeError) as e:      # (RuntimeError: a shape the glide probe does not support, in the library's words)
        print(json.dumps({"error": str(e)}))
        return 2
    out = {"scenario": config.Nickname, "rng": args.rng, "working_months": int(args.working_months),
           "num_simulations": int(config.num_simulations_main), **table, "seconds": round(time.perf_counter() - t0, 3)}
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def best_allocation(args, config: Config, world: int, rank0: bool) -> int:
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    events = []
    try:
        allocation, prob, curve, tied = sim.find_best_allocation(int(args.working_months), resolution=args.allocation_resolution,
                                                                 verbose=False, progress_callback=events.append)
    except ValueError as e:
        print(json.dumps({"error": str(e)}))
        return 2
    out = {
        "scenario": config.Nickname, "rng": args.rng, "working_months": int(args.working_months),
        "own_allocation_inv1_pct": float(config.allocation_inv1_pct), "best_allocation_inv1_pct": allocation, "probability": prob,
        "tied": tied, "probes": len({e["iteration"] for e in events}), "curve": curve,
        "seconds": round(time.perf_counter() - t0, 3),
    }
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def min_income(args, config: Config, world: int, rank0: bool) -> int:
    from monte_carlo_retirement_amd.income import stream_index
    t0 = time.perf_counter()
    sim = _simulator(args, config)
    wm = 0 if args.working_months is None else int(args.working_months)
    index = stream_index(config, _stream_arg(args.min_income))
    events = []
    amount, prob, curve = sim.find_minimum_income_amount(wm, index, start_at_age=args.claim_age, verbose=False,
                                                         progress_callback=events.append, resolution=args.resolution)
    out = {
        "scenario": config.Nickname, "rng": args.rng, "working_months": wm, "stream": index,
        "start_at_age": float(config.other_income_streams[index].start_at_age if args.claim_age is None else args.claim_age),
        "target_probability": config.target_probability, "min_income_amount": amount, "probability": prob,
        "probes": len({e["iteration"] for e in events}), "curve": curve,
        "seconds": round(time.perf_counter() - t0, 3),
    }
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


def _simulator(args, config: Config):
    from monte_carlo_retirement_amd.simulation import RetirementMonteCarloSimulator

    return RetirementMonteCarloSimulator(config, main_seed_override=args.seed, rng=args.rng, market_history=args.market_history)


def _with_market(args, out):
    """The printed object with the `market` key of a --history run (the response document carries its own)"""
    if args.market_history is None or not isinstance(out, dict) or "market" in out or "error" in out:
        return out
    from monte_carlo_retirement_amd.history import market_document

    return dict(out, market=market_document(args.market_history, args.history_as_recorded))


def _csv(text: str, kind):
    return [kind(x) for x in text.split(",") if x.strip()]


def frontier_or_grid(args, config: Config, world: int, rank0: bool) -> int:
    sim = _simulator(args, config)
    if args.frontier:
        months = _csv(args.frontier, int)
        results = sim.find_maximum_monthly_expenses_by_months(months, verbose=False, resolution=args.resolution)
        out = [{"working_months": m, "max_monthly_expenses": expenses, "probability": prob, "levels_evaluated": len(curve)}
               for m, (expenses, prob, curve) in zip(months, results)]
        if args.spending_rule is not None:    # the rule's frontier beside the fixed one: the spending to BEGIN retirement with
            ruled = sim.find_maximum_initial_expenses_by_months(months, args.spending_rule, verbose=False, resolution=args.resolution)
            for row, (expenses, prob, curve) in zip(out, ruled):
                row["with_spending_rule"] = {"max_initial_monthly_expenses": expenses, "probability": prob, "levels_evaluated": len(curve)}
    else:
        months, levels = _csv(args.grid_months, int), _csv(args.grid_expenses, float)
        table = sim.success_probability_grid(months, levels)
        out = {"scenario": config.Nickname, "rng": args.rng, "num_simulations": int(config.num_simulations_main),
               "working_months": months, "monthly_expenses": levels, "probability": table.tolist()}
    if rank0:
        print(json.dumps(_with_market(args, out)))
    if world > 1:
        import torch.distributed as dist

        dist.barrier()
        dist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
