// The CPU oracle's model of a GLIDE PATH (include/mcr.h): the path loop of oracle/mcr_oracle.c (orc_single_path), restated over
// the steps that file exports, with the weight of the row being processed in every place the loop reads a weight.
//
// The unmodified oracle runs one split per run.  It exports every step of its month, though, and orc_rebalance / orc_annual_tax
// read the split from the block they are handed: so this file keeps one copy of the block per table entry and hands over the
// copy of the row's year.  The loop below is orc_single_path's, statement for statement and in its order (the line numbers are
// the ones that file quotes); only `W(t)` stands where it reads `alloc1` or passes `p`.  Row t is the 0-based month from today:
// accumulation month m_idx is row m_idx - 1, retirement month rmi is row working_months + rmi, and
//     w(t) = table[min(t / 12, n - 1)].
// Under a constant table every block copy equals *p and every result equals orc_run_batch's bit for bit
// (tests/test_glide_model_cpu.py), which is what anchors the restatement.
//
// Built by the tests with the host compiler, without FMA contraction like the oracle, against include/mcr.h and linked to the
// oracle's library.
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "mcr.h"

extern "C" {
int32_t orc_stream_start_month_index(double current_age, int32_t working_months, double start_at_age);
void orc_withdraw(double bal_inv, double cb_inv, double net_target, int use_real_tax, double rate, double* new_bal, double* new_cb,
                  double* gross, double* net);
double orc_nlv(double balance, double cost_basis, int use_real, double rate);
void orc_rebalance(const mcr_params* p, double* b1, double* cb1, double* b2, double* cb2);
int orc_annual_tax(const mcr_params* p, double* b1, double* cb1, double* b2, double* cb2, double gain1, double gain2);
double orc_monthly_gross(double mu_log, double sigma_log, double z);
void orc_draw_shocks(uint64_t seed, uint32_t stream_id, uint64_t path, int32_t n_months, double rho, double* out);
int orc_query_sizes(const mcr_params* p, int32_t wm, mcr_sizes* s);
}

namespace {
constexpr int MPY = MCR_MONTHS_PER_YEAR;
constexpr double EPS = MCR_SMALL_EPSILON;
inline double pymax(double a, double b) { return (b > a) ? b : a; }   // (the oracle's: Python's max(a, b) returns a unless b > a)
inline double pymin(double a, double b) { return (b < a) ? b : a; }

const mcr_stream* stream_of(const mcr_params* p, int32_t s) {
    return s < MCR_INLINE_STREAMS ? &p->streams[s] : &p->extra_streams[s - MCR_INLINE_STREAMS];
}

struct Result {
    double start_balance, final_balance, years_to_ruin, first_year_gross, first_year_real_gross, inflation_at_retirement;
    int success;
};

// blocks[y]: *p with allocation_inv1_pct = table[y]
void glide_single_path(const mcr_params* p, const std::vector<mcr_params>& blocks, int32_t working_months, const double* shocks,
                       int32_t shock_rows, Result* res, double* traj_out, double* real_out, double* wr_out, int64_t ts) {
    const int32_t n_table = (int32_t)blocks.size();
    auto B = [&](int32_t t) -> const mcr_params* { return &blocks[(size_t)(t / MPY < n_table - 1 ? t / MPY : n_table - 1)]; };
    auto W = [&](int32_t t) { return B(t)->allocation_inv1_pct; };
    const int32_t ry = p->retirement_years;
    const int use1 = p->inv1_use_realized_gains_tax_system, use2 = p->inv2_use_realized_gains_tax_system;
    const double rate1 = p->inv1_realized_gains_tax_rate, rate2 = p->inv2_realized_gains_tax_rate;
    const int32_t num_working_years = working_months > 0 ? (working_months + MPY - 1) / MPY : 0; /* :585-589 */
    const int32_t expected_len = 1 + num_working_years + ry;                                     /* :902 */
    std::vector<double> traj((size_t)expected_len + 2), px((size_t)expected_len + 2), wr((size_t)ry + 1);
    int32_t n_traj = 0, n_wr = 0;
    traj[n_traj] = p->initial_balance; px[n_traj] = 1.0; n_traj++; /* :490-492 */
    double years_to_ruin = NAN;                                    /* :497 */

    double bal1 = p->initial_balance * W(0);   /* :499  (the initial split reads W[0]) */
    double bal2 = p->initial_balance - bal1;   /* :500 */
    double cb1 = bal1, cb2 = bal2;             /* :501-502 */
    double contrib = p->monthly_contribution;  /* :504 */
    double gacc1 = 0.0, gacc2 = 0.0;           /* :505-506 */
    double infl = 1.0;                         /* :508 */
    int32_t shock_idx = 0;                     /* :509 */
    int pre_fail = 0;                          /* :510 */

    for (int32_t m_idx = 1; m_idx <= working_months; ++m_idx) { /* :513 */
        const int32_t t = m_idx - 1;                            /* the row */
        if ((m_idx - 1) % MPY == 0 && m_idx > 1) {              /* :514 */
            if (p->contribution_growth_rate_annual > 0)         /* :516 */
                contrib *= 1 + p->contribution_growth_rate_annual; /* :517 */
        }
        const double* z = shocks + 3 * (size_t)shock_idx; /* :519 */
        shock_idx++;
        double g1 = orc_monthly_gross(p->inv1_mu_log, p->inv1_sigma_log, z[0]);     /* :522-524 */
        double ginf = orc_monthly_gross(p->inf_mu_log, p->inf_sigma_log, z[1]);     /* :525-527 */
        double gprem = orc_monthly_gross(p->prem_mu_log, p->prem_sigma_log, z[2]);  /* :528-530 */
        double g2 = ginf * gprem;                                                   /* :532 */
        gacc1 += bal1 * (g1 - 1.0); /* :534 */
        gacc2 += bal2 * (g2 - 1.0); /* :535 */
        bal1 *= g1;                 /* :536 */
        bal2 *= g2;                 /* :537 */
        infl *= ginf;               /* :538 */
        double c1 = contrib * W(t); /* :540-542 */
        double c2 = contrib - c1;   /* :543 */
        bal1 += c1; cb1 += c1; bal2 += c2; cb2 += c2; /* :544-547 */
        orc_rebalance(B(t), &bal1, &cb1, &bal2, &cb2); /* :549-553 */
        if (m_idx % MPY == 0) {                        /* :557  ((t + 1) % 12 == 0: the annual tax closes row t) */
            int tf = orc_annual_tax(B(t), &bal1, &cb1, &bal2, &cb2, gacc1, gacc2); /* :558-571 */
            if (tf) pre_fail = 1;                                                  /* :572-573 */
            traj[n_traj] = bal1 + bal2; px[n_traj] = infl; n_traj++;               /* :574-576 */
            gacc1 = 0.0; gacc2 = 0.0;                                              /* :578-579 */
        }
    }
    double start_balance = bal1 + bal2; /* :581 */
    double infl_ret = infl;             /* :582 */
    if (working_months > 0 && working_months % MPY != 0) { /* :590-594 */
        traj[n_traj] = start_balance; px[n_traj] = infl_ret; n_traj++;
    }
    const size_t ns = (size_t)(p->n_streams > 0 ? p->n_streams : 1);
    std::vector<int32_t> s_start(ns), s_dur(ns);
    std::vector<int> s_fixed_set(ns, 0);
    std::vector<double> s_fixed(ns, 0.0);
    for (int32_t s = 0; s < p->n_streams; ++s) {
        s_start[s] = orc_stream_start_month_index(p->current_age, working_months, stream_of(p, s)->start_at_age);
        s_dur[s] = stream_of(p, s)->duration_years < 0 ? -1 : stream_of(p, s)->duration_years * MPY;
    }
    double fy_gross = 0.0, fy_real = 0.0; /* :623-624 */
    int succeeded = !pre_fail;            /* :627 */
    if (pre_fail) years_to_ruin = 0.0;    /* :628-629 */

    for (int32_t year_num = 0; year_num < ry; ++year_num) { /* :632 */
        if (pre_fail) break;                                /* :633-634 */
        double tg1 = 0.0, tg2 = 0.0, treal = 0.0;           /* :635-637 */
        int yfail = 0;                                      /* :638 */
        int32_t rmi = 0;
        for (int32_t mi = 0; mi < MPY; ++mi) {              /* :640 */
            rmi = year_num * MPY + mi;                      /* :641-643 */
            const int32_t t = working_months + rmi;         /* the row */
            double price = infl;                            /* :644 */
            double expenses = p->monthly_expenses * price;  /* :645-647 */
            double income = 0.0;                            /* :649 */
            for (int32_t s = 0; s < p->n_streams; ++s) {    /* :650 */
                int active = rmi >= s_start[s] && (s_dur[s] < 0 || rmi < s_start[s] + s_dur[s]); /* :653-656 */
                if (!active) continue;
                const mcr_stream* st = stream_of(p, s);
                double nominal;
                if (st->inflation_indexed) {
                    nominal = st->monthly_amount_today * price; /* :661-665 */
                } else {
                    if (!s_fixed_set[s]) { s_fixed[s] = st->monthly_amount_today * price; s_fixed_set[s] = 1; } /* :667-671 */
                    nominal = s_fixed[s];
                }
                income += nominal * (1.0 - st->tax_rate); /* :675-677 */
            }
            double need = pymax(0.0, expenses - income); /* :679-682 */
            double tot_before = bal1 + bal2;             /* :684 */
            if (tot_before <= EPS && need > EPS) { yfail = 1; break; } /* :685-690 */
            int32_t si = shock_idx < shock_rows - 1 ? shock_idx : shock_rows - 1; /* :692 */
            const double* z = shocks + 3 * (size_t)si;
            shock_idx++;
            double g1 = orc_monthly_gross(p->inv1_mu_log, p->inv1_sigma_log, z[0]);    /* :695-697 */
            double ginf = orc_monthly_gross(p->inf_mu_log, p->inf_sigma_log, z[1]);    /* :698-700 */
            double gprem = orc_monthly_gross(p->prem_mu_log, p->prem_sigma_log, z[2]); /* :701-703 */
            double g2 = ginf * gprem;                                                  /* :704 */
            gacc1 += bal1 * (g1 - 1.0); /* :706-708 */
            gacc2 += bal2 * (g2 - 1.0); /* :709-711 */
            bal1 *= g1; bal2 *= g2; infl *= ginf; /* :712-714 */
            double tot_after = bal1 + bal2;       /* :715 */
            if (tot_after <= EPS && need > EPS) { /* :717-724 */
                bal1 = pymax(0, bal1); bal2 = pymax(0, bal2);
                yfail = 1; break;
            }
            double cap1 = orc_nlv(bal1, cb1, use1, rate1); /* :726-731 */
            double cap2 = orc_nlv(bal2, cb2, use2, rate2); /* :732-737 */
            double cap = cap1 + cap2;                      /* :738 */
            double target = pymax(0.0, pymin(need, cap));  /* :739-742 */
            if (need > EPS && target < need - EPS) yfail = 1; /* :743-748 */
            double prop1 = cap > EPS ? cap1 / cap : W(t);     /* :750-754  (the dust sub-case reads the row's weight) */
            double prop2 = 1.0 - prop1;                       /* :755 */
            double gw1, nw1, gw2, nw2;
            orc_withdraw(bal1, cb1, target * prop1, use1, rate1, &bal1, &cb1, &gw1, &nw1); /* :757-765 */
            tg1 += gw1;                                                                    /* :766 */
            orc_withdraw(bal2, cb2, target * prop2, use2, rate2, &bal2, &cb2, &gw2, &nw2); /* :768-776 */
            tg2 += gw2;                                                                    /* :777 */
            treal += (gw1 + gw2) * infl_ret / pymax(price, EPS);                           /* :778-782 */
            double net_cash = nw1 + nw2;                                                   /* :784 */
            if (need > EPS && net_cash < need - EPS) yfail = 1;                            /* :785-790 */
            orc_rebalance(B(t), &bal1, &cb1, &bal2, &cb2);                                 /* :792-796 */
            int32_t absm = working_months + rmi + 1;                                       /* :798-800  (= t + 1) */
            if (!yfail && absm % MPY == 0) {                                               /* :801-804 */
                int tf = orc_annual_tax(B(t), &bal1, &cb1, &bal2, &cb2, gacc1, gacc2);     /* :805-818 */
                gacc1 = 0.0; gacc2 = 0.0;                                                  /* :819-820 */
                if (tf) yfail = 1;                                                         /* :821-822 */
            }
            if (yfail) { years_to_ruin = (double)(rmi + 1) / (double)MPY; break; }         /* :824-828 */
        }
        double ygw = tg1 + tg2; /* :830-832 */
        double wr_pct = start_balance > EPS ? (treal / start_balance) * 100.0 : 0.0; /* :834-840 */
        if (yfail) {                                                                 /* :842 */
            succeeded = 0;                                                           /* :843 */
            if (std::isnan(years_to_ruin)) years_to_ruin = (double)(rmi + 1) / (double)MPY; /* :844-847 */
            traj[n_traj] = pymax(0.0, bal1 + bal2); px[n_traj] = infl; n_traj++;     /* :848-849 */
            wr[n_wr++] = NAN;                                                        /* :851 */
            if (year_num == 0) { fy_gross = ygw; fy_real = treal; }                  /* :852-856 */
            break;                                                                   /* :857 */
        }
        wr[n_wr++] = wr_pct;                                    /* :859 */
        if (year_num == 0) { fy_gross = ygw; fy_real = treal; } /* :861-865 */
        traj[n_traj] = bal1 + bal2; px[n_traj] = infl; n_traj++; /* :867-868 */
    }
    int32_t total_sim_months = working_months + ry * MPY; /* :873-875 */
    if (succeeded && total_sim_months % MPY != 0) {       /* :876-879  (the terminal settlement: the last row's weight) */
        int tf = orc_annual_tax(B(total_sim_months - 1), &bal1, &cb1, &bal2, &cb2, gacc1, gacc2); /* :880-893 */
        if (tf) { succeeded = 0; years_to_ruin = (double)ry; }                    /* :894-896 */
        if (n_traj > 0) traj[n_traj - 1] = bal1 + bal2;                           /* :897-898 */
    }
    double final_total = bal1 + bal2; /* :900 */
    if (n_traj < expected_len) {      /* :905-916 */
        double pad = !succeeded ? 0.0 : (n_traj > 0 ? traj[n_traj - 1] : 0.0);
        double last_px = n_traj > 0 ? px[n_traj - 1] : 1.0;
        while (n_traj < expected_len) { traj[n_traj] = pad; px[n_traj] = last_px; n_traj++; }
    } else if (n_traj > expected_len) { /* :917-919 */
        n_traj = expected_len;
    }
    for (int32_t k = 0; k < n_traj; ++k) { /* :928-931 */
        if (traj_out) traj_out[(int64_t)k * ts] = traj[k];
        if (real_out) real_out[(int64_t)k * ts] = px[k] > EPS ? traj[k] / px[k] : 0.0;
    }
    while (n_wr < ry) wr[n_wr++] = NAN; /* :934-935 */
    if (wr_out) for (int32_t y = 0; y < ry; ++y) wr_out[(int64_t)y * ts] = wr[y];

    res->start_balance = start_balance;          /* :940 */
    res->final_balance = pymax(0, final_total);  /* :941 */
    res->success = succeeded;                    /* :942 */
    res->years_to_ruin = years_to_ruin;          /* :943 */
    res->first_year_gross = fy_gross;            /* :944 */
    res->first_year_real_gross = fy_real;        /* :945 */
    res->inflation_at_retirement = infl_ret;     /* :949 */
}
}  // namespace

// orc_run_batch's contract on host buffers (every pointer of `out` may be null; counters, ruin_year_bins and wr_obs_counts are
// not kept), under the glide path table[0 .. n_table).  Returns MCR_OK or MCR_ERR_INVALID_ARG.
extern "C" int glide_model_run_batch(const mcr_params* p, uint64_t seed, uint32_t stream_id, uint64_t path_begin, uint64_t n_paths,
                                     int32_t working_months, const double* table, int32_t n_table, const mcr_outputs* out) {
    mcr_sizes sz;
    if (orc_query_sizes(p, working_months, &sz) != MCR_OK || !out || !table || n_table < 1) return MCR_ERR_INVALID_ARG;
    for (int32_t y = 0; y < n_table; ++y)
        if (!(std::isfinite(table[y]) && table[y] >= 0.0 && table[y] <= 1.0)) return MCR_ERR_INVALID_ARG;
    std::vector<mcr_params> blocks((size_t)n_table, *p);
    for (int32_t y = 0; y < n_table; ++y) blocks[(size_t)y].allocation_inv1_pct = table[y];
    const int64_t ts = out->path_stride > 0 ? out->path_stride : (int64_t)n_paths;
    std::vector<double> shocks(3 * (size_t)sz.shock_rows);
    for (uint64_t i = 0; i < n_paths; ++i) {
        orc_draw_shocks(seed, stream_id, path_begin + i, sz.shock_rows, p->equity_inflation_rho, shocks.data());
        Result r;
        glide_single_path(p, blocks, working_months, shocks.data(), sz.shock_rows, &r, out->trajectory ? out->trajectory + i : nullptr,
                          out->real_trajectory ? out->real_trajectory + i : nullptr,
                          out->withdrawal_rate_trajectory ? out->withdrawal_rate_trajectory + i : nullptr, ts);
        if (out->start_balance) out->start_balance[i] = r.start_balance;
        if (out->final_balance) out->final_balance[i] = r.final_balance;
        if (out->years_to_ruin) out->years_to_ruin[i] = r.years_to_ruin;
        if (out->first_year_gross_withdrawal) out->first_year_gross_withdrawal[i] = r.first_year_gross;
        if (out->first_year_real_gross_withdrawal) out->first_year_real_gross_withdrawal[i] = r.first_year_real_gross;
        if (out->inflation_at_retirement) out->inflation_at_retirement[i] = r.inflation_at_retirement;
        if (out->success) out->success[i] = (uint8_t)r.success;
    }
    return MCR_OK;
}
