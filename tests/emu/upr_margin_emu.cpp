// upr_margin_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the friction-margin jobs of
// upright_amd/csrc/upr_margin.h in both forms, and of the balance-check jobs of upr_balance.h with a friction scale per scenario.
// Next to the other emulation libraries of tests/emu/; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_margin.h"

namespace {
int states(const upr_problem* P, int n, const double* x, std::vector<double>& st) {
    st.resize((size_t)n * UPR_BAL_ST);
    for (int i = 0; i < n; ++i) {
        if (P->nq == 9) upr_bal_state_point<9>(P, x + (size_t)i * 27, st.data() + (size_t)i * UPR_BAL_ST);
        else if (P->nq == 6) upr_bal_state_point<6>(P, x + (size_t)i * 18, st.data() + (size_t)i * UPR_BAL_ST);
        else return 1;
    }
    return 0;
}
upr_bal_args jobs(const upr_problem* P, int n, const double* st, int n_scen, const double* params, int pdiv) {
    upr_bal_args A;
    A.P = P; A.n = n; A.n_scen = n_scen; A.st = st; A.params = params; A.pdiv = pdiv; A.eq_scale = 1.0 / std::sqrt(6.0 * P->nb);
    A.rho = nullptr; A.z = nullptr; A.iters = nullptr;
    return A;
}
int margin(const upr_problem* P, int n, const double* st, int n_scen, const double* params, int pdiv, double kappa_max, double* kappa_hi,
           double* kappa_lo, double* z, double* y, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_mar_args M;
    M.J = jobs(P, n, st, n_scen, params, pdiv);
    M.J.z = z; M.J.iters = iters;
    M.kappa_max = kappa_max; M.kappa_hi = kappa_hi; M.kappa_lo = kappa_lo; M.y = y;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    for (long long job = 0; job < (long long)n * n_scen; ++job) {
        if (lane) { upr_bal_margin_job1(M, L, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a job must write what it reads)
        upr_bal_margin_job(ctx, M, L, job, W.data());
    }
    return 0;
}
}  // namespace

extern "C" {

double emu_mar_feas(void) { return UPR_BAL_FEAS; }
int emu_mar_bisect(void) { return UPR_BAL_BISECT; }

// layouts of emu_bal_points (upr_balance_emu.cpp); kappa_hi[n][n_scen]; kappa_lo, z[..][ncol], y[..][6 nb], iters: each may be NULL.
// form: -1 the form the library launches, 0 a wave per job, 1 a lane per job (one body only)
int emu_mar_points(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, double kappa_max, double* kappa_hi,
                   double* kappa_lo, double* z, double* y, int* iters, int form) {
    std::vector<double> st;
    if (states(P, n, x, st)) return 1;
    return margin(P, n, st.data(), n_scen, params, pdiv, kappa_max, kappa_hi, kappa_lo, z, y, iters, form);
}

// the same on what the state kernel leaves, st[n][18]: C_we (row-major), omega, alpha, a
int emu_mar_states(const upr_problem* P, int n, const double* st, int n_scen, const double* params, int pdiv, double kappa_max, double* kappa_hi,
                   double* kappa_lo, double* z, double* y, int* iters, int form) {
    return margin(P, n, st, n_scen, params, pdiv, kappa_max, kappa_hi, kappa_lo, z, y, iters, form);
}

// the balance check with a friction scale per scenario (mu_scale[n_scen] or NULL: ones)
int emu_mar_rho_points(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, const double* mu_scale,
                       double* rho, double* z, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    std::vector<double> st;
    if (states(P, n, x, st)) return 1;
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_bal_args A = jobs(P, n, st.data(), n_scen, params, pdiv);
    A.rho = rho; A.z = z; A.iters = iters; A.mu_scale = mu_scale;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    for (long long job = 0; job < (long long)n * n_scen; ++job) {
        if (lane) { if (mu_scale) upr_bal_job1<true>(A, L, job); else upr_bal_job1<false>(A, L, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));
        if (mu_scale) upr_bal_job<true>(ctx, A, L, job, W.data()); else upr_bal_job<false>(ctx, A, L, job, W.data());
    }
    return 0;
}
}
