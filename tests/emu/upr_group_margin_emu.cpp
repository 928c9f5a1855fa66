// upr_group_margin_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the group friction margin of
// upright_amd/csrc/upr_margin.h in both forms, of the balance-check jobs of upr_balance.h with a friction scale per scenario and
// contact, and of the reduction over the knots of a plan.  Next to the other emulation libraries of tests/emu/; never part of
// libupright_mi.so.
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
}  // namespace

extern "C" {

// layouts of emu_mar_points (upr_margin_emu.cpp) with a trailing group axis on every output; group_mask[n_grp]; mu_base[n_scen][nc]
// or NULL.  form: -1 the form the library launches, 0 a wave per job, 1 a lane per job (one body only)
int emu_grp_points(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, int n_grp, const unsigned* group_mask,
                   const double* mu_base, double kappa_max, double* kappa_hi, double* kappa_lo, double* z, double* y, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    std::vector<double> st;
    if (states(P, n, x, st)) return 1;
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_grp_args X;
    X.M.J = jobs(P, n, st.data(), n_scen, params, pdiv);
    X.M.J.z = z; X.M.J.iters = iters;
    X.M.kappa_max = kappa_max; X.M.kappa_hi = kappa_hi; X.M.kappa_lo = kappa_lo; X.M.y = y;
    X.n_grp = n_grp; X.group_mask = group_mask; X.mu_base = mu_base;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    const long long njobs = (long long)n * n_scen;
    if (lane) {
        for (int g = 0; g < n_grp; ++g)   // (the launch: the group on blockIdx.y)
            for (long long job = 0; job < njobs; ++job) upr_bal_margin_grp_job1(X, L, job, g);
        return 0;
    }
    for (long long jg = 0; jg < njobs * n_grp; ++jg) {
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a job must write what it reads)
        upr_bal_margin_grp_job(ctx, X, L, jg, W.data());
    }
    return 0;
}

// the balance check with a friction scale per scenario and contact, mu_scale_c[n_scen][nc]
int emu_grp_rho_points(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, const double* mu_scale_c,
                       double* rho, double* z, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if ((lane && P->nb != 1) || !mu_scale_c) return 1;
    std::vector<double> st;
    if (states(P, n, x, st)) return 1;
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_bal_args A = jobs(P, n, st.data(), n_scen, params, pdiv);
    A.rho = rho; A.z = z; A.iters = iters; A.mu_scale = mu_scale_c;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    for (long long job = 0; job < (long long)n * n_scen; ++job) {
        if (lane) { upr_bal_job1<2>(A, L, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));
        upr_bal_job<2>(ctx, A, L, job, W.data());
    }
    return 0;
}

// kappa_hi[B][nk][inner] -> worst[B][inner], knot[B][inner] (or NULL)
int emu_grp_worst(const double* kappa_hi, int B, int nk, long long inner, double* worst, int* knot) {
    for (long long o = 0; o < (long long)B * inner; ++o) upr_bal_margin_worst(kappa_hi, nk, inner, o, worst, knot);
    return 0;
}
}
