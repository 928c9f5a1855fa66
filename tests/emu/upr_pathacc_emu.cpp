// upr_pathacc_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the path-acceleration-margin jobs of
// upright_amd/csrc/upr_pathacc.h in both forms, the right-hand side of a transformed state and the reductions over the knots of a
// plan.  Next to the other emulation libraries of tests/emu/; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_pathacc.h"

namespace {
int states(const upr_problem* P, int n, const double* x, std::vector<double>& st, std::vector<double>& vee) {
    st.resize((size_t)n * UPR_BAL_ST);
    vee.resize((size_t)n * 3);
    for (int i = 0; i < n; ++i) {
        if (P->nq == 9) upr_bal_state_point<9>(P, x + (size_t)i * 27, st.data() + (size_t)i * UPR_BAL_ST, vee.data() + (size_t)i * 3);
        else if (P->nq == 6) upr_bal_state_point<6>(P, x + (size_t)i * 18, st.data() + (size_t)i * UPR_BAL_ST, vee.data() + (size_t)i * 3);
        else return 1;
    }
    return 0;
}
}  // namespace

extern "C" {

// layouts of upr_batch_path_accel_margin_points; z, y, iters: each may be NULL.  form: -1 the form the library launches, 0 a wave per
// job, 1 a lane per job (one body only)
int emu_pac_points(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, double d_max, double speed, double* accel,
                   double* z, double* y, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    std::vector<double> st, vee;
    if (states(P, n, x, st, vee)) return 1;
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_pac_args S;
    S.J.P = P; S.J.n = n; S.J.n_scen = n_scen; S.J.st = st.data(); S.J.params = params; S.J.pdiv = pdiv; S.J.eq_scale = 1.0 / std::sqrt(6.0 * P->nb);
    S.J.rho = nullptr; S.J.z = z; S.J.iters = iters;
    S.d_max = d_max; S.speed = speed; S.vee = vee.data(); S.accel = accel; S.y = y;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    for (long long job = 0; job < (long long)n * n_scen; ++job) {
        if (lane) { upr_bal_pathacc_job1(S, L, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a job must write what it reads)
        upr_bal_pathacc_job(ctx, S, L, job, W.data());
    }
    return 0;
}

// b [n][6 nb] of the states x at sdot = speed, sddot = d under one parameter set theta [nb][10]: the state point with v_ee, the
// transformed record and the rhs routine, as a job builds it
int emu_pac_rhs(const upr_problem* P, int n, const double* x, const double* theta, double speed, double d, double* b) {
    std::vector<double> st, vee;
    if (states(P, n, x, st, vee)) return 1;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    for (int i = 0; i < n; ++i) {
        double ss[UPR_BAL_ST];
        upr_pac_transform(st.data() + (size_t)i * UPR_BAL_ST, vee.data() + (size_t)i * 3, speed, d, ss);
        upr_bal_rhs(ctx, P, ss, theta, 1.0 / std::sqrt(6.0 * P->nb), b + (size_t)i * 6 * P->nb);
    }
    return 0;
}

// the reductions of upr_bal_pathacc_plan_kernel: accel [B][nk][n_scen][4] -> window, knot [B][n_scen][2]; limit [B][2] from xs [B][nk][nx]
// (limit, xs may be NULL)
int emu_pac_plan(const upr_problem* P, int B, int nk, int n_scen, const double* accel, int nx, double speed, const double* xs, double* window, int* knot,
                 double* limit) {
    for (long long o = 0; o < (long long)B * n_scen * 2; ++o) upr_bal_speed_window(accel, nk, n_scen, o, window, knot);
    if (limit)
        for (int b = 0; b < B; ++b) upr_bal_pathacc_limit(P, nk, nx, speed, xs + (size_t)b * nk * nx, limit + 2 * b);
    return 0;
}
}
