// upr_disturb_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the disturbance-margin jobs of
// upright_amd/csrc/upr_disturb.h in both forms, the right-hand side of a displaced record and the reductions over the knots of a plan
// and over the directions.  Next to the other emulation libraries of tests/emu/; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_disturb.h"

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
}  // namespace

extern "C" {

// layouts of upr_batch_disturbance_margin_points (direction-major); z, y, iters: each may be NULL.  form: -1 the form the library
// launches, 0 a wave per job, 1 a lane per job (one body only)
int emu_dst_points(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, int n_dir, const double* dirs, int frame,
                   double r_max, double* reach, double* z, double* y, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    std::vector<double> st;
    if (states(P, n, x, st)) return 1;
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_dst_args S;
    S.J.P = P; S.J.n = n; S.J.n_scen = n_scen; S.J.st = st.data(); S.J.params = params; S.J.pdiv = pdiv; S.J.eq_scale = 1.0 / std::sqrt(6.0 * P->nb);
    S.J.rho = nullptr; S.J.z = z; S.J.iters = iters;
    S.r_max = r_max; S.dirs = dirs; S.n_dir = n_dir; S.frame = frame; S.reach = reach; S.y = y;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    const long long per = (long long)n * n_scen;
    // (the order of the wave kernel: jobs x directions, the direction the slow index)
    for (long long t = 0; t < per * n_dir; ++t) {
        const long long d = t / per, job = t - d * per;
        if (lane) { upr_bal_disturb_job1(S, L, (int)d, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a job must write what it reads)
        upr_bal_disturb_job(ctx, S, L, (int)d, job, W.data());
    }
    return 0;
}

// b [n][6 nb] of the states x displaced by r along u [6] under one parameter set theta [nb][10]: the state point, the displaced record
// and the rhs routine, as a job builds it
int emu_dst_rhs(const upr_problem* P, int n, const double* x, const double* theta, const double* u, int frame, double r, double* b) {
    std::vector<double> st;
    if (states(P, n, x, st)) return 1;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    for (int i = 0; i < n; ++i) {
        double ss[UPR_BAL_ST];
        upr_dst_transform(st.data() + (size_t)i * UPR_BAL_ST, u, frame, r, ss);
        upr_bal_rhs(ctx, P, ss, theta, 1.0 / std::sqrt(6.0 * P->nb), b + (size_t)i * 6 * P->nb);
    }
    return 0;
}

// the reductions of upr_bal_disturb_plan_kernel: reach [n_dir][B][nk][n_scen][4] -> window, knot [n_dir][B][n_scen][2], radius [B][n_scen],
// binding [B][n_scen][3]
int emu_dst_plan(int B, int nk, int n_scen, int n_dir, const double* reach, double* window, int* knot, double* radius, int* binding) {
    const long long nbs = (long long)B * n_scen;
    for (long long bs = 0; bs < nbs; ++bs) upr_bal_disturb_reduce(reach, nk, n_scen, n_dir, nbs, bs, window, knot, radius, binding);
    return 0;
}
}
