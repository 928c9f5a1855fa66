// upr_retime_sub_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the retiming with substeps of
// upright_amd/csrc/upr_retime_sub.h: the refinement of the plan, the state point of upr_pathacc.h on the fine points, the mask jobs in both
// forms, then the programme of upr_retime.h's path kernel, on plan arrays given directly.  Next to the other emulation libraries of
// tests/emu/; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_margin.h"
#include "../../upright_amd/csrc/upr_retime_sub.h"

extern "C" {

// upr_sub_speed on its own
double emu_sub_speed(double sm, double sp, int r, int R) { return upr_sub_speed(sm, sp, r, R); }

// the fine plan xf [B][(nk - 1) R + 1][3 nq] of the plan xs [B][nk][3 nq] (the refinement kernel's body)
int emu_ret_sub_refine(const upr_problem* P, int B, int nk, const double* xs, int substeps, double* xf) {
    if (nk < 2 || substeps < 1 || substeps > UPR_SUB_MAX) return 1;
    upr_sub_refine_args F;
    F.P = P; F.xs = xs; F.nk = nk; F.nx = 3 * P->nq; F.R = substeps; F.h = P->dt; F.xf = xf;
    const long long n = (long long)B * ((long long)(nk - 1) * substeps + 1);
    for (long long p = 0; p < n; ++p) upr_bal_refine(F, p);
    return 0;
}

// layouts of upr_batch_retime_plan_substeps with the plan xs [B][nk][3 nq] given; pdiv: 0 one set of scenarios for all instances, else a
// set per instance.  reach, edges, iters: each may be NULL.  form: -1 the form the library launches, 0 a wave per job, 1 a lane per job
// (one body only)
int emu_ret_sub_plan(const upr_problem* P, int B, int nk, const double* xs, int n_scen, const double* params, int pdiv, int n_lvl, const double* speeds,
                     int start, int end, int common, int boxes, int substeps, double* duration, int* level, int* reach, unsigned* edges, int* iters,
                     int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    if (n_lvl < 1 || n_lvl > UPR_RET_MAX_LEVELS || nk < 2 || substeps < 1 || substeps > UPR_SUB_MAX) return 1;
    const int nx = 3 * P->nq, N = nk - 1, per = N * substeps + 1, n = B * per;
    std::vector<double> xf((size_t)n * nx), st((size_t)n * UPR_BAL_ST), vee((size_t)n * 3);
    if (emu_ret_sub_refine(P, B, nk, xs, substeps, xf.data())) return 1;
    for (int i = 0; i < n; ++i) {
        if (P->nq == 9) upr_bal_state_point<9>(P, xf.data() + (size_t)i * 27, st.data() + (size_t)i * UPR_BAL_ST, vee.data() + (size_t)i * 3);
        else if (P->nq == 6) upr_bal_state_point<6>(P, xf.data() + (size_t)i * 18, st.data() + (size_t)i * UPR_BAL_ST, vee.data() + (size_t)i * 3);
        else return 1;
    }
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    const long long njobs = (long long)B * n_scen * N * n_lvl;
    std::vector<unsigned> own_edges;
    if (!edges) { own_edges.resize((size_t)njobs); edges = own_edges.data(); }
    upr_ret_sub_args S;
    upr_ret_args& T = S.T;
    T.J.P = P; T.J.n = n; T.J.n_scen = n_scen; T.J.st = st.data(); T.J.params = params; T.J.pdiv = pdiv ? per : 0; T.J.eq_scale = 1.0 / std::sqrt(6.0 * P->nb);
    T.J.rho = nullptr; T.J.z = nullptr; T.J.iters = iters;
    T.vee = vee.data(); T.xs = xf.data(); T.speeds = speeds; T.M = n_lvl; T.nk = nk; T.nx = nx; T.boxes = boxes; T.h = P->dt; T.edges = edges;
    S.R = substeps;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    for (long long job = 0; job < njobs; ++job) {
        if (lane) { upr_bal_retime_sub_job1(S, L, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a job must write what it reads)
        upr_bal_retime_sub_job(ctx, S, L, job, W.data());
    }
    const long long nout = (long long)B * (common ? 1 : n_scen);
    std::vector<unsigned char> arg((size_t)nout * N * n_lvl);
    std::vector<double> own_dur;
    if (!duration) { own_dur.resize((size_t)nout); duration = own_dur.data(); }
    upr_ret_path_args Q;
    Q.edges = edges; Q.speeds = speeds; Q.M = n_lvl; Q.nk = nk; Q.n_scen = n_scen; Q.common = common; Q.start = start; Q.end = end; Q.h = P->dt;
    Q.arg = arg.data(); Q.duration = duration; Q.level = level; Q.reach = reach;
    double Tw[2 * UPR_RET_MAX_LEVELS];
    for (long long o = 0; o < nout; ++o) {
        std::fill(Tw, Tw + 2 * UPR_RET_MAX_LEVELS, std::nan(""));
        upr_bal_retime_path(ctx, Q, o, Tw);
    }
    return 0;
}
}
