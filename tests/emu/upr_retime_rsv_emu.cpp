// upr_retime_rsv_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the retiming with a reserve of
// upright_amd/csrc/upr_retime_rsv.h: the mask jobs in both forms, then the dynamic programme of upr_retime.h's path kernel, on plan arrays
// given directly.  Next to the other emulation libraries of tests/emu/; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_retime_rsv.h"

extern "C" {

// emu_ret_plan of upr_retime_emu.cpp with dirs [n_dir][6], frame (0 world, 1 tray) and the reserve r >= 0; layouts of
// upr_batch_retime_plan_reserve with the plan xs [B][nk][3 nq] given; pdiv: 0 one set of scenarios for all instances, else nk (a set per
// instance).  reach, edges, iters: each may be NULL.  form: -1 the form the library launches, 0 a wave per job, 1 a lane per job (one body
// only)
int emu_ret_rsv_plan(const upr_problem* P, int B, int nk, const double* xs, int n_scen, const double* params, int pdiv, int n_lvl, const double* speeds,
                     int start, int end, int common, int boxes, int n_dir, const double* dirs, int frame, double reserve, double* duration, int* level,
                     int* reach, unsigned* edges, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    if (n_lvl < 1 || n_lvl > UPR_RET_MAX_LEVELS || nk < 2) return 1;
    if (n_dir < 1 || n_dir > UPR_DST_MAX_DIRS || !dirs || (frame != 0 && frame != 1) || !(reserve >= 0.0)) return 1;
    const int n = B * nk, nx = 3 * P->nq, N = nk - 1;
    std::vector<double> st((size_t)n * UPR_BAL_ST), vee((size_t)n * 3);
    for (int i = 0; i < n; ++i) {
        if (P->nq == 9) upr_bal_state_point<9>(P, xs + (size_t)i * 27, st.data() + (size_t)i * UPR_BAL_ST, vee.data() + (size_t)i * 3);
        else if (P->nq == 6) upr_bal_state_point<6>(P, xs + (size_t)i * 18, st.data() + (size_t)i * UPR_BAL_ST, vee.data() + (size_t)i * 3);
        else return 1;
    }
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    const long long njobs = (long long)B * n_scen * N * n_lvl;
    std::vector<unsigned> own_edges;
    if (!edges) { own_edges.resize((size_t)njobs); edges = own_edges.data(); }
    upr_ret_rsv_args V;
    upr_ret_args& S = V.T;
    S.J.P = P; S.J.n = n; S.J.n_scen = n_scen; S.J.st = st.data(); S.J.params = params; S.J.pdiv = pdiv; S.J.eq_scale = 1.0 / std::sqrt(6.0 * P->nb);
    S.J.rho = nullptr; S.J.z = nullptr; S.J.iters = iters;
    S.vee = vee.data(); S.xs = xs; S.speeds = speeds; S.M = n_lvl; S.nk = nk; S.nx = nx; S.boxes = boxes; S.h = P->dt; S.edges = edges;
    V.dirs = dirs; V.n_dir = n_dir; V.frame = frame; V.reserve = reserve;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    for (long long job = 0; job < njobs; ++job) {
        if (lane) { upr_bal_retime_rsv_job1(V, L, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a job must write what it reads)
        upr_bal_retime_rsv_job(ctx, V, L, job, W.data());
    }
    const long long nout = (long long)B * (common ? 1 : n_scen);
    std::vector<unsigned char> arg((size_t)nout * N * n_lvl);
    std::vector<double> own_dur;
    if (!duration) { own_dur.resize((size_t)nout); duration = own_dur.data(); }
    upr_ret_path_args Q;
    Q.edges = edges; Q.speeds = speeds; Q.M = n_lvl; Q.nk = nk; Q.n_scen = n_scen; Q.common = common; Q.start = start; Q.end = end; Q.h = P->dt;
    Q.arg = arg.data(); Q.duration = duration; Q.level = level; Q.reach = reach;
    double T[2 * UPR_RET_MAX_LEVELS];
    for (long long o = 0; o < nout; ++o) {
        std::fill(T, T + 2 * UPR_RET_MAX_LEVELS, std::nan(""));
        upr_bal_retime_path(ctx, Q, o, T);
    }
    return 0;
}
}
