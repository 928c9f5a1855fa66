// upr_replay_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the replay of a time law on a clock of
// upright_amd/csrc/upr_replay.h: the sampler's body per plan, the state point of upr_balance.h on the sample states, the jobs in both
// forms and the reduction over the samples, on plan arrays given directly; and the two device functions of the sampler on their own.
// Next to the other emulation libraries of tests/emu/; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_margin.h"
#include "../../upright_amd/csrc/upr_replay.h"

extern "C" {

// upr_rpl_locate on the knot times T [N + 1]
void emu_rpl_locate(const double* T, int N, double t, int* i, double* tp) { upr_rpl_locate(T, N, t, *i, *tp); }

// upr_rpl_state on two knot records; returns the box flag
int emu_rpl_state(const upr_problem* P, const double* x0, const double* x1, double s0, double s1, double h, double tp, double* out) {
    return upr_rpl_state(P, x0, x1, s0, s1, h, tp, out) ? 1 : 0;
}

// layouts of upr_batch_replay_plan with the plan xs [B][nk][3 nq] given; pdiv: 0 one set of scenarios for all instances, else a set per
// instance.  Every output may be NULL; times [B][nk] (or NULL): the knot times the sampler summed (NaN without a law).  form: -1 the form
// the library launches, 0 a wave per job, 1 a lane per job (one body only)
int emu_rpl_plan(const upr_problem* P, int B, int nk, const double* xs, int n_scen, const double* params, int pdiv, int n_lvl, const double* speeds,
                 const int* level, double tick, double t0, int K, int boxes, double* duration, int* count, double* x, double* rho, double* excess,
                 int* iters, double* worst, int* verdict, int* box_first, double* times, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    if (n_lvl < 1 || n_lvl > UPR_RET_MAX_LEVELS || nk < 2 || K < 1 || !level) return 1;
    const int nx = 3 * P->nq;
    const long long n = (long long)B * K, njobs = n * n_scen;
    std::vector<double> own_x, own_exc((size_t)njobs), st((size_t)n * UPR_BAL_ST), W(2 * (size_t)nk);
    std::vector<int> own_count((size_t)B);
    if (!x) { own_x.resize((size_t)n * nx); x = own_x.data(); }
    if (!excess) excess = own_exc.data();
    if (!count) count = own_count.data();
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    upr_rpl_sample_args Y;
    Y.P = P; Y.xs = xs; Y.speeds = speeds; Y.level = level; Y.nk = nk; Y.nx = nx; Y.K = K; Y.boxes = boxes; Y.h = P->dt; Y.tick = tick; Y.t0 = t0;
    Y.x = x; Y.duration = duration; Y.count = count; Y.box_first = box_first;
    for (int b = 0; b < B; ++b) {
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a plan must write what it reads)
        upr_bal_replay_sample(ctx, Y, b, W.data());
        if (times) for (int i = 0; i < nk; ++i) times[(size_t)b * nk + i] = W[nk + i];
    }
    for (long long i = 0; i < n; ++i) {
        if (P->nq == 9) upr_bal_state_point<9>(P, x + (size_t)i * 27, st.data() + (size_t)i * UPR_BAL_ST);
        else if (P->nq == 6) upr_bal_state_point<6>(P, x + (size_t)i * 18, st.data() + (size_t)i * UPR_BAL_ST);
        else return 1;
    }
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_rpl_args S;
    S.J.P = P; S.J.n = (int)n; S.J.n_scen = n_scen; S.J.st = st.data(); S.J.params = params; S.J.pdiv = pdiv ? K : 0;
    S.J.eq_scale = 1.0 / std::sqrt(6.0 * P->nb); S.J.rho = rho; S.J.z = nullptr; S.J.iters = iters;
    S.count = count; S.K = K; S.excess = excess;
    std::vector<double> Wj(L.total);
    for (long long job = 0; job < njobs; ++job) {
        if (lane) { upr_bal_replay_job1(S, L, job); continue; }
        std::fill(Wj.begin(), Wj.end(), std::nan(""));
        upr_bal_replay_job(ctx, S, L, job, Wj.data());
    }
    if (worst || verdict)
        for (long long o = 0; o < (long long)B * n_scen; ++o) upr_bal_replay_plan(excess, count, K, n_scen, o, worst, verdict);
    return 0;
}
}
