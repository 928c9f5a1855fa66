// upr_balance_emu.cpp -- TEST-ONLY host emulation (one thread per wave, -DUPR_HOST_EMU) of the balance-check kernels of
// upright_amd/csrc/upr_balance.h: the state kernel's point function and the projection job.  Next to the other emulation
// libraries of tests/emu/; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_balance.h"

extern "C" {

// the stopping rule and the cap, as the header names them
double emu_bal_tol(void) { return UPR_BAL_TOL; }
int emu_bal_iter_cap(int ncol) { return upr_bal_iter_cap(ncol); }

// x[n][3 nq]; params [n_scen][nb][10] (pdiv 0) or [n / pdiv][n_scen][nb][10]; rho[n][n_scen], z[n][n_scen][ncol] | NULL,
// iters[n][n_scen] | NULL.  form: -1 the form the library launches for this problem (upr_bal_lane_form), 0 the wave-per-job form, 1 the
// lane-per-job form (one body only).  Returns 0, or 1 for a chain length the kernels are not instantiated for / a form the problem cannot take.
int emu_bal_points(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, double* rho, double* z, int* iters, int form) {
    const bool lane = form < 0 ? upr_bal_lane_form(P->nb) : form == 1;
    if (lane && P->nb != 1) return 1;
    std::vector<double> st((size_t)n * UPR_BAL_ST);
    for (int i = 0; i < n; ++i) {
        if (P->nq == 9) upr_bal_state_point<9>(P, x + (size_t)i * 27, st.data() + (size_t)i * UPR_BAL_ST);
        else if (P->nq == 6) upr_bal_state_point<6>(P, x + (size_t)i * 18, st.data() + (size_t)i * UPR_BAL_ST);
        else return 1;
    }
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    upr_bal_args A;
    A.P = P; A.n = n; A.n_scen = n_scen; A.st = st.data(); A.params = params; A.pdiv = pdiv; A.eq_scale = 1.0 / std::sqrt(6.0 * P->nb);
    A.rho = rho; A.z = z; A.iters = iters;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> W(L.total);
    for (long long job = 0; job < (long long)n * n_scen; ++job) {
        if (lane) { upr_bal_job1(A, L, job); continue; }
        std::fill(W.begin(), W.end(), std::nan(""));   // (LDS is not zero: a job must write what it reads)
        upr_bal_job(ctx, A, L, job, W.data());
    }
    return 0;
}

// b[n][n_scen][6 nb] and the dense A[n][n_scen][6 nb][ncol] of the same jobs, columns out of upr_bal_column (the generator-matrix test)
int emu_bal_system(const upr_problem* P, int n, const double* x, int n_scen, const double* params, int pdiv, double* b, double* Am) {
    const upr_bal_dims L = upr_bal_layout(P->nb, P->nc, P->nf);
    const double scale = 1.0 / std::sqrt(6.0 * P->nb);
    for (int i = 0; i < n; ++i) {
        double st[UPR_BAL_ST];
        if (P->nq == 9) upr_bal_state_point<9>(P, x + (size_t)i * 27, st);
        else if (P->nq == 6) upr_bal_state_point<6>(P, x + (size_t)i * 18, st);
        else return 1;
        upr_ee<double> E;
        for (int k = 0; k < 9; ++k) E.C[k] = st[k];
        for (int k = 0; k < 3; ++k) { E.w[k] = st[9 + k]; E.al[k] = st[12 + k]; E.a[k] = st[15 + k]; E.p[k] = 0.0; E.v[k] = 0.0; }
        for (int s = 0; s < n_scen; ++s) {
            const size_t job = (size_t)i * n_scen + s;
            const double* bp = params + (size_t)10 * P->nb * ((pdiv ? (i / pdiv) * n_scen : 0) + s);
            const double zero3[3] = {0.0, 0.0, 0.0};
            for (int k = 0; k < P->nb; ++k) {
                double gb[6];
                upr_body_residual<double>(E, bp + 10 * k, P->gravity, zero3, zero3, gb);
                for (int c = 0; c < 6; ++c) b[job * L.m + 6 * k + c] = scale * gb[c];
            }
            double* Aj = Am + job * L.m * L.ncol;
            for (int e = 0; e < L.m * L.ncol; ++e) Aj[e] = 0.0;
            for (int j = 0; j < L.ncol; ++j) {
                int ba, bb; double va[6], vb[6];
                upr_bal_column(P, bp, scale, L.gpc, j, &ba, va, &bb, vb);
                for (int c = 0; c < 6; ++c) {
                    if (ba >= 0) Aj[(size_t)(6 * ba + c) * L.ncol + j] += va[c];
                    Aj[(size_t)(6 * bb + c) * L.ncol + j] += vb[c];
                }
            }
        }
    }
    return 0;
}
}
