// upr_value.h -- the value function of the last QP, for every instance of the batch: cost-to-go matrices P_k, gradients p_k, the
// cost-to-go J_k of the plan and the expansion points X_k at all knots (upr_value_kernel), and the second-order expansion
// evaluated at arbitrary (instance, t, x) points (upr_value_query_kernel).
//
// What it replaces: ocs2's getValueFunction behind ControllerInterface.valueFunction / valueFunctionStateDerivative
// (upright_control/src/pybindings.cpp:398-402), which the host module upright_amd/value_function.py answers for ONE instance
// with a numpy recursion.  Same stage Hessians, regularisations, terminal form and p_0 as that module (it is the specification;
// tests compare the two), one workgroup per instance, dimensions at run time:
//
//   * forces do not enter the dynamics and the input Hessian is blockdiag(jerk nq x nq DIAGONAL, contacts 3 x 3 | 1 x 1), so
//         P_k = Hxx + A'P+A - (Bq'P+A)' (Rq + Bq'P+Bq)^-1 (Bq'P+A) + C' S^-1 C,      S = Df Hff^-1 Df' + rho_s I
//     (the dual block of the hard equality and the penalty Z of a softened one both eliminate to the same Schur complement:
//     rho_s = 1 / Z, 1e-6 where the forces cannot span the rows, 1e-12 otherwise -- upr_qp_rho_s): an ne-square and an nq-square
//     Cholesky factor per knot, A'XA and Bq'X as combinations of nq-blocks;
//   * a softened inequality row enters with the weight the QP kernels factor, w0 (Z + w_s) / (Z + w0 + w_s), w0 = lam / t,
//     w_s = gam / tau (upr_soft_terms): the slack pairs come out of the multiplier export (upr_batch_qp_slack_pairs);
//   * J_k: tail sums of the stage costs (value_function.qp_objective) plus the penalties 1/2 Z sigma^2 + z sigma of the softened
//     rows and 1/2 Z |g + C dx + Df df|^2 of a softened equality at the knots >= k.
#pragma once
#include "upr_qp.h"

struct upr_vf_args {
    const upr_problem* P;
    upr_dims d;
    const double* xs;    // [B][N+1][nx] linearisation trajectory
    const double* us;    // [B][N][nu]
    const double* lin;   // [B][N+1][lin_stride]
    const double* Df;    // [B][ne][nfc]
    const double* ws;    // [B][ws_stride]: the QP's step at d.ws_dx / d.ws_du
    // the primal-dual point of the QP: the export buffer of the production kernel (upr_qp_args::kkt) or the instance workspace
    // of the kernels that keep their multipliers there; offsets of pi [N+1][nx], nu [N][ne] and of lam, t, sigma, tau, gam
    // [N+1][ni_stage] each.  o_sig < 0: the problem has no softened inequality rows
    const double* mult;
    long long mult_stride;
    int o_pi, o_nu, o_lam, o_t, o_sig, o_tau, o_gam;
    double* Pk;          // [B][N+1][nx][nx]
    double* pk;          // [B][N+1][nx]
    double* J;           // [B][N+1]
    double* X;           // [B][N+1][nx]
    // [B][N][ne] or NULL: the QP's multipliers nu of the object-dynamics rows, copied out of `mult` with the other per-knot stores
    // (the export buffer and the workspace are overwritten by the next QP; this copy is what the nu(t) query reads)
    double* nu_out = nullptr;
};

// LDS layout (doubles)
struct upr_vf_lds {
    int Pm, Tm, Am, BP, Gq, Wq, Mq, Lqi, Cm, Ym, Sm, Lsi, YF, Hfi, w, stg, flag, total;
};
static inline UPR_HD upr_vf_lds upr_vf_lds_layout(const upr_dims& d) {
    upr_vf_lds L; int o = 0;
    auto take = [&](int n) { int r = o; o += (n + 1) & ~1; return r; };
    L.Pm = take(d.nx * d.nx); L.Tm = take(d.nx * d.nx); L.Am = take(d.nx * d.nx);
    L.BP = take(d.nq * d.nx); L.Gq = take(d.nq * d.nx); L.Wq = take(d.nq * d.nx); L.Mq = take(d.nq * d.nq); L.Lqi = take(d.nq * d.nq);
    L.Cm = take(d.ne * d.nx); L.Ym = take(d.ne * d.nx); L.Sm = take(d.ne * d.ne); L.Lsi = take(d.ne * d.ne);
    L.YF = take(d.nfc * d.ne); L.Hfi = take(d.nf == 3 ? 9 * d.nc : d.nc);
    L.w = take(d.ni_stage); L.stg = take(d.N + 1); L.flag = take(2);
    L.total = o;
    return L;
}

// weight of slot j at knot k in the stage Hessian: lam / t, or the effective weight of a softened row
static UPR_HDI double upr_vf_weight(const upr_vf_args& A, const double* M, int k, int j) {
    const upr_dims& d = A.d;
    if (!upr_ineq_active(d, k, j)) return 0.0;
    const int e = k * d.ni_stage + j;
    const double w0 = M[A.o_lam + e] / M[A.o_t + e];
    if (A.o_sig < 0 || !upr_slot_soft(A.P, d, j)) return w0;
    const double Z = upr_slot_upper(d, j) ? A.P->soft_L2_upper : A.P->soft_L2_lower;
    const double wsl = M[A.o_gam + e] / M[A.o_tau + e];
    return w0 * (Z + wsl) / (Z + w0 + wsl);
}

// y[c] (c = beta nq + j) of v A for a row vector v[nx]: the exact discretisation of the triple integrator, A = [[I, h I, h^2/2 I], [0, I, h I], [0, 0, I]]
static UPR_HDI double upr_vf_times_A(const double* v, int nq, double h, int c) {
    const int beta = c / nq, j = c % nq;
    double r = v[c];
    if (beta >= 1) r += h * v[(beta - 1) * nq + j];
    if (beta == 2) r += 0.5 * h * h * v[j];
    return r;
}

static inline UPR_HD void upr_vf_instance(const upr_ctx& ctx, const upr_vf_args& A, int b, double* L) {
    const upr_dims& d = A.d;
    const upr_problem* P = A.P;
    const int nq = d.nq, nx = d.nx, nu = d.nu, ne = d.ne, nfc = d.nfc, nc = d.nc, N = d.N, ni = d.ni_stage, no = d.no;
    const double h = P->dt, h2 = 0.5 * h * h, a1 = h, a2 = 0.5 * h * h, a3 = h * h * h / 6.0;
    const upr_vf_lds o = upr_vf_lds_layout(d);
    const double* xs = A.xs + (size_t)b * (N + 1) * nx;
    const double* us = A.us + (size_t)b * N * nu;
    const double* lin = A.lin + (size_t)b * (N + 1) * d.lin_stride;
    const double* Df = A.Df + (size_t)b * ne * nfc;
    const double* dx = A.ws + (size_t)b * d.ws_stride + d.ws_dx;
    const double* du = A.ws + (size_t)b * d.ws_stride + d.ws_du;
    const double* M = A.mult + (size_t)b * A.mult_stride;
    double* Pk = A.Pk + (size_t)b * (N + 1) * nx * nx;
    double* pk = A.pk + (size_t)b * (N + 1) * nx;
    double* J = A.J + (size_t)b * (N + 1);
    double* X = A.X + (size_t)b * (N + 1) * nx;
    double *Pm = L + o.Pm, *Tm = L + o.Tm, *Am = L + o.Am, *BP = L + o.BP, *Gq = L + o.Gq, *Wq = L + o.Wq, *Mq = L + o.Mq, *Lqi = L + o.Lqi;
    double *Cm = L + o.Cm, *Ym = L + o.Ym, *Sm = L + o.Sm, *Lsi = L + o.Lsi, *YF = L + o.YF, *Hfi = L + o.Hfi, *w = L + o.w;
    const bool soft = A.o_sig >= 0;
    const double rho_s = upr_qp_rho_s(P, ne, nfc);

    // ---- expansion points, gradients of the knots k >= 1 (the costates), cost of every knot (a lane per knot)
    if (ctx.tid == 0) L[o.flag] = 0.0;
    UPR_FOR(e, (N + 1) * nx) { X[e] = xs[e] + dx[e]; if (e >= nx) pk[e] = M[A.o_pi + e]; }
    if (A.nu_out) { double* nuo = A.nu_out + (size_t)b * N * ne; UPR_FOR(e, N * ne) nuo[e] = M[A.o_nu + e]; }
    UPR_FOR(k, N + 1) {
        const double* rec = lin + (size_t)k * d.lin_stride;
        const double* dxk = dx + k * nx;
        double c = 0.0;
        if (k < N) {
            for (int i = 0; i < nx; ++i) { const double e = xs[k * nx + i] + dxk[i] - P->xd[i]; c += 0.5 * P->Qdiag[i] * e * e; }
            for (int i = 0; i < nu; ++i) { const double u = us[k * nu + i] + du[k * nu + i]; c += 0.5 * P->Rdiag[i] * u * u; }
            double ee = rec[d.lin_cost];   // Gauss-Newton model of the end-effector cost at the linearisation point
            for (int i = 0; i < nq; ++i) {
                double hv = 0.0;
                for (int j = 0; j < nq; ++j) hv += rec[d.lin_hess + upr_tri(nq, i, j)] * dxk[j];
                ee += dxk[i] * (rec[d.lin_grad + i] + 0.5 * hv);
            }
            c = h * (c + ee);
            if (P->soft_eq) for (int r = 0; r < ne; ++r) {   // the eliminated slack pair of a softened equality row
                double v = rec[d.lin_g + r];
                for (int i = 0; i < nx; ++i) v += rec[d.lin_gx + r * nx + i] * dxk[i];
                for (int j = 0; j < nfc; ++j) v += Df[r * nfc + j] * du[k * nu + nq + j];
                c += 0.5 * P->soft_L2_lower * v * v;
            }
        }
        if (soft) for (int j = 0; j < ni; ++j) if (upr_ineq_active(d, k, j) && upr_slot_soft(P, d, j)) {
            const double sg = M[A.o_sig + k * ni + j];
            const bool up = upr_slot_upper(d, j);
            c += 0.5 * (up ? P->soft_L2_upper : P->soft_L2_lower) * sg * sg + (up ? P->soft_L1_upper : P->soft_L1_lower) * sg;
        }
        L[o.stg + k] = c;
    }
    // ---- terminal knot: box rows + the proximal form of the terminal equality
    {
        const double* Jp = lin + (size_t)N * d.lin_stride + d.lin_hess;   // (the terminal record keeps the 3 x nq position Jacobian in the Hessian slot)
        UPR_FOR(e, nx * nx) {
            const int a = e / nx, c = e % nx;
            double v = (a == c) ? upr_vf_weight(A, M, N, a) + upr_vf_weight(A, M, N, nx + a) : 0.0;
            if (P->terminal_constraint) {
                if (a < nq && c < nq) { double s = 0.0; for (int r = 0; r < 3; ++r) s += Jp[r * nq + a] * Jp[r * nq + c]; v += s / UPR_QP_RHO_N; }
                else if (a == c) v += 1.0 / UPR_QP_RHO_N;
            }
            Pm[e] = v; Pk[(size_t)N * nx * nx + e] = v;
        }
    }
    UPR_SYNC();
    if (ctx.tid == 0) { double s = 0.0; for (int k = N; k >= 0; --k) { s += L[o.stg + k]; J[k] = s; } }

    for (int k = N - 1; k >= 0; --k) {
        const double* rec = lin + (size_t)k * d.lin_stride;
        UPR_FOR(j, ni) w[j] = upr_vf_weight(A, M, k, j);
        UPR_FOR(e, ne * nx) Cm[e] = rec[d.lin_gx + e];
        UPR_FOR(e, nq * nx) { const int i = e / nx, m = e % nx; BP[e] = a3 * Pm[i * nx + m] + a2 * Pm[(nq + i) * nx + m] + a1 * Pm[(2 * nq + i) * nx + m]; }   // Bq' P+
        UPR_FOR(e, nx * nx) Tm[e] = upr_vf_times_A(Pm + (e / nx) * nx, nq, h, e % nx);                                                                        // P+ A
        UPR_SYNC();
        // contact blocks of the input Hessian: inverse Cholesky factors (3 x 3 per contact, or a scalar)
        UPR_FOR(ci, nc) {
            if (d.nf == 3) {
                double* Bk = Hfi + 9 * ci;
                for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c)
                    Bk[3 * a + c] = (a == c) ? h * P->Rdiag[nq + 3 * ci + a] + w[2 * nx + nq + 3 * ci + a] + w[2 * nx + nu + nq + 3 * ci + a] : 0.0;
                for (int r = 0; r < 5; ++r) {
                    double e[3];
                    upr_friction_row_jac(P, ci, r, e);
                    const double wr = w[2 * nx + 2 * nu + 5 * ci + r];
                    Bk[0] += wr * e[0] * e[0]; Bk[1] += wr * e[0] * e[1]; Bk[2] += wr * e[0] * e[2];
                    Bk[3] += wr * e[1] * e[0]; Bk[4] += wr * e[1] * e[1]; Bk[5] += wr * e[1] * e[2];
                    Bk[6] += wr * e[2] * e[0]; Bk[7] += wr * e[2] * e[1]; Bk[8] += wr * e[2] * e[2];
                }
                if (!upr_chol_inv3(Bk)) L[o.flag] = 1.0;
            } else {
                const double v = h * P->Rdiag[nq + ci] + w[2 * nx + nq + ci] + w[2 * nx + nu + nq + ci];
                if (!(v > 0.0)) L[o.flag] = 1.0;
                Hfi[ci] = 1.0 / sqrt(v > 0.0 ? v : 1.0);
            }
        }
        UPR_FOR(e, nx * nx) { const int a = e / nx, c = e % nx, al = a / nq, i = a % nq;   // A' (P+ A)
            double v = Tm[e];
            if (al >= 1) v += h * Tm[((al - 1) * nq + i) * nx + c];
            if (al == 2) v += h2 * Tm[i * nx + c];
            Am[e] = v;
        }
        UPR_FOR(e, nq * nx) Gq[e] = upr_vf_times_A(BP + (e / nx) * nx, nq, h, e % nx);   // Bq' P+ A
        UPR_FOR(e, nq * nq) { const int i = e / nq, j = e % nq; const double* row = BP + i * nx;   // Rq + Bq' P+ Bq (Rq: h R and the jerk boxes, diagonal)
            double v = a3 * row[j] + a2 * row[nq + j] + a1 * row[2 * nq + j];
            if (i == j) v += h * P->Rdiag[i] + w[2 * nx + i] + w[2 * nx + nu + i];
            Mq[e] = v;
        }
        UPR_SYNC();
        UPR_FOR(e, nfc * ne) { const int i = e / ne, r = e % ne;   // Lf^-1 Df'
            double v;
            if (d.nf == 3) { const int ci = i / 3, a = i % 3; v = 0.0; for (int b2 = 0; b2 <= a; ++b2) v += Hfi[9 * ci + 3 * a + b2] * Df[r * nfc + 3 * ci + b2]; }
            else v = Hfi[i] * Df[r * nfc + i];
            YF[e] = v;
        }
        UPR_SYNC();
        UPR_FOR(e, ne * ne) { const int r = e / ne, s = e % ne;
            double v = (r == s) ? rho_s : 0.0;
            for (int i = 0; i < nfc; ++i) v += YF[i * ne + r] * YF[i * ne + s];
            Sm[e] = v;
        }
        UPR_SYNC();
        upr_chol_inv(ctx, Sm, Lsi, ne, L + o.flag);
        upr_chol_inv(ctx, Mq, Lqi, nq, L + o.flag);
        UPR_FOR(e, ne * nx) { const int r = e / nx, c = e % nx; double v = 0.0; for (int s = 0; s <= r; ++s) v += Lsi[r * ne + s] * Cm[s * nx + c]; Ym[e] = v; }
        UPR_FOR(e, nq * nx) { const int i = e / nx, c = e % nx; double v = 0.0; for (int s = 0; s <= i; ++s) v += Lqi[i * nq + s] * Gq[s * nx + c]; Wq[e] = v; }
        UPR_SYNC();
        const double* Jo = rec + d.lin_obs + no;   // state rows: d row / d q, [no][nq]
        UPR_FOR(e, nx * nx) { const int a = e / nx, c = e % nx;
            double v = Am[e];
            for (int i = 0; i < nq; ++i) v -= Wq[i * nx + a] * Wq[i * nx + c];
            for (int r = 0; r < ne; ++r) v += Ym[r * nx + a] * Ym[r * nx + c];
            if (a == c) v += h * P->Qdiag[a] + w[a] + w[nx + a];
            if (a < nq && c < nq) {
                v += h * rec[d.lin_hess + upr_tri(nq, a, c)];
                if (k >= 1) for (int r = 0; r < no; ++r) v += w[2 * nx + 2 * nu + d.np + r] * Jo[r * nq + a] * Jo[r * nq + c];
            }
            Tm[e] = v;
        }
        UPR_SYNC();
        UPR_FOR(e, nx * nx) { const int a = e / nx, c = e % nx; const double v = 0.5 * (Tm[a * nx + c] + Tm[c * nx + a]); Pm[e] = v; Pk[(size_t)k * nx * nx + e] = v; }
        if (k == 0) {
            // pi_0 is not a multiplier of the QP (x_0 is fixed): the gradient of the Lagrangian in x_0
            const double* pi1 = M + A.o_pi + nx; const double* nu0 = M + A.o_nu;
            UPR_FOR(i, nx) { const int al = i / nq, j = i % nq;
                double g = h * P->Qdiag[i] * (xs[i] + dx[i] - P->xd[i]);
                g += (al == 0) ? pi1[j] : (al == 1 ? h * pi1[j] + pi1[nq + j] : h2 * pi1[j] + h * pi1[nq + j] + pi1[2 * nq + j]);   // A' pi_1
                for (int r = 0; r < ne; ++r) g += Cm[r * nx + i] * nu0[r];
                if (i < nq) { double hv = 0.0; for (int m = 0; m < nq; ++m) hv += rec[d.lin_hess + upr_tri(nq, i, m)] * dx[m]; g += h * (rec[d.lin_grad + i] + hv); }
                pk[i] = g;
            }
        }
        UPR_SYNC();
    }
    // a factor that was not positive definite: no cost-to-go to report
    if (L[o.flag] != 0.0) UPR_FOR(k, N + 1) J[k] = NAN;
}

// ---- query: V and dV/dx at points (inst, t, x), the expansions of the two neighbouring knots interpolated linearly in t
// (value_function.ValueFunction._seg / value / gradient), and the equality multipliers nu(t) of the same segment
// (ValueFunction.equality_multiplier: piecewise linear, the last knot carries none, so nu[min(j + 1, N - 1)] is the right neighbour)
struct upr_vfq_args {
    upr_dims d;
    double dt;
    int n;
    const int* inst;     // [n]
    const double* t;     // [n]
    const double* x;     // [n][nx]
    const double* t0;    // [B] time of knot 0 of the plan the cost-to-go belongs to
    const double *Pk, *pk, *J, *X;
    double* V;           // [n]
    double* dV;          // [n][nx]
    const double* nu = nullptr;   // [B][N][ne] (upr_vf_args::nu_out) or NULL: no multiplier query
    double* nu_q = nullptr;       // [n][ne]
    // (x == NULL: the multiplier query alone -- V and dV are not written)
};
static inline UPR_HD void upr_vf_query_point(const upr_ctx& ctx, const upr_vfq_args& A, int p, double* L) {
    const int nx = A.d.nx, N = A.d.N, b = A.inst[p];
    double s = (A.t[p] - A.t0[b]) / A.dt;
    s = s > 0.0 ? s : 0.0; s = s < (double)N ? s : (double)N;
    int j = (int)s; if (j > N - 1) j = N - 1;
    const double a = s - j;
    if (A.nu) {   // (ne reaches 48 on the robust shape, 64 lanes a point: a loop over the rows, not a lane per row)
        const int ne = A.d.ne, jr = (j + 1 < N - 1) ? j + 1 : N - 1;
        const double* n0 = A.nu + ((size_t)b * N + j) * ne; const double* n1 = A.nu + ((size_t)b * N + jr) * ne;
        UPR_FOR(r, ne) A.nu_q[(size_t)p * ne + r] = (1.0 - a) * n0[r] + a * n1[r];
    }
    if (!A.x) return;
    const double* xp = A.x + (size_t)p * nx;
    UPR_FOR(i, nx) {
        for (int kk = 0; kk < 2; ++kk) {
            const size_t kn = (size_t)b * (N + 1) + j + kk;
            const double* row = A.Pk + (kn * nx + i) * nx; const double* Xk = A.X + kn * nx;
            double hv = 0.0;
            for (int m = 0; m < nx; ++m) hv += row[m] * (xp[m] - Xk[m]);
            const double pi = A.pk[kn * nx + i];
            L[kk * nx + i] = pi + hv;
            L[(2 + kk) * nx + i] = (xp[i] - Xk[i]) * (pi + 0.5 * hv);
        }
    }
    UPR_SYNC();
    UPR_FOR(i, nx) A.dV[(size_t)p * nx + i] = (1.0 - a) * L[i] + a * L[nx + i];
    if (ctx.tid == 0) {
        const size_t kn = (size_t)b * (N + 1) + j;
        double v0 = A.J[kn], v1 = A.J[kn + 1];
        for (int i = 0; i < nx; ++i) { v0 += L[2 * nx + i]; v1 += L[3 * nx + i]; }
        A.V[p] = (1.0 - a) * v0 + a * v1;
    }
}

#ifndef UPR_HOST_EMU
#define UPR_VF_NT 256
__global__ void __launch_bounds__(UPR_VF_NT) upr_value_kernel(upr_vf_args A) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = UPR_VF_NT;
    upr_vf_instance(ctx, A, blockIdx.x, smem);
}
__global__ void __launch_bounds__(64) upr_value_query_kernel(upr_vfq_args A) {
    __shared__ double sm[4 * UPR_MAX_NX];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    upr_vf_query_point(ctx, A, blockIdx.x, sm);
}
#endif
