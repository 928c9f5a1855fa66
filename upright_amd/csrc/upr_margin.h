// upr_margin.h -- batched friction margin: the smallest common scale kappa* on the friction coefficients of an arrangement at
// which a (state, inertial-parameter scenario) pair is balanced.
//
// What it replaces: the --mu re-evaluation of upright_robust/scripts/process_sim_runs.py, one friction coefficient per pass over a
// run directory, and the SLSQP search of upright_cmd/scripts/tools/compute_minimum_mu.py, one arrangement at a time.
//
// The quantity.  A(kappa) is the generator matrix of upr_balance.h with every contact's mu_i replaced by kappa mu_i,
// rho(x; theta, kappa) the distance of upr_balance.h with A(kappa).  The pyramids are nested in kappa, so rho does not increase
// with kappa, and
//
//     kappa*(x; theta) = inf { kappa in [0, kappa_max] : rho(x; theta, kappa) <= UPR_BAL_FEAS max(|b|, 1) },     +inf if there is none.
//
// kappa* < 1: balanced with 1 - kappa* of the friction to spare; kappa* > 1: this much more friction would have been needed;
// kappa* = 0: normal forces alone balance the state; +inf: no friction helps (tipping, lift-off).  The smallest friction
// coefficient of contact i is kappa* mu_i.  The force bounds are not part of it.
//
// The algorithm.  rho at kappa = 0: feasible -> 0.  Else rho at kappa_max: infeasible -> +inf.  Else UPR_BAL_BISECT arithmetic
// halvings of [0, kappa_max]; kappa_hi, the last feasible point, is the answer, kappa_lo the last infeasible one.  Every decision is
// rho <= UPR_BAL_FEAS max(|b|, 1) on the rho the projection of upr_balance.h returns (upr_bal_project / upr_bal_project1, the bodies
// the rho kernels run: shared, cold at every evaluation, no stopping rule of their own here).  nf = 1 generators carry no mu: one
// evaluation, 0 or +inf.  The multipliers z of the last feasible point and the residual y = b + A(kappa_lo) z of the last infeasible
// one go to global memory at the evaluation that produced them (plain stores; nothing of them is carried across projections):
// z >= 0 with |b + A(kappa_hi) z| inside the ball proves kappa_hi feasible, and y' a_j >= 0 for every column with
// y' b / |y| outside the ball proves kappa_lo infeasible (y' (b + A z) >= y' b for every z >= 0).
//
// The margin of a contact group (upr_grp_args; compute_minimum_mu.py:12-30 gives every pair of objects its own friction coefficient,
// compute_contact_idx).  beta[sc][i] >= 0 is a base scale per scenario and contact (1 without a table), G_g a set of contacts, A_g(kappa)
// the generator matrix built on kappa mu_i for i in G_g and on beta[sc][i] mu_i elsewhere, rho_g the distance with A_g, and
//
//     kappa*_g(x; theta) = inf { kappa in [0, kappa_max] : rho_g(x; theta, kappa) <= UPR_BAL_FEAS max(|b|, 1) },     +inf if there is none.
//
// Only the pyramids of G_g grow with kappa, so rho_g does not increase and the algorithm above holds unchanged; the group jobs are the
// job templates below with the per-contact scale source of upr_balance.h (upr_bal_mu_grp), output index
// (point n_scen + scenario) n_grp + group.  kappa*_g = 0: the group's friction is not needed; +inf: no friction on this group alone
// helps.  upr_bal_margin_worst_kernel reduces kappa_hi over the knots of a plan.
#pragma once
#include "upr_balance.h"

// a state counts as balanced when rho <= UPR_BAL_FEAS max(|b|, 1): the tolerance the controller's QP enforces the equality to
#define UPR_BAL_FEAS 1e-8
// halvings of [0, kappa_max]: the final width kappa_max 2^-32 (1.9e-9 at kappa_max = 8) is below the shift the rule above causes
#define UPR_BAL_BISECT 32

struct upr_mar_args {
    upr_bal_args J;          // the jobs: P, n, n_scen, st, params, pdiv, eq_scale; z [n][n_scen][ncol] at kappa_hi or NULL; iters: the
                             // least-squares solves over all evaluations, or NULL; rho and mu_scale are not read
    double kappa_max;
    double* kappa_hi;        // [n][n_scen]
    double* kappa_lo;        // [n][n_scen] or NULL
    double* y;               // [n][n_scen][6 nb] or NULL
};

// the group margin: the jobs of M times n_grp groups; kappa_hi, kappa_lo, iters [n][n_scen][n_grp], z [..][ncol], y [..][6 nb]
struct upr_grp_args {
    upr_mar_args M;
    int n_grp;
    const unsigned* group_mask;   // [n_grp]: bit i set -- contact i belongs to the group
    const double* mu_base;        // [n_scen][nc] or NULL: ones
};
// the scale source of an evaluation at kappa: every contact (the common margin) or the contacts of the job's group
template <bool GRP> struct upr_mar_src {
    typedef upr_bal_mu_all T;
    static UPR_HDI T of(unsigned, const double*, double kap) { return T{kap}; }
};
template <> struct upr_mar_src<true> {
    typedef upr_bal_mu_grp T;
    static UPR_HDI T of(unsigned mask, const double* base, double kap) { return T{mask, kap, base}; }
};

// ---- the residual of an infeasible evaluation as a certificate -----------------------------------------------------------------------
// r = b + A z is orthogonal to its passive columns to the rounding of b and A z, numbers of size |b|; at the boundary |r| is 1e-8 of
// that, and y' b = |y|^2 - sum z_j a_j' y is left with an error of the size of |y|^2 itself.  One least-squares step ON r (every
// number in it is of the size of r) takes the passive columns out of it to the rounding of r: y = r - A_P (A_P' A_P)^-1 A_P' r, still
// b + A z for multipliers that differ from z in their last digits.  The decision was taken before, on the rho of the projection.
static UPR_HDI void upr_bal_polish(const upr_ctx& ctx, const upr_bal_dims& L, double* W, int np) {
    double *r = W + L.o_r, *y = W + L.o_y, *pc = W + L.o_pcol, *G = W + L.o_G;
    const int* pb = (const int*)(W + L.o_int) + L.mp;
    UPR_WSYNC();
    UPR_FOR(i, np) y[i] = -upr_bal_dot_dense(pc, pb, i, r);
    UPR_WSYNC();
    upr_bal_solve(ctx, L.mp, np, G, y);
    upr_bal_residual(ctx, L, np, r, pc, pb, y, r);
}
static UPR_HDI void upr_bal_polish1(const double (&pc)[UPR_BAL1_MP][6], const double (&G)[UPR_BAL1_MP][UPR_BAL1_MP], int np, double (&r)[6]) {
    constexpr int MP = UPR_BAL1_MP;
    double t[MP];
#pragma unroll
    for (int i = 0; i < MP; ++i) {
        double acc = 0.0;
        for (int c = 0; c < 6; ++c) acc += pc[i][c] * r[c];
        t[i] = (i < np) ? -acc : 0.0;
    }
    // (slots from np on are not part of the system, whatever an abandoned column left in their rows)
#pragma unroll
    for (int k = 0; k < MP; ++k) {
        t[k] = (k < np) ? t[k] / G[k][k] : 0.0;
#pragma unroll
        for (int i = k + 1; i < MP; ++i) t[i] -= (i < np) ? G[i][k] * t[k] : 0.0;
    }
#pragma unroll
    for (int k = MP - 1; k >= 0; --k) {
        t[k] = (k < np) ? t[k] / G[k][k] : 0.0;
#pragma unroll
        for (int i = 0; i < k; ++i) t[i] -= G[k][i] * t[k];
    }
#pragma unroll
    for (int i = 0; i < MP; ++i) if (i < np) for (int c = 0; c < 6; ++c) r[c] += t[i] * pc[i][c];
}

// ---- a wave per job ------------------------------------------------------------------------------------------------------------------
// GRP: the margin of one contact group -- mask its contacts, mu_base the table of base scales (or NULL), out the index of the
// job's outputs; without GRP the three are not read and the outputs go to index job
template <bool GRP = false>
static UPR_HDI void upr_bal_margin_job(const upr_ctx& ctx, const upr_mar_args& M, const upr_bal_dims& L, long long job, double* W, long long out_grp = 0,
                                       unsigned mask = 0u, const double* mu_base = nullptr) {
    typedef upr_mar_src<GRP> SRC;
    const upr_bal_args& A = M.J;
    const upr_problem* P = A.P;
    const long long pt = job / A.n_scen;
    const int sc = (int)(job - pt * A.n_scen);
    const double* bp = A.params + (size_t)10 * P->nb * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const long long out = GRP ? out_grp : job;
    const double* base = (GRP && mu_base) ? mu_base + (size_t)sc * P->nc : nullptr;
    double* zo = A.z ? A.z + (size_t)out * L.ncol : nullptr;
    double* yo = M.y ? M.y + (size_t)out * L.m : nullptr;
    const double* r = W + L.o_r;
    const int cap = upr_bal_iter_cap(L.ncol);
    UPR_WSYNC();   // (the previous job of this wave is done with the workspace)
    upr_bal_rhs(ctx, P, A.st + (size_t)pt * UPR_BAL_ST, bp, A.eq_scale, W + L.o_b);
    int np, it, total; double bnorm;
    double lo = 0.0, hi = 0.0;
    const double rho0 = upr_bal_project(ctx, P, L, bp, A.eq_scale, SRC::of(mask, base, 0.0), W, &np, &it, &bnorm);
    total = it;
    const double lim = UPR_BAL_FEAS * (bnorm > 1.0 ? bnorm : 1.0);
    if (rho0 <= lim) {
        if (zo) upr_bal_put_z(ctx, L, W, np, zo);
        if (yo) UPR_FOR(e, L.m) yo[e] = 0.0;
    } else {
        if (yo) { if (it < cap) upr_bal_polish(ctx, L, W, np); UPR_FOR(e, L.m) yo[e] = r[e]; }
        bool feasible = false;
        if (L.gpc == 4) {
            UPR_WSYNC();
            const double rho1 = upr_bal_project(ctx, P, L, bp, A.eq_scale, SRC::of(mask, base, M.kappa_max), W, &np, &it, &bnorm);
            total += it;
            feasible = rho1 <= lim;
        }
        if (!feasible) {
            lo = M.kappa_max; hi = INFINITY;
            if (L.gpc == 4 && yo) { if (it < cap) upr_bal_polish(ctx, L, W, np); UPR_FOR(e, L.m) yo[e] = r[e]; }
            if (zo) UPR_FOR(j, L.ncol) zo[j] = 0.0;
        } else {
            hi = M.kappa_max;
            if (zo) upr_bal_put_z(ctx, L, W, np, zo);
            for (int k = 0; k < UPR_BAL_BISECT; ++k) {
                const double mid = 0.5 * (lo + hi);
                UPR_WSYNC();
                const double rho = upr_bal_project(ctx, P, L, bp, A.eq_scale, SRC::of(mask, base, mid), W, &np, &it, &bnorm);
                total += it;
                if (rho <= lim) { hi = mid; if (zo) upr_bal_put_z(ctx, L, W, np, zo); }
                else { lo = mid; if (yo) { if (it < cap) upr_bal_polish(ctx, L, W, np); UPR_FOR(e, L.m) yo[e] = r[e]; } }
            }
        }
    }
    if (ctx.tid == 0) {
        M.kappa_hi[out] = hi;
        if (M.kappa_lo) M.kappa_lo[out] = lo;
        if (A.iters) A.iters[out] = total;
    }
}

// ---- one-body arrangements: a lane per job ----------------------------------------------------------------------------------------------
template <bool GRP = false>
static UPR_HDI void upr_bal_margin_job1(const upr_mar_args& M, const upr_bal_dims& L, long long job, long long out_grp = 0, unsigned mask = 0u,
                                        const double* mu_base = nullptr) {
    typedef upr_mar_src<GRP> SRC;
    const upr_bal_args& A = M.J;
    const upr_problem* P = A.P;
    const long long pt = job / A.n_scen;
    const int sc = (int)(job - pt * A.n_scen);
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const long long out = GRP ? out_grp : job;
    const double* base = (GRP && mu_base) ? mu_base + (size_t)sc * P->nc : nullptr;
    double* zo = A.z ? A.z + (size_t)out * L.ncol : nullptr;
    double* yo = M.y ? M.y + (size_t)out * 6 : nullptr;
    double b[6];
    upr_bal_rhs1(P, A.st + (size_t)pt * UPR_BAL_ST, bp, A.eq_scale, b);
    double bb2 = 0.0;
    for (int c = 0; c < 6; ++c) bb2 += b[c] * b[c];
    const double bnorm = sqrt(bb2), s1 = bnorm > 1.0 ? bnorm : 1.0, thr = UPR_BAL_TOL * s1, lim = UPR_BAL_FEAS * s1;
    double lo = 0.0, hi = 0.0;
    int total = 0;
    // evaluations: 0 at kappa = 0, 1 at kappa_max, then the halvings -- one copy of the projection's code for all of them
    const int last = (L.gpc == 4) ? 1 + UPR_BAL_BISECT : 0;
    for (int ev = 0; ev <= last; ++ev) {
        const double kap = (ev == 0) ? 0.0 : (ev == 1) ? M.kappa_max : 0.5 * (lo + hi);
        double r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
        int pidx[UPR_BAL1_MP], np;
        const int it = upr_bal_project1(P, L, bp, A.eq_scale, SRC::of(mask, base, kap), b, thr, r, zp, pidx, np, pc, G);
        total += it;
        double rr = 0.0;
        for (int c = 0; c < 6; ++c) rr += r[c] * r[c];
        const bool feasible = sqrt(rr) <= lim;
        if (feasible) {
            hi = kap;
            if (zo) upr_bal_put_z1(L.ncol, zp, pidx, np, zo);
        } else {
            lo = kap;
            if (yo) {
                if (it < upr_bal_iter_cap(L.ncol)) upr_bal_polish1(pc, G, np, r);
                for (int c = 0; c < 6; ++c) yo[c] = r[c];
            }
        }
        if (ev == 0) {
            if (feasible) { if (yo) for (int c = 0; c < 6; ++c) yo[c] = 0.0; break; }
            if (last == 0) { lo = M.kappa_max; hi = INFINITY; }
        } else if (ev == 1 && !feasible) {
            hi = INFINITY;
            break;
        }
    }
    if (hi == INFINITY && zo) for (int j = 0; j < L.ncol; ++j) zo[j] = 0.0;
    M.kappa_hi[out] = hi;
    if (M.kappa_lo) M.kappa_lo[out] = lo;
    if (A.iters) A.iters[out] = total;
}

// ---- the group margin: job jg = (point n_scen + scenario) n_grp + group of the wave form -------------------------------------------
static UPR_HDI void upr_bal_margin_grp_job(const upr_ctx& ctx, const upr_grp_args& X, const upr_bal_dims& L, long long jg, double* W) {
    const long long job = jg / X.n_grp;
    upr_bal_margin_job<true>(ctx, X.M, L, job, W, jg, X.group_mask[(int)(jg - job * X.n_grp)], X.mu_base);
}
// the lane form: the group is uniform over the launch's waves (the mask stays in scalar registers)
static UPR_HDI void upr_bal_margin_grp_job1(const upr_grp_args& X, const upr_bal_dims& L, long long job, int grp) {
    upr_bal_margin_job1<true>(X.M, L, job, job * X.n_grp + grp, X.group_mask[grp], X.mu_base);
}

// ---- the largest kappa_hi over the knots of a plan ------------------------------------------------------------------------------------
// kappa_hi [B][nk][inner] (inner = n_scen n_grp) -> worst [B][inner] and the first knot that attains it; +inf counts as largest.
// One output per call, looping over the knots: no atomics.
static UPR_HDI void upr_bal_margin_worst(const double* kappa_hi, int nk, long long inner, long long o, double* worst, int* knot) {
    const long long b = o / inner, e = o - b * inner;
    const double* src = kappa_hi + (size_t)b * nk * inner + e;
    double w = src[0]; int kw = 0;
    for (int k = 1; k < nk; ++k) {
        const double v = src[(size_t)k * inner];
        if (v > w) { w = v; kw = k; }
    }
    worst[o] = w;
    if (knot) knot[o] = kw;
}

#ifndef UPR_HOST_EMU
// one wave per workgroup, jobs dealt round robin (as upr_bal_project_kernel)
__global__ __launch_bounds__(64) void upr_bal_margin_kernel(upr_mar_args M, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_margin_job(ctx, M, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_margin1_kernel(upr_mar_args M, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_margin_job1(M, L, job);
}
// the group margin, a wave per (job, group): njobs counts them
__global__ __launch_bounds__(64) void upr_bal_margin_grp_kernel(upr_grp_args X, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long jg = blockIdx.x; jg < njobs; jg += gridDim.x) upr_bal_margin_grp_job(ctx, X, L, jg, upr_bal_lds);
}
// one-body arrangements: a lane per (point, scenario) job, the group on blockIdx.y; njobs counts the (point, scenario) jobs
__global__ __launch_bounds__(64) void upr_bal_margin1_grp_kernel(upr_grp_args X, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_margin_grp_job1(X, L, job, (int)blockIdx.y);
}
__global__ __launch_bounds__(64) void upr_bal_margin_worst_kernel(const double* kappa_hi, int nk, long long inner, long long nout, double* worst, int* knot) {
    const long long o = (long long)blockIdx.x * 64 + threadIdx.x;
    if (o < nout) upr_bal_margin_worst(kappa_hi, nk, inner, o, worst, knot);
}
#endif
