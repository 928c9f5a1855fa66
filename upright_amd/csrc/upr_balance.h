// upr_balance.h -- batched balance check: the distance from the wrench the balanced bodies need to the contact wrench cone of
// their arrangement, for many (state, inertial-parameter scenario) pairs at once.
//
// What it replaces: the off-line test of upright_robust/scripts/process_sim_runs.py:87-270 (is the required wrench inside the
// cone of upright_robust/src/upright_robust/modelling.py:106-132, compute_cwc_span_form), which runs one trajectory, one time step
// and one parameter set at a time through cvxpy.
//
// The quantity.  g(x, f; theta) is the engine's object-dynamics residual (balancing_constraints.cpp:114-155: per body divided by
// its mass, the whole vector by sqrt(6 nb), end-effector state out of the chain walk) -- the g of the linearisation record.  The
// friction pyramid of contact i is the cone of the generators n_i + mu s_i0, n_i + mu s_i1, n_i - mu s_i0, n_i - mu s_i1
// (RobustContactPoint.S, modelling.py:39-43, in that order; the cone of the five rows of upr_friction_rows_contact); with nf = 1 the
// one generator is n_i.  Forces are f = S z, z >= 0, z of ncol = 4 nc (nf = 3) or nc (nf = 1) entries, and
//
//     rho(x; theta) = min over z >= 0 of | b + A z |_2,      b = g(x, 0; theta)  (6 nb),   A = dg/df(theta) S  (6 nb x ncol).
//
// rho is the distance, in the units of the constraint the controller enforces, from the needed wrench to the contact wrench cone:
// rho = 0 if and only if balancing forces exist.  The force bounds u_lb / u_ub (+-100) are NOT part of it.  The levers and the
// 1 / m in A follow theta (l = r - c(theta), as in upr_object_wrenches), not the handle's own parameters.  rho is unique, z is not.
//
// The kernels.  upr_bal_state_kernel: one lane per point, the value-only walk of upr_kin.h, leaves what b needs and theta does not
// touch (C_we, omega, alpha, a: UPR_BAL_ST doubles).  The projection runs one job per (point, scenario): b from upr_body_residual,
// the columns of A generated on the fly from the contact tables and theta (a column has at most twelve non-zeros: two bodies, six
// rows each; A is never stored), then the Lawson-Hanson active-set iteration.  The passive set never exceeds min(6 nb, ncol)
// columns; its least-squares step is a Cholesky solve of that size followed by one step of refinement on the residual.  All
// arithmetic is fp64.  Two forms:
//   * one-body arrangements (the study's case: 6 rows, 16 columns with four contacts): upr_bal_project1_kernel, a lane per job, the
//     passive system (at most 6 x 6) in registers, no LDS, no scratch (upr_bal_job1, further down);
//   * every other arrangement, up to 8 bodies and 32 contacts (48 rows, 128 columns): upr_bal_project_kernel, one wave per job, jobs
//     dealt round robin to the waves of the grid, candidate columns spread over the lanes, the passive columns (in their sparse
//     form) and their normal matrix in LDS (upr_bal_job).
// The same source compiles as the one-thread host emulation (tests/emu/upr_balance_emu.cpp).
#pragma once
#include "upr_common.h"
#include "upr_kin.h"

// Stopping rule: column j may enter the passive set only while  -a_j' r > UPR_BAL_TOL |a_j| max(|b|, 1),  r = b + A z.
// Resulting accuracy of rho.  At the exit every free column has a_j' r >= -UPR_BAL_TOL |a_j| max(|b|, 1) and the passive ones are
// orthogonal to r to rounding, so rho exceeds the minimum by at most UPR_BAL_TOL max(|b|, 1) sum_j z*_j |a_j| / rho (and by no more
// than rho itself); UPR_BAL_ZERO below does not loosen this: a multiplier it sets to zero leaves the passive set, the remaining
// columns are solved again exactly, and the dropped column is a free column like any other at the next test -- it comes back if it
// still descends by more than the threshold.  What the constants add up to in the tests: |rho - rho_ref| <= 2.3e-15 max(1, |b|)
// over the case table, a_j' r within 3 % of the certificate's bound 10 UPR_BAL_TOL |a_j| max(|b|, 1), and a plan on the friction
// boundary keeps rho below the residual of its own forces to 1e-12.
#define UPR_BAL_TOL 1e-14
// Entering column: the LOWEST column whose normalised descent -a_j' r / |a_j| is within this fraction of the largest.  The
// generators of symmetric contact patterns tie exactly (pink_bottle: columns 0 and 15 at 3.4958662e-09 against 3.4958665e-09), and
// a tie broken by the last bit makes the path -- and the iteration count -- depend on whether a compiler fuses a multiply-add; with
// the band the choice only moves when a score ratio lies within rounding of 1 - UPR_BAL_TIE.  Any column above the threshold is a
// valid entering column of the Lawson-Hanson iteration.
#define UPR_BAL_TIE 1e-3
// A multiplier of the least-squares step at or below this fraction of the largest one is zero to working precision and is
// treated as non-positive: on a facet of the cone the true multiplier of a passive column IS zero (+-5e-16 computed), and its
// sign must not decide whether the column stays.
#define UPR_BAL_ZERO 1e-12
// a passive system whose Cholesky pivot falls below this fraction of the column's own squared norm is taken as rank deficient:
// the column that was just added is put back and barred until the residual changes
#define UPR_BAL_PIVOT_MIN 1e-13
// doubles per point the state kernel leaves: C_we (9, row-major), omega, alpha, a (world frame)
#define UPR_BAL_ST 18
// iteration cap (least-squares solves per job); a job that reaches it reports exactly this count
static inline UPR_HD int upr_bal_iter_cap(int ncol) { return 3 * ncol; }

#include "upr_bal_dims.h"   // (upr_bal_dims, upr_bal_layout: the layout of a job)

struct upr_bal_args {
    const upr_problem* P;
    int n, n_scen;           // points, scenarios: job = point * n_scen + scenario
    const double* st;        // [n][UPR_BAL_ST]
    // parameter block of a job: params + 10 nb * ((pdiv ? (point / pdiv) * n_scen : 0) + scenario) -- pdiv 0: one set of scenarios
    // for all points; 1: per point; N + 1: per instance of a plan
    const double* params;
    int pdiv;
    double eq_scale;         // 1 / sqrt(6 nb)
    double* rho;             // [n][n_scen]
    double* z;               // [n][n_scen][ncol] or NULL
    int* iters;              // [n][n_scen] or NULL
    // friction scale of every scenario, [n_scen] -- the generators of contact i are formed with mu_scale[sc] mu_i (the --mu of
    // process_sim_runs.py as a scenario axis); read by the _mu kernels only.  The _cmu kernels read it as [n_scen][nc]: a scale per
    // scenario and contact (every pair of objects its own friction coefficient, compute_minimum_mu.py:12-30)
    const double* mu_scale = nullptr;
};

// ---- state kernel body: one point ---------------------------------------------------------------------------------------------
template <int NQ>
static UPR_HDI void upr_bal_state_point(const upr_problem* P, const double* x, double* st) {
    upr_ee<double> E;
    upr_ee_kinematics<double, NQ, true>(P, x, -1, E);
    for (int i = 0; i < 9; ++i) st[i] = E.C[i];
    for (int i = 0; i < 3; ++i) { st[9 + i] = E.w[i]; st[12 + i] = E.al[i]; st[15 + i] = E.a[i]; }
}

// ---- column j of A: the blocks on contact_body1 (ba = -1: the end effector, no block) and contact_body2 ----------------------------
// mu: the source of the friction scale, the pyramid of contact i is built on mu.at(i) mu_i (a scale of 1: mu_i * 1.0 is exact, the
// column is bit for bit the one without a scale; nf = 1 generators carry no mu).  Three sources:
//   upr_bal_mu_one  the constant 1 (the calls without a friction scale: folds away);
//   upr_bal_mu_all  one scale for every contact (a scenario's mu_scale; the kappa of the common friction margin);
//   upr_bal_mu_grp  per contact: kap on the contacts of a group (a 32-bit mask, UPR_MAX_CONTACTS = 32), elsewhere the base scale
//                   base[i] of the job's scenario, read from global memory next to contact_mu[i], or 1 without a table.  An empty
//                   mask with a table is the plain per-contact scale of the _cmu kernels.
struct upr_bal_mu_one { UPR_HDI double at(int) const { return 1.0; } };
struct upr_bal_mu_all { double kap; UPR_HDI double at(int) const { return kap; } };
struct upr_bal_mu_grp {
    unsigned mask; double kap; const double* base;
    UPR_HDI double at(int i) const { return ((mask >> i) & 1u) ? kap : (base ? base[i] : 1.0); }
};
template <class MU = upr_bal_mu_one>
static UPR_HDI void upr_bal_column(const upr_problem* P, const double* bp, double scale, int gpc, int j, int* ba, double* va, int* bb, double* vb,
                                   const MU& mu = MU()) {
    const int i = j / gpc, g = j - i * gpc;
    double d[3];
    for (int a = 0; a < 3; ++a) d[a] = P->contact_normal[i][a];
    if (gpc == 4) {
        const double sm = ((g < 2) ? 1.0 : -1.0) * (P->contact_mu[i] * mu.at(i));
        const double* s = P->contact_span[i] + 3 * (g & 1);
        for (int a = 0; a < 3; ++a) d[a] += sm * s[a];
    }
    const int b1 = P->contact_body1[i], b2 = P->contact_body2[i];
    *ba = b1; *bb = b2;
    if (b1 >= 0) {
        const double* q = bp + 10 * b1;
        const double im = 1.0 / q[0], k = -scale * im;
        const double l[3] = {P->contact_r1[i][0] - q[1] * im, P->contact_r1[i][1] - q[2] * im, P->contact_r1[i][2] - q[3] * im};
        va[0] = k * d[0]; va[1] = k * d[1]; va[2] = k * d[2];
        va[3] = k * (l[1] * d[2] - l[2] * d[1]); va[4] = k * (l[2] * d[0] - l[0] * d[2]); va[5] = k * (l[0] * d[1] - l[1] * d[0]);
    } else {
        for (int a = 0; a < 6; ++a) va[a] = 0.0;
    }
    {
        const double* q = bp + 10 * b2;
        const double im = 1.0 / q[0], k = scale * im;
        const double l[3] = {P->contact_r2[i][0] - q[1] * im, P->contact_r2[i][1] - q[2] * im, P->contact_r2[i][2] - q[3] * im};
        vb[0] = k * d[0]; vb[1] = k * d[1]; vb[2] = k * d[2];
        vb[3] = k * (l[1] * d[2] - l[2] * d[1]); vb[4] = k * (l[2] * d[0] - l[0] * d[2]); vb[5] = k * (l[0] * d[1] - l[1] * d[0]);
    }
}

// ---- reductions over the lanes of the job's wave (the emulation has one lane) ------------------------------------------------------
// largest value and its column; ties go to the lower column, j < 0: no candidate
static UPR_HDI void upr_bal_argmax(const upr_ctx& ctx, double* v, int* j) {
#ifndef UPR_HOST_EMU
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(*v, off);
        const int oj = __shfl_xor(*j, off);
        if (oj >= 0 && (*j < 0 || ov > *v || (ov == *v && oj < *j))) { *v = ov; *j = oj; }
    }
#endif
    (void)ctx;
}

// lowest non-negative column over the lanes (j < 0: none)
static UPR_HDI void upr_bal_minidx(const upr_ctx& ctx, int* j) {
#ifndef UPR_HOST_EMU
    for (int off = 32; off > 0; off >>= 1) {
        const int oj = __shfl_xor(*j, off);
        if (oj >= 0 && (*j < 0 || oj < *j)) *j = oj;
    }
#endif
    (void)ctx;
}

// passive slot s (sparse: bodies pb[2 s], pb[2 s + 1], values pc[12 s ..]) times a dense vector of m rows
static UPR_HDI double upr_bal_dot_dense(const double* pc, const int* pb, int s, const double* v) {
    double acc = 0.0;
    const int ba = pb[2 * s], bb = pb[2 * s + 1];
    if (ba >= 0) for (int c = 0; c < 6; ++c) acc += pc[12 * s + c] * v[6 * ba + c];
    for (int c = 0; c < 6; ++c) acc += pc[12 * s + 6 + c] * v[6 * bb + c];
    return acc;
}
// two passive slots
static UPR_HDI double upr_bal_dot_slots(const double* pc, const int* pb, int s, int t) {
    double acc = 0.0;
    for (int x = 0; x < 2; ++x) {
        const int bx = pb[2 * s + x];
        if (bx < 0) continue;
        for (int y = 0; y < 2; ++y) {
            if (pb[2 * t + y] != bx) continue;
            for (int c = 0; c < 6; ++c) acc += pc[12 * s + 6 * x + c] * pc[12 * t + 6 * y + c];
        }
    }
    return acc;
}
// r = b + sum over the passive slots of coef[t] * column t   (rows over the lanes)
static UPR_HDI void upr_bal_residual(const upr_ctx& ctx, const upr_bal_dims& L, int np, const double* b, const double* pc, const int* pb,
                                     const double* coef, double* r) {
    UPR_FOR(e, L.m) {
        const int body = e / 6, c = e - 6 * body;
        double acc = b[e];
        for (int t = 0; t < np; ++t) {
            if (pb[2 * t] == body) acc += coef[t] * pc[12 * t + c];
            if (pb[2 * t + 1] == body) acc += coef[t] * pc[12 * t + 6 + c];
        }
        r[e] = acc;
    }
    UPR_WSYNC();
}
// G (np x np in the mp-strided store, lower triangle) -> its Cholesky factor in place; false: a pivot below UPR_BAL_PIVOT_MIN dg[k]
static UPR_HDI bool upr_bal_factor(const upr_ctx& ctx, int mp, int np, double* G, const double* dg) {
    for (int k = 0; k < np; ++k) {
        const double d = G[k * mp + k];
        if (!(d > UPR_BAL_PIVOT_MIN * dg[k])) return false;   // (uniform: every lane reads the same entry)
        const double lk = sqrt(d);
        UPR_WSYNC();
        for (int i = k + ctx.tid; i < np; i += ctx.nt) G[i * mp + k] = (i == k) ? lk : G[i * mp + k] / lk;
        UPR_WSYNC();
        const int cnt = np - k - 1;
        for (int e = ctx.tid; e < cnt * cnt; e += ctx.nt) {
            const int i = k + 1 + e / cnt, j = k + 1 + e % cnt;
            if (j <= i) G[i * mp + j] -= G[i * mp + k] * G[j * mp + k];
        }
        UPR_WSYNC();
    }
    return true;
}
// y <- (L L')^-1 y
static UPR_HDI void upr_bal_solve(const upr_ctx& ctx, int mp, int np, const double* G, double* y) {
    for (int k = 0; k < np; ++k) {
        const double yk = y[k] / G[k * mp + k];
        UPR_WSYNC();
        if (ctx.tid == 0) y[k] = yk;
        for (int i = k + 1 + ctx.tid; i < np; i += ctx.nt) y[i] -= G[i * mp + k] * yk;
        UPR_WSYNC();
    }
    for (int k = np - 1; k >= 0; --k) {
        const double xk = y[k] / G[k * mp + k];
        UPR_WSYNC();
        if (ctx.tid == 0) y[k] = xk;
        for (int i = ctx.tid; i < k; i += ctx.nt) y[i] -= G[k * mp + i] * xk;
        UPR_WSYNC();
    }
}

// ---- the projection of one job: the lanes of ctx work on it together, W: L.total doubles of workspace (LDS) -------------------------
// b (W + L.o_b) is written by the caller, not yet synchronised; mu: the friction scale of the generators (upr_bal_column).  A cold
// start: nothing of an earlier projection in W is read.  Leaves r = b + A z (W + L.o_r), the passive slots (zp, pidx, their columns; *np_out of them),
// the column states and in G the Cholesky factor of the last passive system (its leading block is the factor of the slots that
// are left unless the cap was reached); returns rho on every lane, *bnorm_out = |b|, *iters_out the least-squares solves (the cap if it was reached).
template <class MU>
static UPR_HDI double upr_bal_project(const upr_ctx& ctx, const upr_problem* P, const upr_bal_dims& L, const double* bp, double eq_scale,
                                      const MU& mu, double* W, int* np_out, int* iters_out, double* bnorm_out) {
    const int m = L.m, ncol = L.ncol, mp = L.mp;
    double *b = W + L.o_b, *r = W + L.o_r, *zp = W + L.o_zp, *s = W + L.o_s, *y = W + L.o_y, *dg = W + L.o_dg, *pc = W + L.o_pcol, *G = W + L.o_G;
    int* pidx = (int*)(W + L.o_int); int* pb = pidx + mp; int* flag = pb + 2 * mp;
    UPR_FOR(j, ncol) flag[j] = 0;
    UPR_WSYNC();
    double bb2 = 0.0;
    for (int e = 0; e < m; ++e) bb2 += b[e] * b[e];
    const double bnorm = sqrt(bb2), thr = UPR_BAL_TOL * (bnorm > 1.0 ? bnorm : 1.0);
    const int cap = upr_bal_iter_cap(ncol);
    int np = 0, iters = 0;
    bool capped = false;

    while (true) {
        upr_bal_residual(ctx, L, np, b, pc, pb, zp, r);
        if (np == mp) break;
        // the free column with the largest normalised descent -a_j' r / |a_j| above the threshold
        double best = 0.0; int bj = -1;
        for (int pass = 0; pass < 2; ++pass) {   // 0: the best score; 1: the lowest column within UPR_BAL_TIE of it
            const double cut = best * (1.0 - UPR_BAL_TIE);
            int lo = -1;
            UPR_FOR(j, ncol) {
                if (flag[j] != 0) continue;
                int ba, bq; double va[6], vb[6];
                upr_bal_column(P, bp, eq_scale, L.gpc, j, &ba, va, &bq, vb, mu);
                double w = 0.0, n2 = 0.0;
                for (int c = 0; c < 6; ++c) { w -= vb[c] * r[6 * bq + c]; n2 += vb[c] * vb[c]; }
                if (ba >= 0) for (int c = 0; c < 6; ++c) { w -= va[c] * r[6 * ba + c]; n2 += va[c] * va[c]; if (ba == bq) n2 += 2.0 * va[c] * vb[c]; }
                const double nrm = sqrt(n2);
                if (!(w > thr * nrm)) continue;
                const double score = w / nrm;
                if (pass == 0) { if (bj < 0 || score > best) { best = score; bj = j; } }
                else if (score >= cut && lo < 0) lo = j;
            }
            if (pass == 0) { upr_bal_argmax(ctx, &best, &bj); if (bj < 0) break; }
            else { upr_bal_minidx(ctx, &lo); bj = lo; }
        }
        if (bj < 0) break;
        if (iters >= cap) { capped = true; break; }
        UPR_WSYNC();
        if (ctx.tid == 0) {
            int ba, bq; double va[6], vb[6];
            upr_bal_column(P, bp, eq_scale, L.gpc, bj, &ba, va, &bq, vb, mu);
            for (int c = 0; c < 6; ++c) { pc[12 * np + c] = va[c]; pc[12 * np + 6 + c] = vb[c]; }
            pb[2 * np] = ba; pb[2 * np + 1] = bq; pidx[np] = bj; zp[np] = 0.0; flag[bj] = 1;
        }
        ++np;
        UPR_WSYNC();
        bool fresh = true, rejected = false;
        while (true) {
            if (iters >= cap) { capped = true; break; }
            ++iters;
            // normal equations of the passive columns: G s = -A_P' b
            for (int e = ctx.tid; e < np * np; e += ctx.nt) {
                const int i = e / np, j = e - i * np;
                if (j <= i) G[i * mp + j] = upr_bal_dot_slots(pc, pb, i, j);
            }
            UPR_FOR(i, np) s[i] = -upr_bal_dot_dense(pc, pb, i, b);
            UPR_WSYNC();
            UPR_FOR(i, np) dg[i] = G[i * mp + i];
            UPR_WSYNC();
            const bool ok = upr_bal_factor(ctx, mp, np, G, dg);
            if (ok) {
                upr_bal_solve(ctx, mp, np, G, s);
                // one step of refinement on the residual of that solution
                upr_bal_residual(ctx, L, np, b, pc, pb, s, r);
                UPR_FOR(i, np) y[i] = -upr_bal_dot_dense(pc, pb, i, r);
                UPR_WSYNC();
                upr_bal_solve(ctx, mp, np, G, y);
                UPR_FOR(i, np) s[i] += y[i];
                UPR_WSYNC();
            }
            double sfl = 0.0;   // multipliers at or below this are zero to working precision
            if (ok) { for (int t = 0; t < np; ++t) sfl = fabs(s[t]) > sfl ? fabs(s[t]) : sfl; sfl *= UPR_BAL_ZERO; }
            if (!ok || (fresh && !(s[np - 1] > sfl))) {
                // the column that just entered is dependent on the others to working precision: out again, barred until r changes
                UPR_WSYNC();
                if (ctx.tid == 0) flag[pidx[np - 1]] = 2;
                --np;
                rejected = true;
                UPR_WSYNC();
                break;
            }
            fresh = false;
            bool allpos = true;
            double alpha = 2.0; int tmin = -1;
            for (int t = 0; t < np; ++t) {
                if (s[t] > sfl) continue;
                allpos = false;
                const double a0 = zp[t] / (zp[t] - s[t]), a = (a0 >= 0.0 && a0 <= 1.0) ? a0 : 1.0;   // (0 < s <= sfl: the whole step)
                if (tmin < 0 || a < alpha) { alpha = a; tmin = t; }
            }
            UPR_WSYNC();
            if (allpos) {
                UPR_FOR(t, np) zp[t] = s[t];
                UPR_WSYNC();
                break;
            }
            // step to the boundary of the orthant and drop what arrived there
            if (ctx.tid == 0) {
                int q = 0;
                for (int t = 0; t < np; ++t) {
                    const double zt = zp[t] + alpha * (s[t] - zp[t]);
                    const bool drop = (t == tmin) || (s[t] <= sfl && !(zt > sfl));
                    if (drop) { flag[pidx[t]] = 0; continue; }
                    if (q != t) {
                        for (int c = 0; c < 12; ++c) pc[12 * q + c] = pc[12 * t + c];
                        pb[2 * q] = pb[2 * t]; pb[2 * q + 1] = pb[2 * t + 1]; pidx[q] = pidx[t];
                    }
                    zp[q] = zt > 0.0 ? zt : 0.0;
                    ++q;
                }
                y[0] = (double)q;
            }
            UPR_WSYNC();
            np = (int)y[0];
            UPR_WSYNC();
            if (np == 0) break;
        }
        if (capped) break;
        if (!rejected) {   // the residual moves: barred columns may be looked at again
            UPR_FOR(j, ncol) if (flag[j] == 2) flag[j] = 0;
            UPR_WSYNC();
        }
    }
    if (capped) { upr_bal_residual(ctx, L, np, b, pc, pb, zp, r); iters = cap; }
    double rr = 0.0;
    for (int e = 0; e < m; ++e) rr += r[e] * r[e];
    *np_out = np; *iters_out = iters; *bnorm_out = bnorm;
    return sqrt(rr);
}

// b = g(x, 0; theta) of a job into W + L.o_b: the residual of every body without contact wrench, scaled as the linearisation scales
// it (bodies over the lanes; the caller synchronises -- upr_bal_project does)
static UPR_HDI void upr_bal_rhs(const upr_ctx& ctx, const upr_problem* P, const double* st, const double* bp, double eq_scale, double* b) {
    UPR_FOR(k, P->nb) {
        upr_ee<double> E;
        for (int i = 0; i < 9; ++i) E.C[i] = st[i];
        for (int i = 0; i < 3; ++i) { E.w[i] = st[9 + i]; E.al[i] = st[12 + i]; E.a[i] = st[15 + i]; E.p[i] = 0.0; E.v[i] = 0.0; }
        const double zero3[3] = {0.0, 0.0, 0.0};
        double gb[6];
        upr_body_residual<double>(E, bp + 10 * k, P->gravity, zero3, zero3, gb);
        for (int c = 0; c < 6; ++c) b[6 * k + c] = eq_scale * gb[c];
    }
}
// the multipliers of the passive slots, scattered to the ncol entries of zo (columns over the lanes)
static UPR_HDI void upr_bal_put_z(const upr_ctx& ctx, const upr_bal_dims& L, const double* W, int np, double* zo) {
    const double* zp = W + L.o_zp;
    const int* pidx = (const int*)(W + L.o_int); const int* flag = pidx + 3 * L.mp;
    UPR_FOR(j, L.ncol) {
        double v = 0.0;
        if (flag[j] == 1) for (int t = 0; t < np; ++t) if (pidx[t] == j) v = zp[t];
        zo[j] = v;
    }
}

// ---- one (point, scenario) job ------------------------------------------------------------------------------------------------------
// MU: 0 the scale is the constant 1 and folds away (the kernels of the calls without a friction scale keep the code they had before
// there was one); 1 the friction scale of the job's scenario is read from A.mu_scale[sc]; 2 the scale of contact i is read from
// A.mu_scale[sc nc + i]
template <int MU> struct upr_bal_src;
template <> struct upr_bal_src<0> { typedef upr_bal_mu_one T; static UPR_HDI T of(const upr_bal_args&, int, int) { return T(); } };
template <> struct upr_bal_src<1> { typedef upr_bal_mu_all T; static UPR_HDI T of(const upr_bal_args& A, int sc, int) { return T{A.mu_scale[sc]}; } };
template <> struct upr_bal_src<2> {
    typedef upr_bal_mu_grp T;
    static UPR_HDI T of(const upr_bal_args& A, int sc, int nc) { return T{0u, 0.0, A.mu_scale + (size_t)sc * nc}; }
};
template <int MU = 0>
static UPR_HDI void upr_bal_job(const upr_ctx& ctx, const upr_bal_args& A, const upr_bal_dims& L, long long job, double* W) {
    const upr_problem* P = A.P;
    const long long pt = job / A.n_scen;
    const int sc = (int)(job - pt * A.n_scen);
    const double* bp = A.params + (size_t)10 * P->nb * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const typename upr_bal_src<MU>::T mu = upr_bal_src<MU>::of(A, sc, P->nc);
    UPR_WSYNC();   // (the previous job of this wave is done with the workspace)
    upr_bal_rhs(ctx, P, A.st + (size_t)pt * UPR_BAL_ST, bp, A.eq_scale, W + L.o_b);
    int np, iters; double bnorm;
    const double rho = upr_bal_project(ctx, P, L, bp, A.eq_scale, mu, W, &np, &iters, &bnorm);
    if (ctx.tid == 0) {
        A.rho[job] = rho;
        if (A.iters) A.iters[job] = iters;
    }
    if (A.z) upr_bal_put_z(ctx, L, W, np, A.z + (size_t)job * L.ncol);
}

// ---- one-body arrangements: a lane per job ------------------------------------------------------------------------------------------
// The study's own case (6 rows; 16 columns for four contacts with friction): the same iteration as upr_bal_job with the passive
// system -- at most six columns, kept dense: a column's blocks land on the one body -- in registers.  Every array below is indexed
// by compile-time constants after unrolling (a slot that is not in use is an identity row of the normal matrix), so nothing lives
// in scratch; the sets of passive and barred columns are bit masks (up to 128 columns: 32 contacts).
#define UPR_BAL1_MP 6
static UPR_HDI bool upr_bal_bit(unsigned long long lo, unsigned long long hi, int j) { return (((j < 64) ? lo : hi) >> (j & 63)) & 1ull; }
template <class MU>
static UPR_HDI void upr_bal_column1(const upr_problem* P, const double* bp, double scale, int gpc, int j, double* v, const MU& mu) {
    int ba, bb; double va[6], vb[6];
    upr_bal_column(P, bp, scale, gpc, j, &ba, va, &bb, vb, mu);
    for (int c = 0; c < 6; ++c) v[c] = (ba >= 0) ? va[c] + vb[c] : vb[c];
}
// The projection of one job on one lane, cold: b the right-hand side, thr = UPR_BAL_TOL max(|b|, 1), mu the friction scale of the
// generators.  Leaves r = b + A z, the passive slots (pidx, zp, their columns pc; np of them) and in G the Cholesky factor of the
// last passive system (its leading np x np block is the factor of the np slots unless the cap was reached); returns the
// least-squares solves (the cap if reached).
template <class MU>
static UPR_HDI int upr_bal_project1(const upr_problem* P, const upr_bal_dims& L, const double* bp, double eq_scale, const MU& mu, const double (&b)[6],
                                    double thr, double (&r)[6], double (&zp)[UPR_BAL1_MP], int (&pidx)[UPR_BAL1_MP], int& np,
                                    double (&pc)[UPR_BAL1_MP][6], double (&G)[UPR_BAL1_MP][UPR_BAL1_MP]) {
    constexpr int MP = UPR_BAL1_MP;
    const int ncol = L.ncol, mp = L.mp;
    double s[MP], y[MP], dg[MP];
#pragma unroll
    for (int t = 0; t < MP; ++t) { zp[t] = 0.0; s[t] = 0.0; pidx[t] = 0; for (int c = 0; c < 6; ++c) pc[t][c] = 0.0; }
    const int cap = upr_bal_iter_cap(ncol);
    unsigned long long pas0 = 0, pas1 = 0, bar0 = 0, bar1 = 0;
    int iters = 0;
    bool capped = false;
    np = 0;

    while (true) {
        for (int c = 0; c < 6; ++c) r[c] = b[c];
#pragma unroll
        for (int t = 0; t < MP; ++t) if (t < np) for (int c = 0; c < 6; ++c) r[c] += zp[t] * pc[t][c];
        if (np == mp) break;
        double best = 0.0; int bj = -1;
        for (int pass = 0; pass < 2; ++pass) {   // 0: the best score; 1: the lowest column within UPR_BAL_TIE of it
            const double cut = best * (1.0 - UPR_BAL_TIE);
            int lo = -1;
            for (int j = 0; j < ncol; ++j) {
                if (upr_bal_bit(pas0 | bar0, pas1 | bar1, j)) continue;
                double v[6];
                upr_bal_column1(P, bp, eq_scale, L.gpc, j, v, mu);
                double w = 0.0, n2 = 0.0;
                for (int c = 0; c < 6; ++c) { w -= v[c] * r[c]; n2 += v[c] * v[c]; }
                const double nrm = sqrt(n2);
                if (!(w > thr * nrm)) continue;
                const double score = w / nrm;
                if (pass == 0) { if (bj < 0 || score > best) { best = score; bj = j; } }
                else if (score >= cut && lo < 0) lo = j;
            }
            if (pass == 0) { if (bj < 0) break; }
            else bj = lo;
        }
        if (bj < 0) break;
        if (iters >= cap) { capped = true; break; }
        {
            double v[6];
            upr_bal_column1(P, bp, eq_scale, L.gpc, bj, v, mu);
#pragma unroll
            for (int t = 0; t < MP; ++t) if (t == np) { for (int c = 0; c < 6; ++c) pc[t][c] = v[c]; pidx[t] = bj; zp[t] = 0.0; }
            if (bj < 64) pas0 |= 1ull << bj; else pas1 |= 1ull << (bj - 64);
            ++np;
        }
        bool fresh = true, rejected = false;
        while (true) {
            if (iters >= cap) { capped = true; break; }
            ++iters;
            // normal equations of the passive columns, identity in the unused slots
#pragma unroll
            for (int i = 0; i < MP; ++i) {
#pragma unroll
                for (int j = 0; j <= i; ++j) {
                    double acc = 0.0;
                    for (int c = 0; c < 6; ++c) acc += pc[i][c] * pc[j][c];
                    G[i][j] = (i < np) ? acc : (i == j ? 1.0 : 0.0);
                }
                double acc = 0.0;
                for (int c = 0; c < 6; ++c) acc += pc[i][c] * b[c];
                s[i] = (i < np) ? -acc : 0.0;
                dg[i] = G[i][i];
            }
            bool ok = true;
#pragma unroll
            for (int k = 0; k < MP; ++k) {
                double d = G[k][k];
                if (!(d > UPR_BAL_PIVOT_MIN * dg[k])) { ok = false; d = 1.0; }
                const double lk = sqrt(d);
                G[k][k] = lk;
#pragma unroll
                for (int i = k + 1; i < MP; ++i) G[i][k] = G[i][k] / lk;
#pragma unroll
                for (int i = k + 1; i < MP; ++i)
#pragma unroll
                    for (int j = k + 1; j <= i; ++j) G[i][j] -= G[i][k] * G[j][k];
            }
            if (ok) {
#pragma unroll
                for (int pass = 0; pass < 2; ++pass) {
                    // pass 0 solves for s; pass 1 refines it on the residual of that solution
                    if (pass == 1) {
                        double rs[6];
                        for (int c = 0; c < 6; ++c) rs[c] = b[c];
#pragma unroll
                        for (int t = 0; t < MP; ++t) if (t < np) for (int c = 0; c < 6; ++c) rs[c] += s[t] * pc[t][c];
#pragma unroll
                        for (int i = 0; i < MP; ++i) {
                            double acc = 0.0;
                            for (int c = 0; c < 6; ++c) acc += pc[i][c] * rs[c];
                            y[i] = (i < np) ? -acc : 0.0;
                        }
                    } else {
#pragma unroll
                        for (int i = 0; i < MP; ++i) y[i] = s[i];
                    }
#pragma unroll
                    for (int k = 0; k < MP; ++k) {
                        y[k] = y[k] / G[k][k];
#pragma unroll
                        for (int i = k + 1; i < MP; ++i) y[i] -= G[i][k] * y[k];
                    }
#pragma unroll
                    for (int k = MP - 1; k >= 0; --k) {
                        y[k] = y[k] / G[k][k];
#pragma unroll
                        for (int i = 0; i < k; ++i) y[i] -= G[k][i] * y[k];
                    }
#pragma unroll
                    for (int i = 0; i < MP; ++i) s[i] = (pass == 1) ? s[i] + y[i] : y[i];
                }
            }
            double snew = 0.0; int jnew = 0;
#pragma unroll
            for (int t = 0; t < MP; ++t) if (t == np - 1) { snew = s[t]; jnew = pidx[t]; }
            double sfl = 0.0;   // multipliers at or below this are zero to working precision
#pragma unroll
            for (int t = 0; t < MP; ++t) sfl = (t < np && fabs(s[t]) > sfl) ? fabs(s[t]) : sfl;
            sfl *= UPR_BAL_ZERO;
            if (!ok || (fresh && !(snew > sfl))) {
                if (jnew < 64) { pas0 &= ~(1ull << jnew); bar0 |= 1ull << jnew; } else { pas1 &= ~(1ull << (jnew - 64)); bar1 |= 1ull << (jnew - 64); }
                --np;
                rejected = true;
                break;
            }
            fresh = false;
            bool allpos = true;
            double alpha = 2.0; int tmin = -1;
#pragma unroll
            for (int t = 0; t < MP; ++t) {
                if (t >= np || s[t] > sfl) continue;
                allpos = false;
                const double a0 = zp[t] / (zp[t] - s[t]), a = (a0 >= 0.0 && a0 <= 1.0) ? a0 : 1.0;   // (0 < s <= sfl: the whole step)
                if (tmin < 0 || a < alpha) { alpha = a; tmin = t; }
            }
            if (allpos) {
#pragma unroll
                for (int t = 0; t < MP; ++t) if (t < np) zp[t] = s[t];
                break;
            }
            bool drop[MP];
#pragma unroll
            for (int t = 0; t < MP; ++t) {
                const double zt = zp[t] + alpha * (s[t] - zp[t]);
                drop[t] = (t < np) && ((t == tmin) || (s[t] <= sfl && !(zt > sfl)));
                if (t < np) zp[t] = zt > 0.0 ? zt : 0.0;
            }
#pragma unroll
            for (int t = MP - 1; t >= 0; --t) {
                if (!drop[t]) continue;
                const int jd = pidx[t];
                if (jd < 64) pas0 &= ~(1ull << jd); else pas1 &= ~(1ull << (jd - 64));
#pragma unroll
                for (int u = t; u < MP - 1; ++u) { for (int c = 0; c < 6; ++c) pc[u][c] = pc[u + 1][c]; pidx[u] = pidx[u + 1]; zp[u] = zp[u + 1]; }
                --np;
            }
            if (np == 0) break;
        }
        if (capped) break;
        if (!rejected) { bar0 = 0; bar1 = 0; }
    }
    if (capped) {
        for (int c = 0; c < 6; ++c) r[c] = b[c];
#pragma unroll
        for (int t = 0; t < MP; ++t) if (t < np) for (int c = 0; c < 6; ++c) r[c] += zp[t] * pc[t][c];
        iters = cap;
    }
    return iters;
}
// b = g(x, 0; theta) of a one-body job
static UPR_HDI void upr_bal_rhs1(const upr_problem* P, const double* st, const double* bp, double eq_scale, double (&b)[6]) {
    upr_ee<double> E;
    for (int i = 0; i < 9; ++i) E.C[i] = st[i];
    for (int i = 0; i < 3; ++i) { E.w[i] = st[9 + i]; E.al[i] = st[12 + i]; E.a[i] = st[15 + i]; E.p[i] = 0.0; E.v[i] = 0.0; }
    const double zero3[3] = {0.0, 0.0, 0.0};
    double gb[6];
    upr_body_residual<double>(E, bp, P->gravity, zero3, zero3, gb);
    for (int c = 0; c < 6; ++c) b[c] = eq_scale * gb[c];
}
static UPR_HDI void upr_bal_put_z1(int ncol, const double (&zp)[UPR_BAL1_MP], const int (&pidx)[UPR_BAL1_MP], int np, double* zo) {
    for (int j = 0; j < ncol; ++j) zo[j] = 0.0;
#pragma unroll
    for (int t = 0; t < UPR_BAL1_MP; ++t) if (t < np) zo[pidx[t]] = zp[t];
}
template <int MU = 0>
static UPR_HDI void upr_bal_job1(const upr_bal_args& A, const upr_bal_dims& L, long long job) {
    const upr_problem* P = A.P;
    const long long pt = job / A.n_scen;
    const int sc = (int)(job - pt * A.n_scen);
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const typename upr_bal_src<MU>::T mu = upr_bal_src<MU>::of(A, sc, P->nc);
    double b[6], r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
    int pidx[UPR_BAL1_MP], np;
    upr_bal_rhs1(P, A.st + (size_t)pt * UPR_BAL_ST, bp, A.eq_scale, b);
    double bb2 = 0.0;
    for (int c = 0; c < 6; ++c) bb2 += b[c] * b[c];
    const double bnorm = sqrt(bb2), thr = UPR_BAL_TOL * (bnorm > 1.0 ? bnorm : 1.0);
    const int iters = upr_bal_project1(P, L, bp, A.eq_scale, mu, b, thr, r, zp, pidx, np, pc, G);
    double rr = 0.0;
    for (int c = 0; c < 6; ++c) rr += r[c] * r[c];
    A.rho[job] = sqrt(rr);
    if (A.iters) A.iters[job] = iters;
    if (A.z) upr_bal_put_z1(L.ncol, zp, pidx, np, A.z + (size_t)job * L.ncol);
}

// which of the two forms a problem runs: one body -> a lane per job (upr_bal_job1), else a wave per job (upr_bal_job)
static inline UPR_HD bool upr_bal_lane_form(int nb) { return nb == 1; }

#ifndef UPR_HOST_EMU
template <int NQ>
__global__ void upr_bal_state_kernel(const upr_problem* P, int n, const double* x, double* st) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    upr_bal_state_point<NQ>(P, x + (size_t)i * 3 * NQ, st + (size_t)i * UPR_BAL_ST);
}
// one wave per workgroup; the job index is uniform over the wave, so every lane takes every branch of upr_bal_job together
__global__ __launch_bounds__(64) void upr_bal_project_kernel(upr_bal_args A, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_job(ctx, A, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_project1_kernel(upr_bal_args A, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_job1(A, L, job);
}
// the two with a friction scale per scenario (A.mu_scale)
__global__ __launch_bounds__(64) void upr_bal_project_mu_kernel(upr_bal_args A, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_job<1>(ctx, A, L, job, upr_bal_lds);
}
__global__ __launch_bounds__(64) void upr_bal_project1_mu_kernel(upr_bal_args A, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_job1<1>(A, L, job);
}
// the two with a friction scale per scenario and contact (A.mu_scale as [n_scen][nc])
__global__ __launch_bounds__(64) void upr_bal_project_cmu_kernel(upr_bal_args A, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_job<2>(ctx, A, L, job, upr_bal_lds);
}
__global__ __launch_bounds__(64) void upr_bal_project1_cmu_kernel(upr_bal_args A, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_job1<2>(A, L, job);
}
#endif
