// upr_retime_sub.h -- retiming with substeps: the fastest time law on the speed lattice of upr_retime.h whose every segment is balanced at
// R - 1 interior points of the path as well as at its two knots.
//
// The quantity.  Lattice, levels, edges, d, dt, `common`, start / end, the programme and every output are upr_retime.h's.  The new input
// is `substeps` = R, 1 <= R <= 16.
//
// Substep points.  Segment i gets R + 1 path points at tau_r = (double)r h / (double)R, r = 0 .. R.  r = 0 and r = R are knots i and
// i + 1: their records are the plan's, copied verbatim (the knots do not go through the interpolant: h v / h is not v bit for bit).  For
// 0 < r < R the record is (Q, Q', Q'') of upr_replay.h's quintic Hermite interpolant at tau_r, upr_rpl_state(P, x_i, x_{i+1}, 1.0, 1.0, h,
// tau_r, out) as it stands: with s0 = s1 = 1 it gives d = 0, s = 1, tau = t'.  These records do not depend on the edge.  They form a
// "fine plan" xf [B][N R + 1][3 nq]; the point of (b, i, r) is b (N R + 1) + i R + r, so interior knots are shared by two segments.
//
// Speeds.  Constant sddot makes s^2 linear in tau.  On edge (i, m -> m'): s_0 = s_m and s_R = s_m', the lattice doubles themselves; for
// 0 < r < R, s_r = sqrt((((double)(R - r)) (s_m s_m) + ((double)r) (s_m' s_m')) / (double)R) (upr_sub_speed, shared by emulation and
// device); d = upr_ret_accel(s_m, s_m', h) for all r.
//
// State.  The state at point r is (Q, s_r Q', s_r^2 Q'' + d Q'); on the state kernel's record it is upr_pac_transform(st_r, vee_r, s_r, d).
//
// Admissibility.  Edge (i, m -> m') is admissible in scenario c iff the edge exists (s_m + s_m' > 0); with `boxes`,
// upr_ret_in_box(P, xf_r, s_r, d) holds at every r = 0 .. R; and every one of the R + 1 states is accepted by the family's rule, unchanged
// (rho of the cold projection <= UPR_BAL_FEAS max(|b|, 1)).
//
// Order of evaluation.  Fixed, because iters is compared bit for bit: existence; the boxes at r = 0 and r = R with the plain job's
// short-circuit; the boxes at r = 1 .. R - 1 ascending; the projections -- departing (r = 0), arriving (r = R), then the interior ones
// r = 1 .. R - 1 ascending -- stopping at the first rejection.  A mask row costs at most M (R + 1) projections.  With R = 1 the
// evaluations are those of upr_bal_retime_job / upr_bal_retime_job1, one for one.
//
// What is claimed.  The law is balanced at the knots and at the R - 1 interior path points of every segment.  NOTHING is claimed between
// those points; the replay of upr_replay.h on the returned law is the caller's check.  Jerk is not judged (upr_retime.h).
//
// The kernels.  upr_bal_refine_kernel: a lane per fine point, a knot is copied, an interior point goes through upr_rpl_state straight
// into xf; a bounded grid with a stride loop, no atomics, no LDS.  The state kernel upr_bal_state_vee_kernel runs on the B (N R + 1) fine
// points as it is.  Jobs and their decoding (upr_ret_decode) are upr_retime.h's, the point index comes from the fine layout; a job writes
// ONE uint32 and optionally iters; no atomics, no waits on other waves, every loop bounded by M and R.  One flattened loop walks
// (m', point), so a kernel holds ONE copy of the projection's code; s_r and the fine record are read at every evaluation, not held.  The
// path kernel of upr_retime.h serves this quantity as it is.
#pragma once
#include "upr_replay.h"

#define UPR_SUB_MAX 16

struct upr_ret_sub_args {
    upr_ret_args T;          // as the retiming's, on the fine plan: xs is xf, nx is 3 nq, nk stays N + 1; J.st, vee [B (N R + 1)]; J.pdiv N R + 1 or 0
    int R;                   // substeps
};
struct upr_sub_refine_args {
    const upr_problem* P;
    const double* xs;        // [B][nk][nx]: the plan
    int nk, nx, R;
    double h;
    double* xf;              // [B][N R + 1][3 nq]
};

// the speed at point r of an edge between the speeds sm and sp: s^2 is linear in the path time
static UPR_HDI double upr_sub_speed(double sm, double sp, int r, int R) {
    if (r == 0) return sm;
    if (r == R) return sp;
    return sqrt((((double)(R - r)) * (sm * sm) + ((double)r) * (sp * sp)) / (double)R);
}
// fine point p of the fine plan: a knot is the plan's record, an interior point the interpolant's
static UPR_HDI void upr_bal_refine(const upr_sub_refine_args& A, long long p) {
    const int N = A.nk - 1, nq = A.P->nq;
    const long long per = (long long)N * A.R + 1, b = p / per;
    const int j = (int)(p - b * per), i = j / A.R, r = j - i * A.R;
    const double* x0 = A.xs + ((size_t)b * A.nk + i) * A.nx;
    double* out = A.xf + (size_t)p * 3 * nq;
    if (r == 0) {
        for (int c = 0; c < 3 * nq; ++c) out[c] = x0[c];
        return;
    }
    upr_rpl_state(A.P, x0, x0 + A.nx, 1.0, 1.0, A.h, (double)r * A.h / (double)A.R, out);
}

// where the flattened loop of a job stands: the edge m -> mp and the evaluation k = 0 .. R of it
struct upr_sub_walk {
    int mp, k;
    double d;
};
// the path point of evaluation k: the departing knot, the arriving knot, then the interior points ascending
static UPR_HDI int upr_sub_point(int k, int R) { return k == 0 ? 0 : (k == 1 ? R : k - 1); }
// job (knot pt of the plan) -> the fine point of its departing knot
static UPR_HDI long long upr_sub_first(const upr_ret_sub_args& S, long long pt) {
    const long long b = pt / S.T.nk;
    return b * ((long long)(S.T.nk - 1) * S.R + 1) + (pt - b * S.T.nk) * S.R;
}
// before the first evaluation of an edge: its d; false: the edge does not exist or a box cuts it
static UPR_HDI bool upr_sub_edge(const upr_ret_sub_args& S, long long fp, double sm, double sp, double& d) {
    const upr_ret_args& T = S.T;
    d = upr_ret_accel(sm, sp, T.h);
    bool go = sm + sp > 0.0;
    if (go && T.boxes) {
        go = upr_ret_in_box(T.J.P, T.xs + (size_t)fp * T.nx, sm, d) && upr_ret_in_box(T.J.P, T.xs + (size_t)(fp + S.R) * T.nx, sp, d);
        for (int r = 1; go && r < S.R; ++r) go = upr_ret_in_box(T.J.P, T.xs + (size_t)(fp + r) * T.nx, upr_sub_speed(sm, sp, r, S.R), d);
    }
    return go;
}
// the record the walk stands at
static UPR_HDI void upr_sub_record(const upr_ret_sub_args& S, long long fp, double sm, double sp, const upr_sub_walk& w, double (&ss)[UPR_BAL_ST]) {
    const int r = upr_sub_point(w.k, S.R);
    const long long p = fp + r;
    upr_pac_transform(S.T.J.st + (size_t)p * UPR_BAL_ST, S.T.vee + (size_t)p * 3, upr_sub_speed(sm, sp, r, S.R), w.d, ss);
}
// after an evaluation: rejected -> the next edge; accepted -> the next point, after the last one the bit and the next edge
static UPR_HDI void upr_sub_step(upr_sub_walk& w, int R, bool ok, unsigned& mask) {
    if (ok && ++w.k <= R) return;
    if (ok) mask |= 1u << w.mp;
    ++w.mp; w.k = 0;
}

// ---- a wave per job ------------------------------------------------------------------------------------------------------------------
static UPR_HDI void upr_bal_retime_sub_job(const upr_ctx& ctx, const upr_ret_sub_args& S, const upr_bal_dims& L, long long job, double* W) {
    const upr_bal_args& A = S.T.J;
    const upr_problem* P = A.P;
    long long pt; int sc, m;
    upr_ret_decode(S.T, job, pt, sc, m);
    const long long fp = upr_sub_first(S, pt);
    const double* bp = A.params + (size_t)10 * P->nb * ((A.pdiv ? (fp / A.pdiv) * A.n_scen : 0) + sc);
    const double sm = S.T.speeds[m];
    unsigned mask = 0u;
    int total = 0;
    upr_sub_walk w = {0, 0, 0.0};
    while (w.mp < S.T.M) {
        const double sp = S.T.speeds[w.mp];
        if (!w.k && !upr_sub_edge(S, fp, sm, sp, w.d)) { ++w.mp; continue; }
        double ss[UPR_BAL_ST];
        upr_sub_record(S, fp, sm, sp, w, ss);
        UPR_WSYNC();   // (the previous evaluation, or the previous job of this wave, is done with the workspace)
        upr_bal_rhs(ctx, P, ss, bp, A.eq_scale, W + L.o_b);
        int np, it; double bnorm;
        const double rho = upr_bal_project(ctx, P, L, bp, A.eq_scale, upr_bal_mu_one(), W, &np, &it, &bnorm);
        total += it;
        upr_sub_step(w, S.R, rho <= UPR_BAL_FEAS * (bnorm > 1.0 ? bnorm : 1.0), mask);
    }
    if (ctx.tid == 0) {
        S.T.edges[job] = mask;
        if (A.iters) A.iters[job] = total;
    }
}

// ---- one-body arrangements: a lane per job ----------------------------------------------------------------------------------------------
static UPR_HDI void upr_bal_retime_sub_job1(const upr_ret_sub_args& S, const upr_bal_dims& L, long long job) {
    const upr_bal_args& A = S.T.J;
    const upr_problem* P = A.P;
    long long pt; int sc, m;
    upr_ret_decode(S.T, job, pt, sc, m);
    const long long fp = upr_sub_first(S, pt);
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (fp / A.pdiv) * A.n_scen : 0) + sc);
    const double sm = S.T.speeds[m];
    unsigned mask = 0u;
    int total = 0;
    upr_sub_walk w = {0, 0, 0.0};
    while (w.mp < S.T.M) {
        const double sp = S.T.speeds[w.mp];
        if (!w.k && !upr_sub_edge(S, fp, sm, sp, w.d)) { ++w.mp; continue; }
        double ss[UPR_BAL_ST], b[6];
        upr_sub_record(S, fp, sm, sp, w, ss);
        upr_bal_rhs1(P, ss, bp, A.eq_scale, b);
        double bb2 = 0.0;
        for (int c = 0; c < 6; ++c) bb2 += b[c] * b[c];
        const double bnorm = sqrt(bb2), s1 = bnorm > 1.0 ? bnorm : 1.0;
        double r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
        int pidx[UPR_BAL1_MP], np;
        total += upr_bal_project1(P, L, bp, A.eq_scale, upr_bal_mu_one(), b, UPR_BAL_TOL * s1, r, zp, pidx, np, pc, G);
        double rr = 0.0;
        for (int c = 0; c < 6; ++c) rr += r[c] * r[c];
        upr_sub_step(w, S.R, sqrt(rr) <= UPR_BAL_FEAS * s1, mask);
    }
    S.T.edges[job] = mask;
    if (A.iters) A.iters[job] = total;
}

#ifndef UPR_HOST_EMU
// a lane per fine point, a grid the launcher bounds
__global__ __launch_bounds__(64) void upr_bal_refine_kernel(upr_sub_refine_args A, long long npoints) {
    for (long long p = (long long)blockIdx.x * 64 + threadIdx.x; p < npoints; p += (long long)gridDim.x * 64) upr_bal_refine(A, p);
}
// one wave per workgroup, jobs dealt round robin (as upr_bal_retime_kernel)
__global__ __launch_bounds__(64) void upr_bal_retime_sub_kernel(upr_ret_sub_args S, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_retime_sub_job(ctx, S, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_retime_sub1_kernel(upr_ret_sub_args S, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_retime_sub_job1(S, L, job);
}
#endif
