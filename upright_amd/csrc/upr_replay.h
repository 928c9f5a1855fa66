// upr_replay.h -- replay of a time law on a clock: the states (q, qdot, qddot) of a retimed plan at t0 + k tick, and the balance of the
// objects at every one of them, between the knots as well as on them.
//
// The quantity.  Lattice, levels, h = P->dt, d_i = upr_ret_accel(s_i, s_{i+1}, h) are upr_retime.h's.  The caller gives ONE law per
// instance, level [B][N + 1] (lattice indices, or -1 throughout: no law), and a clock, tick > 0, t0 >= 0, K samples at
//
//     t_k = t0 + (double)k tick        (product and sum rounded one after the other, never fused: device, emulation and numpy hold the
//                                       same double, upr_rpl_time)
//
// Knot times: T_0 = 0, T_{i+1} = T_i + 2 h / (s_i + s_{i+1}), added sequentially in this order (numpy's cumsum holds the same doubles);
// the duration is T_N.  Segment of a sample: i the largest index <= N - 1 with T_i <= t (a sample on a knot takes the departing side),
// t' = t - T_i, s = s_i + d_i t', tau = t' (s_i + 0.5 d_i t') clamped to [0, h], sigma = tau / h.  Between the knots the path is, per
// joint, the quintic Hermite interpolant of the two knot records (q, v, a)_i and (q, v, a)_{i+1},
//
//     Q(sigma) = q_i H00 + h v_i H10 + h^2 a_i H20 + q_{i+1} H01 + h v_{i+1} H11 + h^2 a_{i+1} H21,   Q' = dQ/dsigma / h,  Q'' = d2Q/dsigma2 / h^2
//     H00 = 1 - 10 s^3 + 15 s^4 - 6 s^5    H10 = s - 6 s^3 + 8 s^4 - 3 s^5    H20 = s^2 / 2 - 3 s^3 / 2 + 3 s^4 / 2 - s^5 / 2
//     H01 = 10 s^3 - 15 s^4 + 6 s^5        H11 = -4 s^3 + 7 s^4 - 3 s^5       H21 = s^3 / 2 - s^4 + s^5 / 2
//
// defined for every plan (the multiple-shooting plans with defects too), C2 across the knots, equal to the departing state of
// BatchMPC.retimed_states at t' = 0 and to the arriving one at t' = dt_i, and equal to the plan's own cubic wherever the plan satisfies
// its triple-integrator dynamics.  The state of a sample is x(t) = (Q, s Q', s^2 Q'' + d_i Q').  Sample k EXISTS iff t_k <= T_N; count is
// the number of existing samples (t_k does not decrease with k: they are the first count ones).  A sample that does not exist holds the
// state at T_N and is not projected: rho and excess NaN, iters 0.  A plan without a law has count 0, duration +inf, its samples hold
// (q_0, 0, 0).  Acceptance is the family's rule: excess = rho / max(|b|, 1) of the cold projection, accepted iff excess <= UPR_BAL_FEAS.
// With `boxes` a sample is OUTSIDE iff some joint's s Q' or s^2 Q'' + d Q' leaves its velocity or acceleration box; positions do not
// move and jerk is not judged (upr_retime.h).
//
// The kernels.  upr_bal_replay_sample_kernel: one wave per plan; the lanes form the dt of the segments, lane 0 adds them sequentially
// into an LDS row of N + 1 doubles, then the lanes stride over the K samples: a binary search bounded by N, the Hermite per joint, the
// state to x [b][k] at stride 3 nq.  count and box_first are minima over the lanes (a wave reduction).  No atomics, no waits on other
// waves.  The state kernel of upr_balance.h runs on the B K sample states as it is.  upr_bal_replay1_kernel (a lane per job) and
// upr_bal_replay_kernel (a wave per job): job = (plan K + sample) n_scen + scenario; a job of a sample that does not exist writes the NaNs
// and returns (uniform over the wave in the wave form), every other runs upr_bal_rhs1 / upr_bal_rhs and upr_bal_project1 /
// upr_bal_project as they are and writes rho, excess and iters.  upr_bal_replay_plan_kernel: a lane per (plan, scenario), one loop bounded
// by count: worst, the largest excess over the existing samples (NaN without any), and verdict = (first sample attaining it, first
// rejected sample or -1, number rejected).
#pragma once
#include "upr_retime.h"

struct upr_rpl_args {
    upr_bal_args J;          // the points are the samples [B][K]; rho [B][K][n_scen] or NULL, z is not written, iters or NULL; pdiv K or 0
    const int* count;        // [B]
    int K;
    double* excess;          // [B][K][n_scen]
};
struct upr_rpl_sample_args {
    const upr_problem* P;
    const double* xs;        // [B][nk][nx]: the plan
    const double* speeds;    // [M]
    const int* level;        // [B][nk]
    int nk, nx, K, boxes;
    double h, tick, t0;
    double* x;               // [B][K][3 nq]
    double* duration;        // [B] or NULL
    int* count;              // [B]
    int* box_first;          // [B] or NULL
};

// t0 + k tick with the product rounded before the sum
static UPR_HDI double upr_rpl_time(double t0, int k, double tick) {
#ifdef UPR_HOST_EMU
    volatile double p = (double)k * tick;
    return t0 + p;
#else
    {
#pragma clang fp contract(off)
        const double p = (double)k * tick;
        return t0 + p;
    }
#endif
}
// the segment of time t (0 <= t) on the knot times T [N + 1]: i the largest index <= N - 1 with T_i <= t, tp = t - T_i
static UPR_HDI void upr_rpl_locate(const double* T, int N, double t, int& i, double& tp) {
    int lo = 0, hi = N - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (T[mid] <= t) lo = mid; else hi = mid - 1;
    }
    i = lo;
    tp = t - T[lo];
}
// the state of a sample tp after the departing knot of its segment: x0, x1 the records (q, v, a, ..) of the two knots, s0, s1 their
// speeds; out (3 nq).  Returns true iff some joint's velocity or acceleration lies outside its box.
static UPR_HDI bool upr_rpl_state(const upr_problem* P, const double* x0, const double* x1, double s0, double s1, double h, double tp, double* out) {
    const int nq = P->nq;
    const double d = upr_ret_accel(s0, s1, h), s = s0 + d * tp;
    double tau = tp * (s0 + 0.5 * d * tp);
    tau = tau < 0.0 ? 0.0 : (tau > h ? h : tau);
    const double g = tau / h, g2 = g * g, g3 = g2 * g, g4 = g3 * g, g5 = g4 * g;
    const double H00 = 1.0 - 10.0 * g3 + 15.0 * g4 - 6.0 * g5, H10 = g - 6.0 * g3 + 8.0 * g4 - 3.0 * g5, H20 = 0.5 * g2 - 1.5 * g3 + 1.5 * g4 - 0.5 * g5;
    const double H01 = 10.0 * g3 - 15.0 * g4 + 6.0 * g5, H11 = -4.0 * g3 + 7.0 * g4 - 3.0 * g5, H21 = 0.5 * g3 - g4 + 0.5 * g5;
    const double D00 = -30.0 * g2 + 60.0 * g3 - 30.0 * g4, D10 = 1.0 - 18.0 * g2 + 32.0 * g3 - 15.0 * g4, D20 = g - 4.5 * g2 + 6.0 * g3 - 2.5 * g4;
    const double D01 = 30.0 * g2 - 60.0 * g3 + 30.0 * g4, D11 = -12.0 * g2 + 28.0 * g3 - 15.0 * g4, D21 = 1.5 * g2 - 4.0 * g3 + 2.5 * g4;
    const double E00 = -60.0 * g + 180.0 * g2 - 120.0 * g3, E10 = -36.0 * g + 96.0 * g2 - 60.0 * g3, E20 = 1.0 - 9.0 * g + 18.0 * g2 - 10.0 * g3;
    const double E01 = 60.0 * g - 180.0 * g2 + 120.0 * g3, E11 = -24.0 * g + 84.0 * g2 - 60.0 * g3, E21 = 3.0 * g - 12.0 * g2 + 10.0 * g3;
    const double ih = 1.0 / h, s2 = s * s;
    bool outside = false;
    for (int j = 0; j < nq; ++j) {
        const double q0 = x0[j], v0 = h * x0[nq + j], a0 = h * h * x0[2 * nq + j], q1 = x1[j], v1 = h * x1[nq + j], a1 = h * h * x1[2 * nq + j];
        const double Q = q0 * H00 + v0 * H10 + a0 * H20 + q1 * H01 + v1 * H11 + a1 * H21;
        const double Q1 = (q0 * D00 + v0 * D10 + a0 * D20 + q1 * D01 + v1 * D11 + a1 * D21) * ih;
        const double Q2 = (q0 * E00 + v0 * E10 + a0 * E20 + q1 * E01 + v1 * E11 + a1 * E21) * ih * ih;
        const double sv = s * Q1, sa = s2 * Q2 + d * Q1;
        out[j] = Q; out[nq + j] = sv; out[2 * nq + j] = sa;
        outside = outside || !(sv >= P->x_lb[nq + j] && sv <= P->x_ub[nq + j] && sa >= P->x_lb[2 * nq + j] && sa <= P->x_ub[2 * nq + j]);
    }
    return outside;
}
// the smallest value over the lanes of the job's wave (the emulation has one lane)
static UPR_HDI int upr_rpl_min(const upr_ctx& ctx, int v) {
#ifndef UPR_HOST_EMU
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off);
        v = o < v ? o : v;
    }
#endif
    (void)ctx;
    return v;
}

// ---- the sampler: one plan ---------------------------------------------------------------------------------------------------------------
// W: 2 (N + 1) doubles of workspace (LDS on the device), the speeds of the knots and their times
static UPR_HDI void upr_bal_replay_sample(const upr_ctx& ctx, const upr_rpl_sample_args& A, long long b, double* W) {
    const upr_problem* P = A.P;
    const int N = A.nk - 1, nq = P->nq, K = A.K;
    const int* lv = A.level + (size_t)b * A.nk;
    const double* xs = A.xs + (size_t)b * A.nk * A.nx;
    double* xo = A.x + (size_t)b * K * 3 * nq;
    double *S = W, *T = W + A.nk;
    UPR_SYNC();   // (the previous plan of this wave is done with the rows)
    if (lv[0] < 0) {   // (no law: uniform over the wave)
        UPR_FOR(k, K) {
            for (int j = 0; j < nq; ++j) { xo[(size_t)k * 3 * nq + j] = xs[j]; xo[(size_t)k * 3 * nq + nq + j] = 0.0; xo[(size_t)k * 3 * nq + 2 * nq + j] = 0.0; }
        }
        if (ctx.tid == 0) {
            if (A.duration) A.duration[b] = INFINITY;
            A.count[b] = 0;
            if (A.box_first) A.box_first[b] = -1;
        }
        return;
    }
    UPR_FOR(i, A.nk) S[i] = A.speeds[lv[i]];
    UPR_SYNC();
    UPR_FOR(i, N) T[i + 1] = 2.0 * A.h / (S[i] + S[i + 1]);
    UPR_SYNC();
    if (ctx.tid == 0) {
        T[0] = 0.0;
        for (int i = 0; i < N; ++i) T[i + 1] = T[i] + T[i + 1];
    }
    UPR_SYNC();
    const double TN = T[N];
    int first_gone = K, first_out = K;
    UPR_FOR(k, K) {
        double t = upr_rpl_time(A.t0, k, A.tick);
        const bool exists = t <= TN;
        if (!exists) { t = TN; first_gone = k < first_gone ? k : first_gone; }
        int i; double tp;
        upr_rpl_locate(T, N, t, i, tp);
        const bool outside = upr_rpl_state(P, xs + (size_t)i * A.nx, xs + (size_t)(i + 1) * A.nx, S[i], S[i + 1], A.h, tp, xo + (size_t)k * 3 * nq);
        if (exists && outside && A.boxes) first_out = k < first_out ? k : first_out;
    }
    first_gone = upr_rpl_min(ctx, first_gone);
    first_out = upr_rpl_min(ctx, first_out);
    if (ctx.tid == 0) {
        if (A.duration) A.duration[b] = TN;
        A.count[b] = first_gone;
        if (A.box_first) A.box_first[b] = first_out < K ? first_out : -1;
    }
}

// job -> (sample as a point index, scenario, plan, sample of the plan)
static UPR_HDI void upr_rpl_decode(const upr_rpl_args& S, long long job, long long& pt, int& sc, long long& b, int& k) {
    pt = job / S.J.n_scen;
    sc = (int)(job - pt * S.J.n_scen);
    b = pt / S.K;
    k = (int)(pt - b * S.K);
}
// what a job writes: rho, excess = rho / max(|b|, 1), iters
static UPR_HDI void upr_rpl_put(const upr_rpl_args& S, long long job, double rho, double excess, int iters) {
    if (S.J.rho) S.J.rho[job] = rho;
    S.excess[job] = excess;
    if (S.J.iters) S.J.iters[job] = iters;
}

// ---- a wave per job ------------------------------------------------------------------------------------------------------------------
static UPR_HDI void upr_bal_replay_job(const upr_ctx& ctx, const upr_rpl_args& S, const upr_bal_dims& L, long long job, double* W) {
    const upr_bal_args& A = S.J;
    const upr_problem* P = A.P;
    long long pt, b; int sc, k;
    upr_rpl_decode(S, job, pt, sc, b, k);
    if (k >= S.count[b]) {   // (uniform over the wave)
        if (ctx.tid == 0) upr_rpl_put(S, job, NAN, NAN, 0);
        return;
    }
    const double* bp = A.params + (size_t)10 * P->nb * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    UPR_WSYNC();   // (the previous job of this wave is done with the workspace)
    upr_bal_rhs(ctx, P, A.st + (size_t)pt * UPR_BAL_ST, bp, A.eq_scale, W + L.o_b);
    int np, it; double bnorm;
    const double rho = upr_bal_project(ctx, P, L, bp, A.eq_scale, upr_bal_mu_one(), W, &np, &it, &bnorm);
    if (ctx.tid == 0) upr_rpl_put(S, job, rho, rho / (bnorm > 1.0 ? bnorm : 1.0), it);
}

// ---- one-body arrangements: a lane per job ----------------------------------------------------------------------------------------------
static UPR_HDI void upr_bal_replay_job1(const upr_rpl_args& S, const upr_bal_dims& L, long long job) {
    const upr_bal_args& A = S.J;
    const upr_problem* P = A.P;
    long long pt, b; int sc, k;
    upr_rpl_decode(S, job, pt, sc, b, k);
    if (k >= S.count[b]) { upr_rpl_put(S, job, NAN, NAN, 0); return; }
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    double bv[6], r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
    int pidx[UPR_BAL1_MP], np;
    upr_bal_rhs1(P, A.st + (size_t)pt * UPR_BAL_ST, bp, A.eq_scale, bv);
    double bb2 = 0.0;
    for (int c = 0; c < 6; ++c) bb2 += bv[c] * bv[c];
    const double bnorm = sqrt(bb2), s1 = bnorm > 1.0 ? bnorm : 1.0;
    const int iters = upr_bal_project1(P, L, bp, A.eq_scale, upr_bal_mu_one(), bv, UPR_BAL_TOL * s1, r, zp, pidx, np, pc, G);
    double rr = 0.0;
    for (int c = 0; c < 6; ++c) rr += r[c] * r[c];
    const double rho = sqrt(rr);
    upr_rpl_put(S, job, rho, rho / s1, iters);
}

// ---- the reduction over the samples of (plan, scenario) o -------------------------------------------------------------------------------
static UPR_HDI void upr_bal_replay_plan(const double* excess, const int* count, int K, int n_scen, long long o, double* worst, int* verdict) {
    const long long b = o / n_scen;
    const int sc = (int)(o - b * n_scen), n = count[b];
    double w = NAN;
    int at = -1, first = -1, rejected = 0;
    for (int k = 0; k < n; ++k) {
        const double e = excess[((size_t)b * K + k) * n_scen + sc];
        if (k == 0 || e > w) { w = e; at = k; }
        if (!(e <= UPR_BAL_FEAS)) { if (first < 0) first = k; ++rejected; }
    }
    if (worst) worst[o] = w;
    if (verdict) { verdict[3 * o] = at; verdict[3 * o + 1] = first; verdict[3 * o + 2] = rejected; }
}

#ifndef UPR_HOST_EMU
// one wave per workgroup, a plan at a time; LDS: 2 nk doubles
__global__ __launch_bounds__(64) void upr_bal_replay_sample_kernel(upr_rpl_sample_args A, long long nplans) {
    extern __shared__ double upr_rpl_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long b = blockIdx.x; b < nplans; b += gridDim.x) upr_bal_replay_sample(ctx, A, b, upr_rpl_lds);
}
// one wave per workgroup, jobs dealt round robin (as upr_bal_project_kernel)
__global__ __launch_bounds__(64) void upr_bal_replay_kernel(upr_rpl_args S, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_replay_job(ctx, S, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_replay1_kernel(upr_rpl_args S, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_replay_job1(S, L, job);
}
// a lane per (plan, scenario)
__global__ __launch_bounds__(64) void upr_bal_replay_plan_kernel(const double* excess, const int* count, int K, int n_scen, long long nout, double* worst,
                                                                 int* verdict) {
    const long long o = (long long)blockIdx.x * 64 + threadIdx.x;
    if (o < nout) upr_bal_replay_plan(excess, count, K, n_scen, o, worst, verdict);
}
#endif
