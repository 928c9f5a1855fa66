// upr_retime.h -- retiming of a plan on a speed lattice: the fastest time law s(t) that replays the same geometric path with the objects
// balanced at every knot, under one inertial-parameter scenario or under all of them at once.
//
// The quantity.  The path parameter is plan time, the knots are i = 0 .. N, h = P->dt.  The caller gives a lattice of replay speeds
// s_0 < s_1 < .. < s_{M-1} (finite, >= 0, 1 <= M <= 32).  A time law assigns a level m_i to every knot and keeps sddot constant on
// every segment: on segment i, from knot i to knot i + 1,
//
//     d_i = (s_{m_{i+1}}^2 - s_{m_i}^2) / (2 h)        (exact for constant sddot; evaluated as (s' - s) (s' + s) / (2 h), which no
//                                                        compiler contracts: device, emulation and numpy hold the same double)
//     dt_i = 2 h / (s_{m_i} + s_{m_{i+1}})
//
// and an edge whose two speeds sum to 0 does not exist (the replay would never leave the knot).  The state of knot i at speed s and
// path acceleration d is x_i(s, d) = (q_i, s v_i, s^2 a_i + d v_i), in the record of the state kernel upr_pac_transform(st_i, vee_i, s,
// d) of upr_pathacc.h.  Edge (i, m -> m') is ADMISSIBLE in a scenario iff both of its end states are accepted -- the departing state
// x_i(s_m, d) and the arriving state x_{i+1}(s_m', d) -- by the family's rule, rho of the cold projection <= UPR_BAL_FEAS max(|b|, 1),
// and, with `boxes`, iff at both ends s v_j lies inside the velocity box and s^2 a_j + d v_j inside the acceleration box of every
// joint j.  Positions are untouched: the path is.  Jerk is NOT enforced: a step of sddot at a knot is an impulse of jerk (the argument
// of upr_pathacc.h), so no finite jerk bound survives a time law that is piecewise constant in sddot.
//
// The mask kernels.  A job is (instance, scenario, segment, from-level m); it walks m' = 0 .. M - 1 and writes ONE uint32, bit m' set
// iff the edge m -> m' is admissible: no atomics.  The projection is skipped when the edge does not exist or a box fails, and the
// arriving state is skipped when the departing one is rejected: at most 2 M single projections per job.  Each evaluation is
// upr_pac_transform -> upr_bal_rhs1 / upr_bal_rhs -> upr_bal_project1 / upr_bal_project -> the rule, the device functions of the family as
// they are.  The jobs carry no search state.  (Up to the ball of the rule a mask row is one contiguous run of bits: the accepted d of a
// state form an interval and d is monotone in m'.  Nothing here builds on it.)
//
// The path kernel.  One wave per output -- (instance, scenario), or the instance with `common`, where the masks of all scenarios are
// ANDed first -- and a lane per level.  Backward sweep of the exact dynamic programme
//
//     T[N][m] = 0 (only for the `end` level when one is given),  T[i][m] = min over admissible m' of dt(m, m') + T[i + 1][m'],
//
// ties (equal doubles) to the smallest m'; the row of the next knot lives in an LDS row every lane reads, the argmin goes to a table
// [N][M] of bytes.  Then lane 0 walks forward: the start level is `start` when given, else the argmin of T[0][.] (ties to the smallest);
// duration = T there (+inf: no time law on the lattice, level = -1 throughout); reach = (f, g): f the last knot with a non-empty set of
// levels reachable from the start set over admissible edges, g the first knot that has a level with finite T -- (N, 0) for a feasible
// plan, where an infeasible one blocks seen from each side.  All loops are bounded by N and M; no atomics, no waits on other waves.
#pragma once
#include "upr_pathacc.h"

#define UPR_RET_MAX_LEVELS 32
#define UPR_RET_NONE 255

struct upr_ret_args {
    upr_bal_args J;          // the points are the knots [B][nk] of the plan; rho and z are not read; iters [B][n_scen][N][M] or NULL
    const double* vee;       // [n][3]: the linear velocity of the end effector (upr_bal_state_vee_kernel)
    const double* xs;        // [n][nx]: the plan itself, for the boxes
    const double* speeds;    // [M]
    int M, nk, nx, boxes;
    double h;                // P->dt
    unsigned* edges;         // [B][n_scen][N][M]: bit m' of row (i, m)
};
struct upr_ret_path_args {
    const unsigned* edges;   // [B][n_scen][N][M]
    const double* speeds;    // [M]
    int M, nk, n_scen, common, start, end;   // start, end: a level or -1
    double h;
    unsigned char* arg;      // [nout][N][M]: the argmin of every (knot, level), UPR_RET_NONE where T is infinite
    double* duration;        // [nout]
    int* level;              // [nout][nk]
    int* reach;              // [nout][2] or NULL
};

// the path acceleration of an edge between the speeds s and sp
static UPR_HDI double upr_ret_accel(double s, double sp, double h) { return (sp - s) * (sp + s) / (2.0 * h); }
// s v and s^2 a + d v of every joint inside the velocity and acceleration boxes; x = (q, v, a, ..) of one knot
static UPR_HDI bool upr_ret_in_box(const upr_problem* P, const double* x, double s, double d) {
    const int nq = P->nq;
    const double s2 = s * s;
    bool ok = true;
    for (int j = 0; j < nq; ++j) {
        const double v = x[nq + j], sv = s * v, sa = s2 * x[2 * nq + j] + d * v;
        ok = ok && sv >= P->x_lb[nq + j] && sv <= P->x_ub[nq + j] && sa >= P->x_lb[2 * nq + j] && sa <= P->x_ub[2 * nq + j];
    }
    return ok;
}
// job -> (knot of the departing end as a point index, scenario, from-level)
static UPR_HDI void upr_ret_decode(const upr_ret_args& S, long long job, long long& pt, int& sc, int& m) {
    const int N = S.nk - 1;
    long long t = job / S.M;
    m = (int)(job - t * S.M);
    const int i = (int)(t % N); t /= N;
    sc = (int)(t % S.J.n_scen);
    pt = (t / S.J.n_scen) * S.nk + i;
}

// ---- a wave per job ------------------------------------------------------------------------------------------------------------------
static UPR_HDI void upr_bal_retime_job(const upr_ctx& ctx, const upr_ret_args& S, const upr_bal_dims& L, long long job, double* W) {
    const upr_bal_args& A = S.J;
    const upr_problem* P = A.P;
    long long pt; int sc, m;
    upr_ret_decode(S, job, pt, sc, m);
    const double* bp = A.params + (size_t)10 * P->nb * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const double sm = S.speeds[m];
    unsigned mask = 0u;
    int total = 0;
    bool dep = false;
    double d = 0.0;
    // e = 2 m' + end: the departing state of edge m -> m', then its arriving state
    for (int e = 0; e < 2 * S.M; ++e) {
        const int mp = e >> 1, arr = e & 1;
        const double sp = S.speeds[mp];
        if (!arr) {
            d = upr_ret_accel(sm, sp, S.h);
            dep = false;
            bool go = sm + sp > 0.0;
            if (go && S.boxes) go = upr_ret_in_box(P, S.xs + (size_t)pt * S.nx, sm, d) && upr_ret_in_box(P, S.xs + (size_t)(pt + 1) * S.nx, sp, d);
            if (!go) { ++e; continue; }
        } else if (!dep) continue;
        const long long p = pt + arr;
        double ss[UPR_BAL_ST];
        upr_pac_transform(A.st + (size_t)p * UPR_BAL_ST, S.vee + (size_t)p * 3, arr ? sp : sm, d, ss);
        UPR_WSYNC();   // (the previous evaluation, or the previous job of this wave, is done with the workspace)
        upr_bal_rhs(ctx, P, ss, bp, A.eq_scale, W + L.o_b);
        int np, it; double bnorm;
        const double rho = upr_bal_project(ctx, P, L, bp, A.eq_scale, upr_bal_mu_one(), W, &np, &it, &bnorm);
        total += it;
        const bool ok = rho <= UPR_BAL_FEAS * (bnorm > 1.0 ? bnorm : 1.0);
        if (!arr) dep = ok;
        else if (ok) mask |= 1u << mp;
    }
    if (ctx.tid == 0) {
        S.edges[job] = mask;
        if (A.iters) A.iters[job] = total;
    }
}

// ---- one-body arrangements: a lane per job ----------------------------------------------------------------------------------------------
// one copy of the projection's code for both ends of every edge
static UPR_HDI void upr_bal_retime_job1(const upr_ret_args& S, const upr_bal_dims& L, long long job) {
    const upr_bal_args& A = S.J;
    const upr_problem* P = A.P;
    long long pt; int sc, m;
    upr_ret_decode(S, job, pt, sc, m);
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const double sm = S.speeds[m];
    unsigned mask = 0u;
    int total = 0;
    bool dep = false;
    double d = 0.0;
    for (int e = 0; e < 2 * S.M; ++e) {
        const int mp = e >> 1, arr = e & 1;
        const double sp = S.speeds[mp];
        if (!arr) {
            d = upr_ret_accel(sm, sp, S.h);
            dep = false;
            bool go = sm + sp > 0.0;
            if (go && S.boxes) go = upr_ret_in_box(P, S.xs + (size_t)pt * S.nx, sm, d) && upr_ret_in_box(P, S.xs + (size_t)(pt + 1) * S.nx, sp, d);
            if (!go) { ++e; continue; }
        } else if (!dep) continue;
        const long long p = pt + arr;
        double ss[UPR_BAL_ST], b[6];
        upr_pac_transform(A.st + (size_t)p * UPR_BAL_ST, S.vee + (size_t)p * 3, arr ? sp : sm, d, ss);
        upr_bal_rhs1(P, ss, bp, A.eq_scale, b);
        double bb2 = 0.0;
        for (int c = 0; c < 6; ++c) bb2 += b[c] * b[c];
        const double bnorm = sqrt(bb2), s1 = bnorm > 1.0 ? bnorm : 1.0;
        double r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
        int pidx[UPR_BAL1_MP], np;
        total += upr_bal_project1(P, L, bp, A.eq_scale, upr_bal_mu_one(), b, UPR_BAL_TOL * s1, r, zp, pidx, np, pc, G);
        double rr = 0.0;
        for (int c = 0; c < 6; ++c) rr += r[c] * r[c];
        const bool ok = sqrt(rr) <= UPR_BAL_FEAS * s1;
        if (!arr) dep = ok;
        else if (ok) mask |= 1u << mp;
    }
    S.edges[job] = mask;
    if (A.iters) A.iters[job] = total;
}

// ---- the dynamic programme ---------------------------------------------------------------------------------------------------------------
// row (i, m) of the masks of output o: one scenario's, or the AND over all scenarios (E points at the first of ns rows, N M apart)
static UPR_HDI unsigned upr_ret_row(const unsigned* E, int ns, size_t stride, int i, int M, int m) {
    unsigned mask = E[(size_t)i * M + m];
    for (int s = 1; s < ns; ++s) mask &= E[s * stride + (size_t)i * M + m];
    return mask;
}
// T: 2 UPR_RET_MAX_LEVELS doubles of workspace (LDS on the device), the rows of two neighbouring knots
static UPR_HDI void upr_bal_retime_path(const upr_ctx& ctx, const upr_ret_path_args& A, long long o, double* T) {
    const int N = A.nk - 1, M = A.M;
    const long long b = A.common ? o : o / A.n_scen;
    const int sc0 = A.common ? 0 : (int)(o - b * A.n_scen), ns = A.common ? A.n_scen : 1;
    const size_t stride = (size_t)N * M;
    const unsigned* E = A.edges + ((size_t)b * A.n_scen + sc0) * stride;
    unsigned char* arg = A.arg + (size_t)o * stride;
    const double inf = INFINITY;
    UPR_SYNC();   // (the previous output of this wave is done with the rows)
    int cur = 0, g = N;
    UPR_FOR(m, M) T[m] = (A.end < 0 || m == A.end) ? 0.0 : inf;
    for (int i = N - 1; i >= 0; --i) {
        UPR_WSYNC();
        const double* Tn = T + cur * UPR_RET_MAX_LEVELS;
        double* Tc = T + (cur ^ 1) * UPR_RET_MAX_LEVELS;
        UPR_FOR(m, M) {
            const unsigned mask = upr_ret_row(E, ns, stride, i, M, m);
            const double sm = A.speeds[m];
            double best = inf; int a = UPR_RET_NONE;
            for (int mp = 0; mp < M; ++mp) {
                if (!((mask >> mp) & 1u)) continue;
                const double c = 2.0 * A.h / (sm + A.speeds[mp]) + Tn[mp];
                if (c < best) { best = c; a = mp; }
            }
            Tc[m] = best;
            arg[(size_t)i * M + m] = (unsigned char)a;
        }
        UPR_WSYNC();
        bool any = false;
        for (int mp = 0; mp < M; ++mp) any = any || Tc[mp] < inf;
        if (any) g = i;
        cur ^= 1;
    }
    UPR_SYNC();   // (the table of the other lanes is in memory)
    if (ctx.tid != 0) return;
    const double* T0 = T + cur * UPR_RET_MAX_LEVELS;
    int s0 = A.start >= 0 ? A.start : 0;
    if (A.start < 0) for (int m = 1; m < M; ++m) if (T0[m] < T0[s0]) s0 = m;
    const double dur = T0[s0];
    A.duration[o] = dur;
    if (A.level) {
        int* lv = A.level + (size_t)o * A.nk;
        if (dur < inf) {
            int m = s0;
            lv[0] = m;
            for (int i = 0; i < N; ++i) { m = arg[(size_t)i * M + m]; lv[i + 1] = m; }
        } else for (int i = 0; i <= N; ++i) lv[i] = -1;
    }
    if (A.reach) {
        unsigned R = A.start >= 0 ? 1u << A.start : (M >= 32 ? 0xffffffffu : (1u << M) - 1u);
        int f = 0;
        for (int i = 0; i < N; ++i) {
            unsigned Rn = 0u;
            for (int m = 0; m < M; ++m) if ((R >> m) & 1u) Rn |= upr_ret_row(E, ns, stride, i, M, m);
            if (!Rn) break;
            R = Rn; f = i + 1;
        }
        A.reach[2 * o] = f; A.reach[2 * o + 1] = g;
    }
}

#ifndef UPR_HOST_EMU
// one wave per workgroup, jobs dealt round robin (as upr_bal_pathacc_kernel)
__global__ __launch_bounds__(64) void upr_bal_retime_kernel(upr_ret_args S, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_retime_job(ctx, S, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_retime1_kernel(upr_ret_args S, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_retime_job1(S, L, job);
}
// one wave per output, a lane per level
__global__ __launch_bounds__(64) void upr_bal_retime_path_kernel(upr_ret_path_args A, long long nout) {
    __shared__ double T[2 * UPR_RET_MAX_LEVELS];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long o = blockIdx.x; o < nout; o += gridDim.x) upr_bal_retime_path(ctx, A, o, T);
}
#endif
