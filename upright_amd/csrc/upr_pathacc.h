// upr_pathacc.h -- batched path-acceleration margin: how hard a (state, inertial-parameter scenario) pair can brake along its own path,
// or accelerate along it, with the objects still balanced; and, for a state that is not balanced, how much braking would make it so.
//
// The quantity.  A trajectory replayed with the time scaling s(t) has qdot = q' sdot, qddot = q'' sdot^2 + q' sddot; at a knot
// x = (q, v, a) of the plan q' = v, q'' = a.  With sdot = s0 (`speed`) and sddot = d (1 / s) the state is x(s0, d) = (q, s0 v,
// s0^2 a + d v), and in the record of the state kernel (C_we, omega, alpha, a_ee) that is
//
//     (C_we, s0 omega, s0^2 alpha + d omega, s0^2 a_ee + d v_ee)
//
// since J_omega v = omega and J_v v = v_ee.  v_ee is not part of the record (UPR_BAL_ST stays 18): the state kernel of this quantity
// (upr_bal_state_vee_kernel) leaves it in a side array [n][3].  upr_body_residual is linear in alpha and a_ee, so b(d) = b(0) + d b2
// with b2 = b(1) - b(0); A does not depend on d; rho^2 is convex in d and the accepted d form one interval.  As in upr_speed.h the
// kernels do not use the affine form: b(d) is rebuilt by the rhs routine from the transformed record at every evaluation, and d is
// ACCEPTED iff rho(x(s0, d); theta) <= UPR_BAL_FEAS max(|b(d)|, 1) on the rho of the cold projection.  d < 0 is braking: from
// sdot = 1, sddot = -beta stops the replay in 1 / beta seconds if held.
//
// The grid.  d(k) = d_max (k - 2^31) 2^-31, k = 0 .. 2^32, held as the integer k: d(0) = -d_max, d(2^31) = 0 and d(2^32) = d_max
// exactly; a bisected end is a pair of neighbours, in - out = +-d_max 2^-31.
//
// The algorithm is upr_spd_ctl of upr_speed.h as it is, with the nominal point k1 = 2^31 (d = 0: the state itself at speed s0), and
// the job bodies are upr_bal_grid_job / upr_bal_grid_job1 of upr_speed.h with the policy upr_pac_brake below: the grid point -> d map,
// the record transform and the two records (d = 0 and d = 1, both at speed s0) the slope g = r' b2 of the descent search is taken
// between.  The first midpoint of the descent search is the nominal point again: one evaluation is repeated on that path.
// Outputs per job, accel[4] = d_lo, d_lo_out, d_hi, d_hi_out:
//   d_lo      the smallest accepted d found (-d_max if -d_max is accepted);  d_lo_out  the largest rejected d below it (-inf if none);
//   d_hi      the largest accepted d found (+d_max if +d_max is accepted);   d_hi_out  the smallest rejected d above it (+inf if none);
//   no d accepted: (+inf, -d_max, -inf, +d_max).
// 0 in [d_lo, d_hi] iff the state is balanced at speed s0; d_hi < 0: balanced only while braking at least that hard; d_lo: the hardest
// balanced braking.  Certificates and iters as in upr_speed.h: z [2][ncol] at d_lo and d_hi, the polished y [2][6 nb] at the two
// rejected neighbours, zeros where an end does not exist.
//
// upr_bal_pathacc_plan_kernel reduces over the knots of a plan: the largest d_lo, the smallest d_hi, the first knot attaining each
// (upr_bal_speed_window on the four-double layout), and once per instance limit[2]: the interval of d for which s0^2 a_i + d v_i stays
// inside the acceleration box of every joint at every knot ((-inf, +inf) for a plan at rest; lo > hi when s0^2 a is outside the box
// already: reported as computed).  Jerk is NOT part of it: a step in sddot is an impulse of jerk, so no finite jerk bound survives
// the moment the braking sets in; what a retiming may do to the jerk belongs to the pass that shapes sddot(t), not to this slice.
#pragma once
#include "upr_speed.h"

struct upr_pac_args {
    upr_bal_args J;          // the jobs, as upr_spd_args
    double d_max, speed;     // the range [-d_max, d_max] of sddot and sdot = s0
    const double* vee;       // [n][3]: the linear velocity of the end effector, world frame
    double* accel;           // [n][n_scen][4]: d_lo, d_lo_out, d_hi, d_hi_out
    double* y;               // [n][n_scen][2][6 nb] or NULL
};

#define UPR_PAC_HALF (1ll << (UPR_BAL_BISECT - 1))
static UPR_HDI double upr_pac_at(unsigned long long k, double d_max) {
    return d_max * ((double)((long long)k - UPR_PAC_HALF) * (1.0 / (double)UPR_PAC_HALF));
}
// the state kernel's record at sdot = s0, sddot = d: (C_we, s0 omega, s0^2 alpha + d omega, s0^2 a_ee + d v_ee)
static UPR_HDI void upr_pac_transform(const double* st, const double* vee, double s0, double d, double (&out)[UPR_BAL_ST]) {
    const double s2 = s0 * s0;
    for (int i = 0; i < 9; ++i) out[i] = st[i];
    for (int i = 0; i < 3; ++i) {
        out[9 + i] = s0 * st[9 + i];
        out[12 + i] = s2 * st[12 + i] + d * st[9 + i];
        out[15 + i] = s2 * st[15 + i] + d * vee[i];
    }
}
static UPR_HDI void upr_pac_answer(const upr_spd_ctl& c, double d_max, double* out) {
    if (!c.found) { out[0] = INFINITY; out[1] = -d_max; out[2] = -INFINITY; out[3] = d_max; return; }
    out[0] = upr_pac_at(c.lo_in, d_max);
    out[1] = c.e0 ? -INFINITY : upr_pac_at(c.lo_out, d_max);
    out[2] = upr_pac_at(c.hi_in, d_max);
    out[3] = c.eM ? INFINITY : upr_pac_at(c.hi_out, d_max);
}
// the policy of upr_bal_grid_job / upr_bal_grid_job1 for this quantity
struct upr_pac_brake {
    double d_max, s0;
    const double* vee;
    // (a range of 2 puts the nominal point of upr_spd_begin at 2^32 / 2 = 2^31, d = 0)
    UPR_HDI void begin(upr_spd_ctl& c) const { upr_spd_begin(c, 2.0); }
    UPR_HDI void record(const double* st, long long pt, unsigned long long k, double (&out)[UPR_BAL_ST]) const {
        upr_pac_transform(st, vee + (size_t)pt * 3, s0, upr_pac_at(k, d_max), out);
    }
    UPR_HDI void slope_ends(const double* st, long long pt, double (&r0)[UPR_BAL_ST], double (&r1)[UPR_BAL_ST]) const {
        upr_pac_transform(st, vee + (size_t)pt * 3, s0, 0.0, r0);
        upr_pac_transform(st, vee + (size_t)pt * 3, s0, 1.0, r1);
    }
    UPR_HDI void answer(const upr_spd_ctl& c, double* out) const { upr_pac_answer(c, d_max, out); }
};
static UPR_HDI void upr_bal_pathacc_job(const upr_ctx& ctx, const upr_pac_args& S, const upr_bal_dims& L, long long job, double* W) {
    upr_bal_grid_job(ctx, S.J, upr_pac_brake{S.d_max, S.speed, S.vee}, S.accel, S.y, L, job, W);
}
static UPR_HDI void upr_bal_pathacc_job1(const upr_pac_args& S, const upr_bal_dims& L, long long job) {
    upr_bal_grid_job1(S.J, upr_pac_brake{S.d_max, S.speed, S.vee}, S.accel, S.y, L, job);
}

// ---- the state point that keeps v_ee ----------------------------------------------------------------------------------------------------
template <int NQ>
static UPR_HDI void upr_bal_state_point(const upr_problem* P, const double* x, double* st, double* vee) {
    upr_ee<double> E;
    upr_ee_kinematics<double, NQ, true>(P, x, -1, E);
    for (int i = 0; i < 9; ++i) st[i] = E.C[i];
    for (int i = 0; i < 3; ++i) { st[9 + i] = E.w[i]; st[12 + i] = E.al[i]; st[15 + i] = E.a[i]; vee[i] = E.v[i]; }
}

// ---- the knots of a plan ----------------------------------------------------------------------------------------------------------------
// the interval of d with lb <= s0^2 a_i + d v_i <= ub for every joint i at every knot of one instance: xs [nk][nx] = (q, v, a, ..);
// out[0] = lo, out[1] = hi.  A joint at rest (v_i = 0) does not bound d.
static UPR_HDI void upr_bal_pathacc_limit(const upr_problem* P, int nk, int nx, double s0, const double* xs, double* out) {
    const int nq = P->nq;
    const double s2 = s0 * s0;
    double lo = -INFINITY, hi = INFINITY;
    for (int k = 0; k < nk; ++k) {
        for (int i = 0; i < nq; ++i) {
            const double v = xs[(size_t)k * nx + nq + i], a = s2 * xs[(size_t)k * nx + 2 * nq + i];
            if (v == 0.0) continue;
            const double dl = (P->x_lb[2 * nq + i] - a) / v, du = (P->x_ub[2 * nq + i] - a) / v;
            const double l = v > 0.0 ? dl : du, u = v > 0.0 ? du : dl;
            lo = l > lo ? l : lo;
            hi = u < hi ? u : hi;
        }
    }
    out[0] = lo; out[1] = hi;
}

#ifndef UPR_HOST_EMU
template <int NQ>
__global__ void upr_bal_state_vee_kernel(const upr_problem* P, int n, const double* x, double* st, double* vee) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    upr_bal_state_point<NQ>(P, x + (size_t)i * 3 * NQ, st + (size_t)i * UPR_BAL_ST, vee + (size_t)i * 3);
}
// one wave per workgroup, jobs dealt round robin (as upr_bal_speed_kernel)
__global__ __launch_bounds__(64) void upr_bal_pathacc_kernel(upr_pac_args S, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_pathacc_job(ctx, S, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_pathacc1_kernel(upr_pac_args S, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_pathacc_job1(S, L, job);
}
// one lane per (instance, scenario, end); the lanes past nout, one per instance, compute limit [B][2] (may be NULL)
__global__ __launch_bounds__(64) void upr_bal_pathacc_plan_kernel(const upr_problem* P, const double* accel, int nk, int n_scen, long long nout, int B, int nx,
                                                                  double s0, const double* xs, double* window, int* knot, double* limit) {
    const long long o = (long long)blockIdx.x * 64 + threadIdx.x;
    if (o < nout) upr_bal_speed_window(accel, nk, n_scen, o, window, knot);
    else if (limit && o - nout < B) {
        const long long b = o - nout;
        upr_bal_pathacc_limit(P, nk, nx, s0, xs + (size_t)b * nk * nx, limit + 2 * b);
    }
}
#endif
