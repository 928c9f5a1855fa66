// upr_disturb.h -- batched disturbance margin: how much tray acceleration the plan did NOT choose a (state, inertial-parameter scenario)
// pair absorbs along given directions with the objects still balanced -- a bump, a tracking error, a hand on the arm.
//
// The quantity.  A direction u = (u_alpha, u_a) in R^6 (rad/s^2 and m/s^2 per unit r) displaces the record of the state kernel to
//
//     (C_we, omega, alpha + r u_alpha, a_ee + r u_a)
//
// upr_body_residual is linear in alpha and a_ee, so b(r) = b(0) + r b_u with b_u = b(1) - b(0); A does not depend on r; rho^2 is convex
// in r and the accepted r form one interval.  The path-acceleration margin of upr_pathacc.h at speed 1 is the special case u = (omega,
// v_ee).  dirs [n_dir][6] holds the rows (u_alpha, u_a), 1 <= n_dir <= UPR_DST_MAX_DIRS; frame 0: in the frame the record keeps omega,
// alpha and a_ee in (world); frame 1: in the tray frame, u_world = C_we u_tray for both halves with the record's own C_we, rotated at
// every evaluation (nine multiplications next to a projection).  As in upr_speed.h the kernels do not use the affine form: b(r) is
// rebuilt by the rhs routine from the displaced record at every evaluation, and r is ACCEPTED iff rho <= UPR_BAL_FEAS max(|b(r)|, 1) on
// the rho of the cold projection.
//
// The grid is upr_pathacc.h's: r(k) = r_max (k - 2^31) 2^-31, k = 0 .. 2^32, the nominal point r = 0; the decisions are upr_spd_ctl of
// upr_speed.h as they are, the job bodies upr_bal_grid_job / upr_bal_grid_job1 with the policy upr_dst_push below.  A job is (point,
// scenario, direction) and writes reach[4] = r_lo, r_lo_out, r_hi, r_hi_out with the conventions of accel[4] of upr_pathacc.h (open
// ends -inf / +inf, no r accepted: (+inf, -r_max, -inf, +r_max)).  -r_lo is what the state absorbs along -u, r_hi what it absorbs along
// +u; 0 in [r_lo, r_hi] iff the state is balanced.  Certificates z [2][ncol], y [2][6 nb] and iters as there.
//
// The layouts are DIRECTION-MAJOR: reach [n_dir][n][n_scen][4], z, y and iters likewise with a leading n_dir.  One direction is one
// block in the layout the shared job bodies write: a job runs them on a copy of upr_bal_args whose output pointers are offset by its
// block, and upr_bal_speed_window reads a block as it is.
//
// upr_bal_disturb_plan_kernel reduces over the knots of a plan, one lane per (instance, scenario): per direction the window (largest
// r_lo, smallest r_hi) and the first knot attaining each; radius = min over directions of min(-window_lo, window_hi), the largest r every
// knot absorbs along every +-u given (negative when some knot is not balanced, -inf when some job accepts nothing); binding[3] =
// (direction, sign -1 | +1, knot) of the end that attains it -- directions in ascending order, the lower end before the upper, a strict
// comparison replaces, so the first end wins ties.  No atomics; loops bounded by N + 1 and n_dir; no NaN (-(+inf) and -inf compare).
#pragma once
#include "upr_pathacc.h"

#define UPR_DST_MAX_DIRS 32

struct upr_dst_args {
    upr_bal_args J;          // the jobs of ONE direction, as upr_pac_args; z [n_dir][n][n_scen][2][ncol] or NULL; iters [n_dir][n][n_scen] or NULL
    double r_max;            // the range [-r_max, r_max] of r
    const double* dirs;      // [n_dir][6]: (u_alpha, u_a)
    int n_dir, frame;        // frame 0: world, 1: tray
    double* reach;           // [n_dir][n][n_scen][4]: r_lo, r_lo_out, r_hi, r_hi_out
    double* y;               // [n_dir][n][n_scen][2][6 nb] or NULL
};

// the state kernel's record displaced by r along u: (C_we, omega, alpha + r u_alpha, a_ee + r u_a), u rotated by the record's C_we
// (row-major) when it is given in the tray frame
static UPR_HDI void upr_dst_transform(const double* st, const double* u, int frame, double r, double (&out)[UPR_BAL_ST]) {
    for (int i = 0; i < 12; ++i) out[i] = st[i];
    for (int h = 0; h < 2; ++h) {
        const double* uh = u + 3 * h;
        for (int i = 0; i < 3; ++i) {
            const double w = frame ? st[3 * i] * uh[0] + st[3 * i + 1] * uh[1] + st[3 * i + 2] * uh[2] : uh[i];
            out[12 + 3 * h + i] = st[12 + 3 * h + i] + r * w;
        }
    }
}
// the policy of upr_bal_grid_job / upr_bal_grid_job1 for this quantity
struct upr_dst_push {
    double r_max;
    const double* u;         // the six doubles of the job's direction
    int frame;
    UPR_HDI void begin(upr_spd_ctl& c) const { upr_spd_begin(c, 2.0); }   // (the nominal point 2^31, r = 0: as upr_pac_brake)
    UPR_HDI void record(const double* st, long long, unsigned long long k, double (&out)[UPR_BAL_ST]) const {
        upr_dst_transform(st, u, frame, upr_pac_at(k, r_max), out);
    }
    UPR_HDI void slope_ends(const double* st, long long, double (&r0)[UPR_BAL_ST], double (&r1)[UPR_BAL_ST]) const {
        upr_dst_transform(st, u, frame, 0.0, r0);
        upr_dst_transform(st, u, frame, 1.0, r1);
    }
    UPR_HDI void answer(const upr_spd_ctl& c, double* out) const { upr_pac_answer(c, r_max, out); }
};
// the jobs of direction d: S.J with the output pointers moved to the direction's block
static UPR_HDI upr_bal_args upr_dst_block(const upr_dst_args& S, const upr_bal_dims& L, int d, size_t& blk) {
    upr_bal_args A = S.J;
    blk = (size_t)d * A.n * A.n_scen;
    if (A.z) A.z += blk * 2 * L.ncol;
    if (A.iters) A.iters += blk;
    return A;
}
static UPR_HDI void upr_bal_disturb_job(const upr_ctx& ctx, const upr_dst_args& S, const upr_bal_dims& L, int d, long long job, double* W) {
    size_t blk;
    const upr_bal_args A = upr_dst_block(S, L, d, blk);
    upr_bal_grid_job(ctx, A, upr_dst_push{S.r_max, S.dirs + 6 * d, S.frame}, S.reach + blk * 4, S.y ? S.y + blk * 2 * L.m : nullptr, L, job, W);
}
static UPR_HDI void upr_bal_disturb_job1(const upr_dst_args& S, const upr_bal_dims& L, int d, long long job) {
    size_t blk;
    const upr_bal_args A = upr_dst_block(S, L, d, blk);
    upr_bal_grid_job1(A, upr_dst_push{S.r_max, S.dirs + 6 * d, S.frame}, S.reach + blk * 4, S.y ? S.y + blk * 12 : nullptr, L, job);
}

// ---- the knots of a plan ----------------------------------------------------------------------------------------------------------------
// reach [n_dir][B][nk][n_scen][4] -> window, knot [n_dir][B][n_scen][2] (upr_bal_speed_window on every direction block), radius
// [B][n_scen], binding [B][n_scen][3], for bs = instance n_scen + scenario.  radius, binding: each may be NULL.
static UPR_HDI void upr_bal_disturb_reduce(const double* reach, int nk, int n_scen, int n_dir, long long nbs, long long bs, double* window, int* knot,
                                           double* radius, int* binding) {
    double rad = 0.0;
    int bd = 0, sg = -1, bk = 0;
    for (int d = 0; d < n_dir; ++d) {
        double* w = window + (size_t)d * nbs * 2;
        int* kn = knot + (size_t)d * nbs * 2;
        for (int end = 0; end < 2; ++end) {
            const long long o = 2 * bs + end;
            upr_bal_speed_window(reach + (size_t)d * nbs * nk * 4, nk, n_scen, o, w, kn);
            const double c = end == 0 ? -w[o] : w[o];
            if ((d == 0 && end == 0) || c < rad) { rad = c; bd = d; sg = end == 0 ? -1 : 1; bk = kn[o]; }
        }
    }
    if (radius) radius[bs] = rad;
    if (binding) { binding[3 * bs] = bd; binding[3 * bs + 1] = sg; binding[3 * bs + 2] = bk; }
}

#ifndef UPR_HOST_EMU
// one wave per workgroup, jobs x directions dealt round robin; njobs: the jobs of one direction times n_dir
__global__ __launch_bounds__(64) void upr_bal_disturb_kernel(upr_dst_args S, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    const long long per = (long long)S.J.n * S.J.n_scen;
    for (long long t = blockIdx.x; t < njobs; t += gridDim.x) {
        const long long d = t / per;
        upr_bal_disturb_job(ctx, S, L, (int)d, t - d * per, upr_bal_lds);
    }
}
// one-body arrangements: one lane per job, no LDS, the direction on blockIdx.y; njobs: the jobs of one direction
__global__ __launch_bounds__(64) void upr_bal_disturb1_kernel(upr_dst_args S, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_disturb_job1(S, L, (int)blockIdx.y, job);
}
// one lane per (instance, scenario)
__global__ __launch_bounds__(64) void upr_bal_disturb_plan_kernel(const double* reach, int nk, int n_scen, int n_dir, long long nbs, double* window, int* knot,
                                                                  double* radius, int* binding) {
    const long long bs = (long long)blockIdx.x * 64 + threadIdx.x;
    if (bs < nbs) upr_bal_disturb_reduce(reach, nk, n_scen, n_dir, nbs, bs, window, knot, radius, binding);
}
#endif
