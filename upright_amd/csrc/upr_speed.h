// upr_speed.h -- batched speed margin: the interval of uniform replay speeds at which a (state, inertial-parameter scenario) pair is
// balanced.  By what factor must a plan be slowed down under scenario theta, by what factor could it be sped up?
//
// The quantity.  A trajectory replayed s times faster, q(t) -> q(s t), turns a knot x = (q, v, a) into x_s = (q, s v, s^2 a); in the
// record the state kernel leaves (C_we, omega, alpha, a_ee: UPR_BAL_ST doubles, gravity is not in it) that is (C_we, s omega,
// s^2 alpha, s^2 a_ee).  Every dynamic term of upr_body_residual is quadratic in omega or linear in alpha and a_ee, so
// b(s) = b0 + s^2 (b1 - b0) with b0 the right-hand side at rest and b1 the one at s = 1; A does not depend on s.  rho is convex in
// s^2, and at zero tolerance the balanced speeds of a job form one interval [s-, s+].  The kernels do not use the affine form: b(s)
// is rebuilt by the rhs routine of upr_balance.h from the scaled record at every evaluation, and a speed s is ACCEPTED iff
//
//     rho(x_s; theta) <= UPR_BAL_FEAS max(|b(s)|, 1)
//
// on the rho of the cold projection of upr_balance.h (upr_bal_project / upr_bal_project1: the bodies the rho kernels run).
//
// The grid.  Every evaluation lies on s(k) = s_max k 2^-32, k = 0 .. 2^32 (UPR_BAL_BISECT = 32 halvings of [0, s_max]), held as the
// integer k: a bisected end is a pair of neighbours, in - out = +-s_max 2^-32.  The nominal speed is the grid point k1 = floor(2^32 /
// s_max), which is s = 1 itself when s_max is a power of two (the default 4).
//
// The algorithm (upr_spd_ctl: the one copy of the decisions, run by both kernels, the emulation and, transcribed, tests/speed_ref.py).
// F(k): s(k) is accepted.
//   1. F(0), F(2^32).  Both hold: done (class `all`).
//   2. F(0) holds, F(2^32) does not: halvings of [0, 2^32] give the upper end (`upper`).
//   3. F(0) does not hold: a seed is needed -- k1 if F(k1) holds; else 2^32 if F(2^32) held; else a descent search on [0, 2^32]: at the
//      midpoint g = r' (b1 - b0), r the projection's residual, is the slope of rho^2 / 2 in s^2; g < 0: the minimiser lies above,
//      lo = mid, otherwise hi = mid; the first accepted midpoint is the seed; 32 halvings without one: no speed is accepted (`none`).
//   4. With a seed: halvings of [0, seed] for the lower end, of [seed, 2^32] for the upper end unless F(2^32) held (`window`).
// At most 3 + 3 * 32 evaluations.  Outputs per job, speed[4] = s_lo, s_lo_out, s_hi, s_hi_out:
//   s_lo      the smallest accepted speed found (0 if rest is accepted);  s_lo_out  the largest rejected speed below it (0 if none);
//   s_hi      the largest accepted speed found (s_max if s_max is accepted);  s_hi_out  the smallest rejected speed above it (+inf if
//             s_max is accepted);
//   no speed accepted: s_lo = +inf, s_hi = -inf, s_lo_out = 0 and s_hi_out = s_max (the two rejected ends of the range).
// The reported ends are the accepted, conservative side.  Certificates, written at the evaluation that produced them (plain stores,
// only when asked for): z [2][ncol], the multipliers at s_lo and at s_hi (z >= 0, |b(s) + A z| inside the ball; zeros where there is
// no accepted end); y [2][6 nb], the polished residual (upr_bal_polish*) at s_lo_out and at s_hi_out (y' a_j >= 0 for every column,
// y' b(s) / |y| outside the ball; zeros where there is no rejected end).  iters: the least-squares solves over all evaluations.
// nf = 1 shapes take the same path: the speed matters with or without friction.
//
// upr_bal_speed_plan_kernel reduces over the knots of a plan: the largest s_lo, the smallest s_hi, the first knot attaining each,
// and once per instance the limit speed -- the largest s at which s v, s^2 a and s^3 u of every knot stay inside the velocity,
// acceleration and jerk boxes the QP enforces (+inf for a plan at rest; position bounds do not scale).
#pragma once
#include "upr_margin.h"

struct upr_spd_args {
    upr_bal_args J;          // the jobs, as upr_mar_args; z [n][n_scen][2][ncol] or NULL; iters or NULL; rho and mu_scale are not read
    double s_max;
    double* speed;           // [n][n_scen][4]: s_lo, s_lo_out, s_hi, s_hi_out
    double* y;               // [n][n_scen][2][6 nb] or NULL
};

// ---- the decisions of one job -----------------------------------------------------------------------------------------------------------
enum { UPR_SPD_REST = 0, UPR_SPD_TOP = 1, UPR_SPD_NOMINAL = 2, UPR_SPD_DESCENT = 3, UPR_SPD_LOWER = 4, UPR_SPD_UPPER = 5, UPR_SPD_DONE = 6 };
#define UPR_SPD_K (1ull << UPR_BAL_BISECT)
struct upr_spd_ctl {
    unsigned long long k;                            // the grid point under evaluation
    unsigned long long lo_in, lo_out, hi_in, hi_out;   // accepted / rejected neighbours of the lower and of the upper end
    unsigned long long dl, dh;                       // the interval of the descent search
    unsigned long long k1;                           // the nominal speed on the grid
    int phase, left;                                 // left: halvings the descent search has left
    bool e0, eM, found;                              // F(0), F(2^32), an accepted speed exists
};
static UPR_HDI double upr_spd_at(unsigned long long k, double s_max) { return s_max * ((double)k * (1.0 / (double)UPR_SPD_K)); }
static UPR_HDI void upr_spd_begin(upr_spd_ctl& c, double s_max) {
    c.k = 0; c.lo_in = 0; c.lo_out = 0; c.hi_in = 0; c.hi_out = UPR_SPD_K; c.dl = 0; c.dh = UPR_SPD_K;
    c.k1 = (unsigned long long)((double)UPR_SPD_K / s_max);
    c.phase = UPR_SPD_REST; c.left = UPR_BAL_BISECT; c.e0 = false; c.eM = false; c.found = false;
}
// the next point of the two bisections, or the end of the job
static UPR_HDI void upr_spd_pick(upr_spd_ctl& c) {
    if (c.phase == UPR_SPD_LOWER) {
        if (c.lo_in - c.lo_out > 1) { c.k = (c.lo_in + c.lo_out) >> 1; return; }
        c.phase = UPR_SPD_UPPER;
    }
    if (c.phase == UPR_SPD_UPPER) {
        if (!c.eM && c.hi_out - c.hi_in > 1) { c.k = (c.hi_in + c.hi_out) >> 1; return; }
        c.phase = UPR_SPD_DONE;
    }
}
// The answer at c.k: ok -- accepted; g -- the slope r' (b1 - b0), read in the descent search on a rejected point only.  Returns the
// ends whose certificate this evaluation carries (bit 0: the lower end, bit 1: the upper end; z if ok, y if not) and moves on.
static UPR_HDI unsigned upr_spd_feed(upr_spd_ctl& c, bool ok, double g) {
    unsigned ends = 0u;
    const unsigned long long k = c.k;
    switch (c.phase) {
    case UPR_SPD_REST:
        c.e0 = ok; c.found = ok;
        ends = ok ? 3u : 1u;          // (accepted: s_lo = 0, and s_hi = 0 until a larger speed is accepted)
        c.phase = UPR_SPD_TOP; c.k = UPR_SPD_K;
        break;
    case UPR_SPD_TOP:
        c.eM = ok;
        if (ok) { c.hi_in = k; ends = c.e0 ? 2u : 3u; } else ends = 2u;
        if (c.e0) { c.phase = ok ? UPR_SPD_DONE : UPR_SPD_UPPER; upr_spd_pick(c); }
        else if (c.k1 > 0) { c.phase = UPR_SPD_NOMINAL; c.k = c.k1; }
        else if (ok) { c.found = true; c.lo_in = k; c.phase = UPR_SPD_LOWER; upr_spd_pick(c); }
        else { c.phase = UPR_SPD_DESCENT; c.k = (c.dl + c.dh) >> 1; }
        break;
    case UPR_SPD_NOMINAL:
        if (ok) { c.found = true; c.lo_in = k; if (!c.eM) c.hi_in = k; ends = c.eM ? 1u : 3u; c.phase = UPR_SPD_LOWER; upr_spd_pick(c); }
        else if (c.eM) { c.found = true; c.lo_in = UPR_SPD_K; c.phase = UPR_SPD_LOWER; upr_spd_pick(c); }
        else { c.phase = UPR_SPD_DESCENT; c.k = (c.dl + c.dh) >> 1; }
        break;
    case UPR_SPD_DESCENT:
        if (ok) { c.found = true; c.lo_in = k; c.hi_in = k; ends = 3u; c.phase = UPR_SPD_LOWER; upr_spd_pick(c); break; }
        if (g < 0.0) c.dl = k; else c.dh = k;
        --c.left;
        if (c.left == 0 || c.dh - c.dl <= 1) c.phase = UPR_SPD_DONE;
        else c.k = (c.dl + c.dh) >> 1;
        break;
    case UPR_SPD_LOWER:
        if (ok) c.lo_in = k; else c.lo_out = k;
        ends = 1u;
        upr_spd_pick(c);
        break;
    case UPR_SPD_UPPER:
        if (ok) c.hi_in = k; else c.hi_out = k;
        ends = 2u;
        upr_spd_pick(c);
        break;
    default: break;
    }
    return ends;
}
static UPR_HDI void upr_spd_answer(const upr_spd_ctl& c, double s_max, double* out) {
    if (!c.found) { out[0] = INFINITY; out[1] = 0.0; out[2] = -INFINITY; out[3] = s_max; return; }
    out[0] = upr_spd_at(c.lo_in, s_max);
    out[1] = c.e0 ? 0.0 : upr_spd_at(c.lo_out, s_max);
    out[2] = upr_spd_at(c.hi_in, s_max);
    out[3] = c.eM ? INFINITY : upr_spd_at(c.hi_out, s_max);
}
// the state kernel's record replayed s times faster: (C_we, s omega, s^2 alpha, s^2 a_ee)
static UPR_HDI void upr_spd_scale(const double* st, double s, double (&out)[UPR_BAL_ST]) {
    const double s2 = s * s;
    for (int i = 0; i < 9; ++i) out[i] = st[i];
    for (int i = 0; i < 3; ++i) { out[9 + i] = s * st[9 + i]; out[12 + i] = s2 * st[12 + i]; out[15 + i] = s2 * st[15 + i]; }
}
// ---- the job of a one-parameter margin on the grid -----------------------------------------------------------------------------------
// upr_spd_ctl decides on an integer grid and does not know what the grid parametrises.  A POLICY names the places where two
// quantities on it differ (this one and the path-acceleration margin of upr_pathacc.h) -- the grid point -> parameter map, the record
// transform and the two records the slope is taken between:
//   begin(c)                  upr_spd_begin with the nominal point of the quantity;
//   record(st, pt, k, out)    the record of point pt at grid point k;
//   slope_ends(st, pt, a, b)  the two records the slope of rho^2 / 2 is taken between, g = r' (b(b) - b(a));
//   answer(c, out)            the four doubles of the job from the neighbours the decisions ended on.
struct upr_spd_replay {   // this quantity: the replay speed s(k) = s_max k 2^-32
    double s_max;
    UPR_HDI void begin(upr_spd_ctl& c) const { upr_spd_begin(c, s_max); }
    UPR_HDI void record(const double* st, long long, unsigned long long k, double (&out)[UPR_BAL_ST]) const { upr_spd_scale(st, upr_spd_at(k, s_max), out); }
    UPR_HDI void slope_ends(const double* st, long long, double (&s0)[UPR_BAL_ST], double (&s1)[UPR_BAL_ST]) const {
        upr_spd_scale(st, 0.0, s0);
        upr_spd_scale(st, 1.0, s1);
    }
    UPR_HDI void answer(const upr_spd_ctl& c, double* out) const { upr_spd_answer(c, s_max, out); }
};
// r' (b1 - b0) of one body: its rows of the right-hand side at s = 1 and at rest through the rhs routine
static UPR_HDI double upr_spd_slope1(const upr_problem* P, const double* st, const double* bpk, double eq_scale, const double* r) {
    double s0[UPR_BAL_ST], s1[UPR_BAL_ST], b0[6], b1[6];
    upr_spd_scale(st, 0.0, s0);
    upr_spd_scale(st, 1.0, s1);
    upr_bal_rhs1(P, s0, bpk, eq_scale, b0);
    upr_bal_rhs1(P, s1, bpk, eq_scale, b1);
    double g = 0.0;
    for (int c = 0; c < 6; ++c) g += r[c] * (b1[c] - b0[c]);
    return g;
}
// ... and between the two ends a policy names
template <class POL>
static UPR_HDI double upr_spd_slope1(const POL& pol, const upr_problem* P, const double* st, long long pt, const double* bpk, double eq_scale, const double* r) {
    double s0[UPR_BAL_ST], s1[UPR_BAL_ST], b0[6], b1[6];
    pol.slope_ends(st, pt, s0, s1);
    upr_bal_rhs1(P, s0, bpk, eq_scale, b0);
    upr_bal_rhs1(P, s1, bpk, eq_scale, b1);
    double g = 0.0;
    for (int c = 0; c < 6; ++c) g += r[c] * (b1[c] - b0[c]);
    return g;
}

// ---- a wave per job ------------------------------------------------------------------------------------------------------------------
// A: the jobs; out [n][n_scen][4]; y [n][n_scen][2][6 nb] or NULL
template <class POL>
static UPR_HDI void upr_bal_grid_job(const upr_ctx& ctx, const upr_bal_args& A, const POL& pol, double* out, double* y, const upr_bal_dims& L, long long job,
                                     double* W) {
    const upr_problem* P = A.P;
    const long long pt = job / A.n_scen;
    const int sc = (int)(job - pt * A.n_scen);
    const double* bp = A.params + (size_t)10 * P->nb * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const double* st = A.st + (size_t)pt * UPR_BAL_ST;
    double* zo = A.z ? A.z + (size_t)job * 2 * L.ncol : nullptr;
    double* yo = y ? y + (size_t)job * 2 * L.m : nullptr;
    double* r = W + L.o_r;
    // the slope's partial sums, one per body, in the s vector of the projection (mp = min(6 nb, ncol) doubles, free once the
    // projection has returned): needs nb <= mp, which holds whenever every body has a contact (ncol >= nc >= nb); a shape with fewer
    // columns than bodies would run on into the y vector, still inside the workspace and also free here
    double* part = W + L.o_s;
    const int cap = upr_bal_iter_cap(L.ncol);
    if (zo) UPR_FOR(j, L.ncol) { zo[j] = 0.0; zo[L.ncol + j] = 0.0; }
    if (yo) UPR_FOR(e, L.m) { yo[e] = 0.0; yo[L.m + e] = 0.0; }
    upr_spd_ctl c;
    pol.begin(c);
    int total = 0;
    while (c.phase != UPR_SPD_DONE) {
        double ss[UPR_BAL_ST];
        pol.record(st, pt, c.k, ss);
        UPR_WSYNC();   // (the previous evaluation, or the previous job of this wave, is done with the workspace)
        upr_bal_rhs(ctx, P, ss, bp, A.eq_scale, W + L.o_b);
        int np, it; double bnorm;
        const double rho = upr_bal_project(ctx, P, L, bp, A.eq_scale, upr_bal_mu_one(), W, &np, &it, &bnorm);
        total += it;
        const bool ok = rho <= UPR_BAL_FEAS * (bnorm > 1.0 ? bnorm : 1.0);
        double g = 0.0;
        if (!ok && c.phase == UPR_SPD_DESCENT) {
            // a body per lane, then every lane adds the bodies in their order (the s vector of the projection is free by now)
            UPR_WSYNC();
            UPR_FOR(k, P->nb) part[k] = upr_spd_slope1(pol, P, st, pt, bp + 10 * k, A.eq_scale, r + 6 * k);
            UPR_WSYNC();
            for (int k = 0; k < P->nb; ++k) g += part[k];
        }
        const unsigned ends = upr_spd_feed(c, ok, g);
        if (ok) {
            if (zo) for (int e = 0; e < 2; ++e) if ((ends >> e) & 1u) upr_bal_put_z(ctx, L, W, np, zo + (size_t)e * L.ncol);
        } else if (yo && ends) {
            if (it < cap) upr_bal_polish(ctx, L, W, np);
            for (int e = 0; e < 2; ++e) if ((ends >> e) & 1u) UPR_FOR(i, L.m) yo[(size_t)e * L.m + i] = r[i];
        }
    }
    if (ctx.tid == 0) {
        pol.answer(c, out + (size_t)job * 4);
        if (A.iters) A.iters[job] = total;
    }
}
static UPR_HDI void upr_bal_speed_job(const upr_ctx& ctx, const upr_spd_args& S, const upr_bal_dims& L, long long job, double* W) {
    upr_bal_grid_job(ctx, S.J, upr_spd_replay{S.s_max}, S.speed, S.y, L, job, W);
}

// ---- one-body arrangements: a lane per job ----------------------------------------------------------------------------------------------
// one copy of the projection's code for all evaluations, as upr_bal_margin_job1
template <class POL>
static UPR_HDI void upr_bal_grid_job1(const upr_bal_args& A, const POL& pol, double* out, double* y, const upr_bal_dims& L, long long job) {
    const upr_problem* P = A.P;
    const long long pt = job / A.n_scen;
    const int sc = (int)(job - pt * A.n_scen);
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const double* st = A.st + (size_t)pt * UPR_BAL_ST;
    double* zo = A.z ? A.z + (size_t)job * 2 * L.ncol : nullptr;
    double* yo = y ? y + (size_t)job * 12 : nullptr;
    if (zo) for (int j = 0; j < 2 * L.ncol; ++j) zo[j] = 0.0;
    if (yo) for (int e = 0; e < 12; ++e) yo[e] = 0.0;
    upr_spd_ctl c;
    pol.begin(c);
    int total = 0;
    while (c.phase != UPR_SPD_DONE) {
        double ss[UPR_BAL_ST], b[6];
        pol.record(st, pt, c.k, ss);
        upr_bal_rhs1(P, ss, bp, A.eq_scale, b);
        double bb2 = 0.0;
        for (int e = 0; e < 6; ++e) bb2 += b[e] * b[e];
        const double bnorm = sqrt(bb2), s1 = bnorm > 1.0 ? bnorm : 1.0;
        double r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
        int pidx[UPR_BAL1_MP], np;
        const int it = upr_bal_project1(P, L, bp, A.eq_scale, upr_bal_mu_one(), b, UPR_BAL_TOL * s1, r, zp, pidx, np, pc, G);
        total += it;
        double rr = 0.0;
        for (int e = 0; e < 6; ++e) rr += r[e] * r[e];
        const bool ok = sqrt(rr) <= UPR_BAL_FEAS * s1;
        const double g = (!ok && c.phase == UPR_SPD_DESCENT) ? upr_spd_slope1(pol, P, st, pt, bp, A.eq_scale, r) : 0.0;
        const unsigned ends = upr_spd_feed(c, ok, g);
        if (ok) {
            if (zo) for (int e = 0; e < 2; ++e) if ((ends >> e) & 1u) upr_bal_put_z1(L.ncol, zp, pidx, np, zo + (size_t)e * L.ncol);
        } else if (yo && ends) {
            if (it < upr_bal_iter_cap(L.ncol)) upr_bal_polish1(pc, G, np, r);
            for (int e = 0; e < 2; ++e) if ((ends >> e) & 1u) for (int i = 0; i < 6; ++i) yo[6 * e + i] = r[i];
        }
    }
    pol.answer(c, out + (size_t)job * 4);
    if (A.iters) A.iters[job] = total;
}
// The lane form of the speed margin keeps a body of its own: routed through upr_bal_grid_job1 the compiler schedules the 256-VGPR
// kernel differently (equal size, other register assignment), and the speed kernels' code is to stay what it was.  The two differ in
// the three places the policy names and nowhere else.
static UPR_HDI void upr_bal_speed_job1(const upr_spd_args& S, const upr_bal_dims& L, long long job) {
    const upr_bal_args& A = S.J;
    const upr_problem* P = A.P;
    const long long pt = job / A.n_scen;
    const int sc = (int)(job - pt * A.n_scen);
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const double* st = A.st + (size_t)pt * UPR_BAL_ST;
    double* zo = A.z ? A.z + (size_t)job * 2 * L.ncol : nullptr;
    double* yo = S.y ? S.y + (size_t)job * 12 : nullptr;
    if (zo) for (int j = 0; j < 2 * L.ncol; ++j) zo[j] = 0.0;
    if (yo) for (int e = 0; e < 12; ++e) yo[e] = 0.0;
    upr_spd_ctl c;
    upr_spd_begin(c, S.s_max);
    int total = 0;
    while (c.phase != UPR_SPD_DONE) {
        double ss[UPR_BAL_ST], b[6];
        upr_spd_scale(st, upr_spd_at(c.k, S.s_max), ss);
        upr_bal_rhs1(P, ss, bp, A.eq_scale, b);
        double bb2 = 0.0;
        for (int e = 0; e < 6; ++e) bb2 += b[e] * b[e];
        const double bnorm = sqrt(bb2), s1 = bnorm > 1.0 ? bnorm : 1.0;
        double r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
        int pidx[UPR_BAL1_MP], np;
        const int it = upr_bal_project1(P, L, bp, A.eq_scale, upr_bal_mu_one(), b, UPR_BAL_TOL * s1, r, zp, pidx, np, pc, G);
        total += it;
        double rr = 0.0;
        for (int e = 0; e < 6; ++e) rr += r[e] * r[e];
        const bool ok = sqrt(rr) <= UPR_BAL_FEAS * s1;
        const double g = (!ok && c.phase == UPR_SPD_DESCENT) ? upr_spd_slope1(P, st, bp, A.eq_scale, r) : 0.0;
        const unsigned ends = upr_spd_feed(c, ok, g);
        if (ok) {
            if (zo) for (int e = 0; e < 2; ++e) if ((ends >> e) & 1u) upr_bal_put_z1(L.ncol, zp, pidx, np, zo + (size_t)e * L.ncol);
        } else if (yo && ends) {
            if (it < upr_bal_iter_cap(L.ncol)) upr_bal_polish1(pc, G, np, r);
            for (int e = 0; e < 2; ++e) if ((ends >> e) & 1u) for (int i = 0; i < 6; ++i) yo[6 * e + i] = r[i];
        }
    }
    upr_spd_answer(c, S.s_max, S.speed + (size_t)job * 4);
    if (A.iters) A.iters[job] = total;
}

// ---- the knots of a plan ----------------------------------------------------------------------------------------------------------------
// speed [B][nk][n_scen][4] -> window [B][n_scen][2]: the largest s_lo and the smallest s_hi over the knots of an instance; knot
// likewise: the first knot that attains each.  One output per call, o = (instance n_scen + scenario) 2 + end, looping over the
// knots: no atomics.
static UPR_HDI void upr_bal_speed_window(const double* speed, int nk, int n_scen, long long o, double* window, int* knot) {
    const int end = (int)(o & 1);
    const long long bs = o >> 1, b = bs / n_scen, sc = bs - b * n_scen;
    const double* src = speed + ((size_t)b * nk * n_scen + sc) * 4 + 2 * end;
    double w = src[0]; int kw = 0;
    for (int k = 1; k < nk; ++k) {
        const double v = src[(size_t)k * n_scen * 4];
        if (end == 0 ? v > w : v < w) { w = v; kw = k; }
    }
    window[o] = w;
    if (knot) knot[o] = kw;
}
// the largest s with lb <= s^p v <= ub; +inf for v = 0
static UPR_HDI double upr_spd_limit_of(double v, double lb, double ub, int p) {
    if (v == 0.0) return INFINITY;
    const double q = v > 0.0 ? ub / v : lb / v, c = q > 0.0 ? q : 0.0;
    return p == 1 ? c : p == 2 ? sqrt(c) : cbrt(c);
}
// the limit speed of one instance: xs [nk][nx] = (q, v, a, ..), us [nk - 1][nu] = (jerk, ..) against the boxes of the problem
static UPR_HDI double upr_bal_speed_limit(const upr_problem* P, int nk, int nx, int nu, const double* xs, const double* us) {
    const int nq = P->nq;
    double lim = INFINITY;
    for (int k = 0; k < nk; ++k) {
        for (int i = 0; i < nq; ++i) {
            const double lv = upr_spd_limit_of(xs[(size_t)k * nx + nq + i], P->x_lb[nq + i], P->x_ub[nq + i], 1);
            const double la = upr_spd_limit_of(xs[(size_t)k * nx + 2 * nq + i], P->x_lb[2 * nq + i], P->x_ub[2 * nq + i], 2);
            lim = lv < lim ? lv : lim;
            lim = la < lim ? la : lim;
            if (k + 1 < nk) {
                const double lu = upr_spd_limit_of(us[(size_t)k * nu + i], P->u_lb[i], P->u_ub[i], 3);
                lim = lu < lim ? lu : lim;
            }
        }
    }
    return lim;
}

#ifndef UPR_HOST_EMU
// one wave per workgroup, jobs dealt round robin (as upr_bal_margin_kernel)
__global__ __launch_bounds__(64) void upr_bal_speed_kernel(upr_spd_args S, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_speed_job(ctx, S, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_speed1_kernel(upr_spd_args S, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_speed_job1(S, L, job);
}
// one lane per (instance, scenario, end); the lanes past nout, one per instance, compute the limit speed (limit may be NULL)
__global__ __launch_bounds__(64) void upr_bal_speed_plan_kernel(const upr_problem* P, const double* speed, int nk, int n_scen, long long nout, int B,
                                                                int nx, int nu, const double* xs, const double* us, double* window, int* knot,
                                                                double* limit) {
    const long long o = (long long)blockIdx.x * 64 + threadIdx.x;
    if (o < nout) upr_bal_speed_window(speed, nk, n_scen, o, window, knot);
    else if (limit && o - nout < B) {
        const long long b = o - nout;
        limit[b] = upr_bal_speed_limit(P, nk, nx, nu, xs + (size_t)b * nk * nx, us + (size_t)b * (nk - 1) * nu);
    }
}
#endif
