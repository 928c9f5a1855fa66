// upr_retime_rsv.h -- retiming with a reserve: the fastest time law on the speed lattice of upr_retime.h whose every end state still
// absorbs a given unplanned tray acceleration along given directions (the displacement of upr_disturb.h).
//
// The quantity.  Lattice, edges, d, dt, boxes, `common`, start / end, the dynamic programme and the outputs are upr_retime.h's; only the
// acceptance of an end state changes.  The caller also gives dirs [n_dir][6], rows u = (u_alpha, u_a) as in upr_disturb.h (1 <= n_dir <=
// UPR_DST_MAX_DIRS, finite, no row all zero), frame (0: world, 1: tray) and the reserve r >= 0 in the unit of upr_disturb.h's r.  With
// R = upr_pac_transform(st, vee, s, d) the record of an end state, the state is accepted iff, by the family's rule unchanged (rho of the
// cold projection <= UPR_BAL_FEAS max(|b|, 1)),
//
//     R itself is accepted, and, when r > 0, for every k the records upr_dst_transform(R, u_k, frame, +r) and
//     upr_dst_transform(R, u_k, frame, -r) are accepted.
//
// The tray frame uses R's own C_we, which the path transform does not touch.  The order is fixed (iters is compared bit for bit): the
// nominal record first, then k ascending, +r before -r; an end state stops at its first rejection; the departing state is finished
// before the arriving one is begun, and the arriving one is skipped when the departing one is rejected: at most 2 M (1 + 2 n_dir)
// projections per mask row.  With r = 0 no displaced record is evaluated: the evaluations are those of upr_bal_retime_job /
// upr_bal_retime_job1, one for one.
//
// What is claimed.  b is affine in (alpha, a_ee) and the cone is convex: up to the ball of the rule, acceptance at +r u_k and at -r u_k
// certifies the whole segment between them.  NOTHING is claimed for combinations of directions -- no different from the radius of
// upr_disturb.h, which is a minimum over the directions given.
//
// The kernels.  Jobs, their decoding (upr_ret_decode) and the single uint32 a job writes are upr_retime.h's; no atomics; the loops are
// bounded by M and n_dir.  One flattened loop walks (m', end, displacement), so a kernel holds ONE copy of the projection's code.  The
// directions are read from memory at every evaluation, not held.  The path kernel of upr_retime.h serves this quantity as it is.
#pragma once
#include "upr_retime.h"
#include "upr_disturb.h"

struct upr_ret_rsv_args {
    upr_ret_args T;          // as the retiming's
    const double* dirs;      // [n_dir][6]: (u_alpha, u_a)
    int n_dir, frame;        // frame 0: world, 1: tray
    double reserve;          // r >= 0
};

// where the flattened loop of a job stands: the edge m -> mp, its end (0 departing, 1 arriving), the record of that end (0 the nominal
// one, 1 + 2 k + (0 | 1): direction k at +r | -r)
struct upr_rsv_walk {
    int mp, arr, v;
    double d;
};
// the records of an end state: 1, or 1 + 2 n_dir with a reserve
static UPR_HDI int upr_rsv_records(const upr_ret_rsv_args& S) { return S.reserve > 0.0 ? 1 + 2 * S.n_dir : 1; }
// before the nominal record of a departing state: the edge's d; false: the edge does not exist or a box cuts it
static UPR_HDI bool upr_rsv_edge(const upr_ret_args& S, long long pt, double sm, double sp, double& d) {
    d = upr_ret_accel(sm, sp, S.h);
    bool go = sm + sp > 0.0;
    if (go && S.boxes) go = upr_ret_in_box(S.J.P, S.xs + (size_t)pt * S.nx, sm, d) && upr_ret_in_box(S.J.P, S.xs + (size_t)(pt + 1) * S.nx, sp, d);
    return go;
}
// the record the walk stands at
static UPR_HDI void upr_rsv_record(const upr_ret_rsv_args& S, long long pt, double sm, double sp, const upr_rsv_walk& w, double (&ss)[UPR_BAL_ST]) {
    const long long p = pt + w.arr;
    upr_pac_transform(S.T.J.st + (size_t)p * UPR_BAL_ST, S.T.vee + (size_t)p * 3, w.arr ? sp : sm, w.d, ss);
    if (w.v) {
        double t[UPR_BAL_ST];
        upr_dst_transform(ss, S.dirs + 6 * ((w.v - 1) >> 1), S.frame, ((w.v - 1) & 1) ? -S.reserve : S.reserve, t);
        for (int i = 0; i < UPR_BAL_ST; ++i) ss[i] = t[i];
    }
}
// after a record: rejected -> the next edge; the last record of the departing state -> the arriving one; of the arriving one -> the bit
static UPR_HDI void upr_rsv_step(upr_rsv_walk& w, int nv, bool ok, unsigned& mask) {
    if (!ok) { ++w.mp; w.arr = 0; w.v = 0; return; }
    if (++w.v < nv) return;
    w.v = 0;
    if (w.arr) { mask |= 1u << w.mp; ++w.mp; w.arr = 0; }
    else w.arr = 1;
}

// ---- a wave per job ------------------------------------------------------------------------------------------------------------------
static UPR_HDI void upr_bal_retime_rsv_job(const upr_ctx& ctx, const upr_ret_rsv_args& S, const upr_bal_dims& L, long long job, double* W) {
    const upr_bal_args& A = S.T.J;
    const upr_problem* P = A.P;
    long long pt; int sc, m;
    upr_ret_decode(S.T, job, pt, sc, m);
    const double* bp = A.params + (size_t)10 * P->nb * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const double sm = S.T.speeds[m];
    const int nv = upr_rsv_records(S);
    unsigned mask = 0u;
    int total = 0;
    upr_rsv_walk w = {0, 0, 0, 0.0};
    while (w.mp < S.T.M) {
        const double sp = S.T.speeds[w.mp];
        if (!w.arr && !w.v && !upr_rsv_edge(S.T, pt, sm, sp, w.d)) { ++w.mp; continue; }
        double ss[UPR_BAL_ST];
        upr_rsv_record(S, pt, sm, sp, w, ss);
        UPR_WSYNC();   // (the previous evaluation, or the previous job of this wave, is done with the workspace)
        upr_bal_rhs(ctx, P, ss, bp, A.eq_scale, W + L.o_b);
        int np, it; double bnorm;
        const double rho = upr_bal_project(ctx, P, L, bp, A.eq_scale, upr_bal_mu_one(), W, &np, &it, &bnorm);
        total += it;
        upr_rsv_step(w, nv, rho <= UPR_BAL_FEAS * (bnorm > 1.0 ? bnorm : 1.0), mask);
    }
    if (ctx.tid == 0) {
        S.T.edges[job] = mask;
        if (A.iters) A.iters[job] = total;
    }
}

// ---- one-body arrangements: a lane per job ----------------------------------------------------------------------------------------------
static UPR_HDI void upr_bal_retime_rsv_job1(const upr_ret_rsv_args& S, const upr_bal_dims& L, long long job) {
    const upr_bal_args& A = S.T.J;
    const upr_problem* P = A.P;
    long long pt; int sc, m;
    upr_ret_decode(S.T, job, pt, sc, m);
    const double* bp = A.params + (size_t)10 * ((A.pdiv ? (pt / A.pdiv) * A.n_scen : 0) + sc);
    const double sm = S.T.speeds[m];
    const int nv = upr_rsv_records(S);
    unsigned mask = 0u;
    int total = 0;
    upr_rsv_walk w = {0, 0, 0, 0.0};
    while (w.mp < S.T.M) {
        const double sp = S.T.speeds[w.mp];
        if (!w.arr && !w.v && !upr_rsv_edge(S.T, pt, sm, sp, w.d)) { ++w.mp; continue; }
        double ss[UPR_BAL_ST], b[6];
        upr_rsv_record(S, pt, sm, sp, w, ss);
        upr_bal_rhs1(P, ss, bp, A.eq_scale, b);
        double bb2 = 0.0;
        for (int c = 0; c < 6; ++c) bb2 += b[c] * b[c];
        const double bnorm = sqrt(bb2), s1 = bnorm > 1.0 ? bnorm : 1.0;
        double r[6], zp[UPR_BAL1_MP], pc[UPR_BAL1_MP][6], G[UPR_BAL1_MP][UPR_BAL1_MP];
        int pidx[UPR_BAL1_MP], np;
        total += upr_bal_project1(P, L, bp, A.eq_scale, upr_bal_mu_one(), b, UPR_BAL_TOL * s1, r, zp, pidx, np, pc, G);
        double rr = 0.0;
        for (int c = 0; c < 6; ++c) rr += r[c] * r[c];
        upr_rsv_step(w, nv, sqrt(rr) <= UPR_BAL_FEAS * s1, mask);
    }
    S.T.edges[job] = mask;
    if (A.iters) A.iters[job] = total;
}

#ifndef UPR_HOST_EMU
// one wave per workgroup, jobs dealt round robin (as upr_bal_retime_kernel)
__global__ __launch_bounds__(64) void upr_bal_retime_rsv_kernel(upr_ret_rsv_args S, upr_bal_dims L, long long njobs) {
    extern __shared__ double upr_bal_lds[];
    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = 64;
    for (long long job = blockIdx.x; job < njobs; job += gridDim.x) upr_bal_retime_rsv_job(ctx, S, L, job, upr_bal_lds);
}
// one-body arrangements: one lane per job, no LDS
__global__ __launch_bounds__(64) void upr_bal_retime_rsv1_kernel(upr_ret_rsv_args S, upr_bal_dims L, long long njobs) {
    const long long job = (long long)blockIdx.x * 64 + threadIdx.x;
    if (job < njobs) upr_bal_retime_rsv_job1(S, L, job);
}
#endif
