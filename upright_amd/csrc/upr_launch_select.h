// upr_launch_select.h -- which linearisation kernel and which line-search kernel a handle runs, decided ONCE (upr_batch_create)
// and kept as a value, as upr_qp_select.h does for the QP kernel.  Everything here is host arithmetic on the problem, its
// dimensions and the knobs; the only per-launch quantity is the grid.  upr_api_launch.hip resolves a choice to a kernel by expanding the
// lists below, and the host emulation under tests/emu compiles this file with g++ to run the same rules.  (It is not part of a
// kernel's source: the run-time instantiation's cache key does not hash it.)
#pragma once
#include <cstddef>
#include <cstdio>

#include "upr_common.h"
#include "upr_linearize.h"
#include "upr_linearize2.h"
#include "upr_linesearch.h"

#ifndef UPR_LIN_ROW_PASSES_DEFAULT
#define UPR_LIN_ROW_PASSES_DEFAULT 2
#endif

// THE instantiations of upr_linearize_kernel<NQ, ...> (NQ 6 and 9 each): X(USE_MFMA, OCC, ORI, NPASS).  The multi-pass form and
// the three-row-pass form are one instantiation.  upr_linearize2_kernel<NQ> stands beside them.
#define UPR_LIN_FORMS(X) \
    X(true, 2, true, 1) X(false, 2, true, 1) X(false, 2, false, 1) X(true, 3, false, 1) X(true, 4, false, 1) \
    X(true, 2, false, UPR_LIN_PASSES) X(true, 2, false, 2) X(true, 2, false, 1)
// ... and of upr_linesearch_kernel<NQ, 128, ...>, each with STAGE true and false: X(NFM, NBM, EXACT, OBS)
#define UPR_LS_FORMS(X) X(12, 1, true, false) X(12, 1, true, true) X(12, 1, false, true) X(3 * UPR_MAX_CONTACTS, UPR_MAX_BODIES, false, true)

// the environment knobs of the two selections, as upr_batch_create reads them (the defaults are those of an empty environment)
struct upr_lin_knobs {
    bool mfma = true;                               // UPR_LIN_MFMA = 0: the instantiations without matrix instructions
    bool lin2 = true;                               // UPR_LIN2 = 0: upr_linearize_kernel also where upr_linearize2_kernel takes the shape
    int occ = 2;                                    // UPR_LIN_OCC = 3 | 4: workgroups per SIMD the kernel is bounded for (A/B runs)
    int row_passes = UPR_LIN_ROW_PASSES_DEFAULT;    // UPR_LIN_ROW_PASSES = 1 | 2 | 3: passes per workgroup with collision rows
};
struct upr_ls_knobs {
    int stage_full = -1;                            // UPR_LS_STAGE_FULL = 0 | 1 forces either form (A/B runs); -1: by the LDS footprint
};

struct upr_lin_choice {
    int kind = 1;                                   // 1: upr_linearize_kernel<nq, mfma, occ, ori, npass>; 2: upr_linearize2_kernel<nq>
    int nq = 0;
    bool mfma = true; int occ = 2; bool ori = false; int npass = 1;    // kind 1
    int kpw = 8;                                    // knots per workgroup
    size_t lds = 0;                                 // dynamic LDS of a workgroup, bytes
    bool too_large = false;                         // ... which exceeds 160 KiB: no launch
};
struct upr_ls_choice {
    int nq = 0;
    int nfm = 12, nbm = 1; bool exact = false, obs = true, stage = true;
    size_t lds = 0;
};

// upr_lin2_eligible on the arguments every launch of a handle carries: target orientations exactly when the problem has an
// orientation cost, the constant d g / d forces always
static inline bool upr_lin2_takes(bool has_orientation_cost) {
    static const double some = 0.0;
    upr_lin_args A{};
    A.way_q = has_orientation_cost ? &some : nullptr; A.Df = &some;
    return upr_lin2_eligible(A);
}

static inline upr_lin_choice upr_lin_plan(const upr_problem& P, const upr_dims& d, const upr_lin_knobs& k) {
    upr_lin_choice s;
    s.nq = P.nq;
    const bool ori = upr_has_orientation_cost(&P);
    // knots per workgroup: several passes (their value walk side by side) for the plain instantiation without collision rows
    // (the end-effector box rows come out of the position Jacobian in the last phase: they leave the layout as it is)
    const bool multi = UPR_LIN_ANALYTIC && !ori && k.mfma && k.occ == 2 && d.nsr == 0;
    // with collision rows (snapshot form, round 4: 156 instead of 480 doubles of LDS per knot for 16 spheres): UPR_LIN_ROW_PASSES
    // passes per workgroup (1, 2 or 3)
    const bool multi_rows = UPR_LIN_ANALYTIC && UPR_LIN_OBS_SNAP && !ori && k.mfma && k.occ == 2 && d.nsr > 0 && (k.row_passes == 2 || k.row_passes == 3);
    // no orientation cost: the one-round kernel of upr_linearize2.h, as many knots per workgroup as three workgroups per CU hold
    // in LDS and one tangent pass takes in one trip (28 for the headline shape: 768 workgroups)
    if (k.lin2 && upr_lin2_takes(ori) && k.mfma && k.occ == 2) {
        const upr_lin2_lay lay = upr_lin2_layout(d, P.n_sph);
        const int npre = ((UPR_LIN2_NPRE + 1) & ~1) + (d.nsr > 0 ? upr_lin2_table_doubles(P.n_sph) : 0);
        int kpw = (int)((UPR_LIN2_LDS_BUDGET - npre * sizeof(double)) / (lay.per * sizeof(double)));
        if (kpw > 256 / P.nq) kpw = 256 / P.nq;
        if (kpw > 64) kpw = 64;
        if (kpw >= 1) {
            s.kind = 2; s.kpw = kpw;
            s.lds = (size_t)(npre + kpw * lay.per) * sizeof(double);
            return s;
        }
    }
    s.kpw = 8 * (multi ? UPR_LIN_PASSES : (multi_rows ? k.row_passes : 1));
    s.lds = (size_t)s.kpw * upr_lin_lds_doubles(d, P.n_sph) * sizeof(double) + sizeof(upr_problem) + 16;   // (+ the kernel's copy of the problem record)
    s.too_large = s.lds > 160 * 1024;
    // (rounds 1 - 2, one forward-mode walk per tangent lane: 2 -> 0.130 ms, 3 -> 0.142 ms, 4 -> 0.32 ms with spills; round 3, one value
    // walk per knot + closed-form tangents: 2 -> 0.091 ms, 3 -> 0.085 ms;
    // with the walks of three passes side by side: 2 -> 0.073 ms, 3 -> 0.095 ms)
    auto form = [&](bool mfma, int occ, bool o, int npass) { s.mfma = mfma; s.occ = occ; s.ori = o; s.npass = npass; };
    if (ori) form(k.mfma, 2, true, 1);   // end-effector cost with orientation weights
    else if (!k.mfma) form(false, 2, false, 1);
    else if (k.occ == 3) form(true, 3, false, 1);
    else if (k.occ == 4) form(true, 4, false, 1);
    else if (multi) form(true, 2, false, UPR_LIN_PASSES);
    else if (multi_rows) form(true, 2, false, k.row_passes);
    else form(true, 2, false, 1);
    return s;
}

static inline upr_ls_choice upr_ls_plan(const upr_problem& P, const upr_dims& d, const upr_ls_knobs& k) {
    upr_ls_choice s;
    s.nq = P.nq;
    s.lds = (size_t)upr_ls_lds_doubles(d) * sizeof(double) + sizeof(upr_problem) + 16;   // (+ the kernel's copy of the problem record)
    // Three staged copies (trajectory, step, trial trajectory) pay for the small shapes only: with one wave per workgroup the LDS
    // footprint IS the occupancy, and for the large input vectors it costs more than the uncoalesced reads it replaces
    // (r04, tools/r4_lin.sh: configs[2] 1.58 ms staged / 1.01 ms not, configs[3] 0.249 / 0.171; the headline shape, 40 KB
    // staged, stays).
    const bool stage_off = k.stage_full == 0 || (k.stage_full < 0 && s.lds > 41 * 1024);
    if (s.lds > 64 * 1024 || stage_off) {   // (also: long horizons of the large shapes, where three copies do not fit)
        s.stage = false;
        s.lds = (size_t)upr_ls_lds_doubles(d, false) * sizeof(double) + sizeof(upr_problem) + 16;
    }
    auto form = [&](int nfm, int nbm, bool exact, bool obs) { s.nfm = nfm; s.nbm = nbm; s.exact = exact; s.obs = obs; };
    // small shapes (one body, up to four frictional contacts): per-lane vectors sized for them
    // exactly the headline's contact structure (one body on the tray, four frictional contacts): every bound a constant
    if (d.nfc == 12 && d.nb == 1 && P.nf == 3 && P.nc == 4 && d.no == 0) form(12, 1, true, false);
    // ... the same with state rows: collision / projectile rows (configs[4], the obstacle experiments: round 5), the end-effector box
    // (a box-only problem skips the sphere walk: upr_ls_knot)
    else if (d.nfc == 12 && d.nb == 1 && P.nf == 3 && P.nc == 4) form(12, 1, true, true);
    else if (d.nfc <= 12 && d.nb == 1) form(12, 1, false, true);
    else form(3 * UPR_MAX_CONTACTS, UPR_MAX_BODIES, false, true);
    return s;
}

// the instantiation as rocprofv3 prints it (upr_batch_lin_kernel_name, upr_batch_ls_kernel_name); blocks: the workgroups of a launch
static inline void upr_lin_name(const upr_lin_choice& s, int blocks, char* buf, size_t n) {
    if (s.kind == 2) snprintf(buf, n, "upr_linearize2_kernel<%d> kpw=%d blocks=%d", s.nq, s.kpw, blocks);
    else snprintf(buf, n, "upr_linearize_kernel<%d, %s, %d, %s, %d>", s.nq, s.mfma ? "true" : "false", s.occ, s.ori ? "true" : "false", s.npass);
}
static inline void upr_ls_name(const upr_ls_choice& s, char* buf, size_t n) {
    snprintf(buf, n, "upr_linesearch_kernel<%d, 128, %d, %d, %s, %s, %s>", s.nq, s.nfm, s.nbm, s.exact ? "true" : "false", s.obs ? "true" : "false", s.stage ? "true" : "false");
}
