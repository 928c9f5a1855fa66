// upr_vf_emu.cpp -- TEST-ONLY host emulation (one thread per workgroup, -DUPR_HOST_EMU) of the value-function kernels of
// upright_amd/csrc/upr_value.h and of the production QP kernel WITH its multiplier export (upr_qp_args::kkt: multipliers, slacks
// and, for the SOFT instantiations, the slack pairs of the softened rows).  Next to tests/emu/upr_emu.cpp, which runs the QP kernels
// without the export; never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_qp.h"
#include "../../upright_amd/csrc/upr_qp3.h"
#include "../../upright_amd/csrc/upr_qp_select.h"
#include "../../upright_amd/csrc/upr_value.h"

extern "C" {

long emu_vf_kkt_doubles(const upr_problem* P) { return (long)upr_kkt_doubles(upr_make_dims(P)); }

// where the primal-dual point of the QP lies, out[0..7] = o_pi, o_nu, o_lam, o_t, o_sig, o_tau, o_gam (-1: the problem has no
// softened inequality rows), ni: kernel 3 in the export buffer of the production kernel, kernel 1 in the generic kernel's workspace
void emu_vf_offsets(const upr_problem* P, int kernel, int* out) {
    const upr_dims d = upr_make_dims(P);
    upr_qp_choice s;   // (the selection record's offsets for that structure: upr_qp_select.h)
    if (kernel == 3) upr_qp_point_exported(s, *P, d); else upr_qp_fill_generic(s, d);
    out[0] = s.o_pi; out[1] = s.o_nu; out[2] = s.o_lam; out[3] = s.o_t; out[4] = s.o_sig; out[5] = s.o_tau; out[6] = s.o_gam;
    out[7] = d.ni_stage;
}

// production QP kernel body with the export: kkt[B][kkt_stride].  ws == NULL: the workspace (doubles) an instance needs; -1: no
// instantiation for the shape here (the ones the value-function tests use)
long emu_vf_qp3(const upr_problem* P, int B, const double* xs, const double* us, const double* x0, const double* lin, const double* Df,
                double* ws, long ws_stride, double* stats, double* kkt, long kkt_stride) {
    upr_qp_args A;
    A.P = P; A.d = upr_make_dims(P); A.xs = xs; A.us = us; A.x0 = x0; A.lin = lin; A.Df = Df; A.ws = ws; A.stats = stats; A.prof = nullptr;
    A.kkt = kkt; A.kkt_stride = (int)kkt_stride;
    const bool softb = upr_qp_needs_soft(*P, A.d);
#define EMU_QP3(a, b, c, e, n, sf, cond) if (P->nq == a && P->nb == b && P->nc == c && P->nf == e && P->N == n && (cond)) { \
        typedef upr_qp3_cfg<a, b, c, e, n, 1, true, sf, false> C; \
        if (!ws) return (long)upr_qp3_ws<C>::total; \
        A.d.ws_stride = (int)ws_stride; \
        upr_ctx ctx; ctx.tid = 0; ctx.nt = 1; \
        std::vector<double> L(upr_qp3_lds<C>::total + 16, std::nan("")); \
        for (int bb = 0; bb < B; ++bb) upr_qp3_solve<C>(ctx, A, bb, L.data()); \
        return 0; }
    EMU_QP3(9, 1, 4, 3, 20, false, !softb)
    EMU_QP3(9, 1, 4, 3, 20, true, softb)
    EMU_QP3(9, 8, 32, 1, 20, true, true)
#undef EMU_QP3
    return -1;
}

long emu_vf_lds_doubles(const upr_problem* P) { return (long)upr_vf_lds_layout(upr_make_dims(P)).total; }

// cost-to-go kernel body: offs = o_pi, o_nu, o_lam, o_t, o_sig, o_tau, o_gam into mult[B][mult_stride]
void emu_vf_cost_to_go(const upr_problem* P, int B, const double* xs, const double* us, const double* lin, const double* Df,
                       const double* ws, long ws_stride, const double* mult, long mult_stride, const int* offs,
                       double* Pk, double* pk, double* J, double* X) {
    upr_vf_args A;
    A.P = P; A.d = upr_make_dims(P); A.d.ws_stride = (int)ws_stride; A.xs = xs; A.us = us; A.lin = lin; A.Df = Df; A.ws = ws;
    A.mult = mult; A.mult_stride = mult_stride;
    A.o_pi = offs[0]; A.o_nu = offs[1]; A.o_lam = offs[2]; A.o_t = offs[3]; A.o_sig = offs[4]; A.o_tau = offs[5]; A.o_gam = offs[6];
    A.Pk = Pk; A.pk = pk; A.J = J; A.X = X;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    // LDS is not zero on the device: poison the scratch so that a read before the first write cannot pass unnoticed
    std::vector<double> L(upr_vf_lds_layout(A.d).total + 16, std::nan(""));
    for (int b = 0; b < B; ++b) upr_vf_instance(ctx, A, b, L.data());
}

void emu_vf_query(const upr_problem* P, int n, const int* inst, const double* t, const double* x, const double* t0,
                  const double* Pk, const double* pk, const double* J, const double* X, double* V, double* dV) {
    upr_vfq_args A;
    A.d = upr_make_dims(P); A.dt = P->dt; A.n = n; A.inst = inst; A.t = t; A.x = x; A.t0 = t0; A.Pk = Pk; A.pk = pk; A.J = J; A.X = X; A.V = V; A.dV = dV;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> L(4 * UPR_MAX_NX, std::nan(""));
    for (int p = 0; p < n; ++p) upr_vf_query_point(ctx, A, p, L.data());
}
}
