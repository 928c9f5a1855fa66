// upr_vf_nu_emu.cpp -- TEST-ONLY host emulation (one thread per workgroup, -DUPR_HOST_EMU) of the equality-multiplier paths of
// upright_amd/csrc/upr_value.h: the copy of the QP's nu the cost-to-go kernel keeps (upr_vf_args::nu_out) and the nu(t) query
// (upr_vfq_args::nu / nu_q).  Next to tests/emu/upr_vf_emu.cpp, which emulates the QP with its export and the cost-to-go itself;
// never part of libupright_mi.so.
#define UPR_HOST_EMU
#include <vector>

#include "../../upright_amd/csrc/upr_common.h"
#include "../../upright_amd/csrc/upr_kin.h"
#include "../../upright_amd/csrc/upr_qp.h"
#include "../../upright_amd/csrc/upr_value.h"

extern "C" {

// cost-to-go kernel body with the multiplier copy: the arguments of emu_vf_cost_to_go (upr_vf_emu.cpp) and nu_out[B][N][ne]
void emu_vfnu_cost_to_go(const upr_problem* P, int B, const double* xs, const double* us, const double* lin, const double* Df,
                         const double* ws, long ws_stride, const double* mult, long mult_stride, const int* offs,
                         double* Pk, double* pk, double* J, double* X, double* nu_out) {
    upr_vf_args A;
    A.P = P; A.d = upr_make_dims(P); A.d.ws_stride = (int)ws_stride; A.xs = xs; A.us = us; A.lin = lin; A.Df = Df; A.ws = ws;
    A.mult = mult; A.mult_stride = mult_stride;
    A.o_pi = offs[0]; A.o_nu = offs[1]; A.o_lam = offs[2]; A.o_t = offs[3]; A.o_sig = offs[4]; A.o_tau = offs[5]; A.o_gam = offs[6];
    A.Pk = Pk; A.pk = pk; A.J = J; A.X = X; A.nu_out = nu_out;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> L(upr_vf_lds_layout(A.d).total + 16, std::nan(""));
    for (int b = 0; b < B; ++b) upr_vf_instance(ctx, A, b, L.data());
}

// the multiplier query alone (x == NULL): nu_q[n][ne] at (inst, t) from nu[B][N][ne]; t0[B]: time of knot 0
void emu_vfnu_query(const upr_problem* P, int n, const int* inst, const double* t, const double* t0, const double* nu, double* nu_q) {
    upr_vfq_args A;
    A.d = upr_make_dims(P); A.dt = P->dt; A.n = n; A.inst = inst; A.t = t; A.x = nullptr; A.t0 = t0;
    A.Pk = nullptr; A.pk = nullptr; A.J = nullptr; A.X = nullptr; A.V = nullptr; A.dV = nullptr;
    A.nu = nu; A.nu_q = nu_q;
    upr_ctx ctx; ctx.tid = 0; ctx.nt = 1;
    std::vector<double> L(4 * UPR_MAX_NX, std::nan(""));
    for (int p = 0; p < n; ++p) upr_vf_query_point(ctx, A, p, L.data());
}
}
