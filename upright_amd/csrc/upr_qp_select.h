// upr_qp_select.h -- which QP kernel a handle runs, decided ONCE (upr_batch_create) and kept as a value.  Three structures: the
// generic kernel (upr_qp.h: any shape), the second structure (upr_qp2.h: UPR_QP2_SHAPES, no rows, no slacks) and the production
// kernel (upr_qp3.h) in the headline's instantiations, one of the list (upr_qp3_list.h) or one made at run time.  Everything here
// is host arithmetic on the problem and the knobs: upr_api.hip adds the launchers (upr_qp_resolve's visitor) and hiprtc, and the
// host emulation under tests/emu compiles this file with g++ to run the same rules.  (It is not part of a kernel's source: the
// run-time instantiation's cache key does not hash it.)
#pragma once
#include <cstdio>

#include "upr_common.h"
#include "upr_qp.h"
#include "upr_qp2.h"
#include "upr_qp3.h"
#include "upr_qp3_list.h"

// shapes the second-structure kernel is instantiated for: (nq, nb, nc, nf)
// -DUPR_HEADLINE_ONLY: experiment builds of the headline kernel (a tenth of the compile time); never the production library
#ifdef UPR_HEADLINE_ONLY
#define UPR_QP2_SHAPES(X) X(9, 1, 4, 3)
#else
#define UPR_QP2_SHAPES(X) X(9, 1, 4, 3) X(9, 1, 4, 1) X(6, 1, 4, 1) X(6, 1, 4, 3) X(9, 2, 8, 3)
#endif

enum { UPR_QP_STRUCT_GENERIC = 1, UPR_QP_STRUCT_SECOND = 2, UPR_QP_STRUCT_PRODUCTION = 3 };   // (the values of UPR_QP_KERNEL)
enum { UPR_QP_FROM_HEADLINE = 0, UPR_QP_FROM_LIST = 1, UPR_QP_FROM_RUN_TIME = 2 };             // production: where the instantiation comes from

// the environment knobs of the selection, as upr_batch_create reads them (the defaults are those of an empty environment)
struct upr_qp_knobs {
    int qp_kernel = 3;            // UPR_QP_KERNEL = 1 (generic) | 2 | 3: an older structure for A/B measurements and tests
    bool qp_generic = false;      // UPR_QP_GENERIC != 0: the generic kernel
    int qp3_jit = 1;              // UPR_QP3_JIT = 0: no run-time instantiation; 2: also for the listed shapes (diagnostic)
    bool qp_nt_set = false; int qp_nt = 0;                  // UPR_QP_NT: lanes of the headline's / the second structure's workgroup
    bool generic_nt_set = false; int generic_nt = 0;        // UPR_QP_GENERIC_NT: lanes of the generic kernel's workgroup
    int jit_nt = 256;             // UPR_JIT_NT: lanes of a run-time instantiation (128 | 256 | 512, experiments)
    bool fb_fused = true;         // UPR_FB_FUSED = 0: the feedback gains by the gather kernel also behind the production kernel
};

struct upr_qp_choice {
    int structure = UPR_QP_STRUCT_GENERIC;
    int source = UPR_QP_FROM_HEADLINE;                 // production only
    int cfg[8] = {0, 0, 0, 0, 0, 0, 0, 0};             // production only: (nq, nb, nc, nf, N, ROWS, SOFT, DENSE)
    int nt = 0;                                        // lanes per workgroup (second structure: as asked for; it runs 512 at 128)
    int ws_doubles = 0;                                // per-instance workspace the selected kernel needs
    int ws_stride = 0;                                 // the handle's workspace stride: the largest any selectable kernel needs
    bool fb_fused = false;                             // the kernel writes the feedback gains itself (upr_qp_args::fb)
    // where the primal-dual point of a QP with the multiplier export lies: the export buffer (upr_qp_args::kkt, stride
    // upr_kkt_doubles) or the instance workspace; o_sig = o_tau = o_gam = -1: the kernel carries no slack pairs for this problem
    bool exported = false;
    int stride = 0;
    int o_pi = 0, o_nu = 0, o_yN = 0, o_lam = 0, o_t = 0, o_sig = -1, o_tau = -1, o_gam = -1;
    char name[128] = "";                               // the instantiation, as rocprofv3 prints it (upr_batch_qp_kernel_name)
};

// ---- the rules ---------------------------------------------------------------------------------------------------------------
static inline bool upr_qp3_is_headline(const upr_problem& P) { return P.nq == 9 && P.nb == 1 && P.nc == 4 && P.nf == 3 && P.N == 20; }
// does the problem need a SOFT instantiation?  Slacks on its boxes, or slacks.poly_ineq with friction / state-polytopic rows
static inline bool upr_qp_needs_soft(const upr_problem& P, const upr_dims& d) {
    return P.soft_state_box || P.soft_input_box || (P.soft_poly && (d.np > 0 || d.no > 0));
}
// star arrangement: no two bodies share a contact point
static inline bool upr_qp_is_star(const upr_problem& P) {
    for (int i = 0; i < P.nc; ++i) if (P.contact_body1[i] >= 0) return false;
    return true;
}
// does instantiation (a, b, c, e, horizon n, rows, sf, dense) of UPR_QP3_EXTRA take this problem?  (The first match in list order
// is the one that runs: a SOFT problem without state-polytopic rows takes the instantiation without them.)
static inline bool upr_qp3_match(const upr_problem& P, const upr_dims& d, int a, int b, int c, int e, int n, bool rows, bool sf, bool dense) {
    return P.nq == a && P.nb == b && P.nc == c && P.nf == e && P.N == n && (rows || d.no == 0) && (sf || !upr_qp_needs_soft(P, d)) && (dense || upr_qp_is_star(P));
}
// THE expansion of the list: f(upr_qp3_cfg<...>()) for the first entry of UPR_QP3_EXTRA that takes the problem
// (tuple, where asked for: that entry as it is written in the list)
template <class F>
static inline bool upr_qp3_listed(const upr_problem& P, const upr_dims& d, F&& f, int* tuple = nullptr) {
#define X(a, b, c, e, n, rows, sf, dense) if (upr_qp3_match(P, d, a, b, c, e, n, rows, sf, dense)) { \
        const int t[8] = {a, b, c, e, n, rows, sf, dense}; \
        if (tuple) for (int i = 0; i < 8; ++i) tuple[i] = t[i]; \
        f(upr_qp3_cfg<a, b, c, e, n, 256, rows, sf, dense>()); return true; }
    UPR_QP3_EXTRA(X)
#undef X
    return false;
}
// ... and of the second structure's shapes: f(upr_qp2_dims<...>())
template <class F>
static inline bool upr_qp2_shape(const upr_problem& P, F&& f) {
#define X(a, b, c, e) if (P.nq == a && P.nb == b && P.nc == c && P.nf == e) { f(upr_qp2_dims<a, b, c, e>()); return true; }
    UPR_QP2_SHAPES(X)
#undef X
    return false;
}
struct upr_qp_no_visit { template <class T> void operator()(T) const {} };
// can the library's own production kernels take this problem?  0: no; otherwise UPR_QP_FROM_HEADLINE + 1 (hard boxes) or
// UPR_QP_FROM_LIST + 1
static inline int upr_qp3_variant(const upr_problem& P, const upr_dims& d, int* tuple = nullptr) {
    if (d.no > UPR_QP3_NOMAX) return 0;
    // (a hard equality the contact forces cannot span -- frictionless one-body arrangements: nf nc < 6 nb -- gets the proximal
    // treatment of upr_qp.h inside the kernel; multi-body shapes of that kind need soft_eq)
    if (d.nfc < d.ne && !P.soft_eq && P.nb > 1) return 0;
    if (upr_qp3_is_headline(P) && !upr_qp_needs_soft(P, d)) return UPR_QP_FROM_HEADLINE + 1;
    return upr_qp3_listed(P, d, upr_qp_no_visit(), tuple) ? UPR_QP_FROM_LIST + 1 : 0;
}
// can the production structure take this problem at all?  (what upr_qp3.h asserts or assumes; the LDS is checked after the compile)
static inline bool upr_qp3_jit_capable(const upr_problem& P, const upr_dims& d) {
    if (P.nq != 6 && P.nq != 9) return false;
    // (horizons beyond 64 knots: the far-array form of the kernel, upr_qp3_cfg::KFAR -- star arrangements without friction and rows)
    if (d.no > UPR_QP3_NOMAX || P.N < 2 || P.N > 128) return false;
    if (P.N > 64 && (!upr_qp_is_star(P) || P.nb < 2 || P.nf != 1 || d.no != 0)) return false;
    if (d.nfc < d.ne && !P.soft_eq && P.nb > 1) return false;
    return true;
}
// lanes of the generic kernel's workgroup.  Its LDS footprint (one knot's matrices) allows one or two workgroups per CU for the
// multi-body shapes, so the workgroup size IS the occupancy: 64 lanes left 3 of 4 SIMDs of a CU idle.  Chosen by the size of the
// per-knot phases (ne x nx, nx x nx, ne x ne items); UPR_QP_GENERIC_NT overrides it.
static inline int upr_qp_generic_nt(const upr_dims& d, const upr_qp_knobs& k) {
    if (k.generic_nt_set) return k.generic_nt;
    const int big = d.ne * d.nx > d.nx * d.nx ? d.ne * d.nx : d.nx * d.nx;
    return big >= 1024 ? 512 : (big >= 512 ? 256 : 64);
}
// the template arguments of a production instantiation, as rocprofv3 prints them
static inline void upr_qp3_cfg_text(const int* cfg, int nt, char* out, size_t n) {
    snprintf(out, n, "%d, %d, %d, %d, %d, %d, %s, %s, %s", cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], nt, cfg[5] ? "true" : "false", cfg[6] ? "true" : "false", cfg[7] ? "true" : "false");
}

// ---- step 1: structure, source and instantiation (no sizes yet) -----------------------------------------------------------------
// Precedence: the list comes first; a run-time instantiation is planned only where the list has nothing (or under UPR_QP3_JIT=2)
// and no other structure is forced; UPR_QP_KERNEL and UPR_QP_GENERIC apply after that.  run_time_ok = false: the plan of a
// handle whose run-time instantiation failed (the second or the generic structure takes it).
static inline upr_qp_choice upr_qp_plan(const upr_problem& P, const upr_dims& d, const upr_qp_knobs& k, bool run_time_ok = true) {
    upr_qp_choice s;
    // collision rows (state-polytopic inequalities) and slacks: rows the second-structure kernel does not have
    const bool plain = d.no == 0 && !(P.soft_state_box || P.soft_input_box || P.soft_poly || P.soft_eq);
    int listed[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int variant = upr_qp3_variant(P, d, listed);
    bool qp2 = upr_qp2_shape(P, upr_qp_no_visit()) && plain;
    const bool forced_other = k.qp_kernel < 3 || k.qp_generic;
    if (k.qp3_jit == 2) variant = 0;
    if (variant == 0 && !forced_other && k.qp3_jit != 0 && upr_qp3_jit_capable(P, d) && run_time_ok) variant = UPR_QP_FROM_RUN_TIME + 1;
    if (k.qp_kernel < 3) variant = 0;
    if (k.qp_kernel < 2) qp2 = false;
    if (k.qp_generic) { qp2 = false; variant = 0; }
    s.structure = variant ? UPR_QP_STRUCT_PRODUCTION : (qp2 ? UPR_QP_STRUCT_SECOND : UPR_QP_STRUCT_GENERIC);
    s.nt = variant ? 256 : 128;
    if (k.qp_nt_set) s.nt = k.qp_nt;
    if (variant) {
        s.source = variant - 1;
        if (s.source == UPR_QP_FROM_LIST) s.nt = 256;
        if (s.source == UPR_QP_FROM_RUN_TIME) s.nt = k.jit_nt;
        // the instantiation: a listed entry as it is written; otherwise what the problem asks for (the headline: hard rows, one body)
        const int asked[8] = {P.nq, P.nb, P.nc, P.nf, P.N, d.no > 0, upr_qp_needs_soft(P, d), !upr_qp_is_star(P)};
        for (int i = 0; i < 8; ++i) s.cfg[i] = (s.source == UPR_QP_FROM_LIST) ? listed[i] : asked[i];
        if (s.source == UPR_QP_FROM_HEADLINE) s.cfg[6] = s.cfg[7] = 0;
    } else if (!qp2) s.nt = upr_qp_generic_nt(d, k);
    s.fb_fused = variant != 0 && k.fb_fused;
    return s;
}

// ---- step 2: sizes, offsets and the name, one function per structure -------------------------------------------------------------
static inline void upr_qp_point_exported(upr_qp_choice& s, const upr_problem& P, const upr_dims& d) {
    const int nsl = (d.N + 1) * d.ni_stage;
    s.exported = true; s.stride = upr_kkt_doubles(d);
    s.o_pi = 0; s.o_nu = (d.N + 1) * d.nx; s.o_yN = s.o_nu + d.N * d.ne; s.o_lam = s.o_yN + d.neN; s.o_t = s.o_lam + nsl;
    // (the SOFT instantiations export the slack pairs behind the slacks)
    if (d.soft && upr_qp_needs_soft(P, d)) { s.o_sig = s.o_t + nsl; s.o_tau = s.o_sig + nsl; s.o_gam = s.o_tau + nsl; }
    else s.o_sig = s.o_tau = s.o_gam = -1;
}
// a listed or headline instantiation of the production kernel
template <class C>
static inline void upr_qp3_fill(upr_qp_choice& s, const upr_problem& P, const upr_dims& d) {
    s.ws_doubles = upr_qp3_ws<C>::total;
    upr_qp_point_exported(s, P, d);
    char t[96];
    upr_qp3_cfg_text(s.cfg, s.nt, t, sizeof(t));
    snprintf(s.name, sizeof(s.name), "upr_qp3_kernel<upr_qp3_cfg<%s>>", t);
}
// an instantiation made at run time: ws_doubles as its info kernel reported it
static inline void upr_qp3_fill_run_time(upr_qp_choice& s, const upr_problem& P, const upr_dims& d, int ws_doubles) {
    s.ws_doubles = ws_doubles;
    upr_qp_point_exported(s, P, d);
    char t[96];
    upr_qp3_cfg_text(s.cfg, s.nt, t, sizeof(t));
    snprintf(s.name, sizeof(s.name), "upr_qp3_jit<upr_qp3_cfg<%s>>", t);
}
template <class D>
static inline void upr_qp2_fill(upr_qp_choice& s, const upr_dims& d) {
    const upr_qp2_ws<D> w(d.N, d.neN);
    s.ws_doubles = w.total;
    s.exported = false;
    s.o_pi = w.pi; s.o_nu = w.nu; s.o_yN = w.yN; s.o_lam = w.lam; s.o_t = w.t; s.o_sig = s.o_tau = s.o_gam = -1;
    snprintf(s.name, sizeof(s.name), "upr_qp2_kernel<upr_qp2_dims<%d, %d, %d, %d>, %d>", D::NQ, D::NB, D::NC, D::NF, s.nt == 512 ? 128 : s.nt);
}
static inline void upr_qp_fill_generic(upr_qp_choice& s, const upr_dims& d) {
    s.ws_doubles = d.ws_stride;
    s.exported = false;
    s.o_pi = d.ws_pi; s.o_nu = d.ws_nu; s.o_yN = d.ws_yN; s.o_lam = d.ws_lam; s.o_t = d.ws_t;
    if (d.soft) { s.o_sig = d.ws_sig; s.o_tau = d.ws_tau; s.o_gam = d.ws_gam; }
    else s.o_sig = s.o_tau = s.o_gam = -1;
    snprintf(s.name, sizeof(s.name), "upr_qp_kernel<%d>", s.nt);
}

// Fills a plan.  d: the dimensions as upr_make_dims left them (ws_stride: the generic layout's); run_time_ws: the workspace a
// run-time instantiation reported.  visit(upr_qp3_cfg<...>()) / visit(upr_qp2_dims<...>()) is called for the SELECTED kernel where it
// is one of the library's own (upr_api.hip: its launcher and the place of its factors).  Every QP kernel indexes the instance
// workspace with the same stride: the largest of the generic layout's, the second structure's whenever the shape has one
// (selected or not) and the selected production instantiation's.
template <class V>
static inline void upr_qp_resolve(upr_qp_choice& s, const upr_problem& P, const upr_dims& d, int run_time_ws, V&& visit) {
    int ws2 = 0;
    upr_qp2_shape(P, [&](auto D) {
        typedef decltype(D) D2;
        ws2 = (int)upr_qp2_ws_doubles<D2>(d.N, d.neN);
        if (s.structure == UPR_QP_STRUCT_SECOND) { upr_qp2_fill<D2>(s, d); visit(D); }
    });
    auto production = [&](auto C) { upr_qp3_fill<decltype(C)>(s, P, d); visit(C); };
    if (s.structure == UPR_QP_STRUCT_GENERIC) upr_qp_fill_generic(s, d);
    else if (s.structure == UPR_QP_STRUCT_PRODUCTION) {
        if (s.source == UPR_QP_FROM_RUN_TIME) upr_qp3_fill_run_time(s, P, d, run_time_ws);
        // problems without state-polytopic rows run the instantiation that has none compiled in (upr_qp3.h, upr_qp3_cfg)
        else if (s.source == UPR_QP_FROM_HEADLINE) { if (d.no > 0) production(upr_qp3_cfg<9, 1, 4, 3, 20, 256, true>()); else production(upr_qp3_cfg<9, 1, 4, 3, 20, 256, false>()); }
        else upr_qp3_listed(P, d, production);
    }
    s.ws_stride = d.ws_stride;
    if (s.ws_stride < ws2) s.ws_stride = ws2;
    if (s.structure == UPR_QP_STRUCT_PRODUCTION && s.ws_stride < s.ws_doubles) s.ws_stride = s.ws_doubles;
    if (!s.exported) s.stride = s.ws_stride;
}
