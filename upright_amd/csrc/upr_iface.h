// upr_iface.h -- interface states: [robot x (nx = 3 nq) | r v a of every dynamic obstacle (9 n_dyn)], the width every entry of
// the C-ABI that takes or returns states uses (include/upright_mi.h).  The kernels work on the robot block alone; the obstacles
// are data.  This is the ONE place that knows the layout: upr_api.hip narrows and widens through these functions and nowhere else.
// Plain C++ on raw pointers, no HIP and no handle, so that the host emulation compiles and tests it (tests/emu/upr_emu.cpp).
#pragma once

#include <cstddef>
#include <cstring>

static inline size_t upr_iface_dyn_width(int n_dyn) { return 9 * (size_t)n_dyn; }              // the obstacle block
static inline size_t upr_iface_width(int nx, int n_dyn) { return (size_t)nx + upr_iface_dyn_width(n_dyn); }   // a whole state (nxf)

// n interface states xf[n][nxf] -> their robot blocks xr[n][nx] and, where dyn is not NULL, their obstacle blocks dyn[n][9 n_dyn]
static inline void upr_iface_split(int nx, int n_dyn, const double* xf, size_t n, double* xr, double* dyn) {
    const size_t nd = upr_iface_dyn_width(n_dyn), nxf = upr_iface_width(nx, n_dyn);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(xr + i * nx, xf + i * nxf, sizeof(double) * nx);
        if (dyn) std::memcpy(dyn + i * nd, xf + i * nxf + nx, sizeof(double) * nd);
    }
}

// the inverse: robot blocks and obstacle blocks as they are -> out[n][nxf]
static inline void upr_iface_join(int nx, int n_dyn, const double* xr, const double* dyn, size_t n, double* out) {
    const size_t nd = upr_iface_dyn_width(n_dyn), nxf = upr_iface_width(nx, n_dyn);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(out + i * nxf, xr + i * nx, sizeof(double) * nx);
        std::memcpy(out + i * nxf + nx, dyn + i * nd, sizeof(double) * nd);
    }
}

// n rows of robot width -> out[n][nxf] with a zero obstacle block.  A row is whatever is a function of the robot state alone:
// a step of the QP, a row of the feedback gains, a gradient of the value function (the obstacle is data of the QP, not a state
// of its Riccati recursion)
static inline void upr_iface_join_zero(int nx, int n_dyn, const double* xr, size_t n, double* out) {
    const size_t nxf = upr_iface_width(nx, n_dyn);
    for (size_t i = 0; i < n; ++i) {
        std::memcpy(out + i * nxf, xr + i * nx, sizeof(double) * nx);
        for (size_t c = nx; c < nxf; ++c) out[i * nxf + c] = 0.0;
    }
}

// every obstacle of one state, [n_dyn][9], a time tau after it was observed: uncontrolled, constant acceleration
// (system_dynamics.h:29-39)
static inline void upr_iface_obstacle_after(const double* xo, double tau, double* out, int n_dyn) {
    for (int o = 0; o < n_dyn; ++o, xo += 9, out += 9)
        for (int i = 0; i < 3; ++i) { out[6 + i] = xo[6 + i]; out[3 + i] = xo[3 + i] + tau * xo[6 + i]; out[i] = xo[i] + tau * xo[3 + i] + 0.5 * tau * tau * xo[6 + i]; }
}

// ONE state: the robot block xr[nx] and the ballistic continuation of the observed obstacle block dyn[9 n_dyn] after tau -> out[nxf]
static inline void upr_iface_join_ballistic(int nx, int n_dyn, const double* xr, const double* dyn, double tau, double* out) {
    std::memcpy(out, xr, sizeof(double) * nx);
    upr_iface_obstacle_after(dyn, tau, out + nx, n_dyn);
}
