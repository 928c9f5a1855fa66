// upr_api.hip -- C-ABI of libupright_mi.so (include/upright_mi.h): host orchestration of the HIP kernels.
// No CPU compute path: every entry point that computes launches kernels on the current HIP device.
// This unit: the handle's lifecycle, advance_impl, tick and its graph, the solution / evaluate / feedback / KKT / value-function
// entries, the run-time instantiation of the production QP kernel (jit_get), and the small kernels (prepare, evaluate*, feedback,
// core_*, those of upr_value.h).  The handle and the error plumbing are upr_handle.h's; it defines upr_fail for every unit.
// What crosses its boundary (declared in upr_handle.h): it calls upr_bal_resolve (upr_api_balance.hip: the balance family and its
// entries), upr_launch_resolve / launch_linearize / launch_linesearch (upr_api_launch.hip) and qp_generic_launcher / qp2_launcher
// (upr_api_qp_old.hip); of upr_qp.h / upr_qp2.h it reads the host-side layouts only and instantiates no kernel.
#include <hip/hip_runtime.h>
#include <hip/hiprtc.h>

#include <dlfcn.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <fstream>
#include <map>
#include <mutex>
#include <sstream>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "upr_handle.h"
#include "upr_qp3_launch.h"
#include "upr_value.h"
#include "upr_iface.h"

namespace {
thread_local std::string g_err;   // the calling thread's last error (upr_last_error)
}  // namespace

int upr_fail(const std::string& msg) {
    g_err = msg;
    return 1;
}

namespace {

// ---- small kernels -----------------------------------------------------------------------------------
__global__ void core_object_dynamics_kernel(const upr_problem* P, const double* body_params, int n, const double* forces,
                                            const double* C, const double* w, const double* al, const double* a, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int nb = P->nb, nfc = P->nf * P->nc;
    upr_ee<double> E;
    for (int r = 0; r < 9; ++r) E.C[r] = C[(size_t)i * 9 + r];
    for (int r = 0; r < 3; ++r) { E.w[r] = w[(size_t)i * 3 + r]; E.al[r] = al[(size_t)i * 3 + r]; E.a[r] = a[(size_t)i * 3 + r]; E.p[r] = 0; E.v[r] = 0; }
    double Fw[6 * UPR_MAX_BODIES];
    upr_object_wrenches(P, body_params, forces + (size_t)i * nfc, Fw);
    for (int b = 0; b < nb; ++b)
        upr_body_residual<double>(E, body_params + 10 * b, P->gravity, Fw + 6 * b, Fw + 6 * b + 3, out + (size_t)i * 6 * nb + 6 * b);
}

__global__ void core_friction_rows_kernel(const upr_problem* P, int n, const double* forces, double* out) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * P->nc) return;
    int s = i / P->nc, c = i % P->nc;
    upr_friction_rows_contact(P, c, forces + ((size_t)s * P->nc + c) * 3, out + ((size_t)s * P->nc + c) * 5);
}

// initial guess of every instance: previous solution re-sampled on the new grid (warm start), or the
// stationary guess x_k = x0, u = 0 (DefaultInitializer); the first node is always the observation.
__global__ void prepare_kernel(const upr_problem* P, upr_dims d, int B, int has_prev /* a previous solution exists (every instance or none) */, const double* tprev,
                               const double* xs_prev, const double* us_prev, const double* t0, const double* x0,
                               double* xs, double* us, double* stats, int* done) {
    int b = blockIdx.x;
    const int N = d.N, nx = d.nx, nu = d.nu;
    const double* xp = xs_prev + (size_t)b * (N + 1) * nx;
    const double* up = us_prev + (size_t)b * N * nu;
    double* xo = xs + (size_t)b * (N + 1) * nx;
    double* uo = us + (size_t)b * N * nu;
    const bool warm = has_prev != 0;
    for (int e = threadIdx.x; e < (N + 1) * nx; e += blockDim.x) {
        int k = e / nx, i = e % nx;
        double v;
        if (k == 0 || !warm) v = x0[(size_t)b * nx + i];
        else upr_interp(d, P->dt, tprev[b], xp, up, t0[b] + k * P->dt, i, 0, &v, nullptr);
        xo[e] = v;
    }
    for (int e = threadIdx.x; e < N * nu; e += blockDim.x) {
        int k = e / nu, i = e % nu;
        double v = 0.0;
        if (warm) upr_interp(d, P->dt, tprev[b], xp, up, t0[b] + k * P->dt, 0, i, nullptr, &v);
        uo[e] = v;
    }
    for (int e = threadIdx.x; e < UPR_NSTATS; e += blockDim.x) stats[(size_t)b * UPR_NSTATS + e] = 0.0;
    if (threadIdx.x == 0) done[b] = 0;
}

__global__ void evaluate_kernel(const upr_problem* P, upr_dims d, int B, const double* tsol, const double* xs,
                                const double* us, const double* t, int t_stride, double* x_out, double* u_out) {
    int b = blockIdx.x;
    const int N = d.N, nx = d.nx, nu = d.nu;
    const double tau = t[(size_t)b * t_stride];
    for (int i = threadIdx.x; i < nx; i += blockDim.x)
        upr_interp(d, P->dt, tsol[b], xs + (size_t)b * (N + 1) * nx, us + (size_t)b * N * nu, tau, i, 0, x_out + (size_t)b * nx + i, nullptr);
    for (int i = threadIdx.x; i < nu; i += blockDim.x)
        upr_interp(d, P->dt, tsol[b], xs + (size_t)b * (N + 1) * nx, us + (size_t)b * N * nu, tau, 0, i, nullptr, u_out + (size_t)b * nu + i);
}

// Linear feedback gains of the last QP, ocs2 sign convention (u = bias + K x): fb[B][N][nu][nx].
// Jerk rows: -Hjj^-1 Hux from the Riccati recursion; contact-force rows: -Hff^-1 Df' S^-1 C (the forces
// follow the state through the object-dynamics equality).
// NEM / NFM: compile-time bounds of ne / nfc (the per-thread scratch vectors stay in registers for the small shapes)
// The two pieces every reader of the factors shares (the gather of the whole array and the policy that forms one or two knots):
// entry (j, c) of knot k's jerk rows, before the sign ...
__device__ inline double fb_jerk_entry(const upr_dims& d, const upr_fb_src& src, const double* w, int k, int j, int c) {
    const int nq = d.nq, nx = d.nx;
    if (src.kind == 3) return w[src.k_base + (long)k * src.k_stride + j * nx + c];
    const double* V = w + src.k_base + (long)k * src.k_stride;
    const double* Lji = w + src.lji_base + (long)k * src.lji_stride;
    double v = 0.0;
    for (int m = j; m < nq; ++m) v += Lji[m * nq + j] * V[m * nx + c];
    return v;
}
// ... and column c of knot k's contact-force rows, through L_s^-1, D_f', L_f^-1, into out[nu][nx] (the knot's block)
template <int NEM, int NFM>
__device__ inline void fb_force_column(const upr_dims& d, const upr_fb_src& src, const double* w, const double* Ck, const double* Dfb, int k, int c, double* out) {
    const int nq = d.nq, nx = d.nx, ne = d.ne, nfc = d.nfc, nf = d.nf;
    const double* Lsi = w + src.lsi_base + (long)k * src.lsi_stride;
    const double* Lfi = w + src.lfi_base + (long)k * src.lfi_stride;
    double t1[NEM], t2[NEM], t3[NFM];
    // S^-1 C = Lsi' (Lsi C), block by block (a dense factor is one block of ne rows)
    const int sb = src.lsi_sb;
    for (int r = 0; r < ne; ++r) { const int b0 = (r / sb) * sb; const double* Lb = Lsi + (b0 / sb) * sb * sb; double v = 0.0; for (int m = b0; m <= r; ++m) v += Lb[(r - b0) * sb + (m - b0)] * Ck[m * nx + c]; t1[r] = v; }
    for (int r = 0; r < ne; ++r) { const int b0 = (r / sb) * sb; const double* Lb = Lsi + (b0 / sb) * sb * sb; double v = 0.0; for (int m = r; m < b0 + sb; ++m) v += Lb[(m - b0) * sb + (r - b0)] * t1[m]; t2[r] = v; }
    for (int i = 0; i < nfc; ++i) { double v = 0.0; for (int r = 0; r < ne; ++r) v += Dfb[r * nfc + i] * t2[r]; t3[i] = v; }
    for (int ci = 0; ci < d.nc; ++ci) {
        if (nf == 3) {
            const double* Bk = Lfi + 9 * ci; const double* x3 = t3 + 3 * ci;
            double y[3], z[3];
            for (int a = 0; a < 3; ++a) { double v = 0.0; for (int b2 = 0; b2 <= a; ++b2) v += Bk[3 * a + b2] * x3[b2]; y[a] = v; }
            for (int a = 0; a < 3; ++a) { double v = 0.0; for (int b2 = a; b2 < 3; ++b2) v += Bk[3 * b2 + a] * y[b2]; z[a] = v; }
            for (int a = 0; a < 3; ++a) out[(size_t)(nq + 3 * ci + a) * nx + c] = -z[a];
        } else {
            const double lf = Lfi[ci];
            out[(size_t)(nq + ci) * nx + c] = -lf * lf * t3[ci];
        }
    }
}

template <int NEM, int NFM>
__global__ void feedback_kernel(const upr_problem* P, upr_dims d, upr_fb_src src, const double* ws, const double* lin,
                                const double* Df, const double* stats, double* fb) {
    const int b = blockIdx.x;
    const int N = d.N, nq = d.nq, nx = d.nx, nu = d.nu, ne = d.ne, nfc = d.nfc;
    const double* w = ws + (size_t)b * d.ws_stride;
    double* out = fb + (size_t)b * N * nu * nx;
    if (stats[(size_t)b * UPR_NSTATS + 2] == 2.0) {
        // the last QP's factorisation broke down (status 2, no step taken): its factors are not a policy; the instance
        // keeps its plan as a feed-forward input until the next successful solve
        for (int e = threadIdx.x; e < N * nu * nx; e += blockDim.x) out[e] = 0.0;
        return;
    }
    for (int e = threadIdx.x; e < N * nq * nx; e += blockDim.x) {
        const int k = e / (nq * nx), j = (e % (nq * nx)) / nx, c = e % nx;
        out[((size_t)k * nu + j) * nx + c] = -fb_jerk_entry(d, src, w, k, j, c);
    }
    const double* Dfb = Df + (size_t)b * ne * nfc;
    for (int e = threadIdx.x; e < N * nx; e += blockDim.x) {
        const int k = e / nx, c = e % nx;
        const double* Ck = lin + ((size_t)b * (N + 1) + k) * d.lin_stride + d.lin_gx;
        fb_force_column<NEM, NFM>(d, src, w, Ck, Dfb, k, c, out + (size_t)k * nu * nx);
    }
}

// u(t, x) = (1 - a) [u_j + K_j (x - x_j)] + a [u_j+1 + K_j+1 (x - x_j+1)]   (ocs2::LinearController with
// bias_j = u_j - K_j x_j, both arrays interpolated linearly); the last interval keeps u_{N-1}, K_{N-1}.
__global__ void evaluate_policy_kernel(const upr_problem* P, upr_dims d, int B, const double* tsol, const double* xs,
                                       const double* us, const double* fb, const double* t, const double* x_obs,
                                       double* x_out, double* u_out) {
    const int b = blockIdx.x;
    const int N = d.N, nx = d.nx, nu = d.nu;
    const double* X = xs + (size_t)b * (N + 1) * nx; const double* U = us + (size_t)b * N * nu;
    const double* K = fb + (size_t)b * N * nu * nx; const double* xo = x_obs + (size_t)b * nx;
    double s = (t[b] - tsol[b]) / P->dt;
    if (s < 0.0) s = 0.0;
    for (int i = threadIdx.x; i < nx; i += blockDim.x)
        upr_interp(d, P->dt, tsol[b], X, U, t[b], i, 0, x_out + (size_t)b * nx + i, nullptr);
    for (int i = threadIdx.x; i < nu; i += blockDim.x) {
        double v = 0.0;
        if (s <= N) {
            int j = (int)s; if (j > N - 1) j = N - 1;
            const double a = (s >= N - 1) ? 0.0 : s - j;
            const int j1 = (j + 1 < N) ? j + 1 : N - 1;
            double v0 = U[j * nu + i], v1 = U[j1 * nu + i];
            for (int c = 0; c < nx; ++c) {
                v0 += K[((size_t)j * nu + i) * nx + c] * (xo[c] - X[j * nx + c]);
                if (a > 0.0) v1 += K[((size_t)j1 * nu + i) * nx + c] * (xo[c] - X[j1 * nx + c]);
            }
            v = (1.0 - a) * v0 + a * v1;
        }
        u_out[(size_t)b * nu + i] = v;
    }
}

// The same policy while the gains are still in the factors of the advance's last QP (upr_fb_state.h): the workgroup forms the gains
// of knot j -- and of knot j + 1 where the time lies inside an interval -- into LDS as [nu][nx] with the gather's own formulas
// (fb_jerk_entry, fb_force_column: one lane per column of the force rows), then lanes i < nu run the dot products of
// evaluate_policy_kernel in its order.  Per knot it reads K_k, C_k, the two factors and D_f, about what the knot's block of the
// array holds, and writes nothing but the answer.  Dynamic LDS: 2 nu nx doubles (at most 2 x 108 x 36: under the 64 KiB a kernel
// gets without asking).  A QP that ended with status 2 has no policy: its instance gets the plan's input.
template <int NEM, int NFM>
__global__ void evaluate_policy_factors_kernel(const upr_problem* P, upr_dims d, int B, const double* tsol, const double* xs,
                                               const double* us, upr_fb_src src, const double* ws, const double* lin, const double* Df,
                                               const double* stats, const double* t, const double* x_obs, double* x_out, double* u_out) {
    extern __shared__ double fb_lds[];
    const int b = blockIdx.x;
    const int N = d.N, nq = d.nq, nx = d.nx, nu = d.nu, ne = d.ne, nfc = d.nfc;
    const double* X = xs + (size_t)b * (N + 1) * nx; const double* U = us + (size_t)b * N * nu;
    const double* xo = x_obs + (size_t)b * nx;
    double s = (t[b] - tsol[b]) / P->dt;
    if (s < 0.0) s = 0.0;
    for (int i = threadIdx.x; i < nx; i += blockDim.x)
        upr_interp(d, P->dt, tsol[b], X, U, t[b], i, 0, x_out + (size_t)b * nx + i, nullptr);
    // (s, j, j1 and a are the same in every lane of the workgroup: the branches below are uniform)
    int j = (int)s; if (j > N - 1) j = N - 1;
    const double a = (s >= N - 1) ? 0.0 : s - j;
    const int j1 = (j + 1 < N) ? j + 1 : N - 1;
    const bool inside = s <= N, policy = stats[(size_t)b * UPR_NSTATS + 2] != 2.0;
    if (inside && policy) {
        const double* w = ws + (size_t)b * d.ws_stride;
        const double* Dfb = Df + (size_t)b * ne * nfc;
        const int nk = a > 0.0 ? 2 : 1;
        for (int q = 0; q < nk; ++q) {
            const int k = q ? j1 : j;
            double* G = fb_lds + (size_t)q * nu * nx;
            for (int e = threadIdx.x; e < nq * nx; e += blockDim.x) G[e] = -fb_jerk_entry(d, src, w, k, e / nx, e % nx);
            const double* Ck = lin + ((size_t)b * (N + 1) + k) * d.lin_stride + d.lin_gx;
            for (int c = threadIdx.x; c < nx; c += blockDim.x) fb_force_column<NEM, NFM>(d, src, w, Ck, Dfb, k, c, G);
        }
    }
    __syncthreads();
    const double* K0 = fb_lds; const double* K1 = fb_lds + (size_t)nu * nx;
    for (int i = threadIdx.x; i < nu; i += blockDim.x) {
        double v = 0.0;
        if (inside) {
            double v0 = U[j * nu + i], v1 = U[j1 * nu + i];
            if (policy) for (int c = 0; c < nx; ++c) {
                v0 += K0[(size_t)i * nx + c] * (xo[c] - X[j * nx + c]);
                if (a > 0.0) v1 += K1[(size_t)i * nx + c] * (xo[c] - X[j1 * nx + c]);
            }
            v = (1.0 - a) * v0 + a * v1;
        }
        u_out[(size_t)b * nu + i] = v;
    }
}
static_assert(2 * UPR_MAX_NU * UPR_MAX_NX * sizeof(double) <= 64 * 1024, "two knots of gains in the LDS a kernel gets without asking");

int check_problem(const upr_problem* P) {
    if (!P) return upr_fail("upr_problem is NULL");
    if (P->nq != 6 && P->nq != 9) return upr_fail("unsupported chain length nq = " + std::to_string(P->nq) + " (kernels are instantiated for 6 and 9 joints)");
    if (P->nb < 1 || P->nb > UPR_MAX_BODIES) return upr_fail("nb out of range");
    if (P->nc < 1 || P->nc > UPR_MAX_CONTACTS) return upr_fail("nc out of range");
    if (P->nf != 1 && P->nf != 3) return upr_fail("nf must be 1 or 3");
    if (P->N < 1 || P->N > 1000) return upr_fail("N out of range");
    if (!(P->dt > 0)) return upr_fail("dt must be positive");
    if (P->n_way < 1 || P->n_way > UPR_MAX_WAYPOINTS) return upr_fail("n_way out of range");
    for (int i = 0; i < 6; ++i) if (!(P->Wee[i] >= 0)) return upr_fail("end-effector weights must be non-negative");
    if (P->n_sph < 0 || P->n_sph > UPR_MAX_SPHERES) return upr_fail("n_sph out of range");
    if (P->n_pairs < 0 || P->n_pairs > UPR_MAX_PAIRS) return upr_fail("n_pairs out of range");
    if (P->n_dyn < 0 || P->n_dyn > UPR_MAX_DYN) return upr_fail("n_dyn must be in 0 .. UPR_MAX_DYN");
    if (P->n_proj < 0 || P->n_proj > 8 || (P->n_proj > 0 && P->n_dyn < 1)) return upr_fail("projectile rows need a dynamic obstacle (n_proj <= 8; they follow the last one)");
    if (P->soft_state_box || P->soft_input_box || P->soft_poly) {
        if (!(P->soft_L2_lower >= 0) || !(P->soft_L2_upper >= 0) || !(P->soft_L1_lower >= 0) || !(P->soft_L1_upper >= 0)) return upr_fail("slack penalties must be non-negative");
        if (!(P->soft_L2_lower + P->soft_L1_lower > 0) || !(P->soft_L2_upper + P->soft_L1_upper > 0)) return upr_fail("softened rows need a positive L1 or L2 penalty");
    }
    if (P->soft_eq && (!(P->soft_L2_lower > 0) || P->soft_L2_lower != P->soft_L2_upper || P->soft_L1_lower != 0 || P->soft_L1_upper != 0))
        return upr_fail("a softened object-dynamics equality needs equal positive L2 penalties and zero L1 penalties (the slack pair is eliminated to a quadratic penalty)");
    for (int i = 0; i < P->n_proj; ++i) if (P->proj_sph[i] < 0 || P->proj_sph[i] >= P->n_sph || !(P->proj_dist[i] > 0)) return upr_fail("projectile row out of range");
    for (int i = 0; i < P->n_sph; ++i) if (P->sph_frame[i] > P->nq || (P->sph_frame[i] <= -2 && -2 - P->sph_frame[i] >= P->n_dyn)) return upr_fail("sph_frame out of range");
    for (int i = 0; i < P->n_pairs; ++i)
        if (P->pair_a[i] < 0 || P->pair_a[i] >= P->n_sph || P->pair_b[i] < -1 || P->pair_b[i] >= P->n_sph || P->pair_a[i] == P->pair_b[i]) return upr_fail("collision pair out of range");
    if (P->ee_box) for (int i = 0; i < 3; ++i)
        if (!std::isfinite(P->ee_box_lower[i]) || !std::isfinite(P->ee_box_upper[i]) || P->ee_box_lower[i] > P->ee_box_upper[i])
            return upr_fail("end-effector box: lower and upper must be finite with lower <= upper");
    for (int i = 0; i < P->nc; ++i) {
        if (P->contact_body2[i] < 0 || P->contact_body2[i] >= P->nb) return upr_fail("contact_body2 must index a balanced body");
        if (P->contact_body1[i] >= P->nb) return upr_fail("contact_body1 out of range");
    }
    return 0;
}

int need_device() {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n < 1) return upr_fail("no HIP device available: libupright_mi has no CPU path");
    return 0;
}

// third-structure ("production") kernel.  The headline shape (nq 9, nb 1, nc 4, nf 3, N 20) at 256 lanes, with and without
// state-polytopic rows; further (shape, SOFT) instantiations at 256 lanes for the configurations the
// reference ships with HPIPM slacks: thing_demo (one body, frictionless) and the upright_robust 8-corner arrangement.
// (the kernels themselves are instantiated in upr_qp3_inst.hip, one translation unit per part of upr_qp3_list.h, compiled side
// by side; this file only declares their launchers -- -DUPR_MONOLITHIC instantiates them here instead: experiment builds)
template <class C>
int launch_qp3_cfg(upr_batch* h, const upr_qp_args& A) {
    const int rc = upr_qp3_launch<C>(h->stream, h->B, A);
    if (rc == -1) return upr_fail("QP working set exceeds 160 KiB of LDS");
    if (rc != 0) return upr_fail(std::string("upr_qp3_kernel launch: ") + hipGetErrorString((hipError_t)rc));
    return 0;
}
int launch_qp3_bad_nt(upr_batch*, const upr_qp_args&) {
    return upr_fail("the production QP kernel ships at 256 lanes (UPR_QP_NT = 128 | 512 were A/B instantiations of rounds 1 - 5; UPR_QP3_JIT=2 UPR_JIT_NT=... instantiates one at run time)");
}
int launch_qp3_run_time(upr_batch* h, const upr_qp_args& A) {
    const upr_jit_kernel* k = h->qp.jit;
    upr_qp_args Ac = A;
    void* args[] = {&Ac};
    UPR_HIP(hipModuleLaunchKernel(k->fn, (unsigned)h->B, 1, 1, (unsigned)k->nt, 1, 1, (unsigned)k->lds, h->stream, args, nullptr));
    return 0;
}

// what upr_qp_resolve's visitor adds for one of the library's own kernels: its launcher and the place of its per-knot factors
struct qp_sel_own {
    upr_qp_sel& s;
    const upr_dims& d;
    template <int a, int b, int c, int e, int n, int nt, bool rows, bool sf, bool dense>
    void operator()(upr_qp3_cfg<a, b, c, e, n, nt, rows, sf, dense>) const {
        typedef upr_qp3_cfg<a, b, c, e, n, nt, rows, sf, dense> C; typedef upr_qp3_ws<C> W; typedef upr_qp3_far<C> F;
        s.launch = (s.nt == nt) ? launch_qp3_cfg<C> : launch_qp3_bad_nt;   // (UPR_QP_NT on the headline)
        // (these offsets lie in front of everything that depends on the workgroup size or on ROWS / SOFT)
        s.fb.kind = 3; s.fb.k_base = W::far + F::Ks; s.fb.k_stride = C::NQ * C::NX; s.fb.lji_base = 0; s.fb.lji_stride = 0;
        s.fb.lfi_base = W::far + F::lfi; s.fb.lfi_stride = C::NLF; s.fb.lsi_base = W::far + F::lsi; s.fb.lsi_stride = C::NLS; s.fb.lsi_sb = C::SB;
    }
    template <int a, int b, int c, int e>
    void operator()(upr_qp2_dims<a, b, c, e>) const {
        typedef upr_qp2_dims<a, b, c, e> D;
        const upr_qp2_ws<D> w(d.N, d.neN);
        s.launch = qp2_launcher(a, b, c, e, s.nt);
        s.fb.kind = 2; s.fb.k_base = w.store + D::SS_V; s.fb.k_stride = D::SS_STRIDE; s.fb.lji_base = w.store + D::SS_LJI; s.fb.lji_stride = D::SS_STRIDE;
        s.fb.lfi_base = w.pre + D::PR_LFI; s.fb.lfi_stride = D::PR_STRIDE; s.fb.lsi_base = w.pre + D::PR_LSI; s.fb.lsi_stride = D::PR_STRIDE; s.fb.lsi_sb = d.ne;
    }
};
// fills the plan in s (with s.jit where it is a run-time instantiation): sizes, offsets, name, launcher, factors
void qp_resolve(upr_qp_sel& s, const upr_problem& P, const upr_dims& d) {
    upr_qp_resolve(s, P, d, s.jit ? (int)s.jit->ws : 0, qp_sel_own{s, d});
    if (s.jit) { s.launch = launch_qp3_run_time; s.fb = s.jit->fb; }
    else if (s.structure == UPR_QP_STRUCT_GENERIC) {
        s.launch = qp_generic_launcher(s.nt);
        s.fb.kind = 1; s.fb.k_base = d.ws_store + d.ss_kx; s.fb.k_stride = d.ss_stride; s.fb.lji_base = d.ws_store + d.ss_hjj; s.fb.lji_stride = d.ss_stride;
        s.fb.lfi_base = d.ws_store + d.ss_hff; s.fb.lfi_stride = d.ss_stride; s.fb.lsi_base = d.ws_store + d.ss_sinv; s.fb.lsi_stride = d.ss_stride; s.fb.lsi_sb = d.ne;
    }
}

// ---- run-time instantiation of the production kernel (round 4) ---------------------------------------------------------------
// The hand list of upr_qp3_list.h covers the shapes the reference's configs use.  Any other shape the structure can take (one
// chain of 6 or 9 joints, star or stacked arrangement, nf 1 | 3, with or without rows / slacks, a horizon whose working set fits
// the LDS) is instantiated at upr_batch_create with hiprtc out of the SAME header -- upr_qp3.h with its template arguments as a
// macro -- instead of falling back to the second-structure or generic kernel (20 - 40x slower per QP).  The code object is cached
// in memory per process and on disk ($UPR_JIT_CACHE or ~/.cache/upright_amd) under the shape key and a hash of the kernel
// headers, so a shape costs its compile time once per machine -- measured: about TWO SECONDS (comgr in-process; the same
// instantiation takes hipcc 45 s, most of it the host pass), and the code runs as fast as the ahead-of-time one (headline 2.237
// against 2.224 ms per launch, upright_robust 6.31 against 6.35).  UPR_QP3_JIT = 0: never (the second-structure / generic kernels
// take such shapes, as in rounds 1 - 3); = 2: also for the listed shapes (diagnostic); unset or 1: every capable shape.
std::mutex g_jit_mutex;
std::map<std::string, upr_jit_kernel> g_jit;

extern "C" const char* upr_last_error(void);
std::string jit_csrc_dir() {
    if (const char* e = getenv("UPR_CSRC_DIR")) return e;
    Dl_info info;
    if (dladdr((const void*)&upr_last_error, &info) && info.dli_fname) {
        std::string p = info.dli_fname;
        const size_t s = p.rfind('/');
        return (s == std::string::npos ? std::string(".") : p.substr(0, s)) + "/csrc";
    }
    return "upright_amd/csrc";
}
bool jit_read(const std::string& path, std::string* out) {
    std::ifstream f(path, std::ios::binary);
    if (!f) return false;
    std::stringstream ss; ss << f.rdbuf(); *out = ss.str();
    return true;
}
// the instantiation (tuple; nt lanes: UPR_JIT_NT) that upr_qp_plan asked for
int jit_get(const int* tuple, int nt, upr_jit_kernel** out) {
    char cfg[128];
    if (nt != 128 && nt != 256 && nt != 512) return upr_fail("UPR_JIT_NT must be 128, 256 or 512");
    upr_qp3_cfg_text(tuple, nt, cfg, sizeof(cfg));
    int dev = 0;
    UPR_HIP(hipGetDevice(&dev));
    const std::string key = std::string(cfg) + " @" + std::to_string(dev);
    std::lock_guard<std::mutex> lock(g_jit_mutex);
    auto it = g_jit.find(key);
    if (it != g_jit.end()) { *out = &it->second; return 0; }
    const std::string dir = jit_csrc_dir();
    // the translation unit and its options
    const std::string src =
        "#include \"upr_qp3.h\"\n"
        "typedef upr_qp3_cfg<UPR_QP3_JIT_CFG> upr_jit_cfg;\n"
        "extern \"C\" __global__ void __launch_bounds__(upr_jit_cfg::NT, (upr_jit_cfg::NT <= 256 && upr_jit_cfg::NB == 1) ? UPR_QP3_OCC1 : 1) upr_qp3_jit(upr_qp_args A) {\n"
        "    extern __shared__ __attribute__((aligned(16))) double smem[];\n"
        "    upr_ctx ctx; ctx.tid = threadIdx.x; ctx.nt = upr_jit_cfg::NT;\n"
        "    upr_qp3_solve<upr_jit_cfg>(ctx, A, upr_qp_instance(A, blockIdx.x), smem);\n"
        "}\n"
        "extern \"C\" __global__ void upr_qp3_jit_info(int* out) {\n"
        "    typedef upr_qp3_ws<upr_jit_cfg> W; typedef upr_qp3_far<upr_jit_cfg> F;\n"
        "    out[0] = upr_qp3_lds<upr_jit_cfg>::total; out[1] = W::total;\n"
        "    out[2] = W::far + F::Ks; out[3] = upr_jit_cfg::NQ * upr_jit_cfg::NX; out[4] = W::far + F::lfi; out[5] = upr_jit_cfg::NLF;\n"
        "    out[6] = W::far + F::lsi; out[7] = upr_jit_cfg::NLS; out[8] = upr_jit_cfg::SB;\n"
        "}\n";
    const std::string inc = "-I" + dir;
    std::string defc = std::string("-DUPR_QP3_JIT_CFG=") + cfg;
    defc.erase(std::remove(defc.begin(), defc.end(), ' '), defc.end());
    const std::string rinc = std::string("-I") + (getenv("ROCM_PATH") ? getenv("ROCM_PATH") : "/opt/rocm") + "/include";
    std::vector<std::string> optv = {"--offload-arch=gfx950", "-O3", "-std=c++17", "-Wno-unused-value", "-Wno-pass-failed", inc, rinc, defc};
    // UPR_JIT_FLAGS: extra compiler options for experiments (e.g. "-DUPR_QP3_PROF_FLAT=3")
    if (const char* e = getenv("UPR_JIT_FLAGS")) { std::stringstream ss(e); std::string w; while (ss >> w) optv.push_back(w); }
    // version of the code object: FNV-1a over every header the kernel is made of (the C-ABI header with the upr_problem layout
    // among them -- ADVICE r04: a cached kernel compiled for an older layout would read the new struct wrongly), the wrapper
    // above, the options (the include directories excepted: they name a place, not a content) and the compiler's version
    unsigned long long hsh = 1469598103934665603ull;
    auto mix = [&](const std::string& t) { for (unsigned char c : t) { hsh ^= c; hsh *= 1099511628211ull; } hsh ^= 0xff; hsh *= 1099511628211ull; };
    for (const char* f : {"../../include/upright_mi.h", "upr_common.h", "upr_kin.h", "upr_qp.h", "upr_qp2.h", "upr_qp3.h"}) {
        std::string txt;
        if (!jit_read(dir + "/" + f, &txt)) return upr_fail("run-time instantiation: cannot read " + dir + "/" + f + " (set UPR_CSRC_DIR)");
        mix(txt);
    }
    mix(src);
    for (const std::string& o : optv) if (o != inc && o != rinc) mix(o);
    { int vmaj = 0, vmin = 0; (void)hiprtcVersion(&vmaj, &vmin); mix(std::to_string(vmaj) + "." + std::to_string(vmin)); }
    // disk cache: $UPR_JIT_CACHE, else ~/.cache/upright_amd; none when neither is known (no predictable world-writable default)
    std::string cache;
    if (const char* e = getenv("UPR_JIT_CACHE")) cache = e;
    else if (const char* hm = getenv("HOME")) { if (*hm) cache = std::string(hm) + "/.cache/upright_amd"; }
    std::string path;
    if (!cache.empty()) {
        (void)mkdir((cache.substr(0, cache.rfind('/'))).c_str(), 0755);
        (void)mkdir(cache.c_str(), 0755);
        std::string fname = cfg;
        for (char& c : fname) if (c == ',' || c == ' ') c = '_';
        char hx[32]; snprintf(hx, sizeof(hx), "%016llx", hsh);
        path = cache + "/qp3_" + fname + "_" + hx + ".hsaco";
    }
    upr_jit_kernel k;
    k.cfg = cfg; k.nt = nt;
    std::string code;
    bool loaded = false;
    // cache file = [magic "UPRJIT01"][length of the code object][FNV-1a of it][code object]: a truncated or foreign file is recognised
    // HERE -- the loader does not return an error for a cut-off ELF, it crashes -- dropped, and the shape compiled anew
    auto fnv = [](const char* p, size_t n) { unsigned long long h = 1469598103934665603ull; for (size_t i = 0; i < n; ++i) { h ^= (unsigned char)p[i]; h *= 1099511628211ull; } return h; };
    if (!path.empty() && jit_read(path, &code)) {
        bool good = code.size() > 24 && memcmp(code.data(), "UPRJIT01", 8) == 0;
        unsigned long long len = 0, sum = 0;
        if (good) { memcpy(&len, code.data() + 8, 8); memcpy(&sum, code.data() + 16, 8); good = len == code.size() - 24 && sum == fnv(code.data() + 24, (size_t)len); }
        if (good) code.erase(0, 24);
        if (good && hipModuleLoadData(&k.mod, code.data()) == hipSuccess) loaded = true;
        else { (void)hipGetLastError(); (void)unlink(path.c_str()); code.clear(); }
    }
    if (!loaded) {
        fprintf(stderr, "libupright_mi: instantiating the production QP kernel for upr_qp3_cfg<%s> (once per machine: %s)\n", cfg, path.empty() ? "no disk cache" : path.c_str());
        hiprtcProgram prog;
        if (hiprtcCreateProgram(&prog, src.c_str(), "upr_qp3_jit.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS) return upr_fail("hiprtcCreateProgram failed");
        std::vector<const char*> opts;
        for (const std::string& o : optv) opts.push_back(o.c_str());
        const hiprtcResult rc = hiprtcCompileProgram(prog, (int)opts.size(), opts.data());
        if (rc != HIPRTC_SUCCESS) {
            size_t ls = 0; hiprtcGetProgramLogSize(prog, &ls);
            std::string log(ls, 0); if (ls) hiprtcGetProgramLog(prog, &log[0]);
            hiprtcDestroyProgram(&prog);
            return upr_fail("run-time instantiation of upr_qp3_cfg<" + std::string(cfg) + "> failed: " + log.substr(0, 2000));
        }
        size_t cs = 0; hiprtcGetCodeSize(prog, &cs);
        code.resize(cs); hiprtcGetCode(prog, &code[0]);
        hiprtcDestroyProgram(&prog);
        if (!path.empty()) {   // written next to its final name and renamed only when every byte arrived (a full disk leaves no stub behind)
            const std::string tmp = path + ".tmp" + std::to_string((long)getpid());
            bool ok;
            {
                const unsigned long long len = code.size(), sum = fnv(code.data(), code.size());
                std::ofstream f(tmp, std::ios::binary);
                f.write("UPRJIT01", 8); f.write((const char*)&len, 8); f.write((const char*)&sum, 8);
                f.write(code.data(), (std::streamsize)code.size()); f.flush(); ok = f.good();
            }
            if (!ok || rename(tmp.c_str(), path.c_str()) != 0) (void)unlink(tmp.c_str());
        }
        UPR_HIP(hipModuleLoadData(&k.mod, code.data()));
    }
    hipFunction_t info;
    UPR_HIP(hipModuleGetFunction(&k.fn, k.mod, "upr_qp3_jit"));
    UPR_HIP(hipModuleGetFunction(&info, k.mod, "upr_qp3_jit_info"));
    DevBuf<int> di;
    if (di.alloc(9)) return 1;
    int* dp = di;
    void* args[] = {&dp};
    UPR_HIP(hipModuleLaunchKernel(info, 1, 1, 1, 1, 1, 1, 0, nullptr, args, nullptr));
    int hi[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    UPR_HIP(hipMemcpy(hi, dp, sizeof(hi), hipMemcpyDeviceToHost));
    k.lds = (size_t)hi[0] * sizeof(double); k.ws = (size_t)hi[1];
    k.fb.kind = 3; k.fb.k_base = hi[2]; k.fb.k_stride = hi[3]; k.fb.lfi_base = hi[4]; k.fb.lfi_stride = hi[5]; k.fb.lsi_base = hi[6]; k.fb.lsi_stride = hi[7]; k.fb.lsi_sb = hi[8];
    if (k.lds > 160 * 1024) { (void)hipModuleUnload(k.mod); return upr_fail("run-time instantiation: the working set of upr_qp3_cfg<" + std::string(cfg) + "> exceeds 160 KiB of LDS"); }
    if (k.lds > 64 * 1024) UPR_HIP(hipFuncSetAttribute((const void*)k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)k.lds));
    auto ins = g_jit.emplace(key, k);
    *out = &ins.first->second;
    return 0;
}

int launch_qp(upr_batch* h, const upr_qp_args& A) { return h->qp.launch(h, A); }

upr_lin_args traj_lin_args(upr_batch* h) {
    upr_lin_args A;
    A.P = h->dP; A.d = h->d; A.body_params = h->body_params; A.way_p = h->way_p; A.way_q = upr_has_orientation_cost(&h->P) ? h->way_q : nullptr; A.t0 = h->t0;
    A.xs = h->xs; A.us = h->us; A.inst = nullptr; A.lin = h->lin; A.ee_out = nullptr;
    A.npoints = h->B * (h->d.N + 1);
    A.dyn = h->dyn0; A.pflag = h->pflag; A.Df = h->Df;
    return A;
}
upr_qp_args make_qp_args(upr_batch* h) {
    upr_qp_args A;
    A.P = h->dP; A.d = h->d; A.xs = h->xs; A.us = h->us; A.x0 = h->x0; A.lin = h->lin; A.Df = h->Df; A.ws = h->ws; A.stats = h->stats; A.prof = h->prof; A.iter_key = h->iter_key;
    return A;
}

// Per-launch device timing with HIP events recorded on the engine's stream (no host sync inside the
// timed region); upr_batch_kernel_times() reads them back after a stream sync.
struct KernelTimer {
    upr_batch* h; int slot; size_t idx; bool on;
    KernelTimer(upr_batch* h_, int s) : h(h_), slot(s), idx(0), on(h_->timing == 1 || (h_->timing == 2 && s == 1)) {
        if (h->timing == 3 && s == 1) on = (h->timing_qp_count++ % 4u) == 0u;
        if (!on) return;
        hipEvent_t a, b;
        // (reused: upr_batch_enable_timing stocks the free list, so that a timed loop creates none)
        if (h->ev_free.size() >= 2) { a = h->ev_free.back(); h->ev_free.pop_back(); b = h->ev_free.back(); h->ev_free.pop_back(); }
        else { (void)hipEventCreate(&a); (void)hipEventCreate(&b); }
        idx = h->ev_pool.size();
        h->ev_pool.push_back(a); h->ev_pool.push_back(b); h->ev_slot.push_back(slot);
        (void)hipEventRecord(a, h->stream);
    }
    void stop() { if (on) (void)hipEventRecord(h->ev_pool[idx + 1], h->stream); }
};

// ---- value function of the last QP: buffers, launch arguments, working set (upr_value.h)
int vf_alloc(upr_batch* h) {
    if (h->vf_P) return 0;
    const size_t B = (size_t)h->B, n1 = (size_t)h->d.N + 1, nx = (size_t)h->d.nx;
    if (dev_alloc(&h->vf_P, B * n1 * nx * nx) || dev_alloc(&h->vf_p, B * n1 * nx) || dev_alloc(&h->vf_J, B * n1) || dev_alloc(&h->vf_X, B * n1 * nx) || dev_alloc(&h->vf_t0, B) ||
        dev_alloc(&h->vf_nu, B * (size_t)h->d.N * (size_t)h->d.ne)) return 1;
    UPR_HIP(hipEventCreate(&h->vf_ev[0])); UPR_HIP(hipEventCreate(&h->vf_ev[1]));
    return 0;
}
// the cost-to-go kernel on the QP that was launched last (records in lin, step in ws, its point in the export buffer or the workspace)
upr_vf_args make_vf_args(upr_batch* h) {
    upr_vf_args A;
    A.P = h->dP; A.d = h->d; A.xs = h->xs; A.us = h->us; A.lin = h->lin; A.Df = h->Df; A.ws = h->ws;
    const upr_qp_sel& q = h->qp;
    A.mult = q.exported ? h->kkt : h->ws; A.mult_stride = q.stride;
    A.o_pi = q.o_pi; A.o_nu = q.o_nu; A.o_lam = q.o_lam; A.o_t = q.o_t; A.o_sig = q.o_sig; A.o_tau = q.o_tau; A.o_gam = q.o_gam;
    A.Pk = h->vf_P; A.pk = h->vf_p; A.J = h->vf_J; A.X = h->vf_X; A.nu_out = h->vf_nu;
    return A;
}
size_t vf_lds_bytes(const upr_batch* h) { return (size_t)upr_vf_lds_layout(h->d).total * sizeof(double); }
// The dynamic-LDS limit of a kernel is an attribute of the FUNCTION, for the whole process: always the ceiling the callers accept
// (160 KiB), never one handle's working set -- a smaller handle must not lower it under a larger one's in-stream launch or graph node
hipError_t vf_raise_lds_limit() { return hipFuncSetAttribute((const void*)upr_value_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); }

// Longest-first dispatch of the QP launch.  One workgroup solves one instance and a launch of B instances runs on
// 2 x 256 workgroup slots, so its duration is set by the slot that draws the largest SUM of IPM iteration counts: with
// the headline's 10..13 iterations per instance, arrival order gives 25 on some slot against a mean of 22.7.  The
// iteration count of an instance's previous QP predicts the next one well (same problem in a cold-start sweep, the
// neighbouring problem in closed loop), so the launch hands the instances out sorted by it, longest first (LPT rule):
// the short ones fill the gaps at the end.  The rank of an instance (ties by index) is computed by its own workgroup of the
// line-search launch that follows the QP (upr_linesearch.h, order_out): it only permutes which workgroup solves which instance.
// the gains' array from their sources, as the last QP launch on the handle left them (the gather kernel; no synchronisation)
int fb_gather(upr_batch* h) {
    const upr_dims& d = h->d;
    if (!h->fb && dev_alloc(&h->fb, (size_t)h->B * d.N * d.nu * d.nx)) return 1;
    if (h->qp.fb.kind == 0) return upr_fail("feedback gains: the selected QP kernel names no source for them");
    if (d.ne <= 6 && d.nfc <= 12) hipLaunchKernelGGL((feedback_kernel<6, 12>), dim3(h->B), dim3(256), 0, h->stream, h->dP, d, h->qp.fb, h->ws, h->lin, h->Df, h->stats, h->fb);
    else hipLaunchKernelGGL((feedback_kernel<6 * UPR_MAX_BODIES, 3 * UPR_MAX_CONTACTS>), dim3(h->B), dim3(256), 0, h->stream, h->dP, d, h->qp.fb, h->ws, h->lin, h->Df, h->stats, h->fb);
    UPR_HIP(hipGetLastError());
    return 0;
}
// before a call overwrites a source of gains that are still in the factors -- the workspace, the records or the statistics of the
// advance's last QP -- and before the whole array is handed out: gather it (upr_fb_state.h).  The sites: get_feedback_core (the
// request), kkt_launch and qp_step_core (a linearisation and a QP launch on the handle's own buffers, outside an advance),
// upr_batch_hold_stats putting statistics back, an advance that runs no QP (it clears the statistics)
int fb_keep(upr_batch* h) {
    if (!h->fb_on || !upr_fb_must_gather(h->fbt)) return 0;
    if (fb_gather(h)) return 1;
    h->fbt.state = upr_fb_after_gather(h->fbt);
    return 0;
}
// the policy of the stored solution at the times t and the states x_obs (both on the device), by the kernel that reads the gains
// where they are
int launch_policy(upr_batch* h, const double* t, const double* x_obs) {
    const upr_dims& d = h->d;
    if (upr_fb_policy_from_factors(h->fbt.state)) {
        if (h->qp.fb.kind == 0) return upr_fail("feedback gains: the selected QP kernel names no source for them");
        const size_t lds = sizeof(double) * 2 * d.nu * d.nx;
        if (d.ne <= 6 && d.nfc <= 12) hipLaunchKernelGGL((evaluate_policy_factors_kernel<6, 12>), dim3(h->B), dim3(64), lds, h->stream, h->dP, d, h->B, h->tprev, h->xs_prev, h->us_prev, h->qp.fb, h->ws, h->lin, h->Df, h->stats, t, x_obs, h->ev_x, h->ev_u);
        else hipLaunchKernelGGL((evaluate_policy_factors_kernel<6 * UPR_MAX_BODIES, 3 * UPR_MAX_CONTACTS>), dim3(h->B), dim3(64), lds, h->stream, h->dP, d, h->B, h->tprev, h->xs_prev, h->us_prev, h->qp.fb, h->ws, h->lin, h->Df, h->stats, t, x_obs, h->ev_x, h->ev_u);
    } else {
        // (no solve yet: the array of zeros, the plan's input)
        if (!h->fb && dev_alloc(&h->fb, (size_t)h->B * d.N * d.nu * d.nx)) return 1;
        hipLaunchKernelGGL(evaluate_policy_kernel, dim3(h->B), dim3(64), 0, h->stream, h->dP, d, h->B, h->tprev, h->xs_prev, h->us_prev, h->fb, t, x_obs, h->ev_x, h->ev_u);
    }
    UPR_HIP(hipGetLastError());
    return 0;
}

int advance_impl(upr_batch* h) {
    const upr_dims& d = h->d;
    if (h->vf_state) h->vf_state = 2;
    const int sqp_iters = h->sqp_iters_next > 0 ? h->sqp_iters_next : h->P.sqp_iters;
    h->sqp_iters_next = 0;
    upr_fb_advance fba;
    if (h->fb_on) {
        fba = upr_fb_on_advance(h->fbt, sqp_iters, h->qp.fb_fused);
        if (fba.gather_before && fb_keep(h)) return 1;
    }
    if (!h->guess_set) {
        hipLaunchKernelGGL(prepare_kernel, dim3(h->B), dim3(256), 0, h->stream, h->dP, d, h->B, h->has_prev ? 1 : 0, h->tprev,
                           h->xs_prev, h->us_prev, h->t0, h->x0, h->xs, h->us, h->stats, h->done);
        UPR_HIP(hipGetLastError());
    } else {
        UPR_HIP(hipMemsetAsync(h->stats, 0, sizeof(double) * h->B * UPR_NSTATS, h->stream));
        UPR_HIP(hipMemsetAsync(h->done, 0, sizeof(int) * h->B, h->stream));
        h->guess_set = false;
    }
    for (int it = 0; it < sqp_iters; ++it) {
        { KernelTimer T(h, 0); if (launch_linearize(h, traj_lin_args(h))) return 1; T.stop(); }
        {
            upr_qp_args Q = make_qp_args(h);
            // the production kernel writes the feedback gains of the advance's LAST QP itself (no gather kernel afterwards)
            if (fba.kernel_writes && it == sqp_iters - 1) Q.fb = h->fb;
            if (h->order_on && h->order_valid) Q.order = h->order;
            // tracked value function: the advance's LAST QP exports its multipliers (exit-only code of the kernel, behind its step)
            if (h->vf_track && it == sqp_iters - 1 && h->qp.exported) { Q.kkt = h->kkt; Q.kkt_stride = h->qp.stride; }
            KernelTimer T(h, 1); if (launch_qp(h, Q)) return 1; T.stop();
        }
        if (h->vf_track && it == sqp_iters - 1) {
            // ... and the cost-to-go kernel reads that QP before the line search moves xs / us off its linearisation point
            const bool timed = h->timing != 0;   // (a timed handle never captures a tick graph: no event nodes in it)
            if (timed) UPR_HIP(hipEventRecord(h->vf_ev[0], h->stream));
            hipLaunchKernelGGL(upr_value_kernel, dim3(h->B), dim3(UPR_VF_NT), vf_lds_bytes(h), h->stream, make_vf_args(h));
            UPR_HIP(hipGetLastError());
            if (timed) { UPR_HIP(hipEventRecord(h->vf_ev[1], h->stream)); h->vf_ms_pending = true; }
            UPR_HIP(hipMemcpyAsync(h->vf_t0, h->t0, sizeof(double) * h->B, hipMemcpyDeviceToDevice, h->stream));
            h->vf_state = 1; h->vf_tracked = true;
        }
        upr_ls_args L;
        L.P = h->dP; L.d = d; L.xs = h->xs; L.us = h->us; L.x0 = h->x0; L.t0 = h->t0; L.body_params = h->body_params;
        L.way_p = h->way_p; L.way_q = upr_has_orientation_cost(&h->P) ? h->way_q : nullptr; L.lin = h->lin; L.ws = h->ws; L.stats = h->stats; L.done = h->done; L.iter = it; L.dyn = h->dyn0; L.pflag = h->pflag;
        // folded into the line search's launch: the dispatch order of the next QP (rounds 2 - 3a: a one-workgroup counting sort
        // of its own) and, behind the advance's last line search, the copy of the solution the next warm start reads
        if (h->order_on) { L.order_out = h->order; L.iter_key = h->iter_key; }
        if (it == sqp_iters - 1) { L.xs_prev = h->xs_prev; L.us_prev = h->us_prev; L.tprev = h->tprev; }
        { KernelTimer T(h, 2); if (launch_linesearch(h, L)) return 1; T.stop(); }
        if (h->order_on) h->order_valid = true;
    }
    if (fba.gather_after && fb_gather(h)) return 1;   // UPR_FB_FUSED set: the gains of the last QP with every advance
    if (h->fb_on) h->fbt.state = fba.state;
    h->hdyn_prev = h->hdyn0;
    // remember the solution for the next warm start / policy evaluation (the last line search did, unless there was none)
    if (sqp_iters <= 0) {
        UPR_HIP(hipMemcpyAsync(h->xs_prev, h->xs, sizeof(double) * h->B * (d.N + 1) * d.nx, hipMemcpyDeviceToDevice, h->stream));
        UPR_HIP(hipMemcpyAsync(h->us_prev, h->us, sizeof(double) * h->B * d.N * d.nu, hipMemcpyDeviceToDevice, h->stream));
        UPR_HIP(hipMemcpyAsync(h->tprev, h->t0, sizeof(double) * h->B, hipMemcpyDeviceToDevice, h->stream));
    }
    h->has_prev = true;
    return 0;
}

// ---- what several entries share -------------------------------------------------------------------------------------------
// the time of every instance: t[B], or one time for all (t_stride == 0)
void instance_times(int B, const double* t, int t_stride, double* out) {
    for (int b = 0; b < B; ++b) out[b] = t[(size_t)b * (t_stride ? 1 : 0)];
}
// scratch of the evaluate / evaluate_policy / tick calls (per-tick path of the closed loop: preallocated in the handle on first use)
int eval_scratch(upr_batch* h) {
    const size_t B = (size_t)h->B, nx = (size_t)h->d.nx, nu = (size_t)h->d.nu;
    if (!h->ev_t && (dev_alloc(&h->ev_t, B) || dev_alloc(&h->ev_xo, B * nx) || dev_alloc(&h->ev_x, B * (nx + nu)))) return 1;
    h->ev_u = h->ev_x + B * nx;   // (one block: a control period copies both out in one piece)
    return 0;
}
// statistics and dispatch keys of a handle whose stream is idle, into a snapshot and back
int snapshot_take(upr_batch* h, upr_stats_snapshot& s) {
    s.stats.resize((size_t)h->B * UPR_NSTATS); s.keys.resize(((size_t)h->B + 3) & ~(size_t)3);
    UPR_HIP(hipMemcpy(s.stats.data(), h->stats, sizeof(double) * s.stats.size(), hipMemcpyDeviceToHost));
    UPR_HIP(hipMemcpy(s.keys.data(), h->iter_key, s.keys.size(), hipMemcpyDeviceToHost));
    return 0;
}
int snapshot_put_back(upr_batch* h, const upr_stats_snapshot& s) {
    UPR_HIP(hipMemcpy(h->stats, s.stats.data(), sizeof(double) * s.stats.size(), hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(h->iter_key, s.keys.data(), s.keys.size(), hipMemcpyHostToDevice));
    return 0;
}
// the points of a query (value function, multipliers, linearisation): instance and time of each, checked and on the device for the call
struct point_upload {
    DevBuf<int> inst; DevBuf<double> t;
    int up(const upr_batch* h, int n, const int* hinst, const double* ht) {
        for (int i = 0; i < n; ++i) if (hinst[i] < 0 || hinst[i] >= h->B) return upr_fail("instance index out of range");
        if (inst.alloc(n) || t.alloc(n)) return 1;
        UPR_HIP(hipMemcpy(inst, hinst, sizeof(int) * n, hipMemcpyHostToDevice));
        UPR_HIP(hipMemcpy(t, ht, sizeof(double) * n, hipMemcpyHostToDevice));
        return 0;
    }
};

}  // namespace

extern "C" {

const char* upr_last_error(void) { return g_err.c_str(); }

int upr_device_available(void) {
    int n = 0;
    return (hipGetDeviceCount(&n) == hipSuccess && n > 0) ? 1 : 0;
}

int upr_core_object_dynamics(const upr_problem* P, const double* body_params, int n, const double* forces, const double* C,
                             const double* w, const double* al, const double* a, double* out) {
    if (need_device()) return 1;
    if (!P || P->nb < 1 || P->nb > UPR_MAX_BODIES || P->nc < 0 || P->nc > UPR_MAX_CONTACTS) return upr_fail("bad problem dims");
    if (n <= 0) return 0;
    const int nfc = P->nf * P->nc, nb = P->nb;
    DevBuf<upr_problem> dP; DevBuf<double> dbp, df, dC, dw, dal, da, dout;
    if (dP.alloc(1) || dbp.alloc((size_t)nb * 10) || df.alloc((size_t)n * nfc + 1) || dC.alloc((size_t)n * 9) || dw.alloc((size_t)n * 3) ||
        dal.alloc((size_t)n * 3) || da.alloc((size_t)n * 3) || dout.alloc((size_t)n * 6 * nb)) return 1;
    UPR_HIP(hipMemcpy(dP, P, sizeof(upr_problem), hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(dbp, body_params, sizeof(double) * nb * 10, hipMemcpyHostToDevice));
    if (nfc) UPR_HIP(hipMemcpy(df, forces, sizeof(double) * n * nfc, hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(dC, C, sizeof(double) * n * 9, hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(dw, w, sizeof(double) * n * 3, hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(dal, al, sizeof(double) * n * 3, hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(da, a, sizeof(double) * n * 3, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(core_object_dynamics_kernel, dim3((n + 63) / 64), dim3(64), 0, 0, dP.p, dbp.p, n, df.p, dC.p, dw.p, dal.p, da.p, dout.p);
    UPR_HIP(hipGetLastError());
    UPR_HIP(hipMemcpy(out, dout, sizeof(double) * n * 6 * nb, hipMemcpyDeviceToHost));
    return 0;
}

int upr_core_friction_rows(const upr_problem* P, int n, const double* forces, double* out) {
    if (need_device()) return 1;
    if (!P || P->nc < 1 || P->nc > UPR_MAX_CONTACTS) return upr_fail("bad problem dims");
    if (n <= 0) return 0;
    DevBuf<upr_problem> dP; DevBuf<double> df, dout;
    if (dP.alloc(1) || df.alloc((size_t)n * 3 * P->nc) || dout.alloc((size_t)n * 5 * P->nc)) return 1;
    UPR_HIP(hipMemcpy(dP, P, sizeof(upr_problem), hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(df, forces, sizeof(double) * n * 3 * P->nc, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(core_friction_rows_kernel, dim3((n * P->nc + 63) / 64), dim3(64), 0, 0, dP.p, n, df.p, dout.p);
    UPR_HIP(hipGetLastError());
    UPR_HIP(hipMemcpy(out, dout, sizeof(double) * n * 5 * P->nc, hipMemcpyDeviceToHost));
    return 0;
}

upr_batch* upr_batch_create(const upr_problem* P, int B, const double* body_params, const double* way_p) {
    if (check_problem(P)) return nullptr;
    if (B < 1) { upr_fail("B must be >= 1"); return nullptr; }
    if (need_device()) return nullptr;
    upr_batch* h = new upr_batch();
    if (hipGetDevice(&h->device) != hipSuccess) { upr_fail("hipGetDevice failed"); delete h; return nullptr; }
    h->P = *P; h->d = upr_make_dims(P); h->B = B;
    h->nxf = (int)upr_iface_width(h->d.nx, P->n_dyn);
    h->hdyn0.assign((size_t)B * upr_iface_dyn_width(P->n_dyn), 0.0); h->hdyn_prev = h->hdyn0;
    const upr_dims& d = h->d;
    if (d.nx > UPR_LPK) { upr_fail("nx exceeds the 32 tangent lanes of the linearisation kernel"); delete h; return nullptr; }
    {   // the QP kernel of this handle (upr_qp_select.h): planned from the problem and the knobs, a run-time instantiation made where the
        // plan asks for one, then resolved into the record every later site reads
        upr_qp_knobs k;
        if (const char* e = getenv("UPR_QP_KERNEL")) k.qp_kernel = atoi(e);
        if (const char* e = getenv("UPR_QP_GENERIC")) k.qp_generic = atoi(e) != 0;
        if (const char* e = getenv("UPR_QP3_JIT")) k.qp3_jit = atoi(e);
        if (const char* e = getenv("UPR_QP_NT")) { k.qp_nt_set = true; k.qp_nt = atoi(e); }
        if (const char* e = getenv("UPR_QP_GENERIC_NT")) { k.generic_nt_set = true; k.generic_nt = atoi(e); }
        if (const char* e = getenv("UPR_JIT_NT")) k.jit_nt = atoi(e);
        if (const char* e = getenv("UPR_FB_FUSED")) { k.fb_fused = atoi(e) != 0; h->fbt.mode = UPR_FB_EAGER; }
        h->fb_on = P->use_feedback_policy != 0;
        upr_qp_sel& s = h->qp;
        static_cast<upr_qp_choice&>(s) = upr_qp_plan(*P, d, k);
        if (s.source == UPR_QP_FROM_RUN_TIME && s.structure == UPR_QP_STRUCT_PRODUCTION && jit_get(s.cfg, s.nt, &s.jit) != 0) {
            // a shape outside the list whose instantiation failed: falls back with a note
            static_cast<upr_qp_choice&>(s) = upr_qp_plan(*P, d, k, false);
            fprintf(stderr, "libupright_mi: %s -- using the %s kernel instead\n", g_err.c_str(), s.structure == UPR_QP_STRUCT_SECOND ? "second-structure" : "generic");
        }
        qp_resolve(s, *P, d);
        h->d.ws_stride = s.ws_stride;
    }
    if (upr_launch_resolve(h)) { delete h; return nullptr; }   // ... and its linearisation and line-search kernels (upr_api_launch.hip)
    if (const char* e = getenv("UPR_QP_ORDER")) h->order_on = atoi(e) != 0;
    upr_bal_resolve(h);   // ... and the form of its balance family (upr_api_balance.hip)
    auto bad = [&]() { upr_batch_destroy(h); return (upr_batch*)nullptr; };
    if (hipStreamCreate(&h->stream) != hipSuccess) { upr_fail("hipStreamCreate failed"); return bad(); }
    if (hipMalloc((void**)&h->dP, sizeof(upr_problem)) != hipSuccess) { upr_fail("hipMalloc failed"); return bad(); }
    hipMemcpy(h->dP, P, sizeof(upr_problem), hipMemcpyHostToDevice);
    const size_t n1 = d.N + 1;
    if (dev_alloc(&h->body_params, (size_t)B * d.nb * 10) || dev_alloc(&h->way_p, (size_t)B * P->n_way * 3) || dev_alloc(&h->way_q, (size_t)B * P->n_way * 4) ||
        // (observation: time, state and the dynamic obstacles' states in ONE block, [t B][x B nx][dyn B 9 n_dyn] -- a control period
        //  copies it in one piece, upr_batch_tick)
        dev_alloc(&h->t0, (((size_t)B + 1) & ~(size_t)1) + (size_t)B * d.nx + (size_t)B * upr_iface_dyn_width(P->n_dyn)) || dev_alloc(&h->xs, (size_t)B * n1 * d.nx) || dev_alloc(&h->us, (size_t)B * d.N * d.nu) ||
        dev_alloc(&h->xs_prev, (size_t)B * n1 * d.nx) || dev_alloc(&h->us_prev, (size_t)B * d.N * d.nu) || dev_alloc(&h->tprev, B) ||
        dev_alloc(&h->lin, (size_t)B * n1 * d.lin_stride) || dev_alloc(&h->Df, (size_t)B * d.ne * d.nfc) ||
        dev_alloc(&h->ws, (size_t)B * d.ws_stride) || dev_alloc(&h->stats, (size_t)B * UPR_NSTATS) || dev_alloc(&h->done, B) || dev_alloc(&h->order, B) || dev_alloc(&h->iter_key, ((size_t)B + 3) & ~(size_t)3) ||
        (h->fb_on && h->fbt.mode == UPR_FB_EAGER && dev_alloc(&h->fb, (size_t)B * d.N * d.nu * d.nx)) ||
        (P->n_dyn && dev_alloc(&h->pflag, B)))
        return bad();
    h->x0 = h->t0 + (((size_t)B + 1) & ~(size_t)1);   // (the states stay 16-byte aligned)
    if (P->n_dyn) h->dyn0 = h->x0 + (size_t)B * d.nx;
    hipMemcpy(h->body_params, body_params, sizeof(double) * B * d.nb * 10, hipMemcpyHostToDevice);
    hipMemcpy(h->way_p, way_p, sizeof(double) * B * P->n_way * 3, hipMemcpyHostToDevice);
    {   // target orientations default to the identity quaternion (xyzw) until upr_batch_set_target_orientations
        std::vector<double> qi((size_t)B * P->n_way * 4, 0.0);
        for (size_t i = 3; i < qi.size(); i += 4) qi[i] = 1.0;
        hipMemcpy(h->way_q, qi.data(), sizeof(double) * qi.size(), hipMemcpyHostToDevice);
    }
    // constant d(object_dynamics)/d(forces): unit forces through the wrench map (contact_constraints.h:107-157),
    // divided by the body mass and sqrt(6 nb) (balancing_constraints.cpp:144-151), sign of (GIF - F)
    h->hDf.assign((size_t)B * d.ne * d.nfc, 0.0);
    std::vector<double> unit(d.nfc), Fw(6 * d.nb);
    const double scale = 1.0 / std::sqrt(6.0 * d.nb);
    for (int b = 0; b < B; ++b) {
        const double* bp = body_params + (size_t)b * d.nb * 10;
        for (int j = 0; j < d.nfc; ++j) {
            std::fill(unit.begin(), unit.end(), 0.0);
            unit[j] = 1.0;
            upr_object_wrenches(P, bp, unit.data(), Fw.data());
            for (int bb = 0; bb < d.nb; ++bb)
                for (int r = 0; r < 6; ++r) h->hDf[((size_t)b * d.ne + 6 * bb + r) * d.nfc + j] = -scale * Fw[6 * bb + r] / bp[10 * bb];
        }
    }
    hipMemcpy(h->Df, h->hDf.data(), sizeof(double) * h->hDf.size(), hipMemcpyHostToDevice);
    if (hipDeviceSynchronize() != hipSuccess) { upr_fail("device synchronisation failed in create"); return bad(); }
    return h;
}

void upr_batch_destroy(upr_batch* h) {
    if (!h) return;
    hipFree(h->dP); hipFree(h->body_params); hipFree(h->way_p); hipFree(h->way_q); hipFree(h->t0) /* (x0 and dyn0 live in the same block) */; hipFree(h->xs); hipFree(h->us);
    if (h->fb) hipFree(h->fb);
    if (h->pflag) hipFree(h->pflag);
    hipFree(h->xs_prev); hipFree(h->us_prev); hipFree(h->tprev); hipFree(h->lin); hipFree(h->Df); hipFree(h->ws); hipFree(h->stats);
    hipFree(h->done); hipFree(h->order); hipFree(h->iter_key); if (h->pin) (void)hipHostFree(h->pin); if (h->tick_exec) (void)hipGraphExecDestroy(h->tick_exec); hipFree(h->prof); hipFree(h->kkt);
    hipFree(h->vf_P); hipFree(h->vf_p); hipFree(h->vf_J); hipFree(h->vf_X); hipFree(h->vf_t0); hipFree(h->vf_nu);
    for (hipEvent_t e : h->vf_ev) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->bal_ev) if (e) (void)hipEventDestroy(e);
    hipFree(h->bal_buf);
    hipFree(h->ev_t); hipFree(h->ev_xo); hipFree(h->ev_x) /* (ev_u: same block) */;
    for (hipEvent_t e : h->ev_pool) (void)hipEventDestroy(e);
    for (hipEvent_t e : h->ev_free) (void)hipEventDestroy(e);
    if (h->stream) hipStreamDestroy(h->stream);
    delete h;
}

int upr_batch_reset(upr_batch* h, const double* way_p) {
    UPR_ENTER(h);
    if (way_p) UPR_HIP(hipMemcpyAsync(h->way_p, way_p, sizeof(double) * h->B * h->P.n_way * 3, hipMemcpyHostToDevice, h->stream));
    h->has_prev = false;
    UPR_HIP(hipStreamSynchronize(h->stream));
    h->guess_set = false;
    if (h->vf_state) h->vf_state = 2;
    return 0;
}

int upr_batch_set_target_orientations(upr_batch* h, const double* way_q) {
    UPR_ENTER(h);
    if (!way_q) return upr_fail("upr_batch_set_target_orientations: way_q is NULL");
    std::vector<double> q(way_q, way_q + (size_t)h->B * h->P.n_way * 4);
    for (size_t i = 0; i < q.size(); i += 4) {   // unit quaternions (the reference builds Quatd from the target's coefficients)
        const double n = std::sqrt(q[i] * q[i] + q[i + 1] * q[i + 1] + q[i + 2] * q[i + 2] + q[i + 3] * q[i + 3]);
        if (!(n > 0)) return upr_fail("upr_batch_set_target_orientations: zero quaternion");
        for (int c = 0; c < 4; ++c) q[i + c] /= n;
    }
    UPR_HIP(hipMemcpyAsync(h->way_q, q.data(), sizeof(double) * q.size(), hipMemcpyHostToDevice, h->stream));
    UPR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

static int set_observation_core(upr_batch* h, const double* t, int t_stride, const double* x) {
    if (h->vf_state && !h->vf_tracked) h->vf_state = 2;   // (a tracked cost-to-go belongs to the solve: valid until the next advance)
    std::vector<double> tt(h->B);
    instance_times(h->B, t, t_stride, tt.data());
    UPR_HIP(hipMemcpyAsync(h->t0, tt.data(), sizeof(double) * h->B, hipMemcpyHostToDevice, h->stream));
    UPR_HIP(hipMemcpyAsync(h->x0, x, sizeof(double) * h->B * h->d.nx, hipMemcpyHostToDevice, h->stream));
    UPR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

static int set_guess_core(upr_batch* h, const double* xs, const double* us) {
    if (h->vf_state) h->vf_state = 2;
    const upr_dims& d = h->d;
    UPR_HIP(hipMemcpyAsync(h->xs, xs, sizeof(double) * h->B * (d.N + 1) * d.nx, hipMemcpyHostToDevice, h->stream));
    UPR_HIP(hipMemcpyAsync(h->us, us, sizeof(double) * h->B * d.N * d.nu, hipMemcpyHostToDevice, h->stream));
    UPR_HIP(hipStreamSynchronize(h->stream));
    h->guess_set = true;
    return 0;
}

int upr_batch_set_sqp_iterations(upr_batch* h, int n) {
    UPR_ENTER(h);
    if (n < 0 || n > 1000) return upr_fail("upr_batch_set_sqp_iterations: n out of range");
    h->sqp_iters_next = n;
    return 0;
}

int upr_batch_advance_async(upr_batch* h) {
    UPR_ENTER(h);
    return advance_impl(h);
}

int upr_batch_sync(upr_batch* h) {
    UPR_ENTER(h);
    UPR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

int upr_batch_advance(upr_batch* h) {
    UPR_ENTER(h);
    auto t0 = std::chrono::steady_clock::now();
    if (advance_impl(h)) return 1;
    UPR_HIP(hipStreamSynchronize(h->stream));
    h->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return 0;
}

static int get_solution_core(upr_batch* h, double* ts, double* xs, double* us) {
    const upr_dims& d = h->d;
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (ts) {
        std::vector<double> t0(h->B);
        UPR_HIP(hipMemcpy(t0.data(), h->t0, sizeof(double) * h->B, hipMemcpyDeviceToHost));
        for (int b = 0; b < h->B; ++b) for (int k = 0; k <= d.N; ++k) ts[(size_t)b * (d.N + 1) + k] = t0[b] + k * h->P.dt;
    }
    if (xs) UPR_HIP(hipMemcpy(xs, h->xs, sizeof(double) * h->B * (d.N + 1) * d.nx, hipMemcpyDeviceToHost));
    if (us) UPR_HIP(hipMemcpy(us, h->us, sizeof(double) * h->B * d.N * d.nu, hipMemcpyDeviceToHost));
    return 0;
}

// the plan at the times t: evaluate, or (policy) evaluate_policy at the observed robot states x_obs[B][nx]
static int evaluate_core(upr_batch* h, const double* t, int t_stride, bool policy, const double* x_obs, double* x_out, double* u_out) {
    if (policy && !h->fb_on) return upr_fail("upr_batch_evaluate_policy: the batch was created with use_feedback_policy = 0");
    const upr_dims& d = h->d;
    if (eval_scratch(h)) return 1;
    std::vector<double> tt(h->B);
    instance_times(h->B, t, t_stride, tt.data());
    UPR_HIP(hipMemcpyAsync(h->ev_t, tt.data(), sizeof(double) * h->B, hipMemcpyHostToDevice, h->stream));
    if (policy) {
        UPR_HIP(hipMemcpyAsync(h->ev_xo, x_obs, sizeof(double) * h->B * d.nx, hipMemcpyHostToDevice, h->stream));
        if (launch_policy(h, h->ev_t, h->ev_xo)) return 1;
    } else hipLaunchKernelGGL(evaluate_kernel, dim3(h->B), dim3(64), 0, h->stream, h->dP, d, h->B, h->tprev, h->xs_prev, h->us_prev, h->ev_t, 1, h->ev_x, h->ev_u);
    UPR_HIP(hipGetLastError());
    UPR_HIP(hipMemcpyAsync(x_out, h->ev_x, sizeof(double) * h->B * d.nx, hipMemcpyDeviceToHost, h->stream));
    UPR_HIP(hipMemcpyAsync(u_out, h->ev_u, sizeof(double) * h->B * d.nu, hipMemcpyDeviceToHost, h->stream));
    UPR_HIP(hipStreamSynchronize(h->stream));
    return 0;
}

static int get_feedback_core(upr_batch* h, double* K) {
    if (!h->fb_on) return upr_fail("upr_batch_get_feedback: the batch was created with use_feedback_policy = 0");
    const upr_dims& d = h->d;
    if (fb_keep(h)) return 1;   // the first request after an advance gathers the array; later ones only copy
    if (!h->fb && dev_alloc(&h->fb, (size_t)h->B * d.N * d.nu * d.nx)) return 1;   // (no solve yet: zeros)
    UPR_HIP(hipStreamSynchronize(h->stream));
    UPR_HIP(hipMemcpy(K, h->fb, sizeof(double) * h->B * d.N * d.nu * d.nx, hipMemcpyDeviceToHost));
    return 0;
}

double upr_batch_last_solve_ms(const upr_batch* h) { return h ? h->last_ms : 0.0; }

const char* upr_batch_qp_kernel_name(const upr_batch* h) { return h ? h->qp.name : ""; }

const char* upr_batch_ls_kernel_name(upr_batch* h) {
    if (!h || !h->ls_launched) return "";   // (none before the first launch)
    return h->ls_sel.name;
}

const char* upr_batch_lin_kernel_name(upr_batch* h) {
    if (!h || h->lin_blocks_last < 0) return "";
    upr_lin_name(h->lin_sel, h->lin_blocks_last, h->lin_sel.name, sizeof(h->lin_sel.name));
    return h->lin_sel.name;
}

/* restore == 0: keep a copy of the per-instance statistics and of the QP dispatch keys of the last advance; restore != 0: put that
 * copy back.  Brackets a query that solves one more QP on the handle (upr_batch_qp_kkt behind valueFunction): afterwards
 * upr_batch_get_stats and the longest-first dispatch order describe the SOLVE again, not the query's QP. */
int upr_batch_hold_stats(upr_batch* h, int restore) {
    UPR_ENTER(h);
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (!restore) return snapshot_take(h, h->held);
    if (h->held.stats.empty()) return upr_fail("upr_batch_hold_stats: nothing held on this handle");
    if (fb_keep(h)) return 1;   // (the QP status the gains' readers consult is overwritten below)
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (snapshot_put_back(h, h->held)) return 1;
    h->held = upr_stats_snapshot();
    return 0;
}

int upr_batch_get_stats(upr_batch* h, double* stats) {
    UPR_ENTER(h);
    UPR_HIP(hipStreamSynchronize(h->stream));
    UPR_HIP(hipMemcpy(stats, h->stats, sizeof(double) * h->B * UPR_NSTATS, hipMemcpyDeviceToHost));
    return 0;
}

// points mode of the linearisation kernel: records of n arbitrary (x, u) pairs, x[n][nxf] interface states, back on the host
static int linearize_points_impl(upr_batch* h, int n, const int* inst, const double* t, const double* x, const double* u, std::vector<double>& rec, double* ee) {
    const upr_dims& d = h->d;
    const size_t nd = upr_iface_dyn_width(h->P.n_dyn);
    point_upload pts;
    if (pts.up(h, n, inst, t)) return 1;
    std::vector<double> xr, dyn;
    if (h->P.n_dyn) {   // interface states: the robot block is the point, the obstacle block the obstacles' state at that point
        xr.resize((size_t)n * d.nx); dyn.resize((size_t)n * nd);
        upr_iface_split(d.nx, h->P.n_dyn, x, (size_t)n, xr.data(), dyn.data());
        x = xr.data();
    }
    DevBuf<double> dx, du, dlin, dee, ddyn;
    if (dx.alloc((size_t)n * d.nx) || du.alloc((size_t)n * d.nu) || dlin.alloc((size_t)n * d.lin_stride) || dee.alloc((size_t)n * 3)) return 1;
    UPR_HIP(hipMemcpy(dx, x, sizeof(double) * n * d.nx, hipMemcpyHostToDevice));
    UPR_HIP(hipMemcpy(du, u, sizeof(double) * n * d.nu, hipMemcpyHostToDevice));
    upr_lin_args A;
    A.P = h->dP; A.d = d; A.body_params = h->body_params; A.way_p = h->way_p; A.way_q = upr_has_orientation_cost(&h->P) ? h->way_q : nullptr; A.t0 = pts.t; A.xs = dx; A.us = du; A.inst = pts.inst;
    A.lin = dlin; A.ee_out = dee; A.npoints = n; A.Df = h->Df;
    if (h->P.n_dyn) {   // points mode: the obstacle state of every point as given
        if (ddyn.alloc((size_t)n * nd)) return 1;
        UPR_HIP(hipMemcpy(ddyn, dyn.data(), sizeof(double) * n * nd, hipMemcpyHostToDevice));
        A.dyn = ddyn; A.pflag = h->pflag;
    }
    if (launch_linearize(h, A)) return 1;
    UPR_HIP(hipStreamSynchronize(h->stream));
    rec.assign((size_t)n * d.lin_stride, 0.0);
    UPR_HIP(hipMemcpy(rec.data(), dlin, sizeof(double) * rec.size(), hipMemcpyDeviceToHost));
    if (ee) UPR_HIP(hipMemcpy(ee, dee, sizeof(double) * n * 3, hipMemcpyDeviceToHost));
    return 0;
}

int upr_batch_linearize_points(upr_batch* h, int n, const int* inst, const double* t, const double* x, const double* u,
                               double* g, double* gx, double* cost, double* grad, double* hess, double* ee) {
    UPR_ENTER(h);
    if (n <= 0) return 0;
    const upr_dims& d = h->d;
    std::vector<double> rec;
    if (linearize_points_impl(h, n, inst, t, x, u, rec, ee)) return 1;   // (Jacobian outputs keep the 3 nq robot columns)
    for (int i = 0; i < n; ++i) {
        const double* r = rec.data() + (size_t)i * d.lin_stride;
        if (g) std::memcpy(g + (size_t)i * d.ne, r + d.lin_g, sizeof(double) * d.ne);
        if (gx) std::memcpy(gx + (size_t)i * d.ne * d.nx, r + d.lin_gx, sizeof(double) * d.ne * d.nx);
        if (cost) cost[i] = r[d.lin_cost];
        if (grad) std::memcpy(grad + (size_t)i * d.nq, r + d.lin_grad, sizeof(double) * d.nq);
        if (hess) for (int a = 0; a < d.nq; ++a) for (int c = 0; c < d.nq; ++c) hess[((size_t)i * d.nq + a) * d.nq + c] = r[d.lin_hess + upr_tri(d.nq, a, c)];
    }
    return 0;
}

// the first `nr` state rows (slot order of the record) at n points (inst[n], t[n], interface states x[n][nx_full]): d[n][nr], dq[n][nr][nq]
static int state_rows_impl(upr_batch* h, int n, const int* inst, const double* t, const double* x, int nr, double* dd, double* dq) {
    const upr_dims& d = h->d;
    std::vector<double> u((size_t)n * d.nu, 0.0), rec;
    if (linearize_points_impl(h, n, inst, t, x, u.data(), rec, nullptr)) return 1;
    for (int i = 0; i < n; ++i) {
        const double* r = rec.data() + (size_t)i * d.lin_stride + d.lin_obs;
        std::memcpy(dd + (size_t)i * nr, r, sizeof(double) * nr);
        if (dq) std::memcpy(dq + (size_t)i * nr * d.nq, r + d.no, sizeof(double) * nr * d.nq);   // (row r's gradient: r + no + r nq)
    }
    return 0;
}

int upr_batch_obstacle_rows(upr_batch* h, int n, const double* x, double* dd, double* dq) {
    UPR_ENTER(h);
    const upr_dims& d = h->d;
    if (d.nsr == 0) return upr_fail("upr_batch_obstacle_rows: the problem has no collision pairs / projectile rows");
    if (n <= 0) return 0;
    std::vector<int> inst(n, 0);
    std::vector<double> t(n, 0.0);
    return state_rows_impl(h, n, inst.data(), t.data(), x, d.nsr, dd, dq);
}

int upr_batch_state_rows(upr_batch* h, int n, const int* inst, const double* t, const double* x, double* dd, double* dq) {
    UPR_ENTER(h);
    const upr_dims& d = h->d;
    if (d.no == 0) return upr_fail("upr_batch_state_rows: the problem has no state rows");
    if (n <= 0) return 0;
    return state_rows_impl(h, n, inst, t, x, d.no, dd, dq);   // (inst is checked where it is uploaded: point_upload)
}

int upr_batch_eq_input_jacobian(upr_batch* h, int inst, double* gu) {
    UPR_ENTER(h);
    if (inst < 0 || inst >= h->B) return upr_fail("instance index out of range");
    const upr_dims& d = h->d;
    for (int r = 0; r < d.ne; ++r) {
        for (int j = 0; j < d.nq; ++j) gu[(size_t)r * d.nu + j] = 0.0;
        for (int j = 0; j < d.nfc; ++j) gu[(size_t)r * d.nu + d.nq + j] = h->hDf[((size_t)inst * d.ne + r) * d.nfc + j];
    }
    return 0;
}

// linearise at the current trajectory and solve one QP there with the multiplier export (no synchronisation)
static int kkt_launch(upr_batch* h) {
    if (h->qp.exported && !h->kkt && dev_alloc(&h->kkt, (size_t)h->B * h->qp.stride)) return 1;
    if (fb_keep(h)) return 1;   // (records, workspace and statistics of the advance's last QP are overwritten below)
    if (launch_linearize(h, traj_lin_args(h))) return 1;
    upr_qp_args A = make_qp_args(h);
    if (h->qp.exported) { A.kkt = h->kkt; A.kkt_stride = h->qp.stride; }
    return launch_qp(h, A);
}

static int qp_step_core(upr_batch* h, double* dxs, double* dus) {
    const upr_dims& d = h->d;
    if (fb_keep(h)) return 1;   // (as kkt_launch)
    if (launch_linearize(h, traj_lin_args(h))) return 1;
    if (launch_qp(h, make_qp_args(h))) return 1;
    UPR_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> ws((size_t)h->B * d.ws_stride);
    UPR_HIP(hipMemcpy(ws.data(), h->ws, sizeof(double) * ws.size(), hipMemcpyDeviceToHost));
    for (int b = 0; b < h->B; ++b) {
        const double* w = ws.data() + (size_t)b * d.ws_stride;
        if (dxs) std::memcpy(dxs + (size_t)b * (d.N + 1) * d.nx, w + d.ws_dx, sizeof(double) * (d.N + 1) * d.nx);
        if (dus) std::memcpy(dus + (size_t)b * d.N * d.nu, w + d.ws_du, sizeof(double) * d.N * d.nu);
    }
    return 0;
}

/* One QP at the current trajectory with everything an independent KKT check needs: the step and the multipliers the
 * kernel ended with.  pi[B][N+1][nx] costates (pi_0 unused), nu[B][N][ne] stage-equality multipliers, yN[B][neN]
 * terminal-equality multipliers, lam[B][N+1][ni] inequality multipliers, ni = 2 nx + 2 nu + np + no in the slot order
 * [x lower][x upper][u lower][u upper][friction rows][collision / projectile rows]; *ni_out = ni.  Any pointer may be NULL.
 * (upr_batch_qp_kkt, "interface states" further down: dxs in robot width here, as qp_step_core's) */
static int qp_kkt_core(upr_batch* h, double* dxs, double* dus, double* pi, double* nu, double* yN, double* lam, int* ni_out) {
    const upr_dims& d = h->d;
    if (ni_out) *ni_out = d.ni_stage;
    const upr_qp_sel& sel = h->qp;   // (where the selected kernel left the primal-dual point: the export buffer or the workspace)
    if (kkt_launch(h)) return 1;
    UPR_HIP(hipStreamSynchronize(h->stream));
    std::vector<double> ws((size_t)h->B * d.ws_stride), kk;
    UPR_HIP(hipMemcpy(ws.data(), h->ws, sizeof(double) * ws.size(), hipMemcpyDeviceToHost));
    if (sel.exported) { kk.resize((size_t)h->B * sel.stride); UPR_HIP(hipMemcpy(kk.data(), h->kkt, sizeof(double) * kk.size(), hipMemcpyDeviceToHost)); }
    const int n1 = d.N + 1;
    for (int b = 0; b < h->B; ++b) {
        const double* w = ws.data() + (size_t)b * d.ws_stride;
        if (dxs) std::memcpy(dxs + (size_t)b * n1 * d.nx, w + d.ws_dx, sizeof(double) * n1 * d.nx);
        if (dus) std::memcpy(dus + (size_t)b * d.N * d.nu, w + d.ws_du, sizeof(double) * d.N * d.nu);
        const size_t nsl = (size_t)n1 * d.ni_stage;
        const double* m = (sel.exported ? kk.data() : ws.data()) + (size_t)b * sel.stride;
        const double *spi = m + sel.o_pi, *snu = m + sel.o_nu, *sy = m + sel.o_yN, *sl = m + sel.o_lam, *st = m + sel.o_t;
        const double* sp[3] = {nullptr, nullptr, nullptr};   // sigma, tau, gam of the softened rows (problems that have some)
        if (sel.o_sig >= 0) { sp[0] = m + sel.o_sig; sp[1] = m + sel.o_tau; sp[2] = m + sel.o_gam; }
        if (b == 0) {
            h->kkt_slack.assign((size_t)h->B * nsl, 1.0);
            h->kkt_pairs.assign(3 * (size_t)h->B * nsl, 0.0);
            std::fill(h->kkt_pairs.begin() + (size_t)h->B * nsl, h->kkt_pairs.begin() + 2 * (size_t)h->B * nsl, 1.0);   // (sigma 0, tau 1, gam 0 where a slot is not a softened row)
        }
        for (int k = 0; k < n1; ++k) for (int j = 0; j < d.ni_stage; ++j)
            if (upr_ineq_active(d, k, j)) {
                const size_t e = ((size_t)b * n1 + k) * d.ni_stage + j;
                h->kkt_slack[e] = st[(size_t)k * d.ni_stage + j];
                if (sp[0] && upr_slot_soft(&h->P, d, j)) for (int q = 0; q < 3; ++q) h->kkt_pairs[q * (size_t)h->B * nsl + e] = sp[q][(size_t)k * d.ni_stage + j];
            }
        if (pi) std::memcpy(pi + (size_t)b * n1 * d.nx, spi, sizeof(double) * n1 * d.nx);
        if (nu) std::memcpy(nu + (size_t)b * d.N * d.ne, snu, sizeof(double) * d.N * d.ne);
        if (yN && d.neN) std::memcpy(yN + (size_t)b * d.neN, sy, sizeof(double) * d.neN);
        if (lam) {
            // the generic kernels keep a multiplier value in slots that are not rows of the stage (x rows of knot 0, u rows of
            // knot N, collision rows outside knots 1 .. N-1): report 0 there
            for (int k = 0; k < n1; ++k) for (int j = 0; j < d.ni_stage; ++j)
                lam[((size_t)b * n1 + k) * d.ni_stage + j] = upr_ineq_active(d, k, j) ? sl[(size_t)k * d.ni_stage + j] : 0.0;
        }
    }
    return 0;
}

/* Slacks t of the inequality rows at the exit of the QP the last upr_batch_qp_kkt call solved, t[B][N+1][ni] in the slot order of its
 * lam (1 where a slot is not a row of the knot): lam / t are the barrier weights of the last interior-point iterate. */
int upr_batch_qp_slacks(upr_batch* h, double* t) {
    UPR_ENTER(h);
    if (h->kkt_slack.empty()) return upr_fail("upr_batch_qp_slacks: no upr_batch_qp_kkt call on this handle yet");
    if (t) std::memcpy(t, h->kkt_slack.data(), sizeof(double) * h->kkt_slack.size());
    return 0;
}

/* The slack pairs of the softened rows of that QP: sigma (the row's slack variable, cost 1/2 Z sigma^2 + z sigma), tau and gam (the
 * slack and the multiplier of sigma >= 0), each [B][N+1][ni] in the slot order of lam; sigma = 0, tau = 1, gam = 0 in slots that are
 * not softened rows of the knot.  A softened row is factored with the weight w0 (Z + gam / tau) / (Z + w0 + gam / tau), w0 = lam / t.
 * Any pointer may be NULL. */
int upr_batch_qp_slack_pairs(upr_batch* h, double* sigma, double* tau, double* gam) {
    UPR_ENTER(h);
    if (h->kkt_pairs.empty()) return upr_fail("upr_batch_qp_slack_pairs: no upr_batch_qp_kkt call on this handle yet");
    const size_t n = h->kkt_pairs.size() / 3;
    double* out[3] = {sigma, tau, gam};
    for (int q = 0; q < 3; ++q) if (out[q]) std::memcpy(out[q], h->kkt_pairs.data() + q * n, sizeof(double) * n);
    return 0;
}

/* ---- value function of the last QP, batched (upr_value.h) ---- */
int upr_batch_value_function_update_interface(upr_batch* h) {
    UPR_ENTER(h);
    if (!h->has_prev && !h->guess_set) return upr_fail("upr_batch_value_function_update: no plan on this handle yet (advance or set a guess first)");
    const upr_dims& d = h->d;
    const size_t B = (size_t)h->B;
    const size_t lds = vf_lds_bytes(h);
    if (lds > 160 * 1024) return upr_fail("upr_batch_value_function_update: working set exceeds 160 KiB of LDS");
    if (vf_alloc(h)) return 1;
    h->vf_state = 0; h->vf_tracked = false; h->vf_ms_pending = false;
    // statistics and dispatch keys of the solve are put back behind the query's QP (what upr_batch_hold_stats does, on a snapshot
    // of its own: a caller may hold the handle's across this call)
    upr_stats_snapshot solve;
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (snapshot_take(h, solve)) return 1;
    if (kkt_launch(h)) return 1;
    const upr_vf_args A = make_vf_args(h);
    if (lds > 64 * 1024) UPR_HIP(vf_raise_lds_limit());
    UPR_HIP(hipEventRecord(h->vf_ev[0], h->stream));
    hipLaunchKernelGGL(upr_value_kernel, dim3(h->B), dim3(UPR_VF_NT), lds, h->stream, A);
    UPR_HIP(hipGetLastError());
    UPR_HIP(hipEventRecord(h->vf_ev[1], h->stream));
    UPR_HIP(hipMemcpyAsync(h->vf_t0, h->t0, sizeof(double) * B, hipMemcpyDeviceToDevice, h->stream));
    UPR_HIP(hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    UPR_HIP(hipEventElapsedTime(&ms, h->vf_ev[0], h->vf_ev[1]));
    h->vf_ms = ms;
    if (snapshot_put_back(h, solve)) return 1;
    h->vf_state = 1;
    return 0;
}

/* The entry of before: robot-state shapes in every query that follows, so a handle with a dynamic obstacle (interface states) is
 * refused here -- upr_batch_value_function_update_interface is the same update for such a handle. */
int upr_batch_value_function_update(upr_batch* h) {
    UPR_ENTER(h);
    if (h->P.n_dyn) return upr_fail("upr_batch_value_function_update: not available with a dynamic obstacle (interface states): upr_batch_value_function_update_interface takes such a handle");
    return upr_batch_value_function_update_interface(h);
}

static int vf_ready(const upr_batch* h, const char* who) {
    if (h->vf_state == 0) return upr_fail(std::string(who) + ": no upr_batch_value_function_update on this handle yet");
    if (h->vf_state == 2) return upr_fail(std::string(who) + ": the cost-to-go is stale (the plan or the observation changed since upr_batch_value_function_update)");
    return 0;
}

/* Tracked mode: every advance (and tick) with at least one SQP iteration hands its own last QP to the cost-to-go kernel, in-stream
 * between that QP launch and its line search.  Never called inside an advance (between upr_batch_advance_async and upr_batch_sync). */
int upr_batch_track_value_function(upr_batch* h, int on) {
    UPR_ENTER(h);
    if (!on) {
        if (h->vf_track && h->vf_state) h->vf_state = 2;   // (what an advance tracked is dropped with the mode)
        h->vf_track = false; h->vf_tracked = false;
        return 0;
    }
    if (h->vf_track) return 0;
    const size_t lds = vf_lds_bytes(h);
    if (lds > 160 * 1024) return upr_fail("upr_batch_track_value_function: working set exceeds 160 KiB of LDS");
    if (vf_alloc(h)) return 1;
    if (h->qp.exported && !h->kkt && dev_alloc(&h->kkt, (size_t)h->B * h->qp.stride)) return 1;
    if (lds > 64 * 1024) UPR_HIP(vf_raise_lds_limit());
    h->vf_track = true;
    return 0;
}

int upr_batch_value_function(upr_batch* h, int n, const int* inst, const double* t, const double* x, double* V, double* dVdx) {
    UPR_ENTER(h);
    if (vf_ready(h, "upr_batch_value_function")) return 1;
    if (n <= 0) return 0;
    if (!inst || !t || !x) return upr_fail("upr_batch_value_function: null argument");
    const upr_dims& d = h->d;
    point_upload pts;
    if (pts.up(h, n, inst, t)) return 1;
    DevBuf<double> dx, dV, dg;
    if (dx.alloc((size_t)n * d.nx) || dV.alloc(n) || dg.alloc((size_t)n * d.nx)) return 1;
    std::vector<double> xr(h->P.n_dyn ? (size_t)n * d.nx : 0);
    if (h->P.n_dyn) {   // interface states: the robot block is what the expansion is in
        upr_iface_split(d.nx, h->P.n_dyn, x, (size_t)n, xr.data(), nullptr);
        x = xr.data();
    }
    UPR_HIP(hipMemcpy(dx, x, sizeof(double) * n * d.nx, hipMemcpyHostToDevice));
    upr_vfq_args A;
    A.d = d; A.dt = h->P.dt; A.n = n; A.inst = pts.inst; A.t = pts.t; A.x = dx; A.t0 = h->vf_t0;
    A.Pk = h->vf_P; A.pk = h->vf_p; A.J = h->vf_J; A.X = h->vf_X; A.V = dV; A.dV = dg;
    hipLaunchKernelGGL(upr_value_query_kernel, dim3(n), dim3(64), 0, h->stream, A);
    UPR_HIP(hipGetLastError());
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (V) UPR_HIP(hipMemcpy(V, dV, sizeof(double) * n, hipMemcpyDeviceToHost));
    if (dVdx && !h->P.n_dyn) UPR_HIP(hipMemcpy(dVdx, dg, sizeof(double) * n * d.nx, hipMemcpyDeviceToHost));
    else if (dVdx) {   // the obstacle is data of the QP, not a state of its Riccati recursion: zero block
        std::vector<double> gr((size_t)n * d.nx);
        UPR_HIP(hipMemcpy(gr.data(), dg, sizeof(double) * gr.size(), hipMemcpyDeviceToHost));
        upr_iface_join_zero(d.nx, h->P.n_dyn, gr.data(), (size_t)n, dVdx);
    }
    return 0;
}

/* nu(t) of the QP the cost-to-go belongs to, nu_out[n][ne]: multipliers of the object-dynamics rows, piecewise linear between the knots */
int upr_batch_equality_lagrangian(upr_batch* h, int n, const int* inst, const double* t, double* nu_out) {
    UPR_ENTER(h);
    if (vf_ready(h, "upr_batch_equality_lagrangian")) return 1;
    if (n <= 0) return 0;
    if (!inst || !t || !nu_out) return upr_fail("upr_batch_equality_lagrangian: null argument");
    const upr_dims& d = h->d;
    point_upload pts;
    if (pts.up(h, n, inst, t)) return 1;
    DevBuf<double> dn;
    if (dn.alloc((size_t)n * d.ne)) return 1;
    upr_vfq_args A;
    A.d = d; A.dt = h->P.dt; A.n = n; A.inst = pts.inst; A.t = pts.t; A.x = nullptr; A.t0 = h->vf_t0;
    A.Pk = h->vf_P; A.pk = h->vf_p; A.J = h->vf_J; A.X = h->vf_X; A.V = nullptr; A.dV = nullptr;
    A.nu = h->vf_nu; A.nu_q = dn;
    hipLaunchKernelGGL(upr_value_query_kernel, dim3(n), dim3(64), 0, h->stream, A);
    UPR_HIP(hipGetLastError());
    UPR_HIP(hipStreamSynchronize(h->stream));
    UPR_HIP(hipMemcpy(nu_out, dn, sizeof(double) * n * d.ne, hipMemcpyDeviceToHost));
    return 0;
}

int upr_batch_get_cost_to_go(upr_batch* h, double* Pk, double* pk, double* J, double* X) {
    UPR_ENTER(h);
    if (vf_ready(h, "upr_batch_get_cost_to_go")) return 1;
    const size_t B = (size_t)h->B, n1 = (size_t)h->d.N + 1, nx = (size_t)h->d.nx;
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (Pk) UPR_HIP(hipMemcpy(Pk, h->vf_P, sizeof(double) * B * n1 * nx * nx, hipMemcpyDeviceToHost));
    if (pk) UPR_HIP(hipMemcpy(pk, h->vf_p, sizeof(double) * B * n1 * nx, hipMemcpyDeviceToHost));
    if (J) UPR_HIP(hipMemcpy(J, h->vf_J, sizeof(double) * B * n1, hipMemcpyDeviceToHost));
    if (X) UPR_HIP(hipMemcpy(X, h->vf_X, sizeof(double) * B * n1 * nx, hipMemcpyDeviceToHost));
    return 0;
}

double upr_batch_value_function_ms(upr_batch* h) {
    if (!h) return 0.0;
    if (h->vf_ms_pending) {   // a tracked launch on a timed handle: its events are read here, after the advance (waits for the launch)
        float ms = 0.0f;
        if (hipEventSynchronize(h->vf_ev[1]) == hipSuccess && hipEventElapsedTime(&ms, h->vf_ev[0], h->vf_ev[1]) == hipSuccess) h->vf_ms = ms;
        h->vf_ms_pending = false;
    }
    return h->vf_ms;
}

int upr_batch_device_ptrs(upr_batch* h, void** xs, void** us) {
    UPR_ENTER(h);
    if (xs) *xs = h->xs;
    if (us) *us = h->us;
    return 0;
}

/* debug: per-phase cycle counters of the production QP kernel, prof[B][4 waves][16]; allocate on first use.  The stamps are compiled
 * into run-time instantiations only (UPR_QP3_JIT=2 UPR_JIT_FLAGS="-DUPR_QP3_PROF ..."): the library's own kernels carry none. */
int upr_batch_qp_profile(upr_batch* h, double* out) {
    UPR_ENTER(h);
    {
        const char* f = getenv("UPR_JIT_FLAGS");
        if (!h->qp.jit || !f || !strstr(f, "-DUPR_QP3_PROF"))
            return upr_fail("upr_batch_qp_profile: the phase stamps exist in run-time instantiations only: create the handle with UPR_QP3_JIT=2 UPR_JIT_FLAGS=-DUPR_QP3_PROF");
    }
    if (!h->prof) { if (dev_alloc(&h->prof, (size_t)h->B * 64)) return 1; return 0; }
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (out) UPR_HIP(hipMemcpy(out, h->prof, sizeof(double) * h->B * 64, hipMemcpyDeviceToHost));
    UPR_HIP(hipMemset(h->prof, 0, sizeof(double) * h->B * 64));
    return 0;
}

/* debug / test accessor: the per-knot linearisation records of the current trajectory, lin[B][N+1][stride] */
int upr_batch_get_lin(upr_batch* h, double* lin, int* stride) {
    UPR_ENTER(h);
    UPR_HIP(hipStreamSynchronize(h->stream));
    if (stride) *stride = h->d.lin_stride;
    if (lin) UPR_HIP(hipMemcpy(lin, h->lin, sizeof(double) * h->B * (h->d.N + 1) * h->d.lin_stride, hipMemcpyDeviceToHost));
    return 0;
}

int upr_batch_enable_timing(upr_batch* h, int on) {
    UPR_ENTER(h);
    h->timing = (on == 2 || on == 3) ? on : (on != 0 ? 1 : 0);
    h->timing_qp_count = 0;
    if (h->timing) while (h->ev_free.size() < 512) { hipEvent_t e; if (hipEventCreate(&e) != hipSuccess) break; h->ev_free.push_back(e); }
    for (int i = 0; i < 3; ++i) { h->k_ms[i] = 0; h->k_launches[i] = 0; }
    return 0;
}

int upr_batch_kernel_times(upr_batch* h, double* ms, int* launches) {
    UPR_ENTER(h);
    UPR_HIP(hipStreamSynchronize(h->stream));
    for (size_t i = 0; i < h->ev_slot.size(); ++i) {
        float t = 0;
        if (hipEventElapsedTime(&t, h->ev_pool[2 * i], h->ev_pool[2 * i + 1]) == hipSuccess) { h->k_ms[h->ev_slot[i]] += t; h->k_launches[h->ev_slot[i]] += 1; }
        h->ev_free.push_back(h->ev_pool[2 * i]); h->ev_free.push_back(h->ev_pool[2 * i + 1]);
    }
    h->ev_pool.clear(); h->ev_slot.clear();
    for (int i = 0; i < 3; ++i) {
        ms[i] = h->k_launches[i] ? h->k_ms[i] / h->k_launches[i] : 0.0;
        if (launches) launches[i] = h->k_launches[i];
    }
    return 0;
}

/* copy the current solution into caller-owned DEVICE buffers (e.g. torch tensors handed to an RCCL
 * all-gather): xs_dst[B][N+1][nx], us_dst[B][N][nu]; asynchronous on the engine's stream. */
int upr_batch_copy_solution_device(upr_batch* h, void* xs_dst, void* us_dst) {
    UPR_ENTER(h);
    const upr_dims& d = h->d;
    if (xs_dst) UPR_HIP(hipMemcpyAsync(xs_dst, h->xs, sizeof(double) * h->B * (d.N + 1) * d.nx, hipMemcpyDeviceToDevice, h->stream));
    if (us_dst) UPR_HIP(hipMemcpyAsync(us_dst, h->us, sizeof(double) * h->B * d.N * d.nu, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

int upr_batch_copy_policy_device(upr_batch* h, void* u_dst) {
    UPR_ENTER(h);
    if (!h->ev_u) return upr_fail("upr_batch_copy_policy_device: no tick has run on this handle");
    if (!u_dst) return upr_fail("upr_batch_copy_policy_device: null destination");
    UPR_HIP(hipMemcpyAsync(u_dst, h->ev_u, sizeof(double) * h->B * h->d.nu, hipMemcpyDeviceToDevice, h->stream));
    return 0;
}

void* upr_batch_stream(upr_batch* h) { return h ? (void*)h->stream : nullptr; }

int upr_set_device(int device) {
    if (need_device()) return 1;
    int n = 0;
    UPR_HIP(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) return upr_fail("upr_set_device: no such device");
    UPR_HIP(hipSetDevice(device));
    return 0;
}
int upr_batch_device(const upr_batch* h) { return h ? h->device : -1; }
long long upr_batch_ws_doubles(const upr_batch* h) { return h ? (long long)h->d.ws_stride : -1; }

/* forget the previous solution without a host synchronisation (cold start for the next advance) */
int upr_batch_reset_async(upr_batch* h) {
    UPR_ENTER(h);
    h->has_prev = false;
    h->guess_set = false;
    if (h->vf_state) h->vf_state = 2;
    return 0;
}


// ---- interface states: [robot x (3 nq) | r v a of every dynamic obstacle (9 n_dyn)], width nxf --------------------------------
// The kernels work on the robot state; the obstacles are uncontrolled (system_dynamics.h:29-39), so their part of every trajectory
// is the ballistic continuation of what was observed.  With n_dyn == 0 the entries hand the caller's pointers to their cores.
// Otherwise the layout is upr_iface.h's business:
//   upr_iface_split           what comes IN.  The obstacle block goes to hdyn0 (set_observation, tick), is the obstacles' state at
//                             the point (linearize_points, state_rows, obstacle_rows) or is ignored (set_guess, x_obs, value_function)
//   upr_iface_join_zero       what goes OUT as a function of the robot state alone: qp_step, qp_kkt (dx), get_feedback, dV/dx
//   upr_iface_join_ballistic  states that go OUT.  get_solution continues hdyn0, the LAST observation (the one the trajectory on the
//                             device is for), by k dt; evaluate(_policy) continue hdyn_prev, the observation the STORED solution
//                             belongs to (advance_impl copies hdyn0 there), by max(t - tprev, 0)
// tick returns the obstacle block as observed (upr_iface_join): its policy is evaluated at the observation's own time.
int upr_batch_set_observation(upr_batch* h, const double* t, int t_stride, const double* x) {
    UPR_ENTER(h);
    if (!h->P.n_dyn) return set_observation_core(h, t, t_stride, x);
    std::vector<double> xr((size_t)h->B * h->d.nx);
    upr_iface_split(h->d.nx, h->P.n_dyn, x, (size_t)h->B, xr.data(), h->hdyn0.data());
    UPR_HIP(hipMemcpy(h->dyn0, h->hdyn0.data(), sizeof(double) * h->hdyn0.size(), hipMemcpyHostToDevice));
    return set_observation_core(h, t, t_stride, xr.data());
}

int upr_batch_set_guess(upr_batch* h, const double* xs, const double* us) {
    UPR_ENTER(h);
    if (!h->P.n_dyn) return set_guess_core(h, xs, us);
    const size_t n = (size_t)h->B * (h->d.N + 1);
    std::vector<double> xr(n * h->d.nx);
    upr_iface_split(h->d.nx, h->P.n_dyn, xs, n, xr.data(), nullptr);
    return set_guess_core(h, xr.data(), us);
}

int upr_batch_get_solution(upr_batch* h, double* ts, double* xs, double* us) {
    UPR_ENTER(h);
    if (!h->P.n_dyn || !xs) return get_solution_core(h, ts, xs, us);
    const upr_dims& d = h->d;
    const size_t n1 = (size_t)d.N + 1, nd = upr_iface_dyn_width(h->P.n_dyn);
    std::vector<double> xr((size_t)h->B * n1 * d.nx);
    if (get_solution_core(h, ts, xr.data(), us)) return 1;
    for (size_t b = 0; b < (size_t)h->B; ++b) for (size_t k = 0; k < n1; ++k)
        upr_iface_join_ballistic(d.nx, h->P.n_dyn, xr.data() + (b * n1 + k) * d.nx, h->hdyn0.data() + b * nd, (int)k * h->P.dt, xs + (b * n1 + k) * h->nxf);
    return 0;
}

// evaluate and (policy) evaluate_policy
static int evaluate_iface(upr_batch* h, const double* t, int t_stride, bool policy, const double* x_obs, double* x_out, double* u_out) {
    if (!h->P.n_dyn) return evaluate_core(h, t, t_stride, policy, x_obs, x_out, u_out);
    const size_t B = (size_t)h->B, nx = (size_t)h->d.nx, nd = upr_iface_dyn_width(h->P.n_dyn);
    std::vector<double> xo(policy ? B * nx : 0), xr(B * nx), tp(B), tt(B);
    if (policy) upr_iface_split(h->d.nx, h->P.n_dyn, x_obs, B, xo.data(), nullptr);
    if (evaluate_core(h, t, t_stride, policy, xo.data(), xr.data(), u_out)) return 1;
    UPR_HIP(hipMemcpy(tp.data(), h->tprev, sizeof(double) * B, hipMemcpyDeviceToHost));
    instance_times(h->B, t, t_stride, tt.data());
    for (size_t b = 0; b < B; ++b) {
        const double tau = tt[b] - tp[b];
        upr_iface_join_ballistic(h->d.nx, h->P.n_dyn, xr.data() + b * nx, h->hdyn_prev.data() + b * nd, tau > 0.0 ? tau : 0.0, x_out + b * h->nxf);
    }
    return 0;
}
int upr_batch_evaluate(upr_batch* h, const double* t, int t_stride, double* x_out, double* u_out) {
    UPR_ENTER(h);
    return evaluate_iface(h, t, t_stride, false, nullptr, x_out, u_out);
}
int upr_batch_evaluate_policy(upr_batch* h, const double* t, int t_stride, const double* x_obs, double* x_out, double* u_out) {
    UPR_ENTER(h);
    return evaluate_iface(h, t, t_stride, true, x_obs, x_out, u_out);
}

int upr_batch_tick(upr_batch* h, const double* t, int t_stride, const double* x, double* x_out, double* u_out, double* stats_out) {
    UPR_ENTER(h);
    if (!t || !x || !x_out || !u_out) return upr_fail("upr_batch_tick: null argument");
    if (h->vf_state) h->vf_state = 2;
    const upr_dims& d = h->d;
    const size_t B = (size_t)h->B, nx = (size_t)d.nx, nu = (size_t)d.nu, ndyn = upr_iface_dyn_width(h->P.n_dyn);
    if (eval_scratch(h)) return 1;
    // pinned staging: [t B (+ pad)][x B nx][dyn B 9 n_dyn] in (the layout of the device block h->t0), [x B nx][u B nu][stats B NSTATS] out
    const size_t Bt = (B + 1) & ~(size_t)1;   // (the block of times is padded to an even count, as on the device)
    const size_t n_in = Bt + B * nx + B * ndyn, n_out = B * nx + B * nu + B * UPR_NSTATS;
    if (!h->pin) {
        UPR_HIP(hipHostMalloc((void**)&h->pin, sizeof(double) * (n_in + n_out), hipHostMallocDefault));
    }
    double* pt = h->pin; double* px = pt + Bt; double* pd = px + B * nx;
    double* ox = h->pin + n_in; double* ou = ox + B * nx; double* os = ou + B * nu;
    instance_times(h->B, t, t_stride, pt);
    upr_iface_split(d.nx, h->P.n_dyn, x, B, px, ndyn ? pd : nullptr);
    if (ndyn) std::memcpy(h->hdyn0.data(), pd, sizeof(double) * B * ndyn);
    auto t0c = std::chrono::steady_clock::now();
    // the stream operations of one control period
    auto enqueue = [&]() -> int {
        // (round 5: one copy in and one out -- device and pinned host blocks have the same layout -- instead of three each: a copy
        //  node of the period's graph costs about as much as a small kernel launch)
        UPR_HIP(hipMemcpyAsync(h->t0, pt, sizeof(double) * n_in, hipMemcpyHostToDevice, h->stream));
        if (advance_impl(h)) return 1;
        // the policy at the observation: time t0, state x0 (both already on the device)
        if (h->fb_on) { if (launch_policy(h, h->t0, h->x0)) return 1; }
        else hipLaunchKernelGGL(evaluate_kernel, dim3(h->B), dim3(64), 0, h->stream, h->dP, d, h->B, h->tprev, h->xs_prev, h->us_prev, h->t0, 1, h->ev_x, h->ev_u);
        UPR_HIP(hipGetLastError());
        UPR_HIP(hipMemcpyAsync(ox, h->ev_x, sizeof(double) * (B * nx + B * nu), hipMemcpyDeviceToHost, h->stream));
        if (stats_out) UPR_HIP(hipMemcpyAsync(os, h->stats, sizeof(double) * B * UPR_NSTATS, hipMemcpyDeviceToHost, h->stream));
        return 0;
    };
    if (h->tick_graph_on < 0) { const char* e = getenv("UPR_TICK_GRAPH"); h->tick_graph_on = (e && atoi(e) == 0) ? 0 : 1; }
    // what decides which operations a tick enqueues (advance_impl): warm start or not, a guess handed in, the SQP iteration count,
    // the dispatch order being valid, the feedback policy and who writes it, event timing, the statistics copy
    const int sqp_now = h->sqp_iters_next > 0 ? h->sqp_iters_next : h->P.sqp_iters;
    unsigned long long sig = 1469598103934665603ull;
    for (unsigned long long v : {(unsigned long long)h->has_prev, (unsigned long long)h->guess_set, (unsigned long long)sqp_now, (unsigned long long)(h->order_on && h->order_valid),
                                 (unsigned long long)h->fb_on, (unsigned long long)h->qp.fb_fused, (unsigned long long)h->fbt.mode /* (with sqp_now: which policy kernel the period enqueues) */, (unsigned long long)h->timing, (unsigned long long)(stats_out != nullptr),
                                 (unsigned long long)h->qp.structure, (unsigned long long)h->qp.source, (unsigned long long)h->qp.nt, (unsigned long long)(uintptr_t)h->pin,
                                 (unsigned long long)(uintptr_t)h->prof /* (passed BY VALUE in upr_qp_args: a graph captured before upr_batch_qp_profile allocated it would keep nullptr) */,
                                 (unsigned long long)h->vf_track /* (one more kernel node and one more copy node in the period) */}) { sig ^= v; sig *= 1099511628211ull; }
    // (... and, with the feedback policy, gains that are in the factors: the period then gathers and allocates nothing, and its policy
    //  kernel is the one every later period enqueues)
    const bool steady = h->tick_graph_on && !h->timing && h->has_prev && !h->guess_set && h->sqp_iters_next == 0 && (!h->order_on || h->order_valid) &&
                        (!h->fb_on || upr_fb_capturable(h->fbt, sqp_now));
    if (steady && h->tick_exec && sig == h->tick_sig) {
        UPR_HIP(hipGraphLaunch(h->tick_exec, h->stream));
        // (what advance_impl does on the host besides enqueueing)
        h->hdyn_prev = h->hdyn0;
        if (h->fb_on) h->fbt.state = upr_fb_on_replay(h->fbt, sqp_now, h->qp.fb_fused);
        if (h->vf_track && sqp_now > 0) { h->vf_state = 1; h->vf_tracked = true; }
        ++h->tick_replays;
    } else {
        if (h->tick_exec && sig != h->tick_sig) { (void)hipGraphExecDestroy(h->tick_exec); h->tick_exec = nullptr; h->tick_steady = 0; }
        h->tick_steady = (steady && sig == h->tick_sig) ? h->tick_steady + 1 : 0;
        h->tick_sig = sig;
        if (steady && h->tick_steady >= 2 && !h->tick_exec) {
            // third steady tick in a row: capture it, run the captured graph for this tick
            hipGraph_t g = nullptr;
            UPR_HIP(hipStreamBeginCapture(h->stream, hipStreamCaptureModeThreadLocal));
            const int rc = enqueue();
            const hipError_t ec = hipStreamEndCapture(h->stream, &g);
            if (rc || ec != hipSuccess || !g) { if (g) (void)hipGraphDestroy(g); h->tick_graph_on = 0; if (rc) return 1; if (enqueue()) return 1; }
            else {
                const hipError_t ei = hipGraphInstantiate(&h->tick_exec, g, nullptr, nullptr, 0);
                (void)hipGraphDestroy(g);
                if (ei != hipSuccess) { h->tick_exec = nullptr; h->tick_graph_on = 0; if (enqueue()) return 1; }
                else UPR_HIP(hipGraphLaunch(h->tick_exec, h->stream));
            }
        } else if (enqueue()) return 1;
    }
    UPR_HIP(hipStreamSynchronize(h->stream));
    h->last_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0c).count();
    upr_iface_join(d.nx, h->P.n_dyn, ox, pd, B, x_out);   // (evaluated at the observation's own time: the obstacle where it was observed)
    std::memcpy(u_out, ou, sizeof(double) * B * nu);
    if (stats_out) std::memcpy(stats_out, os, sizeof(double) * B * UPR_NSTATS);
    return 0;
}

long long upr_batch_tick_graph_replays(upr_batch* h) { return h ? h->tick_replays : 0; }

int upr_batch_get_feedback(upr_batch* h, double* K) {
    UPR_ENTER(h);
    if (!h->P.n_dyn) return get_feedback_core(h, K);
    const upr_dims& d = h->d;
    std::vector<double> Kr((size_t)h->B * d.N * d.nu * d.nx);
    if (get_feedback_core(h, Kr.data())) return 1;
    upr_iface_join_zero(d.nx, h->P.n_dyn, Kr.data(), (size_t)h->B * d.N * d.nu, K);   // the obstacle is not fed back: zero columns
    return 0;
}

int upr_batch_qp_step(upr_batch* h, double* dxs, double* dus) {
    UPR_ENTER(h);
    if (!h->P.n_dyn || !dxs) return qp_step_core(h, dxs, dus);
    const upr_dims& d = h->d;
    std::vector<double> xr((size_t)h->B * (d.N + 1) * d.nx);
    if (qp_step_core(h, xr.data(), dus)) return 1;
    upr_iface_join_zero(d.nx, h->P.n_dyn, xr.data(), (size_t)h->B * (d.N + 1), dxs);   // the obstacle is data of the QP: its step is zero
    return 0;
}

int upr_batch_qp_kkt(upr_batch* h, double* dxs, double* dus, double* pi, double* nu, double* yN, double* lam, int* ni_out) {
    UPR_ENTER(h);
    if (!h->P.n_dyn || !dxs) return qp_kkt_core(h, dxs, dus, pi, nu, yN, lam, ni_out);
    const upr_dims& d = h->d;
    std::vector<double> xr((size_t)h->B * (d.N + 1) * d.nx);
    if (qp_kkt_core(h, xr.data(), dus, pi, nu, yN, lam, ni_out)) return 1;
    upr_iface_join_zero(d.nx, h->P.n_dyn, xr.data(), (size_t)h->B * (d.N + 1), dxs);
    return 0;
}

int upr_batch_set_projectile_flag(upr_batch* h, const double* sflag) {
    UPR_ENTER(h);
    if (!h->pflag) return upr_fail("upr_batch_set_projectile_flag: the problem has no dynamic obstacle");
    UPR_HIP(hipMemcpy(h->pflag, sflag, sizeof(double) * h->B, hipMemcpyHostToDevice));
    return 0;
}
}  // extern "C"
