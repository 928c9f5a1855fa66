// upr_handle.h -- what the translation units of the C-ABI share (host only): the handle (struct upr_batch) with every type it is made
// of, the error plumbing (upr_fail, UPR_HIP, UPR_ENTER, DevBuf, dev_alloc) and the few functions that cross from one unit to another.
// The units: upr_api.hip (lifecycle, advance, tick, queries, run-time instantiation), upr_api_balance.hip (the balance family),
// upr_api_launch.hip (linearisation and line search), upr_api_qp_old.hip (the generic and second-structure QP kernels).  Every
// function declared here has hidden visibility: none of them is a symbol of libupright_mi.so.
#pragma once
// the phase counters of the instrumented builds (-DUPR_LIN_PROF, -DUPR_LS_PROF) are device variables of the kernel headers: one
// definition, in the unit that instantiates those kernels
#ifndef UPR_UNIT_LAUNCH
#undef UPR_LIN_PROF
#undef UPR_LS_PROF
#endif
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "upr_common.h"
#include "upr_kin.h"
#include "upr_linearize.h"
#include "upr_linearize2.h"
#include "upr_linesearch.h"
#include "upr_qp.h"
#include "upr_qp2.h"
#include "upr_qp3.h"
#include "upr_qp3_list.h"
#include "upr_qp_select.h"
#include "upr_fb_state.h"
#include "upr_launch_select.h"
#include "upr_bal_dims.h"

#define UPR_HIDDEN __attribute__((visibility("hidden")))

// sets the calling thread's error string (upr_last_error) and returns 1 (upr_api.hip)
UPR_HIDDEN int upr_fail(const std::string& msg);

#define UPR_HIP(call)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return upr_fail(std::string(#call) + ": " + hipGetErrorString(e_) + " (" __FILE_NAME__ ":" + std::to_string(__LINE__) + ")"); \
    } while (0)

// device scratch of one call: freed on every exit path (the early returns of UPR_HIP included)
template <class T>
struct UPR_HIDDEN DevBuf {
    T* p = nullptr;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) {
        UPR_HIP(hipMalloc((void**)&p, (n ? n : 1) * sizeof(T)));
        UPR_HIP(hipMemset(p, 0, (n ? n : 1) * sizeof(T)));
        return 0;
    }
    operator T*() const { return p; }
};

template <class T>
UPR_HIDDEN int dev_alloc(T** p, size_t n) {
    UPR_HIP(hipMalloc((void**)p, n * sizeof(T)));
    UPR_HIP(hipMemset(*p, 0, n * sizeof(T)));
    return 0;
}

// every entry point that takes a handle: the handle's own device is made current for the calling thread (the HIP "current
// device" is per thread; a stream may only be used with its device current), so that one process can hold engines on several
// GPUs and a launcher's rank r runs on the GPU its engine was created on whatever another library selected in between
#define UPR_ENTER(h) do { if (!(h)) return upr_fail("null batch"); if ((h)->device >= 0) UPR_HIP(hipSetDevice((h)->device)); } while (0)

// Where the QP kernel that ran left its per-knot factors (doubles, relative to the instance workspace)
struct upr_fb_src {
    int kind;                       // 3: K stored; 1, 2: V = Lj^-1 Hux and Lji = Lj^-1 stored
    long k_base; int k_stride;      // kind 3: K_k ; kinds 1, 2: V_k
    long lji_base; int lji_stride;  // kinds 1, 2
    long lfi_base; int lfi_stride;  // inverse Cholesky factor of the contact-force blocks of Hff
    long lsi_base; int lsi_stride;  // inverse Cholesky factor of S = Df Hff^-1 Df'
    int lsi_sb;                     // its block size: ne (one dense factor per knot) or 6 (star arrangements of the production kernel: one 6 x 6 block per body)
};

// an instantiation of the production QP kernel made at run time (hiprtc; upr_api.hip "run-time instantiation")
struct upr_jit_kernel {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    size_t lds = 0, ws = 0;
    int nt = 256;       // lanes per workgroup (UPR_JIT_NT: 128 | 256 | 512, experiments)
    std::string cfg;    // the template arguments, as rocprofv3 prints them
    upr_fb_src fb{};    // where this instantiation leaves K, Lf^-1, Ls^-1, as its own info kernel reported them
};

typedef int (*upr_qp_launcher)(struct upr_batch*, const upr_qp_args&);

// the QP kernel of a handle, resolved once at upr_batch_create: the record of upr_qp_select.h and what only upr_api.hip knows
struct upr_qp_sel : upr_qp_choice {
    int (*launch)(struct upr_batch*, const upr_qp_args&) = nullptr;
    upr_jit_kernel* jit = nullptr;   // production kernel from a run-time instantiation: its module function, nt and lds
    upr_fb_src fb{};                 // where the kernel leaves its per-knot factors (kind 0 = no source: the feedback launch is refused)
};

// ... and its linearisation and line-search kernels (upr_launch_select.h), resolved there too: the record and the kernel it names
struct upr_lin_sel : upr_lin_choice {
    const void* kern = nullptr;   // upr_linearize_kernel<...>(A), or upr_linearize2_kernel<NQ>(A, kpw, n_sph) for kind 2
    char name[128] = "";          // the instantiation with the workgroups of the last launch (upr_batch_lin_kernel_name)
};
struct upr_ls_sel : upr_ls_choice {
    void (*kern)(upr_ls_args) = nullptr;
    char name[128] = "";          // the instantiation, as rocprofv3 prints it (upr_batch_ls_kernel_name)
};

// ... and the form of its balance family (upr_balance.h, upr_margin.h; upr_api_balance.hip)
enum { BAL_LANE = 0, BAL_WAVE = 1 };
struct upr_bal_choice {
    upr_bal_dims L{};      // the layout of a job
    size_t lds = 0;        // dynamic LDS of a workgroup of the wave form, bytes
    int form = BAL_WAVE;   // BAL_LANE: a lane per job (one-body shapes); BAL_WAVE: a wave per job
};
// statistics and QP dispatch keys of a handle as the last advance left them, taken before a query solves one more QP on the handle
// and put back behind it (snapshot_take / snapshot_put_back)
struct UPR_HIDDEN upr_stats_snapshot {
    std::vector<double> stats; std::vector<unsigned char> keys;
};

struct upr_batch {
    upr_problem P;
    upr_dims d;
    int B = 0;
    int device = -1;            // HIP device the handle's buffers and stream live on (the current device at upr_batch_create)
    hipStream_t stream = nullptr;
    upr_problem* dP = nullptr;
    double *body_params = nullptr, *way_p = nullptr, *way_q = nullptr, *t0 = nullptr, *x0 = nullptr;
    double *xs = nullptr, *us = nullptr, *xs_prev = nullptr, *us_prev = nullptr, *tprev = nullptr;
    double *lin = nullptr, *Df = nullptr, *ws = nullptr, *stats = nullptr;
    int *done = nullptr;
    bool has_prev = false;   // a solution of a previous advance exists (warm start, policy evaluation)
    unsigned char* iter_key = nullptr;   // [B] IPM iteration count of the last QP, one byte per instance (what `order` is ranked by)
    int* order = nullptr;       // dispatch order of the QP launch: instances by the iteration count of their last QP, longest first
    bool order_on = true, order_valid = false;
    double* prof = nullptr;
    double *ev_t = nullptr, *ev_xo = nullptr, *ev_x = nullptr, *ev_u = nullptr;   // scratch of the evaluate / evaluate_policy calls
    double* kkt = nullptr;   // multiplier export of the register-resident QP kernel (upr_batch_qp_kkt), allocated on first use
    // feedback gains (sqp.use_feedback_policy, fb_on): where those of the last advance are (upr_fb_state.h) and the array
    // fb[B][N][nu][nx] they are gathered into -- allocated at create where UPR_FB_FUSED is set, at the first gather otherwise
    bool fb_on = false;
    upr_fb_track fbt;
    double *fb = nullptr, *xs_lin = nullptr;
    // dynamic obstacle (n_dyn == 1): observed state per instance (device + host copies, and the one the stored
    // solution belongs to), activation flag of the projectile rows
    double *dyn0 = nullptr, *pflag = nullptr;
    std::vector<double> hdyn0, hdyn_prev;
    double* pin = nullptr;   // pinned host staging of upr_batch_tick
    // upr_batch_tick as a HIP graph: the eleven stream operations of a control period (three copies in, prepare, linearise, QP,
    // line search, policy, three copies out) captured once the handle is in its steady state and replayed while that state --
    // tick_sig: everything on the host that decides WHICH operations a tick enqueues -- stays the same
    hipGraphExec_t tick_exec = nullptr;
    unsigned long long tick_sig = 0;
    int tick_steady = 0;        // ticks in a row with the same signature
    int tick_graph_on = -1;     // UPR_TICK_GRAPH (default 1), read once
    long long tick_replays = 0;
    int nxf = 0;   // interface state dimension 3 nq + 9 n_dyn
    bool guess_set = false;
    int sqp_iters_next = 0;   // > 0: SQP iterations of the next advance only (init_sqp_iteration of the first solve)
    double last_ms = 0.0;
    upr_qp_sel qp;   // the QP kernel instantiation this handle launches
    upr_lin_sel lin_sel;   // the linearisation kernel instantiation this handle launches
    upr_ls_sel ls_sel;     // ... and the line-search one
    int lin_blocks_last = -1;   // workgroups of the last linearisation launch (upr_batch_lin_kernel_name); -1: none yet
    bool ls_launched = false;   // a line search was launched (upr_batch_ls_kernel_name)
    int timing = 0;   // 0: no events; 1: around every kernel of an advance; 2: around the QP kernel only; 3: around every FOURTH QP launch
    unsigned timing_qp_count = 0;   // QP launches since upr_batch_enable_timing (mode 3 samples those with count % 4 == 0)
    double k_ms[3] = {0, 0, 0};
    int k_launches[3] = {0, 0, 0};
    std::vector<double> hDf;
    upr_stats_snapshot held;   // upr_batch_hold_stats
    std::vector<double> kkt_slack;   // slacks of the rows at the exit of the last upr_batch_qp_kkt ([B][N+1][ni]; upr_batch_qp_slacks)
    std::vector<double> kkt_pairs;   // slack pairs of the softened rows of that QP, [3: sigma, tau, gam][B][N+1][ni] (upr_batch_qp_slack_pairs)
    // value function of the last QP (upr_batch_value_function_update): cost-to-go matrices, gradients, cost-to-go of the plan and
    // expansion points of every instance on the device, and the time of knot 0 of the plan they belong to
    double *vf_P = nullptr, *vf_p = nullptr, *vf_J = nullptr, *vf_X = nullptr, *vf_t0 = nullptr;
    int vf_state = 0;        // 0: no update yet; 1: current; 2: stale (the plan or the observation changed since)
    double vf_ms = 0.0;      // device time of the last cost-to-go launch
    hipEvent_t vf_ev[2] = {nullptr, nullptr};
    double* vf_nu = nullptr;   // [B][N][ne] equality multipliers of that QP (the cost-to-go kernel's copy: upr_batch_equality_lagrangian)
    // tracked mode (upr_batch_track_value_function): the advance hands its own last QP to the cost-to-go kernel in-stream.
    // vf_tracked: the current cost-to-go came from an advance -- it belongs to the solve and outlives upr_batch_set_observation
    bool vf_track = false, vf_tracked = false;
    bool vf_ms_pending = false;   // events of a tracked launch on a timed handle recorded, vf_ms not read back yet
    // balance check (upr_balance.h): HIP events around the two launches of the last call and their distance (upr_batch_balance_ms)
    hipEvent_t bal_ev[2] = {nullptr, nullptr};
    double bal_ms = 0.0;
    void* bal_buf = nullptr; size_t bal_cap = 0;   // scratch of the balance-check calls, grown on demand, used for nothing else
    upr_bal_choice bal;   // the form of the balance family's kernels on this handle
    std::vector<hipEvent_t> ev_pool, ev_free;   // events in use (pairs, in launch order) / harvested ones waiting for reuse
    std::vector<int> ev_slot;
};

// ---- what crosses from one unit to another ---------------------------------------------------------------------------------
// upr_api_balance.hip: fills h->bal at upr_batch_create (UPR_BAL_FORM)
UPR_HIDDEN void upr_bal_resolve(upr_batch* h);
// upr_api_launch.hip: fills h->lin_sel / h->ls_sel at upr_batch_create (their knobs); non-zero, with the error set, when a planned
// form is not in the lists of upr_launch_select.h.  The launches of the two kernels on the handle's stream
UPR_HIDDEN int upr_launch_resolve(upr_batch* h);
UPR_HIDDEN int launch_linearize(upr_batch* h, const upr_lin_args& A);
UPR_HIDDEN int launch_linesearch(upr_batch* h, const upr_ls_args& A0);
// upr_api_qp_old.hip: the launcher of the generic QP kernel at nt lanes, and of the second-structure kernel of a shape of
// UPR_QP2_SHAPES (nullptr for any other shape); a bad nt gets a launcher that refuses
UPR_HIDDEN upr_qp_launcher qp_generic_launcher(int nt);
UPR_HIDDEN upr_qp_launcher qp2_launcher(int nq, int nb, int nc, int nf, int nt);
