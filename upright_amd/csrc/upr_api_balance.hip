// upr_api_balance.hip -- the balance family of libupright_mi.so (include/upright_mi.h): request, validation, launcher and the
// twenty entries upr_batch_balance_* / *_margin_* / upr_batch_retime_plan* / upr_batch_replay_plan with upr_batch_balance_ms.  The one
// unit that includes upr_balance.h, upr_margin.h, upr_speed.h, upr_pathacc.h, upr_retime.h, upr_disturb.h, upr_retime_rsv.h,
// upr_replay.h and upr_retime_sub.h: their kernels are defined here and nowhere else.
// What crosses to upr_api.hip (upr_handle.h): upr_bal_resolve, the part of upr_batch_create that fills the handle's choice of form;
// from there it takes upr_fail.  The family reads and writes the handle's bal, bal_buf / bal_cap, bal_ev and bal_ms, nothing else.
#include "upr_handle.h"

#include <cmath>

#include "upr_balance.h"
#include "upr_margin.h"
#include "upr_speed.h"
#include "upr_pathacc.h"
#include "upr_retime.h"
#include "upr_disturb.h"
#include "upr_retime_rsv.h"
#include "upr_replay.h"
#include "upr_retime_sub.h"

// the form of a handle's balance family (UPR_BAL_FORM=0: the wave form for the one-body shapes too; tests)
void upr_bal_resolve(upr_batch* h) {
    const upr_dims& d = h->d;
    const char* e = getenv("UPR_BAL_FORM");
    h->bal.L = upr_bal_layout(d.nb, d.nc, d.nf);
    h->bal.lds = (size_t)h->bal.L.total * sizeof(double);
    h->bal.form = (upr_bal_lane_form(d.nb) && !(e && atoi(e) == 0)) ? BAL_LANE : BAL_WAVE;
}

namespace {

// ---- balance family (upr_balance.h, upr_margin.h, upr_speed.h, upr_pathacc.h, upr_retime.h, upr_disturb.h, upr_retime_rsv.h, upr_replay.h, upr_retime_sub.h): the twenty entry points end here, in balance_call.  An entry fills a REQUEST, which
// names what the call is: where its points and its scenarios come from, which friction scale, which quantity, where the answers
// go.  balance_validate holds every refusal of the family, in one order.  What depends on the handle alone -- the layout of a job,
// the LDS of the wave form, lane or wave -- is the CHOICE resolved at upr_batch_create (upr_bal_choice).  The LAUNCHER reads the two:
// it carves the scratch block region by region, noting with every region what is copied into it before the kernels and out of it
// after them, and takes the kernel from a table by form and quantity.  Everything is enqueued on the handle's stream behind
// whatever is in flight and the one synchronisation is the last statement.  The scratch of the calls is one block on the handle
// that serves nothing else and only grows (bal_buf): a call in the steady state allocates and frees nothing.
enum { BAL_MU_NONE = 0, BAL_MU_SCENARIO = 1, BAL_MU_CONTACT = 2 };   // the friction scale: ones | [n_scen] | [n_scen][nc]
// the quantity: the distance rho | the common friction margin | one per contact group | the speed margin (upr_speed.h) | the
// path-acceleration margin (upr_pathacc.h) | the retiming of a plan on a speed lattice (upr_retime.h) | the disturbance margin
// (upr_disturb.h) | the retiming with a reserve (upr_retime_rsv.h) | the replay of a time law on a clock (upr_replay.h) | the retiming
// with substeps (upr_retime_sub.h)
enum { BAL_RHO = 0, BAL_MARGIN = 1, BAL_MARGIN_GROUPS = 2, BAL_SPEED = 3, BAL_PATHACC = 4, BAL_RETIME = 5, BAL_DISTURB = 6, BAL_RETIME_RSV = 7, BAL_REPLAY = 8,
       BAL_RETIME_SUB = 9 };
struct bal_request {
    const char* who = "";     // the entry, as its messages name it
    const char* needs = "";   // ... and what they say about its required pointers
    // the points: the knots of the handle's plan where they lie on the device, or n states x [n][3 nq] on the host
    bool plan = false; int n = 0; const double* x = nullptr;
    // the scenarios: parameter blocks on the host, [n_scen][nb][10] for all points or (per) a set of their own for every point /
    // every instance of the plan.  NULL (plan, n_scen == 1): every instance against its own body parameters
    int n_scen = 0; const double* params = nullptr; bool per = false;
    // the friction scale of every scenario (BAL_RHO)
    int scale = BAL_MU_NONE; const double* mu_scale = nullptr;
    // the quantity.  The margins (upr_margin.h) run on the same jobs: out is kappa_hi, z the multipliers there, iters the solves
    // over all evaluations.  Per group every output gains a trailing [n_grp]; mu_base: the scales of the contacts outside the group
    // ([n_scen][nc]; NULL: ones)
    int quantity = BAL_RHO; double kappa_max = 0.0; int n_grp = 1; const unsigned* group_mask = nullptr; const double* mu_base = nullptr;
    // the speed margin: out is speed, four doubles per job; z and y hold two certificates per job, the lower end first; worst /
    // worst_knot ([B][n_scen][2]; plan) are the window over the knots and the knots that attain it, limit [B] the limit speed
    double s_max = 0.0; double* limit = nullptr;
    // the path-acceleration margin: out is accel, four doubles per job, certificates and reductions as the speed margin's; the range
    // [-d_max, d_max] of sddot at sdot = speed; limit [B][2] the interval of sddot the acceleration boxes allow
    double d_max = 0.0, speed = 1.0;
    // the retiming (plan only): the lattice speeds [n_lvl]; start / end a level or -1; common: one time law under all scenarios;
    // boxes: the velocity and acceleration boxes cut edges.  out is duration, one double per (instance, scenario) or per instance
    // with common; level [..][N + 1], reach [..][2]; edges [B][n_scen][N][n_lvl] and iters, one per mask row, stay per scenario
    const double* speeds = nullptr; int n_lvl = 0, start = -1, end = -1; bool common = false, boxes = true;
    int *level = nullptr, *reach = nullptr; unsigned* edges = nullptr;
    // the disturbance margin: dirs [n_dir][6] = (u_alpha, u_a) in the world (frame 0) or the tray frame (1), the range [-r_max, r_max];
    // out is reach, four doubles per job, and every per-job output gains a LEADING [n_dir]; worst / worst_knot ([n_dir][B][n_scen][2];
    // plan) the window per direction, radius [B][n_scen] and binding [B][n_scen][3] the reduction over the directions
    const double* dirs = nullptr; int n_dir = 0, frame = 0; double r_max = 0.0; double* radius = nullptr; int* binding = nullptr;
    // the retiming with a reserve: the retiming's fields, dirs / n_dir / frame as the disturbance margin's and the reserve r >= 0 every
    // end state must absorb along every +-u; the outputs and their layouts are the retiming's
    double reserve = 0.0;
    // the retiming with substeps: the retiming's fields and substeps = R, the path points per segment beyond its departing knot at which
    // an edge must be balanced; the points are the B (N R + 1) points of the fine plan; the outputs and their layouts are the retiming's
    int substeps = 1;
    // the replay (plan only): speeds / n_lvl and boxes as the retiming's; level_in [B][N + 1] one law per instance (lattice indices, or -1
    // throughout: no law); the clock tick, t0, n_samp.  The points are the B n_samp samples.  out is rho [B][K][n_scen], limit the duration
    // [B]; count [B], excess and iters [B][K][n_scen], worst [B][n_scen], verdict [B][n_scen][3], box_first [B], x_out [B][K][3 nq]
    const int* level_in = nullptr; double tick = 0.0, t0 = 0.0; int n_samp = 0;
    int *count = nullptr, *verdict = nullptr, *box_first = nullptr; double *excess = nullptr, *x_out = nullptr;
    // the answers on the host; all but the required ones may be NULL.  worst / worst_knot ([B][n_scen][n_grp]; plan, per group): the
    // largest kappa_hi over the knots of an instance, reduced on the device; out may then be NULL and kappa_hi stays on the device
    double* out = nullptr;   // rho | kappa_hi
    double *kappa_lo = nullptr, *z = nullptr, *y = nullptr; int* iters = nullptr; double* worst = nullptr; int* worst_knot = nullptr;
};
long long bal_points(const upr_batch* h, const bal_request& r) {
    if (r.quantity == BAL_REPLAY) return (long long)h->B * r.n_samp;
    // (a substeps outside 1 .. UPR_SUB_MAX counts as 1 here: the checks on the points come first, the refusal of the value is its own)
    if (r.quantity == BAL_RETIME_SUB) return (long long)h->B * ((long long)h->d.N * (r.substeps >= 1 && r.substeps <= UPR_SUB_MAX ? r.substeps : 1) + 1);
    return r.plan ? (long long)h->B * (h->d.N + 1) : r.n;
}
size_t bal_param_sets(const upr_batch* h, const bal_request& r) { return (size_t)(r.per ? (r.plan ? h->B : r.n) : 1) * r.n_scen; }

size_t bal_up(size_t bytes) { return (bytes + 255) & ~(size_t)255; }
// the next region of a scratch block of `total` bytes so far: its offset (a region that is not wanted takes no room)
size_t bal_take(size_t& total, size_t bytes, bool wanted) { const size_t o = total; total += wanted ? bal_up(bytes) : 0; return o; }
int balance_scratch(upr_batch* h, size_t bytes) {
    if (bytes <= h->bal_cap) return 0;
    if (h->bal_buf) { UPR_HIP(hipFree(h->bal_buf)); h->bal_buf = nullptr; h->bal_cap = 0; }
    UPR_HIP(hipMalloc(&h->bal_buf, bytes));
    h->bal_cap = bytes;
    return 0;
}
int balance_check_groups(const upr_batch* h, int n_grp, const unsigned* group_mask) {
    if (n_grp < 1 || n_grp > 65535) return upr_fail("friction margin of contact groups: n_grp must be in 1 .. 65535");
    if (!group_mask) return upr_fail("friction margin of contact groups: group_mask must not be NULL");
    const int nc = h->d.nc;
    for (int g = 0; g < n_grp; ++g) {
        if (group_mask[g] == 0u) return upr_fail("friction margin of contact groups: group " + std::to_string(g) + " has an empty mask");
        if (nc < 32 && (group_mask[g] >> nc) != 0u)
            return upr_fail("friction margin of contact groups: group " + std::to_string(g) + " has a mask bit >= nc = " + std::to_string(nc));
    }
    return 0;
}
int balance_check_scales(const double* v, size_t count, const char* what) {
    if (v) for (size_t i = 0; i < count; ++i)
        if (!(v[i] >= 0) || !std::isfinite(v[i])) return upr_fail(std::string("balance check: every ") + what + " must be finite and >= 0");
    return 0;
}
// 0: a request to launch; 1: refused (upr_last_error says why); 2: no points, nothing to do
int balance_validate(const upr_batch* h, const bal_request& r) {
    const upr_dims& d = h->d;
    auto refuse = [&](const char* why) { return upr_fail(std::string(r.who) + ": " + why); };
    const bool margin = r.quantity == BAL_MARGIN || r.quantity == BAL_MARGIN_GROUPS;
    if (margin && (!(r.kappa_max > 0) || !std::isfinite(r.kappa_max))) return upr_fail("friction margin: kappa_max must be finite and > 0");
    if (r.quantity == BAL_SPEED && (!(r.s_max > 1) || !std::isfinite(r.s_max))) return upr_fail("speed margin: s_max must be finite and > 1");
    if (r.quantity == BAL_PATHACC && (!(r.d_max > 0) || !std::isfinite(r.d_max) || !(r.speed >= 0) || !std::isfinite(r.speed)))
        return upr_fail("path-acceleration margin: d_max must be finite and > 0, speed finite and >= 0");
    if (r.quantity == BAL_MARGIN_GROUPS && balance_check_groups(h, r.n_grp, r.group_mask)) return 1;
    if (!r.plan && r.n <= 0) return 2;
    if ((!r.plan && (!r.x || !r.params)) || (r.scale == BAL_MU_CONTACT && !r.mu_scale) || (!r.out && !r.worst && !r.level && !r.radius && !r.x_out && !r.excess)) return refuse(r.needs);
    if (r.plan && !r.params) {
        if (r.n_scen != 1) return refuse("params == NULL needs n_scen == 1 (every instance's own body parameters)");
    } else if (r.n_scen < 1) return refuse("n_scen must be >= 1");
    if (r.params) for (size_t i = 0, e = bal_param_sets(h, r) * d.nb; i < e; ++i)
        if (!(r.params[10 * i] > 0) || !std::isfinite(r.params[10 * i])) return upr_fail("balance check: every body of every scenario needs a positive finite mass");
    if (balance_check_scales(r.mu_scale, (size_t)r.n_scen * (r.scale == BAL_MU_CONTACT ? d.nc : 1), "mu_scale")) return 1;
    if (balance_check_scales(r.mu_base, (size_t)r.n_scen * d.nc, "mu_base")) return 1;
    const long long n = bal_points(h, r);
    if (n > (1ll << 31) - 64 || n * r.n_scen * r.n_grp > (1ll << 36)) return upr_fail("balance check: too many points");
    if (r.quantity == BAL_RETIME || r.quantity == BAL_RETIME_RSV || r.quantity == BAL_REPLAY || r.quantity == BAL_RETIME_SUB) {
        bool ok = r.speeds && r.n_lvl >= 1 && r.n_lvl <= UPR_RET_MAX_LEVELS;
        for (int m = 0; ok && m < r.n_lvl; ++m) ok = std::isfinite(r.speeds[m]) && r.speeds[m] >= 0 && (m == 0 || r.speeds[m] > r.speeds[m - 1]);
        if (!ok) return upr_fail("retime: speeds must be 1 .. 32 finite values >= 0 in strictly increasing order");
        if (r.start < -1 || r.start >= r.n_lvl || r.end < -1 || r.end >= r.n_lvl) return upr_fail("retime: start and end must be -1 or a level index");
        if (r.quantity == BAL_RETIME_SUB && (r.substeps < 1 || r.substeps > UPR_SUB_MAX)) return upr_fail("retime: substeps must be 1 .. 16");
        // (the jobs: a mask row each, counted on the knots of the plan)
        const long long knots = r.quantity == BAL_RETIME_SUB ? (long long)h->B * (d.N + 1) : n;
        if (r.quantity != BAL_REPLAY && knots * r.n_scen * r.n_lvl > (1ll << 36)) return upr_fail("balance check: too many points");
    }
    if (r.quantity == BAL_DISTURB) {
        if (!(r.r_max > 0) || !std::isfinite(r.r_max)) return upr_fail("disturbance margin: r_max must be finite and > 0");
        bool ok = r.dirs && r.n_dir >= 1 && r.n_dir <= UPR_DST_MAX_DIRS;
        for (int k = 0; ok && k < r.n_dir; ++k) {
            bool any = false;
            for (int i = 0; ok && i < 6; ++i) { ok = std::isfinite(r.dirs[6 * k + i]); any = any || r.dirs[6 * k + i] != 0.0; }
            ok = ok && any;
        }
        if (!ok) return upr_fail("disturbance margin: dirs must be 1 .. 32 finite non-zero directions");
        if (r.frame != 0 && r.frame != 1) return upr_fail("disturbance margin: frame must be 0 (world) or 1 (tray)");
        if (n * r.n_scen * r.n_dir > (1ll << 36)) return upr_fail("balance check: too many points");   // (the jobs: one per direction)
    }
    if (r.quantity == BAL_RETIME_RSV) {
        if (!(r.reserve >= 0) || !std::isfinite(r.reserve)) return upr_fail("retime: reserve must be finite and >= 0");
        bool ok = r.dirs && r.n_dir >= 1 && r.n_dir <= UPR_DST_MAX_DIRS;
        for (int k = 0; ok && k < r.n_dir; ++k) {
            bool any = false;
            for (int i = 0; ok && i < 6; ++i) { ok = std::isfinite(r.dirs[6 * k + i]); any = any || r.dirs[6 * k + i] != 0.0; }
            ok = ok && any;
        }
        if (!ok) return upr_fail("retime: dirs must be 1 .. 32 finite non-zero directions");
        if (r.frame != 0 && r.frame != 1) return upr_fail("retime: frame must be 0 (world) or 1 (tray)");
    }
    if (r.quantity == BAL_REPLAY) {
        if (!(r.tick > 0) || !std::isfinite(r.tick) || !(r.t0 >= 0) || !std::isfinite(r.t0)) return upr_fail("replay: tick must be finite and > 0, t0 finite and >= 0");
        if (r.n_samp < 1 || r.n_samp > 65536) return upr_fail("replay: n_samp must be 1 .. 65536");
        if (!r.level_in) return upr_fail("replay: level must not be NULL");
        const int nk = d.N + 1;
        for (int b = 0; b < h->B; ++b) {
            const int* lv = r.level_in + (size_t)b * nk;
            for (int i = 0; i < nk; ++i)
                if (lv[i] < -1 || lv[i] >= r.n_lvl || ((lv[i] < 0) != (lv[0] < 0))) return upr_fail("replay: level must hold lattice indices, or -1 throughout a plan");
        }
        for (int b = 0; b < h->B; ++b) {
            const int* lv = r.level_in + (size_t)b * nk;
            for (int i = 0; lv[0] >= 0 && i + 1 < nk; ++i)
                if (!(r.speeds[lv[i]] + r.speeds[lv[i + 1]] > 0.0)) return upr_fail("replay: a law must not hold speed 0 over a segment");
        }
    }
    return 0;
}

// form x quantity -> kernel; the columns: rho, rho with mu_scale, rho with a scale per contact, the common margin, the margin per
// group, the speed margin, the path-acceleration margin, the edge masks of the retiming, the disturbance margin, the edge masks of the retiming with a reserve, the jobs of the replay, the edge masks of the retiming with substeps.  Every kernel takes
// (its record, upr_bal_dims, long long jobs); the record is upr_bal_args, upr_mar_args for the common margin, upr_grp_args for the
// groups, upr_spd_args for the speed margin, upr_pac_args for the path-acceleration margin, upr_ret_args for the retiming,
// upr_dst_args for the disturbance margin, upr_ret_rsv_args for the retiming with a reserve, upr_rpl_args for the replay and
// upr_ret_sub_args for the retiming with substeps.
const void* const bal_kernels[2][12] = {
    /* BAL_LANE */ {(const void*)upr_bal_project1_kernel, (const void*)upr_bal_project1_mu_kernel, (const void*)upr_bal_project1_cmu_kernel,
                    (const void*)upr_bal_margin1_kernel, (const void*)upr_bal_margin1_grp_kernel, (const void*)upr_bal_speed1_kernel,
                    (const void*)upr_bal_pathacc1_kernel, (const void*)upr_bal_retime1_kernel, (const void*)upr_bal_disturb1_kernel,
                    (const void*)upr_bal_retime_rsv1_kernel, (const void*)upr_bal_replay1_kernel, (const void*)upr_bal_retime_sub1_kernel},
    /* BAL_WAVE */ {(const void*)upr_bal_project_kernel, (const void*)upr_bal_project_mu_kernel, (const void*)upr_bal_project_cmu_kernel,
                    (const void*)upr_bal_margin_kernel, (const void*)upr_bal_margin_grp_kernel, (const void*)upr_bal_speed_kernel,
                    (const void*)upr_bal_pathacc_kernel, (const void*)upr_bal_retime_kernel, (const void*)upr_bal_disturb_kernel,
                    (const void*)upr_bal_retime_rsv_kernel, (const void*)upr_bal_replay_kernel, (const void*)upr_bal_retime_sub_kernel}};
struct bal_copy { size_t off; void* host; size_t bytes; };   // a region of the scratch block and its side on the host

int balance_launch(upr_batch* h, const bal_request& r) {
    const upr_dims& d = h->d;
    upr_bal_dims L = h->bal.L;
    const bool wave = h->bal.form == BAL_WAVE, pathacc = r.quantity == BAL_PATHACC, disturb = r.quantity == BAL_DISTURB;
    const bool speed = r.quantity == BAL_SPEED || pathacc || disturb;   // (speed: the four-double layout)
    const bool reserve = r.quantity == BAL_RETIME_RSV, sub = r.quantity == BAL_RETIME_SUB;
    const bool retime = r.quantity == BAL_RETIME || reserve || sub;   // (retime: what the three retimings do)
    // (replay: the sampler leaves the B K sample states where a points call uploads its x; jobs: somebody asks for more than the states)
    const bool replay = r.quantity == BAL_REPLAY, jobs = !replay || r.out || r.excess || r.iters || r.worst || r.verdict;
    const bool margin = r.quantity != BAL_RHO && !speed && !retime && !replay, groups = r.quantity == BAL_MARGIN_GROUPS;
    // (the retiming: a job is a mask row, (instance, scenario, segment, level); nplans outputs of the path kernel)
    const long long n = bal_points(h, r), njobs = retime ? (long long)h->B * r.n_scen * d.N * r.n_lvl : n * r.n_scen, ng = disturb ? r.n_dir : r.n_grp, nout = njobs * ng;
    const long long nplans = retime ? (long long)h->B * (r.common ? 1 : r.n_scen) : 0;
    // (the disturbance margin: njobs the jobs of one direction, ng the directions -- the groups' place, but the leading axis)
    const bool want_worst = r.worst || r.worst_knot || r.radius || r.binding || r.verdict;
    const long long nworst = want_worst ? (long long)h->B * r.n_scen * (disturb ? 2 * ng : speed ? 2 : ng) : 0;
    const size_t per_out = speed ? 4 : 1, ends = speed ? 2 : 1;   // doubles of `out` and certificates per job
    const double* scale_host = groups ? r.mu_base : r.mu_scale;
    const size_t scale_count = (size_t)r.n_scen * ((groups || r.scale == BAL_MU_CONTACT) ? d.nc : 1);
    // the scratch block, region by region, with what goes into a region before the kernels (from) and out of it after them (to)
    bal_copy up[4], down[10];
    int nup = 0, ndown = 0; size_t total = 0;
    auto region = [&](size_t bytes, bool wanted, const void* from, void* to) {
        const size_t o = bal_take(total, bytes, wanted);
        if (wanted && from) up[nup++] = {o, const_cast<void*>(from), bytes};
        if (wanted && to) down[ndown++] = {o, to, bytes};
        return o;
    };
    const size_t o_st = region(sizeof(double) * n * UPR_BAL_ST, true, nullptr, nullptr);
    const size_t o_rho = region(sizeof(double) * (retime ? nplans : nout * per_out), true, nullptr, r.out);
    const size_t o_z = region(sizeof(double) * nout * ends * L.ncol, r.z != nullptr, nullptr, r.z);
    const size_t o_it = region(sizeof(int) * nout, r.iters != nullptr, nullptr, r.iters);
    const size_t o_par = region(sizeof(double) * bal_param_sets(h, r) * d.nb * 10, r.params != nullptr, r.params, nullptr);
    const size_t o_x = region(sizeof(double) * n * (replay ? 3 * h->P.nq : d.nx), !r.plan || replay, replay ? nullptr : r.x, replay ? r.x_out : nullptr);
    const size_t o_mu = region(sizeof(double) * scale_count, scale_host != nullptr, scale_host, nullptr);
    const size_t o_lo = region(sizeof(double) * nout, r.kappa_lo != nullptr, nullptr, r.kappa_lo);
    const size_t o_y = region(sizeof(double) * nout * ends * L.m, r.y != nullptr, nullptr, r.y);
    const size_t o_gm = region(sizeof(unsigned) * ng, groups, r.group_mask, nullptr);
    const size_t o_w = region(sizeof(double) * nworst, want_worst, nullptr, r.worst);
    const size_t o_wk = region(sizeof(int) * nworst, want_worst && !replay, nullptr, r.worst_knot);
    const size_t o_lim = region(sizeof(double) * h->B * (pathacc ? 2 : 1), r.limit != nullptr, nullptr, r.limit);   // (replay: the duration)
    const size_t o_vee = region(sizeof(double) * n * 3, pathacc || retime, nullptr, nullptr);
    const size_t o_spd = region(sizeof(double) * r.n_lvl, retime || replay, r.speeds, nullptr);
    const size_t o_edg = region(sizeof(unsigned) * nout, retime, nullptr, r.edges);
    const size_t o_arg = region((size_t)nplans * d.N * r.n_lvl, retime, nullptr, nullptr);
    const size_t o_lvl = region(sizeof(int) * nplans * (d.N + 1), retime, nullptr, r.level);
    const size_t o_rch = region(sizeof(int) * nplans * 2, retime && r.reach, nullptr, r.reach);
    const size_t o_dir = region(sizeof(double) * (reserve ? r.n_dir : ng) * 6, disturb || reserve, r.dirs, nullptr);
    const size_t o_rad = region(sizeof(double) * h->B * r.n_scen, disturb && r.radius, nullptr, r.radius);
    const size_t o_bnd = region(sizeof(int) * h->B * r.n_scen * 3, disturb && r.binding, nullptr, r.binding);
    const size_t o_lin = region(sizeof(int) * h->B * (d.N + 1), replay, r.level_in, nullptr);
    const size_t o_cnt = region(sizeof(int) * h->B, replay, nullptr, r.count);
    const size_t o_exc = region(sizeof(double) * nout, replay && jobs, nullptr, r.excess);
    const size_t o_ver = region(sizeof(int) * nworst * 3, replay && r.verdict, nullptr, r.verdict);
    const size_t o_bxf = region(sizeof(int) * h->B, replay && r.box_first, nullptr, r.box_first);
    const size_t o_xf = region(sizeof(double) * n * 3 * h->P.nq, sub, nullptr, nullptr);   // (the fine plan)
    if (balance_scratch(h, total)) return 1;
    char* base = (char*)h->bal_buf;
    for (int i = 0; i < nup; ++i) UPR_HIP(hipMemcpyAsync(base + up[i].off, up[i].host, up[i].bytes, hipMemcpyHostToDevice, h->stream));
    if (!h->bal_ev[0]) { UPR_HIP(hipEventCreate(&h->bal_ev[0])); UPR_HIP(hipEventCreate(&h->bal_ev[1])); }
    UPR_HIP(hipEventRecord(h->bal_ev[0], h->stream));
    const double* dx = sub ? (const double*)(base + o_xf) : (r.plan && !replay) ? h->xs : (const double*)(base + o_x);
    double *dst = (double*)(base + o_st), *drho = (double*)(base + o_rho);
    const dim3 sg((unsigned)((n + 63) / 64)), sb(64);
    if (replay) {
        upr_rpl_sample_args Y;
        Y.P = h->dP; Y.xs = h->xs; Y.speeds = (const double*)(base + o_spd); Y.level = (const int*)(base + o_lin); Y.nk = d.N + 1; Y.nx = d.nx;
        Y.K = r.n_samp; Y.boxes = r.boxes ? 1 : 0; Y.h = h->P.dt; Y.tick = r.tick; Y.t0 = r.t0; Y.x = (double*)(base + o_x);
        Y.duration = r.limit ? (double*)(base + o_lim) : nullptr; Y.count = (int*)(base + o_cnt); Y.box_first = r.box_first ? (int*)(base + o_bxf) : nullptr;
        hipLaunchKernelGGL(upr_bal_replay_sample_kernel, dim3((unsigned)(h->B < 16384 ? h->B : 16384)), dim3(64), sizeof(double) * 2 * (d.N + 1), h->stream, Y,
                           (long long)h->B);
        UPR_HIP(hipGetLastError());
    }
    if (sub) {
        upr_sub_refine_args F;
        F.P = h->dP; F.xs = h->xs; F.nk = d.N + 1; F.nx = d.nx; F.R = r.substeps; F.h = h->P.dt; F.xf = (double*)(base + o_xf);
        hipLaunchKernelGGL(upr_bal_refine_kernel, dim3((unsigned)((n + 63) / 64 < 16384 ? (n + 63) / 64 : 16384)), dim3(64), 0, h->stream, F, n);
        UPR_HIP(hipGetLastError());
    }
    if (!jobs) {}   // (the states alone: the sampler was all)
    else if ((pathacc || retime) && h->P.nq == 6) hipLaunchKernelGGL(upr_bal_state_vee_kernel<6>, sg, sb, 0, h->stream, h->dP, (int)n, dx, dst, (double*)(base + o_vee));
    else if (pathacc || retime) hipLaunchKernelGGL(upr_bal_state_vee_kernel<9>, sg, sb, 0, h->stream, h->dP, (int)n, dx, dst, (double*)(base + o_vee));
    else if (h->P.nq == 6) hipLaunchKernelGGL(upr_bal_state_kernel<6>, sg, sb, 0, h->stream, h->dP, (int)n, dx, dst);
    else hipLaunchKernelGGL(upr_bal_state_kernel<9>, sg, sb, 0, h->stream, h->dP, (int)n, dx, dst);
    UPR_HIP(hipGetLastError());
    upr_bal_args A;
    A.P = h->dP; A.n = (int)n; A.n_scen = r.n_scen; A.st = dst; A.eq_scale = d.eq_scale;
    A.params = r.params ? (const double*)(base + o_par) : h->body_params;
    A.pdiv = r.plan ? ((r.per || !r.params) ? (replay ? r.n_samp : sub ? d.N * r.substeps + 1 : d.N + 1) : 0) : (r.per ? 1 : 0);   // points that share a parameter set
    A.rho = drho; A.z = r.z ? (double*)(base + o_z) : nullptr; A.iters = r.iters ? (int*)(base + o_it) : nullptr;
    A.mu_scale = r.mu_scale ? (const double*)(base + o_mu) : nullptr;
    upr_mar_args M;
    if (margin) {
        M.J = A; M.J.rho = nullptr; M.kappa_max = r.kappa_max; M.kappa_hi = drho;
        M.kappa_lo = r.kappa_lo ? (double*)(base + o_lo) : nullptr; M.y = r.y ? (double*)(base + o_y) : nullptr;
    }
    upr_spd_args S;
    if (speed && !pathacc && !disturb) { S.J = A; S.J.rho = nullptr; S.s_max = r.s_max; S.speed = drho; S.y = r.y ? (double*)(base + o_y) : nullptr; }
    upr_pac_args C;
    if (pathacc) {
        C.J = A; C.J.rho = nullptr; C.d_max = r.d_max; C.speed = r.speed; C.vee = (const double*)(base + o_vee); C.accel = drho;
        C.y = r.y ? (double*)(base + o_y) : nullptr;
    }
    upr_dst_args D;
    if (disturb) {
        D.J = A; D.J.rho = nullptr; D.r_max = r.r_max; D.dirs = (const double*)(base + o_dir); D.n_dir = (int)ng; D.frame = r.frame; D.reach = drho;
        D.y = r.y ? (double*)(base + o_y) : nullptr;
    }
    upr_ret_args T;
    if (retime) {
        T.J = A; T.J.rho = nullptr; T.vee = (const double*)(base + o_vee); T.xs = dx; T.speeds = (const double*)(base + o_spd); T.M = r.n_lvl;
        T.nk = d.N + 1; T.nx = sub ? 3 * h->P.nq : d.nx; T.boxes = r.boxes ? 1 : 0; T.h = h->P.dt; T.edges = (unsigned*)(base + o_edg);
    }
    upr_ret_rsv_args V;
    if (reserve) { V.T = T; V.dirs = (const double*)(base + o_dir); V.n_dir = r.n_dir; V.frame = r.frame; V.reserve = r.reserve; }
    upr_ret_sub_args U;
    if (sub) { U.T = T; U.R = r.substeps; }
    upr_rpl_args Rp;
    if (replay) { Rp.J = A; Rp.J.rho = r.out ? drho : nullptr; Rp.count = (const int*)(base + o_cnt); Rp.K = r.n_samp; Rp.excess = (double*)(base + o_exc); }
    upr_grp_args X;
    if (groups) { X.M = M; X.n_grp = (int)ng; X.group_mask = (const unsigned*)(base + o_gm); X.mu_base = r.mu_base ? (const double*)(base + o_mu) : nullptr; }
    // lane form: 64 jobs per workgroup, the groups on the y axis.  Wave form: a workgroup is one wave and the jobs (for the groups:
    // job x group) are dealt round robin to a grid that fills the device a few times over (its LDS, at most 26.4 KB, lets six of
    // the largest shape share a CU inside the 160 KiB)
    long long count = (wave && (groups || disturb)) ? nout : njobs;
    const dim3 grid = wave ? dim3((unsigned)(count < 16384 ? count : 16384)) : dim3((unsigned)((njobs + 63) / 64), (unsigned)ng);
    void* args[] = {replay ? (void*)&Rp : sub ? (void*)&U : reserve ? (void*)&V : disturb ? (void*)&D : retime ? (void*)&T : pathacc ? (void*)&C : speed ? (void*)&S : groups ? (void*)&X : margin ? (void*)&M : (void*)&A, &L, &count};
    if (jobs) UPR_HIP(hipLaunchKernel(bal_kernels[h->bal.form][r.quantity != BAL_RHO ? 2 + r.quantity : r.scale], grid, dim3(64), args, wave ? h->bal.lds : 0, h->stream));
    if (replay) {
        if (want_worst) {
            hipLaunchKernelGGL(upr_bal_replay_plan_kernel, dim3((unsigned)((nworst + 63) / 64)), dim3(64), 0, h->stream, (const double*)(base + o_exc),
                               (const int*)(base + o_cnt), r.n_samp, r.n_scen, nworst, r.worst ? (double*)(base + o_w) : nullptr,
                               r.verdict ? (int*)(base + o_ver) : nullptr);
            UPR_HIP(hipGetLastError());
        }
    } else if (retime) {
        upr_ret_path_args Q;
        Q.edges = T.edges; Q.speeds = T.speeds; Q.M = r.n_lvl; Q.nk = d.N + 1; Q.n_scen = r.n_scen; Q.common = r.common ? 1 : 0; Q.start = r.start; Q.end = r.end;
        Q.h = h->P.dt; Q.arg = (unsigned char*)(base + o_arg); Q.duration = drho; Q.level = (int*)(base + o_lvl); Q.reach = r.reach ? (int*)(base + o_rch) : nullptr;
        hipLaunchKernelGGL(upr_bal_retime_path_kernel, dim3((unsigned)(nplans < 16384 ? nplans : 16384)), dim3(64), 0, h->stream, Q, nplans);
        UPR_HIP(hipGetLastError());
    } else if (disturb && want_worst) {
        const long long nbs = (long long)h->B * r.n_scen;
        hipLaunchKernelGGL(upr_bal_disturb_plan_kernel, dim3((unsigned)((nbs + 63) / 64)), dim3(64), 0, h->stream, (const double*)drho, d.N + 1, r.n_scen,
                           (int)ng, nbs, (double*)(base + o_w), (int*)(base + o_wk), r.radius ? (double*)(base + o_rad) : nullptr,
                           r.binding ? (int*)(base + o_bnd) : nullptr);
        UPR_HIP(hipGetLastError());
    } else if (pathacc && (want_worst || r.limit)) {
        const long long lanes = nworst + (r.limit ? h->B : 0);
        hipLaunchKernelGGL(upr_bal_pathacc_plan_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, h->stream, (const upr_problem*)h->dP, (const double*)drho,
                           d.N + 1, r.n_scen, nworst, h->B, d.nx, r.speed, (const double*)h->xs, (double*)(base + o_w),
                           r.worst_knot ? (int*)(base + o_wk) : nullptr, r.limit ? (double*)(base + o_lim) : nullptr);
        UPR_HIP(hipGetLastError());
    } else if (speed && !disturb && (want_worst || r.limit)) {
        const long long lanes = nworst + (r.limit ? h->B : 0);
        hipLaunchKernelGGL(upr_bal_speed_plan_kernel, dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, h->stream, (const upr_problem*)h->dP, (const double*)drho,
                           d.N + 1, r.n_scen, nworst, h->B, d.nx, d.nu, (const double*)h->xs, (const double*)h->us, (double*)(base + o_w),
                           r.worst_knot ? (int*)(base + o_wk) : nullptr, r.limit ? (double*)(base + o_lim) : nullptr);
        UPR_HIP(hipGetLastError());
    } else if (want_worst) {
        hipLaunchKernelGGL(upr_bal_margin_worst_kernel, dim3((unsigned)((nworst + 63) / 64)), dim3(64), 0, h->stream, (const double*)drho, d.N + 1,
                           (long long)r.n_scen * ng, nworst, (double*)(base + o_w), r.worst_knot ? (int*)(base + o_wk) : nullptr);
        UPR_HIP(hipGetLastError());
    }
    UPR_HIP(hipEventRecord(h->bal_ev[1], h->stream));
    for (int i = 0; i < ndown; ++i) UPR_HIP(hipMemcpyAsync(down[i].host, base + down[i].off, down[i].bytes, hipMemcpyDeviceToHost, h->stream));
    UPR_HIP(hipStreamSynchronize(h->stream));
    float ms = 0.0f;
    UPR_HIP(hipEventElapsedTime(&ms, h->bal_ev[0], h->bal_ev[1]));
    h->bal_ms = ms;
    return 0;
}
int balance_call(upr_batch* h, const bal_request& r) {
    if (const int v = balance_validate(h, r)) return v == 1;
    return balance_launch(h, r);
}

}  // namespace

extern "C" {

// the balance family: every entry names its request ("balance family" above)
int upr_batch_balance_points_mu(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, const double* mu_scale,
                                double* rho, double* z, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_balance_points", .needs = "x, params and rho must not be NULL", .n = n, .x = x, .n_scen = n_scen,
                            .params = params, .per = per_point != 0, .scale = mu_scale ? BAL_MU_SCENARIO : BAL_MU_NONE, .mu_scale = mu_scale,
                            .out = rho, .z = z, .iters = iters});
}
int upr_batch_balance_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, double* rho, double* z, int* iters) {
    return upr_batch_balance_points_mu(h, n, x, n_scen, params, per_point, nullptr, rho, z, iters);
}

int upr_batch_balance_plan_mu(upr_batch* h, int n_scen, const double* params, int per_instance, const double* mu_scale, double* rho, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_balance_plan", .needs = "rho must not be NULL", .plan = true, .n_scen = n_scen, .params = params,
                            .per = per_instance != 0, .scale = mu_scale ? BAL_MU_SCENARIO : BAL_MU_NONE, .mu_scale = mu_scale, .out = rho, .iters = iters});
}
int upr_batch_balance_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double* rho, int* iters) {
    return upr_batch_balance_plan_mu(h, n_scen, params, per_instance, nullptr, rho, iters);
}

int upr_batch_friction_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, double kappa_max,
                                     double* kappa_hi, double* kappa_lo, double* z, double* y, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_friction_margin_points", .needs = "x, params and kappa_hi must not be NULL", .n = n, .x = x, .n_scen = n_scen,
                            .params = params, .per = per_point != 0, .quantity = BAL_MARGIN, .kappa_max = kappa_max, .out = kappa_hi, .kappa_lo = kappa_lo,
                            .z = z, .y = y, .iters = iters});
}

int upr_batch_friction_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double kappa_max, double* kappa_hi,
                                   double* kappa_lo, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_friction_margin_plan", .needs = "kappa_hi must not be NULL", .plan = true, .n_scen = n_scen, .params = params,
                            .per = per_instance != 0, .quantity = BAL_MARGIN, .kappa_max = kappa_max, .out = kappa_hi, .kappa_lo = kappa_lo, .iters = iters});
}

int upr_batch_balance_points_cmu(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, const double* mu_scale_c,
                                 double* rho, double* z, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_balance_points_cmu", .needs = "x, params, mu_scale_c and rho must not be NULL", .n = n, .x = x,
                            .n_scen = n_scen, .params = params, .per = per_point != 0, .scale = BAL_MU_CONTACT, .mu_scale = mu_scale_c, .out = rho, .z = z,
                            .iters = iters});
}

int upr_batch_balance_plan_cmu(upr_batch* h, int n_scen, const double* params, int per_instance, const double* mu_scale_c, double* rho, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_balance_plan_cmu", .needs = "mu_scale_c and rho must not be NULL", .plan = true, .n_scen = n_scen,
                            .params = params, .per = per_instance != 0, .scale = BAL_MU_CONTACT, .mu_scale = mu_scale_c, .out = rho, .iters = iters});
}

int upr_batch_friction_margin_groups_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, int n_grp,
                                            const unsigned* group_mask, const double* mu_base, double kappa_max, double* kappa_hi, double* kappa_lo,
                                            double* z, double* y, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_friction_margin_groups_points", .needs = "x, params and kappa_hi must not be NULL", .n = n, .x = x,
                            .n_scen = n_scen, .params = params, .per = per_point != 0, .quantity = BAL_MARGIN_GROUPS, .kappa_max = kappa_max, .n_grp = n_grp,
                            .group_mask = group_mask, .mu_base = mu_base, .out = kappa_hi, .kappa_lo = kappa_lo, .z = z, .y = y, .iters = iters});
}

int upr_batch_friction_margin_groups_plan(upr_batch* h, int n_scen, const double* params, int per_instance, int n_grp, const unsigned* group_mask,
                                          const double* mu_base, double kappa_max, double* kappa_hi, double* kappa_lo, int* iters, double* worst,
                                          int* worst_knot) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_friction_margin_groups_plan", .needs = "kappa_hi and worst must not both be NULL", .plan = true,
                            .n_scen = n_scen, .params = params, .per = per_instance != 0, .quantity = BAL_MARGIN_GROUPS, .kappa_max = kappa_max,
                            .n_grp = n_grp, .group_mask = group_mask, .mu_base = mu_base, .out = kappa_hi, .kappa_lo = kappa_lo, .iters = iters,
                            .worst = worst, .worst_knot = worst_knot});
}

int upr_batch_speed_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, double s_max, double* speed,
                                  double* z, double* y, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_speed_margin_points", .needs = "x, params and speed must not be NULL", .n = n, .x = x, .n_scen = n_scen,
                            .params = params, .per = per_point != 0, .quantity = BAL_SPEED, .s_max = s_max, .out = speed, .z = z, .y = y, .iters = iters});
}

int upr_batch_speed_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double s_max, double* speed, int* iters,
                                double* window, int* knot, double* limit) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_speed_margin_plan", .needs = "speed and window must not both be NULL", .plan = true, .n_scen = n_scen,
                            .params = params, .per = per_instance != 0, .quantity = BAL_SPEED, .s_max = s_max, .limit = limit, .out = speed, .iters = iters,
                            .worst = window, .worst_knot = knot});
}

int upr_batch_path_accel_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, double d_max, double speed,
                                       double* accel, double* z, double* y, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_path_accel_margin_points", .needs = "x, params and accel must not be NULL", .n = n, .x = x, .n_scen = n_scen,
                            .params = params, .per = per_point != 0, .quantity = BAL_PATHACC, .d_max = d_max, .speed = speed, .out = accel, .z = z, .y = y,
                            .iters = iters});
}

int upr_batch_path_accel_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance, double d_max, double speed, double* accel, int* iters,
                                     double* window, int* knot, double* limit) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_path_accel_margin_plan", .needs = "accel and window must not both be NULL", .plan = true, .n_scen = n_scen,
                            .params = params, .per = per_instance != 0, .quantity = BAL_PATHACC, .limit = limit, .d_max = d_max, .speed = speed, .out = accel,
                            .iters = iters, .worst = window, .worst_knot = knot});
}

int upr_batch_retime_plan(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds, int start_level, int end_level,
                          int common, int boxes, double* duration, int* level, int* reach, unsigned* edges, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_retime_plan", .needs = "duration and level must not both be NULL", .plan = true, .n_scen = n_scen, .params = params,
                            .per = per_instance != 0, .quantity = BAL_RETIME, .speeds = speeds, .n_lvl = n_lvl, .start = start_level, .end = end_level,
                            .common = common != 0, .boxes = boxes != 0, .level = level, .reach = reach, .edges = edges, .out = duration, .iters = iters});
}

int upr_batch_retime_plan_reserve(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds, int start_level,
                                  int end_level, int common, int boxes, int n_dir, const double* dirs, int frame, double reserve, double* duration, int* level,
                                  int* reach, unsigned* edges, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_retime_plan_reserve", .needs = "duration and level must not both be NULL", .plan = true, .n_scen = n_scen,
                            .params = params, .per = per_instance != 0, .quantity = BAL_RETIME_RSV, .speeds = speeds, .n_lvl = n_lvl, .start = start_level,
                            .end = end_level, .common = common != 0, .boxes = boxes != 0, .level = level, .reach = reach, .edges = edges, .dirs = dirs,
                            .n_dir = n_dir, .frame = frame, .reserve = reserve, .out = duration, .iters = iters});
}

int upr_batch_disturbance_margin_points(upr_batch* h, int n, const double* x, int n_scen, const double* params, int per_point, int n_dir, const double* dirs,
                                        int frame, double r_max, double* reach, double* z, double* y, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_disturbance_margin_points", .needs = "x, params and reach must not be NULL", .n = n, .x = x, .n_scen = n_scen,
                            .params = params, .per = per_point != 0, .quantity = BAL_DISTURB, .dirs = dirs, .n_dir = n_dir, .frame = frame, .r_max = r_max,
                            .out = reach, .z = z, .y = y, .iters = iters});
}

int upr_batch_disturbance_margin_plan(upr_batch* h, int n_scen, const double* params, int per_instance, int n_dir, const double* dirs, int frame, double r_max,
                                      double* reach, int* iters, double* window, int* knot, double* radius, int* binding) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_disturbance_margin_plan", .needs = "reach, window and radius must not all be NULL", .plan = true,
                            .n_scen = n_scen, .params = params, .per = per_instance != 0, .quantity = BAL_DISTURB, .dirs = dirs, .n_dir = n_dir,
                            .frame = frame, .r_max = r_max, .radius = radius, .binding = binding, .out = reach, .iters = iters, .worst = window,
                            .worst_knot = knot});
}

int upr_batch_replay_plan(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds, const int* level, double tick,
                          double t0, int n_samp, int boxes, double* duration, int* count, double* x, double* rho, double* excess, int* iters, double* worst,
                          int* verdict, int* box_first) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_replay_plan", .needs = "x, rho, excess and worst must not all be NULL", .plan = true, .n_scen = n_scen,
                            .params = params, .per = per_instance != 0, .quantity = BAL_REPLAY, .limit = duration, .speeds = speeds, .n_lvl = n_lvl,
                            .boxes = boxes != 0, .level_in = level, .tick = tick, .t0 = t0, .n_samp = n_samp, .count = count, .verdict = verdict,
                            .box_first = box_first, .excess = excess, .x_out = x, .out = rho, .iters = iters, .worst = worst});
}

int upr_batch_retime_plan_substeps(upr_batch* h, int n_scen, const double* params, int per_instance, int n_lvl, const double* speeds, int start_level,
                                   int end_level, int common, int boxes, int substeps, double* duration, int* level, int* reach, unsigned* edges, int* iters) {
    UPR_ENTER(h);
    return balance_call(h, {.who = "upr_batch_retime_plan_substeps", .needs = "duration and level must not both be NULL", .plan = true, .n_scen = n_scen,
                            .params = params, .per = per_instance != 0, .quantity = BAL_RETIME_SUB, .speeds = speeds, .n_lvl = n_lvl, .start = start_level,
                            .end = end_level, .common = common != 0, .boxes = boxes != 0, .level = level, .reach = reach, .edges = edges, .substeps = substeps,
                            .out = duration, .iters = iters});
}

double upr_batch_balance_ms(upr_batch* h) { return h ? h->bal_ms : 0.0; }

}  // extern "C"
