// upr_fb_state.h -- where the feedback gains of a handle's last advance are (sqp.use_feedback_policy), and what every event on the
// handle does about it.  The gains are formed when, and as far as, somebody asks for them: an advance leaves them IN THE FACTORS
// of its last QP (K_k and the inverse contact and Schur factors in the instance workspace, the rows C_k in the linearisation
// records, D_f, the QP status in the statistics); the policy reads one or two knots straight from there
// (evaluate_policy_factors_kernel of upr_api.hip) and the full array fb[B][N][nu][nx] is gathered at the first request for it, or
// before a call overwrites one of those sources.  Everything here is host arithmetic: upr_api.hip acts on the answers, and the host
// emulation under tests/emu compiles this file with g++ to drive the same rules.
#pragma once

// the gains of the last advance
enum { UPR_FB_NONE = 0,      // no solve yet (the array, where it exists, is zero)
       UPR_FB_FACTORS = 1,   // in the factors of the advance's last QP
       UPR_FB_ARRAY = 2 };   // materialised in the handle's array
// UPR_FB_FUSED, read at upr_batch_create
enum { UPR_FB_ON_DEMAND = 0,   // unset: the above
       UPR_FB_EAGER = 1 };     // 1 | 0: the array is written with every advance, by the QP kernel's exit (1, where the selected kernel
                               //        can: upr_qp_choice::fb_fused) or by the gather kernel behind the advance (0)

struct upr_fb_track {
    int mode = UPR_FB_ON_DEMAND;
    int state = UPR_FB_NONE;
};

// what an advance with `qps` QP launches does about the gains
struct upr_fb_advance {
    bool gather_before = false;   // gather the array from the sources first: the advance is about to overwrite one of them
    bool kernel_writes = false;   // the advance's last QP writes the array at its exit (upr_qp_args::fb)
    bool gather_after = false;    // the gather kernel behind the advance
    int state = UPR_FB_NONE;      // ... and where the gains are afterwards
};
static inline upr_fb_advance upr_fb_on_advance(const upr_fb_track& t, int qps, bool kernel_can_write) {
    upr_fb_advance a;
    if (t.mode == UPR_FB_EAGER) {
        a.kernel_writes = kernel_can_write && qps > 0;
        a.gather_after = !a.kernel_writes;
        a.state = UPR_FB_ARRAY;
        return a;
    }
    if (qps > 0) { a.state = UPR_FB_FACTORS; return a; }   // the new gains supersede the old ones: nothing to keep
    // no QP: the gains stay those of the advance before, but the statistics are cleared -- the QP status with them, which says
    // whose factors are no policy
    a.gather_before = t.state == UPR_FB_FACTORS;
    a.state = t.state == UPR_FB_FACTORS ? UPR_FB_ARRAY : t.state;
    return a;
}
// a control period replayed from the captured graph (upr_batch_tick): the host does not run the advance, the state moves as if it had.
// A period is captured only where its advance gathers nothing first (upr_fb_capturable)
static inline int upr_fb_on_replay(const upr_fb_track& t, int qps, bool kernel_can_write) { return upr_fb_on_advance(t, qps, kernel_can_write).state; }
static inline bool upr_fb_capturable(const upr_fb_track& t, int qps) {
    return t.mode == UPR_FB_EAGER || (t.state == UPR_FB_FACTORS && qps > 0);
}
// which policy kernel reads the gains in `state`: the one that forms them from the factors, or the one that reads the array
static inline bool upr_fb_policy_from_factors(int state) { return state == UPR_FB_FACTORS; }
// a request for the whole array, or a call that is about to overwrite a source of the gains (a QP or a linearisation launch on the
// handle's own workspace / records / statistics outside an advance, statistics put back over the solve's): gather first?
static inline bool upr_fb_must_gather(const upr_fb_track& t) { return t.state == UPR_FB_FACTORS; }
static inline int upr_fb_after_gather(const upr_fb_track& t) { return t.state == UPR_FB_FACTORS ? UPR_FB_ARRAY : t.state; }
