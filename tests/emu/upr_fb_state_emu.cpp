// Host binding of upr_fb_state.h for tests/test_fb_state.py: the rules upr_api.hip follows for where the feedback gains of a
// handle's last advance are, driven event by event.
#include "../../upright_amd/csrc/upr_fb_state.h"

extern "C" {
// an advance with `qps` QP launches from (mode, state): out[5] = gather_before, kernel_writes, gather_after, state, capturable
void emu_fb_advance(int mode, int state, int qps, int kernel_can_write, int* out) {
    upr_fb_track t; t.mode = mode; t.state = state;
    const upr_fb_advance a = upr_fb_on_advance(t, qps, kernel_can_write != 0);
    out[0] = a.gather_before; out[1] = a.kernel_writes; out[2] = a.gather_after; out[3] = a.state; out[4] = upr_fb_capturable(t, qps);
}
int emu_fb_replay(int mode, int state, int qps, int kernel_can_write) {
    upr_fb_track t; t.mode = mode; t.state = state;
    return upr_fb_on_replay(t, qps, kernel_can_write != 0);
}
// a full request or a clobbering call from (mode, state): out[2] = gathers, state afterwards
void emu_fb_keep(int mode, int state, int* out) {
    upr_fb_track t; t.mode = mode; t.state = state;
    out[0] = upr_fb_must_gather(t); out[1] = out[0] ? upr_fb_after_gather(t) : state;
}
int emu_fb_policy_from_factors(int state) { return upr_fb_policy_from_factors(state); }
}
