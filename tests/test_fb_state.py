"""Where the feedback gains of a handle's last advance are (upr_fb_state.h): the rules upr_api.hip follows, on the host.  The gains
are formed on demand -- an advance leaves them in the factors of its last QP, the policy reads them there, the whole array is
gathered at the first request or before a call overwrites a source -- unless UPR_FB_FUSED is set (the array with every advance).
tests/emu/upr_fb_state_emu.cpp binds the header; tests/test_gpu_feedback_on_demand.py holds the device against the same sequences."""
import ctypes as C
from pathlib import Path

import pytest

HERE = Path(__file__).resolve().parent
NONE, FACTORS, ARRAY = 0, 1, 2
ON_DEMAND, EAGER = 0, 1


@pytest.fixture(scope="module")
def emu():
    lib = C.CDLL(str(HERE / "emu" / "libupr_fb_state_emu.so"))
    lib.emu_fb_advance.argtypes = [C.c_int] * 4 + [C.POINTER(C.c_int)]
    lib.emu_fb_replay.argtypes = [C.c_int] * 4
    lib.emu_fb_keep.argtypes = [C.c_int] * 2 + [C.POINTER(C.c_int)]
    return lib


class Handle:
    """The host side of a handle: the state and a log of what the events launched."""

    def __init__(self, emu, mode, kernel_can_write=True):
        self.emu, self.mode, self.can, self.state, self.log = emu, mode, kernel_can_write, NONE, []

    def advance(self, qps=1):
        out = (C.c_int * 5)()
        self.emu.emu_fb_advance(self.mode, self.state, qps, int(self.can), out)
        before, writes, after, state, _ = list(out)
        qp = ["qp"] * (qps - 1) + ["qp+fb" if writes else "qp"] if qps > 0 else []      # (the advance's LAST QP writes, where one does)
        self.log += ["gather"] * before + qp + ["gather"] * after
        self.state = state

    def capturable(self, qps=1):
        out = (C.c_int * 5)()
        self.emu.emu_fb_advance(self.mode, self.state, qps, int(self.can), out)
        return bool(out[4])

    def replay(self, qps=1):
        self.state = self.emu.emu_fb_replay(self.mode, self.state, qps, int(self.can))

    def keep(self):      # a full request, or a call that overwrites a source
        out = (C.c_int * 2)()
        self.emu.emu_fb_keep(self.mode, self.state, out)
        self.log += ["gather"] * out[0]
        self.state = out[1]

    def policy_kernel(self):
        return "factors" if self.emu.emu_fb_policy_from_factors(self.state) else "array"


def test_advance_then_requests(emu):
    h = Handle(emu, ON_DEMAND)
    assert h.state == NONE and h.policy_kernel() == "array"
    h.keep()
    assert h.state == NONE and h.log == []                  # no solve yet: nothing to gather
    h.advance()
    assert h.state == FACTORS and h.log == ["qp"]           # neither the kernel's exit nor a gather behind it
    assert h.policy_kernel() == "factors"
    h.keep()
    assert h.state == ARRAY and h.log == ["qp", "gather"]   # the first request gathers ...
    h.keep()
    assert h.state == ARRAY and h.log == ["qp", "gather"]   # ... later ones only copy
    assert h.policy_kernel() == "array"


def test_advance_then_clobbering_call_then_request(emu):
    h = Handle(emu, ON_DEMAND)
    h.advance()
    h.keep()            # (upr_batch_qp_kkt, upr_batch_qp_step, upr_batch_value_function_update, upr_batch_hold_stats putting back)
    assert h.state == ARRAY and h.log == ["qp", "gather"]
    h.keep()            # the request behind it
    assert h.log == ["qp", "gather"]


@pytest.mark.parametrize("first", [FACTORS, ARRAY])
def test_next_advance_supersedes(emu, first):
    h = Handle(emu, ON_DEMAND)
    h.advance()
    if first == ARRAY:
        h.keep()
    n = len(h.log)
    h.advance(3)
    assert h.state == FACTORS and h.log[n:] == ["qp"] * 3   # the old gains are not gathered for nobody


def test_replayed_tick(emu):
    h = Handle(emu, ON_DEMAND)
    assert not h.capturable()       # no solve yet
    h.advance()
    assert h.capturable() and not h.capturable(qps=0)
    h.keep()
    assert h.state == ARRAY and not h.capturable()      # (a period is captured from gains in the factors only)
    h.replay()                                          # a replay is the advance as captured: it needs nothing of the old gains
    assert h.state == FACTORS and h.policy_kernel() == "factors"
    h.replay()
    assert h.state == FACTORS


def test_advance_without_a_qp(emu):
    h = Handle(emu, ON_DEMAND)
    h.advance(0)
    assert h.state == NONE and h.log == []
    h.advance()
    h.advance(0)        # clears the statistics (the QP status with them): the gains of the advance before are gathered first
    assert h.state == ARRAY and h.log == ["qp", "gather"]
    h.advance(0)
    assert h.state == ARRAY and h.log == ["qp", "gather"]


@pytest.mark.parametrize("can", [True, False])
def test_knob_set_is_the_array_with_every_advance(emu, can):
    """UPR_FB_FUSED = 1 on the production kernel: its exit writes; = 0, or a kernel that cannot: the gather behind the advance."""
    h = Handle(emu, EAGER, kernel_can_write=can)
    h.advance(2)
    assert h.state == ARRAY and h.log == (["qp", "qp+fb"] if can else ["qp", "qp", "gather"])
    assert h.capturable() and h.policy_kernel() == "array"
    h.keep()
    assert h.log.count("gather") == (0 if can else 1)
    h.replay()
    assert h.state == ARRAY
    h.advance(0)
    assert h.state == ARRAY and h.log[-1] == "gather"    # (as before this rule existed: no QP, the gather kernel)
