"""The retiming with substeps on the MI355X (upr_batch_retime_plan_substeps, upright_amd/csrc/upr_retime_sub.h): the assertions of
tests/test_retime_substeps.py with the device's answers on the same plans (tests/retime_sub_ref.py), installed with set_guess; R = 1
against upr_batch_retime_plan bit for bit; the device against the host emulation of the same source; both forms on the one-body shape and
a two-body arrangement; the laws through replay_plan and balance_check; retimed_substates; the layouts of params; the absence of side
effects on the handle; the refusals."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import balance_ref as R
import replay_ref as Y
import retime_ref as Q
import retime_sub_ref as U
from upright_amd._capi import iptr, ptr
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

_HANDLES = {}
_SLOWEST = [0.0, ""]


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.time()
    yield
    dt = time.time() - t0
    if dt > _SLOWEST[0]:
        _SLOWEST[:] = [dt, request.node.name]
    print("retime with substeps (device): %s took %.1f s; the slowest so far: %s, %.1f s" % (request.node.name, dt, _SLOWEST[1], _SLOWEST[0]))


def _handle(P, B):
    """one handle per (problem, batch, form of the balance kernels) for the module"""
    key = (id(P), B, os.environ.get("UPR_BAL_FORM", ""))
    if key not in _HANDLES:
        _HANDLES[key] = (BatchMPC(P, B), P)
        assert _HANDLES[key][0].nxf == 3 * P.nq
    return _HANDLES[key][0]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h, _ in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def run(P, xs, params, speeds, substeps=1, start=-1, end=-1, common=False, boxes=True, form=-1):
    return U.run_device(_handle(P, xs.shape[0]), xs, params, np.asarray(speeds, dtype=np.float64), substeps, start, end, common, boxes)


def plain(P, xs, params, speeds, start=-1, end=-1, common=False, boxes=True, form=-1):
    speeds = np.asarray(speeds, dtype=np.float64)
    return Q.run_device(_handle(P, xs.shape[0]), xs, params, speeds, None if start < 0 else speeds[start], None if end < 0 else speeds[end], common, boxes)


def test_closed_form_slide_between_the_knots(arrangements):
    """1. and the laws through upr_batch_replay_plan on a 10 ms clock; the device's answers are the emulation's."""
    def replay(P, xs, params, speeds, level, tick, K):
        return Y.run_device(_handle(P, xs.shape[0]), xs, params, speeds, level, tick, K=K, boxes=False)
    outs = U.body_slide(run, arrangements, replay)
    S = Q.slide_case(arrangements)
    for c in (((1.1185,), 4), (U.NARROW, 4), (U.NARROW, 8)):
        emu = U.run_emu(S["P"], S["xs"], S["params"], np.array(c[0]), substeps=c[1], boxes=False)
        assert U.same(outs[c], emu, ("edges", "duration", "level", "reach")), c
    # BatchMPC.retime_plan: substeps=1 is the plain entry, substeps > 1 the new one
    h = _handle(S["P"], 2)
    h.set_guess(S["xs"], np.zeros((2, h.N, h.nu)))
    assert np.all(np.isfinite(h.retime_plan([1.1185], boxes=False)[0])) and np.all(np.isfinite(h.retime_plan([1.1185], boxes=False, substeps=2)[0]))
    assert np.all(np.isinf(h.retime_plan([1.1185], boxes=False, substeps=4)[0]))
    dur, level = h.retime_plan(U.NARROW, boxes=False, substeps=4)
    assert np.array_equal(dur, outs[U.NARROW, 4]["duration"]) and np.array_equal(level, outs[U.NARROW, 4]["level"])
    assert np.all(h.replay_plan(level[:, 0], U.NARROW, 0.01, boxes=False, reductions=True)[3][..., 2] == 0)


def test_one_substep_is_the_plain_retiming(arrangements, monkeypatch):
    """2. R = 1 through the new entry against upr_batch_retime_plan: edges, iters, duration, level and reach bit for bit, lane and wave
    form."""
    assert U.body_r1_is_the_plain_retiming(run, plain, arrangements, forms=(-1,)) == 4
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    assert U.body_r1_is_the_plain_retiming(run, plain, arrangements, forms=(0,)) == 4


def test_reference_on_generic_plans(arrangements):
    """3. and 8.: the lane form against the reference and against its emulation."""
    out = U.body_reference(run, arrangements)
    G = U.generic_case(arrangements)
    assert _handle(G["P"], 3).balance_ms() > 0.0
    emu = U.run_emu(G["P"], G["xs"], G["params"], G["speeds"], substeps=3)
    assert U.agree(out, emu, G["sub"], 2, exact=True) >= 100


def test_one_body_shape_on_the_wave_form(arrangements, monkeypatch):
    """8. UPR_BAL_FORM=0 sends the one-body shape through the wave-per-job kernel: test 3's assertions, the emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    out = U.body_reference(run, arrangements)
    G = U.generic_case(arrangements)
    emu = U.run_emu(G["P"], G["xs"], G["params"], G["speeds"], substeps=3, form=0)
    assert U.agree(out, emu, G["sub"], 2, exact=True) >= 100
    S = Q.slide_case(arrangements)
    assert np.array_equal(run(S["P"], S["xs"], S["params"], np.array(U.NARROW), substeps=4, boxes=False)["edges"], U.slide_ref(arrangements, U.NARROW, 4)["masks"])


def test_multi_body_arrangement(arrangements):
    """3. and 8.: foam_die2 (two bodies, eight contacts: the wave form), B = 2, M = 3, R = 2, and the device against the emulation."""
    kw = dict(name="foam_die2", B=2, plans=2, speeds=(0.5, 1.0, 1.5), Rs=2)
    out = U.body_reference(run, arrangements, **kw)
    G = U.generic_case(arrangements, **kw)
    emu = U.run_emu(G["P"], G["xs"], G["params"], G["speeds"], substeps=2)
    assert U.agree(out, emu, G["sub"], 2, exact=True) >= 50


def test_the_point_sets_nest(arrangements):
    """4."""
    U.body_nesting(run, arrangements)


def test_substates(arrangements):
    """5. every substate of every feasible generic law through balance_check; BatchMPC.retimed_substates against numpy's, r = 0 and r = R
    against retimed_states as doubles."""
    G = U.generic_case(arrangements)
    P, h = G["P"], _handle(G["P"], 3)
    out = U.body_substates_are_balanced(run, arrangements, lambda P_, x, th: h.balance_check(x, th[None])[:, 0])
    full = run(P, G["xs"], G["params"], G["speeds"], substeps=3)
    assert np.array_equal(full["level"][:2], out["level"])
    t, x = h.retimed_substates(full["level"], G["speeds"], 3)
    T, dep, arr = h.retimed_states(full["level"], G["speeds"])
    ok = np.isfinite(full["duration"])
    assert t.shape == full["duration"].shape + (P.N, 4) and x.shape == t.shape + (3 * P.nq,)
    assert ok.any() and np.array_equal(x[ok][:, :, 0], dep[ok]) and np.array_equal(x[ok][:, :, 3], arr[ok]) and np.array_equal(t[ok][:, :, 0], T[ok][:, :-1])
    assert np.all(np.isnan(t[~ok])) and np.all(np.isnan(x[~ok]))
    t0, x0 = U.substates(P, G["xs"], full["level"], G["speeds"], 3)
    assert np.allclose(t[ok], t0[ok], rtol=1e-13, atol=0)
    Y.assert_states(x[ok], x0[ok])
    one = h.retimed_substates(full["level"][:, 0], G["speeds"], 1)      # (B, N + 1): one law per instance, R = 1
    assert one[0].shape == (3, P.N, 2) and one[1].shape == (3, P.N, 2, 3 * P.nq)


def test_boxes(arrangements):
    """6."""
    U.body_boxes(run, arrangements)


def test_common_time_law(arrangements):
    """7."""
    U.body_common(run, arrangements)


def test_layouts_of_params(arrangements):
    """9. NULL, shared and per instance; substeps > 1 with a reserve is a ValueError."""
    U.body_layouts(run, arrangements)
    G = Q.generic_case(arrangements)
    h = _handle(G["P"], 3)
    dirs = np.array([[0, 0, 0, 0, 0, 1.0]])
    with pytest.raises(ValueError, match="reserve"):
        h.retime_plan(G["speeds"], G["params"], substeps=2, reserve=0.25, dirs=dirs)
    with pytest.raises(ValueError, match="integer"):
        h.retime_plan(G["speeds"], G["params"], substeps=2.5)
    assert h.retime_plan(G["speeds"], G["params"], substeps=1, reserve=0.25, dirs=dirs)[0].shape == (3, 2)


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_calls_leave_the_handle_as_it_was(arrangements):
    """11. Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the retiming with
    substeps on one of them only, between the other calls: solution(), stats(), the next advance() and the ticks (the later ones
    replayed from the captured graph) are bitwise equal."""
    B = 3
    (H, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = Q.shifted(H.problem)
    sp = np.array(Q.SLIDE_SPEEDS)
    probe = lambda: (H.retime_plan(sp, want_reach=True, want_edges=True, want_iters=True, substeps=4),   # noqa: E731
                     H.retime_plan(sp, scen, common=True, end=0.0, substeps=2),
                     H.retime_plan(sp[1:], scen, start=1.0, boxes=False, want_edges=True, substeps=16))
    for h in (H, T):
        h.track_value_function()
        h.set_observation(0.0, x0)
    probe()
    for h in (H, T):
        h.advance()
    first = probe()
    for k, (u, v) in enumerate(zip(H.solution(), T.solution())):
        assert np.array_equal(u, v), k
    sa, st = H.stats(), T.stats()
    assert all(np.array_equal(sa[k], st[k]) for k in sa)
    again = probe()
    assert all(np.array_equal(a, b) for u, v in zip(first, again) for a, b in zip(u, v))
    for h in (H, T):
        h.set_observation(0.1, x0)
        h.advance()
    for u, v in zip(H.solution(), T.solution()):
        assert np.array_equal(u, v)
    x = x0.copy()
    for k in range(5):
        xa, ua = H.tick(0.2 + 0.01 * k, x)
        xt, ut = T.tick(0.2 + 0.01 * k, x)
        assert np.array_equal(xa, xt) and np.array_equal(ua, ut), k
        if k >= 2:
            probe()
        x = xa
    assert H.tick_graph_replays() == T.tick_graph_replays() >= 1
    H.close(); T.close()


@pytest.mark.parametrize("form", ["", "0"])
def test_refusals(arrangements, form, monkeypatch):
    """10. substeps 0, -1, 17; after the two retime refusals, a bad mass first; both outputs NULL -- through ctypes so that nothing in
    Python refuses first: the message, the output buffers untouched, the handle answers as before."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    S = Q.slide_case(arrangements)
    P = S["P"]
    h = BatchMPC(P, 2)
    h.set_guess(S["xs"], np.zeros((2, P.N, P.nu)))
    scen = np.ascontiguousarray(Q.shifted(P))
    good = np.array(Q.SLIDE_SPEEDS)
    before = h.retime_plan(good, scen, want_reach=True, want_edges=True, want_iters=True, substeps=3)
    POISON = -7
    room = 2 * 2 * (P.N + 1) * 40
    bufs = dict(duration=np.full(room, float(POISON)), level=np.full(room, POISON, dtype=np.int32), reach=np.full(room, POISON, dtype=np.int32),
                edges=np.full(room, 7, dtype=np.uint32), iters=np.full(room, POISON, dtype=np.int32))
    lib = h._lib
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))   # noqa: E731

    def call(speeds=good, M=6, start=-1, end=-1, substeps=3, params=scen, duration=bufs["duration"], level=bufs["level"]):
        speeds = np.ascontiguousarray(speeds, dtype=np.float64)
        return lib.upr_batch_retime_plan_substeps(h._h, 2, ptr(params), 0, M, ptr(speeds), start, end, 0, 1, substeps, ptr(duration), iptr(level),
                                                  iptr(bufs["reach"]), up(bufs["edges"]), iptr(bufs["iters"]))
    m_sub = b"retime: substeps must be 1 .. 16"
    m_lattice = b"retime: speeds must be 1 .. 32 finite values >= 0 in strictly increasing order"
    m_levels = b"retime: start and end must be -1 or a level index"
    for r in (0, -1, 17):
        assert call(substeps=r) != 0 and m_sub in lib.upr_last_error(), (r, lib.upr_last_error())
    # the order: the two retime refusals before it, a bad mass before everything
    assert call(start=6, substeps=0) != 0 and m_levels in lib.upr_last_error()
    assert call(speeds=[1.0, 0.5], M=2, start=6, substeps=17) != 0 and m_lattice in lib.upr_last_error()
    heavy = scen.copy(); heavy[0, 0, 0] = -1.0
    assert call(M=0, substeps=0, params=heavy) != 0 and b"positive finite mass" in lib.upr_last_error()
    assert call(duration=None, level=None, substeps=0) != 0
    assert b"upr_batch_retime_plan_substeps: duration and level must not both be NULL" in lib.upr_last_error()
    assert all(np.all(v == v.dtype.type(7 if k == "edges" else POISON)) for k, v in bufs.items())
    with pytest.raises(RuntimeError, match="substeps must be 1 .. 16"):
        h.retime_plan(good, scen, substeps=17)
    with pytest.raises(RuntimeError, match="substeps must be 1 .. 16"):
        h.retime_plan(good, scen, substeps=0)
    # NULL outputs are not copied: duration alone, level alone
    assert call(level=None) == 0 and np.all(bufs["level"] == POISON) and np.array_equal(bufs["duration"][:4].reshape(2, 2), before[0])
    bufs["duration"][:] = POISON
    assert call(duration=None) == 0 and np.all(bufs["duration"] == POISON) and np.array_equal(bufs["level"][:before[1].size].reshape(before[1].shape), before[1])
    after = h.retime_plan(good, scen, want_reach=True, want_edges=True, want_iters=True, substeps=3)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    h.close()
