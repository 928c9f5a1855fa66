"""The replay of a time law on a clock on the MI355X (upr_batch_replay_plan, upright_amd/csrc/upr_replay.h): the assertions of
tests/test_replay.py with the device's answers on the same plans (tests/replay_ref.py), installed with set_guess; the device against the
host emulation of the same source; both forms on the one-body shape and a multi-body arrangement; BatchMPC.replay_plan; the absence of
side effects on the handle; the refusals.

Observed on the device (MI355X): slide at 1.1185, tick 0.01: rejected 37 38 39 140 141 142, between knots 4-5 and 15-16, the
retiming's duration finite, decisions and verdict equal to the emulation's; slide laws: rejected 21, 17, 19, the closed form's; generic
plans: counts 31 37 31 / 27 / 43, 0 of 198 / 162 / 258 jobs undecided, rejected 0 under the law's own scenario / 76 / 107, box_first -1 -1 -1
/ 6 -1 -1 / 11 12 12, states against numpy 9.9e-16 (q), 6.1e-15 (qdot), 3.2e-13 (qddot) at the scale max(1, |x|_inf), against the emulation
9.3e-16, 6.1e-15, 3.2e-13, iters and verdict equal; foam_die2: 0 of 172 undecided, 31 rejected, states 1.4e-15, 3.5e-15, 1.9e-13.  The
file takes 4.3 s, its slowest test 2.0 s."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import balance_ref as R
import replay_ref as V
import retime_ref as Q
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
    print("replay (device): %s took %.1f s; the slowest so far: %s, %.1f s" % (request.node.name, dt, _SLOWEST[1], _SLOWEST[0]))


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


def run(P, xs, params, speeds, level, tick, t0=0.0, K=None, boxes=True, form=-1):
    return V.run_device(_handle(P, xs.shape[0]), xs, params, speeds, level, tick, t0, K, boxes)


def _retime(P, xs, params, speeds):
    h = _handle(P, xs.shape[0])
    h.set_guess(xs, np.zeros((h.B, h.N, h.nu)))
    return h.retime_plan(speeds, params, boxes=False)[0]


def test_between_the_knots(arrangements):
    """1. the slide at 1.1185 on a 10 ms clock: the device rejects the closed form's samples, between knots 4-5 and 15-16, where
    retime_plan returns a finite duration; and answers as the emulation does."""
    assert V.body_between_knots(run, arrangements, retime=_retime) == [37, 38, 39, 140, 141, 142]
    S = Q.slide_case(arrangements)
    level, sp = np.zeros((2, S["P"].N + 1), dtype=np.int32), np.array([1.1185])
    dev = run(S["P"], S["xs"], S["params"], sp, level, 0.01, K=179, boxes=False)
    emu = V.run_emu(S["P"], S["xs"], S["params"], sp, level, 0.01, K=179, boxes=False)
    assert np.array_equal(dev["excess"] <= V.EPS, emu["excess"] <= V.EPS) and np.array_equal(dev["verdict"][..., 1:], emu["verdict"][..., 1:])
    assert _handle(S["P"], 2).balance_ms() > 0.0


def test_slide_laws_with_path_acceleration(arrangements):
    """2."""
    V.body_slide_laws(run, arrangements)


def test_generic_plans(arrangements):
    """3., 4. and 6. the generic plans under their three laws: states, T_N and count against numpy, decisions against the reference,
    the reductions against numpy's on the answer's own excess; then the device against the emulation of the form it runs."""
    res = V.body_generic(run, arrangements)
    assert res["top"][2] == 162 and res["zigzag"][2] == 258
    G, laws = V.generic_laws(arrangements)
    for name, level in laws:
        dev = run(G["P"], G["xs"], G["params"], G["speeds"], level, 0.05)
        emu = V.run_emu(G["P"], G["xs"], G["params"], G["speeds"], level, 0.05)
        assert V.agree(dev, emu, G["P"], G["xs"], G["params"], G["speeds"], level, 0.05, exact=True) >= 60
        print("replay, device against the emulation, %s: state errors %s" % (name, V.state_errors(dev["x"], emu["x"])))


def test_shapes_and_edges(arrangements):
    """5."""
    V.body_edges(run, arrangements)


def test_multi_body_arrangement(arrangements):
    """5. foam_die2 (two bodies, eight contacts: the wave form), B = 2, and the device against the emulation."""
    dev = V.body_multi_body(run, arrangements)
    M = V.multi_body_case(arrangements)
    emu = V.run_emu(M["P"], M["xs"], M["params"], M["speeds"], M["level"], 0.05)
    V.agree(dev, emu, M["P"], M["xs"], M["params"], M["speeds"], M["level"], 0.05, exact=True)


def test_one_body_shape_on_the_wave_form(arrangements, monkeypatch):
    """5. UPR_BAL_FORM=0 sends the one-body shape through the wave-per-job kernel: checks 1 and 4, against the emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    V.body_between_knots(run, arrangements)
    V.body_generic(run, arrangements)
    G, laws = V.generic_laws(arrangements)
    name, level = laws[2]
    dev = run(G["P"], G["xs"], G["params"], G["speeds"], level, 0.05)
    emu = V.run_emu(G["P"], G["xs"], G["params"], G["speeds"], level, 0.05, form=0)
    V.agree(dev, emu, G["P"], G["xs"], G["params"], G["speeds"], level, 0.05, exact=True)


def test_python_entry(arrangements):
    """BatchMPC.replay_plan: (t, x, excess) with NaN past the end, want_rho / want_iters, n_samples=None from the durations,
    reductions=True equal to numpy's reduction of the full call, a law per scenario refused; x alone through the C entry."""
    G, laws = V.generic_laws(arrangements)
    P, own = G["P"], laws[0][1]
    h = _handle(P, 3)
    h.set_guess(G["xs"], np.zeros((h.B, h.N, h.nu)))
    raw = run(P, G["xs"], G["params"], G["speeds"], own, 0.05)
    t, x, excess, rho, iters = h.replay_plan(own, G["speeds"], 0.05, G["params"], want_rho=True, want_iters=True)
    K = raw["x"].shape[1]
    assert t.shape == (K,) and np.array_equal(t, 0.05 * np.arange(K)) and x.shape == raw["x"].shape and excess.shape == raw["excess"].shape
    for b in range(3):
        n = raw["count"][b]
        assert np.array_equal(x[b, :n], raw["x"][b, :n]) and np.all(np.isnan(x[b, n:])) and np.all(np.isnan(excess[b, n:]))
    assert np.array_equal(excess, raw["excess"], equal_nan=True) and np.array_equal(rho, raw["rho"], equal_nan=True) and np.array_equal(iters, raw["iters"])
    assert len(h.replay_plan(own, G["speeds"], 0.05, G["params"])) == 3
    dur, count, worst, verdict, bfirst = h.replay_plan(own, G["speeds"], 0.05, G["params"], reductions=True)
    for a, b in ((dur, raw["duration"]), (count, raw["count"]), (worst, raw["worst"]), (verdict, raw["verdict"]), (bfirst, raw["box_first"])):
        assert np.array_equal(a, b, equal_nan=True)
    t2, x2, e2 = h.replay_plan(own, G["speeds"], 0.05, G["params"], t0=0.2, n_samples=5, boxes=False)
    assert np.array_equal(t2, 0.2 + 0.05 * np.arange(5)) and x2.shape[1] == 5
    with pytest.raises(ValueError, match="once per scenario"):
        h.replay_plan(np.zeros((3, 2, P.N + 1), dtype=np.int32), G["speeds"], 0.05, G["params"])
    # x alone: nothing is projected, the states are those of the full call
    xo = np.full(raw["x"].shape, -7.0)
    sp, lv = np.ascontiguousarray(G["speeds"]), np.ascontiguousarray(own, dtype=np.int32)
    assert h._lib.upr_batch_replay_plan(h._h, 1, None, 0, sp.size, ptr(sp), iptr(lv), 0.05, 0.0, K, 1, None, None, ptr(xo), None, None, None, None, None, None) == 0
    assert np.array_equal(xo, raw["x"])


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_calls_leave_the_handle_as_it_was(arrangements):
    """7. Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the replay on one of
    them only, between the other calls: solution(), stats(), the next advance() and the ticks (the later ones replayed from the captured
    graph) are bitwise equal."""
    B = 3
    (H, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = Q.shifted(H.problem)
    sp = np.array(Q.SLIDE_SPEEDS)
    ones = np.full((B, H.N + 1), 3, dtype=np.int32)
    ramp = np.tile(np.array(V.RAMP, dtype=np.int32), (B, 1))
    probe = lambda: (H.replay_plan(ones, sp, 0.01, want_rho=True, want_iters=True),   # noqa: E731
                     H.replay_plan(ramp, sp, 0.037, scen, t0=0.1, boxes=False),
                     H.replay_plan(ramp, sp, 0.05, scen, reductions=True))
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
    assert all(np.array_equal(a, b, equal_nan=True) for u, v in zip(first, again) for a, b in zip(u, v))
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
    """7. tick 0, -1, inf, NaN and t0 -1, NaN; n_samp 0, -1, 65537; level NULL; a level out of the lattice, -2, -1 in part of a plan;
    speed 0 held over a segment; their order among themselves, after the lattice refusal, a bad mass first; every output NULL -- through
    ctypes so that nothing in Python refuses first: the message, the output buffers untouched, the handle answers as before."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    S = Q.slide_case(arrangements)
    P = S["P"]
    h = BatchMPC(P, 2)
    h.set_guess(S["xs"], np.zeros((2, P.N, P.nu)))
    scen = np.ascontiguousarray(Q.shifted(P))
    good = np.array(Q.SLIDE_SPEEDS)
    ramp = np.tile(np.array(V.RAMP, dtype=np.int32), (2, 1))
    before = h.replay_plan(ramp, good, 0.037, scen, want_rho=True, want_iters=True)
    K = before[1].shape[1]
    bufs = V.blank(P, 2, K, 2)
    lib = h._lib

    def call(speeds=good, M=6, level=ramp, tick=0.037, t0=0.0, n_samp=K, params=scen, keep=("duration", "count", "x", "rho", "excess", "iters", "worst", "verdict", "box_first")):
        speeds = np.ascontiguousarray(speeds, dtype=np.float64)
        level = None if level is None else np.ascontiguousarray(level, dtype=np.int32)
        o = {k: (bufs[k] if k in keep else None) for k in bufs}
        return lib.upr_batch_replay_plan(h._h, 2, ptr(params), 0, M, ptr(speeds), iptr(level), C.c_double(tick), C.c_double(t0), n_samp, 1, ptr(o["duration"]),
                                         iptr(o["count"]), ptr(o["x"]), ptr(o["rho"]), ptr(o["excess"]), iptr(o["iters"]), ptr(o["worst"]), iptr(o["verdict"]),
                                         iptr(o["box_first"]))
    m_clock = b"replay: tick must be finite and > 0, t0 finite and >= 0"
    m_samp = b"replay: n_samp must be 1 .. 65536"
    m_null = b"replay: level must not be NULL"
    m_level = b"replay: level must hold lattice indices, or -1 throughout a plan"
    m_rest = b"replay: a law must not hold speed 0 over a segment"
    m_lattice = b"retime: speeds must be 1 .. 32 finite values >= 0 in strictly increasing order"
    for kw in (dict(tick=0.0), dict(tick=-1.0), dict(tick=np.inf), dict(tick=np.nan), dict(t0=-1.0), dict(t0=np.nan), dict(t0=np.inf)):
        assert call(**kw) != 0 and m_clock in lib.upr_last_error(), (kw, lib.upr_last_error())
    for n in (0, -1, 65537):
        assert call(n_samp=n) != 0 and m_samp in lib.upr_last_error(), (n, lib.upr_last_error())
    assert call(level=None) != 0 and m_null in lib.upr_last_error()
    high, low, part, rest = ramp.copy(), ramp.copy(), ramp.copy(), ramp.copy()
    high[1, 7] = 6
    low[0, 0] = -2
    part[1, 20] = -1
    rest[1, 9:11] = 0
    for lv in (high, low, part):
        assert call(level=lv) != 0 and m_level in lib.upr_last_error(), lib.upr_last_error()
    assert call(level=rest) != 0 and m_rest in lib.upr_last_error()
    # the order among themselves; the lattice refusal before all of them; a bad mass before everything
    assert call(tick=0.0, n_samp=0, level=None) != 0 and m_clock in lib.upr_last_error()
    assert call(n_samp=0, level=None) != 0 and m_samp in lib.upr_last_error()
    both = part.copy(); both[0, 9:11] = 0
    assert call(level=both) != 0 and m_level in lib.upr_last_error()
    assert call(speeds=[1.0, 0.5], M=2, tick=0.0, n_samp=0, level=None) != 0 and m_lattice in lib.upr_last_error()
    heavy = scen.copy(); heavy[0, 0, 0] = -1.0
    assert call(M=0, tick=np.nan, level=None, params=heavy) != 0 and b"positive finite mass" in lib.upr_last_error()
    assert call(tick=0.0, keep=("duration", "count", "iters", "verdict", "box_first")) != 0
    assert b"upr_batch_replay_plan: x, rho, excess and worst must not all be NULL" in lib.upr_last_error()
    assert all(np.all(v == v.dtype.type(-7)) for v in bufs.values())
    with pytest.raises(RuntimeError, match="tick must be finite"):
        h.replay_plan(ramp, good, 0.0, scen, n_samples=4)
    with pytest.raises(RuntimeError, match="speed 0 over a segment"):
        h.replay_plan(rest, good, 0.037, scen)
    # NULL outputs are not copied: worst alone
    assert call(keep=("worst",)) == 0 and all(np.all(v == v.dtype.type(-7)) for k, v in bufs.items() if k != "worst")
    e = before[2]
    assert np.array_equal(bufs["worst"], np.nanmax(e, axis=1))
    after = h.replay_plan(ramp, good, 0.037, scen, want_rho=True, want_iters=True)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(before, after))
    h.close()
