"""The retiming with a reserve on the MI355X (upr_batch_retime_plan_reserve, upright_amd/csrc/upr_retime_rsv.h): the assertions of
tests/test_retime_reserve.py with the device's answers on the same plans (tests/retime_rsv_ref.py), installed with set_guess; the device
against the host emulation of the same source; both forms on the one-body shape and a multi-body arrangement; the laws through
disturbance_margin; the layouts of params; the absence of side effects on the handle; the refusals."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import balance_ref as R
import retime_ref as Q
import retime_rsv_ref as V
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
    print("retime with a reserve (device): %s took %.1f s; the slowest so far: %s, %.1f s" % (request.node.name, dt, _SLOWEST[1], _SLOWEST[0]))


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


def run(P, xs, params, speeds, dirs=None, reserve=None, frame="tray", start=-1, end=-1, common=False, boxes=True, form=-1):
    speeds = np.asarray(speeds, dtype=np.float64)
    h = _handle(P, xs.shape[0])
    return V.run_device(h, xs, params, speeds, dirs, reserve, frame, None if start < 0 else speeds[start], None if end < 0 else speeds[end], common, boxes)


def _against_emulation(out, G, form=-1):
    """9. masks and iters on decided edges (rows), duration, level and reach on decided plans"""
    n = G["plans"]
    emu = V.run_emu(G["P"], G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=G["r"], form=form)
    dec = G["rsv"]["decided"]
    bits = Q.decided_bits(dec)
    assert np.array_equal(out["edges"][:n] & bits, emu["edges"][:n] & bits)
    rows = dec.all(axis=-1)
    assert rows.sum() >= 100 and np.array_equal(out["iters"][:n][rows], emu["iters"][:n][rows])
    plans = dec.all(axis=(2, 3, 4))
    assert plans.any() and np.array_equal(out["duration"][:n][plans], emu["duration"][:n][plans]) and np.array_equal(out["level"][:n][plans], emu["level"][:n][plans])
    assert np.array_equal(out["reach"][:n][plans], emu["reach"][:n][plans])


def test_closed_form_slide(arrangements):
    outs = V.body_closed_form(run, arrangements)
    S = V.slide_case(arrangements)
    for k in (0, 2):
        emu = V.run_emu(S["P"], S["xs"], S["params"], S["speeds"], dirs=S["dirs"][k:k + 1], reserve=S["r"], boxes=False)
        assert all(np.array_equal(outs[k][key], emu[key]) for key in ("edges", "duration", "level", "reach")), k


def test_reference_on_generic_plans(arrangements):
    out = V.body_reference(run, arrangements)
    G = V.generic_case(arrangements)
    assert _handle(G["P"], 3).balance_ms() > 0.0
    _against_emulation(out, G)


def test_zero_reserve_is_the_plain_retiming(arrangements, monkeypatch):
    assert V.body_zero_reserve(run, arrangements, forms=(-1,)) == 3
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    assert V.body_zero_reserve(run, arrangements, forms=(0,)) == 3


def test_monotone_in_the_reserve_and_the_directions(arrangements):
    V.body_monotone(run, arrangements)


def test_the_law_keeps_what_it_reserved(arrangements):
    def margin(P, x, theta, dirs):
        return _handle(P, 3).disturbance_margin(x, theta[None], dirs, r_max=8.0)[:, :, 0]
    V.body_keeps_reserve(run, arrangements, margin)
    # BatchMPC.retimed_states of the device's laws are numpy's
    G = V.generic_case(arrangements)
    P, h = G["P"], _handle(G["P"], 3)
    out = run(P, G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=G["r"])
    t, dep, arr = h.retimed_states(out["level"], G["speeds"])
    t0, dep0, arr0 = Q.retimed_states(G["xs"], out["level"], G["speeds"], float(P.dt), P.nq)
    ok = np.isfinite(out["duration"])
    assert ok.any() and np.array_equal(t[ok], t0[ok]) and np.array_equal(dep[ok], dep0[ok]) and np.array_equal(arr[ok], arr0[ok])


def test_frames_and_order(arrangements):
    V.body_frames_and_order(run, arrangements)


def test_shapes(arrangements):
    V.body_shapes(run, arrangements)


def test_one_body_shape_on_the_wave_form(arrangements, monkeypatch):
    """8. UPR_BAL_FORM=0 sends the one-body shape through the wave-per-job kernel: test 2's assertions, the emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    out = V.body_reference(run, arrangements)
    _against_emulation(out, V.generic_case(arrangements), form=0)
    S = V.slide_case(arrangements)
    assert np.array_equal(run(S["P"], S["xs"], S["params"], S["speeds"], dirs=S["dirs"][:1], reserve=S["r"], boxes=False)["edges"], S["refs"][0]["masks"])


def test_multi_body_arrangement(arrangements):
    """8. foam_die2 (two bodies, eight contacts), B = 1, M = 3, n_dir = 2, and the device against the emulation."""
    kw = dict(name="foam_die2", B=1, plans=1, speeds=(0.5, 1.0, 1.5), n_dir=2)
    out = V.body_reference(run, arrangements, **kw)
    G = V.generic_case(arrangements, **kw)
    emu = V.run_emu(G["P"], G["xs"], G["params"], G["speeds"], dirs=G["dirs"], reserve=G["r"])
    bits = Q.decided_bits(G["rsv"]["decided"])
    rows = G["rsv"]["decided"].all(axis=-1)
    assert np.array_equal(out["edges"] & bits, emu["edges"] & bits) and np.array_equal(out["iters"][rows], emu["iters"][rows])
    assert np.array_equal(out["duration"], emu["duration"]) and np.array_equal(out["level"], emu["level"]) and np.array_equal(out["reach"], emu["reach"])


def test_layouts_of_params(arrangements):
    """10. scenarios per instance (B, n_scen, nb, 10) and params=None (every instance's own body parameters) give what the shared layout
    gives for the same parameters."""
    G = V.generic_case(arrangements)
    P, xs, sp, kw = G["P"], G["xs"], G["speeds"], dict(dirs=G["dirs"], reserve=G["r"])
    B = xs.shape[0]
    shared = run(P, xs, G["params"], sp, **kw)
    per = run(P, xs, np.repeat(G["params"][None], B, axis=0), sp, **kw)
    assert all(np.array_equal(shared[k], per[k]) for k in shared)
    dur, level = _handle(P, B).retime_plan(sp, **kw)
    assert dur.shape == (B, 1) and level.shape == (B, 1, P.N + 1)
    assert np.array_equal(dur[:, 0], shared["duration"][:, 0]) and np.array_equal(level[:, 0], shared["level"][:, 0])


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_calls_leave_the_handle_as_it_was(arrangements):
    """10. Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the retiming with a
    reserve on one of them only, between the other calls: solution(), stats(), the next advance() and the ticks (the later ones
    replayed from the captured graph) are bitwise equal."""
    B = 3
    (H, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = Q.shifted(H.problem)
    sp = np.array(Q.SLIDE_SPEEDS)
    dirs = V.tray3(H.problem)
    probe = lambda: (H.retime_plan(sp, want_reach=True, want_edges=True, want_iters=True, reserve=0.25, dirs=dirs),   # noqa: E731
                     H.retime_plan(sp, scen, common=True, end=0.0, reserve=0.5, dirs=dirs[2:], frame="world"),
                     H.retime_plan(sp[1:], scen, start=1.0, boxes=False, want_edges=True, reserve=0.0, dirs=dirs[:1]))
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
    """11. reserve -1, inf, NaN; n_dir 0, 33, -1, dirs NULL, a NaN entry, a zero row; frame 2, -1; their order among themselves and after
    the two retime refusals, a bad mass first; both outputs NULL -- through ctypes so that nothing in Python refuses first: the message,
    the output buffers untouched, the handle answers as before."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    S = Q.slide_case(arrangements)
    P = S["P"]
    h = BatchMPC(P, 2)
    h.set_guess(S["xs"], np.zeros((2, P.N, P.nu)))
    scen = np.ascontiguousarray(Q.shifted(P))
    good = np.array(Q.SLIDE_SPEEDS)
    gd = np.ascontiguousarray(V.tray3(P))
    before = h.retime_plan(good, scen, want_reach=True, want_edges=True, want_iters=True, reserve=0.25, dirs=gd)
    POISON = -7
    room = 2 * 2 * (P.N + 1) * 40
    bufs = dict(duration=np.full(room, float(POISON)), level=np.full(room, POISON, dtype=np.int32), reach=np.full(room, POISON, dtype=np.int32),
                edges=np.full(room, 7, dtype=np.uint32), iters=np.full(room, POISON, dtype=np.int32))
    lib = h._lib
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))   # noqa: E731

    def call(speeds=good, M=6, start=-1, end=-1, n_dir=3, dirs=gd, frame=1, reserve=0.25, params=scen, duration=bufs["duration"], level=bufs["level"]):
        speeds = np.ascontiguousarray(speeds, dtype=np.float64)
        dirs = None if dirs is None else np.ascontiguousarray(dirs, dtype=np.float64)
        return lib.upr_batch_retime_plan_reserve(h._h, 2, ptr(params), 0, M, ptr(speeds), start, end, 0, 1, n_dir, ptr(dirs), frame, C.c_double(reserve),
                                                 ptr(duration), iptr(level), iptr(bufs["reach"]), up(bufs["edges"]), iptr(bufs["iters"]))
    m_rsv = b"retime: reserve must be finite and >= 0"
    m_dirs = b"retime: dirs must be 1 .. 32 finite non-zero directions"
    m_frame = b"retime: frame must be 0 (world) or 1 (tray)"
    m_lattice = b"retime: speeds must be 1 .. 32 finite values >= 0 in strictly increasing order"
    m_levels = b"retime: start and end must be -1 or a level index"
    for r in (-1.0, np.inf, np.nan):
        assert call(reserve=r) != 0 and m_rsv in lib.upr_last_error(), (r, lib.upr_last_error())
    nan_entry, zero_row = gd.copy(), gd.copy()
    nan_entry[1, 4] = np.nan
    zero_row[2] = 0.0
    for kw in (dict(n_dir=0), dict(n_dir=33, dirs=np.repeat(gd[:1], 33, axis=0)), dict(n_dir=-1), dict(dirs=None), dict(dirs=nan_entry), dict(dirs=zero_row)):
        assert call(**kw) != 0 and m_dirs in lib.upr_last_error(), (kw, lib.upr_last_error())
    for f in (2, -1):
        assert call(frame=f) != 0 and m_frame in lib.upr_last_error(), (f, lib.upr_last_error())
    # the order: reserve before dirs before frame; the two retime refusals before all three; a bad mass before everything
    assert call(reserve=-1.0, n_dir=0, frame=2) != 0 and m_rsv in lib.upr_last_error()
    assert call(n_dir=0, frame=2) != 0 and m_dirs in lib.upr_last_error()
    assert call(start=6, reserve=-1.0, n_dir=0, frame=2) != 0 and m_levels in lib.upr_last_error()
    assert call(speeds=[1.0, 0.5], M=2, start=6, reserve=-1.0, dirs=None, frame=2) != 0 and m_lattice in lib.upr_last_error()
    heavy = scen.copy(); heavy[0, 0, 0] = -1.0
    assert call(M=0, reserve=np.nan, dirs=None, frame=2, params=heavy) != 0 and b"positive finite mass" in lib.upr_last_error()
    assert call(duration=None, level=None, reserve=-1.0) != 0
    assert b"upr_batch_retime_plan_reserve: duration and level must not both be NULL" in lib.upr_last_error()
    assert all(np.all(v == v.dtype.type(7 if k == "edges" else POISON)) for k, v in bufs.items())
    with pytest.raises(RuntimeError, match="reserve must be finite"):
        h.retime_plan(good, scen, reserve=-0.5, dirs=gd)
    with pytest.raises(RuntimeError, match="finite non-zero directions"):
        h.retime_plan(good, scen, reserve=0.5)
    with pytest.raises(ValueError, match="frame"):
        h.retime_plan(good, scen, reserve=0.5, dirs=gd, frame="body")
    # NULL outputs are not copied: duration alone, level alone
    assert call(level=None) == 0 and np.all(bufs["level"] == POISON) and np.array_equal(bufs["duration"][:4].reshape(2, 2), before[0])
    bufs["duration"][:] = POISON
    assert call(duration=None) == 0 and np.all(bufs["duration"] == POISON) and np.array_equal(bufs["level"][:before[1].size].reshape(before[1].shape), before[1])
    after = h.retime_plan(good, scen, want_reach=True, want_edges=True, want_iters=True, reserve=0.25, dirs=gd)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    h.close()
