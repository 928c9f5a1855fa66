"""The retiming of a plan on a speed lattice on the MI355X (upr_batch_retime_plan, upright_amd/csrc/upr_retime.h): the assertions of
tests/test_retime.py with the device's answers on the same plans (tests/retime_ref.py), installed with set_guess; the device against the
host emulation of the same source; both forms on the one-body shape and a multi-body arrangement; consistency with balance_check,
speed_margin_plan and path_accel_margin_plan; the layouts of params; the absence of side effects on the handle; the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import balance_ref as R
import retime_ref as Q
from upright_amd._capi import iptr, ptr
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

_HANDLES = {}


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


def run(P, xs, params, speeds, start=-1, end=-1, common=False, boxes=True, form=-1):
    speeds = np.asarray(speeds, dtype=np.float64)
    h = _handle(P, xs.shape[0])
    return Q.run_device(h, xs, params, speeds, None if start < 0 else speeds[start], None if end < 0 else speeds[end], common, boxes)


def test_closed_form_slide(arrangements):
    Q.body_closed_form(run, arrangements)


def test_reference_on_generic_plans(arrangements):
    out = Q.body_reference(run, arrangements)
    G = Q.generic_case(arrangements)
    assert _handle(G["P"], 3).balance_ms() > 0.0
    # 11. the device against the emulation: masks and iters on decided edges (rows), duration and level on decided plans
    emu = Q.run_emu(G["P"], G["xs"], G["params"], G["speeds"])
    dec = G["ref"]["decided"]
    bits = Q.decided_bits(dec)
    assert np.array_equal(out["edges"] & bits, emu["edges"] & bits)
    rows = dec.all(axis=-1)
    assert rows.sum() >= 100 and np.array_equal(out["iters"][rows], emu["iters"][rows])
    plans = dec.all(axis=(2, 3, 4))
    assert plans.any() and np.array_equal(out["duration"][plans], emu["duration"][plans]) and np.array_equal(out["level"][plans], emu["level"][plans])
    assert np.array_equal(out["reach"][plans], emu["reach"][plans])


def test_invariants_on_the_answer_alone(arrangements):
    Q.body_invariants(run, arrangements)


def test_retimed_states_are_balanced(arrangements):
    """4. BatchMPC.retimed_states of the device's laws through balance_check, and against numpy's states."""
    G = Q.generic_case(arrangements)
    P = G["P"]
    h = _handle(P, 3)
    Q.body_independent_path(run, arrangements, lambda P_, x, th: h.balance_check(x, th[None])[:, 0])
    out = run(P, G["xs"], G["params"], G["speeds"])
    t, dep, arr = h.retimed_states(out["level"], G["speeds"])
    t0, dep0, arr0 = Q.retimed_states(G["xs"], out["level"], G["speeds"], float(P.dt), P.nq)
    ok = np.isfinite(out["duration"])
    assert ok.any() and np.array_equal(t[ok], t0[ok]) and np.array_equal(dep[ok], dep0[ok]) and np.array_equal(arr[ok], arr0[ok])
    assert np.all(np.isnan(t[~ok]))
    one = run(P, G["xs"], G["params"], G["speeds"], common=True)
    t1, dep1, _ = h.retimed_states(one["level"], G["speeds"])
    assert t1.shape == (3, P.N + 1) and dep1.shape == (3, P.N, 3 * P.nq)
    fin = np.isfinite(one["duration"])
    assert np.allclose(t1[fin, -1], one["duration"][fin], rtol=1e-12, atol=0)


def test_one_level_against_the_speed_margin(arrangements):
    def speed4(P, xs, params):
        h = _handle(P, xs.shape[0])
        h.set_guess(xs, np.zeros((h.B, h.N, h.nu)))
        s, out = h.speed_margin_plan(params, want_out=True)
        sp = np.empty(s.shape[:3] + (4,))
        sp[..., 0::2], sp[..., 1::2] = s, out
        w, knot, _ = h.speed_margin_plan(params, window=True)
        assert np.array_equal(w[..., 1], sp[..., 2].min(axis=1))
        return sp
    Q.body_speed_margin(run, arrangements, speed4)


def test_admissible_edges_lie_in_the_path_accel_window(arrangements):
    def pathacc(P, xs, params, speed, d_max):
        h = _handle(P, xs.shape[0])
        h.set_guess(xs, np.zeros((h.B, h.N, h.nu)))
        return h.path_accel_margin_plan(params, d_max=d_max, speed=speed)
    Q.body_path_accel(run, arrangements, pathacc)


def test_common_time_law(arrangements):
    Q.body_common(run, arrangements)


def test_boxes(arrangements):
    Q.body_boxes(run, arrangements)


def test_edge_shapes(arrangements):
    Q.body_edge_shapes(run, arrangements)


def test_one_body_shape_on_the_wave_form(arrangements, monkeypatch):
    """10. UPR_BAL_FORM=0 sends the one-body shape through the wave-per-job kernel: test 2's assertions, the emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    out = Q.body_reference(run, arrangements)
    G = Q.generic_case(arrangements)
    emu = Q.run_emu(G["P"], G["xs"], G["params"], G["speeds"], form=0)
    bits = Q.decided_bits(G["ref"]["decided"])
    assert np.array_equal(out["edges"] & bits, emu["edges"] & bits)
    rows = G["ref"]["decided"].all(axis=-1)
    assert np.array_equal(out["iters"][rows], emu["iters"][rows])
    S = Q.slide_case(arrangements)
    assert np.array_equal(run(S["P"], S["xs"], S["params"], S["speeds"], boxes=False)["edges"], S["ref"]["masks"])


def test_multi_body_arrangement(arrangements):
    """10. foam_die2 (two bodies, eight contacts), B = 2, M = 3, and the device against the emulation."""
    out = Q.body_reference(run, arrangements, name="foam_die2", B=2, speeds=(0.5, 1.0, 1.5))
    G = Q.generic_case(arrangements, "foam_die2", 2, (0.5, 1.0, 1.5))
    emu = Q.run_emu(G["P"], G["xs"], G["params"], G["speeds"])
    bits = Q.decided_bits(G["ref"]["decided"])
    rows = G["ref"]["decided"].all(axis=-1)
    assert np.array_equal(out["edges"] & bits, emu["edges"] & bits) and np.array_equal(out["iters"][rows], emu["iters"][rows])
    assert np.array_equal(out["duration"], emu["duration"])


def test_layouts_of_params(arrangements):
    """Scenarios per instance (B, n_scen, nb, 10) and params=None (every instance's own body parameters) give what the shared layout
    gives for the same parameters; outputs that are not asked for are not returned."""
    G = Q.generic_case(arrangements)
    P, xs, sp = G["P"], G["xs"], G["speeds"]
    B = xs.shape[0]
    shared = run(P, xs, G["params"], sp)
    per = run(P, xs, np.repeat(G["params"][None], B, axis=0), sp)
    assert all(np.array_equal(shared[k], per[k]) for k in shared)
    h = _handle(P, B)
    dur, level = h.retime_plan(sp)
    assert dur.shape == (B, 1) and level.shape == (B, 1, P.N + 1)
    assert np.array_equal(dur[:, 0], shared["duration"][:, 0]) and np.array_equal(level[:, 0], shared["level"][:, 0])
    with pytest.raises(ValueError, match="lattice"):
        h.retime_plan(sp, end=0.6)


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_calls_leave_the_handle_as_it_was(arrangements):
    """12. Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the retiming on one of
    them only, between the other calls: solution(), stats(), the next advance() and the ticks (the later ones replayed from the
    captured graph) are bitwise equal."""
    B = 3
    (H, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = Q.shifted(H.problem)
    sp = np.array(Q.SLIDE_SPEEDS)
    probe = lambda: (H.retime_plan(sp, want_reach=True, want_edges=True, want_iters=True), H.retime_plan(sp, scen, common=True, end=0.0),   # noqa: E731
                     H.retime_plan(sp[1:], scen, start=1.0, boxes=False, want_edges=True))
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
    Va, Vt = H.value_function(0.05, x0), T.value_function(0.05, x0)
    assert np.array_equal(Va[0], Vt[0]) and np.array_equal(Va[1], Vt[1])
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
    """13. M = 0 and M = 33, a negative, non-finite or repeated speed, a descending lattice, start or end out of range, both outputs
    NULL, through ctypes so that nothing in Python refuses first: the message, the output buffers untouched, the handle answers as
    before."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    S = Q.slide_case(arrangements)
    P = S["P"]
    h = BatchMPC(P, 2)
    h.set_guess(S["xs"], np.zeros((2, P.N, P.nu)))
    scen = np.ascontiguousarray(Q.shifted(P))
    good = np.array(Q.SLIDE_SPEEDS)
    before = h.retime_plan(good, scen, want_reach=True, want_edges=True, want_iters=True)
    POISON = -7
    room = 2 * 2 * (P.N + 1) * 40
    bufs = dict(duration=np.full(room, float(POISON)), level=np.full(room, POISON, dtype=np.int32), reach=np.full(room, POISON, dtype=np.int32),
                edges=np.full(room, 7, dtype=np.uint32), iters=np.full(room, POISON, dtype=np.int32))
    lib = h._lib
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint))   # noqa: E731

    def call(speeds, M, start=-1, end=-1, duration=bufs["duration"], level=bufs["level"]):
        speeds = np.ascontiguousarray(speeds, dtype=np.float64)
        return lib.upr_batch_retime_plan(h._h, 2, ptr(scen), 0, M, ptr(speeds), start, end, 0, 1, ptr(duration), iptr(level), iptr(bufs["reach"]),
                                         up(bufs["edges"]), iptr(bufs["iters"]))
    lattice = b"retime: speeds must be 1 .. 32 finite values >= 0 in strictly increasing order"
    big = np.linspace(0.1, 1.0, 33)
    bad = [(good, 0), (big, 33), (good, -1), ([-0.5, 1.0], 2), ([0.5, np.inf], 2), ([0.5, np.nan], 2), ([0.5, 0.5, 1.0], 3), ([1.0, 0.5], 2)]
    for speeds, M in bad:
        assert call(speeds, M) != 0 and lattice in lib.upr_last_error(), (speeds, M, lib.upr_last_error())
    levels = b"retime: start and end must be -1 or a level index"
    for start, end in ((6, -1), (-2, -1), (-1, 6), (-1, -2), (100, 0)):
        assert call(good, 6, start, end) != 0 and levels in lib.upr_last_error(), (start, end, lib.upr_last_error())
    assert call(good, 6, duration=None, level=None) != 0
    assert b"upr_batch_retime_plan: duration and level must not both be NULL" in lib.upr_last_error()
    # (the family's earlier refusals keep their precedence: a bad mass wins over a bad lattice)
    heavy = scen.copy(); heavy[0, 0, 0] = -1.0
    rc = lib.upr_batch_retime_plan(h._h, 2, ptr(heavy), 0, 0, ptr(good), -1, -1, 0, 1, ptr(bufs["duration"]), iptr(bufs["level"]), None, None, None)
    assert rc != 0 and b"positive finite mass" in lib.upr_last_error()
    assert all(np.all(v == v.dtype.type(7 if k == "edges" else POISON)) for k, v in bufs.items())
    with pytest.raises(RuntimeError, match="strictly increasing"):
        h.retime_plan([1.0, 0.5], scen)
    # NULL outputs are not copied: duration alone, level alone
    assert call(good, 6, level=None) == 0 and np.all(bufs["level"] == POISON) and np.array_equal(bufs["duration"][:4].reshape(2, 2), before[0])
    bufs["duration"][:] = POISON
    assert call(good, 6, duration=None) == 0 and np.all(bufs["duration"] == POISON) and np.array_equal(bufs["level"][:before[1].size].reshape(before[1].shape), before[1])
    after = h.retime_plan(good, scen, want_reach=True, want_edges=True, want_iters=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    h.close()
