"""The batched speed margin on the MI355X (upr_batch_speed_margin_points / _plan, upright_amd/csrc/upr_speed.h): the assertions of
tests/test_speed_margin.py on the same table (tests/speed_ref.py) with the device's answers, the device against the host emulation of
the same source, both forms on the one-body shapes, the plan form against the points form with its reductions, the absence of side
effects on the handle, and the s_max refusals."""
import ctypes as C

import numpy as np
import pytest

import balance_ref as R
import speed_ref as S
from upright_amd._capi import iptr, ptr
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

_DEVICE = {}


def _speed(h, L, **kw):
    s, out, z, y, it = h.speed_margin(L["x"], L["params"], want_out=True, want_z=True, want_y=True, want_iters=True, **kw)
    speed = np.empty(s.shape[:2] + (4,))
    speed[..., 0::2], speed[..., 1::2] = s, out
    return dict(speed=speed, z=z, y=y, iters=it)


def _device(arrangements, name):
    """The launches of the table (reference classes and emulation: S.cases) run once on the device: key "dev"."""
    if name not in _DEVICE:
        launches = S.cases(arrangements, name)
        h = BatchMPC(launches[0]["P"], 1)
        for L in launches:
            L["dev"] = _speed(h, L)
        assert h.balance_ms() > 0.0
        h.close()
        _DEVICE[name] = launches
    return _DEVICE[name]


def _against_emulation(launches, key, emu_of):
    """Same class everywhere; same answer and iteration counts on the jobs that bisect no end; the largest difference of a finite end
    on the others."""
    w = 0.0
    for L in launches:
        d, e = L[key], emu_of(L)
        assert np.array_equal(S.device_class(d["speed"]), S.device_class(e["speed"]))
        m = S.steady(L)
        assert np.array_equal(d["iters"][m], e["iters"][m]) and np.array_equal(d["speed"][m], e["speed"][m])
        fin = np.isfinite(d["speed"]) & np.isfinite(e["speed"])
        w = max(w, float(np.abs(d["speed"][fin] - e["speed"][fin]).max()))
    return w


@pytest.mark.parametrize("name", S.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """S.check_answer on the device's answer to every launch of the table (conventions, bracket, both certificates at both ends on the
    oracle's b and A, rho_ref at every in and out, the reference's class); the device against the emulation; the known answers."""
    launches = _device(arrangements, name)
    for k, L in enumerate(launches):
        bad = S.check_answer(L, L["dev"])
        assert not bad, (name, k, bad[:5])
    w = _against_emulation(launches, "dev", lambda L: L["emu"])
    print("speed margin, %s: device vs emulation, largest difference of an end %.2e" % (name, w))
    L = launches[0]
    ka = S.known_answers(L, L["dev"]["speed"])
    print("speed margin on the device, %s: largest |s - s_known| facet %.2e, lift-off %.2e, window %.2e" % (name, ka["facet"], ka["liftoff"], ka["window"]))
    assert ka["liftoff"] <= 1e-6
    if name in S.SLIDING_BINDS:
        assert ka["facet"] <= 1e-6 and ka["window"] <= 1e-6


@pytest.mark.parametrize("name", S.ONE_BODY)
def test_one_body_arrangements_on_the_wave_form(arrangements, name, monkeypatch):
    """UPR_BAL_FORM=0 sends one-body arrangements through the wave-per-job kernel: the same checks on the same jobs, against the
    emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    launches = S.cases(arrangements, name)
    h = BatchMPC(launches[0]["P"], 1)
    outs = []
    for k, L in enumerate(launches):
        out = _speed(h, L)
        bad = S.check_answer(L, out)
        assert not bad, (name, k, bad[:5])
        outs.append(dict(L, wave=out))
    h.close()
    _against_emulation(outs, "wave", lambda L: S.run_emu(L["P"], L["x"], L["params"], L["per_point"], form=0))


@pytest.mark.parametrize("name", S.NAMES)
def test_monotone_sanity_on_upper_jobs(arrangements, name):
    """On every upper job of the first launch with s_hi >= 1e-3 (below that 1 % of s_hi moves rho by less than the rule's ball),
    balance_check at x_s: balanced at 0.99 s_hi, not balanced at 1.01 s_hi_out.  One call per side."""
    L = _device(arrangements, name)[0]
    P = L["P"]
    sp = L["dev"]["speed"]
    rows = np.argwhere(np.char.startswith(L["sclass"], "upper") & (sp[..., 2] >= 1e-3))
    assert len(rows) >= 5
    h = BatchMPC(P, 1)
    for factor, col, inside in ((0.99, 2, True), (1.01, 3, False)):
        x = np.stack([S.scaled_state(L["x"][i], factor * sp[i, sc, col], P.nq) for i, sc in rows])
        rho = h.balance_check(x, np.stack([L["params"][sc:sc + 1] for _, sc in rows]))
        assert np.all((rho[:, 0] <= 1e-8) == inside), (name, factor, rows[(rho[:, 0] <= 1e-8) != inside][:5])
    h.close()


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_plan_form(arrangements):
    """Headline handle, B = 12, N = 20, one cold solve: 252 jobs per scenario.  speed_margin_plan equals the points form on the
    downloaded plan, ==, with a shared scenario, scenarios per instance and params=None (every instance's own body_params); window and
    knot equal numpy's max / min / first argmax over the per-knot values exactly; limit equals numpy's to 1e-12 relative."""
    B = 12
    mpc, x0, bp = _headline(arrangements, B)
    P = mpc.problem
    N = P.N
    mpc.set_observation(0.0, x0)
    mpc.advance()
    _, xs, us = mpc.solution()
    pts = xs.reshape(B * (N + 1), P.nx)
    assert pts.shape[0] == 252
    scen = S.scenario_set(P)
    layouts = ((scen[1:2], scen[1:2]),
               (np.stack([R.scenarios(P, np.random.default_rng(b), 5)[4:5] for b in range(B)]), None),
               (None, np.repeat(bp[:, None, None], N + 1, axis=1).reshape(B * (N + 1), 1, P.nb, 10)))
    for plan_params, point_params in layouts:
        if point_params is None:
            point_params = np.repeat(plan_params[:, None], N + 1, axis=1).reshape(B * (N + 1), 1, P.nb, 10)
        got = mpc.speed_margin_plan(plan_params, want_out=True, want_iters=True)
        assert mpc.balance_ms() > 0.0
        want = mpc.speed_margin(pts, point_params, want_out=True, want_iters=True)
        assert got[0].shape == (B, N + 1, 1, 2) and not np.any(np.isnan(got[0]))
        assert all(np.array_equal(g.reshape(w.shape), w) for g, w in zip(got, want))
        w, kn, lim = mpc.speed_margin_plan(plan_params, window=True)
        speed = np.empty((B, N + 1, 1, 4))
        speed[..., 0::2], speed[..., 1::2] = got[0], got[1]
        w0, kn0, lim0 = S.numpy_plan(P, speed, xs, us)
        assert np.array_equal(w, w0) and np.array_equal(kn, kn0)
        assert np.all(np.isfinite(lim0)) and np.all(lim0 > 0)
        rel = np.abs(lim - lim0) / lim0
        print("speed margin, plan form: window lower %s upper %s; limit speed %.4f .. %.4f, device vs numpy %.2e relative"
              % (w[..., 0].max(), w[..., 1].min(), lim.min(), lim.max(), rel.max()))
        assert rel.max() <= 1e-12
    s4 = mpc.speed_margin_plan(scen, s_max=2.0)
    assert s4.shape == (B, N + 1, 4, 2) and not np.any(np.isnan(s4)) and np.all((s4[..., 1] <= 2.0) | np.isinf(s4[..., 1]))
    mpc.close()


def test_calls_leave_the_handle_as_it_was(arrangements):
    """Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the speed margin in
    both forms on one of them only, between the other calls: solution(), stats(), the next advance() and the ticks (the later ones
    replayed from the captured graph) are bitwise equal."""
    B = 3
    (A, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = R.scenarios(A.problem)
    probe = lambda: (A.speed_margin(x0, scen, want_out=True, want_z=True, want_y=True, want_iters=True), A.speed_margin_plan(),   # noqa: E731
                     A.speed_margin_plan(scen, want_iters=True), A.speed_margin_plan(scen, window=True))
    for h in (A, T):
        h.track_value_function()
        h.set_observation(0.0, x0)
    probe()
    for h in (A, T):
        h.advance()
    probe()
    for k, (u, v) in enumerate(zip(A.solution(), T.solution())):
        assert np.array_equal(u, v), k
    sa, st = A.stats(), T.stats()
    assert all(np.array_equal(sa[k], st[k]) for k in sa)
    Va, Vt = A.value_function(0.05, x0), T.value_function(0.05, x0)
    assert np.array_equal(Va[0], Vt[0]) and np.array_equal(Va[1], Vt[1])
    for h in (A, T):
        h.set_observation(0.1, x0)
        h.advance()
    for u, v in zip(A.solution(), T.solution()):
        assert np.array_equal(u, v)
    x = x0.copy()
    for k in range(5):
        xa, ua = A.tick(0.2 + 0.01 * k, x)
        xt, ut = T.tick(0.2 + 0.01 * k, x)
        assert np.array_equal(xa, xt) and np.array_equal(ua, ut), k
        if k >= 2:
            probe()
        x = xa
    assert A.tick_graph_replays() == T.tick_graph_replays() >= 1
    A.close(); T.close()


@pytest.mark.parametrize("form", ["", "0"])
def test_s_max_refusals(arrangements, form, monkeypatch):
    """s_max must be finite and > 1, through ctypes so that nothing in Python refuses first: the message; it wins over a NULL output
    and a bad n_scen (it stands beside kappa_max, first in the order of the checks); the output buffers are untouched; the handle
    answers as before."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    P = R.table_problem(arrangements, "fixture_box")
    h = BatchMPC(P, 1)
    x = R.points(P, ["lift", "inside"], seed=1)
    scen = np.ascontiguousarray(R.scenarios(P))
    before = h.speed_margin(x, scen, want_out=True, want_z=True, want_y=True, want_iters=True)
    POISON = -7.0
    room = (P.N + 1) * 4 * 2 * 32
    bufs = dict(speed=np.full(room, POISON), z=np.full(room, POISON), y=np.full(room, POISON), iters=np.full(room, int(POISON), dtype=np.int32),
                window=np.full(room, POISON), knot=np.full(room, int(POISON), dtype=np.int32), limit=np.full(room, POISON))
    msg = b"speed margin: s_max must be finite and > 1"
    lib = h._lib
    for s_max in (1.0, 0.5, 0.0, -2.0, np.inf, np.nan):
        for n_scen, speed in ((4, bufs["speed"]), (0, None)):
            rc = lib.upr_batch_speed_margin_points(h._h, 2, ptr(x), n_scen, ptr(scen), 0, C.c_double(s_max), ptr(speed), ptr(bufs["z"]), ptr(bufs["y"]),
                                                   iptr(bufs["iters"]))
            assert rc != 0 and msg in lib.upr_last_error(), (s_max, lib.upr_last_error())
            rc = lib.upr_batch_speed_margin_plan(h._h, n_scen, ptr(scen), 0, C.c_double(s_max), ptr(speed), iptr(bufs["iters"]), ptr(bufs["window"]),
                                                 iptr(bufs["knot"]), ptr(bufs["limit"]))
            assert rc != 0 and msg in lib.upr_last_error(), (s_max, lib.upr_last_error())
    assert all(np.all(v == v.dtype.type(POISON)) for v in bufs.values())
    with pytest.raises(RuntimeError, match="s_max"):
        h.speed_margin(x, scen, s_max=1.0)
    with pytest.raises(RuntimeError, match="s_max"):
        h.speed_margin_plan(scen, s_max=np.inf)
    # the family's other refusals reach the new entries through the same validation
    rc = lib.upr_batch_speed_margin_points(h._h, 2, ptr(x), 4, ptr(scen), 0, C.c_double(4.0), None, None, None, None)
    assert rc != 0 and b"upr_batch_speed_margin_points: x, params and speed must not be NULL" in lib.upr_last_error()
    rc = lib.upr_batch_speed_margin_plan(h._h, 4, ptr(scen), 0, C.c_double(4.0), None, None, None, None, None)
    assert rc != 0 and b"upr_batch_speed_margin_plan: speed and window must not both be NULL" in lib.upr_last_error()
    after = h.speed_margin(x, scen, want_out=True, want_z=True, want_y=True, want_iters=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    h.close()
