"""The batched path-acceleration margin on the MI355X (upr_batch_path_accel_margin_points / _plan, upright_amd/csrc/upr_pathacc.h): the
assertions of tests/test_path_accel_margin.py on the same table (tests/pathacc_ref.py) with the device's answers, the device against the
host emulation of the same source, both forms on the one-body shapes, consistency with balance_check and speed_margin, the plan form
against the points form with its reductions, the absence of side effects on the handle, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import balance_ref as R
import pathacc_ref as A
from upright_amd._capi import iptr, ptr
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

_DEVICE = {}


def _accel(h, L, **kw):
    kw = dict(dict(d_max=L["d_max"], speed=L["speed"]), **kw)
    d, out, z, y, it = h.path_accel_margin(L["x"], L["params"], want_out=True, want_z=True, want_y=True, want_iters=True, **kw)
    accel = np.empty(d.shape[:2] + (4,))
    accel[..., 0::2], accel[..., 1::2] = d, out
    return dict(accel=accel, z=z, y=y, iters=it)


def _device(arrangements, name):
    """The launches of the table (reference classes and emulation: A.cases) run once on the device: key "dev"."""
    if name not in _DEVICE:
        launches = A.cases(arrangements, name)
        h = BatchMPC(launches[0]["P"], 1)
        for L in launches:
            L["dev"] = _accel(h, L)
        assert h.balance_ms() > 0.0
        h.close()
        _DEVICE[name] = launches
    return _DEVICE[name]


def _against_emulation(launches, key, emu_of):
    """Same class everywhere; same answer and solve counts on the jobs that bisect no end and whose decisions lie 1e-9 max(|b|, 1) away
    from the boundary (A.steady); the largest difference of a finite end on the others."""
    w = 0.0
    for L in launches:
        d, e = L[key], emu_of(L)
        assert np.array_equal(A.device_class(d["accel"], L["d_max"]), A.device_class(e["accel"], L["d_max"]))
        m = A.steady(L)
        assert np.array_equal(d["iters"][m], e["iters"][m]) and np.array_equal(d["accel"][m], e["accel"][m])
        fin = np.isfinite(d["accel"]) & np.isfinite(e["accel"])
        w = max(w, float(np.abs(d["accel"][fin] - e["accel"][fin]).max()))
    return w


@pytest.mark.parametrize("name", A.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """A.check_answer on the device's answer to every launch of the table (conventions, bracket, both certificates at both ends on the
    oracle's b and A, rho_ref at every in and out, the reference's class); the device against the emulation; the known answers."""
    launches = _device(arrangements, name)
    for k, L in enumerate(launches):
        bad = A.check_answer(L, L["dev"])
        assert not bad, (name, k, bad[:5])
    w = _against_emulation(launches, "dev", lambda L: L["emu"])
    print("path-acceleration margin, %s: device vs emulation, largest difference of an end %.2e" % (name, w))
    for k in (0, 6):
        L = launches[k]
        ka = A.known_answers(L, L["dev"]["accel"], name)
        print("path-acceleration margin on the device, %s, launch %d: largest relative |d - d_known| vertical %.2e, slide %.2e, comp %.2e"
              % (name, k, ka["vertical"], ka["slide"], ka["comp"]))
        assert ka["n"] >= 5 or k == 6          # (d_max = 3 clips most of the closed-form ends of the slow launch)
        assert ka["vertical"] <= 1e-6 and ka["slide"] <= 1e-6 and ka["comp"] <= 1e-6


@pytest.mark.parametrize("name", A.NAMES)
def test_descent_seeded_windows(arrangements, name):
    """The windows only the descent search seeds (compensated tilt, friction shapes): the device agrees with the replay on rho_ref."""
    launches = _device(arrangements, name)
    if launches[0]["P"].nf != 3:
        return
    n = 0
    for L in launches[:4]:
        J = L["jobs"]
        for i, kind in enumerate(L["kinds"]):
            for sc in range(J.ns):
                if kind.startswith("comp") and L["pclass"][i, sc] == "window" and n < 8:
                    ac, _ = J.replay(i, sc)
                    assert np.abs(L["dev"]["accel"][i, sc] - ac).max() <= 1e-6 * np.abs(ac).max(), (name, i, sc, L["dev"]["accel"][i, sc], ac)
                    n += 1
    assert n >= 5


@pytest.mark.parametrize("name", A.ONE_BODY)
def test_one_body_arrangements_on_the_wave_form(arrangements, name, monkeypatch):
    """UPR_BAL_FORM=0 sends one-body arrangements through the wave-per-job kernel: the same checks on the same jobs, against the
    emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    launches = A.cases(arrangements, name)
    h = BatchMPC(launches[0]["P"], 1)
    outs = []
    for k, L in enumerate(launches):
        out = _accel(h, L)
        bad = A.check_answer(L, out)
        assert not bad, (name, k, bad[:5])
        outs.append(dict(L, wave=out))
    h.close()
    _against_emulation(outs, "wave", lambda L: A.run_launch(L, form=0))


@pytest.mark.parametrize("name", A.NAMES)
def test_zero_inside_iff_balanced(arrangements, name):
    """0 in [d_lo, d_hi] iff balance_check calls the state balanced (rho <= 1e-8 max(|b|, 1)), on every job of the first launch whose
    decision at d = 0 lies 1e-9 max(|b|, 1) away from the boundary on the reference."""
    L = _device(arrangements, name)[0]
    J = L["jobs"]
    h = BatchMPC(L["P"], 1)
    rho = h.balance_check(L["x"], L["params"])
    h.close()
    ac = L["dev"]["accel"]
    n = 0
    for i in range(J.n):
        for sc in range(J.ns):
            if J.near(i, sc, 0.0) <= A.RHO_TOL:
                continue
            r = J.ref(i, sc, 0.0)
            balanced = rho[i, sc] <= A.EPS * max(r["bnorm"], 1.0)
            assert (ac[i, sc, 0] <= 0.0 <= ac[i, sc, 2]) == balanced, (name, i, sc, ac[i, sc], rho[i, sc])
            n += 1
    assert n >= 200


@pytest.mark.parametrize("name", A.NAMES)
def test_consistent_with_the_speed_margin(arrangements, name):
    """On `upper` jobs of speed_margin (rest accepted, an upper end s_hi >= 1e-3 below s_max; the falling and rising states of the
    first launch are such: s_hi = sqrt(g0 / (g0 + k))): at speed = 0.99 s_hi the d-window contains 0, at speed = 1.01 s_hi_out it does
    not.  The class is read off the device's own speed answer; one call per job and side (the speed is one number per call): the
    first eight."""
    L = A.cases(arrangements, name)[0]
    h = BatchMPC(L["P"], 1)
    s, out = h.speed_margin(L["x"], L["params"], want_out=True)
    upper = (s[..., 0] == 0.0) & (out[..., 0] == 0.0) & np.isfinite(out[..., 1]) & (s[..., 1] >= 1e-3)
    rows = np.argwhere(upper)[:8]
    assert len(rows) >= 5
    for i, sc in rows:
        for speed, inside in ((0.99 * s[i, sc, 1], True), (1.01 * out[i, sc, 1], False)):
            d = h.path_accel_margin(L["x"][i:i + 1], L["params"][sc:sc + 1], speed=speed)[0, 0]
            assert (d[0] <= 0.0 <= d[1]) == inside, (name, i, sc, speed, d)
    h.close()


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_plan_form(arrangements):
    """Headline handle, B = 12, N = 20, one cold solve: 252 jobs per scenario.  path_accel_margin_plan equals the points form on the
    downloaded plan, ==, with a shared scenario, scenarios per instance and params=None (every instance's own body_params); window and
    knot equal numpy's max / min / first argmax over the per-knot values exactly; limit equals numpy's to 1e-12 relative; window=True
    alone downloads the reductions only."""
    B = 12
    mpc, x0, bp = _headline(arrangements, B)
    P = mpc.problem
    N = P.N
    mpc.set_observation(0.0, x0)
    mpc.advance()
    _, xs, us = mpc.solution()
    pts = xs.reshape(B * (N + 1), P.nx)
    assert pts.shape[0] == 252
    scen = A.scenario_set(P)
    layouts = ((scen[1:2], scen[1:2]),
               (np.stack([R.scenarios(P, np.random.default_rng(b), 5)[4:5] for b in range(B)]), None),
               (None, np.repeat(bp[:, None, None], N + 1, axis=1).reshape(B * (N + 1), 1, P.nb, 10)))
    for speed in (1.0, 0.7):
        for plan_params, point_params in layouts:
            if point_params is None:
                point_params = np.repeat(plan_params[:, None], N + 1, axis=1).reshape(B * (N + 1), 1, P.nb, 10)
            got = mpc.path_accel_margin_plan(plan_params, speed=speed, want_out=True, want_iters=True)
            assert mpc.balance_ms() > 0.0
            want = mpc.path_accel_margin(pts, point_params, speed=speed, want_out=True, want_iters=True)
            assert got[0].shape == (B, N + 1, 1, 2) and not np.any(np.isnan(got[0]))
            assert all(np.array_equal(g.reshape(w.shape), w) for g, w in zip(got, want))
            w, kn, lim = mpc.path_accel_margin_plan(plan_params, speed=speed, window=True)
            accel = np.empty((B, N + 1, 1, 4))
            accel[..., 0::2], accel[..., 1::2] = got[0], got[1]
            w0, kn0, lim0 = A.numpy_plan(P, accel, xs, speed)
            assert np.array_equal(w, w0) and np.array_equal(kn, kn0)
            assert lim.shape == (B, 2) and np.all(np.isfinite(lim0))
            rel = np.abs(lim - lim0) / np.abs(lim0)
            print("path-acceleration margin, plan form, speed %g: window lower %s upper %s; limit %.3f .. %.3f, device vs numpy %.2e relative"
                  % (speed, w[..., 0].max(), w[..., 1].min(), lim[:, 0].max(), lim[:, 1].min(), rel.max()))
            assert rel.max() <= 1e-12
    d4 = mpc.path_accel_margin_plan(scen, d_max=3.0)
    assert d4.shape == (B, N + 1, 4, 2) and not np.any(np.isnan(d4)) and np.all((np.abs(d4) <= 3.0) | np.isinf(d4))
    mpc.close()


def test_calls_leave_the_handle_as_it_was(arrangements):
    """Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the path-acceleration
    margin in both forms on one of them only, between the other calls: solution(), stats(), the next advance() and the ticks (the later
    ones replayed from the captured graph) are bitwise equal."""
    B = 3
    (H, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = R.scenarios(H.problem)
    probe = lambda: (H.path_accel_margin(x0, scen, want_out=True, want_z=True, want_y=True, want_iters=True), H.path_accel_margin_plan(),   # noqa: E731
                     H.path_accel_margin_plan(scen, speed=0.8, want_iters=True), H.path_accel_margin_plan(scen, window=True))
    for h in (H, T):
        h.track_value_function()
        h.set_observation(0.0, x0)
    probe()
    for h in (H, T):
        h.advance()
    probe()
    for k, (u, v) in enumerate(zip(H.solution(), T.solution())):
        assert np.array_equal(u, v), k
    sa, st = H.stats(), T.stats()
    assert all(np.array_equal(sa[k], st[k]) for k in sa)
    Va, Vt = H.value_function(0.05, x0), T.value_function(0.05, x0)
    assert np.array_equal(Va[0], Vt[0]) and np.array_equal(Va[1], Vt[1])
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
    """d_max must be finite and > 0, speed finite and >= 0, through ctypes so that nothing in Python refuses first: the message; it
    wins over a NULL output and a bad n_scen (it stands beside s_max's); the output buffers are untouched; n <= 0 returns 0 and writes
    nothing; the handle answers as before."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    P = R.table_problem(arrangements, "fixture_box")
    h = BatchMPC(P, 1)
    x = R.points(P, ["lift", "inside"], seed=1)
    scen = np.ascontiguousarray(R.scenarios(P))
    before = h.path_accel_margin(x, scen, want_out=True, want_z=True, want_y=True, want_iters=True)
    POISON = -7.0
    room = (P.N + 1) * 4 * 2 * 32
    bufs = dict(accel=np.full(room, POISON), z=np.full(room, POISON), y=np.full(room, POISON), iters=np.full(room, int(POISON), dtype=np.int32),
                window=np.full(room, POISON), knot=np.full(room, int(POISON), dtype=np.int32), limit=np.full(room, POISON))
    msg = b"path-acceleration margin: d_max must be finite and > 0, speed finite and >= 0"
    lib = h._lib
    bad = [(d, 1.0) for d in (0.0, -1.0, np.inf, np.nan)] + [(8.0, s) for s in (-1.0, np.inf, np.nan)]
    for d_max, speed in bad:
        for n_scen, accel in ((4, bufs["accel"]), (0, None)):
            rc = lib.upr_batch_path_accel_margin_points(h._h, 2, ptr(x), n_scen, ptr(scen), 0, C.c_double(d_max), C.c_double(speed), ptr(accel),
                                                        ptr(bufs["z"]), ptr(bufs["y"]), iptr(bufs["iters"]))
            assert rc != 0 and msg in lib.upr_last_error(), (d_max, speed, lib.upr_last_error())
            rc = lib.upr_batch_path_accel_margin_plan(h._h, n_scen, ptr(scen), 0, C.c_double(d_max), C.c_double(speed), ptr(accel), iptr(bufs["iters"]),
                                                      ptr(bufs["window"]), iptr(bufs["knot"]), ptr(bufs["limit"]))
            assert rc != 0 and msg in lib.upr_last_error(), (d_max, speed, lib.upr_last_error())
    for n in (0, -3):
        rc = lib.upr_batch_path_accel_margin_points(h._h, n, ptr(x), 4, ptr(scen), 0, C.c_double(8.0), C.c_double(1.0), ptr(bufs["accel"]), ptr(bufs["z"]),
                                                    ptr(bufs["y"]), iptr(bufs["iters"]))
        assert rc == 0
    assert all(np.all(v == v.dtype.type(POISON)) for v in bufs.values())
    with pytest.raises(RuntimeError, match="d_max"):
        h.path_accel_margin(x, scen, d_max=0.0)
    with pytest.raises(RuntimeError, match="speed finite"):
        h.path_accel_margin_plan(scen, speed=-1.0)
    # the family's other refusals reach the new entries through the same validation
    rc = lib.upr_batch_path_accel_margin_points(h._h, 2, ptr(x), 4, ptr(scen), 0, C.c_double(8.0), C.c_double(1.0), None, None, None, None)
    assert rc != 0 and b"upr_batch_path_accel_margin_points: x, params and accel must not be NULL" in lib.upr_last_error()
    rc = lib.upr_batch_path_accel_margin_plan(h._h, 4, ptr(scen), 0, C.c_double(8.0), C.c_double(1.0), None, None, None, None, None)
    assert rc != 0 and b"upr_batch_path_accel_margin_plan: accel and window must not both be NULL" in lib.upr_last_error()
    assert h.path_accel_margin(x, scen, speed=0.0).shape == (2, 4, 2)     # (speed = 0 is allowed: the state at rest on its path)
    after = h.path_accel_margin(x, scen, want_out=True, want_z=True, want_y=True, want_iters=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    h.close()
