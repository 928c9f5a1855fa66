"""The batched disturbance margin on the MI355X (upr_batch_disturbance_margin_points / _plan, upright_amd/csrc/upr_disturb.h): the
assertions of tests/test_disturbance_margin.py on the same table (tests/disturb_ref.py) with the device's answers, the device against the
host emulation of the same source in both forms, the path-acceleration margin as the special case u = (omega, v_ee), tray against world
frame, the symmetry under u -> -u, consistency with balance_check at r = 0 and at displaced states, the plan form against the points
form with its reductions, the absence of side effects on the handle, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import balance_ref as R
import disturb_ref as D
import pathacc_ref as A
from oracle.oracle import Oracle
from upright_amd._capi import iptr, ptr
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

_DEVICE = {}


def _reach(h, L, **kw):
    kw = dict(dict(dirs=L["dirs"], r_max=L["r_max"], frame=L["frame"]), **kw)
    r, out, z, y, it = h.disturbance_margin(L["x"], L["params"], want_out=True, want_z=True, want_y=True, want_iters=True, **kw)
    reach = np.empty(r.shape[:3] + (4,))
    reach[..., 0::2], reach[..., 1::2] = r, out
    return dict(reach=reach, z=z, y=y, iters=it)


def _device(arrangements, name):
    """The launches of the table (reference classes and emulation: D.cases) run once on the device: key "dev"."""
    if name not in _DEVICE:
        launches = D.cases(arrangements, name)
        h = BatchMPC(launches[0]["P"], 1)
        for L in launches:
            L["dev"] = _reach(h, L)
        assert h.balance_ms() > 0.0
        h.close()
        _DEVICE[name] = launches
    return _DEVICE[name]


def _against_emulation(launches, key, emu_of):
    """Same class everywhere; iters and reach bit-equal on the steady jobs; the largest difference of a finite end on the others."""
    w = 0.0
    for L in launches:
        d, e = L[key], emu_of(L)
        assert np.array_equal(D.classes_of(d, L["r_max"]), D.classes_of(e, L["r_max"]))
        m = D.steady(L)
        assert np.array_equal(d["iters"][m], e["iters"][m]) and np.array_equal(d["reach"][m], e["reach"][m])
        fin = np.isfinite(d["reach"]) & np.isfinite(e["reach"])
        w = max(w, float(np.abs(d["reach"][fin] - e["reach"][fin]).max()))
    return w


def _close(a, b, tol):
    """the infinities in the same places with the same signs, the finite ends within tol"""
    fin = np.isfinite(a)
    return np.array_equal(fin, np.isfinite(b)) and np.array_equal(a[~fin], b[~fin]) and (not fin.any() or np.abs(a[fin] - b[fin]).max() <= tol)


@pytest.mark.parametrize("name", D.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """pathacc_ref.check_answer on the device's answer to every launch and every direction block (class equal to the reference's on all
    jobs, bracket exact, both certificates on the oracle's b and A within EPS +- RHO_TOL); the device against the emulation (the lane
    form on the one-body shapes, the wave form on the others); the known answers to 1e-6 relative, at least five ends."""
    launches = _device(arrangements, name)
    for k, L in enumerate(launches):
        bad = D.check_launch(L, L["dev"])
        assert not bad, (name, k, bad[:5])
    w = _against_emulation(launches, "dev", lambda L: L["emu"])
    print("disturbance margin, %s: device vs emulation, largest difference of an end %.2e" % (name, w))
    n = 0
    for k in (0, 4, 5):
        L = launches[k]
        ka = D.known_answers(L, L["dev"]["reach"], name)
        print("disturbance margin on the device, %s, launch %d: largest relative |r - r_known| vertical %.2e, slide %.2e, comp %.2e (%d ends)"
              % (name, k, ka["vertical"], ka["slide"], ka["comp"], ka["n"]))
        assert ka["vertical"] <= 1e-6 and ka["slide"] <= 1e-6 and ka["comp"] <= 1e-6
        n += ka["n"]
    assert n >= 5


@pytest.mark.parametrize("name", D.ONE_BODY)
def test_one_body_arrangements_on_the_wave_form(arrangements, name, monkeypatch):
    """UPR_BAL_FORM=0 sends one-body arrangements through the wave-per-job kernel: the same checks on the same jobs, against the
    emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    launches = D.cases(arrangements, name)
    h = BatchMPC(launches[0]["P"], 1)
    outs = []
    for k, L in enumerate(launches):
        out = _reach(h, L)
        bad = D.check_launch(L, out)
        assert not bad, (name, k, bad[:5])
        outs.append(dict(L, wave=out))
    h.close()
    _against_emulation(outs, "wave", lambda L: D.run_launch(L, form=0))


@pytest.mark.parametrize("name", ["pink_bottle", "foam_die2"])
def test_equals_the_path_acceleration_margin(arrangements, name):
    """n = 1, frame = world, dirs = [(omega, v_ee)] of the oracle, r_max = d_max against path_accel_margin(speed=1) on states of
    pathacc's table of every class: equal class, ends within two grid steps (the two transforms may contract differently, by one ulp
    of b: a threshold crossing moves by ~1e-16 / |b_u| against a grid step of 3.7e-9)."""
    L = A.cases(arrangements, name)[0]
    rows = []
    for c in A.CLASSES:
        rows += [(int(i), int(sc)) for i, sc in np.argwhere((L["pclass"] == c) & L["jobs"].moving[:, None])[:2]]
    assert len(rows) >= 8 and len({L["pclass"][i, sc] for i, sc in rows}) >= 6
    P, dm = L["P"], L["d_max"]
    O = Oracle(P)
    h = BatchMPC(P, 1)
    for i, sc in rows:
        _, v, om, _, _ = D.ee_of(O, L["x"][i])
        x, th = L["x"][i:i + 1], L["params"][sc:sc + 1]
        r, rout = h.disturbance_margin(x, th, np.concatenate([om, v])[None], r_max=dm, frame="world", want_out=True)
        d, dout = h.path_accel_margin(x, th, d_max=dm, speed=1.0, want_out=True)
        got, want = np.concatenate([r[0, 0, 0], rout[0, 0, 0]]), np.concatenate([d[0, 0], dout[0, 0]])
        assert _close(got, want, 2.0 * D.step(dm)), (name, i, sc, got, want)
    h.close()


@pytest.mark.parametrize("name", ["pink_bottle", "blue_cups"])
def test_tray_against_world_and_symmetry(arrangements, name):
    """Tray-frame dirs against the same directions rotated in numpy and passed as world, point by point: equal class, ends within two
    grid steps.  dirs (u, -u) in one call: r_lo(-u) = -r_hi(u) and r_hi(-u) = -r_lo(u), == on steady jobs and within two grid steps
    elsewhere; swapping the direction order permutes the blocks bit for bit."""
    L = _device(arrangements, name)[0]
    P, dirs, rm = L["P"], L["dirs"], L["r_max"]
    tol = 2.0 * D.step(rm)
    uw = D.world_dirs(P, L["x"], dirs)
    h = BatchMPC(P, 1)
    for i in range(len(L["x"])):
        r, rout = h.disturbance_margin(L["x"][i:i + 1], L["params"], uw[i], r_max=rm, frame="world", want_out=True)
        got = np.empty(r.shape[:3] + (4,))
        got[..., 0::2], got[..., 1::2] = r, rout
        assert np.array_equal(A.device_class(got[:, 0], rm), A.device_class(L["dev"]["reach"][:, i], rm))
        assert _close(got[:, 0], L["dev"]["reach"][:, i], tol), (name, i)
    nd = len(dirs)
    both = _reach(h, L, dirs=np.concatenate([dirs, -dirs]))
    assert all(np.array_equal(both[k][:nd], L["dev"][k]) for k in both)
    mirror = -both["reach"][nd:][..., [2, 3, 0, 1]]
    m = D.steady(L)
    assert m.sum() >= 5 and np.array_equal(mirror[m], both["reach"][:nd][m])
    assert _close(mirror, both["reach"][:nd], tol)
    perm = np.arange(nd)[::-1]
    swapped = _reach(h, L, dirs=dirs[perm])
    assert all(np.array_equal(swapped[k], L["dev"][k][perm]) for k in swapped)
    h.close()


@pytest.mark.parametrize("name", D.NAMES)
def test_zero_inside_iff_balanced(arrangements, name):
    """0 in [r_lo, r_hi] in every direction iff balance_check calls the state balanced (rho <= 1e-8 max(|b|, 1)), on every job of the
    first launch whose decision at r = 0 lies 1e-9 max(|b|, 1) away from the boundary on the reference."""
    L = _device(arrangements, name)[0]
    h = BatchMPC(L["P"], 1)
    rho = h.balance_check(L["x"], L["params"])
    h.close()
    J = D.blocks_of(L)[0]["jobs"]
    reach = L["dev"]["reach"]
    n = 0
    for i in range(J.n):
        for sc in range(J.ns):
            if J.near(i, sc, 0.0) <= D.RHO_TOL:
                continue
            balanced = rho[i, sc] <= D.EPS * max(J.ref(i, sc, 0.0)["bnorm"], 1.0)
            inside = (reach[:, i, sc, 0] <= 0.0) & (0.0 <= reach[:, i, sc, 2])
            assert np.all(inside == balanced), (name, i, sc, reach[:, i, sc], rho[i, sc])
            n += 1
    assert n >= 25


@pytest.mark.parametrize("name", ["pink_bottle", "box_arch"])
def test_displaced_states(arrangements, name):
    """The state displaced to 0.999 r_hi is accepted by balance_check and the one displaced to 1.001 r_hi_out is rejected, where
    rho_ref is decided there (1e-9 max(|b|, 1) away from the boundary), on the jobs of the first launch with a bisected upper end
    r_hi > 0 whose lower end lies below 0.999 r_hi (for r_hi < 0 the factor 0.999 moves outwards, not inwards): at least 20 jobs."""
    L = _device(arrangements, name)[0]
    P = L["P"]
    uw = D.world_dirs(P, L["x"], L["dirs"])
    reach = L["dev"]["reach"]
    xs, th, want = [], [], []
    for d, blk in enumerate(D.blocks_of(L)):
        J = blk["jobs"]
        for i in range(J.n):
            for sc in range(J.ns):
                lo, _, hi, hi_out = reach[d, i, sc]
                if not (np.isfinite(hi_out) and hi > 0.0 and lo <= 0.999 * hi) or len(xs) >= 60:
                    continue
                for r, ok in ((0.999 * hi, True), (1.001 * hi_out, False)):
                    if J.near(i, sc, r) > D.RHO_TOL:
                        xs.append(D.displaced(P, L["x"][i], uw[i, d], r)); th.append(L["params"][sc:sc + 1]); want.append(ok)
    assert len(xs) >= 20 and any(want) and not all(want)
    h = BatchMPC(P, 1)
    rho, z = h.balance_check(np.stack(xs), np.stack(th), want_z=True)
    h.close()
    for k, (x, t, ok) in enumerate(zip(xs, th, want)):
        bn = np.linalg.norm(R.system(P, t[0], x)[0])
        assert (rho[k, 0] <= D.EPS * max(bn, 1.0)) == ok, (name, k, rho[k, 0], bn, ok)


def _plan_case(arrangements):
    """P, xs (3, N + 1, 3 nq) out of the states of the table, dirs with a repeated direction, scenarios.  Instance 0: states that are
    balanced under the nominal scenario; instance 1: the same with one knot that is not -- a level tray accelerating by 1.3 mu0 g0
    along span_0, which every direction of dirs can still balance (span_0 by braking, e_z and the tilted one by pressing); instance 2:
    with a falling knot, which accepts nothing along span_0."""
    launches = D.cases(arrangements, "pink_bottle")
    L = launches[0]
    P = L["P"]
    kinds = L["kinds"]
    good = [i for i, k in enumerate(kinds) if k in ("rest", "slide1.0", "lift", "inside")]
    N = P.N
    xs = np.stack([np.stack([L["x"][good[(k + b) % len(good)]] for k in range(N + 1)]) for b in range(3)])
    O = Oracle(P)
    q = L["x"][kinds.index("rest")][:P.nq]
    Cm = D.ee_of(O, np.concatenate([q, np.zeros(2 * P.nq)]))[0]
    push = 1.3 * float(P.contact_mu[0]) * R.G0 * (Cm @ L["dirs"][0, 3:])
    xs[1, 7] = R.state_for(O, q, np.zeros(P.nq), push, np.zeros(3))
    xs[2, 11] = L["x"][kinds.index("falling")]
    dirs = L["dirs"][[0, 2, 0, 3]]                                             # (direction 2 repeats direction 0)
    return P, xs, dirs, np.asarray(L["params"])


def test_plan_form(arrangements):
    """B = 3, N = 20, plans installed with set_guess.  disturbance_margin_plan equals the points form on the downloaded knots, ==, with
    shared scenarios, scenarios per instance and params=None; window / knot equal numpy's max / min / first argmax per direction;
    radius / binding equal numpy with the stated tie order -- a plan with an unbalanced knot (radius < 0), one with a knot that accepts
    nothing (-inf), ties from a repeated direction; radius >= 0 iff balance_check_plan accepts every knot, on decided knots; n_dir = 1
    and 32."""
    P, xs, dirs, scen = _plan_case(arrangements)
    B, N = 3, P.N
    h = BatchMPC(P, B)
    h.set_guess(xs, np.zeros((B, N, P.nu)))
    pts = xs.reshape(B * (N + 1), -1)
    per = np.stack([scen[[b % 4, (b + 1) % 4]] for b in range(B)])
    own = np.repeat(np.asarray(P.body_params, dtype=np.float64)[None, None], B * (N + 1), axis=0).reshape(B * (N + 1), 1, P.nb, 10)
    layouts = ((scen, scen), (per, np.repeat(per[:, None], N + 1, axis=1).reshape(B * (N + 1), 2, P.nb, 10)), (None, own))
    nd = len(dirs)
    for plan_params, point_params in layouts:
        got = h.disturbance_margin_plan(dirs, plan_params, want_out=True, want_iters=True)
        assert h.balance_ms() > 0.0
        want = h.disturbance_margin(pts, point_params, dirs, want_out=True, want_iters=True)
        ns = got[0].shape[3]
        assert got[0].shape == (nd, B, N + 1, ns, 2) and not np.any(np.isnan(got[0]))
        assert all(np.array_equal(g.reshape(w.shape), w) for g, w in zip(got, want))
        w, kn, rad, bind = h.disturbance_margin_plan(dirs, plan_params, window=True, radius=True)
        reach = np.empty((nd, B, N + 1, ns, 4))
        reach[..., 0::2], reach[..., 1::2] = got[0], got[1]
        w0, kn0, rad0, bind0 = D.numpy_plan(reach)
        assert np.array_equal(w, w0) and np.array_equal(kn, kn0) and np.array_equal(rad, rad0) and np.array_equal(bind, bind0)
        assert not np.any(np.isnan(w)) and not np.any(np.isnan(rad))
        w1, kn1 = h.disturbance_margin_plan(dirs, plan_params, window=True)
        rad1, bind1 = h.disturbance_margin_plan(dirs, plan_params, radius=True)
        assert np.array_equal(w1, w) and np.array_equal(kn1, kn) and np.array_equal(rad1, rad) and np.array_equal(bind1, bind)
        assert not np.any(bind[..., 0] == 2)                                       # (the repeated direction never binds: the first end wins)
        if plan_params is scen:
            assert rad[0, 0] > 0.0 and -np.inf < rad[1, 0] < 0.0 and rad[2, 0] == -np.inf
            assert bind[1, 0, 2] == 7 and bind[2, 0, 2] == 11
        # radius >= 0 iff every knot is balanced, on plans whose knots are all decided at r = 0 on the reference
        rho = h.balance_check_plan(plan_params)
        for b in range(B):
            for sc in range(ns):
                th = (scen[sc] if plan_params is scen else per[b, sc] if plan_params is per else np.asarray(P.body_params, dtype=np.float64))
                ref = R.reference(P, xs[b], th[None], False)
                s1 = np.maximum(ref["bnorm"][:, 0], 1.0)
                if np.any(np.abs(ref["rho"][:, 0] - D.EPS * s1) <= D.RHO_TOL * s1):
                    continue
                assert (rad[b, sc] >= 0.0) == bool(np.all(rho[b, :, sc] <= D.EPS * s1)), (b, sc, rad[b, sc])
    for dd in (dirs[2:3], np.concatenate([dirs] * 8)):
        r = h.disturbance_margin_plan(dd, scen[:1])
        rad, bind = h.disturbance_margin_plan(dd, scen[:1], radius=True)
        assert r.shape == (len(dd), B, N + 1, 1, 2) and not np.any(np.isnan(r))
        assert np.array_equal(rad, np.minimum(-r[..., 0].max(axis=2), r[..., 1].min(axis=2)).min(axis=0))
        assert np.array_equal(r, h.disturbance_margin(pts, scen[:1], dd).reshape(r.shape))
    h.close()


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_calls_leave_the_handle_as_it_was(arrangements):
    """Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the disturbance margin in
    both forms on one of them only, between the other calls: solution(), stats(), the next advance() and the ticks (the later ones
    replayed from the captured graph) are bitwise equal."""
    B = 3
    (H, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = R.scenarios(H.problem)
    dirs = D.tray_dirs(H.problem)
    probe = lambda: (H.disturbance_margin(x0, scen, dirs, want_out=True, want_z=True, want_y=True, want_iters=True),   # noqa: E731
                     H.disturbance_margin_plan(dirs), H.disturbance_margin_plan(dirs, scen, frame="world", want_iters=True),
                     H.disturbance_margin_plan(dirs, scen, window=True, radius=True))
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
    """The three refusals of the quantity through ctypes, on both entries and both forms: r_max in {0, -1, inf, NaN}; n_dir in {0, 33,
    -1}, dirs NULL, a NaN / inf entry, a zero row; frame = 2 -- in that order of precedence; a bad mass (an earlier refusal) wins over
    them; required pointers NULL; the output buffers are untouched; n <= 0 returns 0 and writes nothing; the handle answers as before."""
    if form:
        monkeypatch.setenv("UPR_BAL_FORM", form)
    P = R.table_problem(arrangements, "fixture_box")
    h = BatchMPC(P, 1)
    x = R.points(P, ["lift", "inside"], seed=1)
    scen = np.ascontiguousarray(R.scenarios(P))
    dirs = np.ascontiguousarray(np.tile(D.tray_dirs(P), (7, 1))[:33])
    before = h.disturbance_margin(x, scen, dirs[:5], want_out=True, want_z=True, want_y=True, want_iters=True)
    POISON = -7.0
    room = 33 * (P.N + 1) * 4 * 2 * 32
    bufs = dict(reach=np.full(room, POISON), z=np.full(room, POISON), y=np.full(room, POISON), iters=np.full(room, int(POISON), dtype=np.int32),
                window=np.full(room, POISON), knot=np.full(room, int(POISON), dtype=np.int32), radius=np.full(room, POISON),
                binding=np.full(room, int(POISON), dtype=np.int32))
    lib = h._lib

    def points(n_dir, dd, frame, r_max, params=scen, reach=bufs["reach"], n=2):
        return lib.upr_batch_disturbance_margin_points(h._h, n, ptr(x), 4, ptr(params), 0, n_dir, ptr(dd), frame, C.c_double(r_max), ptr(reach),
                                                       ptr(bufs["z"]), ptr(bufs["y"]), iptr(bufs["iters"]))

    def plan(n_dir, dd, frame, r_max, params=scen, reach=bufs["reach"], window=bufs["window"], radius=bufs["radius"]):
        return lib.upr_batch_disturbance_margin_plan(h._h, 4, ptr(params), 0, n_dir, ptr(dd), frame, C.c_double(r_max), ptr(reach), iptr(bufs["iters"]),
                                                     ptr(window), iptr(bufs["knot"]), ptr(radius), iptr(bufs["binding"]))

    def with_entry(k, v):
        d = dirs[:5].copy()
        d.flat[k] = v
        return d
    zero_row = dirs[:5].copy()
    zero_row[3] = 0.0
    m_r = b"disturbance margin: r_max must be finite and > 0"
    m_d = b"disturbance margin: dirs must be 1 .. 32 finite non-zero directions"
    m_f = b"disturbance margin: frame must be 0 (world) or 1 (tray)"
    bad = [((5, dirs, 1, r), m_r) for r in (0.0, -1.0, np.inf, np.nan)]
    bad += [((0, dirs, 2, np.nan), m_r), ((5, zero_row, 2, 0.0), m_r)]                     # (r_max before dirs and frame)
    bad += [((nd, dirs, 1, 8.0), m_d) for nd in (0, 33, -1)]
    bad += [((5, None, 1, 8.0), m_d), ((5, with_entry(7, np.nan), 0, 8.0), m_d), ((5, with_entry(29, np.inf), 1, 8.0), m_d), ((5, zero_row, 1, 8.0), m_d)]
    bad += [((5, zero_row, 2, 8.0), m_d)]                                                 # (dirs before frame)
    bad += [((5, dirs, 2, 8.0), m_f), ((5, dirs, -1, 8.0), m_f)]
    heavy = scen.copy()
    heavy[2, 0, 0] = -1.0
    for entry in (points, plan):
        for args, msg in bad:
            assert entry(*args) != 0 and msg in lib.upr_last_error(), (entry.__name__, args[0], args[2:], lib.upr_last_error())
            assert entry(*args, params=heavy) != 0 and b"positive finite mass" in lib.upr_last_error(), (entry.__name__, lib.upr_last_error())
    assert points(5, dirs, 1, 8.0, reach=None) != 0
    assert b"upr_batch_disturbance_margin_points: x, params and reach must not be NULL" in lib.upr_last_error()
    assert points(5, dirs, 1, 8.0, params=None) != 0
    assert b"upr_batch_disturbance_margin_points: x, params and reach must not be NULL" in lib.upr_last_error()
    assert plan(5, dirs, 1, 8.0, reach=None, window=None, radius=None) != 0
    assert b"upr_batch_disturbance_margin_plan: reach, window and radius must not all be NULL" in lib.upr_last_error()
    for n in (0, -3):
        assert points(5, dirs, 1, 8.0, n=n) == 0
    assert all(np.all(v == v.dtype.type(POISON)) for v in bufs.values())
    with pytest.raises(RuntimeError, match="r_max"):
        h.disturbance_margin(x, scen, dirs[:5], r_max=0.0)
    with pytest.raises(RuntimeError, match="dirs must be"):
        h.disturbance_margin_plan(dirs, scen)
    with pytest.raises(ValueError, match="frame"):
        h.disturbance_margin(x, scen, dirs[:5], frame="body")
    assert h.disturbance_margin(x, scen, dirs[:32]).shape == (32, 2, 4, 2) and h.disturbance_margin(x, scen, dirs[2]).shape == (1, 2, 4, 2)
    after = h.disturbance_margin(x, scen, dirs[:5], want_out=True, want_z=True, want_y=True, want_iters=True)
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    h.close()
