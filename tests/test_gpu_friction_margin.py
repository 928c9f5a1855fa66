"""The batched friction margin on the MI355X (upr_batch_friction_margin_points / _plan, upright_amd/csrc/upr_margin.h) and the
balance check with a friction scale (upr_batch_balance_points_mu / _plan_mu): the assertions of tests/test_friction_margin.py on
the same table (tests/margin_ref.py) with the device's answers, the device against the host emulation of the same source, the plan
form against the points form, the absence of side effects on the handle, and one large launch."""
import numpy as np
import pytest

import balance_ref as R
import margin_ref as M
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

_DEVICE = {}
KEYS = ("kappa_hi", "kappa_lo", "z", "y", "iters")


def _margin(h, L, **kw):
    return dict(zip(KEYS, h.friction_margin(L["x"], L["params"], want_lo=True, want_z=True, want_y=True, want_iters=True, **kw)))


def _device(arrangements, name):
    """The launches of the table (reference classes and emulation: M.cases) run once on the device: key "dev"."""
    if name not in _DEVICE:
        launches = M.cases(arrangements, name)
        h = BatchMPC(launches[0]["P"], 1)
        for L in launches:
            L["dev"] = _margin(h, L)
        assert h.balance_ms() > 0.0
        h.close()
        _DEVICE[name] = launches
    return _DEVICE[name]


@pytest.mark.parametrize("name", M.NAMES)
def test_bracket_certificates_and_reference(arrangements, name):
    """Checks 1 - 4 and the cap on every job of the table, on the device's kappa_hi, kappa_lo, z, y, iters (M.check_answer: the
    bracket exactly, both certificates on the oracle's b and A without a solver, rho_ref at both ends, the reference's class).
    Prints the largest |kappa - kappa_ref| against full CPU bisections and against the emulation (DESIGN 3.8 records them)."""
    launches = _device(arrangements, name)
    for k, L in enumerate(launches):
        bad = M.check_answer(L, L["dev"])
        assert not bad, (name, k, bad[:5])
    bs = M.reference_bisections(launches)
    w_ref = max([abs(launches[k]["dev"]["kappa_hi"][i, s] - hi) for k, i, s, hi, _ in bs] or [0.0])
    fin = [np.isfinite(L["dev"]["kappa_hi"]) & np.isfinite(L["emu"]["kappa_hi"]) for L in launches]
    w_emu = max(float(np.abs(L["dev"]["kappa_hi"][f] - L["emu"]["kappa_hi"][f]).max()) if f.any() else 0.0 for L, f in zip(launches, fin))
    print("friction margin, %s: %d finite jobs, largest |kappa - kappa_ref| device vs reference %.2e, device vs emulation %.2e" % (name, len(bs), w_ref, w_emu))


@pytest.mark.parametrize("name", M.NAMES)
def test_device_against_the_emulation(arrangements, name):
    """The same source on the device and on the host: the same class on every job, and the same iteration count on every job whose
    decisions all keep 1e-9 max(|b|, 1) away from the boundary on the reference (M.near_masks; the others, at most 5 % of the
    arrangement's jobs, end their bisection on the boundary, where a decision may hang on the last bits of rho); zero-class jobs
    take one evaluation: the count of the rho call at kappa = 0."""
    launches = _device(arrangements, name)
    masks = M.near_masks(launches)
    share = sum(int(m.sum()) for m in masks) / float(sum(m.size for m in masks))
    print("friction margin, %s: iteration counts not compared on %.2f %% of the jobs" % (name, 100.0 * share))
    assert share <= 0.05
    h = BatchMPC(launches[0]["P"], 1)
    for L, near in zip(launches, masks):
        d, e = L["dev"], L["emu"]
        assert np.array_equal(M.device_class(d["kappa_hi"]), M.device_class(e["kappa_hi"]))
        assert np.array_equal(d["iters"][~near], e["iters"][~near]), (name, np.argwhere((d["iters"] != e["iters"]) & ~near)[:5])
        zero = L["mclass"] == "zero"
        _, it0 = h.balance_check(L["x"], L["params"], want_iters=True, mu_scale=0.0)
        assert np.array_equal(d["iters"][zero], it0[zero])
    h.close()


@pytest.mark.parametrize("name", M.ONE_BODY)
def test_one_body_arrangements_on_the_wave_form(arrangements, name, monkeypatch):
    """UPR_BAL_FORM=0 sends one-body arrangements through the wave-per-job kernel: the same checks on the same jobs, the class and
    (away from the boundary) the iteration counts of the emulated wave form."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    launches = M.cases(arrangements, name)
    masks = M.near_masks(launches)
    h = BatchMPC(launches[0]["P"], 1)
    for k, (L, near) in enumerate(zip(launches, masks)):
        out = _margin(h, L)
        bad = M.check_answer(L, out)
        assert not bad, (name, k, bad[:5])
        emu = M.run_emu(L["P"], L["x"], L["params"], L["per_point"], form=0)
        assert np.array_equal(M.device_class(out["kappa_hi"]), M.device_class(emu["kappa_hi"]))
        assert np.array_equal(out["iters"][~near], emu["iters"][~near])
    h.close()


@pytest.mark.parametrize("name", ["pink_bottle", "pink_bottle_arm", "fixture_box", "bottle_20_contacts"])
def test_known_answers(arrangements, name):
    """Facet states in the scenarios that keep them on the facet: |kappa - 1| <= 1e-6; the fixture box pushed 5 % further:
    |kappa - 1.05| <= 1e-6 (the derivation of the 1e-6: tests/test_friction_margin.py::test_known_answers)."""
    launches = _device(arrangements, name)
    L = launches[0]
    rows = [i for i, k in enumerate(L["kinds"]) if k == "facet"]
    assert len(rows) == 2
    k1 = L["dev"]["kappa_hi"][rows][:, list(R.FACET_SCENARIOS)]
    print("friction margin on the device, facet states of %s: largest |kappa - 1| %.2e" % (name, np.abs(k1 - 1.0).max()))
    assert np.abs(k1 - 1.0).max() <= 1e-6
    if name == "fixture_box":
        Lb = launches[-1]
        assert Lb["kinds"] == ["beyond"] * 2
        kb = Lb["dev"]["kappa_hi"][:, list(R.FACET_SCENARIOS)]
        print("friction margin on the device, pushed facet states of fixture_box: largest |kappa - 1.05| %.2e" % np.abs(kb - 1.05).max())
        assert np.abs(kb - 1.05).max() <= 1e-6


@pytest.mark.parametrize("name", M.NAMES)
def test_rho_with_a_friction_scale(arrangements, name):
    """balance_check(..., mu_scale=kappa), first launch of the arrangement: rho at kappa in {0.5, 1, 2} does not increase (to 1e-9
    max(|b|, 1)), at kappa = 1 it equals the call without mu_scale bit for bit (iteration counts too), |rho - rho_ref| <= 1e-9
    max(1, |b|) at kappa in {0.5, 2}, and one scale per scenario in one call gives the columns of the single-scale calls."""
    L = M.cases(arrangements, name)[0]
    h = BatchMPC(L["P"], 1)
    rho = {k: h.balance_check(L["x"], L["params"], mu_scale=k) for k in (0.5, 2.0)}
    rho[1.0], it1 = h.balance_check(L["x"], L["params"], want_iters=True, mu_scale=1.0)
    plain, it = h.balance_check(L["x"], L["params"], want_iters=True)
    assert np.array_equal(rho[1.0], plain) and np.array_equal(it1, it)
    M.check_rho_scaled(L["jobs"], rho, name, "device")
    mixed = h.balance_check(L["x"], L["params"], mu_scale=np.array([0.5, 1.0, 2.0, 1.0]))
    assert all(np.array_equal(mixed[:, s], rho[k][:, s]) for s, k in enumerate((0.5, 1.0, 2.0, 1.0)))
    with pytest.raises(RuntimeError, match="mu_scale"):
        h.balance_check(L["x"], L["params"], mu_scale=-1.0)
    with pytest.raises(RuntimeError, match="kappa_max"):
        h.friction_margin(L["x"], L["params"], kappa_max=0.0)
    with pytest.raises(RuntimeError, match="kappa_max"):
        h.friction_margin(L["x"], L["params"], kappa_max=np.inf)
    h.close()


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_plan_form(arrangements):
    """Headline handle, B = 3, N = 20, one cold solve, 4 scenarios: 252 jobs.  friction_margin_plan equals the points form on the
    downloaded plan, == on kappa_hi, kappa_lo and iters, with shared scenarios, scenarios per instance and params=None (every
    instance's own body_params); the device time is reported; balance_check_plan(mu_scale=...) equals its points form likewise."""
    B = 3
    mpc, x0, bp = _headline(arrangements, B)
    P = mpc.problem
    N = P.N
    assert N == 20
    mpc.set_observation(0.0, x0)
    mpc.advance()
    _, xs, _ = mpc.solution()
    pts = xs.reshape(B * (N + 1), P.nx)
    scen = R.scenarios(P)
    got = mpc.friction_margin_plan(scen, want_lo=True, want_iters=True)
    assert mpc.balance_ms() > 0.0
    want = mpc.friction_margin(pts, scen, want_lo=True, want_iters=True)
    assert got[0].shape == (B, N + 1, 4) and got[0].size == 252
    assert all(np.array_equal(g.reshape(-1, 4), w) for g, w in zip(got, want))
    assert not np.any(np.isnan(got[0])) and np.any(np.isfinite(got[0]) & (got[0] > 0))
    per = np.stack([R.scenarios(P, np.random.default_rng(b), 4) for b in range(B)])
    got = mpc.friction_margin_plan(per, want_lo=True, want_iters=True)
    want = mpc.friction_margin(pts, np.repeat(per[:, None], N + 1, axis=1).reshape(B * (N + 1), 4, P.nb, 10), want_lo=True, want_iters=True)
    assert all(np.array_equal(g.reshape(-1, 4), w) for g, w in zip(got, want))
    got = mpc.friction_margin_plan(want_lo=True, want_iters=True)
    own = np.repeat(bp[:, None, None], N + 1, axis=1).reshape(B * (N + 1), 1, P.nb, 10)
    want = mpc.friction_margin(pts, own, want_lo=True, want_iters=True)
    assert got[0].shape == (B, N + 1, 1) and all(np.array_equal(g.reshape(-1, 1), w) for g, w in zip(got, want))
    k2 = mpc.friction_margin_plan(scen, kappa_max=2.0)
    assert not np.any(np.isnan(k2)) and np.all((k2 <= 2.0) | np.isinf(k2))
    mu = np.array([0.5, 1.0, 2.0, 0.0])
    assert np.array_equal(mpc.balance_check_plan(scen, mu_scale=mu).reshape(-1, 4), mpc.balance_check(pts, scen, mu_scale=mu))
    assert np.array_equal(mpc.balance_check_plan(scen, mu_scale=1.0), mpc.balance_check_plan(scen))
    assert np.array_equal(mpc.balance_check_plan(mu_scale=0.5).reshape(-1, 1), mpc.balance_check(pts, own, mu_scale=0.5))
    mpc.close()


def test_calls_leave_the_handle_as_it_was(arrangements):
    """Twin handles (headline, B = 3, feedback policy and tracked value function on), the same calls on both, the friction margin in
    both forms and the scaled balance check on one of them only, between the other calls: solution(), stats(), the next advance()
    and the ticks (the later ones replayed from the captured graph) are bitwise equal."""
    B = 3
    (A, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = R.scenarios(A.problem)
    probe = lambda: (A.friction_margin(x0, scen, want_lo=True, want_z=True, want_y=True, want_iters=True), A.friction_margin_plan(),   # noqa: E731
                     A.friction_margin_plan(scen), A.balance_check_plan(scen, mu_scale=0.5))
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
    Va, Vt = A.value_function(0.05, x0), T.value_function(0.05, x0)          # (raises "stale" had the call invalidated it)
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


def test_one_large_launch(arrangements):
    """Headline B = 64, 21 knots, the study's 45 scenarios, plan form: 60 480 jobs in one launch; kappa_hi is finite or +inf, never
    NaN, on every job; on a fixed seeded sample of 256 jobs the points form returns the same kappa, and checks 1 - 4 (both
    certificates among them) hold on its z and y."""
    B = 64
    mpc, x0, bp = _headline(arrangements, B, seed=11)
    P = mpc.problem
    mpc.set_observation(0.0, x0)
    mpc.advance()
    scen = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    hi, lo, it = mpc.friction_margin_plan(scen, want_lo=True, want_iters=True)
    ms = mpc.balance_ms()
    assert hi.shape == (B, P.N + 1, 45) and not np.any(np.isnan(hi)) and hi.min() >= 0.0 and not np.any(np.isnan(lo))
    assert it.min() >= 0 and it.max() <= 34 * 3 * 16
    _, xs, _ = mpc.solution()
    rng = np.random.default_rng(2024)
    jb, jk, js = rng.integers(0, B, 256), rng.integers(0, P.N + 1, 256), rng.integers(0, 45, 256)
    L = dict(P=P, x=xs[jb, jk], params=scen[js][:, None], per_point=True)
    L["jobs"] = M.Jobs(L)
    L["jobs"].classes()
    out = _margin(mpc, L)
    assert np.array_equal(out["kappa_hi"][:, 0], hi[jb, jk, js]) and np.array_equal(out["kappa_lo"][:, 0], lo[jb, jk, js])
    bad = M.check_answer(L, out)
    assert not bad, bad[:5]
    fin = np.isfinite(hi)
    print("friction margin, B = 64 x 21 knots x 45 scenarios: %.3f ms on the device; kappa* = 0 on %.1f %%, finite on %.1f %% (mean %.3f, max %.3f), "
          "inf on %.1f %% of the jobs; solves per job mean %.1f max %d" % (ms, 100.0 * (hi == 0).mean(), 100.0 * (fin & (hi > 0)).mean(),
          hi[fin & (hi > 0)].mean() if (fin & (hi > 0)).any() else 0.0, hi[fin].max(), 100.0 * (~fin).mean(), it.mean(), it.max()))
    mpc.close()
