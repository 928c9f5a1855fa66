"""The batched balance check on the MI355X (upr_batch_balance_points / upr_batch_balance_plan, upright_amd/csrc/upr_balance.h): the
points form against tests/balance_ref.py on the case table of tests/test_balance_check.py with the same bound, the optimality
certificate on the device's z, the device against the host emulation of the same source (a race screen), the plan form against the
points form, the absence of side effects on the handle, and one large launch."""
import numpy as np
import pytest

import balance_ref as R
from upright_amd.engine import BatchMPC
from upright_amd.problem import thing_problem
from upright_amd.sampling import level_tray_states, waypoints_for

pytestmark = pytest.mark.gpu

NAMES = [r[0] for r in R.TABLE + R.EXTRA]
ONE_BODY = [r[0] for r in R.TABLE + R.EXTRA if r[4][0] == 1]
_DEVICE = {}


def _device(arrangements, name):
    """The launches of the table (with reference and emulation, R.cases) run once on the device: key "dev" = dict(rho, z, iters)."""
    if name not in _DEVICE:
        launches = R.cases(arrangements, name)
        handles = {}
        for L in launches:
            P = L["P"]
            if id(P) not in handles:
                handles[id(P)] = BatchMPC(P, 1)
            rho, z, it = handles[id(P)].balance_check(L["x"], L["params"], want_z=True, want_iters=True)
            L["dev"] = dict(rho=rho, z=z, iters=it)
        for h in handles.values():
            h.close()
        _DEVICE[name] = launches
    return _DEVICE[name]


@pytest.mark.parametrize("name", NAMES)
def test_points_form_against_the_reference(arrangements, name):
    """|rho - rho_ref| <= 1e-9 max(1, |b|) on every job of the table (both parameter layouts, job counts 1, 37, 256, 259), every
    iteration count below the cap, and the optimality certificate on the device's z."""
    tol = R.emu_lib().emu_bal_tol()
    worst = 0.0
    for L in _device(arrangements, name):
        d, ref = L["dev"], L["ref"]
        assert d["rho"].shape == ref["rho"].shape and np.all(np.isfinite(d["rho"])) and np.all(np.isfinite(d["z"]))
        worst = max(worst, float((np.abs(d["rho"] - ref["rho"]) / np.maximum(1.0, ref["bnorm"])).max()))
        assert d["iters"].min() >= 0 and d["iters"].max() < 3 * R.ncol(L["P"])
        zmin, dual, comp = R.certificate(ref, d["z"], tol)
        assert zmin >= 0.0 and dual <= 1.0 and comp <= 1.0, (name, zmin, dual, comp)
        for k in ("outside_zero", "free_fall"):
            assert np.all(d["iters"][L["classes"][k]] == 0) and np.all(d["z"][L["classes"][k]] == 0.0)
        assert np.all(d["rho"][L["classes"]["free_fall"]] == 0.0)
    print("balance check, device vs nnls, %s: %.2e" % (name, worst))
    assert worst <= 1e-9, (name, worst)


@pytest.mark.parametrize("name", NAMES)
def test_device_against_the_emulation(arrangements, name):
    """The same source on the device (a lane a job in registers, or 64 lanes a job and LDS) and on the host (one thread): identical
    iteration counts, rho to 1e-13 max(1, |b|).  The two sides round differently (fused multiply-adds, sincos), so the iteration
    counts are equal only because no decision of the iteration hangs on a last bit: exact ties between generators of symmetric
    contacts go to the lowest column (UPR_BAL_TIE), multipliers that are zero on a facet count as zero (UPR_BAL_ZERO).  Before
    those two rules 5 .. 11 of 256 jobs per one-body launch differed by two solves (6 against 8)."""
    worst = 0.0
    for L in _device(arrangements, name):
        d, e = L["dev"], L["emu"]
        assert np.array_equal(d["iters"], e["iters"]), (name, np.argwhere(d["iters"] != e["iters"])[:5])
        worst = max(worst, float((np.abs(d["rho"] - e["rho"]) / np.maximum(1.0, L["ref"]["bnorm"])).max()))
    print("balance check, device vs emulation, %s: %.2e" % (name, worst))
    assert worst <= 1e-13, (name, worst)


@pytest.mark.parametrize("name", ONE_BODY)
def test_one_body_arrangements_on_the_wave_form(arrangements, name, monkeypatch):
    """One-body arrangements launch the lane-per-job kernel (the tests above); UPR_BAL_FORM=0 sends them through the wave-per-job
    kernel: same bound against the reference, iteration counts of the emulated wave form, rho to 1e-13 max(1, |b|)."""
    monkeypatch.setenv("UPR_BAL_FORM", "0")
    launches = R.cases(arrangements, name)
    h = BatchMPC(launches[0]["P"], 1)
    for L in launches[:-1]:                 # (the free-fall launch has a problem of its own, without gravity)
        rho, it = h.balance_check(L["x"], L["params"], want_iters=True)
        emu = R.run_emu(L["P"], L["x"], L["params"], L["per_point"], form=0)
        scale = np.maximum(1.0, L["ref"]["bnorm"])
        assert (np.abs(rho - L["ref"]["rho"]) / scale).max() <= 1e-9
        assert np.array_equal(it, emu["iters"]) and (np.abs(rho - emu["rho"]) / scale).max() <= 1e-13
    h.close()


def _headline(arrangements, B, seed=3, **settings):
    P = thing_problem(arrangements["pink_bottle"], **settings)
    x0 = level_tray_states(B, seed=seed)
    rng = np.random.default_rng(seed)
    bp = np.stack([R.scale_mass(P.body_params, rng.uniform(0.9, 1.1)) for _ in range(B)])   # every instance its own mass
    return BatchMPC(P, B, body_params=bp, way_p=waypoints_for(P, x0)), x0, bp


def test_plan_form(arrangements):
    """Headline handle, B = 37, one cold solve.  balance_check_plan() equals the points form on the downloaded solution() with the same
    parameters, bitwise, in its three parameter layouts; at knots 0 .. N-1 rho_k <= |g(x_k, u_k)|_2 + 1e-12 (the plan's own forces
    satisfy the hard friction rows, so they are a feasible z; g from linearize_points); and with a CoM-box-vertex scenario at least
    one knot of at least one instance has rho > 1e-3 -- asserted on the reference first."""
    B = 37
    mpc, x0, bp = _headline(arrangements, B)
    P = mpc.problem
    N = P.N
    mpc.set_observation(0.0, x0)
    mpc.advance()
    _, xs, us = mpc.solution()
    pts = xs.reshape(B * (N + 1), P.nx)
    # nominal: every instance's own parameters
    rho, it = mpc.balance_check_plan(want_iters=True)
    own = np.repeat(bp[:, None, None], N + 1, axis=1).reshape(B * (N + 1), 1, P.nb, 10)
    rho_p, it_p = mpc.balance_check(pts, own, want_iters=True)
    assert rho.shape == (B, N + 1, 1) and np.array_equal(rho.reshape(-1, 1), rho_p) and np.array_equal(it.reshape(-1, 1), it_p)
    assert it.max() < 3 * 16
    lin = mpc.linearize_points(xs[:, :N].reshape(B * N, -1), us.reshape(B * N, -1), inst=np.repeat(np.arange(B), N))
    gn = np.linalg.norm(lin["g"], axis=1).reshape(B, N)
    assert np.all(rho[:, :N, 0] <= gn + 1e-12), float((rho[:, :N, 0] - gn).max())
    # shared scenarios, and scenarios per instance
    scen = R.scenarios(P)
    rho_s = mpc.balance_check_plan(scen)
    assert rho_s.shape == (B, N + 1, 4) and np.array_equal(rho_s.reshape(-1, 4), mpc.balance_check(pts, scen))
    per = np.stack([R.scenarios(P, np.random.default_rng(b), 5) for b in range(B)])
    rho_i = mpc.balance_check_plan(per)
    assert np.array_equal(rho_i.reshape(-1, 5), mpc.balance_check(pts, np.repeat(per[:, None], N + 1, axis=1).reshape(B * (N + 1), 5, P.nb, 10)))
    # the CoM-box vertex: the reference finds knots that lose balance, and so does the device, at the bound of the table -- on every
    # knot of every instance (R.solve: the reference is the smallest feasible residual of its three CPU answers, so no job is
    # without one), with the optimality certificate on the device's z of the same jobs (points form: the plan form returns no z)
    ref = R.reference(P, pts, scen[1:2], False)
    assert ref["rho"].max() > 1e-3, ref["rho"].max()
    assert (np.abs(rho_s.reshape(-1, 4)[:, 1:2] - ref["rho"]) / np.maximum(1.0, ref["bnorm"])).max() <= 1e-9
    rho_z, z = mpc.balance_check(pts, scen[1:2], want_z=True)
    assert np.array_equal(rho_z, rho_s.reshape(-1, 4)[:, 1:2])
    zmin, dual, comp = R.certificate(ref, z, R.emu_lib().emu_bal_tol())
    assert zmin >= 0.0 and dual <= 1.0 and comp <= 1.0, (zmin, dual, comp)
    assert rho_s[:, :, 1].max() > 1e-3
    mpc.close()


def test_calls_leave_the_handle_as_it_was(arrangements):
    """Twin handles (headline, B = 5, feedback policy and tracked value function on), the same calls on both, the balance check in
    both forms on one of them only, between all the other calls: solution(), stats(), feedback gains, the tracked value function
    (still valid) and the next advance() are bitwise equal; so are ticks, the later ones replayed from the captured graph."""
    B = 5
    (A, x0, bp), (T, _, _) = _headline(arrangements, B, use_feedback_policy=True), _headline(arrangements, B, use_feedback_policy=True)
    scen = R.scenarios(A.problem)
    probe = lambda: (A.balance_check(x0, scen, want_z=True, want_iters=True), A.balance_check_plan(), A.balance_check_plan(scen))   # noqa: E731
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
    assert np.array_equal(A.feedback_gains(), T.feedback_gains())
    Va, Vt = A.value_function(0.05, x0), T.value_function(0.05, x0)          # (raises "stale" had the call invalidated it)
    assert np.array_equal(Va[0], Vt[0]) and np.array_equal(Va[1], Vt[1])
    for h in (A, T):
        h.set_observation(0.1, x0)
        h.advance()
    for u, v in zip(A.solution(), T.solution()):
        assert np.array_equal(u, v)
    sa, st = A.stats(), T.stats()
    assert all(np.array_equal(sa[k], st[k]) for k in sa)
    # ticks: the graph is captured in the third period of a run; the check runs between replays
    x = x0.copy()
    for k in range(7):
        xa, ua = A.tick(0.2 + 0.01 * k, x)
        xt, ut = T.tick(0.2 + 0.01 * k, x)
        assert np.array_equal(xa, xt) and np.array_equal(ua, ut), k
        if k >= 2:
            probe()
        x = xa
    assert A.tick_graph_replays() == T.tick_graph_replays() >= 1
    A.close(); T.close()


def test_one_large_launch(arrangements):
    """Headline B = 1024, the study's 45 scenarios, plan form: 967 680 jobs in one launch, all finite, all below the cap; a fixed
    seeded sample of 256 jobs agrees with the reference at the bound of the table."""
    B = 1024
    mpc, x0, bp = _headline(arrangements, B, seed=11)
    P = mpc.problem
    mpc.set_observation(0.0, x0)
    mpc.advance()
    scen = R.study_sweep(P.body_params, [0.02, 0.02, 0.03])
    assert scen.shape == (45, 1, 10)
    rho, it = mpc.balance_check_plan(scen, want_iters=True)
    assert rho.shape == (B, P.N + 1, 45) and np.all(np.isfinite(rho)) and rho.min() >= 0.0
    assert it.min() >= 0 and it.max() < 3 * 16
    _, xs, _ = mpc.solution()
    rng = np.random.default_rng(2024)
    jb, jk, js = rng.integers(0, B, 256), rng.integers(0, P.N + 1, 256), rng.integers(0, 45, 256)
    # all 256 drawn jobs against the reference (the smallest feasible residual of its three CPU answers: R.solve), and the
    # optimality certificate on the device's z of the same jobs (points form, parameters per point; the plan form returns no z)
    ref = R.reference(P, xs[jb, jk], scen[js][:, None], True)
    got = rho[jb, jk, js][:, None]
    worst = float((np.abs(got - ref["rho"]) / np.maximum(1.0, ref["bnorm"])).max())
    rho_z, z = mpc.balance_check(xs[jb, jk], scen[js][:, None], want_z=True)
    assert np.array_equal(rho_z, got)
    zmin, dual, comp = R.certificate(ref, z, R.emu_lib().emu_bal_tol())
    assert zmin >= 0.0 and dual <= 1.0 and comp <= 1.0, (zmin, dual, comp)
    print("jobs of the sample on which nnls and lsq_linear differ by more than 1e-10: %d" % int((ref["floor"] > 1e-10).sum()))
    print("balance check, B = 1024 x 45 scenarios, sample of 256 vs nnls: %.2e; iterations mean %.2f max %d; rho > 1e-6 in %.1f %% of the jobs"
          % (worst, it.mean(), it.max(), 100.0 * (rho > 1e-6).mean()))
    assert worst <= 1e-9
    mpc.close()
