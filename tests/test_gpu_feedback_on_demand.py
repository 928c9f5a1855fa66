"""The feedback gains on demand (upr_fb_state.h): an advance leaves them in the factors of its last QP, the policy forms the one or two
knots it needs from there (evaluate_policy_factors_kernel) and the array fb[B][N][nu][nx] is gathered at the first request, or before a
call overwrites a source.  Every test holds a handle created with UPR_FB_FUSED unset against one created with UPR_FB_FUSED = 1, which
writes the array at the exit of every advance's last QP as the library did before.  Inputs: fb_case of tests/test_fb_reference.py at
three shapes that reach every branch of the formulas -- the headline (6 x 6 Schur blocks, nf = 3), the robust shape (SOFT, nf = 1,
block-diagonal Schur) and box_arch (ROWS, DENSE: one 18 x 18 factor) -- all instantiations of the library's list (no run-time
instantiation, hence no child process).

Bounds.  Gains: jerk rows are a signed copy of K_k, equal bit for bit; force rows within 1e-8 of the instance's max |K|, the bound
tests/test_gpu_fb_screen.py uses between two evaluations of the same source.  Policy: per input i
2 (nx + 4) 2^-53 (|u_j,i| + sum_c |K_j,ic| |dx_c| + the same for knot j + 1 where the time lies inside an interval), the rounding of the
two dot products and the interpolation, against policy_reference of tests/test_gpu_fb_screen.py on the gains of the UPR_FB_FUSED = 1
handle -- evaluated in extended precision, since that reference forms bias = u - K x* and K x separately and its own float64 rounding,
eps sum |K| (|x| + |x*|), would exceed a bound that scales with |dx|.

Every test prints its measured figure; MEASURED below keeps those of the run the file was written against."""
import copy
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from test_fb_reference import fb_case
from test_gpu_fb_screen import CUPS, _time_at, policy_reference
from test_gpu_qp_screen import CASES, _ids
from upright_amd.engine import BatchMPC

pytestmark = pytest.mark.gpu

HEADLINE = (9, 1, 4, 3, 20, False, False, False)
ROBUST = (9, 8, 32, 1, 20, False, True, False)
BOX_ARCH = (9, 3, 16, 3, 20, True, False, True)
SHAPES = [HEADLINE, ROBUST, BOX_ARCH]
FORCE_TOL = 1e-8
# MEASURED on MI355X (profiles/NOTES_r07.md, "Feedback gains on demand"):
#   gains, on demand vs UPR_FB_FUSED = 1: force rows max |dK| / max |K| = 0 at every shape, after one advance, after two, behind the
#       diagnostics and behind the last replayed tick -- write_feedback and fb_force_column run the same sums in the same order (the
#       compact D_f of BIGF skips only products with structural zeros), so no row differs and nothing is contracted differently
#   policy, worst |u - u_ref| / threshold: 0.036 headline, 0.055 robust, 0.059 box_arch, 0.118 seven cups; against the UPR_FB_FUSED = 1
#       handle's own evaluate_policy the outputs are equal bit for bit (seven cups, ticks)


def _handle(c, knob, monkeypatch, P=None):
    """A handle with UPR_FB_FUSED = knob (None: unset) at its creation."""
    if knob is None:
        monkeypatch.delenv("UPR_FB_FUSED", raising=False)
    else:
        monkeypatch.setenv("UPR_FB_FUSED", knob)
    mpc = BatchMPC(P if P is not None else c["P"], c["B"], body_params=c["bp"], way_p=c["way"])
    monkeypatch.delenv("UPR_FB_FUSED", raising=False)
    return mpc


def _first_advance(mpc, c):
    mpc.set_observation(0.0, c["x0"])
    mpc.set_guess(c["xs0"], c["us0"])
    mpc.set_sqp_iterations(1)
    mpc.advance()


_CACHE = {}


def _case(cfg, monkeypatch):
    """The case and what the UPR_FB_FUSED = 1 handle gives after one advance, computed once per shape: gains, plan, statistics."""
    if cfg not in _CACHE:
        c = fb_case(cfg)
        mpc = _handle(c, "1", monkeypatch)
        try:
            _first_advance(mpc, c)
            ts, X, U = mpc.solution()
            c["parent"] = dict(K=mpc.feedback_gains(), X=X, U=U, status=mpc.stats()["qp_status_last"].copy())
        finally:
            mpc.close()
        assert np.all(np.isfinite(c["parent"]["K"])) and np.abs(c["parent"]["K"]).max() > 1e-3
        _CACHE[cfg] = c
    return _CACHE[cfg]


def _assert_gains(K, Kp, nq, what):
    """Jerk rows bit for bit, force rows within FORCE_TOL of the instance's max |K|; prints and returns the measured maximum."""
    assert K.shape == Kp.shape and np.all(np.isfinite(K))
    assert np.array_equal(K[:, :, :nq, :], Kp[:, :, :nq, :]), what + ": jerk rows differ"
    worst = 0.0
    for b in range(K.shape[0]):
        scale = np.abs(Kp[b]).max()
        worst = max(worst, np.abs(K[b, :, nq:, :] - Kp[b, :, nq:, :]).max() / scale)
    print("%s: force rows, max |K - K_fused| / max |K| = %.3e (bound %.0e)" % (what, worst, FORCE_TOL))
    assert worst <= FORCE_TOL, (what, worst)
    return worst


def _assert_policy(P, t0, X, U, K, t, xo, ud, what):
    """ud[B][nu] against policy_reference (extended precision) on the gains K, per input within the rounding bound of the module's
    docstring; returns the largest |u - u_ref| / threshold."""
    N, nx = P.N, P.nx
    L = np.longdouble
    worst = 0.0
    for b in range(ud.shape[0]):
        tb = float(t[b])
        _, ur, _ = policy_reference(P, t0, X[b, :, :nx].astype(L), U[b].astype(L), K[b, :, :, :nx].astype(L), tb, xo[b, :nx].astype(L))
        s = max((tb - t0) / P.dt, 0.0)
        if s > N:
            assert np.all(ud[b] == 0.0), (what, b)
            continue
        j = min(int(s), N - 1); a = 0.0 if s >= N - 1 else s - j; j1 = min(j + 1, N - 1)
        thr = np.abs(U[b, j]) + np.abs(K[b, j, :, :nx]) @ np.abs(xo[b, :nx] - X[b, j, :nx])
        if a > 0.0:
            thr = thr + np.abs(U[b, j1]) + np.abs(K[b, j1, :, :nx]) @ np.abs(xo[b, :nx] - X[b, j1, :nx])
        thr = 2.0 * (nx + 4) * 2.0 ** -53 * thr
        err = np.abs(ud[b].astype(L) - ur).astype(float)
        ok = thr > 0
        if np.any(ok):
            worst = max(worst, float((err[ok] / thr[ok]).max()))
        assert np.all(err <= thr), (what, b, s, float((err[ok] / thr[ok]).max()) if np.any(ok) else err.max())
    return worst


@pytest.mark.parametrize("cfg", SHAPES, ids=_ids)
def test_lazy_export_equals_the_fused_one(cfg, monkeypatch):
    """feedback_gains() after one advance with the knob unset (the first request gathers the array, the second only copies) against the
    array the QP kernel's exit wrote."""
    c = _case(cfg, monkeypatch)
    mpc = _handle(c, None, monkeypatch)
    try:
        _first_advance(mpc, c)
        K = mpc.feedback_gains()
        K2 = mpc.feedback_gains()
        st = mpc.stats()["qp_status_last"]
    finally:
        mpc.close()
    assert np.array_equal(st, c["parent"]["status"])
    assert np.array_equal(K, K2)
    _assert_gains(K, c["parent"]["K"], c["P"].nq, "lazy export " + _ids(cfg))


@pytest.mark.parametrize("cfg", SHAPES, ids=_ids)
def test_policy_reads_the_factors(cfg, monkeypatch):
    """evaluate_policy on a handle whose gains are still in the factors -- nobody asked for the array -- at a time in the first interval,
    in the middle of the plan with 0 < a < 1, in the last interval (a = 0, j = N - 1) and beyond the plan (zero input), at observed
    states off the plan."""
    c = _case(cfg, monkeypatch)
    P, B, par = c["P"], c["B"], c["parent"]
    N, dt = P.N, P.dt
    rng = np.random.default_rng(5)
    mpc = _handle(c, None, monkeypatch)
    worst = 0.0
    try:
        _first_advance(mpc, c)
        assert np.array_equal(mpc.solution()[1], par["X"])
        for s in (0.4, 7.3, N - 0.4, N + 0.7):
            t = np.full(B, s * dt)
            xo = par["X"][:, min(int(round(s)), N)] + 0.03 * rng.standard_normal(par["X"][:, 0].shape)
            _, ud = mpc.evaluate(t, x_obs=xo)
            if s < N:
                assert np.abs(ud - par["U"][:, min(int(s), N - 1)]).max() > 1e-6      # (the feedback term is there)
            worst = max(worst, _assert_policy(P, 0.0, par["X"], par["U"], par["K"], t, xo, ud, "policy %s s=%g" % (_ids(cfg), s)))
    finally:
        mpc.close()
    print("policy from the factors %s: worst |u - u_ref| / threshold %.3f" % (_ids(cfg), worst))


def test_policy_reads_the_factors_seven_cups(monkeypatch):
    """The seven-cup policy case of tests/test_gpu_fb_screen.py (nu = 93 inputs over 64 lanes, two knots of 20 KB each in LDS, BIGF), B = 8,
    one time per instance: before the plan's start, on knots, between knots, in the last interval, at N dt, past the horizon."""
    builder, kw, _ = CASES[CUPS]
    c = builder(**kw)
    P = copy.copy(c["P"]); P.use_feedback_policy = True
    B, N, dt = 8, P.N, P.dt
    assert P.nu == 93
    rng = np.random.default_rng(11)
    x0 = np.tile(c["x0"][:1], (B, 1))
    x0[:, P.nq:2 * P.nq] += rng.uniform(-0.05, 0.05, (B, P.nq))
    way = np.tile(np.asarray(c["way"])[:1], (B, 1, 1))
    cc = dict(B=B, bp=None, way=way)
    t0 = -0.125
    s = np.array([-1.5, 0.0, 8.0, 11.3, N - 1.0, N - 0.4, float(N), N + 0.7])
    t = np.array([t0 + v * dt if v != int(v) else _time_at(v, dt, t0) for v in s])
    par, lazy = _handle(cc, "1", monkeypatch, P), _handle(cc, None, monkeypatch, P)
    try:
        for m in (par, lazy):
            m.set_observation(t0, x0)
            m.advance()
        _, X, U = par.solution()
        K = par.feedback_gains()
        assert np.array_equal(lazy.solution()[1], X)
        xo = np.stack([X[b, min(max(int(round(s[b])), 0), N)] for b in range(B)]) + 0.03 * rng.standard_normal((B, X.shape[2]))
        _, ud = lazy.evaluate(t, x_obs=xo)
        _, up = par.evaluate(t, x_obs=xo)
        Kl = lazy.feedback_gains()
    finally:
        par.close(); lazy.close()
    worst = _assert_policy(P, t0, X, U, K, t, xo, ud, "policy seven cups")
    print("policy from the factors, seven cups: worst |u - u_ref| / threshold %.3f, max |u - u_fused| %.3e" % (worst, np.abs(ud - up).max()))
    _assert_gains(Kl, K, P.nq, "lazy export seven cups")


@pytest.mark.parametrize("cfg", SHAPES, ids=_ids)
def test_gains_survive_the_calls_that_overwrite_their_sources(cfg, monkeypatch):
    """After an advance: upr_batch_qp_kkt, upr_batch_qp_step and upr_batch_value_function_update relaunch the linearisation and a QP on the
    handle's own records, workspace and statistics (lin_records only reads the records); the gains handed out behind them are those of
    the advance, bit for bit what a twin hands out straight after it -- and the policy the same before and behind."""
    c = _case(cfg, monkeypatch)
    P, B = c["P"], c["B"]
    a, twin = _handle(c, None, monkeypatch), _handle(c, None, monkeypatch)
    try:
        _first_advance(a, c); _first_advance(twin, c)
        Kt = twin.feedback_gains()
        t = np.full(B, 3.3 * P.dt)
        xo = c["parent"]["X"][:, 3] + 0.03 * np.random.default_rng(9).standard_normal(c["parent"]["X"][:, 0].shape)
        _, u0 = a.evaluate(t, x_obs=xo)          # (from the factors)
        a.lin_records()
        a.qp_kkt()
        a.qp_step()
        if cfg == HEADLINE:
            a.value_function_update()
        _, u1 = a.evaluate(t, x_obs=xo)          # (from the array gathered in front of the first of them)
        Ka = a.feedback_gains()
    finally:
        a.close(); twin.close()
    assert np.array_equal(Ka, Kt)
    assert np.array_equal(u0, u1)


@pytest.mark.parametrize("cfg", SHAPES, ids=_ids)
def test_second_advance_supersedes(cfg, monkeypatch):
    """Two advances in a row without any request: the gains are those of the second."""
    c = _case(cfg, monkeypatch)
    lazy, par = _handle(c, None, monkeypatch), _handle(c, "1", monkeypatch)
    try:
        for m in (lazy, par):
            _first_advance(m, c)
            m.advance()
        K, Kp = lazy.feedback_gains(), par.feedback_gains()
        assert np.array_equal(lazy.solution()[1], par.solution()[1])
    finally:
        lazy.close(); par.close()
    assert np.abs(Kp - c["parent"]["K"]).max() > 0      # (not the first advance's)
    _assert_gains(K, Kp, c["P"].nq, "second advance " + _ids(cfg))


def test_tick_replays_keep_the_state(arrangements, monkeypatch):
    """Six control periods of the thrown-ball problem: the first is cold, the second to fourth are the three steady periods the capture
    waits for (the fourth is captured), the fifth and sixth are replayed -- tests/test_gpu_parity.py, test_tick_equals_the_three_calls,
    holds that schedule.  u of every period against the UPR_FB_FUSED = 1 handle's gains with the policy bound; feedback_gains() behind
    the last replayed period: the replay branch has to set the state itself."""
    from test_emu import _projectile_case

    B = 4
    P, x0r, way, _, _, dyn = _projectile_case(arrangements, B, use_feedback_policy=True)
    c = dict(B=B, bp=None, way=way)
    lazy, par = _handle(c, None, monkeypatch, P), _handle(c, "1", monkeypatch, P)
    worst, diff = 0.0, 0.0
    try:
        lazy.set_projectile_flag(1.0); par.set_projectile_flag(1.0)
        x = np.concatenate([x0r, dyn], axis=1)
        t, dt = 0.0, 0.01
        for tick in range(6):
            xl, ul = lazy.tick(t, x)
            xp, up = par.tick(t, x)
            _, X, U = par.solution()
            assert np.array_equal(lazy.solution()[1], X)
            K = par.feedback_gains()
            worst = max(worst, _assert_policy(P, t, X, U, K, np.full(B, t), x, ul, "tick %d" % tick))
            diff = max(diff, np.abs(ul - up).max())
            assert np.array_equal(xl, xp)
            j = ul[:, :9]
            q, v, acc = x[:, :9], x[:, 9:18], x[:, 18:27]
            ro, vo, ao = x[:, 27:30], x[:, 30:33], x[:, 33:36]
            x = np.concatenate([q + dt * v + dt ** 2 / 2 * acc + dt ** 3 / 6 * j, v + dt * acc + dt ** 2 / 2 * j, acc + dt * j,
                                ro + dt * vo + 0.5 * dt * dt * ao, vo + dt * ao, ao], axis=1)
            t += dt
        assert lazy.tick_graph_replays() >= 2, lazy.tick_graph_replays()
        Kl, Kp = lazy.feedback_gains(), par.feedback_gains()
    finally:
        lazy.close(); par.close()
    print("ticks: worst |u - u_ref| / threshold %.3f, max |u - u_fused| %.3e" % (worst, diff))
    _assert_gains(Kl, Kp, P.nq, "behind the last replayed tick")
