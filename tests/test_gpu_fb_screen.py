"""Device screen of the feedback gains (sqp.use_feedback_policy: the controller sends u = u* + K (x - x*), not the plan) of EVERY
instantiation of the production QP kernel and of the gather kernel behind it, on the table of tests/test_gpu_qp_screen.py, and the
edges of the policy evaluation.  tests/test_fb_reference.py is the CPU twin: it explains the two-run regime (the point exported with
qp_iter_max = k is the point the run with k + 1 factors), holds the threshold table FB_TOL and the inputs of the cases.

Per case, on the device's own linearisation records:
  * fused gains (write_feedback at the kernel's exit) against the gains of the same source on the host (emu_qp3_cfg_fb): 1e-8 relative
    to the instance's max |K| -- the race and indexing check, the QP screen's bound (EMU_TOL: where a case needs more);
  * fused gains against the dense reference K_ref (tests/fb_check.py) at the point the device exported, per knot and block, FB_TOL;
  * UPR_FB_FUSED = 0: the gather kernel (feedback_kernel of upr_api.hip, source kind 3) against K_ref, FB_TOL.
Two more cases run the headline shape on the generic and on the second-structure QP kernel (UPR_QP_KERNEL = 1, 2): source kinds 1 and
2 of the gather kernel against K_ref at the point the same kernel exported; four more (KIND_CASES) do the same on the dice under both
kinds and, under kind 1, on the eight-corner arrangement and on the headline with collision rows.  The run-time instantiated case runs in a fresh child
process (measure_in_child: the library keeps such an instantiation per process)."""
import copy
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

import fb_check
from test_fb_reference import CAP, FB_TOL, K_IT, fb_case, reference_gains
from test_gpu_qp_screen import CASES, RUN_TIME_HEADLINE, _ids, jit_cache, parse_qp_kernel  # noqa: F401  (jit_cache: fixture)
from upright_amd.engine import BatchMPC

pytestmark = pytest.mark.gpu

# fused gains against the emulated gains: cases that need more than 1e-8 of the instance's max |K| (measured value and reason)
# (all three are the cases with the largest steps of the table, max |dx| 10: the N = 12 case is the one the QP screen gives 5e-8 for the
#  same reason, the two ur10 cases carry the moved target of FB_WAY_OFFSET; the device's reciprocal / rsqrt rounding enters K through
#  systems the float64 reference itself solves to 3e-9 only, and device and emulation each sit within 6.2e-9 of K_ref)
EMU_TOL = {
    (6, 1, 4, 1, 20, False, True, False): 5e-8,     # measured 1.23e-8
    (6, 1, 4, 1, 10, False, True, False): 5e-8,     # measured 2.30e-8
    (9, 1, 4, 3, 12, False, False, False): 1e-7,    # measured 3.05e-8
}
# source kinds 1 and 2 of the gather kernel on the headline shape: (threshold, a: float64 reference vs extended-precision twin, b: device
# gains vs twin), threshold = 10 max(a, b) as in FB_TOL, measured on the device run
KIND_TOL = {
    "1": (3.4e-8, 3.38e-9, 2.33e-9),     # worst instance 3.57e-9
    "2": (3.6e-8, 3.54e-9, 2.73e-9),     # worst instance 5.73e-9
}
KIND_NAME = {"1": "upr_qp_kernel<256>", "2": "upr_qp2_kernel<upr_qp2_dims<9, 1, 4, 3>, 128>"}


def _softened(P):
    return any(bool((P.slacks or {}).get(k)) for k in ("state_box", "input_box", "poly_ineq"))


def _handle(c, iters):
    P = copy.copy(c["P"]); P.qp_iter_max = int(iters)
    return BatchMPC(P, c["B"], body_params=c["bp"], way_p=c["way"])


def _check_kernel(mpc, cfg, jit):
    name = mpc.kernel_times()["qp_kernel"].replace("  ", " ")
    if isinstance(cfg, str):
        assert name == cfg, (name, cfg)
        return
    ran, is_jit = parse_qp_kernel(name)
    assert ran == cfg and is_jit == (jit is not None), (ran, cfg, name)


def exported_point(c, cfg, jit):
    """The primal-dual point after K_IT iterations, the device's records and iteration counts: (sol [B], pairs [B], lin)."""
    P, B = c["P"], c["B"]
    mpc = _handle(c, K_IT)
    try:
        _check_kernel(mpc, cfg, jit)
        mpc.set_observation(0.0, c["x0"])
        mpc.set_guess(c["xs0"], c["us0"])
        kkt = mpc.qp_kkt()
        pairs = mpc.qp_slack_pairs() if _softened(P) else None
        st = mpc.stats()
        lin = mpc.lin_records()
    finally:
        mpc.close()
    assert np.all(st["qp_iters_last"] == K_IT), st["qp_iters_last"]
    assert not np.any(st["qp_status_last"] == 2), st["qp_status_last"]
    sol = [dict(lam=kkt["lam"][b], slack=kkt["slack"][b]) for b in range(B)]
    return sol, [None if pairs is None else tuple(q[b] for q in pairs) for b in range(B)], lin


def device_gains(c, cfg, jit):
    """K [B][N][nu][nx] of the handle that runs K_IT + 1 iterations: one SQP iteration from the same guess."""
    mpc = _handle(c, K_IT + 1)
    try:
        _check_kernel(mpc, cfg, jit)
        mpc.set_observation(0.0, c["x0"])
        mpc.set_guess(c["xs0"], c["us0"])
        mpc.set_sqp_iterations(1)
        mpc.advance()
        K = mpc.feedback_gains()
        st = mpc.stats()
    finally:
        mpc.close()
    assert np.all(st["qp_iters_last"] == K_IT + 1), st["qp_iters_last"]
    assert not np.any(st["qp_status_last"] == 2), st["qp_status_last"]
    assert np.all(np.isfinite(K))
    return K[:, :, :, :c["P"].nx]


def _against_reference(c, K, Kref):
    return max(fb_check.block_errors(K[b], Kref[b], c["P"].nq).max() for b in range(c["B"]))


def measure_case(cfg, jit):
    """The device runs of one case and its three figures: dict(e_emu, e_fused, e_gath).  Sets UPR_FB_FUSED in the process's
    environment for the gathered run (the caller restores it)."""
    c = fb_case(cfg)
    P, B = c["P"], c["B"]
    sol, pairs, lin = exported_point(c, cfg, jit)
    fused = device_gains(c, cfg, jit)
    os.environ["UPR_FB_FUSED"] = "0"
    gathered = device_gains(c, cfg, jit)
    # the same source on the host, on the device's records
    emu = fb_check.emu_qp3_cfg_fb(cfg, P, B, c["xs0"], c["us0"], c["x0"], lin, c["bp"], K_IT + 1)
    assert np.all(emu["stats"][:, 1] == K_IT + 1) and not np.any(emu["stats"][:, 2] == 2)
    e_emu = max(np.abs(fused[b] - emu["K"][b]).max() / np.abs(emu["K"][b]).max() for b in range(B))
    Kref = [reference_gains(P, lin[b], sol[b], pairs[b], c["bp"][b])[0] for b in range(B)]
    return dict(e_emu=float(e_emu), e_fused=float(_against_reference(c, fused, Kref)), e_gath=float(_against_reference(c, gathered, Kref)))


CHILD = {"dead": None}     # set to the case whose child ended by signal, abort or time limit: no further child is started


def measure_in_child(cfg, jit, jit_cache):
    """A run-time instantiation is kept per process and shape (upr_api.hip: g_jit), and tests/test_gpu_parity.py's
    test_unlisted_shape_is_instantiated_at_run_time, which runs later in the same session, holds the FIRST instantiation of this very
    shape against its disk cache: the case runs in a fresh child process, which also makes it compile (or load) like a new process
    does.  The child prints measure_case's figures as JSON."""
    assert CHILD["dead"] is None, "the child for %s did not end normally: no further child process started" % (CHILD["dead"],)
    env = dict(os.environ)
    env["UPR_QP3_JIT"] = jit
    env["UPR_JIT_CACHE"] = jit_cache
    env["PYTHONPATH"] = os.pathsep.join([str(HERE.parent), str(HERE)] + ([env["PYTHONPATH"]] if env.get("PYTHONPATH") else []))
    try:
        p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", _ids(cfg), jit], env=env, cwd=str(HERE.parent),
                           capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired:
        CHILD["dead"] = cfg
        raise
    if p.returncode != 0:
        if p.returncode < 0 or p.returncode in (124, 134, 137, 139):
            CHILD["dead"] = cfg
        raise AssertionError("child %s ended with %d:\n%s\n%s" % (_ids(cfg), p.returncode, p.stdout[-2000:], p.stderr[-2000:]))
    return json.loads([l for l in p.stdout.splitlines() if l.startswith("{")][-1])


def _fb_screen(cfg, jit, jit_cache, monkeypatch):
    if jit is not None:
        r = measure_in_child(cfg, jit, jit_cache)
    else:
        monkeypatch.setenv("UPR_FB_FUSED", "1")      # (measure_case sets it to 0 for its last handle: put back behind the test)
        r = measure_case(cfg, None)
    e_emu, e_fused, e_gath = r["e_emu"], r["e_fused"], r["e_gath"]
    tol_emu, tol = EMU_TOL.get(cfg, 1e-8), FB_TOL[cfg][0]
    print("fb screen %s%s: fused vs emulated %.2e (tolerance %.0e)  fused vs K_ref %.2e  gathered vs K_ref %.2e (threshold %.1e)"
          % (_ids(cfg), "" if jit is None else " jit " + jit, e_emu, tol_emu, e_fused, e_gath, tol))
    assert tol <= CAP
    assert e_emu < tol_emu, (e_emu, tol_emu)
    assert e_fused < tol, (e_fused, tol)
    assert e_gath < tol, (e_gath, tol)


@pytest.mark.parametrize("cfg", list(CASES), ids=_ids)
def test_feedback_gains_of_every_instantiation(cfg, jit_cache, monkeypatch):
    _fb_screen(cfg, CASES[cfg][2], jit_cache, monkeypatch)


def test_table_reaches_both_gather_sizes_and_both_schur_forms():
    """feedback_kernel<6, 12> serves ne <= 6 and nfc <= 12, the maximal instantiation the rest; the production kernel leaves the inverse
    Schur factor as 6 x 6 blocks (star arrangements) or as one dense factor (DENSE): the table has all four."""
    small = {6 * c[1] <= 6 and c[3] * c[2] <= 12 for c in CASES}
    dense = {c[7] for c in CASES if c[1] > 1}
    assert small == {True, False} and dense == {True, False}


@pytest.mark.parametrize("kind", ["1", "2"])
def test_gather_kernel_source_kinds_of_the_other_qp_kernels(kind, monkeypatch):
    """UPR_QP_KERNEL = 1 (generic kernel: source kind 1) and 2 (second structure: kind 2) on the headline shape: the gather kernel forms
    the jerk rows from V_k and the inverse factor of H_jj there.  Point and gains come from the same kernel, K_IT and K_IT + 1
    iterations; prints a (float64 reference vs its extended-precision twin) and b (device gains vs twin) on instance 0."""
    _kind_screen(kind, RUN_TIME_HEADLINE, KIND_NAME[kind], KIND_TOL[kind][0], monkeypatch)


def _kind_screen(kind, cfg, name, tol, monkeypatch):
    monkeypatch.setenv("UPR_QP_KERNEL", kind)
    c = fb_case(cfg)
    P, B = c["P"], c["B"]
    sol, pairs, lin = exported_point(c, name, None)
    K = device_gains(c, name, None)
    Kref = [reference_gains(P, lin[b], sol[b], pairs[b], c["bp"][b])[0] for b in range(B)]
    Kx = reference_gains(P, lin[0], sol[0], pairs[0], c["bp"][0], extended=True)[0]
    a, bb = fb_check.block_errors(Kref[0], Kx, P.nq).max(), fb_check.block_errors(K[0], Kx, P.nq).max()
    err = _against_reference(c, K, Kref)
    print("fb screen UPR_QP_KERNEL=%s %s [%s]: a %.2e  b %.2e  worst instance %.2e (threshold %.1e)" % (kind, _ids(cfg), name, a, bb, err, tol))
    assert tol <= CAP and err < tol, (err, tol)


# The same screen behind the generic kernel and the second structure on shapes beyond the headline's: two bodies with shared contacts (a
# dense 12 x 12 inverse Schur factor; kinds 1 and 2), the eight-corner frictionless arrangement with softened rows and per-instance
# inertial parameters (eight diagonal blocks of Lsi, the generic kernel's 512-lane form) and hard collision rows.
# (kind, case of the QP screen's table) -> (kernel that has to run, threshold = 10 max(a, b), a, b as in KIND_TOL, measured on the device run)
DICE, ROBUST, ROWS = (9, 2, 8, 3, 20, False, False, True), (9, 8, 32, 1, 20, False, True, False), (9, 1, 4, 3, 20, True, False, False)
KIND_CASES = {
    ("1", DICE): ("upr_qp_kernel<256>", 3.4e-8, 3.03e-9, 3.37e-9),                                # worst instance 4.07e-9
    ("2", DICE): ("upr_qp2_kernel<upr_qp2_dims<9, 2, 8, 3>, 128>", 3.1e-8, 3.02e-9, 2.93e-9),     # worst instance 2.25e-9
    ("1", ROBUST): ("upr_qp_kernel<512>", 2.0e-8, 1.96e-9, 1.00e-9),                              # worst instance 2.52e-9
    ("1", ROWS): ("upr_qp_kernel<256>", 4.2e-8, 3.39e-9, 4.14e-9),                                # worst instance 3.77e-9
}


@pytest.mark.parametrize("kind,cfg", list(KIND_CASES), ids=["%s-%s" % (k, _ids(c)) for k, c in KIND_CASES])
def test_gather_kernel_source_kinds_on_more_shapes(kind, cfg, monkeypatch):
    name, tol, _, _ = KIND_CASES[(kind, cfg)]
    _kind_screen(kind, cfg, name, tol, monkeypatch)


# ---- policy evaluation at its edges ---------------------------------------------------------------------------------------------------------
CUPS = (9, 7, 28, 3, 20, False, False, False)


def _time_at(s, dt, t0):
    """A time t with (t - t0) / dt == s exactly in double precision (the kernel's own quotient), for integral s."""
    t = t0 + s * dt
    for _ in range(16):
        q = (t - t0) / dt
        if q == s:
            return t
        t = np.nextafter(t, -np.inf if q > s else np.inf)
    raise AssertionError((s, dt, t0))


def policy_reference(P, t0, X, U, K, t, x):
    """ocs2::LinearController over the knots j = 0 .. N-1 of one instance: bias_j = u_j - K_j x_j; bias and K interpolated linearly, both
    held over the last interval, zero input past the horizon; the state by upr_interp's rule (held outside the plan).  Returns
    (x*(t), u, bound): bound = 64 eps (sum_c |K_c| (|x_c| + |x*_c|) + |u|), the rounding of the sums."""
    N, dt = P.N, P.dt
    s = max((t - t0) / dt, 0.0)
    if s >= N:
        xr = X[N].copy()
    else:
        j = int(s); xr = (1.0 - (s - j)) * X[j] + (s - j) * X[j + 1]
    if s > N:
        return xr, np.zeros(P.nu), np.zeros(P.nu)
    j = min(int(s), N - 1)
    a = 0.0 if s >= N - 1 else s - j
    j1 = min(j + 1, N - 1)
    bias = (1.0 - a) * (U[j] - K[j] @ X[j]) + a * (U[j1] - K[j1] @ X[j1])
    Kt = (1.0 - a) * K[j] + a * K[j1]
    bound = 64.0 * np.finfo(float).eps * ((1.0 - a) * (np.abs(K[j]) @ (np.abs(x) + np.abs(X[j])) + np.abs(U[j]))
                                          + a * (np.abs(K[j1]) @ (np.abs(x) + np.abs(X[j1])) + np.abs(U[j1])))
    return xr, bias + Kt @ x, bound


def test_policy_evaluation_at_the_edges_of_the_plan(monkeypatch):
    """evaluate_policy_kernel on the seven-cup shape (nu = 93 inputs over its 64 lanes: the stride loop runs), B = 8, one time per
    instance: before the plan's start, exactly on its first knot, exactly on an inner knot, between knots, exactly on knot N - 1, inside
    the last interval, exactly at N dt, past the horizon; observed states off the plan.  Against policy_reference above, each output
    within the rounding bound; the returned state upr_interp's rule to rounding.  tick() returns what set_observation + advance +
    evaluate return for the same times."""
    builder, kw, _ = CASES[CUPS]
    c = builder(**kw)
    P = c["P"]; P.use_feedback_policy = True
    B, N, dt = 8, P.N, P.dt
    assert P.nu == 93 and P.nu > 64
    rng = np.random.default_rng(11)
    x0 = np.tile(c["x0"][:1], (B, 1))
    x0[:, P.nq:2 * P.nq] += rng.uniform(-0.05, 0.05, (B, P.nq))
    way = np.tile(np.asarray(c["way"])[:1], (B, 1, 1))
    t0 = -0.125      # (a plan that does not start at zero; with it the knot times below have an exact quotient (t - t0) / dt)
    mpc = BatchMPC(P, B, way_p=way)
    try:
        mpc.set_observation(t0, x0)
        mpc.advance()
        ts, X, U = mpc.solution()
        K = mpc.feedback_gains()
        s = np.array([-1.5, 0.0, 8.0, 11.3, N - 1.0, N - 0.4, float(N), N + 0.7])
        t = np.array([t0 + v * dt if v != int(v) else _time_at(v, dt, t0) for v in s])
        exact = [i for i, v in enumerate(s) if v == int(v) and v >= 0]
        assert all((t[i] - t0) / dt == s[i] for i in exact), ((t - t0) / dt, s)
        assert np.all(ts[:, 0] == t0)
        # observed states: the plan's state at a nearby knot plus an offset of a few per cent
        xo = np.stack([X[b, min(max(int(round(s[b])), 0), N)] for b in range(B)]) + 0.03 * rng.standard_normal((B, X.shape[2]))
        xd, ud = mpc.evaluate(t, x_obs=xo)
    finally:
        mpc.close()
    assert np.abs(K).max() > 1e-3
    worst = 0.0
    for b in range(B):
        xr, ur, bound = policy_reference(P, t0, X[b], U[b], K[b], t[b], xo[b])
        # (the state: two products and a sum per entry, fused or not)
        assert np.all(np.abs(xd[b] - xr) <= 4.0 * np.finfo(float).eps * np.abs(X[b]).max(axis=0)), (b, np.abs(xd[b] - xr).max())
        if s[b] > N:
            assert np.all(ud[b] == 0.0)
        else:
            assert np.abs(ur).max() > 0 and np.all(bound > 0)
            worst = max(worst, (np.abs(ud[b] - ur) / bound).max())
            assert np.all(np.abs(ud[b] - ur) <= bound), (b, s[b], (np.abs(ud[b] - ur) / bound).max())
    print("policy at the edges: worst |u - u_ref| / bound %.3f" % worst)
    # tick = set_observation + advance + evaluate, one time per instance
    tt = 0.1 + 0.01 * np.arange(B)
    one = BatchMPC(P, B, way_p=way)
    two = BatchMPC(P, B, way_p=way)
    try:
        x1, u1 = one.tick(tt, xo)
        two.set_observation(tt, xo)
        two.advance()
        x2, u2 = two.evaluate(tt, x_obs=xo)
    finally:
        one.close(); two.close()
    assert np.array_equal(u1, u2) and np.array_equal(x1, x2)
    assert np.abs(u1).max() > 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--child":
        key = [c for c in CASES if _ids(c) == sys.argv[2]][0]
        print(json.dumps(measure_case(key, sys.argv[3])))
